"""Pictures for the tests of include/homer_gpu.h section 12j: the ctypes mirror of hmr_gpu_scaled_rgb_picture, the comparator of every test - the composition of the two
numpy restatements that already exist (tests/rgb_cases.py: section 12f; tests/scale_cases.py: section 12g), which never call the library - and the size pairs and
contents the tests run."""
import ctypes as C

import numpy as np

import rgb_cases as rc
import scale_cases as sc

FORMS = sorted(rc.FORMS)
# (source, destination) sizes: 2 : 1 (two luma and two chroma tile columns), 3 : 2 (a tile boundary inside a footprint), nearly 1 : 1 with the largest sx sy (a width
# that is a multiple of neither 16 nor 32: every form takes the row-tail path), one axis only, 8 : 1 (nine-row footprints, the widest tile row), the identity
GPU_PAIRS = [((400, 272), (200, 136)), ((300, 204), (200, 136)), ((330, 266), (328, 264)), ((416, 480), (416, 240)), ((1600, 1088), (200, 136)), ((200, 136), (200, 136))]
# the host twin's: those, one output per chroma plane, and a ratio above 8 (the bound of 8 is the kernel's)
HOST_PAIRS = GPU_PAIRS + [((32, 16), (2, 2)), ((1800, 1224), (200, 136))]


class ScaledRgbPicture(C.Structure):
    """hmr_gpu_scaled_rgb_picture"""
    _fields_ = [("pic", rc.RgbPicture), ("width", C.c_int32), ("height", C.c_int32)]


def descriptor(fmt, pixel_bytes, offsets, addresses, pitches, matrix, full_range, width, height):
    return ScaledRgbPicture(pic=rc.descriptor(fmt, pixel_bytes, offsets, addresses, pitches, matrix, full_range), width=width, height=height)


def comparator(form, chans, matrix, full_range, dst_w, dst_h):
    """section 12j in numpy: 12g's area average of the 8-bit 4:2:0 picture 12f makes of the source - (Y [dst_h, dst_w], U, V [dst_h / 2, dst_w / 2]) as uint8"""
    return sc.restate(rc.restate(*rc.eight_bit(form, chans), matrix, full_range), dst_w, dst_h)


def comparator_bytes(form, chans, matrix, full_range, dst_w, dst_h):
    return sc.as_bytes(comparator(form, chans, matrix, full_range, dst_w, dst_h))


def real_valued(r, g, b, matrix, full_range, dst_w, dst_h):
    """the real-valued area average of the real-valued BT formula on 8-bit R, G, B, clipped to 0 .. 255: what every output has to be within 1.01 of"""
    y, u, v = rc.real_valued(r, g, b, matrix, full_range)
    return [np.clip(sc.real_valued_plane(p, w, h), 0.0, 255.0) for p, (w, h) in zip((y, u, v), ((dst_w, dst_h), (dst_w // 2, dst_h // 2), (dst_w // 2, dst_h // 2)))]


def chans_of(form, rng, r, g, b):
    """8-bit planes in the form's sample type"""
    return rc.as_floats(form, rng, r, g, b) if form in rc.FLOAT_TYPES else [r, g, b]


def content(kind, rng, w, h):
    """8-bit R, G, B [h, w]: noise, 8 x 8 blocks of random colours, or the extremes 0 / 255 per channel and pixel"""
    if kind == "noise":
        return rc.noise(rng, w, h)
    if kind == "blocks":
        return [rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8), dtype=np.uint8).repeat(8, axis=0).repeat(8, axis=1)[:h, :w] for _ in range(3)]
    assert kind == "extremes"
    return [(rng.integers(0, 2, (h, w)) * 255).astype(np.uint8) for _ in range(3)]
