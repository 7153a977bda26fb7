"""Pictures for the tests of include/homer_gpu.h section 12l: the ctypes mirror of hmr_gpu_scaled_yuv_picture, the comparator of every test - the composition of the two
numpy restatements that already exist (tests/yuv_cases.py: section 12k; tests/scale_cases.py: section 12g), which never call the library - the real-valued planes the
section's bound is stated against, the size pairs, the forms (one per class of k_yuv_ladder, and how all 50 are dealt over the pairs) and the contents the tests run."""
import ctypes as C

import numpy as np

import rgb_scale_cases as rs
import scale_cases as sc
import yuv_cases as yc

# (source, destination) sizes: rgb_scale_cases' as they are - two tile columns per class, a tile boundary inside a footprint, a width that is a multiple of neither 16 nor
# 32, one axis only, ratio 8, the identity; all even, so every packed form is legal
GPU_PAIRS = rs.GPU_PAIRS
# the host twin's: those, one output per chroma plane, and a ratio above 8 (the bound of 8 is the kernel's)
HOST_PAIRS = GPU_PAIRS + [((32, 16), (2, 2)), ((1800, 1224), (200, 136))]


def class_of(form):
    """what k_yuv_ladder is specialised on: (layout, container bytes, log2 of the chroma taps)"""
    fmt, chroma, bits, _, _ = yc.FORMS[form]
    return fmt, yc.sample_bytes(bits), yc.CHROMA[chroma]


# one form per class: three planar and three semi-planar tap counts in 8 bits and in 16-bit containers (10 bits in the low and in the high bits, 12 and 16 among them),
# packed 8-bit and packed 16-bit
CLASSES = ["planar_420_8", "planar_422_8", "planar_444_8", "planar_420_10", "planar_422_12", "planar_444_16", "semi_uv_420_8", "semi_vu_422_8", "semi_uv_444_8",
           "semi_uv_420_10msb", "semi_vu_422_12", "semi_uv_444_16", "uyvy_8", "y210"]
assert len(CLASSES) == 14 and len({class_of(f) for f in CLASSES}) == 14 == len({class_of(f) for f in yc.NAMES})


class ScaledYuvPicture(C.Structure):
    """hmr_gpu_scaled_yuv_picture"""
    _fields_ = [("pic", yc.YuvPicture), ("width", C.c_int32), ("height", C.c_int32)]


def descriptor(form, addresses, pitches, width, height):
    return ScaledYuvPicture(pic=yc.descriptor(form, addresses, pitches), width=width, height=height)


def declare(lib):
    """the argument types of section 12l's three functions, and of nothing else, onto a handle of the library (picture_gpu.load()'s: its table stops at 12k)"""
    one, many = [C.c_void_p, C.c_int, C.POINTER(ScaledYuvPicture), C.c_void_p], [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.POINTER(ScaledYuvPicture), C.c_void_p]
    lib.hmr_gpu_enc_load_source_scaled_yuv.argtypes = one
    lib.hmr_gpu_enc_load_sources_scaled_yuv.argtypes = many
    lib.hmr_gpu_scale_yuv_host.argtypes = [C.POINTER(ScaledYuvPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def comparator(form, y, u, v, dst_w, dst_h):
    """section 12l in numpy: 12g's area average of the 8-bit 4:2:0 picture 12k makes of the source - (Y [dst_h, dst_w], U, V [dst_h / 2, dst_w / 2]) as uint8"""
    return sc.restate(yc.restate(form, y, u, v), dst_w, dst_h)


def comparator_bytes(form, y, u, v, dst_w, dst_h):
    return sc.as_bytes(comparator(form, y, u, v, dst_w, dst_h))


def real_valued(form, y, u, v, dst_w, dst_h):
    """the real-valued area average of the min(255, x) planes, x the real-valued tap average of v / 2^s: what every output has to be within 1.0 of"""
    planes = [np.minimum(255.0, p) for p in yc.real_valued(form, y, u, v)]
    return [sc.real_valued_plane(p, w, h) for p, (w, h) in zip(planes, ((dst_w, dst_h), (dst_w // 2, dst_h // 2), (dst_w // 2, dst_h // 2)))]


def content(kind, form, rng, w, h):
    """the containers' values y [h, w], u, v [Hc, Wc]: noise over the container's range (yc.noise), 8 x 8 blocks of random values, or the extremes 0 / the container's
    largest value per sample"""
    if kind == "noise":
        return yc.noise(form, rng, w, h)
    _, chroma, bits, _, _ = yc.FORMS[form]
    wc, hc = yc.chroma_size(chroma, w, h)
    top, t = (256 if bits == 8 else 65536), yc.container_type(bits)
    shapes = [(h, w), (hc, wc), (hc, wc)]
    if kind == "blocks":
        return [rng.integers(0, top, ((r + 7) // 8, (c + 7) // 8)).repeat(8, axis=0).repeat(8, axis=1)[:r, :c].astype(t) for r, c in shapes]
    assert kind == "extremes"
    return [(rng.integers(0, 2, s) * (top - 1)).astype(t) for s in shapes]


def gpu_runs(pair):
    """[(form, padded)] of one GPU pair: the 14 class forms in the padded layout at every pair; the other 36 forms dealt over the pairs, so that every form of F appears
    somewhere, the first of each class in the tight layout; and the classes that have one form only once more, tight"""
    at = GPU_PAIRS.index(pair)
    runs = [(form, True) for form in CLASSES]
    seen, extras = set(), []
    for form in yc.NAMES:
        if form not in CLASSES:
            extras.append((form, class_of(form) in seen))
            seen.add(class_of(form))
    extras += [(form, False) for form in CLASSES if class_of(form) not in seen]
    return runs + [run for k, run in enumerate(extras) if k % len(GPU_PAIRS) == at]
