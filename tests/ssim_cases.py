"""Helper of the SSIM tests (include/homer_gpu.h section 12h): an oracle that shares nothing with the library - block sums by numpy reshape, then the header's formula
per window in Python integers, whose `//` is the floor towards minus infinity the definition asks for - the content pairs the tests run on, and pictures in host memory
in the layouts hmr_gpu_ssim_host takes."""
import ctypes as C
import os
import sys

import numpy as np

import encoder_cases as ec
from homerhevc_amd.encoder import PIC_I420, PIC_NV12, Picture

sys.path.insert(0, os.path.join(ec.ROOT, "tools"))
import gen_yuv  # noqa: E402

ONE, C1, C2 = 1 << 30, 416, 235963
LAYOUTS = ["tight_i420", "offset_i420", "nv12"]


def windows(w, h):
    """of a w x h plane"""
    return (w // 4 - 1) * (h // 4 - 1)


def picture_windows(width, height):
    return [windows(width, height), windows(width // 2, height // 2), windows(width // 2, height // 2)]


def plane_values(a, b):
    """q of every window of two planes (2-D uint8 arrays of one shape, multiples of 4), as an object array of Python ints [bh - 1, bw - 1]; the header's bounds are
    asserted on the way"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    h, w = a.shape
    assert a.shape == b.shape and h % 4 == 0 and w % 4 == 0 and h >= 8 and w >= 8

    def window_sums(x):
        s = x.reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3))
        return (s[:-1, :-1] + s[:-1, 1:] + s[1:, :-1] + s[1:, 1:]).astype(object)
    S1, S2, SS, S12 = window_sums(a), window_sums(b), window_sums(a * a + b * b), window_sums(a * b)
    var, cov = 64 * SS - S1 * S1 - S2 * S2, 64 * S12 - S1 * S2
    N, D = (2 * S1 * S2 + C1) * (2 * cov + C2), (S1 * S1 + S2 * S2 + C1) * (var + C2)
    assert D.min() > 0 and D.max() < 1 << 57 and (abs(N) <= D).all()
    q = (N * ONE) // D
    assert q.min() >= -ONE and q.max() <= ONE
    return q


def plane_sum(a, b):
    return int(plane_values(a, b).sum())


def planes_of(picture, width, height):
    """(y, u, v) as 2-D uint8 arrays of an I420 picture given as bytes or as three planes' bytes"""
    if isinstance(picture, (tuple, list)):
        picture = b"".join(bytes(p) for p in picture)
    d = np.frombuffer(picture, np.uint8)
    y, c = width * height, (width // 2) * (height // 2)
    return d[:y].reshape(height, width), d[y:y + c].reshape(height // 2, width // 2), d[y + c:y + 2 * c].reshape(height // 2, width // 2)


def picture_sums(a, b, width, height):
    """the three sums of two I420 pictures (bytes, or (y, u, v) bytes)"""
    return [plane_sum(pa, pb) for pa, pb in zip(planes_of(a, width, height), planes_of(b, width, height))]


def _i420(planes):
    return b"".join(np.ascontiguousarray(p, dtype=np.uint8).tobytes() for p in planes)


def content_pairs(width, height, seed=7):
    """{name: (a, b)}: pairs of width x height I420 pictures as bytes"""
    rng = np.random.default_rng([seed, width, height])
    shapes = [(height, width), (height // 2, width // 2), (height // 2, width // 2)]
    noise = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    other = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    stripes = [np.where((np.arange(s[1]) // 4) % 2 == 1, 255, 0).astype(np.uint8)[None, :].repeat(s[0], axis=0) for s in shapes]
    pairs = {
        "noise_noise": (_i420(noise), _i420(other)),
        "noise_inverse": (_i420(noise), _i420([255 - p for p in noise])),
        "identical": (_i420(noise), _i420(noise)),
        "zero_255": (_i420([np.zeros(s, np.uint8) for s in shapes]), _i420([np.full(s, 255, np.uint8) for s in shapes])),
        "stripes_inverse": (_i420(stripes), _i420([255 - p for p in stripes])),
    }
    for content in gen_yuv.CONTENTS:      # two frames of each family of tools/gen_yuv.py
        first, second = list(gen_yuv.gen_frames(width, height, 2, seed=seed, content=content))
        pairs[f"gen_yuv_{content}"] = (_i420(first), _i420(second))
    return pairs


class HostPicture:
    """An I420 picture (bytes) in host memory in one of LAYOUTS: tightly packed, I420 planes at odd offsets and pitches inside larger random buffers, NV12"""

    def __init__(self, picture, width, height, layout, seed=0):
        rng = np.random.default_rng(seed)
        y, u, v = planes_of(picture, width, height)
        self.pic = Picture(format=PIC_NV12 if layout == "nv12" else PIC_I420, reserved=0)
        if layout == "tight_i420":
            geometry = [(y, width, 0), (u, width // 2, 0), (v, width // 2, 0)]
        elif layout == "offset_i420":
            geometry = [(y, width + 13, 1), (u, width // 2 + 7, 3), (v, width // 2 + 3, 5)]
        else:
            geometry = [(y, width + 6, 0), (np.stack([u, v], axis=2).reshape(height // 2, width), width + 6, 1)]
        self.buffers = []
        for c, (plane, pitch, offset) in enumerate(geometry):
            rows, row_bytes = plane.shape
            buf = rng.integers(0, 256, offset + pitch * (rows - 1) + row_bytes, dtype=np.uint8)      # (ends with the plane's last row)
            np.lib.stride_tricks.as_strided(buf[offset:], (rows, row_bytes), (pitch, 1))[:] = plane
            self.buffers.append(buf)
            self.pic.plane[c], self.pic.pitch[c] = buf.ctypes.data + offset, pitch


def host_sums(lib, a, b, width, height, layout_a="tight_i420", layout_b="tight_i420"):
    """hmr_gpu_ssim_host (through picture_gpu.load()'s binding) on two I420 pictures given as bytes"""
    pa, pb = HostPicture(a, width, height, layout_a, seed=1), HostPicture(b, width, height, layout_b, seed=2)
    out = (C.c_int64 * 3)()
    assert lib.hmr_gpu_ssim_host(C.byref(pa.pic), C.byref(pb.pic), width, height, out) == 0, lib.hmr_gpu_last_error()
    return list(out)
