"""Helper of the scene-cut tests (include/homer_gpu.h section 12m): the argument types of the section's four functions (picture_gpu.py's table stops at 12k), a
restatement of the section's arithmetic that shares nothing with the library - numpy on integer arrays (no value leaves 32 bits before it is summed in 64), by brute force over the 289 shifts, never a call into the
library - the content pairs the tests run on, and pictures in host memory in the layouts hmr_gpu_cut_stats_host takes."""
import ctypes as C
import os
import sys

import numpy as np

import encoder_cases as ec
from homerhevc_amd.encoder import PIC_I420, PIC_NV12, Picture

sys.path.insert(0, os.path.join(ec.ROOT, "tools"))
import gen_yuv  # noqa: E402

VALUES, RANGE = 8, 8
SAD_Y, SAD_U, SAD_V, HIST, INTRA, INTER, NINTRA, LUMA = range(8)
MAX_ACT = 522240
LAYOUTS = ["tight_i420", "pitched_i420", "tight_nv12", "pitched_nv12"]
SHIFTS = [(8, -8), (-8, 8), (7, 3), (0, -8)]
FAMILIES = list(gen_yuv.CONTENTS)


def declare(lib):
    """the argument types of section 12m's four functions, and of nothing else, onto a handle of the library (picture_gpu.load()'s: its table stops at 12k)"""
    P, I = C.c_void_p, C.c_int
    lib.hmr_gpu_enc_cut_stats.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(I), P, P]
    lib.hmr_gpu_enc_cut_stats_one.argtypes = [P, I, I, P, P]
    lib.hmr_gpu_cut_stats_host.argtypes = [C.POINTER(Picture), C.POINTER(Picture), I, I, C.POINTER(C.c_int64)]
    lib.hmr_gpu_cut_score.argtypes = [C.POINTER(C.c_int64), I, I, C.POINTER(C.c_double)]
    return lib


# ---- the restatement ----
def block_terms(cur, prev):
    """(act, msad) of every 8 x 8 block of the luma planes cur against prev (2-D uint8 arrays of one shape, multiples of 8), as integer arrays [H / 8, W / 8]"""
    cur, prev = cur.astype(np.int32), prev.astype(np.int32)
    H, W = cur.shape
    assert cur.shape == prev.shape and H % 8 == 0 and W % 8 == 0 and H > 0 and W > 0
    bh, bw = H // 8, W // 8
    blocks = cur.reshape(bh, 8, bw, 8)
    S = blocks.sum(axis=(1, 3))
    act = np.abs(64 * blocks - S[:, None, :, None]).sum(axis=(1, 3))
    assert act.max() <= MAX_ACT
    msad = np.full((bh, bw), 1 << 30, np.int64)
    for dy in range(-RANGE, RANGE + 1):
        for dx in range(-RANGE, RANGE + 1):
            # the blocks whose displaced position lies wholly inside the picture: 0 <= 8 b + d and 8 b + d + 8 <= size
            x_lo, x_hi = (-dx + 7) // 8 if dx < 0 else 0, min(bw, (W - 8 - dx) // 8 + 1)
            y_lo, y_hi = (-dy + 7) // 8 if dy < 0 else 0, min(bh, (H - 8 - dy) // 8 + 1)
            if x_lo >= x_hi or y_lo >= y_hi:
                continue
            a = cur[8 * y_lo:8 * y_hi, 8 * x_lo:8 * x_hi]
            b = prev[8 * y_lo + dy:8 * y_hi + dy, 8 * x_lo + dx:8 * x_hi + dx]
            sad = np.abs(a - b).reshape(y_hi - y_lo, 8, x_hi - x_lo, 8).sum(axis=(1, 3))
            msad[y_lo:y_hi, x_lo:x_hi] = np.minimum(msad[y_lo:y_hi, x_lo:x_hi], sad)
    assert msad.max() <= 64 * 255      # (0, 0) is valid for every block
    return act, msad


def restate(cur, prev, width, height):
    """the eight values of two I420 pictures (bytes, or (y, u, v) bytes), as Python ints"""
    (cy, cu, cv), (py, pu, pv) = planes_of(cur, width, height), planes_of(prev, width, height)
    sads = [int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum()) for a, b in ((cy, py), (cu, pu), (cv, pv))]
    hist = int(np.abs(np.bincount(cy.ravel(), minlength=256).astype(np.int64) - np.bincount(py.ravel(), minlength=256).astype(np.int64)).sum())
    assert 0 <= hist <= 2 * width * height
    act, msad = block_terms(cy, py)
    return sads + [hist, int(act.sum()), int(np.minimum(64 * msad, act).sum()), int((act < 64 * msad).sum()), int(cy.astype(np.int64).sum())]


def planes_of(picture, width, height):
    """(y, u, v) as 2-D uint8 arrays of an I420 picture given as bytes or as three planes' bytes"""
    if isinstance(picture, (tuple, list)):
        picture = b"".join(bytes(p) for p in picture)
    d = np.frombuffer(picture, np.uint8)
    y, c = width * height, (width // 2) * (height // 2)
    return d[:y].reshape(height, width), d[y:y + c].reshape(height // 2, width // 2), d[y + c:y + 2 * c].reshape(height // 2, width // 2)


def _i420(planes):
    return b"".join(np.ascontiguousarray(p, dtype=np.uint8).tobytes() for p in planes)


# ---- the content ----
def shifted(prev, other, dx, dy):
    """a luma plane whose sample (x, y) is prev's (x + dx, y + dy) wherever that lies inside the picture, and `other`'s elsewhere: a block displaced by (dx, dy) finds itself"""
    h, w = prev.shape
    out = other.copy()
    xs, ys = np.arange(w), np.arange(h)
    inside_x, inside_y = (xs + dx >= 0) & (xs + dx < w), (ys + dy >= 0) & (ys + dy < h)
    out[np.ix_(inside_y, inside_x)] = prev[np.ix_(ys[inside_y] + dy, xs[inside_x] + dx)]
    return out


def content_pairs(width, height, seed=7):
    """{name: (cur, prev)}: pairs of width x height I420 pictures as bytes"""
    rng = np.random.default_rng([seed, width, height])
    shapes = [(height, width), (height // 2, width // 2), (height // 2, width // 2)]
    noise = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    other = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    stripes = [np.where((np.arange(s[1]) // 4) % 2 == 1, 255, 0).astype(np.uint8)[None, :].repeat(s[0], axis=0) for s in shapes]
    zero, full = [np.zeros(s, np.uint8) for s in shapes], [np.full(s, 255, np.uint8) for s in shapes]
    pairs = {
        "identical": (_i420(noise), _i420(noise)),
        "zero_255": (_i420(zero), _i420(full)),
        "255_zero": (_i420(full), _i420(zero)),
        "stripes_inverse": (_i420(stripes), _i420([255 - p for p in stripes])),
        "noise_noise": (_i420(noise), _i420(other)),
        "shift_9": (_i420([shifted(noise[0], other[0], 9, 0)] + other[1:]), _i420(noise)),
    }
    for dx, dy in SHIFTS:
        pairs[f"shift_{dx}_{dy}"] = (_i420([shifted(noise[0], other[0], dx, dy)] + other[1:]), _i420(noise))
    for content in FAMILIES:      # frames 0, 1, 2 of each family of tools/gen_yuv.py with a cut in front of frame 1
        frames = list(gen_yuv.gen_frames(width, height, 3, seed=seed, cut_at=1, content=content))
        pairs[f"gen_yuv_{content}_cut"] = (_i420(frames[1]), _i420(frames[0]))
        pairs[f"gen_yuv_{content}_next"] = (_i420(frames[2]), _i420(frames[1]))
    return pairs


class HostPicture:
    """An I420 picture (bytes) in host memory in one of LAYOUTS: I420 or NV12, tightly packed or at odd offsets and pitches inside larger random buffers"""

    def __init__(self, picture, width, height, layout, seed=0):
        rng = np.random.default_rng(seed)
        y, u, v = planes_of(picture, width, height)
        nv12, pitched = layout.endswith("nv12"), layout.startswith("pitched")
        self.pic = Picture(format=PIC_NV12 if nv12 else PIC_I420, reserved=0)
        if nv12:
            geometry = [(y, width + (6 if pitched else 0), 0), (np.stack([u, v], axis=2).reshape(height // 2, width), width + (10 if pitched else 0), 1 if pitched else 0)]
        else:
            geometry = [(y, width + (13 if pitched else 0), 1 if pitched else 0), (u, width // 2 + (7 if pitched else 0), 3 if pitched else 0), (v, width // 2 + (3 if pitched else 0), 5 if pitched else 0)]
        self.buffers = []
        for c, (plane, pitch, offset) in enumerate(geometry):
            rows, row_bytes = plane.shape
            buf = rng.integers(0, 256, offset + pitch * (rows - 1) + row_bytes, dtype=np.uint8)      # (ends with the plane's last row)
            np.lib.stride_tricks.as_strided(buf[offset:], (rows, row_bytes), (pitch, 1))[:] = plane
            self.buffers.append(buf)
            self.pic.plane[c], self.pic.pitch[c] = buf.ctypes.data + offset, pitch


def host_stats(lib, cur, prev, width, height, layout_cur="tight_i420", layout_prev="tight_i420"):
    """hmr_gpu_cut_stats_host (through a handle that declare() has seen) on two I420 pictures given as bytes"""
    a, b = HostPicture(cur, width, height, layout_cur, seed=1), HostPicture(prev, width, height, layout_prev, seed=2)
    out = (C.c_int64 * VALUES)()
    assert lib.hmr_gpu_cut_stats_host(C.byref(a.pic), C.byref(b.pic), width, height, out) == 0, lib.hmr_gpu_last_error()
    return list(out)


def score(lib, stats, width, height):
    out = (C.c_double * 4)()
    assert lib.hmr_gpu_cut_score((C.c_int64 * VALUES)(*stats), width, height, out) == 0, lib.hmr_gpu_last_error()
    return list(out)


def is_intra(au):
    """an Annex-B access unit holds parameter sets and an IDR slice: what the encoder writes for slice type I, and for nothing else"""
    types, at = [], au.find(b"\x00\x00\x01")
    while 0 <= at < len(au) - 3:
        types.append((au[at + 3] >> 1) & 0x3f)
        at = au.find(b"\x00\x00\x01", at + 3)
    assert types, "no NAL unit"
    return 32 in types and any(16 <= t <= 23 for t in types)
