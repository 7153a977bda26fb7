"""Pictures for the tests of include/homer_gpu.h section 12g: a numpy restatement of the section's area-averaging arithmetic, written from its formulas in Python integers
(the comparator of every test - it never calls the library), the size pairs the tests run, picture contents, and 4:2:0 source pictures laid out in host buffers at odd
addresses and padded pitches with random bytes around the rows."""
import ctypes as C
from math import gcd

import numpy as np

PIC_I420, PIC_NV12 = 0, 1
# (source, destination) sizes: 2 : 1, 3 : 2, nearly 1 : 1 with the largest sx sy, the 540 of the header, one axis only, 8 : 1, the identity, one output per chroma plane
PAIRS = [((400, 272), (200, 136)), ((300, 204), (200, 136)), ((330, 266), (328, 264)), ((1920, 1080), (416, 240)), ((416, 480), (416, 240)), ((1600, 1088), (200, 136)),
         ((200, 136), (200, 136)), ((32, 16), (2, 2))]
CONTENTS = ["noise", "zeros", "ones", "checkerboard"]


class Picture(C.Structure):
    """hmr_gpu_picture"""
    _fields_ = [("format", C.c_int32), ("reserved", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int64 * 3)]


class ScaledPicture(C.Structure):
    """hmr_gpu_scaled_picture"""
    _fields_ = [("pic", Picture), ("width", C.c_int32), ("height", C.c_int32)]


def pair_id(pair):
    (ws, hs), (wd, hd) = pair
    return f"{ws}x{hs}-{wd}x{hd}"


def reduced(S, D):
    g = gcd(S, D)
    return S // g, D // g


def taps(S, D):
    """the taps of one axis: [(source index [D], weight [D])], at most ceil(S / D) + 1 of them; w(x, i) = min((x + 1) s, (i + 1) d) - max(x s, i d) where that is
    positive, 0 (with any valid index) elsewhere.  Integers throughout."""
    s, d = reduced(S, D)
    x = np.arange(D, dtype=np.int64)
    lo, hi = x * s, (x + 1) * s
    first = lo // d
    out, total = [], np.zeros(D, np.int64)
    for k in range(-(-S // D) + 1):
        i = first + k
        w = np.minimum(hi, (i + 1) * d) - np.maximum(lo, i * d)
        w = np.where((w > 0) & (i < S), w, 0)
        out.append((np.minimum(i, S - 1), w))
        total += w
    assert (total == s).all()      # the weights of one output sum to s: no tap beyond ceil(S / D) + 1
    return out


def reduce_rows(src, D):
    """[S, n] -> [D, n]: the weighted sums along the first axis, nothing divided"""
    acc = np.zeros((D, src.shape[1]), src.dtype)
    for i, w in taps(src.shape[0], D):
        acc += w[:, None].astype(src.dtype) * src[i]
    return acc


def restate_plane(src, D_w, D_h):
    """one plane [Hs, Ws] -> [D_h, D_w]: (sum_j sum_i wy wx src + (sx sy >> 1)) // (sx sy), one rounding"""
    src = np.asarray(src).astype(np.int64)
    hs, ws = src.shape
    den = reduced(ws, D_w)[0] * reduced(hs, D_h)[0]
    assert den * 255 + (den >> 1) < 1 << 32
    out = (reduce_rows(reduce_rows(src, D_h).T, D_w).T + (den >> 1)) // den
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def restate(planes, dst_w, dst_h):
    """section 12g in numpy: (Y [hs, ws], U, V [hs / 2, ws / 2]) -> (Y [dst_h, dst_w], U, V [dst_h / 2, dst_w / 2]) as uint8; every plane on its own"""
    y, u, v = planes
    return restate_plane(y, dst_w, dst_h), restate_plane(u, dst_w // 2, dst_h // 2), restate_plane(v, dst_w // 2, dst_h // 2)


def real_valued_plane(src, D_w, D_h):
    """the area average in float64 (the same weights, summed and divided in floating point): what every output has to be within 0.5 of"""
    src = np.asarray(src).astype(np.float64)
    hs, ws = src.shape
    den = reduced(ws, D_w)[0] * reduced(hs, D_h)[0]
    return reduce_rows(reduce_rows(src, D_h).T, D_w).T / den


def content(kind, rng, w, h):
    """(Y [h, w], U, V [h / 2, w / 2]) as uint8"""
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    if kind == "noise":
        return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    if kind == "zeros":
        return [np.zeros(s, np.uint8) for s in shapes]
    if kind == "ones":
        return [np.full(s, 255, np.uint8) for s in shapes]
    assert kind == "checkerboard"
    return [(((np.add.outer(np.arange(s[0]), np.arange(s[1]))) & 1) * 255).astype(np.uint8) for s in shapes]


def as_bytes(planes):
    return b"".join(np.ascontiguousarray(p).tobytes() for p in planes)


def embed(rng, rows2d, pitch, offset):
    """the rows at byte `offset` and pitch `pitch` of a buffer of random bytes that ends with the last row"""
    rows, row_bytes = rows2d.shape
    buf = rng.integers(0, 256, offset + pitch * (rows - 1) + row_bytes, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(buf[offset:], (rows, row_bytes), (pitch, 1))[:] = rows2d
    return buf


def lay_out(planes, fmt, rng, padded=True):
    """the picture in host buffers: [(buffer, offset of the plane, pitch)] - I420: three planes, NV12: luma and the interleaved pairs.  padded: odd base addresses and
    pitches beyond a row's bytes; else tightly packed buffers of their own"""
    y, u, v = planes
    h, w = y.shape
    if fmt == PIC_NV12:
        uv = np.stack([u, v], axis=2).reshape(h // 2, w)
        parts = [(y, w + 6, 3), (uv, w + 10, 1)]
    else:
        parts = [(y, w + 13, 1), (u, w // 2 + 7, 2), (v, w // 2 + 3, 3)]
    out = []
    for rows2d, pitch, offset in parts:
        if not padded:
            pitch, offset = rows2d.shape[1], 0
        out.append((embed(rng, rows2d, pitch, offset), offset, pitch))
    return out


def descriptor(fmt, addresses, pitches, width, height):
    pic = ScaledPicture(width=width, height=height)
    pic.pic.format, pic.pic.reserved = fmt, 0
    for c, (a, p) in enumerate(zip(addresses, pitches)):
        pic.pic.plane[c], pic.pic.pitch[c] = a, p
    return pic
