"""RGB pictures for the tests of include/homer_gpu.h section 12f: a numpy restatement of the section's arithmetic, written from its formulas and its table (the comparator
of every test - it never calls the library), and RGB pictures in every form the interface takes, laid out in host buffers at odd addresses and padded pitches."""
import ctypes as C

import numpy as np

RGB_PACKED8, RGB_PLANAR8, RGB_PLANAR_F16, RGB_PLANAR_F32 = 0, 1, 2, 3
MATRIX_RANGES = [("bt601", 0), ("bt601", 1), ("bt709", 0), ("bt709", 1)]
MATRIX_ID = {"bt601": 0, "bt709": 1}
# (Yr, Yg, Yb), (Ur, Ug, Ub), (Vr, Vg, Vb), yoff
TABLE = {
    ("bt601", 0): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681), 16),
    ("bt601", 1): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329), 0),
    ("bt709", 0): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639), 16),
    ("bt709", 1): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005), 0),
}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
# form -> (format, pixel bytes, byte of R, G, B)
FORMS = {"rgb": (RGB_PACKED8, 3, (0, 1, 2)), "bgr": (RGB_PACKED8, 3, (2, 1, 0)), "rgba": (RGB_PACKED8, 4, (0, 1, 2)), "bgra": (RGB_PACKED8, 4, (2, 1, 0)),
         "argb": (RGB_PACKED8, 4, (1, 2, 3)), "abgr": (RGB_PACKED8, 4, (3, 2, 1)), "planar8": (RGB_PLANAR8, 0, (0, 0, 0)), "f16": (RGB_PLANAR_F16, 0, (0, 0, 0)),
         "f32": (RGB_PLANAR_F32, 0, (0, 0, 0))}
FLOAT_TYPES = {"f16": np.float16, "f32": np.float32}


class RgbPicture(C.Structure):
    """hmr_gpu_rgb_picture"""
    _fields_ = [("format", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32), ("reserved", C.c_int32), ("pixel_bytes", C.c_int32), ("offset", C.c_int32 * 3),
                ("plane", C.c_void_p * 3), ("pitch", C.c_int64 * 3)]


def quantize(x):
    """a float sample as 8 bits: q = x > 0 ? (x < 1 ? x : 1) : 0 (NaN: 0), rint(float32(q) * float32(255))"""
    x = np.asarray(x).astype(np.float32)      # (binary16 widens exactly)
    with np.errstate(invalid="ignore"):
        q = np.where(x > 0, np.where(x < 1, x, np.float32(1)), np.float32(0)).astype(np.float32)
    return np.rint(q * np.float32(255)).astype(np.int64)


def restate(r, g, b, matrix, full_range):
    """section 12f in numpy: 8-bit R, G, B [h, w] -> (Y [h, w], U, V [h / 2, w / 2]) as uint8"""
    (yr, yg, yb), ku, kv, yoff = TABLE[(matrix, int(full_range))]
    r, g, b = (np.asarray(p).astype(np.int64) for p in (r, g, b))
    h, w = r.shape
    y = ((yr * r + yg * g + yb * b + 32768) >> 16) + yoff
    sr, sg, sb = (p.reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3)) for p in (r, g, b))
    u, v = (np.clip(((k[0] * sr + k[1] * sg + k[2] * sb + 131072) >> 18) + 128, 0, 255) for k in (ku, kv))
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


def real_valued(r, g, b, matrix, full_range):
    """the BT formula in float64 on 8-bit R, G, B [h, w]: (Y' [h, w], Cb, Cr [h / 2, w / 2] of the 2 x 2 averages), not rounded, not clamped"""
    kr, kb = KR_KB[matrix]
    r, g, b = (np.asarray(p).astype(np.float64) for p in (r, g, b))
    h, w = r.shape
    luma = lambda r, g, b: kr * r + (1.0 - kr - kb) * g + kb * b
    ar, ag, ab = (p.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3)) for p in (r, g, b))
    ey, ay = luma(r, g, b), luma(ar, ag, ab)
    cb, cr = (ab - ay) / (2.0 * (1.0 - kb)), (ar - ay) / (2.0 * (1.0 - kr))
    if full_range:
        return ey, 128.0 + cb, 128.0 + cr
    return 16.0 + 219.0 / 255.0 * ey, 128.0 + 224.0 / 255.0 * cb, 128.0 + 224.0 / 255.0 * cr


def as_floats(form, rng, r, g, b):
    """8-bit planes as float planes of the form's type that quantize back to them - v / 255 - with a little noise well inside the rounding interval"""
    t = FLOAT_TYPES[form]
    out = []
    for p in (r, g, b):
        x = p.astype(np.float64) / 255.0
        if t is np.float32:
            x = x + rng.uniform(-0.3, 0.3, p.shape) / 255.0
        out.append(x.astype(t))
    return out


def special_floats(t, rng, w, h):
    """float planes with what a model can leave in them: NaN, infinities, negatives, values above 1, the exact halves (k + 0.5) / 255, subnormals, signed zeros, and noise"""
    bits = {np.float16: np.uint16, np.float32: np.uint32}[t]
    mantissa = {np.float16: 10, np.float32: 23}[t]
    special = np.concatenate([
        np.array([np.nan, -np.nan, np.inf, -np.inf, -1.0, -0.25, -1e-8, 0.0, -0.0, 1.0, 1.0009765625, 1.5, 2.0, 255.0, 65504.0, 0.5, 0.25, 0.001953125, 0.998046875, 0.99951171875]).astype(t),
        ((np.arange(256) + 0.5) / 255.0).astype(t),
        (np.arange(256) / 255.0).astype(t),
        np.nextafter(((np.arange(256) + 0.5) / 255.0).astype(t), t(2)), np.nextafter(((np.arange(256) + 0.5) / 255.0).astype(t), t(-1)),
        rng.integers(1, 1 << mantissa, 64).astype(bits).view(t),                               # positive subnormals
        (rng.integers(1, 1 << mantissa, 16).astype(bits) | bits(1 << (mantissa + (5 if t is np.float16 else 8)))).view(t),      # negative subnormals
        np.array([1, (1 << mantissa) - 1], bits).view(t),                                       # the smallest and the largest subnormal
        rng.integers(0, np.iinfo(bits).max, 512, dtype=np.uint64).astype(bits).view(t),          # any bit pattern at all
    ])
    planes = []
    for _ in range(3):
        p = rng.uniform(-0.2, 1.2, (h, w)).astype(t)
        where = rng.random((h, w)) < 0.5
        p[where] = rng.choice(special, int(where.sum()))
        planes.append(p)
    return planes


def lay_out(form, chans, rng, padded):
    """The picture in host memory.  chans: three [h, w] arrays - uint8 for the 8-bit forms, float16 / float32 for the float forms.  padded: odd base addresses (a multiple
    of the element size, never of 16) and pitches beyond a row's bytes, random bytes around the rows; every buffer ends with its plane's last row.
    Returns (format, pixel_bytes, offsets, planes) with planes = [(buffer as uint8 array, byte offset of the plane in it, pitch in bytes)]."""
    fmt, pixel_bytes, offsets = FORMS[form]
    h, w = chans[0].shape
    planes = []

    def embed(rows, base, pitch):
        row_bytes = rows.shape[1]
        buf = rng.integers(0, 256, base + pitch * (h - 1) + row_bytes, dtype=np.uint8)
        np.lib.stride_tricks.as_strided(buf[base:], (h, row_bytes), (pitch, 1))[:] = rows
        return buf, base, pitch

    if fmt == RGB_PACKED8:
        px = rng.integers(0, 256, (h, w, pixel_bytes), dtype=np.uint8)      # (the fourth byte: anything)
        for c in range(3):
            px[:, :, offsets[c]] = chans[c]
        planes.append(embed(px.reshape(h, w * pixel_bytes), 3 if padded else 0, w * pixel_bytes + (5 if padded else 0)))
        return fmt, pixel_bytes, offsets, planes
    elem = chans[0].dtype.itemsize
    assert elem == {RGB_PLANAR8: 1, RGB_PLANAR_F16: 2, RGB_PLANAR_F32: 4}[fmt]
    for c in range(3):
        rows = np.ascontiguousarray(chans[c]).view(np.uint8).reshape(h, w * elem)
        planes.append(embed(rows, elem * (1 + 2 * c) if padded else 0, elem * (w + ((13, 7, 3)[c] if padded else 0))))
    return fmt, pixel_bytes, offsets, planes


def descriptor(fmt, pixel_bytes, offsets, addresses, pitches, matrix, full_range):
    pic = RgbPicture(format=fmt, matrix=MATRIX_ID[matrix], full_range=int(full_range), reserved=0, pixel_bytes=pixel_bytes)
    for c in range(3):
        pic.offset[c] = offsets[c]
        pic.plane[c] = addresses[c] if c < len(addresses) else None
        pic.pitch[c] = pitches[c] if c < len(pitches) else 0
    return pic


def eight_bit(form, chans):
    """the 8-bit R, G, B the arithmetic starts from"""
    return [quantize(p) for p in chans] if form in FLOAT_TYPES else [np.asarray(p).astype(np.int64) for p in chans]


def noise(rng, w, h):
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]


def yuv_to_rgb(planes, w, h):
    """a fixed mapping from a clip's 4:2:0 picture (y, u, v bytes) to something that looks natural as RGB: BT.601 full range, chroma repeated 2 x 2"""
    y = np.frombuffer(planes[0], np.uint8).reshape(h, w).astype(np.float64)
    u, v = (np.frombuffer(p, np.uint8).reshape(h // 2, w // 2).repeat(2, axis=0).repeat(2, axis=1).astype(np.float64) - 128.0 for p in planes[1:])
    rgb = (y + 1.402 * v, y - 0.344136 * u - 0.714136 * v, y + 1.772 * u)
    return [np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in rgb]
