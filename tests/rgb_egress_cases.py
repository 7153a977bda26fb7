"""RGB egress for the tests of include/homer_gpu.h section 12i: a numpy restatement of the section's arithmetic, written from its formulas and its table (the comparator of
every test - it never calls the library), the real-valued inverse BT matrices in float64, and output pictures in every form the interface writes, laid out in host buffers
at odd addresses and padded pitches with random bytes around the rows."""
import numpy as np

import rgb_cases as rc

# Ky, Rv, Gu, Gv, Bu, yoff
TABLE = {
    ("bt601", 0): (19077, 26149, -6419, -13320, 33050, 16),
    ("bt601", 1): (16384, 22970, -5638, -11700, 29032, 0),
    ("bt709", 0): (19077, 29372, -3494, -8731, 34610, 16),
    ("bt709", 1): (16384, 25802, -3069, -7670, 30402, 0),
}
ELEM = {rc.RGB_PLANAR8: 1, rc.RGB_PLANAR_F16: 2, rc.RGB_PLANAR_F32: 4}


def _taps(n):
    """per luma position 0 .. 2 n - 1 of an axis with n chroma samples: the two clamped chroma indices and the weight of the first (the second has 4 minus it)"""
    p = np.arange(2 * n)
    first = np.where(p & 1, p >> 1, (p >> 1) - 1)      # an even position takes c - 1 (weight 1) and c (3), an odd one c (3) and c + 1 (1)
    return np.clip(first, 0, n - 1), np.clip(first + 1, 0, n - 1), np.where(p & 1, 3, 1)


def chroma16(c):
    """a chroma plane [h / 2, w / 2] at every luma position [h, w]: bilinear, scaled by 16, not rounded"""
    c = np.asarray(c).astype(np.int64)
    y0, y1, wy = _taps(c.shape[0])
    x0, x1, wx = _taps(c.shape[1])
    rows = wy[:, None] * c[y0] + (4 - wy)[:, None] * c[y1]
    return wx[None, :] * rows[:, x0] + (4 - wx)[None, :] * rows[:, x1]


def restate(y, u, v, matrix, full_range):
    """section 12i in numpy: 8-bit Y [h, w], U, V [h / 2, w / 2] -> (R, G, B) [h, w] as uint8"""
    ky, rv, gu, gv, bu, yoff = TABLE[(matrix, int(full_range))]
    l = 16 * ky * (np.asarray(y).astype(np.int64) - yoff)
    u16, v16 = chroma16(u) - 2048, chroma16(v) - 2048
    assert max(np.abs(l + rv * v16).max(), np.abs(l + gu * u16 + gv * v16).max(), np.abs(l + bu * u16).max()) + 131072 < 1.5e8
    r, g, b = ((s + 131072) >> 18 for s in (l + rv * v16, l + gu * u16 + gv * v16, l + bu * u16))
    return [np.clip(p, 0, 255).astype(np.uint8) for p in (r, g, b)]


def restate_bytes(planes, w, h, matrix, full_range):
    """... of an I420 picture given as (y, u, v) bytes or as one bytes object"""
    data = np.frombuffer(planes if isinstance(planes, (bytes, bytearray)) else b"".join(planes), np.uint8)
    y, u, v = data[:w * h].reshape(h, w), data[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), data[w * h * 5 // 4:].reshape(h // 2, w // 2)
    return restate(y, u, v, matrix, full_range)


def real_valued(y, u, v, matrix, full_range):
    """the inverse BT matrix in float64 on 8-bit Y and the SAME bilinear chroma (C16 / 16): (R, G, B), not rounded, not clamped"""
    kr, kb = rc.KR_KB[matrix]
    kg = 1.0 - kr - kb
    yy = np.asarray(y).astype(np.float64)
    cb, cr = chroma16(u) / 16.0 - 128.0, chroma16(v) / 16.0 - 128.0
    if not full_range:
        yy, cb, cr = (yy - 16.0) * 255.0 / 219.0, cb * 255.0 / 224.0, cr * 255.0 / 224.0
    return yy + 2.0 * (1.0 - kr) * cr, yy - 2.0 * (1.0 - kb) * kb / kg * cb - 2.0 * (1.0 - kr) * kr / kg * cr, yy + 2.0 * (1.0 - kb) * cb


def unit(v, form):
    """the float output of 8-bit values: one binary32 division, then - for binary16 - one rounding to nearest even"""
    x = np.asarray(v).astype(np.float32) / np.float32(255)
    return x.astype(np.float16) if form == "f16" else x


def noise_yuv(rng, w, h):
    return [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)]


def extremes_yuv(rng, w, h):
    """every sample one of the values at which a range begins or ends"""
    return [rng.choice(np.array([0, 15, 16, 235, 255], np.uint8), (h, w)), rng.choice(np.array([0, 16, 240, 255], np.uint8), (h // 2, w // 2)),
            rng.choice(np.array([0, 16, 240, 255], np.uint8), (h // 2, w // 2))]


class Canvas:
    """An output picture of one form in host memory (rc.lay_out's geometry: odd base addresses, padded pitches, random bytes around the rows).  `buffers` are what the
    call writes into - or, for a device test, what is uploaded and downloaded; channels(buffers) gathers R, G, B (and the alpha bytes) and asserts that every byte outside
    the rows is what it was."""

    def __init__(self, form, w, h, rng, padded=True):
        self.form, self.w, self.h = form, w, h
        fmt = rc.FORMS[form][0]
        dtype = rc.FLOAT_TYPES.get(form, np.uint8)
        self.fmt, self.pixel_bytes, self.offsets, planes = rc.lay_out(form, [np.zeros((h, w), dtype)] * 3, rng, padded)
        self.geometry = [(base, pitch) for _, base, pitch in planes]
        self.before = []
        for buf, base, pitch in planes:      # (the rows themselves start as random bytes too)
            buf[:] = rng.integers(0, 256, buf.size, dtype=np.uint8)
            self.before.append(buf.copy())
        self.buffers = [b.copy() for b in self.before]
        self.row_bytes = w * (self.pixel_bytes if fmt == rc.RGB_PACKED8 else ELEM[fmt])

    def descriptor(self, addresses, matrix, full_range):
        return rc.descriptor(self.fmt, self.pixel_bytes, self.offsets, [a + base for a, (base, _) in zip(addresses, self.geometry)], [pitch for _, pitch in self.geometry], matrix, full_range)

    def rows(self, buf, k):
        base, pitch = self.geometry[k]
        return np.lib.stride_tricks.as_strided(buf[base:], (self.h, self.row_bytes), (pitch, 1))

    def channels(self, buffers):
        """([R, G, B] as the form's element type, the alpha bytes or None)"""
        got = []
        for k, (buf, before) in enumerate(zip(buffers, self.before)):
            after = np.array(buf, copy=True)
            got.append(self.rows(after, k).copy())
            self.rows(after, k)[:] = self.rows(before, k)
            assert np.array_equal(after, before), f"{self.form}: bytes outside the picture's rows were written"
        if self.fmt == rc.RGB_PACKED8:
            px = got[0].reshape(self.h, self.w, self.pixel_bytes)
            alpha = px[:, :, 6 - sum(self.offsets)] if self.pixel_bytes == 4 else None
            return [px[:, :, o] for o in self.offsets], alpha
        dtype = rc.FLOAT_TYPES.get(self.form, np.uint8)
        return [np.ascontiguousarray(p).view(dtype).reshape(self.h, self.w) for p in got], None

    def check(self, buffers, rgb):
        """the buffers hold the 8-bit picture `rgb` in this form, bit for bit, an alpha byte of 255, and nothing else was written"""
        chans, alpha = self.channels(buffers)
        for name, got, want in zip("RGB", chans, rgb):
            want = unit(want, self.form) if self.form in rc.FLOAT_TYPES else want
            bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[want.dtype.itemsize]
            same = got.view(bits) == want.view(bits)
            assert same.all(), (self.form, name, int((~same).sum()), np.argwhere(~same)[:4].tolist(), got[~same][:4].tolist(), want[~same][:4].tolist())
        assert alpha is None or (alpha == 255).all(), (self.form, "the alpha byte is not 255")


def numpy_ssd(ref8, rgb):
    """the three sums of squared differences between the 8-bit reference channels and the 8-bit picture"""
    return [int(((np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)) ** 2).sum()) for a, b in zip(ref8, rgb)]
