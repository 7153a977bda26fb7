"""Y'CbCr pictures for the tests of include/homer_gpu.h section 12k: a numpy restatement of the section's arithmetic, written from its text (the comparator of every
test - it never calls the library), the set F of forms the tests cover, and pictures in every form, laid out in host buffers at odd, sample-aligned addresses and padded
pitches."""
import ctypes as C
import zlib

import numpy as np

YUV_PLANAR, YUV_SEMIPLANAR, YUV_PACKED422 = 0, 1, 2
CHROMA = {"420": 0, "422": 1, "444": 2}
DEPTHS = {"8": (8, 0), "10": (10, 0), "10msb": (10, 1), "12": (12, 0), "16": (16, 0)}
PACKED = {"yuyv": (0, 1, 3), "uyvy": (1, 0, 2), "yvyu": (0, 3, 1), "vyuy": (1, 2, 0)}

# F: name -> (format, chroma as "420" / "422" / "444", bits, msb_aligned, offset[3])
FORMS = {}
for _layout, (_fmt, _offs) in {"planar": (YUV_PLANAR, (0, 0, 0)), "semi_uv": (YUV_SEMIPLANAR, (0, 0, 1)), "semi_vu": (YUV_SEMIPLANAR, (0, 1, 0))}.items():
    for _chroma in CHROMA:
        for _depth, (_bits, _msb) in DEPTHS.items():
            FORMS[f"{_layout}_{_chroma}_{_depth}"] = (_fmt, _chroma, _bits, _msb, _offs)
for _order, _offs in PACKED.items():
    FORMS[f"{_order}_8"] = (YUV_PACKED422, "422", 8, 0, _offs)
FORMS["y210"] = (YUV_PACKED422, "422", 10, 1, PACKED["yuyv"])
assert len(FORMS) == 3 * 3 * 5 + 5
NAMES = sorted(FORMS)


class YuvPicture(C.Structure):
    """hmr_gpu_yuv_picture"""
    _fields_ = [("format", C.c_int32), ("chroma", C.c_int32), ("bits", C.c_int32), ("msb_aligned", C.c_int32), ("offset", C.c_int32 * 3), ("reserved", C.c_int32),
                ("plane", C.c_void_p * 3), ("pitch", C.c_int64 * 3)]


def sample_bytes(bits):
    return 1 if bits == 8 else 2


def chroma_size(chroma, w, h):
    """(Wc, Hc) of the SOURCE's chroma planes"""
    return (w if chroma == "444" else w // 2), (h // 2 if chroma == "420" else h)


def r(t):
    return 1 << (t - 1) if t else 0


def values(raw, bits, msb):
    """v of the containers' values"""
    raw = np.asarray(raw).astype(np.int64)
    return raw >> (16 - bits) if msb else np.minimum(raw, (1 << bits) - 1)


def restate(form, y, u, v):
    """section 12k in numpy: the containers' values y [h, w], u, v [Hc, Wc] -> (Y [h, w], U, V [h / 2, w / 2]) as uint8"""
    _, chroma, bits, msb, _ = FORMS[form]
    s, k = bits - 8, CHROMA[chroma]
    luma = np.minimum(255, (values(y, bits, msb) + r(s)) >> s)
    out = [luma]
    for plane in (u, v):
        val = values(plane, bits, msb)
        hc, wc = val.shape
        if k == 1:
            val = val[0::2] + val[1::2]
        elif k == 2:
            val = val.reshape(hc // 2, 2, wc // 2, 2).sum(axis=(1, 3))
        out.append(np.minimum(255, (val + r(s + k)) >> (s + k)))
    assert all(p.min() >= 0 for p in out)
    return tuple(p.astype(np.uint8) for p in out)


def real_valued(form, y, u, v):
    """the real-valued averages of v / 2^s: (Y [h, w], U, V [h / 2, w / 2]) in float64, not rounded, not clamped"""
    _, chroma, bits, msb, _ = FORMS[form]
    s, k = bits - 8, CHROMA[chroma]
    out = [values(y, bits, msb).astype(np.float64) / (1 << s)]
    for plane in (u, v):
        val = values(plane, bits, msb).astype(np.float64) / (1 << s)
        hc, wc = val.shape
        if k == 1:
            val = (val[0::2] + val[1::2]) / 2.0
        elif k == 2:
            val = val.reshape(hc // 2, 2, wc // 2, 2).mean(axis=(1, 3))
        out.append(val)
    return out


def container_type(bits):
    return np.uint8 if bits == 8 else np.dtype("<u2")


def noise(form, rng, w, h):
    """noise over the full container range: bits above `bits` set in low-aligned forms (the min), dirty low bits in msb-aligned ones (the shift drops them)"""
    _, chroma, bits, _, _ = FORMS[form]
    wc, hc = chroma_size(chroma, w, h)
    top = 256 if bits == 8 else 65536
    planes = [rng.integers(0, top, shape).astype(container_type(bits)) for shape in ((h, w), (hc, wc), (hc, wc))]
    if bits not in (8, 16):      # half of the samples inside the nominal range, so that not everything clamps in the low-aligned forms
        for p in planes:
            inside = rng.random(p.shape) < 0.5
            p[inside] &= (1 << bits) - 1
    return planes


def widened(form, y8, u8, v8, rng=None):
    """8-bit planes (chroma already of the form's chroma size) as the form's containers: v << s at the form's alignment; msb-aligned forms get dirty low bits from rng"""
    _, _, bits, msb, _ = FORMS[form]
    out = []
    for p in (y8, u8, v8):
        q = np.asarray(p).astype(np.int64) << (bits - 8)
        if msb:
            q = q << (16 - bits)
            if rng is not None:
                q = q | rng.integers(0, 1 << (16 - bits), q.shape)
        out.append(q.astype(container_type(bits)))
    return out


def golden_picture(form, w=64, h=48):
    """the seeded picture of tests/golden/yuv_ingest.json for this form"""
    return noise(form, np.random.default_rng(zlib.crc32(form.encode())), w, h)


def lay_out(form, y, u, v, rng, padded):
    """The picture in host memory.  y, u, v: the containers' values.  padded: odd base addresses in samples (a multiple of the container's bytes, never of 16) and pitches
    beyond a row's bytes, random bytes around the rows; every buffer ends with its plane's last row.
    Returns planes = [(buffer as uint8 array, byte offset of the plane in it, pitch in bytes)]."""
    fmt, chroma, bits, _, offs = FORMS[form]
    sb, t = sample_bytes(bits), container_type(bits)
    h, w = y.shape

    def embed(rows, base, pitch):
        rows = np.ascontiguousarray(rows.astype(t)).view(np.uint8).reshape(rows.shape[0], -1)
        n, row_bytes = rows.shape
        buf = rng.integers(0, 256, base + pitch * (n - 1) + row_bytes, dtype=np.uint8)
        np.lib.stride_tricks.as_strided(buf[base:], (n, row_bytes), (pitch, 1))[:] = rows
        return buf, base, pitch

    def place(c, rows):
        row_bytes = rows.shape[1] * sb
        return embed(rows, sb * (1 + 2 * c) if padded else 0, row_bytes + (sb * (13, 7, 3)[c] if padded else 0))

    if fmt == YUV_PLANAR:
        return [place(0, y), place(1, u), place(2, v)]
    if fmt == YUV_SEMIPLANAR:
        pairs = np.zeros((u.shape[0], u.shape[1], 2), t)
        pairs[:, :, offs[1]], pairs[:, :, offs[2]] = u, v
        return [place(0, y), place(1, pairs.reshape(u.shape[0], -1))]
    groups = np.zeros((h, w // 2, 4), t)
    groups[:, :, offs[0]], groups[:, :, offs[0] + 2] = y[:, 0::2], y[:, 1::2]
    groups[:, :, offs[1]], groups[:, :, offs[2]] = u, v
    return [place(0, groups.reshape(h, -1))]


def descriptor(form, addresses, pitches):
    fmt, chroma, bits, msb, offs = FORMS[form]
    pic = YuvPicture(format=fmt, chroma=CHROMA[chroma], bits=bits, msb_aligned=msb, reserved=0)
    for c in range(3):
        pic.offset[c] = offs[c]
        pic.plane[c] = addresses[c] if c < len(addresses) else None
        pic.pitch[c] = pitches[c] if c < len(pitches) else 0
    return pic
