"""Deep, 4:2:2 and 4:4:4 Y'CbCr pictures (include/homer_gpu.h section 12k), the parts that need no GPU: the host check of a descriptor, hmr_gpu_yuv_convert_host - the
arithmetic the kernel compiles (csrc/yuv_depth.h) - against the numpy restatement of tests/yuv_cases.py byte for byte, the properties the header states, the golden
digests, what the package imports, and what the cross-compile makes of k_ingest_yuv."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libs
import yuv_cases as yc
from homerhevc_amd.encoder import Picture
from homerhevc_amd.encoder import YuvPicture as PackageYuvPicture

ERR_ARG = -3
W, H = 416, 240
SOME = 0x1000          # any non-NULL, even value: the check never follows a pointer
HIPCC = "/opt/rocm/bin/hipcc"
SIZES = [(2, 2), (8, 8), (200, 136), (416, 240)]
GOLDEN = os.path.join(libs.ROOT, "tests", "golden", "yuv_ingest.json")


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    lib = C.CDLL(libs.GPU_SO)
    lib.hmr_gpu_yuv_picture_check.argtypes = [C.POINTER(yc.YuvPicture), C.c_int, C.c_int]
    lib.hmr_gpu_yuv_convert_host.argtypes = [C.POINTER(yc.YuvPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_picture_check.argtypes = [C.POINTER(Picture), C.c_int, C.c_int]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


# ---- the descriptor check ----
def row_bytes(form, w=W):
    fmt, chroma, bits, _, _ = yc.FORMS[form]
    sb, wc = yc.sample_bytes(bits), yc.chroma_size(chroma, w, 2)[0]
    if fmt == yc.YUV_PLANAR:
        return [w * sb, wc * sb, wc * sb]
    return [w * sb, 2 * wc * sb] if fmt == yc.YUV_SEMIPLANAR else [2 * w * sb]


def desc(form, pad=0, **kw):
    """a good descriptor of the form at pitches of a row's bytes plus `pad` samples, then changed by the keywords (plane0 .. plane2, pitch0 .. pitch2, offset0 .. offset2, fields)"""
    sb = yc.sample_bytes(yc.FORMS[form][2])
    rows = row_bytes(form)
    pic = yc.descriptor(form, [SOME + 64 * c for c in range(len(rows))], [n + pad * sb for n in rows])
    for k, v in kw.items():
        if k[-1].isdigit():
            getattr(pic, k[:-1])[int(k[-1])] = v
        else:
            setattr(pic, k, v)
    return pic


@pytest.mark.parametrize("form", yc.NAMES)
def test_descriptors_that_are_accepted(lib, form):
    for pad in (0, 7):
        assert lib.hmr_gpu_yuv_picture_check(C.byref(desc(form, pad)), W, H) == 0, lib.hmr_gpu_last_error()
    pic = yc.descriptor(form, [SOME + 64 * c for c in range(len(row_bytes(form, 2)))], row_bytes(form, 2))
    assert lib.hmr_gpu_yuv_picture_check(C.byref(pic), 2, 2) == 0, lib.hmr_gpu_last_error()


REFUSED = {
    "unknown format": (desc("planar_420_8", format=3), W, H, b"format"),
    "negative format": (desc("planar_420_8", format=-1), W, H, b"format"),
    "unknown chroma": (desc("planar_444_8", chroma=3), W, H, b"chroma"),
    "negative chroma": (desc("semi_uv_420_10msb", chroma=-1), W, H, b"chroma"),
    "bits 7": (desc("planar_420_8", bits=7), W, H, b"bits"),
    "bits 17": (desc("planar_420_16", bits=17), W, H, b"bits"),
    "msb_aligned 2": (desc("semi_uv_420_10msb", msb_aligned=2), W, H, b"msb_aligned"),
    "msb_aligned -1": (desc("planar_422_12", msb_aligned=-1), W, H, b"msb_aligned"),
    "msb_aligned with 8 bits": (desc("planar_420_8", msb_aligned=1), W, H, b"msb_aligned"),
    "msb_aligned with 16 bits": (desc("semi_vu_444_16", msb_aligned=1), W, H, b"msb_aligned"),
    "reserved": (desc("yuyv_8", reserved=1), W, H, b"reserved"),
    "odd width": (desc("planar_420_8", 7), W + 1, H, b"width"),
    "odd height": (desc("semi_uv_422_10"), W, H - 1, b"height"),
    "zero width": (desc("uyvy_8"), 0, H, b"width"),
    "negative height": (desc("planar_444_16"), W, -2, b"height"),
    "packed 4:2:0": (desc("yuyv_8", chroma=0), W, H, b"chroma"),
    "packed 4:4:4": (desc("y210", chroma=2), W, H, b"chroma"),
    "planar with an offset": (desc("planar_422_8", offset1=1), W, H, b"offset[1]"),
    "planar with a luma offset": (desc("planar_420_10", offset0=1), W, H, b"offset[0]"),
    "semi-planar with a luma offset": (desc("semi_uv_420_8", offset0=1), W, H, b"offset[0]"),
    "semi-planar offset 2": (desc("semi_uv_420_8", offset2=2), W, H, b"offset[2]"),
    "semi-planar negative offset": (desc("semi_vu_444_12", offset1=-1), W, H, b"offset[1]"),
    "semi-planar offsets repeated": (desc("semi_uv_422_10msb", offset2=0), W, H, b"offset[2]"),
    "packed luma offset 2": (desc("yuyv_8", offset0=2), W, H, b"offset[0]"),
    "packed chroma offset 4": (desc("uyvy_8", offset2=4), W, H, b"offset[2]"),
    "packed negative offset": (desc("yvyu_8", offset1=-1), W, H, b"offset[1]"),
    "packed chroma at a luma place": (desc("yuyv_8", offset1=2), W, H, b"offset[1]"),
    "packed V at the first luma place": (desc("vyuy_8", offset2=1), W, H, b"offset[2]"),
    "packed offsets repeated": (desc("y210", offset2=1), W, H, b"offset[2]"),
    "no luma plane": (desc("planar_420_8", plane0=None), W, H, b"plane[0]"),
    "no U plane": (desc("planar_422_10", plane1=None), W, H, b"plane[1]"),
    "no V plane": (desc("planar_444_16", plane2=None), W, H, b"plane[2]"),
    "no plane of pairs": (desc("semi_uv_420_10msb", plane1=None), W, H, b"plane[1]"),
    "no packed plane": (desc("uyvy_8", plane0=None), W, H, b"plane[0]"),
    "third plane with SEMIPLANAR": (desc("semi_vu_420_8", plane2=SOME), W, H, b"plane[2]"),
    "second plane with PACKED422": (desc("yuyv_8", plane1=SOME), W, H, b"plane[1]"),
    "third plane with PACKED422": (desc("y210", plane2=SOME), W, H, b"plane[2]"),
    "negative pitch": (desc("planar_420_8", pitch2=-W), W, H, b"pitch[2]"),
    "negative packed pitch": (desc("yuyv_8", pitch0=-2 * W), W, H, b"pitch[0]"),
    "luma pitch below a row": (desc("planar_420_8", pitch0=W - 1), W, H, b"pitch[0]"),
    "16-bit luma pitch below a row": (desc("semi_uv_420_10msb", pitch0=2 * W - 2), W, H, b"pitch[0]"),
    "4:2:0 chroma pitch below a row": (desc("planar_420_8", pitch1=W // 2 - 1), W, H, b"pitch[1]"),
    "4:4:4 chroma pitch below a row": (desc("planar_444_8", pitch2=W - 1), W, H, b"pitch[2]"),
    "pairs' pitch below a row": (desc("semi_uv_422_8", pitch1=W - 1), W, H, b"pitch[1]"),
    "4:4:4 pairs' pitch below a row": (desc("semi_vu_444_16", pitch1=4 * W - 2), W, H, b"pitch[1]"),
    "packed pitch below a row": (desc("vyuy_8", pitch0=2 * W - 1), W, H, b"pitch[0]"),
    "Y210 pitch below a row": (desc("y210", pitch0=4 * W - 2), W, H, b"pitch[0]"),
    "16-bit plane at an odd address": (desc("planar_420_10", plane1=SOME + 1), W, H, b"plane[1]"),
    "16-bit packed plane at an odd address": (desc("y210", plane0=SOME + 3), W, H, b"plane[0]"),
    "16-bit pitch odd": (desc("semi_uv_420_10msb", pitch1=2 * W + 1), W, H, b"pitch[1]"),
    "16-bit luma pitch odd": (desc("planar_444_16", pitch0=2 * W + 3), W, H, b"pitch[0]"),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_descriptors_that_are_refused(lib, why):
    pic, w, h, field = REFUSED[why]
    assert lib.hmr_gpu_yuv_picture_check(C.byref(desc("planar_420_8")), W, H) == 0      # (so that the error text below is this refusal's)
    assert lib.hmr_gpu_yuv_picture_check(C.byref(pic), w, h) == ERR_ARG
    text = lib.hmr_gpu_last_error()
    assert text and field in text, text
    out = np.zeros(8, np.uint8)
    assert lib.hmr_gpu_yuv_convert_host(C.byref(pic), w, h, out.ctypes.data, out.ctypes.data, out.ctypes.data) == ERR_ARG      # (refused before a pointer is followed)


def test_null_is_refused(lib):
    assert lib.hmr_gpu_yuv_picture_check(None, W, H) == ERR_ARG
    assert lib.hmr_gpu_last_error()
    out = np.zeros(4, np.uint8)
    assert lib.hmr_gpu_yuv_convert_host(None, 2, 2, out.ctypes.data, out.ctypes.data, out.ctypes.data) == ERR_ARG
    src = np.zeros(16, np.uint8)
    pic = yc.descriptor("yuyv_8", [src.ctypes.data], [4])
    assert lib.hmr_gpu_yuv_convert_host(C.byref(pic), 2, 2, out.ctypes.data, None, out.ctypes.data) == ERR_ARG


def test_the_8_bit_descriptor_still_refuses_format_2(lib):
    p = Picture(format=2, reserved=0)
    for c in range(3):
        p.plane[c], p.pitch[c] = SOME + c, W
    assert lib.hmr_gpu_picture_check(C.byref(p), W, H) == ERR_ARG
    assert b"format" in lib.hmr_gpu_last_error()


def test_descriptor_struct_is_the_tests_mirror():
    assert [(n, t) for n, t in PackageYuvPicture._fields_] == [(n, t) for n, t in yc.YuvPicture._fields_]
    assert C.sizeof(PackageYuvPicture) == C.sizeof(yc.YuvPicture) == 80
    assert yc.YuvPicture.offset.offset == 16 and yc.YuvPicture.reserved.offset == 28 and yc.YuvPicture.plane.offset == 32 and yc.YuvPicture.pitch.offset == 56


# ---- the host conversion against the restatement ----
def convert(lib, form, planes3, rng, padded):
    """hmr_gpu_yuv_convert_host on the picture laid out in host memory: (y, u, v) as arrays"""
    h, w = planes3[0].shape
    planes = yc.lay_out(form, *planes3, rng, padded)
    before = [buf.copy() for buf, _, _ in planes]
    pic = yc.descriptor(form, [buf.ctypes.data + base for buf, base, _ in planes], [pitch for _, _, pitch in planes])
    guard = 64
    out = [np.full(n + 2 * guard, 0xA5, np.uint8) for n in (w * h, w * h // 4, w * h // 4)]
    assert lib.hmr_gpu_yuv_convert_host(C.byref(pic), w, h, *[o.ctypes.data + guard for o in out]) == 0, lib.hmr_gpu_last_error()
    for o in out:
        assert (o[:guard] == 0xA5).all() and (o[-guard:] == 0xA5).all()
    for (buf, _, _), b in zip(planes, before):
        assert np.array_equal(buf, b)
    return out[0][guard:-guard].reshape(h, w), out[1][guard:-guard].reshape(h // 2, w // 2), out[2][guard:-guard].reshape(h // 2, w // 2)


def same(lib, form, planes3, rng, padded=True):
    got = convert(lib, form, planes3, rng, padded)
    want = yc.restate(form, *planes3)
    for name, g, x in zip("YUV", got, want):
        assert np.array_equal(g, x), (form, name, np.argwhere(g != x)[:4].tolist())
    return got


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_noise_in_every_form(lib, size):
    w, h = size
    rng = np.random.default_rng(w * 7 + h)
    for k, form in enumerate(yc.NAMES):
        same(lib, form, yc.noise(form, rng, w, h), rng, padded=bool(k & 1))


def shaped(form, rng, luma, chroma_u, chroma_v):
    """pictures given as functions of (yy, xx) index grids, evaluated on the form's luma and chroma grids, reduced to the container's range"""
    _, chroma, bits, _, _ = yc.FORMS[form]
    top = 256 if bits == 8 else 65536
    w, h = 48, 16
    wc, hc = yc.chroma_size(chroma, w, h)
    out = []
    for fn, (rows, cols) in ((luma, (h, w)), (chroma_u, (hc, wc)), (chroma_v, (hc, wc))):
        yy, xx = np.mgrid[0:rows, 0:cols]
        out.append((np.asarray(fn(yy, xx, top)) % top).astype(yc.container_type(bits)))
    return out


def test_corners_ramps_and_checkerboards(lib):
    """the container's extremes, ramps over its whole range and along both axes, checkerboards at sample, row and 2 x 2 block period"""
    rng = np.random.default_rng(5)
    flat = lambda value: (lambda yy, xx, top: np.full(yy.shape, value(top)))
    board = lambda cell_y, cell_x: (lambda yy, xx, top: np.where((yy // cell_y + xx // cell_x) & 1, top - 1, 0))
    pictures = [(flat(a), flat(b), flat(c))
                for a, b, c in [(lambda t: 0,) * 3, (lambda t: t - 1,) * 3, (lambda t: 0, lambda t: t - 1, lambda t: 0), (lambda t: t - 1, lambda t: 0, lambda t: t - 1),
                                (lambda t: t // 2, lambda t: t // 2 - 1, lambda t: t // 2 + 1)]]
    pictures.append((lambda yy, xx, top: (yy * 48 + xx) * top // 768, lambda yy, xx, top: xx * top // 48, lambda yy, xx, top: yy * top // 16))     # ramps
    pictures.append((lambda yy, xx, top: (yy * 48 + xx) * 257 + 128, lambda yy, xx, top: xx * 1031 + yy, lambda yy, xx, top: top - 1 - xx * 523 - yy * 77))     # finer ramps, wrapped
    pictures.append((board(1, 1), board(1, 1), board(1, 10 ** 6)))        # sample period; V: row period
    pictures.append((board(1, 10 ** 6), board(1, 10 ** 6), board(1, 1)))  # row period
    pictures.append((board(2, 2), board(2, 2), board(10 ** 6, 1)))        # block period; V: column period
    for form in yc.NAMES:
        for luma, cu, cv in pictures:
            same(lib, form, shaped(form, rng, luma, cu, cv), rng)


# ---- the properties the header states ----
@pytest.mark.parametrize("form", yc.NAMES)
def test_within_half_of_the_real_valued_average_and_the_clamp_rule(form):
    """every output is within 0.5 of the real-valued average of v / 2^s; where that average is >= 255.5 the result is 255: the restatement on noise and on every pair of
    extreme taps"""
    rng = np.random.default_rng(3)
    _, chroma, bits, msb, _ = yc.FORMS[form]
    top = 256 if bits == 8 else 65536
    pictures = [yc.noise(form, rng, 128, 64) for _ in range(2)]
    edge = np.array([0, 1, top // 2 - 1, top // 2, top - 2, top - 1] + ([(1 << bits) - 2, (1 << bits) - 1, 1 << bits] if not msb and bits < 16 else []))
    taps = rng.choice(edge, (64, 64)).astype(yc.container_type(bits))
    wc, hc = yc.chroma_size(chroma, 64, 64)
    pictures.append([taps, rng.choice(edge, (hc, wc)).astype(taps.dtype), rng.choice(edge, (hc, wc)).astype(taps.dtype)])
    for planes3 in pictures:
        got, real = yc.restate(form, *planes3), yc.real_valued(form, *planes3)
        for name, g, x in zip("YUV", got, real):
            g = g.astype(np.float64)
            clamped = x >= 255.5
            assert (g[clamped] == 255).all(), (form, name)
            assert np.abs(g[~clamped] - x[~clamped]).max() <= 0.5, (form, name, np.abs(g[~clamped] - x[~clamped]).max())


def test_the_header_s_examples():
    one = lambda form, value, shape_c: yc.restate(form, np.full((2, 2), value), np.full(shape_c, value), np.full(shape_c, value))
    assert [int(p[0, 0]) for p in one("planar_420_10", 1023, (1, 1))] == [255, 255, 255]
    assert [int(p[0, 0]) for p in one("planar_444_16", 65535, (2, 2))] == [255, 255, 255]
    # 10-bit limited range stays limited range
    for form, shape_c in (("planar_420_10", (1, 1)), ("planar_422_10", (2, 1)), ("planar_444_10", (2, 2))):
        for ten, eight in ((64, 16), (940, 235), (960, 240), (512, 128), (0, 0)):
            assert [int(p[0, 0]) for p in one(form, ten, shape_c)] == [eight] * 3, (form, ten)
    assert [int(p[0, 0]) for p in one("semi_uv_420_10msb", 940 << 6, (1, 2))][0] == 235


def test_8_bit_420_is_the_identity(lib):
    rng = np.random.default_rng(12)
    for form in ("planar_420_8", "semi_uv_420_8", "semi_vu_420_8"):
        y, u, v = yc.noise(form, rng, 200, 136)
        got = same(lib, form, [y, u, v], rng)
        assert np.array_equal(got[0], y) and np.array_equal(got[1], u) and np.array_equal(got[2], v)


@pytest.mark.parametrize("form", yc.NAMES)
def test_a_widened_8_bit_picture_comes_back(lib, form):
    """v << s in either alignment (dirty low bits under an msb-aligned sample), the widened chroma constant over its taps"""
    rng = np.random.default_rng(13)
    _, chroma, _, _, _ = yc.FORMS[form]
    w, h = 72, 40
    y8, u8, v8 = (rng.integers(0, 256, shape, dtype=np.uint8) for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    wc, hc = yc.chroma_size(chroma, w, h)
    spread = lambda p: p.repeat(hc // (h // 2), axis=0).repeat(wc // (w // 2), axis=1)
    got = same(lib, form, yc.widened(form, y8, spread(u8), spread(v8), rng), rng)
    assert np.array_equal(got[0], y8) and np.array_equal(got[1], u8) and np.array_equal(got[2], v8), form


# ---- the golden digests ----
def digest(planes):
    return hashlib.sha256(b"".join(np.ascontiguousarray(p).tobytes() for p in planes)).hexdigest()


def test_golden_digests(lib):
    """tests/golden/yuv_ingest.json (minted by tests/golden/make_yuv_ingest_golden.py): the restatement and the host twin both still give the recorded pictures"""
    gold = json.load(open(GOLDEN))
    assert sorted(gold["sha256"]) == yc.NAMES and (gold["width"], gold["height"]) == (64, 48)
    rng = np.random.default_rng(0)
    for form in yc.NAMES:
        planes3 = yc.golden_picture(form, gold["width"], gold["height"])
        assert digest(yc.restate(form, *planes3)) == gold["sha256"][form], ("the restatement", form)
        assert digest(convert(lib, form, planes3, rng, True)) == gold["sha256"][form], ("hmr_gpu_yuv_convert_host", form)


# ---- the package and the header ----
def test_package_import_needs_neither_torch_nor_a_gpu():
    code = ("import homerhevc_amd, homerhevc_amd.encoder as m; assert 'torch' not in sys.modules, 'torch imported'; assert homerhevc_amd.YUVFrame is m.YUVFrame; "
            "f = m.YUVFrame((None, None), chroma='422', bits=10, msb_aligned=True, order='vu'); assert (f.chroma, f.bits, f.msb_aligned, f.offsets) == ('422', 10, True, (0, 1, 0)); "
            "assert m.YUVFrame(None, chroma='422', order='uyvy').offsets == (1, 0, 2); assert m.yuv_picture_of and m.YuvPicture; assert 'torch' not in sys.modules, 'torch imported'")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {libs.ROOT!r}); " + code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from homerhevc_amd.encoder import ScaledFrame, YUVFrame
    for bad in (dict(chroma="411"), dict(bits=7), dict(bits=17), dict(order="yuyv")):
        with pytest.raises(ValueError):
            YUVFrame((None, None, None), **bad)
    with pytest.raises(ValueError):
        YUVFrame(None, chroma="420")
    with pytest.raises(ValueError):
        YUVFrame((None, None), order="yuyv")
    with pytest.raises(TypeError):
        ScaledFrame(YUVFrame((None, None, None)), 1920, 1080)


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_yuv_picture_check", "hmr_gpu_yuv_convert_host", "hmr_gpu_enc_load_source_yuv_device", "hmr_gpu_enc_load_sources_yuv_device"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert re.search(r"^typedef struct hmr_gpu_yuv_picture \{", text, re.M)
    assert "12k." in text
    for name, value in (("HMR_GPU_YUV_PLANAR", 0), ("HMR_GPU_YUV_SEMIPLANAR", 1), ("HMR_GPU_YUV_PACKED422", 2), ("HMR_GPU_CHROMA_420", 0), ("HMR_GPU_CHROMA_422", 1), ("HMR_GPU_CHROMA_444", 2)):
        assert re.search(name + r" = %d\b" % value, text), name


# ---- the kernel as compiled ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_yuv_ingest_kernel_as_compiled():
    """k_ingest_yuv for gfx950, from the compiler's resource remarks alone: no private memory, no spills, and as many waves a SIMD as k_ingest_rgb in the same compile"""
    remarks, asm = libs.picture_io_as_compiled()
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        seen[blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]): (\d+)", blk)}
    yuv, rgb = [n for n in seen if "k_ingest_yuv" in n], [n for n in seen if "k_ingest_rgb" in n]
    assert len(yuv) == 1 and len(rgb) == 1, sorted(seen)
    f, g = seen[yuv[0]], seen[rgb[0]]
    print(f, g)
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
    assert f["Occupancy [waves/SIMD]"] >= g["Occupancy [waves/SIMD]"], (f, g)
