"""RGB egress (include/homer_gpu.h section 12i), the parts that need no GPU: the numpy restatement of tests/rgb_egress_cases.py against the real-valued inverse BT
matrices, hmr_gpu_rgb_from_yuv_host - the arithmetic the kernel compiles (csrc/yuv_rgb.h) - against the restatement byte for byte, the float forms, the round trip through
section 12f, the host sums and PSNR, what the package imports, and what the cross-compile makes of k_egress_rgb."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libs
import rgb_cases as rc
import rgb_egress_cases as re_

ERR_ARG = -3
HIPCC = "/opt/rocm/bin/hipcc"
SIZES = [(2, 2), (4, 2), (2, 4), (6, 10), (34, 18), (200, 136), (416, 240)]
FORMS = sorted(rc.FORMS)


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    lib = C.CDLL(libs.GPU_SO)
    R = C.POINTER(rc.RgbPicture)
    lib.hmr_gpu_rgb_from_yuv_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, R]
    lib.hmr_gpu_rgb_ssd_host.argtypes = [R, R, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    lib.hmr_gpu_psnr_rgb.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.hmr_gpu_rgb_convert_host.argtypes = [R, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


def from_yuv(lib, yuv, form, matrix, full, rng, padded):
    """hmr_gpu_rgb_from_yuv_host into a canvas of the form; checked against the restatement, the bytes around the rows and the alpha byte"""
    y, u, v = (np.ascontiguousarray(p) for p in yuv)
    h, w = y.shape
    canvas = re_.Canvas(form, w, h, rng, padded)
    pic = canvas.descriptor([b.ctypes.data for b in canvas.buffers], matrix, full)
    before = [p.copy() for p in (y, u, v)]
    assert lib.hmr_gpu_rgb_from_yuv_host(y.ctypes.data, u.ctypes.data, v.ctypes.data, w, h, C.byref(pic)) == 0, lib.hmr_gpu_last_error()
    assert all(np.array_equal(a, b) for a, b in zip((y, u, v), before))
    canvas.check(canvas.buffers, re_.restate(y, u, v, matrix, full))


# ---- the restated arithmetic against the real-valued formula ----
@pytest.mark.parametrize("matrix,full", rc.MATRIX_RANGES)
def test_within_0_52_of_the_real_valued_formula(matrix, full):
    """half an LSB of rounding plus at most 0.5 x (16 x 239 + 2 x 2048) / 2^18 = 0.015 of coefficient error (include/homer_gpu.h section 12i): 0.52 - on noise and on
    pictures of the values at which the ranges begin and end"""
    rng = np.random.default_rng(3)
    pictures = [re_.noise_yuv(rng, 256, 256) for _ in range(4)] + [re_.extremes_yuv(rng, 128, 128) for _ in range(4)]
    for ylev in (0, 15, 16, 235, 255):      # flat pictures of the extremes
        for ulev in (0, 16, 240, 255):
            for vlev in (0, 16, 240, 255):
                pictures.append([np.full((4, 4), ylev, np.uint8), np.full((2, 2), ulev, np.uint8), np.full((2, 2), vlev, np.uint8)])
    worst = 0.0
    for y, u, v in pictures:
        got, want = re_.restate(y, u, v, matrix, full), re_.real_valued(y, u, v, matrix, full)
        for name, a, b in zip("RGB", got, want):
            err = np.abs(a.astype(np.float64) - np.clip(b, 0.0, 255.0)).max()
            worst = max(worst, err)
            assert err <= 0.52, (matrix, full, name, err)
    print(f"{matrix} full_range={full}: largest distance to the real-valued formula {worst:.4f}")


@pytest.mark.parametrize("matrix,full", rc.MATRIX_RANGES)
def test_grey_and_flat_chroma(matrix, full):
    ramp = np.tile(np.arange(256, dtype=np.uint8), (4, 1))
    flat = np.full((2, 128), 128, np.uint8)
    r, g, b = re_.restate(ramp, flat, flat, matrix, full)
    assert np.array_equal(r, g) and np.array_equal(g, b)
    if full:
        assert np.array_equal(r, ramp)
    rng = np.random.default_rng(1)
    for level in (0, 1, 127, 128, 255):
        for shape in ((1, 1), (1, 5), (3, 1), (4, 6)):
            assert (re_.chroma16(np.full(shape, level)) == 16 * level).all()
    c = rng.integers(0, 256, (5, 7))
    up = re_.chroma16(c)
    assert up.shape == (10, 14) and up.min() >= 0 and up.max() <= 4080
    assert up[0, 0] == 16 * c[0, 0] and up[-1, -1] == 16 * c[-1, -1] and up[0, 1] == 4 * (3 * c[0, 0] + c[0, 1]) and up[2, 0] == 4 * (c[0, 0] + 3 * c[1, 0])
    assert up[3, 4] == 3 * (c[1, 1] + 3 * c[1, 2]) + (c[2, 1] + 3 * c[2, 2])


def test_coefficients_are_the_rounded_inverse_matrices():
    for (matrix, full), (ky, rv, gu, gv, bu, yoff) in re_.TABLE.items():
        kr, kb = rc.KR_KB[matrix]
        kg = 1.0 - kr - kb
        sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
        want = [sy, sc * 2 * (1 - kr), -sc * 2 * (1 - kb) * kb / kg, -sc * 2 * (1 - kr) * kr / kg, sc * 2 * (1 - kb)]
        assert [ky, rv, gu, gv, bu] == [round(x * 16384) for x in want] and yoff == (0 if full else 16)


# ---- the host conversion against the restatement ----
@pytest.mark.parametrize("matrix,full", rc.MATRIX_RANGES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_conversion_in_every_form(lib, size, matrix, full):
    w, h = size
    rng = np.random.default_rng(w * 7 + h + full)
    for k, form in enumerate(FORMS):
        yuv = re_.extremes_yuv(rng, w, h) if k % 3 == 2 else re_.noise_yuv(rng, w, h)
        for padded in (False, True):
            from_yuv(lib, yuv, form, matrix, full, rng, padded)


# ---- the float forms ----
@pytest.mark.parametrize("form", ["f16", "f32"])
def test_all_256_float_values(lib, form):
    """full range with chroma 128 gives R = G = B = Y: a ramp puts every 8-bit value into the float output"""
    rng = np.random.default_rng(2)
    ramp = np.tile(np.arange(256, dtype=np.uint8), (2, 1))
    flat = np.full((1, 128), 128, np.uint8)
    canvas = re_.Canvas(form, 256, 2, rng, False)
    pic = canvas.descriptor([b.ctypes.data for b in canvas.buffers], "bt709", 1)
    assert lib.hmr_gpu_rgb_from_yuv_host(ramp.ctypes.data, flat.ctypes.data, flat.ctypes.data, 256, 2, C.byref(pic)) == 0, lib.hmr_gpu_last_error()
    chans, _ = canvas.channels(canvas.buffers)
    v = np.arange(256)
    want32 = v.astype(np.float32) / np.float32(255)
    want = want32.astype(np.float16) if form == "f16" else want32
    for got in chans:
        assert got.dtype == want.dtype and np.array_equal(got[0].view(np.uint8), want.view(np.uint8)) and np.array_equal(got[1].view(np.uint8), want.view(np.uint8))
        assert np.array_equal(rc.quantize(got[0]), v)
    assert np.array_equal(rc.quantize(re_.unit(v, form)), v)


# ---- through section 12f and back ----
@pytest.mark.parametrize("matrix,full", rc.MATRIX_RANGES)
def test_round_trip_of_flat_pictures(lib, matrix, full):
    """hmr_gpu_rgb_convert_host, then hmr_gpu_rgb_from_yuv_host: within 1 in full range, within 2 in limited range"""
    rng = np.random.default_rng(9)
    colours = [(255 * ((k >> 2) & 1), 255 * ((k >> 1) & 1), 255 * (k & 1)) for k in range(8)] + [(g, g, g) for g in range(256)] + [tuple(c) for c in rng.integers(0, 256, (4096, 3)).tolist()]
    # a flat picture's chroma is flat after the 2 x 2 average and after the bilinear upsampling: 2 x 2 pixels say what any size says
    w = h = 2
    worst = 0
    y, u, v = np.zeros((h, w), np.uint8), np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8)
    out = np.zeros((3, h, w), np.uint8)
    src = np.zeros((h, w, 3), np.uint8)
    src_pic = rc.descriptor(rc.RGB_PACKED8, 3, (0, 1, 2), [src.ctypes.data], [3 * w], matrix, full)
    out_pic = rc.descriptor(rc.RGB_PLANAR8, 0, (0, 0, 0), [out[c].ctypes.data for c in range(3)], [w] * 3, matrix, full)
    for colour in colours:
        src[:] = colour
        assert lib.hmr_gpu_rgb_convert_host(C.byref(src_pic), w, h, y.ctypes.data, u.ctypes.data, v.ctypes.data) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_rgb_from_yuv_host(y.ctypes.data, u.ctypes.data, v.ctypes.data, w, h, C.byref(out_pic)) == 0, lib.hmr_gpu_last_error()
        err = int(np.abs(out.astype(int) - np.array(colour).reshape(3, 1, 1)).max())
        worst = max(worst, err)
        assert err <= (1 if full else 2), (colour, out[:, 0, 0].tolist())
    print(f"{matrix} full_range={full}: largest round-trip error {worst}")


# ---- sums and PSNR ----
def host_picture(form, chans, rng, padded, matrix="bt709", full=0):
    fmt, pb, offs, planes = rc.lay_out(form, chans, rng, padded)
    return rc.descriptor(fmt, pb, offs, [buf.ctypes.data + base for buf, base, _ in planes], [pitch for _, _, pitch in planes], matrix, full), planes


def test_host_sums_with_mixed_forms(lib):
    rng = np.random.default_rng(4)
    for w, h in ((2, 2), (34, 18), (200, 136)):
        for k, fa in enumerate(FORMS):
            fb = FORMS[(k * 4 + 3) % len(FORMS)]
            a = rc.special_floats(rc.FLOAT_TYPES[fa], rng, w, h) if fa in rc.FLOAT_TYPES else rc.noise(rng, w, h)
            b = rc.special_floats(rc.FLOAT_TYPES[fb], rng, w, h) if fb in rc.FLOAT_TYPES and k & 1 else (rc.as_floats(fb, rng, *rc.noise(rng, w, h)) if fb in rc.FLOAT_TYPES else rc.noise(rng, w, h))
            pa, keep_a = host_picture(fa, a, rng, bool(k & 1), "bt601", 1)
            pb, keep_b = host_picture(fb, b, rng, not k & 1)
            got = (C.c_uint64 * 3)(7, 7, 7)
            assert lib.hmr_gpu_rgb_ssd_host(C.byref(pa), C.byref(pb), w, h, got) == 0, lib.hmr_gpu_last_error()
            assert list(got) == re_.numpy_ssd(rc.eight_bit(fa, a), rc.eight_bit(fb, b)), (fa, fb, w, h)
    same, _ = host_picture("f32", rc.as_floats("f32", rng, *[np.full((2, 2), 9, np.uint8)] * 3), rng, False)
    eight, _ = host_picture("bgra", [np.full((2, 2), 9, np.uint8)] * 3, rng, True)
    got = (C.c_uint64 * 3)(7, 7, 7)
    assert lib.hmr_gpu_rgb_ssd_host(C.byref(same), C.byref(eight), 2, 2, got) == 0 and list(got) == [0, 0, 0]


def test_psnr_rgb(lib):
    out = (C.c_double * 4)()
    for ssd, w, h in (([12345, 678, 9], 416, 240), ([1, 0, 5 * 10 ** 11], 3840, 2160), ([0, 0, 0], 2, 2), ([255 * 255 * 4] * 3, 2, 2)):
        assert lib.hmr_gpu_psnr_rgb((C.c_uint64 * 3)(*ssd), w, h, out) == 0, lib.hmr_gpu_last_error()
        want = [10.0 * math.log10(255.0 * 255.0 * w * h / s) if s else 99.99 for s in ssd]
        want.append(10.0 * math.log10(255.0 * 255.0 * 3.0 * w * h / sum(ssd)) if sum(ssd) else 99.99)
        assert all(abs(a - b) <= 1e-9 for a, b in zip(out, want)), (ssd, list(out), want)      # (one log10 in double on either side: a few ulp of about 50)
    assert lib.hmr_gpu_psnr_rgb((C.c_uint64 * 3)(0, 0, 0), 2, 2, out) == 0 and list(out) == [99.99] * 4
    from homerhevc_amd import psnr_rgb
    assert all(abs(a - b) <= 1e-9 for a, b in zip(psnr_rgb([12345, 678, 9], 416, 240), [10.0 * math.log10(255.0 * 255.0 * 416 * 240 / s) for s in (12345, 678, 9)]))
    assert len(psnr_rgb([0, 0, 0], 2, 2)) == 4 and psnr_rgb([0, 0, 0], 2, 2)[3] == 99.99
    with pytest.raises(ValueError):
        psnr_rgb([1, 2], 2, 2)
    with pytest.raises(ValueError):
        psnr_rgb([1, 2, 3], 3, 2)


# ---- refusals ----
def test_refusals(lib):
    rng = np.random.default_rng(6)
    y, u, v = re_.noise_yuv(rng, 4, 4)
    out = np.zeros((3, 4, 4), np.uint8)
    good = rc.descriptor(rc.RGB_PLANAR8, 0, (0, 0, 0), [out[c].ctypes.data for c in range(3)], [4] * 3, "bt709", 0)
    narrow = rc.descriptor(rc.RGB_PLANAR8, 0, (0, 0, 0), [out[c].ctypes.data for c in range(3)], [4, 3, 4], "bt709", 0)
    ssd, res = (C.c_uint64 * 3)(), (C.c_double * 4)()
    P = lambda a: a.ctypes.data
    refused = {
        "from_yuv: NULL y": lambda: lib.hmr_gpu_rgb_from_yuv_host(None, P(u), P(v), 4, 4, C.byref(good)),
        "from_yuv: NULL v": lambda: lib.hmr_gpu_rgb_from_yuv_host(P(y), P(u), None, 4, 4, C.byref(good)),
        "from_yuv: NULL descriptor": lambda: lib.hmr_gpu_rgb_from_yuv_host(P(y), P(u), P(v), 4, 4, None),
        "from_yuv: odd width": lambda: lib.hmr_gpu_rgb_from_yuv_host(P(y), P(u), P(v), 3, 4, C.byref(good)),
        "from_yuv: odd height": lambda: lib.hmr_gpu_rgb_from_yuv_host(P(y), P(u), P(v), 4, 3, C.byref(good)),
        "from_yuv: pitch below a row": lambda: lib.hmr_gpu_rgb_from_yuv_host(P(y), P(u), P(v), 4, 4, C.byref(narrow)),
        "ssd: NULL a": lambda: lib.hmr_gpu_rgb_ssd_host(None, C.byref(good), 4, 4, ssd),
        "ssd: NULL b": lambda: lib.hmr_gpu_rgb_ssd_host(C.byref(good), None, 4, 4, ssd),
        "ssd: NULL sums": lambda: lib.hmr_gpu_rgb_ssd_host(C.byref(good), C.byref(good), 4, 4, None),
        "ssd: odd width": lambda: lib.hmr_gpu_rgb_ssd_host(C.byref(good), C.byref(good), 3, 4, ssd),
        "ssd: bad descriptor": lambda: lib.hmr_gpu_rgb_ssd_host(C.byref(good), C.byref(narrow), 4, 4, ssd),
        "psnr: NULL sums": lambda: lib.hmr_gpu_psnr_rgb(None, 4, 4, res),
        "psnr: NULL results": lambda: lib.hmr_gpu_psnr_rgb(ssd, 4, 4, None),
        "psnr: odd height": lambda: lib.hmr_gpu_psnr_rgb(ssd, 4, 5, res),
        "psnr: zero width": lambda: lib.hmr_gpu_psnr_rgb(ssd, 0, 4, res),
    }
    for why, call in refused.items():
        assert lib.hmr_gpu_rgb_ssd_host(C.byref(good), C.byref(good), 4, 4, ssd) == 0      # (so that the text below is this refusal's)
        assert call() == ERR_ARG and lib.hmr_gpu_last_error(), why
    assert (out == 0).all()


# ---- the package and the header ----
def test_package_exports_and_import_needs_neither_torch_nor_the_library():
    code = ("import homerhevc_amd, homerhevc_amd.encoder as m; assert 'torch' not in sys.modules, 'torch imported'; assert homerhevc_amd.psnr_rgb is m.psnr_rgb; "
            "assert m.Encoder.export_rgb and m.BatchEncoder.export_rgb; assert m._lib is None and m._host_lib is None, 'the native library was loaded'; "
            "assert 'torch' not in sys.modules, 'torch imported'")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {libs.ROOT!r}); " + code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_enc_export_pictures_rgb_device", "hmr_gpu_enc_export_picture_rgb_device", "hmr_gpu_rgb_from_yuv_host", "hmr_gpu_rgb_ssd_host", "hmr_gpu_psnr_rgb"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert "12i." in text and text.index("12h.") < text.index("12i.") < text.index(" 13. ")
    for row in re_.TABLE.values():      # the table a caller reproduces the samples from
        assert re.search(r"\s+".join(str(k).replace("-", r"\-") for k in row), text), row


# ---- the kernel as compiled ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_rgb_egress_kernel_as_compiled():
    """k_egress_rgb for gfx950: no private memory, no spills, global_ (not flat_) accesses, 16-byte loads and stores"""
    remarks, asm = libs.picture_io_as_compiled()
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        seen[blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]): (\d+)", blk)}
    names = [n for n in seen if "k_egress_rgb" in n]
    assert len(names) == 1, sorted(seen)
    f = seen[names[0]]
    print(f)
    # (the job's record, 52 dwords, is held in scalar registers: the compiler parks some scalars in lanes of a vector register - not in memory - which the report counts
    # as spilled SGPRs; reading the record where it lies instead turns every use into a vector load per lane)
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0, f
    assert f["VGPRs"] <= 128 and f["Occupancy [waves/SIMD]"] >= 4, f      # (DESIGN.md records 123 and 4)
    body = asm[asm.index(names[0] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    code = [l.split(";")[0] for l in body.splitlines()]
    assert not [l for l in code if "flat_" in l or "scratch_" in l]
    # 16-byte accesses: the four chroma loads and two luma loads of a span, the reference's rows, and 3 + 4 + 3 + 6 + 12 stores of a row in the five output forms
    assert sum("global_load_dwordx4" in l for l in code) >= 6 + 3 + 4 + 3 + 6 and sum("global_store_dwordx4" in l for l in code) >= 3 + 4 + 3 + 6 + 12
