"""RGB pictures (include/homer_gpu.h section 12f), the parts that need no GPU: the host check of an RGB descriptor, hmr_gpu_rgb_convert_host - the arithmetic the kernel
compiles (csrc/rgb_yuv.h) - against the numpy restatement of tests/rgb_cases.py byte for byte, the restated arithmetic against the real-valued BT formulas, what the package
imports, and what the cross-compile makes of k_ingest_rgb."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libs
import rgb_cases as rc
from homerhevc_amd.encoder import Picture
from homerhevc_amd.encoder import RgbPicture as PackageRgbPicture

ERR_ARG = -3
W, H = 416, 240
SOME = 0x1000          # any non-NULL value: the check never follows a pointer
HIPCC = "/opt/rocm/bin/hipcc"
SIZES = [(2, 2), (8, 8), (200, 136), (416, 240), (1920, 1080)]


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    lib = C.CDLL(libs.GPU_SO)
    lib.hmr_gpu_rgb_picture_check.argtypes = [C.POINTER(rc.RgbPicture), C.c_int, C.c_int]
    lib.hmr_gpu_rgb_convert_host.argtypes = [C.POINTER(rc.RgbPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_picture_check.argtypes = [C.POINTER(Picture), C.c_int, C.c_int]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


# ---- the descriptor check ----
def tight(form, w=W):
    fmt, pb, offs = rc.FORMS[form]
    elem = pb if fmt == rc.RGB_PACKED8 else {rc.RGB_PLANAR8: 1, rc.RGB_PLANAR_F16: 2, rc.RGB_PLANAR_F32: 4}[fmt]
    return fmt, pb, offs, elem, w * elem


def desc(form, pad=0, **kw):
    """a good descriptor of the form at a pitch of a row's bytes plus `pad` elements, then changed by the keywords (plane0 .. plane2, pitch0 .. pitch2, offset0 .. offset2, fields)"""
    fmt, pb, offs, elem, row = tight(form)
    planes = 1 if fmt == rc.RGB_PACKED8 else 3
    pic = rc.descriptor(fmt, pb, offs, [SOME + 64 * c for c in range(planes)], [row + pad * (1 if fmt == rc.RGB_PACKED8 else elem)] * planes, "bt709", 0)
    for k, v in kw.items():
        if k[-1].isdigit():
            getattr(pic, k[:-1])[int(k[-1])] = v
        else:
            setattr(pic, k, v)
    return pic


@pytest.mark.parametrize("form", sorted(rc.FORMS))
def test_descriptors_that_are_accepted(lib, form):
    for pad in (0, 7):
        for matrix in (0, 1):
            for full in (0, 1):
                assert lib.hmr_gpu_rgb_picture_check(C.byref(desc(form, pad, matrix=matrix, full_range=full)), W, H) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_rgb_picture_check(C.byref(desc(form)), 2, 2) == 0, lib.hmr_gpu_last_error()


REFUSED = {
    "unknown format": (desc("planar8", format=4), W, H, b"format"),
    "negative format": (desc("planar8", format=-1), W, H, b"format"),
    "unknown matrix": (desc("rgb", matrix=2), W, H, b"matrix"),
    "negative matrix": (desc("f32", matrix=-1), W, H, b"matrix"),
    "full_range 2": (desc("rgba", full_range=2), W, H, b"full_range"),
    "full_range -1": (desc("f16", full_range=-1), W, H, b"full_range"),
    "reserved": (desc("bgr", reserved=1), W, H, b"reserved"),
    "pixel_bytes 2": (desc("rgb", pixel_bytes=2), W, H, b"pixel_bytes"),
    "pixel_bytes 5": (desc("rgba", pixel_bytes=5), W, H, b"pixel_bytes"),
    "pixel_bytes 0 packed": (desc("rgba", pixel_bytes=0), W, H, b"pixel_bytes"),
    "pixel_bytes with a planar format": (desc("planar8", pixel_bytes=3), W, H, b"pixel_bytes"),
    "offset repeated (G = R)": (desc("rgb", offset1=0), W, H, b"offset[1]"),
    "offset repeated (B = G)": (desc("rgba", offset2=1), W, H, b"offset[2]"),
    "offset repeated (B = R)": (desc("rgba", offset2=0), W, H, b"offset[2]"),
    "offset 3 of 3 bytes": (desc("rgb", offset2=3), W, H, b"offset[2]"),
    "offset 4 of 4 bytes": (desc("rgba", offset0=4), W, H, b"offset[0]"),
    "negative offset": (desc("bgra", offset1=-1), W, H, b"offset[1]"),
    "offset with a planar format": (desc("f32", offset2=1), W, H, b"offset[2]"),
    "no packed plane": (desc("rgb", plane0=None), W, H, b"plane[0]"),
    "no G plane": (desc("planar8", plane1=None), W, H, b"plane[1]"),
    "no B plane": (desc("f16", plane2=None), W, H, b"plane[2]"),
    "second plane with PACKED8": (desc("rgba", plane1=SOME), W, H, b"plane[1]"),
    "third plane with PACKED8": (desc("bgr", plane2=SOME), W, H, b"plane[2]"),
    "packed pitch below a row (3 bytes)": (desc("rgb", pitch0=3 * W - 1), W, H, b"pitch[0]"),
    "packed pitch below a row (4 bytes)": (desc("rgba", pitch0=4 * W - 1), W, H, b"pitch[0]"),
    "planar pitch below a row": (desc("planar8", pitch1=W - 1), W, H, b"pitch[1]"),
    "binary16 pitch below a row": (desc("f16", pitch2=2 * W - 2), W, H, b"pitch[2]"),
    "binary32 pitch below a row": (desc("f32", pitch0=4 * W - 4), W, H, b"pitch[0]"),
    "negative pitch": (desc("planar8", pitch2=-W), W, H, b"pitch[2]"),
    "negative packed pitch": (desc("rgba", pitch0=-4 * W), W, H, b"pitch[0]"),
    "binary16 pitch not element-aligned": (desc("f16", pitch1=2 * W + 1), W, H, b"pitch[1]"),
    "binary32 pitch not element-aligned": (desc("f32", pitch2=4 * W + 2), W, H, b"pitch[2]"),
    "binary16 plane not element-aligned": (desc("f16", plane0=SOME + 1), W, H, b"plane[0]"),
    "binary32 plane not element-aligned": (desc("f32", plane1=SOME + 2), W, H, b"plane[1]"),
    "odd width": (desc("planar8", 7), W + 1, H, b"width"),
    "odd height": (desc("rgb"), W, H - 1, b"height"),
    "zero width": (desc("rgba"), 0, H, b"width"),
    "negative height": (desc("f32"), W, -2, b"height"),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_descriptors_that_are_refused(lib, why):
    pic, w, h, field = REFUSED[why]
    assert lib.hmr_gpu_rgb_picture_check(C.byref(desc("planar8")), W, H) == 0      # (so that the error text below is this refusal's)
    assert lib.hmr_gpu_rgb_picture_check(C.byref(pic), w, h) == ERR_ARG
    text = lib.hmr_gpu_last_error()
    assert text and field in text, text
    out = np.zeros(8, np.uint8)
    assert lib.hmr_gpu_rgb_convert_host(C.byref(pic), w, h, out.ctypes.data, out.ctypes.data, out.ctypes.data) == ERR_ARG      # (refused before a pointer is followed)


def test_null_is_refused(lib):
    assert lib.hmr_gpu_rgb_picture_check(None, W, H) == ERR_ARG
    assert lib.hmr_gpu_last_error()
    out = np.zeros(4, np.uint8)
    assert lib.hmr_gpu_rgb_convert_host(None, 2, 2, out.ctypes.data, out.ctypes.data, out.ctypes.data) == ERR_ARG
    src = np.zeros(16, np.uint8)
    pic = rc.descriptor(rc.RGB_PACKED8, 3, (0, 1, 2), [src.ctypes.data], [6], "bt601", 0)
    assert lib.hmr_gpu_rgb_convert_host(C.byref(pic), 2, 2, out.ctypes.data, None, out.ctypes.data) == ERR_ARG


def test_the_yuv_descriptor_still_refuses_format_2(lib):
    p = Picture(format=2, reserved=0)
    for c in range(3):
        p.plane[c], p.pitch[c] = SOME + c, W
    assert lib.hmr_gpu_picture_check(C.byref(p), W, H) == ERR_ARG
    assert b"format" in lib.hmr_gpu_last_error()


def test_descriptor_struct_is_the_tests_mirror():
    assert [(n, t) for n, t in PackageRgbPicture._fields_] == [(n, t) for n, t in rc.RgbPicture._fields_]
    assert C.sizeof(PackageRgbPicture) == C.sizeof(rc.RgbPicture) == 80
    assert rc.RgbPicture.plane.offset == 32 and rc.RgbPicture.pitch.offset == 56


# ---- the host conversion against the restatement ----
def convert(lib, form, chans, matrix, full, rng, padded):
    """hmr_gpu_rgb_convert_host on the picture laid out in host memory: (y, u, v) as arrays"""
    h, w = chans[0].shape
    fmt, pb, offs, planes = rc.lay_out(form, chans, rng, padded)
    before = [buf.copy() for buf, _, _ in planes]
    pic = rc.descriptor(fmt, pb, offs, [buf.ctypes.data + base for buf, base, _ in planes], [pitch for _, _, pitch in planes], matrix, full)
    guard = 64
    out = [np.full(n + 2 * guard, 0xA5, np.uint8) for n in (w * h, w * h // 4, w * h // 4)]
    assert lib.hmr_gpu_rgb_convert_host(C.byref(pic), w, h, *[o.ctypes.data + guard for o in out]) == 0, lib.hmr_gpu_last_error()
    for o in out:
        assert (o[:guard] == 0xA5).all() and (o[-guard:] == 0xA5).all()
    for (buf, _, _), b in zip(planes, before):
        assert np.array_equal(buf, b)
    return out[0][guard:-guard].reshape(h, w), out[1][guard:-guard].reshape(h // 2, w // 2), out[2][guard:-guard].reshape(h // 2, w // 2)


def same(lib, form, chans, matrix, full, rng, padded=True):
    got = convert(lib, form, chans, matrix, full, rng, padded)
    want = rc.restate(*rc.eight_bit(form, chans), matrix, full)
    for name, g, x in zip("YUV", got, want):
        assert np.array_equal(g, x), (form, matrix, full, name, np.argwhere(g != x)[:4].tolist())


def of_form(form, rng, r, g, b):
    return rc.as_floats(form, rng, r, g, b) if form in rc.FLOAT_TYPES else [r, g, b]


@pytest.mark.parametrize("matrix,full", rc.MATRIX_RANGES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_noise_in_every_form(lib, size, matrix, full):
    w, h = size
    rng = np.random.default_rng(w * 7 + h + full)
    for k, form in enumerate(sorted(rc.FORMS)):
        same(lib, form, of_form(form, rng, *rc.noise(rng, w, h)), matrix, full, rng, padded=bool((k + full) & 1) or w < 8)


@pytest.mark.parametrize("matrix,full", rc.MATRIX_RANGES)
def test_corners_ramp_and_checkerboard(lib, matrix, full):
    rng = np.random.default_rng(5)
    w, h = 32, 8
    pictures = [[np.full((h, w), 255 * bit, np.uint8) for bit in ((k >> 2) & 1, (k >> 1) & 1, k & 1)] for k in range(8)]      # the eight corners, flat
    ramp = np.tile(np.arange(256, dtype=np.uint8), (4, 1))
    pictures.append([ramp, ramp, ramp])
    yy, xx = np.mgrid[0:16, 0:48]
    for colour in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (17, 200, 90)):      # a checkerboard of a colour and its complement, per pixel and per 2 x 2 block
        for cell in (1, 2):
            on = ((yy // cell + xx // cell) & 1).astype(bool)
            pictures.append([np.where(on, c, 255 - c).astype(np.uint8) for c in colour])
    for r, g, b in pictures:
        for form in sorted(rc.FORMS):
            same(lib, form, of_form(form, rng, r, g, b), matrix, full, rng)
    # grey: U = V = 128 at every level, luma monotone
    y, u, v = convert(lib, "planar8", [ramp, ramp, ramp], matrix, full, rng, False)
    assert (u == 128).all() and (v == 128).all()
    assert (np.diff(y[0].astype(int)) >= 0).all() and y[0, 0] == (0 if full else 16) and y[0, 255] == (255 if full else 235)


@pytest.mark.parametrize("form", ["f16", "f32"])
def test_floats_nobody_ordered(lib, form):
    rng = np.random.default_rng(11)
    t = rc.FLOAT_TYPES[form]
    # the restatement's own quantiser on the values whose result is known without arithmetic
    known = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 0.0, 1.0, 7.0, 0.5], t)
    assert rc.quantize(known).tolist() == [0, 255, 0, 0, 0, 0, 255, 255, 128]      # (127.5 rounds half to even)
    assert rc.quantize(np.array([1, 1023], np.uint16).view(np.float16)).tolist() == [0, 0]
    for (w, h), (matrix, full) in zip([(200, 136), (64, 48), (416, 240), (16, 2)], rc.MATRIX_RANGES):
        same(lib, form, rc.special_floats(t, rng, w, h), matrix, full, rng)


# ---- the restated arithmetic against the real-valued formulas ----
@pytest.mark.parametrize("matrix,full", rc.MATRIX_RANGES)
def test_within_0_51_of_the_real_valued_formula(matrix, full):
    """half an LSB of rounding plus at most 3 x 1020 x 0.5 / 2^18 of coefficient error (include/homer_gpu.h section 12f): 0.51 - held on every level of every channel
    pair, on random pictures (random 2 x 2 sums), on flat corner pictures and on blocks of mixed corners (the extreme sums)"""
    rng = np.random.default_rng(3)
    lv = np.arange(256)
    pictures = [rc.noise(rng, 512, 512) for _ in range(4)]
    a, b = np.meshgrid(lv, lv)
    for fixed in (0, 77, 255):
        pictures += [[a, b, np.full_like(a, fixed)], [a, np.full_like(a, fixed), b], [np.full_like(a, fixed), a, b]]
    pictures += [[np.full((2, 2), 255 * bit) for bit in ((k >> 2) & 1, (k >> 1) & 1, k & 1)] for k in range(8)]
    pictures.append([rng.integers(0, 2, (256, 256)) * 255 for _ in range(3)])
    worst = 0.0
    for r, g, b in pictures:
        got = rc.restate(r, g, b, matrix, full)
        want = rc.real_valued(r, g, b, matrix, full)
        for name, x, y in zip("YUV", got, want):
            err = np.abs(x.astype(np.float64) - np.clip(y, 0.0, 255.0)).max()
            worst = max(worst, err)
            assert err <= 0.51, (matrix, full, name, err)
        if not full:
            assert got[0].min() >= 16 and got[0].max() <= 235 and min(got[1].min(), got[2].min()) >= 16 and max(got[1].max(), got[2].max()) <= 240
    print(f"{matrix} full_range={full}: largest distance to the real-valued formula {worst:.4f}")
    grey = np.tile(lv, (2, 1))
    y, u, v = rc.restate(grey, grey, grey, matrix, full)
    assert (u == 128).all() and (v == 128).all() and (np.diff(y[0].astype(int)) >= 0).all()


def test_rows_of_the_table_sum_as_the_header_says():
    for (matrix, full), (ky, ku, kv, yoff) in rc.TABLE.items():
        assert sum(ky) == (65536 if full else round(65536 * 219 / 255)) and sum(ku) == 0 and sum(kv) == 0 and yoff == (0 if full else 16)


# ---- the package ----
def test_package_import_needs_neither_torch_nor_a_gpu():
    code = ("import homerhevc_amd, homerhevc_amd.encoder as m; assert 'torch' not in sys.modules, 'torch imported'; assert homerhevc_amd.RGBFrame is m.RGBFrame; "
            "f = m.RGBFrame(None, order='bgra', matrix='bt601', full_range=True); assert (f.order, f.matrix, f.full_range) == ('bgra', 'bt601', True); "
            "assert m.rgb_picture_of and m.Encoder.source and m.BatchEncoder.source; assert 'torch' not in sys.modules, 'torch imported'")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {libs.ROOT!r}); " + code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from homerhevc_amd.encoder import RGBFrame
    with pytest.raises(ValueError):
        RGBFrame(None, matrix="bt2020")
    with pytest.raises(ValueError):
        RGBFrame(None, order="grb")


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_rgb_picture_check", "hmr_gpu_rgb_convert_host", "hmr_gpu_enc_load_source_rgb_device", "hmr_gpu_enc_load_sources_rgb_device",
                 "hmr_gpu_enc_export_source_device", "hmr_gpu_enc_export_sources_device"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert "12f." in text
    for (matrix, full), (ky, ku, kv, yoff) in rc.TABLE.items():      # the table a caller reproduces the samples from
        for row in (ky, ku, kv):
            assert ", ".join(str(k) for k in row) in text, (matrix, full, row)


# ---- the kernel as compiled ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_rgb_ingest_kernel_as_compiled():
    """k_ingest_rgb for gfx950: no private memory, no spills, global_ (not flat_) accesses, 16-byte loads and stores"""
    remarks, asm = libs.picture_io_as_compiled()
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        seen[blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]): (\d+)", blk)}
    names = [n for n in seen if "k_ingest_rgb" in n]
    assert len(names) == 1, sorted(seen)
    f = seen[names[0]]
    print(f)
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
    assert f["VGPRs"] <= 128 and f["Occupancy [waves/SIMD]"] >= 4, f      # (DESIGN.md records 127 and 4)
    body = asm[asm.index(names[0] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    code = [l.split(";")[0] for l in body.splitlines()]
    assert not [l for l in code if "flat_" in l or "scratch_" in l]
    assert sum("global_load_dwordx4" in l for l in code) >= 3 + 4 + 3 + 6 + 6 and sum("global_store_dwordx4" in l for l in code) >= 6
