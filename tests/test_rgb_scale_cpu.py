"""The downscaling RGB ingest (include/homer_gpu.h section 12j), the parts that need no GPU: hmr_gpu_scale_rgb_host - the arithmetic k_rgb_ladder compiles (csrc/rgb_yuv.h,
csrc/scale_area.h) - against the composition of the numpy restatements of sections 12f and 12g (tests/rgb_scale_cases.py) byte for byte and against the two older host
functions applied one after the other, the bound of 1.01 to the real-valued area average of the real-valued BT formula, what is refused, the struct's layout, what the
package imports, and what the cross-compile makes of k_rgb_ladder."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libs
import rgb_cases as rc
import rgb_scale_cases as rs
import scale_cases as sc
from homerhevc_amd.encoder import ScaledRgbPicture as PackageScaledRgbPicture
from test_rgb_ingest_cpu import REFUSED as RGB_REFUSED
from test_scale_cpu import REFUSED as SCALE_REFUSED

ERR_ARG = -3
HIPCC = "/opt/rocm/bin/hipcc"
LDS_OF_A_CU = 160 * 1024
SOME = 0x1000          # any non-NULL value: the checks never follow a pointer


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    lib = C.CDLL(libs.GPU_SO)
    lib.hmr_gpu_scale_rgb_host.argtypes = [C.POINTER(rs.ScaledRgbPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_rgb_convert_host.argtypes = [C.POINTER(rc.RgbPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_scale_host.argtypes = [C.POINTER(sc.ScaledPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


# ---- the host twin against the comparator ----
def planes_of(flat, w, h):
    return flat[0].reshape(h, w), flat[1].reshape(h // 2, w // 2), flat[2].reshape(h // 2, w // 2)


def scale_rgb_host(lib, form, chans, matrix, full, dst, rng, padded):
    """hmr_gpu_scale_rgb_host on the picture laid out in host memory, and hmr_gpu_scale_host applied to hmr_gpu_rgb_convert_host's planes: two (y, u, v) triples; the
    source buffers and the bytes around the outputs stay what they were"""
    h, w = chans[0].shape
    wd, hd = dst
    fmt, pb, offs, planes = rc.lay_out(form, chans, rng, padded)
    before = [buf.copy() for buf, _, _ in planes]
    addresses, pitches = [buf.ctypes.data + base for buf, base, _ in planes], [pitch for _, _, pitch in planes]
    pic = rs.descriptor(fmt, pb, offs, addresses, pitches, matrix, full, w, h)
    guard = 64
    out = [np.full(n + 2 * guard, 0xA5, np.uint8) for n in (wd * hd, wd * hd // 4, wd * hd // 4)]
    assert lib.hmr_gpu_scale_rgb_host(C.byref(pic), wd, hd, *[o.ctypes.data + guard for o in out]) == 0, lib.hmr_gpu_last_error()
    for o in out:
        assert (o[:guard] == 0xA5).all() and (o[-guard:] == 0xA5).all()
    for (buf, _, _), b in zip(planes, before):
        assert np.array_equal(buf, b)
    # the two older host functions, one after the other: the full-size picture in between exists here
    mid = [np.zeros(n, np.uint8) for n in (w * h, w * h // 4, w * h // 4)]
    assert lib.hmr_gpu_rgb_convert_host(C.byref(pic.pic), w, h, *[m.ctypes.data for m in mid]) == 0, lib.hmr_gpu_last_error()
    yuv = sc.descriptor(sc.PIC_I420, [m.ctypes.data for m in mid], [w, w // 2, w // 2], w, h)
    two = [np.zeros(n, np.uint8) for n in (wd * hd, wd * hd // 4, wd * hd // 4)]
    assert lib.hmr_gpu_scale_host(C.byref(yuv), wd, hd, *[t.ctypes.data for t in two]) == 0, lib.hmr_gpu_last_error()
    return planes_of([o[guard:-guard] for o in out], wd, hd), planes_of(two, wd, hd)


def check(lib, form, chans, dst, rng, rows=rc.MATRIX_RANGES, layouts=(True, False)):
    for matrix, full in rows:
        want = rs.comparator(form, chans, matrix, full, *dst)
        for padded in layouts:
            got, composed = scale_rgb_host(lib, form, chans, matrix, full, dst, rng, padded)
            for name, g, c, x in zip("YUV", got, composed, want):
                assert np.array_equal(g, x), (form, matrix, full, padded, name, np.argwhere(g != x)[:4].tolist())
                assert np.array_equal(c, x), (form, matrix, full, padded, name, "the two host functions one after the other")


@pytest.mark.parametrize("form", rs.FORMS)
@pytest.mark.parametrize("pair", rs.HOST_PAIRS, ids=sc.pair_id)
def test_host_twin_equals_the_comparator(lib, pair, form):
    """every size pair x every form x all four matrix / range rows x the padded and the tight layout"""
    (ws, hs), dst = pair
    rng = np.random.default_rng(ws * 3 + hs + len(form))
    check(lib, form, rs.chans_of(form, rng, *rc.noise(rng, ws, hs)), dst, rng)


@pytest.mark.parametrize("form", ["f16", "f32"])
def test_floats_nobody_ordered(lib, form):
    rng = np.random.default_rng(11)
    for ((ws, hs), dst), row in zip([((400, 272), (200, 136)), ((330, 266), (328, 264)), ((32, 16), (2, 2)), ((300, 204), (200, 136))], rc.MATRIX_RANGES):
        check(lib, form, rc.special_floats(rc.FLOAT_TYPES[form], rng, ws, hs), dst, rng, rows=[row], layouts=(True,))


# ---- the bound the header states ----
@pytest.mark.parametrize("pair", [p for p in rs.HOST_PAIRS if p[0] != (1800, 1224)], ids=sc.pair_id)
def test_within_1_01_of_the_real_valued_average_of_the_real_valued_formula(pair):
    """0.51 from section 12f for every converted sample, which an average cannot enlarge, plus 0.5 from section 12g's single rounding"""
    (ws, hs), (wd, hd) = pair
    rng = np.random.default_rng(ws + hd)
    worst = 0.0
    for kind in ("noise", "blocks", "extremes"):
        r, g, b = rs.content(kind, rng, ws, hs)
        for matrix, full in rc.MATRIX_RANGES:
            got = rs.comparator("planar8", [r, g, b], matrix, full, wd, hd)
            want = rs.real_valued(r, g, b, matrix, full, wd, hd)
            for name, x, y in zip("YUV", got, want):
                err = np.abs(x.astype(np.float64) - y).max()
                worst = max(worst, err)
                assert err <= 1.01, (pair, kind, matrix, full, name, err)
    print(f"{sc.pair_id(pair)}: largest distance to the real-valued average of the real-valued formula {worst:.5f}")


# ---- refusals ----
def good(w=400, h=272):
    return rs.descriptor(rc.RGB_PLANAR8, 0, (0, 0, 0), [SOME, SOME + 64, SOME + 128], [w, w, w], "bt709", 0, w, h)


def refused(lib, pic, dst, field):
    out = np.zeros(16, np.uint8)
    o = out.ctypes.data
    assert lib.hmr_gpu_scale_rgb_host(C.byref(good()), 200, 136, o, None, o) == ERR_ARG and b"output" in lib.hmr_gpu_last_error()      # (the text below is this refusal's)
    assert lib.hmr_gpu_scale_rgb_host(C.byref(pic) if pic is not None else None, dst[0], dst[1], o, o, o) == ERR_ARG
    text = lib.hmr_gpu_last_error()
    assert text and field in text, text


def test_null_is_refused(lib):
    refused(lib, None, (200, 136), b"NULL")
    out = np.zeros(16, np.uint8)
    o = out.ctypes.data
    for outs in ((None, o, o), (o, None, o), (o, o, None)):
        assert lib.hmr_gpu_scale_rgb_host(C.byref(good()), 200, 136, *outs) == ERR_ARG and b"output" in lib.hmr_gpu_last_error()


@pytest.mark.parametrize("why", sorted(RGB_REFUSED))
def test_what_the_rgb_descriptor_check_refuses(lib, why):
    """the descriptor is checked against the SOURCE's size; the destination is half of it where that is a size at all"""
    pic, w, h, field = RGB_REFUSED[why]
    refused(lib, rs.ScaledRgbPicture(pic=pic, width=w, height=h), (max(w // 2, 2) & ~1, max(h // 2, 2) & ~1), field)


def test_the_pitch_is_checked_against_the_source_width(lib):
    pic = good()
    pic.pic.pitch[1] = 398      # (enough for the destination's 200)
    refused(lib, pic, (200, 136), b"pitch[1]")


@pytest.mark.parametrize("why", sorted(w for w in SCALE_REFUSED if "ratio" not in w))
def test_what_the_size_check_refuses(lib, why):
    """everything hmr_gpu_scale_check refuses but the ratio bound; a bad SOURCE size is the descriptor check's to name: it comes first"""
    (ws, hs, wd, hd), field = SCALE_REFUSED[why]
    field = {b"src_w": b"width", b"src_h": b"height"}.get(field, field)
    refused(lib, good(ws, hs), (wd, hd), field)


def test_any_ratio_is_taken(lib):
    for why in sorted(w for w in SCALE_REFUSED if "ratio" in w):
        (ws, hs, wd, hd), _ = SCALE_REFUSED[why]
        rng = np.random.default_rng(ws)
        chans = rc.noise(rng, ws, hs)
        got, _ = scale_rgb_host(lib, "planar8", chans, "bt601", 1, (wd, hd), rng, False)
        assert all(np.array_equal(g, x) for g, x in zip(got, rs.comparator("planar8", chans, "bt601", 1, wd, hd))), why


# ---- structure ----
def test_struct_is_the_tests_mirror_and_the_headers_layout():
    flat = lambda st: [(n, t._fields_ if hasattr(t, "_fields_") else t) for n, t in st._fields_]
    assert flat(PackageScaledRgbPicture) == flat(rs.ScaledRgbPicture)
    assert C.sizeof(PackageScaledRgbPicture) == C.sizeof(rs.ScaledRgbPicture) == 88
    assert rs.ScaledRgbPicture.pic.offset == 0 and rs.ScaledRgbPicture.width.offset == 80 and rs.ScaledRgbPicture.height.offset == 84
    assert PackageScaledRgbPicture.pic.offset == 0 and PackageScaledRgbPicture.width.offset == 80 and PackageScaledRgbPicture.height.offset == 84
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    assert re.search(r"typedef struct hmr_gpu_scaled_rgb_picture \{\s*hmr_gpu_rgb_picture pic;[^}]*int32_t width, height;[^}]*\} hmr_gpu_scaled_rgb_picture;", text)


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_enc_load_sources_scaled_rgb_device", "hmr_gpu_enc_load_source_scaled_rgb_device", "hmr_gpu_scale_rgb_host"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    section = text[text.index("12j."):text.index("typedef struct hmr_gpu_scaled_rgb_picture")]
    flat = " ".join(section.replace("*", " ").split())
    assert "12g's area average (source size -> encoder size, every plane on its own, one rounding) of the 8-bit 4:2:0 picture that 12f's conversion makes of the RGB source at the source's size" in flat
    assert "hmr_gpu_scale_host(hmr_gpu_rgb_convert_host(rgb))" in flat and "within 1.01" in flat
    assert "RGB sources: section 12j" in text      # (where section 12g's closing sentence points now)


def test_package_import_needs_neither_torch_nor_a_gpu():
    code = ("import homerhevc_amd, homerhevc_amd.encoder as m; assert 'torch' not in sys.modules, 'torch imported'; assert homerhevc_amd.ScaledRGBFrame is m.ScaledRGBFrame; "
            "assert 'ScaledRGBFrame' in homerhevc_amd.__all__; f = m.ScaledRGBFrame(m.RGBFrame(None, order='bgra'), 3840, 2160); assert (f.width, f.height, f.frame.order) == (3840, 2160, 'bgra'); "
            "assert m.scaled_rgb_picture_of and m.ScaledRgbPicture; assert 'torch' not in sys.modules, 'torch imported'")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {libs.ROOT!r}); " + code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from homerhevc_amd.encoder import RGBFrame, ScaledFrame, ScaledRGBFrame
    for frame in (None, object(), (1, 2, 3), ScaledFrame(None, 1920, 1080), ScaledRGBFrame(RGBFrame(None), 1920, 1080)):
        with pytest.raises(TypeError):
            ScaledRGBFrame(frame, 1920, 1080)
    with pytest.raises(TypeError):
        ScaledFrame(RGBFrame(None), 1920, 1080)


# ---- the kernel as compiled ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_rgb_ladder_kernel_as_compiled():
    """k_rgb_ladder for gfx950: no private memory, no spills, a group segment of at most half a CU's LDS, global_ (not flat_) accesses, 16-byte loads and stores"""
    remarks, asm = libs.picture_io_as_compiled()
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        seen[blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", blk)}
    names = [n for n in seen if "k_rgb_ladder" in n]
    assert len(names) == 1, sorted(seen)
    for other in ("k_downscale", "k_ingest_rgb", "k_egress_rgb", "k_ssim"):      # (the siblings' tests pick their kernels by these substrings)
        assert len([n for n in seen if other in n]) == 1, (other, sorted(seen))
    f = seen[names[0]]
    print(f)
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
    assert 0 < f["LDS Size [bytes/block]"] <= LDS_OF_A_CU // 2, f
    meta = asm[asm.index("amdhsa.kernels"):]
    entries = [e for e in re.split(r"\n  - ", meta) if re.search(r"\.name:\s+" + names[0] + r"\n", e)]      # the kernel's own record of the metadata
    assert len(entries) == 1
    entry = entries[0]
    assert re.search(r"\.private_segment_fixed_size: 0\b", entry) and re.search(r"\.group_segment_fixed_size: " + str(f["LDS Size [bytes/block]"]) + r"\b", entry), entry
    body = asm[asm.index(names[0] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    code = [l.split(";")[0] for l in body.splitlines()]
    assert not [l for l in code if "flat_" in l or "scratch_" in l]
    assert any("global_load_dwordx4" in l for l in code) and any("global_store_dwordx4" in l for l in code)
