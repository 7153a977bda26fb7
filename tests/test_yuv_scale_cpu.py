"""The downscaling deep / 4:2:2 / 4:4:4 ingest (include/homer_gpu.h section 12l), the parts that need no GPU: hmr_gpu_scale_yuv_host - the arithmetic k_yuv_ladder compiles
(csrc/yuv_depth.h, csrc/scale_area.h) - against the composition of the numpy restatements of sections 12k and 12g (tests/yuv_scale_cases.py) byte for byte and against the
two older host functions applied one after the other, the bound of 1.0 to the real-valued area average of the min(255, x) planes, what is refused, the struct's layout,
what the package imports, and what the cross-compile makes of k_yuv_ladder."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libs
import scale_cases as sc
import yuv_cases as yc
import yuv_scale_cases as ys
from homerhevc_amd.encoder import ScaledYuvPicture as PackageScaledYuvPicture
from test_scale_cpu import REFUSED as SCALE_REFUSED
from test_yuv_ingest_cpu import REFUSED as YUV_REFUSED

ERR_ARG = -3
HIPCC = "/opt/rocm/bin/hipcc"
SOME = 0x1000          # any non-NULL, even value: the checks never follow a pointer
SMALL_PAIRS = [((300, 204), (200, 136)), ((32, 16), (2, 2))]


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    lib = ys.declare(C.CDLL(libs.GPU_SO))
    lib.hmr_gpu_yuv_convert_host.argtypes = [C.POINTER(yc.YuvPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_scale_host.argtypes = [C.POINTER(sc.ScaledPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


# ---- the host twin against the comparator ----
def planes_of(flat, w, h):
    return flat[0].reshape(h, w), flat[1].reshape(h // 2, w // 2), flat[2].reshape(h // 2, w // 2)


def scale_yuv_host(lib, form, planes3, dst, rng, padded):
    """hmr_gpu_scale_yuv_host on the picture laid out in host memory, and hmr_gpu_scale_host applied to hmr_gpu_yuv_convert_host's planes: two (y, u, v) triples; the
    source buffers and the bytes around the outputs stay what they were"""
    h, w = planes3[0].shape
    wd, hd = dst
    planes = yc.lay_out(form, *planes3, rng, padded)
    before = [buf.copy() for buf, _, _ in planes]
    pic = ys.descriptor(form, [buf.ctypes.data + base for buf, base, _ in planes], [pitch for _, _, pitch in planes], w, h)
    guard = 64
    out = [np.full(n + 2 * guard, 0xA5, np.uint8) for n in (wd * hd, wd * hd // 4, wd * hd // 4)]
    assert lib.hmr_gpu_scale_yuv_host(C.byref(pic), wd, hd, *[o.ctypes.data + guard for o in out]) == 0, lib.hmr_gpu_last_error()
    for o in out:
        assert (o[:guard] == 0xA5).all() and (o[-guard:] == 0xA5).all()
    for (buf, _, _), b in zip(planes, before):
        assert np.array_equal(buf, b)
    # the two older host functions, one after the other: the full-size picture in between exists here
    mid = [np.zeros(n, np.uint8) for n in (w * h, w * h // 4, w * h // 4)]
    assert lib.hmr_gpu_yuv_convert_host(C.byref(pic.pic), w, h, *[m.ctypes.data for m in mid]) == 0, lib.hmr_gpu_last_error()
    yuv = sc.descriptor(sc.PIC_I420, [m.ctypes.data for m in mid], [w, w // 2, w // 2], w, h)
    two = [np.zeros(n, np.uint8) for n in (wd * hd, wd * hd // 4, wd * hd // 4)]
    assert lib.hmr_gpu_scale_host(C.byref(yuv), wd, hd, *[t.ctypes.data for t in two]) == 0, lib.hmr_gpu_last_error()
    return planes_of([o[guard:-guard] for o in out], wd, hd), planes_of(two, wd, hd)


def check(lib, form, planes3, dst, rng, layouts=(True, False)):
    want = ys.comparator(form, *planes3, *dst)
    for padded in layouts:
        got, composed = scale_yuv_host(lib, form, planes3, dst, rng, padded)
        for name, g, c, x in zip("YUV", got, composed, want):
            assert np.array_equal(g, x), (form, padded, name, np.argwhere(g != x)[:4].tolist())
            assert np.array_equal(c, x), (form, padded, name, "the two host functions one after the other")


@pytest.mark.parametrize("pair", SMALL_PAIRS, ids=sc.pair_id)
def test_host_twin_equals_the_comparator_in_every_form(lib, pair):
    """all 50 forms on noise over the container's range (the clamp, the dirty low bits) x the padded and the tight layout"""
    (ws, hs), dst = pair
    for form in yc.NAMES:
        rng = np.random.default_rng(ws * 3 + hs + len(form))
        check(lib, form, yc.noise(form, rng, ws, hs), dst, rng)


@pytest.mark.parametrize("form", ys.CLASSES)
@pytest.mark.parametrize("pair", ys.HOST_PAIRS, ids=sc.pair_id)
def test_host_twin_equals_the_comparator_at_every_pair(lib, pair, form):
    """every host pair x one form per class of the kernel x the padded and the tight layout"""
    (ws, hs), dst = pair
    rng = np.random.default_rng(ws + hs * 5 + len(form))
    check(lib, form, yc.noise(form, rng, ws, hs), dst, rng)


# ---- the bound the header states ----
@pytest.mark.parametrize("pair", [p for p in ys.HOST_PAIRS if p[0] != (1800, 1224)], ids=sc.pair_id)
def test_within_1_of_the_real_valued_average_of_the_clamped_planes(pair):
    """Every 12k sample is within 0.5 of min(255, x), x the real-valued tap average of v / 2^s (rounding: at most 0.5 below 255; the clamp: exactly 255 above it); an
    average with weights that sum to 1 cannot enlarge that; 12g's single rounding adds at most 0.5.  1e-9 is for the float restatement."""
    (ws, hs), (wd, hd) = pair
    rng = np.random.default_rng(ws + hd)
    worst = 0.0
    for kind in ("noise", "blocks", "extremes"):
        for form in ys.CLASSES:
            planes3 = ys.content(kind, form, rng, ws, hs)
            got = ys.comparator(form, *planes3, wd, hd)
            want = ys.real_valued(form, *planes3, wd, hd)
            for name, x, y in zip("YUV", got, want):
                err = np.abs(x.astype(np.float64) - y).max()
                worst = max(worst, err)
                assert err <= 1.0 + 1e-9, (pair, kind, form, name, err)
    print(f"{sc.pair_id(pair)}: largest distance to the real-valued average of the clamped planes {worst:.5f}")


# ---- refusals ----
def good(w=400, h=272):
    return ys.descriptor("planar_420_8", [SOME, SOME + 64, SOME + 128], [w, w // 2, w // 2], w, h)


def refused(lib, pic, dst, field):
    out = np.zeros(16, np.uint8)
    o = out.ctypes.data
    assert lib.hmr_gpu_scale_yuv_host(C.byref(good()), 200, 136, o, None, o) == ERR_ARG and b"output" in lib.hmr_gpu_last_error()      # (the text below is this refusal's)
    assert lib.hmr_gpu_scale_yuv_host(C.byref(pic) if pic is not None else None, dst[0], dst[1], o, o, o) == ERR_ARG
    text = lib.hmr_gpu_last_error()
    assert text and field in text, text


def test_null_is_refused(lib):
    refused(lib, None, (200, 136), b"NULL")
    out = np.zeros(16, np.uint8)
    o = out.ctypes.data
    for outs in ((None, o, o), (o, None, o), (o, o, None)):
        assert lib.hmr_gpu_scale_yuv_host(C.byref(good()), 200, 136, *outs) == ERR_ARG and b"output" in lib.hmr_gpu_last_error()


@pytest.mark.parametrize("why", sorted(YUV_REFUSED))
def test_what_the_yuv_descriptor_check_refuses(lib, why):
    """the descriptor is checked against the SOURCE's size; the destination is half of it where that is a size at all"""
    pic, w, h, field = YUV_REFUSED[why]
    refused(lib, ys.ScaledYuvPicture(pic=pic, width=w, height=h), (max(w // 2, 2) & ~1, max(h // 2, 2) & ~1), field)


def test_the_pitch_is_checked_against_the_source_width(lib):
    pic = good()
    pic.pic.pitch[0] = 398      # (enough for the destination's 200)
    refused(lib, pic, (200, 136), b"pitch[0]")
    pic = ys.descriptor("y210", [SOME], [4 * 400 - 2], 400, 272)      # (enough for a 16-bit packed row of 399 pixels)
    refused(lib, pic, (200, 136), b"pitch[0]")


@pytest.mark.parametrize("why", sorted(w for w in SCALE_REFUSED if "ratio" not in w))
def test_what_the_size_check_refuses(lib, why):
    """everything hmr_gpu_scale_check refuses but the ratio bound; a bad SOURCE size is the descriptor check's to name: it comes first"""
    (ws, hs, wd, hd), field = SCALE_REFUSED[why]
    field = {b"src_w": b"width", b"src_h": b"height"}.get(field, field)
    refused(lib, good(ws, hs), (wd, hd), field)


def test_any_ratio_is_taken(lib):
    for k, why in enumerate(sorted(w for w in SCALE_REFUSED if "ratio" in w)):
        (ws, hs, wd, hd), _ = SCALE_REFUSED[why]
        rng = np.random.default_rng(ws)
        form = ("semi_uv_420_10msb", "planar_444_12", "yuyv_8")[k % 3]
        planes3 = yc.noise(form, rng, ws, hs)
        got, _ = scale_yuv_host(lib, form, planes3, (wd, hd), rng, False)
        assert all(np.array_equal(g, x) for g, x in zip(got, ys.comparator(form, *planes3, wd, hd))), why


# ---- structure ----
def test_struct_is_the_tests_mirror_and_the_headers_layout():
    flat = lambda st: [(n, t._fields_ if hasattr(t, "_fields_") else t) for n, t in st._fields_]
    assert flat(PackageScaledYuvPicture) == flat(ys.ScaledYuvPicture)
    assert C.sizeof(PackageScaledYuvPicture) == C.sizeof(ys.ScaledYuvPicture) == 88
    assert ys.ScaledYuvPicture.pic.offset == 0 and ys.ScaledYuvPicture.width.offset == 80 and ys.ScaledYuvPicture.height.offset == 84
    assert PackageScaledYuvPicture.pic.offset == 0 and PackageScaledYuvPicture.width.offset == 80 and PackageScaledYuvPicture.height.offset == 84
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    assert re.search(r"typedef struct hmr_gpu_scaled_yuv_picture \{\s*hmr_gpu_yuv_picture pic;[^}]*int32_t width, height;[^}]*\} hmr_gpu_scaled_yuv_picture;", text)


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_enc_load_sources_scaled_yuv", "hmr_gpu_enc_load_source_scaled_yuv", "hmr_gpu_scale_yuv_host"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert text.index("12k.") < text.index("12l.") < text.index("typedef struct hmr_gpu_scaled_yuv_picture") < text.index(" 13. Phase planes")
    section = text[text.index("12l."):text.index("typedef struct hmr_gpu_scaled_yuv_picture")]
    flat = " ".join(section.replace("*", " ").split())
    assert "12g's area average (source size -> encoder size, every plane on its own, one rounding) of the 8-bit 4:2:0 picture that 12k's rounding makes of the source at the source's size" in flat
    assert "hmr_gpu_scale_host(hmr_gpu_yuv_convert_host(yuv))" in flat and "within 1.0 of the real-valued area average of the min(255, x) planes" in flat
    assert "their names deliberately do not end in _device" in flat
    assert "12l rounds and scales them in one launch" in text      # (where section 12k's out-of-scope clause points now)


def test_package_import_needs_neither_torch_nor_a_gpu():
    code = ("import homerhevc_amd, homerhevc_amd.encoder as m; assert 'torch' not in sys.modules, 'torch imported'; assert homerhevc_amd.ScaledYUVFrame is m.ScaledYUVFrame; "
            "assert 'ScaledYUVFrame' in homerhevc_amd.__all__; f = m.ScaledYUVFrame(m.YUVFrame((None, None), bits=10, msb_aligned=True), 3840, 2160); "
            "assert (f.width, f.height, f.frame.bits, f.frame.order) == (3840, 2160, 10, 'uv'); assert m.scaled_yuv_picture_of and m.ScaledYuvPicture; assert 'torch' not in sys.modules, 'torch imported'")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {libs.ROOT!r}); " + code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from homerhevc_amd.encoder import RGBFrame, ScaledFrame, ScaledRGBFrame, ScaledYUVFrame, YUVFrame
    yuv = YUVFrame((None, None, None), chroma="422", bits=10)
    for frame in (None, object(), (1, 2, 3), RGBFrame(None), ScaledFrame(None, 1920, 1080), ScaledRGBFrame(RGBFrame(None), 1920, 1080), ScaledYUVFrame(yuv, 1920, 1080)):
        with pytest.raises(TypeError):
            ScaledYUVFrame(frame, 1920, 1080)
    with pytest.raises(TypeError):      # (8-bit 4:2:0 sources stay ScaledFrame's, and it keeps refusing a YUVFrame)
        ScaledFrame(yuv, 1920, 1080)


# ---- the kernel as compiled ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_yuv_ladder_kernel_as_compiled():
    """k_yuv_ladder for gfx950, from ONE device-only compile of picture_io.hip: exactly one kernel of that name and still one per sibling's substring, no private memory, no
    spills of either kind, k_downscale's group segment, global_ (not flat_, not scratch_) accesses, 16-byte loads and stores"""
    remarks, asm = libs.picture_io_as_compiled()
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        seen[blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", blk)}
    names = [n for n in seen if "k_yuv_ladder" in n]
    assert len(names) == 1, sorted(seen)
    for other in ("k_downscale", "k_rgb_ladder", "k_ingest_yuv", "k_ingest_rgb", "k_egress_rgb", "k_ssim"):      # (the siblings' tests pick their kernels by these substrings)
        assert len([n for n in seen if other in n]) == 1, (other, sorted(seen))
    f = seen[names[0]]
    print(f)
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
    downscale = seen[[n for n in seen if "k_downscale" in n][0]]
    assert 0 < f["LDS Size [bytes/block]"] == downscale["LDS Size [bytes/block]"], (f, downscale)
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
