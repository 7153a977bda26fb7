"""The downscaling ingest (include/homer_gpu.h section 12g), the parts that need no GPU: hmr_gpu_scale_host - the arithmetic the kernel compiles (csrc/scale_area.h) -
against the numpy restatement of tests/scale_cases.py byte for byte, the restated arithmetic's properties (2 : 1 block mean, within 0.5 of the real-valued area average,
constants stay constant), what hmr_gpu_scale_check accepts and refuses, the struct's layout, what the package imports, and what the cross-compile makes of k_downscale."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libs
import scale_cases as sc
from homerhevc_amd.encoder import ScaledPicture as PackageScaledPicture

ERR_ARG = -3
HIPCC = "/opt/rocm/bin/hipcc"
LDS_OF_A_CU = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    lib = C.CDLL(libs.GPU_SO)
    lib.hmr_gpu_scale_check.argtypes = [C.c_int] * 4
    lib.hmr_gpu_scale_host.argtypes = [C.POINTER(sc.ScaledPicture), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


# ---- the host twin against the restatement ----
def scale_host(lib, planes, fmt, dst, rng, padded=True):
    """hmr_gpu_scale_host on the picture laid out in host memory: (y, u, v) as arrays; the source buffers and the bytes around the outputs stay what they were"""
    h, w = planes[0].shape
    wd, hd = dst
    parts = sc.lay_out(planes, fmt, rng, padded)
    before = [buf.copy() for buf, _, _ in parts]
    pic = sc.descriptor(fmt, [buf.ctypes.data + off for buf, off, _ in parts], [pitch for _, _, pitch in parts], w, h)
    guard = 64
    out = [np.full(n + 2 * guard, 0xA5, np.uint8) for n in (wd * hd, wd * hd // 4, wd * hd // 4)]
    assert lib.hmr_gpu_scale_host(C.byref(pic), wd, hd, *[o.ctypes.data + guard for o in out]) == 0, lib.hmr_gpu_last_error()
    for o in out:
        assert (o[:guard] == 0xA5).all() and (o[-guard:] == 0xA5).all()
    for (buf, _, _), b in zip(parts, before):
        assert np.array_equal(buf, b)
    return out[0][guard:-guard].reshape(hd, wd), out[1][guard:-guard].reshape(hd // 2, wd // 2), out[2][guard:-guard].reshape(hd // 2, wd // 2)


@pytest.mark.parametrize("kind", sc.CONTENTS)
@pytest.mark.parametrize("pair", sc.PAIRS, ids=sc.pair_id)
def test_host_twin_equals_the_restatement(lib, pair, kind):
    (ws, hs), dst = pair
    rng = np.random.default_rng(ws * 3 + hs + len(kind))
    planes = sc.content(kind, rng, ws, hs)
    want = sc.restate(planes, *dst)
    for fmt in (sc.PIC_I420, sc.PIC_NV12):
        got = scale_host(lib, planes, fmt, dst, rng)
        for name, g, x in zip("YUV", got, want):
            assert np.array_equal(g, x), (pair, kind, fmt, name, np.argwhere(g != x)[:4].tolist())
    got = scale_host(lib, planes, sc.PIC_I420, dst, rng, padded=False)
    assert all(np.array_equal(g, x) for g, x in zip(got, want))


def test_host_twin_refuses_before_it_follows_a_pointer(lib):
    out = np.zeros(16, np.uint8)
    o = out.ctypes.data
    assert lib.hmr_gpu_scale_host(None, 2, 2, o, o, o) == ERR_ARG and lib.hmr_gpu_last_error()
    good = sc.descriptor(sc.PIC_I420, [0x1000, 0x2000, 0x3000], [8, 4, 4], 8, 8)
    assert lib.hmr_gpu_scale_host(C.byref(good), 4, 4, o, None, o) == ERR_ARG and b"output" in lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_scale_host(C.byref(good), 16, 4, o, o, o) == ERR_ARG and b"dst_w" in lib.hmr_gpu_last_error()
    narrow = sc.descriptor(sc.PIC_I420, [0x1000, 0x2000, 0x3000], [6, 4, 4], 8, 8)      # the pitch is checked against the SOURCE's width
    assert lib.hmr_gpu_scale_host(C.byref(narrow), 4, 4, o, o, o) == ERR_ARG and b"pitch[0]" in lib.hmr_gpu_last_error()


# ---- the arithmetic's properties (on the restatement; the host twin equals it above) ----
def test_two_to_one_is_the_block_mean():
    rng = np.random.default_rng(1)
    for w, h in ((400, 272), (36, 20), (4, 4)):
        for kind in sc.CONTENTS:
            for p in sc.content(kind, rng, w, h):
                a = p.astype(np.int64)
                want = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
                assert np.array_equal(sc.restate_plane(p, p.shape[1] // 2, p.shape[0] // 2), want)


def test_equal_sizes_are_the_identity():
    rng = np.random.default_rng(2)
    for p in sc.content("noise", rng, 200, 136):
        assert np.array_equal(sc.restate_plane(p, p.shape[1], p.shape[0]), p)


@pytest.mark.parametrize("pair", sc.PAIRS, ids=sc.pair_id)
def test_within_half_of_the_real_valued_area_average(pair):
    (ws, hs), (wd, hd) = pair
    rng = np.random.default_rng(ws + hd)
    worst = 0.0
    for kind in sc.CONTENTS:
        for p, (dw, dh) in zip(sc.content(kind, rng, ws, hs), ((wd, hd), (wd // 2, hd // 2), (wd // 2, hd // 2))):
            err = np.abs(sc.restate_plane(p, dw, dh).astype(np.float64) - sc.real_valued_plane(p, dw, dh)).max()
            worst = max(worst, err)
            assert err <= 0.5 + 1e-9, (pair, kind, err)
    print(f"{sc.pair_id(pair)}: largest distance to the real-valued area average {worst:.6f}")


@pytest.mark.parametrize("pair", sc.PAIRS, ids=sc.pair_id)
def test_a_constant_picture_stays_constant(pair):
    """every level 0 .. 255: the levels side by side, scaled vertically alone (columns stay levels), and each level as a small flat plane through both axes' weights"""
    (ws, hs), (wd, hd) = pair
    levels = np.tile(np.arange(256, dtype=np.uint8), (hs, 1))
    assert np.array_equal(sc.restate_plane(levels, 256, hd), np.tile(np.arange(256, dtype=np.uint8), (hd, 1)))
    assert np.array_equal(sc.restate_plane(np.tile(np.arange(256, dtype=np.uint8)[:, None], (1, ws)), wd, 256), np.tile(np.arange(256, dtype=np.uint8)[:, None], (1, wd)))
    sx, sy = sc.reduced(ws, wd)[0], sc.reduced(hs, hd)[0]
    den = sx * sy
    lv = np.arange(256)
    assert np.array_equal((lv * den + (den >> 1)) // den, lv)      # (what a flat plane gives: the weights of an output sum to sx sy)
    flat = sc.restate_plane(np.full((hs, ws), 173, np.uint8), wd, hd)
    assert (flat == 173).all()


def test_the_denominators_the_header_names():
    for (src, dst), want in ((((1920, 1080), (1280, 720)), 9), (((1920, 1080), (416, 240)), 540), (((330, 266), (328, 264)), 21945)):
        assert sc.reduced(src[0], dst[0])[0] * sc.reduced(src[1], dst[1])[0] == want
        assert sc.reduced(src[0] // 2, dst[0] // 2) == sc.reduced(src[0], dst[0])      # chroma has luma's ratio


# ---- hmr_gpu_scale_check ----
def test_sizes_that_are_accepted(lib):
    """every pair of the host-twin test but 32 x 16 -> 2 x 2: its width ratio is 16, which the check has to refuse (ratio above 8) - the host twin, whose loop has no
    tile to size, takes it, and so that pair stays in the host-twin test"""
    assert lib.hmr_gpu_scale_check(32, 16, 2, 2) == ERR_ARG and b"src_w" in lib.hmr_gpu_last_error()
    for (ws, hs), (wd, hd) in [p for p in sc.PAIRS if p != ((32, 16), (2, 2))] + [((16, 16), (2, 2)), ((1920, 1080), (1280, 720)), ((1920, 1080), (960, 544)), ((3840, 2160), (1920, 1080)), ((8192, 4320), (8190, 4318)), ((8192, 4320), (1024, 540))]:
        assert lib.hmr_gpu_scale_check(ws, hs, wd, hd) == 0, lib.hmr_gpu_last_error()


def test_every_even_size_up_to_8192_by_4320_fits_32_bits():
    """the largest sx sy for S <= 8192 x 4320 is S itself per axis (gcd 2 at worst gives S / 2): (8192 / 2) x (4320 / 2) x 255 + half < 2^32"""
    den = (8192 // 2) * (4320 // 2)
    assert den * 255 + (den >> 1) < 1 << 32


REFUSED = {
    "odd src_w": ((401, 272, 200, 136), b"src_w"),
    "odd src_h": ((400, 271, 200, 136), b"src_h"),
    "odd dst_w": ((400, 272, 201, 136), b"dst_w"),
    "odd dst_h": ((400, 272, 200, 135), b"dst_h"),
    "zero src_w": ((0, 272, 200, 136), b"src_w"),
    "zero src_h": ((400, 0, 200, 136), b"src_h"),
    "zero dst_w": ((400, 272, 0, 136), b"dst_w"),
    "zero dst_h": ((400, 272, 200, 0), b"dst_h"),
    "negative src_w": ((-400, 272, 200, 136), b"src_w"),
    "negative src_h": ((400, -272, 200, 136), b"src_h"),
    "negative dst_w": ((400, 272, -200, 136), b"dst_w"),
    "negative dst_h": ((400, 272, 200, -136), b"dst_h"),
    "upscale in width": ((200, 272, 202, 136), b"dst_w"),
    "upscale in height": ((400, 136, 200, 138), b"dst_h"),
    "ratio above 8 in width": ((1602, 272, 200, 136), b"src_w"),
    "ratio above 8 in height": ((400, 1090, 200, 136), b"src_h"),
    "ratio 9": ((1800, 1224, 200, 136), b"src_w"),
    "the sum does not fit 32 bits": ((32766, 32766, 32764, 32764), b"32 bits"),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_sizes_that_are_refused(lib, why):
    sizes, field = REFUSED[why]
    assert lib.hmr_gpu_scale_check(400, 272, 200, 136) == 0      # (so that the error text below is this refusal's)
    assert lib.hmr_gpu_scale_check(*sizes) == ERR_ARG
    text = lib.hmr_gpu_last_error()
    assert text and field in text, text


# ---- structure ----
def test_struct_is_the_tests_mirror_and_the_headers_layout():
    flat = lambda st: [(n, t._fields_ if hasattr(t, "_fields_") else t) for n, t in st._fields_]
    assert flat(PackageScaledPicture) == flat(sc.ScaledPicture)
    assert C.sizeof(PackageScaledPicture) == C.sizeof(sc.ScaledPicture) == 64
    assert sc.ScaledPicture.pic.offset == 0 and sc.ScaledPicture.width.offset == 56 and sc.ScaledPicture.height.offset == 60
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    assert re.search(r"typedef struct hmr_gpu_scaled_picture \{\s*hmr_gpu_picture pic;[^}]*int32_t width, height;[^}]*\} hmr_gpu_scaled_picture;", text)


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_scale_check", "hmr_gpu_scale_host", "hmr_gpu_enc_load_source_scaled_device", "hmr_gpu_enc_load_sources_scaled_device"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert "12g." in text and "min((x + 1) s, (i + 1) d) - max(x s, i d)" in text and "(sx sy >> 1)) / (sx sy)" in text


def test_package_import_needs_neither_torch_nor_a_gpu():
    code = ("import homerhevc_amd, homerhevc_amd.encoder as m; assert 'torch' not in sys.modules, 'torch imported'; assert homerhevc_amd.ScaledFrame is m.ScaledFrame; "
            "f = m.ScaledFrame(None, 1920, 1080); assert (f.width, f.height) == (1920, 1080); assert m.scaled_picture_of and m.ScaledPicture; "
            "assert 'torch' not in sys.modules, 'torch imported'")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {libs.ROOT!r}); " + code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    from homerhevc_amd.encoder import RGBFrame, ScaledFrame
    with pytest.raises(TypeError):
        ScaledFrame(RGBFrame(None), 1920, 1080)


# ---- the kernel as compiled ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_downscale_kernel_as_compiled():
    """k_downscale for gfx950: no private memory, no spills, a group segment of at most half a CU's LDS, global_ (not flat_) accesses, 16-byte loads and stores"""
    remarks, asm = libs.picture_io_as_compiled()
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        seen[blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", blk)}
    names = [n for n in seen if "k_downscale" in n]
    assert len(names) == 1, sorted(seen)
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
