"""SSIM of reconstructed pictures (include/homer_gpu.h section 12h), the parts that need no GPU: hmr_gpu_ssim_host - the host twin of the device kernel, the same
csrc/ssim_window.h - against the Python-integer oracle of tests/ssim_cases.py on hostile content, hmr_gpu_ssim against exact fractions, the fixture minted from the
compiled reference (tests/golden/ssim.json, made by tests/golden/make_ssim_golden.py) against the checker build's reconstruction, what the Python module offers without
torch, and the header's declarations."""
import ctypes as C
import json
import os
import re
from fractions import Fraction

import pytest

import encoder_cases as ec
import libs
import picture_gpu
import ssim_cases as sc
from homerhevc_amd.encoder import Picture
from test_egress_cpu import QUALITY_CASES
from test_ingest_cpu import in_a_fresh_process
from test_stream_cpu import GOLD, cpu, encode  # noqa: F401  (cpu: the fixture that builds and loads the checker build)

SSIM = json.load(open(os.path.join(ec.GOLDEN, "ssim.json")))
ERR_ARG = -3
HIPCC = "/opt/rocm/bin/hipcc"
# 16 x 16: one chroma window a plane; 24 x 16 and 72 x 16: chroma planes of 3 and 9 block columns (odd: the last 8 samples of a row are a block and a half);
# 200 x 136: 25 x 17 chroma blocks, more than one row of windows
SIZES = [(16, 16), (24, 16), (72, 16), (200, 136)]


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    return picture_gpu.load()


@pytest.fixture(scope="module")
def pairs():
    """per size: {name: (a, b, the oracle's sums)} - computed once"""
    return {(w, h): {name: (a, b, sc.picture_sums(a, b, w, h)) for name, (a, b) in sc.content_pairs(w, h).items()} for w, h in SIZES}


def native_ssim(lib, sums, w, h):
    out = (C.c_double * 3)()
    assert lib.hmr_gpu_ssim((C.c_int64 * 3)(*sums), w, h, out) == 0, lib.hmr_gpu_last_error()
    return list(out)


@pytest.mark.parametrize("layouts", [("tight_i420", "tight_i420"), ("offset_i420", "nv12"), ("nv12", "offset_i420")])
@pytest.mark.parametrize("size", SIZES)
def test_host_sums_are_the_oracles(lib, pairs, size, layouts):
    w, h = size
    for name, (a, b, want) in pairs[size].items():
        assert sc.host_sums(lib, a, b, w, h, *layouts) == want, (name, size, layouts)


@pytest.mark.parametrize("size", SIZES)
def test_identical_pictures_give_one_and_inverted_noise_is_negative(lib, pairs, size):
    w, h = size
    a, b, want = pairs[size]["identical"]
    assert want == sc.host_sums(lib, a, b, w, h) == [sc.ONE * n for n in sc.picture_windows(w, h)]
    assert native_ssim(lib, want, w, h) == [1.0, 1.0, 1.0]
    a, b, want = pairs[size]["noise_inverse"]
    got = sc.host_sums(lib, a, b, w, h)
    assert got == want and all(s < 0 for s in got), got
    if size == (200, 136):
        assert all(v < -0.9 for v in native_ssim(lib, got, w, h))
    # every window of all-0 against all-255 has the same value, far from both ends
    a, b, want = pairs[size]["zero_255"]
    assert 0 < want[0] < sc.ONE * sc.windows(w, h) // 100


def test_mean_ssim_is_the_correctly_rounded_quotient(lib, pairs):
    cases = [(list(want), w, h) for (w, h), by_name in pairs.items() for _, _, want in by_name.values()]
    w, h = 3840, 2160
    identical_2160p = [sc.ONE * n for n in sc.picture_windows(w, h)]
    assert identical_2160p[0] == sc.ONE * 959 * 539 > 5e14
    cases += [(identical_2160p, w, h), ([s - 1 for s in identical_2160p], w, h), ([-s for s in identical_2160p], w, h), ([1, -1, 0], w, h), ([-12345678901, 3, 7], 416, 240)]
    for sums, w, h in cases:
        want = [float(Fraction(s, sc.ONE * n)) for s, n in zip(sums, sc.picture_windows(w, h))]
        assert native_ssim(lib, sums, w, h) == want, (sums, w, h)


def test_the_fixture_holds_every_case_and_the_reference_reconstruction():
    assert sorted(SSIM) == sorted(QUALITY_CASES)
    for case, s in SSIM.items():
        g = GOLD[case]
        assert (s["width"], s["height"], s["frames"]) == (g["width"], g["height"], g["frames"]), case
        assert s["recon_md5"] == g["recon_md5"] and s["windows"] == sc.picture_windows(s["width"], s["height"]), case
        assert len(s["ssim"]) == s["frames"], case
        for sums in s["ssim"]:
            assert all(-sc.ONE * n <= v <= sc.ONE * n for v, n in zip(sums, s["windows"])), case
    assert SSIM["3840x2160_cfg2_wpp32"]["ssim"][0][0] > 1 << 32


@pytest.mark.parametrize("case", ["200x136", "416x240_flat_qp4", "328x264_wpp3"])
def test_host_sums_reproduce_the_fixture(lib, cpu, case):
    """the reconstruction the minting saw is not kept; the checker build (the device path's CPU twin) reproduces it - its md5 is the fixture's - and hmr_gpu_ssim_host
    between the clip's first frame and that reconstruction gives the fixture's sums"""
    s, g = SSIM[case], GOLD[case]
    w, h = s["width"], s["height"]
    raw = []
    _, recon, _ = encode(cpu, case, raw_recon=raw)
    assert recon == s["recon_md5"]
    keys = g["keys"]
    clip = ec.clip_frames(w, h, g["frames"], keys.get("cut_at"), keys.get("clip_seed", 1234), keys.get("content", "default"))
    assert sc.host_sums(lib, b"".join(clip[0]), raw[0], w, h, "offset_i420", "nv12") == s["ssim"][0]


def test_argument_errors(lib):
    w, h = 24, 16
    a = sc.HostPicture(bytes(w * h * 3 // 2), w, h, "tight_i420")
    b = sc.HostPicture(bytes(w * h * 3 // 2), w, h, "nv12")
    out, dbl, sums = (C.c_int64 * 3)(), (C.c_double * 3)(), (C.c_int64 * 3)(1, 2, 3)

    def changed(pic, **kw):
        p = Picture(format=pic.format, reserved=pic.reserved)
        for c in range(3):
            p.plane[c], p.pitch[c] = pic.plane[c], pic.pitch[c]
        for k, v in kw.items():
            if k in ("format", "reserved"):
                setattr(p, k, v)
            else:
                getattr(p, k[:-1])[int(k[-1])] = v
        return p

    pa, pb = C.byref(a.pic), C.byref(b.pic)
    host = {
        "NULL a": (None, pb, w, h, out), "NULL b": (pa, None, w, h, out), "NULL sums": (pa, pb, w, h, None),
        "unknown format": (C.byref(changed(a.pic, format=5)), pb, w, h, out), "reserved": (pa, C.byref(changed(b.pic, reserved=1)), w, h, out),
        "a missing plane": (C.byref(changed(a.pic, plane2=None)), pb, w, h, out), "a pitch below a row": (pa, C.byref(changed(b.pic, pitch1=w - 1)), w, h, out),
        "a third plane with NV12": (pa, C.byref(changed(b.pic, plane2=a.pic.plane[2])), w, h, out),
        "width not a multiple of 8": (pa, pb, 20, h, out), "height not a multiple of 8": (pa, pb, w, 12, out), "odd width": (pa, pb, 23, h, out),
        "width 8": (pa, pb, 8, h, out), "height 8": (pa, pb, w, 8, out), "width 0": (pa, pb, 0, h, out), "negative height": (pa, pb, w, -16, out),
    }
    for why, args in host.items():
        assert lib.hmr_gpu_ssim_host(pa, pb, w, h, out) == 0
        assert lib.hmr_gpu_ssim_host(*args) == ERR_ARG and lib.hmr_gpu_last_error(), why
    one = sc.ONE * sc.windows(416, 240)
    mean = {
        "NULL sums": (None, 416, 240, dbl), "NULL results": (sums, 416, 240, None), "width not a multiple of 8": (sums, 420, 240, dbl),
        "height not a multiple of 8": (sums, 416, 236, dbl), "width 8": (sums, 8, 240, dbl), "height 8": (sums, 416, 8, dbl), "width 0": (sums, 0, 240, dbl),
        "negative height": (sums, 416, -240, dbl), "a sum above 2^30 windows": ((C.c_int64 * 3)(one + 1, 0, 0), 416, 240, dbl),
        "a sum below -2^30 windows": ((C.c_int64 * 3)(0, 0, -(1 << 63)), 416, 240, dbl),
    }
    for why, args in mean.items():
        assert lib.hmr_gpu_ssim(sums, 416, 240, dbl) == 0
        assert lib.hmr_gpu_ssim(*args) == ERR_ARG and lib.hmr_gpu_last_error(), why
    assert native_ssim(lib, [one, -sc.ONE * sc.windows(208, 120), 0], 416, 240) == [1.0, -1.0, 0.0]      # (the ends themselves are legal)


def test_python_ssim_needs_neither_torch_nor_a_gpu():
    s = SSIM["416x240"]
    code = (f"from homerhevc_amd.encoder import ssim; import homerhevc_amd; v = ssim({s['ssim'][0]!r}, 416, 240); assert 'torch' not in sys.modules, 'torch imported'; "
            "assert homerhevc_amd.ssim is ssim; print(repr(list(v)))")
    r = in_a_fresh_process(code)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == [float(Fraction(v, sc.ONE * n)) for v, n in zip(s["ssim"][0], s["windows"])]
    r = in_a_fresh_process("from homerhevc_amd.encoder import ssim\nfor bad in ([1, 2, 3], 412, 240), ([-(1 << 63)] * 3, 416, 240), ([1, 2], 416, 240):\n"
                           "    try:\n        ssim(*bad)\n    except ValueError as e:\n        print('refused', e)")
    assert r.returncode == 0 and r.stdout.count("refused") == 3, (r.stdout, r.stderr)


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_enc_ssim_device", "hmr_gpu_enc_ssim_one_device", "hmr_gpu_ssim", "hmr_gpu_ssim_host"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert "12h." in text


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_ssim_kernel_as_compiled():
    """k_ssim for gfx950: no private memory, no spills, eight waves per SIMD, a few KB of LDS, global_ (not flat_) 16-byte loads, the products by v_dot2, and no store to
    memory but ONE 64-bit atomic add"""
    remarks, asm = libs.picture_io_as_compiled()
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        seen[blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", blk)}
    names = [n for n in seen if "k_ssim" in n]
    assert len(names) == 1, sorted(seen)
    f = seen[names[0]]
    print(f)
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["Occupancy [waves/SIMD]"] == 8, f
    assert 0 < f["LDS Size [bytes/block]"] <= 4096, f
    body = asm[asm.index(names[0] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    code = [l.split(";")[0].split() for l in body.splitlines()]
    ops = [l[0] for l in code if l]
    assert not [o for o in ops if o.startswith(("flat_", "scratch_", "global_store", "buffer_store"))]
    assert ops.count("global_load_dwordx4") == 8 and sum(o.startswith("v_dot2") for o in ops) == 80
    assert [o for o in ops if o.startswith("global_atomic")] == ["global_atomic_add_x2"]
