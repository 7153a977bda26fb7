"""Reconstructed pictures and PSNR on the GPU (include/homer_gpu.h section 12e), the parts that need no GPU: hmr_gpu_psnr against the values minted from the compiled
reference (tests/golden/quality.json, made by tests/golden/make_quality_golden.py), the fixture's sums against the checker build's reconstruction, what the Python
module offers without torch, and the header's declarations."""
import ctypes as C
import os
import json
import re

import numpy as np
import pytest

import encoder_cases as ec
import libs
from test_ingest_cpu import in_a_fresh_process
from test_stream_cpu import GOLD, cpu, encode  # noqa: F401  (cpu: the fixture that builds and loads the checker build)

QUALITY = json.load(open(os.path.join(ec.GOLDEN, "quality.json")))
QUALITY_CASES = ["200x136", "416x240", "328x264_wpp3", "416x240_wpp_rows", "832x480_wpp_rows", "416x240_scene_cut_wpp_rows", "416x240_cbr400_perf1",
                 "832x480_cbr1500_perf1_wpp_rows", "416x240_eng2", "416x240_eng3_wpp_rows", "416x240_flat", "416x240_flat_qp4", "416x240_extremes_qp4", "416x240_chroma",
                 "384x192_noise_qp0", "1920x1080_cfg2_wpp_rows", "3840x2160_cfg2_wpp32"]
QUALITY_CASES += ["416x240_cbr300_nosao_wpp_rows", "416x240_noise_wpp_rows", "416x240_extremes_wpp_rows"]      # (the rest of the batch tests' sequences)
ERR_ARG = -3
# Derived, not measured: both sides are 10 * log10 of the same double quotient; libm's log10 is good to about an ulp, an ulp at 100 is 1.4e-14, while the smallest plausible
# slip of the formula (256 for 255, the luma sample count for a chroma plane) moves the value by 0.03 dB or more.
PSNR_TOLERANCE = 1e-9


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    lib = C.CDLL(libs.GPU_SO)
    lib.hmr_gpu_psnr.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


def native_psnr(lib, ssd, w, h):
    out = (C.c_double * 3)()
    assert lib.hmr_gpu_psnr((C.c_uint64 * 3)(*ssd), w, h, out) == 0, lib.hmr_gpu_last_error()
    return list(out)


def test_the_fixture_holds_every_case_and_the_reference_reconstruction():
    assert sorted(QUALITY) == sorted(QUALITY_CASES)
    for case, q in QUALITY.items():
        g = GOLD[case]
        assert (q["width"], q["height"], q["frames"]) == (g["width"], g["height"], g["frames"]), case
        assert q["recon_md5"] == g["recon_md5"], case
        assert len(q["ssd"]) == len(q["psnr"]) == q["frames"], case
    # the zero-sum branch is reached by the reference's own data
    assert QUALITY["416x240_flat"]["ssd"][3][2] == 0 and QUALITY["416x240_flat_qp4"]["ssd"][0] == [2, 0, 1] and QUALITY["416x240_flat_qp4"]["ssd"][1] == [39, 16, 0]
    assert QUALITY["416x240"]["ssd"][0] == [4779849, 75564, 96993]


@pytest.mark.parametrize("case", QUALITY_CASES)
def test_psnr_is_the_references(lib, case):
    q = QUALITY[case]
    zero_sums = 0
    for f in range(q["frames"]):
        got = native_psnr(lib, q["ssd"][f], q["width"], q["height"])
        for c in range(3):
            assert abs(got[c] - q["psnr"][f][c]) <= PSNR_TOLERANCE, (case, f, c, got[c], q["psnr"][f][c])
            if q["ssd"][f][c] == 0:
                assert got[c] == 99.99
                zero_sums += 1
    if case == "416x240_flat_qp4":
        assert zero_sums >= 2


def test_psnr_of_a_zero_sum_and_of_a_sum_beyond_32_bits(lib):
    assert native_psnr(lib, [0, 0, 0], 416, 240) == [99.99, 99.99, 99.99]
    # every sample off by 255 at 2160p: 255^2 * samples, far beyond 2^32; the quotient is 1, the PSNR 0
    w, h = 3840, 2160
    sums = [255 * 255 * w * h, 255 * 255 * (w // 2) * (h // 2), 255 * 255 * (w // 2) * (h // 2)]
    assert sums[0] > 1 << 32
    assert native_psnr(lib, sums, w, h) == [0.0, 0.0, 0.0]


def test_psnr_argument_errors(lib):
    out, ssd = (C.c_double * 3)(), (C.c_uint64 * 3)(1, 2, 3)
    for args in [(None, 416, 240, out), (ssd, 416, 240, None), (ssd, 415, 240, out), (ssd, 416, 239, out), (ssd, 0, 240, out), (ssd, 416, 0, out), (ssd, -416, 240, out),
                 (ssd, 416, -240, out)]:
        assert lib.hmr_gpu_psnr(ssd, 416, 240, out) == 0
        assert lib.hmr_gpu_psnr(*args) == ERR_ARG, args[1:3]
        assert lib.hmr_gpu_last_error()


@pytest.mark.parametrize("case", ["200x136", "416x240_flat_qp4", "328x264_wpp3"])
def test_the_fixture_sums_are_those_of_the_checker_builds_reconstruction(cpu, case):
    """numpy's sums of squared differences between the clip and what the checker build (the device path's CPU twin) reconstructs are quality.json's: the fixture is tied
    to the pictures the device path is held to"""
    q, g = QUALITY[case], GOLD[case]
    w, h = q["width"], q["height"]
    raw = []
    _, recon, _ = encode(cpu, case, raw_recon=raw)
    assert recon == q["recon_md5"]
    keys = g["keys"]
    clip = ec.clip_frames(w, h, g["frames"], keys.get("cut_at"), keys.get("clip_seed", 1234), keys.get("content", "default"))
    for f, planes in enumerate(clip):
        d = (np.frombuffer(b"".join(planes), np.uint8).astype(np.int64) - np.frombuffer(raw[f], np.uint8).astype(np.int64)) ** 2
        y, c = w * h, (w // 2) * (h // 2)
        assert [int(d[:y].sum()), int(d[y:y + c].sum()), int(d[y + c:].sum())] == q["ssd"][f], (case, f)


def test_python_psnr_needs_neither_torch_nor_a_gpu():
    q = QUALITY["416x240"]
    code = (f"from homerhevc_amd.encoder import psnr; import homerhevc_amd; v = psnr({q['ssd'][0]!r}, 416, 240); assert 'torch' not in sys.modules, 'torch imported'; "
            "assert homerhevc_amd.psnr is psnr; assert psnr([0, 5, 0], 416, 240)[::2] == (99.99, 99.99); print(repr(list(v)))")
    r = in_a_fresh_process(code)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert all(abs(a - b) <= PSNR_TOLERANCE for a, b in zip(got, q["psnr"][0])), (got, q["psnr"][0])
    r = in_a_fresh_process("from homerhevc_amd.encoder import psnr\ntry:\n    psnr([1, 2, 3], 415, 240)\nexcept ValueError as e:\n    print('refused', e)")
    assert r.returncode == 0 and "refused" in r.stdout, r.stderr


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_enc_export_pictures_device", "hmr_gpu_enc_export_picture_device", "hmr_gpu_psnr"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert "12e." in text
