"""-m gpu: the consolidation copies of the P-slice walk (enc_ctu.h: put / get_back_consolidated_info, consolidate_prediction_info, refresh_deeper_windows).
The walk leaves out a copy where its destination is known to hold the bytes already - the commit of a CU into window 0 after a get_back, the chroma planes of a
get_back after a put and a luma-only intra evaluation - so every branch that sets, clears or uses that knowledge has a fixture here, run as a batch of more than
one worker per compute unit (the throughput kernel, whose walk is the lean instantiation), plus one launch of the generic kernel and one of the latency kernel.
Every stream is its fixture's, byte for byte."""
import ctypes as C
import hashlib
import json
import os

import pytest

import encoder_cases as ec
import libs

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(ec.GOLDEN, "streams.json")))
KERNEL_LAT, KERNEL_LEAN, KERNEL_FULL = 0, 1, 2


@pytest.fixture(scope="module")
def gpu():
    lib = libs.load_gpu()
    P, I, L = C.c_void_p, C.c_int, C.c_long
    lib.hmr_gpu_create.argtypes = [C.POINTER(P), I, P]
    lib.hmr_gpu_enc_create.argtypes = [P, C.POINTER(ec.EncCfg), C.POINTER(P)]
    lib.hmr_gpu_enc_destroy.argtypes = [P]
    lib.hmr_gpu_enc_load_source.argtypes = [P, I] + [C.c_char_p] * 3
    lib.hmr_gpu_enc_encode_batch.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(I), C.POINTER(C.c_char_p), C.POINTER(L), C.POINTER(L)]
    lib.hmr_gpu_enc_last_pool_kernel.argtypes = [P]
    lib.hmr_gpu_last_error.restype = C.c_char_p
    ctx = P()
    assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
    lib._ctx = ctx
    import torch
    lib._cus = torch.cuda.get_device_properties(0).multi_processor_count
    return lib


def run_batch(lib, case, count):
    """`count` sequences of one fixture, all of them in ONE launch per frame; returns the kernels the launches ran and the set of the sequences' stream digests"""
    g = GOLD[case]
    keys = dict(g["keys"])
    cut_at, seed, content = keys.pop("cut_at", None), keys.pop("clip_seed", 1234), keys.pop("content", "default")
    force_intra = keys.pop("force_intra", 0)
    cfg = ec.default_cfg(g["width"], g["height"], **keys)
    clip = ec.clip_frames(g["width"], g["height"], g["frames"], cut_at, seed, content)
    # the workers a picture brings to a launch (k_encode_object.inc pool_inflight): a CTU of every second column, at most one per row; about half under rate control
    inflight = min((g["height"] + 63) // 64, ((g["width"] + 63) // 64 + 1) // 2)
    if keys.get("bitrate_mode", 0):
        inflight = (inflight + 1) // 2
    if count > 1:
        assert inflight * count > lib._cus, f"{count} sequences are {inflight * count} workers: not more than one per compute unit of this device ({lib._cus})"
    encs = []
    try:
        for _ in range(count):
            enc = C.c_void_p()
            assert lib.hmr_gpu_enc_create(lib._ctx, C.byref(cfg), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
            encs.append(enc)
            for f, planes in enumerate(clip):
                assert lib.hmr_gpu_enc_load_source(enc, f, *planes) == 0, lib.hmr_gpu_last_error()
        bufs = [C.create_string_buffer(1 << 18) for _ in range(count)]
        out = [b""] * count
        e_arr = (C.c_void_p * count)(*encs)
        ptrs = (C.c_char_p * count)(*[C.cast(b, C.c_char_p) for b in bufs])
        caps = (C.c_long * count)(*[len(b) for b in bufs])
        types = (C.c_int * count)(*([3 if force_intra else 0] * count))
        got = (C.c_long * count)()
        kernels = set()
        for f in range(g["frames"]):
            assert lib.hmr_gpu_enc_encode_batch(e_arr, count, (C.c_int * count)(*([f] * count)), types, ptrs, caps, got) == 0, lib.hmr_gpu_last_error()
            kernels.add(lib.hmr_gpu_enc_last_pool_kernel(encs[0]))
            for i in range(count):
                out[i] += bufs[i].raw[:got[i]]
    finally:      # (also when an assertion fails: the encoders of this case are not left to the next one)
        for enc in encs:
            lib.hmr_gpu_enc_destroy(enc)
    return kernels, {(len(o), hashlib.md5(o).hexdigest()) for o in out}


def fixture_digest(case):
    return {(GOLD[case]["stream_bytes"], GOLD[case]["stream_md5"])}


@pytest.mark.parametrize("case,count", [
    ("416x240_motion_wpp_rows", 72),          # the motion search beats the merge candidates: put, luma-only intra evaluation, get_back without the chroma planes
    ("416x240_flat_wpp_rows", 72),            # skipped CUs and ended recursions: get_back, then the consolidation whose copy is left out
    ("416x240_noise_wpp_rows", 72),           # the chroma half of the intra evaluation runs, intra wins inside P pictures: nothing may be left out
    ("416x240_extremes_wpp_rows", 72),
    ("416x240_chroma_wpp_rows", 72),          # full-range chroma: a chroma plane that was wrongly not restored shows
    ("416x240_cbr400_perf1_wpp_rows", 144),   # rate control (the CTU's qp in the record; two workers per picture: 144 sequences for the throughput kernel), performance_mode 1
    ("400x104_qp22_perf0_nosao_wpp_rows_clip657909", 144),      # evaluations on a stale prediction window (two CTU rows: 144 sequences again), performance_mode 0
    ("416x240_perf3_wpp_rows", 72),           # performance_mode 3
])
def test_lean_kernel_writes_the_fixture(gpu, case, count):
    kernels, digests = run_batch(gpu, case, count)
    assert kernels == {KERNEL_LEAN}
    assert digests == fixture_digest(case)


def test_generic_kernel_writes_the_fixture(gpu):
    case = "416x240_rdfull_wpp_rows"
    kernels, digests = run_batch(gpu, case, 72)
    assert kernels == {KERNEL_FULL}
    assert digests == fixture_digest(case)


def test_latency_kernel_writes_the_fixture(gpu):
    case = "416x240_scene_cut_wpp_rows"      # (one sequence alone: the walk with the background intra search; the I walk inside P frames after the cut)
    kernels, digests = run_batch(gpu, case, 1)
    assert kernels == {KERNEL_LAT}
    assert digests == fixture_digest(case)
