"""-m gpu: which kernel a pool launch runs, and that each of them writes the reference's streams (k_encode_object.inc launch_pool, enc_platform.h WaveGrpLean).
A launch of more than one worker per compute unit runs k_encode_pool, whose decision walk is compiled without full RDO, unless one of its pictures is RD_FULL:
then it runs k_encode_full, the generic walk.  At most one worker per compute unit is the latency kernel, which stays generic.  A 416 x 240 picture has at most
four CTUs in flight, so 72 sequences in one hmr_gpu_enc_encode_batch call are 288 workers - more than one per compute unit of an MI355X (256); the tests say so
themselves on a device with more compute units than that."""
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


def run_batch(lib, plan):
    """plan: [(fixture, sequences)] - all of them in ONE launch per frame; returns the kernels the launches ran and, per fixture, the set of its sequences' stream digests"""
    encs, case_of, itype = [], [], []
    try:
        return run_batch_on(lib, plan, encs, case_of, itype)
    finally:      # (also when an assertion fails: the encoders of this case are not left to the next one)
        for enc in encs:
            lib.hmr_gpu_enc_destroy(enc)


def run_batch_on(lib, plan, encs, case_of, itype):
    for case, count in plan:
        g = GOLD[case]
        keys = dict(g["keys"])
        cut_at = keys.pop("cut_at", None)
        force_intra = keys.pop("force_intra", 0)
        cfg = ec.default_cfg(g["width"], g["height"], **keys)
        clip = list(ec.clip_frames(g["width"], g["height"], g["frames"], cut_at))
        for _ in range(count):
            enc = C.c_void_p()
            assert lib.hmr_gpu_enc_create(lib._ctx, C.byref(cfg), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
            for f, planes in enumerate(clip):
                assert lib.hmr_gpu_enc_load_source(enc, f, *planes) == 0, lib.hmr_gpu_last_error()
            encs.append(enc); case_of.append(case); itype.append(3 if force_intra else 0)
    n = len(encs)
    if n > 1:      # (pool_inflight of a 416 x 240 picture is 4: the launch must be one of more than one worker per compute unit)
        assert 4 * n > lib._cus, f"{n} sequences are {4 * n} workers: not more than one per compute unit of this device ({lib._cus})"
    assert len({GOLD[c]["frames"] for c in case_of}) == 1      # (the fixtures of one plan have the same length: every launch has all the sequences)
    bufs = [C.create_string_buffer(1 << 16) for _ in range(n)]
    out = [b""] * n
    e_arr = (C.c_void_p * n)(*encs)
    ptrs = (C.c_char_p * n)(*[C.cast(b, C.c_char_p) for b in bufs])
    caps = (C.c_long * n)(*[len(b) for b in bufs])
    types = (C.c_int * n)(*itype)
    got = (C.c_long * n)()
    kernels = set()
    for f in range(GOLD[case_of[0]]["frames"]):
        assert lib.hmr_gpu_enc_encode_batch(e_arr, n, (C.c_int * n)(*([f] * n)), types, ptrs, caps, got) == 0, lib.hmr_gpu_last_error()
        kernels.add(lib.hmr_gpu_enc_last_pool_kernel(encs[0]))
        for i in range(n):
            out[i] += bufs[i].raw[:got[i]]
    digests = {}
    for case, o in zip(case_of, out):
        digests.setdefault(case, set()).add((len(o), hashlib.md5(o).hexdigest()))
    return kernels, digests


def fixture_digest(case):
    return {(GOLD[case]["stream_bytes"], GOLD[case]["stream_md5"])}


@pytest.mark.parametrize("case", ["416x240_wpp_rows", "416x240_scene_cut_wpp_rows"])      # (the scene cut: the I walk inside P frames)
def test_launch_without_rd_full_runs_the_lean_kernel(gpu, case):
    kernels, digests = run_batch(gpu, [(case, 72)])
    assert kernels == {KERNEL_LEAN}
    assert digests[case] == fixture_digest(case)


def test_launch_of_rd_full_pictures_runs_the_full_kernel(gpu):
    case = "416x240_rdfull_wpp_rows"
    kernels, digests = run_batch(gpu, [(case, 72)])
    assert kernels == {KERNEL_FULL}
    assert digests[case] == fixture_digest(case)


def test_mixed_launch_runs_the_full_kernel(gpu):
    plain, rd = "416x240_wpp_rows", "416x240_rdfull_wpp_rows"
    kernels, digests = run_batch(gpu, [(plain, 36), (rd, 36)])
    assert kernels == {KERNEL_FULL}
    assert digests[plain] == fixture_digest(plain)
    assert digests[rd] == fixture_digest(rd)


def test_one_rd_full_sequence_alone_runs_the_latency_kernel(gpu):
    """at most one worker per compute unit: the latency kernel, which keeps full RDO"""
    case = "416x240_force_intra_rdfull_tr4_wpp_rows"
    kernels, digests = run_batch(gpu, [(case, 1)])
    assert kernels == {KERNEL_LAT}
    assert digests[case] == fixture_digest(case)
