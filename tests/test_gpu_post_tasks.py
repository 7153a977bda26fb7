"""-m gpu: the post-decision stage of the device - deblocking, SAO statistics / candidates / decision, the SAO and CTU syntax through the lane-spread CABAC, the offset
pass and border padding from the byte tiles, task F, task S, the scheduler (enc_post.h, enc_entropy.h, enc_sao.h, subpel_task.h) - on GIVEN CTU records: the product's
own k_post_frame launched by hmr_gpu_enc_post_records (include/homer_gpu.h section 17) over the sweep of tests/post_cases.py, whose make-up tests/test_post_cases_cpu.py
checks without a GPU.  Every comparison is exact:
  * unit arrays, deblocked picture, final picture with all its margins, phase planes: the oracle chain (hmr_oracle.c's restatements of the reference's functions);
  * sub-stream bytes and lengths, cumbits, contexts, the SAO decision: the one-lane checker build (henc_cpu_post_records), which the CPU file holds to the oracle chain;
  * what the stage must not touch still holds the poison; errors[] is zero;
  * `groups` workgroups give the bytes one workgroup gives: a difference there is a missing dependency in post_scan, not noise - it is reported, never rerun."""
import ctypes as C
import functools

import numpy as np
import pytest

import encoder_cases as ec
import libs
import post_cases as pc

pytestmark = pytest.mark.gpu
CASE_IDS = [c["name"] for c in pc.cases()]
OUTPUTS = ("dbk0", "dbk1", "dbk2", "fin0", "fin1", "fin2", "mvx", "mvy", "ref", "uqp", "flags", "sao_recon", "sao_coded", "bs", "bytecnt", "cumbits", "errors")


@pytest.fixture(scope="module")
def gpu():
    lib = libs.load_gpu()
    lib.hmr_gpu_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    lib.hmr_gpu_enc_create.argtypes = [C.c_void_p, C.POINTER(ec.EncCfg), C.POINTER(C.c_void_p)]
    lib.hmr_gpu_enc_create_serial_pool.argtypes = [C.c_void_p, C.POINTER(ec.EncCfg), C.POINTER(C.c_void_p)]
    lib.hmr_gpu_enc_destroy.argtypes = [C.c_void_p]
    lib.hmr_gpu_enc_post_sizes.argtypes = [C.c_void_p, C.POINTER(pc.PostOut)]
    lib.hmr_gpu_enc_post_records.argtypes = pc.POST_ARGS
    lib.hmr_gpu_last_error.restype = C.c_char_p
    ctx = C.c_void_p()
    assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_record_bytes() == ec.REC
    lib._ctx = ctx
    return lib


@functools.lru_cache(None)
def checker_run(i):
    rc, out, _ = pc.run_checker(pc.cases()[i])
    assert rc == 0, (pc.cases()[i]["name"], rc)
    return out


def make_encoder(gpu, case, serial_pool=False):
    cfg = pc.make_cfg(case)
    enc = C.c_void_p()
    create = gpu.hmr_gpu_enc_create_serial_pool if serial_pool else gpu.hmr_gpu_enc_create
    assert create(gpu._ctx, C.byref(cfg), C.byref(enc)) == 0, (case["name"], gpu.hmr_gpu_last_error())
    return enc


def run_device(gpu, enc, case, groups, with_planes):
    o = pc.PostOut()
    assert gpu.hmr_gpu_enc_post_sizes(enc, C.byref(o)) == 0, gpu.hmr_gpu_last_error()
    a = pc.alloc_out(o, with_planes)
    rec, src = case["records"], case["src"]
    rc = gpu.hmr_gpu_enc_post_records(enc, case["slice"], case["qp"], rec.ctypes.data, rec.nbytes, src[0].ctypes.data, src[1].ctypes.data, src[2].ctypes.data, groups,
                                      int(with_planes), C.byref(o))
    assert rc == 0, (case["name"], groups, rc, gpu.hmr_gpu_last_error(), a["errors"])
    return a


@pytest.mark.parametrize("i", range(len(CASE_IDS)), ids=CASE_IDS)
def test_post_stage_matches_oracle_and_checker(i, gpu, oracle):
    case = pc.cases()[i]
    ref = checker_run(i)
    nx, ny = pc.grid(case["size"])
    # (the one-thread cases without rate control alternate between the two ways to make such an encoder)
    enc = make_encoder(gpu, case, serial_pool=case["threads"] == 1 and not case["rc"] and i % 2 == 1)
    try:
        one = run_device(gpu, enc, case, 1, case["planes"])
        many = run_device(gpu, enc, case, case["groups"], case["planes"]) if case["groups"] > 1 else None
    finally:
        gpu.hmr_gpu_enc_destroy(enc)
    for got, what in ((one, "device, 1 workgroup"), (many, f"device, {case['groups']} workgroups")):
        if got is None:
            continue
        _, exp = pc.check_against_oracle(oracle, case, got, ref, ref["geom"], what)
        pc.check_streams(case, got, ref, what)
        if case["planes"]:
            want = pc.oracle_phase_planes(oracle, exp["fin"])
            for k in range(3):
                y0, y1, x0, x1 = pc.phase_region(case, k, ref["geom"])
                g = got[f"planes{k}"][y0:y1, :, x0:x1].transpose(1, 0, 2)
                bad = np.argwhere(g != want[k][:, y0 - 4:y1 - 4, x0 - 4:x1 - 4])
                assert not len(bad), f"{what} {case['name']}: phase planes of component {k}: {len(bad)} samples differ, first (phase, y - {y0}, x - {x0}) {bad[:4].tolist()}"
    if many is not None:
        nrows = ny if case["wpp"] else 1
        for name in OUTPUTS + (("planes0", "planes1", "planes2") if case["planes"] else ()):
            assert np.array_equal(one[name], many[name]), f"{case['name']}: `{name}` with {case['groups']} workgroups differs from one workgroup's: a dependency of post_scan does not hold"
        assert np.array_equal(one["ctx"][:nrows], many["ctx"][:nrows]) and np.array_equal(one["saved"][:max(nrows - 1, 0)], many["saved"][:max(nrows - 1, 0)]), case["name"]


def test_harness_refuses_what_it_cannot_run(gpu):
    case = pc.cases()[0]
    enc = make_encoder(gpu, case)
    try:
        o = pc.PostOut()
        assert gpu.hmr_gpu_enc_post_sizes(enc, C.byref(o)) == 0
        a = pc.alloc_out(o, False)
        rec, src = case["records"], case["src"]
        good = [enc, case["slice"], case["qp"], rec.ctypes.data, rec.nbytes, src[0].ctypes.data, src[1].ctypes.data, src[2].ctypes.data, 1, 0, C.byref(o)]
        for at, value in ((8, 0), (8, 33), (3, None), (5, None), (0, None), (4, rec.nbytes - ec.REC), (4, rec.nbytes + 1), (1, 0), (1, 3), (2, 52), (2, -1)):
            args = list(good)
            args[at] = value
            assert gpu.hmr_gpu_enc_post_records(*args) == -3, (at, value)
            assert gpu.hmr_gpu_last_error()
        assert gpu.hmr_gpu_enc_post_records(*good[:10], None) == -3
        keep = o.fin[1]
        o.fin[1] = None
        assert gpu.hmr_gpu_enc_post_records(*good) == -3      # a NULL output pointer
        o.fin[1] = keep
        assert gpu.hmr_gpu_enc_post_records(*good[:9], 1, C.byref(o)) == -3      # with_planes without plane buffers
        o.row_cap += 1
        assert gpu.hmr_gpu_enc_post_records(*good) == -3      # sizes that are not the encoder's
        o.row_cap -= 1
        assert gpu.hmr_gpu_enc_post_records(*good) == 0, gpu.hmr_gpu_last_error()
        assert np.array_equal(a["errors"], np.zeros(4, np.int32))
    finally:
        gpu.hmr_gpu_enc_destroy(enc)
