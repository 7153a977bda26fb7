"""The merge evaluation of an 8 x 8 or 16 x 16 CU as the device runs it - quad_load_cands -> quad_prepare (luma tiles on the worker, chroma tiles on the helper through
HJOB_QUAD_C) -> quad_merge_loop -> quad_commit, enc/enc_quad.h - and the device-only body of motion_compensate_cu, one CU at a time on a worker with its real helper
wavefront (include/homer_gpu.h section 19).  The one-lane checker has none of this code; tests/test_gpu_walk_forms.py pins the tiles' arithmetic, this file what the
replay makes of it: which evaluation wins, what the node, the windows of two depths, the per-depth buffers, the CTU's record, the prediction window and Enc::inter_ssq
hold afterwards - field by field, so that a failure names the field and the outcome class.  Expected values: the Python statement of the sequential loop in
tests/merge_cases.py on the oracle's figures (held to the checker's own check_rd_cost_merge by tests/test_merge_cases_cpu.py), numpy for motion compensation; every
comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import encoder_cases as ec
import libs
import merge_cases as mc

pytestmark = pytest.mark.gpu
CU_SIZES = (8, 16)


@pytest.fixture(scope="module")
def gpu():
    lib = libs.load_gpu()
    lib.hmr_gpu_walk_merge_forms.argtypes = mc.GPU_ARGTYPES
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


def run_steps(gpu, arr, arena):
    out = np.zeros(len(arr), mc.MERGE_OUT)
    rc = gpu.hmr_gpu_walk_merge_forms(arr.ctypes.data, len(arr), arena.ctypes.data, arena.size, out.ctypes.data)
    assert rc == 0, gpu.hmr_gpu_last_error()
    return out


_sweeps = {}


def sweep_out(gpu, cu):
    """the sweep of one CU size on the device: one launch, shared by the tests that read it"""
    if cu not in _sweeps:
        b = mc.merge_bundle(cu)
        _sweeps[cu] = run_steps(gpu, b["arr"], b["arena"])
    return _sweeps[cu]


def tag_of(c, o):
    return (f"CU {c['cu']} {c['scenario']} classes {mc.classify(c, o)} qp={c['qp']} avg_dist={c['avg_dist']} at=({c['x']},{c['y']}) sbh={c['sbh']} cqo={c['cqo']} perf={c['perf_mode']} "
            f"picture {c['width']}x{c['height']}+{c['margin']} ctu ({c['ctu_x']},{c['ctu_y']}) cands={c['cands']} modes={c['modes']} "
            f"evals={[(e['cand'], e['no_res'], e['cost'], e['won']) for e in o['evals']]}")


def compare(cases, got, want, fields, what):
    """every case, every field; the message says how many cases differ, which fields went wrong in which outcome class, and shows the first three"""
    fails, by_class = [], {}
    for c, g, o in zip(cases, got, want):
        bad = mc.differences(g, o, fields)
        if bad:
            fails.append(f"{tag_of(c, o)}: differs in {bad}: " + "; ".join(f"{k}: gpu {np.asarray(g[k]).ravel()[:24]} {what} {np.asarray(o[k]).ravel()[:24]}" for k in bad[:4]))
            for k in mc.classify(c, o) or ["refused"]:
                by_class.setdefault(k, set()).update(bad)
    assert not fails, f"{len(fails)} of {len(cases)} cases differ from {what}; fields by class: { {k: sorted(v) for k, v in sorted(by_class.items())} }\n" + "\n".join(fails[:3])


@pytest.mark.parametrize("cu", CU_SIZES)
def test_merge_replay_and_commit_match_the_sequential_loop(cu, gpu, oracle):
    b = mc.merge_bundle(cu)
    exp = mc.merge_expected(oracle, b)
    out = sweep_out(gpu, cu)
    assert len(out) == len(exp) == len(mc.GRID)
    compare(b["cus"], out, exp, mc.COMPARED, "model")
    assert not out["stray"].any()


@pytest.mark.parametrize("cu", CU_SIZES)
def test_quad_prepare_refuses_and_touches_nothing(cu, gpu, oracle):
    """performance_mode 0 and, per side of the padded picture, a candidate one sample outside it: slot word -1, node, windows, buffers, record and prediction window as
    planted; the same case one sample inside is evaluated"""
    b = mc.refusal_bundle(cu)
    exp = mc.merge_expected(oracle, b)
    out = run_steps(gpu, b["arr"], b["arena"])
    assert [int(s) for s in out["slots"]] == [-1 if o["refused"] else 0x10 for o in exp], [(c["scenario"], int(s)) for c, s in zip(b["cus"], out["slots"])]
    assert sum(o["refused"] for o in exp) == 5
    compare(b["cus"], out, exp, mc.COMPARED, "model")
    assert not out["stray"].any()


@pytest.mark.parametrize("size", mc.MC_SIZES)
def test_motion_compensation_fetches_the_three_blocks(size, gpu):
    b = mc.mc_bundle(size)
    out = run_steps(gpu, b["arr"], b["arena"])
    for c, o, e in zip(b["cus"], out, b["exp"]):
        where = f"node {c['node']} ({size} x {size} at ({c['x']},{c['y']})) mv={c['vec'][0]} ctu ({c['ctu_x']},{c['ctu_y']}) pitches {c['stride_y']}, {c['stride_c']}"
        m = mc.cu_mask(c["node"])
        assert np.array_equal(o["pred"][m], e["pred"][m]), f"{where}: the blocks are not the planes' bytes at the address of section 13"
        assert np.array_equal(o["pred"][~m], e["before"][~m]) and o["pred_rest"] == e["pred_rest"], f"{where}: the prediction window changed outside the CU's blocks"
        assert o["stray"] == 0, f"{where}: {o['stray']} words of the windows or the record changed"


@pytest.mark.parametrize("cu", CU_SIZES)
def test_device_replay_equals_the_checkers_sequential_loop(cu, gpu):
    """identical input to the device (tiles + replay) and to the one-lane checker's own check_rd_cost_merge (the sequential loop on a reference picture, the list derived
    from planted neighbour units): every output but the slot word, which the checker does not have"""
    checker = C.CDLL(os.path.join(libs.ORACLE_DIR, "libenc_cpu.so"))
    checker.henc_cpu_merge_cases.argtypes = mc.CPU_ARGTYPES
    b = mc.merge_bundle(cu)
    idx = [i for i, c in enumerate(b["cus"]) if c["witness"]]
    assert 2 * len(idx) >= len(b["cus"])
    cfg = ec.default_cfg(128, 64)
    arr, nbr = np.ascontiguousarray(b["arr"][idx]), np.ascontiguousarray(b["nbr"][idx])
    cpu = np.zeros(len(idx), mc.MERGE_OUT)
    assert checker.henc_cpu_merge_cases(C.addressof(cfg), arr.ctypes.data, nbr.ctypes.data, len(idx), b["arena"].ctypes.data, b["arena"].size, cpu.ctypes.data) == 0
    out = sweep_out(gpu, cu)[idx]
    fields = tuple(k for k in mc.COMPARED if k != "slots")
    bad = [(i, mc.differences(g, w, fields)) for i, g, w in zip(idx, out, cpu) if mc.differences(g, w, fields)]
    assert not bad, f"{len(bad)} of {len(idx)} cases differ between the device and the checker: " + "; ".join(f"case {i} {b['cus'][i]['scenario']} qp={b['cus'][i]['qp']} cands={b['cus'][i]['cands']}: {f}" for i, f in bad[:5])
    derived = [[(int(w["cand_mv"][k][0]), int(w["cand_mv"][k][1]), int(w["cand_ref"][k])) for k in range(2)] for w in cpu]
    assert derived == [b["cus"][i]["cands"] for i in idx]


def test_harness_refuses_what_it_cannot_run(gpu):
    """every refusal text of the entry a build with one helper and the merge tiles can give, each from one field of an otherwise valid case"""
    b = mc.merge_bundle(8)
    out = np.zeros(1, mc.MERGE_OUT)
    size = b["arena"].size
    mc_case = mc.mc_bundle(8)
    tries = [("step", 0, "step"), ("step", 3, "step"), ("node", 341, "node"), ("node", -1, "node"), ("node", 4, "node (MERGE: an 8 x 8 or 16 x 16 CU)"), ("qp", 52, "qp"),
             ("perf_mode", 4, "perf_mode"), ("chroma_qp_offset", 13, "chroma_qp_offset"), ("sign_hiding", 2, "sign_hiding"), ("avg_dist", -1.0, "avg_dist / chroma_weight"),
             ("chroma_weight", 0.0, "avg_dist / chroma_weight"), ("ctu_x", 32, "ctu_x / ctu_y"), ("ctu_y", -64, "ctu_x / ctu_y"), ("width", 4, "width / height / margin"),
             ("margin", -1, "width / height / margin"), ("stride_y", 0, "stride"), ("stride_c", 1 << 21, "stride"), ("reserved", 1, "reserved"), ("mv", 1 << 15, "mv"),
             ("ref_idx", -2, "ref_idx"), ("inter_modes", 256, "inter_modes"), ("old_ref_index", 128, "old_ref_index"), ("curr", size - 100, "curr"), ("curr", 2, "curr"), ("pred", -4, "pred"),
             ("sub_y", size, "a luma prediction block outside the arena"), ("sub_y", -(1 << 40), "a luma prediction block outside the arena"),
             ("sub_c", size, "a chroma prediction block outside the arena")]
    for field, value, text in tries:
        one = b["arr"][:1].copy()
        one[field] = value
        assert gpu.hmr_gpu_walk_merge_forms(one.ctypes.data, 1, b["arena"].ctypes.data, size, out.ctypes.data) == -3, field
        assert gpu.hmr_gpu_last_error().decode() == f"hmr_gpu_walk_merge_forms: case 0 refused: {text}", (field, gpu.hmr_gpu_last_error())
    one = mc_case["arr"][:1].copy()
    one["node"] = 85      # (a 4 x 4 node)
    assert gpu.hmr_gpu_walk_merge_forms(one.ctypes.data, 1, mc_case["arena"].ctypes.data, mc_case["arena"].size, out.ctypes.data) == -3
    assert gpu.hmr_gpu_last_error().decode().endswith("refused: node (MC: a CU of 8 to 64)")
    # a refused case anywhere in a call refuses the call, and says which
    two = b["arr"][:2].copy()
    two["qp"][1] = -1
    assert gpu.hmr_gpu_walk_merge_forms(two.ctypes.data, 2, b["arena"].ctypes.data, size, out.ctypes.data) == -3
    assert gpu.hmr_gpu_last_error().decode() == "hmr_gpu_walk_merge_forms: case 1 refused: qp"
    assert gpu.hmr_gpu_walk_merge_forms(None, 1, b["arena"].ctypes.data, size, out.ctypes.data) == -3
    assert gpu.hmr_gpu_last_error().decode() == "hmr_gpu_walk_merge_forms: NULL argument or ncases outside 1 .. 2^16"
