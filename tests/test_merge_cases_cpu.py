"""The merge-evaluation cases of tests/merge_cases.py without a GPU: the sweep holds what it is meant to hold (conditions on the inputs: a class that falls short is
mended in the generator, not here), and the Python model of the candidate loop agrees, field for field, with the one-lane checker's own check_rd_cost_merge
(oracle/enc_cpu.cpp henc_cpu_merge_cases) on every case that can go through it - the checker derives its candidate list from neighbour units planted in the CTU's
record, and that list has to be the case's."""
import ctypes as C
import os

import numpy as np
import pytest

import encoder_cases as ec
import libs
import merge_cases as mc
import walk_cases as wc

CU_SIZES = (8, 16)
CPU_FIELDS = tuple(k for k in mc.COMPARED if k != "slots")      # (the checker has no slot word)


@pytest.fixture(scope="module")
def checker():
    lib = C.CDLL(os.path.join(libs.ORACLE_DIR, "libenc_cpu.so"))
    lib.henc_cpu_merge_cases.argtypes = mc.CPU_ARGTYPES
    return lib


def run_checker(checker, bundle, idx):
    """the witness cases `idx` of a bundle through the sequential loop; {case index: output record}"""
    cfg = ec.default_cfg(128, 64)
    arr, nbr = np.ascontiguousarray(bundle["arr"][idx]), np.ascontiguousarray(bundle["nbr"][idx])
    out = np.zeros(len(idx), mc.MERGE_OUT)
    rc = checker.henc_cpu_merge_cases(C.addressof(cfg), arr.ctypes.data, nbr.ctypes.data, len(idx), bundle["arena"].ctypes.data, bundle["arena"].size, out.ctypes.data)
    assert rc == 0, rc
    return dict(zip(idx, out))


def tag_of(c, o):
    return (f"CU {c['cu']} {c['scenario']} classes {mc.classify(c, o)} qp={c['qp']} avg_dist={c['avg_dist']} at=({c['x']},{c['y']}) sbh={c['sbh']} cqo={c['cqo']} perf={c['perf_mode']} "
            f"cands={c['cands']} modes={c['modes']} evals={[(e['cand'], e['no_res'], e['cost'], e['won']) for e in o['evals']]}")


@pytest.mark.parametrize("cu", CU_SIZES)
def test_sweep_holds_every_outcome_class(cu, oracle):
    b = mc.merge_bundle(cu)
    exp = mc.merge_expected(oracle, b)
    cus = b["cus"]
    count, witnessed = {}, {}
    for c, o in zip(cus, exp):
        assert not o["refused"], tag_of(c, o)
        for k in mc.classify(c, o):
            count[k] = count.get(k, 0) + 1
            witnessed[k] = witnessed.get(k, 0) + c["witness"]
    print(cu, sorted(count.items()), "through the checker:", sorted(witnessed.items()))
    # every class at least 8 times; the losing second candidate of class C with levels and level-free
    assert all(count.get(k, 0) >= 8 for k in mc.CLASSES), count
    assert count.get("C/levels", 0) >= 1 and count.get("C/free", 0) >= 1, count
    # the CPU witness: at least half of the sweep and every class
    assert 2 * sum(c["witness"] for c in cus) >= len(cus)
    assert all(witnessed.get(k, 0) >= 1 for k in mc.CLASSES + ("C/levels", "C/free")), witnessed
    # a no-residual evaluation that beats the coded evaluation of the same prediction: only where the keep-or-drop test dropped levels
    for c, o in zip(cus, exp):
        if "E" in mc.classify(c, o):
            assert "dropped" in [o["ev"][0, comp]["cls"] for comp in range(3)], tag_of(c, o)
    # the grid, and what is drawn per grid point
    assert sorted((c["qp"], c["avg_dist"], mc.SCENARIOS.index(c["scenario"])) for c in cus) == sorted(mc.GRID)
    assert {(c["x"], c["y"]) for c in cus} == set(wc.POSITIONS[cu])
    assert {(c["sbh"], c["cqo"]) for c in cus} == {(0, 0), (0, 2), (1, 0), (1, 2)}
    assert {c["perf_mode"] for c in cus} == {1, 2, 3}
    vec = np.array([v for c in cus for v in c["vec"]])
    assert (vec < 0).any(axis=0).all() and (vec > 0).any(axis=0).all()
    assert len({(x & 3, y & 3) for x, y in vec}) == 16
    assert any(x % 8 == 0 and y % 8 == 0 for x, y in vec) and any(x % 4 or y % 4 for x, y in vec)
    lists = [tuple(c["cands"]) for c in cus]
    assert ((0, 0, 0), (0, 0, 0)) in lists and any(a == b and (a[0] or a[1]) for a, b in lists)
    assert {m[2] for pair in lists for m in pair} == {0, -1}
    assert any(a[:2] == b[:2] and a[2] != b[2] for a, b in lists)      # one vector, two references: two candidates, one prediction
    # ties are exact ties: the second candidate's evaluation costs what the first one's cost
    for c, o in zip(cus, exp):
        if "T" in mc.classify(c, o):
            assert o["merge_idx"] == 0 and all(not e["won"] for e in o["evals"] if e["cand"] == 1), tag_of(c, o)
    assert b["arena"].size < 128 << 20


@pytest.mark.parametrize("cu", CU_SIZES)
def test_model_equals_the_sequential_checker(cu, oracle, checker):
    b = mc.merge_bundle(cu)
    exp = mc.merge_expected(oracle, b)
    idx = [i for i, c in enumerate(b["cus"]) if c["witness"]]
    got = run_checker(checker, b, idx)
    via_b0, fails, by_class = 0, [], {}
    for i in idx:
        c, o, g = b["cus"][i], exp[i], got[i]
        derived = [(int(g["cand_mv"][k][0]), int(g["cand_mv"][k][1]), int(g["cand_ref"][k])) for k in range(2)]
        assert derived == c["cands"] and list(g["cand_modes"]) == c["modes"], f"{tag_of(c, o)}: get_merge_candidates derived {derived} modes {list(g['cand_modes'])}"
        bad = mc.differences(g, o, CPU_FIELDS)
        if bad:      # (every case is looked at: the message says which classes and which fields went wrong)
            fails.append(f"{tag_of(c, o)}: the checker and the model differ in {bad}: " + "; ".join(f"{k}: checker {np.asarray(g[k]).ravel()[:24]} model {np.asarray(o[k]).ravel()[:24]}" for k in bad[:4]))
            for k in mc.classify(c, o):
                by_class.setdefault(k, set()).update(bad)
        assert g["n_stale_pred"] == 0
        via_b0 += c["via_b0"] and c["cands"][0][:2] != (0, 0)
    assert not fails, f"{len(fails)} of {len(idx)} cases differ; fields by class: { {k: sorted(v) for k, v in sorted(by_class.items())} }\n" + "\n".join(fails[:3])
    # a non-zero [a, a] list through the top-right unit (B0 equal to A1, B1 intra) where that unit precedes the CU, through two units of different inter_mode elsewhere
    assert via_b0 >= (8 if cu == 16 else 0)
    assert sum(c["witness"] and c["cands"][0] == c["cands"][1] and c["cands"][0][:2] != (0, 0) for c in b["cus"]) >= 8
    assert sum(c["witness"] and (c["x"], c["y"]) == (0, 0) for c in b["cus"]) >= 8


@pytest.mark.parametrize("cu", CU_SIZES)
def test_refusal_cases(cu, oracle):
    """performance_mode 0, and per side of the padded picture a block one sample outside it next to the same case one sample inside"""
    b = mc.refusal_bundle(cu)
    exp = mc.merge_expected(oracle, b)
    want = [True, False] + [False, True] * 4
    assert [o["refused"] for o in exp] == want, [(c["scenario"], o["refused"]) for c, o in zip(b["cus"], exp)]
    for c, o in zip(b["cus"], exp):
        if o["refused"]:
            assert o["slots"] == -1 and np.array_equal(o["pred"], c["pred_window"]) and (o["lv"][:, :cu * cu * 3 // 2] == wc.POISON).all() and o["inter_ref_index"] == mc.SENT_REF
        else:
            assert o["slots"] == 0x10 and o["merge_flag"] == 1
    inside, outside = b["cus"][2::2], b["cus"][3::2]
    assert all(max(abs(a["cands"][1][0] - z["cands"][1][0]), abs(a["cands"][1][1] - z["cands"][1][1])) == 4 for a, z in zip(inside, outside))


@pytest.mark.parametrize("size", mc.MC_SIZES)
def test_motion_compensation_cases(size):
    b = mc.mc_bundle(size)
    vec = np.array([c["vec"][0] for c in b["cus"]])
    assert len({(x & 7, y & 7) for x, y in vec}) == 64 and len({(x & 3, y & 3) for x, y in vec}) == 16
    assert (vec < 0).any(axis=0).all() and (vec > 0).any(axis=0).all()
    assert {c["stride_y"] % 2 for c in b["cus"]} == {0, 1} and {c["stride_c"] % 2 for c in b["cus"]} == {0, 1}
    assert all(wc.GEO[c["node"]]["size"] == size for c in b["cus"])
    # the expected window differs from the one before in the CU's blocks and nowhere else
    for c, e in zip(b["cus"], b["exp"]):
        m = mc.cu_mask(c["node"])
        assert np.array_equal(e["pred"][~m], e["before"][~m]) and not np.array_equal(e["pred"][m], e["before"][m])
    assert b["arena"].size < 64 << 20
