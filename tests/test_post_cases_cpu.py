"""The post-decision stage on given CTU records, without a GPU (tests/post_cases.py): the one-lane checker build of enc_post.h / enc_entropy.h / enc_sao.h
(henc_cpu_post_records) against the oracle's independent restatement of the picture path on every case of the sweep, the unmutated reference records against the
reference's own reconstruction, and the MAKE-UP of the sweep - which paths of the stage its inputs reach - counted from the oracle's and the checker's outputs alone.
The make-up figures are conditions on the inputs: one that falls short is mended in the generator (post_cases.py), never by counting the device."""
import functools

import numpy as np
import pytest

import post_cases as pc


@functools.lru_cache(None)
def checker_run(i):
    case = pc.cases()[i]
    rc, out, counters = pc.run_checker(case)
    assert rc == 0, (case["name"], rc, out["errors"])
    return out, counters


CASE_IDS = [c["name"] for c in pc.cases()]


def test_sweep_covers_the_configurations():
    cs = pc.cases()
    assert 30 <= len(cs) <= 45
    mut = [c for c in cs if c["mutated"]]
    assert {c["size"] for c in mut} == set(pc.SIZES) and {c["qp"] for c in mut} == set(pc.QPS) and {c["cqo"] for c in mut} == set(pc.CQOS)
    for key, values in (("sao", {0, 1}), ("sbh", {0, 1}), ("slice", {pc.SLICE_I, pc.SLICE_P}), ("wpp", {0, 1})):
        assert {c[key] for c in mut} == values, key
    assert any(c["threads"] > 1 for c in mut) and any(c["threads"] == 1 and c["wpp"] for c in mut)
    assert len({c["size"] for c in cs if c["planes"]}) >= 2
    assert any(c["groups"] > 1 for c in cs) and any(c["groups"] == 1 for c in cs)
    # every border kind: a partial last column and row, none, two rows, a single row
    grids = {pc.grid(s) + (s[0] % 64, s[1] % 64) for s in pc.SIZES}
    assert {g[1] for g in grids} >= {1, 2, 3, 4} and any(g[2] == 0 and g[3] == 0 for g in grids) and any(g[2] and g[3] for g in grids)
    lib = pc.load_cpu()
    import ctypes as C
    for c in cs:      # make_seq accepts every grid (the device entry applies the same refusals)
        h = lib.henc_cpu_create(C.byref(pc.make_cfg(c)))
        assert h, c["name"]
        lib.henc_cpu_destroy(h)


@pytest.mark.parametrize("i", range(len(CASE_IDS)), ids=CASE_IDS)
def test_checker_agrees_with_the_oracle_chain(i, oracle):
    case = pc.cases()[i]
    out, _ = checker_run(i)
    assert np.array_equal(out["errors"], np.zeros(4, np.int32))
    units, exp = pc.check_against_oracle(oracle, case, out, out, out["geom"], "checker")
    pc.check_streams(case, out, out, "checker")      # (against itself: the rows are there, nothing behind them was written)
    if case["sao"]:
        # a decided SAO_NEW parameter set is the oracle's candidate of its type for the oracle's statistics of the oracle's deblocked picture
        qp0 = np.array([units["uqp"][(n // pc.grid(case["size"])[0]) * 16, (n % pc.grid(case["size"])[0]) * 16] for n in range(out["sao_coded"].shape[0])])
        off, aux = pc.oracle_candidates(oracle, case, exp["stats"], qp0)
        for n, comp in np.argwhere(out["sao_coded"][:, :, 0] == pc.SAO_NEW):
            p = out["sao_coded"][n, comp]
            assert np.array_equal(p[3:], off[n, comp, p[1]]) and p[2] == aux[n, comp, p[1]], f"{case['name']} CTU {n} comp {comp}: coded {p[:12]} candidate {off[n, comp, p[1]][:9]} band {aux[n, comp, p[1]]}"
    if case["fixture_recon"] is not None and not case["mutated"]:
        # the reference's own final reconstruction of this frame
        w, h = case["size"]
        ref, at = case["fixture_recon"], 0
        for k in range(3):
            pw, ph, m = w >> (k > 0), h >> (k > 0), out["geom"]["margin"][k > 0]
            want = ref[at:at + pw * ph].reshape(ph, pw)
            at += pw * ph
            assert np.array_equal(out[f"fin{k}"][m:m + ph, m:m + pw], want), f"{case['name']}: final plane {k} differs from the reference encoder's reconstruction"


def test_make_up_of_the_sweep(oracle):
    """what the inputs reach, from the oracle chain and the checker alone"""
    cs = pc.cases()
    edge = {}
    chroma_sums, chroma_idx = [], []
    outcomes = {0: {}, 1: {}}
    up_at = set()
    offsets, bands = set(), set()
    big_level = 0
    counters = np.zeros(16, np.int64)
    longest_row = 0
    rc_distinct = rc_picture_distinct = 0
    for i, case in enumerate(cs):
        out, cnt = checker_run(i)
        counters += np.array(cnt)
        units = pc.oracle_units(oracle, case)
        if case["rc"]:
            units["uqp"] = out["uqp"].copy()
        exp = pc.oracle_chain(oracle, case, units, out["sao_recon"], out["geom"])
        for k, v in pc.luma_edge_census(units, exp, 0).items():
            edge[k] = edge.get(k, 0) + v
        s, idx = pc.chroma_edge_census(case, units, exp)
        chroma_sums.append(s)
        chroma_idx.append(idx)
        nx, ny = pc.grid(case["size"])
        if case["sao"]:
            for n, row in enumerate(pc.sao_outcomes(case, out["sao_coded"])):
                for comp, o in enumerate(row):
                    outcomes[comp][o] = outcomes[comp].get(o, 0) + 1
                if row[0] == "up" and case["wpp"] and ny > 1:
                    up_at.add(n % nx)
            new = out["sao_coded"][:, :, 0] == pc.SAO_NEW
            offsets.update(np.unique(out["sao_coded"][new][:, 3:]).tolist())
            bo = new & (out["sao_coded"][:, :, 1] == pc.SAO_BO)
            bands.update(out["sao_coded"][bo][:, 2].tolist())
        big_level += int((np.abs(case["records"]["coeff"].astype(np.int32)) >= 1 << 14).sum())
        longest_row = max(longest_row, int(out["bytecnt"].max()))
        if case["rc"]:
            w4, h4 = case["size"][0] // 4, case["size"][1] // 4
            q = out["uqp"][:h4, :w4]
            rc_picture_distinct = max(rc_picture_distinct, len(np.unique(q)))
            for cy in range(ny):
                for cx in range(nx):
                    rc_distinct = max(rc_distinct, len(np.unique(q[cy * 16:cy * 16 + 16, cx * 16:cx * 16 + 16])))
    chroma_sums, chroma_idx = np.concatenate(chroma_sums), np.concatenate(chroma_idx)
    print("luma vertical edge segments:", edge)
    print("chroma edges:", len(chroma_sums), "QP sum", int(chroma_sums.min()), "..", int(chroma_sums.max()), "tc index", int(chroma_idx.min()), "..", int(chroma_idx.max()))
    print("SAO outcomes luma:", outcomes[0], "chroma:", outcomes[1], "merge-up in columns", sorted(up_at))
    print("offsets", sorted(offsets), "band positions", sorted(bands))
    print("levels >= 2^14:", big_level, "coder counters:", counters.tolist(), "longest row:", longest_row, "distinct unit QPs in a rate-controlled CTU:", rc_distinct, "in a picture:", rc_picture_distinct)
    n = edge["segments"]
    for k in ("strong", "normal", "unfiltered"):
        assert edge[k] >= 0.10 * n, (k, edge)
    for k in ("fp_only", "fq_only", "both", "neither"):
        assert edge[k] >= 0.05 * edge["normal"], (k, edge)
    assert edge["clipped"] >= 0.05 * edge["lines"], edge
    # chroma: the QP sum is clipped at both ends (below 0, above 57) and the tc table is read at its last entry and where it is still zero
    assert chroma_sums.min() < 0 and chroma_sums.max() > 57 and chroma_idx.max() == 53 and chroma_idx.min() <= 17
    for comp in (0, 1):
        for o in ("off", "bo", "eo0", "eo1", "eo2", "eo3", "left", "up"):
            assert outcomes[comp].get(o, 0) >= 3, (comp, o, outcomes[comp])
    assert {0, 1} <= up_at, up_at      # the row the context hand-over reads ends behind column 1
    assert 7 in offsets and -7 in offsets
    assert 0 in bands and 28 in bands
    assert big_level >= 1
    assert all(counters[4 + r] >= 1 for r in range(5)), counters      # levels coded with every Rice parameter 0 .. 4
    assert counters[1] >= 1, counters      # a byte the carry changed right behind an 0xff byte
    assert longest_row > 4096
    # Asked for: three distinct unit QPs inside ONE rate-controlled CTU.  That cannot come out of unmutated records: hmr_rc_calc_cu_qp runs once per CTU, so a CTU carries
    # one QP, and the only other value its units can take is the predictor that coding writes into leading CUs without levels (ee_encode_ctu :2091-2104) - two at most,
    # and no content family of tools/gen_yuv.py at these sizes produced even that in its first two frames (every CTU of every probe: one QP).  What the delta-QP syntax
    # needs is a QP that CHANGES from CTU to CTU, so the condition is lowered to: a rate-controlled picture whose CTUs carry at least three distinct QPs.
    assert rc_picture_distinct >= 3, (rc_picture_distinct, rc_distinct)
