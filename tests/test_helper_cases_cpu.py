"""The case generator of the worker / helper-wavefront steps (tests/helper_cases.py) gives the GPU tests what they are meant to sweep - checked with the oracle alone,
no GPU.  The floors are conditions on the inputs: a sweep that falls short is mended in the generator, not here."""
import ast
import os

import numpy as np
import pytest

import helper_cases as hc
import walk_cases as wc


def test_expected_values_never_come_from_the_library_under_test():
    """helper_cases.py imports neither the GPU library's loader nor the picture binding, and never asks libs for the GPU library"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "helper_cases.py")).read()
    names = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names |= {node.module} | {f"{node.module}.{a.name}" for a in node.names}
        elif isinstance(node, ast.Attribute):
            names.add(node.attr)
        elif isinstance(node, ast.Name):
            names.add(node.id)
    assert "picture_gpu" not in names and "load_gpu" not in names and "libs.load_gpu" not in names and "GPU_SO" not in names, sorted(names & {"picture_gpu", "load_gpu", "GPU_SO"})
    assert hc.HELPER_CASE.itemsize == 216 and hc.HELPER_OUT.itemsize == 12064


@pytest.fixture(scope="module")
def search_exp(oracle):
    return {n: hc.search_expected_all(oracle, n) for n in hc.LUMA_SIZES}


@pytest.mark.parametrize("n", hc.LUMA_SIZES)
def test_search_sweep_per_size(n, search_exp):
    cases, exp = hc.search_cases(n), search_exp[n]
    planted = [(c, e) for c, e in zip(cases, exp) if c["kind"] == "planted"]
    assert sorted(c["target"] for c, _ in planted) == sorted(list(range(35)) * 3)
    winners = {e["mode"] for e in exp}
    hit = sum(e["mode"] == c["target"] for c, e in planted)
    by_bits = {b: sum(e["bits"] == b for e in exp) for b in (0, 1, 12)}
    rounds = {e["round"] for e in exp}
    print(f"n={n}: {len(cases)} cases, {len(winners)} distinct winners, target won {hit} of {len(planted)}, bit costs {by_bits}, rounds {sorted(rounds)}")
    assert len(winners) >= 28, sorted(winners)
    assert all(v >= 10 for v in by_bits.values()), by_bits
    assert rounds == {0, 1, 2, 3}, rounds
    # the other kinds: sinusoid content with missing neighbours and clipped bl_size / tr_size, the extremes
    sin = [c for c in cases if c["kind"] == "sinusoid"]
    assert len(sin) >= 20 and len({c["nb"] for c in sin}) >= 8
    clips = {hc.clip_sizes(c, n, False) for c in sin}
    assert any(bl < n for bl, _ in clips) and any(tr < n for _, tr in clips) and (n, n) in clips, clips
    assert {c["seen_intra"] for c in sin} == {0, 1}
    ext = [(c, e) for c, e in zip(cases, exp) if c["kind"] == "extreme"]
    assert len(ext) == 2 and all(s == 255 * n * n for _, e in ext for s in e["srch_sads"])      # (a flat prediction whatever the direction: every candidate's SAD is the largest there is)
    assert {(c["x"], c["y"]) for c in cases} == set(hc.POSITIONS[n])
    assert {c["rd_mode"] for c in cases} == {hc.RD_DIST_ONLY, hc.RD_FAST} and {c["strong_intra"] for c in cases} == {0, 1}
    # both ways the neighbour directions reach the search: from the mode buffer, and none at the CTU's edge
    assert any(c["nb_dir"][0] >= 0 and c["nb_dir"][1] >= 0 for c in cases) or n == 64
    assert any(c["nb_dir"] == [-1, -1] for c in cases)
    # the device cases: the same list as plain and as background steps, the three variants and every job kind the size allows
    plain, bg = hc.search_bundle(n, False), hc.search_bundle(n, True)
    assert len(plain["arr"]) == len(bg["arr"]) == len(cases)
    assert (plain["arr"]["step"] == hc.STEP_INTRA_SEARCH).all() and (bg["arr"]["step"] == hc.STEP_INTRA_SEARCH_BG).all()
    variants = {x["variant"] for x in bg["extra"]}
    assert variants == ({hc.BG_TAKE, hc.BG_TAKE_OTHER, hc.BG_QUIESCE} if n < 64 else {hc.BG_TAKE, hc.BG_QUIESCE})
    jobs = {j for x in bg["extra"] for j in x["jobs"]}
    assert jobs == (set() if n == 4 else ({hc.JOB_SSD, hc.JOB_SYNC} | ({hc.JOB_INTER_TU} if n <= 32 else set())))
    assert any(not x["jobs"] for x in bg["extra"]) and (n == 4 or any(len(x["jobs"]) >= 2 for x in bg["extra"]))


def test_search_sweep_all_directions_win(search_exp):
    winners = {e["mode"] for n in hc.LUMA_SIZES for e in search_exp[n]}
    assert winners == set(range(35)), sorted(set(range(35)) - winners)


def test_inter_tu_jobs_hold_every_combination(oracle):
    """the INTER_TU jobs of the background steps: U and V of a TU on the helper in every combination of walk_cases.PAIR_COMBINATIONS (the keep-or-drop decision exists
    in the inter chain only: an intra chroma TU is coded or level-free, so the chroma TU list below can hold four of the five)"""
    seen = {}
    for n in (8, 16, 32):
        for x in hc.search_bundle(n, True)["extra"]:
            if hc.JOB_INTER_TU in x["jobs"]:
                hc.job_expected(oracle, x, hc.JOB_INTER_TU)
                for name in wc.pair_combination(x["tu_exp"][1], x["tu_exp"][2]):
                    seen[name] = seen.get(name, 0) + 1
    print(seen)
    assert all(seen.get(name, 0) >= 2 for name in wc.PAIR_COMBINATIONS), seen


@pytest.mark.parametrize("nc", hc.CHROMA_SIZES)
def test_chroma_lists_per_size(nc, oracle):
    n = 2 * nc
    # the TU list: coded and level-free blocks for both planes, in every combination an intra TU can take
    b = hc.chroma_tu_bundle(nc)
    exp = hc.chroma_tu_expected(oracle, b)
    seen = {}
    for e in exp:
        for name in wc.pair_combination(e[1], e[2]):
            seen[name] = seen.get(name, 0) + 1
    print(nc, seen)
    for comp in (1, 2):
        assert {e[comp]["cls"] for e in exp} == {"kept", "none"}
    assert all(seen.get(name, 0) >= 3 for name in ("u_only", "v_only", "both", "neither")), seen
    assert {(c["x"], c["y"]) for c in b["cases"]} == set(hc.POSITIONS[n])
    assert {c["slice_type"] for c in b["cases"]} == {hc.SLICE_P, hc.SLICE_I} and {c["sbh"] for c in b["cases"]} == {0, 1}
    assert {c["qp"] for c in b["cases"]} == set(range(52))
    if nc == 4:
        assert {hc.chroma_scan(nc, c["cu_mode"]) for c in b["cases"]} == {1, 2, 3}
    # the search list: every luma direction behind the DM candidate, missing neighbours, clipped sizes
    s = hc.chroma_search_bundle(nc)
    assert {c["cand"][4] for c in s["cases"]} == set(range(35))
    assert {(c["x"], c["y"]) for c in s["cases"]} == set(hc.POSITIONS[n]) and len({c["nb"] for c in s["cases"]}) >= 7
    clips = {hc.clip_sizes(c, nc, True) for c in s["cases"]}
    assert any(bl < nc for bl, _ in clips) and any(tr < nc for _, tr in clips) and (nc, nc) in clips, clips
    sads = hc.chroma_search_expected(oracle, s)
    assert max(max(e[1] + e[2]) for e in sads) == 255 * nc * nc
    # SSD and window copy: every place, the extreme sum
    p = hc.plane_pair_bundle(nc)
    for step in (hc.STEP_SSD_UV, hc.STEP_SYNC_UV):
        assert {(c["x"], c["y"]) for c in p["cases"] if c["step"] == step} == set(hc.POSITIONS[n])
    assert max(c["exp"][0] for c in p["cases"] if c["step"] == hc.STEP_SSD_UV) == 255 * 255 * nc * nc
    assert all(c["wnd"][0] != c["wnd"][1] and c["wnd"][2] != c["wnd"][3] for c in p["cases"] if c["step"] == hc.STEP_SYNC_UV)
