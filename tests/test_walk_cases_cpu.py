"""The case generator of the device-only walk forms (tests/walk_cases.py) gives the GPU tests what they are meant to sweep - checked with the oracle alone, no GPU.
The floors are conditions on the inputs: a share that falls short is mended in the generator, not here."""
import numpy as np
import pytest

import walk_cases as wc


def shares(evals):
    n = len(evals)
    cls = [e["cls"] for e in evals]
    return dict(n=n, none=cls.count("none") / n, dropped=cls.count("dropped") / n, kept=cls.count("kept") / n, sbh=sum(e["sbh_changed"] for e in evals) / n,
                big=sum(e["max_level"] >= 255 for e in evals))


def check_floors(s, what):
    print(what, {k: (round(v, 3) if isinstance(v, float) else v) for k, v in s.items()})
    for key in ("none", "dropped", "kept", "sbh"):
        assert s[key] >= 0.10, (what, key, s)
    assert s["big"] >= 5, (what, s)


@pytest.mark.parametrize("shape", list(wc.SHAPES))
def test_merge_tile_cases_hold_the_sweep(shape, oracle):
    b = wc.quad_bundle(shape)
    exp = wc.quad_expected(oracle, b)
    cu, chroma = wc.SHAPES[shape]
    cus = b["cus"]
    check_floors(shares([e for per_cu in exp for e in per_cu.values()]), shape)
    # the sweep's grid is all there, and so is everything that is drawn per grid point
    sweep = [c for c in cus if not c["overlap"]]
    assert sorted((c["qp"], c["avg_dist"], c["kind"]) for c in sweep) == sorted(wc.GRID)
    assert {(c["k"], (c["x"], c["y"])) for c in sweep} == {(k, p) for k in wc.SLOT_PATTERNS[cu] for p in wc.POSITIONS[cu]}
    assert {(c["sbh"], c["cqo"]) for c in cus} == {(0, 0), (0, 2), (1, 0), (1, 2)}
    assert any(c["x"] >= 32 or c["y"] >= 32 for c in cus)      # (a node outside the first quadrant: the worker keeps the deep nodes of one quadrant at a time)
    assert all(wc.GEO[c["node"]]["size"] == cu and (wc.GEO[c["node"]]["x"], wc.GEO[c["node"]]["y"]) == (c["x"], c["y"]) for c in cus)
    vec = np.array([c["mvs"][s] for c in cus for s in range(c["k"])])
    assert (vec < 0).any(axis=0).all() and (vec >= 0).any(axis=0).all()
    assert len({(x & 3, y & 3) for x, y in vec}) == 16 and (not chroma or len({(x & 7, y & 7) for x, y in vec}) == 64)
    sh = 3 if chroma else 2
    assert {(x >> sh) & 3 for x, _ in vec} == {0, 1, 2, 3} and {(y >> sh) & 3 for _, y in vec} == {0, 1, 2, 3}
    # the byte the first load of a row starts at: every alignment
    assert {(c["sub_c"][0] if chroma else c["sub_y"]) + ((c["ctu_x"] + c["x"]) >> chroma) + (c["mvs"][s][0] >> sh) & 3 for c in cus for s in range(c["k"])} == {0, 1, 2, 3}
    # distinct slots of a sweep case address distinct planes and hold exactly the blocks made for them; the slots behind them repeat slot 0
    for c in sweep:
        assert len({(x & 3, y & 3) for x, y in c["mvs"][:c["k"]]}) == c["k"] and all(m == c["mvs"][0] for m in c["mvs"][c["k"]:])
        for key, blk in c["made"].items():
            assert np.array_equal(c["pred"][key], blk)
    over = [c for c in cus if c["overlap"]]
    assert len(over) >= 50 and all(len({(x & 7, y & 7) for x, y in c["mvs"]}) == 1 and len(set(c["mvs"][:c["k"]])) == c["k"] for c in over)
    n = b["cus"][0]["n"]
    assert all(abs((a[0] >> sh) - (d[0] >> sh)) < n and abs((a[1] >> sh) - (d[1] >> sh)) < n for c in over for a in c["mvs"] for d in c["mvs"])
    # the device cases: every tile step, and a sequential chain per distinct slot and component
    steps = b["arr"]["step"]
    assert (steps != wc.STEP_TU).sum() == len(cus) * (2 if shape == "y16" else 1)
    assert (steps == wc.STEP_TU).sum() == sum(c["k"] * len(c["comps"]) for c in cus)
    assert b["arena"].size < 128 << 20


@pytest.mark.parametrize("n", [4, 8])
def test_wave_half_cases_hold_the_sweep(n, oracle):
    b = wc.pair_bundle(n)
    exp = wc.pair_expected(oracle, b)
    check_floors(shares([e[comp] for e in exp for comp in (1, 2)]), f"pair {n}")
    assert sorted((t["qp"], t["avg_dist"], t["kind"]) for t in b["tus"]) == sorted(wc.GRID)
    seen = {}
    for e in exp:
        for name in wc.pair_combination(e[1], e[2]):
            seen[name] = seen.get(name, 0) + 1
    print(seen)
    assert all(seen.get(name, 0) >= 5 for name in wc.PAIR_COMBINATIONS), seen
    assert {(t["x"], t["y"]) for t in b["tus"]} == set(wc.POSITIONS[2 * n])
    assert list(b["arr"]["step"][:3]) == [wc.STEP_TU_PAIR, wc.STEP_TU, wc.STEP_TU] and len(b["arr"]) == 3 * len(wc.GRID)


def test_multi_sad_cases():
    for maxc in wc.SAD_MAXC:
        for n in wc.SAD_SIZES:
            c = wc.sad_case(maxc, n)
            off = c["off"]
            assert c["stride"] % 2 == 1
            for k in range(maxc):
                col = off[:, k]
                assert {int(o) & 3 for o in col[col >= 0]} == {0, 1, 2, 3}
            present = off >= 0
            assert present.all(axis=1).any() and (~present).all(axis=1).any()
            for k in range(maxc):
                assert any((~row[k]) and row.sum() == maxc - 1 for row in present) and any(row[k] and row.sum() == 1 for row in present)
            assert (c["exp"][~present] == 0).all() and (c["exp"][present] > 0).all()
            x = wc.sad_case(maxc, n, True)
            assert (x["exp"][x["off"] >= 0] == n * n * 255).all()
    assert wc.sad_case(9, 64, True)["exp"].max() == 64 * 64 * 255
