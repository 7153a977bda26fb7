"""The worker / helper-wavefront protocol of the CTU walk against the CPU oracle, step by step: the device-only branches behind HENC_HELPERS (the intra mode search in rounds
of two candidates, the chroma candidate search and the chroma TU with U on the helper, the both-planes SSD of the skip evaluation, the both-planes window copy), the job
bodies of helper_serve, both helper loops and the background intra search with its cancellation (bg_post / bg_take / bg_quiesce, helper_bg_search).  The one-lane checker
build has none of this code and whole streams only say "frame 3 differs"; here each step runs as the walk calls it on a worker with its real helper wavefront
(include/homer_gpu.h section 18) over the cases of tests/helper_cases.py, whose make-up tests/test_helper_cases_cpu.py checks without a GPU.  Expected values: the oracle
and numpy alone; every comparison is exact, the search cost as the bits of the double."""
import ctypes as C

import numpy as np
import pytest

import helper_cases as hc
import libs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    lib = libs.load_gpu()
    lib.hmr_gpu_walk_helper_forms.argtypes = hc.ARGTYPES
    lib.hmr_gpu_last_error.restype = C.c_char_p
    return lib


def run_steps(gpu, arr, arena):
    out = np.zeros(len(arr), hc.HELPER_OUT)
    rc = gpu.hmr_gpu_walk_helper_forms(arr.ctypes.data, len(arr), arena.ctypes.data, arena.size, out.ctypes.data)
    assert rc == 0, gpu.hmr_gpu_last_error()
    return out


_plain = {}


def plain_search(gpu, n):
    """the plain search of block size n: one launch, shared by the tests that compare against it"""
    if n not in _plain:
        b = hc.search_bundle(n, False)
        _plain[n] = run_steps(gpu, b["arr"], b["arena"])
    return _plain[n]


def tag_of(step, i, c):
    return (f"{step} n={c['n']} case {i} ({c['kind']}, target {c['target']}) node {c['node']} at ({c['x']},{c['y']}) nb={c['nb']} rd_mode={c['rd_mode']} dirs={c['nb_dir']} "
            f"seen={c['seen_intra']} sqrt_lambda={c['sqrt_lambda']} strong={c['strong_intra']} picture {c['width']}x{c['height']} ctu ({c['ctu_x']},{c['ctu_y']})")


def check_search(o, e, n, where, own_search):
    """winner, bit cost, cost bits, the neighbour arrays; for a search the worker ran itself also the rounds' buffers as the walk leaves them"""
    got = (int(o["mode"]), int(o["bits"]), int(o["cost_bits"]) if own_search else 0)
    want = (e["mode"], e["bits"], e["cost_bits"] if own_search else 0)
    assert got == want, f"{where}: mode, bits, cost bits gpu={got[0]}, {got[1]}, {got[2]:#018x} ora={want[0]}, {want[1]}, {want[2]:#018x} (candidates {e['preds']}, visited {e['visited']})"
    assert np.array_equal(o["adi"][:4 * n + 1], e["adi"]), f"{where}: Work::adi\ngpu={o['adi'][:4 * n + 1]}\nora={e['adi']}"
    assert np.array_equal(o["adi_f"][:4 * n + 1], e["adi_f"]), f"{where}: Work::adi_f\ngpu={o['adi_f'][:4 * n + 1]}\nora={e['adi_f']}"
    assert not o["adi"][4 * n + 1:].any() and not o["adi_f"][4 * n + 1:].any(), f"{where}: the neighbour arrays behind their 4 n + 1 entries"
    modes, sads = (e["srch_modes"], e["srch_sads"]) if own_search else ([0] * 6, [0] * 5)
    assert list(o["srch_modes"]) == modes and list(o["srch_sads"]) == sads, f"{where}: round buffers gpu={list(o['srch_modes'])} {list(o['srch_sads'])} ora={modes} {sads}"
    assert o["last_slog"] == -1, f"{where}: last_slog {o['last_slog']}"
    assert o["stray"] == 0, f"{where}: {o['stray']} words of the windows changed"


@pytest.mark.parametrize("n", hc.LUMA_SIZES)
def test_intra_search_rounds_with_helper(n, gpu, oracle):
    b = hc.search_bundle(n, False)
    exp = hc.search_expected_all(oracle, n)
    out = plain_search(gpu, n)
    looked = 0
    for i, (o, c, e) in enumerate(zip(out, b["cases"], exp)):
        where = tag_of("INTRA_SEARCH", i, c)
        check_search(o, e, n, where, True)
        assert o["taken"] == -1, where
        looked += 1
    assert looked == len(out) == len(b["cases"]) >= 125


@pytest.mark.parametrize("n", hc.LUMA_SIZES)
def test_intra_search_in_the_background(n, gpu, oracle):
    b = hc.search_bundle(n, True)
    exp = hc.search_expected_all(oracle, n)
    out = run_steps(gpu, b["arr"], b["arena"])
    plain = plain_search(gpu, n)
    seen = {hc.BG_TAKE: 0, hc.BG_TAKE_OTHER: 0, hc.BG_QUIESCE: 0}
    jobs_seen = 0
    for i, (o, p, c, x, e) in enumerate(zip(out, plain, b["cases"], b["extra"], exp)):
        v = x["variant"]
        where = tag_of("INTRA_SEARCH_BG", i, c) + f" variant {('TAKE', 'TAKE_OTHER', 'QUIESCE')[v]} bg_node {x['bg_node']} jobs {x['jobs']}"
        assert o["taken"] == {hc.BG_TAKE: 1, hc.BG_TAKE_OTHER: 0, hc.BG_QUIESCE: -1}[v], f"{where}: bg_take returned {o['taken']}"
        check_search(o, e, n, where, v != hc.BG_TAKE)
        assert (o["mode"], o["bits"]) == (p["mode"], p["bits"]), f"{where}: the background step gives {o['mode']}, {o['bits']}, the plain step {p['mode']}, {p['bits']}"
        nn = (n // 2) ** 2
        for k, job in enumerate(x["jobs"]):
            want = hc.job_expected(oracle, x, job)
            if want is not None:
                assert [int(r) for r in o["job_r"][k][:len(want)]] == want, f"{where}: job {k} ({('', 'SSD', 'INTER_TU', 'SYNC')[job]}) HelperBox::r gpu={list(o['job_r'][k])} expected={want}"
            else:
                for comp in (0, 1):
                    assert np.array_equal(o["lv"][comp][:nn], x["sync"][comp]) and np.array_equal(o["rec"][comp][:nn], x["sync"][2 + comp]), f"{where}: job {k} (SYNC) plane {comp}"
            jobs_seen += 1
        seen[v] += 1
    assert sum(seen.values()) == len(out) == len(b["cases"]) and seen[hc.BG_TAKE] >= 40 and seen[hc.BG_QUIESCE] >= 40 and (n == 64 or seen[hc.BG_TAKE_OTHER] >= 40), seen
    assert jobs_seen == sum(len(x["jobs"]) for x in b["extra"]) and (n == 4 or jobs_seen >= 60)


@pytest.mark.parametrize("nc", hc.CHROMA_SIZES)
def test_chroma_search_u_on_the_helper(nc, gpu, oracle):
    b = hc.chroma_search_bundle(nc)
    exp = hc.chroma_search_expected(oracle, b)
    out = run_steps(gpu, b["arr"], b["arena"])
    looked = 0
    for i, (o, c, e) in enumerate(zip(out, b["cases"], exp)):
        where = f"CHROMA_SEARCH nc={nc} case {i} node {c['node']} at ({c['x']},{c['y']}) nb={c['nb']} cand={c['cand']} picture {c['width']}x{c['height']} ctu ({c['ctu_x']},{c['ctu_y']})"
        assert list(o["sad_u"]) == e[1], f"{where}: sad_u (helper) gpu={list(o['sad_u'])} ora={e[1]}"
        assert list(o["sad_v"]) == e[2], f"{where}: sad_v (worker) gpu={list(o['sad_v'])} ora={e[2]}"
        assert o["stray"] == 0, f"{where}: {o['stray']} words of the windows changed"
        looked += 1
    assert looked == len(out) == len(b["cases"]) >= 40


@pytest.mark.parametrize("nc", hc.CHROMA_SIZES)
def test_chroma_tu_u_on_the_helper(nc, gpu, oracle):
    b = hc.chroma_tu_bundle(nc)
    exp = hc.chroma_tu_expected(oracle, b)
    out = run_steps(gpu, b["arr"], b["arena"])
    nn = nc * nc
    looked = 0
    for i, (o, c, e) in enumerate(zip(out, b["cases"], exp)):
        where = (f"CHROMA_TU nc={nc} case {i} node {c['node']} at ({c['x']},{c['y']}) nb={c['nb']} mode={c['cu_mode']} qp={c['qp']} cqo={c['cqo']} sbh={c['sbh']} slice={c['slice_type']} "
                 f"classes={e[1]['cls']}/{e[2]['cls']}")
        for comp in (1, 2):
            who = f"{where}: plane {comp} ({'helper' if comp == 1 else 'worker'})"
            assert np.array_equal(o["pred"][comp - 1][:nn], e[comp]["pred"]), f"{who}: prediction"
            assert np.array_equal(o["lv"][comp - 1][:nn], e[comp]["lv"]), f"{who}: levels\ngpu={o['lv'][comp - 1][:nn]}\nora={e[comp]['lv']}"
            assert np.array_equal(o["rec"][comp - 1][:nn], e[comp]["rec"]), f"{who}: reconstruction"
            got = (int(o["tu_dist"][comp - 1]), int(o["tu_sum"][comp - 1]))
            assert got == (e[comp]["dist"], e[comp]["sum"]), f"{who}: weighted distortion, level sum gpu={got} ora={(e[comp]['dist'], e[comp]['sum'])}"
        assert np.array_equal(o["cbf_chroma"], e["cbf"]), f"{where}: Work::cbf_chroma"
        assert o["stray"] == 0, f"{where}: {o['stray']} words of the windows changed outside the blocks"
        looked += 1
    assert looked == len(out) == len(b["cases"]) >= 76


@pytest.mark.parametrize("nc", hc.CHROMA_SIZES)
def test_ssd_and_window_copy_of_both_planes(nc, gpu):
    b = hc.plane_pair_bundle(nc)
    out = run_steps(gpu, b["arr"], b["arena"])
    nn = nc * nc
    looked = {hc.STEP_SSD_UV: 0, hc.STEP_SYNC_UV: 0}
    for i, (o, c) in enumerate(zip(out, b["cases"])):
        if c["step"] == hc.STEP_SSD_UV:
            where = f"SSD_UV nc={nc} case {i} node {c['node']} at ({c['x']},{c['y']})"
            assert [int(v) for v in o["ssd"]] == c["exp"], f"{where}: U, V (helper), luma (worker) gpu={list(o['ssd'])} numpy={c['exp']}"
        else:
            where = f"SYNC_UV nc={nc} case {i} node {c['node']} at ({c['x']},{c['y']}) windows {c['wnd']}"
            for comp in (0, 1):
                assert np.array_equal(o["lv"][comp][:nn], c["sync"][comp]), f"{where}: levels of plane {comp}"
                assert np.array_equal(o["rec"][comp][:nn], c["sync"][2 + comp]), f"{where}: reconstruction of plane {comp}"
        assert o["stray"] == 0, f"{where}: {o['stray']} words of the windows changed outside the blocks"
        looked[c["step"]] += 1
    assert looked[hc.STEP_SSD_UV] == looked[hc.STEP_SYNC_UV] == 12 and len(out) == 24


def test_harness_refuses_before_it_launches(gpu):
    """every refusal reason of section 18 (but the one of a build with two helpers per worker, which this library is not) for a case built to trigger it"""
    search, bg, bg64 = hc.search_bundle(16, False), hc.search_bundle(16, True), hc.search_bundle(64, True)
    cs, tu, pp = hc.chroma_search_bundle(8), hc.chroma_tu_bundle(8), hc.plane_pair_bundle(8)
    inner = next(i for i, c in enumerate(search["cases"]) if c["x"] > 0 and c["y"] > 0)
    ssd = next(i for i, c in enumerate(pp["cases"]) if c["step"] == hc.STEP_SSD_UV)
    syn = next(i for i, c in enumerate(pp["cases"]) if c["step"] == hc.STEP_SYNC_UV)
    take = next(i for i, x in enumerate(bg["extra"]) if x["variant"] == hc.BG_TAKE)
    plan = [
        (search, inner, "step", 0, "step"), (search, inner, "node", 400, "node"), (cs, 0, "node", 85, "node (a chroma step needs a CU of 8 or more)"),
        (bg64, 0, "jobs", [hc.JOB_INTER_TU, 0, 0, 0], "node (an INTER_TU job: a CU of 8 to 32)"), (bg, take, "bg_variant", 3, "bg_variant"), (bg, take, "bg_node", 0, "bg_node"),
        (search, inner, "jobs", [hc.JOB_SSD, 0, 0, 0], "jobs"), (search, inner, "ctu_x", 32, "ctu_x / ctu_y"), (search, inner, "width", 8, "width / height"),
        (search, inner, "nb", [2, 0, 0, 0], "nb"), (search, inner, "rd_mode", 1, "strong_intra / rd_mode / seen_intra"), (search, inner, "nb_dir", [35, 1], "nb_dir"),
        (search, inner, "sqrt_lambda", -1.0, "sqrt_lambda"), (search, inner, "qp", 52, "qp"), (search, inner, "chroma_qp_offset", 13, "chroma_qp_offset"),
        (search, inner, "slice_type", 7, "slice_type"), (search, inner, "sign_hiding", 2, "sign_hiding"), (search, inner, "chroma_weight", 0.0, "avg_dist / chroma_weight"),
        (cs, 0, "cand", [35, 0, 0, 0, 0], "cand"), (tu, 0, "cu_mode", 36, "cu_mode"), (tu, 0, "cbf_shift", [5, 0], "cbf_shift"), (pp, syn, "wnd", [7, 0, 0, 1], "wnd"),
        (search, inner, "curr", search["arena"].size - 100, "curr"), (pp, ssd, "pred", -1, "pred"), (search, inner, "nbr", search["arena"].size - 4, "nbr"), (pp, syn, "sync", -1, "sync"),
    ]
    out = np.full(1, 0x55, np.uint8).repeat(hc.HELPER_OUT.itemsize).view(hc.HELPER_OUT)
    for b, i, field, value, reason in plan:
        one = b["arr"][i:i + 1].copy()
        one[field] = value
        rc = gpu.hmr_gpu_walk_helper_forms(one.ctypes.data, 1, b["arena"].ctypes.data, b["arena"].size, out.ctypes.data)
        text = gpu.hmr_gpu_last_error().decode()
        assert rc == -3 and text.endswith("refused: " + reason), (field, value, rc, text)
        assert (out.view(np.uint8) == 0x55).all(), f"{field}: a refused call wrote its output"
    # the case behind the refusals is a good one
    good = run_steps(gpu, search["arr"][inner:inner + 1].copy(), search["arena"])
    assert good["stray"][0] == 0 and good["taken"][0] == -1
