"""The device-only code of the CTU walk against the CPU oracle, block by block (the way test_gpu_prims.py holds the plain primitives): the merge tiles of enc_quad.h
(quad_chain<8 | 16, luma | chroma>: all merge slots of a CU in one matrix-core tile), the two-halves instantiation of the inter TU chain (encode_inter_tu<PairGrp>: the helper
wavefront's U and V plane side by side) and every result of the motion search's multi-candidate byte SAD (multi_sad_u8<4 | 8 | 9>).  The one-lane checker build has none of
these paths and whole streams reach them only with what an encode happens to produce; here each runs as the walk calls it on a synthetic worker (include/homer_gpu.h
section 16) over the sweep of tests/walk_cases.py, whose make-up tests/test_walk_cases_cpu.py checks without a GPU.  Expected values: ora_predict + ora_inter_tu_chain and
numpy; every comparison is exact.  The tiles, the sequential WaveGrp chain on the same data and the oracle must all agree.  (The harness instantiates encode_inter_tu for
group types of its own that derive from WaveGrp and PairGrp: the same statements - every choice is by G::n - compiled a second time, so that the product kernels' code
stays what it is without the harness.  The tiles are the walk's own instantiations.)"""
import ctypes as C

import numpy as np
import pytest

import libs
import walk_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return libs.load_gpu()


def run_walk(gpu, arr, arena):
    out = np.zeros(len(arr), wc.WALK_OUT)
    gpu.hmr_gpu_walk_forms.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    gpu.hmr_gpu_last_error.restype = C.c_char_p
    rc = gpu.hmr_gpu_walk_forms(arr.ctypes.data, len(arr), arena.ctypes.data, arena.size, out.ctypes.data)
    assert rc == 0, gpu.hmr_gpu_last_error()
    return out


def check_block(o, slot, comp, at, e, where):
    """One block of a step's output against eval_block's figures: levels, reconstruction, distortion, level sum, no-residual distortion, cbf."""
    nn = e["lv"].size
    assert np.array_equal(o["lv"][slot][at:at + nn], e["lv"]), f"{where}: levels\ngpu={o['lv'][slot][at:at + nn]}\nora={e['lv']}"
    assert np.array_equal(o["rec"][slot][at:at + nn], e["rec"]), f"{where}: reconstruction\ngpu={o['rec'][slot][at:at + nn]}\nora={e['rec']}"
    got = (int(o["dist"][slot][comp]), int(o["sum"][slot][comp]), int(o["raw"][slot][comp]), int(o["cbf"][slot][comp]))
    assert got == (e["dist"], e["sum"], e["raw"], e["cbf"]), f"{where}: dist, sum, raw, cbf gpu={got} ora={(e['dist'], e['sum'], e['raw'], e['cbf'])}"


@pytest.mark.parametrize("shape", list(wc.SHAPES))
def test_merge_tile_matches_oracle_and_sequential_chain(shape, gpu, oracle):
    b = wc.quad_bundle(shape)
    exp = wc.quad_expected(oracle, b)
    out = run_walk(gpu, b["arr"], b["arena"])
    nslots = 4 if wc.SHAPES[shape][0] == 8 else 2
    n_quad = n_tu = 0
    for o, (ci, kind, s, comp, _, _) in zip(out, b["recs"]):
        c = b["cus"][ci]
        nn = c["n"] * c["n"]
        tag = f"{shape} CU {ci} qp={c['qp']} avg_dist={c['avg_dist']} kind={c['kind']} k={c['k']} at=({c['x']},{c['y']}) sbh={c['sbh']} cqo={c['cqo']} mv={c['mvs']} overlap={c['overlap']}"
        if kind == "quad":
            # every slot of the tile: the distinct ones and the ones that repeat slot 0 (a luma tile of a 16 x 16 CU holds the one slot of the step)
            for slot in ((s,) if shape == "y16" else range(nslots)):
                src_slot = slot if slot < c["k"] else 0
                for pi, cp in enumerate(c["comps"]):
                    where = f"{tag}: tile slot {slot} comp {cp}"
                    assert np.array_equal(o["pred"][slot][pi * nn:(pi + 1) * nn], c["pred"][src_slot, cp].ravel()), f"{where}: prediction"
                    check_block(o, slot, cp, pi * nn, exp[ci][src_slot, cp], where)
            n_quad += 1
        else:
            at = nn if comp == 2 else 0
            where = f"{tag}: sequential chain slot {s} comp {comp}"
            assert np.array_equal(o["pred"][0][at:at + nn], c["pred"][s, comp].ravel()), f"{where}: prediction window"
            check_block(o, 0, comp, at, exp[ci][s, comp], where)
            assert o["stray"] == 0, f"{where}: {o['stray']} words of the windows changed outside the block"
            n_tu += 1
    # every case was looked at: one tile step per CU (two for a 16 x 16 luma CU, one_slot 0 and 1), one sequential call per distinct slot and component
    distinct = sum(c["k"] * len(c["comps"]) for c in b["cus"])
    assert len(b["cus"]) >= len(wc.GRID) and n_quad == len(b["cus"]) * (2 if shape == "y16" else 1) and n_tu == distinct and n_quad + n_tu == len(out)


@pytest.mark.parametrize("n", [4, 8])
def test_wave_halves_match_oracle_and_sequential_chain(n, gpu, oracle):
    b = wc.pair_bundle(n)
    exp = wc.pair_expected(oracle, b)
    out = run_walk(gpu, b["arr"], b["arena"])
    nn = n * n
    for o, (ti, step, comp) in zip(out, b["recs"]):
        t = b["tus"][ti]
        tag = f"{n} x {n} TU {ti} qp={t['qp']} avg_dist={t['avg_dist']} kind={t['kind']} at=({t['x']},{t['y']}) sbh={t['sbh']} cqo={t['cqo']} classes={exp[ti][1]['cls']}/{exp[ti][2]['cls']}"
        for cp in ((1, 2) if step == wc.STEP_TU_PAIR else (comp,)):
            where = f"{tag}: {'two halves' if step == wc.STEP_TU_PAIR else 'one wavefront'} comp {cp}"
            check_block(o, 0, cp, (cp - 1) * nn, exp[ti][cp], where)
        # nothing but the blocks' level and reconstruction areas of the poisoned windows changed, and a step leaves no figures for a plane it did not run
        assert o["stray"] == 0, f"{tag}: step {step}: {o['stray']} words of the windows changed outside the blocks"
        if step == wc.STEP_TU:
            other = 3 - comp
            assert (o["dist"][0][other], o["sum"][0][other], o["raw"][0][other], o["cbf"][0][other]) == (0, 0, 0, 0)


@pytest.mark.parametrize("maxc", wc.SAD_MAXC)
def test_multi_candidate_sad_every_result(maxc, gpu):
    gpu.hmr_gpu_prim_multi_sad.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    gpu.hmr_gpu_last_error.restype = C.c_char_p
    for n in wc.SAD_SIZES:
        for extreme in (False, True):
            c = wc.sad_case(maxc, n, extreme)
            got = np.full(c["off"].shape, 0xdeadbeef, np.uint32)
            rc = gpu.hmr_gpu_prim_multi_sad(maxc, c["src"].ctypes.data, c["plane"].ctypes.data, c["plane"].size, c["off"].ctypes.data, len(c["off"]), c["stride"], n, got.ctypes.data)
            assert rc == 0, gpu.hmr_gpu_last_error()
            present = c["off"] >= 0
            bad = np.argwhere(present & (got != c["exp"]))
            assert bad.size == 0, f"maxc={maxc} n={n} extreme={extreme}: list, candidate {bad[:8].tolist()} offsets={c['off'][bad[0][0]].tolist()} gpu={got[bad[0][0]].tolist()} numpy={c['exp'][bad[0][0]].tolist()}"
            assert (got[~present] == 0).all(), f"maxc={maxc} n={n}: a skipped candidate reports {got[~present].max()}, not 0"
        if n == 64:
            assert got[present].max() == 64 * 64 * 255


def test_harness_refuses_what_it_cannot_read(gpu):
    """The entries check on the host that every address a call can form lies inside what it was given."""
    gpu.hmr_gpu_walk_forms.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    b = wc.quad_bundle("y8")
    out = np.zeros(1, wc.WALK_OUT)
    for field, value in (("sub_y", b["arena"].size), ("sub_y", -(1 << 40)), ("stride_y", 0), ("curr", b["arena"].size - 100), ("node", 5), ("step", 9), ("qp", 52), ("mv", 1 << 20)):
        one = b["arr"][:1].copy()
        one[field] = value
        assert gpu.hmr_gpu_walk_forms(one.ctypes.data, 1, b["arena"].ctypes.data, b["arena"].size, out.ctypes.data) == -3, field
    gpu.hmr_gpu_prim_multi_sad.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    c = wc.sad_case(4, 8)
    got = np.zeros(4, np.uint32)
    for off, maxc, n, stride in (([0, 0, 0, c["plane"].size - 7 * c["stride"] - 7], 4, 8, c["stride"]), ([0, -2, 0, 0], 4, 8, c["stride"]), ([0] * 4, 5, 8, c["stride"]), ([0] * 4, 4, 12, c["stride"]),
                                 ([0] * 4, 4, 8, 0)):
        o = np.array(off, np.int64)
        assert gpu.hmr_gpu_prim_multi_sad(maxc, c["src"].ctypes.data, c["plane"].ctypes.data, c["plane"].size, o.ctypes.data, 1, stride, n, got.ctypes.data) == -3, (off, maxc, n, stride)
