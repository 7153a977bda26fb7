"""Cases and expected values for the merge evaluation of an 8 x 8 or 16 x 16 CU as the device runs it (enc/enc_quad.h: quad_load_cands -> quad_prepare -> quad_merge_loop ->
quad_commit, through include/homer_gpu.h section 19) and for the device-only body of motion_compensate_cu.  Nothing here loads the library under test: a case is numpy
arrays in the layouts the entries take; what one evaluation produces comes from walk_cases.eval_block (ora_predict + ora_inter_tu_chain) per distinct vector and
component; the loop on top of it is `merge_model` below - the sequential loop of check_rd_cost_merge (enc/enc_ctu.h) written out statement by statement, WITHOUT its
repeated-candidate shortcut and WITHOUT the reuse of Enc::inter_ssq: every candidate goes through both evaluations under the loop's own skip rules.

One case is one CU.  The sweep per CU size: node QP 0 .. 51 x avg_dist {0, 400, 6000} x eight scenarios (SCENARIOS) = 1248 cases; CU position, sign hiding, chroma QP
offset, performance mode, picture size, vectors and plane pitches are drawn per case.  The scenarios choose content so that every outcome class of CLASSES occurs; which
class a case IS comes from the model alone (classify), and tests/test_merge_cases_cpu.py holds the counts.

Cases whose vectors are multiples of 8 quarter samples (`witness`) also go through the one-lane checker's own check_rd_cost_merge (oracle/enc_cpu.cpp
henc_cpu_merge_cases), which derives its candidate list from neighbour units planted in the CTU's record (`nbr`)."""
import ctypes as C
import functools

import numpy as np

import walk_cases as wc
from walk_cases import GEO, POISON, POSITIONS, Arena, chroma_weight, node_at, window

STEP_MERGE, STEP_MC = 1, 2
MAX_COST = 0xffffffff // 8
# what the harness plants before a MERGE step (include/homer_gpu.h section 19)
SENT_REF = -7                # Node::inter_ref_index
SENT_NODE = 0xEE             # every other byte of the node but qp
SENT_BUF = 0x77              # Work::cbf_buffs[0..2][depth][units], Work::tr_idx_buffs[depth][units]
SENT_SSQ, SENT_SSQ_VALID = 0xEEEEEEEE, -1


def sent_mode(k, u):         # Work::intra_mode_buffs[k][depth][first unit + u]
    return 0x40 + 0x20 * k + (u & 15)


def sent_cbf(k):             # CtuPublic::cbf[k][units]
    return 0xa0 + k


def record_poison(k):        # a byte array of the record that starts at an even offset, entry k, while it holds the poison word 0x12341234
    return 0x34 if k % 2 == 0 else 0x12


MERGE_CASE = np.dtype([("step", "<i4"), ("node", "<i4"), ("qp", "<i4"), ("perf_mode", "<i4"), ("ctu_x", "<i4"), ("ctu_y", "<i4"), ("width", "<i4"), ("height", "<i4"),
                       ("margin", "<i4"), ("stride_y", "<i4"), ("stride_c", "<i4"), ("sign_hiding", "<i4"), ("chroma_qp_offset", "<i4"), ("old_ref_index", "<i4"),
                       ("reserved", "<i4", (2,)), ("mv", "<i4", (2, 2)), ("ref_idx", "<i4", (2,)), ("inter_modes", "<i4", (2,)), ("avg_dist", "<f8"), ("chroma_weight", "<f8"),
                       ("sub_y", "<i8"), ("sub_c", "<i8", (2,)), ("curr", "<i8"), ("pred", "<i8")])
MERGE_OUT = np.dtype([("slots", "<i4"), ("ret", "<u4"), ("skipped", "<i4"), ("inter_mv", "<i4", (2,)), ("inter_ref_index", "<i4"), ("cost", "<u4"), ("distortion", "<u4"),
                      ("merge_flag", "<i4"), ("merge_idx", "<i4"), ("inter_mode", "<i4"), ("sum", "<u4"), ("inter_cbf", "<i4", (3,)), ("inter_tr_idx", "<i4"),
                      ("inter_ssq", "<u4", (3,)), ("inter_ssq_valid", "<i4"), ("stray", "<u4"), ("pred_rest", "<u4"), ("cand_mv", "<i4", (2, 2)), ("cand_ref", "<i4", (2,)),
                      ("cand_modes", "<i4", (2,)), ("n_stale_pred", "<i4"), ("reserved", "<u4"), ("cbf_buffs", "u1", (3, 16)), ("tr_idx_buffs", "u1", (16,)),
                      ("rec_cbf", "u1", (3, 16)), ("rec_tr_idx", "u1", (16,)), ("rec_intra_mode", "u1", (2, 16)), ("rec_mv_ref_idx", "i1", (16,)),
                      ("lv", "<i2", (2, 384)), ("dec", "<i2", (2, 384)), ("pred", "u1", (6144,))])
# the neighbour units the checker's get_merge_candidates reads (left of the bottom-left unit, above the top-right unit, the top-right unit): pred_mode -1 = not planted
MERGE_NBR = np.dtype([("pred_mode", "<i4"), ("inter_mode", "<i4"), ("mv", "<i4", (2,)), ("ref_idx", "<i4")])
assert MERGE_CASE.itemsize == 152 and MERGE_OUT.itemsize == 9520 and MERGE_NBR.itemsize == 20
GPU_ARGTYPES = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]                  # hmr_gpu_walk_merge_forms(cases, ncases, arena, arena_bytes, out)
CPU_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]      # henc_cpu_merge_cases(cfg, cases, nbr, ncases, arena, arena_bytes, out)

SCENARIOS = ("zero", "rep_levels", "rep_free", "two_coded", "coded_then_free", "free_then_other", "tie", "mixed")
CLASSES = ("A", "B", "C", "D", "E", "F", "G", "T")
GRID = [(qp, ad, s) for qp in wc.QPS for ad in wc.AVG_DISTS for s in range(len(SCENARIOS))]
PM_INTER, PM_INTRA = 0, 1


def depth_of(cu):
    return 3 if cu == 8 else 2


def units_of(cu):
    return cu * cu // 16


def u32(x):
    """(uint32_t)x of a non-negative double below 2^32"""
    return int(x) & 0xffffffff


def cost_rd(avg_dist, s):      # enc_common.h
    return min(max(avg_dist / 1.75, 0.0), 20000.0) * s


def qstep(qp):
    return 2.0 ** ((qp - 4) / 6.0)


# ---- content ---------------------------------------------------------------------------------------------------------------------------------------------------
STRONG = (("dc", 1.0), ("noise", 80), ("inv",), ("dc", -1.0), ("qnoise", 6.0))
WEAK = (("noise", 0), ("noise", 1), ("qnoise", 0.5), ("qnoise", 1.0), ("qnoise", 1.5), ("noise", 3), ("qnoise", 2.5))


def make_pred(rng, src, spec, qp):
    n = src.shape[0]
    s = src.astype(np.int32)
    if spec[0] == "inv":
        return np.where(src >= 128, 0, 255).astype(np.uint8)
    if spec[0] == "dc":          # a constant offset: one large DC coefficient, levels at every QP
        d = int(np.sign(spec[1]) * min(max(np.ceil(abs(spec[1]) * (6.0 * qstep(qp) / n + 3)), 2), 120))
        return np.clip(s + d, 0, 255).astype(np.uint8)
    amp = spec[1] if spec[0] == "noise" else int(min(max(round(qstep(qp) * spec[1]), 1), 120))
    return np.clip(s + rng.integers(-amp, amp + 1, src.shape), 0, 255).astype(np.uint8)


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def hunt_dropped_worse(rng, ora, srcs, qp, cqo, sbh, avg_dist, weight, tries=120):
    """Class E needs a CU whose coded evaluation comes out level-free and dearer than its prediction: a block whose levels the keep-or-drop test zeroes is charged the
    distortion of the levels it dropped (enc_ctu.h, the comment in check_rd_cost_merge).  Small noise at QP 5 .. 22 does that for a few blocks in a hundred, so: two
    components predicted exactly, the third drawn until the oracle says "dropped, and worse than the prediction" (or the tries run out: the case is then what it is)."""
    k = int(rng.integers(3))
    preds = [s.copy() for s in srcs]
    for _ in range(tries):
        preds[k] = make_pred(rng, srcs[k], ("qnoise", 0.5 if rng.integers(3) else 1.0), qp)
        e = wc.eval_block(ora, srcs[k], preds[k], k, qp, cqo, sbh, avg_dist, weight)
        if e["cls"] == "dropped" and e["dist"] > (e["raw"] if k == 0 else u32(weight * e["raw"])):
            break
    return preds


def scenario_content(rng, name, qp):
    """per slot (a, b) and component the kind of prediction; b None: the list repeats a"""
    def all3(spec):
        return [spec, spec, spec]
    if name == "zero":
        return all3(pick(rng, STRONG + WEAK)), None
    if name == "rep_levels":
        return all3(pick(rng, STRONG)), None
    if name == "rep_free":
        return [pick(rng, WEAK[:5]) for _ in range(3)], None
    if name == "two_coded":
        return all3(pick(rng, STRONG)), all3(pick(rng, STRONG))
    if name == "coded_then_free":
        return all3(("dc", float(pick(rng, (0.3, 0.5, 1.0, -0.5))))), (all3(pick(rng, WEAK[2:])) if rng.integers(2) else [pick(rng, WEAK) for _ in range(3)])
    if name == "free_then_other":
        if rng.integers(3) == 0:      # the second prediction IS the source: its no-residual evaluation costs nothing
            return [pick(rng, WEAK[1:5]) for _ in range(3)], all3(("noise", 0))
        return [pick(rng, WEAK[:5]) for _ in range(3)], [pick(rng, WEAK) for _ in range(3)]
    if name == "tie":
        return all3(pick(rng, STRONG + WEAK)), "same"
    return [pick(rng, STRONG + WEAK) for _ in range(3)], [pick(rng, STRONG + WEAK) for _ in range(3)]


# ---- the phase planes of one case ------------------------------------------------------------------------------------------------------------------------------
def build_region(rng, n, chroma, gx, gy, vectors, blocks, stride=None):
    """(walk_cases._region with the stretch fitted to the vectors: whole-sample candidates a block apart share plane 0 and reach further than its fixed margins.)
    Row-interleaved phase planes (include/homer_gpu.h section 13) over the bounding box of the blocks the vectors address, one sample more on every side, random
    bytes, with blocks[k] (or None: the planes' own bytes) written where vectors[k] points.  stride: the row pitch (V takes U's), or None: the box's width plus 0 .. 3.
    Returns the bytes, the row pitch and where sample (0, 0) of plane 0 lies relative to them."""
    phases, sh, mask = (64, 3, 7) if chroma else (16, 2, 3)
    ix = [mx >> sh for mx, _ in vectors]
    iy = [my >> sh for _, my in vectors]
    pad = 1
    rows, cols = max(iy) - min(iy) + n + 2 * pad, max(ix) - min(ix) + n + 2 * pad
    stride = cols + int(rng.integers(0, 4)) if stride is None else stride
    assert stride >= cols
    reg = rng.integers(0, 256, rows * phases * stride).astype(np.uint8)
    for (mx, my), b in zip(vectors, blocks):
        if b is None:
            continue
        f = (my & mask) * (mask + 1) + (mx & mask)
        for r in range(n):
            o = (((my >> sh) - min(iy) + pad + r) * phases + f) * stride + (mx >> sh) - min(ix) + pad
            reg[o:o + n] = b[r]
    origin = (pad - min(iy) - gy) * phases * stride + pad - min(ix) - gx
    return reg, stride, origin


def add_planes(rng, arena, c, blocks):
    """the phase planes of a case's three components into the arena (blocks[comp][k]: what vector k of c["vec"] addresses, or None); sets sub_y, sub_c and the pitches"""
    q = GEO[c["node"]]
    for comp in range(3):
        chroma = comp != 0
        gx, gy = ((c["ctu_x"] >> 1) + q["x"] // 2, (c["ctu_y"] >> 1) + q["y"] // 2) if chroma else (c["ctu_x"] + q["x"], c["ctu_y"] + q["y"])
        reg, stride, origin = build_region(rng, q["size"] // 2 if chroma else q["size"], chroma, gx, gy, c["vec"], blocks[comp], c["stride_c"] if comp == 2 else None)
        at = arena.add(reg) + origin
        if comp == 0:
            c["sub_y"], c["stride_y"] = at, stride
        else:
            c["sub_c"][comp - 1], c["stride_c"] = at, stride


def plane_block(arena, c, mv, comp):
    """the bytes a vector addresses (walk_cases.plane_block with the vector given)"""
    return wc.plane_block(arena, dict(node=c["node"], mvs=[mv], stride_y=c["stride_y"], stride_c=c["stride_c"], sub_y=c["sub_y"], sub_c=c["sub_c"], ctu_x=c["ctu_x"], ctu_y=c["ctu_y"]), 0, comp)


def outside_picture(c, mv):
    """quirk Q12 (enc_ctu.h, enc_quad.h): the candidate's block leaves the padded picture"""
    q = GEO[c["node"]]
    n = q["size"]
    # (C division truncates toward zero)
    spx, spy = c["ctu_x"] + q["x"] + int(mv[0] / 4), c["ctu_y"] + q["y"] + int(mv[1] / 4)
    return spx < -c["margin"] or spx + n > c["width"] + c["margin"] or spy < -c["margin"] or spy + n > c["height"] + c["margin"]


def draw_vectors(rng, cu, whole, two, same_mv=False):
    """one or two vectors in quarter samples.  whole: multiples of 8 (whole luma AND chroma samples), two distinct ones at least a block apart (they share plane 0);
    else two distinct quarter-sample phases (hence distinct planes, luma and chroma)."""
    if whole:
        a = (8 * int(rng.integers(-4, 5)), 8 * int(rng.integers(-4, 5)))
        if not two or same_mv:
            return [a, a][:2 if two else 1]
        d = (int(rng.choice([-1, 1])) * (4 * cu + 8 * int(rng.integers(0, 3))), 8 * int(rng.integers(-2, 3)))
        if rng.integers(2):
            d = (d[1], d[0])
        return [a, (a[0] + d[0], a[1] + d[1])]
    phs = rng.permutation(16)[:2]
    v = [(int(rng.integers(-4, 4)) * 4 + int(p % 4), int(rng.integers(-4, 4)) * 4 + int(p // 4)) for p in phs]
    if not two or same_mv:
        return [v[0], v[0]][:2 if two else 1]
    return v


def plant_neighbours(cu, pos, cands, modes):
    """The neighbour units from which get_merge_candidates derives the list [cands], or None where no planting yields it (a CU at the CTU's origin with anything but
    the zero list).  Returns (nbr[3], whether the derivation goes through the top-right unit)."""
    nbr = np.zeros(3, MERGE_NBR)
    nbr["pred_mode"] = -1
    x, y = POSITIONS[cu][pos]
    (ax, ay, ar), (bx, by, br) = cands
    if (x, y) == (0, 0):
        return (nbr, False) if cands == [(0, 0, 0), (0, 0, 0)] and list(modes) == [1, 1] else None

    def unit(k, mode, mv, ref):
        nbr[k]["pred_mode"], nbr[k]["inter_mode"], nbr[k]["mv"], nbr[k]["ref_idx"] = PM_INTER, mode, mv, ref
    unit(0, modes[0], (ax, ay), ar)      # A1
    if (ax, ay, ar) != (bx, by, br) or modes[0] != modes[1]:
        unit(1, modes[1], (bx, by), br)      # B1 differs from A1 in its vector, its reference or its inter_mode: equal_motion is 0
        return nbr, False
    # B0 equal to A1 with B1 intra: where the top-right unit precedes the CU in z-order (the 16 x 16 CU at (16, 32))
    q = GEO[node_at(x, y, cu)]
    tr_x, tr_y = x + cu, y - 4
    if tr_x < 64 and GEO[node_at(tr_x, tr_y, 4)]["abs_index"] < q["abs_index"]:
        nbr[1]["pred_mode"] = PM_INTRA
        unit(2, modes[1], (bx, by), br)
        return nbr, True
    return None


# ---- the sweep -------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def merge_bundle(cu):
    """The MERGE cases of one CU size: descriptions (`cus`), device cases (`arr`), neighbour plantings (`nbr`) and the arena."""
    import libs
    ora = libs.load_oracle()
    rng = np.random.default_rng(7100 + cu)
    arena, cus = Arena(), []
    n, nc = cu, cu // 2
    for gi, (qp, ad, si) in enumerate(GRID):
        name = SCENARIOS[si]
        two = name not in ("zero", "rep_levels", "rep_free")
        whole = name == "zero" or rng.random() < 0.75
        pos = int(rng.integers(3)) if name == "zero" or not whole else int(rng.choice(3, p=[0.1, 0.45, 0.45]))
        x, y = POSITIONS[cu][pos]
        node = node_at(x, y, cu)
        sbh, cqo, perf = int(rng.integers(4) != 0), int(rng.choice([0, 2])), int(rng.choice([1, 2, 2, 3]))
        ctu_x, ctu_y = 64 * int(rng.integers(0, 30)), 64 * int(rng.integers(0, 17))
        width, height, margin = ctu_x + 64 * int(rng.integers(1, 3)), ctu_y + 64 * int(rng.integers(1, 3)), 80
        sa, sb = scenario_content(rng, name, qp)
        tie_by_ref = name == "tie" and (gi // len(SCENARIOS)) % 2 == 1      # the same vector twice, references 0 and the list's default -1: two candidates, one prediction
        if name == "zero":
            vec = [(0, 0)]
        else:
            vec = draw_vectors(rng, cu, whole, two, same_mv=tie_by_ref)
        refs = [0, -1] if tie_by_ref else ([int(rng.choice([0, 0, -1]))] * 2 if name != "zero" else [0, 0])
        if two and not tie_by_ref and rng.integers(4) == 0:
            refs = [int(rng.choice([0, -1])), int(rng.choice([0, -1]))]
        modes = [1, 1] if name == "zero" else [int(rng.choice([1, 3])), int(rng.choice([1, 3]))]
        if not two and name != "zero":
            # a repeated vector: from the left and the top-right unit where the latter precedes the CU (B0 equal to A1, B1 intra), else from the left and the top
            # unit with different inter_mode (equal units, and the derivation would drop the second)
            modes = [3, 3] if (cu, pos) == (16, 2) and gi % 3 else [1, 3]
        cands = [(vec[0][0], vec[0][1], refs[0]), (vec[-1][0], vec[-1][1], refs[1])]
        distinct_mv = list(dict.fromkeys(vec))
        # source and predictions per distinct vector
        src, made = {}, {}
        for comp in range(3):
            m = n if comp == 0 else nc
            checker = sa[comp][0] == "inv" or (sb not in (None, "same") and sb[comp][0] == "inv")
            src[comp] = wc.checker(m, int(rng.choice([1, 2, 4])), int(rng.integers(2))) if checker else rng.integers(0, 256, (m, m)).astype(np.uint8)
            made[0, comp] = make_pred(rng, src[comp], sa[comp], qp)
            if len(distinct_mv) == 2:
                made[1, comp] = made[0, comp].copy() if sb == "same" else make_pred(rng, src[comp], sb[comp], qp)
        if name == "rep_free" and 5 <= qp <= 22 and gi % 2 == 0:
            for comp, p in enumerate(hunt_dropped_worse(rng, ora, [src[k] for k in range(3)], qp, cqo, sbh, ad, chroma_weight(qp, cqo))):
                made[0, comp] = p
        c = dict(cu=cu, node=node, pos=pos, x=x, y=y, qp=qp, avg_dist=ad, scenario=name, sbh=sbh, cqo=cqo, perf_mode=perf, weight=chroma_weight(qp, cqo), ctu_x=ctu_x, ctu_y=ctu_y,
                 width=width, height=height, margin=margin, cands=cands, modes=modes, vec=distinct_mv, whole=whole, src=src, made=made, old_ref=SENT_REF, sub_c=[0, 0])
        add_planes(rng, arena, c, [[made[s_, comp] for s_ in range(len(distinct_mv))] for comp in range(3)])
        c["curr"] = arena.add(window(rng, src, x, y))
        c["pred_at"] = arena.add(rng.integers(0, 256, wc.WINDOW_BYTES).astype(np.uint8))
        planted = plant_neighbours(cu, pos, cands, modes) if all(v[0] % 8 == 0 and v[1] % 8 == 0 for v in vec) else None
        c["witness"] = planted is not None
        c["nbr"], c["via_b0"] = planted if planted else (None, False)
        cus.append(c)
    bytes_ = arena.bytes()
    for c in cus:
        c["pred"] = {(s, comp): plane_block(bytes_, c, c["vec"][s], comp) for s in range(len(c["vec"])) for comp in range(3)}
        c["pred_window"] = bytes_[c["pred_at"]:c["pred_at"] + wc.WINDOW_BYTES]
        for key, blk in c["made"].items():
            assert np.array_equal(c["pred"][key], blk), "a prediction block was overwritten by another slot's"
    return dict(cu=cu, cus=cus, arr=case_array(cus), nbr=nbr_array(cus), arena=bytes_)


def case_array(cus, step=STEP_MERGE):
    arr = np.zeros(len(cus), MERGE_CASE)
    for a, c in zip(arr, cus):
        a["step"], a["node"], a["qp"], a["perf_mode"] = step, c["node"], c["qp"], c["perf_mode"]
        a["ctu_x"], a["ctu_y"], a["width"], a["height"], a["margin"] = c["ctu_x"], c["ctu_y"], c["width"], c["height"], c["margin"]
        a["stride_y"], a["stride_c"], a["sign_hiding"], a["chroma_qp_offset"], a["old_ref_index"] = c["stride_y"], c["stride_c"], c["sbh"], c["cqo"], c["old_ref"]
        a["mv"] = [(m[0], m[1]) for m in c["cands"]]
        a["ref_idx"] = [m[2] for m in c["cands"]]
        a["inter_modes"] = c["modes"]
        a["avg_dist"], a["chroma_weight"] = c["avg_dist"], c["weight"]
        a["sub_y"], a["sub_c"], a["curr"], a["pred"] = c["sub_y"], c["sub_c"], c["curr"], c["pred_at"]
    return arr


def nbr_array(cus):
    nbr = np.zeros((len(cus), 3), MERGE_NBR)
    nbr["pred_mode"] = -1
    for i, c in enumerate(cus):
        if c.get("nbr") is not None:
            nbr[i] = c["nbr"]
    return nbr


def merge_expected(ora, bundle):
    """Per case the model's outputs (computed once per bundle): eval_block per distinct vector and component, then the loop."""
    if "exp" not in bundle:
        exp = []
        for c in bundle["cus"]:
            ev = {(s, comp): wc.eval_block(ora, c["src"][comp], c["pred"][s, comp], comp, c["qp"], c["cqo"], c["sbh"], c["avg_dist"], c["weight"])
                  for s in range(len(c["vec"])) for comp in range(3)}
            exp.append(merge_model(c, ev))
        bundle["exp"] = exp
    return bundle["exp"]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------------------
def merge_model(c, ev):
    """check_rd_cost_merge (enc/enc_ctu.h) for one CU of 8 or 16 under performance_mode >= 1 (the CU is one TU at its own depth): for cand in the list, for the coded and
    the no-residual evaluation, under the loop's skip rules - merge_cand_buffer, best_is_skip - with everything an evaluation writes: encode_inter (enc_inter.h: node
    cbf / tr_idx / sum, the windows and per-depth buffers of the CU's depth, the record's mv_ref_idx from the node's OLD reference index, Enc::inter_ssq), the
    no-residual branch, put_consolidated_info (window 0 and the record).  Returns the fields of MERGE_OUT and how the case went (`evals`, for classify)."""
    cu, depth, units = c["cu"], depth_of(c["cu"]), units_of(c["cu"])
    nn = (cu * cu, cu * cu // 4, cu * cu // 4)
    at = (0, nn[0], nn[0] + nn[1])
    q = GEO[c["node"]]
    cands, modes = c["cands"], c["modes"]
    pw = np.array(c["pred_window"], np.uint8).copy()

    def pw_block(comp):
        m, p, base = (cu, 64, 0) if comp == 0 else (cu // 2, 32, 4096 + (comp - 1) * 1024)
        x, y = (q["x"], q["y"]) if comp == 0 else (q["x"] // 2, q["y"] // 2)
        idx = base + (y + np.arange(m))[:, None] * p + x + np.arange(m)[None, :]
        return idx
    o = dict(slots=-1, ret=0, skipped=SENT_NODE, inter_mv=[-4370, -4370], inter_ref_index=SENT_REF, cost=0xEEEEEEEE, distortion=0xEEEEEEEE, merge_flag=SENT_NODE,
             merge_idx=SENT_NODE, inter_mode=SENT_NODE, sum=0xEEEEEEEE, inter_cbf=[SENT_NODE] * 3, inter_tr_idx=SENT_NODE, inter_ssq=[SENT_SSQ] * 3,
             inter_ssq_valid=SENT_SSQ_VALID, stray=0, n_stale_pred=0)
    cbf_buffs, tr_idx_buffs = np.full((3, units), SENT_BUF, np.uint8), np.full(units, SENT_BUF, np.uint8)
    rec_cbf = np.array([[sent_cbf(k)] * units for k in range(3)], np.uint8)
    rec_tr_idx = np.array([record_poison(q["abs_index"] + u) for u in range(units)], np.uint8)
    rec_intra = np.array([[record_poison(q["abs_index"] + u) for u in range(units)]] * 2, np.uint8)
    rec_ref = np.array([record_poison(q["abs_index"] + u) for u in range(units)], np.int8)
    mode_buffs = np.array([[sent_mode(k, u) for u in range(units)] for k in range(2)], np.uint8)
    lv, dec = np.full((2, 384), POISON, np.int16), np.full((2, 384), POISON, np.int16)      # [0]: the windows of depth + 1, [1]: window 0
    evals = []
    refused = c["perf_mode"] < 1 or any(outside_picture(c, m) for m in cands)
    if not refused:
        # quad_prepare's slot word: the slot of candidate k in bits 4 k .. 4 k + 3, a slot per distinct (vector, reference)
        keys = list(dict.fromkeys(cands))
        o["slots"] = sum(keys.index(m) << (4 * k) for k, m in enumerate(cands))
        vslot = [c["vec"].index((m[0], m[1])) for m in cands]      # the prediction behind a candidate
        nd = dict(cbf=[SENT_NODE] * 3, tr_idx=SENT_NODE, sum=0xEEEEEEEE, ref=c["old_ref"])
        mcb = [0, 0]
        best_is_skip = best_candidate = have_ctu_cbf = 0
        best_dist = best_cost = MAX_COST
        best_sum = ctu_cbf = 0
        best_mv, best_ref = (0, 0), 0
        for cand in range(2):
            mc_done = False
            s = vslot[cand]
            e3 = [ev[s, comp] for comp in range(3)]
            for no_res in (0, 1):
                if no_res == 1 and mcb[cand] == 1:
                    continue
                if best_is_skip and no_res == 0:
                    continue
                if not mc_done:
                    for comp in range(3):
                        pw[pw_block(comp)] = c["pred"][s, comp]
                    mc_done = True
                if no_res == 0:
                    for comp in range(3):
                        lv[0, at[comp]:at[comp] + nn[comp]] = e3[comp]["lv"]
                        dec[0, at[comp]:at[comp] + nn[comp]] = e3[comp]["rec"]
                    nd["cbf"], nd["tr_idx"], nd["sum"] = [e["cbf"] for e in e3], 0, sum(e["sum"] for e in e3)
                    cbf_buffs[:] = np.array(nd["cbf"], np.uint8)[:, None]
                    tr_idx_buffs[:] = nd["tr_idx"]
                    rec_ref[:] = nd["ref"]
                    o["inter_ssq"], o["inter_ssq_valid"] = [e["raw"] for e in e3], 1
                    dist = (e3[0]["dist"] + e3[1]["dist"] + e3[2]["dist"]) & 0xffffffff
                    cost = u32(float(dist) + cost_rd(c["avg_dist"], nd["sum"]))
                else:
                    dist = e3[0]["raw"]
                    dist = (dist + u32(c["weight"] * e3[1]["raw"])) & 0xffffffff
                    dist = (dist + u32(c["weight"] * e3[2]["raw"])) & 0xffffffff
                    nd["cbf"], nd["tr_idx"], nd["sum"] = [0, 0, 0], 0, 0
                    cost = dist
                won = cost < best_cost      # ("<": the earlier evaluation stays on a tie)
                evals.append(dict(cand=cand, no_res=no_res, cost=cost, won=won, levels=nd["sum"] > 0))
                if won:
                    best_mv, best_ref, best_candidate, best_dist, best_cost, best_sum = (cands[cand][0], cands[cand][1]), cands[cand][2], cand, dist, cost, nd["sum"]
                    if no_res == 1:
                        for comp in range(3):
                            dec[0, at[comp]:at[comp] + nn[comp]] = pw[pw_block(comp)].ravel()
                        lv[0, :] = 0
                        cbf_buffs[:] = np.array(nd["cbf"], np.uint8)[:, None]
                        tr_idx_buffs[:] = nd["tr_idx"]
                    # put_consolidated_info
                    rec_cbf[:], rec_tr_idx[:], rec_intra[:] = cbf_buffs, tr_idx_buffs, mode_buffs
                    lv[1], dec[1] = lv[0], dec[0]
                    ctu_cbf = int(cbf_buffs[0, 0] | cbf_buffs[1, 0] | cbf_buffs[2, 0])
                    have_ctu_cbf = 1
                    best_is_skip = int((ctu_cbf & 1) == 0)
                if no_res == 0:
                    if not have_ctu_cbf:
                        ctu_cbf, have_ctu_cbf = int(rec_cbf[0, 0] | rec_cbf[1, 0] | rec_cbf[2, 0]), 1
                    if ((ctu_cbf >> depth) & 1) == 0:
                        mcb[cand] = 1
        o.update(ret=best_dist, skipped=best_is_skip, inter_mv=list(best_mv), inter_ref_index=best_ref, cost=best_dist, distortion=best_dist, merge_flag=1,
                 merge_idx=best_candidate, inter_mode=modes[best_candidate], sum=best_sum, inter_cbf=nd["cbf"], inter_tr_idx=nd["tr_idx"])
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 16 - units), a.dtype)], axis=1) if a.ndim == 2 else np.concatenate([a, np.zeros(16 - units, a.dtype)])
    o.update(cbf_buffs=pad(cbf_buffs), tr_idx_buffs=pad(tr_idx_buffs), rec_cbf=pad(rec_cbf), rec_tr_idx=pad(rec_tr_idx), rec_intra_mode=pad(rec_intra), rec_mv_ref_idx=pad(rec_ref),
             lv=lv, dec=dec, pred=pw, pred_rest=pred_rest(pw, c["node"]), refused=refused, evals=evals)
    # (the blocks of an 8 x 8 CU take the first 64 + 16 + 16 entries of lv / dec; what lies behind them is 0 in the outputs)
    used = nn[0] + nn[1] + nn[2]
    o["lv"][:, used:] = 0
    o["dec"][:, used:] = 0
    o["ev"] = ev
    return o


def cu_mask(node):
    """the bytes of a 6144-byte window image that belong to the node's three blocks"""
    q = GEO[node]
    m = np.zeros(wc.WINDOW_BYTES, bool)
    m[:4096].reshape(64, 64)[q["y"]:q["y"] + q["size"], q["x"]:q["x"] + q["size"]] = True
    for p in range(2):
        m[4096 + 1024 * p:5120 + 1024 * p].reshape(32, 32)[q["y"] // 2:(q["y"] + q["size"]) // 2, q["x"] // 2:(q["x"] + q["size"]) // 2] = True
    return m


def pred_rest(pw, node):
    """section 19's checksum of the prediction window outside the CU's blocks: sum of (i + 1) x byte i, modulo 2^32"""
    keep = ~cu_mask(node)
    return int(((np.arange(1, wc.WINDOW_BYTES + 1, dtype=np.uint64) * pw.astype(np.uint64))[keep]).sum() & np.uint64(0xffffffff))


def classify(c, o):
    """The outcome classes of a case, from the model's own record of the evaluations."""
    if o["refused"]:
        return []
    ev, evals = o["ev"], o["evals"]
    distinct = c["cands"][0] != c["cands"][1]
    first_levels = sum(ev[0, comp]["sum"] for comp in range(3)) > 0
    second = [e for e in evals if e["cand"] == 1]
    out = []
    if not distinct:
        if first_levels:
            out.append("A")
        else:
            nores = [e for e in second if e["no_res"] == 1]
            assert len(nores) == 1
            out.append("E" if nores[0]["won"] else "D")
    else:
        if first_levels:
            coded = [e for e in second if e["no_res"] == 0]
            assert len(coded) == 1
            out += ["B"] if coded[0]["won"] else ["C", "C/levels" if coded[0]["levels"] else "C/free"]
        else:
            nores = [e for e in second if e["no_res"] == 1]
            assert len(nores) == 1 and not [e for e in second if e["no_res"] == 0]
            out.append("F" if nores[0]["won"] else "G")
        s1 = len(c["vec"]) - 1
        # an exact tie: identical bytes behind both candidates AND equal costs (identical bytes alone are not one: where the first candidate's coded evaluation dropped
        # levels, the second's no-residual evaluation of the same bytes can cost less - class E's mechanism, counted under F)
        first_cost = min(e["cost"] for e in evals if e["cand"] == 0)
        if all(np.array_equal(c["pred"][0, comp], c["pred"][s1, comp]) for comp in range(3)) and all(e["cost"] == first_cost for e in second):
            out.append("T")
    return out


# ---- refusals: quad_prepare returns -1 and touches nothing -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refusal_bundle(cu):
    """performance_mode 0; and per side of the padded picture a vector whose block leaves it by one sample, next to the same case one sample inside (quirk Q12).  The
    planes cover every block the vectors address: a case that is NOT refused is evaluated like any other."""
    rng = np.random.default_rng(4200 + cu)
    arena, cus = Arena(), []
    n, nc = cu, cu // 2
    x, y = POSITIONS[cu][2]
    node = node_at(x, y, cu)
    q = GEO[node]

    def add(perf, width, height, margin, ctu_x, ctu_y, vec, tag):
        src = {comp: rng.integers(0, 256, ((n, n) if comp == 0 else (nc, nc))).astype(np.uint8) for comp in range(3)}
        c = dict(cu=cu, node=node, pos=2, x=x, y=y, qp=30, avg_dist=400.0, scenario=tag, sbh=1, cqo=2, perf_mode=perf, weight=chroma_weight(30, 2), ctu_x=ctu_x, ctu_y=ctu_y,
                 width=width, height=height, margin=margin, cands=[(0, 0, 0), (vec[0], vec[1], 0)], modes=[1, 1], vec=list(dict.fromkeys([(0, 0), vec])), whole=False, src=src,
                 old_ref=SENT_REF, sub_c=[0, 0], witness=False, nbr=None)
        add_planes(rng, arena, c, [[make_pred(rng, src[comp], ("noise", 8), 30) for _ in c["vec"]] for comp in range(3)])
        c["curr"] = arena.add(window(rng, src, x, y))
        c["pred_at"] = arena.add(rng.integers(0, 256, wc.WINDOW_BYTES).astype(np.uint8))
        cus.append(c)
    add(0, 128, 128, 80, 0, 0, (4, -8), "perf_mode 0")
    add(1, 128, 128, 80, 0, 0, (4, -8), "perf_mode 1 (taken)")
    # a picture of one CTU with a small margin: the CU at (x, y), one vector per side
    m = 8
    for side, (dx, dy) in (("left", (-(x + m), 0)), ("right", (64 + m - x - n, 0)), ("top", (0, -(y + m))), ("bottom", (0, 64 + m - y - n))):
        sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
        add(1, 64, 64, m, 0, 0, (4 * dx, 4 * dy), f"{side}: the block ends at the padded picture's edge (taken)")
        add(1, 64, 64, m, 0, 0, (4 * (dx + sx), 4 * (dy + sy)), f"{side}: one sample outside")
    bytes_ = arena.bytes()
    for c in cus:
        c["pred"] = {(s, comp): plane_block(bytes_, c, c["vec"][s], comp) for s in range(len(c["vec"])) for comp in range(3)}
        c["pred_window"] = bytes_[c["pred_at"]:c["pred_at"] + wc.WINDOW_BYTES]
    return dict(cu=cu, cus=cus, arr=case_array(cus), nbr=nbr_array(cus), arena=bytes_)


# ---- motion_compensate_cu ----------------------------------------------------------------------------------------------------------------------------------------
MC_SIZES = (8, 16, 32, 64)


@functools.lru_cache(maxsize=None)
def mc_bundle(size):
    """motion_compensate_cu on a node of `size`: every eighth-sample phase pair (all 64 chroma planes, hence all 16 luma planes), integer parts -3 .. 3 of both signs, odd
    and even plane pitches, the node at every place of POSITIONS' kind (the origin, the far corner, another quadrant)."""
    rng = np.random.default_rng(900 + size)
    arena, cus = Arena(), []
    places = {8: POSITIONS[8], 16: POSITIONS[16], 32: ((0, 0), (32, 32), (32, 0)), 64: ((0, 0),)}[size]
    for ph in range(64):
        x, y = places[ph % len(places)]
        node = node_at(x, y, size)
        q = GEO[node]
        mv = (8 * int(rng.integers(-3, 4)) + (ph & 7), 8 * int(rng.integers(-3, 4)) + (ph >> 3))
        ctu_x, ctu_y = 64 * int(rng.integers(0, 30)), 64 * int(rng.integers(0, 17))
        c = dict(cu=size, node=node, x=x, y=y, qp=30, avg_dist=400.0, sbh=1, cqo=0, perf_mode=2, weight=1.0, ctu_x=ctu_x, ctu_y=ctu_y, width=ctu_x + 64, height=ctu_y + 64, margin=80,
                 cands=[(mv[0], mv[1], 0), (0, 0, 0)], modes=[1, 1], vec=[mv], old_ref=SENT_REF, sub_c=[0, 0])
        add_planes(rng, arena, c, [[None]] * 3)
        c["curr"] = arena.add(rng.integers(0, 256, wc.WINDOW_BYTES).astype(np.uint8))
        c["pred_at"] = arena.add(rng.integers(0, 256, wc.WINDOW_BYTES).astype(np.uint8))
        cus.append(c)
    bytes_ = arena.bytes()
    exp = []
    for c in cus:
        pw = bytes_[c["pred_at"]:c["pred_at"] + wc.WINDOW_BYTES].copy()
        q = GEO[c["node"]]
        pw[:4096].reshape(64, 64)[q["y"]:q["y"] + size, q["x"]:q["x"] + size] = plane_block(bytes_, c, c["vec"][0], 0)
        for p in range(2):
            pw[4096 + 1024 * p:5120 + 1024 * p].reshape(32, 32)[q["y"] // 2:(q["y"] + size) // 2, q["x"] // 2:(q["x"] + size) // 2] = plane_block(bytes_, c, c["vec"][0], 1 + p)
        exp.append(dict(pred=pw, pred_rest=pred_rest(pw, c["node"]), before=bytes_[c["pred_at"]:c["pred_at"] + wc.WINDOW_BYTES]))
    return dict(size=size, cus=cus, arr=case_array(cus, STEP_MC), arena=bytes_, exp=exp)


COMPARED = ("slots", "ret", "skipped", "inter_mv", "inter_ref_index", "cost", "distortion", "merge_flag", "merge_idx", "inter_mode", "sum", "inter_cbf", "inter_tr_idx", "inter_ssq",
            "inter_ssq_valid", "cbf_buffs", "tr_idx_buffs", "rec_cbf", "rec_tr_idx", "rec_intra_mode", "rec_mv_ref_idx", "lv", "dec", "pred", "pred_rest", "stray")


def differences(got, want, fields=COMPARED):
    """the names of the fields in which one output record differs from the model's (or another witness's) record"""
    return [k for k in fields if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64))]
