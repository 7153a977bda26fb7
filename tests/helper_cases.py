"""Cases and expected values for the worker / helper-wavefront steps of the CTU walk (include/homer_gpu.h section 18): the intra mode search in rounds of two candidates, the
same search as the helper's background job, the chroma candidate search and the chroma TU with U on the helper, the both-planes SSD and the both-planes window copy.
Nothing here touches the GPU: the cases are numpy arrays in the layouts the entry takes, the expected values come from the CPU oracle alone (ora_intra_search,
ora_fill_reference_samples + ora_intra_planar / ora_intra_angular + ora_sad, ora_intra_tu_chain, ora_inter_tu_chain through walk_cases.eval_block) and from numpy.

The search sweep plants the direction: the neighbours are a random walk, the source is the oracle's own prediction of a target direction from those neighbours plus noise
of +-2 - every target 0 .. 34 three times per block size, rd_mode, the neighbour directions and sqrt_lambda drawn per case; then about twenty cases of sinusoid content
with clipped bl_size / tr_size and missing neighbours, and the extremes.  Block sizes: 4 (the NxN partitions of an 8 x 8 CU), 8, 16, 32 and 64 (depth 0) - encode_intra_luma
calls the search for the node of every depth, so no size is left out.  tests/test_helper_cases_cpu.py holds the sweep to its make-up."""
import ctypes as C
import functools
import struct

import numpy as np

import walk_cases as wc
from kernel_cases import intra_is_filtered, mpm_list

STEP_INTRA_SEARCH, STEP_INTRA_SEARCH_BG, STEP_CHROMA_SEARCH, STEP_CHROMA_TU, STEP_SSD_UV, STEP_SYNC_UV = 1, 2, 3, 4, 5, 6
BG_TAKE, BG_TAKE_OTHER, BG_QUIESCE = 0, 1, 2
JOB_NONE, JOB_SSD, JOB_INTER_TU, JOB_SYNC = 0, 1, 2, 3
SLICE_P, SLICE_I = 1, 2
RD_DIST_ONLY, RD_FAST = 0, 2
NWND = 7
POISON = 0x1234

HELPER_CASE = np.dtype([("step", "<i4"), ("node", "<i4"), ("bg_node", "<i4"), ("bg_variant", "<i4"), ("ctu_x", "<i4"), ("ctu_y", "<i4"), ("width", "<i4"), ("height", "<i4"),
                        ("strong_intra", "<i4"), ("rd_mode", "<i4"), ("seen_intra", "<i4"), ("slice_type", "<i4"), ("nb", "<i4", (4,)), ("nb_dir", "<i4", (2,)), ("qp", "<i4"),
                        ("chroma_qp_offset", "<i4"), ("sign_hiding", "<i4"), ("cu_mode", "<i4"), ("cbf_shift", "<i4", (2,)), ("cand", "<i4", (5,)), ("jobs", "<i4", (4,)),
                        ("wnd", "<i4", (4,)), ("reserved", "<i4", (3,)), ("sqrt_lambda", "<f8"), ("chroma_weight", "<f8"), ("avg_dist", "<f8"), ("curr", "<i8"), ("pred", "<i8"),
                        ("nbr", "<i8"), ("sync", "<i8")])
HELPER_OUT = np.dtype([("mode", "<i4"), ("bits", "<i4"), ("taken", "<i4"), ("last_slog", "<i4"), ("cost_bits", "<u8"), ("srch_sads", "<i8", (5,)), ("srch_modes", "<i4", (6,)),
                       ("sad_u", "<u4", (5,)), ("sad_v", "<u4", (5,)), ("job_r", "<u4", (4, 6)), ("tu_dist", "<i4", (2,)), ("tu_sum", "<i4", (2,)), ("ssd", "<u4", (3,)),
                       ("stray", "<u4"), ("cbf_chroma", "u1", (2, 256)), ("adi", "<i2", (264,)), ("adi_f", "<i2", (264,)), ("pred", "u1", (2, 1024)), ("lv", "<i2", (2, 1024)),
                       ("rec", "<i2", (2, 1024))])
assert HELPER_CASE.itemsize == 216 and HELPER_OUT.itemsize == 12064
ARGTYPES = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]      # hmr_gpu_walk_helper_forms(cases, ncases, arena, arena_bytes, out)

LUMA_SIZES = (4, 8, 16, 32, 64)
CHROMA_SIZES = (4, 8, 16, 32)            # the chroma block of a CU of 8 .. 64
# the node's origin in the CTU: both corners and an interior place of another quadrant (a 32 x 32 node is a quadrant: the one beside the first; the 64 x 64 node is the CTU)
POSITIONS = {4: ((0, 0), (60, 60), (24, 40)), 8: wc.POSITIONS[8], 16: wc.POSITIONS[16], 32: ((0, 0), (32, 32), (32, 0)), 64: ((0, 0),)}
SEARCH_POINTS = ((0, 1, 0, 8, 16), (2, 10, 16, 22, 30), (-4, -2, 2, 4, 0), (-1, 1, 0, 0, 0))
NUM_SEARCH_POINTS = (2, 5, 4, 2)
MAX_COST = float(0xffffffff // 8)


def _vp(a, off=0):
    return C.c_void_p(a.ctypes.data + off * a.dtype.itemsize)


def double_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def abs_index(x, y):
    """z-order number of the 4 x 4 unit at (x, y)"""
    a = 0
    for b in range(4):
        a |= (((x >> 2) >> b) & 1) << (2 * b) | (((y >> 2) >> b) & 1) << (2 * b + 1)
    return a


def random_walk(rng, count, step=6):
    return np.clip(int(rng.integers(30, 226)) + np.cumsum(rng.integers(-step, step + 1, count)), 0, 255).astype(np.int16)


def plane_around(nbr, n):
    """A decoded plane that holds the poison everywhere but the 4 n + 1 samples around the block at (1, 1): section 18's nbr order - the column left of it top to
    bottom, the corner, the row above it.  Returns the plane (pitch 2 n + 1)."""
    p = np.full((2 * n + 1, 2 * n + 1), POISON, np.int16)
    p[1:, 0] = nbr[:2 * n]
    p[0, 0] = nbr[2 * n]
    p[0, 1:] = nbr[2 * n + 1:]
    return p


def clip_sizes(c, n, chroma):
    """bl_size / tr_size as node_fill_refs clips them at the picture's edge"""
    q = wc.GEO[c["node"]]
    sh = 1 if chroma else 0
    bl = min(n, (c["height"] >> sh) - ((c["ctu_y"] >> sh) + (q["y"] >> sh) + n))
    tr = min(n, (c["width"] >> sh) - ((c["ctu_x"] >> sh) + (q["x"] >> sh) + n))
    return bl, tr


def predict(ora, adi, n, mode, is_luma):
    pred = np.zeros((n, n), np.int16)
    if mode == 0:
        ora.ora_intra_planar(_vp(pred), n, _vp(adi), 4 * n + 1, n)
    else:
        ora.ora_intra_angular(_vp(pred), n, _vp(adi), 4 * n + 1, n, mode, is_luma)
    return pred


def sad(ora, a, b):
    n = a.shape[0]
    a16, b16 = np.ascontiguousarray(a, np.int16), np.ascontiguousarray(b, np.int16)      # (held here: the call sees only their addresses)
    ora.ora_sad.restype = C.c_uint32
    return int(ora.ora_sad(_vp(a16), n, _vp(b16), n, n))


def neighbour_dirs(c):
    """left / top direction as intra_neighbour_dirs finds them: inside the CTU from the worker's mode buffer when the thread has seen an intra walk, else DC (-1 here)"""
    q = wc.GEO[c["node"]]
    return (c["nb_dir"][0] if q["x"] > 0 and c["seen_intra"] else -1, c["nb_dir"][1] if q["y"] > 0 and c["seen_intra"] else -1)


def search_expected(ora, c):
    """What intra_mode_search leaves for a case: ora_intra_search for winner, bit cost, cost and the neighbour arrays; the walk replayed on the oracle's SADs for the
    round the winner came from and for what the round buffers hold in the end (srch_modes / srch_sads are reused from round to round)."""
    n = c["n"]
    plane = plane_around(c["nbr"], n)
    orig = np.ascontiguousarray(c["src"], np.int16)
    bl, tr = clip_sizes(c, n, False)
    preds = mpm_list(*neighbour_dirs(c))
    pbits, other = (([1, 1, 1], 12) if c["rd_mode"] == RD_FAST else ([0, 0, 0], 0))
    adi, adif, pred = np.zeros(4 * n + 1, np.int16), np.zeros(4 * n + 1, np.int16), np.zeros((n, n), np.int16)
    out, cost = np.zeros(2, np.int32), C.c_double(0)
    pa, ba = np.array(preds, np.int32), np.array(pbits, np.int32)
    ora.ora_intra_search(_vp(orig), n, _vp(plane), 2 * n + 1, n, *[int(v) for v in c["nb"]], bl, tr, c["strong_intra"], _vp(pa), _vp(ba), other, C.c_double(c["sqrt_lambda"]),
                         _vp(adi), _vp(adif), _vp(pred), n, _vp(out), C.byref(cost))
    # the replay
    best, new_best, best_bits, lo, hi, best_cost, won_in = 0, 0, 0, 0, 1, MAX_COST, -1
    modes_buf, sads_buf, visited = [0] * 6, [0] * 5, []
    for loop in range(4):
        if loop == 1:
            best, lo, hi = 2, 2, 34
        cand = [best + SEARCH_POINTS[loop][k] for k in range(NUM_SEARCH_POINTS[loop])]
        cand = [m for m in cand if lo <= m <= hi]
        for k, m in enumerate(cand):
            s = sad(ora, orig, predict(ora, adif if intra_is_filtered(n, m) else adi, n, m, 1))
            modes_buf[k], sads_buf[k] = m, s
            bits = (1 if m in preds else 12) if c["rd_mode"] == RD_FAST else 0
            cst = float(s) + bits * c["sqrt_lambda"]
            visited.append(m)
            if cst < best_cost:
                best_cost, new_best, best_bits, won_in = cst, m, bits, loop
        best = new_best
    assert (best, best_bits, double_bits(best_cost)) == (int(out[0]), int(out[1]), double_bits(cost.value)), "the replay of the walk and ora_intra_search disagree"
    return dict(mode=int(out[0]), bits=int(out[1]), cost_bits=double_bits(cost.value), adi=adi, adi_f=adif, round=won_in, srch_modes=modes_buf, srch_sads=sads_buf, visited=visited,
                preds=preds)


def planted_source(ora, rng, nbr, n, target, nb, bl, tr, strong):
    """the oracle's prediction of `target` from the neighbours as the search will see them, plus noise of +-2"""
    plane = plane_around(nbr, n)
    adi, adif = np.zeros(4 * n + 1, np.int16), np.zeros(4 * n + 1, np.int16)
    ora.ora_fill_reference_samples(_vp(plane), 2 * n + 1, n, *nb, bl, tr, _vp(adi))
    ora.ora_adi_filter(_vp(adi), _vp(adif), 4 * n + 1, n, strong)
    p = predict(ora, adif if intra_is_filtered(n, target) else adi, n, target, 1)
    return np.clip(p.astype(np.int32) + rng.integers(-2, 3, (n, n)), 0, 255).astype(np.uint8)


def _picture(rng, x, y, n, clip):
    """CTU origin and picture size for a node at (x, y): far from the edges, or with the picture ending `clip` = (below, right) samples behind the block"""
    ctu_x, ctu_y = 64 * int(rng.integers(0, 20)), 64 * int(rng.integers(0, 12))
    if clip is None:
        return ctu_x, ctu_y, ctu_x + 192, ctu_y + 192
    return ctu_x, ctu_y, (ctu_x + x + n + clip[1] + 7) & ~7, (ctu_y + y + n + clip[0] + 7) & ~7      # (a picture is a multiple of the smallest CU)


@functools.lru_cache(maxsize=None)
def search_cases(n):
    """The luma cases of block size n (dicts; the oracle makes the planted sources, so the list needs it - loaded here, never the library under test)."""
    import libs
    ora = libs.load_oracle()
    rng = np.random.default_rng(1800 + n)
    cases = []
    pos = POSITIONS[n]

    def add(kind, x, y, nbr, src_fn, nb, clip, rd_mode, dirs, lam, strong, seen=1, target=-1):
        ctu_x, ctu_y, width, height = _picture(rng, x, y, n, clip)
        c = dict(kind=kind, n=n, node=wc.node_at(x, y, n), x=x, y=y, nbr=nbr, nb=nb, ctu_x=ctu_x, ctu_y=ctu_y, width=width, height=height, rd_mode=rd_mode,
                 nb_dir=[dirs[0] if x > 0 else -1, dirs[1] if y > 0 else -1], sqrt_lambda=lam, strong_intra=strong, seen_intra=seen, target=target)
        c["src"] = src_fn(c)
        cases.append(c)

    # every target three times: the direction planted in the source
    for rep in range(3):
        for target in range(35):
            i = rep * 35 + target
            x, y = pos[(i + rep) % len(pos)]
            nbr = random_walk(rng, 4 * n + 1)
            rd_mode = RD_FAST if i % 3 else RD_DIST_ONLY
            # the neighbour directions: the target itself on one side in half of the priced cases (its bit cost is 1 then), anything else otherwise
            dirs = [int(rng.integers(0, 35)), int(rng.integers(0, 35))]
            if rd_mode == RD_FAST and i % 2:
                dirs[int(rng.integers(2)) if x > 0 and y > 0 else (0 if x > 0 else 1)] = target
            lam = float(rng.choice([0.75, 1.5, 3.0, 5.25]))
            strong = int(rng.integers(2))
            nb = (1, 1, 1, 1)
            add("planted", x, y, nbr, lambda c: planted_source(ora, rng, c["nbr"], n, target, nb, *clip_sizes(c, n, False), strong), nb, None, rd_mode, dirs, lam, strong, target=target)
    # sinusoid content (the kind of kernel_cases.k_intra_search) with missing neighbours and clipped bl_size / tr_size
    for i in range(20):
        x, y = pos[i % len(pos)]
        th, period, amp = float(rng.uniform(0, np.pi)), float(rng.uniform(3, 24)), float(rng.uniform(10, 100))
        yy, xx = np.mgrid[0:2 * n + 1, 0:2 * n + 1]
        base = np.clip(128 + amp * np.sin((xx * np.cos(th) + yy * np.sin(th)) / period) + rng.integers(-3, 4, xx.shape), 0, 255).astype(np.int16)
        nbr = np.concatenate([base[1:, 0], base[0:1, 0], base[0, 1:]])
        nb = tuple(int(v) for v in ((1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (1, 1, 0, 1), (1, 1, 1, 0), (1, 0, 1, 0), (0, 1, 0, 1))[i % 8])
        clip = ((0, 0), (8, 0), (0, 8), (n, 8), (64, 64))[i % 5]
        add("sinusoid", x, y, nbr, lambda c: base[1:n + 1, 1:n + 1].astype(np.uint8), nb, clip, RD_FAST if i % 2 else RD_DIST_ONLY, [int(rng.integers(0, 35)), int(rng.integers(0, 35))],
            float(rng.uniform(0.5, 9.0)), i % 2, seen=int(i % 7 != 0))
    # the extremes: all-0 source against all-255 neighbours, and the reverse
    for lo, hi in ((0, 255), (255, 0)):
        x, y = pos[-1]
        add("extreme", x, y, np.full(4 * n + 1, hi, np.int16), lambda c: np.full((n, n), lo, np.uint8), (1, 1, 1, 1), None, RD_FAST, [10, 26], 4.0, 1)
    return cases


def search_expected_all(ora, n):
    cases = search_cases(n)
    if "exp" not in cases[0]:
        for c in cases:
            c["exp"] = search_expected(ora, c)
    return [c["exp"] for c in cases]


def chroma_blocks(rng, nc, kind):
    """source and prediction blocks of both chroma planes with different kinds of content (walk_cases' kinds)"""
    src = {comp: wc.source_block(rng, nc, (kind + 3 * (comp - 1)) % wc.KINDS) for comp in (1, 2)}
    pred = {comp: wc.prediction_block(rng, src[comp], (kind + 3 * (comp - 1)) % wc.KINDS) for comp in (1, 2)}
    return src, pred


def _fill_common(a, c):
    a["node"], a["ctu_x"], a["ctu_y"], a["width"], a["height"] = c["node"], c["ctu_x"], c["ctu_y"], c["width"], c["height"]
    a["slice_type"], a["chroma_weight"] = c.get("slice_type", SLICE_P), c.get("weight", 1.0)
    a["qp"], a["chroma_qp_offset"], a["sign_hiding"], a["avg_dist"] = c.get("qp", 30), c.get("cqo", 0), c.get("sbh", 0), c.get("avg_dist", 0.0)
    a["nb"] = c.get("nb", (0, 0, 0, 0))
    a["curr"] = a["pred"] = a["nbr"] = a["sync"] = -1


@functools.lru_cache(maxsize=None)
def search_bundle(n, bg):
    """The device cases of block size n: the plain search (bg False), or the same cases as background steps - the three variants in turn, with job lists drawn from
    the chroma jobs of the inter evaluation (a CU of 8 or more has chroma blocks a job can work on; INTER_TU: up to 32)."""
    cases = search_cases(n)
    rng = np.random.default_rng(77 + n)
    arena = wc.Arena()
    arr = np.zeros(len(cases), HELPER_CASE)
    extra = []
    for i, (c, a) in enumerate(zip(cases, arr)):
        _fill_common(a, c)
        a["step"] = STEP_INTRA_SEARCH_BG if bg else STEP_INTRA_SEARCH
        a["strong_intra"], a["rd_mode"], a["seen_intra"], a["nb_dir"], a["sqrt_lambda"] = c["strong_intra"], c["rd_mode"], c["seen_intra"], c["nb_dir"], c["sqrt_lambda"]
        a["nbr"] = arena.add(np.ascontiguousarray(c["nbr"], "<i2").view(np.uint8))
        x = dict(variant=-1, jobs=[], bg_node=0)
        blocks = {0: c["src"]}
        if bg:
            x["variant"] = (BG_TAKE, BG_TAKE_OTHER, BG_QUIESCE)[i % 3]
            first = {64: 0, 32: 1, 16: 5, 8: 21, 4: 85}[n]      # (the first node of the depth; TAKE_OTHER posts the search for the node's z-order neighbour)
            x["bg_node"] = c["node"] if x["variant"] != BG_TAKE_OTHER else (first + ((c["node"] - first) ^ 1) if n < 64 else None)
            if x["bg_node"] is None:      # (the 64 x 64 node is alone at its depth)
                x["variant"], x["bg_node"] = BG_TAKE, c["node"]
            if n >= 8:
                kinds = [JOB_SSD, JOB_SYNC] + ([JOB_INTER_TU] if n <= 32 else [])
                x["jobs"] = [int(k) for k in rng.permutation(kinds)[:int(rng.integers(0, len(kinds) + 1))]]
                nc = n // 2
                qp, ad, kind = wc.GRID[(37 * i + n) % len(wc.GRID)]
                x.update(qp=qp, avg_dist=ad, cqo=int(rng.choice([0, 2])), sbh=int(rng.integers(4) != 0))
                x["weight"] = wc.chroma_weight(qp, x["cqo"])
                x["csrc"], x["cpred"] = chroma_blocks(rng, nc, kind)
                x["sync"] = rng.integers(-2000, 2000, (4, nc * nc)).astype("<i2")
                blocks.update(x["csrc"])
                a["qp"], a["chroma_qp_offset"], a["sign_hiding"], a["avg_dist"], a["chroma_weight"] = qp, x["cqo"], x["sbh"], ad, x["weight"]
                if JOB_SSD in x["jobs"] or JOB_INTER_TU in x["jobs"]:
                    a["pred"] = arena.add(wc.window(rng, x["cpred"], c["x"], c["y"]))
                if JOB_SYNC in x["jobs"]:
                    a["sync"] = arena.add(x["sync"].view(np.uint8))
            a["bg_variant"], a["bg_node"] = x["variant"], x["bg_node"]
            a["jobs"] = x["jobs"] + [JOB_NONE] * (4 - len(x["jobs"]))
        a["curr"] = arena.add(wc.window(rng, blocks, c["x"], c["y"]))
        extra.append(x)
    return dict(n=n, bg=bg, cases=cases, extra=extra, arr=arr, arena=arena.bytes())


def job_expected(ora, x, job):
    """HelperBox::r after an ordinary job of a background step"""
    if job == JOB_SSD:
        return [int(((x["csrc"][comp].astype(np.int64) - x["cpred"][comp].astype(np.int64)) ** 2).sum()) for comp in (1, 2)]
    if job == JOB_INTER_TU:
        key = "tu_exp"
        if key not in x:
            x[key] = {comp: wc.eval_block(ora, x["csrc"][comp], x["cpred"][comp], comp, x["qp"], x["cqo"], x["sbh"], x["avg_dist"], x["weight"]) for comp in (1, 2)}
        return [v for comp in (1, 2) for v in (x[key][comp]["dist"], x[key][comp]["sum"] & 0xffffffff, x[key][comp]["raw"])]
    return None


def chroma_scan(nc, mode):
    """find_scan_mode for an intra chroma TU: mode dependent for 4 x 4 only"""
    return (1 if abs(mode - 26) < 5 else (2 if abs(mode - 10) < 5 else 3)) if nc == 4 else 3


def _chroma_setting(rng, nc, i):
    n = 2 * nc
    x, y = POSITIONS[n][i % len(POSITIONS[n])]
    nb = tuple(int(v) for v in ((1, 1, 1, 1), (1, 1, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1), (0, 0, 0, 0), (1, 1, 1, 0), (1, 1, 0, 1))[i % 7])
    clip = (None, (0, 0), (8, 16), (16, 8), (n, n))[i % 5]
    ctu_x, ctu_y, width, height = _picture(rng, x, y, n, clip)
    return dict(nc=nc, node=wc.node_at(x, y, n), x=x, y=y, nb=nb, ctu_x=ctu_x, ctu_y=ctu_y, width=width, height=height,
                nbr={comp: random_walk(rng, 4 * nc + 1, 9) for comp in (1, 2)})


@functools.lru_cache(maxsize=None)
def chroma_search_bundle(nc):
    rng = np.random.default_rng(4100 + nc)
    arena, cases = wc.Arena(), []
    for i in range(42):
        c = _chroma_setting(rng, nc, i)
        luma_mode = i if i < 35 else int(rng.integers(0, 35))
        lst = [0, 26, 10, 1]
        c["cand"] = [34 if m == luma_mode else m for m in lst] + [luma_mode]      # chroma_dir_list with the DM entry resolved, as encode_intra_chroma posts it
        kind = i % wc.KINDS
        c["src"] = {comp: wc.source_block(rng, nc, (kind + 3 * (comp - 1)) % wc.KINDS) for comp in (1, 2)}
        if i % 6 == 5:      # the extremes
            c["src"] = {1: np.zeros((nc, nc), np.uint8), 2: np.full((nc, nc), 255, np.uint8)}
            c["nbr"] = {1: np.full(4 * nc + 1, 255, np.int16), 2: np.zeros(4 * nc + 1, np.int16)}
        cases.append(c)
    arr = np.zeros(len(cases), HELPER_CASE)
    for c, a in zip(cases, arr):
        _fill_common(a, c)
        a["step"], a["cand"] = STEP_CHROMA_SEARCH, c["cand"]
        a["nbr"] = arena.add(np.concatenate([c["nbr"][1], c["nbr"][2]]).astype("<i2").view(np.uint8))
        a["curr"] = arena.add(wc.window(rng, c["src"], c["x"], c["y"]))
    return dict(nc=nc, cases=cases, arr=arr, arena=arena.bytes())


def chroma_search_expected(ora, b):
    if "exp" not in b:
        exp = []
        for c in b["cases"]:
            nc = c["nc"]
            bl, tr = clip_sizes(c, nc, True)
            sads = {}
            for comp in (1, 2):
                plane, adi = plane_around(c["nbr"][comp], nc), np.zeros(4 * nc + 1, np.int16)
                ora.ora_fill_reference_samples(_vp(plane), 2 * nc + 1, nc, *c["nb"], bl, tr, _vp(adi))
                sads[comp] = [sad(ora, c["src"][comp], predict(ora, adi, nc, m, 0)) for m in c["cand"]]
            exp.append(sads)
        b["exp"] = exp
    return b["exp"]


@functools.lru_cache(maxsize=None)
def chroma_tu_bundle(nc):
    """Chroma TUs of size nc: node QP over the whole range, the source a prediction-like block plus noise of several amplitudes (so that level-free and coded blocks
    meet in one TU in every combination), both slice types, with and without sign hiding."""
    rng = np.random.default_rng(5200 + nc)
    arena, cases = wc.Arena(), []
    for i, qp in enumerate(list(range(0, 52)) + [22, 27, 32, 37] * 6):
        c = _chroma_setting(rng, nc, i)
        c.update(qp=qp, cqo=int(rng.choice([0, 2, -3])), sbh=int(rng.integers(3) != 0), slice_type=SLICE_I if i % 3 else SLICE_P, cu_mode=int(rng.integers(0, 35)),
                 cbf_shift=[int(rng.integers(0, 3)), int(rng.integers(0, 3))])
        c["weight"] = wc.chroma_weight(qp, c["cqo"])
        # per plane: flat content close to what the neighbours predict (level-free at most QPs), or busy content (coded)
        busy = {1: (i >> 0) & 1, 2: (i >> 1) & 1}
        c["src"] = {}
        for comp in (1, 2):
            if busy[comp]:
                c["src"][comp] = rng.integers(0, 256, (nc, nc)).astype(np.uint8) if i % 5 else wc.checker(nc, 1, comp & 1)
            else:
                c["nbr"][comp] = np.clip(int(c["nbr"][comp][0]) + rng.integers(-1, 2, 4 * nc + 1), 0, 255).astype(np.int16)
                c["src"][comp] = np.full((nc, nc), int(c["nbr"][comp][0]), np.uint8)
        cases.append(c)
    arr = np.zeros(len(cases), HELPER_CASE)
    for c, a in zip(cases, arr):
        _fill_common(a, c)
        a["step"], a["cu_mode"], a["cbf_shift"] = STEP_CHROMA_TU, c["cu_mode"], c["cbf_shift"]
        a["nbr"] = arena.add(np.concatenate([c["nbr"][1], c["nbr"][2]]).astype("<i2").view(np.uint8))
        a["curr"] = arena.add(wc.window(rng, c["src"], c["x"], c["y"]))
    return dict(nc=nc, cases=cases, arr=arr, arena=arena.bytes())


def chroma_tu_expected(ora, b):
    """ora_intra_tu_chain per plane on a plane of its own (the reconstruction goes back into it, as in the window); the weight applied as chroma_tu_comp applies it"""
    if "exp" not in b:
        exp = []
        ora.ora_intra_tu_chain.restype = C.c_uint32
        for c in b["cases"]:
            nc = c["nc"]
            bl, tr = clip_sizes(c, nc, True)
            per, rem = divmod(wc.chroma_qp(c["qp"], c["cqo"]), 6)
            e = {}
            for comp in (1, 2):
                plane = plane_around(c["nbr"][comp], nc)
                st = 2 * nc + 1
                orig = np.ascontiguousarray(c["src"][comp], np.int16)
                pred, lev, ac = np.zeros((nc, nc), np.int16), np.full(nc * nc, POISON, np.int16), C.c_int(0)
                raw = ora.ora_intra_tu_chain(_vp(orig), nc, _vp(plane), st, *c["nb"], bl, tr, 0, 0, c["cu_mode"], 0, _vp(pred), nc, _vp(lev), _vp(plane, st + 1), st, nc, 0,
                                             chroma_scan(nc, c["cu_mode"]), comp, int(c["slice_type"] == SLICE_I), c["sbh"], per, rem, C.byref(ac))
                e[comp] = dict(pred=pred.astype(np.uint8).ravel(), lv=lev, rec=plane[1:nc + 1, 1:nc + 1].ravel().copy(), dist=int(c["weight"] * int(raw)), sum=int(ac.value),
                               cls="kept" if ac.value else "none")
            # the node's units of Work::cbf_chroma: both bit positions set where the plane has levels
            q = wc.GEO[c["node"]]
            cbf = np.zeros((2, 256), np.uint8)
            for comp in (1, 2):
                if e[comp]["sum"]:
                    cbf[comp - 1, q["abs_index"]:q["abs_index"] + (q["size"] * q["size"] >> 4)] = (1 << c["cbf_shift"][0]) | (1 << c["cbf_shift"][1])
            e["cbf"] = cbf
            exp.append(e)
        b["exp"] = exp
    return b["exp"]


@functools.lru_cache(maxsize=None)
def plane_pair_bundle(nc):
    """SSD_UV and SYNC_UV cases of chroma size nc at the CTU's corners and an interior place: random and extreme content, every window pair of the walk's copies"""
    rng = np.random.default_rng(6300 + nc)
    n = 2 * nc
    arena, cases = wc.Arena(), []
    for i in range(24):
        x, y = POSITIONS[n][i % len(POSITIONS[n])]
        ctu_x, ctu_y, width, height = _picture(rng, x, y, n, None)
        c = dict(nc=nc, node=wc.node_at(x, y, n), x=x, y=y, ctu_x=ctu_x, ctu_y=ctu_y, width=width, height=height)
        if i < 12:
            c["step"] = STEP_SSD_UV
            if i % 6 == 5:
                c["src"] = {0: np.zeros((n, n), np.uint8), 1: np.zeros((nc, nc), np.uint8), 2: np.full((nc, nc), 255, np.uint8)}
                c["pred"] = {0: np.full((n, n), 255, np.uint8), 1: np.full((nc, nc), 255, np.uint8), 2: np.zeros((nc, nc), np.uint8)}
            else:
                c["src"] = {0: rng.integers(0, 256, (n, n)).astype(np.uint8), 1: rng.integers(0, 256, (nc, nc)).astype(np.uint8), 2: rng.integers(0, 256, (nc, nc)).astype(np.uint8)}
                c["pred"] = {k: wc.prediction_block(rng, v, int(rng.integers(1, len(wc.AMPS)))) for k, v in c["src"].items()}
            c["exp"] = [int(((c["src"][k].astype(np.int64) - c["pred"][k].astype(np.int64)) ** 2).sum()) for k in (1, 2, 0)]
        else:
            c["step"] = STEP_SYNC_UV
            src_w, dst_w = int(rng.integers(0, NWND)), int(rng.integers(0, NWND - 1))
            dst_w += dst_w >= src_w
            c["wnd"] = [src_w, dst_w, src_w, dst_w] if i % 2 else [src_w, dst_w, dst_w, src_w]
            c["sync"] = rng.integers(-32768, 32768, (4, nc * nc)).astype("<i2")
        cases.append(c)
    arr = np.zeros(len(cases), HELPER_CASE)
    for c, a in zip(cases, arr):
        _fill_common(a, c)
        a["step"] = c["step"]
        if c["step"] == STEP_SSD_UV:
            a["curr"] = arena.add(wc.window(rng, c["src"], c["x"], c["y"]))
            a["pred"] = arena.add(wc.window(rng, c["pred"], c["x"], c["y"]))
        else:
            a["wnd"] = c["wnd"]
            a["sync"] = arena.add(c["sync"].view(np.uint8))
    return dict(nc=nc, cases=cases, arr=arr, arena=arena.bytes())
