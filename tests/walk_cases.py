"""Cases and expected values for the device-only forms of the CTU walk (include/homer_gpu.h section 16 and hmr_gpu_prim_multi_sad): the merge tiles of enc_quad.h, the
two-halves instantiation of the inter TU chain, the multi-candidate byte SAD.  Nothing here touches the GPU: the cases are numpy arrays in the layouts the entries take, the
expected values come from the CPU oracle alone (ora_predict + ora_inter_tu_chain, the call pattern of test_gpu_batches.py::test_inter_tu_chain_from_source) and from numpy.

The sweep of the merge tiles and of the wave halves is one family per block shape (4 x 4 chroma, 8 x 8 luma, 8 x 8 chroma, 16 x 16 luma): node QP 0 .. 51 x avg_dist
{0, 400, 6000} x seven kinds of content (prediction = clip(source + U[-amp, amp]) for amp 0, 1, 3, 8, 24, 80 on random source bytes, and 0 / 255 checker blocks against
their inverse) = 1092 grid points.  Slot pattern, CU position, sign hiding and chroma QP offset are drawn per grid point instead of multiplying the grid; the blocks that sit
side by side in a tile take different kinds of content, so that coded, dropped and level-free blocks meet in one tile.  tests/test_walk_cases_cpu.py holds the family to the
shares the sweep is meant to have."""
import ctypes as C
import functools

import numpy as np

from kernel_cases import CHROMA_QP

STEP_QUAD8_Y, STEP_QUAD8_C, STEP_QUAD16_Y, STEP_QUAD16_C, STEP_TU, STEP_TU_PAIR = 1, 2, 3, 4, 5, 6
SLICE_P = 1
POISON = 0x1234

WALK_CASE = np.dtype([("step", "<i4"), ("node", "<i4"), ("comp", "<i4"), ("one_slot", "<i4"), ("qp", "<i4"), ("ctu_x", "<i4"), ("ctu_y", "<i4"), ("slice_type", "<i4"),
                      ("sign_hiding", "<i4"), ("chroma_qp_offset", "<i4"), ("stride_y", "<i4"), ("stride_c", "<i4"), ("mv", "<i4", (4, 2)), ("avg_dist", "<f8"),
                      ("chroma_weight", "<f8"), ("sub_y", "<i8"), ("sub_c", "<i8", (2,)), ("curr", "<i8"), ("pred", "<i8")])
WALK_OUT = np.dtype([("dist", "<u4", (4, 3)), ("sum", "<i4", (4, 3)), ("raw", "<u4", (4, 3)), ("cbf", "<u4", (4, 3)), ("stray", "<u4"), ("reserved", "<u4", (15,)),
                     ("pred", "u1", (4, 256)), ("rec", "<i2", (4, 256)), ("lv", "<i2", (4, 256))])
assert WALK_CASE.itemsize == 136 and WALK_OUT.itemsize == 5376
WINDOW_BYTES = 64 * 64 + 2 * 32 * 32

QPS = range(52)
AVG_DISTS = (0.0, 400.0, 6000.0)
AMPS = (0, 1, 3, 8, 24, 80)
KINDS = len(AMPS) + 1                 # the amplitudes, then the checker
GRID = [(qp, ad, j) for qp in QPS for ad in AVG_DISTS for j in range(KINDS)]
SHAPES = {"c4": (8, True), "y8": (8, False), "c8": (16, True), "y16": (16, False)}      # block shape -> (CU size, chroma)
POSITIONS = {8: ((0, 0), (56, 56), (24, 40)), 16: ((0, 0), (48, 48), (16, 32))}        # CU origin in the CTU: both corners and an interior place of another quadrant
SLOT_PATTERNS = {8: (1, 2, 4), 16: (1, 2)}                                             # distinct vectors of a CU (the slots behind them repeat slot 0, as quad_prepare leaves them)


def make_geo():
    """The partition tree as make_geo (enc_host.h) numbers it: breadth first, the four children of a node in z-order."""
    geo = [dict(depth=0, size=64, x=0, y=0, abs_index=0)]
    for p in range(85):
        par = geo[p]
        size = par["size"] // 2
        for k in range(4):
            geo.append(dict(depth=par["depth"] + 1, size=size, x=par["x"] + (k & 1) * size, y=par["y"] + (k >> 1) * size, abs_index=par["abs_index"] + k * (size * size >> 4)))
    return geo


GEO = make_geo()


def node_at(x, y, size):
    return next(i for i, q in enumerate(GEO) if (q["x"], q["y"], q["size"]) == (x, y, size))


def chroma_qp(qp, offset):
    return CHROMA_QP[min(max(qp + offset, 0), 57)]


def chroma_weight(qp, offset):
    return 2.0 ** ((qp - chroma_qp(qp, offset)) / 3.0)


def checker(n, cell, phase):
    yy, xx = np.mgrid[0:n, 0:n]
    return (255 * (((yy // cell + xx // cell + phase) & 1))).astype(np.uint8)


def source_block(rng, n, kind):
    return checker(n, int(rng.choice([1, 2, 4])), int(rng.integers(2))) if kind == KINDS - 1 else rng.integers(0, 256, (n, n)).astype(np.uint8)


def prediction_block(rng, src, kind):
    if kind == KINDS - 1:
        return np.where(src >= 128, 0, 255).astype(np.uint8)      # (a checker source: its inverse)
    amp = AMPS[kind]
    return np.clip(src.astype(np.int32) + rng.integers(-amp, amp + 1, src.shape), 0, 255).astype(np.uint8)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def eval_block(ora, src, pred, comp, qp, cqo, sbh, avg_dist, weight_c, slice_is_intra=0):
    """What the inter TU chain leaves for one block, from the oracle alone; and how the block counts in the sweep's shares."""
    n = src.shape[0]
    s16, p16 = np.ascontiguousarray(src, np.int16), np.ascontiguousarray(pred, np.int16)
    res = np.zeros((n, n), np.int16)
    ora.ora_predict(_vp(s16), n, _vp(p16), n, _vp(res), n, n)
    qpc = qp if comp == 0 else chroma_qp(qp, cqo)
    per, rem = divmod(qpc, 6)
    weight = 1.0 if comp == 0 else weight_c
    thr = min(max(avg_dist / 2.5 - 5.0, 1.0), 20000.0)
    lev, rec, ac = np.full(n * n, POISON, np.int16), np.full((n, n), POISON, np.int16), C.c_int(0)
    ora.ora_inter_tu_chain.restype = C.c_uint32
    dist = ora.ora_inter_tu_chain(_vp(res), n, _vp(p16), n, _vp(lev), _vp(rec), n, n, 3, comp, slice_is_intra, sbh, per, rem, C.c_double(weight), C.c_double(thr), C.byref(ac))
    raw = int(((src.astype(np.int64) - pred.astype(np.int64)) ** 2).sum())
    # the classes of the sweep: the levels before the keep-or-drop test, with and without sign hiding
    depth = 6 - (n.bit_length() - 1) - (comp != 0)
    coef, q1, q0, s1, s0 = np.zeros(n * n, np.int16), np.zeros(n * n, np.int16), np.zeros(n * n, np.int16), C.c_int(0), C.c_int(0)
    ora.ora_transform(_vp(res), _vp(coef), n, n, 0)
    ora.ora_quant(_vp(coef), _vp(q1), None, 3, depth, comp, 0, slice_is_intra, sbh, C.byref(s1), n, per, rem)
    changed = False
    if sbh:
        ora.ora_quant(_vp(coef), _vp(q0), None, 3, depth, comp, 0, slice_is_intra, 0, C.byref(s0), n, per, rem)
        changed = not np.array_equal(q0, q1)
    cls = "none" if s1.value == 0 else ("dropped" if ac.value == 0 else "kept")
    return dict(lv=lev, rec=rec.ravel().copy(), dist=int(dist), sum=int(ac.value), raw=raw, cbf=int(ac.value != 0), cls=cls, sbh_changed=changed,
                max_level=int(np.abs(q1.astype(np.int32)).max()))


class Arena:
    """Bytes of one call, in pieces that start at multiples of 4."""

    def __init__(self):
        self.pieces, self.size = [], 0

    def add(self, a):
        a = np.ascontiguousarray(a, np.uint8).ravel()
        off = self.size
        pad = -a.size & 3
        self.pieces.append(a if not pad else np.concatenate([a, np.zeros(pad, np.uint8)]))
        self.size += a.size + pad
        return off

    def bytes(self):
        return np.concatenate(self.pieces)


def window(rng, blocks, x, y):
    """A worker's window image (64 x 64 luma at pitch 64, then U and V, 32 x 32 at pitch 32) of random bytes with `blocks` {comp: block} at the CU at (x, y)."""
    w = rng.integers(0, 256, WINDOW_BYTES).astype(np.uint8)
    for comp, b in blocks.items():
        n = b.shape[0]
        if comp == 0:
            w[:4096].reshape(64, 64)[y:y + n, x:x + n] = b
        else:
            w[4096 + (comp - 1) * 1024:4096 + comp * 1024].reshape(32, 32)[y // 2:y // 2 + n, x // 2:x // 2 + n] = b
    return w


def plane_block(arena, case, slot, comp):
    """The n x n prediction bytes of a slot at the address of include/homer_gpu.h section 13, from the arena's bytes (the planes are just bytes to the tiles)."""
    q = GEO[case["node"]]
    mx, my = case["mvs"][slot]
    if comp == 0:
        n, s = q["size"], case["stride_y"]
        base = case["sub_y"] + ((my & 3) * 4 + (mx & 3)) * s + (case["ctu_y"] + q["y"] + (my >> 2)) * 16 * s + case["ctu_x"] + q["x"] + (mx >> 2)
        pitch = 16 * s
    else:
        n, s = q["size"] // 2, case["stride_c"]
        base = case["sub_c"][comp - 1] + ((my & 7) * 8 + (mx & 7)) * s + ((case["ctu_y"] >> 1) + q["y"] // 2 + (my >> 3)) * 64 * s + (case["ctu_x"] >> 1) + q["x"] // 2 + (mx >> 3)
        pitch = 64 * s
    idx = base + pitch * np.arange(n)[:, None] + np.arange(n)[None, :]
    assert idx.min() >= 0 and idx.max() < arena.size
    return arena[idx]


def _region(rng, n, chroma, stride, ctu_x, ctu_y, q, mvs, preds):
    """The stretch of the row-interleaved phase planes a CU's slots can reach (integer displacements -4 .. 3 luma, -2 .. 1 chroma), random bytes, with the slots'
    prediction blocks written where their vectors point (preds: per slot an n x n block, or None: the plane's own bytes).  Returns the bytes and where plane 0's
    first valid sample lies relative to them (negative: the picture starts before the stretch)."""
    phases, margin, sh, mask = (64, 2, 3, 7) if chroma else (16, 4, 2, 3)
    rows = n + 2 * margin
    assert stride >= n + 2 * margin
    reg = rng.integers(0, 256, rows * phases * stride).astype(np.uint8)
    for (mx, my), p in zip(mvs, preds):
        if p is None:
            continue
        f = (my & mask) * (mask + 1) + (mx & mask)
        ly, lx = margin + (my >> sh), margin + (mx >> sh)
        for r in range(n):
            o = ((ly + r) * phases + f) * stride + lx
            reg[o:o + n] = p[r]
    gx, gy = ((ctu_x >> 1) + q["x"] // 2, (ctu_y >> 1) + q["y"] // 2) if chroma else (ctu_x + q["x"], ctu_y + q["y"])
    origin = margin * phases * stride + margin - gy * phases * stride - gx
    return reg, origin


@functools.lru_cache(maxsize=None)
def quad_bundle(shape):
    """The merge-tile cases of one block shape: the CU descriptions (`cus`), the device cases (`arr`: the tile steps, then the sequential WaveGrp TU of every distinct
    slot and component) and the arena they address."""
    cu, chroma = SHAPES[shape]
    n = cu // 2 if chroma else cu
    comps = (1, 2) if chroma else (0,)
    rng = np.random.default_rng(20240 + 7 * cu + chroma)
    arena, cus = Arena(), []
    # the sweep, then a group with equal phases and overlapping blocks on the planes' own random content
    plan = [(qp, ad, j, False) for qp, ad, j in GRID] + [(qp, 400.0, int(rng.integers(len(AMPS))), True) for qp in QPS]
    strides_y, strides_c = ((24, 27, 29), (12, 13, 15)) if cu == 8 else ((32, 35, 37), (16, 17, 19))
    for qp, ad, j, overlap in plan:
        k = int(rng.choice(SLOT_PATTERNS[cu])) if not overlap else SLOT_PATTERNS[cu][-1]
        x, y = POSITIONS[cu][int(rng.integers(3))]
        node = node_at(x, y, cu)
        q = GEO[node]
        sbh, cqo = int(rng.integers(8) != 0), int(rng.choice([0, 2]))
        ctu_x, ctu_y = 64 * int(rng.integers(0, 30)), 64 * int(rng.integers(0, 17))
        stride_y, stride_c = int(rng.choice(strides_y)), int(rng.choice(strides_c))
        if overlap:
            # one eighth-sample phase for all slots (so the quarter-sample phase is shared too), distinct integer parts less than a block apart
            ph = rng.integers(0, 8, 2)
            ints = rng.permutation(16)[:k]
            mvs = [(int((i % 4 - 2) * 8 + ph[0]), int((i // 4 - 2) * 8 + ph[1])) for i in ints]
        else:
            # distinct quarter-sample phases (hence distinct planes, luma and chroma): the slots' blocks cannot overlap
            phs = rng.permutation(16)[:k]
            mvs = [(int(rng.integers(-4, 4)) * 4 + int(p % 4), int(rng.integers(-4, 4)) * 4 + int(p // 4)) for p in phs]
        mvs += [mvs[0]] * (4 - k)
        src, preds = {}, {}
        for ci, comp in enumerate(comps):
            jc = (j + 3 * ci) % KINDS
            src[comp] = source_block(rng, n, jc)
            for s in range(k):
                preds[s, comp] = None if overlap else prediction_block(rng, src[comp], (jc + 2 * s) % KINDS)
        c = dict(shape=shape, cu=cu, chroma=chroma, n=n, comps=comps, node=node, x=x, y=y, qp=qp, avg_dist=ad, kind=j, overlap=overlap, k=k, sbh=sbh, cqo=cqo,
                 weight=chroma_weight(qp, cqo), ctu_x=ctu_x, ctu_y=ctu_y, stride_y=stride_y, stride_c=stride_c, mvs=mvs, sub_y=0, sub_c=[0, 0], made=preds)
        for comp in comps:
            reg, origin = _region(rng, n, chroma, stride_c if chroma else stride_y, ctu_x, ctu_y, q, mvs[:k], [preds[s, comp] for s in range(k)])
            at = arena.add(reg) + origin
            if comp == 0:
                c["sub_y"] = at
            else:
                c["sub_c"][comp - 1] = at
            if overlap:      # the source follows the plane's bytes at slot 0: the other slots' blocks overlap it and differ from it as random bytes do
                m, ph_n, sh, mask = (2, 64, 3, 7) if chroma else (4, 16, 2, 3)
                mx, my = mvs[0]
                stride = stride_c if chroma else stride_y
                rows = np.array([reg[((m + (my >> sh) + r) * ph_n + (my & mask) * (mask + 1) + (mx & mask)) * stride + m + (mx >> sh):][:n] for r in range(n)])
                src[comp] = prediction_block(rng, rows, j)
        c["src"] = src
        c["curr"] = arena.add(window(rng, src, x, y))
        cus.append(c)
    bytes_ = None
    # the device cases: the tile step(s) of every CU ...
    recs = []
    for ci, c in enumerate(cus):
        step = {"c4": STEP_QUAD8_C, "y8": STEP_QUAD8_Y, "c8": STEP_QUAD16_C, "y16": STEP_QUAD16_Y}[shape]
        for one_slot in ((0, 1) if shape == "y16" else (0,)):
            recs.append((ci, "quad", one_slot, 0, step, -1))
    # ... then the sequential chain on the same data: the slot's prediction in the prediction window (its bytes as the planes hold them), one call per component
    bytes_ = arena.bytes()
    extra = Arena()
    extra.size = bytes_.size
    for ci, c in enumerate(cus):
        c["pred"] = {(s, comp): plane_block(bytes_, c, s, comp) for s in range(c["k"]) for comp in comps}
        for s in range(c["k"]):
            at = extra.add(window(rng, {comp: c["pred"][s, comp] for comp in comps}, c["x"], c["y"]))
            for comp in comps:
                recs.append((ci, "tu", s, comp, STEP_TU, at))
    bytes_ = np.concatenate([bytes_] + extra.pieces)
    arr = np.zeros(len(recs), WALK_CASE)
    for i, (ci, _, s, comp, step, pred_at) in enumerate(recs):
        c = cus[ci]
        a = arr[i]
        a["step"], a["node"], a["comp"], a["one_slot"] = step, c["node"], comp, s if step != STEP_TU else 0
        a["qp"], a["ctu_x"], a["ctu_y"], a["slice_type"] = c["qp"], c["ctu_x"], c["ctu_y"], SLICE_P
        a["sign_hiding"], a["chroma_qp_offset"], a["stride_y"], a["stride_c"] = c["sbh"], c["cqo"], c["stride_y"], c["stride_c"]
        a["mv"] = c["mvs"]
        a["avg_dist"], a["chroma_weight"] = c["avg_dist"], c["weight"]
        a["sub_y"], a["sub_c"], a["curr"], a["pred"] = c["sub_y"], c["sub_c"], c["curr"], pred_at
    return dict(shape=shape, cus=cus, recs=recs, arr=arr, arena=bytes_)


def quad_expected(ora, bundle):
    """Per CU, distinct slot and component: eval_block on the source block and the slot's prediction (computed once per bundle)."""
    if "exp" not in bundle:
        bundle["exp"] = [{(s, comp): eval_block(ora, c["src"][comp], c["pred"][s, comp], comp, c["qp"], c["cqo"], c["sbh"], c["avg_dist"], c["weight"])
                          for s in range(c["k"]) for comp in c["comps"]} for c in bundle["cus"]]
    return bundle["exp"]


@functools.lru_cache(maxsize=None)
def pair_bundle(n):
    """The wave-half cases of chroma block size n (4: an 8 x 8 CU, 8: a 16 x 16 CU): per grid point the U and the V block of one TU with different kinds of content;
    the device cases are the two-halves step and the two sequential WaveGrp calls on the same windows."""
    cu = 2 * n
    rng = np.random.default_rng(515 + n)
    arena, tus, recs = Arena(), [], []
    for qp, ad, j in GRID:
        x, y = POSITIONS[cu][int(rng.integers(3))]
        sbh, cqo = int(rng.integers(8) != 0), int(rng.choice([0, 2]))
        src = {comp: source_block(rng, n, (j + 3 * (comp - 1)) % KINDS) for comp in (1, 2)}
        pred = {comp: prediction_block(rng, src[comp], (j + 3 * (comp - 1)) % KINDS) for comp in (1, 2)}
        t = dict(n=n, node=node_at(x, y, cu), x=x, y=y, qp=qp, avg_dist=ad, kind=j, sbh=sbh, cqo=cqo, weight=chroma_weight(qp, cqo), src=src, pred=pred,
                 curr=arena.add(window(rng, src, x, y)), pred_at=arena.add(window(rng, pred, x, y)))
        ti = len(tus)
        tus.append(t)
        recs += [(ti, STEP_TU_PAIR, 0), (ti, STEP_TU, 1), (ti, STEP_TU, 2)]
    arr = np.zeros(len(recs), WALK_CASE)
    for i, (ti, step, comp) in enumerate(recs):
        t, a = tus[ti], arr[i]
        a["step"], a["node"], a["comp"], a["qp"], a["slice_type"] = step, t["node"], comp, t["qp"], SLICE_P
        a["sign_hiding"], a["chroma_qp_offset"], a["stride_y"], a["stride_c"] = t["sbh"], t["cqo"], 64, 32
        a["avg_dist"], a["chroma_weight"], a["curr"], a["pred"] = t["avg_dist"], t["weight"], t["curr"], t["pred_at"]
    return dict(n=n, tus=tus, recs=recs, arr=arr, arena=arena.bytes())


def pair_expected(ora, bundle):
    if "exp" not in bundle:
        bundle["exp"] = [{comp: eval_block(ora, t["src"][comp], t["pred"][comp], comp, t["qp"], t["cqo"], t["sbh"], t["avg_dist"], t["weight"]) for comp in (1, 2)}
                         for t in bundle["tus"]]
    return bundle["exp"]


PAIR_COMBINATIONS = ("u_only", "v_only", "both", "neither", "one_dropped_other_kept")


def pair_combination(eu, ev):
    """Which of the combinations the wave-half list has to contain a TU is (cls: none / dropped / kept, eval_block)."""
    out = []
    cu, cv = eu["cls"], ev["cls"]
    if cu == "kept" and cv == "none":
        out.append("u_only")
    if cv == "kept" and cu == "none":
        out.append("v_only")
    if cu == "kept" and cv == "kept":
        out.append("both")
    if cu == "none" and cv == "none":
        out.append("neither")
    if {cu, cv} == {"dropped", "kept"}:
        out.append("one_dropped_other_kept")
    return out


# ---- the multi-candidate byte SAD ------------------------------------------------------------------------------------------------------------------------------
SAD_MAXC = (4, 8, 9)
SAD_SIZES = (8, 16, 32, 64)


@functools.lru_cache(maxsize=None)
def sad_case(maxc, n, extreme=False):
    """One call of hmr_gpu_prim_multi_sad: a source block at pitch 64, a plane with an odd row pitch, lists of candidate offsets (-1: skipped) - every candidate
    position at every byte alignment, nobody skipped, every position skipped alone, every position present alone (maxc 9: the ninth with and without the others) -
    and every expected sum (0 for a skipped candidate).  extreme: an all-0 block against an all-255 plane."""
    rng = np.random.default_rng(99 + 16 * maxc + n + 1000 * extreme)
    stride, rows = 2 * n + 13, n + 5
    src = np.zeros((n, 64), np.uint8)
    src[:, :n] = 0 if extreme else rng.integers(0, 256, (n, n))
    plane = np.full(stride * rows, 255, np.uint8) if extreme else rng.integers(0, 256, stride * rows).astype(np.uint8)

    def offsets(shift):      # candidate k: a row displacement of its own, a column displacement that puts it at byte alignment (k + shift) % 4 of the plane's start
        return [int((k % 5) * stride + 4 * ((k // 4) % 3) + (k + shift) % 4) for k in range(maxc)]
    lists = [offsets(sh) for sh in range(4)]
    for k in range(maxc):
        lists.append([-1 if i == k else o for i, o in enumerate(offsets(k))])
        lists.append([o if i == k else -1 for i, o in enumerate(offsets(k + 1))])
    lists.append([-1] * maxc)
    off = np.array(lists, np.int64)
    exp = np.zeros(off.shape, np.uint32)
    idx = stride * np.arange(n)[:, None] + np.arange(n)[None, :]
    for i, j in np.argwhere(off >= 0):
        exp[i, j] = np.abs(src[:, :n].astype(np.int64) - plane[off[i, j] + idx].astype(np.int64)).sum()
    assert (off[off >= 0] + (n - 1) * stride + n <= plane.size).all()
    return dict(maxc=maxc, n=n, stride=stride, src=src, plane=plane, off=off, exp=exp)
