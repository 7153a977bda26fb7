"""Cases and expected values for the post-decision stage run on given CTU records (include/homer_gpu.h section 17: hmr_gpu_enc_post_records, and its one-lane twin
henc_cpu_post_records in oracle/enc_cpu.cpp).  Nothing here touches the GPU.

A case is (configuration, picture size, slice type, QP, records, source).  Records start from valid ones - the reference fixture tests/golden/ctus_200x136.npz, or the
checker's own encode of tools/gen_yuv.py content - so that trees, modes and merge flags are what the syntax expects, and are then mutated in ways that keep the syntax
valid: level VALUES at the non-zero positions, motion vector differences of non-merge inter units, motion vectors and reference indices (which only the boundary strength
reads), unit QPs, and the whole reconstruction and source (seeded pictures made to sit on the deblocking filter's thresholds and to make each SAO type pay).

Expected values come from two places, neither of them the device:
  * the ORACLE chain (oracle/hmr_oracle.c, pinned to the reference function by function): ora_units_from_ctus + ora_make_edge_flags -> unit arrays;
    ora_deblock_frame -> deblocked picture; ora_sao_stats_frame + ora_sao_offsets_ctu -> the candidates a decided SAO_NEW parameter set must come from;
    ora_sao_apply_frame with the decided parameters + ora_pad_plane -> the final picture with its margins; ora_mc_luma / ora_mc_chroma over that -> phase planes;
  * the CHECKER (the one-lane build of the same enc_post.h / enc_entropy.h, whose streams the CPU suite holds byte-identical to the compiled reference's): sub-stream
    bytes, contexts, cumbits and the SAO decision.
tests/test_post_cases_cpu.py holds checker and oracle chain together on every case and counts what the sweep reaches; tests/test_gpu_post_tasks.py holds the device to both."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

import encoder_cases as ec
import libs
from kernel_cases import CHROMA_QP

SEED = int(os.environ.get("HOMER_TEST_SEED", "0"))
POISON = 0x5a
POISON16 = 0x5a5a
SLICE_P, SLICE_I = 1, 2
PM_INTRA = 1
SAO_OFF, SAO_NEW, SAO_MERGE, SAO_BO = 0, 1, 2, 4
CTX_BYTES = 179 + 5
VP = C.c_void_p

REC_DTYPE = np.dtype([("hdr", "<i4", (8,)), ("cbf", "u1", (3, 256)), ("intra_mode", "u1", (2, 256)), ("inter_mode", "u1", (256,)), ("tr_idx", "u1", (256,)),
                      ("pred_depth", "u1", (256,)), ("part_size_type", "u1", (256,)), ("pred_mode", "u1", (256,)), ("skipped", "u1", (256,)), ("merge", "u1", (256,)),
                      ("merge_idx", "u1", (256,)), ("qp", "u1", (256,)), ("mv_ref_idx", "i1", (256,)), ("mv_diff_ref_idx", "u1", (256,)), ("mv_ref", "<i4", (256, 2)),
                      ("mv_diff", "<i4", (256, 2)), ("coeff", "<i2", (6144,)), ("recon", "<i2", (6144,)), ("mode_buffs", "u1", (2560,))])
assert REC_DTYPE.itemsize == ec.REC

TC_TABLE = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24], np.int64)        # (HEVC table 8-12)
BETA_TABLE = np.array([0] * 16 + list(range(6, 19)) + list(range(20, 66, 2)), np.int64)
assert TC_TABLE.size == 54 and BETA_TABLE.size == 52


class PostOut(C.Structure):
    """hmr_gpu_post_out"""
    _fields_ = [("plane_elems", C.c_int64 * 3), ("units", C.c_int64), ("phase_bytes", C.c_int64 * 3), ("nctu", C.c_int32), ("rows", C.c_int32), ("row_cap", C.c_int32),
                ("ctx_bytes", C.c_int32), ("stride_y", C.c_int32), ("stride_c", C.c_int32), ("margin_y", C.c_int32), ("margin_c", C.c_int32), ("units_stride", C.c_int32),
                ("reserved", C.c_int32), ("dbk", VP * 3), ("fin", VP * 3), ("mvx", VP), ("mvy", VP), ("ref", VP), ("uqp", VP), ("flags", VP), ("sao_recon", VP),
                ("sao_coded", VP), ("bs", VP), ("bytecnt", VP), ("cumbits", VP), ("ctx", VP), ("saved", VP), ("errors", VP), ("planes", VP * 3)]


def alloc_out(o, with_planes):
    """numpy arrays behind the pointers of a PostOut whose sizes are filled in; returns them by name (the struct keeps pointing at them: keep the dict alive)"""
    a = {}
    for c in range(3):
        rows, stride = o.plane_elems[c] // (o.stride_c if c else o.stride_y), (o.stride_c if c else o.stride_y)
        a[f"dbk{c}"] = np.zeros((rows, stride), np.int16)
        a[f"fin{c}"] = np.zeros((rows, stride), np.int16)
        o.dbk[c], o.fin[c] = a[f"dbk{c}"].ctypes.data, a[f"fin{c}"].ctypes.data
        if with_planes:
            phases = 64 if c else 16
            a[f"planes{c}"] = np.zeros((rows, phases, stride), np.uint8)
            assert a[f"planes{c}"].nbytes == o.phase_bytes[c]
            o.planes[c] = a[f"planes{c}"].ctypes.data
    urows = o.units // o.units_stride
    for name, dt in (("mvx", np.int16), ("mvy", np.int16), ("ref", np.int8), ("uqp", np.uint8), ("flags", np.uint8)):
        a[name] = np.zeros((urows, o.units_stride), dt)
    a["sao_recon"], a["sao_coded"] = np.zeros((o.nctu, 3, 35), np.int32), np.zeros((o.nctu, 3, 35), np.int32)
    a["bs"] = np.zeros((o.rows, o.row_cap), np.uint8)
    a["bytecnt"], a["cumbits"] = np.zeros(o.rows, np.int32), np.zeros(o.nctu, np.uint32)
    a["ctx"], a["saved"] = np.zeros((o.rows, o.ctx_bytes), np.uint8), np.zeros((o.rows, o.ctx_bytes), np.uint8)
    a["errors"] = np.zeros(4, np.int32)
    for name in ("mvx", "mvy", "ref", "uqp", "flags", "sao_recon", "sao_coded", "bs", "bytecnt", "cumbits", "ctx", "saved", "errors"):
        setattr(o, name, a[name].ctypes.data)
    return a


POST_ARGS = [VP, C.c_int, C.c_int, VP, C.c_size_t, VP, VP, VP, C.c_int, C.c_int, C.POINTER(PostOut)]


@functools.lru_cache(None)
def load_cpu():
    so = os.path.join(libs.ORACLE_DIR, "libenc_cpu.so")
    subprocess.check_call(["make", "-s", "-C", libs.ORACLE_DIR, so])
    lib = C.CDLL(so)
    lib.henc_cpu_create.restype = VP
    lib.henc_cpu_create.argtypes = [C.POINTER(ec.EncCfg)]
    lib.henc_cpu_destroy.argtypes = [VP]
    lib.henc_cpu_records.restype = C.POINTER(C.c_uint8)
    lib.henc_cpu_records.argtypes = [VP]
    lib.henc_cpu_encode_frame.restype = C.c_long
    lib.henc_cpu_encode_frame.argtypes = [VP, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, VP, C.c_long, VP]
    lib.henc_cpu_post_sizes.argtypes = [VP, C.POINTER(PostOut)]
    lib.henc_cpu_post_records.argtypes = POST_ARGS
    lib.henc_cpu_post_counters.restype = C.POINTER(C.c_long * 16)
    assert lib.henc_cpu_record_bytes() == ec.REC
    return lib


def make_cfg(case):
    w, h = case["size"]
    return ec.default_cfg(w, h, qp=case["cfg_qp"], cqo=case["cqo"], sao=case["sao"], sign_hiding=case["sbh"], wpp=case["threads"], wfpp_enable=case["wpp"], **case["rc"])


def run_checker(case):
    """henc_cpu_post_records on the case; returns (status, outputs by name, the coder's counters for this run)"""
    lib = load_cpu()
    cfg = make_cfg(case)
    h = lib.henc_cpu_create(C.byref(cfg))
    assert h, case["name"]
    o = PostOut()
    assert lib.henc_cpu_post_sizes(h, C.byref(o)) == 0
    a = alloc_out(o, False)
    cnt = lib.henc_cpu_post_counters().contents
    before = list(cnt)
    rec, src = case["records"], case["src"]
    rc = lib.henc_cpu_post_records(h, case["slice"], case["qp"], rec.ctypes.data, rec.nbytes, src[0].ctypes.data, src[1].ctypes.data, src[2].ctypes.data, 1, 0, C.byref(o))
    counters = [int(x) - b for x, b in zip(cnt, before)]
    lib.henc_cpu_destroy(h)
    a["geom"] = dict(stride=(o.stride_y, o.stride_c), margin=(o.margin_y, o.margin_c), units_stride=o.units_stride, row_cap=o.row_cap)
    return rc, a, counters


# ---- base records ---------------------------------------------------------------------------------------------------------------------------------------

def grid(size):
    return (size[0] + 63) // 64, (size[1] + 63) // 64


@functools.lru_cache(None)
def checker_records(size, content, frame, rc_items=()):
    """records of frame `frame` (0: I, 1: P) of the checker's own encode of gen_yuv content at this size; with rate control when rc_items says so"""
    lib = load_cpu()
    w, h = size
    cfg = ec.default_cfg(w, h, **dict(rc_items))
    enc = lib.henc_cpu_create(C.byref(cfg))
    assert enc, (size, rc_items)
    nctu = grid(size)[0] * grid(size)[1]
    stream = C.create_string_buffer(8 << 20)
    out = None
    for f, planes in enumerate(ec.clip_frames(w, h, frame + 1, seed=1234 + SEED, content=content)):
        n = lib.henc_cpu_encode_frame(enc, *planes, 0, stream, len(stream), None)
        assert n > 0, (size, content, f, n)
        out = C.string_at(lib.henc_cpu_records(enc), ec.REC * nctu)
    lib.henc_cpu_destroy(enc)
    return ec.crop_recon(out, w, h, grid(size)[0])


@functools.lru_cache(None)
def fixture_records(frame):
    fx = ec.load_fixture("ctus_200x136")
    return ec.crop_recon(fx[f"f{frame}_records"].tobytes(), 200, 136, 4), fx[f"f{frame}_recon"].copy()


def as_records(raw):
    return np.frombuffer(bytearray(raw), REC_DTYPE).copy()


# ---- pictures of a record set ------------------------------------------------------------------------------------------------------------------------------

def recon_planes(recs, size):
    """the records' reconstruction as three tight planes (int16), cropped to the picture"""
    w, h = size
    nx, ny = grid(size)
    y = recs["recon"][:, :4096].reshape(ny, nx, 64, 64).transpose(0, 2, 1, 3).reshape(ny * 64, nx * 64)[:h, :w]
    u = recs["recon"][:, 4096:5120].reshape(ny, nx, 32, 32).transpose(0, 2, 1, 3).reshape(ny * 32, nx * 32)[:h // 2, :w // 2]
    v = recs["recon"][:, 5120:].reshape(ny, nx, 32, 32).transpose(0, 2, 1, 3).reshape(ny * 32, nx * 32)[:h // 2, :w // 2]
    return [np.ascontiguousarray(p) for p in (y, u, v)]


def set_recon(recs, size, planes):
    w, h = size
    nx, ny = grid(size)
    for k, (n, lo) in enumerate(((64, 0), (32, 4096), (32, 5120))):
        full = np.zeros((ny * n, nx * n), np.int16)
        full[:planes[k].shape[0], :planes[k].shape[1]] = planes[k]
        recs["recon"][:, lo:lo + n * n] = full.reshape(ny, n, nx, n).transpose(0, 2, 1, 3).reshape(ny * nx, n * n)


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------------------------

LEVEL_CLASSES = ("ones", "small", "geometric", "extreme")


def mutate_levels(rng, recs, bias):
    """new values at the non-zero positions (cbf, last position and coded_sub_block_flag stay what they are); a class per CTU, `bias` the case's favourite"""
    for r in recs:
        nz = np.flatnonzero(r["coeff"])
        if not nz.size:
            continue
        cls = bias if rng.random() < 0.6 else LEVEL_CLASSES[int(rng.integers(4))]
        if cls == "ones":
            mag = np.ones(nz.size, np.int64)
        elif cls == "small":
            mag = rng.integers(1, 4, nz.size)
        elif cls == "geometric":
            mag = np.minimum(rng.geometric(0.03, nz.size), 600)
        else:
            mag = rng.choice([1, 2, 3, 7, 40, 255, 1000, 16384, 20000, 32767], nz.size)
        val = mag * rng.choice([-1, 1], nz.size)
        if cls == "extreme":
            val[rng.random(nz.size) < 0.05] = -32768
        r["coeff"][nz] = val.astype(np.int16)


def mutate_mvd(rng, recs):
    inter = (recs["pred_mode"] != PM_INTRA) & (recs["merge"] == 0) & (recs["skipped"] == 0)
    n = int(inter.sum())
    pick = rng.integers(0, 9, (n, 2))
    small = rng.integers(-70, 71, (n, 2))
    table = np.array([0, 1, -1, 2, -2, 0, 0, 32767, -32767])
    val = np.where(pick == 5, small, np.where(pick == 6, -small, table[pick]))
    recs["mv_diff"][inter] = val.astype(np.int32)


def mutate_mv_ref(rng, recs, with_missing_ref):
    """vectors of inter units: a base per CTU, and per unit 0, 3, 4 or 5 quarter samples more or less per component - both sides of the boundary-strength threshold
    at every edge; with_missing_ref: some inter units lose their reference index (the `ref_idx < 0` side of get_bs)"""
    inter = recs["pred_mode"] != PM_INTRA
    base = rng.integers(-60, 61, (len(recs), 1, 2))
    d = rng.choice([0, 3, 4, 5], (len(recs), 256, 2)) * rng.choice([-1, 1], (len(recs), 256, 2))
    recs["mv_ref"][inter] = (base + d)[inter].astype(np.int32)
    if with_missing_ref:
        drop = inter & (rng.random(inter.shape) < 0.08)
        recs["mv_ref_idx"][drop] = -1


def thresholds(qp):
    """step heights that sit on the luma filter's decisions at this QP (bs 1 and 2)"""
    out = {0, 1, 2}
    beta = int(BETA_TABLE[min(max(qp, 0), 51)])
    for bs in (1, 2):
        tc = int(TC_TABLE[min(max(qp + 2 * (bs - 1), 0), 53)])
        for t in (beta, beta >> 2, beta >> 3, (5 * tc + 1) >> 1, 10 * tc, 2 * tc, (16 * tc + 8) // 9, (160 * tc + 8) // 9):
            out.update((max(t - 1, 0), t, t + 1))
    return np.array(sorted(out))


def walk(rng, n, steps, lo, hi):
    v = np.zeros(n, np.int64)
    v[0] = rng.integers(lo, hi + 1)
    for i in range(1, n):
        s = int(rng.choice(steps)) * int(rng.choice([-1, 1]))
        if not lo <= v[i - 1] + s <= hi:
            s = -s
        v[i] = min(max(v[i - 1] + s, lo), hi)
    return v


def plane_steps(rng, h, w, blk, qp):
    """flat blk x blk blocks whose differences across vertical and horizontal edges are drawn around the filter's thresholds; kinks next to some edges so that one side
    alone fails its smoothness test (dp / dq pick fp / fq separately)"""
    nb_y, nb_x = (h + blk - 1) // blk, (w + blk - 1) // blk
    steps = thresholds(qp)
    lo, hi = (0, 255) if rng.random() < 0.3 else (24, 231)
    vals = walk(rng, nb_y, steps, lo, hi)[:, None] + walk(rng, nb_x, steps, lo, hi)[None, :] - (lo + hi) // 2 + rng.integers(-1, 2, (nb_y, nb_x))
    p = np.kron(np.clip(vals, 0, 255), np.ones((blk, blk), np.int64))
    if blk >= 8:
        for by in range(nb_y):
            for bx in range(nb_x):
                k = rng.integers(0, 5)       # 0, 1: none; 2: the p side of the edge behind the block; 3: the q side of the edge before it; 4: both
                amp = int(rng.integers(1, 4))
                horiz = rng.random() < 0.5
                blkv = p[by * blk:(by + 1) * blk, bx * blk:(bx + 1) * blk]
                if k in (2, 4):
                    (blkv[:, blk - 2:blk - 1] if horiz else blkv[blk - 2:blk - 1, :]).__iadd__(amp)
                if k in (3, 4):
                    (blkv[:, 1:2] if horiz else blkv[1:2, :]).__iadd__(amp)
    return np.clip(p[:h, :w], 0, 255).astype(np.int16)


def plane_clips(rng, h, w, blk):
    """blocks at and next to 0 and 255, and steep ramps that start there: the filters' and the offsets' clips to the sample range"""
    nb_y, nb_x = (h + blk - 1) // blk, (w + blk - 1) // blk
    flat = rng.choice([0, 0, 1, 2, 3, 252, 253, 254, 255, 255, 8, 247, 16, 30, 225, 239], (nb_y, nb_x))
    p = np.kron(flat, np.ones((blk, blk), np.int64))
    ramp = rng.random((nb_y, nb_x)) < 0.3
    slope = rng.integers(1, 30, (nb_y, nb_x))
    xx = np.tile(np.arange(blk), (blk, 1))
    for by, bx in zip(*np.nonzero(ramp)):
        r = xx * slope[by, bx] if rng.random() < 0.5 else xx.T * slope[by, bx]
        p[by * blk:(by + 1) * blk, bx * blk:(bx + 1) * blk] = r if flat[by, bx] < 128 else 255 - r
    return np.clip(p[:h, :w], 0, 255).astype(np.int16)


def plane_noise(rng, h, w):
    """texture: low-amplitude noise on a slowly varying level (local extrema of every edge class, still smooth enough to be filtered) with patches of full-range noise"""
    level = np.kron(rng.integers(0, 256, ((h + 31) // 32, (w + 31) // 32)), np.ones((32, 32), np.int64))[:h, :w]
    p = level + rng.integers(-3, 4, (h, w))
    wild = np.kron(rng.random(((h + 15) // 16, (w + 15) // 16)) < 0.25, np.ones((16, 16), bool))[:h, :w]
    p[wild] = rng.integers(0, 256, (h, w))[wild]
    return np.clip(p, 0, 255).astype(np.int16)


RECON_FAMILIES = ("steps", "clips", "noise")


def make_recon(rng, size, family, qp):
    w, h = size
    if family == "steps":
        return [plane_steps(rng, h, w, int(rng.choice([8, 8, 4])), qp), plane_steps(rng, h // 2, w // 2, 8, qp), plane_steps(rng, h // 2, w // 2, int(rng.choice([8, 4])), qp)]
    if family == "clips":
        return [plane_clips(rng, h, w, 8), plane_clips(rng, h // 2, w // 2, 8), plane_clips(rng, h // 2, w // 2, 4)]
    return [plane_noise(rng, h, w), plane_noise(rng, h // 2, w // 2), plane_noise(rng, h // 2, w // 2)]


SOURCE_MODES = ("band", "edge0", "edge1", "edge2", "edge3", "noise1", "shift+", "shift-", "same")
EO_NEIGHBOURS = (((0, -1), (0, 1)), ((-1, 0), (1, 0)), ((-1, -1), (1, 1)), ((-1, 1), (1, -1)))      # (dy, dx) of the two neighbours per edge type


def source_region(rng, rec, mode):
    """what the encoder would have seen for this part of the picture so that SAO's `mode` pays: rec is the part with a one-sample ring"""
    r = rec.astype(np.int64)
    core = r[1:-1, 1:-1]
    if mode == "band":
        start = int(rng.choice([0, 28, int(rng.integers(0, 29))]))
        shift = np.zeros(32, np.int64)
        shift[start:start + 4] = rng.choice([-7, -3, -2, -1, 1, 2, 3, 7], 4)
        out = core + shift[core >> 3]
    elif mode.startswith("edge"):
        (ay, ax), (by, bx) = EO_NEIGHBOURS[int(mode[4])]
        a = r[1 + ay:r.shape[0] - 1 + ay, 1 + ax:r.shape[1] - 1 + ax]
        b = r[1 + by:r.shape[0] - 1 + by, 1 + bx:r.shape[1] - 1 + bx]
        k = np.sign(core - a) + np.sign(core - b)
        amp = rng.integers(1, 8, 5)
        out = core - np.where(k > 0, 1, np.where(k < 0, -1, 0)) * amp[k + 2]
    elif mode == "noise1":
        out = core + rng.integers(-1, 2, core.shape)
    elif mode == "shift+":
        out = core + 20
    elif mode == "shift-":
        out = core - 20
    else:
        out = core
    return np.clip(out, 0, 255)


def make_source(rng, size, recon):
    """the reconstruction plus, per CTU, one of SOURCE_MODES; neighbouring CTUs often share a mode AND its random draw's statistics, which is what makes merging pay"""
    nx, ny = grid(size)
    seed_of_case = rng.integers(1 << 30)
    palette = [SOURCE_MODES[i] for i in rng.permutation(len(SOURCE_MODES))[:int(rng.integers(2, 5))]]
    # runs of equal modes along rows, columns that repeat the row above: merge-left and merge-up candidates
    modes = np.empty((ny, nx), object)
    for cy in range(ny):
        for cx in range(nx):
            u = rng.random()
            modes[cy, cx] = modes[cy, cx - 1] if cx and u < 0.35 else (modes[cy - 1, cx] if cy and u < 0.7 else palette[int(rng.integers(len(palette)))])
    out = []
    for k, p in enumerate(recon):
        n = 32 if k else 64
        ring = np.pad(p, 1, mode="edge")
        s = np.zeros(p.shape, np.uint8)
        for cy in range(ny):
            for cx in range(nx):
                y0, x0, y1, x1 = cy * n, cx * n, min(cy * n + n, p.shape[0]), min(cx * n + n, p.shape[1])
                sub = np.random.default_rng([SEED, 77, SOURCE_MODES.index(modes[cy, cx]), int(seed_of_case)]) if rng.random() < 0.5 else rng      # (a shared draw: the same offsets pay in both CTUs)
                s[y0:y1, x0:x1] = source_region(sub, ring[y0:y1 + 2, x0:x1 + 2], modes[cy, cx])
        out.append(s)
    return out, modes


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------------------------

SIZES = ((200, 136), (416, 240), (264, 72), (192, 128), (264, 64))      # 4x3 (rem 8, 8), 7x4 (32, 48), 5x2 (8, 8), 3x2 (none), 5x1: every border kind
QPS = (0, 15, 16, 17, 32, 45, 51)
CQOS = (-12, 0, 2, 12)
CONTENT_OF = {(200, 136): "default", (416, 240): "extremes", (264, 72): "noise", (192, 128): "chroma", (264, 64): "motion"}


def _str_seed(name):
    return [SEED, 17] + [ord(ch) for ch in name]


def build_case(name, size, slice_type, qp, *, base, cqo=2, sao=1, sbh=1, threads=1, wpp=1, rc=None, mutate=True, recon="steps", levels="small", planes=False):
    rng = np.random.default_rng(_str_seed(name))
    rc = rc or {}
    fixture_recon = None
    if base == "fixture":
        raw, fixture_recon = fixture_records({SLICE_I: 0, SLICE_P: 1}[slice_type])
    else:
        raw = checker_records(size, CONTENT_OF[size], 0 if slice_type == SLICE_I else 1, tuple(sorted(rc.items())))
    recs = as_records(raw)
    case = dict(name=name, size=size, slice=slice_type, qp=qp, cfg_qp=32 if rc else qp, cqo=cqo, sao=sao, sbh=sbh, threads=threads, wpp=wpp, rc=rc, planes=planes, mutated=mutate,
                fixture_recon=fixture_recon, groups=min(grid(size)[1], 32))
    if mutate:
        mutate_levels(rng, recs, levels)
        mutate_mvd(rng, recs)
        mutate_mv_ref(rng, recs, slice_type == SLICE_P)
        if not rc:
            recs["qp"][:] = qp      # (rate-controlled records keep their per-CU QPs and with them a consistent delta-QP syntax)
        rec_planes = make_recon(rng, size, recon, qp)
        set_recon(recs, size, rec_planes)
        src, modes = make_source(rng, size, rec_planes)
        case["modes"] = modes
    else:
        # the source of the encode the records come from
        planes_ = list(ec.clip_frames(size[0], size[1], 2, seed=1234 if base == "fixture" else 1234 + SEED, content="default" if base == "fixture" else CONTENT_OF[size]))[0 if slice_type == SLICE_I else 1]
        src = [np.frombuffer(p, np.uint8).reshape((size[1] >> (k > 0), size[0] >> (k > 0))).copy() for k, p in enumerate(planes_)]
    case["records"] = recs
    case["src"] = [np.ascontiguousarray(s, np.uint8) for s in src]
    return case


@functools.lru_cache(None)
def cases():
    """about 40 cases: the crossing of the issue's configurations is sampled, every value of every axis occurs, the thin combinations are named"""
    out = []
    # unmutated: the reference's own records (its reconstruction is in the fixture) and the checker's own, fixed QP and rate controlled
    out.append(build_case("fixture-I", (200, 136), SLICE_I, 32, base="fixture", mutate=False))
    out.append(build_case("fixture-P", (200, 136), SLICE_P, 32, base="fixture", mutate=False, threads=3))
    out.append(build_case("checker-P-416", (416, 240), SLICE_P, 32, base="checker", mutate=False, planes=False))
    for k, (size, st, sao, threads) in enumerate((((416, 240), SLICE_P, 1, 1), ((416, 240), SLICE_I, 1, 4), ((200, 136), SLICE_P, 0, 1), ((264, 64), SLICE_P, 1, 1))):
        out.append(build_case(f"rc-{k}", size, st, 32, base="checker", mutate=False, sao=sao, threads=threads, rc={"bitrate_mode": 1 + (k & 1), "bitrate": 300 + 200 * k}))
    # mutated: sizes x QPs x families, the other axes dealt round robin so that every pair of neighbouring axes meets
    k = 0
    for size in SIZES:
        for qp in QPS:
            st = SLICE_P if k % 3 else SLICE_I
            hctu = grid(size)[1]
            wpp_kind = k % 4      # 0, 1: one thread, a sub-stream per row; 2: a thread per row; 3: one sub-stream for the picture
            out.append(build_case(f"mut-{size[0]}x{size[1]}-qp{qp}", size, st, qp, base="checker" if size != (200, 136) or k % 2 else "fixture", cqo=CQOS[k % 4], sao=0 if k % 5 == 4 else 1,
                                  sbh=(k // 2) % 2, threads=hctu if wpp_kind == 2 else 1, wpp=0 if wpp_kind == 3 else 1, recon=RECON_FAMILIES[(k + k // 3) % 3],
                                  levels=LEVEL_CLASSES[(k + k // 4) % 4], planes=(size in ((200, 136), (264, 72)) and qp == 45)))
            k += 1
    return out


# ---- the oracle chain --------------------------------------------------------------------------------------------------------------------------------------

def ptr(a, offset=0):
    return VP(a.ctypes.data + offset * a.itemsize)


def oracle_units(ora, case):
    recs, size = case["records"], case["size"]
    nx, ny = grid(size)
    us = nx * 16
    shape = (ny * 16, us)
    o = dict(mvx=np.zeros(shape, np.int16), mvy=np.zeros(shape, np.int16), ref=np.zeros(shape, np.int8), uqp=np.zeros(shape, np.uint8), flags=np.zeros(shape, np.uint8))
    pd, ti = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    mvx, mvy = np.ascontiguousarray(recs["mv_ref"][:, :, 0].astype(np.int16)), np.ascontiguousarray(recs["mv_ref"][:, :, 1].astype(np.int16))
    cont = {k: np.ascontiguousarray(recs[k]) for k in ("mv_ref_idx", "qp", "pred_mode", "pred_depth", "tr_idx")}
    cbf_y = np.ascontiguousarray(recs["cbf"][:, 0, :])
    ora.ora_units_from_ctus(ptr(mvx), ptr(mvy), ptr(cont["mv_ref_idx"]), ptr(cont["qp"]), ptr(cont["pred_mode"]), ptr(cbf_y), ptr(cont["pred_depth"]), ptr(cont["tr_idx"]),
                            C.c_int(nx), C.c_int(ny), C.c_int(us), ptr(o["mvx"]), ptr(o["mvy"]), ptr(o["ref"]), ptr(o["uqp"]), ptr(o["flags"]), ptr(pd), ptr(ti))
    ora.ora_make_edge_flags.restype = None
    ora.ora_make_edge_flags(ptr(pd), ptr(ti), C.c_int(size[0]), C.c_int(size[1]), C.c_int(us), ptr(o["flags"]))
    return o


def sao_lambdas(case, qp0):
    """hmr_wpp_sao_ctu :1415-1430: by the QP of the CTU's first unit"""
    factor = 0.57 if case["slice"] == SLICE_I else 0.4624
    return factor * math.pow(1.4, (qp0 - 12) / 1.4), factor * math.pow(1.4, (qp0 - 12 + case["cqo"]) / 1.4)


def oracle_chain(ora, case, units, sao_recon, geom):
    """deblocked picture, SAO statistics and candidates, final padded picture from the oracle; `units` its unit arrays (under rate control with the coded QPs),
    sao_recon [nctu][3][35] the parameters the checker decided"""
    w, h = case["size"]
    nx, ny = grid(case["size"])
    us = nx * 16
    rec = recon_planes(case["records"], case["size"])
    dbk = [p.copy() for p in rec]
    bsv, bsh = np.zeros(units["flags"].shape, np.uint8), np.zeros(units["flags"].shape, np.uint8)
    ora.ora_deblock_frame(ptr(dbk[0]), C.c_int(w), ptr(dbk[1]), ptr(dbk[2]), C.c_int(w // 2), C.c_int(w), C.c_int(h), C.c_int(us), ptr(units["mvx"]), ptr(units["mvy"]), ptr(units["ref"]),
                          ptr(units["uqp"]), ptr(units["flags"]), C.c_int(case["cqo"]), C.c_int(case["cqo"]), C.c_int(0), C.c_int(0), ptr(bsv), ptr(bsh))
    out = dict(rec=rec, dbk=dbk, bs_ver=bsv, bs_hor=bsh)
    fin = [p.copy() for p in dbk]
    if case["sao"]:
        src16 = [np.ascontiguousarray(s, np.int16) for s in case["src"]]
        stats = np.zeros((nx * ny, 3, 5, 2, 32), np.int32)
        ora.ora_sao_stats_frame(ptr(src16[0]), ptr(src16[1]), ptr(src16[2]), C.c_int(w), C.c_int(w // 2), ptr(dbk[0]), ptr(dbk[1]), ptr(dbk[2]), C.c_int(w), C.c_int(w // 2),
                                C.c_int(w), C.c_int(h), ptr(stats))
        out["stats"] = stats
        params = np.zeros((nx * ny, 3, 34), np.int32)
        params[:, :, 0] = sao_recon[:, :, 0] != SAO_OFF
        params[:, :, 1] = sao_recon[:, :, 1]
        params[:, :, 2:] = sao_recon[:, :, 3:]
        ora.ora_sao_apply_frame(ptr(dbk[0]), ptr(dbk[1]), ptr(dbk[2]), ptr(fin[0]), ptr(fin[1]), ptr(fin[2]), C.c_int(w), C.c_int(w // 2), C.c_int(w), C.c_int(h), ptr(params))
    padded = []
    for k, p in enumerate(fin):
        st, m = geom["stride"][k > 0], geom["margin"][k > 0]
        P = np.full((p.shape[0] + 2 * m, st), POISON16, np.int16)
        P[m:m + p.shape[0], m:m + p.shape[1]] = p
        ora.ora_pad_plane(ptr(P, m * st + m), C.c_int(st), C.c_int(p.shape[1]), C.c_int(p.shape[0]), C.c_int(m), C.c_int(m))
        padded.append(P)
    out["fin"] = padded
    return out


def oracle_candidates(ora, case, stats, qp0):
    """per CTU the candidate offsets [3][5][32] and band positions [3][5] of SAO_NEW (qp0: the QP of each CTU's first unit)"""
    n = stats.shape[0]
    off, aux, dist = np.zeros((n, 3, 5, 32), np.int32), np.zeros((n, 3, 5), np.int32), np.zeros((n, 3, 5), np.int64)
    for i in range(n):
        ly, lc = sao_lambdas(case, int(qp0[i]))
        lam = (C.c_double * 3)(ly, lc, lc)
        ora.ora_sao_offsets_ctu(ptr(stats[i]), lam, ptr(off[i]), ptr(aux[i]), ptr(dist[i]))
    return off, aux


def tiles(n, t):
    return list(range(0, n - t + 1, t)) + ([n - t] if n % t else [])


def phase_region(case, k, geom):
    """(y0, y1, x0, x1) in allocation coordinates: the part of component k's phase planes that is compared - what a vector can address.  subpel_task.h: the search keeps a
    block inside the picture, refinement and merge candidates move it at most 64 + 1 luma samples out and the taps reach four more, so the outermost columns and rows of
    the 80-sample margin (chroma: 40) are never read.  They are also where the task's input is not picture: its taps stop at the allocation's edge where the oracle's run
    on linearly, and the columns behind the right margin (a stride rounded up to 16 bytes) hold whatever the allocation holds - the poison here - which the task's 16-bit
    horizontal stage is not made for.  Compared: everything at least 8 luma / 4 chroma samples inside the padded picture, 72 / 36 samples of margin on every side."""
    w, h = case["size"][0] >> (k > 0), case["size"][1] >> (k > 0)
    m, inset = geom["margin"][k > 0], 4 if k else 8
    return inset, h + 2 * m - inset, inset, w + 2 * m - inset


def oracle_phase_planes(ora, fin):
    """the phase planes of section 13 from the final padded picture by the oracle's motion compensation, where subpel_task.h produces them from the same samples: every
    sample at least four away from the allocation's edge (nearer, the task's taps stop at the edge and the oracle's run on linearly; no vector reads there)"""
    ora.ora_mc_luma.argtypes = [VP, C.c_int, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    ora.ora_mc_chroma.argtypes = [VP, C.c_int, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    out = []
    for k, P in enumerate(fin):
        rows, stride = P.shape
        hh, ww = rows - 8, stride - 8
        phases = 64 if k else 16
        want = np.zeros((phases, hh, ww), np.int16)
        base = P.ctypes.data + 2 * (4 * stride + 4)
        for f in range(phases):
            fx, fy = (f & 7, f >> 3) if k else (f & 3, f >> 2)
            for y0 in tiles(hh, 8):
                for x0 in tiles(ww, 8):
                    src, dst = VP(base + 2 * (y0 * stride + x0)), VP(want.ctypes.data + 2 * ((f * hh + y0) * ww + x0))
                    if k:
                        ora.ora_mc_chroma(src, stride, dst, ww, 8, fx, fy, 0)
                    else:
                        ora.ora_mc_luma(src, stride, dst, ww, 8, 8, fx, fy, 0)
        out.append(want.astype(np.uint8))
    return out


# ---- comparisons (shared by the CPU and the GPU test: `got` is the checker's or the device's output) ------------------------------------------------------------

def check_against_oracle(ora, case, got, decided, geom, what):
    """unit arrays, deblocked picture, poison, final picture with margins of `got` against the oracle chain run with the SAO parameters `decided` (the checker's)"""
    w, h = case["size"]
    units = oracle_units(ora, case)
    u4, w4 = h // 4, w // 4
    for name in ("mvx", "mvy", "ref", "uqp", "flags"):
        if name == "uqp" and case["rc"]:
            continue      # (coding rewrites the QP of CUs without levels under rate control: held to the checker, and the oracle filters with what the checker coded)
        bad = np.argwhere(got[name][:u4, :w4] != units[name][:u4, :w4])
        assert not len(bad), f"{what} {case['name']}: unit array {name}: {len(bad)} units differ, first {bad[:4].tolist()}"
    if case["rc"]:
        units["uqp"] = decided["uqp"].copy()
    exp = oracle_chain(ora, case, units, decided["sao_recon"], geom)
    for k in range(3):
        m = geom["margin"][k > 0]
        ph, pw = exp["dbk"][k].shape
        g = got[f"dbk{k}"]
        bad = np.argwhere(g[m:m + ph, m:m + pw] != exp["dbk"][k])
        assert not len(bad), f"{what} {case['name']}: deblocked plane {k}: {len(bad)} samples differ, first (y, x) {bad[:4].tolist()} got {g[m:m + ph, m:m + pw][tuple(bad[0])]} want {exp['dbk'][k][tuple(bad[0])]}"
        outside = g.copy()
        outside[m:m + ph, m:m + pw] = POISON16
        bad = np.argwhere(outside != POISON16)
        assert not len(bad), f"{what} {case['name']}: deblocked plane {k}: {len(bad)} samples outside the picture were written, first {bad[:4].tolist()}"
        f = got[f"fin{k}"]
        bad = np.argwhere(f != exp["fin"][k])
        assert not len(bad), f"{what} {case['name']}: final plane {k} (allocation coordinates, margin {m}): {len(bad)} samples differ, first {bad[:4].tolist()} got {f[tuple(bad[0])]} want {exp['fin'][k][tuple(bad[0])]}"
    return units, exp


def check_streams(case, got, ref, what):
    """sub-streams, bit counts, contexts and the SAO decision of `got` against the checker's `ref`"""
    nx, ny = grid(case["size"])
    name = f"{what} {case['name']}"
    assert np.array_equal(got["errors"], np.zeros(4, np.int32)), f"{name}: errors {got['errors']}"
    for k in ("sao_coded", "sao_recon"):
        if case["sao"]:
            bad = np.argwhere((got[k] != ref[k]).any(axis=2))
            assert not len(bad), f"{name}: {k}: (CTU, component) {bad[:6].tolist()} got {got[k][tuple(bad[0])][:8]} want {ref[k][tuple(bad[0])][:8]}"
    nrows = ny if case["wpp"] else 1
    assert np.array_equal(got["bytecnt"][:nrows], ref["bytecnt"][:nrows]), f"{name}: bytecnt {got['bytecnt']} want {ref['bytecnt']}"
    flat_g, flat_r = got["bs"].reshape(-1), ref["bs"].reshape(-1)
    cap = got["bs"].shape[1]
    used = np.zeros(flat_g.size, bool)
    for r in range(nrows):
        n = int(ref["bytecnt"][r])
        assert n > 0, f"{name}: row {r} is empty"
        used[r * cap:r * cap + n] = True
        bad = np.flatnonzero(flat_g[r * cap:r * cap + n] != flat_r[r * cap:r * cap + n])
        assert not bad.size, f"{name}: sub-stream {r}: {bad.size} of {n} bytes differ, first at {bad[:4].tolist()}"
    assert (flat_g[~used] == POISON).all(), f"{name}: bytes behind a sub-stream's end were written: {np.flatnonzero((flat_g != POISON) & ~used)[:6].tolist()}"
    assert np.array_equal(got["cumbits"], ref["cumbits"]), f"{name}: cumbits, first CTU {np.flatnonzero(got['cumbits'] != ref['cumbits'])[:4].tolist()}"
    assert np.array_equal(got["ctx"][:nrows, :179], ref["ctx"][:nrows, :179]), f"{name}: RowEnt::ctx rows {np.flatnonzero((got['ctx'][:nrows, :179] != ref['ctx'][:nrows, :179]).any(axis=1)).tolist()}"
    if case["wpp"] and ny > 1:
        assert np.array_equal(got["saved"][:ny - 1, :179], ref["saved"][:ny - 1, :179]), f"{name}: RowEnt::saved"
    if case["rc"]:
        u4, w4 = case["size"][1] // 4, case["size"][0] // 4
        assert np.array_equal(got["uqp"][:u4, :w4], ref["uqp"][:u4, :w4]), f"{name}: unit QPs after coding"


# ---- what the sweep reaches: counted from the oracle's and the checker's outputs -----------------------------------------------------------------------------------

def luma_edge_census(units, exp, direction):
    """the luma filter's decisions per four-sample edge segment with bs > 0, from the oracle's boundary strengths and the samples the filter reads: the reconstruction
    for vertical edges (filtered first; the edges are eight apart and write three samples each side, so none reads another's output) - direction 0 only"""
    assert direction == 0
    y = exp["rec"][0].astype(np.int64)
    bs = exp["bs_ver"]
    qp = units["uqp"].astype(np.int64)
    uy, ux = np.nonzero((bs & 0x80) != 0)
    keep = (bs[uy, ux] & 3) > 0
    uy, ux = uy[keep], ux[keep]
    b = (bs[uy, ux] & 3).astype(np.int64)
    qpa = (qp[uy, ux - 1] + qp[uy, ux] + 1) >> 1
    tc, beta = TC_TABLE[np.clip(qpa + 2 * (b - 1), 0, 53)], BETA_TABLE[np.clip(qpa, 0, 51)]
    m = np.stack([np.stack([y[uy * 4 + l, ux * 4 + k - 4] for k in range(8)], axis=1) for l in range(4)], axis=1)      # [segment][line][p3 .. q3]
    dp = np.abs(m[:, :, 1] - 2 * m[:, :, 2] + m[:, :, 3])
    dq = np.abs(m[:, :, 4] - 2 * m[:, :, 5] + m[:, :, 6])
    d0, d3 = dp[:, 0] + dq[:, 0], dp[:, 3] + dq[:, 3]
    on = d0 + d3 < beta
    side = (beta + (beta >> 1)) >> 3
    fp, fq = dp[:, 0] + dp[:, 3] < side, dq[:, 0] + dq[:, 3] < side

    def strong(l, d):
        return (np.abs(m[:, l, 0] - m[:, l, 3]) + np.abs(m[:, l, 7] - m[:, l, 4]) < (beta >> 3)) & (2 * d < (beta >> 2)) & (np.abs(m[:, l, 3] - m[:, l, 4]) < ((tc * 5 + 1) >> 1))
    sw = on & strong(0, d0) & strong(3, d3)
    delta = (9 * (m[:, :, 4] - m[:, :, 3]) - 3 * (m[:, :, 5] - m[:, :, 2]) + 8) >> 4
    normal_line = (on & ~sw)[:, None] & (np.abs(delta) < 10 * tc[:, None])
    normal = normal_line.any(axis=1)
    clipped = normal_line & (np.abs(delta) > tc[:, None])
    return dict(segments=len(uy), strong=int(sw.sum()), normal=int(normal.sum()), unfiltered=int(len(uy) - sw.sum() - normal.sum()),
                fp_only=int((normal & fp & ~fq).sum()), fq_only=int((normal & ~fp & fq).sum()), both=int((normal & fp & fq).sum()), neither=int((normal & ~fp & ~fq).sum()),
                lines=int(4 * sw.sum() + normal_line.sum()), clipped=int(clipped.sum()))


def chroma_edge_census(case, units, exp):
    """the QP sums (before the clip to 0 .. 57) and tc indices of the chroma edges that are filtered (bs 2 on the 16-sample luma grid), both directions"""
    sums, idx = [], []
    qp = units["uqp"].astype(np.int64)
    for bs, dy, dx in ((exp["bs_ver"], 0, 1), (exp["bs_hor"], 1, 0)):
        uy, ux = np.nonzero((bs & 3) == 2)
        keep = ((ux if dx else uy) & 3) == 0
        uy, ux = uy[keep], ux[keep]
        qpa = (qp[uy - dy, ux - dx] + qp[uy, ux] + 1) >> 1
        s = qpa + case["cqo"]
        sums.append(s)
        idx.append(np.clip(np.array(CHROMA_QP)[np.clip(s, 0, 57)] + 2, 0, 53))
    return np.concatenate(sums), np.concatenate(idx)


def sao_outcomes(case, coded):
    """per CTU, luma and chroma: "off", "bo", "eo0" .. "eo3", "left", "up" """
    res = []
    for n in range(coded.shape[0]):
        row = []
        for comp in (0, 1):
            mode, typ = int(coded[n, comp, 0]), int(coded[n, comp, 1])
            row.append("off" if mode == SAO_OFF else (("left", "up")[typ] if mode == SAO_MERGE else ("bo" if typ == SAO_BO else f"eo{typ}")))
        res.append(row)
    return res
