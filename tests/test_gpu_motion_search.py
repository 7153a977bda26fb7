"""-m gpu: the walk's motion search on the device (motion_estimation<WaveGrp>, homerhevc_amd/csrc/enc/enc_inter.h, through hmr_gpu_prim_motion_search of include/homer_gpu.h
section 15) against the pinned oracle's ora_motion_estimation, which tests/test_motion.py and tests/golden/motion.npz hold equal to the reference's own function.  On the
device a round's positions, window tests and vector costs are computed in the lanes and the walk reads them with scalar indices - a form the one-lane checker build does
not have, so no device / checker comparison sees it.  Vector, sub-sample part and SAD must be EQUAL for every case.

One small picture (96 x 80 with a margin of 16 samples), its sixteen phase planes from hmr_gpu_subpel_planes (tests/test_gpu_subpel.py pins them), a hundred and some
seeded cases per block size in one launch per size.  The picture is a smooth texture (the search walks far on it) with a flat, a periodic and a noise rectangle in three
of its corners; the source blocks are displaced pieces of the picture, the co-located block itself (SAD 0: the early exits), flat, periodic and noise blocks.  A model of
the integer search in this file - held to the oracle's result for every case - counts what the walks of the case set reach."""
import ctypes as C

import numpy as np
import pytest

import libs

pytestmark = pytest.mark.gpu
VP = C.c_void_p
W, H, M = 96, 80, 16                      # the picture and its margin
STRIDE, ROWS = W + 2 * M, H + 2 * M
RX, RY = 128, 64                          # SEARCH_RANGE_X / _Y (enc_types.h)
PEL, HALF, QUARTER = 1, 2, 4
SIZES = (8, 16, 32, 64)


class MeCase(C.Structure):
    _fields_ = [("gx", C.c_int32), ("gy", C.c_int32), ("n_amvp", C.c_int32), ("amvp", C.c_int32 * 2 * 2), ("n_search", C.c_int32), ("search", C.c_int32 * 2 * 3),
                ("action", C.c_int32), ("start", C.c_int32 * 2), ("reserved", C.c_int32), ("corr", C.c_double)]


class MeOut(C.Structure):
    _fields_ = [("mv", C.c_int32 * 2), ("subpix", C.c_int32 * 2), ("sad", C.c_uint32)]


def make_picture():
    """the padded reference picture (int16, 0 .. 255)"""
    rng = np.random.default_rng(20240607)
    y, x = np.mgrid[0:ROWS, 0:STRIDE].astype(np.float64)
    tex = 128 + 55 * np.sin(x / 9.0 + y / 17.0) + 40 * np.cos(y / 7.0 - x / 23.0) + 20 * np.sin((x + 2 * y) / 5.0)
    pic = np.clip(np.rint(tex + rng.normal(0, 1.5, tex.shape)), 0, 255).astype(np.int16)
    pic[M:M + 32, M:M + 40] = 128                                                                              # flat: the top left corner
    pic[M:M + 24, M + 56:M + W] = rng.integers(0, 256, (24, W - 56))                                           # noise: top right
    py, px = np.mgrid[0:32, 0:W - 56]
    pic[M + 48:M + H, M + 56:M + W] = np.where(((px // 2) + (py // 2)) % 2 == 0, 60, 190)                      # period 4 both ways: bottom right
    return pic


def window(gx, gy, size):
    xlow = -gx if gx - RX < 0 else -RX
    xhigh = W - gx - size if gx + RX > W - size else RX
    ylow = -gy if gy - RY < 0 else -RY
    yhigh = H - gy - size if gy + RY > H - size else RY
    return xlow, xhigh, ylow, yhigh


def make_cases(pic, size, seed):
    """[(case fields, source block)]: positions at the corners, the edges and inside x source kinds x actions x lists x corr"""
    rng = np.random.default_rng(seed)
    xs, ys = sorted({0, (W - size) // 2 & ~3, W - size}), sorted({0, (H - size) // 2 & ~3, H - size})
    places = [(x, y) for y in ys for x in xs]
    places += [(int(rng.integers(0, W - size + 1)), int(rng.integers(0, H - size + 1))) for _ in range(6)]      # any position, odd ones too
    kinds = ["shift", "shift_far", "equal", "flat", "periodic", "noise"]
    actions = [PEL, PEL | HALF, PEL | HALF | QUARTER, HALF | QUARTER]
    corrs = [0.0, 0.37, 4.0, 900.0]                    # none, small, a QP-like weight, one under which the vector cost decides
    out = []
    k = 0
    for rep in range(2):
        for (gx, gy) in places:
            for kind in kinds:
                if (k + rep) % 2 and kind not in ("shift", "shift_far"):      # (half of the others: the displaced blocks are where the walks are long)
                    k += 1
                    continue
                action, corr = actions[k % 4], corrs[(k // 4 + k // 16) % 4]
                k += 1
                xlow, xhigh, ylow, yhigh = window(gx, gy, size)
                if kind in ("shift", "shift_far"):
                    r = 5 if kind == "shift" else 14
                    dx, dy = int(np.clip(rng.integers(-r, r + 1), xlow, xhigh)), int(np.clip(rng.integers(-r, r + 1), ylow, yhigh))
                    blk = pic[M + gy + dy:M + gy + dy + size, M + gx + dx:M + gx + dx + size].copy()
                    if rng.integers(0, 2):
                        blk = np.clip(blk + rng.integers(-2, 3, blk.shape), 0, 255).astype(np.int16)
                elif kind == "equal":
                    blk = pic[M + gy:M + gy + size, M + gx:M + gx + size].copy()
                elif kind == "flat":
                    blk = np.full((size, size), 128, np.int16)
                elif kind == "periodic":
                    py, px = np.mgrid[0:size, 0:size]
                    blk = np.where(((px // 2) + (py // 2)) % 2 == 0, 60, 190).astype(np.int16)
                else:
                    blk = rng.integers(0, 256, (size, size)).astype(np.int16)
                n_amvp = 1 + int(rng.integers(0, 2))
                amvp = [[int(v) for v in rng.integers(-24, 25, 2)] for _ in range(2)]
                if rng.integers(0, 4) == 0:
                    amvp[0] = [0, 0]
                if n_amvp == 1:
                    amvp[1] = [0, 0]
                n_search = int(rng.integers(0, 4))
                pool = [[int(v) for v in rng.integers(-40, 41, 2)], [0, int(rng.integers(-30, 31))], [int(rng.integers(-30, 31)), 0], [3, 2], [0, 0], [600, -20], [-8, 300],
                        [4 * xhigh, 4 * yhigh], [4 * xlow - 1, 4 * ylow]]
                search = [pool[int(i)] for i in rng.integers(0, len(pool), 3)]
                start = [0, 0]
                if not action & PEL:      # the sub-sample rounds alone, from a given vector inside the window
                    start = [4 * int(rng.integers(xlow, xhigh + 1)) + int(rng.integers(0, 4)), 4 * int(rng.integers(ylow, yhigh + 1)) + int(rng.integers(0, 4))]
                out.append((dict(gx=gx, gy=gy, n_amvp=n_amvp, amvp=amvp, n_search=n_search, search=search, action=action, start=start, corr=corr, kind=kind), blk))
    return out


def oracle_result(ora, pic, size, case, blk):
    c = case
    amvp, search, out = np.array(c["amvp"], np.int32).ravel(), np.array(c["search"], np.int32).ravel(), np.zeros(4, np.int32)
    orig = np.ascontiguousarray(blk, np.int16)
    ref = pic.ctypes.data + 2 * ((M + c["gy"]) * STRIDE + M + c["gx"])
    sad = ora.ora_motion_estimation(VP(orig.ctypes.data), size, VP(ref), STRIDE, c["gx"], c["gy"], c["start"][0] >> 2, c["start"][1] >> 2, size, RX, RY, W, H,
                                    VP(amvp.ctypes.data), c["n_amvp"], VP(search.ctypes.data), c["n_search"], C.c_double(c["corr"]), c["action"], VP(out.ctypes.data))
    return [int(v) for v in out], int(sad)


def model_integer_search(pic, size, c, blk):
    """The integer search (hmr_motion_inter.c:1404-1661 as oracle/hmr_oracle.c restates it) with counters: the whole-sample vector, did the distance-4 round run, iterations
    of the small-diamond descent, did a walk move its own bounds (next_start / search_size)."""
    gx, gy = c["gx"], c["gy"]
    xlow, xhigh, ylow, yhigh = window(gx, gy, size)
    amvp, corr = c["amvp"][:c["n_amvp"]], c["corr"]
    src = blk.astype(np.int64)

    def sad(x, y):
        return int(np.abs(src - pic[M + gy + y:M + gy + y + size, M + gx + x:M + gx + x + size]).sum())

    def cost(x, y):
        best = 0x7fffffff
        for ax, ay in amvp:
            best = min(best, int(corr * float(abs(ax - 4 * x)) + corr * float(abs(ay - 4 * y)) + .5))
        return best

    st = {"dist4": False, "descent": 0, "moved": 0}
    cur = {"x": int(np.clip(0, xlow, xhigh)), "y": int(np.clip(0, ylow, yhigh))}
    cur["sad"] = sad(cur["x"], cur["y"])
    cur["rd"] = (cur["sad"] + cost(cur["x"], cur["y"])) & 0xffffffff

    def attempt(x, y):
        if xlow <= x <= xhigh and ylow <= y <= yhigh:
            s = sad(x, y)
            rd = (s + cost(x, y)) & 0xffffffff
            if rd < cur["rd"]:
                cur.update(sad=s, rd=rd, x=x, y=y)
                return True
        return False

    ds = [(-1, 0), (0, -1), (1, 0), (0, 1)]
    db = [(-2, 0), (-1, -1), (0, -2), (1, -1), (2, 0), (1, 1), (0, 2), (-1, 1)]
    early = cur["sad"] <= 0
    if not early:
        for i in range(c["n_search"]):
            x, y = c["search"][i][0] >> 2, c["search"][i][1] >> 2
            if x == 0 and y == 0:
                continue
            attempt(x, y)
        early = cur["sad"] <= 0
    if not early:
        bx, by = cur["x"], cur["y"]
        for dx, dy in ds:
            attempt(bx + dx, by + dy)
        dist, end = 2, 4 if (bx != 0 and by != 0) else 8
        next_start, search_size = 0, 8
        bx, by = cur["x"], cur["y"]
        while dist < end:
            if dist == 4:
                st["dist4"] = True
            i = next_start
            while i < next_start + search_size:
                idx = i % 8
                if attempt(bx + db[idx][0] * dist, by + db[idx][1] * dist):
                    st["moved"] += 1
                    next_start, search_size = (idx - 2 + 8) % 8, 5
                i += 1
            dist *= 2
    bx, by = cur["x"], cur["y"]
    next_start, search_size = 0, 4
    while True:
        st["descent"] += 1
        i = next_start
        while i < next_start + search_size:
            idx = i % 4
            if attempt(bx + ds[idx][0], by + ds[idx][1]):
                st["moved"] += 1
                next_start, search_size = (idx - 1 + 4) % 4, 3
            i += 1
        if bx == cur["x"] and by == cur["y"]:
            break
        bx, by = cur["x"], cur["y"]
    return cur["x"], cur["y"], st


@pytest.fixture(scope="module")
def rig():
    """the picture, its phase planes from the device, every size's cases with the oracle's results: made once, read by all tests"""
    gpu, ora = libs.load_gpu(), libs.load_oracle()
    gpu.hmr_gpu_create.argtypes = [C.POINTER(VP), C.c_int, VP]
    gpu.hmr_gpu_malloc.argtypes = [VP, C.POINTER(VP), C.c_size_t]
    gpu.hmr_gpu_upload.argtypes = [VP, VP, VP, C.c_size_t]
    gpu.hmr_gpu_download.argtypes = [VP, VP, VP, C.c_size_t]
    gpu.hmr_gpu_free.argtypes = [VP, VP]
    gpu.hmr_gpu_subpel_planes.argtypes = [VP] * 4 + [C.c_int] * 4 + [VP] * 3
    gpu.hmr_gpu_prim_motion_search.argtypes = [VP, C.c_int, C.c_int, VP, VP, C.c_size_t, C.c_int64, C.c_int, C.c_int, C.c_int, VP]
    gpu.hmr_gpu_last_error.restype = C.c_char_p
    ora.ora_motion_estimation.restype = C.c_uint32
    ora.ora_motion_estimation.argtypes = [VP, C.c_int, VP, C.c_int] + [C.c_int] * 9 + [VP, C.c_int, VP, C.c_int, C.c_double, C.c_int, VP]
    ctx = VP()
    assert gpu.hmr_gpu_create(C.byref(ctx), 0, None) == 0, gpu.hmr_gpu_last_error()
    pic = make_picture()
    planes = np.zeros((ROWS, 16, STRIDE), np.uint8)
    d_pic, d_out = VP(), VP()
    assert gpu.hmr_gpu_malloc(ctx, C.byref(d_pic), C.c_size_t(pic.nbytes)) == 0 and gpu.hmr_gpu_malloc(ctx, C.byref(d_out), C.c_size_t(planes.nbytes)) == 0
    assert gpu.hmr_gpu_upload(ctx, d_pic, VP(pic.ctypes.data), C.c_size_t(pic.nbytes)) == 0
    assert gpu.hmr_gpu_subpel_planes(ctx, d_pic, None, None, STRIDE, ROWS, 0, 0, d_out, None, None) == 0, gpu.hmr_gpu_last_error()
    assert gpu.hmr_gpu_download(ctx, VP(planes.ctypes.data), d_out, C.c_size_t(planes.nbytes)) == 0
    gpu.hmr_gpu_free(ctx, d_pic)
    gpu.hmr_gpu_free(ctx, d_out)
    assert np.array_equal(planes[:, 0, :], pic.astype(np.uint8)), "plane 0 is the picture itself"
    sets = {}
    for size in SIZES:
        cases = make_cases(pic, size, 7000 + size)
        sets[size] = (cases, [oracle_result(ora, pic, size, c, blk) for c, blk in cases])
    return gpu, pic, planes, sets


def run_device(gpu, planes, size, cases):
    arr = (MeCase * len(cases))()
    for a, (c, _) in zip(arr, cases):
        a.gx, a.gy, a.n_amvp, a.n_search, a.action, a.corr = c["gx"], c["gy"], c["n_amvp"], c["n_search"], c["action"], c["corr"]
        for i in range(2):
            a.amvp[i][0], a.amvp[i][1] = c["amvp"][i]
        for i in range(3):
            a.search[i][0], a.search[i][1] = c["search"][i]
        a.start[0], a.start[1] = c["start"]
    src = np.ascontiguousarray(np.stack([blk for _, blk in cases]).astype(np.uint8))
    out = (MeOut * len(cases))()
    origin = (M * 16) * STRIDE + M
    rc = gpu.hmr_gpu_prim_motion_search(arr, len(cases), size, VP(src.ctypes.data), VP(planes.ctypes.data), C.c_size_t(planes.nbytes), origin, STRIDE, W, H, out)
    assert rc == 0, gpu.hmr_gpu_last_error()
    return [([o.mv[0], o.mv[1], o.subpix[0], o.subpix[1]], int(o.sad)) for o in out]


@pytest.mark.parametrize("size", SIZES)
def test_device_search_equals_the_oracle(rig, size):
    gpu, pic, planes, sets = rig
    cases, want = sets[size]
    assert len(cases) >= 100
    got = run_device(gpu, planes, size, cases)
    bad = [(i, cases[i][0], got[i], want[i]) for i in range(len(cases)) if got[i][0] != want[i][0] or got[i][1] != want[i][1]]
    assert not bad, f"{len(bad)} of {len(cases)} cases differ (case, device, oracle), first: {bad[:3]}"


def test_the_case_set_reaches_the_walks(rig):
    """the model of the integer search agrees with the oracle on every case with an integer search, so its counters say what the oracle's walks did"""
    gpu, pic, planes, sets = rig
    reach = {"dist4": 0, "descent3": 0, "moved": 0, "early": 0, "by_cost": 0}
    seen_actions, seen_nsearch, seen_namvp = set(), set(), set()
    for size in SIZES:
        cases, want = sets[size]
        for (c, blk), (mv, sad) in zip(cases, want):
            seen_actions.add(c["action"])
            seen_nsearch.add(c["n_search"])
            seen_namvp.add(c["n_amvp"])
            if not c["action"] & PEL:
                continue
            x, y, st = model_integer_search(pic, size, c, blk)
            assert (4 * x, 4 * y) == (mv[0] - mv[2], mv[1] - mv[3]), (size, c)
            reach["dist4"] += st["dist4"]
            reach["descent3"] += st["descent"] >= 3
            reach["moved"] += st["moved"] > 0
            reach["early"] += c["kind"] == "equal"
            if c["corr"] == 900.0 and c["action"] == PEL:      # the vector cost decides: the search does not go where the SAD alone would lead it
                c0 = dict(c, corr=0.0)
                reach["by_cost"] += model_integer_search(pic, size, c0, blk)[:2] != (x, y)
    print(reach)
    assert seen_actions == {PEL, PEL | HALF, PEL | HALF | QUARTER, HALF | QUARTER} and seen_nsearch == {0, 1, 2, 3} and seen_namvp == {1, 2}
    assert reach["dist4"] >= 10 and reach["descent3"] >= 10 and reach["moved"] >= 10 and reach["early"] >= 10 and reach["by_cost"] >= 3, reach
