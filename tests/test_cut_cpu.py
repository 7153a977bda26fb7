"""Scene-cut statistics (include/homer_gpu.h section 12m), the parts that need no GPU: hmr_gpu_cut_stats_host - the host twin of the device kernel, the same
csrc/cut_stats.h - against the numpy restatement of tests/cut_cases.py on hostile content, hmr_gpu_cut_score against exact fractions, the argument errors, what the
Python module offers without torch, the header's declarations, the SceneCut policy on given rows, the condition on the `default` clip, and k_cut as compiled."""
import ctypes as C
import json
import os
import re
from fractions import Fraction

import pytest

import cut_cases as cc
import encoder_cases as ec
import libs
import picture_gpu
from homerhevc_amd.encoder import IMAGE_AUTO, IMAGE_I, Picture, SceneCut, cut_score
from test_ingest_cpu import in_a_fresh_process

ERR_ARG = -3
HIPCC = "/opt/rocm/bin/hipcc"
# 8 x 8: one block, one vector; 16 x 8: two blocks, nine vectors each; 24 x 24: only the centre block has its full range; 40 x 40: five blocks an axis;
# 136 x 40 and 200 x 136: more than one tile column / row of the kernel, odd block counts
SIZES = [(8, 8), (16, 8), (24, 24), (40, 40), (136, 40), (200, 136)]
LAYOUT_PAIRS = [("tight_i420", "tight_i420"), ("pitched_i420", "tight_nv12"), ("tight_nv12", "pitched_nv12"), ("pitched_nv12", "pitched_i420")]
CLIPS = [(64, 64), (136, 40), (416, 240)]


@pytest.fixture(scope="module")
def lib():
    from homerhevc_amd.build import build_native
    build_native()
    return cc.declare(picture_gpu.load())


@pytest.fixture(scope="module")
def pairs():
    """per size: {name: (cur, prev, the restatement's values)} - computed once"""
    return {(w, h): {name: (a, b, cc.restate(a, b, w, h)) for name, (a, b) in cc.content_pairs(w, h).items()} for w, h in SIZES}


@pytest.mark.parametrize("layouts", LAYOUT_PAIRS)
@pytest.mark.parametrize("size", SIZES)
def test_host_sums_are_the_restatements(lib, pairs, size, layouts):
    w, h = size
    for name, (a, b, want) in pairs[size].items():
        assert cc.host_stats(lib, a, b, w, h, *layouts) == want, (name, size, layouts)


@pytest.mark.parametrize("size", SIZES)
def test_what_the_content_has_to_give(pairs, size):
    """the restatement itself on the contents whose values are known beforehand"""
    w, h = size
    blocks = w * h // 64
    a, b, s = pairs[size]["identical"]
    act, msad = cc.block_terms(cc.planes_of(a, w, h)[0], cc.planes_of(b, w, h)[0])
    assert s[cc.SAD_Y] == s[cc.SAD_U] == s[cc.SAD_V] == s[cc.HIST] == s[cc.INTER] == s[cc.NINTRA] == 0 and s[cc.INTRA] == int(act.sum()) > 0 and not msad.any()
    for name in ("zero_255", "255_zero"):
        s = pairs[size][name][2]
        assert s[cc.SAD_Y] == 255 * w * h and s[cc.SAD_U] == s[cc.SAD_V] == 255 * w * h // 4 and s[cc.HIST] == 2 * w * h, name
        assert s[cc.INTRA] == s[cc.INTER] == 0 and s[cc.NINTRA] == blocks and s[cc.LUMA] == (0 if name == "zero_255" else 255 * w * h), name
    s = pairs[size]["stripes_inverse"][2]
    assert s[cc.SAD_Y] == 255 * w * h and s[cc.HIST] == 0 and s[cc.INTRA] == blocks * cc.MAX_ACT      # (every block: 32 samples of 0 and 32 of 255)
    for dx, dy in cc.SHIFTS:
        a, b, s = pairs[size][f"shift_{dx}_{dy}"]
        _, msad = cc.block_terms(cc.planes_of(a, w, h)[0], cc.planes_of(b, w, h)[0])
        for by in range(h // 8):
            for bx in range(w // 8):
                if 0 <= 8 * bx + dx and 8 * bx + dx + 8 <= w and 0 <= 8 * by + dy and 8 * by + dy + 8 <= h:
                    assert msad[by, bx] == 0, (size, dx, dy, bx, by)
    a, b, s = pairs[size]["shift_9"]
    _, msad = cc.block_terms(cc.planes_of(a, w, h)[0], cc.planes_of(b, w, h)[0])
    assert msad.min() > 0


def test_scores_are_the_correctly_rounded_quotients(lib, pairs):
    cases = [(list(want), w, h) for (w, h), by_name in pairs.items() for _, _, want in by_name.values()]
    w, h = 3840, 2160
    cases += [([255 * w * h, 255 * w * h // 4, 0, 2 * w * h, cc.MAX_ACT * (w * h // 64), cc.MAX_ACT * (w * h // 64), w * h // 64, 255 * w * h], w, h),
              ([1, 2, 3, 7, 3, 1, 1, 0], w, h), ([0] * 8, w, h), ([25459199, 3, 7, 199679, 10 ** 8 + 7, 10 ** 8 - 1, 1499, 5], 416, 240), ([0, 0, 0, 0, 0, 0, 0, 9], 8, 8)]
    seen_zero_intra = False
    for s, w, h in cases:
        want = [float(Fraction(s[cc.SAD_Y], w * h)), float(Fraction(s[cc.HIST], 2 * w * h)), float(Fraction(s[cc.NINTRA], w * h // 64)),
                float(Fraction(s[cc.INTER], s[cc.INTRA])) if s[cc.INTRA] else 1.0]
        seen_zero_intra |= s[cc.INTRA] == 0
        assert cc.score(lib, s, w, h) == want == list(cut_score(s, w, h)), (s, w, h)
    assert seen_zero_intra


def test_argument_errors(lib):
    w, h = 24, 16
    a = cc.HostPicture(bytes(w * h * 3 // 2), w, h, "tight_i420")
    b = cc.HostPicture(bytes(w * h * 3 // 2), w, h, "pitched_nv12")
    out, dbl = (C.c_int64 * 8)(), (C.c_double * 4)()

    def changed(pic, **kw):
        p = Picture(format=pic.format, reserved=pic.reserved)
        for c in range(3):
            p.plane[c], p.pitch[c] = pic.plane[c], pic.pitch[c]
        for k, v in kw.items():
            if k in ("format", "reserved"):
                setattr(p, k, v)
            else:
                getattr(p, k[:-1])[int(k[-1])] = v
        return p

    pa, pb = C.byref(a.pic), C.byref(b.pic)
    host = {
        "NULL cur": (None, pb, w, h, out), "NULL prev": (pa, None, w, h, out), "NULL stats": (pa, pb, w, h, None),
        "unknown format": (C.byref(changed(a.pic, format=5)), pb, w, h, out), "reserved": (pa, C.byref(changed(b.pic, reserved=1)), w, h, out),
        "a missing plane": (C.byref(changed(a.pic, plane2=None)), pb, w, h, out), "a pitch below a row": (pa, C.byref(changed(b.pic, pitch1=w - 1)), w, h, out),
        "width not a multiple of 8": (pa, pb, 20, h, out), "height not a multiple of 8": (pa, pb, w, 12, out), "odd width": (pa, pb, 23, h, out),
        "width 0": (pa, pb, 0, h, out), "negative height": (pa, pb, w, -16, out),
    }
    for why, args in host.items():
        assert lib.hmr_gpu_cut_stats_host(pa, pb, w, h, out) == 0
        assert lib.hmr_gpu_cut_stats_host(*args) == ERR_ARG and lib.hmr_gpu_last_error(), why
    W, H = 416, 240
    blocks, good = W * H // 64, [5, 4, 3, 2, 100, 50, 1, 77]

    def with_value(k, v):
        s = list(good)
        s[k] = v
        return (C.c_int64 * 8)(*s)

    ok = (C.c_int64 * 8)(*good)
    score = {
        "NULL stats": (None, W, H, dbl), "NULL results": (ok, W, H, None), "width not a multiple of 8": (ok, 420, H, dbl), "height not a multiple of 8": (ok, W, 236, dbl),
        "width 0": (ok, 0, H, dbl), "negative height": (ok, W, -240, dbl), "a negative value": (with_value(cc.SAD_U, -1), W, H, dbl),
        "SAD_Y above 255 W H": (with_value(cc.SAD_Y, 255 * W * H + 1), W, H, dbl), "SAD_V above 255 W H / 4": (with_value(cc.SAD_V, 255 * W * H // 4 + 1), W, H, dbl),
        "HIST above 2 W H": (with_value(cc.HIST, 2 * W * H + 1), W, H, dbl), "NINTRA above the blocks": (with_value(cc.NINTRA, blocks + 1), W, H, dbl),
        "INTRA above its most": (with_value(cc.INTRA, cc.MAX_ACT * blocks + 1), W, H, dbl), "INTER above INTRA": (with_value(cc.INTER, 101), W, H, dbl),
        "LUMA above 255 W H": (with_value(cc.LUMA, 255 * W * H + 1), W, H, dbl), "the all -1 row of a sequence without a pair": ((C.c_int64 * 8)(*([-1] * 8)), W, H, dbl),
    }
    for why, args in score.items():
        assert lib.hmr_gpu_cut_score(ok, W, H, dbl) == 0
        assert lib.hmr_gpu_cut_score(*args) == ERR_ARG and lib.hmr_gpu_last_error(), why


def test_python_cut_score_needs_neither_torch_nor_a_gpu():
    stats = [100, 2, 3, 50, 1000, 500, 1, 77]
    code = (f"from homerhevc_amd.encoder import cut_score, SceneCut; import homerhevc_amd; v = cut_score({stats!r}, 16, 8); assert 'torch' not in sys.modules, 'torch imported'; "
            "assert homerhevc_amd.cut_score is cut_score and homerhevc_amd.SceneCut is SceneCut; "
            f"assert SceneCut(min_gap=0).decide([0], [{stats!r}], [(16, 8)]) == [True]; assert 'torch' not in sys.modules; print(repr(list(v)))")
    r = in_a_fresh_process(code)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == [float(Fraction(100, 128)), float(Fraction(50, 256)), 0.5, 0.5]
    r = in_a_fresh_process("from homerhevc_amd.encoder import cut_score\nfor bad in ([1] * 8, 412, 240), ([-1] * 8, 416, 240), ([1, 2, 3], 416, 240):\n"
                           "    try:\n        cut_score(*bad)\n    except ValueError as e:\n        print('refused', e)")
    assert r.returncode == 0 and r.stdout.count("refused") == 3, (r.stdout, r.stderr)


def test_the_header_declares_the_calls():
    text = open(os.path.join(libs.ROOT, "include", "homer_gpu.h")).read()
    for name in ("hmr_gpu_enc_cut_stats", "hmr_gpu_enc_cut_stats_one", "hmr_gpu_cut_stats_host", "hmr_gpu_cut_score"):
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert "12m." in text and re.search(r"^#define HMR_GPU_CUT_VALUES 8$", text, re.M) and re.search(r"^#define HMR_GPU_CUT_RANGE 8$", text, re.M)


# ---- the policy as pure Python: rows of a 16 x 8 picture (two blocks), whose NINTRA decides ----
SIZE = (16, 8)
CUT, CALM, NONE = [9, 0, 0, 4, 50, 50, 2, 7], [9, 0, 0, 4, 50, 10, 0, 7], [-1] * 8


def test_policy_share_and_pairs():
    p = SceneCut(share=0.5, min_gap=0)
    assert p.decide([0, 1, 2], [CUT, CALM, NONE], [SIZE] * 3) == [True, False, False]
    assert p.decide([0, 1, 2], [None, [9, 0, 0, 4, 50, 30, 1, 7], CUT], [SIZE] * 3) == [False, True, True]      # (one block of two: exactly the share)
    assert SceneCut(share=0.51, min_gap=0).decide([0], [[9, 0, 0, 4, 50, 30, 1, 7]], [SIZE]) == [False]
    assert p.decide([1], [CUT, CUT, CUT], [SIZE] * 3) == [False, True, False]      # (sequences that are not live are not decided for)


def test_policy_min_gap():
    p = SceneCut(share=0.5, min_gap=3)
    got = [p.decide([0], [CUT if f else NONE], [SIZE])[0] for f in range(9)]
    assert got == [False, True, False, False, True, False, False, True, False]      # (no intra picture seen before frame 1; then every third frame)
    # an intra picture the encoder returned (frame 0, seen when it comes back) and one the caller asked for (frame 4) count
    p = SceneCut(share=0.5, min_gap=3)
    got = []
    for f in range(9):
        got.append(p.decide([0], [CUT if f else NONE], [SIZE], [IMAGE_I if f == 4 else IMAGE_AUTO])[0])
        p.observe(0, f == 0)
    assert got == [False, False, False, True, False, False, False, True, False]
    # a pipelined encoder reports a picture one step late: frame 5's intra picture is seen behind frame 6's decision
    p = SceneCut(share=0.5, min_gap=3)
    got = []
    for f in range(10):
        got.append(p.decide([0], [CUT if f >= 6 else NONE], [SIZE])[0])
        if f:
            p.observe(0, f - 1 == 5, back=1)
    assert got == [False] * 6 + [True, False, False, True]


def test_policy_groups():
    p = SceneCut(share=0.5, min_gap=0, groups=[[0, 1], [2, 3]])
    # the first member decides for its group, in either direction; sequence 4 is in no group
    assert p.decide([0, 1, 2, 3, 4], [CUT, CALM, CALM, CUT, CUT], [SIZE] * 5) == [True, True, False, False, True]
    # a lead member that is idle: the next live member leads; an idle member is not cut
    assert p.decide([1, 3, 4], [CUT, CALM, CUT, CUT, CALM], [SIZE] * 5) == [False, False, False, True, False]
    # a lead member without a pair decides "no" for the group; a member without a pair is cut with its group
    assert p.decide([0, 1, 2, 3], [NONE, CUT, CUT, NONE, None], [SIZE] * 5) == [False, False, True, True, False]
    with pytest.raises(ValueError):
        SceneCut(groups=[[0, 1], [1, 2]])


def test_policy_keeps_the_callers_intra_picture():
    """the decision is the policy's alone; the encoders pass IMAGE_I where either the caller or the policy asks for it (test_gpu_cut.py), and the policy counts both"""
    p = SceneCut(share=0.5, min_gap=2)
    assert p.decide([0, 1], [CALM, CALM], [SIZE] * 2, [IMAGE_I, IMAGE_AUTO]) == [False, False]
    assert p.decide([0, 1], [CUT, CUT], [SIZE] * 2, [IMAGE_AUTO, IMAGE_AUTO]) == [False, True]      # (sequence 0's intra picture was one frame ago)
    assert p.decide([0, 1], [CUT, CUT], [SIZE] * 2, None) == [True, False]


# ---- the condition on the clip ----
@pytest.mark.parametrize("size", CLIPS)
def test_the_default_clip_is_cut_where_its_cut_is(lib, size):
    """`default` with cut_at = 3 and seed 1234: NINTRA / blocks was at least 0.71 at frame 3 and at most 0.40 at frames 1, 2, 4 and 5 at these three sizes.  (The other
    families are hostile by design - noise and motion read as a cut at every frame, flat and extremes give almost none - and are compared for equality only.)"""
    w, h = size
    clip = ec.clip_frames(w, h, 6, 3, 1234, "default")
    for f in range(1, 6):
        share = cc.score(lib, cc.host_stats(lib, b"".join(clip[f]), b"".join(clip[f - 1]), w, h), w, h)[2]
        print(size, f, share)
        assert share >= 0.5 if f == 3 else share < 0.5, (size, f, share)


# ---- the kernel as compiled ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_cut_kernel_as_compiled():
    """k_cut for gfx950: no private memory, no spills, LDS that lets at least four workgroups share a CU (160 KB), global_ (not flat_) loads, the search on the
    unmasked quad SAD, and no store to memory but the 32- and 64-bit atomic adds; k_cut_finish: one plain store, the only writer of HIST"""
    remarks, asm = libs.picture_io_as_compiled()
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        seen[blk.split()[0]] = {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", blk)}

    def ops_of(name):
        body = asm[asm.index(name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        return [l[0] for l in (line.split(";")[0].split() for line in body.splitlines()) if l]

    names = [n for n in seen if "k_cut" in n and "finish" not in n]
    assert len(names) == 1, sorted(seen)
    f = seen[names[0]]
    print(f)
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0 and f["Occupancy [waves/SIMD]"] >= 4, f
    assert 0 < f["LDS Size [bytes/block]"] <= 160 * 1024 // 4, f
    ops = ops_of(names[0])
    assert not [o for o in ops if o.startswith(("flat_", "scratch_", "global_store", "buffer_"))]
    assert "global_load_dwordx4" in ops and ops.count("v_qsad_pk_u16_u8") == 32 and not [o for o in ops if o.startswith(("v_mqsad", "v_msad"))]
    assert sorted(set(o for o in ops if o.startswith("global_atomic"))) == ["global_atomic_add", "global_atomic_add_x2"]
    names = [n for n in seen if "k_cut_finish" in n]
    assert len(names) == 1, sorted(seen)
    f = seen[names[0]]
    assert f["ScratchSize [bytes/lane]"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, f
    ops = ops_of(names[0])
    assert not [o for o in ops if o.startswith(("flat_", "scratch_", "buffer_", "global_atomic"))] and [o for o in ops if o.startswith("global_store")] == ["global_store_dwordx2"]
