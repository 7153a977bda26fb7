"""-m gpu: scene-cut statistics of a picture slot against the slot of the frame before (include/homer_gpu.h section 12m, k_cut in csrc/picture_io.hip,
homerhevc_amd/encoder.py).  Expected: the numpy restatement of tests/cut_cases.py, and hmr_gpu_cut_stats_host, on the pictures read back from the two slots by
hmr_gpu_enc_export_source_device.  Everything is asserted for equality.
The kernel's luma tile is 16 x 8 blocks of 8 x 8 samples = 128 x 64 samples (its search window: 144 x 80).  TILE_SHAPES: exactly one tile, one block more and one
block less on each axis.  The policy tests run the `default` clip of tools/gen_yuv.py (seed 1234) at 416 x 240, where NINTRA / blocks by hmr_gpu_cut_stats_host is
0.244, 0.248, 0.714, 0.207, 0.196 at frames 1 .. 5 with cut_at = 3 (test_cut_cpu.py asserts that one) and 0.244, 0.248, 0.220, 0.708, 0.196, 0.189 at frames 1 .. 6
with cut_at = 4: a share of 0.5 cuts exactly at the cut.  The 208 x 120 rungs are members of a group that their 416 x 240 rung leads."""
import ctypes as C

import numpy as np
import pytest

import cut_cases as cc
import encoder_cases as ec
from homerhevc_amd.encoder import IMAGE_AUTO, IMAGE_I, PIC_I420, SLICE_I, SLICE_P, BatchEncoder, Encoder, EncoderConfig, Picture, ScaledFrame, SceneCut, cut_score
from picture_gpu import LAYOUTS, current_stream, drop, gpu, slot_picture, upload  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_ARG = -3
# hmr_gpu_enc_create takes no picture narrower than two CTUs, and none of two CTU columns with more than one CTU row: of test_cut_cpu.py's sizes 136 x 40 and 200 x 136
# remain; 72 x 8 is the smallest size on both axes (one block row: no vertical vector is valid), 72 x 24 the smallest whose centre block row has its full vertical range
SMALL_SHAPES = [(72, 8), (72, 24), (136, 40), (200, 136)]
TILE_SHAPES = [(128, 64), (136, 72), (120, 56)]


@pytest.fixture(scope="module")
def lib(gpu):
    return cc.declare(gpu)


def new_stats(n=1):
    import torch
    return torch.full((n, cc.VALUES), -7, dtype=torch.int64, device="cuda")


def try_encoder(lib, w, h, **keys):
    ctx, enc = C.c_void_p(), C.c_void_p()
    assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
    if lib.hmr_gpu_enc_create(ctx, C.byref(ec.default_cfg(w, h, **keys)), C.byref(enc)) != 0:
        lib.hmr_gpu_destroy(ctx)
        return None, None
    return ctx, enc


def load(lib, enc, slot, picture, w, h, layout, seed=0):
    pic, keep = upload([p.tobytes() for p in cc.planes_of(picture, w, h)], w, h, layout, seed)
    assert lib.hmr_gpu_enc_load_source_device(enc, slot, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    del keep


def stats_one(lib, enc, slot, prev_slot, stats=None):
    stats = new_stats() if stats is None else stats
    assert lib.hmr_gpu_enc_cut_stats_one(enc, slot, prev_slot, C.c_void_p(stats.data_ptr()), current_stream()) == 0, lib.hmr_gpu_last_error()
    return stats[0].tolist()


def stats_many(lib, encs, slots, prev_slots, stats):
    k = len(encs)
    assert lib.hmr_gpu_enc_cut_stats((C.c_void_p * k)(*encs), k, (C.c_int * k)(*slots), (C.c_int * k)(*prev_slots), C.c_void_p(stats.data_ptr()), current_stream()) == 0, lib.hmr_gpu_last_error()
    return stats[:k].tolist()


@pytest.mark.parametrize("shape", SMALL_SHAPES + TILE_SHAPES)
def test_device_sums(lib, shape):
    """every content pair: prev into slot 0, cur into slot 1 - before anything has been encoded - then the single call, and the batched call with one entry, against
    the restatement and the host function on what the two slots hold"""
    import torch
    w, h = shape
    ctx, enc = try_encoder(lib, w, h)
    assert enc is not None, lib.hmr_gpu_last_error()
    for k, (name, (cur, prev)) in enumerate(cc.content_pairs(w, h, seed=11).items()):
        load(lib, enc, 0, prev, w, h, LAYOUTS[k % 3], seed=k)
        load(lib, enc, 1, cur, w, h, LAYOUTS[(k + 1) % 3], seed=k + 1)
        held_prev, held_cur = slot_picture(lib, enc, 0, w, h, "nv12", seed=3), slot_picture(lib, enc, 1, w, h, "tight_i420", seed=4)
        assert held_prev == prev and held_cur == cur, (shape, name)
        want = cc.restate(held_cur, held_prev, w, h)
        got = stats_one(lib, enc, 1, 0)
        assert got == want == cc.host_stats(lib, held_cur, held_prev, w, h, "pitched_nv12", "pitched_i420"), (shape, name)
        assert stats_many(lib, [enc], [1], [0], new_stats(2)) == [want], (shape, name)
        if name == "noise_noise":      # the other direction: the slots' roles are the call's, not the encoder's
            assert stats_one(lib, enc, 0, 1) == cc.restate(held_prev, held_cur, w, h), (shape, name)
    drop(lib, ctx, enc)
    torch.cuda.synchronize()


def test_full_size_pair(lib):
    """1920 x 1080: noise displaced by (7, 3) against the noise - every block away from the right and bottom edge finds itself - exact at size"""
    w, h = 1920, 1080
    ctx, enc = try_encoder(lib, w, h, wpp=17)
    assert enc is not None, lib.hmr_gpu_last_error()
    rng = np.random.default_rng(5)
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    noise, other = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes], [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    prev = b"".join(p.tobytes() for p in noise)
    cur = b"".join(p.tobytes() for p in [cc.shifted(noise[0], other[0], 7, 3)] + other[1:])
    load(lib, enc, 0, prev, w, h, "tight_i420")
    load(lib, enc, 1, cur, w, h, "nv12")
    want = cc.restate(cur, prev, w, h)
    blocks = w * h // 64
    assert blocks - want[cc.NINTRA] >= (w // 8 - 1) * (h // 8 - 1) and want[cc.SAD_Y] > 1 << 26
    assert stats_one(lib, enc, 1, 0) == want == cc.host_stats(lib, cur, prev, w, h)
    drop(lib, ctx, enc)


def test_batch_of_mixed_sizes(lib):
    """ONE call over encoders of different sizes, one of them twice - once in each direction"""
    shapes = [(200, 136), (136, 72), (128, 64)]
    made, want = [], []
    for k, (w, h) in enumerate(shapes):
        ctx, enc = try_encoder(lib, w, h)
        assert enc is not None, lib.hmr_gpu_last_error()
        pairs = cc.content_pairs(w, h, seed=20 + k)
        cur, prev = pairs[["gen_yuv_default_cut", "shift_-8_8", "noise_noise"][k]]
        load(lib, enc, 0, prev, w, h, LAYOUTS[k % 3], seed=k)
        load(lib, enc, 1, cur, w, h, LAYOUTS[(k + 1) % 3], seed=k)
        made.append((ctx, enc, cur, prev, w, h))
        want.append(cc.restate(cur, prev, w, h))
    ctx, enc, cur, prev, w, h = made[1]
    want.append(cc.restate(prev, cur, w, h))
    stats = new_stats(6)
    got = stats_many(lib, [m[1] for m in made] + [enc], [1, 1, 1, 0], [0, 0, 0, 1], stats)
    assert got == want
    assert stats[4:].min().item() == stats[4:].max().item() == -7      # (nothing behind the call's rows is written)
    for m in made:
        drop(lib, m[0], m[1])


def test_refusals_leave_the_encoder_working(lib):
    """every refusal of the header's list is HMR_GPU_ERR_ARG with a text, nothing is queued or written, and the encoders then still give their values and encode.
    (As in the SSIM test, host pointers and freed tensors are deliberately not tried.)"""
    import torch
    w, h = 136, 72
    ctx, enc = try_encoder(lib, w, h)
    ctx2, enc2 = try_encoder(lib, w, h)
    ctx3, one_slot = try_encoder(lib, w, h)
    assert enc and enc2 and one_slot, lib.hmr_gpu_last_error()
    cur, prev = cc.content_pairs(w, h, seed=31)["gen_yuv_default_cut"]
    for e in (enc, enc2):
        load(lib, e, 0, prev, w, h, "tight_i420")
        load(lib, e, 1, cur, w, h, "offset_i420")
    load(lib, one_slot, 0, prev, w, h, "tight_i420")
    st = current_stream()
    stats = new_stats(513)
    dev = C.c_void_p(stats.data_ptr())

    def many(encs, slots, prevs, out, n=None):
        k = len(encs)
        rc = lib.hmr_gpu_enc_cut_stats((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*slots) if slots is not None else None,
                                              (C.c_int * k)(*prevs) if prevs is not None else None, out, st)
        return rc, lib.hmr_gpu_last_error()

    refused = {
        "n = 0": many([enc], [1], [0], dev, n=0),
        "n = 513": many([enc] * 513, [1] * 513, [0] * 513, dev),
        "NULL encs": (lib.hmr_gpu_enc_cut_stats(None, 1, (C.c_int * 1)(1), (C.c_int * 1)(0), dev, st), lib.hmr_gpu_last_error()),
        "NULL slots": many([enc], None, [0], dev),
        "NULL prev_slots": many([enc], [1], None, dev),
        "NULL dev_stats": many([enc], [1], [0], None),
        "a NULL encoder": many([enc, None], [1, 1], [0, 0], dev),
        "a slot that does not exist": many([enc], [2], [0], dev),
        "a previous slot that does not exist": many([enc, enc2], [1, 1], [0, 2], dev),
        "a previous slot that does not exist yet": many([one_slot], [0], [1], dev),
        "a negative slot": many([enc, enc2], [1, -1], [0, 0], dev),
        "a negative previous slot": many([enc], [1], [-1], dev),
        "slot == prev_slot": many([enc, enc2], [1, 0], [0, 0], dev),
        "NULL encoder (single call)": (lib.hmr_gpu_enc_cut_stats_one(None, 1, 0, dev, st), lib.hmr_gpu_last_error()),
        "NULL dev_stats (single call)": (lib.hmr_gpu_enc_cut_stats_one(enc, 1, 0, None, st), lib.hmr_gpu_last_error()),
        "slot == prev_slot (single call)": (lib.hmr_gpu_enc_cut_stats_one(enc, 1, 1, dev, st), lib.hmr_gpu_last_error()),
    }
    if torch.cuda.device_count() > 1:
        ctx5, enc5 = C.c_void_p(), C.c_void_p()
        assert lib.hmr_gpu_create(C.byref(ctx5), 1, None) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_create(ctx5, C.byref(ec.default_cfg(w, h)), C.byref(enc5)) == 0, lib.hmr_gpu_last_error()
        refused["encoders on different devices"] = many([enc, enc5], [1, 1], [0, 0], dev)
        other = torch.zeros(8, dtype=torch.int64, device="cuda:1")
        refused["dev_stats on another device"] = many([enc], [1], [0], C.c_void_p(other.data_ptr()))
        drop(lib, ctx5, enc5)
    for why, (rc, text) in refused.items():
        assert rc == ERR_ARG and text, (why, rc, text)
    torch.cuda.synchronize()
    assert stats.min().item() == stats.max().item() == -7      # nothing was written by the refused calls
    want = cc.restate(cur, prev, w, h)
    rc, text = many([enc, enc2, enc], [1, 1, 1], [0, 0, 0], dev)      # the same encoder twice in one call is fine
    assert rc == 0, text
    assert stats[:3].tolist() == [want] * 3 and stats[3:].min().item() == stats[3:].max().item() == -7
    buf, n = C.create_string_buffer(1 << 20), C.c_long()
    assert lib.hmr_gpu_enc_encode_source(enc, 0, 0, buf, len(buf), C.byref(n), None) == SLICE_I, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_encode_source(enc, 1, 0, buf, len(buf), C.byref(n), None) == SLICE_P, lib.hmr_gpu_last_error()
    assert stats_one(lib, enc, 1, 0) == want      # (encoding leaves the slots as they were)
    for c, e in ((ctx, enc), (ctx2, enc2), (ctx3, one_slot)):
        drop(lib, c, e)


def test_cut_stats_are_ordered_against_the_consumer_stream(lib):
    """The values tensor is overwritten on a torch side stream behind so much queued work that the overwrite has not run when the call returns; that stream is the
    call's consumer stream, and a copy of the values queued on it right after the call - nothing is synchronised by the test - has to hold the expected values: the
    kernel (and the zeroing in front of it) waited for the consumer's earlier work, and the consumer's later work waited for the kernel.  The next frame is loaded
    into the older slot at once: it must not reach the slot before the kernel has read it."""
    import torch
    w, h, frames = 416, 240, 5
    clip = ec.clip_frames(w, h, frames, 3, 1234, "default")
    want = [None] + [cc.host_stats(lib, b"".join(clip[f]), b"".join(clip[f - 1]), w, h) for f in range(1, frames)]
    ctx, enc = try_encoder(lib, w, h, wpp=4)
    assert enc is not None, lib.hmr_gpu_last_error()
    clean = [torch.from_numpy(np.frombuffer(b"".join(planes), np.uint8).copy()).cuda() for planes in clip]
    pics = []
    for t in clean:
        pic = Picture(format=PIC_I420, reserved=0)
        pic.plane[0], pic.plane[1], pic.plane[2] = t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4
        pic.pitch[0], pic.pitch[1], pic.pitch[2] = w, w // 2, w // 2
        pics.append(pic)
    stats, copies = new_stats(), [new_stats() for _ in clip]
    ballast = torch.ones(1 << 28, dtype=torch.float32, device="cuda")      # 1 GB
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ballast.mul_(1.0)
    torch.cuda.synchronize()      # (set-up is over: from here on nothing waits on the host)
    pending = []
    for f in range(frames):
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pics[f]), current_stream()) == 0, lib.hmr_gpu_last_error()
        if f == 0:
            continue
        overwritten = torch.cuda.Event()
        with torch.cuda.stream(side):
            for _ in range(40):
                ballast.mul_(1.0)
            stats.fill_(-1)
            overwritten.record(side)
        assert lib.hmr_gpu_enc_cut_stats_one(enc, f & 1, (f & 1) ^ 1, C.c_void_p(stats.data_ptr()), C.c_void_p(side.cuda_stream)) == 0, lib.hmr_gpu_last_error()
        pending.append(not overwritten.query())
        with torch.cuda.stream(side):
            copies[f].copy_(stats, non_blocking=True)
    torch.cuda.synchronize()
    drop(lib, ctx, enc)
    assert all(pending), f"the values had already been overwritten when the call returned ({pending}): the test did not exercise the ordering"
    for f in range(1, frames):
        assert copies[f][0].tolist() == want[f], f


# ---- Encoder / BatchEncoder with a policy ----
def clip_tensors(w, h, frames, cut_at):
    import torch
    return [torch.from_numpy(np.frombuffer(b"".join(planes), np.uint8).copy()).cuda().view(h * 3 // 2, w) for planes in ec.clip_frames(w, h, frames, cut_at, 1234, "default")]


def test_encoder_class_with_a_policy(lib):
    w, h, frames, cut_at = 416, 240, 6, 3
    clip = clip_tensors(w, h, frames, cut_at)
    host = ec.clip_frames(w, h, frames, cut_at, 1234, "default")
    policy = SceneCut(share=0.5, min_gap=2)
    with Encoder(EncoderConfig(w, h, wfpp_num_threads=4)) as enc:
        with pytest.raises(RuntimeError):
            enc.cut_stats()
        stream, types, cuts = b"", [], []
        for f in range(frames):
            au, slice_type = enc.encode(clip[f], scene_cut=policy)
            stream += au
            types.append(slice_type)
            cuts.append(enc.last_cuts[0])
            stats = enc.cut_stats()
            assert stats.is_cuda and stats.dtype.is_floating_point is False and tuple(stats.shape) == (8,)
            if f == 0:
                assert stats.tolist() == [-1] * 8
            else:
                assert stats.tolist() == cc.host_stats(lib, b"".join(host[f]), b"".join(host[f - 1]), w, h), f
                assert (cut_score(stats.tolist(), w, h)[2] >= 0.5) == (f == cut_at)
    assert types == [SLICE_I if f in (0, cut_at) else SLICE_P for f in range(frames)] and cuts == [f == cut_at for f in range(frames)]
    with Encoder(EncoderConfig(w, h, wfpp_num_threads=4)) as enc:      # the same image types given by hand, no policy: the same stream
        again = b"".join(enc.encode(clip[f], IMAGE_I if f == cut_at else IMAGE_AUTO)[0] for f in range(frames))
        assert enc.last_cuts is None
    assert again == stream
    with Encoder(EncoderConfig(w, h, wfpp_num_threads=4)) as enc:      # an intra picture the caller asks for stays, and counts for min_gap
        policy = SceneCut(share=0.5, min_gap=2)
        types = [enc.encode(clip[f], IMAGE_I if f == 2 else IMAGE_AUTO, scene_cut=policy)[1] for f in range(frames)]
        assert types == [SLICE_I if f in (0, 2) else SLICE_P for f in range(frames)]      # (frame 3 is one frame behind the intra picture at 2)


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_encoder_class_with_a_policy(lib, pipelined):
    """two ladders of two rungs, each fed by ScaledFrames of its own 416 x 240 clip: ladder A (7 frames) cuts at frame 3, ladder B (6 frames, idle in the last step) at 4"""
    w, h = 416, 240
    clips = [clip_tensors(w, h, 7, 3), clip_tensors(w, h, 6, 4)]
    cut_at = [3, 3, 4, 4]
    cfgs = lambda: [EncoderConfig(416, 240, wfpp_num_threads=4), EncoderConfig(208, 120, wfpp_num_threads=2)] * 2      # noqa: E731
    frames_of = lambda f: [ScaledFrame(clips[i // 2][f], w, h) if f < len(clips[i // 2]) else None for i in range(4)]      # noqa: E731

    def run(policy, image_types):
        per_frame, all_cuts = [[] for _ in range(4)], []
        with BatchEncoder(cfgs(), pipelined=pipelined) as enc:
            sources = None
            for f in range(7):
                frames = frames_of(f)
                aus = enc.step(frames, image_types[f] if image_types else None, scene_cut=policy)
                for i, au in enumerate(aus):
                    if au:
                        per_frame[i].append(au)
                if policy is None:
                    assert enc.last_cuts is None
                    continue
                all_cuts.append(list(enc.last_cuts))
                table = enc.cut_stats()
                assert tuple(table.shape) == (4, 8) and table.is_cuda
                now = [bytes(p.cpu().numpy().tobytes()) if p is not None else None for p in enc.source()]
                for i in range(4):
                    if f == 0 or frames[i] is None:
                        assert table[i].tolist() == [-1] * 8, (f, i)
                    else:
                        assert table[i].tolist() == cc.host_stats(lib, now[i], sources[i], enc.cfgs[i].width, enc.cfgs[i].height), (f, i)
                sources = now
            for i, au in enumerate(enc.flush()):
                if au:
                    per_frame[i].append(au)
        return per_frame, all_cuts

    per_frame, cuts = run(SceneCut(share=0.5, min_gap=2, groups=[[0, 1], [2, 3]]), None)
    for i in range(4):
        assert len(per_frame[i]) == (7 if i < 2 else 6), i
        assert [cc.is_intra(au) for au in per_frame[i]] == [f in (0, cut_at[i]) for f in range(len(per_frame[i]))], i
    assert cuts == [[f == cut_at[i] and f < (7 if i < 2 else 6) for i in range(4)] for f in range(7)]
    by_hand, _ = run(None, [[IMAGE_I if f == cut_at[i] else IMAGE_AUTO for i in range(4)] for f in range(7)])
    assert by_hand == per_frame
