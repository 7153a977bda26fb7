"""-m gpu: SSIM sums of the reconstructed pictures left in device memory (include/homer_gpu.h section 12h, k_ssim in csrc/picture_io.hip, homerhevc_amd/encoder.py).
The fixtures' expectation is tests/golden/ssim.json - the sums between the clip and the compiled reference's own reconstruction, by the Python-integer oracle of
tests/ssim_cases.py; the hostile shapes' is that oracle, and hmr_gpu_ssim_host, on the pictures downloaded from the device.  Everything is asserted for equality."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import encoder_cases as ec
import ssim_cases as sc
from homerhevc_amd.encoder import PIC_I420, BatchEncoder, Encoder, Picture, ssim
from picture_gpu import (BATCH_CASES, GOLD, LAYOUTS, Output, as_tensors, config_of, current_stream, drop, export_one, gpu, make_encoder, new_sums,  # noqa: F401
                         upload)

pytestmark = pytest.mark.gpu
SSIM = json.load(open(os.path.join(ec.GOLDEN, "ssim.json")))
ERR_ARG = -3
IDLE = -(1 << 63)
CASES = ["200x136", "328x264_wpp3", "416x240_wpp_rows", "384x192_noise_qp0", "416x240_extremes_qp4", "1920x1080_cfg2_wpp_rows"]
# The kernel's tile is 32 x 8 windows = 33 x 9 blocks of 4 x 4 samples.  Block counts per axis, luma (always even) and chroma: one tile exactly where a size exists
# (chroma 33 across: 264; 9 down: 72), the nearest accepted size above (luma 34 x 10: 136 x 40; chroma 34 x 10: 272 x 80) and below (luma 32 x 8: 128 x 32; chroma
# 32 x 8: 256 x 64); 136 x 40 and 200 x 136 have odd chroma block counts (17 x 5, 25 x 17), 200 x 136 more than one tile row in both planes.
SHAPES = [(128, 32), (136, 40), (256, 64), (264, 72), (272, 80), (200, 136)]
FAMILIES = ["default", "noise", "extremes", "flat", "motion", "chroma"]


def ssim_one(lib, enc, slot, sums):
    assert lib.hmr_gpu_enc_ssim_one_device(enc, slot, C.c_void_p(sums.data_ptr()), current_stream()) == 0, lib.hmr_gpu_last_error()
    return sums[0].tolist()


def ssim_many(lib, encs, slots, sums):
    k = len(encs)
    assert lib.hmr_gpu_enc_ssim_device((C.c_void_p * k)(*encs), k, (C.c_int * k)(*slots), C.c_void_p(sums.data_ptr()), current_stream()) == 0, lib.hmr_gpu_last_error()
    return sums[:k].tolist()


def tight(t, w, h):
    """the descriptor of a tightly packed I420 picture in the uint8 CUDA tensor t"""
    pic = Picture(format=PIC_I420, reserved=0)
    pic.plane[0], pic.plane[1], pic.plane[2] = t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4
    pic.pitch[0], pic.pitch[1], pic.pitch[2] = w, w // 2, w // 2
    return pic


@pytest.mark.parametrize("case", CASES)
def test_single_sums(gpu, case):
    """hmr_gpu_enc_load_source_device + hmr_gpu_enc_encode_source + hmr_gpu_enc_ssim_one_device, frame by frame"""
    lib, g, s = gpu, GOLD[case], SSIM[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    buf, n, stream = C.create_string_buffer(max(4 << 20, w * h * 2)), C.c_long(), b""
    for f, planes in enumerate(clip):
        pic, keep = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        del keep
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        assert ssim_one(lib, enc, f & 1, new_sums()) == s["ssim"][f], (case, f)
    drop(lib, ctx, enc)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_sums(gpu, pipelined):
    """sequences of different sizes: one load, one batch launch and ONE SSIM call per step for those that still have frames.  Pipelined: the call follows its step
    directly, while that step's access units are still outstanding."""
    lib = gpu
    made = [make_encoder(lib, case) for case in BATCH_CASES]
    bufs = [C.create_string_buffer(1 << 20) for _ in made]
    streams = [b"" for _ in made]

    def call(live, slot):
        k = len(live)
        got = (C.c_long * k)()
        fn = lib.hmr_gpu_enc_encode_batch_pipelined if pipelined else lib.hmr_gpu_enc_encode_batch
        assert fn((C.c_void_p * k)(*[made[i][1] for i in live]), k, (C.c_int * k)(*([slot] * k)) if slot is not None else None,
                  (C.c_int * k)(*[made[i][4] for i in live]), (C.c_char_p * k)(*[C.cast(bufs[i], C.c_char_p) for i in live]), (C.c_long * k)(*[len(bufs[i]) for i in live]),
                  got) == 0, lib.hmr_gpu_last_error()
        for j, i in enumerate(live):
            streams[i] += C.string_at(bufs[i], got[j])

    prev = None
    for f in range(max(len(m[5]) for m in made)):
        live = [i for i, m in enumerate(made) if f < len(m[5])]
        k, slot = len(live), f & 1
        pics, keep = (Picture * k)(), []
        for j, i in enumerate(live):
            pics[j], t = upload(made[i][5][f], made[i][2], made[i][3], LAYOUTS[(i + f) % 3], seed=100 * i + f)
            keep.append(t)
        assert lib.hmr_gpu_enc_load_sources_device((C.c_void_p * k)(*[made[i][1] for i in live]), k, (C.c_int * k)(*([slot] * k)), pics, current_stream()) == 0, lib.hmr_gpu_last_error()
        del keep
        if pipelined and prev is not None and prev != live:
            call(prev, None)
        call(live, slot)
        prev = live
        got = ssim_many(lib, [made[i][1] for i in live], [slot] * k, new_sums(k))
        for j, i in enumerate(live):
            assert got[j] == SSIM[BATCH_CASES[i]]["ssim"][f], (BATCH_CASES[i], f)
    if pipelined:
        call(prev, None)
    for i, case in enumerate(BATCH_CASES):
        assert len(streams[i]) == GOLD[case]["stream_bytes"] and hashlib.md5(streams[i]).hexdigest() == GOLD[case]["stream_md5"], case
    for m in made:
        drop(lib, m[0], m[1])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_small_hostile_shapes(gpu, shape, family):
    """one all-intra frame of the family at qp 0; then hostile partner pictures are loaded into the OTHER slot, one after the other, and SSIM is taken against that slot.
    Expected: the oracle, and hmr_gpu_ssim_host, on the pictures downloaded from the device (the final picture and what the slot holds)."""
    import torch
    lib, (w, h) = gpu, shape
    ctx, enc = C.c_void_p(), C.c_void_p()
    assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_create(ctx, C.byref(ec.default_cfg(w, h, qp=0)), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
    pairs = sc.content_pairs(w, h, seed=11)
    source = pairs[f"gen_yuv_{family}"][0]
    planes = [p.tobytes() for p in sc.planes_of(source, w, h)]
    pic, keep = upload(planes, w, h, "offset_i420", seed=1)
    assert lib.hmr_gpu_enc_load_source_device(enc, 0, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    buf, n = C.create_string_buffer(4 << 20), C.c_long()
    assert lib.hmr_gpu_enc_encode_source(enc, 0, 3, buf, len(buf), C.byref(n), None) == 2, lib.hmr_gpu_last_error()
    out = Output(w, h, "tight_i420", seed=2)
    export_one(lib, enc, out, -1, None)
    rec = out.picture()
    own = ssim_one(lib, enc, 0, new_sums())
    assert own == sc.picture_sums(source, rec, w, h) == sc.host_sums(lib, source, rec, w, h), (shape, family)
    inverse = bytes(255 - np.frombuffer(source, np.uint8))
    partners = {"inverse": inverse, "the final picture itself": rec, "noise": pairs["noise_noise"][1], "all 255": pairs["zero_255"][1], "stripes": pairs["stripes_inverse"][0]}
    for k, (name, partner) in enumerate(partners.items()):
        pic, keep = upload([p.tobytes() for p in sc.planes_of(partner, w, h)], w, h, LAYOUTS[k % 3], seed=k)
        assert lib.hmr_gpu_enc_load_source_device(enc, 1, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        held = Output(w, h, "nv12", seed=3)
        assert lib.hmr_gpu_enc_export_source_device(enc, 1, C.byref(held.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        assert held.picture() == partner
        got = ssim_one(lib, enc, 1, new_sums())
        assert got == sc.picture_sums(partner, rec, w, h) == sc.host_sums(lib, partner, rec, w, h, "nv12", "offset_i420"), (shape, family, name)
        if name == "the final picture itself":
            assert got == [sc.ONE * v for v in sc.picture_windows(w, h)]
            assert got[0] > 1 << 32      # (every shape has more than four luma windows)
        if name == "inverse" and family == "noise":
            assert all(v < 0 for v in got), got
    assert ssim_one(lib, enc, 0, new_sums()) == own      # (the slot the frame came from is as it was)
    drop(lib, ctx, enc)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(3840, 2160)])
def test_identity(gpu, shape):
    """an all-zero intra frame; its final picture is exported, loaded back into the other slot, and SSIM against that slot is exactly 2^30 x windows - 5.5e14 in luma"""
    import torch
    lib, (w, h) = gpu, shape
    ctx, enc = C.c_void_p(), C.c_void_p()
    assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_create(ctx, C.byref(ec.default_cfg(w, h, wpp=32)), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
    black, back = torch.zeros(w * h * 3 // 2, dtype=torch.uint8, device="cuda"), torch.full((w * h * 3 // 2,), 0x55, dtype=torch.uint8, device="cuda")
    assert lib.hmr_gpu_enc_load_source_device(enc, 0, C.byref(tight(black, w, h)), current_stream()) == 0, lib.hmr_gpu_last_error()
    buf, n = C.create_string_buffer(w * h * 2), C.c_long()
    assert lib.hmr_gpu_enc_encode_source(enc, 0, 3, buf, len(buf), C.byref(n), None) == 2, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_export_picture_device(enc, C.byref(tight(back, w, h)), -1, None, current_stream()) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_load_source_device(enc, 1, C.byref(tight(back, w, h)), current_stream()) == 0, lib.hmr_gpu_last_error()
    got = ssim_one(lib, enc, 1, new_sums())
    assert got == [sc.ONE * v for v in sc.picture_windows(w, h)] and got[0] == sc.ONE * 959 * 539 > 5e14
    assert ssim(got, w, h) == (1.0, 1.0, 1.0)
    drop(lib, ctx, enc)


def test_chain_sums(gpu):
    """hmr_gpu_enc_encode_chain (three engine objects, three frames per launch): one SSIM call over all objects of each chain; every object holds its own frame's sums"""
    lib, case = gpu, "416x240_eng3_wpp_rows"
    g, s = GOLD[case], SSIM[case]
    w, h, frames, keys = g["width"], g["height"], g["frames"], dict(g["keys"])
    E = keys["engines"]
    cfg = ec.default_cfg(w, h, **keys)
    ctxs, encs = [], []
    for k in range(E):
        ctx, enc = C.c_void_p(), C.c_void_p()
        assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_create_engine(ctx, C.byref(cfg), k, C.byref(enc)) == 0, lib.hmr_gpu_last_error()
        ctxs.append(ctx)
        encs.append(enc)
    clip = ec.clip_frames(w, h, frames)
    for f, planes in enumerate(clip):      # frame f: object f % E, its slot f // E
        pic, keep = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(encs[f % E], f // E, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    bufs = [C.create_string_buffer(1 << 20) for _ in range(E)]
    stream = b""
    for first in range(0, frames, E):
        fs = list(range(first, min(first + E, frames)))
        k = len(fs)
        chain = [encs[f % E] for f in fs]
        got = (C.c_long * k)()
        assert lib.hmr_gpu_enc_encode_chain((C.c_void_p * k)(*chain), k, encs[(first - 1) % E] if first else None, (C.c_int * k)(*[f // E for f in fs]), None,
                                            (C.c_char_p * k)(*[C.cast(bufs[i], C.c_char_p) for i in range(k)]), (C.c_long * k)(*[len(bufs[i]) for i in range(k)]),
                                            got) == 0, lib.hmr_gpu_last_error()
        for i in range(k):
            stream += bufs[i].raw[:got[i]]
        assert ssim_many(lib, chain, [f // E for f in fs], new_sums(k)) == [s["ssim"][f] for f in fs], fs
    for enc in reversed(encs):
        lib.hmr_gpu_enc_destroy(enc)
    for ctx in ctxs:
        lib.hmr_gpu_destroy(ctx)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


def test_ssim_is_ordered_against_the_consumer_stream(gpu):
    """The sums tensor is overwritten on a torch side stream behind so much queued work that the overwrite has not run when the SSIM call returns; that stream is the
    call's consumer stream, and a copy of the sums queued on it right after the call - nothing is synchronised by the test - has to hold the fixture's sums: the kernel
    (and the zeroing in front of it) waited for the consumer's earlier work, and the consumer's later work waited for the kernel.  The next frame is loaded and encoded
    at once."""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    g, s = GOLD[case], SSIM[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    clean = [torch.from_numpy(np.frombuffer(b"".join(planes), np.uint8).copy()).cuda() for planes in clip]
    sums, sums_copies = new_sums(), [new_sums() for _ in clip]
    ballast = torch.ones(1 << 28, dtype=torch.float32, device="cuda")      # 1 GB
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ballast.mul_(1.0)
    torch.cuda.synchronize()      # (set-up is over: from here on nothing waits on the host but the encode calls themselves)
    buf, n, stream, pending = C.create_string_buffer(1 << 20), C.c_long(), b"", []
    for f in range(len(clip)):
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(tight(clean[f], w, h)), current_stream()) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        overwritten = torch.cuda.Event()
        with torch.cuda.stream(side):
            for _ in range(40):
                ballast.mul_(1.0)
            sums.fill_(-1)
            overwritten.record(side)
        assert lib.hmr_gpu_enc_ssim_one_device(enc, f & 1, C.c_void_p(sums.data_ptr()), C.c_void_p(side.cuda_stream)) == 0, lib.hmr_gpu_last_error()
        pending.append(not overwritten.query())
        with torch.cuda.stream(side):
            sums_copies[f].copy_(sums, non_blocking=True)
    torch.cuda.synchronize()
    drop(lib, ctx, enc)
    assert all(pending), f"the sums had already been overwritten when the SSIM call returned (frames {pending}): the test did not exercise the ordering"
    for f in range(len(clip)):
        assert sums_copies[f][0].tolist() == s["ssim"][f], f
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


def test_encoder_class_ssim(gpu):
    case = "416x240"
    cfg, image_type, clip = config_of(case)
    w, h = cfg.width, cfg.height
    with Encoder(cfg) as enc:
        with pytest.raises(RuntimeError):
            enc.ssim()
        stream = b""
        for f, planes in enumerate(clip):
            stream += enc.encode(as_tensors(planes, w, h, f % 3, f), image_type)[0]
            sums = enc.ssim()
            assert sums.is_cuda and sums.dtype.is_floating_point is False and tuple(sums.shape) == (3,)
            assert sums.tolist() == SSIM[case]["ssim"][f], f
            want = tuple(v / (sc.ONE * k) for v, k in zip(SSIM[case]["ssim"][f], SSIM[case]["windows"]))      # (Python's int / int is the correctly rounded quotient)
            assert ssim(sums.tolist(), w, h) == want and all(0 < v < 1 for v in want)
    assert len(stream) == GOLD[case]["stream_bytes"] and hashlib.md5(stream).hexdigest() == GOLD[case]["stream_md5"]


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_encoder_class_ssim(gpu, pipelined):
    made = [config_of(case) for case in BATCH_CASES]
    streams = [b"" for _ in made]
    idle_rows = 0
    with BatchEncoder([m[0] for m in made], pipelined=pipelined) as enc:
        with pytest.raises(RuntimeError):
            enc.ssim()
        for f in range(max(len(m[2]) for m in made)):
            frames = [as_tensors(m[2][f], m[0].width, m[0].height, (i + f) % 3, 100 * i + f) if f < len(m[2]) else None for i, m in enumerate(made)]
            for i, au in enumerate(enc.step(frames, [m[1] for m in made])):
                streams[i] += au
            sums = enc.ssim()      # of the frames just given - in pipelined mode their access units are still outstanding
            assert tuple(sums.shape) == (len(made), 3)
            for i, case in enumerate(BATCH_CASES):
                if frames[i] is None:
                    assert sums[i].tolist() == [IDLE] * 3
                    idle_rows += 1
                else:
                    assert sums[i].tolist() == SSIM[case]["ssim"][f], (case, f)
        for i, au in enumerate(enc.flush()):
            streams[i] += au
    assert idle_rows
    for i, case in enumerate(BATCH_CASES):
        assert len(streams[i]) == GOLD[case]["stream_bytes"] and hashlib.md5(streams[i]).hexdigest() == GOLD[case]["stream_md5"], case


def test_refusals_leave_the_encoder_working(gpu):
    """every refusal of the header's list is HMR_GPU_ERR_ARG with a text, nothing is queued or written, and the encoders then still produce their fixture's stream and
    sums.  (As in the egress test, host pointers and freed tensors are deliberately not tried.)"""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    g, s = GOLD[case], SSIM[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    ctx2, enc2 = make_encoder(lib, case)[:2]
    ctx3, fresh = make_encoder(lib, case)[:2]
    st = current_stream()
    buf, n, stream = C.create_string_buffer(1 << 20), C.c_long(), b""
    src, keep = upload(clip[0], w, h, "tight_i420")
    sums = new_sums(513)
    dev = C.c_void_p(sums.data_ptr())
    for e in (enc, enc2):
        assert lib.hmr_gpu_enc_load_source_device(e, 0, C.byref(src), st) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_encode_source(enc2, 0, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()

    def many(encs, slots, out, n=None):
        k = len(encs)
        rc = lib.hmr_gpu_enc_ssim_device((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*slots) if slots is not None else None, out, st)
        return rc, lib.hmr_gpu_last_error()

    before_first_frame = many([enc], [0], dev)      # (enc has a loaded slot but has not encoded anything)
    assert lib.hmr_gpu_enc_encode_source(enc, 0, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
    stream += buf.raw[:n.value]
    # a picture whose chroma planes have one block row: 72 x 8 is a size the encoder takes (the size is refused before the missing picture is)
    ctx4, low = C.c_void_p(), C.c_void_p()
    assert lib.hmr_gpu_create(C.byref(ctx4), 0, None) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_create(ctx4, C.byref(ec.default_cfg(72, 8)), C.byref(low)) == 0, lib.hmr_gpu_last_error()
    grey = torch.full((72 * 8 * 3 // 2,), 128, dtype=torch.uint8, device="cuda")
    assert lib.hmr_gpu_enc_load_source_device(low, 0, C.byref(tight(grey, 72, 8)), st) == 0, lib.hmr_gpu_last_error()
    refused = {
        "an encoder without an encoded picture": before_first_frame,
        "an encoder without an encoded picture, among others": many([enc, fresh], [0, 0], dev),
        "n = 0": many([enc], [0], dev, n=0),
        "n = 513": many([enc] * 513, [0] * 513, dev),
        "NULL encs": (lib.hmr_gpu_enc_ssim_device(None, 1, (C.c_int * 1)(0), dev, st), lib.hmr_gpu_last_error()),
        "NULL slots": many([enc], None, dev),
        "NULL dev_ssim": many([enc], [0], None),
        "a NULL encoder": many([enc, None], [0, 0], dev),
        "a slot that does not exist": many([enc], [1], dev),
        "a negative slot": many([enc, enc2], [0, -1], dev),
        "height below 16": many([enc, low], [0, 0], dev),
        "NULL encoder (single call)": (lib.hmr_gpu_enc_ssim_one_device(None, 0, dev, st), lib.hmr_gpu_last_error()),
        "NULL dev_ssim (single call)": (lib.hmr_gpu_enc_ssim_one_device(enc, 0, None, st), lib.hmr_gpu_last_error()),
        "height below 16 (single call)": (lib.hmr_gpu_enc_ssim_one_device(low, 0, dev, st), lib.hmr_gpu_last_error()),
    }
    if torch.cuda.device_count() > 1:
        ctx5, enc5 = C.c_void_p(), C.c_void_p()
        assert lib.hmr_gpu_create(C.byref(ctx5), 1, None) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_create(ctx5, C.byref(ec.default_cfg(w, h, wpp=4)), C.byref(enc5)) == 0, lib.hmr_gpu_last_error()
        refused["encoders on different devices"] = many([enc, enc5], [0, 0], dev)
        other = torch.zeros(3, dtype=torch.int64, device="cuda:1")
        refused["dev_ssim on another device"] = many([enc], [0], C.c_void_p(other.data_ptr()))
        drop(lib, ctx5, enc5)
    for why, (rc, text) in refused.items():
        assert rc == ERR_ARG and text, (why, rc, text)
    torch.cuda.synchronize()
    assert sums.min().item() == sums.max().item() == -7      # nothing was written by the refused calls
    rc, text = many([enc, enc], [0, 0], dev)      # the same encoder twice in one call is fine
    assert rc == 0, text
    assert sums[0].tolist() == sums[1].tolist() == s["ssim"][0] and sums[2:].min().item() == sums[2:].max().item() == -7
    for f, planes in enumerate(clip):
        if f == 0:
            continue
        pic, t = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), st) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        assert ssim_one(lib, enc, f & 1, sums) == s["ssim"][f]
    drop(lib, ctx, enc)
    drop(lib, ctx2, enc2)
    drop(lib, ctx3, fresh)
    drop(lib, ctx4, low)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]
