"""-m gpu: reconstructed pictures and quality sums left in device memory (include/homer_gpu.h section 12e, csrc/picture_io.hip, homerhevc_amd/encoder.py).  Every
expectation is the compiled reference's: tests/golden/streams.json `recon_md5` for the pictures, tests/golden/quality.json (the sums of squared differences between the
clip and the reference's own reconstruction, and homer_psnr's values of them) for the sums.  The pictures are exported tightly packed, as I420 planes at odd addresses
inside larger buffers and as NV12; every byte of the output buffers outside the pictures' rows has to stay what it was."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import encoder_cases as ec
from homerhevc_amd.encoder import PIC_I420, BatchEncoder, Encoder, Picture, psnr
from picture_gpu import (BATCH_CASES, GOLD, LAYOUTS, Output, as_tensors, config_of, current_stream, drop, export_many, export_one, gpu, make_encoder, new_sums,  # noqa: F401
                         upload)

pytestmark = pytest.mark.gpu
QUALITY = json.load(open(os.path.join(ec.GOLDEN, "quality.json")))
ERR_ARG = -3
PSNR_TOLERANCE = 1e-9          # (tests/test_egress_cpu.py says where it comes from)
CASES = ["200x136", "416x240", "328x264_wpp3", "416x240_wpp_rows", "832x480_wpp_rows", "416x240_scene_cut_wpp_rows", "416x240_cbr400_perf1",
         "832x480_cbr1500_perf1_wpp_rows", "416x240_eng2", "416x240_eng3_wpp_rows", "416x240_flat", "416x240_flat_qp4", "416x240_extremes_qp4", "416x240_chroma",
         "384x192_noise_qp0", "1920x1080_cfg2_wpp_rows", "3840x2160_cfg2_wpp32"]


def numpy_ssd(a, b, w, h):
    d = (np.frombuffer(a, np.uint8).astype(np.int64) - np.frombuffer(b, np.uint8).astype(np.int64)) ** 2
    y, c = w * h, (w // 2) * (h // 2)
    return [int(d[:y].sum()), int(d[y:y + c].sum()), int(d[y + c:].sum())]


@pytest.mark.parametrize("case", CASES)
def test_single_pictures_and_sums(gpu, case):
    """hmr_gpu_enc_load_source_device + hmr_gpu_enc_encode_source + hmr_gpu_enc_export_picture_device, frame by frame, every frame in the three output layouts"""
    lib, g, q = gpu, GOLD[case], QUALITY[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    buf, n, stream = C.create_string_buffer(max(4 << 20, w * h * 2)), C.c_long(), b""
    for f, planes in enumerate(clip):
        pic, keep = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        del keep
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        for layout in LAYOUTS:
            out, sums = Output(w, h, layout, seed=1000 + f), new_sums()
            export_one(lib, enc, out, f & 1, sums)
            assert hashlib.md5(out.picture()).hexdigest() == g["recon_md5"][f], (case, f, layout)
            assert sums[0].tolist() == q["ssd"][f], (case, f, layout)
    drop(lib, ctx, enc)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_pictures_and_sums(gpu, pipelined):
    """sequences of different sizes: one load, one batch launch and ONE export per step for those that still have frames, the three layouts mixed within a call.  Pipelined:
    the export follows its step directly, while that step's access units are still outstanding."""
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
        outs = [Output(made[i][2], made[i][3], LAYOUTS[(i + 2 * f + 1) % 3], seed=7 * i + f) for i in live]
        sums = new_sums(k)
        export_many(lib, [made[i][1] for i in live], outs, [slot] * k, sums)
        for j, i in enumerate(live):
            case = BATCH_CASES[i]
            assert hashlib.md5(outs[j].picture()).hexdigest() == GOLD[case]["recon_md5"][f], (case, f)
            assert sums[j].tolist() == QUALITY[case]["ssd"][f], (case, f)
    if pipelined:
        call(prev, None)
    for i, case in enumerate(BATCH_CASES):
        assert len(streams[i]) == GOLD[case]["stream_bytes"] and hashlib.md5(streams[i]).hexdigest() == GOLD[case]["stream_md5"], case
    for m in made:
        drop(lib, m[0], m[1])


def test_picture_only_sums_only_and_both_agree(gpu):
    """... and the sums against the OTHER slot are numpy's for the picture that slot holds"""
    lib, case = gpu, "416x240_wpp_rows"
    g, q = GOLD[case], QUALITY[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    buf, n = C.create_string_buffer(1 << 20), C.c_long()
    for f, planes in enumerate(clip):
        pic, keep = upload(planes, w, h, "tight_i420")
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        for layout in LAYOUTS:
            only_picture, both, sums_both, sums_only = Output(w, h, layout, seed=f), Output(w, h, layout, seed=f + 50), new_sums(), new_sums()
            export_one(lib, enc, only_picture, -1, None)
            export_one(lib, enc, None, f & 1, sums_only)
            export_one(lib, enc, both, f & 1, sums_both)
            rec = both.picture()
            assert only_picture.picture() == rec and hashlib.md5(rec).hexdigest() == g["recon_md5"][f]
            assert sums_only[0].tolist() == sums_both[0].tolist() == q["ssd"][f]
            if f:
                other = new_sums()
                export_one(lib, enc, None, (f & 1) ^ 1, other)
                assert other[0].tolist() == numpy_ssd(b"".join(clip[f - 1]), rec, w, h)
                assert other[0].tolist() != q["ssd"][f]
    drop(lib, ctx, enc)


def test_sums_beyond_32_bits(gpu):
    """an all-zero 2160p picture is encoded, an all-255 picture is loaded into the second slot and the sums are taken against that slot: about 5.4e11 and 1.3e11"""
    import torch
    lib, w, h = gpu, 3840, 2160
    ctx, enc = C.c_void_p(), C.c_void_p()
    assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
    cfg = ec.default_cfg(w, h, wpp=32)
    assert lib.hmr_gpu_enc_create(ctx, C.byref(cfg), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
    black, white = torch.zeros(w * h * 3 // 2, dtype=torch.uint8, device="cuda"), torch.full((w * h * 3 // 2,), 255, dtype=torch.uint8, device="cuda")
    for slot, t in enumerate((black, white)):
        pic = Picture(format=PIC_I420, reserved=0)
        pic.plane[0], pic.plane[1], pic.plane[2] = t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4
        pic.pitch[0], pic.pitch[1], pic.pitch[2] = w, w // 2, w // 2
        assert lib.hmr_gpu_enc_load_source_device(enc, slot, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    buf, n = C.create_string_buffer(w * h * 2), C.c_long()
    assert lib.hmr_gpu_enc_encode_source(enc, 0, 0, buf, len(buf), C.byref(n), None) == 2, lib.hmr_gpu_last_error()
    out, sums = Output(w, h, "nv12", seed=5), new_sums()
    export_one(lib, enc, out, 1, sums)
    rec = out.picture()
    got = sums[0].tolist()
    assert got == numpy_ssd(bytes([255]) * (w * h * 3 // 2), rec, w, h)
    assert all(s > 1 << 32 for s in got), got
    drop(lib, ctx, enc)


def test_chain_pictures_and_sums(gpu):
    """hmr_gpu_enc_encode_chain (three engine objects, three frames per launch): one export of all objects of each chain; every object holds its own frame's picture"""
    lib, case = gpu, "416x240_eng3_wpp_rows"
    g, q = GOLD[case], QUALITY[case]
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
        outs, sums = [Output(w, h, LAYOUTS[(f + 1) % 3], seed=f) for f in fs], new_sums(k)
        export_many(lib, chain, outs, [f // E for f in fs], sums)
        for j, f in enumerate(fs):
            assert hashlib.md5(outs[j].picture()).hexdigest() == g["recon_md5"][f], f
            assert sums[j].tolist() == q["ssd"][f], f
    for enc in reversed(encs):
        lib.hmr_gpu_enc_destroy(enc)
    for ctx in ctxs:
        lib.hmr_gpu_destroy(ctx)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


def test_egress_is_ordered_against_the_consumer_stream(gpu):
    """The output tensor is overwritten on a torch side stream behind so much queued work that the overwrite has not run when the export call returns; that stream is the
    call's consumer stream, and a copy of the output queued on it right after the call - nothing is synchronised by the test - has to hold the reference's picture: the
    egress waited for the consumer's earlier work, and the consumer's later work waited for the egress.  The next frame is loaded and encoded at once."""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    g, q = GOLD[case], QUALITY[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    clean = [torch.from_numpy(np.frombuffer(b"".join(planes), np.uint8).copy()).cuda() for planes in clip]
    out = torch.zeros(w * h * 3 // 2, dtype=torch.uint8, device="cuda")
    copies = [torch.zeros_like(out) for _ in clip]
    sums, sums_copies = new_sums(), [new_sums() for _ in clip]
    ballast = torch.ones(1 << 28, dtype=torch.float32, device="cuda")      # 1 GB
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ballast.mul_(1.0)
    torch.cuda.synchronize()      # (set-up is over: from here on nothing waits on the host but the encode calls themselves)
    pic = Picture(format=PIC_I420, reserved=0)
    pic.plane[0], pic.plane[1], pic.plane[2] = out.data_ptr(), out.data_ptr() + w * h, out.data_ptr() + w * h * 5 // 4
    pic.pitch[0], pic.pitch[1], pic.pitch[2] = w, w // 2, w // 2
    src = Picture(format=PIC_I420, reserved=0)
    buf, n, stream, pending = C.create_string_buffer(1 << 20), C.c_long(), b"", []
    for f in range(len(clip)):
        base = clean[f].data_ptr()
        src.plane[0], src.plane[1], src.plane[2] = base, base + w * h, base + w * h * 5 // 4
        src.pitch[0], src.pitch[1], src.pitch[2] = w, w // 2, w // 2
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(src), current_stream()) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        overwritten = torch.cuda.Event()
        with torch.cuda.stream(side):
            for _ in range(40):
                ballast.mul_(1.0)
            out.fill_(0x55)
            sums.fill_(-1)
            overwritten.record(side)
        assert lib.hmr_gpu_enc_export_picture_device(enc, C.byref(pic), f & 1, C.c_void_p(sums.data_ptr()), C.c_void_p(side.cuda_stream)) == 0, lib.hmr_gpu_last_error()
        pending.append(not overwritten.query())
        with torch.cuda.stream(side):
            copies[f].copy_(out, non_blocking=True)
            sums_copies[f].copy_(sums, non_blocking=True)
    torch.cuda.synchronize()
    drop(lib, ctx, enc)
    assert all(pending), f"the output had already been overwritten when the export call returned (frames {pending}): the test did not exercise the ordering"
    for f in range(len(clip)):
        assert hashlib.md5(copies[f].cpu().numpy().tobytes()).hexdigest() == g["recon_md5"][f], f
        assert sums_copies[f][0].tolist() == q["ssd"][f], f
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


def gathered(picture):
    """the I420 bytes of what Encoder.export returned: one tensor, or a (y, uv) pair"""
    if isinstance(picture, (tuple, list)) and len(picture) == 2:
        y, uv = (t.cpu().numpy() for t in picture)
        uv = uv.reshape(uv.shape[0], -1)
        return y.tobytes() + uv[:, 0::2].tobytes() + uv[:, 1::2].tobytes()
    if isinstance(picture, (tuple, list)):
        return b"".join(t.cpu().numpy().tobytes() for t in picture)
    return picture.cpu().numpy().tobytes()


def check_psnr(sums, case, f, w, h):
    got = psnr(sums.tolist(), w, h)
    assert sums.tolist() == QUALITY[case]["ssd"][f], (case, f)
    assert all(abs(a - b) <= PSNR_TOLERANCE for a, b in zip(got, QUALITY[case]["psnr"][f])), (case, f, got)


def views(w, h, seed):
    """(y, u, v) views into larger tensors of random bytes, and a function that asserts that those tensors are unchanged outside the views"""
    import torch
    rng = np.random.default_rng(seed)
    bigs, tensors, out = [], [], []
    for rows, cols, pad, left in ((h, w, 13, 1), (h // 2, w // 2, 7, 2), (h // 2, w // 2, 3, 3)):
        big = rng.integers(0, 256, (rows + 2, cols + pad), dtype=np.uint8)
        t = torch.from_numpy(big.copy()).cuda()
        bigs.append(big)
        tensors.append(t)
        out.append(t[1:rows + 1, left:left + cols])

    def untouched_outside():
        for big, t, (rows, cols, pad, left) in zip(bigs, tensors, ((h, w, 13, 1), (h // 2, w // 2, 7, 2), (h // 2, w // 2, 3, 3))):
            after = t.cpu().numpy().copy()
            after[1:rows + 1, left:left + cols] = big[1:rows + 1, left:left + cols]
            assert np.array_equal(after, big)
    return tuple(out), untouched_outside


def test_encoder_class_export(gpu):
    case = "416x240"
    cfg, image_type, clip = config_of(case)
    w, h = cfg.width, cfg.height
    with Encoder(cfg) as enc:
        with pytest.raises(RuntimeError):
            enc.export()
        stream = b""
        for f, planes in enumerate(clip):
            stream += enc.encode(as_tensors(planes, w, h, f % 3, f), image_type)[0]
            picture, sums = enc.export(ssd=True)
            assert tuple(picture.shape) == (h * 3 // 2, w) and picture.is_contiguous() and sums.dtype.is_floating_point is False and tuple(sums.shape) == (3,)
            assert hashlib.md5(gathered(picture)).hexdigest() == GOLD[case]["recon_md5"][f]
            check_psnr(sums, case, f, w, h)
            picture, sums = enc.export(nv12=True)
            assert sums is None and tuple(picture[1].shape) == (h // 2, w // 2, 2)
            assert hashlib.md5(gathered(picture)).hexdigest() == GOLD[case]["recon_md5"][f]
            picture, sums = enc.export(picture=False, ssd=True)
            assert picture is None
            check_psnr(sums, case, f, w, h)
            out, untouched_outside = views(w, h, f)
            picture, sums = enc.export(ssd=True, out=out)
            assert picture is out
            assert hashlib.md5(gathered(out)).hexdigest() == GOLD[case]["recon_md5"][f]
            untouched_outside()
            check_psnr(sums, case, f, w, h)
            with pytest.raises(ValueError):
                enc.export(picture=False, ssd=False)
    assert len(stream) == GOLD[case]["stream_bytes"] and hashlib.md5(stream).hexdigest() == GOLD[case]["stream_md5"]


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_encoder_class_export(gpu, pipelined):
    made = [config_of(case) for case in BATCH_CASES]
    streams = [b"" for _ in made]
    with BatchEncoder([m[0] for m in made], pipelined=pipelined) as enc:
        with pytest.raises(RuntimeError):
            enc.export()
        for f in range(max(len(m[2]) for m in made)):
            frames = [as_tensors(m[2][f], m[0].width, m[0].height, (i + f) % 3, 100 * i + f) if f < len(m[2]) else None for i, m in enumerate(made)]
            for i, au in enumerate(enc.step(frames, [m[1] for m in made])):
                streams[i] += au
            # the pictures of the frames just given - in pipelined mode their access units are still outstanding
            outs, checks = [None] * len(made), [None] * len(made)
            if f % 2:
                for i, m in enumerate(made):
                    if frames[i] is not None:
                        outs[i], checks[i] = views(m[0].width, m[0].height, 10 * i + f)
            pictures, sums = enc.export(ssd=True, out=outs if f % 2 else None, nv12=f % 4 == 2)
            assert tuple(sums.shape) == (len(made), 3)
            for i, (m, case) in enumerate(zip(made, BATCH_CASES)):
                if frames[i] is None:
                    assert pictures[i] is None and sums[i].tolist() == [-1, -1, -1]
                    continue
                assert hashlib.md5(gathered(pictures[i])).hexdigest() == GOLD[case]["recon_md5"][f], (case, f)
                check_psnr(sums[i], case, f, m[0].width, m[0].height)
                if checks[i]:
                    assert pictures[i] is outs[i]
                    checks[i]()
        for i, au in enumerate(enc.flush()):
            streams[i] += au
    for i, case in enumerate(BATCH_CASES):
        assert len(streams[i]) == GOLD[case]["stream_bytes"] and hashlib.md5(streams[i]).hexdigest() == GOLD[case]["stream_md5"], case


def test_refusals_leave_the_encoder_working(gpu):
    """every refusal of the header's list is HMR_GPU_ERR_ARG with a text, nothing is queued, and the encoders then still produce their fixture's stream and pictures.
    (As in the ingest test, host pointers and freed tensors are deliberately not tried.)"""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    g = GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    ctx2, enc2 = make_encoder(lib, case)[:2]
    ctx3, fresh = make_encoder(lib, case)[:2]
    st = current_stream()
    buf, n, stream = C.create_string_buffer(1 << 20), C.c_long(), b""
    src, keep = upload(clip[0], w, h, "tight_i420")
    out, nv, sums = Output(w, h, "tight_i420"), Output(w, h, "nv12"), new_sums(513)
    dev = C.c_void_p(sums.data_ptr())
    for e in (enc, enc2):
        assert lib.hmr_gpu_enc_load_source_device(e, 0, C.byref(src), st) == 0, lib.hmr_gpu_last_error()
    assert lib.hmr_gpu_enc_encode_source(enc2, 0, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()

    def many(encs, pics, slots, ssd, n=None):
        k = len(encs)
        rc = lib.hmr_gpu_enc_export_pictures_device((C.c_void_p * k)(*encs), k if n is None else n, (Picture * k)(*pics) if pics is not None else None,
                                                    (C.c_int * k)(*slots) if slots is not None else None, ssd, st)
        return rc, lib.hmr_gpu_last_error()

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

    before_first_frame = many([enc], [out.pic], [0], dev)      # (enc has a loaded slot but has not encoded anything)
    assert lib.hmr_gpu_enc_encode_source(enc, 0, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
    stream += buf.raw[:n.value]
    refused = {
        "an encoder without an encoded picture": before_first_frame,
        "an encoder without an encoded picture, among others": many([enc, fresh], [out.pic, out.pic], None, None),
        "n = 0": many([enc], [out.pic], [0], dev, n=0),
        "n = 513": many([enc] * 513, [out.pic] * 513, [0] * 513, dev),
        "a NULL encoder": many([enc, None], [out.pic, out.pic], [0, 0], dev),
        "neither pictures nor slots": many([enc], None, None, None),
        "slots without dev_ssd": many([enc], [out.pic], [0], None),
        "dev_ssd without slots": many([enc], [out.pic], None, dev),
        "a slot that does not exist": many([enc], [out.pic], [1], dev),
        "a negative slot": many([enc, enc2], None, [0, -1], dev),
        "unknown format": many([enc], [changed(out.pic, format=7)], None, None),
        "reserved": many([enc], [changed(out.pic, reserved=1)], None, None),
        "missing plane": many([enc], [changed(out.pic, plane1=None)], None, None),
        "third plane with NV12": many([enc], [changed(nv.pic, plane2=out.pic.plane[2])], None, None),
        "pitch below a row": many([enc, enc2], [out.pic, changed(out.pic, pitch0=w - 2)], [0, 0], dev),
        "negative pitch": many([enc], [changed(out.pic, pitch2=-(w // 2))], None, None),
        "NULL encoder (single call)": (lib.hmr_gpu_enc_export_picture_device(None, C.byref(out.pic), -1, None, st), lib.hmr_gpu_last_error()),
        "nothing asked for (single call)": (lib.hmr_gpu_enc_export_picture_device(enc, None, -1, None, st), lib.hmr_gpu_last_error()),
        "sums without a slot (single call)": (lib.hmr_gpu_enc_export_picture_device(enc, C.byref(out.pic), -1, dev, st), lib.hmr_gpu_last_error()),
        "a slot without sums (single call)": (lib.hmr_gpu_enc_export_picture_device(enc, C.byref(out.pic), 0, None, st), lib.hmr_gpu_last_error()),
        "NULL encoders": (lib.hmr_gpu_enc_export_pictures_device(None, 1, C.byref(out.pic), None, None, st), lib.hmr_gpu_last_error()),
    }
    if torch.cuda.device_count() > 1:
        ctx4, enc4 = C.c_void_p(), C.c_void_p()
        assert lib.hmr_gpu_create(C.byref(ctx4), 1, None) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_create(ctx4, C.byref(ec.default_cfg(w, h, wpp=4)), C.byref(enc4)) == 0, lib.hmr_gpu_last_error()
        refused["encoders on different devices"] = many([enc, enc4], [out.pic, out.pic], None, None)
        other = torch.zeros(w * h * 3 // 2, dtype=torch.uint8, device="cuda:1")
        refused["an output plane on another device"] = many([enc], [changed(out.pic, plane1=other.data_ptr())], None, None)
        drop(lib, ctx4, enc4)
    for why, (rc, text) in refused.items():
        assert rc == ERR_ARG and text, (why, rc, text)
    # nothing was written by the refused calls, and the same encoder twice in one call is fine
    assert out.picture() != b"" and sums.min().item() == -7
    out_a, out_b = Output(w, h, "offset_i420", seed=1), Output(w, h, "nv12", seed=2)
    rc, text = many([enc, enc], [out_a.pic, out_b.pic], [0, 0], dev)
    assert rc == 0, text
    assert hashlib.md5(out_a.picture()).hexdigest() == hashlib.md5(out_b.picture()).hexdigest() == g["recon_md5"][0]
    assert sums[0].tolist() == sums[1].tolist() == QUALITY[case]["ssd"][0]
    for f, planes in enumerate(clip):
        if f == 0:
            continue
        pic, t = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), st) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        o = Output(w, h, LAYOUTS[f % 3], seed=f)
        export_one(lib, enc, o, f & 1, sums)
        assert hashlib.md5(o.picture()).hexdigest() == g["recon_md5"][f] and sums[0].tolist() == QUALITY[case]["ssd"][f]
    drop(lib, ctx, enc)
    drop(lib, ctx2, enc2)
    drop(lib, ctx3, fresh)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]
