"""-m gpu: pictures that are already in device memory (include/homer_gpu.h section 12d, csrc/picture_io.hip, homerhevc_amd/encoder.py).  The clips of the reference's
fixtures are uploaded with torch - tightly packed I420, I420 planes at odd addresses inside larger tensors, NV12 - and go into the encoders' picture slots by the ingest
kernel; every stream and every reconstructed picture must be what the compiled reference produced (tests/golden/streams.json)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import encoder_cases as ec
from homerhevc_amd.encoder import PIC_I420, BatchEncoder, Encoder, Picture
from picture_gpu import BATCH_CASES, GOLD, LAYOUTS, as_tensors, config_of, current_stream, drop, gpu, make_encoder, upload  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu
ERR_ARG = -3


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", ["200x136", "328x264_wpp3", "392x136_qp22_clip931814", "416x240_scene_cut", "416x240_cbr400_perf1", "416x240_extremes", "416x240_noise_qp4",
                                  "1920x1080_cfg2"])
def test_single_pictures_from_device_memory(gpu, case, layout):
    """hmr_gpu_enc_load_source_device + hmr_gpu_enc_encode_source, two slots in turn: the reference's stream and reconstructed pictures"""
    lib, g = gpu, GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    buf, rec, n = C.create_string_buffer(4 << 20), C.create_string_buffer(w * h * 3 // 2), C.c_long()
    stream, recon = b"", []
    for f, planes in enumerate(clip):
        pic, keep = upload(planes, w, h, layout, seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        del keep      # (torch may hand the memory on: whatever it queues on its stream runs behind the ingest)
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), rec) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
        recon.append(hashlib.md5(rec.raw).hexdigest())
    drop(lib, ctx, enc)
    assert recon == g["recon_md5"], [f for f in range(len(recon)) if recon[f] != g["recon_md5"][f]]
    assert len(stream) == g["stream_bytes"]
    assert hashlib.md5(stream).hexdigest() == g["stream_md5"]


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_from_device_memory(gpu, pipelined):
    """ONE hmr_gpu_enc_load_sources_device per step for all sequences that still have frames - the three layouts mixed within the call - then one batch launch.  Pipelined:
    two slots in turn, each written again while the access units of the call before are still to be delivered."""
    lib = gpu
    made = [make_encoder(lib, case) for case in BATCH_CASES]
    bufs = [C.create_string_buffer(1 << 20) for _ in made]
    out = [b"" for _ in made]

    def call(live, slot):
        k = len(live)
        got = (C.c_long * k)()
        fn = lib.hmr_gpu_enc_encode_batch_pipelined if pipelined else lib.hmr_gpu_enc_encode_batch
        assert fn((C.c_void_p * k)(*[made[i][1] for i in live]), k, (C.c_int * k)(*([slot] * k)) if slot is not None else None,
                  (C.c_int * k)(*[made[i][4] for i in live]), (C.c_char_p * k)(*[C.cast(bufs[i], C.c_char_p) for i in live]), (C.c_long * k)(*[len(bufs[i]) for i in live]),
                  got) == 0, lib.hmr_gpu_last_error()
        for j, i in enumerate(live):
            out[i] += C.string_at(bufs[i], got[j])

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
            call(prev, None)      # (the encoder list changes: flush with the previous one)
        call(live, slot)
        prev = live
    if pipelined:
        call(prev, None)
    for i, case in enumerate(BATCH_CASES):
        assert len(out[i]) == GOLD[case]["stream_bytes"] and hashlib.md5(out[i]).hexdigest() == GOLD[case]["stream_md5"], case
    for m in made:
        drop(lib, m[0], m[1])


def test_ingest_is_ordered_against_the_producer_stream(gpu):
    """Every picture is produced on a torch side stream behind so much queued work that it does not exist yet when the load call returns, and its memory is overwritten
    on the same stream right after the call; nothing is synchronised before the encode call.  The stream is the fixture's only if the ingest waited for the producer and
    the producer's next work waited for the ingest."""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    g = GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    clean = [torch.from_numpy(np.frombuffer(b"".join(planes), np.uint8).copy()).cuda() for planes in clip]
    staging = torch.zeros(w * h * 3 // 2, dtype=torch.uint8, device="cuda")
    ballast = torch.ones(1 << 28, dtype=torch.float32, device="cuda")      # 1 GB
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ballast.mul_(1.0)
    torch.cuda.synchronize()      # (set-up is over: from here on nothing waits on the host but the encode calls themselves)
    pic = Picture(format=PIC_I420, reserved=0)
    pic.plane[0], pic.plane[1], pic.plane[2] = staging.data_ptr(), staging.data_ptr() + w * h, staging.data_ptr() + w * h * 5 // 4
    pic.pitch[0], pic.pitch[1], pic.pitch[2] = w, w // 2, w // 2
    buf, n, stream, pending = C.create_string_buffer(1 << 20), C.c_long(), b"", []
    for f in range(len(clip)):
        produced = torch.cuda.Event()
        with torch.cuda.stream(side):
            for _ in range(40):
                ballast.mul_(1.0)
            staging.copy_(clean[f], non_blocking=True)
            produced.record(side)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), C.c_void_p(side.cuda_stream)) == 0, lib.hmr_gpu_last_error()
        pending.append(not produced.query())
        with torch.cuda.stream(side):
            staging.fill_(0x55)
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
    torch.cuda.synchronize()
    drop(lib, ctx, enc)
    assert all(pending), f"the picture was already produced when the load call returned (frames {pending}): the test did not exercise the ordering"
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


@pytest.mark.parametrize("case", ["416x240", "416x240_force_intra"])
def test_encoder_class(gpu, case):
    cfg, image_type, clip = config_of(case)
    stream, types = b"", []
    with Encoder(cfg) as enc:
        for f, planes in enumerate(clip):
            au, slice_type = enc.encode(as_tensors(planes, cfg.width, cfg.height, f % 3, f), image_type)
            stream += au
            types.append(slice_type)
    assert types[0] == 2 and set(types) <= {1, 2} and (image_type != 3 or set(types) == {2})
    assert len(stream) == GOLD[case]["stream_bytes"] and hashlib.md5(stream).hexdigest() == GOLD[case]["stream_md5"]


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_encoder_class(gpu, pipelined):
    made = [config_of(case) for case in BATCH_CASES]
    out = [b"" for _ in made]
    with BatchEncoder([m[0] for m in made], pipelined=pipelined) as enc:
        for f in range(max(len(m[2]) for m in made)):
            frames = [as_tensors(m[2][f], m[0].width, m[0].height, (i + f) % 3, 100 * i + f) if f < len(m[2]) else None for i, m in enumerate(made)]
            aus = enc.step(frames, [m[1] for m in made])
            if pipelined and f == 0:
                assert not any(aus)      # (late delivery: nothing yet)
            for i, au in enumerate(aus):
                out[i] += au
        for i, au in enumerate(enc.flush()):
            assert pipelined or not au
            out[i] += au
    for i, case in enumerate(BATCH_CASES):
        assert len(out[i]) == GOLD[case]["stream_bytes"] and hashlib.md5(out[i]).hexdigest() == GOLD[case]["stream_md5"], case


def test_refusals_leave_the_encoder_working(gpu):
    """every argument error the host can see without following a pointer is HMR_GPU_ERR_ARG with a text, nothing is launched, and the encoder still produces its fixture's
    stream.  (Host pointers and freed tensors are deliberately not tried: see the pointer-attribute check in csrc/k_encode_picture_io.inc.)"""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    g = GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    ctx2, enc2 = make_encoder(lib, case)[:2]
    good, keep = upload(clip[0], w, h, "tight_i420")
    nv, keep_nv = upload(clip[0], w, h, "nv12")
    st = current_stream()

    def many(encs, slots, pics, n=None):
        k = len(encs)
        rc = lib.hmr_gpu_enc_load_sources_device((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*slots), (Picture * k)(*pics), st)
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

    refused = {
        "n = 0": many([enc], [0], [good], n=0),
        "n = 513": many([enc] * 513, list(range(513)), [good] * 513),
        "a NULL encoder": many([enc, None], [0, 0], [good, good]),
        "slot -1": many([enc], [-1], [good]),
        "slot 4097": many([enc], [4097], [good]),
        "the same encoder and slot twice": many([enc, enc2, enc], [1, 1, 1], [good, good, good]),
        "unknown format": many([enc], [0], [changed(good, format=7)]),
        "reserved": many([enc], [0], [changed(good, reserved=1)]),
        "missing plane": many([enc], [0], [changed(good, plane1=None)]),
        "third plane with NV12": many([enc], [0], [changed(nv, plane2=good.plane[2])]),
        "pitch below a row": many([enc, enc2], [0, 0], [good, changed(good, pitch0=w - 2)]),
        "negative pitch": many([enc], [0], [changed(good, pitch2=-(w // 2))]),
        "NULL picture (single call)": (lib.hmr_gpu_enc_load_source_device(enc, 0, None, st), lib.hmr_gpu_last_error()),
        "NULL encoder (single call)": (lib.hmr_gpu_enc_load_source_device(None, 0, C.byref(good), st), lib.hmr_gpu_last_error()),
        "NULL slots": (lib.hmr_gpu_enc_load_sources_device((C.c_void_p * 1)(enc), 1, None, C.byref(good), st), lib.hmr_gpu_last_error()),
    }
    if torch.cuda.device_count() > 1:
        ctx3, enc3 = C.c_void_p(), C.c_void_p()
        assert lib.hmr_gpu_create(C.byref(ctx3), 1, None) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_create(ctx3, C.byref(ec.default_cfg(w, h, wpp=4)), C.byref(enc3)) == 0, lib.hmr_gpu_last_error()
        refused["encoders on different devices"] = many([enc, enc3], [0, 0], [good, good])
        drop(lib, ctx3, enc3)
    for why, (rc, text) in refused.items():
        assert rc == ERR_ARG and text, (why, rc, text)
    # the same (encoder, slot) is fine in two calls, and the same slot number on two encoders in one
    assert many([enc, enc2], [0, 0], [good, nv])[0] == 0, lib.hmr_gpu_last_error()
    buf, n, stream = C.create_string_buffer(1 << 20), C.c_long(), b""
    for f, planes in enumerate(clip):
        pic, t = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), st) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
    drop(lib, ctx, enc)
    drop(lib, ctx2, enc2)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]
