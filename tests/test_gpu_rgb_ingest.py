"""-m gpu: RGB pictures in device memory (include/homer_gpu.h section 12f, k_ingest_rgb in csrc/picture_io.hip, homerhevc_amd/encoder.py).  Every case loads RGB with
hmr_gpu_enc_load_source(s)_rgb_device and reads the slot back with hmr_gpu_enc_export_source(s)_device; the slot must equal the numpy restatement of the section's
arithmetic (tests/rgb_cases.py) exactly - the comparator is the restatement, never the kernel.  End to end, the streams and reconstructions of encoders fed with RGB must be
byte-identical to those of encoders fed, through the existing hmr_gpu_enc_load_sources_device, with the numpy-converted I420 of the same RGB (that the control path is the
reference's is what the unchanged tests of test_gpu_ingest.py show).

What the canaries see: every byte of the RGB buffers (the rows and the random bytes around them) is what it was after the load, and every byte of the export's output
buffers outside the pictures' rows is what it was.  The slots' own planes cannot be read outside width x height through the interface (their stride is the width rounded up
to 8 samples, so a 200- or 328-wide slot has four unused chroma samples a row); that nothing is written there follows from the kernel's spans (whole spans lie inside the
width; the tail writes sample by sample) and is not observed here."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import rgb_cases as rc
from homerhevc_amd.encoder import BatchEncoder, Encoder, Picture, RGBFrame
from picture_gpu import (BATCH_CASES, GOLD, LAYOUTS, Output, as_tensors, config_of, current_stream, drop, first_difference, gpu, make_encoder, new_encoder,  # noqa: F401
                         rgb_frame, slot_picture, upload)
from picture_gpu import RgbSource as Source      # rc.lay_out's buffers uploaded, rc.descriptor over them, rc.restate's picture as `want`
from rgb_scale_cases import chans_of

pytestmark = pytest.mark.gpu
ERR_ARG = -3
FORMS = sorted(rc.FORMS)


@pytest.mark.parametrize("size", [(200, 136), (328, 264), (416, 240), (1920, 1080)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_pictures(gpu, size):
    """every format, order, matrix and range; noise and, for the float formats, whatever a float can hold; two slots in turn; the slot read back as I420 and as NV12"""
    lib, (w, h) = gpu, size
    ctx, enc = new_encoder(lib, w, h)
    rng = np.random.default_rng(w + h)
    k = 0
    for form in FORMS:
        for matrix, full in rc.MATRIX_RANGES:
            if form in rc.FLOAT_TYPES and (k & 1):
                chans = rc.special_floats(rc.FLOAT_TYPES[form], rng, w, h)
            else:
                chans = chans_of(form, rng, *rc.noise(rng, w, h))
            src = Source(form, chans, matrix, full, rng, padded=k % 3 != 2)
            slot = k & 1
            assert lib.hmr_gpu_enc_load_source_rgb_device(enc, slot, C.byref(src.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
            for layout in ("offset_i420", "nv12"):
                got = slot_picture(lib, enc, slot, w, h, layout, seed=k)
                assert got == src.want, (form, matrix, full, layout, first_difference(got, src.want, w, h))
            assert src.untouched(), (form, "the RGB buffers were written")
            k += 1
    drop(lib, ctx, enc)


def test_special_pictures(gpu):
    """the eight corners, a grey ramp and a checkerboard of complementary colours, in every form, several pictures per load call with the forms mixed"""
    lib, (w, h) = gpu, (256, 64)
    rng = np.random.default_rng(9)
    pictures = [[np.full((h, w), 255 * bit, np.uint8) for bit in ((k >> 2) & 1, (k >> 1) & 1, k & 1)] for k in range(8)]
    ramp = np.tile(np.arange(256, dtype=np.uint8), (h, 1))
    pictures.append([ramp, ramp, ramp])
    yy, xx = np.mgrid[0:h, 0:w]
    for cell in (1, 2):
        on = ((yy // cell + xx // cell) & 1).astype(bool)
        pictures.append([np.where(on, c, 255 - c).astype(np.uint8) for c in (255, 0, 17)])
    made = [new_encoder(lib, w, h) for _ in pictures]
    for shift, (matrix, full) in enumerate(rc.MATRIX_RANGES):
        for turn in range(len(FORMS)):
            srcs = [Source(FORMS[(i + turn) % len(FORMS)], chans_of(FORMS[(i + turn) % len(FORMS)], rng, *p), *rc.MATRIX_RANGES[(i + shift) % 4], rng) for i, p in enumerate(pictures)]
            n = len(srcs)
            assert lib.hmr_gpu_enc_load_sources_rgb_device((C.c_void_p * n)(*[m[1] for m in made]), n, (C.c_int * n)(*([turn & 1] * n)), (rc.RgbPicture * n)(*[s.pic for s in srcs]),
                                                           current_stream()) == 0, lib.hmr_gpu_last_error()
            outs = [Output(w, h, LAYOUTS[(i + turn) % 3], seed=i) for i in range(n)]
            assert lib.hmr_gpu_enc_export_sources_device((C.c_void_p * n)(*[m[1] for m in made]), n, (C.c_int * n)(*([turn & 1] * n)), (Picture * n)(*[o.pic for o in outs]),
                                                         current_stream()) == 0, lib.hmr_gpu_last_error()
            for i, (s, o) in enumerate(zip(srcs, outs)):
                got = o.picture()
                assert got == s.want, (i, turn, first_difference(got, s.want, w, h))
    for ctx, enc in made:
        drop(lib, ctx, enc)


def rgb_of_clip(made):
    """per sequence and frame: (form, matrix, full, channel arrays, the numpy-converted I420 planes as bytes)"""
    rng = np.random.default_rng(77)
    table = []
    for i, m in enumerate(made):
        w, h, clip = m[2], m[3], m[5]
        frames = []
        for f, planes in enumerate(clip):
            form, (matrix, full) = FORMS[(i + f) % len(FORMS)], rc.MATRIX_RANGES[(i + 2 * f) % 4]
            chans = chans_of(form, rng, *rc.yuv_to_rgb(planes, w, h))
            frames.append((form, matrix, full, chans, tuple(p.tobytes() for p in rc.restate(*rc.eight_bit(form, chans), matrix, full))))
        table.append(frames)
    return table


@pytest.mark.parametrize("pipelined", [False, True])
def test_end_to_end_against_the_converted_i420(gpu, pipelined):
    """The clips of picture_gpu.BATCH_CASES as RGB: ONE hmr_gpu_enc_load_sources_rgb_device per step for all sequences that still have frames, formats, matrices and
    ranges mixed within the call, then one batch launch.  The control encoders get the numpy-converted I420 through hmr_gpu_enc_load_sources_device.  Streams and exported
    reconstructions are byte-identical, sequence by sequence, and so are the slots."""
    lib = gpu
    made = [make_encoder(lib, case) for case in BATCH_CASES]
    control = [make_encoder(lib, case) for case in BATCH_CASES]
    table = rgb_of_clip(made)
    rng = np.random.default_rng(1)
    streams = {id(made): [b"" for _ in made], id(control): [b"" for _ in made]}
    bufs = {id(made): [C.create_string_buffer(1 << 20) for _ in made], id(control): [C.create_string_buffer(1 << 20) for _ in made]}

    def call(group, live, slot):
        k = len(live)
        got = (C.c_long * k)()
        fn = lib.hmr_gpu_enc_encode_batch_pipelined if pipelined else lib.hmr_gpu_enc_encode_batch
        assert fn((C.c_void_p * k)(*[group[i][1] for i in live]), k, (C.c_int * k)(*([slot] * k)) if slot is not None else None,
                  (C.c_int * k)(*[group[i][4] for i in live]), (C.c_char_p * k)(*[C.cast(bufs[id(group)][i], C.c_char_p) for i in live]), (C.c_long * k)(*[len(bufs[id(group)][i]) for i in live]),
                  got) == 0, lib.hmr_gpu_last_error()
        for j, i in enumerate(live):
            streams[id(group)][i] += C.string_at(bufs[id(group)][i], got[j])

    def pictures(group, live, sources, slot):
        k = len(live)
        outs = [Output(group[i][2], group[i][3], "tight_i420", seed=i) for i in live]
        encs = (C.c_void_p * k)(*[group[i][1] for i in live])
        if sources:
            assert lib.hmr_gpu_enc_export_sources_device(encs, k, (C.c_int * k)(*([slot] * k)), (Picture * k)(*[o.pic for o in outs]), current_stream()) == 0, lib.hmr_gpu_last_error()
        else:
            assert lib.hmr_gpu_enc_export_pictures_device(encs, k, (Picture * k)(*[o.pic for o in outs]), None, None, current_stream()) == 0, lib.hmr_gpu_last_error()
        return [o.picture() for o in outs]

    prev = None
    for f in range(max(len(m[5]) for m in made)):
        live = [i for i, m in enumerate(made) if f < len(m[5])]
        k, slot = len(live), f & 1
        srcs = [Source(table[i][f][0], table[i][f][3], table[i][f][1], table[i][f][2], rng, padded=(i + f) % 3 != 0) for i in live]
        assert lib.hmr_gpu_enc_load_sources_rgb_device((C.c_void_p * k)(*[made[i][1] for i in live]), k, (C.c_int * k)(*([slot] * k)), (rc.RgbPicture * k)(*[s.pic for s in srcs]),
                                                       current_stream()) == 0, lib.hmr_gpu_last_error()
        del srcs
        pics, keep = (Picture * k)(), []
        for j, i in enumerate(live):
            pics[j], t = upload(table[i][f][4], made[i][2], made[i][3], LAYOUTS[(i + f) % 3], seed=100 * i + f)
            keep.append(t)
        assert lib.hmr_gpu_enc_load_sources_device((C.c_void_p * k)(*[control[i][1] for i in live]), k, (C.c_int * k)(*([slot] * k)), pics, current_stream()) == 0, lib.hmr_gpu_last_error()
        del keep
        slots_rgb, slots_yuv = pictures(made, live, True, slot), pictures(control, live, True, slot)
        for j, i in enumerate(live):
            assert slots_rgb[j] == b"".join(table[i][f][4]), (BATCH_CASES[i], f, table[i][f][:3])
            assert slots_yuv[j] == slots_rgb[j], (BATCH_CASES[i], f)
        for group in (made, control):
            if pipelined and prev is not None and prev != live:
                call(group, prev, None)
            call(group, live, slot)
        assert pictures(made, live, False, slot) == pictures(control, live, False, slot), f
        prev = live
    if pipelined:
        call(made, prev, None)
        call(control, prev, None)
    for i, case in enumerate(BATCH_CASES):
        assert len(streams[id(made)][i]) > 0 and streams[id(made)][i] == streams[id(control)][i], case
    for m in made + control:
        drop(lib, m[0], m[1])


def test_ingest_is_ordered_against_the_producer_stream(gpu):
    """The mirror of test_gpu_ingest.py's test: every RGBA picture is produced on a torch side stream behind so much queued work that it does not exist yet when the load call
    returns, and its memory is overwritten on the same stream right after the call; nothing is synchronised before the encode call."""
    import torch
    lib, case = gpu, "416x240_wpp_rows"
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    ctx2, enc2 = make_encoder(lib, case)[:2]
    rng = np.random.default_rng(4)
    rgba, converted = [], []
    for planes in clip:
        r, g, b = rc.yuv_to_rgb(planes, w, h)
        rgba.append(np.stack([r, g, b, rng.integers(0, 256, (h, w), dtype=np.uint8)], axis=2))
        converted.append(tuple(p.tobytes() for p in rc.restate(r, g, b, "bt709", 0)))
    buf, n = C.create_string_buffer(1 << 20), C.c_long()
    expected = b""
    for f, planes in enumerate(converted):      # the control: the converted I420, everything synchronised
        pic, keep = upload(planes, w, h, "tight_i420")
        assert lib.hmr_gpu_enc_load_source_device(enc2, f & 1, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        torch.cuda.synchronize()
        assert lib.hmr_gpu_enc_encode_source(enc2, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        expected += buf.raw[:n.value]
    clean = [torch.from_numpy(p).cuda() for p in rgba]
    staging = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    ballast = torch.ones(1 << 28, dtype=torch.float32, device="cuda")      # 1 GB
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ballast.mul_(1.0)
    torch.cuda.synchronize()      # (set-up is over: from here on nothing waits on the host but the encode calls themselves)
    pic = rc.descriptor(rc.RGB_PACKED8, 4, (0, 1, 2), [staging.data_ptr()], [4 * w], "bt709", 0)
    stream, pending = b"", []
    for f in range(len(clip)):
        produced = torch.cuda.Event()
        with torch.cuda.stream(side):
            for _ in range(40):
                ballast.mul_(1.0)
            staging.copy_(clean[f], non_blocking=True)
            produced.record(side)
        assert lib.hmr_gpu_enc_load_source_rgb_device(enc, f & 1, C.byref(pic), C.c_void_p(side.cuda_stream)) == 0, lib.hmr_gpu_last_error()
        pending.append(not produced.query())
        with torch.cuda.stream(side):
            staging.fill_(0x55)
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
    torch.cuda.synchronize()
    drop(lib, ctx, enc)
    drop(lib, ctx2, enc2)
    assert all(pending), f"the picture was already produced when the load call returned (frames {pending}): the test did not exercise the ordering"
    assert stream == expected


def test_refusals_leave_the_encoder_working(gpu):
    """every argument error the host can see without following a pointer is HMR_GPU_ERR_ARG with a text, nothing is launched, and the encoder still produces its fixture's
    stream"""
    lib, case = gpu, "416x240_wpp_rows"
    g = GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    ctx2, enc2 = make_encoder(lib, case)[:2]
    rng = np.random.default_rng(2)
    good = Source("rgba", rc.noise(rng, w, h), "bt709", 0, rng)
    planar = Source("f32", rc.as_floats("f32", rng, *rc.noise(rng, w, h)), "bt601", 1, rng)
    st = current_stream()

    def many(encs, slots, pics, n=None):
        k = len(encs)
        rc_ = lib.hmr_gpu_enc_load_sources_rgb_device((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*slots), (rc.RgbPicture * k)(*pics), st)
        return rc_, lib.hmr_gpu_last_error()

    def changed(pic, **kw):
        p = rc.RgbPicture.from_buffer_copy(pic)
        for k, v in kw.items():
            if k[-1].isdigit():
                getattr(p, k[:-1])[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return p

    refused = {
        "n = 0": many([enc], [0], [good.pic], n=0),
        "n = 513": many([enc] * 513, list(range(513)), [good.pic] * 513),
        "a NULL encoder": many([enc, None], [0, 0], [good.pic, good.pic]),
        "slot -1": many([enc], [-1], [good.pic]),
        "slot 4097": many([enc], [4097], [good.pic]),
        "the same encoder and slot twice": many([enc, enc2, enc], [1, 1, 1], [good.pic] * 3),
        "unknown format": many([enc], [0], [changed(good.pic, format=4)]),
        "unknown matrix": many([enc], [0], [changed(good.pic, matrix=2)]),
        "full_range 2": many([enc], [0], [changed(planar.pic, full_range=2)]),
        "reserved": many([enc], [0], [changed(good.pic, reserved=1)]),
        "pixel_bytes 5": many([enc], [0], [changed(good.pic, pixel_bytes=5)]),
        "pixel_bytes with a planar format": many([enc], [0], [changed(planar.pic, pixel_bytes=4)]),
        "offset repeated": many([enc], [0], [changed(good.pic, offset2=0)]),
        "offset out of range": many([enc], [0], [changed(good.pic, offset1=4)]),
        "missing plane": many([enc], [0], [changed(planar.pic, plane1=None)]),
        "second plane with PACKED8": many([enc], [0], [changed(good.pic, plane1=good.pic.plane[0])]),
        "pitch below a row": many([enc, enc2], [0, 0], [good.pic, changed(good.pic, pitch0=4 * w - 1)]),
        "negative pitch": many([enc], [0], [changed(planar.pic, pitch2=-4 * w)]),
        "float pitch not element-aligned": many([enc], [0], [changed(planar.pic, pitch0=planar.pic.pitch[0] + 2)]),
        "float plane not element-aligned": many([enc], [0], [changed(planar.pic, plane2=planar.pic.plane[2] + 1)]),
        "NULL picture (single call)": (lib.hmr_gpu_enc_load_source_rgb_device(enc, 0, None, st), lib.hmr_gpu_last_error()),
        "NULL encoder (single call)": (lib.hmr_gpu_enc_load_source_rgb_device(None, 0, C.byref(good.pic), st), lib.hmr_gpu_last_error()),
        "NULL slots": (lib.hmr_gpu_enc_load_sources_rgb_device((C.c_void_p * 1)(enc), 1, None, C.byref(good.pic), st), lib.hmr_gpu_last_error()),
    }
    for why, (rc_, text) in refused.items():
        assert rc_ == ERR_ARG and text, (why, rc_, text)
    # export of a slot: nothing loaded yet - the slot does not exist
    out = Output(w, h, "tight_i420")
    assert lib.hmr_gpu_enc_export_source_device(enc, 0, C.byref(out.pic), st) == ERR_ARG and b"slot" in lib.hmr_gpu_last_error()
    # the same (encoder, slot) is fine in two calls, the same slot number on two encoders in one, and two formats in one
    assert many([enc, enc2], [0, 0], [good.pic, planar.pic])[0] == 0, lib.hmr_gpu_last_error()
    bad = Picture.from_buffer_copy(out.pic)
    bad.pitch[0] = w - 2
    rgb_format = Picture.from_buffer_copy(out.pic)
    rgb_format.format = 2
    export_refused = {
        "slot 1 does not exist": (lib.hmr_gpu_enc_export_source_device(enc, 1, C.byref(out.pic), st), lib.hmr_gpu_last_error()),
        "slot -1": (lib.hmr_gpu_enc_export_source_device(enc, -1, C.byref(out.pic), st), lib.hmr_gpu_last_error()),
        "pitch below a row": (lib.hmr_gpu_enc_export_source_device(enc, 0, C.byref(bad), st), lib.hmr_gpu_last_error()),
        "format 2": (lib.hmr_gpu_enc_export_source_device(enc, 0, C.byref(rgb_format), st), lib.hmr_gpu_last_error()),
        "NULL output": (lib.hmr_gpu_enc_export_source_device(enc, 0, None, st), lib.hmr_gpu_last_error()),
        "NULL encoder": (lib.hmr_gpu_enc_export_source_device(None, 0, C.byref(out.pic), st), lib.hmr_gpu_last_error()),
        "n = 0": (lib.hmr_gpu_enc_export_sources_device((C.c_void_p * 1)(enc), 0, (C.c_int * 1)(0), C.byref(out.pic), st), lib.hmr_gpu_last_error()),
    }
    for why, (rc_, text) in export_refused.items():
        assert rc_ == ERR_ARG and text, (why, rc_, text)
    assert slot_picture(lib, enc, 0, w, h, "nv12") == good.want and slot_picture(lib, enc2, 0, w, h, "offset_i420") == planar.want
    buf, n, stream = C.create_string_buffer(1 << 20), C.c_long(), b""
    for f, planes in enumerate(clip):
        pic, t = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), st) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
    drop(lib, ctx, enc)
    drop(lib, ctx2, enc2)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


# ---- the Python classes ----
TENSOR_FORMS = ["hwc3", "hwc3_bgr_view", "hwc4_rgba", "hwc4_bgra_view", "hwc4_argb", "hwc4_abgr", "chw_u8", "chw_u8_slice", "chw_f16", "chw_f16_view", "chw_f32", "chw_f32_slice"]


def test_encoder_class(gpu):
    """Encoder.encode(RGBFrame) in every tensor form against an Encoder fed with the converted I420; source() is the converted picture, whole or into `out`, I420 or NV12"""
    import torch
    cfg, image_type, clip = config_of("416x240")
    w, h = cfg.width, cfg.height
    rng = np.random.default_rng(6)
    got = want = b""
    with Encoder(cfg) as enc, Encoder(config_of("416x240")[0]) as control:
        with pytest.raises(RuntimeError):
            enc.source()
        for f, planes in enumerate(clip):
            matrix, full = rc.MATRIX_RANGES[f % 4]
            frame, eight = rgb_frame(TENSOR_FORMS[f % len(TENSOR_FORMS)], *rc.yuv_to_rgb(planes, w, h), matrix, full, rng)
            yuv = b"".join(p.tobytes() for p in rc.restate(*eight, matrix, full))
            au, slice_type = enc.encode(frame, image_type)
            got += au
            if f % 2:
                y, uv = enc.source(nv12=True)
                uv = uv.cpu().numpy()
                assert y.cpu().numpy().tobytes() + uv[:, :, 0].tobytes() + uv[:, :, 1].tobytes() == yuv, f
            else:
                out = torch.zeros((h * 3 // 2, w), dtype=torch.uint8, device="cuda")
                assert enc.source(out=out) is out and out.cpu().numpy().tobytes() == yuv, (f, TENSOR_FORMS[f % len(TENSOR_FORMS)])
            want += control.encode(torch.from_numpy(np.frombuffer(yuv, np.uint8).copy()).cuda().view(h * 3 // 2, w), image_type)[0]
            assert control.source().cpu().numpy().tobytes() == yuv
    assert got and got == want
    # every tensor form at least once, whatever the clip's length
    with Encoder(cfg) as enc:
        r, g, b = rc.noise(rng, w, h)
        for k, kind in enumerate(TENSOR_FORMS):
            matrix, full = rc.MATRIX_RANGES[k % 4]
            frame, eight = rgb_frame(kind, r, g, b, matrix, full, rng)
            enc.encode(frame)
            assert enc.source().cpu().numpy().tobytes() == b"".join(p.tobytes() for p in rc.restate(*eight, matrix, full)), kind
        with pytest.raises(ValueError):
            enc.encode(RGBFrame(torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda"), order="rgb"))
        with pytest.raises(ValueError):
            enc.encode(RGBFrame(torch.zeros((3, h, w), dtype=torch.float64, device="cuda")))
        with pytest.raises(ValueError):
            enc.encode(RGBFrame(torch.zeros((3, h, 2 * w), dtype=torch.float32, device="cuda")[:, :, ::2]))


@pytest.mark.parametrize("pipelined", [False, True])
def test_batch_encoder_class(gpu, pipelined):
    """BatchEncoder.step with RGB frames for some sequences and YUV frames (the converted I420 of the same RGB) for others - which is which changes from step to step -
    against a BatchEncoder fed with the converted I420 alone: the same access units; source() returns the converted pictures"""
    made = [config_of(case) for case in BATCH_CASES]
    rng = np.random.default_rng(8)
    out, want = [b"" for _ in made], [b"" for _ in made]
    with BatchEncoder([m[0] for m in made], pipelined=pipelined) as enc, BatchEncoder([config_of(case)[0] for case in BATCH_CASES], pipelined=pipelined) as control:
        for f in range(max(len(m[2]) for m in made)):
            frames, yuv_frames, yuv_bytes = [], [], []
            for i, m in enumerate(made):
                if f >= len(m[2]):
                    frames.append(None), yuv_frames.append(None), yuv_bytes.append(None)
                    continue
                w, h = m[0].width, m[0].height
                matrix, full = rc.MATRIX_RANGES[(i + f) % 4]
                frame, eight = rgb_frame(TENSOR_FORMS[(3 * i + f) % len(TENSOR_FORMS)], *rc.yuv_to_rgb(m[2][f], w, h), matrix, full, rng)
                planes = tuple(p.tobytes() for p in rc.restate(*eight, matrix, full))
                yuv_bytes.append(b"".join(planes))
                yuv_frames.append(as_tensors(planes, w, h, (i + f) % 3, 100 * i + f))
                frames.append(frame if (i + f) % 3 else as_tensors(planes, w, h, f % 3, 100 * i + f))      # a third of the frames as YUV: the step makes two load calls
            assert f or (any(isinstance(x, RGBFrame) for x in frames) and any(x is not None and not isinstance(x, RGBFrame) for x in frames))
            types = [m[1] for m in made]
            for i, au in enumerate(enc.step(frames, types)):
                out[i] += au
            for i, au in enumerate(control.step(yuv_frames, types)):
                want[i] += au
            for i, pic in enumerate(enc.source()):
                assert (pic is None) == (yuv_bytes[i] is None)
                assert pic is None or pic.cpu().numpy().tobytes() == yuv_bytes[i], (BATCH_CASES[i], f)
        for i, au in enumerate(enc.flush()):
            out[i] += au
        for i, au in enumerate(control.flush()):
            want[i] += au
    for i, case in enumerate(BATCH_CASES):
        assert out[i] and out[i] == want[i], case
