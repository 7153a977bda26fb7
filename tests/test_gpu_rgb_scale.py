"""-m gpu: a resolution ladder from RGB pictures in device memory (include/homer_gpu.h section 12j, k_rgb_ladder in csrc/picture_io.hip, homerhevc_amd/encoder.py).  Every
case loads larger RGB pictures with hmr_gpu_enc_load_source(s)_scaled_rgb_device and reads the slot back with hmr_gpu_enc_export_source(s)_device; the slot must equal the
composition of the numpy restatements of sections 12f and 12g (tests/rgb_scale_cases.py) exactly - the comparator is the restatement, never the kernel.  End to end, the
access units, sources and quality sums of encoders fed through ScaledRGBFrame must equal those of encoders fed, through the existing load, with the comparator's I420.

What the canaries see: every byte of the source buffers (the rows and the random bytes around them) is what it was after the load, and every byte of the export's output
buffers outside the pictures' rows is what it was.  A padded source buffer ends with its plane's last row: a byte read beyond a row's end is outside the allocation's rows."""
import ctypes as C

import numpy as np
import pytest

import encoder_cases as ec
import picture_gpu
import rgb_cases as rc
import rgb_scale_cases as rs
import scale_cases as sc
from homerhevc_amd.encoder import BatchEncoder, Encoder, EncoderConfig, Picture, RGBFrame, ScaledFrame, ScaledRGBFrame, scaled_rgb_picture_of
from picture_gpu import LAYOUTS, Output, current_stream, drop, first_difference, gpu, new_encoder, slot_picture  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu
ERR_ARG = -3


class Source(picture_gpu.Source):
    """An RGB picture laid out by rc.lay_out, with the descriptor of section 12j"""

    def __init__(self, form, chans, matrix, full, rng, padded=True):
        fmt, pb, offs, planes = rc.lay_out(form, chans, rng, padded)
        super().__init__(planes)
        self.form, self.chans, self.matrix, self.full, (self.h, self.w) = form, chans, matrix, full, chans[0].shape
        self.pic = rs.descriptor(fmt, pb, offs, self.addresses, self.pitches, matrix, full, self.w, self.h)

    def want(self, wd, hd):
        """the I420 picture a wd x hd slot has to hold"""
        return rs.comparator_bytes(self.form, self.chans, self.matrix, self.full, wd, hd)


def load_one(lib, enc, slot, src):
    assert lib.hmr_gpu_enc_load_source_scaled_rgb_device(enc, slot, C.byref(src.pic), current_stream()) == 0, lib.hmr_gpu_last_error()


@pytest.mark.parametrize("pair", rs.GPU_PAIRS, ids=sc.pair_id)
def test_single_pictures(gpu, pair):
    """all nine forms in the padded layout at every size pair, the four matrix / range rows in turn; every form once in the tight layout (spread over the pairs); slots 0
    and 1 in turn; the slot read back as I420 and as NV12"""
    lib, ((ws, hs), (wd, hd)) = gpu, pair
    ctx, enc = new_encoder(lib, wd, hd)
    rng = np.random.default_rng(ws + hd)
    eight = rc.noise(rng, ws, hs)      # the float forms hold values that quantise back to these: one comparator per matrix / range row
    wants = {}
    runs = [(form, True) for form in rs.FORMS] + [(form, False) for k, form in enumerate(rs.FORMS) if k % len(rs.GPU_PAIRS) == rs.GPU_PAIRS.index(pair)]
    for k, (form, padded) in enumerate(runs):
        matrix, full = rc.MATRIX_RANGES[(k + rs.GPU_PAIRS.index(pair)) % 4]
        if (matrix, full) not in wants:
            wants[(matrix, full)] = rs.comparator_bytes("planar8", eight, matrix, full, wd, hd)
        want = wants[(matrix, full)]
        src = Source(form, rs.chans_of(form, rng, *eight), matrix, full, rng, padded)
        slot = k & 1
        load_one(lib, enc, slot, src)
        layout = ("offset_i420", "nv12")[k & 1]
        got = slot_picture(lib, enc, slot, wd, hd, layout, seed=k)
        assert got == want, (pair, form, padded, matrix, full, layout, first_difference(got, want, wd, hd))
        assert src.untouched(), (pair, form, "the source buffers were written")
    drop(lib, ctx, enc)


@pytest.mark.parametrize("form", ["f16", "f32"])
def test_floats_nobody_ordered(gpu, form):
    """NaN, infinities, negatives, values above 1, the exact halves, subnormals: quantised as section 12f says, then averaged"""
    lib, (ws, hs), (wd, hd) = gpu, (400, 272), (200, 136)
    ctx, enc = new_encoder(lib, wd, hd)
    rng = np.random.default_rng(11)
    for k, (matrix, full) in enumerate(rc.MATRIX_RANGES[:2] if form == "f16" else rc.MATRIX_RANGES[2:]):
        src = Source(form, rc.special_floats(rc.FLOAT_TYPES[form], rng, ws, hs), matrix, full, rng, padded=not k)
        load_one(lib, enc, k, src)
        got, want = slot_picture(lib, enc, k, wd, hd, "tight_i420"), src.want(wd, hd)
        assert got == want, (form, matrix, full, first_difference(got, want, wd, hd))
    drop(lib, ctx, enc)


def test_equal_sizes_give_what_the_rgb_load_gives(gpu):
    lib, (w, h) = gpu, (416, 240)
    rng = np.random.default_rng(3)
    made = [new_encoder(lib, w, h) for _ in range(2)]
    eight = rc.noise(rng, w, h)
    for k, form in enumerate(rs.FORMS):
        matrix, full = rc.MATRIX_RANGES[k % 4]
        src = Source(form, rs.chans_of(form, rng, *eight), matrix, full, rng, padded=bool(k % 3))
        load_one(lib, made[0][1], k & 1, src)
        assert lib.hmr_gpu_enc_load_source_rgb_device(made[1][1], k & 1, C.byref(src.pic.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        a, b = slot_picture(lib, made[0][1], k & 1, w, h, "tight_i420"), slot_picture(lib, made[1][1], k & 1, w, h, "tight_i420")
        assert a == b, (form, first_difference(a, b, w, h))
        assert a == b"".join(p.tobytes() for p in rc.restate(*eight, matrix, full)), form
    for ctx, enc in made:
        drop(lib, ctx, enc)


def test_one_call_with_mixed_entries(gpu):
    """eleven entries: five sources of different sizes, forms, matrices and ranges; the first feeds four encoders of four sizes (one at ratio 8, ratios that are no whole
    numbers), the second three (one at its own size)"""
    lib = gpu
    rng = np.random.default_rng(12)
    ladder = [((1600, 1088), "rgba", "bt601", 0, [(200, 136), (416, 240), (832, 480), (400, 272)]),
              ((832, 480), "f16", "bt709", 1, [(416, 240), (328, 264), (832, 480)]),
              ((400, 272), "bgr", "bt601", 1, [(200, 136), (392, 136)]),
              ((330, 266), "f32", "bt709", 0, [(328, 264)]),
              ((416, 480), "planar8", "bt709", 1, [(416, 240)])]
    sources = [Source(form, rs.chans_of(form, rng, *rc.noise(rng, *size)), matrix, full, rng, padded=k != 2) for k, (size, form, matrix, full, _) in enumerate(ladder)]
    entries = [(src, dst) for src, row in zip(sources, ladder) for dst in row[4]]
    wants = [src.want(*dst) for src, dst in entries]
    n = len(entries)
    assert n == 11
    made = [new_encoder(lib, *dst) for _, dst in entries]
    for turn in range(2):      # both slots; the second call finds the slots allocated
        assert lib.hmr_gpu_enc_load_sources_scaled_rgb_device((C.c_void_p * n)(*[m[1] for m in made]), n, (C.c_int * n)(*([turn] * n)), (rs.ScaledRgbPicture * n)(*[s.pic for s, _ in entries]),
                                                              current_stream()) == 0, lib.hmr_gpu_last_error()
        outs = [Output(dst[0], dst[1], LAYOUTS[(i + turn) % 3], seed=i) for i, (_, dst) in enumerate(entries)]
        assert lib.hmr_gpu_enc_export_sources_device((C.c_void_p * n)(*[m[1] for m in made]), n, (C.c_int * n)(*([turn] * n)), (Picture * n)(*[o.pic for o in outs]),
                                                     current_stream()) == 0, lib.hmr_gpu_last_error()
        for i, ((src, dst), o, want) in enumerate(zip(entries, outs, wants)):
            got = o.picture()
            assert got == want, (i, (src.w, src.h), src.form, dst, first_difference(got, want, *dst))
    assert all(s.untouched() for s in sources)
    for ctx, enc in made:
        drop(lib, ctx, enc)


def i420_tensor(data, w, h):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda().view(h * 3 // 2, w)


def as_bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("kind", ["bgra_view", "f16"])
def test_the_composition_on_the_device_fills_the_same_slot(gpu, kind):
    """what the library offered before: the RGBFrame into an encoder of the SOURCE's size, its source(), and that picture as a ScaledFrame into the rung - the rung's
    slot and access unit equal those of a rung given the ScaledRGBFrame directly"""
    import torch
    (ws, hs), (wd, hd) = (400, 272), (200, 136)
    rng = np.random.default_rng(21)
    r, g, b = rc.noise(rng, ws, hs)
    if kind == "f16":
        chans = rc.as_floats("f16", rng, r, g, b)
        frame, form = RGBFrame(torch.from_numpy(np.stack(chans)).cuda(), matrix="bt601", full_range=True), "f16"
    else:
        big = rng.integers(0, 256, (hs + 2, ws + 5, 4), dtype=np.uint8)
        for c, p in zip((2, 1, 0), (r, g, b)):
            big[1:1 + hs, 3:3 + ws, c] = p
        frame, form, chans = RGBFrame(torch.from_numpy(big).cuda()[1:1 + hs, 3:3 + ws], order="bgra", matrix="bt601", full_range=True), "bgra", [r, g, b]
    want = rs.comparator_bytes(form, chans, "bt601", 1, wd, hd)
    with Encoder(EncoderConfig(ws, hs)) as top, Encoder(EncoderConfig(wd, hd)) as rung, Encoder(EncoderConfig(wd, hd)) as direct:
        top.encode(frame)
        composed_au = rung.encode(ScaledFrame(top.source(), ws, hs))[0]
        direct_au = direct.encode(ScaledRGBFrame(frame, ws, hs))[0]
        a, b_ = as_bytes(rung.source()), as_bytes(direct.source())
        assert a == b_, first_difference(b_, a, wd, hd)
        assert b_ == want, first_difference(b_, want, wd, hd)
        assert direct_au and direct_au == composed_au


def rgb_clip(frames=2):
    """an 832 x 480 clip rendered to RGB, and per frame the I420 pictures the 832 x 480 and the 416 x 240 rung have to hold"""
    w, h = 832, 480
    rgb = [rc.yuv_to_rgb(f, w, h) for f in ec.clip_frames(w, h, frames)]
    top = [b"".join(p.tobytes() for p in rc.restate(*p3, "bt709", 0)) for p3 in rgb]
    low = [rs.comparator_bytes("planar8", p3, "bt709", 0, 416, 240) for p3 in rgb]
    return w, h, rgb, top, low


def test_through_the_encoder_class(gpu):
    """Encoder.encode(ScaledRGBFrame): access units, source(), export(ssd=True) and ssim() equal those of a control encoder given the comparator's I420 picture; the
    frames as planar float32 and as packed RGB"""
    import torch
    w, h, rgb, _, low = rgb_clip()
    rng = np.random.default_rng(6)
    got = want = b""
    types = []
    with Encoder(EncoderConfig(416, 240)) as enc, Encoder(EncoderConfig(416, 240)) as control:
        for f, (r, g, b) in enumerate(rgb):
            if f:
                frame = RGBFrame(torch.from_numpy(np.stack([r, g, b], axis=2).copy()).cuda(), order="rgb")
            else:
                frame = RGBFrame(torch.from_numpy(np.stack(rc.as_floats("f32", rng, r, g, b))).cuda())
            au, slice_type = enc.encode(ScaledRGBFrame(frame, w, h))
            got += au
            types.append(slice_type)
            want += control.encode(i420_tensor(low[f], 416, 240))[0]
            assert as_bytes(enc.source()) == as_bytes(control.source()) == low[f], f
            (pa, sa), (pb, sb) = enc.export(ssd=True), control.export(ssd=True)
            assert as_bytes(pa) == as_bytes(pb) and sa.tolist() == sb.tolist(), f      # (the sums are against the SCALED picture)
            assert enc.ssim().tolist() == control.ssim().tolist(), f
            shown, control_shown = enc.export_rgb(source=True), control.export_rgb(source=True)
            assert as_bytes(shown) == as_bytes(control_shown), f
    assert types == [2, 1] and got and got == want


@pytest.mark.parametrize("pipelined", [False, True])
def test_through_the_batch_encoder_class(gpu, pipelined):
    """BatchEncoder.step with the RGBFrame itself for the 832 x 480 rung and a ScaledRGBFrame of it for the 416 x 240 rung - two load calls a step - against a BatchEncoder
    fed with the I420 pictures alone: the same access units, source(), sums and SSIM"""
    import torch
    w, h, rgb, top, low = rgb_clip()
    rungs = [(832, 480), (416, 240)]
    cfgs = lambda: [EncoderConfig(rw, rh, wfpp_num_threads=(rh + 63) // 64) for rw, rh in rungs]      # (a thread per CTU row: the batch schedule at any width)
    got, want = [b"" for _ in rungs], [b"" for _ in rungs]
    with BatchEncoder(cfgs(), pipelined=pipelined) as enc, BatchEncoder(cfgs(), pipelined=pipelined) as control:
        for f, (r, g, b) in enumerate(rgb):
            frame = RGBFrame(torch.from_numpy(np.stack([r, g, b])).cuda()) if f else RGBFrame(torch.from_numpy(np.stack([b, g, r, r], axis=2).copy()).cuda(), order="bgra")
            for i, au in enumerate(enc.step([frame, ScaledRGBFrame(frame, w, h)])):
                got[i] += au
            for i, au in enumerate(control.step([i420_tensor(top[f], 832, 480), i420_tensor(low[f], 416, 240)])):
                want[i] += au
            for i, (a, b_) in enumerate(zip(enc.source(), control.source())):
                assert as_bytes(a) == as_bytes(b_) == (top[f], low[f])[i], (f, i)
            (pa, sa), (pb, sb) = enc.export(ssd=True), control.export(ssd=True)
            assert sa.tolist() == sb.tolist() and enc.ssim().tolist() == control.ssim().tolist(), f
            for i, (a, b_) in enumerate(zip(pa, pb)):
                assert as_bytes(a) == as_bytes(b_), (f, i)
        for i, au in enumerate(enc.flush()):
            got[i] += au
        for i, au in enumerate(control.flush()):
            want[i] += au
    for i in range(len(rungs)):
        assert got[i] and got[i] == want[i], rungs[i]


def test_a_crop_is_just_a_view(gpu):
    """a [:, y0 : y0 + h, x0 : x0 + w] view of a larger float tensor and a row / column slice of a packed tensor as sources, through scaled_rgb_picture_of"""
    import torch
    lib, (ws, hs), (wd, hd) = gpu, (300, 204), (200, 136)
    ctx, enc = new_encoder(lib, wd, hd)
    rng = np.random.default_rng(17)
    planar = rng.random((3, hs + 37, ws + 51), dtype=np.float32) * 1.2 - 0.1
    packed = rng.integers(0, 256, (hs + 9, ws + 14, 4), dtype=np.uint8)
    y0, x0 = 21, 33      # (odd offsets: the view's rows start at any element)
    cases = [(RGBFrame(torch.from_numpy(planar).cuda()[:, y0:y0 + hs, x0:x0 + ws], matrix="bt709", full_range=True), "f32", list(planar[:, y0:y0 + hs, x0:x0 + ws]), "bt709", 1),
             (RGBFrame(torch.from_numpy(packed).cuda()[5:5 + hs, 7:7 + ws], order="argb", matrix="bt601"), "argb", [packed[5:5 + hs, 7:7 + ws, c] for c in (1, 2, 3)], "bt601", 0)]
    for k, (frame, form, chans, matrix, full) in enumerate(cases):
        assert not frame.tensor.is_contiguous()
        pic, keep = scaled_rgb_picture_of(ScaledRGBFrame(frame, ws, hs))
        assert lib.hmr_gpu_enc_load_source_scaled_rgb_device(enc, k, C.byref(rs.ScaledRgbPicture.from_buffer_copy(pic)), current_stream()) == 0, lib.hmr_gpu_last_error()
        got, want = slot_picture(lib, enc, k, wd, hd, "nv12"), rs.comparator_bytes(form, chans, matrix, full, wd, hd)
        assert got == want, (form, first_difference(got, want, wd, hd))
        del keep
    drop(lib, ctx, enc)


def test_load_is_ordered_against_the_producer_stream(gpu):
    """The source tensor is written on torch's stream just before the load call and overwritten right after it returns, with no host synchronisation in between: the
    slot holds the first content's picture (the load waited for the producer, the producer's next work waited for the kernel)."""
    import torch
    lib, (ws, hs), (wd, hd) = gpu, (1920, 1080), (416, 240)
    ctx, enc = new_encoder(lib, wd, hd)
    rng = np.random.default_rng(8)
    r, g, b = rc.noise(rng, ws, hs)
    first = torch.from_numpy(np.stack([r, g, b, r], axis=2).copy()).cuda()
    staging = torch.zeros_like(first)
    pic = rs.descriptor(rc.RGB_PACKED8, 4, (0, 1, 2), [staging.data_ptr()], [4 * ws], "bt709", 0, ws, hs)
    assert lib.hmr_gpu_enc_load_source_scaled_rgb_device(enc, 0, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()      # (allocates the slot: the only host wait)
    torch.cuda.synchronize()
    staging.copy_(first, non_blocking=True)
    assert lib.hmr_gpu_enc_load_source_scaled_rgb_device(enc, 0, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    staging.fill_(0x55)
    got = slot_picture(lib, enc, 0, wd, hd, "tight_i420")
    drop(lib, ctx, enc)
    want = rs.comparator_bytes("rgba", [r, g, b], "bt709", 0, wd, hd)
    assert got == want, first_difference(got, want, wd, hd)


def test_refusals_leave_the_encoders_working(gpu):
    """each refusal is HMR_GPU_ERR_ARG with a text before anything is queued; after EACH of them the same encoders take a good call and hold the right pictures"""
    lib = gpu
    rng = np.random.default_rng(2)
    ctx, enc = new_encoder(lib, 200, 136)
    ctx2, enc2 = new_encoder(lib, 200, 136)
    good = Source("rgba", rc.noise(rng, 400, 272), "bt709", 0, rng)
    other = Source("f32", rc.as_floats("f32", rng, *rc.noise(rng, 300, 204)), "bt601", 1, rng)
    small = Source("planar8", rc.noise(rng, 192, 128), "bt709", 0, rng)
    nine = Source("planar8", rc.noise(rng, 1800, 1224), "bt709", 0, rng, padded=False)
    want, want2 = good.want(200, 136), other.want(200, 136)
    st = current_stream()

    def many(encs, slots, pics, n=None):
        k = len(encs)
        rc_ = lib.hmr_gpu_enc_load_sources_scaled_rgb_device((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*slots), (rs.ScaledRgbPicture * k)(*pics), st)
        return rc_, lib.hmr_gpu_last_error()

    def changed(pic, **kw):
        p = rs.ScaledRgbPicture.from_buffer_copy(pic)
        for k, v in kw.items():
            if k[-1].isdigit():
                getattr(p.pic, k[:-1])[int(k[-1])] = v
            elif k in ("width", "height"):
                setattr(p, k, v)
            else:
                setattr(p.pic, k, v)
        return p

    host = np.zeros(400 * 272 * 4, np.uint8)
    refusals = {
        "n = 0": (lambda: many([enc], [0], [good.pic], n=0), b""),
        "a host pointer as a plane": (lambda: many([enc], [0], [changed(good.pic, plane0=host.ctypes.data)]), b"plane[0]"),
        "upscale": (lambda: many([enc], [0], [small.pic]), b"dst_w"),
        "ratio 9": (lambda: many([enc], [0], [nine.pic]), b"src_w"),
        "the same (encoder, slot) twice": (lambda: many([enc, enc2, enc], [1, 1, 1], [good.pic] * 3), b"twice"),
        "a pitch too narrow for the SOURCE width": (lambda: many([enc, enc2], [0, 0], [good.pic, changed(good.pic, pitch0=4 * 400 - 1)]), b"pitch[0]"),
        "an unknown matrix": (lambda: many([enc], [0], [changed(good.pic, matrix=2)]), b"matrix"),
        "an odd source width": (lambda: many([enc], [0], [changed(good.pic, width=399)]), b"width"),
        "a NULL encoder": (lambda: many([enc, None], [0, 0], [good.pic, good.pic]), b""),
        "NULL picture (single call)": (lambda: (lib.hmr_gpu_enc_load_source_scaled_rgb_device(enc, 0, None, st), lib.hmr_gpu_last_error()), b""),
    }
    for k, (why, (call, field)) in enumerate(refusals.items()):
        rc_, text = call()
        assert rc_ == ERR_ARG and text and field in text, (why, rc_, text)
        # the same source twice in one call is the ladder; the same slot number on two encoders is fine
        pics = [good.pic, other.pic] if k & 1 else [good.pic, good.pic]
        assert many([enc, enc2], [k & 1, k & 1], pics)[0] == 0, (why, lib.hmr_gpu_last_error())
        got, got2 = slot_picture(lib, enc, k & 1, 200, 136, "nv12"), slot_picture(lib, enc2, k & 1, 200, 136, "offset_i420")
        assert got == want, (why, first_difference(got, want, 200, 136))
        assert got2 == (want2 if k & 1 else want), why
    buf, n = C.create_string_buffer(1 << 20), C.c_long()
    assert lib.hmr_gpu_enc_encode_source(enc, 0, 0, buf, len(buf), C.byref(n), None) == 2 and n.value > 0, lib.hmr_gpu_last_error()
    drop(lib, ctx, enc)
    drop(lib, ctx2, enc2)
