"""-m gpu: a resolution ladder from Y'CbCr pictures of 8 .. 16 bits, 4:2:0 / 4:2:2 / 4:4:4, planar, semi-planar or packed, in device memory (include/homer_gpu.h section
12l, k_yuv_ladder in csrc/picture_io.hip, homerhevc_amd/encoder.py).  Every case loads larger pictures with hmr_gpu_enc_load_source(s)_scaled_yuv and reads the slot back
with hmr_gpu_enc_export_source(s)_device; the slot must equal the composition of the numpy restatements of sections 12k and 12g (tests/yuv_scale_cases.py) exactly - the
comparator is the restatement, never the kernel.  End to end, the access units and sources of encoders fed through ScaledYUVFrame must equal those of encoders fed,
through the existing load, with the comparator's I420, and the slot must equal what the three launches YUVFrame -> source() -> ScaledFrame leave.

What the canaries see: every byte of the source buffers (the rows and the random bytes around them) is what it was after the load, and every byte of the export's output
buffers outside the pictures' rows is what it was.  A padded source buffer ends with its plane's last row: a byte read beyond a row's end is outside the allocation's rows."""
import ctypes as C

import numpy as np
import pytest

import encoder_cases as ec
import picture_gpu
import rgb_cases as rc
import scale_cases as sc
import yuv_cases as yc
import yuv_scale_cases as ys
from homerhevc_amd.encoder import BatchEncoder, Encoder, EncoderConfig, Picture, RGBFrame, ScaledFrame, ScaledYUVFrame, YUVFrame
from picture_gpu import LAYOUTS, Output, as_tensors, current_stream, drop, first_difference, new_encoder, slot_picture

pytestmark = pytest.mark.gpu
ERR_ARG = -3


@pytest.fixture(scope="module")
def gpu():
    """picture_gpu's one handle, with section 12l's three functions declared on it (its table stops at 12k; ys.declare touches only its own names)"""
    return ys.declare(picture_gpu.load())


class Source(picture_gpu.Source):
    """A picture laid out by yc.lay_out (sample-aligned base addresses), with the descriptor of section 12l"""

    def __init__(self, form, planes3, rng, padded=True):
        super().__init__(yc.lay_out(form, *planes3, rng, padded))
        self.form, self.planes3, (self.h, self.w) = form, planes3, planes3[0].shape
        self.pic = ys.descriptor(form, self.addresses, self.pitches, self.w, self.h)

    def want(self, wd, hd):
        """the I420 picture a wd x hd slot has to hold"""
        return ys.comparator_bytes(self.form, *self.planes3, wd, hd)


def load_one(lib, enc, slot, src):
    assert lib.hmr_gpu_enc_load_source_scaled_yuv(enc, slot, C.byref(src.pic), current_stream()) == 0, lib.hmr_gpu_last_error()


def test_the_runs_cover_every_form_and_every_class_in_both_layouts():
    runs = [run for pair in ys.GPU_PAIRS for run in ys.gpu_runs(pair)]
    assert {form for form, _ in runs} == set(yc.NAMES)
    assert sorted(ys.class_of(form) for form, padded in runs if not padded) == sorted(ys.class_of(form) for form in ys.CLASSES)
    assert all([(form, True) for form in ys.CLASSES] == ys.gpu_runs(pair)[:14] for pair in ys.GPU_PAIRS)


@pytest.mark.parametrize("pair", ys.GPU_PAIRS, ids=sc.pair_id)
def test_single_pictures(gpu, pair):
    """the 14 class forms in the padded layout at every size pair, the other 36 forms and each class's tight layout dealt over the pairs (ys.gpu_runs); noise over the
    container's range; slots 0 and 1 in turn; the slot read back as I420 and as NV12"""
    lib, ((ws, hs), (wd, hd)) = gpu, pair
    ctx, enc = new_encoder(lib, wd, hd)
    rng = np.random.default_rng(ws + hd)
    for k, (form, padded) in enumerate(ys.gpu_runs(pair)):
        src = Source(form, yc.noise(form, rng, ws, hs), rng, padded)
        slot = k & 1
        load_one(lib, enc, slot, src)
        layout = ("offset_i420", "nv12")[(k >> 1) & 1]
        got, want = slot_picture(lib, enc, slot, wd, hd, layout, seed=k), src.want(wd, hd)
        assert got == want, (pair, form, padded, layout, first_difference(got, want, wd, hd))
        assert src.untouched(), (pair, form, "the source buffers were written")
    drop(lib, ctx, enc)


def test_equal_sizes_give_what_the_yuv_load_gives(gpu):
    lib, (w, h) = gpu, (416, 240)
    rng = np.random.default_rng(3)
    made = [new_encoder(lib, w, h) for _ in range(2)]
    for k, form in enumerate(ys.CLASSES):
        planes3 = yc.noise(form, rng, w, h)
        src = Source(form, planes3, rng, padded=bool(k % 3))
        load_one(lib, made[0][1], k & 1, src)
        assert lib.hmr_gpu_enc_load_source_yuv_device(made[1][1], k & 1, C.byref(src.pic.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        a, b = slot_picture(lib, made[0][1], k & 1, w, h, "tight_i420"), slot_picture(lib, made[1][1], k & 1, w, h, "tight_i420")
        assert a == b, (form, first_difference(a, b, w, h))
        assert a == b"".join(p.tobytes() for p in yc.restate(form, *planes3)), form
    for ctx, enc in made:
        drop(lib, ctx, enc)


def test_one_call_with_mixed_entries(gpu):
    """twelve entries: five sources of different sizes, forms and depths; the first feeds four encoders of four sizes (one at ratio 8, ratios that are no whole numbers),
    the second three (one at its own size); both slots in turn"""
    lib = gpu
    rng = np.random.default_rng(12)
    ladder = [((1600, 1088), "semi_uv_420_10msb", [(200, 136), (416, 240), (832, 480), (400, 272)]),
              ((832, 480), "planar_422_10", [(416, 240), (328, 264), (832, 480)]),
              ((400, 272), "uyvy_8", [(200, 136), (392, 136)]),
              ((330, 266), "planar_444_16", [(328, 264)]),
              ((416, 480), "y210", [(416, 240), (208, 136)])]
    sources = [Source(form, yc.noise(form, rng, *size), rng, padded=k != 2) for k, (size, form, _) in enumerate(ladder)]
    entries = [(src, dst) for src, row in zip(sources, ladder) for dst in row[2]]
    wants = [src.want(*dst) for src, dst in entries]
    n = len(entries)
    assert n == 12
    made = [new_encoder(lib, *dst) for _, dst in entries]
    for turn in range(2):      # both slots; the second call finds the slots allocated
        assert lib.hmr_gpu_enc_load_sources_scaled_yuv((C.c_void_p * n)(*[m[1] for m in made]), n, (C.c_int * n)(*([turn] * n)), (ys.ScaledYuvPicture * n)(*[s.pic for s, _ in entries]),
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


def test_refusals_leave_the_encoders_working(gpu):
    """each refusal is HMR_GPU_ERR_ARG with a text before anything is queued; after EACH of them the same encoders take a good call and hold the right pictures"""
    lib = gpu
    rng = np.random.default_rng(2)
    ctx, enc = new_encoder(lib, 200, 136)
    ctx2, enc2 = new_encoder(lib, 200, 136)
    good = Source("semi_uv_420_10msb", yc.noise("semi_uv_420_10msb", rng, 400, 272), rng)
    other = Source("planar_444_12", yc.noise("planar_444_12", rng, 300, 204), rng)
    small = Source("planar_420_8", yc.noise("planar_420_8", rng, 192, 128), rng)
    nine = Source("yuyv_8", yc.noise("yuyv_8", rng, 1800, 1224), rng, padded=False)
    want, want2 = good.want(200, 136), other.want(200, 136)
    st = current_stream()

    def many(encs, slots, pics, n=None):
        k = len(encs)
        rc_ = lib.hmr_gpu_enc_load_sources_scaled_yuv((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*slots), (ys.ScaledYuvPicture * k)(*pics), st)
        return rc_, lib.hmr_gpu_last_error()

    def changed(pic, **kw):
        p = ys.ScaledYuvPicture.from_buffer_copy(pic)
        for k, v in kw.items():
            if k[-1].isdigit():
                getattr(p.pic, k[:-1])[int(k[-1])] = v
            elif k in ("width", "height"):
                setattr(p, k, v)
            else:
                setattr(p.pic, k, v)
        return p

    host = np.zeros(2 * 400 * 272 + 64, np.uint8)
    refusals = {
        "n = 0": (lambda: many([enc], [0], [good.pic], n=0), b""),
        "a host pointer as a plane": (lambda: many([enc], [0], [changed(good.pic, plane1=host.ctypes.data)]), b"plane[1]"),
        "an encoder larger than its source": (lambda: many([enc], [0], [small.pic]), b"dst_w"),
        "ratio 9": (lambda: many([enc], [0], [nine.pic]), b"src_w"),
        "the same (encoder, slot) twice": (lambda: many([enc, enc2, enc], [1, 1, 1], [good.pic] * 3), b"twice"),
        "a pitch too narrow for the SOURCE width": (lambda: many([enc, enc2], [0, 0], [good.pic, changed(good.pic, pitch0=2 * 400 - 2)]), b"pitch[0]"),
        "bits 17": (lambda: many([enc], [0], [changed(good.pic, bits=17)]), b"bits"),
        "an odd source width": (lambda: many([enc], [0], [changed(good.pic, width=399)]), b"width"),
        "a NULL encoder": (lambda: many([enc, None], [0, 0], [good.pic, good.pic]), b""),
        "NULL picture (single call)": (lambda: (lib.hmr_gpu_enc_load_source_scaled_yuv(enc, 0, None, st), lib.hmr_gpu_last_error()), b""),
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


def deep_tensor(a):
    """a container array as a CUDA tensor: uint8 as it is, 16-bit containers as int16 (the same bits)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()


def test_load_is_ordered_against_the_producer_stream(gpu):
    """The source is written on a side stream just before the load call, with that stream passed in, and overwritten there right after the call returns, with no host
    synchronisation in between: the slot holds the first content's picture (the load waited for the producer, the producer's next work waited for the kernel)."""
    import torch
    lib, (ws, hs), (wd, hd), form = gpu, (1600, 1088), (416, 240), "semi_uv_420_10msb"
    ctx, enc = new_encoder(lib, wd, hd)
    rng = np.random.default_rng(8)
    y, u, v = yc.noise(form, rng, ws, hs)
    first = [deep_tensor(y), deep_tensor(np.stack([u, v], axis=2).reshape(hs // 2, ws))]
    staging = [torch.zeros_like(t) for t in first]
    pic = ys.descriptor(form, [t.data_ptr() for t in staging], [2 * ws, 2 * ws], ws, hs)
    assert lib.hmr_gpu_enc_load_source_scaled_yuv(enc, 0, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()      # (allocates the slot: the only host wait)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for s, f in zip(staging, first):
            s.copy_(f, non_blocking=True)
        assert lib.hmr_gpu_enc_load_source_scaled_yuv(enc, 0, C.byref(pic), C.c_void_p(side.cuda_stream)) == 0, lib.hmr_gpu_last_error()
        for s in staging:
            s.fill_(0x55)
    got = slot_picture(lib, enc, 0, wd, hd, "tight_i420")
    torch.cuda.synchronize()
    drop(lib, ctx, enc)
    want = ys.comparator_bytes(form, y, u, v, wd, hd)
    assert got == want, first_difference(got, want, wd, hd)


# ---- the Python classes ----
def i420_tensor(data, w, h):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda().view(h * 3 // 2, w)


def as_bytes(t):
    return t.cpu().numpy().tobytes()


def p010_frame(rng, w, h):
    """(YUVFrame, the containers) of P010 noise: tensors [H, W], [H / 2, W / 2, 2] that are views into larger ones"""
    form = "semi_uv_420_10msb"
    y, u, v = yc.noise(form, rng, w, h)
    big_y = rng.integers(0, 65536, (h + 2, w + 6)).astype("<u2")
    big_y[1:h + 1, 4:4 + w] = y
    big_uv = rng.integers(0, 65536, (h // 2 + 1, w // 2 + 3, 2)).astype("<u2")
    big_uv[1:, 2:2 + w // 2, 0], big_uv[1:, 2:2 + w // 2, 1] = u, v
    ty, tuv = deep_tensor(big_y)[1:h + 1, 4:4 + w], deep_tensor(big_uv)[1:, 2:2 + w // 2]
    assert not ty.is_contiguous() and not tuv.is_contiguous()
    return YUVFrame((ty, tuv), chroma="420", bits=10, msb_aligned=True), (form, y, u, v)


RUNGS = [(832, 480), (416, 240), (328, 264)]


def test_through_the_encoder_class_and_the_three_launch_composition(gpu):
    """Encoder.encode(ScaledYUVFrame) of one P010 source at three rung sizes: access units and source() equal those of control encoders given the comparator's I420
    picture, and the slot equals what YUVFrame into an encoder of the source's size, its source(), and that picture as a ScaledFrame leave"""
    ws, hs = RUNGS[0]
    rng = np.random.default_rng(6)
    frame, cont = p010_frame(rng, ws, hs)
    with Encoder(EncoderConfig(ws, hs, wfpp_num_threads=(hs + 63) // 64)) as top:
        top.encode(frame)
        eight = top.source()
        assert as_bytes(eight) == b"".join(p.tobytes() for p in yc.restate(*cont))
        for wd, hd in [(416, 240), (328, 264), (200, 136)]:
            want = ys.comparator_bytes(*cont, wd, hd)
            with Encoder(EncoderConfig(wd, hd)) as direct, Encoder(EncoderConfig(wd, hd)) as composed, Encoder(EncoderConfig(wd, hd)) as control:
                au = direct.encode(ScaledYUVFrame(frame, ws, hs))[0]
                assert au and au == control.encode(i420_tensor(want, wd, hd))[0] == composed.encode(ScaledFrame(eight, ws, hs))[0], (wd, hd)
                a, b, c = as_bytes(direct.source()), as_bytes(composed.source()), as_bytes(control.source())
                assert a == want, first_difference(a, want, wd, hd)
                assert a == b == c, (wd, hd)


@pytest.mark.parametrize("pipelined", [False, True])
def test_through_the_batch_encoder_class(gpu, pipelined):
    """BatchEncoder.step of a ladder at three rung sizes, one P010 source feeding all three (the top rung at the source's own size) - ONE load call a step - against a
    BatchEncoder fed with the comparator's I420 pictures: the same access units and source()"""
    ws, hs = RUNGS[0]
    cfgs = lambda: [EncoderConfig(rw, rh, wfpp_num_threads=(rh + 63) // 64) for rw, rh in RUNGS]      # (a thread per CTU row: the batch schedule at any width)
    rng = np.random.default_rng(16)
    got, want = [b"" for _ in RUNGS], [b"" for _ in RUNGS]
    with BatchEncoder(cfgs(), pipelined=pipelined) as enc, BatchEncoder(cfgs(), pipelined=pipelined) as control:
        enc.lib = counting = CountingLibrary(enc.lib)
        for f in range(2):
            frame, cont = p010_frame(rng, ws, hs)
            low = [ys.comparator_bytes(*cont, wd, hd) for wd, hd in RUNGS]
            for i, au in enumerate(enc.step([ScaledYUVFrame(frame, ws, hs)] * 3)):
                got[i] += au
            for i, au in enumerate(control.step([i420_tensor(p, wd, hd) for p, (wd, hd) in zip(low, RUNGS)])):
                want[i] += au
            for i, (a, b) in enumerate(zip(enc.source(), control.source())):
                assert as_bytes(a) == as_bytes(b) == low[i], (f, i)
        assert counting.calls == {"hmr_gpu_enc_load_sources_scaled_yuv": 2}, counting.calls
        enc.lib = counting._lib
        for i, au in enumerate(enc.flush()):
            got[i] += au
        for i, au in enumerate(control.flush()):
            want[i] += au
    for i in range(len(RUNGS)):
        assert got[i] and got[i] == want[i], RUNGS[i]


class CountingLibrary:
    """the library with its load calls counted by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("hmr_gpu_enc_load_"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_a_step_with_every_kind_makes_one_call_per_kind(gpu):
    """one step with a plain frame, an RGBFrame, a YUVFrame, a ScaledFrame and two ScaledYUVFrames of one source: exactly one library call per kind; source() returns the
    restated pictures"""
    import torch
    w, h = 416, 240
    ws, hs = 832, 480
    rng = np.random.default_rng(21)
    planes = ec.clip_frames(w, h, 1)[0]
    big = ec.clip_frames(ws, hs, 1)[0]
    r, g, b = rc.yuv_to_rgb(planes, w, h)
    p010, cont = p010_frame(rng, w, h)
    deep, deep_cont = p010_frame(rng, ws, hs)
    frames = [as_tensors(planes, w, h, 1, 5), RGBFrame(torch.from_numpy(np.stack([r, g, b])).cuda()), p010, ScaledFrame(i420_tensor(b"".join(big), ws, hs), ws, hs),
              ScaledYUVFrame(deep, ws, hs), ScaledYUVFrame(deep, ws, hs)]
    sizes = [(w, h)] * 5 + [(328, 264)]
    y8, u8, v8 = (np.frombuffer(p, np.uint8).reshape(shape) for p, shape in zip(big, ((hs, ws), (hs // 2, ws // 2), (hs // 2, ws // 2))))
    want = [b"".join(planes), b"".join(p.tobytes() for p in rc.restate(r, g, b, "bt709", 0)), b"".join(p.tobytes() for p in yc.restate(*cont)),
            sc.as_bytes(sc.restate((y8, u8, v8), w, h)), ys.comparator_bytes(*deep_cont, w, h), ys.comparator_bytes(*deep_cont, 328, 264)]
    with BatchEncoder([EncoderConfig(rw, rh, wfpp_num_threads=(rh + 63) // 64) for rw, rh in sizes], pipelined=False) as enc:
        enc.lib = counting = CountingLibrary(enc.lib)
        aus = enc.step(frames)
        assert counting.calls == {"hmr_gpu_enc_load_sources_device": 1, "hmr_gpu_enc_load_sources_rgb_device": 1, "hmr_gpu_enc_load_sources_yuv_device": 1,
                                  "hmr_gpu_enc_load_sources_scaled_device": 1, "hmr_gpu_enc_load_sources_scaled_yuv": 1}, counting.calls
        assert all(aus)
        for i, pic in enumerate(enc.source()):
            assert as_bytes(pic) == want[i], i
        enc.lib = counting._lib
