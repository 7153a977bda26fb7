"""-m gpu: a resolution ladder from pictures in device memory (include/homer_gpu.h section 12g, k_downscale in csrc/picture_io.hip, homerhevc_amd/encoder.py).  Every case
loads larger pictures with hmr_gpu_enc_load_source(s)_scaled_device and reads the slot back with hmr_gpu_enc_export_source(s)_device; the slot must equal the numpy
restatement of the section's arithmetic (tests/scale_cases.py) exactly - the comparator is the restatement, never the kernel.  End to end, the access units and
reconstructions of encoders fed through ScaledFrame must be byte-identical to those of encoders fed, through the existing load, with the restatement's I420.

What the canaries see: every byte of the source buffers (the rows and the random bytes around them) is what it was after the load, and every byte of the export's output
buffers outside the pictures' rows is what it was."""
import ctypes as C

import numpy as np
import pytest

import encoder_cases as ec
import picture_gpu
import scale_cases as sc
from homerhevc_amd.encoder import BatchEncoder, Encoder, EncoderConfig, Picture, ScaledFrame
from picture_gpu import LAYOUTS, Output, current_stream, drop, first_difference, gpu, new_encoder, slot_picture  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu
ERR_ARG = -3
# every pair of scale_cases.PAIRS whose destination the encoder accepts, and the identity at the end-to-end test's size
SINGLE = [p for p in sc.PAIRS if p[1] != (2, 2)] + [((400, 272), (400, 272))]


class Source(picture_gpu.Source):
    """A 4:2:0 picture laid out by sc.lay_out, with the descriptor of section 12g"""

    def __init__(self, planes, fmt, rng, padded=True):
        super().__init__(sc.lay_out(planes, fmt, rng, padded))
        self.planes, (self.h, self.w) = planes, planes[0].shape
        self.pic = sc.descriptor(fmt, self.addresses, self.pitches, self.w, self.h)

    def want(self, wd, hd):
        """the I420 picture a wd x hd slot has to hold"""
        return sc.as_bytes(sc.restate(self.planes, wd, hd))


@pytest.mark.parametrize("pair", SINGLE, ids=sc.pair_id)
def test_single_pictures(gpu, pair):
    """I420 and NV12 sources, noise and the checkerboard, slots 0 and 1 in turn; the slot read back as I420 and as NV12"""
    lib, ((ws, hs), (wd, hd)) = gpu, pair
    ctx, enc = new_encoder(lib, wd, hd)
    rng = np.random.default_rng(ws + hd)
    k = 0
    for kind in ("noise", "checkerboard"):
        planes = sc.content(kind, rng, ws, hs)
        want = sc.as_bytes(sc.restate(planes, wd, hd))
        for fmt in (sc.PIC_I420, sc.PIC_NV12):
            src = Source(planes, fmt, rng, padded=k != 3)
            slot = k & 1
            assert lib.hmr_gpu_enc_load_source_scaled_device(enc, slot, C.byref(src.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
            for layout in ("offset_i420", "nv12"):
                got = slot_picture(lib, enc, slot, wd, hd, layout, seed=k)
                assert got == want, (pair, kind, fmt, layout, first_difference(got, want, wd, hd))
            assert src.untouched(), (pair, "the source buffers were written")
            k += 1
    drop(lib, ctx, enc)


def test_equal_sizes_give_what_the_plain_load_gives(gpu):
    lib, (w, h) = gpu, (416, 240)
    rng = np.random.default_rng(3)
    planes = sc.content("noise", rng, w, h)
    made = [new_encoder(lib, w, h) for _ in range(2)]
    for k, fmt in enumerate((sc.PIC_I420, sc.PIC_NV12)):
        src = Source(planes, fmt, rng)
        assert lib.hmr_gpu_enc_load_source_scaled_device(made[0][1], k, C.byref(src.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_load_source_device(made[1][1], k, C.byref(Picture.from_buffer_copy(src.pic.pic)), current_stream()) == 0, lib.hmr_gpu_last_error()
        a, b = slot_picture(lib, made[0][1], k, w, h, "tight_i420"), slot_picture(lib, made[1][1], k, w, h, "tight_i420")
        assert a == b == sc.as_bytes(planes)
    for ctx, enc in made:
        drop(lib, ctx, enc)


def test_one_call_with_mixed_entries(gpu):
    """twelve entries: three sources of different sizes, each feeding four encoders of different sizes, I420 and NV12 mixed, one entry at ratio 8 and identities"""
    lib = gpu
    rng = np.random.default_rng(12)
    ladder = {(1600, 1088): [(200, 136), (416, 240), (832, 480), (400, 272)],      # 8 : 1, and ratios that are no whole numbers
              (832, 480): [(416, 240), (328, 264), (384, 192), (832, 480)],       # 2 : 1, 104 : 41 x 20 : 11, ..., the identity
              (400, 272): [(200, 136), (328, 264), (392, 136), (400, 272)]}
    sources = {size: [Source(planes, fmt, rng) for fmt in (sc.PIC_I420, sc.PIC_NV12)] for size in ladder for planes in [sc.content("noise", rng, *size)]}
    entries = [(size, dst, sources[size][(i + k) & 1]) for i, size in enumerate(ladder) for k, dst in enumerate(ladder[size])]
    n = len(entries)
    assert n == 12
    made = [new_encoder(lib, *dst) for _, dst, _ in entries]
    for turn in range(2):      # both slots; the second call finds the slots allocated
        assert lib.hmr_gpu_enc_load_sources_scaled_device((C.c_void_p * n)(*[m[1] for m in made]), n, (C.c_int * n)(*([turn] * n)), (sc.ScaledPicture * n)(*[e[2].pic for e in entries]),
                                                          current_stream()) == 0, lib.hmr_gpu_last_error()
        outs = [Output(dst[0], dst[1], LAYOUTS[(i + turn) % 3], seed=i) for i, (_, dst, _) in enumerate(entries)]
        assert lib.hmr_gpu_enc_export_sources_device((C.c_void_p * n)(*[m[1] for m in made]), n, (C.c_int * n)(*([turn] * n)), (Picture * n)(*[o.pic for o in outs]),
                                                     current_stream()) == 0, lib.hmr_gpu_last_error()
        for i, ((size, dst, src), o) in enumerate(zip(entries, outs)):
            got, want = o.picture(), src.want(*dst)
            assert got == want, (i, size, dst, first_difference(got, want, *dst))
    assert all(s.untouched() for pair in sources.values() for s in pair)
    for ctx, enc in made:
        drop(lib, ctx, enc)


def ladder_clip(frames=2):
    """a 400 x 272 source per frame, and per rung the restatement's I420 of it"""
    w, h = 400, 272
    clip = ec.clip_frames(w, h, frames)
    planes = [[np.frombuffer(p, np.uint8).reshape(s) for p, s in zip(f, ((h, w), (h // 2, w // 2), (h // 2, w // 2)))] for f in clip]
    rungs = [(400, 272), (200, 136)]
    return w, h, planes, rungs, [[sc.as_bytes(sc.restate(p, *r)) for r in rungs] for p in planes]


def i420_tensor(data, w, h):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda().view(h * 3 // 2, w)


@pytest.mark.parametrize("pipelined", [False, True])
def test_ladder_end_to_end(gpu, pipelined):
    """One 400 x 272 source per frame for two frames (I, then P) into a BatchEncoder of 400 x 272 / 200 x 136 rungs through ScaledFrame - the top rung at equal size, the
    source as (y, u, v) views in one frame and as NV12 in the other - against a BatchEncoder fed with the restatement's I420 through the existing path: access units,
    export() pictures, their sums and source() are byte-identical."""
    w, h, planes, rungs, scaled = ladder_clip()
    cfgs = lambda: [EncoderConfig(rw, rh, wfpp_num_threads=(rh + 63) // 64) for rw, rh in rungs]      # (a thread per CTU row: the batch schedule at any width)
    got, want = [b"" for _ in rungs], [b"" for _ in rungs]
    rng = np.random.default_rng(5)
    with BatchEncoder(cfgs(), pipelined=pipelined) as enc, BatchEncoder(cfgs(), pipelined=pipelined) as control:
        for f, p in enumerate(planes):
            src = Source(p, sc.PIC_NV12 if f else sc.PIC_I420, rng)
            import torch
            if f:
                frame = (torch.as_strided(src.tensors[0], (h, w), (src.pic.pic.pitch[0], 1), 3), torch.as_strided(src.tensors[1], (h // 2, w), (src.pic.pic.pitch[1], 1), 1))
            else:
                frame = tuple(torch.as_strided(t, shape, (src.pic.pic.pitch[c], 1), off)
                              for c, (t, shape, off) in enumerate(zip(src.tensors, ((h, w), (h // 2, w // 2), (h // 2, w // 2)), (1, 2, 3))))
            for i, au in enumerate(enc.step([ScaledFrame(frame, w, h) for _ in rungs])):
                got[i] += au
            for i, au in enumerate(control.step([i420_tensor(scaled[f][i], *r) for i, r in enumerate(rungs)])):
                want[i] += au
            for i, (a, b) in enumerate(zip(enc.source(), control.source())):
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == scaled[f][i], (f, i)
            (pa, sa), (pb, sb) = enc.export(ssd=True), control.export(ssd=True)
            assert sa.tolist() == sb.tolist()      # (the sums are against the SCALED source)
            for i, (a, b) in enumerate(zip(pa, pb)):
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (f, i)
        for i, au in enumerate(enc.flush()):
            got[i] += au
        for i, au in enumerate(control.flush()):
            want[i] += au
    for i in range(len(rungs)):
        assert got[i] and got[i] == want[i], rungs[i]


def test_ladder_through_the_encoder_class(gpu):
    w, h, planes, rungs, scaled = ladder_clip()
    rw, rh = rungs[1]
    got = want = b""
    types = []
    with Encoder(EncoderConfig(rw, rh)) as enc, Encoder(EncoderConfig(rw, rh)) as control:
        for f, p in enumerate(planes):
            au, slice_type = enc.encode(ScaledFrame(i420_tensor(sc.as_bytes(p), w, h), w, h))
            got += au
            types.append(slice_type)
            want += control.encode(i420_tensor(scaled[f][1], rw, rh))[0]
            assert enc.source().cpu().numpy().tobytes() == scaled[f][1]
            assert enc.export()[0].cpu().numpy().tobytes() == control.export()[0].cpu().numpy().tobytes()
    assert types == [2, 1] and got and got == want


def test_load_is_ordered_against_the_producer_stream(gpu):
    """The source tensor is overwritten on torch's stream right after the load call returns, with no host synchronisation in between: the slot still holds the first
    picture's scaling (the producer's next work waited for the kernel)."""
    import torch
    lib, (ws, hs), (wd, hd) = gpu, (1920, 1080), (416, 240)
    ctx, enc = new_encoder(lib, wd, hd)
    rng = np.random.default_rng(8)
    planes = sc.content("noise", rng, ws, hs)
    first = torch.from_numpy(np.frombuffer(sc.as_bytes(planes), np.uint8).copy()).cuda()
    staging = torch.zeros_like(first)
    pic = sc.descriptor(sc.PIC_I420, [staging.data_ptr(), staging.data_ptr() + ws * hs, staging.data_ptr() + ws * hs * 5 // 4], [ws, ws // 2, ws // 2], ws, hs)
    assert lib.hmr_gpu_enc_load_source_scaled_device(enc, 0, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()      # (allocates the slot: the only host wait)
    torch.cuda.synchronize()
    staging.copy_(first, non_blocking=True)
    assert lib.hmr_gpu_enc_load_source_scaled_device(enc, 0, C.byref(pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    staging.fill_(0x55)
    got = slot_picture(lib, enc, 0, wd, hd, "tight_i420")
    drop(lib, ctx, enc)
    want = sc.as_bytes(sc.restate(planes, wd, hd))
    assert got == want, first_difference(got, want, wd, hd)


def test_refusals_leave_the_encoders_working(gpu):
    """each refusal is HMR_GPU_ERR_ARG with a text before anything is queued; afterwards the same encoders take a good call and hold the right pictures"""
    lib = gpu
    rng = np.random.default_rng(2)
    ctx, enc = new_encoder(lib, 200, 136)
    ctx2, enc2 = new_encoder(lib, 200, 136)
    good = Source(sc.content("noise", rng, 400, 272), sc.PIC_I420, rng)
    small = Source(sc.content("noise", rng, 192, 128), sc.PIC_NV12, rng)
    nine = Source(sc.content("noise", rng, 1800, 1224), sc.PIC_I420, rng, padded=False)
    st = current_stream()

    def many(encs, slots, pics, n=None):
        k = len(encs)
        rc = lib.hmr_gpu_enc_load_sources_scaled_device((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*slots), (sc.ScaledPicture * k)(*pics), st)
        return rc, lib.hmr_gpu_last_error()

    def changed(pic, **kw):
        p = sc.ScaledPicture.from_buffer_copy(pic)
        for k, v in kw.items():
            if k[-1].isdigit():
                getattr(p.pic, k[:-1])[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return p

    host = np.zeros(400 * 272 * 3 // 2, np.uint8)
    refused = {
        "upscale": (many([enc], [0], [small.pic]), b"dst_w"),
        "ratio 9": (many([enc], [0], [nine.pic]), b"src_w"),
        "a descriptor too narrow for the SOURCE width": (many([enc, enc2], [0, 0], [good.pic, changed(good.pic, pitch0=398)]), b"pitch[0]"),
        "a pitch that would do for the encoder's width": (many([enc], [0], [changed(good.pic, pitch1=100)]), b"pitch[1]"),
        "a host pointer": (many([enc], [0], [changed(good.pic, plane0=host.ctypes.data)]), b"plane[0]"),
        "the same (encoder, slot) twice": (many([enc, enc2, enc], [1, 1, 1], [good.pic] * 3), b"twice"),
        "an odd source width": (many([enc], [0], [changed(good.pic, width=399)]), b"width"),
        "n = 0": (many([enc], [0], [good.pic], n=0), b""),
        "n = 513": (many([enc] * 513, list(range(513)), [good.pic] * 513), b""),
        "a NULL encoder": (many([enc, None], [0, 0], [good.pic, good.pic]), b""),
        "NULL picture (single call)": ((lib.hmr_gpu_enc_load_source_scaled_device(enc, 0, None, st), lib.hmr_gpu_last_error()), b""),
    }
    for why, ((rc, text), field) in refused.items():
        assert rc == ERR_ARG and text and field in text, (why, rc, text)
    # the same source twice in one call is the ladder; the same slot number on two encoders is fine
    assert many([enc, enc2], [0, 0], [good.pic, good.pic])[0] == 0, lib.hmr_gpu_last_error()
    want = good.want(200, 136)
    assert slot_picture(lib, enc, 0, 200, 136, "nv12") == want and slot_picture(lib, enc2, 0, 200, 136, "offset_i420") == want
    buf, n = C.create_string_buffer(1 << 20), C.c_long()
    assert lib.hmr_gpu_enc_encode_source(enc, 0, 0, buf, len(buf), C.byref(n), None) == 2 and n.value > 0, lib.hmr_gpu_last_error()
    drop(lib, ctx, enc)
    drop(lib, ctx2, enc2)
