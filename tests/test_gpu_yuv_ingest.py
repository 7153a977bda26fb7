"""-m gpu: Y'CbCr pictures of 8 .. 16 bits in 4:2:0, 4:2:2 or 4:4:4, planar, semi-planar or packed, in device memory (include/homer_gpu.h section 12k, k_ingest_yuv in
csrc/picture_io.hip, homerhevc_amd/encoder.py).  Every case loads a picture with hmr_gpu_enc_load_source(s)_yuv_device and reads the slot back with
hmr_gpu_enc_export_source(s)_device; the slot must equal the numpy restatement of the section's arithmetic (tests/yuv_cases.py) exactly - the comparator is the
restatement, never the kernel.  End to end, the streams and reconstructions of encoders fed with YUVFrames must be byte-identical to those of a twin fed, through the
existing hmr_gpu_enc_load_sources_device, with the numpy-converted I420.

What the canaries see: every byte of the source buffers (the rows and the random bytes around them; every buffer ends with its plane's last row) is what it was after the
load, and every byte of the export's output buffers outside the pictures' rows is what it was (picture_gpu.Output)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import picture_gpu
import rgb_cases as rc
import yuv_cases as yc
from homerhevc_amd.encoder import BatchEncoder, Encoder, Picture, RGBFrame, ScaledFrame, YUVFrame, yuv_picture_of
from picture_gpu import (GOLD, LAYOUTS, Output, as_tensors, config_of, current_stream, drop, first_difference, gpu, make_encoder, new_encoder, slot_picture,  # noqa: F401
                         upload)

pytestmark = pytest.mark.gpu
ERR_ARG = -3


class Source(picture_gpu.Source):
    """A picture laid out by yc.lay_out (sample-aligned base addresses), with the descriptor of section 12k and, as `want`, the I420 picture the slot has to hold"""

    def __init__(self, form, planes3, rng, padded=True):
        super().__init__(yc.lay_out(form, *planes3, rng, padded))
        self.pic = yc.descriptor(form, self.addresses, self.pitches)
        self.want = b"".join(p.tobytes() for p in yc.restate(form, *planes3))


@pytest.mark.parametrize("size", [(200, 136), (328, 264), (416, 240)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_pictures(gpu, size):
    """every form of F on noise over the container's range; two slots in turn; the slot read back as I420 and as NV12.  200 x 136: a luma tail of 8 and a chroma tail of 4;
    416 x 240: no tail"""
    lib, (w, h) = gpu, size
    ctx, enc = new_encoder(lib, w, h)
    rng = np.random.default_rng(w + h)
    for k, form in enumerate(yc.NAMES):
        src = Source(form, yc.noise(form, rng, w, h), rng, padded=k % 3 != 2)
        slot = k & 1
        assert lib.hmr_gpu_enc_load_source_yuv_device(enc, slot, C.byref(src.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
        for layout in ("offset_i420", "nv12"):
            got = slot_picture(lib, enc, slot, w, h, layout, seed=k)
            assert got == src.want, (form, layout, first_difference(got, src.want, w, h))
        assert src.untouched(), (form, "the source buffers were written")
    drop(lib, ctx, enc)


@pytest.mark.parametrize("form", ["semi_uv_420_10msb", "planar_444_16"])
def test_1080p(gpu, form):
    lib, (w, h) = gpu, (1920, 1080)
    ctx, enc = new_encoder(lib, w, h)
    rng = np.random.default_rng(1080)
    src = Source(form, yc.noise(form, rng, w, h), rng)
    assert lib.hmr_gpu_enc_load_source_yuv_device(enc, 0, C.byref(src.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    got = slot_picture(lib, enc, 0, w, h, "tight_i420")
    assert got == src.want, (form, first_difference(got, src.want, w, h))
    assert src.untouched()
    drop(lib, ctx, enc)


def test_a_batch_of_mixed_sizes_and_forms(gpu):
    """ONE call for 14 encoders of four sizes, a form of every layout, depth and chroma format among them; then the same (encoder, slot) twice: refused, nothing queued"""
    lib = gpu
    sizes = [(200, 136), (416, 240), (328, 264), (256, 64)]
    forms = ["semi_uv_420_10msb", "planar_444_16", "yuyv_8", "planar_420_10", "y210", "semi_vu_422_12", "planar_422_8", "uyvy_8", "semi_uv_444_8", "planar_444_10msb",
             "semi_vu_420_8", "vyuy_8", "planar_420_8", "semi_uv_422_16"]
    rng = np.random.default_rng(14)
    made = [new_encoder(lib, *sizes[i % 4]) for i in range(len(forms))]
    n = len(made)
    encs, slots = (C.c_void_p * n)(*[m[1] for m in made]), (C.c_int * n)(*([1] * n))
    srcs = [Source(form, yc.noise(form, rng, *sizes[i % 4]), rng, padded=i % 3 != 1) for i, form in enumerate(forms)]
    assert lib.hmr_gpu_enc_load_sources_yuv_device(encs, n, slots, (yc.YuvPicture * n)(*[s.pic for s in srcs]), current_stream()) == 0, lib.hmr_gpu_last_error()

    def slots_hold_the_pictures():
        outs = [Output(*sizes[i % 4], LAYOUTS[i % 3], seed=i) for i in range(n)]
        assert lib.hmr_gpu_enc_export_sources_device(encs, n, slots, (Picture * n)(*[o.pic for o in outs]), current_stream()) == 0, lib.hmr_gpu_last_error()
        for i, (s, o) in enumerate(zip(srcs, outs)):
            got = o.picture()
            assert got == s.want, (i, forms[i], first_difference(got, s.want, *sizes[i % 4]))

    slots_hold_the_pictures()
    assert all(s.untouched() for s in srcs)
    # other pictures for the same encoders, the first encoder and slot a second time at the end of the call
    other = [Source(form, yc.noise(form, rng, *sizes[i % 4]), rng) for i, form in enumerate(forms)]
    twice = (C.c_void_p * (n + 1))(*([m[1] for m in made] + [made[0][1]]))
    assert lib.hmr_gpu_enc_load_sources_yuv_device(twice, n + 1, (C.c_int * (n + 1))(*([1] * (n + 1))), (yc.YuvPicture * (n + 1))(*([s.pic for s in other] + [other[0].pic])),
                                                   current_stream()) == ERR_ARG
    assert b"twice" in lib.hmr_gpu_last_error()
    slots_hold_the_pictures()
    for ctx, enc in made:
        drop(lib, ctx, enc)


def test_refusals_leave_the_encoder_working(gpu):
    """what the host can see without following a pointer is HMR_GPU_ERR_ARG with a text, nothing is launched, and the encoder still produces its fixture's stream"""
    lib, case = gpu, "416x240_wpp_rows"
    g = GOLD[case]
    ctx, enc, w, h, image_type, clip = make_encoder(lib, case)
    rng = np.random.default_rng(2)
    good = Source("semi_uv_420_10msb", yc.noise("semi_uv_420_10msb", rng, w, h), rng)
    st = current_stream()

    def many(encs, slots, pics, n=None):
        k = len(encs)
        rc_ = lib.hmr_gpu_enc_load_sources_yuv_device((C.c_void_p * k)(*encs), k if n is None else n, (C.c_int * k)(*slots), (yc.YuvPicture * k)(*pics), st)
        return rc_, lib.hmr_gpu_last_error()

    def changed(pic, **kw):
        p = yc.YuvPicture.from_buffer_copy(pic)
        for k, v in kw.items():
            if k[-1].isdigit():
                getattr(p, k[:-1])[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return p

    host = np.zeros(2 * w * h + 64, np.uint8)
    small = Source("semi_uv_420_10msb", yc.noise("semi_uv_420_10msb", rng, w - 16, h), rng, padded=False)      # a picture of another size: its pitches are below this encoder's rows
    refused = {
        "a host pointer as a plane": many([enc], [0], [changed(good.pic, plane1=host.ctypes.data)]),
        "a host pointer as the luma plane": many([enc], [0], [changed(good.pic, plane0=host.ctypes.data)]),
        "a descriptor for the wrong size": many([enc], [0], [small.pic]),
        "n = 0": many([enc], [0], [good.pic], n=0),
        "n = 513": many([enc] * 513, list(range(513)), [good.pic] * 513),
        "a NULL encoder": many([enc, None], [0, 0], [good.pic, good.pic]),
        "NULL encoder (single call)": (lib.hmr_gpu_enc_load_source_yuv_device(None, 0, C.byref(good.pic), st), lib.hmr_gpu_last_error()),
        "NULL picture (single call)": (lib.hmr_gpu_enc_load_source_yuv_device(enc, 0, None, st), lib.hmr_gpu_last_error()),
        "slot 4097": many([enc], [4097], [good.pic]),
        "bits 17": many([enc], [0], [changed(good.pic, bits=17)]),
        "packed 4:2:0": many([enc], [0], [changed(good.pic, format=2, plane1=None)]),
    }
    for why, (rc_, text) in refused.items():
        assert rc_ == ERR_ARG and text, (why, rc_, text)
    assert b"not device memory" in refused["a host pointer as a plane"][1] and b"pitch" in refused["a descriptor for the wrong size"][1]
    # nothing was queued: no slot exists yet
    out = Output(w, h, "tight_i420")
    assert lib.hmr_gpu_enc_export_source_device(enc, 0, C.byref(out.pic), st) == ERR_ARG and b"slot" in lib.hmr_gpu_last_error()
    assert many([enc], [0], [good.pic])[0] == 0, lib.hmr_gpu_last_error()
    assert slot_picture(lib, enc, 0, w, h, "nv12") == good.want
    buf, n, stream = C.create_string_buffer(1 << 20), C.c_long(), b""
    for f, planes in enumerate(clip):
        pic, t = upload(planes, w, h, LAYOUTS[f % 3], seed=f)
        assert lib.hmr_gpu_enc_load_source_device(enc, f & 1, C.byref(pic), st) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_encode_source(enc, f & 1, image_type, buf, len(buf), C.byref(n), None) in (1, 2), lib.hmr_gpu_last_error()
        stream += buf.raw[:n.value]
    drop(lib, ctx, enc)
    assert len(stream) == g["stream_bytes"] and hashlib.md5(stream).hexdigest() == g["stream_md5"]


# ---- the Python classes ----
def deep_tensor(a):
    """a container array as a CUDA tensor: uint8 as it is, 16-bit containers as int16 (the same bits)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()


def p010_of(y8, u8, v8, rng):
    """an 8-bit 4:2:0 picture as P010 - the 10-bit value 4 p + d (d in 0 .. 1: it rounds back to p) in the high bits, dirty low bits - in tensors [H, W], [H / 2, W / 2, 2]
    that are views into larger ones; returns (YUVFrame, the containers)"""
    planes = []
    for p in (y8, u8, v8):
        ten = (p.astype(np.int64) << 2) + rng.integers(0, 2, p.shape)
        planes.append(((ten << 6) | rng.integers(0, 64, p.shape)).astype("<u2"))
    y, u, v = planes
    h, w = y.shape
    big_y = rng.integers(0, 65536, (h + 2, w + 6)).astype("<u2")
    big_y[1:h + 1, 4:4 + w] = y
    big_uv = rng.integers(0, 65536, (h // 2 + 1, w // 2 + 3, 2)).astype("<u2")
    big_uv[1:, 2:2 + w // 2, 0], big_uv[1:, 2:2 + w // 2, 1] = u, v
    ty, tuv = deep_tensor(big_y)[1:h + 1, 4:4 + w], deep_tensor(big_uv)[1:, 2:2 + w // 2]
    assert not ty.is_contiguous() and not tuv.is_contiguous()
    return YUVFrame((ty, tuv), chroma="420", bits=10, msb_aligned=True), planes


def planar444_of(y8, u8, v8, rng, uint16):
    """the same picture as planar 4:4:4 of 10 bits in the low bits: chroma repeated 2 x 2, every tap 4 p + d; as uint16 tensors where torch has them"""
    import torch
    planes = [((p.astype(np.int64) << 2) + rng.integers(0, 2, p.shape)).astype("<u2") for p in (y8, u8.repeat(2, axis=0).repeat(2, axis=1), v8.repeat(2, axis=0).repeat(2, axis=1))]
    tensors = [deep_tensor(p) for p in planes]
    if uint16 and hasattr(torch, "uint16"):
        tensors = [t.view(torch.uint16) for t in tensors]
    return YUVFrame(tuple(tensors), chroma="444", bits=10), planes


def test_end_to_end_against_the_converted_i420(gpu):
    """416 x 240, two frames (I then P), three encoders: P010 and planar 4:4:4 10-bit as YUVFrames, and a twin fed with the numpy-converted I420 through the existing
    hmr_gpu_enc_load_sources_device: the access units, export() and source() are byte-identical"""
    import torch
    cfg, image_type, clip = config_of("416x240")
    w, h = cfg.width, cfg.height
    rng = np.random.default_rng(10)
    types = []
    with Encoder(cfg) as a, Encoder(config_of("416x240")[0]) as b, Encoder(config_of("416x240")[0]) as twin:
        for f, planes in enumerate(clip[:2]):
            y8, u8, v8 = (np.frombuffer(p, np.uint8).reshape(shape) for p, shape in zip(planes, ((h, w), (h // 2, w // 2), (h // 2, w // 2))))
            frame_a, cont_a = p010_of(y8, u8, v8, rng)
            frame_b, cont_b = planar444_of(y8, u8, v8, rng, uint16=bool(f))
            i420 = b"".join(p.tobytes() for p in yc.restate("semi_uv_420_10msb", *cont_a))
            assert i420 == b"".join(p.tobytes() for p in yc.restate("planar_444_10", *cont_b)) == b"".join(planes)
            want, slice_type = twin.encode(torch.from_numpy(np.frombuffer(i420, np.uint8).copy()).cuda().view(h * 3 // 2, w), image_type)
            types.append(slice_type)
            rec = twin.export()[0].cpu().numpy().tobytes()
            for name, enc, frame in (("P010", a, frame_a), ("planar 4:4:4", b, frame_b)):
                au, st = enc.encode(frame, image_type)
                assert st == slice_type and au and au == want, (name, f)
                pic, ssd = enc.export(ssd=True)
                assert pic.cpu().numpy().tobytes() == rec, (name, f)
                assert ssd.tolist() == twin.export(picture=False, ssd=True)[1].tolist()
                assert enc.source().cpu().numpy().tobytes() == i420, (name, f)
                assert enc.ssim().tolist() == twin.ssim().tolist()
    assert types == [2, 1]


class CountingLibrary:
    """the library with its calls counted by name"""

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


def test_batch_encoder_step_with_every_kind(gpu):
    """one step with a plain frame, an RGBFrame and two YUVFrames: one load call per kind; source() returns the restated pictures"""
    import torch
    case = "416x240_wpp_rows"
    made = [config_of(case) for _ in range(4)]
    w, h = made[0][0].width, made[0][0].height
    planes = made[0][2][0]
    rng = np.random.default_rng(21)
    y8, u8, v8 = (np.frombuffer(p, np.uint8).reshape(shape) for p, shape in zip(planes, ((h, w), (h // 2, w // 2), (h // 2, w // 2))))
    r, g, b = rc.yuv_to_rgb(planes, w, h)
    p010, cont = p010_of(y8, u8, v8, rng)
    packed = yc.noise("uyvy_8", rng, w, h)
    buf, base, pitch = yc.lay_out("uyvy_8", *packed, rng, True)[0]
    uyvy = torch.from_numpy(buf).cuda()[base:].as_strided((h, 2 * w), (pitch, 1))
    frames = [as_tensors(planes, w, h, 1, 5), RGBFrame(torch.from_numpy(np.stack([r, g, b])).cuda()), p010, YUVFrame(uyvy, chroma="422", order="uyvy")]
    want = [b"".join(planes), b"".join(p.tobytes() for p in rc.restate(r, g, b, "bt709", 0)), b"".join(p.tobytes() for p in yc.restate("semi_uv_420_10msb", *cont)),
            b"".join(p.tobytes() for p in yc.restate("uyvy_8", *packed))]
    with BatchEncoder([m[0] for m in made], pipelined=False) as enc:
        enc.lib = counting = CountingLibrary(enc.lib)
        aus = enc.step(frames, [m[1] for m in made])
        assert counting.calls == {"hmr_gpu_enc_load_sources_device": 1, "hmr_gpu_enc_load_sources_rgb_device": 1, "hmr_gpu_enc_load_sources_yuv_device": 1}, counting.calls
        assert all(aus) and aus[0] == aus[2]      # (the P010 picture rounds back to the clip's frame)
        for i, pic in enumerate(enc.source()):
            assert pic.cpu().numpy().tobytes() == want[i], i
        enc.lib = counting._lib
    with pytest.raises(TypeError):
        ScaledFrame(p010, w, h)
    with pytest.raises(TypeError):      # 10 bits in uint8 tensors
        yuv_picture_of(YUVFrame((torch.zeros((h, w), dtype=torch.uint8, device="cuda"),) * 3, chroma="444", bits=10), w, h)
    with pytest.raises(ValueError):     # a 4:2:0 chroma plane where 4:4:4 is announced
        yuv_picture_of(YUVFrame((deep_tensor(y8), deep_tensor(u8), deep_tensor(v8)), chroma="444"), w, h)
