"""What the picture GPU tests (tests/test_gpu_*ingest.py, *scale.py, *egress.py, test_gpu_ssim.py) and the picture bench tools (tools/*_bench.py over tools/picture_bench.py)
share: ONE ctypes binding of the library's picture interface (include/homer_gpu.h sections 12d .. 12k and the encoder calls around them), the `gpu` fixture that returns it,
and the helpers that put pictures into device memory and read them back.  The structures are the tests' own mirrors (encoder_cases, rgb_cases, yuv_cases, scale_cases,
rgb_scale_cases) - the CPU tests hold them to the package's and to the header - and the package's Picture for hmr_gpu_picture."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import encoder_cases as ec
import libs
import rgb_cases as rc
import rgb_scale_cases as rs
import scale_cases as sc
import yuv_cases as yc
from homerhevc_amd.encoder import PIC_I420, PIC_NV12, EncoderConfig, Picture, RGBFrame

GOLD = json.load(open(os.path.join(ec.GOLDEN, "streams.json")))
LAYOUTS = ["tight_i420", "offset_i420", "nv12"]
BATCH_CASES = ["416x240_wpp_rows", "832x480_wpp_rows", "416x240_scene_cut_wpp_rows", "328x264_wpp3", "832x480_cbr1500_perf1_wpp_rows", "416x240_cbr300_nosao_wpp_rows",
               "416x240_noise_wpp_rows", "416x240_extremes_wpp_rows"]

# ---- the binding: name -> (argtypes, restype); None leaves ctypes' default (int) ----
P, I, L = C.c_void_p, C.c_int, C.c_long
_ONE, _MANY = lambda T: [P, I, C.POINTER(T), P], lambda T: [C.POINTER(P), I, C.POINTER(I), C.POINTER(T), P]      # (encoder, slot, picture, stream) and its batched form
_BATCH = [C.POINTER(P), I, C.POINTER(I), C.POINTER(I), C.POINTER(C.c_char_p), C.POINTER(L), C.POINTER(L)]
_R = C.POINTER(rc.RgbPicture)
SIGNATURES = {
    "hmr_gpu_last_error": (None, C.c_char_p),
    "hmr_gpu_create": ([C.POINTER(P), I, P], None),
    "hmr_gpu_destroy": ([P], None),
    "hmr_gpu_enc_create": ([P, C.POINTER(ec.EncCfg), C.POINTER(P)], None),
    "hmr_gpu_enc_create_engine": ([P, C.POINTER(ec.EncCfg), I, C.POINTER(P)], None),
    "hmr_gpu_enc_destroy": ([P], None),
    "hmr_gpu_enc_load_source": ([P, I] + [C.c_char_p] * 3, None),
    "hmr_gpu_enc_encode_source": ([P, I, I, C.c_char_p, L, C.POINTER(L), C.c_char_p], None),
    "hmr_gpu_enc_encode_batch": (_BATCH, None),
    "hmr_gpu_enc_encode_batch_pipelined": (_BATCH, None),
    "hmr_gpu_enc_encode_chain": ([C.POINTER(P), I, P, C.POINTER(I), C.POINTER(I), C.POINTER(C.c_char_p), C.POINTER(L), C.POINTER(L)], None),
    "hmr_gpu_enc_export_references8": ([C.POINTER(P), I, P, L, P], None),
    "hmr_gpu_enc_reference_bytes": ([P], L),
    "hmr_gpu_enc_state_bytes": (None, I),
    # 12d, 12e: 4:2:0 pictures in, reconstructed pictures and sums of squared differences out
    "hmr_gpu_enc_load_source_device": (_ONE(Picture), None),
    "hmr_gpu_enc_load_sources_device": (_MANY(Picture), None),
    "hmr_gpu_enc_export_picture_device": ([P, C.POINTER(Picture), I, P, P], None),
    "hmr_gpu_enc_export_pictures_device": ([C.POINTER(P), I, C.POINTER(Picture), C.POINTER(I), P, P], None),
    # 12f: RGB in, and a slot's picture out
    "hmr_gpu_enc_load_source_rgb_device": (_ONE(rc.RgbPicture), None),
    "hmr_gpu_enc_load_sources_rgb_device": (_MANY(rc.RgbPicture), None),
    "hmr_gpu_enc_export_source_device": (_ONE(Picture), None),
    "hmr_gpu_enc_export_sources_device": (_MANY(Picture), None),
    # 12g, 12j: downscaling, from 4:2:0 and from RGB
    "hmr_gpu_enc_load_source_scaled_device": (_ONE(sc.ScaledPicture), None),
    "hmr_gpu_enc_load_sources_scaled_device": (_MANY(sc.ScaledPicture), None),
    "hmr_gpu_enc_load_source_scaled_rgb_device": (_ONE(rs.ScaledRgbPicture), None),
    "hmr_gpu_enc_load_sources_scaled_rgb_device": (_MANY(rs.ScaledRgbPicture), None),
    # 12h: SSIM sums
    "hmr_gpu_enc_ssim_one_device": ([P, I, P, P], None),
    "hmr_gpu_enc_ssim_device": ([C.POINTER(P), I, C.POINTER(I), P, P], None),
    "hmr_gpu_ssim": ([C.POINTER(C.c_int64), I, I, C.POINTER(C.c_double)], None),
    "hmr_gpu_ssim_host": ([C.POINTER(Picture), C.POINTER(Picture), I, I, C.POINTER(C.c_int64)], None),
    # 12i: RGB out
    "hmr_gpu_enc_export_picture_rgb_device": ([P, I, _R, _R, P, P], None),
    "hmr_gpu_enc_export_pictures_rgb_device": ([C.POINTER(P), I, C.POINTER(I), _R, _R, P, P], None),
    # 12k: deep, 4:2:2 and 4:4:4 Y'CbCr in
    "hmr_gpu_enc_load_source_yuv_device": (_ONE(yc.YuvPicture), None),
    "hmr_gpu_enc_load_sources_yuv_device": (_MANY(yc.YuvPicture), None),
}


def declare(lib):
    """the whole table onto a handle of the library"""
    for name, (argtypes, restype) in SIGNATURES.items():
        fn = getattr(lib, name)
        if argtypes is not None:
            fn.argtypes = argtypes
        if restype is not None:
            fn.restype = restype
    return lib


_loaded = None


def load():
    """libs.load_gpu()'s one handle with the table applied - once: no caller declares anything of its own, so no call depends on who ran before it"""
    global _loaded
    if _loaded is None:
        _loaded = declare(libs.load_gpu())
    return _loaded


@pytest.fixture(scope="module")
def gpu():
    return load()


# ---- encoders ----
def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def new_encoder(lib, w, h, **keys):
    ctx, enc = C.c_void_p(), C.c_void_p()
    assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()      # a context (stream) of its own per sequence
    cfg = ec.default_cfg(w, h, **keys)
    assert lib.hmr_gpu_enc_create(ctx, C.byref(cfg), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
    return ctx, enc


def drop(lib, ctx, enc):
    lib.hmr_gpu_enc_destroy(enc)
    lib.hmr_gpu_destroy(ctx)


def case_clip(case):
    """(width, height, configuration keys, image_type, the clip's frames as (y, u, v) bytes) of a fixture"""
    g = GOLD[case]
    keys = dict(g["keys"])
    cut_at, seed, content = keys.pop("cut_at", None), keys.pop("clip_seed", 1234), keys.pop("content", "default")
    image_type = 3 if keys.pop("force_intra", 0) else 0
    return g["width"], g["height"], keys, image_type, ec.clip_frames(g["width"], g["height"], g["frames"], cut_at, seed, content)


def make_encoder(lib, case):
    w, h, keys, image_type, clip = case_clip(case)
    ctx, enc = new_encoder(lib, w, h, **keys)
    return ctx, enc, w, h, image_type, clip


def config_of(case):
    w, h, keys, image_type, clip = case_clip(case)
    return EncoderConfig(w, h, **{ec.KEY_NAMES.get(k, k): v for k, v in keys.items()}), image_type, clip


# ---- 4:2:0 pictures into device memory ----
def embed(rng, plane, rows, row_bytes, pitch, offset):
    """a plane of `rows` rows at byte `offset` and pitch `pitch` of a buffer that ends with the plane's last row; every other byte is random"""
    buf = rng.integers(0, 256, offset + pitch * (rows - 1) + row_bytes, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[offset:], (rows, row_bytes), (pitch, 1))
    view[:] = np.frombuffer(plane, np.uint8).reshape(rows, row_bytes)
    return buf


def upload(planes, w, h, layout, seed=0):
    """the picture in device memory in one of the three layouts: (descriptor, the tensors that hold it)"""
    import torch
    rng = np.random.default_rng(seed)
    y, u, v = planes
    pic = Picture(format=PIC_I420, reserved=0)
    if layout == "tight_i420":
        t = torch.from_numpy(np.frombuffer(y + u + v, np.uint8).copy()).cuda()
        pic.plane[0], pic.plane[1], pic.plane[2] = t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4
        pic.pitch[0], pic.pitch[1], pic.pitch[2] = w, w // 2, w // 2
        return pic, [t]
    if layout == "offset_i420":
        geometry = [(y, h, w, w + 13, 1), (u, h // 2, w // 2, w // 2 + 7, 2), (v, h // 2, w // 2, w // 2 + 3, 3)]
    else:
        uv = np.stack([np.frombuffer(u, np.uint8), np.frombuffer(v, np.uint8)], axis=1).tobytes()
        geometry = [(y, h, w, w + 6, 0), (uv, h // 2, w, w + 6, 0)]
        pic.format = PIC_NV12
    keep = []
    for c, (plane, rows, row_bytes, pitch, offset) in enumerate(geometry):
        t = torch.from_numpy(embed(rng, plane, rows, row_bytes, pitch, offset)).cuda()
        pic.plane[c], pic.pitch[c] = t.data_ptr() + offset, pitch
        keep.append(t)
    return pic, keep


def as_tensors(planes, w, h, form, seed):
    """what Encoder.encode takes: one contiguous [h * 3 // 2, w] tensor, (y, u, v) views into larger tensors, or (y, uv) for NV12"""
    import torch
    y, u, v = planes
    if form == 0:
        return torch.from_numpy(np.frombuffer(y + u + v, np.uint8).copy()).cuda().view(h * 3 // 2, w)
    rng = np.random.default_rng(seed)
    if form == 1:
        views = []
        for plane, rows, cols, pad, left in ((y, h, w, 13, 1), (u, h // 2, w // 2, 7, 2), (v, h // 2, w // 2, 3, 3)):
            big = rng.integers(0, 256, (rows + 2, cols + pad), dtype=np.uint8)
            big[1:rows + 1, left:left + cols] = np.frombuffer(plane, np.uint8).reshape(rows, cols)
            views.append(torch.from_numpy(big).cuda()[1:rows + 1, left:left + cols])
        assert not any(t.is_contiguous() for t in views)
        return tuple(views)
    uv = np.stack([np.frombuffer(u, np.uint8).reshape(h // 2, w // 2), np.frombuffer(v, np.uint8).reshape(h // 2, w // 2)], axis=2)
    return torch.from_numpy(np.frombuffer(y, np.uint8).reshape(h, w).copy()).cuda(), torch.from_numpy(uv.copy()).cuda()


class Source:
    """A source picture in device memory from the (buffer, base, pitch) parts a cases module's lay_out returns - odd base addresses, padded pitches, random bytes around
    the rows, every buffer ending with its plane's last row - uploaded buffer by buffer.  A test module's Source adds the descriptor of its section (over `addresses` and
    `pitches`) and the picture the slot has to hold."""

    def __init__(self, parts):
        import torch
        self.before = [buf for buf, _, _ in parts]
        self.tensors = [torch.from_numpy(buf.copy()).cuda() for buf in self.before]
        self.addresses = [t.data_ptr() + base for t, (_, base, _) in zip(self.tensors, parts)]
        self.pitches = [pitch for _, _, pitch in parts]

    def untouched(self):
        return all(np.array_equal(t.cpu().numpy(), b) for t, b in zip(self.tensors, self.before))


class RgbSource(Source):
    """An RGB picture laid out by rc.lay_out, with the descriptor of section 12f and, as `want`, the I420 picture a slot of its size has to hold"""

    def __init__(self, form, chans, matrix, full, rng, padded=True):
        fmt, pb, offs, planes = rc.lay_out(form, chans, rng, padded)
        super().__init__(planes)
        self.pic = rc.descriptor(fmt, pb, offs, self.addresses, self.pitches, matrix, full)
        self.want = b"".join(p.tobytes() for p in rc.restate(*rc.eight_bit(form, chans), matrix, full))


def rgb_frame(kind, r, g, b, matrix, full, rng):
    """(RGBFrame, the 8-bit R, G, B it stands for) in one of the tensor forms"""
    import torch
    h, w = r.shape
    if kind.startswith("hwc"):
        order = {"hwc3": "rgb", "hwc3_bgr_view": "bgr", "hwc4_rgba": "rgba", "hwc4_bgra_view": "bgra", "hwc4_argb": "argb", "hwc4_abgr": "abgr"}[kind]
        pb, offs = {"rgb": (3, (0, 1, 2)), "bgr": (3, (2, 1, 0)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0)), "argb": (4, (1, 2, 3)), "abgr": (4, (3, 2, 1))}[order]
        view = kind.endswith("_view")
        big = rng.integers(0, 256, (h + (2 if view else 0), w + (5 if view else 0), pb), dtype=np.uint8)
        for c, p in enumerate((r, g, b)):
            big[(1 if view else 0):(1 if view else 0) + h, (3 if view else 0):(3 if view else 0) + w, offs[c]] = p
        t = torch.from_numpy(big).cuda()
        if view:
            t = t[1:1 + h, 3:3 + w]
            assert not t.is_contiguous()
        return RGBFrame(t, order=order, matrix=matrix, full_range=full), [r, g, b]
    dtype = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}[kind.split("_")[1]]
    chans = [r, g, b] if dtype is np.uint8 else rc.as_floats("f16" if dtype is np.float16 else "f32", rng, r, g, b)
    if kind.endswith("_slice"):      # channels 1 .. 3 of a four-channel tensor
        big = np.stack([chans[0] * 0] + chans)
        t = torch.from_numpy(big).cuda()[1:]
    elif kind.endswith("_view"):     # a window of a larger tensor
        big = np.zeros((3, h + 3, w + 7), dtype)
        big[:, 2:2 + h, 5:5 + w] = np.stack(chans)
        t = torch.from_numpy(big).cuda()[:, 2:2 + h, 5:5 + w]
        assert not t.is_contiguous()
    else:
        t = torch.from_numpy(np.stack(chans)).cuda()
    return RGBFrame(t, matrix=matrix, full_range=full), rc.eight_bit("f16" if dtype is np.float16 else "f32" if dtype is np.float32 else "planar8", chans)


# ---- pictures and sums out of device memory ----
class Output:
    """An output picture in device memory in one of the three layouts.  Every buffer is filled with seeded random bytes first and ends with its plane's last row;
    picture() gathers the I420 bytes the export left and asserts that every byte outside the rows is what it was."""

    def __init__(self, w, h, layout, seed=0):
        import torch
        rng = np.random.default_rng(seed)
        self.w, self.h, self.layout = w, h, layout
        self.pic = Picture(format=PIC_NV12 if layout == "nv12" else PIC_I420, reserved=0)
        if layout == "tight_i420":
            geometry = [(h * 3 // 2, w, w, 0)]
        elif layout == "offset_i420":
            geometry = [(h, w, w + 13, 1), (h // 2, w // 2, w // 2 + 7, 2), (h // 2, w // 2, w // 2 + 3, 3)]
        else:
            geometry = [(h, w, w + 6, 0), (h // 2, w, w + 6, 0)]
        self.geometry, self.before, self.tensors = geometry, [], []
        for c, (rows, row_bytes, pitch, offset) in enumerate(geometry):
            buf = rng.integers(0, 256, offset + pitch * (rows - 1) + row_bytes, dtype=np.uint8)
            self.before.append(buf)
            self.tensors.append(torch.from_numpy(buf.copy()).cuda())
        if layout == "tight_i420":
            base = self.tensors[0].data_ptr()
            self.pic.plane[0], self.pic.plane[1], self.pic.plane[2] = base, base + w * h, base + w * h * 5 // 4
            self.pic.pitch[0], self.pic.pitch[1], self.pic.pitch[2] = w, w // 2, w // 2
        else:
            for c, (rows, row_bytes, pitch, offset) in enumerate(geometry):
                self.pic.plane[c], self.pic.pitch[c] = self.tensors[c].data_ptr() + offset, pitch

    def picture(self):
        planes = []
        for (rows, row_bytes, pitch, offset), before, t in zip(self.geometry, self.before, self.tensors):
            after = t.cpu().numpy().copy()
            view = np.lib.stride_tricks.as_strided(after[offset:], (rows, row_bytes), (pitch, 1))
            planes.append(view.copy())
            view[:] = np.lib.stride_tricks.as_strided(before[offset:], (rows, row_bytes), (pitch, 1))
            assert np.array_equal(after, before), f"{self.layout}: bytes outside the picture's rows were written"
        if self.layout == "nv12":
            y, uv = planes
            return y.tobytes() + uv[:, 0::2].tobytes() + uv[:, 1::2].tobytes()
        return b"".join(p.tobytes() for p in planes)


def slot_picture(lib, enc, slot, w, h, layout, seed=0):
    out = Output(w, h, layout, seed)
    assert lib.hmr_gpu_enc_export_source_device(enc, slot, C.byref(out.pic), current_stream()) == 0, lib.hmr_gpu_last_error()
    return out.picture()      # (synchronises; asserts the bytes around the rows)


def first_difference(got, want, w, h):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    k = int(np.flatnonzero(a != b)[0])
    plane, at = ("Y", k) if k < w * h else ("U", k - w * h) if k < w * h * 5 // 4 else ("V", k - w * h * 5 // 4)
    pw = w if plane == "Y" else w // 2
    return f"{int((a != b).sum())} bytes differ, first in {plane} at x = {at % pw}, y = {at // pw}: got {a[k]}, want {b[k]}"


def new_sums(n=1):
    import torch
    return torch.full((n, 3), -7, dtype=torch.int64, device="cuda")


def export_one(lib, enc, out, slot, sums):
    assert lib.hmr_gpu_enc_export_picture_device(enc, C.byref(out.pic) if out is not None else None, slot, C.c_void_p(sums.data_ptr()) if sums is not None else None,
                                                 current_stream()) == 0, lib.hmr_gpu_last_error()


def export_many(lib, encs, outs, slots, sums):
    k = len(encs)
    assert lib.hmr_gpu_enc_export_pictures_device((C.c_void_p * k)(*encs), k, (Picture * k)(*[o.pic for o in outs]) if outs is not None else None,
                                                  (C.c_int * k)(*slots) if slots is not None else None, C.c_void_p(sums.data_ptr()) if sums is not None else None,
                                                  current_stream()) == 0, lib.hmr_gpu_last_error()
