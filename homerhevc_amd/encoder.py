"""The frame encoder on torch tensors: pictures that are already on the GPU in, access units (Annex-B bytes) out.

    cfg = EncoderConfig(1920, 1080, wfpp_num_threads=17)
    enc = Encoder(cfg)
    au, slice_type = enc.encode(frame)          # frame: a uint8 CUDA tensor [H * 3 // 2, W] (I420), or a tuple of plane tensors

    au, slice_type = enc.encode(RGBFrame(rgb))  # rgb: a [3, H, W] tensor (uint8, or float16 / float32 in 0 .. 1) or packed uint8 [H, W, 3 or 4]; BT.709 limited range
    yuv = enc.source()                          # the 4:2:0 picture that frame was encoded from, as a uint8 CUDA tensor
    au, slice_type = enc.encode(YUVFrame((y16, uv16), bits=10, msb_aligned=True))      # P010 from a decoder: int16 / uint16 tensors [H, W], [H / 2, W / 2, 2]; rounded to 8 bits by the ingest
    au, slice_type = enc.encode(YUVFrame((y, u, v), chroma="444"))                     # planar 4:4:4 (a JPEG decoder): chroma averaged 2 x 2;  YUVFrame(yuyv, order="yuyv"): packed 4:2:2

    ladder = BatchEncoder([EncoderConfig(1920, 1080, ...), EncoderConfig(1280, 720, ...), EncoderConfig(960, 544, ...)])
    ladder.step([frame, ScaledFrame(frame, 1920, 1080), ScaledFrame(frame, 1920, 1080)])      # one 1080p picture, area-averaged down to each rung by ONE launch
    ladder.step([RGBFrame(rgb)] + [ScaledRGBFrame(RGBFrame(rgb), 1920, 1080)] * 2)            # the same from an RGB frame: converted and averaged by ONE launch (and one for the top rung)
    small.encode(ScaledRGBFrame(RGBFrame(render[:, 60:2100, 120:3720]), 3600, 2040))          # a crop of a 2160p render into a smaller encoder: no encoder of the source's size
    p010 = YUVFrame((y16, uv16), bits=10, msb_aligned=True)                                   # a decoder's 2160p picture
    ladder.step([ScaledYUVFrame(p010, 3840, 2160)] * 3)                                       # rounded to 8 bits and averaged down to each rung by ONE launch

    rec, ssd = enc.export(ssd=True)             # the reconstructed picture as a uint8 CUDA tensor, the sums of squared differences to `frame` as int64 [3]
    y, u, v = psnr(ssd.tolist(), 1920, 1080)    # the reference's PSNR (homer_psnr)
    sums = enc.ssim()                           # the exact fixed-point SSIM sums between the reconstructed picture and `frame` as int64 [3], by one launch of k_ssim
    y, u, v = ssim(sums.tolist(), 1920, 1080)   # the mean SSIM of each plane, 1.0 for identical pictures
    out, ssd = enc.export_rgb(dtype=torch.float16, reference=RGBFrame(rgb))     # the reconstructed picture as RGB [3, H, W], the sums of squared differences to `rgb` as int64 [3]
    r, g, b, all3 = psnr_rgb(ssd.tolist(), 1920, 1080)                          # PSNR against the RGB frame that was supplied

    policy = SceneCut(share=0.5, min_gap=20, groups=[[0, 1, 2]])                # one ladder: its rungs get their intra pictures on the same frame
    ladder.step(frames, scene_cut=policy)                                       # one launch of k_cut over this step's and the last step's pictures decides; ladder.last_cuts
    stats = enc.cut_stats()                                                     # the eight exact statistics of the last frame against the one before, int64 [8]
    sad, hist, share, ratio = cut_score(stats.tolist(), 1920, 1080)             # share: the part of the 8 x 8 blocks that the previous frame does not explain

ctypes on the C ABI of libhomer_gpu.so (include/homer_gpu.h sections 12, 12d, 12e, 12f, 12g, 12h, 12i, 12j, 12k, 12l and 12m).  The pictures go from the tensors into the encoder's picture slots by one launch of
the ingest kernel (k_ingest, csrc/picture_io.hip; RGB frames: k_ingest_rgb, which converts colour in the same pass; YUVFrame - more than 8 bits, 4:2:2, 4:4:4, packed -: k_ingest_yuv, which rounds to 8-bit 4:2:0 in the same pass; scaled frames: k_downscale, which area-averages in the same pass; scaled RGB frames: k_rgb_ladder, which does both; scaled YUVFrames: k_yuv_ladder, which rounds and averages) and the reconstructed pictures and their quality sums come back by one launch of the egress kernel (k_egress, same file), the SSIM sums by one launch of k_ssim (same file), the scene-cut statistics of a slot against the slot of the frame before by one launch of k_cut (same file), RGB pictures and the sums against an RGB reference by one launch of k_egress_rgb (same file), all
ordered against torch's current stream by events: nothing is copied to the host, and neither side waits for the other on the host (a SceneCut policy reads its
statistics on the host before the encode call: the one wait it adds).
Importing this module needs neither torch nor a GPU; constructing an encoder without a GPU raises with the library's error text.
"""
import ctypes as C

from .build import LIB_PATH

PIC_I420, PIC_NV12 = 0, 1
RGB_PACKED8, RGB_PLANAR8, RGB_PLANAR_F16, RGB_PLANAR_F32 = 0, 1, 2, 3
YUV_PLANAR, YUV_SEMIPLANAR, YUV_PACKED422 = 0, 1, 2
CHROMAS = {"420": 0, "422": 1, "444": 2}
PAIR_ORDERS = {"uv": (0, 0, 1), "vu": (0, 1, 0)}                                                               # offset[] of a semi-planar picture
PACKED_ORDERS = {"yuyv": (0, 1, 3), "uyvy": (1, 0, 2), "yvyu": (0, 3, 1), "vyuy": (1, 2, 0)}                   # offset[] of a packed 4:2:2 picture
MATRICES = {"bt601": 0, "bt709": 1}
ORDERS = {"rgb": (3, (0, 1, 2)), "bgr": (3, (2, 1, 0)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0)), "argb": (4, (1, 2, 3)), "abgr": (4, (3, 2, 1))}      # pixel bytes, byte of R, G, B
SLICE_P, SLICE_I = 1, 2
IMAGE_AUTO, IMAGE_I = 0, 3          # encoder_in_out_t.image_type
CUT_VALUES = 8                      # HMR_GPU_CUT_VALUES: SAD_Y, SAD_U, SAD_V, HIST, INTRA, INTER, NINTRA, LUMA


class EncoderConfig(C.Structure):
    """hmr_gpu_enc_cfg (the reference's HVENC_Cfg): EncoderConfig(width, height, **fields) with the header's field names as keywords.  Fields that are not given have the
    values of BASELINE.json configs[1]; the VBV buffer follows the bit rate (vbv_size = bitrate, vbv_init = 35 % of it, as the reference's driver sets them) unless given."""
    _fields_ = [("size", C.c_int32), ("profile", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("frame_rate", C.c_float), ("cu_size", C.c_int32),
                ("max_pred_partition_depth", C.c_int32), ("max_intra_tr_depth", C.c_int32), ("max_inter_tr_depth", C.c_int32), ("intra_period", C.c_int32),
                ("gop_size", C.c_int32), ("num_b", C.c_int32), ("num_ref_frames", C.c_int32), ("motion_estimation_precision", C.c_int32), ("qp", C.c_int32),
                ("chroma_qp_offset", C.c_int32), ("num_enc_engines", C.c_int32), ("wfpp_enable", C.c_int32), ("wfpp_num_threads", C.c_int32),
                ("sign_hiding", C.c_int32), ("sample_adaptive_offset", C.c_int32), ("bitrate_mode", C.c_int32), ("bitrate", C.c_int32), ("vbv_size", C.c_int32),
                ("vbv_init", C.c_int32), ("reinit_gop_on_scene_change", C.c_int32), ("rd_mode", C.c_int32), ("performance_mode", C.c_int32)]
    DEFAULTS = dict(profile=1, frame_rate=25.0, cu_size=64, max_pred_partition_depth=4, max_intra_tr_depth=2, max_inter_tr_depth=1, intra_period=100, gop_size=1, num_b=0,
                    num_ref_frames=1, motion_estimation_precision=2, qp=32, chroma_qp_offset=2, num_enc_engines=1, wfpp_enable=1, wfpp_num_threads=1, sign_hiding=1,
                    sample_adaptive_offset=1, bitrate_mode=0, bitrate=20000, reinit_gop_on_scene_change=1, rd_mode=2, performance_mode=2)

    def __init__(self, width, height, **fields):
        names = {f[0] for f in self._fields_}
        unknown = sorted(set(fields) - names)
        if unknown:
            raise TypeError(f"EncoderConfig: no such field(s) {unknown}")
        values = dict(self.DEFAULTS, size=C.sizeof(type(self)), width=int(width), height=int(height))
        values.update(fields)
        values.setdefault("vbv_size", int(values["bitrate"]))
        values.setdefault("vbv_init", int(0.35 * int(values["bitrate"])))
        super().__init__(**{k: (float(v) if k == "frame_rate" else int(v)) for k, v in values.items()})


class Picture(C.Structure):
    """hmr_gpu_picture"""
    _fields_ = [("format", C.c_int32), ("reserved", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int64 * 3)]


class RgbPicture(C.Structure):
    """hmr_gpu_rgb_picture"""
    _fields_ = [("format", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32), ("reserved", C.c_int32), ("pixel_bytes", C.c_int32), ("offset", C.c_int32 * 3),
                ("plane", C.c_void_p * 3), ("pitch", C.c_int64 * 3)]


class YuvPicture(C.Structure):
    """hmr_gpu_yuv_picture"""
    _fields_ = [("format", C.c_int32), ("chroma", C.c_int32), ("bits", C.c_int32), ("msb_aligned", C.c_int32), ("offset", C.c_int32 * 3), ("reserved", C.c_int32),
                ("plane", C.c_void_p * 3), ("pitch", C.c_int64 * 3)]


class ScaledPicture(C.Structure):
    """hmr_gpu_scaled_picture"""
    _fields_ = [("pic", Picture), ("width", C.c_int32), ("height", C.c_int32)]


class ScaledRgbPicture(C.Structure):
    """hmr_gpu_scaled_rgb_picture"""
    _fields_ = [("pic", RgbPicture), ("width", C.c_int32), ("height", C.c_int32)]


class ScaledYuvPicture(C.Structure):
    """hmr_gpu_scaled_yuv_picture"""
    _fields_ = [("pic", YuvPicture), ("width", C.c_int32), ("height", C.c_int32)]


class ScaledFrame:
    """A 4:2:0 picture that is LARGER than the encoder's, for Encoder.encode / BatchEncoder.step: area-averaged down to the encoder's size by the ingest kernel itself, in
    the integer arithmetic of include/homer_gpu.h section 12g (every sample can be reproduced from the formula there; hmr_gpu_scale_host is the same arithmetic on the host).
      frame: anything picture_of takes for a width x height picture (I420 tensor, (y, u, v) or (y, uv) views: a crop is just a view); width, height: ITS size.
    The same frame may be given to any number of sequences of a step - a resolution ladder - and the step makes ONE scaled load call for all of them.  Downscaling only, by
    at most 8 per axis; equal sizes are legal and give what the plain frame gives.  source() returns the scaled picture of each rung, export(ssd=True) gives the sums
    against that SCALED picture, not against `frame`, and export_rgb(source=True) shows the scaled picture as RGB.
    RGB sources are not taken here: ScaledRGBFrame takes them, and fills the slot with exactly what this class makes of the RGBFrame's source()."""

    def __init__(self, frame, width, height):
        if isinstance(frame, (RGBFrame, ScaledFrame, YUVFrame)):
            raise TypeError("ScaledFrame: the frame has to be an 8-bit 4:2:0 picture (what picture_of takes), not an RGBFrame, a YUVFrame or a ScaledFrame")
        self.frame, self.width, self.height = frame, int(width), int(height)


def scaled_picture_of(frame):
    """The descriptor (hmr_gpu_scaled_picture) of a ScaledFrame; nothing is copied.  Returns (ScaledPicture, tensors): keep the tensors until the load call has returned."""
    pic, keep = picture_of(frame.frame, frame.width, frame.height)
    return ScaledPicture(pic=pic, width=frame.width, height=frame.height), keep


class RGBFrame:
    """An RGB picture for Encoder.encode / BatchEncoder.step: converted to 8-bit 4:2:0 by the ingest kernel itself, in the integer arithmetic of include/homer_gpu.h section
    12f (every sample can be reproduced from the table there; hmr_gpu_rgb_convert_host is the same arithmetic on the host).
      tensor: a uint8 CUDA tensor [H, W, 3] or [H, W, 4], packed: unit stride over the channels, a pixel every 3 / 4 bytes, any row stride - `order` names the bytes of a
              pixel: "rgb", "bgr" (3 bytes), "rgba", "bgra", "argb", "abgr" (4 bytes; the alpha byte is ignored);
              or a [3, H, W] tensor of uint8, float16 or float32 (R, G, B planes; floats are clamped to 0 .. 1 and scaled by 255, NaN counts as 0) with unit stride along
              a row - views and channel slices of larger tensors are fine, `order` is ignored.
      matrix: "bt709" or "bt601"; full_range: False for 16 .. 235 / 16 .. 240, True for 0 .. 255.
    The stream does NOT say which matrix or range was used (the parameter sets carry no colour description, as the reference's): tell the decoder's side by other means.
    The same class describes what comes BACK: Encoder.export_rgb writes the reconstructed picture (or the encoded source) into an RGBFrame's tensor in its order, matrix
    and range - the inverse arithmetic of section 12i - and takes the frame that was supplied as `reference` for the sums of squared differences in RGB."""

    def __init__(self, tensor, order="rgb", matrix="bt709", full_range=False):
        if matrix not in MATRICES:
            raise ValueError(f"RGBFrame: matrix has to be one of {sorted(MATRICES)}, got {matrix!r}")
        if order not in ORDERS:
            raise ValueError(f"RGBFrame: order has to be one of {sorted(ORDERS)}, got {order!r}")
        self.tensor, self.order, self.matrix, self.full_range = tensor, order, matrix, bool(full_range)


def rgb_picture_of(frame, width, height):
    """The descriptor (hmr_gpu_rgb_picture) of a width x height RGBFrame; nothing is copied, the tensor's strides become the pitches.  Returns (RgbPicture, tensors): keep
    the tensors until the load call that takes the descriptor has returned."""
    import torch
    w, h, t = int(width), int(height), frame.tensor
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 3:
        raise TypeError("rgb_picture_of: the frame has to be a three-dimensional CUDA tensor")
    pic = RgbPicture(matrix=MATRICES[frame.matrix], full_range=int(frame.full_range), reserved=0)
    if tuple(t.shape[:2]) == (h, w) and t.shape[2] in (3, 4) and t.dtype == torch.uint8 and tuple(t.shape) != (3, h, w):
        pixel_bytes, offsets = ORDERS[frame.order]
        if pixel_bytes != t.shape[2]:
            raise ValueError(f"rgb_picture_of: order {frame.order!r} names {pixel_bytes} bytes a pixel, the tensor has {t.shape[2]}")
        if t.stride(2) != 1 or t.stride(1) != pixel_bytes:
            raise ValueError(f"rgb_picture_of: a packed frame has to have unit stride over the channels and a pixel every {pixel_bytes} bytes, got strides {t.stride()}")
        pic.format, pic.pixel_bytes = RGB_PACKED8, pixel_bytes
        pic.offset[0], pic.offset[1], pic.offset[2] = offsets
        pic.plane[0], pic.pitch[0] = t.data_ptr(), t.stride(0)
        return pic, (t,)
    formats = {torch.uint8: RGB_PLANAR8, torch.float16: RGB_PLANAR_F16, torch.float32: RGB_PLANAR_F32}
    if tuple(t.shape) != (3, h, w) or t.dtype not in formats:
        raise ValueError(f"rgb_picture_of: a uint8 tensor [{h}, {w}, 3 or 4] or a uint8 / float16 / float32 tensor [3, {h}, {w}], got {t.dtype} {tuple(t.shape)}")
    if t.stride(2) != 1:
        raise ValueError(f"rgb_picture_of: a planar frame has to have unit stride along a row, got strides {t.stride()}")
    pic.format, pic.pixel_bytes = formats[t.dtype], 0
    for c in range(3):
        pic.plane[c], pic.pitch[c] = t.data_ptr() + c * t.stride(0) * t.element_size(), t.stride(1) * t.element_size()
    return pic, (t,)


class YUVFrame:
    """A Y'CbCr picture that is not 8-bit 4:2:0 I420 / NV12, for Encoder.encode / BatchEncoder.step: more than 8 bits, 4:2:2 or 4:4:4, NV21, packed.  Rounded to 8-bit 4:2:0
    by the ingest kernel itself (k_ingest_yuv), in the integer arithmetic of include/homer_gpu.h section 12k: ONE rounding per sample, chroma averaged over its 1, 2 or 4
    taps, no range, matrix or transfer conversion, no dithering (hmr_gpu_yuv_convert_host is the same arithmetic on the host).
      planes: (y, u, v)  planar: [H, W] and two [Hc, Wc] tensors;
              (y, uv)    semi-planar: uv [Hc, Wc, 2] or [Hc, 2 Wc]; order "uv" (NV12, P010: the default) or "vu" (NV21);
              one tensor [H, W, 2] or [H, 2 W]: packed 4:2:2; order "yuyv" (the default), "uyvy", "yvyu" or "vyuy"; chroma has to be "422";
              Wc = W / 2 for chroma "420" and "422", W for "444"; Hc = H / 2 for "420", H otherwise.
      bits: 8 .. 16.  uint8 tensors for 8 bits; int16 - or uint16 where torch has it - for more (the 16 bits are read as unsigned either way).
      msb_aligned: the sample lies in the container's high bits (P010, P016's 12-bit form, Y210) rather than in its low bits (yuv420p10le).
    The tensors need unit stride along a row; views and crops of larger tensors are fine.  source(), export(ssd=True), ssim() and export_rgb(source=True) then see the
    8-bit picture that was encoded.  A ScaledFrame does not take one; a ScaledYUVFrame does."""

    def __init__(self, planes, chroma="420", bits=8, msb_aligned=False, order=None):
        chroma = str(chroma)
        if chroma not in CHROMAS:
            raise ValueError(f"YUVFrame: chroma has to be one of {sorted(CHROMAS)}, got {chroma!r}")
        if not 8 <= int(bits) <= 16:
            raise ValueError(f"YUVFrame: bits has to be 8 .. 16, got {bits!r}")
        planes = tuple(planes) if isinstance(planes, (tuple, list)) else (planes,)
        if len(planes) not in (1, 2, 3):
            raise ValueError("YUVFrame: (y, u, v), (y, uv) or one packed tensor")
        orders = {1: PACKED_ORDERS, 2: PAIR_ORDERS, 3: {None: (0, 0, 0)}}[len(planes)]
        if order is None:
            order = {1: "yuyv", 2: "uv", 3: None}[len(planes)]
        if order not in orders:
            raise ValueError(f"YUVFrame: order has to be one of {sorted(k for k in orders if k)} for {len(planes)} tensor(s), got {order!r}")
        if len(planes) == 1 and chroma != "422":
            raise ValueError("YUVFrame: a packed picture is 4:2:2")
        self.planes, self.chroma, self.bits, self.msb_aligned, self.order = planes, chroma, int(bits), bool(msb_aligned), order
        self.offsets = orders[order]


def yuv_picture_of(frame, width, height):
    """The descriptor (hmr_gpu_yuv_picture) of a width x height YUVFrame; nothing is copied, the tensors' strides become the pitches.  Returns (YuvPicture, tensors): keep
    the tensors until the load call that takes the descriptor has returned."""
    import torch
    w, h = int(width), int(height)
    wide = frame.bits > 8
    dtypes = (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ()) if wide else (torch.uint8,)
    sb = 2 if wide else 1
    planes = list(frame.planes)
    for i, t in enumerate(planes):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes:
            raise TypeError(f"yuv_picture_of: plane {i} has to be a CUDA tensor of {' or '.join(str(d) for d in dtypes)} for {frame.bits} bits")
    wc, hc = (w if frame.chroma == "444" else w // 2), (h // 2 if frame.chroma == "420" else h)
    pic = YuvPicture(format=(YUV_PACKED422, YUV_SEMIPLANAR, YUV_PLANAR)[len(planes) - 1], chroma=CHROMAS[frame.chroma], bits=frame.bits, msb_aligned=int(frame.msb_aligned), reserved=0)
    pic.offset[0], pic.offset[1], pic.offset[2] = frame.offsets

    def rows_of(t, rows, cols, group, what):
        """t as [rows, cols * group] with unit stride along a row: [rows, cols, group] tensors have their groups next to each other"""
        if t.dim() == 3 and group > 1:
            if tuple(t.shape) != (rows, cols, group) or t.stride(2) != 1 or t.stride(1) != group:
                raise ValueError(f"yuv_picture_of: {what} has to be [{rows}, {cols}, {group}] with the samples of a group next to each other, got {tuple(t.shape)} with strides {t.stride()}")
            return t.as_strided((rows, cols * group), (t.stride(0), 1))
        if t.dim() != 2 or tuple(t.shape) != (rows, cols * group) or t.stride(1) != 1:
            raise ValueError(f"yuv_picture_of: {what} has to be [{rows}, {cols * group}] with unit stride along a row, got {tuple(t.shape)} with strides {t.stride()}")
        return t

    if len(planes) == 1:
        planes = [rows_of(planes[0], h, w, 2, "the packed picture")]
    elif len(planes) == 2:
        planes = [rows_of(planes[0], h, w, 1, "the luma plane"), rows_of(planes[1], hc, wc, 2, "the plane of pairs")]
    else:
        planes = [rows_of(planes[0], h, w, 1, "the luma plane"), rows_of(planes[1], hc, wc, 1, "the U plane"), rows_of(planes[2], hc, wc, 1, "the V plane")]
    for c, t in enumerate(planes):
        pic.plane[c], pic.pitch[c] = t.data_ptr(), t.stride(0) * sb
    return pic, tuple(planes)


class ScaledRGBFrame:
    """An RGB picture that is LARGER than the encoder's, for Encoder.encode / BatchEncoder.step: converted to 8-bit 4:2:0 and area-averaged down to the encoder's size by
    ONE launch of the ingest kernel k_rgb_ladder (include/homer_gpu.h section 12j).  No new arithmetic: the slot holds section 12g's average of the picture section 12f
    makes of the frame - what encoding the RGBFrame at its own size, taking source() and giving that to a ScaledFrame would put there, bit for bit - but no encoder of
    the source's size is needed and the picture in between never exists (hmr_gpu_scale_rgb_host is the same arithmetic on the host).
      frame: an RGBFrame of width x height pixels - any of its tensor forms, orders, matrices and ranges; a crop is just a view; width, height: ITS size.
    The same frame may be given to any number of sequences of a step and the step makes ONE load call for all its ScaledRGBFrames.  Downscaling only, by at most 8 per
    axis; equal sizes are legal and give what the RGBFrame itself gives.  source() returns the scaled 4:2:0 picture, export(ssd=True) and ssim() measure against that
    picture, and export_rgb(source=True) shows it as RGB."""

    def __init__(self, frame, width, height):
        if not isinstance(frame, RGBFrame):
            raise TypeError("ScaledRGBFrame: the frame has to be an RGBFrame (a 4:2:0 picture goes into a ScaledFrame)")
        self.frame, self.width, self.height = frame, int(width), int(height)


def scaled_rgb_picture_of(frame):
    """The descriptor (hmr_gpu_scaled_rgb_picture) of a ScaledRGBFrame; nothing is copied.  Returns (ScaledRgbPicture, tensors): keep the tensors until the load call has
    returned."""
    pic, keep = rgb_picture_of(frame.frame, frame.width, frame.height)
    return ScaledRgbPicture(pic=pic, width=frame.width, height=frame.height), keep


class ScaledYUVFrame:
    """A Y'CbCr picture of more than 8 bits, 4:2:2, 4:4:4 or packed that is LARGER than the encoder's, for Encoder.encode / BatchEncoder.step: rounded to 8-bit 4:2:0 and
    area-averaged down to the encoder's size by ONE launch of the ingest kernel k_yuv_ladder (include/homer_gpu.h section 12l).  No new arithmetic: the slot holds section
    12g's average of the picture section 12k makes of the frame - what encoding the YUVFrame at its own size, taking source() and giving that to a ScaledFrame would put
    there in three launches, bit for bit - but no encoder of the source's size is needed and the picture in between never exists (hmr_gpu_scale_yuv_host is the same
    arithmetic on the host).
      frame: a YUVFrame of width x height pixels - any of its layouts, depths, alignments and chroma formats; a crop is just a view; width, height: ITS size.
    The same frame may be given to any number of sequences of a step and the step makes ONE load call for all its ScaledYUVFrames.  Downscaling only, by at most 8 per
    axis; equal sizes are legal and give what the YUVFrame itself gives.  source() returns the scaled 8-bit 4:2:0 picture, export(ssd=True) and ssim() measure against that
    picture, and export_rgb(source=True) shows it as RGB."""

    def __init__(self, frame, width, height):
        if not isinstance(frame, YUVFrame):
            raise TypeError("ScaledYUVFrame: the frame has to be a YUVFrame (an 8-bit 4:2:0 picture goes into a ScaledFrame, an RGBFrame into a ScaledRGBFrame)")
        self.frame, self.width, self.height = frame, int(width), int(height)


def scaled_yuv_picture_of(frame):
    """The descriptor (hmr_gpu_scaled_yuv_picture) of a ScaledYUVFrame; nothing is copied.  Returns (ScaledYuvPicture, tensors): keep the tensors until the load call has
    returned."""
    pic, keep = yuv_picture_of(frame.frame, frame.width, frame.height)
    return ScaledYuvPicture(pic=pic, width=frame.width, height=frame.height), keep


_lib = None
_host_lib = None


def _declare_metrics(lib):
    lib.hmr_gpu_last_error.restype = C.c_char_p
    lib.hmr_gpu_psnr.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.hmr_gpu_psnr_rgb.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.hmr_gpu_ssim.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.hmr_gpu_cut_score.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(C.c_double)]
    return lib


def _metric_library():
    """the handle psnr, psnr_rgb, ssim and cut_score call through: load_library()'s once it has run, else one cached handle that needs neither torch nor a GPU"""
    global _host_lib
    if _lib is not None:
        return _lib
    if _host_lib is None:
        _host_lib = _declare_metrics(C.CDLL(LIB_PATH))
    return _host_lib


def psnr(ssd, width, height):
    """homer_psnr's three values (Y, U, V, in dB; 99.99 for a zero sum) of three sums of squared differences - Python ints, e.g. export(ssd=True)[1].tolist() - of a
    width x height 4:2:0 picture, through hmr_gpu_psnr.  Pure host arithmetic: needs neither torch nor a GPU."""
    lib = _metric_library()
    sums = [int(v) for v in ssd]
    if len(sums) != 3 or min(sums) < 0:
        raise ValueError(f"psnr: three non-negative sums, got {sums}")
    out = (C.c_double * 3)()
    if lib.hmr_gpu_psnr((C.c_uint64 * 3)(*sums), int(width), int(height), out) != 0:
        raise ValueError((lib.hmr_gpu_last_error() or b"hmr_gpu_psnr").decode(errors="replace"))
    return tuple(out)


def psnr_rgb(ssd, width, height):
    """PSNR in dB of R, G, B and of the three together (99.99 for a zero sum) from three sums of squared differences - Python ints, e.g. export_rgb(reference=...)[1].tolist()
    - of a width x height RGB picture, through hmr_gpu_psnr_rgb (include/homer_gpu.h section 12i).  Pure host arithmetic: needs neither torch nor a GPU."""
    lib = _metric_library()
    sums = [int(v) for v in ssd]
    if len(sums) != 3 or min(sums) < 0:
        raise ValueError(f"psnr_rgb: three non-negative sums, got {sums}")
    out = (C.c_double * 4)()
    if lib.hmr_gpu_psnr_rgb((C.c_uint64 * 3)(*sums), int(width), int(height), out) != 0:
        raise ValueError((lib.hmr_gpu_last_error() or b"hmr_gpu_psnr_rgb").decode(errors="replace"))
    return tuple(out)


def ssim(sums, width, height):
    """The mean SSIM of each plane (Y, U, V; 1.0 for identical pictures, negative for inverted ones) from three SSIM sums - Python ints, e.g. Encoder.ssim().tolist() - of a
    width x height 4:2:0 picture, through hmr_gpu_ssim: sum / (2^30 x the plane's windows), include/homer_gpu.h section 12h.  Pure host arithmetic: needs neither torch
    nor a GPU."""
    lib = _metric_library()
    values = [int(v) for v in sums]
    if len(values) != 3 or not all(-(1 << 63) <= v < 1 << 63 for v in values):
        raise ValueError(f"ssim: three 64-bit sums, got {values}")
    out = (C.c_double * 3)()
    if lib.hmr_gpu_ssim((C.c_int64 * 3)(*values), int(width), int(height), out) != 0:
        raise ValueError((lib.hmr_gpu_last_error() or b"hmr_gpu_ssim").decode(errors="replace"))
    return tuple(out)


def cut_score(stats, width, height):
    """The four scores of a frame against its predecessor from the eight scene-cut statistics - Python ints, e.g. Encoder.cut_stats().tolist() - of a width x height
    picture, through hmr_gpu_cut_score (include/homer_gpu.h section 12m): (SAD_Y / (W H), HIST / (2 W H), NINTRA / blocks, INTER / INTRA or 1.0 when INTRA is 0), each
    the correctly rounded quotient.  Pure host arithmetic: needs neither torch nor a GPU."""
    lib = _metric_library()
    values = [int(v) for v in stats]
    if len(values) != CUT_VALUES or not all(-(1 << 63) <= v < 1 << 63 for v in values):
        raise ValueError(f"cut_score: eight 64-bit values, got {values}")
    out = (C.c_double * 4)()
    if lib.hmr_gpu_cut_score((C.c_int64 * CUT_VALUES)(*values), int(width), int(height), out) != 0:
        raise ValueError((lib.hmr_gpu_last_error() or b"hmr_gpu_cut_score").decode(errors="replace"))
    return tuple(out)


def _au_is_intra(au):
    """an access unit holds an intra picture: one of its NAL units is an IRAP slice (types 16 .. 23; the encoder writes every I slice as an IDR picture)"""
    at = au.find(b"\x00\x00\x01")
    while 0 <= at < len(au) - 3:
        if 16 <= (au[at + 3] >> 1) & 0x3f <= 23:
            return True
        at = au.find(b"\x00\x00\x01", at + 3)
    return False


class SceneCut:
    """The policy that turns scene-cut statistics into intra pictures, for Encoder.encode(..., scene_cut=policy) and BatchEncoder.step(..., scene_cut=policy).  Pure
    Python on the statistics' rows: needs neither torch nor a GPU.  One object serves one encoder for its whole life (it counts that encoder's frames).
    A sequence CUTS in a step when all three hold: it has a pair (it was given a picture in the immediately preceding step too); cut_score's share of blocks that the
    previous frame does not explain, NINTRA / blocks, is at least `share`; and at least `min_gap` frames have passed since the last intra picture the object saw for
    it - one it forced, one the caller asked for, or one the encoder returned as slice type I (a pipelined BatchEncoder returns a frame's access unit one step late,
    so an intra picture the encoder chose by itself is seen one frame late).  20 is the reference's own distance (hmr_motion_inter.c:3791).
    groups: lists of sequence indices, each one ladder: the group's first member that has a picture in the step decides for all its members that have one, so the
    rungs get their intra pictures on the same frame.  Sequences in no group decide alone."""

    def __init__(self, share=0.5, min_gap=20, groups=None):
        self.share, self.min_gap = float(share), int(min_gap)
        self.groups = [[int(i) for i in g] for g in (groups or [])]
        members = [i for g in self.groups for i in g]
        if len(set(members)) != len(members) or min(members, default=0) < 0:
            raise ValueError(f"SceneCut: a sequence belongs to one group at most, indices start at 0: {self.groups}")
        self.frames = {}           # sequence -> the pictures it has been given
        self.last_intra = {}       # sequence -> the number of its last intra picture (absent: none seen)

    def wants(self, i, row, size):
        """sequence i alone: its row (eight values; None or all -1: no pair) of a picture of `size` says cut, and its last intra picture is far enough back"""
        if row is None or all(int(v) == -1 for v in row):
            return False
        if i in self.last_intra and self.frames.get(i, 0) - self.last_intra[i] < self.min_gap:
            return False
        return cut_score(row, size[0], size[1])[2] >= self.share

    def decide(self, live, rows, sizes, image_types=None):
        """One step.  live: the sequences that have a picture in it; rows[i], sizes[i], image_types[i]: the statistics (None or all -1: no pair), the (width, height)
        and the image type the caller asked for, per SEQUENCE.  Returns one bool per sequence: the policy's decision.  The step's pictures are counted, and the intra
        pictures that follow - decided here or asked for by the caller - are remembered."""
        cuts = [False] * len(rows)
        grouped = set()
        for g in self.groups:
            members = [i for i in g if i in live]
            grouped.update(g)
            if members and self.wants(members[0], rows[members[0]], sizes[members[0]]):
                for i in members:
                    cuts[i] = True
        for i in live:
            if i not in grouped:
                cuts[i] = self.wants(i, rows[i], sizes[i])
        for i in live:
            if cuts[i] or (image_types is not None and int(image_types[i]) == IMAGE_I):
                self.last_intra[i] = self.frames.get(i, 0)
            self.frames[i] = self.frames.get(i, 0) + 1
        return cuts

    def observe(self, i, intra, back=0):
        """what the encoder returned for sequence i's picture `back` pictures before its last: an intra picture is remembered"""
        if intra:
            self.last_intra[i] = max(self.last_intra.get(i, -1), self.frames.get(i, 0) - 1 - back)


def load_library():
    """libhomer_gpu.so with the argument types of the calls this module makes.  torch brings up its HIP runtime first where it finds a GPU."""
    global _lib
    if _lib is None:
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        lib = _declare_metrics(C.CDLL(LIB_PATH))
        P, I, L = C.c_void_p, C.c_int, C.c_long
        lib.hmr_gpu_create.argtypes = [C.POINTER(P), I, P]
        lib.hmr_gpu_destroy.argtypes = [P]
        lib.hmr_gpu_enc_create.argtypes = [P, C.POINTER(EncoderConfig), C.POINTER(P)]
        lib.hmr_gpu_enc_destroy.argtypes = [P]
        lib.hmr_gpu_picture_check.argtypes = [C.POINTER(Picture), I, I]
        lib.hmr_gpu_enc_load_source_device.argtypes = [P, I, C.POINTER(Picture), P]
        lib.hmr_gpu_enc_load_sources_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(Picture), P]
        lib.hmr_gpu_enc_load_source_rgb_device.argtypes = [P, I, C.POINTER(RgbPicture), P]
        lib.hmr_gpu_enc_load_sources_rgb_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(RgbPicture), P]
        lib.hmr_gpu_enc_load_source_yuv_device.argtypes = [P, I, C.POINTER(YuvPicture), P]
        lib.hmr_gpu_enc_load_sources_yuv_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(YuvPicture), P]
        lib.hmr_gpu_enc_load_source_scaled_device.argtypes = [P, I, C.POINTER(ScaledPicture), P]
        lib.hmr_gpu_enc_load_sources_scaled_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(ScaledPicture), P]
        lib.hmr_gpu_enc_load_source_scaled_rgb_device.argtypes = [P, I, C.POINTER(ScaledRgbPicture), P]
        lib.hmr_gpu_enc_load_sources_scaled_rgb_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(ScaledRgbPicture), P]
        lib.hmr_gpu_enc_load_source_scaled_yuv.argtypes = [P, I, C.POINTER(ScaledYuvPicture), P]
        lib.hmr_gpu_enc_load_sources_scaled_yuv.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(ScaledYuvPicture), P]
        lib.hmr_gpu_enc_export_sources_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(Picture), P]
        lib.hmr_gpu_enc_encode_source.argtypes = [P, I, I, C.c_char_p, L, C.POINTER(L), C.c_char_p]
        lib.hmr_gpu_enc_export_pictures_device.argtypes = [C.POINTER(P), I, C.POINTER(Picture), C.POINTER(I), P, P]
        lib.hmr_gpu_enc_ssim_device.argtypes = [C.POINTER(P), I, C.POINTER(I), P, P]
        lib.hmr_gpu_enc_cut_stats.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(I), P, P]
        lib.hmr_gpu_enc_export_pictures_rgb_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(RgbPicture), C.POINTER(RgbPicture), P, P]
        batch = [C.POINTER(P), I, C.POINTER(I), C.POINTER(I), C.POINTER(C.c_char_p), C.POINTER(L), C.POINTER(L)]
        lib.hmr_gpu_enc_encode_batch.argtypes = batch
        lib.hmr_gpu_enc_encode_batch_pipelined.argtypes = batch
        _lib = lib
    return _lib


def _fail(lib, what):
    raise RuntimeError(f"{what}: {(lib.hmr_gpu_last_error() or b'').decode(errors='replace')}")


def _plane(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
        raise TypeError(f"picture_of: {what} has to be a uint8 CUDA tensor")
    return t


def picture_of(frame, width, height):
    """The descriptor (hmr_gpu_picture) of a width x height 4:2:0 picture held by uint8 CUDA tensors; nothing is copied, the tensors' strides become the pitches.
      one tensor [height * 3 // 2, width], contiguous      I420: the luma rows, then the U plane, then the V plane (each width / 2 x height / 2, tightly packed)
      (y, u, v): [height, width], 2 x [height / 2, width / 2]  I420 planes; any row stride, unit stride along a row (views into larger tensors are fine)
      (y, uv): [height, width], [height / 2, width / 2, 2] or [height / 2, width]  NV12: uv holds the U, V pairs of a row next to each other
    Returns (Picture, tensors): keep the tensors until the load call that takes the descriptor has returned."""
    w, h = int(width), int(height)
    pic = Picture(format=PIC_I420, reserved=0)
    if not isinstance(frame, (tuple, list)):
        t = _plane(frame, "the frame")
        if tuple(t.shape) != (h * 3 // 2, w) or not t.is_contiguous():
            raise ValueError(f"picture_of: a single tensor has to be contiguous [{h * 3 // 2}, {w}] (I420), got {tuple(t.shape)} with strides {t.stride()}")
        base = t.data_ptr()
        pic.plane[0], pic.plane[1], pic.plane[2] = base, base + w * h, base + w * h + (w // 2) * (h // 2)
        pic.pitch[0], pic.pitch[1], pic.pitch[2] = w, w // 2, w // 2
        return pic, (t,)
    planes = [_plane(t, f"plane {i}") for i, t in enumerate(frame)]
    if len(planes) == 2 and planes[1].dim() == 3:
        uv = planes[1]
        if tuple(uv.shape) != (h // 2, w // 2, 2) or uv.stride(2) != 1 or uv.stride(1) != 2:
            raise ValueError(f"picture_of: the UV plane has to be [{h // 2}, {w // 2}, 2] with the pairs next to each other, got {tuple(uv.shape)} with strides {uv.stride()}")
        planes[1] = uv.as_strided((h // 2, w), (uv.stride(0), 1))
    if len(planes) not in (2, 3):
        raise ValueError("picture_of: (y, u, v) for I420 or (y, uv) for NV12")
    shapes = [(h, w), (h // 2, w)] if len(planes) == 2 else [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    pic.format = PIC_NV12 if len(planes) == 2 else PIC_I420
    for c, (t, shape) in enumerate(zip(planes, shapes)):
        if tuple(t.shape) != shape or t.stride(1) != 1:
            raise ValueError(f"picture_of: plane {c} has to be {list(shape)} with unit stride along a row, got {tuple(t.shape)} with strides {t.stride()}")
        pic.plane[c], pic.pitch[c] = t.data_ptr(), t.stride(0)
    return pic, tuple(planes)


def _stream_of(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _output(cfg, out, nv12, device):
    """the tensor(s) an export writes: `out` (what picture_of takes), or a new I420 tensor / NV12 pair"""
    import torch
    if out is not None:
        return out
    w, h = int(cfg.width), int(cfg.height)
    if nv12:
        return (torch.empty((h, w), dtype=torch.uint8, device=f"cuda:{device}"), torch.empty((h // 2, w // 2, 2), dtype=torch.uint8, device=f"cuda:{device}"))
    return torch.empty((h * 3 // 2, w), dtype=torch.uint8, device=f"cuda:{device}")


def _outputs(cfgs, outs, nv12, device):
    """the output descriptors of an export: (Picture array, the tensors written, the tensors to keep until the call has returned)"""
    pics, results, keep = (Picture * len(cfgs))(), [], []
    for k, cfg in enumerate(cfgs):
        target = _output(cfg, outs[k] if outs is not None else None, nv12, device)
        pics[k], t = picture_of(target, cfg.width, cfg.height)
        keep.append(t)
        results.append(target)
    return pics, results, keep


def _export(lib, device, encs, cfgs, slot, picture, ssd, outs, nv12):
    """ONE hmr_gpu_enc_export_pictures_device for the encoders `encs`: (their pictures or None, an int64 tensor [len(encs), 3] or None)"""
    import torch
    n = len(encs)
    if not picture and not ssd:
        raise ValueError("export: neither the picture nor the sums asked for")
    pics, results, keep = _outputs(cfgs, outs, nv12, device) if picture else (None, None, [])
    sums = torch.empty((n, 3), dtype=torch.int64, device=f"cuda:{device}") if ssd else None
    if lib.hmr_gpu_enc_export_pictures_device((C.c_void_p * n)(*encs), n, pics, (C.c_int * n)(*([slot] * n)) if ssd else None,
                                              C.c_void_p(sums.data_ptr()) if ssd else None, _stream_of(device)) != 0:
        _fail(lib, "hmr_gpu_enc_export_pictures_device")
    del keep
    return results, sums


def _ssim(lib, device, encs, slot):
    """ONE hmr_gpu_enc_ssim_device for the encoders `encs`: an int64 tensor [len(encs), 3]"""
    import torch
    n = len(encs)
    sums = torch.empty((n, 3), dtype=torch.int64, device=f"cuda:{device}")
    if lib.hmr_gpu_enc_ssim_device((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([slot] * n)), C.c_void_p(sums.data_ptr()), _stream_of(device)) != 0:
        _fail(lib, "hmr_gpu_enc_ssim_device")
    return sums


def _cut_stats(lib, device, encs, slot):
    """ONE hmr_gpu_enc_cut_stats for the encoders `encs`, slot `slot` against the other slot: an int64 tensor [len(encs), 8]"""
    import torch
    n = len(encs)
    stats = torch.empty((n, CUT_VALUES), dtype=torch.int64, device=f"cuda:{device}")
    if lib.hmr_gpu_enc_cut_stats((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([slot] * n)), (C.c_int * n)(*([slot ^ 1] * n)), C.c_void_p(stats.data_ptr()), _stream_of(device)) != 0:
        _fail(lib, "hmr_gpu_enc_cut_stats")
    return stats


def _cut_table(lib, device, encs, sequences, pairs, slot):
    """the statistics of the sequences `pairs` (indices into encs; slot `slot` against the other slot) as an int64 tensor [sequences, 8]; every other row is -1"""
    import torch
    table = torch.full((sequences, CUT_VALUES), -1, dtype=torch.int64, device=f"cuda:{device}")
    if pairs:
        table[torch.tensor(pairs, device=table.device)] = _cut_stats(lib, device, [encs[i] for i in pairs], slot)
    return table


# What a frame class is loaded by: (ctypes struct, C call, the function that describes frame k of a step).  Consulted in this order; anything else is what
# picture_of takes (a tensor or a tuple of tensors) and goes through _PLAIN_LOAD.
_PLAIN_LOAD = (Picture, "hmr_gpu_enc_load_sources_device", lambda f, cfg: picture_of(f, cfg.width, cfg.height))
_FRAME_LOADS = [
    (RGBFrame, (RgbPicture, "hmr_gpu_enc_load_sources_rgb_device", lambda f, cfg: rgb_picture_of(f, cfg.width, cfg.height))),
    (YUVFrame, (YuvPicture, "hmr_gpu_enc_load_sources_yuv_device", lambda f, cfg: yuv_picture_of(f, cfg.width, cfg.height))),
    (ScaledFrame, (ScaledPicture, "hmr_gpu_enc_load_sources_scaled_device", lambda f, cfg: scaled_picture_of(f))),
    (ScaledRGBFrame, (ScaledRgbPicture, "hmr_gpu_enc_load_sources_scaled_rgb_device", lambda f, cfg: scaled_rgb_picture_of(f))),
    (ScaledYUVFrame, (ScaledYuvPicture, "hmr_gpu_enc_load_sources_scaled_yuv", lambda f, cfg: scaled_yuv_picture_of(f))),
]


def _load(lib, device, encs, cfgs, slot, frames):
    """the frames (what picture_of takes, RGBFrame, YUVFrame, ScaledFrame, ScaledRGBFrame or ScaledYUVFrame) into slot `slot` of their encoders: ONE load call per kind of frame"""
    members = {load: [] for load in [_PLAIN_LOAD] + [load for _, load in _FRAME_LOADS]}      # (in the order the calls are made)
    for k, f in enumerate(frames):
        members[next((load for cls, load in _FRAME_LOADS if isinstance(f, cls)), _PLAIN_LOAD)].append(k)
    keep = []
    for (struct, name, describe), ks in members.items():
        n = len(ks)
        if not n:
            continue
        pics = (struct * n)()
        for j, k in enumerate(ks):
            pics[j], t = describe(frames[k], cfgs[k])
            keep.append(t)
        if getattr(lib, name)((C.c_void_p * n)(*[encs[k] for k in ks]), n, (C.c_int * n)(*([slot] * n)), pics, _stream_of(device)) != 0:
            _fail(lib, name)
    return keep


def _export_sources(lib, device, encs, cfgs, slot, outs, nv12):
    """ONE hmr_gpu_enc_export_sources_device: what slot `slot` of the encoders holds, as 8-bit 4:2:0"""
    n = len(encs)
    pics, results, keep = _outputs(cfgs, outs, nv12, device)
    if lib.hmr_gpu_enc_export_sources_device((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([slot] * n)), pics, _stream_of(device)) != 0:
        _fail(lib, "hmr_gpu_enc_export_sources_device")
    del keep
    return results


def _rgb_output(cfg, out, order, dtype, matrix, full_range, device):
    """the RGBFrame an RGB export writes: `out`, or one around a new packed [H, W, 3 or 4] uint8 tensor (`order` given) or a new planar [3, H, W] tensor of `dtype`"""
    import torch
    if out is not None:
        if not isinstance(out, RGBFrame):
            raise TypeError("export_rgb: out has to be an RGBFrame around the tensor to write")
        return out
    w, h = int(cfg.width), int(cfg.height)
    if order is not None:
        if order not in ORDERS:
            raise ValueError(f"export_rgb: order has to be one of {sorted(ORDERS)}, got {order!r}")
        if dtype not in (None, torch.uint8):
            raise ValueError("export_rgb: a packed picture is uint8")
        t = torch.empty((h, w, ORDERS[order][0]), dtype=torch.uint8, device=f"cuda:{device}")
        return RGBFrame(t, order=order, matrix=matrix, full_range=full_range)
    return RGBFrame(torch.empty((3, h, w), dtype=dtype or torch.uint8, device=f"cuda:{device}"), matrix=matrix, full_range=full_range)


def _export_rgb(lib, device, encs, cfgs, which, outs, order, dtype, matrix, full_range, references):
    """ONE hmr_gpu_enc_export_pictures_rgb_device for the encoders `encs`: (their tensors or None, an int64 tensor [len(encs), 3] or None).  outs: False (no pictures),
    None, or a list of RGBFrame / None; references: None or a list of RGBFrame"""
    import torch
    n = len(encs)
    picture = outs is not False
    if not picture and references is None:
        raise ValueError("export_rgb: neither the picture nor the sums asked for")
    pics, refs, results, keep = None, None, None, []
    if picture:
        pics, results = (RgbPicture * n)(), []
        for k, cfg in enumerate(cfgs):
            target = _rgb_output(cfg, outs[k] if outs is not None else None, order, dtype, matrix, full_range, device)
            pics[k], t = rgb_picture_of(target, cfg.width, cfg.height)
            keep.append(t)
            results.append(target.tensor)
    if references is not None:
        refs = (RgbPicture * n)()
        for k, cfg in enumerate(cfgs):
            if not isinstance(references[k], RGBFrame):
                raise TypeError("export_rgb: reference has to be an RGBFrame")
            # (sums alone: the reference's descriptor carries the matrix and range of the call)
            frame = references[k] if picture else RGBFrame(references[k].tensor, order=references[k].order, matrix=matrix, full_range=full_range)
            refs[k], t = rgb_picture_of(frame, cfg.width, cfg.height)
            keep.append(t)
    sums = torch.empty((n, 3), dtype=torch.int64, device=f"cuda:{device}") if refs is not None else None
    if lib.hmr_gpu_enc_export_pictures_rgb_device((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([which] * n)), pics, refs, C.c_void_p(sums.data_ptr()) if sums is not None else None,
                                                  _stream_of(device)) != 0:
        _fail(lib, "hmr_gpu_enc_export_pictures_rgb_device")
    del keep
    return results, sums


def _au_capacity(cfg):
    return max(1 << 20, int(cfg.width) * int(cfg.height) * 2)


class Encoder:
    """One sequence: encode(frame) -> (access unit bytes, slice type).  The picture is read on the device, ordered behind what torch's current stream holds when encode is
    called; work queued on that stream afterwards (writing the tensor again, the allocator reusing it) runs after the picture has been read."""

    def __init__(self, cfg, device=0):
        self.lib = lib = load_library()
        self.cfg, self.device = cfg, int(device)
        self.ctx, self.enc = C.c_void_p(), C.c_void_p()
        if lib.hmr_gpu_create(C.byref(self.ctx), self.device, None) != 0:
            self.ctx = C.c_void_p()
            _fail(lib, "hmr_gpu_create")
        if lib.hmr_gpu_enc_create(self.ctx, C.byref(cfg), C.byref(self.enc)) != 0:
            self.enc = C.c_void_p()
            err = (lib.hmr_gpu_last_error() or b"").decode(errors="replace")
            self.close()
            raise RuntimeError(f"hmr_gpu_enc_create: {err}")
        self.buf = C.create_string_buffer(_au_capacity(cfg))
        self.slot = 0
        self.slot_used = None            # the slot of the last encoded frame (export)
        self.has_pair = False            # the other slot holds the frame before it (cut_stats)
        self.last_cuts = None            # the SceneCut policy's decision of the last encode() that had one: [bool]

    def encode(self, frame, image_type=IMAGE_AUTO, scene_cut=None):
        """frame: what picture_of takes, an RGBFrame, a YUVFrame, a ScaledFrame, a ScaledRGBFrame or a ScaledYUVFrame.  image_type 0: the encoder decides (intra_period, scene changes), 3: an intra picture.  Returns (bytes, 1 for P /
        2 for I).
        scene_cut: a SceneCut policy (the encoder is its sequence 0).  Behind the load, one launch of k_cut compares the frame with the one before, the eight values are
        copied to the host - the one host wait the policy adds - and where the policy cuts, the frame is encoded as an intra picture; an image_type the caller set to
        intra stays.  The decision is readable as last_cuts.  Without a policy the calls are exactly those of before."""
        lib = self.lib
        keep = _load(lib, self.device, [self.enc], [self.cfg], self.slot, [frame])
        pair = self.slot_used is not None
        if scene_cut is not None:
            row = _cut_stats(lib, self.device, [self.enc], self.slot)[0].tolist() if pair else None
            self.last_cuts = scene_cut.decide([0], [row], [(int(self.cfg.width), int(self.cfg.height))], [image_type])
            if self.last_cuts[0]:
                image_type = IMAGE_I
        n = C.c_long()
        slice_type = lib.hmr_gpu_enc_encode_source(self.enc, self.slot, int(image_type), self.buf, len(self.buf), C.byref(n), None)
        del keep
        if slice_type < 0:
            _fail(lib, "hmr_gpu_enc_encode_source")
        self.slot_used, self.has_pair = self.slot, pair
        self.slot ^= 1
        if scene_cut is not None:
            scene_cut.observe(0, slice_type == SLICE_I)
        return self.buf.raw[:n.value], slice_type

    def cut_stats(self):
        """The eight exact scene-cut statistics (SAD_Y, SAD_U, SAD_V, HIST, INTRA, INTER, NINTRA, LUMA: include/homer_gpu.h section 12m) of the frame the last encode()
        encoded against the frame the encode() before it encoded, as they lie in the two picture slots, as an int64 CUDA tensor [8]; all -1 after the first frame, which
        has no predecessor.  cut_score(stats.tolist(), W, H) gives the scores.  One launch of k_cut, ordered on torch's current stream: what is queued there afterwards
        sees the values, nothing waits on the host."""
        if self.slot_used is None:
            raise RuntimeError("Encoder.cut_stats: nothing has been encoded yet")
        return _cut_table(self.lib, self.device, [self.enc], 1, [0] if self.has_pair else [], self.slot_used)[0]

    def export(self, picture=True, ssd=False, out=None, nv12=False):
        """The reconstructed picture of the frame the last encode() encoded (the final picture: after deblocking and SAO, what a decoder makes of the access unit) and / or
        the three exact sums of squared differences between it and the picture that frame was encoded from (for a ScaledFrame, ScaledRGBFrame or ScaledYUVFrame: the SCALED picture in the slot, what source() returns).  Returns (picture, ssd); whichever was not asked for is None.
        picture: `out` written in place (anything picture_of takes: views into larger tensors are fine, only the rows' bytes are written), else a new contiguous uint8
        tensor [H * 3 // 2, W] (I420), with nv12=True a (y, uv) pair [H, W], [H / 2, W / 2, 2].  ssd: an int64 CUDA tensor [3] (Y, U, V); psnr(ssd.tolist(), W, H) gives dB.
        One launch of the egress kernel, ordered on torch's current stream: what is queued there afterwards sees the results, nothing waits on the host."""
        if self.slot_used is None:
            raise RuntimeError("Encoder.export: nothing has been encoded yet")
        pics, sums = _export(self.lib, self.device, [self.enc], [self.cfg], self.slot_used, picture, ssd, [out] if out is not None else None, nv12)
        return (pics[0] if pics else None), (sums[0] if sums is not None else None)

    def ssim(self):
        """The three exact SSIM sums (Y, U, V) between the reconstructed picture of the frame the last encode() encoded and the picture that frame was encoded from (for a
        ScaledFrame: the SCALED picture in the slot), as an int64 CUDA tensor [3]; ssim(sums.tolist(), W, H) gives the mean SSIM of each plane.  Integer arithmetic
        (include/homer_gpu.h section 12h): the sums are the same bit for bit on every run.  One launch of k_ssim, ordered on torch's current stream: what is queued there
        afterwards sees the sums, nothing waits on the host."""
        if self.slot_used is None:
            raise RuntimeError("Encoder.ssim: nothing has been encoded yet")
        return _ssim(self.lib, self.device, [self.enc], self.slot_used)[0]

    def export_rgb(self, out=None, order=None, dtype=None, matrix="bt709", full_range=False, reference=None, source=False):
        """The reconstructed picture of the frame the last encode() encoded - with source=True: the picture that frame was encoded from, as it lies in the slot - as RGB,
        converted by the egress kernel itself in the integer arithmetic of include/homer_gpu.h section 12i (bilinear chroma, every sample reproducible from the table there;
        hmr_gpu_rgb_from_yuv_host is the same arithmetic on the host).
          out: an RGBFrame around the tensor to write - its order, matrix and range are used, views and channel slices are fine, only the rows' bytes are written;
               None: a new planar [3, H, W] tensor of `dtype` (torch.uint8 - the default -, float16 or float32: v / 255), or with `order` ("rgb", "bgra", ...: the alpha
               byte is 255) a new packed [H, W, 3 or 4] uint8 tensor, in `matrix` and `full_range`; False (with a reference): no picture, the sums alone.
          reference: an RGBFrame, normally the frame that was given to encode(): the call also returns the three exact sums of squared differences (R, G, B) between its
               8-bit values and the 8-bit values of the conversion, as an int64 CUDA tensor [3]; psnr_rgb(sums.tolist(), W, H) gives dB.
        Returns the tensor, (tensor, sums) with a reference, or the sums alone with out=False.  A float result fed back as an RGBFrame is the same 8-bit picture.  One launch
        of k_egress_rgb, ordered on torch's current stream: what is queued there afterwards sees the results, nothing waits on the host."""
        if self.slot_used is None:
            raise RuntimeError("Encoder.export_rgb: nothing has been encoded yet")
        pics, sums = _export_rgb(self.lib, self.device, [self.enc], [self.cfg], self.slot_used if source else -1, False if out is False else ([out] if out is not None else None),
                                 order, dtype, matrix, full_range, [reference] if reference is not None else None)
        if pics is None:
            return sums[0]
        return (pics[0], sums[0]) if sums is not None else pics[0]

    def source(self, out=None, nv12=False):
        """The picture the last encode() encoded, as it lies in the encoder's picture slot: for an RGBFrame the 4:2:0 samples the conversion made, for a YUVFrame the 8-bit 4:2:0 picture the rounding made, for a ScaledFrame, a ScaledRGBFrame or a ScaledYUVFrame the scaled 4:2:0 picture.  `out` and nv12 as in
        export(); one launch of the egress kernel, ordered on torch's current stream."""
        if self.slot_used is None:
            raise RuntimeError("Encoder.source: nothing has been encoded yet")
        return _export_sources(self.lib, self.device, [self.enc], [self.cfg], self.slot_used, [out] if out is not None else None, nv12)[0]

    def close(self):
        if self.enc:
            self.lib.hmr_gpu_enc_destroy(self.enc)
            self.enc = C.c_void_p()
        if self.ctx:
            self.lib.hmr_gpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BatchEncoder:
    """Several sequences (configurations with wfpp_num_threads > 1: the batch schedule), one picture of each per step(): ONE ingest launch for all their pictures and ONE
    launch for all their CTU stages.  Every sequence has a context - a stream - of its own.

    step(frames): frames[i] is sequence i's next picture (what picture_of takes, an RGBFrame, a YUVFrame, a ScaledFrame, a ScaledRGBFrame or a ScaledYUVFrame; a step that has several kinds makes one load call per kind) or None when it has none this step.  Returns a list with one entry per sequence.
    Not pipelined: entry i is the access unit of frames[i] (b"" for None).
    Pipelined (the default): access units are delivered ONE STEP LATE, as by hmr_gpu_enc_encode_batch_pipelined - entry i is the access unit of the picture sequence i was
    given in the previous step (b"" if it was given none), whose download and entropy coding ran beside this step's launch; flush() returns those of the last step.  When
    the set of sequences that have a picture changes from one step to the next, the step flushes first; what it returns is the same.

    export(): the reconstructed pictures and quality sums of the frames given to the LAST step, ONE launch for all of them.  In pipelined mode that step returned the
    access units of the step BEFORE: the pictures are one step ahead of the access units (a frame's picture exists when its launch has run, its access unit a call later)."""

    def __init__(self, cfgs, device=0, pipelined=True):
        self.lib = lib = load_library()
        self.device, self.pipelined = int(device), bool(pipelined)
        self.cfgs, self.ctxs, self.encs, self.bufs = list(cfgs), [], [], []
        try:
            for cfg in self.cfgs:
                ctx, enc = C.c_void_p(), C.c_void_p()
                if lib.hmr_gpu_create(C.byref(ctx), self.device, None) != 0:
                    _fail(lib, "hmr_gpu_create")
                self.ctxs.append(ctx)
                if lib.hmr_gpu_enc_create(ctx, C.byref(cfg), C.byref(enc)) != 0:
                    _fail(lib, "hmr_gpu_enc_create")
                self.encs.append(enc)
                self.bufs.append(C.create_string_buffer(_au_capacity(cfg)))
        except Exception:
            self.close()
            raise
        self.slot = 0
        self.outstanding = None          # pipelined: the sequences of the step whose access units have not been delivered
        self.last_live, self.slot_used = [], None      # the sequences of the last step that had a picture, and the slot they were encoded from (export)
        self.before, self.pairs = [], []               # the sequences that had a picture in the step before this one, and those of last_live whose other slot holds it
        self.last_cuts = None                          # the SceneCut policy's decision of the last step() that had one: a bool per sequence

    def _call(self, live, slots, image_types):
        n = len(live)
        got = (C.c_long * n)()
        call = self.lib.hmr_gpu_enc_encode_batch_pipelined if self.pipelined else self.lib.hmr_gpu_enc_encode_batch
        rc = call((C.c_void_p * n)(*[self.encs[i] for i in live]), n, (C.c_int * n)(*slots) if slots is not None else None,
                  (C.c_int * n)(*image_types) if image_types is not None else None, (C.c_char_p * n)(*[C.cast(self.bufs[i], C.c_char_p) for i in live]),
                  (C.c_long * n)(*[len(self.bufs[i]) for i in live]), got)
        if rc != 0:
            _fail(self.lib, "hmr_gpu_enc_encode_batch_pipelined" if self.pipelined else "hmr_gpu_enc_encode_batch")
        return {i: C.string_at(self.bufs[i], got[k]) for k, i in enumerate(live)}

    def step(self, frames, image_types=None, scene_cut=None):
        """scene_cut: a SceneCut policy.  Behind the load, ONE launch of k_cut compares every sequence's picture with the one it was given in the step before, the
        8 x n values are copied to the host - the one host wait the policy adds - and the sequences the policy cuts are encoded as intra pictures; an image type the
        caller set to intra stays.  The decision is readable as last_cuts.  Without a policy the calls are exactly those of before."""
        if len(frames) != len(self.encs):
            raise ValueError(f"BatchEncoder.step: {len(self.encs)} sequences, {len(frames)} frames")
        live = [i for i, f in enumerate(frames) if f is not None]
        out = {}
        if self.outstanding is not None and self.outstanding != live:
            out.update(self.flush_dict())
        if live:
            slots = [self.slot] * len(live)
            keep = _load(self.lib, self.device, [self.encs[i] for i in live], [self.cfgs[i] for i in live], self.slot, [frames[i] for i in live])
            pairs = [i for i in live if i in self.before]
            if scene_cut is not None:
                rows = _cut_table(self.lib, self.device, self.encs, len(self.encs), pairs, self.slot).tolist()
                self.last_cuts = scene_cut.decide(live, rows, [(int(c.width), int(c.height)) for c in self.cfgs], image_types)
                image_types = [IMAGE_I if cut else (int(image_types[i]) if image_types is not None else IMAGE_AUTO) for i, cut in enumerate(self.last_cuts)]
            for i, au in self._call(live, slots, [int(image_types[i]) for i in live] if image_types is not None else None).items():
                out[i] = out.get(i, b"") + au      # (behind a flush the call itself delivers nothing)
            del keep
            self.last_live, self.slot_used, self.pairs = live, self.slot, pairs
            self.slot ^= 1
            if self.pipelined:
                self.outstanding = live
            if scene_cut is not None:
                for i, au in out.items():      # (pipelined: the access unit of the picture before the one just given)
                    scene_cut.observe(i, _au_is_intra(au), 1 if self.pipelined and i in live else 0)
        self.before = live
        return [out.get(i, b"") for i in range(len(self.encs))]

    def export(self, picture=True, ssd=False, out=None, nv12=False):
        """As Encoder.export, for every sequence that was given a picture in the last step(), with ONE launch.  Returns (pictures, ssd): a list with one entry per
        sequence (None for a sequence without a picture in that step; `out`, when given, is such a list too and its entries are written in place) or None, and an int64
        CUDA tensor [sequences, 3] whose rows of idle sequences are -1, or None."""
        import torch
        live = self.last_live
        if not live:
            raise RuntimeError("BatchEncoder.export: the last step encoded nothing")
        if out is not None and len(out) != len(self.encs):
            raise ValueError(f"BatchEncoder.export: {len(self.encs)} sequences, {len(out)} outputs")
        pics, sums = _export(self.lib, self.device, [self.encs[i] for i in live], [self.cfgs[i] for i in live], self.slot_used, picture, ssd,
                             [out[i] for i in live] if out is not None else None, nv12)
        pictures, table = None, None
        if pics is not None:
            pictures = [None] * len(self.encs)
            for k, i in enumerate(live):
                pictures[i] = pics[k]
        if sums is not None:
            table = torch.full((len(self.encs), 3), -1, dtype=torch.int64, device=sums.device)
            table[torch.tensor(live, device=sums.device)] = sums
        return pictures, table

    def ssim(self):
        """As Encoder.ssim, for every sequence that was given a picture in the last step(), with ONE launch: an int64 CUDA tensor [sequences, 3]; the rows of idle sequences
        hold -2^63 (no sum reaches it; -1 is a possible sum)."""
        import torch
        live = self.last_live
        if not live:
            raise RuntimeError("BatchEncoder.ssim: the last step encoded nothing")
        sums = _ssim(self.lib, self.device, [self.encs[i] for i in live], self.slot_used)
        table = torch.full((len(self.encs), 3), -(1 << 63), dtype=torch.int64, device=sums.device)
        table[torch.tensor(live, device=sums.device)] = sums
        return table

    def cut_stats(self):
        """As Encoder.cut_stats, for every sequence that was given a picture in the last step() AND in the step before it, with ONE launch: an int64 CUDA tensor
        [sequences, 8]; the row of a sequence that has no such pair - idle in either step, or the first step - is all -1 (no statistic is negative)."""
        if not self.last_live:
            raise RuntimeError("BatchEncoder.cut_stats: the last step encoded nothing")
        return _cut_table(self.lib, self.device, self.encs, len(self.encs), self.pairs, self.slot_used)

    def export_rgb(self, out=None, order=None, dtype=None, matrix="bt709", full_range=False, reference=None, source=False):
        """As Encoder.export_rgb, for every sequence that was given a picture in the last step(), with ONE launch - also with access units outstanding.  `out` and
        `reference`, when given, are lists with one entry per sequence (the entries of idle sequences are ignored; out=False: the sums alone).  Returns a list of tensors
        with one entry per sequence (None for a sequence without a picture in that step), (that list, sums) with references, or the sums alone with out=False; sums: an
        int64 CUDA tensor [sequences, 3] whose rows of idle sequences are -1."""
        import torch
        live = self.last_live
        if not live:
            raise RuntimeError("BatchEncoder.export_rgb: the last step encoded nothing")
        for name, given in (("outputs", out), ("references", reference)):
            if given is not None and given is not False and len(given) != len(self.encs):
                raise ValueError(f"BatchEncoder.export_rgb: {len(self.encs)} sequences, {len(given)} {name}")
        pics, sums = _export_rgb(self.lib, self.device, [self.encs[i] for i in live], [self.cfgs[i] for i in live], self.slot_used if source else -1,
                                 False if out is False else ([out[i] for i in live] if out is not None else None), order, dtype, matrix, full_range,
                                 [reference[i] for i in live] if reference is not None else None)
        pictures, table = None, None
        if pics is not None:
            pictures = [None] * len(self.encs)
            for k, i in enumerate(live):
                pictures[i] = pics[k]
        if sums is not None:
            table = torch.full((len(self.encs), 3), -1, dtype=torch.int64, device=sums.device)
            table[torch.tensor(live, device=sums.device)] = sums
        if pictures is None:
            return table
        return (pictures, table) if table is not None else pictures

    def source(self, out=None, nv12=False):
        """As Encoder.source, for every sequence that was given a picture in the last step(), with ONE launch: a list with one entry per sequence (None for a sequence
        without a picture in that step; `out`, when given, is such a list too)."""
        live = self.last_live
        if not live:
            raise RuntimeError("BatchEncoder.source: the last step encoded nothing")
        if out is not None and len(out) != len(self.encs):
            raise ValueError(f"BatchEncoder.source: {len(self.encs)} sequences, {len(out)} outputs")
        pics = _export_sources(self.lib, self.device, [self.encs[i] for i in live], [self.cfgs[i] for i in live], self.slot_used,
                               [out[i] for i in live] if out is not None else None, nv12)
        pictures = [None] * len(self.encs)
        for k, i in enumerate(live):
            pictures[i] = pics[k]
        return pictures

    def flush_dict(self):
        if self.outstanding is None:
            return {}
        live, self.outstanding = self.outstanding, None
        return self._call(live, None, None)

    def flush(self):
        """pipelined: the access units still outstanding, one entry per sequence (b"" where there is none)"""
        out = self.flush_dict()
        return [out.get(i, b"") for i in range(len(self.encs))]

    def close(self):
        for enc in self.encs:
            self.lib.hmr_gpu_enc_destroy(enc)
        for ctx in self.ctxs:
            self.lib.hmr_gpu_destroy(ctx)
        self.encs, self.ctxs = [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
