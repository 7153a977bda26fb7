"""homerhevc_amd - MI355X (gfx950) backend for HomerHEVC's per-block encode hot path.

The product is `libhomer_gpu.so` (hand-written HIP kernels behind the C ABI of include/homer_gpu.h);
this package is the thin Python host side: the build recipe (build.py), the encoder on torch tensors (encoder.py: pictures that are already on
the GPU in, access units, reconstructed pictures - 4:2:0 or RGB -, PSNR and SSIM sums and scene-cut statistics out) and the engine-per-GPU ring bench.py --gpus N runs (engines.py).  (The ctypes mirror of the batched kernel ABI that the kernel tests use is test infrastructure: tests/gpu_abi.py.)
There is no CPU fallback: importing works anywhere, calling a kernel without the native library or
without a GPU raises.
"""
from .build import LIB_PATH, build_native  # noqa: F401
from .encoder import BatchEncoder, Encoder, EncoderConfig, RGBFrame, ScaledFrame, ScaledRGBFrame, ScaledYUVFrame, SceneCut, YUVFrame, cut_score, psnr, psnr_rgb, ssim  # noqa: F401  (imports neither torch nor the native library)

__all__ = ["LIB_PATH", "build_native", "BatchEncoder", "Encoder", "EncoderConfig", "RGBFrame", "ScaledFrame", "ScaledRGBFrame", "ScaledYUVFrame", "SceneCut", "YUVFrame", "cut_score", "psnr", "psnr_rgb", "ssim"]
