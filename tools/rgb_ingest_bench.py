#!/usr/bin/env python3
"""GPU box tool: what the colour-converting ingest (include/homer_gpu.h section 12f, k_ingest_rgb in csrc/picture_io.hip) costs and what it replaces, on bench.py's
flagship workload (256 sequences of 1920x1080, bench.py's configuration and clips).  Follows tools/ingest_bench.py.  Writes profiles/rgb_ingest_bench.json.

    python tools/rgb_ingest_bench.py [--sequences 256] [--steps 20] [--bench-this FILE --bench-parent FILE]

  kernel_rate      k_ingest_rgb's time for one launch over all sequences' pictures, per format (3- and 4-byte packed, planar 8-bit, binary16, binary32), and k_ingest's
                   over I420 pictures in the same run, from `rocprofv3 --kernel-trace --stats` in a run of its own (this program starts it as a child, the traced
                   program behind `--`, no counters).  Every job has a source tensor of its own.  Bytes from the formula in the comment at k_ingest_rgb (csrc/picture_io.hip):
                   3, 4, 3, 6 or 12 W H read, 4 W H written per picture (k_ingest: 1.5 W H read, 3 W H written)
  replaces         wall time of ONE hmr_gpu_enc_load_sources_rgb_device over one float32 [3, H, W] frame (and one RGBA frame) per sequence, against what a user writes
                   today: the same conversion in torch ops, frame by frame, into I420 tensors, then ONE hmr_gpu_enc_load_sources_device; alternating, five repetitions
  streaming_step   ms per step of hmr_gpu_enc_encode_batch_pipelined with the slots preloaded and with a fresh RGBA picture ingested for every sequence before every
                   step, alternating, three repetitions each; the condition streaming <= preloaded + kernel time + spread of preloaded.  Both kinds of window encode
                   the same samples: the preloaded slots hold the conversion of the RGBA pictures
  bench            bench.py's line of this build and of the parent commit's, when the two files are given (both from the same GPU visit)
Timed windows are walls between two device synchronisations, in one process with the steady state warmed first."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import ingest_bench as ib  # noqa: E402  (the workload, the encoders' set-up, the timed loops)
import picture_bench as pb  # noqa: E402
from ingest_bench import CLIP_FRAMES, CLIP_SEEDS, KEYS, H, W  # noqa: E402
from picture_bench import spread  # noqa: E402


FORMATS = ["rgb", "rgba", "planar8", "f16", "f32"]
READ_BYTES = {"rgb": 3, "rgba": 4, "planar8": 3, "f16": 6, "f32": 12}      # per pixel
LAUNCHES = 6                                                                # per format: a warm-up and five timed


def picture_bytes(fmt):
    """algorithmic bytes of one picture: the comment at k_ingest_rgb in csrc/picture_io.hip (k_ingest: 1.5 W H read, 3 W H written)"""
    return 4.5 * W * H if fmt == "i420" else (READ_BYTES[fmt] + 4.0) * W * H


def rgb_picture(t, fmt):
    """the descriptor of a tensor in one of FORMATS: [H, W, 3], [H, W, 4], [3, H, W] uint8 / float16 / float32; BT.709 limited range"""
    from homerhevc_amd.encoder import RGBFrame, rgb_picture_of
    from rgb_cases import RgbPicture
    return RgbPicture.from_buffer_copy(rgb_picture_of(RGBFrame(t, order="rgba" if fmt == "rgba" else "rgb"), W, H)[0])


def new_source(torch, fmt):
    if fmt == "i420":
        return torch.randint(0, 256, (W * H * 3 // 2,), dtype=torch.uint8, device="cuda")
    if fmt in ("rgb", "rgba"):
        return torch.randint(0, 256, (H, W, len(fmt)), dtype=torch.uint8, device="cuda")
    if fmt == "planar8":
        return torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda")
    return torch.rand((3, H, W), dtype=torch.float16 if fmt == "f16" else torch.float32, device="cuda")


def load(lib, encs, slot, pics, rgb):
    from rgb_cases import RgbPicture
    if rgb:
        ib.load_many(lib, "hmr_gpu_enc_load_sources_rgb_device", RgbPicture, encs, slot, pics)
    else:
        ib.load_device(lib, encs, slot, pics)


def kernel_child(S):
    """the traced program: per format a warm-up launch and five timed ones over S pictures, each with a source tensor of its own (the kernel's time does not depend on the
    samples); k_ingest over I420 first"""
    import torch
    lib = pb.library()
    made = pb.encoders(lib, S, W, H, **KEYS)
    encs = [e for _, e in made]
    for fmt in ["i420"] + FORMATS:
        tensors = [new_source(torch, fmt) for _ in range(S)]
        pics = [ib.i420(t) if fmt == "i420" else rgb_picture(t, fmt) for t in tensors]
        torch.cuda.synchronize()
        for _ in range(LAUNCHES):
            load(lib, encs, 0, pics, fmt != "i420")
            torch.cuda.synchronize()
        del tensors, pics
        torch.cuda.empty_cache()
    pb.close(lib, made)


def kernel_rate(S):
    rows, command = pb.traced_child(__file__, ["--sequences", str(S)], "rgb_ingest", timeout=1500)
    yuv, rgb = pb.launch_groups(rows, "k_ingest", 1, LAUNCHES), pb.launch_groups(rows, "k_ingest_rgb", len(FORMATS), LAUNCHES)
    for groups in (yuv, rgb):
        if isinstance(groups, dict):
            return groups
    res = {"source_pictures": "one tensor per sequence (no two jobs of a launch share source bytes)", "command": command, "pictures_per_launch": S}
    for fmt, part in zip(["i420"] + FORMATS, yuv + rgb):
        res[fmt] = pb.rate(part, picture_bytes(fmt) * S, kernel="k_ingest" if fmt == "i420" else "k_ingest_rgb", bytes_per_launch=picture_bytes(fmt) * S)
    for fmt in FORMATS:
        res[fmt]["rate_over_k_ingest_i420"] = round(res[fmt]["tb_per_s"] / res["i420"]["tb_per_s"], 3)
    return res


def torch_convert(torch, rgb, out):
    """what a user writes today: float R, G, B planes in 0 .. 1 ([3, H, W]) to an I420 tensor [H * 3 // 2, W] with 2 x 2 chroma averaging, BT.709 limited range"""
    q = (rgb.clamp(0.0, 1.0) * 255.0).round()
    avg = torch.nn.functional.avg_pool2d(q[None], 2)[0]
    kr, kb = 0.2126, 0.0722
    kg = 1.0 - kr - kb
    y = 16.0 + (219.0 / 255.0) * (kr * q[0] + kg * q[1] + kb * q[2])
    ay = kr * avg[0] + kg * avg[1] + kb * avg[2]
    cb = 128.0 + (224.0 / 255.0) * (avg[2] - ay) / (2.0 * (1.0 - kb))
    cr = 128.0 + (224.0 / 255.0) * (avg[0] - ay) / (2.0 * (1.0 - kr))
    out[:H] = y.round().to(torch.uint8)
    out[H:H + H // 4] = cb.round().clamp(0, 255).to(torch.uint8).view(H // 4, W)
    out[H + H // 4:] = cr.round().clamp(0, 255).to(torch.uint8).view(H // 4, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--bench-this", help="file with bench.py's JSON line on this build")
    ap.add_argument("--bench-parent", help="file with bench.py's JSON line on the parent commit's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_ingest_bench.json"))
    a = ap.parse_args()
    S = a.sequences
    if a.kernel_child:
        kernel_child(S)
        return
    import numpy as np
    import encoder_cases as ec
    import rgb_cases as rc
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/rgb_ingest_bench.py", "source_digest": source_digest(), "sequences": S, "width": W, "height": H, "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": {fmt: picture_bytes(fmt) for fmt in ["i420"] + FORMATS}}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(S)
    import torch
    lib = pb.library()
    made = pb.encoders(lib, S, W, H, **KEYS)
    encs = [e for _, e in made]
    sync = torch.cuda.synchronize

    # ---- replaces ----
    replaces = {"what": f"one frame of each of {S} sequences into a slot, wall ms between device synchronisations, alternating; torch route: clamp, scale, round, the BT.709 "
                        "limited-range matrix in float32, avg_pool2d for the chroma, round, to uint8, frame by frame into I420 tensors, then one hmr_gpu_enc_load_sources_device"}
    for fmt in ("f32", "rgba"):
        frames = [new_source(torch, fmt) for _ in range(S)]
        yuv = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(S)]
        rgb_pics, yuv_pics = [rgb_picture(t, fmt) for t in frames], [ib.i420(t) for t in yuv]

        def torch_route():
            for t, o in zip(frames, yuv):
                torch_convert(torch, t if fmt == "f32" else t[:, :, :3].permute(2, 0, 1).to(torch.float32) / 255.0, o)
            load(lib, encs, 1, yuv_pics, False)

        torch_route()
        load(lib, encs, 0, rgb_pics, True)
        sync()
        torch_ms, fused_ms = ib.alternating(torch, torch_route, lambda: load(lib, encs, 0, rgb_pics, True))
        replaces[fmt] = {"torch_ops_then_load_sources_device_ms": spread(torch_ms), "load_sources_rgb_device_ms": spread(fused_ms),
                         "ratio_of_medians": round(statistics.median(torch_ms) / statistics.median(fused_ms), 1)}
        del frames, yuv, rgb_pics, yuv_pics
        torch.cuda.empty_cache()
    result["replaces"] = replaces

    # ---- streaming step ----
    nclip = len(CLIP_SEEDS)
    rng = np.random.default_rng(0)
    rgba, converted = [], []
    for sd in CLIP_SEEDS:
        frames_dev, frames_yuv = [], []
        for planes in ec.clip_frames(W, H, CLIP_FRAMES, seed=sd):
            r, g, b = rc.yuv_to_rgb(planes, W, H)
            frames_dev.append(torch.from_numpy(np.stack([r, g, b, rng.integers(0, 256, (H, W), dtype=np.uint8)], axis=2)).cuda())
            frames_yuv.append(tuple(p.tobytes() for p in rc.restate(r, g, b, "bt709", 0)))
        rgba.append(frames_dev)
        converted.append(frames_yuv)
    # slots 0 .. CLIP_FRAMES - 1: the converted clip through the host entry (bench.py's preload); slots CLIP_FRAMES, CLIP_FRAMES + 1: the RGB path's two
    for i, e in enumerate(encs):
        for f, planes in enumerate(converted[i % nclip]):
            assert lib.hmr_gpu_enc_load_source(e, f, *planes) == 0, lib.hmr_gpu_last_error()
    pics = [[rgb_picture(rgba[i % nclip][f], "rgba") for i in range(S)] for f in range(CLIP_FRAMES)]
    for s in (CLIP_FRAMES, CLIP_FRAMES + 1):
        load(lib, encs, s, pics[0], True)
    sync()
    kr = result["kernel_rate"]
    result["streaming_step"] = ib.streaming_step(torch, lib, encs, a.steps, lambda slot, f: load(lib, encs, slot, pics[f], True), kr["rgba"]["median_us"] / 1e3 if "rgba" in kr else None,
                                                 f"every window encodes the clips' {CLIP_FRAMES} pictures (as RGBA, BT.709 limited range) in turn, starting at the first")
    for name, path in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        if pb.bench_lines(path):
            result.setdefault("bench", {})[name] = pb.bench_lines(path)
    pb.close(lib, made)
    pb.write_result(result, a.out)


if __name__ == "__main__":
    main()
