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
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_bench import CLIP_FRAMES, CLIP_SEEDS, COPY_PEAK_TBS, KEYS, H, W, spread  # noqa: E402

FORMATS = ["rgb", "rgba", "planar8", "f16", "f32"]
READ_BYTES = {"rgb": 3, "rgba": 4, "planar8": 3, "f16": 6, "f32": 12}      # per pixel
LAUNCHES = 6                                                                # per format: a warm-up and five timed


def picture_bytes(fmt):
    """algorithmic bytes of one picture: the comment at k_ingest_rgb in csrc/picture_io.hip (k_ingest: 1.5 W H read, 3 W H written)"""
    return 4.5 * W * H if fmt == "i420" else (READ_BYTES[fmt] + 4.0) * W * H


def setup(S):
    import torch
    import encoder_cases as ec
    import libs
    from homerhevc_amd.encoder import Picture, RgbPicture
    lib = libs.load_gpu()
    P, I, L = C.c_void_p, C.c_int, C.c_long
    lib.hmr_gpu_last_error.restype = C.c_char_p
    lib.hmr_gpu_create.argtypes = [C.POINTER(P), I, P]
    lib.hmr_gpu_destroy.argtypes = [P]
    lib.hmr_gpu_enc_create.argtypes = [P, C.POINTER(ec.EncCfg), C.POINTER(P)]
    lib.hmr_gpu_enc_destroy.argtypes = [P]
    lib.hmr_gpu_enc_load_source.argtypes = [P, I] + [C.c_char_p] * 3
    lib.hmr_gpu_enc_load_sources_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(Picture), P]
    lib.hmr_gpu_enc_load_sources_rgb_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(RgbPicture), P]
    lib.hmr_gpu_enc_encode_batch_pipelined.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(I), C.POINTER(C.c_char_p), C.POINTER(L), C.POINTER(L)]
    encs, ctxs = [], []
    for _ in range(S):
        ctx, enc = P(), P()
        assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_create(ctx, C.byref(ec.default_cfg(W, H, **KEYS)), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
        encs.append(enc)
        ctxs.append(ctx)
    return torch, lib, encs, ctxs


def i420_picture(t):
    from homerhevc_amd.encoder import Picture
    p = Picture(format=0, reserved=0)
    p.plane[0], p.plane[1], p.plane[2] = t.data_ptr(), t.data_ptr() + W * H, t.data_ptr() + W * H * 5 // 4
    p.pitch[0], p.pitch[1], p.pitch[2] = W, W // 2, W // 2
    return p


def rgb_picture(t, fmt):
    """the descriptor of a tensor in one of FORMATS: [H, W, 3], [H, W, 4], [3, H, W] uint8 / float16 / float32; BT.709 limited range"""
    from homerhevc_amd.encoder import RGBFrame, rgb_picture_of
    return rgb_picture_of(RGBFrame(t, order="rgba" if fmt == "rgba" else "rgb"), W, H)[0]


def new_source(torch, fmt):
    if fmt == "i420":
        return torch.randint(0, 256, (W * H * 3 // 2,), dtype=torch.uint8, device="cuda")
    if fmt in ("rgb", "rgba"):
        return torch.randint(0, 256, (H, W, len(fmt)), dtype=torch.uint8, device="cuda")
    if fmt == "planar8":
        return torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda")
    return torch.rand((3, H, W), dtype=torch.float16 if fmt == "f16" else torch.float32, device="cuda")


def load(lib, torch, encs, slot, pics, rgb):
    from homerhevc_amd.encoder import Picture, RgbPicture
    S = len(encs)
    fn = lib.hmr_gpu_enc_load_sources_rgb_device if rgb else lib.hmr_gpu_enc_load_sources_device
    assert fn((C.c_void_p * S)(*encs), S, (C.c_int * S)(*([slot] * S)), ((RgbPicture if rgb else Picture) * S)(*pics), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, \
        lib.hmr_gpu_last_error()


def kernel_child(S):
    """the traced program: per format a warm-up launch and five timed ones over S pictures, each with a source tensor of its own (the kernel's time does not depend on the
    samples); k_ingest over I420 first"""
    torch, lib, encs, ctxs = setup(S)
    for fmt in ["i420"] + FORMATS:
        tensors = [new_source(torch, fmt) for _ in range(S)]
        pics = [i420_picture(t) if fmt == "i420" else rgb_picture(t, fmt) for t in tensors]
        torch.cuda.synchronize()
        for _ in range(LAUNCHES):
            load(lib, torch, encs, 0, pics, fmt != "i420")
            torch.cuda.synchronize()
        del tensors, pics
        torch.cuda.empty_cache()
    for e, c in zip(encs, ctxs):
        lib.hmr_gpu_enc_destroy(e)
        lib.hmr_gpu_destroy(c)


def kernel_rate(S):
    with tempfile.TemporaryDirectory(prefix="rgb_ingest_prof_") as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "rgb_ingest", "--", sys.executable, os.path.abspath(__file__), "--kernel-child",
               "--sequences", str(S)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        if r.returncode != 0:
            return {"error": f"rocprofv3 run failed ({r.returncode})", "stderr_tail": r.stderr[-1500:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written", "files": sorted(os.listdir(out))}
        rows = [r for r in csv.DictReader(open(traces[0])) if "k_ingest" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    yuv = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "k_ingest_rgb" not in r["Kernel_Name"]]
    rgb = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "k_ingest_rgb" in r["Kernel_Name"]]
    if len(yuv) != LAUNCHES or len(rgb) != LAUNCHES * len(FORMATS):
        return {"error": f"{len(yuv)} launches of k_ingest and {len(rgb)} of k_ingest_rgb in the trace, {LAUNCHES} and {LAUNCHES * len(FORMATS)} expected", "k_ingest_us": yuv, "k_ingest_rgb_us": rgb}
    res = {"source_pictures": "one tensor per sequence (no two jobs of a launch share source bytes)",
           "command": "rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_DIR -o rgb_ingest -- python tools/rgb_ingest_bench.py --kernel-child --sequences " + str(S),
           "pictures_per_launch": S}
    parts = {"i420": yuv[1:]}
    for k, fmt in enumerate(FORMATS):
        parts[fmt] = rgb[LAUNCHES * k + 1:LAUNCHES * (k + 1)]
    for fmt, part in parts.items():
        med = statistics.median(part)
        tbs = picture_bytes(fmt) * S / (med * 1e-6) / 1e12
        res[fmt] = {"kernel": "k_ingest" if fmt == "i420" else "k_ingest_rgb", "bytes_per_launch": picture_bytes(fmt) * S, "launch_us": [round(x, 1) for x in part], "median_us": round(med, 1),
                    "tb_per_s": round(tbs, 3), "share_of_float4_copy_6.29": round(tbs / COPY_PEAK_TBS, 3)}
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
    torch, lib, encs, ctxs = setup(S)
    sync = torch.cuda.synchronize

    # ---- replaces ----
    replaces = {"what": f"one frame of each of {S} sequences into a slot, wall ms between device synchronisations, alternating; torch route: clamp, scale, round, the BT.709 "
                        "limited-range matrix in float32, avg_pool2d for the chroma, round, to uint8, frame by frame into I420 tensors, then one hmr_gpu_enc_load_sources_device"}
    for fmt in ("f32", "rgba"):
        frames = [new_source(torch, fmt) for _ in range(S)]
        yuv = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(S)]
        rgb_pics, yuv_pics = [rgb_picture(t, fmt) for t in frames], [i420_picture(t) for t in yuv]

        def torch_route():
            for t, o in zip(frames, yuv):
                torch_convert(torch, t if fmt == "f32" else t[:, :, :3].permute(2, 0, 1).to(torch.float32) / 255.0, o)
            load(lib, torch, encs, 1, yuv_pics, False)

        torch_route()
        load(lib, torch, encs, 0, rgb_pics, True)
        sync()
        fused_ms, torch_ms = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            torch_route()
            sync()
            torch_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            load(lib, torch, encs, 0, rgb_pics, True)
            sync()
            fused_ms.append((time.perf_counter() - t0) * 1e3)
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
        load(lib, torch, encs, s, pics[0], True)
    sync()
    bufs = [C.create_string_buffer(4 << 20) for _ in range(S)]
    e_arr = (C.c_void_p * S)(*encs)
    ptrs = (C.c_char_p * S)(*[C.cast(b, C.c_char_p) for b in bufs])
    caps = (C.c_long * S)(*[len(b) for b in bufs])
    got = (C.c_long * S)()
    frame = [0]

    def step(streaming):
        f = frame[0] % CLIP_FRAMES
        frame[0] += 1
        slot = f
        if streaming:
            slot = CLIP_FRAMES + (frame[0] & 1)
            load(lib, torch, encs, slot, pics[f], True)
        assert lib.hmr_gpu_enc_encode_batch_pipelined(e_arr, S, (C.c_int * S)(*([slot] * S)), None, ptrs, caps, got) == 0, lib.hmr_gpu_last_error()

    def window(streaming):
        sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step(streaming)
        sync()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    for _ in range(CLIP_FRAMES // 2):      # steady state: the pool's buffers, the staging buffers, both paths' first calls; one round of the clip
        step(False)
        step(True)
    pre, stream = [], []
    for _ in range(3):
        pre.append(window(False))
        stream.append(window(True))
    assert lib.hmr_gpu_enc_encode_batch_pipelined(e_arr, S, None, None, ptrs, caps, got) == 0, lib.hmr_gpu_last_error()
    kr = result["kernel_rate"]
    kernel_ms = kr["rgba"]["median_us"] / 1e3 if "rgba" in kr else None
    sp, ss = spread(pre), spread(stream)
    result["streaming_step"] = {"steps_per_window": a.steps, "pictures": f"every window encodes the clips' {CLIP_FRAMES} pictures (as RGBA, BT.709 limited range) in turn, starting at the first",
                                "preloaded_ms_per_step": sp, "streaming_ms_per_step": ss, "ingest_kernel_ms": kernel_ms}
    if kernel_ms is not None:
        bound = sp["median"] + kernel_ms + sp["spread"]
        result["streaming_step"].update({"bound_ms": round(bound, 3), "condition": "median streaming <= median preloaded + ingest kernel + spread of preloaded",
                                         "holds": bool(ss["median"] <= bound)})
    for name, path in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        if path and os.path.exists(path):
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
            if lines:
                result.setdefault("bench", {})[name] = [{k: b.get(k) for k in ("value", "unit", "ms_per_step", "steps", "warmup", "build")} for b in map(json.loads, lines)]
    for e, c in zip(encs, ctxs):
        lib.hmr_gpu_enc_destroy(e)
        lib.hmr_gpu_destroy(c)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
