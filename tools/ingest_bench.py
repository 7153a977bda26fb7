#!/usr/bin/env python3
"""GPU box tool: what the device ingest (include/homer_gpu.h section 12d, k_ingest in csrc/picture_io.hip) costs and what it replaces, on bench.py's flagship workload
(256 sequences of 1920x1080, bench.py's configuration and clips).  Writes profiles/ingest_bench.json.

    python tools/ingest_bench.py [--sequences 256] [--steps 20] [--bench-this FILE --bench-parent FILE]

  kernel_rate      k_ingest's time for one launch over all sequences' pictures, I420 and NV12, from `rocprofv3 --kernel-trace --stats` in a run of its own (this
                   program starts it as a child, the traced program behind `--`, no counters); bytes from the formula 1.5 W H read + 3 W H written per picture
  replaces         wall time to bring one picture of every sequence into a slot through hmr_gpu_enc_load_source (host planes) and through ONE
                   hmr_gpu_enc_load_sources_device, alternating, five repetitions each.  The host entry runs the same kernel (one picture per launch): what is left
                   between the two figures is its copies from host memory, a launch and a synchronisation per picture
  streaming_step   ms per step of hmr_gpu_enc_encode_batch_pipelined with the slots preloaded (what bench.py times) and with a fresh device picture ingested for every
                   sequence before every step, alternating, three repetitions each; the condition streaming <= preloaded + kernel time + spread of preloaded
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
W, H, KEYS = 1920, 1080, {"wpp": 17}          # bench.py WORKLOADS["cfg2-1080p-encode"]
CLIP_SEEDS = [1234, 1, 2, 3, 4, 5, 6, 7]      # bench.py CLIP_SEEDS
CLIP_FRAMES = 10                              # (a timed window of 20 steps is two rounds of a clip: every window encodes the same pictures)
COPY_PEAK_TBS = 6.29                          # float4 copy, measured (the microarchitecture notes' HBM figure; 8.0 TB/s is the specification)
PICTURE_BYTES = 1.5 * W * H + 3.0 * W * H


def setup(S, with_clips):
    import numpy as np
    import torch
    import encoder_cases as ec
    import libs
    from homerhevc_amd.encoder import Picture
    lib = libs.load_gpu()
    P, I, L = C.c_void_p, C.c_int, C.c_long
    lib.hmr_gpu_last_error.restype = C.c_char_p
    lib.hmr_gpu_create.argtypes = [C.POINTER(P), I, P]
    lib.hmr_gpu_destroy.argtypes = [P]
    lib.hmr_gpu_enc_create.argtypes = [P, C.POINTER(ec.EncCfg), C.POINTER(P)]
    lib.hmr_gpu_enc_destroy.argtypes = [P]
    lib.hmr_gpu_enc_load_source.argtypes = [P, I] + [C.c_char_p] * 3
    lib.hmr_gpu_enc_load_sources_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(Picture), P]
    lib.hmr_gpu_enc_encode_batch_pipelined.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(I), C.POINTER(C.c_char_p), C.POINTER(L), C.POINTER(L)]
    encs, ctxs = [], []
    for _ in range(S):
        ctx, enc = P(), P()
        assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
        assert lib.hmr_gpu_enc_create(ctx, C.byref(ec.default_cfg(W, H, **KEYS)), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
        encs.append(enc)
        ctxs.append(ctx)
    if with_clips:
        clips = [ec.clip_frames(W, H, CLIP_FRAMES, seed=sd) for sd in CLIP_SEEDS]
        dev = [[torch.from_numpy(np.frombuffer(b"".join(planes), np.uint8).copy()).cuda() for planes in clip] for clip in clips]
    else:      # (the kernel's time does not depend on the samples; a picture of its own per sequence, so that no launch finds its source in a cache: S x 3.1 MB)
        clips = None
        dev = [[torch.randint(0, 256, (W * H * 3 // 2,), dtype=torch.uint8, device="cuda")] for _ in range(S)]
    torch.cuda.synchronize()

    def i420(t):
        p = Picture(format=0, reserved=0)
        p.plane[0], p.plane[1], p.plane[2] = t.data_ptr(), t.data_ptr() + W * H, t.data_ptr() + W * H * 5 // 4
        p.pitch[0], p.pitch[1], p.pitch[2] = W, W // 2, W // 2
        return p

    return torch, lib, Picture, encs, ctxs, clips, dev, i420


def load_device(lib, Picture, encs, slot, pics, torch):
    S = len(encs)
    assert lib.hmr_gpu_enc_load_sources_device((C.c_void_p * S)(*encs), S, (C.c_int * S)(*([slot] * S)), (Picture * S)(*pics),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, lib.hmr_gpu_last_error()


def kernel_child(S):
    """the traced program: a warm-up launch and five timed ones over S I420 pictures, then the same over S NV12 pictures"""
    torch, lib, Picture, encs, ctxs, clips, dev, i420 = setup(S, with_clips=False)
    nv = []
    for clip in dev:
        t = clip[0]
        uv = torch.stack([t[W * H:W * H * 5 // 4], t[W * H * 5 // 4:]], dim=1).reshape(-1)
        nv.append(torch.cat([t[:W * H], uv]).contiguous())
    torch.cuda.synchronize()

    def nv12(t):
        p = Picture(format=1, reserved=0)
        p.plane[0], p.plane[1] = t.data_ptr(), t.data_ptr() + W * H
        p.pitch[0], p.pitch[1] = W, W
        return p

    for pics in ([i420(dev[i % len(dev)][0]) for i in range(S)], [nv12(nv[i % len(nv)]) for i in range(S)]):
        for _ in range(6):
            load_device(lib, Picture, encs, 0, pics, torch)
            torch.cuda.synchronize()
    for e, c in zip(encs, ctxs):
        lib.hmr_gpu_enc_destroy(e)
        lib.hmr_gpu_destroy(c)


def kernel_rate(S):
    with tempfile.TemporaryDirectory(prefix="ingest_prof_") as out:
        return kernel_rate_in(S, out)


def kernel_rate_in(S, out):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "ingest", "--", sys.executable, os.path.abspath(__file__), "--kernel-child",
           "--sequences", str(S)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return {"error": f"rocprofv3 run failed ({r.returncode})", "stderr_tail": r.stderr[-1500:]}
    traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        return {"error": "no kernel trace written", "files": sorted(os.listdir(out))}
    rows = [r for r in csv.DictReader(open(traces[0])) if "k_ingest" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    if len(us) != 12:
        return {"error": f"{len(us)} launches of k_ingest in the trace, 12 expected", "us": us}
    res = {"source_pictures": "one tensor per sequence (no two jobs of a launch share source bytes)", "command": " ".join(cmd[:6] + ["TRACE_DIR"] + cmd[7:9] + ["--"] + ["python", "tools/ingest_bench.py", "--kernel-child", "--sequences", str(S)]), "pictures_per_launch": S,
           "bytes_per_launch": PICTURE_BYTES * S, "yardstick": "k_subpel_*: 1.98 TB/s (VERDICT 12)"}
    for name, part in (("i420", us[1:6]), ("nv12", us[7:12])):
        med = statistics.median(part)
        tbs = PICTURE_BYTES * S / (med * 1e-6) / 1e12
        res[name] = {"launch_us": [round(x, 1) for x in part], "median_us": round(med, 1), "tb_per_s": round(tbs, 3), "share_of_float4_copy_6.29": round(tbs / COPY_PEAK_TBS, 3)}
    return res


def spread(xs):
    return {"runs": [round(x, 3) for x in xs], "median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "spread": round(max(xs) - min(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--bench-this", help="file with bench.py's JSON line on this build")
    ap.add_argument("--bench-parent", help="file with bench.py's JSON line on the parent commit's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    a = ap.parse_args()
    S = a.sequences
    if a.kernel_child:
        kernel_child(S)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/ingest_bench.py", "source_digest": source_digest(), "sequences": S, "width": W, "height": H, "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": PICTURE_BYTES}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(S)
    torch, lib, Picture, encs, ctxs, clips, dev, i420 = setup(S, with_clips=True)
    sync = torch.cuda.synchronize
    nclip = len(clips)
    # slots 0 .. CLIP_FRAMES - 1: the clip through the host entry (bench.py's preload); slots CLIP_FRAMES, CLIP_FRAMES + 1: the device path's two
    t0 = time.perf_counter()
    for i, e in enumerate(encs):
        for f, planes in enumerate(clips[i % nclip]):
            assert lib.hmr_gpu_enc_load_source(e, f, *planes) == 0, lib.hmr_gpu_last_error()
    sync()
    result["preload_all_slots_s"] = round(time.perf_counter() - t0, 2)
    pics = [[i420(dev[i % nclip][f]) for i in range(S)] for f in range(CLIP_FRAMES)]
    for s in (CLIP_FRAMES, CLIP_FRAMES + 1):
        load_device(lib, Picture, encs, s, pics[0], torch)
    sync()

    host_ms, device_ms = [], []
    for rep in range(5):
        f = rep % CLIP_FRAMES
        sync()
        t0 = time.perf_counter()
        for i, e in enumerate(encs):
            assert lib.hmr_gpu_enc_load_source(e, f, *clips[i % nclip][f]) == 0, lib.hmr_gpu_last_error()
        sync()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        load_device(lib, Picture, encs, CLIP_FRAMES, pics[f], torch)
        t1 = time.perf_counter()
        sync()
        device_ms.append((time.perf_counter() - t0) * 1e3)
        result.setdefault("load_sources_device_call_returns_after_ms", []).append(round((t1 - t0) * 1e3, 3))
    result["replaces"] = {"what": f"one picture of each of {S} sequences into a slot, wall ms between device synchronisations, alternating",
                          "hmr_gpu_enc_load_source_ms": spread(host_ms), "hmr_gpu_enc_load_sources_device_ms": spread(device_ms),
                          "ratio_of_medians": round(statistics.median(host_ms) / statistics.median(device_ms), 1)}

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
            load_device(lib, Picture, encs, slot, pics[f], torch)
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
    kernel_ms = kr["i420"]["median_us"] / 1e3 if "i420" in kr else None
    sp, ss = spread(pre), spread(stream)
    result["streaming_step"] = {"steps_per_window": a.steps, "pictures": f"every window encodes the clips' {CLIP_FRAMES} pictures in turn, starting at the first", "preloaded_ms_per_step": sp, "streaming_ms_per_step": ss, "ingest_kernel_ms": kernel_ms}
    if kernel_ms is not None:
        bound = sp["median"] + kernel_ms + sp["spread"]
        result["streaming_step"].update({"bound_ms": round(bound, 3), "condition": "median streaming <= median preloaded + ingest kernel + spread of preloaded",
                                         "holds": bool(ss["median"] <= bound)})
    for name, path in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        if path and os.path.exists(path):
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
            if lines:
                b = json.loads(lines[-1])
                result.setdefault("bench", {})[name] = {k: b.get(k) for k in ("value", "unit", "ms_per_step", "steps", "warmup", "build")}
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
