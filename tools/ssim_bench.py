#!/usr/bin/env python3
"""GPU box tool: what the device SSIM (include/homer_gpu.h section 12h, k_ssim in csrc/picture_io.hip) costs, on bench.py's flagship workload (256 sequences of
1920x1080, bench.py's configuration and clips).  Writes profiles/ssim_bench.json.

    python tools/ssim_bench.py [--sequences 256] [--steps 20] [--bench-this FILE ... --bench-parent FILE ...]

  kernel_rate      k_ssim's time for one launch over all sequences' pictures from `rocprofv3 --kernel-trace --stats` in a run of its own (this program starts it as a
                   child, the traced program behind `--`, no counters); bytes from ssim_bytes() below.  The yardstick beside it, from the same trace: k_egress with
                   sums only on the same encoders - the parent commit's kernel, which reads the same 6 W H bytes per picture; the bar is k_ssim <= 1.5 x that launch
  streaming_step   ms per step of hmr_gpu_enc_encode_batch_pipelined plain and with an SSIM call over every sequence after every step, alternating, three windows
                   each; the condition: median with SSIM <= median plain + k_ssim's time + spread of plain
  bench            bench.py's lines of this build and of the parent commit's, when the files are given (all from the same GPU visit, alternating)
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
import ingest_bench as ib  # noqa: E402  (the workload and the encoders' set-up)
from egress_bench import encode_one_step  # noqa: E402

W, H, CLIP_FRAMES, COPY_PEAK_TBS = ib.W, ib.H, ib.CLIP_FRAMES, ib.COPY_PEAK_TBS
BAR = 1.5
LAUNCHES = 6      # per kernel in the traced child: a warm-up and five timed


def ssim_bytes(width, height):
    """algorithmic bytes of one picture through k_ssim (the comment at k_ssim in csrc/picture_io.hip): the int16 planes of the final picture and of the slot are read once"""
    return 6.0 * float(width) * height


def declare(lib, Picture):
    P, I = C.c_void_p, C.c_int
    lib.hmr_gpu_enc_ssim_device.argtypes = [C.POINTER(P), I, C.POINTER(I), P, P]
    lib.hmr_gpu_enc_export_pictures_device.argtypes = [C.POINTER(P), I, C.POINTER(Picture), C.POINTER(I), P, P]


def ssim_device(lib, encs, slot, sums, torch):
    S = len(encs)
    assert lib.hmr_gpu_enc_ssim_device((C.c_void_p * S)(*encs), S, (C.c_int * S)(*([slot] * S)), C.c_void_p(sums.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, lib.hmr_gpu_last_error()


def ssd_device(lib, encs, slot, sums, torch):
    S = len(encs)
    assert lib.hmr_gpu_enc_export_pictures_device((C.c_void_p * S)(*encs), S, None, (C.c_int * S)(*([slot] * S)), C.c_void_p(sums.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, lib.hmr_gpu_last_error()


def kernel_child(S):
    """the traced program: every sequence encodes one picture, then LAUNCHES launches of k_ssim and as many of k_egress (sums only) over the S pictures, alternating"""
    torch, lib, Picture, encs, ctxs, clips, dev, i420 = ib.setup(S, with_clips=True)      # (the clips: a picture the encoder is known to take; every sequence has planes of its own)
    declare(lib, Picture)
    ib.load_device(lib, Picture, encs, 0, [i420(dev[i % len(dev)][0]) for i in range(S)], torch)
    bufs, e_arr, ptrs, caps, got = encode_one_step(lib, encs, 0)
    lib.hmr_gpu_enc_encode_batch.argtypes = lib.hmr_gpu_enc_encode_batch_pipelined.argtypes
    assert lib.hmr_gpu_enc_encode_batch(e_arr, S, (C.c_int * S)(*([0] * S)), None, ptrs, caps, got) == 0, lib.hmr_gpu_last_error()
    sums = torch.zeros((S, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(LAUNCHES):
        for call in (ssim_device, ssd_device):
            call(lib, encs, 0, sums, torch)
            torch.cuda.synchronize()
    for e, c in zip(encs, ctxs):
        lib.hmr_gpu_enc_destroy(e)
        lib.hmr_gpu_destroy(c)


def kernel_rate(S):
    with tempfile.TemporaryDirectory(prefix="ssim_prof_") as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "ssim", "--", sys.executable, os.path.abspath(__file__), "--kernel-child",
               "--sequences", str(S)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": f"rocprofv3 run failed ({r.returncode})", "stderr_tail": r.stderr[-1500:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written", "files": sorted(os.listdir(out))}
        rows = list(csv.DictReader(open(traces[0])))
    res = {"command": "rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_DIR -o ssim -- python tools/ssim_bench.py --kernel-child --sequences " + str(S),
           "pictures_per_launch": S, "bytes_formula": "3 W H read (final picture) + 3 W H read (slot), per picture: the same for both kernels",
           "bytes_per_launch": ssim_bytes(W, H) * S}
    for name in ("k_ssim", "k_egress"):
        mine = sorted((r for r in rows if name in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine]
        if len(us) != LAUNCHES:
            return {"error": f"{len(us)} launches of {name} in the trace, {LAUNCHES} expected", "us": us}
        part = us[1:]
        med = statistics.median(part)
        tbs = res["bytes_per_launch"] / (med * 1e-6) / 1e12
        res[name if name == "k_ssim" else "k_egress_sums_only"] = {"launch_us": [round(x, 1) for x in part], "median_us": round(med, 1), "tb_per_s": round(tbs, 3),
                                                                  "share_of_float4_copy_6.29": round(tbs / COPY_PEAK_TBS, 3),
                                                                  "vgpr_sgpr_lds": [mine[-1].get(k) for k in ("VGPR_Count", "SGPR_Count", "LDS_Block_Size")]}
    ratio = res["k_ssim"]["median_us"] / res["k_egress_sums_only"]["median_us"]
    res.update({"ratio_k_ssim_to_k_egress_sums_only": round(ratio, 3), "bar": BAR, "within_bar": bool(ratio <= BAR)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--no-streaming-step", action="store_true")
    ap.add_argument("--bench-this", nargs="*", default=[], help="files with bench.py's JSON line on this build")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="files with bench.py's JSON line on the parent commit's build, from runs alternating with those")
    ap.add_argument("--notes", help="a text file whose lines become the result's notes (what the ISA or a trace shows about the rates)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_bench.json"))
    a = ap.parse_args()
    S = a.sequences
    if a.kernel_child:
        kernel_child(S)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/ssim_bench.py", "source_digest": source_digest(), "sequences": S, "width": W, "height": H, "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": ssim_bytes(W, H)}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(S)
    if a.no_streaming_step:
        result["streaming_step"] = {"skipped": True}
    else:
        result["streaming_step"] = streaming_step(S, a.steps, result["kernel_rate"])
    for name, paths in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        runs = []
        for path in paths:
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")] if os.path.exists(path) else []
            if lines:
                b = json.loads(lines[-1])
                runs.append({k: b.get(k) for k in ("value", "unit", "ms_per_step", "steps", "warmup", "build")})
        if runs:
            values = [r["value"] for r in runs]
            result.setdefault("bench", {})[name] = {"runs": runs, "median": statistics.median(values), "spread": round(max(values) - min(values), 4)}
    if "bench" not in result:
        result["bench"] = "not measured"
    if a.notes and os.path.exists(a.notes):
        result["notes"] = [ln.strip() for ln in open(a.notes) if ln.strip()]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


def streaming_step(S, steps, kr):
    torch, lib, Picture, encs, ctxs, clips, dev, i420 = ib.setup(S, with_clips=True)
    declare(lib, Picture)
    sync = torch.cuda.synchronize
    nclip = len(clips)
    pics = [[i420(dev[i % nclip][f]) for i in range(S)] for f in range(CLIP_FRAMES)]
    for s in (0, 1):
        ib.load_device(lib, Picture, encs, s, pics[0], torch)
    bufs, e_arr, ptrs, caps, got = encode_one_step(lib, encs, 0)
    sums = torch.zeros((S, 3), dtype=torch.int64, device="cuda")
    frame = [0]

    def step(with_ssim):
        f = frame[0] % CLIP_FRAMES
        frame[0] += 1
        slot = frame[0] & 1
        ib.load_device(lib, Picture, encs, slot, pics[f], torch)
        assert lib.hmr_gpu_enc_encode_batch_pipelined(e_arr, S, (C.c_int * S)(*([slot] * S)), None, ptrs, caps, got) == 0, lib.hmr_gpu_last_error()
        if with_ssim:
            ssim_device(lib, encs, slot, sums, torch)

    for _ in range(CLIP_FRAMES // 2):      # steady state: the pool's buffers, the staging buffers, both paths' first calls; one round of the clip
        step(False)
        step(True)
    sync()

    def window(with_ssim):
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(with_ssim)
        sync()
        return (time.perf_counter() - t0) * 1e3 / steps

    plain, measuring = [], []
    for _ in range(3):
        plain.append(window(False))
        measuring.append(window(True))
    assert lib.hmr_gpu_enc_encode_batch_pipelined(e_arr, S, None, None, ptrs, caps, got) == 0, lib.hmr_gpu_last_error()
    last = sums.cpu()
    kernel_ms = kr["k_ssim"]["median_us"] / 1e3 if "k_ssim" in kr else None
    sp, sm = ib.spread(plain), ib.spread(measuring)
    res = {"steps_per_window": steps, "pictures": f"every step ingests a fresh device picture per sequence (the clips' {CLIP_FRAMES} pictures in turn) and encodes it",
           "plain_ms_per_step": sp, "with_ssim_ms_per_step": sm, "k_ssim_ms": kernel_ms,
           "mean_luma_ssim_of_the_last_step": round(float(last[:, 0].double().mean()) / float(((W // 4 - 1) * (H // 4 - 1)) << 30), 4)}
    if kernel_ms is not None:
        bound = sp["median"] + kernel_ms + sp["spread"]
        res.update({"bound_ms": round(bound, 3), "condition": "median with SSIM <= median plain + k_ssim + spread of plain", "holds": bool(sm["median"] <= bound)})
    else:
        res["holds"] = "not measured (no kernel time)"
    for e, c in zip(encs, ctxs):
        lib.hmr_gpu_enc_destroy(e)
        lib.hmr_gpu_destroy(c)
    return res


if __name__ == "__main__":
    main()
