#!/usr/bin/env python3
"""GPU box tool: what the downscaling ingest (include/homer_gpu.h section 12g, k_downscale in csrc/picture_io.hip) costs and what it replaces, on a resolution ladder:
64 different 1920x1080 sources x the rungs 1920x1080, 1280x720, 960x544, 640x360 = 256 jobs in ONE launch; and 64 different 3840x2160 sources -> 1920x1080 alone.
Writes profiles/scale_ingest_bench.json.

    python tools/scale_ingest_bench.py [--sources 64] [--counters] [--bench-this FILE ... --bench-parent FILE ...]

  kernel_rate   k_downscale's time for one launch over all jobs, from `rocprofv3 --kernel-trace --stats` in a run of its own (this program starts it as a child, the
                traced program behind `--`, no counters): five launches and the median; bytes from the formula in the comment at k_downscale (csrc/picture_io.hip): 1.5 Ws Hs read + 3 Wd Hd written per job
  replaces      wall ms to fill the 256 slots of the ladder through ONE hmr_gpu_enc_load_sources_scaled_device, and through what the library offered before:
                torch.nn.functional.interpolate(mode="area") per rung on float planes, rounded and cast to uint8, then ONE hmr_gpu_enc_load_sources_device;
                alternating, five repetitions each
  counters      (--counters) one `rocprofv3 --pmc` pass of its own over the same child: wave cycles, waiting, issuing, LDS activity and bank conflicts per launch
  bench         bench.py's line of this build and of the parent commit's, when their files are given (alternating runs of the same GPU visit)
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
SRC = (1920, 1080)
RUNGS = [(1920, 1080), (1280, 720), (960, 544), (640, 360)]
BIG, BIG_RUNG = (3840, 2160), (1920, 1080)
COPY_PEAK_TBS = 6.29          # float4 copy, measured (the figure the other profile files use)
K_INGEST_TBS = 4.9            # profiles/ingest_bench.json: k_ingest on 256 x 1080p


def scale_bytes(src, dst):
    """the formula in the comment at k_downscale (csrc/picture_io.hip)"""
    return 1.5 * src[0] * src[1] + 3.0 * dst[0] * dst[1]


def setup(n_sources, big):
    import torch
    import encoder_cases as ec
    import libs
    from homerhevc_amd.encoder import Picture, ScaledPicture
    lib = libs.load_gpu()
    P, I = C.c_void_p, C.c_int
    lib.hmr_gpu_last_error.restype = C.c_char_p
    lib.hmr_gpu_create.argtypes = [C.POINTER(P), I, P]
    lib.hmr_gpu_destroy.argtypes = [P]
    lib.hmr_gpu_enc_create.argtypes = [P, C.POINTER(ec.EncCfg), C.POINTER(P)]
    lib.hmr_gpu_enc_destroy.argtypes = [P]
    lib.hmr_gpu_enc_load_sources_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(Picture), P]
    lib.hmr_gpu_enc_load_sources_scaled_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(ScaledPicture), P]
    encs, ctxs, sizes = [], [], []
    for _ in range(n_sources):      # job order: source by source, its rungs next to each other
        for w, h in RUNGS:
            ctx, enc = P(), P()
            assert lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, lib.hmr_gpu_last_error()
            assert lib.hmr_gpu_enc_create(ctx, C.byref(ec.default_cfg(w, h)), C.byref(enc)) == 0, lib.hmr_gpu_last_error()
            encs.append(enc)
            ctxs.append(ctx)
            sizes.append((w, h))
    # (the kernel's time does not depend on the samples; a picture of its own per source: 64 x 3.1 MB, and 64 x 12.4 MB for 2160p)
    w, h = SRC
    srcs = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(n_sources)]
    bigs = [torch.randint(0, 256, (BIG[1] * 3 // 2, BIG[0]), dtype=torch.uint8, device="cuda") for _ in range(n_sources)] if big else []
    torch.cuda.synchronize()

    def i420(t, w, h):
        p = Picture(format=0, reserved=0)
        p.plane[0], p.plane[1], p.plane[2] = t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4
        p.pitch[0], p.pitch[1], p.pitch[2] = w, w // 2, w // 2
        return p

    def scaled(t, w, h):
        return ScaledPicture(pic=i420(t, w, h), width=w, height=h)

    return torch, lib, Picture, ScaledPicture, encs, ctxs, sizes, srcs, bigs, i420, scaled


def stream_of(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def load_scaled(lib, ScaledPicture, encs, pics, torch):
    n = len(encs)
    assert lib.hmr_gpu_enc_load_sources_scaled_device((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([0] * n)), (ScaledPicture * n)(*pics), stream_of(torch)) == 0, lib.hmr_gpu_last_error()


def kernel_child(n_sources):
    """the traced program: a warm-up launch and five timed ones of the ladder, then the same of 2160p -> 1080p"""
    torch, lib, Picture, ScaledPicture, encs, ctxs, sizes, srcs, bigs, i420, scaled = setup(n_sources, big=True)
    ladder = [scaled(srcs[k // len(RUNGS)], *SRC) for k in range(len(encs))]
    top = [e for e, s in zip(encs, sizes) if s == BIG_RUNG]
    for group, pics in ((encs, ladder), (top, [scaled(t, *BIG) for t in bigs])):
        for _ in range(6):
            load_scaled(lib, ScaledPicture, group, pics, torch)
            torch.cuda.synchronize()
    for e, c in zip(encs, ctxs):
        lib.hmr_gpu_enc_destroy(e)
        lib.hmr_gpu_destroy(c)


def kernel_rate(n_sources):
    with tempfile.TemporaryDirectory(prefix="scale_prof_") as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "scale", "--", sys.executable, os.path.abspath(__file__), "--kernel-child",
               "--sources", str(n_sources)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": f"rocprofv3 run failed ({r.returncode})", "stderr_tail": r.stderr[-1500:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written", "files": sorted(os.listdir(out))}
        rows = [r for r in csv.DictReader(open(traces[0])) if "k_downscale" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    if len(us) != 12:
        return {"error": f"{len(us)} launches of k_downscale in the trace, 12 expected", "us": us}
    res = {"source_pictures": "one tensor per source; the four rungs of a source read the same bytes (that is the ladder)",
           "command": "rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_DIR -o scale -- python tools/scale_ingest_bench.py --kernel-child --sources " + str(n_sources),
           "yardsticks": {"float4_copy_tb_per_s": COPY_PEAK_TBS, "k_ingest_tb_per_s": K_INGEST_TBS}}
    ladder_bytes = n_sources * sum(scale_bytes(SRC, r) for r in RUNGS)
    for name, part, nbytes, jobs in (("ladder_1080p_x4", us[1:6], ladder_bytes, n_sources * len(RUNGS)), ("2160p_to_1080p", us[7:12], n_sources * scale_bytes(BIG, BIG_RUNG), n_sources)):
        med = statistics.median(part)
        tbs = nbytes / (med * 1e-6) / 1e12
        res[name] = {"jobs_per_launch": jobs, "bytes_per_launch": nbytes, "launch_us": [round(x, 1) for x in part], "median_us": round(med, 1), "tb_per_s": round(tbs, 3),
                     "share_of_float4_copy_6.29": round(tbs / COPY_PEAK_TBS, 3), "share_of_k_ingest_4.9": round(tbs / K_INGEST_TBS, 3)}
    return res


PMC = ["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_LDS_BANK_CONFLICT", "GRBM_GUI_ACTIVE"]


def counters(n_sources):
    """ONE counter pass of its own (no tracing beside it) over the kernel child: per workload the mean of each counter over k_downscale's dispatches"""
    with tempfile.TemporaryDirectory(prefix="scale_pmc_") as out:
        cmd = ["rocprofv3", "--pmc"] + PMC + ["--output-format", "csv", "-d", out, "-o", "pmc", "--", sys.executable, os.path.abspath(__file__), "--kernel-child", "--sources", str(n_sources)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": f"rocprofv3 run failed ({r.returncode})", "stderr_tail": r.stderr[-1500:]}
        files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
        if not files:
            return {"error": "no counter file written", "files": sorted(os.listdir(out))}
        rows = [r for r in csv.DictReader(open(files[0])) if "k_downscale" in r["Kernel_Name"]]
    res = {"command": "rocprofv3 --pmc " + " ".join(PMC) + " --output-format csv -d DIR -o pmc -- python tools/scale_ingest_bench.py --kernel-child --sources " + str(n_sources)}
    ids = sorted({int(r["Dispatch_Id"]) for r in rows})
    if len(ids) != 12:
        return dict(res, error=f"{len(ids)} dispatches of k_downscale, 12 expected")
    for name, part in (("ladder_1080p_x4", ids[1:6]), ("2160p_to_1080p", ids[7:12])):
        agg = {}
        for r in rows:
            if int(r["Dispatch_Id"]) in part:
                agg.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
        res[name] = {k: round(sum(v) / len(v)) for k, v in sorted(agg.items())}
    return res


def spread(xs):
    return {"runs": [round(x, 3) for x in xs], "median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "spread": round(max(xs) - min(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--counters", action="store_true", help="beside the rest: one rocprofv3 --pmc pass of its own over the kernel child (what binds the kernel)")
    ap.add_argument("--bench-this", nargs="+", default=[], help="files with bench.py's JSON line on this build (runs alternating with the parent's)")
    ap.add_argument("--bench-parent", nargs="+", default=[], help="files with bench.py's JSON line on the parent commit's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_ingest_bench.json"))
    a = ap.parse_args()
    N = a.sources
    if a.kernel_child:
        kernel_child(N)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/scale_ingest_bench.py", "source_digest": source_digest(), "sources": N, "source_size": list(SRC), "rungs": [list(r) for r in RUNGS],
              "algorithmic_bytes_per_job": {f"{r[0]}x{r[1]}": scale_bytes(SRC, r) for r in RUNGS}}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(N)
    if a.counters:
        result["counters"] = counters(N)
    torch, lib, Picture, ScaledPicture, encs, ctxs, sizes, srcs, bigs, i420, scaled = setup(N, big=False)
    import torch.nn.functional as F
    sync = torch.cuda.synchronize
    n = len(encs)
    ladder = [scaled(srcs[k // len(RUNGS)], *SRC) for k in range(n)]
    w, h = SRC
    batch = torch.stack(srcs)      # [N, h * 3 / 2, w]: the composition scales all sources of a rung at once (its best case)

    def composition():
        """what the parent commit offers: interpolate(mode="area") per rung on float planes, rounded, cast to uint8, then ONE hmr_gpu_enc_load_sources_device"""
        y = batch[:, :h].unsqueeze(1).float()
        c = batch[:, h:].reshape(N, 2, h // 2, w // 2).float()
        made = {}
        for rw, rh in RUNGS:
            if (rw, rh) == SRC:
                made[(rw, rh)] = batch
                continue
            ys = F.interpolate(y, size=(rh, rw), mode="area").add_(0.5).to(torch.uint8)
            cs = F.interpolate(c, size=(rh // 2, rw // 2), mode="area").add_(0.5).to(torch.uint8)
            made[(rw, rh)] = torch.cat([ys.reshape(N, rh, rw), cs.reshape(N, rh // 2, rw)], dim=1)
        pics = [i420(made[sizes[k]][k // len(RUNGS)], *sizes[k]) for k in range(n)]
        assert lib.hmr_gpu_enc_load_sources_device((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([0] * n)), (Picture * n)(*pics), stream_of(torch)) == 0, lib.hmr_gpu_last_error()
        return made

    for _ in range(2):      # steady state: the slots, both paths' first calls, torch's allocator
        load_scaled(lib, ScaledPicture, encs, ladder, torch)
        composition()
        sync()
    scaled_ms, composed_ms = [], []
    for _ in range(5):
        sync()
        t0 = time.perf_counter()
        load_scaled(lib, ScaledPicture, encs, ladder, torch)
        t1 = time.perf_counter()
        sync()
        scaled_ms.append((time.perf_counter() - t0) * 1e3)
        result.setdefault("load_sources_scaled_device_call_returns_after_ms", []).append(round((t1 - t0) * 1e3, 3))
        t0 = time.perf_counter()
        keep = composition()
        sync()
        composed_ms.append((time.perf_counter() - t0) * 1e3)
        del keep
    ss, sc_ = spread(scaled_ms), spread(composed_ms)
    result["replaces"] = {"what": f"{n} slots of the ladder filled from {N} sources, wall ms between device synchronisations, alternating",
                          "hmr_gpu_enc_load_sources_scaled_device_ms": ss, "interpolate_area_then_load_sources_device_ms": sc_,
                          "ratio_of_medians": round(sc_["median"] / ss["median"], 2),
                          "condition": "median scaled < median composition - (spread of scaled + spread of composition)",
                          "holds": bool(ss["median"] < sc_["median"] - (ss["spread"] + sc_["spread"]))}
    for name, paths in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        runs = []
        for path in paths:
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")] if os.path.exists(path) else []
            if lines:
                b = json.loads(lines[-1])
                runs.append({k: b.get(k) for k in ("value", "unit", "ms_per_step", "steps", "warmup", "build")})
        if runs:
            result.setdefault("bench", {})[name] = {"runs": runs, "frames_per_s": spread([r["value"] for r in runs])}
    if set(result.get("bench", {})) == {"this_build", "parent"}:
        t, p = result["bench"]["this_build"]["frames_per_s"], result["bench"]["parent"]["frames_per_s"]
        result["bench"]["condition"] = "median of this build >= median of the parent - the parent's run-to-run spread"
        result["bench"]["holds"] = bool(t["median"] >= p["median"] - p["spread"])
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
