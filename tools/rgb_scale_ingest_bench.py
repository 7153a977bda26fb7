#!/usr/bin/env python3
"""GPU box tool: what the downscaling RGB ingest (include/homer_gpu.h section 12j, k_rgb_ladder in csrc/picture_io.hip) costs and what it replaces.  Two workloads:
(a) 64 different 1920x1080 planar float16 sources x the rungs 1280x720, 960x544, 640x360 = 192 jobs in ONE launch; (b) 64 different 3840x2160 packed RGBA sources ->
1920x1080.  Writes profiles/rgb_scale_ingest_bench.json.

    python tools/rgb_scale_ingest_bench.py [--sources 64] [--bench-this FILE ... --bench-parent FILE ...]

  kernel_rate   k_rgb_ladder's time for one launch over all jobs, from `rocprofv3 --kernel-trace --stats` in a run of its own (this program starts it as a child, the
                traced program behind `--`, no counters): a warm-up and five launches per workload, the median; bytes from the formula in the comment at k_rgb_ladder (csrc/picture_io.hip): 2 x (source pixel
                bytes x Ws Hs) read - luma and chroma tiles each read the source - + 3 Wd Hd written per job
  replaces      wall ms to fill the slots through ONE hmr_gpu_enc_load_sources_scaled_rgb_device, and through the composition the library offered before:
                hmr_gpu_enc_load_sources_rgb_device into source-sized encoders, hmr_gpu_enc_export_sources_device of their slots, then
                hmr_gpu_enc_load_sources_scaled_device of those pictures - three launches, the int16 slot and the 8-bit copy written and read in between;
                alternating, five repetitions each, per workload.  No ratio is fixed in advance.  Expected on (b): the new call is not slower (it moves
                2 x 4 Ws Hs + 3 Wd Hd bytes against 4 Ws Hs + 2 x 3 Ws Hs + 2 x 1.5 Ws Hs + 3 Wd Hd, in one launch instead of three); on (a) the composition converts once
                and scales three times from 8 bits, so it may win: whichever is true is recorded
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
WORKLOADS = {"ladder_1080p_f16_x3": {"source": (1920, 1080), "form": "f16", "pixel_bytes": 6, "rungs": [(1280, 720), (960, 544), (640, 360)]},
             "2160p_rgba_to_1080p": {"source": (3840, 2160), "form": "rgba", "pixel_bytes": 4, "rungs": [(1920, 1080)]}}
COPY_PEAK_TBS = 6.29          # float4 copy, measured (the figure the other profile files use)


def rgb_scale_bytes(src, dst, pixel_bytes):
    """the formula in the comment at k_rgb_ladder (csrc/picture_io.hip)"""
    return 2.0 * pixel_bytes * src[0] * src[1] + 3.0 * dst[0] * dst[1]


def composition_bytes(src, rungs, pixel_bytes):
    """the three launches: the source read and its int16 slot written (3 Ws Hs), the slot read and the 8-bit picture written (1.5 Ws Hs) once per source, then the formula at k_downscale
    per rung (the 8-bit picture read, the rung's slot written)"""
    wh = src[0] * src[1]
    return (pixel_bytes + 3.0) * wh + (3.0 + 1.5) * wh + sum(1.5 * wh + 3.0 * r[0] * r[1] for r in rungs)


class Setup:
    """the library, and per workload: the sources, the rungs' encoders (job order: source by source, its rungs next to each other), the source-sized encoders of the
    composition with the 8-bit pictures their slots are exported into"""

    def __init__(self, n_sources, names, composition):
        import torch
        import encoder_cases as ec
        import libs
        from homerhevc_amd.encoder import Picture, RgbPicture, ScaledPicture, ScaledRgbPicture
        self.torch, self.n = torch, n_sources
        self.Picture, self.RgbPicture, self.ScaledPicture, self.ScaledRgbPicture = Picture, RgbPicture, ScaledPicture, ScaledRgbPicture
        self.lib = lib = libs.load_gpu()
        P, I = C.c_void_p, C.c_int
        lib.hmr_gpu_last_error.restype = C.c_char_p
        lib.hmr_gpu_create.argtypes = [C.POINTER(P), I, P]
        lib.hmr_gpu_destroy.argtypes = [P]
        lib.hmr_gpu_enc_create.argtypes = [P, C.POINTER(ec.EncCfg), C.POINTER(P)]
        lib.hmr_gpu_enc_destroy.argtypes = [P]
        lib.hmr_gpu_enc_load_sources_rgb_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(RgbPicture), P]
        lib.hmr_gpu_enc_load_sources_scaled_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(ScaledPicture), P]
        lib.hmr_gpu_enc_load_sources_scaled_rgb_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(ScaledRgbPicture), P]
        lib.hmr_gpu_enc_export_sources_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(Picture), P]
        self.made = []
        self.work = {}
        for name in names:
            wl = WORKLOADS[name]
            w, h = wl["source"]
            if wl["form"] == "f16":      # (the kernel's time does not depend on the samples; a tensor of its own per source)
                srcs = [torch.rand((3, h, w), dtype=torch.float16, device="cuda") for _ in range(n_sources)]
            else:
                srcs = [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(n_sources)]
            rung_encs = [self.encoder(ec, *r) for _ in range(n_sources) for r in wl["rungs"]]
            rgb = [self.rgb_picture(t, wl["form"], w, h) for t in srcs]
            entry = {"srcs": srcs, "rung_encs": rung_encs, "rgb": rgb,
                     "scaled_rgb": [ScaledRgbPicture(pic=rgb[k // len(wl["rungs"])], width=w, height=h) for k in range(len(rung_encs))]}
            if composition:
                entry["top_encs"] = [self.encoder(ec, w, h) for _ in range(n_sources)]
                entry["mid"] = [torch.empty((h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(n_sources)]
                entry["mid_pics"] = [self.i420(t, w, h) for t in entry["mid"]]
                entry["scaled"] = [ScaledPicture(pic=entry["mid_pics"][k // len(wl["rungs"])], width=w, height=h) for k in range(len(rung_encs))]
            self.work[name] = entry
        torch.cuda.synchronize()

    def encoder(self, ec, w, h):
        ctx, enc = C.c_void_p(), C.c_void_p()
        assert self.lib.hmr_gpu_create(C.byref(ctx), 0, None) == 0, self.lib.hmr_gpu_last_error()
        assert self.lib.hmr_gpu_enc_create(ctx, C.byref(ec.default_cfg(w, h)), C.byref(enc)) == 0, self.lib.hmr_gpu_last_error()
        self.made.append((ctx, enc))
        return enc

    def rgb_picture(self, t, form, w, h):
        p = self.RgbPicture(matrix=1, full_range=0, reserved=0)
        if form == "f16":
            p.format, p.pixel_bytes = 2, 0
            for c in range(3):
                p.plane[c], p.pitch[c] = t.data_ptr() + 2 * c * w * h, 2 * w
        else:
            p.format, p.pixel_bytes = 0, 4
            p.offset[0], p.offset[1], p.offset[2] = 0, 1, 2
            p.plane[0], p.pitch[0] = t.data_ptr(), 4 * w
        return p

    def i420(self, t, w, h):
        p = self.Picture(format=0, reserved=0)
        p.plane[0], p.plane[1], p.plane[2] = t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4
        p.pitch[0], p.pitch[1], p.pitch[2] = w, w // 2, w // 2
        return p

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def call(self, name, encs, pics, struct):
        n = len(encs)
        assert getattr(self.lib, name)((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([0] * n)), (struct * n)(*pics), self.stream()) == 0, self.lib.hmr_gpu_last_error()

    def new_call(self, name):
        e = self.work[name]
        self.call("hmr_gpu_enc_load_sources_scaled_rgb_device", e["rung_encs"], e["scaled_rgb"], self.ScaledRgbPicture)

    def composition(self, name):
        e = self.work[name]
        self.call("hmr_gpu_enc_load_sources_rgb_device", e["top_encs"], e["rgb"], self.RgbPicture)
        self.call("hmr_gpu_enc_export_sources_device", e["top_encs"], e["mid_pics"], self.Picture)
        self.call("hmr_gpu_enc_load_sources_scaled_device", e["rung_encs"], e["scaled"], self.ScaledPicture)

    def close(self):
        for ctx, enc in self.made:
            self.lib.hmr_gpu_enc_destroy(enc)
            self.lib.hmr_gpu_destroy(ctx)


def kernel_child(n_sources):
    """the traced program: per workload a warm-up launch and five timed ones"""
    for name in WORKLOADS:      # (one workload's tensors at a time: 64 2160p RGBA sources are 2.1 GB)
        s = Setup(n_sources, [name], composition=False)
        for _ in range(6):
            s.new_call(name)
            s.torch.cuda.synchronize()
        s.close()
        del s


def kernel_rate(n_sources):
    with tempfile.TemporaryDirectory(prefix="rgb_scale_prof_") as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "rgb_scale", "--", sys.executable, os.path.abspath(__file__), "--kernel-child",
               "--sources", str(n_sources)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": f"rocprofv3 run failed ({r.returncode})", "stderr_tail": r.stderr[-1500:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written", "files": sorted(os.listdir(out))}
        rows = [r for r in csv.DictReader(open(traces[0])) if "k_rgb_ladder" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    if len(us) != 12:
        return {"error": f"{len(us)} launches of k_rgb_ladder in the trace, 12 expected", "us": us}
    res = {"command": "rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_DIR -o rgb_scale -- python tools/rgb_scale_ingest_bench.py --kernel-child --sources " + str(n_sources),
           "yardsticks": {"float4_copy_tb_per_s": COPY_PEAK_TBS}}
    for k, (name, wl) in enumerate(WORKLOADS.items()):
        part = us[6 * k + 1:6 * k + 6]
        nbytes = n_sources * sum(rgb_scale_bytes(wl["source"], r, wl["pixel_bytes"]) for r in wl["rungs"])
        med = statistics.median(part)
        tbs = nbytes / (med * 1e-6) / 1e12
        res[name] = {"jobs_per_launch": n_sources * len(wl["rungs"]), "bytes_per_launch": nbytes, "launch_us": [round(x, 1) for x in part], "median_us": round(med, 1),
                     "gb_per_s": round(tbs * 1e3, 1), "share_of_float4_copy_6.29": round(tbs / COPY_PEAK_TBS, 3)}
    return res


def spread(xs):
    return {"runs": [round(x, 3) for x in xs], "median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "spread": round(max(xs) - min(xs), 3)}


def replaces(n_sources, name):
    wl = WORKLOADS[name]
    s = Setup(n_sources, [name], composition=True)
    sync = s.torch.cuda.synchronize
    for _ in range(2):      # steady state: the slots, both paths' first calls
        s.new_call(name)
        s.composition(name)
        sync()
    new_ms, composed_ms, returns = [], [], []
    for _ in range(5):
        sync()
        t0 = time.perf_counter()
        s.new_call(name)
        t1 = time.perf_counter()
        sync()
        new_ms.append((time.perf_counter() - t0) * 1e3)
        returns.append(round((t1 - t0) * 1e3, 3))
        t0 = time.perf_counter()
        s.composition(name)
        sync()
        composed_ms.append((time.perf_counter() - t0) * 1e3)
    s.close()
    a, b = spread(new_ms), spread(composed_ms)
    return {"what": f"{n_sources * len(wl['rungs'])} slots filled from {n_sources} {wl['source'][0]}x{wl['source'][1]} {wl['form']} sources, wall ms between device synchronisations, alternating",
            "model_bytes": {"new_call": n_sources * sum(rgb_scale_bytes(wl["source"], r, wl["pixel_bytes"]) for r in wl["rungs"]),
                            "composition": n_sources * composition_bytes(wl["source"], wl["rungs"], wl["pixel_bytes"])},
            "hmr_gpu_enc_load_sources_scaled_rgb_device_ms": a, "call_returns_after_ms": returns,
            "load_rgb_then_export_sources_then_load_scaled_ms": b,
            "composition_over_new_call": round(b["median"] / a["median"], 2),
            "new_call_is_not_slower": bool(a["median"] <= b["median"] + (a["spread"] + b["spread"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--bench-this", nargs="+", default=[], help="files with bench.py's JSON line on this build (runs alternating with the parent's)")
    ap.add_argument("--bench-parent", nargs="+", default=[], help="files with bench.py's JSON line on the parent commit's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_scale_ingest_bench.json"))
    a = ap.parse_args()
    N = a.sources
    if a.kernel_child:
        kernel_child(N)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/rgb_scale_ingest_bench.py", "source_digest": source_digest(), "sources": N,
              "workloads": {k: {"source": list(v["source"]), "form": v["form"], "rungs": [list(r) for r in v["rungs"]],
                                "algorithmic_bytes_per_job": {f"{r[0]}x{r[1]}": rgb_scale_bytes(v["source"], r, v["pixel_bytes"]) for r in v["rungs"]}} for k, v in WORKLOADS.items()}}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(N)
    result["replaces"] = {name: replaces(N, name) for name in WORKLOADS}
    result["replaces"]["expected"] = "2160p_rgba_to_1080p: the new call is not slower than the composition; ladder_1080p_f16_x3: either may win (the composition converts once)"
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
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
