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
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import picture_bench as pb  # noqa: E402
from picture_bench import COPY_PEAK_TBS, spread  # noqa: E402
from scale_ingest_bench import ladder_bench  # noqa: E402

WORKLOADS = {"ladder_1080p_f16_x3": {"source": (1920, 1080), "form": "f16", "pixel_bytes": 6, "rungs": [(1280, 720), (960, 544), (640, 360)]},
             "2160p_rgba_to_1080p": {"source": (3840, 2160), "form": "rgba", "pixel_bytes": 4, "rungs": [(1920, 1080)]}}
LAUNCHES = 6                  # per workload in the traced child: a warm-up and five timed

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
        import rgb_cases as rc
        import rgb_scale_cases as rs
        import scale_cases as sc
        from homerhevc_amd.encoder import Picture
        self.torch, self.n, self.lib, self.made, self.work = torch, n_sources, pb.library(), [], {}
        self.structs = {"hmr_gpu_enc_load_sources_rgb_device": rc.RgbPicture, "hmr_gpu_enc_load_sources_scaled_device": sc.ScaledPicture,
                        "hmr_gpu_enc_load_sources_scaled_rgb_device": rs.ScaledRgbPicture, "hmr_gpu_enc_export_sources_device": Picture}
        for name in names:
            wl = WORKLOADS[name]
            w, h = wl["source"]
            if wl["form"] == "f16":      # (the kernel's time does not depend on the samples; a tensor of its own per source)
                srcs = [torch.rand((3, h, w), dtype=torch.float16, device="cuda") for _ in range(n_sources)]
                rgb = [rc.descriptor(rc.RGB_PLANAR_F16, 0, (0, 0, 0), [t.data_ptr() + 2 * c * w * h for c in range(3)], [2 * w] * 3, "bt709", 0) for t in srcs]
            else:
                srcs = [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(n_sources)]
                rgb = [rc.descriptor(rc.RGB_PACKED8, 4, (0, 1, 2), [t.data_ptr()], [4 * w], "bt709", 0) for t in srcs]
            rung_encs = [self.encoder(*r) for _ in range(n_sources) for r in wl["rungs"]]
            entry = {"srcs": srcs, "rung_encs": rung_encs, "rgb": rgb,
                     "scaled_rgb": [rs.ScaledRgbPicture(pic=rgb[k // len(wl["rungs"])], width=w, height=h) for k in range(len(rung_encs))]}
            if composition:
                entry["top_encs"] = [self.encoder(w, h) for _ in range(n_sources)]
                entry["mid"] = [torch.empty((h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(n_sources)]
                entry["mid_pics"] = [pb.i420_picture(t, w, h) for t in entry["mid"]]
                planes = lambda t: [t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4]
                entry["scaled"] = [sc.descriptor(0, planes(entry["mid"][k // len(wl["rungs"])]), [w, w // 2, w // 2], w, h) for k in range(len(rung_encs))]
            self.work[name] = entry
        torch.cuda.synchronize()

    def encoder(self, w, h):
        self.made += pb.encoders(self.lib, 1, w, h)
        return self.made[-1][1]

    def call(self, name, encs, pics):
        n = len(encs)
        assert getattr(self.lib, name)((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([0] * n)), (self.structs[name] * n)(*pics), pb.stream_of()) == 0, self.lib.hmr_gpu_last_error()

    def new_call(self, name):
        e = self.work[name]
        self.call("hmr_gpu_enc_load_sources_scaled_rgb_device", e["rung_encs"], e["scaled_rgb"])

    def composition(self, name):
        e = self.work[name]
        self.call("hmr_gpu_enc_load_sources_rgb_device", e["top_encs"], e["rgb"])
        self.call("hmr_gpu_enc_export_sources_device", e["top_encs"], e["mid_pics"])
        self.call("hmr_gpu_enc_load_sources_scaled_device", e["rung_encs"], e["scaled"])

    def close(self):
        pb.close(self.lib, self.made)


def kernel_child(n_sources):
    """the traced program: per workload a warm-up launch and five timed ones"""
    for name in WORKLOADS:      # (one workload's tensors at a time: 64 2160p RGBA sources are 2.1 GB)
        s = Setup(n_sources, [name], composition=False)
        for _ in range(LAUNCHES):
            s.new_call(name)
            s.torch.cuda.synchronize()
        s.close()
        del s


def kernel_rate(n_sources):
    rows, command = pb.traced_child(__file__, ["--sources", str(n_sources)], "rgb_scale")
    groups = pb.launch_groups(rows, "k_rgb_ladder", len(WORKLOADS), LAUNCHES)
    if isinstance(groups, dict):
        return groups
    res = {"command": command, "yardsticks": {"float4_copy_tb_per_s": COPY_PEAK_TBS}}
    for (name, wl), part in zip(WORKLOADS.items(), groups):
        nbytes = n_sources * sum(rgb_scale_bytes(wl["source"], r, wl["pixel_bytes"]) for r in wl["rungs"])
        record = pb.rate(part, nbytes, jobs_per_launch=n_sources * len(wl["rungs"]), bytes_per_launch=nbytes)
        record["tb_per_s"] = round(pb.tb_per_s(part, nbytes) * 1e3, 1)      # (this file has always recorded GB/s)
        res[name] = {"gb_per_s" if k == "tb_per_s" else k: v for k, v in record.items()}
    return res


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
    ladder_bench(result, a)
    pb.write_result(result, a.out)


if __name__ == "__main__":
    main()
