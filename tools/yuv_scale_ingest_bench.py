#!/usr/bin/env python3
"""GPU box tool: what the downscaling deep / 4:2:2 / 4:4:4 ingest (include/homer_gpu.h section 12l, k_yuv_ladder in csrc/picture_io.hip) costs and what it replaces.  Three
workloads: (a) 64 different 3840x2160 P010 sources x the rungs 1920x1080, 1280x720, 640x360 = 192 jobs in ONE launch; (b) 64 different 1920x1080 10-bit 4:2:2 planar
sources x 1280x720, 960x544, 640x360; (c) 64 different 1920x1080 UYVY sources -> 960x544.  Writes profiles/yuv_scale_ingest_bench.json.

    python tools/yuv_scale_ingest_bench.py [--sources 64] [--bench-this FILE ... --bench-parent FILE ...]

  kernel_rate   k_yuv_ladder's time for one launch over all jobs, from `rocprofv3 --kernel-trace --stats` in a run of its own (this program starts it as a child, the
                traced program behind `--`, no counters): a warm-up and five launches per workload, the median; bytes from the formula in the comment at k_yuv_ladder
                (csrc/picture_io.hip): sb (Ws Hs + 2 Wc Hc) read - a packed source's single plane is read by both tile classes and counts twice - + 3 Wd Hd written per
                job.  The yardstick is k_downscale over the SAME jobs from 8-bit I420 pictures of the same sizes in the same run (1.5 Ws Hs + 3 Wd Hd per job): it moves
                fewer source bytes and converts nothing; the record says what share of its rate, and what multiple of its time, each workload reaches.  No ratio is
                fixed in advance.
  replaces      wall ms to fill the slots through ONE hmr_gpu_enc_load_sources_scaled_yuv, and through the composition the library offered before:
                hmr_gpu_enc_load_sources_yuv_device into source-sized encoders, hmr_gpu_enc_export_sources_device of their slots, then
                hmr_gpu_enc_load_sources_scaled_device of those pictures - three launches, the int16 slot and the 8-bit copy written and read in between; alternating,
                five repetitions each, per workload.  On the ladders the composition converts once and scales three times from 8 bits, so it may win on kernel time
                and lose on wall time: whichever is true is recorded
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

WORKLOADS = {"ladder_2160p_p010_x3": {"source": (3840, 2160), "form": "semi_uv_420_10msb", "rungs": [(1920, 1080), (1280, 720), (640, 360)]},
             "ladder_1080p_422p10_x3": {"source": (1920, 1080), "form": "planar_422_10", "rungs": [(1280, 720), (960, 544), (640, 360)]},
             "1080p_uyvy_to_960x544": {"source": (1920, 1080), "form": "uyvy_8", "rungs": [(960, 544)]}}
LAUNCHES = 6                  # per workload and kernel in the traced child: a warm-up and five timed


def plane_rows(form, w, h):
    """[(rows, row bytes)] of the form's planes"""
    import yuv_cases as yc
    fmt, chroma, bits, _, _ = yc.FORMS[form]
    sb = yc.sample_bytes(bits)
    wc, hc = yc.chroma_size(chroma, w, h)
    if fmt == yc.YUV_PLANAR:
        return [(h, w * sb), (hc, wc * sb), (hc, wc * sb)]
    return [(h, w * sb), (hc, 2 * wc * sb)] if fmt == yc.YUV_SEMIPLANAR else [(h, 2 * w * sb)]


def yuv_scale_bytes(form, src, dst):
    """the formula in the comment at k_yuv_ladder (csrc/picture_io.hip)"""
    read = sum(rows * row_bytes for rows, row_bytes in plane_rows(form, *src))
    return (2.0 if len(plane_rows(form, *src)) == 1 else 1.0) * read + 3.0 * dst[0] * dst[1]


def downscale_bytes(src, dst):
    """the formula in the comment at k_downscale"""
    return 1.5 * src[0] * src[1] + 3.0 * dst[0] * dst[1]


def composition_bytes(form, src, rungs):
    """the three launches: the source read and its int16 slot written (3 Ws Hs), the slot read and the 8-bit picture written (1.5 Ws Hs) once per source, then the formula
    at k_downscale per rung"""
    wh = src[0] * src[1]
    return sum(rows * row_bytes for rows, row_bytes in plane_rows(form, *src)) + 3.0 * wh + (3.0 + 1.5) * wh + sum(downscale_bytes(src, r) for r in rungs)


class Setup:
    """the library, and per workload: the sources, the rungs' encoders (job order: source by source, its rungs next to each other), 8-bit I420 pictures of the sources'
    size (the yardstick's sources, and what the composition exports into), and the source-sized encoders of the composition"""

    def __init__(self, n_sources, names, composition):
        import torch
        import scale_cases as sc
        import yuv_cases as yc
        import yuv_scale_cases as ys
        from homerhevc_amd.encoder import Picture
        self.torch, self.n, self.lib, self.made, self.work = torch, n_sources, ys.declare(pb.library()), [], {}
        self.structs = {"hmr_gpu_enc_load_sources_yuv_device": yc.YuvPicture, "hmr_gpu_enc_load_sources_scaled_device": sc.ScaledPicture,
                        "hmr_gpu_enc_load_sources_scaled_yuv": ys.ScaledYuvPicture, "hmr_gpu_enc_export_sources_device": Picture}
        for name in names:
            wl = WORKLOADS[name]
            w, h = wl["source"]
            rows = plane_rows(wl["form"], w, h)
            offsets = [sum(r * b for r, b in rows[:c]) for c in range(len(rows))]
            # (the kernel's time does not depend on the samples: random bytes are containers over their full range; a tensor of its own per source)
            srcs = [torch.randint(0, 256, (sum(r * b for r, b in rows),), dtype=torch.uint8, device="cuda") for _ in range(n_sources)]
            yuv = [yc.descriptor(wl["form"], [t.data_ptr() + o for o in offsets], [b for _, b in rows]) for t in srcs]
            rung_encs = [self.encoder(*r) for _ in range(n_sources) for r in wl["rungs"]]
            per = len(wl["rungs"])
            mid = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(n_sources)]
            planes = lambda t: [t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4]
            entry = {"srcs": srcs, "rung_encs": rung_encs, "yuv": yuv, "mid": mid,
                     "scaled_yuv": [ys.ScaledYuvPicture(pic=yuv[k // per], width=w, height=h) for k in range(len(rung_encs))],
                     "scaled": [sc.descriptor(0, planes(mid[k // per]), [w, w // 2, w // 2], w, h) for k in range(len(rung_encs))]}
            if composition:
                entry["top_encs"] = [self.encoder(w, h) for _ in range(n_sources)]
                entry["mid_pics"] = [pb.i420_picture(t, w, h) for t in mid]
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
        self.call("hmr_gpu_enc_load_sources_scaled_yuv", e["rung_encs"], e["scaled_yuv"])

    def yardstick(self, name):
        """the same jobs through k_downscale, from 8-bit I420 pictures of the sources' size"""
        e = self.work[name]
        self.call("hmr_gpu_enc_load_sources_scaled_device", e["rung_encs"], e["scaled"])

    def composition(self, name):
        e = self.work[name]
        self.call("hmr_gpu_enc_load_sources_yuv_device", e["top_encs"], e["yuv"])
        self.call("hmr_gpu_enc_export_sources_device", e["top_encs"], e["mid_pics"])
        self.call("hmr_gpu_enc_load_sources_scaled_device", e["rung_encs"], e["scaled"])

    def close(self):
        pb.close(self.lib, self.made)


def kernel_child(n_sources):
    """the traced program: per workload a warm-up launch and five timed ones of k_yuv_ladder, then as many of k_downscale over the same jobs"""
    for name in WORKLOADS:      # (one workload's tensors at a time: 64 2160p P010 sources are 1.6 GB)
        s = Setup(n_sources, [name], composition=False)
        for launch in (s.new_call, s.yardstick):
            for _ in range(LAUNCHES):
                launch(name)
                s.torch.cuda.synchronize()
        s.close()
        del s


def kernel_rate(n_sources):
    rows, command = pb.traced_child(__file__, ["--sources", str(n_sources)], "yuv_scale")
    groups = pb.launch_groups(rows, "k_yuv_ladder", len(WORKLOADS), LAUNCHES)
    yard = pb.launch_groups(rows, "k_downscale", len(WORKLOADS), LAUNCHES)
    for g in (groups, yard):
        if isinstance(g, dict):
            return g
    res = {"command": command, "yardsticks": {"float4_copy_tb_per_s": COPY_PEAK_TBS, "k_downscale": "the same jobs from 8-bit I420 pictures of the same sizes, in the same run"}}
    for (name, wl), part, ypart in zip(WORKLOADS.items(), groups, yard):
        jobs = n_sources * len(wl["rungs"])
        nbytes = n_sources * sum(yuv_scale_bytes(wl["form"], wl["source"], r) for r in wl["rungs"])
        ybytes = n_sources * sum(downscale_bytes(wl["source"], r) for r in wl["rungs"])
        record = pb.rate(part, nbytes, jobs_per_launch=jobs, bytes_per_launch=nbytes)
        record["k_downscale"] = pb.rate(ypart, ybytes, jobs_per_launch=jobs, bytes_per_launch=ybytes)
        record["share_of_k_downscale_rate"] = round(record["tb_per_s"] / record["k_downscale"]["tb_per_s"], 3)
        record["time_over_k_downscale"] = round(record["median_us"] / record["k_downscale"]["median_us"], 3)
        res[name] = record
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
            "model_bytes": {"new_call": n_sources * sum(yuv_scale_bytes(wl["form"], wl["source"], r) for r in wl["rungs"]),
                            "composition": n_sources * composition_bytes(wl["form"], wl["source"], wl["rungs"])},
            "hmr_gpu_enc_load_sources_scaled_yuv_ms": a, "call_returns_after_ms": returns,
            "load_yuv_then_export_sources_then_load_scaled_ms": b,
            "composition_over_new_call": round(b["median"] / a["median"], 2),
            "new_call_is_not_slower": bool(a["median"] <= b["median"] + (a["spread"] + b["spread"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--bench-this", nargs="+", default=[], help="files with bench.py's JSON line on this build (runs alternating with the parent's)")
    ap.add_argument("--bench-parent", nargs="+", default=[], help="files with bench.py's JSON line on the parent commit's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_scale_ingest_bench.json"))
    a = ap.parse_args()
    N = a.sources
    if a.kernel_child:
        kernel_child(N)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/yuv_scale_ingest_bench.py", "source_digest": source_digest(), "sources": N,
              "workloads": {k: {"source": list(v["source"]), "form": v["form"], "rungs": [list(r) for r in v["rungs"]],
                                "algorithmic_bytes_per_job": {f"{r[0]}x{r[1]}": yuv_scale_bytes(v["form"], v["source"], r) for r in v["rungs"]}} for k, v in WORKLOADS.items()}}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(N)
    result["replaces"] = {name: replaces(N, name) for name in WORKLOADS}
    result["replaces"]["expected"] = "nothing fixed in advance: on the ladders the composition converts once and scales three times from 8 bits, so it may win on kernel time and lose on wall time"
    ladder_bench(result, a)
    pb.write_result(result, a.out)


if __name__ == "__main__":
    main()
