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
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import picture_bench as pb  # noqa: E402
from picture_bench import COPY_PEAK_TBS, spread  # noqa: E402

SRC = (1920, 1080)
RUNGS = [(1920, 1080), (1280, 720), (960, 544), (640, 360)]
BIG, BIG_RUNG = (3840, 2160), (1920, 1080)
K_INGEST_TBS = 4.9            # profiles/ingest_bench.json: k_ingest on 256 x 1080p
LAUNCHES = 6                  # per workload in the traced child: a warm-up and five timed


def scale_bytes(src, dst):
    """the formula in the comment at k_downscale (csrc/picture_io.hip)"""
    return 1.5 * src[0] * src[1] + 3.0 * dst[0] * dst[1]


def setup(n_sources, big):
    """(torch, the library, the ladder's encoders as (context, encoder) pairs - job order: source by source, its rungs next to each other -, their sizes, the sources)"""
    import torch
    lib = pb.library()
    sizes = [r for _ in range(n_sources) for r in RUNGS]
    made = [pb.encoders(lib, 1, w, h)[0] for w, h in sizes]
    # (the kernel's time does not depend on the samples; a picture of its own per source: 64 x 3.1 MB, and 64 x 12.4 MB for 2160p)
    w, h = SRC
    srcs = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(n_sources)]
    bigs = [torch.randint(0, 256, (BIG[1] * 3 // 2, BIG[0]), dtype=torch.uint8, device="cuda") for _ in range(n_sources)] if big else []
    torch.cuda.synchronize()
    return torch, lib, made, sizes, srcs, bigs


def scaled(t, w, h):
    """the descriptor of a tightly packed I420 source picture of w x h in the tensor t"""
    import scale_cases
    return scale_cases.descriptor(0, [t.data_ptr(), t.data_ptr() + w * h, t.data_ptr() + w * h * 5 // 4], [w, w // 2, w // 2], w, h)


def load_scaled(lib, encs, pics):
    import scale_cases
    n = len(encs)
    assert lib.hmr_gpu_enc_load_sources_scaled_device((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([0] * n)), (scale_cases.ScaledPicture * n)(*pics), pb.stream_of()) == 0, lib.hmr_gpu_last_error()


def kernel_child(n_sources):
    """the traced program: a warm-up launch and five timed ones of the ladder, then the same of 2160p -> 1080p"""
    torch, lib, made, sizes, srcs, bigs = setup(n_sources, big=True)
    encs = [e for _, e in made]
    ladder = [scaled(srcs[k // len(RUNGS)], *SRC) for k in range(len(encs))]
    top = [e for e, s in zip(encs, sizes) if s == BIG_RUNG]
    for group, pics in ((encs, ladder), (top, [scaled(t, *BIG) for t in bigs])):
        for _ in range(LAUNCHES):
            load_scaled(lib, group, pics)
            torch.cuda.synchronize()
    pb.close(lib, made)


def workloads(n_sources):
    """(name, bytes per launch, jobs per launch) of the child's two groups of launches"""
    return [("ladder_1080p_x4", n_sources * sum(scale_bytes(SRC, r) for r in RUNGS), n_sources * len(RUNGS)), ("2160p_to_1080p", n_sources * scale_bytes(BIG, BIG_RUNG), n_sources)]


def kernel_rate(n_sources):
    rows, command = pb.traced_child(__file__, ["--sources", str(n_sources)], "scale")
    groups = pb.launch_groups(rows, "k_downscale", 2, LAUNCHES)
    if isinstance(groups, dict):
        return groups
    res = {"source_pictures": "one tensor per source; the four rungs of a source read the same bytes (that is the ladder)", "command": command,
           "yardsticks": {"float4_copy_tb_per_s": COPY_PEAK_TBS, "k_ingest_tb_per_s": K_INGEST_TBS}}
    for (name, nbytes, jobs), part in zip(workloads(n_sources), groups):
        res[name] = pb.rate(part, nbytes, jobs_per_launch=jobs, bytes_per_launch=nbytes)
        res[name]["share_of_k_ingest_4.9"] = round(pb.tb_per_s(part, nbytes) / K_INGEST_TBS, 3)
    return res


PMC = ["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_LDS_BANK_CONFLICT", "GRBM_GUI_ACTIVE"]


def counters(n_sources):
    """ONE counter pass of its own (no tracing beside it) over the kernel child: per workload the mean of each counter over k_downscale's dispatches"""
    rows, command = pb.counted_child(__file__, ["--sources", str(n_sources)], PMC)
    if isinstance(rows, dict):
        return rows
    rows = [r for r in rows if pb.is_kernel(r["Kernel_Name"], "k_downscale")]
    res = {"command": command}
    ids = sorted({int(r["Dispatch_Id"]) for r in rows})
    if len(ids) != 2 * LAUNCHES:
        return dict(res, error=f"{len(ids)} dispatches of k_downscale, {2 * LAUNCHES} expected")
    for name, part in (("ladder_1080p_x4", ids[1:LAUNCHES]), ("2160p_to_1080p", ids[LAUNCHES + 1:])):
        agg = {}
        for r in rows:
            if int(r["Dispatch_Id"]) in part:
                agg.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
        res[name] = {k: round(sum(v) / len(v)) for k, v in sorted(agg.items())}
    return res


def ladder_bench(result, a):
    """the bench section of the two ladder tools: the last line of every file, and whether this build's median is within the parent's run-to-run spread"""
    for name, paths in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        runs = pb.last_bench_lines(paths)
        if runs:
            result.setdefault("bench", {})[name] = {"runs": runs, "frames_per_s": spread([r["value"] for r in runs])}
    if set(result.get("bench", {})) == {"this_build", "parent"}:
        t, p = result["bench"]["this_build"]["frames_per_s"], result["bench"]["parent"]["frames_per_s"]
        result["bench"]["condition"] = "median of this build >= median of the parent - the parent's run-to-run spread"
        result["bench"]["holds"] = bool(t["median"] >= p["median"] - p["spread"])


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
    torch, lib, made, sizes, srcs, bigs = setup(N, big=False)
    from homerhevc_amd.encoder import Picture
    encs = [e for _, e in made]
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
        rung = {}
        for rw, rh in RUNGS:
            if (rw, rh) == SRC:
                rung[(rw, rh)] = batch
                continue
            ys = F.interpolate(y, size=(rh, rw), mode="area").add_(0.5).to(torch.uint8)
            cs = F.interpolate(c, size=(rh // 2, rw // 2), mode="area").add_(0.5).to(torch.uint8)
            rung[(rw, rh)] = torch.cat([ys.reshape(N, rh, rw), cs.reshape(N, rh // 2, rw)], dim=1)
        pics = [pb.i420_picture(rung[sizes[k]][k // len(RUNGS)], *sizes[k]) for k in range(n)]
        assert lib.hmr_gpu_enc_load_sources_device((C.c_void_p * n)(*encs), n, (C.c_int * n)(*([0] * n)), (Picture * n)(*pics), pb.stream_of()) == 0, lib.hmr_gpu_last_error()
        return rung

    for _ in range(2):      # steady state: the slots, both paths' first calls, torch's allocator
        load_scaled(lib, encs, ladder)
        composition()
        sync()
    scaled_ms, composed_ms = [], []
    for _ in range(5):
        sync()
        t0 = time.perf_counter()
        load_scaled(lib, encs, ladder)
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
    ladder_bench(result, a)
    pb.close(lib, made)
    pb.write_result(result, a.out)


if __name__ == "__main__":
    main()
