#!/usr/bin/env python3
"""GPU box tool: what the deep / 4:2:2 / 4:4:4 ingest (include/homer_gpu.h section 12k, k_ingest_yuv in csrc/picture_io.hip) costs and what it replaces, on bench.py's
flagship workload (256 sequences of 1920x1080, bench.py's configuration and clips).  Follows tools/rgb_ingest_bench.py.  Writes profiles/yuv_ingest_bench.json.

    python tools/yuv_ingest_bench.py [--sequences 256] [--steps 20] [--bench-this FILE --bench-parent FILE] [--rgb-bench FILE] [--from-files]

  kernel_rate      k_ingest_yuv's time for one launch over all sequences' pictures, per form (8-bit 4:2:2 planar, 8-bit 4:4:4 planar, YUYV, P010 4:2:0, 10-bit low-aligned
                   planar 4:2:0, 16-bit 4:4:4 planar), and k_ingest's over I420 pictures in the same run - the yardstick -, from `rocprofv3 --kernel-trace --stats` in a run
                   of its own (this program starts it as a child, the traced program behind `--`, no counters).  Every job has a source of its own.  Bytes from the
                   formula in the comment at k_ingest_yuv (csrc/picture_io.hip): sb (W H + 2 Wc Hc) read, 3 W H written per picture (k_ingest: 1.5 W H read, 3 W H written).
                   With --rgb-bench (profiles/rgb_ingest_bench.json of the same GPU visit): the comparison kernel's share - k_ingest_rgb planar 8-bit over k_ingest -
                   and whether every form reaches that share of k_ingest's rate, the margin being the spread of the five timed launches
  replaces         wall time of ONE hmr_gpu_enc_load_sources_yuv_device over one P010 frame per sequence, against what a user writes today: the rounding in torch ops,
                   frame by frame, into I420 tensors, then ONE hmr_gpu_enc_load_sources_device; alternating, five repetitions
  streaming_step   ms per step of hmr_gpu_enc_encode_batch_pipelined with the slots preloaded and with a fresh P010 picture ingested for every sequence before every
                   step, alternating, three repetitions each; the condition: median streaming <= median preloaded + kernel time + spread of preloaded.  Both kinds of
                   window encode the same samples: the P010 pictures round to the preloaded clip
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

# form -> (tensors of a YUVFrame: "planar" / "semi" / "packed", chroma, bits, msb_aligned)
FORMS = {"planar_422_8": ("planar", "422", 8, False), "planar_444_8": ("planar", "444", 8, False), "yuyv_8": ("packed", "422", 8, False), "p010_420": ("semi", "420", 10, True),
         "planar_420_10": ("planar", "420", 10, False), "planar_444_16": ("planar", "444", 16, False)}
LAUNCHES = 6                                                                # per form: a warm-up and five timed


def picture_bytes(form):
    """algorithmic bytes of one picture: the comment at k_ingest_yuv in csrc/picture_io.hip (k_ingest: 1.5 W H read, 3 W H written)"""
    if form == "i420":
        return 4.5 * W * H
    _, chroma, bits, _ = FORMS[form]
    return ((2 if bits > 8 else 1) * {"420": 1.5, "422": 2.0, "444": 3.0}[chroma] + 3.0) * W * H


def setup(S):
    import torch
    import encoder_cases as ec
    import libs
    from homerhevc_amd.encoder import Picture, YuvPicture
    lib = libs.load_gpu()
    P, I, L = C.c_void_p, C.c_int, C.c_long
    lib.hmr_gpu_last_error.restype = C.c_char_p
    lib.hmr_gpu_create.argtypes = [C.POINTER(P), I, P]
    lib.hmr_gpu_destroy.argtypes = [P]
    lib.hmr_gpu_enc_create.argtypes = [P, C.POINTER(ec.EncCfg), C.POINTER(P)]
    lib.hmr_gpu_enc_destroy.argtypes = [P]
    lib.hmr_gpu_enc_load_source.argtypes = [P, I] + [C.c_char_p] * 3
    lib.hmr_gpu_enc_load_sources_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(Picture), P]
    lib.hmr_gpu_enc_load_sources_yuv_device.argtypes = [C.POINTER(P), I, C.POINTER(I), C.POINTER(YuvPicture), P]
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


def new_source(torch, form):
    """(the tensors of one picture of the form, its descriptor): random containers"""
    from homerhevc_amd.encoder import YUVFrame, yuv_picture_of
    if form == "i420":
        t = torch.randint(0, 256, (W * H * 3 // 2,), dtype=torch.uint8, device="cuda")
        return t, i420_picture(t)
    kind, chroma, bits, msb = FORMS[form]
    wc, hc = (W if chroma == "444" else W // 2), (H // 2 if chroma == "420" else H)

    def plane(rows, cols):
        if bits == 8:
            return torch.randint(0, 256, (rows, cols), dtype=torch.uint8, device="cuda")
        return torch.randint(-32768, 32768, (rows, cols), dtype=torch.int16, device="cuda")      # (the 16 bits are read as unsigned)

    tensors = {"planar": lambda: (plane(H, W), plane(hc, wc), plane(hc, wc)), "semi": lambda: (plane(H, W), plane(hc, 2 * wc)), "packed": lambda: (plane(H, 2 * W),)}[kind]()
    frame = YUVFrame(tensors if len(tensors) > 1 else tensors[0], chroma=chroma, bits=bits, msb_aligned=msb)
    return tensors, yuv_picture_of(frame, W, H)[0]


def load(lib, torch, encs, slot, pics, deep):
    from homerhevc_amd.encoder import Picture, YuvPicture
    S = len(encs)
    fn = lib.hmr_gpu_enc_load_sources_yuv_device if deep else lib.hmr_gpu_enc_load_sources_device
    assert fn((C.c_void_p * S)(*encs), S, (C.c_int * S)(*([slot] * S)), ((YuvPicture if deep else Picture) * S)(*pics), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, \
        lib.hmr_gpu_last_error()


def kernel_child(S):
    """the traced program: per form a warm-up launch and five timed ones over S pictures, each with a source of its own (the kernel's time does not depend on the
    samples); k_ingest over I420 first"""
    torch, lib, encs, ctxs = setup(S)
    for form in ["i420"] + list(FORMS):
        made = [new_source(torch, form) for _ in range(S)]
        pics = [m[1] for m in made]
        torch.cuda.synchronize()
        for _ in range(LAUNCHES):
            load(lib, torch, encs, 0, pics, form != "i420")
            torch.cuda.synchronize()
        del made, pics
        torch.cuda.empty_cache()
    for e, c in zip(encs, ctxs):
        lib.hmr_gpu_enc_destroy(e)
        lib.hmr_gpu_destroy(c)


def kernel_rate(S, rgb_bench):
    with tempfile.TemporaryDirectory(prefix="yuv_ingest_prof_") as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "yuv_ingest", "--", sys.executable, os.path.abspath(__file__), "--kernel-child",
               "--sequences", str(S)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        if r.returncode != 0:
            return {"error": f"rocprofv3 run failed ({r.returncode})", "stderr_tail": r.stderr[-1500:]}
        traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not traces:
            return {"error": "no kernel trace written", "files": sorted(os.listdir(out))}
        rows = [r for r in csv.DictReader(open(traces[0])) if "k_ingest" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    plain = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "k_ingest_yuv" not in r["Kernel_Name"]]
    deep = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "k_ingest_yuv" in r["Kernel_Name"]]
    if len(plain) != LAUNCHES or len(deep) != LAUNCHES * len(FORMS):
        return {"error": f"{len(plain)} launches of k_ingest and {len(deep)} of k_ingest_yuv in the trace, {LAUNCHES} and {LAUNCHES * len(FORMS)} expected", "k_ingest_us": plain, "k_ingest_yuv_us": deep}
    res = {"source_pictures": "one set of tensors per sequence (no two jobs of a launch share source bytes)",
           "command": "rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_DIR -o yuv_ingest -- python tools/yuv_ingest_bench.py --kernel-child --sequences " + str(S),
           "pictures_per_launch": S}
    parts = {"i420": plain[1:]}
    for k, form in enumerate(FORMS):
        parts[form] = deep[LAUNCHES * k + 1:LAUNCHES * (k + 1)]
    for form, part in parts.items():
        med = statistics.median(part)
        tbs = picture_bytes(form) * S / (med * 1e-6) / 1e12
        res[form] = {"kernel": "k_ingest" if form == "i420" else "k_ingest_yuv", "bytes_per_launch": picture_bytes(form) * S, "launch_us": [round(x, 1) for x in part], "median_us": round(med, 1),
                     "tb_per_s": round(tbs, 3), "share_of_float4_copy_6.29": round(tbs / COPY_PEAK_TBS, 3)}
    for form in FORMS:
        res[form]["rate_over_k_ingest_i420"] = round(res[form]["tb_per_s"] / res["i420"]["tb_per_s"], 3)
    res["target"] = target_of(res, rgb_bench)
    return res


def target_of(res, rgb_bench):
    """The target: no form below the share of k_ingest's rate that k_ingest_rgb planar 8-bit reaches (tools/rgb_ingest_bench.py, same GPU visit); margin: the spread of
    the form's five timed launches, as a share of their median.  From the figures a result file holds, so it can be made again without a GPU (--from-files)."""
    target = {"comparison_kernel": "k_ingest_rgb planar 8-bit over k_ingest I420, from tools/rgb_ingest_bench.py in the same GPU visit", "measured": False}
    if not rgb_bench or not os.path.exists(rgb_bench):
        return target
    kr = json.load(open(rgb_bench)).get("kernel_rate", {})
    if "planar8" not in kr or "rate_over_k_ingest_i420" not in kr["planar8"]:
        return target
    share = kr["planar8"]["rate_over_k_ingest_i420"]
    missed = {}
    for form in FORMS:
        part = res[form]["launch_us"]
        margin = (max(part) - min(part)) / statistics.median(part)
        if res[form]["rate_over_k_ingest_i420"] * (1.0 + margin) < share:
            missed[form] = {"rate_over_k_ingest_i420": res[form]["rate_over_k_ingest_i420"], "margin": round(margin, 3)}
    target.update({"measured": True, "share": share, "holds": not missed, "forms_below": missed,
                   "comparison": {"k_ingest_i420_median_us": kr["i420"]["median_us"], "k_ingest_rgb_planar8_median_us": kr["planar8"]["median_us"], "k_ingest_rgb_planar8_tb_per_s": kr["planar8"]["tb_per_s"]},
                   # the two formulas do not count alike: the formula at k_ingest_rgb takes 4 W H for the slot's int16 planes, the formula at k_ingest_yuv and k_ingest's 4.5 W H take the 3 W H
                   # they hold (Y 2 W H, U and V W H / 2 each).  The pair below moves the same bytes whichever way they are counted: three 8-bit planes of W x H in, one slot out
                   "same_traffic": {"what": "planar 8-bit 4:4:4 through k_ingest_yuv against planar 8-bit RGB through k_ingest_rgb: 3 W H read and one slot written by both",
                                    "k_ingest_yuv_planar_444_8_median_us": res["planar_444_8"]["median_us"], "k_ingest_rgb_planar8_median_us": kr["planar8"]["median_us"],
                                    "time_ratio": round(res["planar_444_8"]["median_us"] / kr["planar8"]["median_us"], 3)},
                   "reason_if_missed": "the comparison's share is by hmr_ingest_rgb_bytes, which counts 4 W H written where the slot holds 3 W H: 7 instead of 6 W H for planar 8-bit, a "
                                       "factor 1.167 that hmr_ingest_yuv_bytes does not have; see same_traffic"})
    return target


def bench_lines(path):
    lines = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
    return [{k: b.get(k) for k in ("value", "unit", "ms_per_step", "steps", "warmup", "build")} for b in lines if b.get("value") is not None and "metric" in b]


def bench_of(result, a):
    """bench.py's lines of this build and of the parent's, and whether this build's median lies inside (or above) the parent's run-to-run spread"""
    for name, path in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        if path and os.path.exists(path):
            runs = bench_lines(path)
            if runs:
                values = [r["value"] for r in runs]
                result.setdefault("bench", {})[name] = {"runs": runs, "median": round(statistics.median(values), 4), "min": min(values), "max": max(values)}
    b = result.get("bench", {})
    if "this_build" in b and "parent" in b:
        b["this_build_not_below_the_parents_runs"] = bool(b["this_build"]["median"] >= b["parent"]["min"])


def torch_round_p010(torch, y16, uv16, out):
    """what a user writes today: P010 ([H, W] and [H / 2, W] int16, the ten bits on top) to an I420 tensor [H * 3 // 2, W], rounded to 8 bits"""
    def eight(t):
        ten = (t.to(torch.int32) & 0xffff) >> 6
        return ((ten + 2) >> 2).clamp(max=255).to(torch.uint8)
    out[:H] = eight(y16)
    c = eight(uv16).view(H // 2, W // 2, 2)
    out[H:H + H // 4] = c[:, :, 0].reshape(H // 4, W)
    out[H + H // 4:] = c[:, :, 1].reshape(H // 4, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--bench-this", help="file with bench.py's JSON line on this build")
    ap.add_argument("--bench-parent", help="file with bench.py's JSON line on the parent commit's build")
    ap.add_argument("--rgb-bench", help="profiles/rgb_ingest_bench.json of the same GPU visit: the comparison kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_ingest_bench.json"))
    ap.add_argument("--from-files", action="store_true", help="no GPU: make the `target` and `bench` sections of the --out file again from --rgb-bench, --bench-this and --bench-parent")
    a = ap.parse_args()
    S = a.sequences
    if a.kernel_child:
        kernel_child(S)
        return
    if a.from_files:
        result = json.load(open(a.out))
        if "i420" in result.get("kernel_rate", {}):
            result["kernel_rate"]["target"] = target_of(result["kernel_rate"], a.rgb_bench)
        result.pop("bench", None)
        bench_of(result, a)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        print(json.dumps({k: result.get(k) for k in ("bench",)}), json.dumps(result["kernel_rate"].get("target")))
        return
    import numpy as np
    import encoder_cases as ec
    from homerhevc_amd.build import source_digest
    from homerhevc_amd.encoder import YUVFrame, yuv_picture_of
    result = {"tool": "tools/yuv_ingest_bench.py", "source_digest": source_digest(), "sequences": S, "width": W, "height": H, "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": {form: picture_bytes(form) for form in ["i420"] + list(FORMS)}}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(S, a.rgb_bench)
    torch, lib, encs, ctxs = setup(S)
    sync = torch.cuda.synchronize

    # ---- replaces ----
    made = [new_source(torch, "p010_420") for _ in range(S)]
    yuv = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(S)]
    deep_pics, yuv_pics = [m[1] for m in made], [i420_picture(t) for t in yuv]

    def torch_route():
        for (tensors, _), o in zip(made, yuv):
            torch_round_p010(torch, tensors[0], tensors[1], o)
        load(lib, torch, encs, 1, yuv_pics, False)

    torch_route()
    load(lib, torch, encs, 0, deep_pics, True)
    sync()
    fused_ms, torch_ms = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        torch_route()
        sync()
        torch_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        load(lib, torch, encs, 0, deep_pics, True)
        sync()
        fused_ms.append((time.perf_counter() - t0) * 1e3)
    result["replaces"] = {"what": f"one P010 frame of each of {S} sequences into a slot, wall ms between device synchronisations, alternating; torch route: widen to int32, mask, shift, "
                                  "round, clamp, to uint8, split the pairs, frame by frame into I420 tensors, then one hmr_gpu_enc_load_sources_device",
                          "p010_420": {"torch_ops_then_load_sources_device_ms": spread(torch_ms), "load_sources_yuv_device_ms": spread(fused_ms),
                                       "ratio_of_medians": round(statistics.median(torch_ms) / statistics.median(fused_ms), 1)}}
    del made, yuv, deep_pics, yuv_pics
    torch.cuda.empty_cache()

    # ---- streaming step ----
    nclip = len(CLIP_SEEDS)
    rng = np.random.default_rng(0)
    p010, clips = [], []
    for sd in CLIP_SEEDS:
        frames_dev, frames_yuv = [], []
        for planes in ec.clip_frames(W, H, CLIP_FRAMES, seed=sd):
            y8, u8, v8 = (np.frombuffer(p, np.uint8).reshape(shape).astype(np.int64) for p, shape in zip(planes, ((H, W), (H // 2, W // 2), (H // 2, W // 2))))
            wide = lambda p: ((((p << 2) + rng.integers(0, 2, p.shape)) << 6) | rng.integers(0, 64, p.shape)).astype("<u2").view(np.int16)      # rounds back to p
            ty, tuv = torch.from_numpy(wide(y8)).cuda(), torch.from_numpy(np.stack([wide(u8), wide(v8)], axis=2)).cuda()
            frames_dev.append(YUVFrame((ty, tuv), bits=10, msb_aligned=True))
            frames_yuv.append(planes)
        p010.append(frames_dev)
        clips.append(frames_yuv)
    # slots 0 .. CLIP_FRAMES - 1: the clip through the host entry (bench.py's preload); slots CLIP_FRAMES, CLIP_FRAMES + 1: the P010 path's two
    for i, e in enumerate(encs):
        for f, planes in enumerate(clips[i % nclip]):
            assert lib.hmr_gpu_enc_load_source(e, f, *planes) == 0, lib.hmr_gpu_last_error()
    pics = [[yuv_picture_of(p010[i % nclip][f], W, H)[0] for i in range(S)] for f in range(CLIP_FRAMES)]
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
    kernel_ms = kr["p010_420"]["median_us"] / 1e3 if "p010_420" in kr else None
    sp, ss = spread(pre), spread(stream)
    result["streaming_step"] = {"steps_per_window": a.steps, "pictures": f"every window encodes the clips' {CLIP_FRAMES} pictures (as P010) in turn, starting at the first",
                                "preloaded_ms_per_step": sp, "streaming_ms_per_step": ss, "ingest_kernel_ms": kernel_ms}
    if kernel_ms is not None:
        bound = sp["median"] + kernel_ms + sp["spread"]
        result["streaming_step"].update({"bound_ms": round(bound, 3), "condition": "median streaming <= median preloaded + ingest kernel + spread of preloaded",
                                         "holds": bool(ss["median"] <= bound)})
    bench_of(result, a)
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
