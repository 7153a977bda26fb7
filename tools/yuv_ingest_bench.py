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
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import ingest_bench as ib  # noqa: E402  (the workload, the encoders' set-up, the timed loops)
import picture_bench as pb  # noqa: E402
from ingest_bench import CLIP_FRAMES, CLIP_SEEDS, KEYS, H, W  # noqa: E402
from picture_bench import spread  # noqa: E402


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


def yuv_picture(frame):
    from homerhevc_amd.encoder import yuv_picture_of
    from yuv_cases import YuvPicture
    return YuvPicture.from_buffer_copy(yuv_picture_of(frame, W, H)[0])


def new_source(torch, form):
    """(the tensors of one picture of the form, its descriptor): random containers"""
    from homerhevc_amd.encoder import YUVFrame
    if form == "i420":
        t = torch.randint(0, 256, (W * H * 3 // 2,), dtype=torch.uint8, device="cuda")
        return t, ib.i420(t)
    kind, chroma, bits, msb = FORMS[form]
    wc, hc = (W if chroma == "444" else W // 2), (H // 2 if chroma == "420" else H)

    def plane(rows, cols):
        if bits == 8:
            return torch.randint(0, 256, (rows, cols), dtype=torch.uint8, device="cuda")
        return torch.randint(-32768, 32768, (rows, cols), dtype=torch.int16, device="cuda")      # (the 16 bits are read as unsigned)

    tensors = {"planar": lambda: (plane(H, W), plane(hc, wc), plane(hc, wc)), "semi": lambda: (plane(H, W), plane(hc, 2 * wc)), "packed": lambda: (plane(H, 2 * W),)}[kind]()
    frame = YUVFrame(tensors if len(tensors) > 1 else tensors[0], chroma=chroma, bits=bits, msb_aligned=msb)
    return tensors, yuv_picture(frame)


def load(lib, encs, slot, pics, deep):
    from yuv_cases import YuvPicture
    if deep:
        ib.load_many(lib, "hmr_gpu_enc_load_sources_yuv_device", YuvPicture, encs, slot, pics)
    else:
        ib.load_device(lib, encs, slot, pics)


def kernel_child(S):
    """the traced program: per form a warm-up launch and five timed ones over S pictures, each with a source of its own (the kernel's time does not depend on the
    samples); k_ingest over I420 first"""
    import torch
    lib = pb.library()
    made = pb.encoders(lib, S, W, H, **KEYS)
    encs = [e for _, e in made]
    for form in ["i420"] + list(FORMS):
        made_pics = [new_source(torch, form) for _ in range(S)]
        pics = [m[1] for m in made_pics]
        torch.cuda.synchronize()
        for _ in range(LAUNCHES):
            load(lib, encs, 0, pics, form != "i420")
            torch.cuda.synchronize()
        del made_pics, pics
        torch.cuda.empty_cache()
    pb.close(lib, made)


def kernel_rate(S, rgb_bench):
    rows, command = pb.traced_child(__file__, ["--sequences", str(S)], "yuv_ingest", timeout=1500)
    plain, deep = pb.launch_groups(rows, "k_ingest", 1, LAUNCHES), pb.launch_groups(rows, "k_ingest_yuv", len(FORMS), LAUNCHES)
    for groups in (plain, deep):
        if isinstance(groups, dict):
            return groups
    res = {"source_pictures": "one set of tensors per sequence (no two jobs of a launch share source bytes)", "command": command, "pictures_per_launch": S}
    for form, part in zip(["i420"] + list(FORMS), plain + deep):
        res[form] = pb.rate(part, picture_bytes(form) * S, kernel="k_ingest" if form == "i420" else "k_ingest_yuv", bytes_per_launch=picture_bytes(form) * S)
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


def bench_of(result, a):
    """bench.py's lines of this build and of the parent's, and whether this build's median lies inside (or above) the parent's run-to-run spread"""
    for name, path in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        runs = pb.bench_lines(path)
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
    from homerhevc_amd.encoder import YUVFrame
    result = {"tool": "tools/yuv_ingest_bench.py", "source_digest": source_digest(), "sequences": S, "width": W, "height": H, "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": {form: picture_bytes(form) for form in ["i420"] + list(FORMS)}}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(S, a.rgb_bench)
    import torch
    lib = pb.library()
    made = pb.encoders(lib, S, W, H, **KEYS)
    encs = [e for _, e in made]
    sync = torch.cuda.synchronize

    # ---- replaces ----
    sources = [new_source(torch, "p010_420") for _ in range(S)]
    yuv = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device="cuda") for _ in range(S)]
    deep_pics, yuv_pics = [m[1] for m in sources], [ib.i420(t) for t in yuv]

    def torch_route():
        for (tensors, _), o in zip(sources, yuv):
            torch_round_p010(torch, tensors[0], tensors[1], o)
        load(lib, encs, 1, yuv_pics, False)

    torch_route()
    load(lib, encs, 0, deep_pics, True)
    sync()
    torch_ms, fused_ms = ib.alternating(torch, torch_route, lambda: load(lib, encs, 0, deep_pics, True))
    result["replaces"] = {"what": f"one P010 frame of each of {S} sequences into a slot, wall ms between device synchronisations, alternating; torch route: widen to int32, mask, shift, "
                                  "round, clamp, to uint8, split the pairs, frame by frame into I420 tensors, then one hmr_gpu_enc_load_sources_device",
                          "p010_420": {"torch_ops_then_load_sources_device_ms": spread(torch_ms), "load_sources_yuv_device_ms": spread(fused_ms),
                                       "ratio_of_medians": round(statistics.median(torch_ms) / statistics.median(fused_ms), 1)}}
    del sources, yuv, deep_pics, yuv_pics
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
    pics = [[yuv_picture(p010[i % nclip][f]) for i in range(S)] for f in range(CLIP_FRAMES)]
    for s in (CLIP_FRAMES, CLIP_FRAMES + 1):
        load(lib, encs, s, pics[0], True)
    sync()
    kr = result["kernel_rate"]
    result["streaming_step"] = ib.streaming_step(torch, lib, encs, a.steps, lambda slot, f: load(lib, encs, slot, pics[f], True), kr["p010_420"]["median_us"] / 1e3 if "p010_420" in kr else None,
                                                 f"every window encodes the clips' {CLIP_FRAMES} pictures (as P010) in turn, starting at the first")
    bench_of(result, a)
    pb.close(lib, made)
    pb.write_result(result, a.out)


if __name__ == "__main__":
    main()
