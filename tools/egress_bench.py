#!/usr/bin/env python3
"""GPU box tool: what the device egress (include/homer_gpu.h section 12e, k_egress in csrc/picture_io.hip) costs and what it replaces, on bench.py's flagship workload
(256 sequences of 1920x1080, bench.py's configuration and clips).  Writes profiles/egress_bench.json.

    python tools/egress_bench.py [--sequences 256] [--steps 20] [--bench-this FILE ... --bench-parent FILE ...]

  kernel_rate      k_egress's time for one launch over all sequences' pictures - picture only, sums only, both; I420 and NV12 - from `rocprofv3 --kernel-trace --stats`
                   in a run of its own (this program starts it as a child, the traced program behind `--`, no counters); bytes from egress_bytes() below.  Yardsticks in
                   the same file: k_ingest re-measured in the same visit by tools/ingest_bench.py's own trace, and the 6.29 TB/s float4 copy.
  replaces         wall time between device synchronisations to leave one 8-bit picture of every sequence in device memory through hmr_gpu_enc_export_references8
                   and through ONE hmr_gpu_enc_export_pictures_device, alternating, five repetitions each.  The former runs the same kernel (one picture per launch on the
                   sequence's own stream): what is left between the two figures is a launch per picture and the host synchronisations
  streaming_step   ms per step of hmr_gpu_enc_encode_batch_pipelined plain and with an export (picture and sums) of every sequence after every step, alternating,
                   three windows each; the condition: median with export <= median plain + egress kernel time + spread of plain
  bench            bench.py's lines of this build and of the parent commit's, when the files are given (all from the same GPU visit, alternating)
Timed windows are walls between two device synchronisations, in one process with the steady state warmed first."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import ingest_bench as ib  # noqa: E402  (the workload, the encoders' set-up and k_ingest's trace)
import picture_bench as pb  # noqa: E402
from picture_bench import COPY_PEAK_TBS, spread  # noqa: E402

W, H, CLIP_FRAMES = ib.W, ib.H, ib.CLIP_FRAMES
VARIANTS = [("picture", True, False), ("sums", False, True), ("both", True, True)]
LAUNCHES = 6      # per variant and format in the traced child: a warm-up and five timed


def egress_bytes(width, height, picture, sums):
    """algorithmic bytes of one picture through k_egress (the formula in the header comment of csrc/picture_io.hip): the final picture is read (int16: 3 W H), the slot's picture is read when
    sums are asked for (3 W H), the 8-bit picture is written when one is asked for (1.5 W H)"""
    wh = float(width) * height
    return 3.0 * wh + (3.0 * wh if sums else 0.0) + (1.5 * wh if picture else 0.0)


def export_device(lib, encs, pics, slot, sums):
    from homerhevc_amd.encoder import Picture
    S = len(encs)
    assert lib.hmr_gpu_enc_export_pictures_device((C.c_void_p * S)(*encs), S, (Picture * S)(*pics) if pics is not None else None,
                                                  (C.c_int * S)(*([slot] * S)) if sums is not None else None, C.c_void_p(sums.data_ptr()) if sums is not None else None,
                                                  pb.stream_of()) == 0, lib.hmr_gpu_last_error()


def outputs(torch, S):
    """an output picture of its own per sequence, as I420 and as NV12 descriptors of the same memory"""
    outs = [torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda") for _ in range(S)]
    return outs, [ib.i420(t) for t in outs], [pb.nv12_picture(t, W, H) for t in outs]


def encoded_once(S):
    """what the egress and SSIM kernel children begin with: every sequence has encoded one picture of the clips (a picture the encoder is known to take; every sequence
    has planes of its own) from slot 0"""
    torch, lib, made, clips, dev = ib.setup(S, with_clips=True)
    encs = [e for _, e in made]
    ib.load_device(lib, encs, 0, [ib.i420(dev[i % len(dev)][0]) for i in range(S)])
    ib.Streams(lib, encs).encode(lib.hmr_gpu_enc_encode_batch, 0)
    return torch, lib, made, encs


def kernel_child(S):
    """the traced program: every sequence encodes one picture, then per variant and format a warm-up launch and five timed ones over the S pictures"""
    torch, lib, made, encs = encoded_once(S)
    outs, as_i420, as_nv12 = outputs(torch, S)
    sums = torch.zeros((S, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for pics in (as_i420, as_nv12):
        for _, picture, with_sums in VARIANTS:
            for _ in range(LAUNCHES):
                export_device(lib, encs, pics if picture else None, 0, sums if with_sums else None)
                torch.cuda.synchronize()
    pb.close(lib, made)


def kernel_rate(S):
    rows, command = pb.traced_child(__file__, ["--sequences", str(S)], "egress")
    groups = pb.launch_groups(rows, "k_egress", 2 * len(VARIANTS), LAUNCHES)
    if isinstance(groups, dict):
        return groups
    res = {"command": command, "pictures_per_launch": S, "output_pictures": "one tensor per sequence",
           "bytes_formula": "3 W H read + 3 W H read (sums) + 1.5 W H written (picture), per picture"}
    names = [(fmt, variant) for fmt in ("i420", "nv12") for variant in VARIANTS]
    for (fmt, (name, picture, with_sums)), part in zip(names, groups):
        nbytes = egress_bytes(W, H, picture, with_sums) * S
        res[f"{fmt}_{name}"] = pb.rate(part, nbytes, bytes_per_launch=nbytes)
    return res


def bench_runs(result, a):
    """the bench section of the egress and SSIM tools: the last line of every file, their median and spread"""
    for name, paths in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        runs = pb.last_bench_lines(paths)
        if runs:
            values = [r["value"] for r in runs]
            result.setdefault("bench", {})[name] = {"runs": runs, "median": statistics.median(values), "spread": round(max(values) - min(values), 4)}
    if "bench" not in result:
        result["bench"] = "not measured"
    if a.notes and os.path.exists(a.notes):
        result["notes"] = [ln.strip() for ln in open(a.notes) if ln.strip()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--bench-this", nargs="*", default=[], help="files with bench.py's JSON line on this build")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="files with bench.py's JSON line on the parent commit's build, from runs alternating with those")
    ap.add_argument("--notes", help="a text file whose lines become the result's notes (what the ISA or a trace shows about the rates)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "egress_bench.json"))
    a = ap.parse_args()
    S = a.sequences
    if a.kernel_child:
        kernel_child(S)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/egress_bench.py", "source_digest": source_digest(), "sequences": S, "width": W, "height": H, "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": {name: egress_bytes(W, H, p, s) for name, p, s in VARIANTS}}
    # (the traced children first: this process has not opened the GPU yet)
    if a.no_kernel_rate:
        result["kernel_rate"] = {"skipped": True}
    else:
        result["kernel_rate"] = kernel_rate(S)
        ingest = ib.kernel_rate(S)
        result["kernel_rate"]["yardsticks"] = {"k_ingest_same_visit": {k: ingest.get(k) for k in ("i420", "nv12", "error") if k in ingest},
                                               "k_ingest_profiles_ingest_bench_json_tb_per_s": {"i420": 4.94, "nv12": 5.27}, "float4_copy_tb_per_s": COPY_PEAK_TBS}
    torch, lib, made, clips, dev = ib.setup(S, with_clips=True)
    encs = [e for _, e in made]
    sync = torch.cuda.synchronize
    nclip = len(clips)
    pics = [[ib.i420(dev[i % nclip][f]) for i in range(S)] for f in range(CLIP_FRAMES)]
    for s in (0, 1):
        ib.load_device(lib, encs, s, pics[0])
    streams = ib.Streams(lib, encs)
    frame = [0]

    def step(export):
        f = frame[0] % CLIP_FRAMES
        frame[0] += 1
        slot = frame[0] & 1
        ib.load_device(lib, encs, slot, pics[f])
        streams.encode(lib.hmr_gpu_enc_encode_batch_pipelined, slot)
        if export:
            export_device(lib, encs, as_i420, slot, sums)

    outs, as_i420, as_nv12 = outputs(torch, S)
    sums = torch.zeros((S, 3), dtype=torch.int64, device="cuda")
    for _ in range(CLIP_FRAMES // 2):      # steady state: the pool's buffers, the staging buffers, both paths' first calls; one round of the clip
        step(False)
        step(True)
    sync()

    # replaces: the encoders hold the final pictures of the last step
    nb = lib.hmr_gpu_enc_reference_bytes(encs[0])
    rows8 = torch.empty((S, nb), dtype=torch.uint8, device="cuda")
    states = C.create_string_buffer(lib.hmr_gpu_enc_state_bytes() * S)
    old_ms, new_ms, returns_ms = [], [], []
    for rep in range(5):
        sync()
        t0 = time.perf_counter()
        assert lib.hmr_gpu_enc_export_references8(streams.encs, S, C.c_void_p(rows8.data_ptr()), nb, states) == 0, lib.hmr_gpu_last_error()
        sync()
        old_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        export_device(lib, encs, as_i420, 0, None)
        t1 = time.perf_counter()
        sync()
        new_ms.append((time.perf_counter() - t0) * 1e3)
        returns_ms.append(round((t1 - t0) * 1e3, 3))
    same = all(bool(torch.equal(rows8[i], outs[i])) for i in range(S))
    result["replaces"] = {"what": f"one 8-bit picture of each of {S} sequences left in device memory, wall ms between device synchronisations, alternating",
                          "hmr_gpu_enc_export_references8_ms": spread(old_ms), "hmr_gpu_enc_export_pictures_device_ms": spread(new_ms),
                          "export_pictures_device_call_returns_after_ms": returns_ms, "both_left_the_same_pictures": same,
                          "ratio_of_medians": round(statistics.median(old_ms) / statistics.median(new_ms), 1)}

    plain, exporting = ib.windows(torch, a.steps, step)
    streams.encode(lib.hmr_gpu_enc_encode_batch_pipelined, None)
    kr = result["kernel_rate"]
    kernel_ms = kr["i420_both"]["median_us"] / 1e3 if "i420_both" in kr else None
    sp, se = spread(plain), spread(exporting)
    result["streaming_step"] = {"steps_per_window": a.steps, "pictures": f"every step ingests a fresh device picture per sequence (the clips' {CLIP_FRAMES} pictures in turn) and encodes it",
                                "plain_ms_per_step": sp, "with_export_ms_per_step": se, "egress_kernel_ms": kernel_ms}
    if kernel_ms is not None:
        bound = sp["median"] + kernel_ms + sp["spread"]
        result["streaming_step"].update({"bound_ms": round(bound, 3), "condition": "median with export <= median plain + egress kernel + spread of plain", "holds": bool(se["median"] <= bound)})
    else:
        result["streaming_step"]["holds"] = "not measured (no kernel time)"
    bench_runs(result, a)
    pb.close(lib, made)
    pb.write_result(result, a.out)


if __name__ == "__main__":
    main()
