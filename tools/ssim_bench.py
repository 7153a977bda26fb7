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
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import egress_bench as eb  # noqa: E402  (the kernel child's first step, k_egress with sums only, the bench section)
import ingest_bench as ib  # noqa: E402  (the workload and the encoders' set-up)
import picture_bench as pb  # noqa: E402

W, H, CLIP_FRAMES = ib.W, ib.H, ib.CLIP_FRAMES
BAR = 1.5
LAUNCHES = 6      # per kernel in the traced child: a warm-up and five timed


def ssim_bytes(width, height):
    """algorithmic bytes of one picture through k_ssim (the comment at k_ssim in csrc/picture_io.hip): the int16 planes of the final picture and of the slot are read once"""
    return 6.0 * float(width) * height


def ssim_device(lib, encs, slot, sums):
    S = len(encs)
    assert lib.hmr_gpu_enc_ssim_device((C.c_void_p * S)(*encs), S, (C.c_int * S)(*([slot] * S)), C.c_void_p(sums.data_ptr()), pb.stream_of()) == 0, lib.hmr_gpu_last_error()


def ssd_device(lib, encs, slot, sums):
    eb.export_device(lib, encs, None, slot, sums)


def kernel_child(S):
    """the traced program: every sequence encodes one picture, then LAUNCHES launches of k_ssim and as many of k_egress (sums only) over the S pictures, alternating"""
    torch, lib, made, encs = eb.encoded_once(S)
    sums = torch.zeros((S, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(LAUNCHES):
        for call in (ssim_device, ssd_device):
            call(lib, encs, 0, sums)
            torch.cuda.synchronize()
    pb.close(lib, made)


def kernel_rate(S):
    rows, command = pb.traced_child(__file__, ["--sequences", str(S)], "ssim")
    res = {"command": command, "pictures_per_launch": S, "bytes_formula": "3 W H read (final picture) + 3 W H read (slot), per picture: the same for both kernels",
           "bytes_per_launch": ssim_bytes(W, H) * S}
    for name in ("k_ssim", "k_egress"):
        groups = pb.launch_groups(rows, name, 1, LAUNCHES)
        if isinstance(groups, dict):
            return groups
        last = pb.kernel_rows(rows, name)[-1]
        res[name if name == "k_ssim" else "k_egress_sums_only"] = dict(pb.rate(groups[0], res["bytes_per_launch"]), vgpr_sgpr_lds=[last.get(k) for k in ("VGPR_Count", "SGPR_Count", "LDS_Block_Size")])
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
    eb.bench_runs(result, a)
    pb.write_result(result, a.out)


def streaming_step(S, steps, kr):
    torch, lib, made, clips, dev = ib.setup(S, with_clips=True)
    encs = [e for _, e in made]
    nclip = len(clips)
    pics = [[ib.i420(dev[i % nclip][f]) for i in range(S)] for f in range(CLIP_FRAMES)]
    for s in (0, 1):
        ib.load_device(lib, encs, s, pics[0])
    streams = ib.Streams(lib, encs)
    sums = torch.zeros((S, 3), dtype=torch.int64, device="cuda")
    frame = [0]

    def step(with_ssim):
        f = frame[0] % CLIP_FRAMES
        frame[0] += 1
        slot = frame[0] & 1
        ib.load_device(lib, encs, slot, pics[f])
        streams.encode(lib.hmr_gpu_enc_encode_batch_pipelined, slot)
        if with_ssim:
            ssim_device(lib, encs, slot, sums)

    for _ in range(CLIP_FRAMES // 2):      # steady state: the pool's buffers, the staging buffers, both paths' first calls; one round of the clip
        step(False)
        step(True)
    torch.cuda.synchronize()
    plain, measuring = ib.windows(torch, steps, step)
    streams.encode(lib.hmr_gpu_enc_encode_batch_pipelined, None)
    last = sums.cpu()
    kernel_ms = kr["k_ssim"]["median_us"] / 1e3 if "k_ssim" in kr else None
    sp, sm = pb.spread(plain), pb.spread(measuring)
    res = {"steps_per_window": steps, "pictures": f"every step ingests a fresh device picture per sequence (the clips' {CLIP_FRAMES} pictures in turn) and encodes it",
           "plain_ms_per_step": sp, "with_ssim_ms_per_step": sm, "k_ssim_ms": kernel_ms,
           "mean_luma_ssim_of_the_last_step": round(float(last[:, 0].double().mean()) / float(((W // 4 - 1) * (H // 4 - 1)) << 30), 4)}
    if kernel_ms is not None:
        bound = sp["median"] + kernel_ms + sp["spread"]
        res.update({"bound_ms": round(bound, 3), "condition": "median with SSIM <= median plain + k_ssim + spread of plain", "holds": bool(sm["median"] <= bound)})
    else:
        res["holds"] = "not measured (no kernel time)"
    pb.close(lib, made)
    return res


if __name__ == "__main__":
    main()
