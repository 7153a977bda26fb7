#!/usr/bin/env python3
"""GPU box tool: what the scene-cut statistics (include/homer_gpu.h section 12m, k_cut in csrc/picture_io.hip) cost, on bench.py's flagship workload (256 sequences of
1920x1080, bench.py's configuration and clips, consecutive frames of the clips in the two slots).  Writes profiles/cut_bench.json.

    python tools/cut_bench.py [--sequences 256] [--steps 20] [--bench-this FILE ... --bench-parent FILE ...]

  kernel_rate      k_cut's (and k_cut_finish's) time for one call over all sequences' pictures from `rocprofv3 --kernel-trace --stats` in a run of its own (this program
                   starts it as a child, the traced program behind `--`, no counters), and the rate in candidate-SAD samples per second: 289 vectors x W x H sample
                   differences a picture, nominal (a block at the picture's edge has fewer valid vectors; the kernel's 340 slots a block are not counted).  Beside it,
                   from the same trace: k_ssim over the same encoders - the sibling that reads the same two int16 pictures (6 W H bytes) - and the ratio of the two.
                   No bar is set: nobody had measured this kernel.
  streaming_step   ms per step of BatchEncoder.step (pipelined) without and with a SceneCut policy, alternating, three windows each.  The clips are played forwards and
                   backwards in turn, so that no step but a clip's own cut sees one: the difference is the launch, the copy of 8 x n values and the host wait.
  bench            bench.py's lines of this build and of the parent commit's, when the files are given (all from the same GPU visit, alternating); no code bench.py
                   runs has changed, so equality within the run-to-run spread is expected
Timed windows are walls between two device synchronisations, in one process with the steady state warmed first."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import ingest_bench as ib  # noqa: E402  (the workload and the encoders' set-up)
import picture_bench as pb  # noqa: E402
import scale_ingest_bench as sb  # noqa: E402  (the bench section)
import ssim_bench as ssb  # noqa: E402  (the sibling's call)

W, H, CLIP_FRAMES = ib.W, ib.H, ib.CLIP_FRAMES
LAUNCHES = 6      # per kernel in the traced child: a warm-up and five timed
RANGE = 8


def cut_bytes(width, height):
    """algorithmic bytes of one picture through k_cut: the int16 planes of the two slots are read once (the kernel's comment has what the search window's rim adds)"""
    return 6.0 * float(width) * height


def candidate_samples(width, height):
    return float((2 * RANGE + 1) ** 2) * width * height


def cut_device(lib, encs, slot, stats):
    S = len(encs)
    assert lib.hmr_gpu_enc_cut_stats((C.c_void_p * S)(*encs), S, (C.c_int * S)(*([slot] * S)), (C.c_int * S)(*([slot ^ 1] * S)), C.c_void_p(stats.data_ptr()), pb.stream_of()) == 0, \
        lib.hmr_gpu_last_error()


def declared(lib):
    import cut_cases
    return cut_cases.declare(lib)


def kernel_child(S):
    """the traced program: every sequence encodes frame 0 of its clip from slot 0 and gets frame 1 into slot 1, then LAUNCHES calls of the cut statistics (slot 1 against
    slot 0) and as many of k_ssim (the final picture against slot 0) over the S pictures, alternating"""
    torch, lib, made, clips, dev = ib.setup(S, with_clips=True)
    lib = declared(lib)
    encs = [e for _, e in made]
    ib.load_device(lib, encs, 0, [ib.i420(dev[i % len(dev)][0]) for i in range(S)])
    ib.Streams(lib, encs).encode(lib.hmr_gpu_enc_encode_batch, 0)
    ib.load_device(lib, encs, 1, [ib.i420(dev[i % len(dev)][1]) for i in range(S)])
    stats = torch.zeros((S, 8), dtype=torch.int64, device="cuda")
    sums = torch.zeros((S, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(LAUNCHES):
        cut_device(lib, encs, 1, stats)
        torch.cuda.synchronize()
        ssb.ssim_device(lib, encs, 0, sums)
        torch.cuda.synchronize()
    pb.close(lib, made)


def kernel_rate(S):
    rows, command = pb.traced_child(__file__, ["--sequences", str(S)], "cut")
    res = {"command": command, "pictures_per_launch": S, "bytes_formula": "3 W H read (cur's slot) + 3 W H read (prev's slot), per picture: the same as k_ssim's two pictures",
           "bytes_per_launch": cut_bytes(W, H) * S, "candidate_samples_per_launch": candidate_samples(W, H) * S}
    for name in ("k_cut", "k_cut_finish", "k_ssim"):
        groups = pb.launch_groups(rows, name, 1, LAUNCHES)
        if isinstance(groups, dict):
            return groups
        last = pb.kernel_rows(rows, name)[-1]
        res[name] = dict(pb.rate(groups[0], res["bytes_per_launch"]), vgpr_sgpr_lds=[last.get(k) for k in ("VGPR_Count", "SGPR_Count", "LDS_Block_Size")])
    res["k_cut"]["candidate_sad_samples_per_s"] = float(f"{res['candidate_samples_per_launch'] / (res['k_cut']['median_us'] * 1e-6):.4g}")
    res["ratio_k_cut_to_k_ssim"] = round(res["k_cut"]["median_us"] / res["k_ssim"]["median_us"], 3)
    return res


def streaming_step(S, steps):
    import encoder_cases as ec
    from homerhevc_amd.encoder import BatchEncoder, EncoderConfig, SceneCut
    torch, lib, made, clips, dev = ib.setup(0, with_clips=True)
    nclip = len(dev)
    views = [[t.view(H * 3 // 2, W) for t in clip] for clip in dev]
    cfgs = [EncoderConfig(W, H, **{ec.KEY_NAMES.get(k, k): v for k, v in ib.KEYS.items()}) for _ in range(S)]
    order = list(range(CLIP_FRAMES)) + list(range(CLIP_FRAMES - 2, 0, -1))      # forwards, then backwards: no jump at the clip's end
    frame, cuts = [0], [0]
    policy = SceneCut()
    with BatchEncoder(cfgs) as enc:
        def step(with_policy):
            f = order[frame[0] % len(order)]
            frame[0] += 1
            enc.step([views[i % nclip][f] for i in range(S)], scene_cut=policy if with_policy else None)
            if with_policy:
                cuts[0] += sum(enc.last_cuts)

        for _ in range(len(order) // 2):      # steady state: the pool's buffers, both paths' first calls; one round of the clip
            step(False)
            step(True)
        torch.cuda.synchronize()
        cuts[0] = 0
        plain, with_policy = ib.windows(torch, steps, step)
        enc.flush()
        last = enc.cut_stats().cpu()
    sp, sw = pb.spread(plain), pb.spread(with_policy)
    return {"steps_per_window": steps, "pictures": f"every step ingests a fresh device picture per sequence (the clips' {CLIP_FRAMES} pictures forwards and backwards in turn) and encodes it",
            "plain_ms_per_step": sp, "with_scene_cut_ms_per_step": sw, "difference_of_medians_ms": round(sw["median"] - sp["median"], 3),
            "cuts_in_the_timed_windows": cuts[0], "mean_share_of_the_last_step": round(float(last[:, 6].double().mean()) / (W * H // 64), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--no-streaming-step", action="store_true")
    ap.add_argument("--bench-this", nargs="*", default=[], help="files with bench.py's JSON line on this build")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="files with bench.py's JSON line on the parent commit's build, from runs alternating with those")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_bench.json"))
    a = ap.parse_args()
    S = a.sequences
    if a.kernel_child:
        kernel_child(S)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/cut_bench.py", "source_digest": source_digest(), "sequences": S, "width": W, "height": H, "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": cut_bytes(W, H), "candidate_sad_samples_per_picture": candidate_samples(W, H), "resources": pb.resources("k_cut")}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(S)
    result["streaming_step"] = {"skipped": True} if a.no_streaming_step else streaming_step(S, a.steps)
    sb.ladder_bench(result, a)
    if "bench" not in result:
        result["bench"] = "not measured yet"
    pb.write_result(result, a.out)


if __name__ == "__main__":
    main()
