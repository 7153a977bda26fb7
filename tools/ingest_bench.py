#!/usr/bin/env python3
"""GPU box tool: what the device ingest (include/homer_gpu.h section 12d, k_ingest in csrc/picture_io.hip) costs and what it replaces, on bench.py's flagship workload
(256 sequences of 1920x1080, bench.py's configuration and clips).  Writes profiles/ingest_bench.json.

    python tools/ingest_bench.py [--sequences 256] [--steps 20] [--bench-this FILE --bench-parent FILE]

  kernel_rate      k_ingest's time for one launch over all sequences' pictures, I420 and NV12, from `rocprofv3 --kernel-trace --stats` in a run of its own (this
                   program starts it as a child, the traced program behind `--`, no counters); bytes from the formula 1.5 W H read + 3 W H written per picture
  replaces         wall time to bring one picture of every sequence into a slot through hmr_gpu_enc_load_source (host planes) and through ONE
                   hmr_gpu_enc_load_sources_device, alternating, five repetitions each.  The host entry runs the same kernel (one picture per launch): what is left
                   between the two figures is its copies from host memory, a launch and a synchronisation per picture
  streaming_step   ms per step of hmr_gpu_enc_encode_batch_pipelined with the slots preloaded (what bench.py times) and with a fresh device picture ingested for every
                   sequence before every step, alternating, three repetitions each; the condition streaming <= preloaded + kernel time + spread of preloaded
  bench            bench.py's line of this build and of the parent commit's, when the two files are given (both from the same GPU visit)
Timed windows are walls between two device synchronisations, in one process with the steady state warmed first."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import picture_bench as pb  # noqa: E402
from picture_bench import spread  # noqa: E402

W, H, KEYS = 1920, 1080, {"wpp": 17}          # bench.py WORKLOADS["cfg2-1080p-encode"]
CLIP_SEEDS = [1234, 1, 2, 3, 4, 5, 6, 7]      # bench.py CLIP_SEEDS
CLIP_FRAMES = 10                              # (a timed window of 20 steps is two rounds of a clip: every window encodes the same pictures)
PICTURE_BYTES = 1.5 * W * H + 3.0 * W * H
LAUNCHES = 6                                  # per format in the traced child: a warm-up and five timed


def setup(S, with_clips):
    """(torch, the library, S encoders of the workload as (context, encoder) pairs, the clips' frames or None, a device tensor per picture)"""
    import numpy as np
    import torch
    import encoder_cases as ec
    lib = pb.library()
    made = pb.encoders(lib, S, W, H, **KEYS)
    if with_clips:
        clips = [ec.clip_frames(W, H, CLIP_FRAMES, seed=sd) for sd in CLIP_SEEDS]
        dev = [[torch.from_numpy(np.frombuffer(b"".join(planes), np.uint8).copy()).cuda() for planes in clip] for clip in clips]
    else:      # (the kernel's time does not depend on the samples; a picture of its own per sequence, so that no launch finds its source in a cache: S x 3.1 MB)
        clips = None
        dev = [[torch.randint(0, 256, (W * H * 3 // 2,), dtype=torch.uint8, device="cuda")] for _ in range(S)]
    torch.cuda.synchronize()
    return torch, lib, made, clips, dev


def i420(t):
    return pb.i420_picture(t, W, H)


def load_many(lib, name, struct, encs, slot, pics):
    """ONE hmr_gpu_enc_load_sources_*_device call: a picture of `struct` per encoder, all into `slot`"""
    S = len(encs)
    assert getattr(lib, name)((C.c_void_p * S)(*encs), S, (C.c_int * S)(*([slot] * S)), (struct * S)(*pics), pb.stream_of()) == 0, lib.hmr_gpu_last_error()


def load_device(lib, encs, slot, pics):
    from homerhevc_amd.encoder import Picture
    load_many(lib, "hmr_gpu_enc_load_sources_device", Picture, encs, slot, pics)


class Streams:
    """the access-unit buffers of S encoders and the arguments hmr_gpu_enc_encode_batch(_pipelined) takes for them"""

    def __init__(self, lib, encs):
        S = len(encs)
        self.lib, self.S, self.bufs = lib, S, [C.create_string_buffer(4 << 20) for _ in range(S)]
        self.encs = (C.c_void_p * S)(*encs)
        self.ptrs = (C.c_char_p * S)(*[C.cast(b, C.c_char_p) for b in self.bufs])
        self.caps = (C.c_long * S)(*[len(b) for b in self.bufs])
        self.got = (C.c_long * S)()

    def encode(self, fn, slot):
        """one call of fn over all encoders; slot None flushes the pipelined entry"""
        slots = (C.c_int * self.S)(*([slot] * self.S)) if slot is not None else None
        assert fn(self.encs, self.S, slots, None, self.ptrs, self.caps, self.got) == 0, self.lib.hmr_gpu_last_error()


def windows(torch, steps, step, repetitions=3):
    """ms per step of `steps` calls of step(False) and of step(True) between two device synchronisations, alternating: (the first kind's windows, the second's)"""
    def window(flag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(flag)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    plain, other = [], []
    for _ in range(repetitions):
        plain.append(window(False))
        other.append(window(True))
    return plain, other


def kernel_child(S):
    """the traced program: a warm-up launch and five timed ones over S I420 pictures, then the same over S NV12 pictures"""
    torch, lib, made, clips, dev = setup(S, with_clips=False)
    encs = [e for _, e in made]
    nv = []
    for clip in dev:
        t = clip[0]
        uv = torch.stack([t[W * H:W * H * 5 // 4], t[W * H * 5 // 4:]], dim=1).reshape(-1)
        nv.append(torch.cat([t[:W * H], uv]).contiguous())
    torch.cuda.synchronize()
    for pics in ([i420(dev[i % len(dev)][0]) for i in range(S)], [pb.nv12_picture(nv[i % len(nv)], W, H) for i in range(S)]):
        for _ in range(LAUNCHES):
            load_device(lib, encs, 0, pics)
            torch.cuda.synchronize()
    pb.close(lib, made)


def kernel_rate(S):
    rows, command = pb.traced_child(__file__, ["--sequences", str(S)], "ingest")
    groups = pb.launch_groups(rows, "k_ingest", 2, LAUNCHES)
    if isinstance(groups, dict):
        return groups
    res = {"source_pictures": "one tensor per sequence (no two jobs of a launch share source bytes)", "command": command, "pictures_per_launch": S,
           "bytes_per_launch": PICTURE_BYTES * S, "yardstick": "k_subpel_*: 1.98 TB/s (VERDICT 12)"}
    for name, part in zip(("i420", "nv12"), groups):
        res[name] = pb.rate(part, PICTURE_BYTES * S)
    return res


def alternating(torch, first, second, repetitions=5):
    """wall ms of first() and of second(), each up to the device synchronisation behind it, in turn: (first's times, second's)"""
    times = ([], [])
    for _ in range(repetitions):
        for fn, ms in zip((first, second), times):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
    return times


def streaming_step(torch, lib, encs, steps, load_fresh, kernel_ms, pictures):
    """The streaming_step section of the ingest tools.  Slots 0 .. CLIP_FRAMES - 1 hold the clip (bench.py's preload); load_fresh(slot, f) ingests picture f of every
    sequence into one of the slots CLIP_FRAMES, CLIP_FRAMES + 1.  Windows of `steps` pipelined batch steps, preloaded and streaming in turn."""
    streams = Streams(lib, encs)
    frame = [0]

    def step(streaming):
        f = frame[0] % CLIP_FRAMES
        frame[0] += 1
        slot = f
        if streaming:
            slot = CLIP_FRAMES + (frame[0] & 1)
            load_fresh(slot, f)
        streams.encode(lib.hmr_gpu_enc_encode_batch_pipelined, slot)

    for _ in range(CLIP_FRAMES // 2):      # steady state: the pool's buffers, the staging buffers, both paths' first calls; one round of the clip
        step(False)
        step(True)
    pre, stream = windows(torch, steps, step)
    streams.encode(lib.hmr_gpu_enc_encode_batch_pipelined, None)
    sp, ss = spread(pre), spread(stream)
    res = {"steps_per_window": steps, "pictures": pictures, "preloaded_ms_per_step": sp, "streaming_ms_per_step": ss, "ingest_kernel_ms": kernel_ms}
    if kernel_ms is not None:
        bound = sp["median"] + kernel_ms + sp["spread"]
        res.update({"bound_ms": round(bound, 3), "condition": "median streaming <= median preloaded + ingest kernel + spread of preloaded", "holds": bool(ss["median"] <= bound)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernel-rate", action="store_true")
    ap.add_argument("--bench-this", help="file with bench.py's JSON line on this build")
    ap.add_argument("--bench-parent", help="file with bench.py's JSON line on the parent commit's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    a = ap.parse_args()
    S = a.sequences
    if a.kernel_child:
        kernel_child(S)
        return
    from homerhevc_amd.build import source_digest
    result = {"tool": "tools/ingest_bench.py", "source_digest": source_digest(), "sequences": S, "width": W, "height": H, "configuration": "bench.py cfg2-1080p-encode (wfpp_num_threads 17)",
              "algorithmic_bytes_per_picture": PICTURE_BYTES}
    # (the traced child first: this process has not opened the GPU yet)
    result["kernel_rate"] = {"skipped": True} if a.no_kernel_rate else kernel_rate(S)
    torch, lib, made, clips, dev = setup(S, with_clips=True)
    encs = [e for _, e in made]
    sync = torch.cuda.synchronize
    nclip = len(clips)
    # slots 0 .. CLIP_FRAMES - 1: the clip through the host entry (bench.py's preload); slots CLIP_FRAMES, CLIP_FRAMES + 1: the device path's two
    t0 = time.perf_counter()
    for i, e in enumerate(encs):
        for f, planes in enumerate(clips[i % nclip]):
            assert lib.hmr_gpu_enc_load_source(e, f, *planes) == 0, lib.hmr_gpu_last_error()
    sync()
    result["preload_all_slots_s"] = round(time.perf_counter() - t0, 2)
    pics = [[i420(dev[i % nclip][f]) for i in range(S)] for f in range(CLIP_FRAMES)]
    for s in (CLIP_FRAMES, CLIP_FRAMES + 1):
        load_device(lib, encs, s, pics[0])
    sync()

    host_ms, device_ms = [], []
    for rep in range(5):
        f = rep % CLIP_FRAMES
        sync()
        t0 = time.perf_counter()
        for i, e in enumerate(encs):
            assert lib.hmr_gpu_enc_load_source(e, f, *clips[i % nclip][f]) == 0, lib.hmr_gpu_last_error()
        sync()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        load_device(lib, encs, CLIP_FRAMES, pics[f])
        t1 = time.perf_counter()
        sync()
        device_ms.append((time.perf_counter() - t0) * 1e3)
        result.setdefault("load_sources_device_call_returns_after_ms", []).append(round((t1 - t0) * 1e3, 3))
    result["replaces"] = {"what": f"one picture of each of {S} sequences into a slot, wall ms between device synchronisations, alternating",
                          "hmr_gpu_enc_load_source_ms": spread(host_ms), "hmr_gpu_enc_load_sources_device_ms": spread(device_ms),
                          "ratio_of_medians": round(statistics.median(host_ms) / statistics.median(device_ms), 1)}

    kr = result["kernel_rate"]
    result["streaming_step"] = streaming_step(torch, lib, encs, a.steps, lambda slot, f: load_device(lib, encs, slot, pics[f]), kr["i420"]["median_us"] / 1e3 if "i420" in kr else None,
                                              f"every window encodes the clips' {CLIP_FRAMES} pictures in turn, starting at the first")
    for name, path in (("this_build", a.bench_this), ("parent", a.bench_parent)):
        for b in pb.bench_lines(path)[-1:]:
            result.setdefault("bench", {})[name] = b
    pb.close(lib, made)
    pb.write_result(result, a.out)


if __name__ == "__main__":
    main()
