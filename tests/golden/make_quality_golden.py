#!/usr/bin/env python3
"""Mint the quality fixtures from the COMPILED REFERENCE (build container only), like make_stream_golden.py: for each case below the reference encodes the synthetic clip
(oracle/_ref/ref_lockstep, or ref_ctudump under HOMER_TURNSTILE for the wpp / engines cases) and writes its reconstruction; this script records, per frame, the three sums
of squared differences between the clip and THE REFERENCE'S OWN reconstruction (numpy, int64), the three PSNR values by the formula of homer_psnr (hmr_metics.c:66-104, in
Python doubles) and the reconstruction's md5, which has to be streams.json's recon_md5.  tests/golden/quality.json is what hmr_gpu_psnr and the device egress
(csrc/k_egress.hip) have to reproduce."""
import hashlib
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_stream_golden import CASES, gen_yuv  # noqa: E402

QUALITY_CASES = ["200x136", "416x240", "328x264_wpp3", "416x240_wpp_rows", "832x480_wpp_rows", "416x240_scene_cut_wpp_rows", "416x240_cbr400_perf1",
                 "832x480_cbr1500_perf1_wpp_rows", "416x240_eng2", "416x240_eng3_wpp_rows", "416x240_flat", "416x240_flat_qp4", "416x240_extremes_qp4", "416x240_chroma",
                 "384x192_noise_qp0", "1920x1080_cfg2_wpp_rows", "3840x2160_cfg2_wpp32"]
# ... and the sequences of the batch tests (tests/test_gpu_ingest.py BATCH_CASES) that are not among them
QUALITY_CASES += ["416x240_cbr300_nosao_wpp_rows", "416x240_noise_wpp_rows", "416x240_extremes_wpp_rows"]


def psnr_of(ssd, width, height):
    """homer_psnr: 10 * log10(255 * 255 * samples / ssd), 99.99 for a zero sum; the chroma planes have (width / 2) * (height / 2) samples"""
    samples = [width * height, (width // 2) * (height // 2), (width // 2) * (height // 2)]
    return [10.0 * math.log10(float(255 * 255 * n) / float(s)) if s else 99.99 for s, n in zip(ssd, samples)]


def plane_ssd(a, b, width, height):
    """the three sums of squared differences of two I420 pictures given as bytes"""
    a, b = np.frombuffer(a, np.uint8).astype(np.int64), np.frombuffer(b, np.uint8).astype(np.int64)
    d = (a - b) ** 2
    y, c = width * height, (width // 2) * (height // 2)
    return [int(d[:y].sum()), int(d[y:y + c].sum()), int(d[y + c:y + 2 * c].sum())]


def run(width, height, frames, keys, recon_md5):
    keys = dict(keys)
    cut_at, clip_seed, content = keys.pop("cut_at", None), keys.pop("clip_seed", None), keys.pop("content", None)
    with tempfile.TemporaryDirectory() as tmp:
        yuv = os.path.join(tmp, "in.yuv")
        gen_yuv.write_clip(yuv, width, height, frames, seed=clip_seed or 1234, cut_at=cut_at, content=content or "default")
        turnstile = int(keys.get("wpp", 1)) > 1 or int(keys.get("engines", 1)) > 1
        cmd = [os.path.join(ROOT, "oracle", "_ref", "ref_ctudump" if turnstile else "ref_lockstep"), yuv, os.path.join(tmp, "out.265"), str(width), str(height), str(frames),
               "recon=" + os.path.join(tmp, "rec.yuv")] + [f"{k}={v}" for k, v in keys.items()]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL, env=dict(os.environ, HOMER_TURNSTILE="1") if turnstile else None)
        clip = open(yuv, "rb").read()
        rec = open(os.path.join(tmp, "rec.yuv"), "rb").read()
    fsz = width * height * 3 // 2
    md5 = [hashlib.md5(rec[f * fsz:(f + 1) * fsz]).hexdigest() for f in range(frames)]
    assert md5 == recon_md5, "the reference's reconstruction is not the one streams.json was minted from"
    ssd = [plane_ssd(clip[f * fsz:(f + 1) * fsz], rec[f * fsz:(f + 1) * fsz], width, height) for f in range(frames)]
    return {"width": width, "height": height, "frames": frames, "recon_md5": md5, "ssd": ssd, "psnr": [psnr_of(s, width, height) for s in ssd]}


if __name__ == "__main__":
    streams = json.load(open(os.path.join(HERE, "streams.json")))
    by_name = {name: (w, h, f, keys) for name, w, h, f, keys in CASES}
    out = {name: run(*by_name[name], streams[name]["recon_md5"]) for name in QUALITY_CASES}
    with open(os.path.join(HERE, "quality.json"), "w") as fp:
        fp.write("{\n" + ",\n".join(f" {json.dumps(name)}: {json.dumps(v)}" for name, v in out.items()) + "\n}\n")
    for name, v in out.items():
        print(name, v["ssd"][0], [round(p, 2) for p in v["psnr"][0]])
