#!/usr/bin/env python3
"""Mint the SSIM fixture from the COMPILED REFERENCE (build container only), like make_quality_golden.py and for the same cases: the reference encodes the synthetic clip
(oracle/_ref/ref_lockstep, or ref_ctudump under HOMER_TURNSTILE for the wpp / engines cases) and writes its reconstruction, whose md5 has to be streams.json's
recon_md5; this script records, per frame, the three SSIM sums of include/homer_gpu.h section 12h between the clip and THE REFERENCE'S OWN reconstruction, computed by
the oracle of tests/ssim_cases.py (numpy block sums, the formula per window in Python integers).  tests/golden/ssim.json is what hmr_gpu_ssim_host and the device kernel
(k_ssim, csrc/picture_io.hip) have to reproduce."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from make_quality_golden import QUALITY_CASES  # noqa: E402
from make_stream_golden import CASES, gen_yuv  # noqa: E402
import ssim_cases  # noqa: E402


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
    sums = [ssim_cases.picture_sums(clip[f * fsz:(f + 1) * fsz], rec[f * fsz:(f + 1) * fsz], width, height) for f in range(frames)]
    return {"width": width, "height": height, "frames": frames, "recon_md5": md5, "windows": ssim_cases.picture_windows(width, height), "ssim": sums}


if __name__ == "__main__":
    streams = json.load(open(os.path.join(HERE, "streams.json")))
    by_name = {name: (w, h, f, keys) for name, w, h, f, keys in CASES}
    out = {}
    for name in QUALITY_CASES:
        out[name] = run(*by_name[name], streams[name]["recon_md5"])
        print(name, out[name]["ssim"][0], [round(s / (n << 30), 4) for s, n in zip(out[name]["ssim"][0], out[name]["windows"])], flush=True)
    with open(os.path.join(HERE, "ssim.json"), "w") as fp:
        fp.write("{\n" + ",\n".join(f" {json.dumps(name)}: {json.dumps(v)}" for name, v in out.items()) + "\n}\n")
