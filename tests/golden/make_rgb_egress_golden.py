#!/usr/bin/env python3
"""Mint the RGB egress fixture from the COMPILED REFERENCE (build container only), like make_quality_golden.py: the reference encodes the synthetic clip
(oracle/_ref/ref_lockstep, or ref_ctudump under HOMER_TURNSTILE for the wpp cases) and writes its reconstruction, whose md5 has to be streams.json's recon_md5; this
script records, per frame, the md5 of each channel of the BT.709 limited-range RGB picture that the numpy restatement of include/homer_gpu.h section 12i
(tests/rgb_egress_cases.py) makes of THE REFERENCE'S OWN reconstruction, and the three sums of squared differences between that picture and
rgb_cases.yuv_to_rgb(the clip's frame).  tests/golden/rgb_egress.json - digests and integers only - is what the device kernel (k_egress_rgb, csrc/picture_io.hip) has to
reproduce."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_stream_golden import CASES, gen_yuv  # noqa: E402
import rgb_cases  # noqa: E402
import rgb_egress_cases  # noqa: E402

RGB_EGRESS_CASES = ["200x136", "416x240_wpp_rows"]


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
    fsz, y, c = width * height * 3 // 2, width * height, (width // 2) * (height // 2)
    md5 = [hashlib.md5(rec[f * fsz:(f + 1) * fsz]).hexdigest() for f in range(frames)]
    assert md5 == recon_md5, "the reference's reconstruction is not the one streams.json was minted from"
    rgb_md5, ssd = [], []
    for f in range(frames):
        rgb = rgb_egress_cases.restate_bytes(rec[f * fsz:(f + 1) * fsz], width, height, "bt709", 0)
        frame = clip[f * fsz:(f + 1) * fsz]
        original = rgb_cases.yuv_to_rgb((frame[:y], frame[y:y + c], frame[y + c:]), width, height)
        rgb_md5.append([hashlib.md5(np.ascontiguousarray(p).tobytes()).hexdigest() for p in rgb])
        ssd.append(rgb_egress_cases.numpy_ssd(original, rgb))
    return {"width": width, "height": height, "frames": frames, "matrix": "bt709", "full_range": 0, "recon_md5": md5, "rgb_md5": rgb_md5, "ssd": ssd}


if __name__ == "__main__":
    streams = json.load(open(os.path.join(HERE, "streams.json")))
    by_name = {name: (w, h, f, keys) for name, w, h, f, keys in CASES}
    out = {name: run(*by_name[name], streams[name]["recon_md5"]) for name in RGB_EGRESS_CASES}
    with open(os.path.join(HERE, "rgb_egress.json"), "w") as fp:
        fp.write("{\n" + ",\n".join(f" {json.dumps(name)}: {json.dumps(v)}" for name, v in out.items()) + "\n}\n")
    for name, v in out.items():
        print(name, v["ssd"][0], v["rgb_md5"][0][0])
