#!/usr/bin/env python3
"""Mints tests/golden/yuv_ingest.json: per form of tests/yuv_cases.py the sha256 of the I420 picture that the numpy restatement of include/homer_gpu.h section 12k makes
of the form's seeded 64 x 48 picture (yuv_cases.golden_picture).  tests/test_yuv_ingest_cpu.py holds the restatement AND hmr_gpu_yuv_convert_host to these digests, so
the header's arithmetic and its restatement cannot drift together unnoticed.  Run it again only when section 12k itself changes:

    python tests/golden/make_yuv_ingest_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import yuv_cases as yc  # noqa: E402

W, H = 64, 48


def main():
    digests = {}
    for form in yc.NAMES:
        planes = yc.restate(form, *yc.golden_picture(form, W, H))
        digests[form] = hashlib.sha256(b"".join(p.tobytes() for p in planes)).hexdigest()
    with open(os.path.join(HERE, "yuv_ingest.json"), "w") as f:
        json.dump({"width": W, "height": H, "picture": "yuv_cases.golden_picture(form): noise over the container's range, seeded by crc32 of the form's name", "sha256": digests}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
