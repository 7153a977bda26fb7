"""The synthetic clips every encoder test and the benchmark read (tools/gen_yuv.py): the published clip stays what it was, and the content families are
reproducible, cover the sample range they are meant to and have chroma of their own."""
import hashlib

import numpy as np
import pytest

import encoder_cases  # noqa: F401  (tools/ on the path)
import gen_yuv


def test_published_clip_md5(tmp_path):
    """1920x1080 x 8 frames, seed 1234: the md5 the docstring publishes (and bench.py's inputs, as the default content)"""
    assert gen_yuv.write_clip(str(tmp_path / "c.yuv"), 1920, 1080, 8) == "feb867ccc9a69dc281ee193445ab234f"
    assert gen_yuv.write_clip(str(tmp_path / "d.yuv"), 1920, 1080, 8, content="default") == "feb867ccc9a69dc281ee193445ab234f"


@pytest.mark.parametrize("content", [c for c in gen_yuv.CONTENTS if c != "default"])
def test_content_family(content):
    w, h, n = 200, 136, 4
    frames = list(gen_yuv.gen_frames(w, h, n, seed=7, content=content))
    assert len(frames) == n
    for planes in frames:
        assert [p.shape for p in planes] == [(h, w), (h // 2, w // 2), (h // 2, w // 2)] and all(p.dtype == np.uint8 for p in planes)
    digest = [hashlib.md5(b"".join(p.tobytes() for p in f)).hexdigest() for f in frames]
    assert digest == [hashlib.md5(b"".join(p.tobytes() for p in f)).hexdigest() for f in gen_yuv.gen_frames(w, h, n, seed=7, content=content)]     # seeded
    assert digest != [hashlib.md5(b"".join(p.tobytes() for p in f)).hexdigest() for f in gen_yuv.gen_frames(w, h, n, seed=8, content=content)]
    assert len(set(digest)) > 1 or content == "flat"        # (the content changes from frame to frame)
    Y = np.stack([f[0] for f in frames])
    U, V = np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames])
    if content in ("noise", "extremes"):
        assert Y.min() == 0 and Y.max() == 255 and U.min() == 0 and U.max() == 255 and V.min() == 0 and V.max() == 255
    if content == "extremes":
        assert set(np.unique(Y)) == {0, 255} and set(np.unique(U)) == {0, 255}
    if content == "flat":
        assert all(len(np.unique(y)) <= 2 for y in Y)
        assert {int(np.bincount(y.ravel(), minlength=256).argmax()) for y in Y} == {0, 255}      # (the background alternates; the box is a quarter at most)
    if content == "chroma":
        assert U.min() == 0 and U.max() == 255 and V.min() == 0 and V.max() == 255 and int(Y.max()) - int(Y.min()) < 64
    if content == "motion":
        # the pan moves the picture by 20 ... 60 samples per frame: frame 1 is not frame 0 shifted by a small whole-sample vector
        a, b = Y[0].astype(int), Y[1].astype(int)
        best = min(np.abs(a[8:-8, 8:-8] - np.roll(np.roll(b, dy, 0), dx, 1)[8:-8, 8:-8]).mean() for dy in range(-4, 5) for dx in range(-4, 5))
        assert best > 10


def test_unknown_content_is_refused():
    with pytest.raises(ValueError):
        next(gen_yuv.gen_frames(64, 64, 1, content="nonsense"))
