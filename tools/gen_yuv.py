#!/usr/bin/env python3
"""Synthetic planar I420 clip generator.

Sinusoid base + seeded +-12 texture, global pan (3,2) px/frame and a moving
240x160 ramp box, so motion estimation, sub-pel refinement and the intra
fallback all have work to do.  `default_rng(1234)` makes clips reproducible;
the md5 of the 1080p x 8 clip is feb867ccc9a69dc281ee193445ab234f.

That clip ("default") almost never reaches 0 or 255, its chroma is nearly flat and it moves by whole samples.  The other content families
(CONTENTS) are made to be hostile to an encoder, each seeded and in integer arithmetic (numpy only, the same samples on every host):
  noise     iid 0..255 in all planes: large levels, escape binarisation, the most bits per CTU
  extremes  moving hard 0/255 edges and checkerboards, chroma at 0/255: reconstruction clipping, strong deblocking, SAO edge classes
  flat      constant pictures that alternate between 0 and 255, a moving flat box: skip, merge, all-zero CBF, empty SAO classes
  motion    a detailed image resampled at 1/16-sample offsets, panned 20-60 samples per frame: ME window clipping, sub-pel motion, large MVDs,
            vectors into the padding
  chroma    full-range chroma texture with mild luma: chroma TUs with levels, the chroma intra search, chroma deblocking and SAO
"""
import argparse
import hashlib
import sys

import numpy as np


CONTENTS = ("default", "noise", "extremes", "flat", "motion", "chroma")


def _smooth(rng, h, w, cell):
    """0..255 noise on a grid of `cell` samples, bilinearly upsampled to h x w in integer arithmetic"""
    g = rng.integers(0, 256, size=(h // cell + 2, w // cell + 2)).astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    gy, gx, fy, fx = yy // cell, xx // cell, yy % cell, xx % cell
    top = g[gy, gx] * (cell - fx) + g[gy, gx + 1] * fx
    bot = g[gy + 1, gx] * (cell - fx) + g[gy + 1, gx + 1] * fx
    return (top * (cell - fy) + bot * fy + cell * cell // 2) // (cell * cell)


def _sample(tex, oy16, ox16, h, w):
    """h x w window of the periodic texture `tex` at offset (oy16, ox16) in 1/16 samples, bilinear, integer"""
    th, tw = tex.shape
    yy, xx = np.mgrid[0:h, 0:w]
    iy, ix, fy, fx = yy + (oy16 >> 4), xx + (ox16 >> 4), oy16 & 15, ox16 & 15
    a, b = tex[iy % th, ix % tw], tex[iy % th, (ix + 1) % tw]
    c, d = tex[(iy + 1) % th, ix % tw], tex[(iy + 1) % th, (ix + 1) % tw]
    return ((a * (16 - fx) + b * fx) * (16 - fy) + (c * (16 - fx) + d * fx) * fy + 128) >> 8


def _noise(width, height, rng):
    def frame(n):
        return (rng.integers(0, 256, size=(height, width), dtype=np.uint8), rng.integers(0, 256, size=(height // 2, width // 2), dtype=np.uint8),
                rng.integers(0, 256, size=(height // 2, width // 2), dtype=np.uint8))
    return frame


def _extremes(width, height, rng):
    cs, ccs = int(rng.choice([1, 2, 4, 8, 16])), int(rng.choice([1, 2, 4, 8]))       # checkerboard cells: luma, chroma
    vx, vy, ex, ey = (int(v) for v in rng.integers(-9, 10, size=4))                   # board motion, edge motion
    kx, ky = int(rng.integers(1, 4)), int(rng.integers(-3, 4))                          # the slanted edge's direction
    bw, bh = max(8, width // 4), max(8, height // 4)
    bx, by, bdx, bdy = int(rng.integers(0, width)), int(rng.integers(0, height)), int(rng.integers(-13, 14)), int(rng.integers(-9, 10))
    yy, xx = np.mgrid[0:height, 0:width]
    cy, cx = yy[::2, ::2] // 2, xx[::2, ::2] // 2

    def frame(n):
        board = (((xx + vx * n) // cs + (yy + vy * n) // cs) & 1) * 255
        stripes = (((yy + ey * n) // 8) & 1) * 255
        side = kx * (xx - width // 2 - ex * n) + ky * (yy - height // 2) > 0
        Y = np.where(side, board, stripes)
        x0, y0 = (bx + bdx * n) % (width + bw) - bw, (by + bdy * n) % (height + bh) - bh
        inb = (xx >= x0) & (xx < x0 + bw) & (yy >= y0) & (yy < y0 + bh)
        Y = np.where(inb, ((xx + yy) & 1) * 255, Y)
        U = (((cx - vy * n) // ccs + (cy + vx * n) // ccs) & 1) * 255
        V = np.where(kx * (cx - width // 4 + ex * n) - ky * (cy - height // 4) > 0, 255, 0)
        V = np.where(inb[::2, ::2], 255 - V, V)
        return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)
    return frame


def _flat(width, height, rng):
    period = int(rng.integers(1, 3))               # frames per level: 1 alternates every frame, 2 gives pictures identical to the one before
    first = int(rng.integers(0, 2)) * 255
    bw, bh = int(rng.integers(16, max(17, width // 2))), int(rng.integers(16, max(17, height // 2)))
    bx, by, bdx, bdy = int(rng.integers(0, width)), int(rng.integers(0, height)), int(rng.integers(-16, 17)), int(rng.integers(-12, 13))
    bv, bu, bvv = (int(v) for v in rng.integers(0, 256, size=3))
    yy, xx = np.mgrid[0:height, 0:width]

    def frame(n):
        lvl = first if (n // period) % 2 == 0 else 255 - first
        x0, y0 = (bx + bdx * n) % (width + bw) - bw, (by + bdy * n) % (height + bh) - bh
        inb = (xx >= x0) & (xx < x0 + bw) & (yy >= y0) & (yy < y0 + bh)
        cin = inb[::2, ::2]
        return (np.where(inb, bv, lvl).astype(np.uint8), np.where(cin, bu, 255 - lvl).astype(np.uint8), np.where(cin, bvv, lvl).astype(np.uint8))
    return frame


def _motion(width, height, rng):
    th, tw = height + 96 + int(rng.integers(0, 64)), width + 96 + int(rng.integers(0, 64))      # the texture's period: larger than the picture
    tex = (3 * _smooth(rng, th, tw, 16) + 2 * _smooth(rng, th, tw, 4) + rng.integers(0, 256, size=(th, tw))) // 6
    for _ in range(12):                              # hard-edged patches inside the texture
        h0, w0 = int(rng.integers(4, th // 3)), int(rng.integers(4, tw // 3))
        y0, x0 = int(rng.integers(0, th - h0)), int(rng.integers(0, tw - w0))
        tex[y0:y0 + h0, x0:x0 + w0] = int(rng.integers(0, 256))
    ctex = [_smooth(rng, th // 2 + 1, tw // 2 + 1, 8) // 2 + 64 for _ in range(2)]
    # pans of 20 ... 60 samples per frame in 1/16 samples (even: the chroma offset is exactly half of it), either sign
    v = [int(rng.integers(20 * 8, 60 * 8 + 1)) * 2 * (1 if rng.integers(0, 2) else -1) for _ in range(2)]
    o = [int(rng.integers(0, 16 * 64)) for _ in range(2)]
    # an object with its own (fast) motion that leaves the picture on one side and comes back on the other
    obw, obh = max(16, width // 5), max(16, height // 4)
    obj = _sample(tex, 16 * int(rng.integers(0, th)), 16 * int(rng.integers(0, tw)), obh, obw)[::-1, ::-1]
    ox, oy, odx, ody = int(rng.integers(0, width)), int(rng.integers(0, height)), int(rng.integers(-64, 65)), int(rng.integers(-40, 41))
    yy, xx = np.mgrid[0:height, 0:width]

    def frame(n):
        oy16, ox16 = o[0] + v[0] * n, o[1] + v[1] * n
        Y = _sample(tex, oy16, ox16, height, width)
        U = _sample(ctex[0], oy16 // 2, ox16 // 2, height // 2, width // 2)
        V = _sample(ctex[1], oy16 // 2, ox16 // 2, height // 2, width // 2)
        x0, y0 = (ox + odx * n) % (width + obw) - obw, (oy + ody * n) % (height + obh) - obh
        inb = (xx >= x0) & (xx < x0 + obw) & (yy >= y0) & (yy < y0 + obh)
        Y = np.where(inb, obj[np.clip(yy - y0, 0, obh - 1), np.clip(xx - x0, 0, obw - 1)], Y)
        return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)
    return frame


def _chroma(width, height, rng):
    ch, cw = height // 2, width // 2
    cu = np.clip((3 * _smooth(rng, ch + 64, cw + 64, 8) + rng.integers(0, 256, size=(ch + 64, cw + 64))) // 2 - 128, 0, 255)
    cv = _smooth(rng, ch + 64, cw + 64, 4)
    cv = np.where(((np.arange(ch + 64)[:, None] // 8 + np.arange(cw + 64)[None, :] // 8) & 1) == 1, 255 - cv, cv)     # hard 8 x 8 edges in V
    lum = 120 + (_smooth(rng, height + 64, width + 64, 16) - 128) // 12 + rng.integers(-3, 4, size=(height + 64, width + 64))
    vx, vy = int(rng.integers(-3, 4)), int(rng.integers(-2, 3))

    def frame(n):
        tx, ty = (vx * n) % 64, (vy * n) % 64
        cx, cy = (vx * n // 2) % 64, (vy * n // 2) % 64
        return (lum[ty:ty + height, tx:tx + width].astype(np.uint8), cu[cy:cy + ch, cx:cx + cw].astype(np.uint8), cv[cy:cy + ch, (64 - cx) % 64:(64 - cx) % 64 + cw].astype(np.uint8))
    return frame


_FAMILIES = {"noise": _noise, "extremes": _extremes, "flat": _flat, "motion": _motion, "chroma": _chroma}


def gen_frames(width, height, frames, seed=1234, cut_at=None, content="default"):
    """Yield (Y, U, V) uint8 planes for `frames` frames.  cut_at = n: from frame n on the content is a different scene (new texture, mirrored and
    re-scaled base) - what the encoder's scene-change detection reacts to; None (the published clips) = no cut.  content: one of CONTENTS (a family other
    than "default" cuts to a second clip of the same family, drawn from seed + 1)."""
    if content != "default":
        if content not in _FAMILIES:
            raise ValueError(f"unknown content {content!r}: one of {CONTENTS}")
        scenes = [_FAMILIES[content](width, height, np.random.default_rng([seed, CONTENTS.index(content)]))]
        if cut_at is not None:
            scenes.append(_FAMILIES[content](width, height, np.random.default_rng([seed + 1, CONTENTS.index(content)])))
        for n in range(frames):
            yield scenes[1 if cut_at is not None and n >= cut_at else 0](n)
        return
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    # seed 1234 is the published clip; any other seed is a different clip of the same kind: its own texture, pan, base pattern and box path (bench.py encodes
    # several of them side by side so that the sequences of a batch do not all walk the same decisions)
    pan_x, pan_y, f1, f2, f3, box_x, box_y, box_dx, box_dy = 3, 2, 53.0, 41.0, 17.0, 200, 300, 11, 7
    if seed != 1234:
        prm = np.random.default_rng(seed ^ 0x5EED)
        pan_x, pan_y = int(prm.integers(1, 6)), int(prm.integers(0, 4))
        f1, f2, f3 = 53.0 * float(prm.uniform(0.6, 1.5)), 41.0 * float(prm.uniform(0.6, 1.5)), 17.0 * float(prm.uniform(0.7, 1.6))
        box_x, box_y = int(prm.integers(0, max(width - 240, 1))), int(prm.integers(0, max(height - 160, 1)))
        box_dx, box_dy = int(prm.integers(-9, 13)), int(prm.integers(-5, 9))
    base = (128 + 60 * np.sin(xx / f1) * np.cos(yy / f2) + 40 * np.sin((xx + yy) / f3)).astype(np.float32)
    tex = rng.integers(-12, 13, size=(height + 64, width + 64)).astype(np.float32)
    base2 = tex2 = None
    if cut_at is not None:
        base2 = (120 + 70 * np.cos(xx[:, ::-1] / 23.0) * np.sin(yy / 19.0) + 30 * np.sin((2 * xx - yy) / 11.0)).astype(np.float32)
        tex2 = np.random.default_rng(seed + 1).integers(-40, 41, size=(height + 64, width + 64)).astype(np.float32)
    for n in range(frames):
        dx, dy = pan_x * n, pan_y * n
        if cut_at is not None and n >= cut_at:
            base, tex = base2, tex2
        tx, ty = dx % 64, dy % 64      # the texture window wraps after 21 frames (identical to the published definition before that)
        Y = np.roll(np.roll(base, dx, axis=1), dy, axis=0) + tex[ty:ty + height, tx:tx + width]
        bx, by = box_x + box_dx * n, box_y + box_dy * n
        if 0 <= by < height and 0 <= bx < width:
            bh, bw = min(160, height - by), min(240, width - bx)
            Y[by:by + bh, bx:bx + bw] = (200 - 0.2 * np.arange(240))[None, :bw]
        Y = np.clip(Y, 0, 255).astype(np.uint8)
        # chroma is sampled on the even luma grid (x2 = 0, 2, 4, ...)
        U = np.clip(128 + 30 * np.sin((xx[::2, ::2] + dx) / 97.0), 0, 255).astype(np.uint8)
        V = np.clip(128 + 30 * np.cos((yy[::2, ::2] + dy) / 89.0), 0, 255).astype(np.uint8)
        yield Y, U, V


def write_clip(path, width, height, frames, seed=1234, cut_at=None, content="default"):
    md5 = hashlib.md5()
    with open(path, "wb") as f:
        for planes in gen_frames(width, height, frames, seed, cut_at, content):
            for p in planes:
                b = p.tobytes()
                md5.update(b)
                f.write(b)
    return md5.hexdigest()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("out")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--content", choices=CONTENTS, default="default")
    a = ap.parse_args(argv)
    print(write_clip(a.out, a.width, a.height, a.frames, a.seed, content=a.content))


if __name__ == "__main__":
    sys.exit(main())
