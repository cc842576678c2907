"""Content with an occluder over a textured background, for "lp-gop" (DESIGN.md section 9d): what is uncovered again is found in an OLDER picture -- the
key picture -- and in none of the pictures just before.  Built from the checker's synthetic pictures (orc.synth_frame): the background is one of them held
still, the occluder a rectangle cut out of another."""
import numpy as np

import orc

SEED = 0x0CC1DE00


def _planes(fr, w, h):
    return fr[:w * h].reshape(h, w), fr[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), fr[w * h * 5 // 4:].reshape(h // 2, w // 2)


def _paste(bg, fg, w, h, x0, y0, bw, bh):
    out = bg.copy()
    x0, y0 = max(0, min(w - 2, x0)) & ~1, max(0, min(h - 2, y0)) & ~1
    x1, y1 = min(w, x0 + bw) & ~1, min(h, y0 + bh) & ~1
    for po, pf, s in zip(_planes(out, w, h), _planes(fg, w, h), (1, 2, 2)):
        po[y0 // s:y1 // s, x0 // s:x1 // s] = pf[y0 // s:y1 // s, x0 // s:x1 // s]
    return out


def blink_clip(w, h, n, covered=(1, 2, 3, 4), kind=0, seed=SEED):
    """n I420 pictures: a still background, and in the pictures `covered` a rectangle (a quarter of the width, half the height, in the middle) of other
    content over it -- the picture after them shows background that only pictures before them hold"""
    bg, fg = orc.synth_frame(kind, seed, w, h, 0), orc.synth_frame(2 if kind != 2 else 0, seed ^ 0x5A5A, w, h, 7)
    bw, bh = (w // 4 + 31) & ~31, (h // 2 + 31) & ~31
    x0, y0 = ((w - bw) // 2) & ~31, ((h - bh) // 2) & ~31
    return [_paste(bg, fg, w, h, x0, y0, bw, bh) if t in covered else bg.copy() for t in range(n)]


def region(w, h):
    """(y0, y1, x0, x1) of blink_clip's rectangle in luma samples"""
    bw, bh = (w // 4 + 31) & ~31, (h // 2 + 31) & ~31
    x0, y0 = ((w - bw) // 2) & ~31, ((h - bh) // 2) & ~31
    return y0, min(h, y0 + bh), x0, min(w, x0 + bw)


def passing_clip(w, h, n, speed=None, kind=0, seed=SEED):
    """n I420 pictures: a rectangle an eighth of the width wide and two thirds of the height high crosses the still background from left to right and back,
    `speed` samples a picture (default: its own width every three pictures) -- a hand or a head passing in front of a wall"""
    bg, fg = orc.synth_frame(kind, seed, w, h, 0), orc.synth_frame(2 if kind != 2 else 0, seed ^ 0x5A5A, w, h, 7)
    bw, bh = max(32, (w // 8) & ~15), (2 * h // 3) & ~15
    speed = speed or max(2, (bw // 3) & ~1)
    span = max(2, w - bw)
    out = []
    for t in range(n):
        p = (t * speed) % (2 * span)
        out.append(_paste(bg, fg, w, h, p if p < span else 2 * span - p, (h - bh) // 2, bw, bh))
    return out
