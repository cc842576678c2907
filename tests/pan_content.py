"""Seeded, integer-only test content with a global pan: a textured canvas and a w x h crop of it that moves by (vx, vy) samples per picture.

Canvas = clip(16 + sum over cells of 32, 8 and 2 samples of fmix32(cell index hash) & (127, 63, 15), 16, 235): structure at every scale, so a block matches
its true position and nothing else.  Picture t = the crop at (x0 + t * vx, y0 + t * vy) plus per-sample noise (fmix32(..) & 7) - 3 that changes every
picture (so no block terminates the search early and none matches exactly).  The block at p of picture t lies at p + (vx, vy) in picture t - 1.  Chroma
likewise at half size, from canvases of their own.  kind "flat": every picture the same constant picture (every block terminates early)."""
import numpy as np

SEED = 0x5EED0101


def fmix(h):
    h = h.astype(np.uint32)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16); h *= np.uint32(0x85EBCA6B); h ^= h >> np.uint32(13); h *= np.uint32(0xC2B2AE35); h ^= h >> np.uint32(16)
    return h


def canvas(H, W, seed, y0=0, x0=0):
    """the H x W region of the (unbounded) canvas whose top-left sample is (x0, y0)"""
    ys, xs = np.mgrid[y0:y0 + H, x0:x0 + W].astype(np.uint32)
    v = np.zeros((H, W), np.int64)
    with np.errstate(over="ignore"):
        for cell, amp in ((32, 127), (8, 63), (2, 15)):
            idx = (ys // cell) * np.uint32(40503) + (xs // cell) * np.uint32(0x9E3779B1) + np.uint32((seed + cell) & 0xFFFFFFFF)
            v += (fmix(idx) & np.uint32(amp)).astype(np.int64)
    return np.clip(16 + v, 16, 235).astype(np.uint8)


def pan_frame(cv, w, h, t, vx, vy, x0, y0, seed):
    x, y = x0 + t * vx, y0 + t * vy
    assert 0 <= x and x + w <= cv.shape[1] and 0 <= y and y + h <= cv.shape[0], "the crop leaves the canvas"
    f = cv[y:y + h, x:x + w].astype(np.int64)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.uint32)
    with np.errstate(over="ignore"):
        n = (fmix((ys * np.uint32(w) + xs) * np.uint32(0x85EBCA77) ^ np.uint32((seed + 977 * t) & 0xFFFFFFFF)) & np.uint32(7)).astype(np.int64) - 3
    return np.clip(f + n, 0, 255).astype(np.uint8)


def _origin(n, vx, vy):
    """canvas position of picture 0's crop: max(210, |vx|) * n, max(160, |vy|) * n -- every picture's crop has non-negative coordinates"""
    return max(210, abs(vx)) * n, max(160, abs(vy)) * n


def _region(size, n, v, o):
    """(first, length) of the canvas span the n crops of `size` samples starting at o + t * v cover"""
    lo = min(o, o + (n - 1) * v)
    return lo, max(o, o + (n - 1) * v) + size - lo


def luma_frames(w, h, n, vx, vy, seed=SEED):
    """n luma pictures (h, w) of the pan (vx, vy)"""
    mx, my = _origin(n, vx, vy)
    (cx, cw), (cy, ch) = _region(w, n, vx, mx), _region(h, n, vy, my)
    cv = canvas(ch, cw, seed, cy, cx)
    return [pan_frame(cv, w, h, t, vx, vy, mx - cx, my - cy, seed) for t in range(n)]


def clip(w, h, n, vx, vy, seed=SEED):
    """n I420 pictures (flat uint8 arrays of w * h * 3 / 2) of the pan (vx, vy); chroma moves by (vx, vy) / 2, rounded down per picture position"""
    ys = luma_frames(w, h, n, vx, vy, seed)
    mx, my = _origin(n, vx, vy)
    (cx, cw), (cy, ch) = _region(w, n, vx, mx), _region(h, n, vy, my)
    out = []
    planes = []
    for c in (1, 2):
        cv = canvas(ch // 2 + 2, cw // 2 + 2, seed + 0x1000 * c, cy >> 1, cx >> 1)
        planes.append([pan_frame(cv, w // 2, h // 2, 0, 0, 0, ((mx + t * vx) >> 1) - (cx >> 1), ((my + t * vy) >> 1) - (cy >> 1), seed + 0x1000 * c + 31 * t) for t in range(n)])
    for t in range(n):
        out.append(np.concatenate([ys[t].ravel(), planes[0][t].ravel(), planes[1][t].ravel()]))
    return out


def flat_clip(w, h, n, value=120):
    return [np.full(w * h * 3 // 2, value, np.uint8) for _ in range(n)]


def interior(w, h, vx, vy):
    """[by, bx] mask of the 32x32 blocks whose block displaced by the pan lies inside the reference picture"""
    ys, xs = np.mgrid[0:h // 32, 0:w // 32]
    return (xs * 32 + vx >= 0) & (xs * 32 + 32 + vx <= w) & (ys * 32 + vy >= 0) & (ys * 32 + 32 + vy <= h)
