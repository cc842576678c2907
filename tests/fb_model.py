""""uvgx loss feedback v1" (kvazaar.h loss_feedback): the statement of record, in numpy and plain loops.  The device arithmetic (the fb_*
functions of kvazzup_amd/csrc/hevc_core.h, fb_kernels.hip) is held to this file by tests/test_loss_feedback_host.py and tests/test_gpu_loss_feedback.py.

A CELL is an 8x8 luma block of the coded picture (cw x ch, multiples of 64), a map one uint8 per cell in a (ch / 8, cw / 8) grid: non-zero where a decoder's
picture may differ from the encoder's reconstruction.  A picture's RECORD is (mv, intra, log2): per cell its final vector in quarter samples (x, y), whether the
cell lies in an intra unit, and the log2 of its unit's size -- the encoder's cu_mv / cu_intra / cu_log2 arrays as they are.  filt: deblocking or SAO is on."""
import numpy as np


def dilate(s):
    """a cell or one of its eight neighbours is set"""
    gh, gw = s.shape
    p = np.zeros((gh + 2, gw + 2), dtype=bool)
    p[1:-1, 1:-1] = s != 0
    out = np.zeros((gh, gw), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + gh, dx:dx + gw]
    return out.astype(np.uint8)


def seed(cw, ch, reports, filt):
    """D_n: the cells of the reported coding tree blocks [(first, count)] -- 64x64 blocks in raster order, count <= 0 the whole picture --, each report dilated
    by one cell when a loop filter is on"""
    gh, gw = ch // 8, cw // 8
    ctb = (np.arange(gh)[:, None] // 8) * (cw // 64) + np.arange(gw)[None, :] // 8
    d = np.zeros((gh, gw), dtype=np.uint8)
    for first, count in reports:
        s = np.ones((gh, gw), dtype=np.uint8) if count <= 0 else ((ctb >= first) & (ctb < first + count)).astype(np.uint8)
        d |= dilate(s) if filt else s
    return d


def _any(m, x0, y0, x1, y1):
    """a cell of m set inside the sample rectangle [x0, x1] x [y0, y1] (inclusive)"""
    return bool(m[y0 >> 3:(y1 >> 3) + 1, x0 >> 3:(x1 >> 3) + 1].any())


def inter_reads(prev, cw, ch, cx, cy, mx, my):
    """does the inter cell (cx, cy) with the vector (mx, my) read a cell of prev: the cell moved by (mx >> 2, my >> 2), widened by 4 samples on both sides in
    x when mx is not a multiple of 8 and likewise in y, the coordinates clamped to the picture"""
    ix, iy = int(mx) >> 2, int(my) >> 2
    wx, wy = (4 if int(mx) & 7 else 0), (4 if int(my) & 7 else 0)
    cl = lambda v, hi: min(max(v, 0), hi)
    return _any(prev, cl(cx * 8 + ix - wx, cw - 1), cl(cy * 8 + iy - wy, ch - 1), cl(cx * 8 + 7 + ix + wx, cw - 1), cl(cy * 8 + 7 + iy + wy, ch - 1))


def intra_reads(s, cw, ch, cx, cy, l2):
    """does the intra unit the cell lies in have a reference sample in a cell of s: above-left, above and above-right up to 2 nb, left and below-left up to 2 nb;
    what lies outside the picture is left out (it is substituted from the others)"""
    nb = 1 << int(l2)
    x, y = (cx * 8) & ~(nb - 1), (cy * 8) & ~(nb - 1)
    if y > 0 and _any(s, max(x - 1, 0), y - 1, min(x + 2 * nb - 1, cw - 1), y - 1):
        return True
    return x > 0 and _any(s, x - 1, max(y - 1, 0), x - 1, min(y + 2 * nb - 1, ch - 1))


def step(prev, record, cw, ch, filt, clean=False):
    """D_(k-1) -> D_k through picture k's record; clean: picture k is an IDR picture"""
    gh, gw = ch // 8, cw // 8
    s = np.zeros((gh, gw), dtype=np.uint8)
    if clean:
        return s
    mv, intra, log2 = record
    if prev.any():
        for cy in range(gh):
            for cx in range(gw):
                if not intra[cy, cx] and inter_reads(prev, cw, ch, cx, cy, mv[cy, cx, 0], mv[cy, cx, 1]):
                    s[cy, cx] = 1
    cells = [(int(cy), int(cx)) for cy, cx in np.argwhere(np.asarray(intra) != 0)]
    changed = bool(s.any())
    while changed:                                     # intra units feed intra units: to the fixed point
        changed = False
        for cy, cx in cells:
            if not s[cy, cx] and intra_reads(s, cw, ch, cx, cy, log2[cy, cx]):
                s[cy, cx] = 1
                changed = True
    return dilate(s) if filt else s


def heal_map(cw, ch, records, reports, t, H, filt):
    """D' = D_(t-1) of the heal picture with POC t: reports = [(poc, first, count)], records = {poc: record} of the P pictures since the oldest reported one.  A
    report further back than H pictures: everything is damaged"""
    gh, gw = ch // 8, cw // 8
    oldest = min(r[0] for r in reports)
    if t - oldest > H:
        return np.ones((gh, gw), dtype=np.uint8)
    d = np.zeros((gh, gw), dtype=np.uint8)
    for k in range(oldest, t):
        if k > oldest:
            d = step(d, records[k], cw, ch, filt)
        d |= seed(cw, ch, [(f, c) for n, f, c in reports if n == k], filt)
    return d


ZERO_ONLY = 0xff


def quarter(d, qx, qy):
    """(forced, dist) of the 16x16 quarter (qx, qy): forced -- a cell of d lies inside it; dist -- the Chebyshev distance in samples from the quarter to the nearest
    cell of d outside it (None: no cell)"""
    if d[2 * qy:2 * qy + 2, 2 * qx:2 * qx + 2].any():
        return True, 0
    ys, xs = np.nonzero(d)
    if not len(ys):
        return False, None
    x0, y0 = 16 * qx, 16 * qy
    dx = np.maximum(np.maximum(x0 - (8 * xs + 8), 8 * xs - (x0 + 16)), 0)
    dy = np.maximum(np.maximum(y0 - (8 * ys + 8), 8 * ys - (y0 + 16)), 0)
    return False, int(np.maximum(dx, dy).min())


def block_records(d, cw, ch, me_range):
    """per 32x32 block (forced-quarter nibble, reach): bit k of the nibble -- quarter k (raster of 2 x 2) is forced intra; the reach in full samples is the
    least over the block's free quarters of min(me_range, dist - 4) for dist >= 8, and ZERO_ONLY where a free quarter has dist 0 or no quarter is free"""
    out = np.zeros((ch // 32, cw // 32, 2), dtype=np.uint8)
    for by in range(ch // 32):
        for bx in range(cw // 32):
            forced, reach, zero = 0, me_range, False
            for k in range(4):
                f, dist = quarter(d, 2 * bx + (k & 1), 2 * by + (k >> 1))
                if f:
                    forced |= 1 << k
                elif dist is not None and dist < 8:
                    zero = True
                elif dist is not None:
                    reach = min(reach, dist - 4)
            out[by, bx] = (forced, ZERO_ONLY if zero or forced == 15 else reach)
    return out


def reach_of(code):
    return 0 if code == ZERO_ONLY else int(code)


def vector_within(mv, code):
    """the quarter-sample vector keeps the block's reach"""
    r = 4 * reach_of(code)
    return abs(int(mv[0])) <= r and abs(int(mv[1])) <= r
