"""numpy restatement of "uvgx coarse-to-fine search v1" (kvazaar.h me-coarse): the statement of record of the two-level integer search.

1. Quarter picture of an input picture: q(x, y) = (sum of the 4x4 luma samples at (4x.., 4y..) of the PADDED source plane + 8) >> 4.
2. Coarse stage, per 32x32 block at (x0, y0) and reference k: the 8x8 block at (x0 / 4, y0 / 4) of the quarter picture of input t against the quarter picture of
   INPUT picture t - 1 - k (whatever me-source says), candidates (dxq, dyq) in [-Rq, Rq]^2, Rq = me-coarse / 4, samples outside the quarter picture clamped to
   its edge; a candidate is admissible when the 32x32 block displaced by (4 dxq, 4 dyq) passes the tile / mv-constraint rules of the fine search;
   cost = 16 * SAD(8x8) + ((lambda_q4 * (mvd_bits(16 dxq) + mvd_bits(16 dyq))) >> 4); the first minimum in raster order of (dyq, dxq) wins;
   centre c_k = (4 dxq, 4 dyq).
3. Fine stage (k_me): reference k's candidates are the zero window [-R, R]^2 and, iff |c_k.x| > R - 4 or |c_k.y| > R - 4, the window c_k + [-R, R]^2.  Cost as in
   tests/lp_refs_model.py -- SAD per quarter and per block, mvd_bits of the WHOLE vector, ref_bins(k) --, admissibility on the whole vector.  Order: lower
   cost, lower reference, zero window before centred window, lower index inside the window.  Early termination, split rule: unchanged; a block that
   terminates early uses no centre.
With me_coarse = 0 this is lp_refs_model.search (tests/test_me_coarse_model.py pins that)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from lp_refs_model import LAMBDA_Q4, SPLIT_BITS, mvd_bits, ref_bins, _tile_bounds


def quarter(p):
    p = np.asarray(p, dtype=np.int32)
    h, w = p.shape
    return ((p.reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3)) + 8) >> 4).astype(np.uint8)


def _ok_axis(v, p0, lo, hi, size, mv_frame):
    """the fine search's rule for one axis of a full-sample displacement v of the 32-sample block at p0 (tile [lo, hi), picture [0, size))"""
    m = 4 if v & 1 else 0
    if (lo > 0 and p0 + v - m < lo) or (hi < size and p0 + v + 32 + m > hi):
        return False
    if mv_frame:
        mm = 4 if (mv_frame == 2 and (v & 1)) else 0
        if p0 + v - mm < 0 or p0 + v + 32 + mm > size:
            return False
    return True


def _block_tiles(ch, cw, tile_rows, tile_cols, x0, y0):
    return _tile_bounds(0, ch // 64, tile_rows, y0 // 64), _tile_bounds(0, cw // 64, tile_cols, x0 // 64)


def coarse(src_in, ref_in, qp, me_coarse, tile_rows=1, tile_cols=1, mv_frame=0):
    """centres [by, bx, 2] (x, y; full samples, multiples of 4) and their costs [by, bx] of one reference; src_in, ref_in: padded input luma planes (ch, cw)"""
    lam = LAMBDA_Q4[qp]
    Rq = me_coarse // 4
    ch, cw = np.asarray(src_in).shape
    cq, rq = quarter(src_in).astype(np.int32), quarter(ref_in).astype(np.int32)
    hq, wq = cq.shape
    nby, nbx = ch // 32, cw // 32
    pad = np.pad(rq, Rq, mode="edge")
    d = np.arange(-Rq, Rq + 1)
    okx = np.zeros((nbx, len(d)), bool); oky = np.zeros((nby, len(d)), bool)
    for bx in range(nbx):
        lo, hi = _tile_bounds(0, cw // 64, tile_cols, bx * 32 // 64)
        okx[bx] = [_ok_axis(4 * int(v), bx * 32, lo, hi, cw, mv_frame) for v in d]
    for by in range(nby):
        lo, hi = _tile_bounds(0, ch // 64, tile_rows, by * 32 // 64)
        oky[by] = [_ok_axis(4 * int(v), by * 32, lo, hi, ch, mv_frame) for v in d]
    mb = np.array([mvd_bits(16 * int(v)) for v in d])
    best = np.full((nby, nbx), np.iinfo(np.int64).max, np.int64); c = np.zeros((nby, nbx, 2), np.int32)
    for iy, dy in enumerate(d):
        for ix, dx in enumerate(d):
            s = 16 * np.abs(cq - pad[Rq + dy:Rq + dy + hq, Rq + dx:Rq + dx + wq]).reshape(nby, 8, nbx, 8).sum(axis=(1, 3)).astype(np.int64) + ((lam * int(mb[ix] + mb[iy])) >> 4)
            m = (s < best) & oky[:, iy][:, None] & okx[:, ix][None, :]
            best[m] = s[m]; c[m] = (4 * dx, 4 * dy)
    return c, best


def second_window(c, R):
    return abs(int(c[0])) > R - 4 or abs(int(c[1])) > R - 4


def search(src, refs, qp, me_range, tile_rows=1, tile_cols=1, mv_frame=0, me_early=1, me_coarse=0, src_in=None, refs_in=None, detail=None):
    """src: (ch, cw) luma the fine search codes; refs: the n planes it searches (reconstructions, or with me-source input pictures); src_in / refs_in: the
    padded INPUT luma planes of the picture and of its references (the coarse stage; src_in defaults to src).  Returns log2, mv, ref per 8x8 block and the centres
    [n, by, bx, 2]; detail (a dict) receives "early" [by, bx], "cost" [by, bx, 5] (the quarters' and the block's chosen cost), "cost_zero" (the same, zero
    windows only) and "second" [n, by, bx]."""
    src = np.asarray(src, dtype=np.int32)
    ch, cw = src.shape
    n = len(refs)
    R, W = me_range, 2 * me_range + 1
    lam = LAMBDA_Q4[qp]
    nby, nbx = ch // 32, cw // 32
    centres = np.zeros((n, nby, nbx, 2), np.int32)
    if me_coarse:
        for k in range(n):
            centres[k], _ = coarse(src if src_in is None else src_in, refs_in[k], qp, me_coarse, tile_rows, tile_cols, mv_frame)
    P = R + me_coarse + 32
    pads = [np.pad(np.asarray(r, dtype=np.int32), P, mode="edge") for r in refs]
    log2 = np.zeros((ch // 8, cw // 8), np.uint8)
    mv = np.zeros((ch // 8, cw // 8, 2), np.int16)
    rf = np.zeros((ch // 8, cw // 8), np.uint8)
    early = np.zeros((nby, nbx), bool); second = np.zeros((n, nby, nbx), bool)
    cost = np.zeros((nby, nbx, 5), np.int64); cost_zero = np.zeros((nby, nbx, 5), np.int64)
    r0 = np.asarray(refs[0], dtype=np.int32)
    d = np.arange(W) - R
    BIG = np.iinfo(np.int64).max
    for by in range(nby):
        for bx in range(nbx):
            x0, y0 = bx * 32, by * 32
            blk = src[y0:y0 + 32, x0:x0 + 32]
            b8 = (slice(y0 // 8, y0 // 8 + 4), slice(x0 // 8, x0 // 8 + 4))
            if me_early and np.abs(blk - r0[y0:y0 + 32, x0:x0 + 32]).sum() <= 64 * lam:
                log2[b8] = 5
                early[by, bx] = True
                continue
            (ty0, ty1), (tx0, tx1) = _block_tiles(ch, cw, tile_rows, tile_cols, x0, y0)
            best = [None] * 5; best0 = [None] * 5
            for k in range(n):
                wins = [(0, 0)]
                if me_coarse and second_window(centres[k, by, bx], R):
                    wins.append((int(centres[k, by, bx, 0]), int(centres[k, by, bx, 1])))
                    second[k, by, bx] = True
                for wi, (ox, oy) in enumerate(wins):
                    region = pads[k][P + y0 + oy - R:P + y0 + oy + R + 32, P + x0 + ox - R:P + x0 + ox + R + 32]
                    v = sliding_window_view(region, (32, 32))                                  # [dyi, dxi, 32, 32]
                    q = np.abs(v - blk).reshape(W, W, 2, 16, 2, 16).sum(axis=(3, 5)).reshape(W, W, 4).astype(np.int64)
                    oky = np.array([_ok_axis(oy + int(t), y0, ty0, ty1, ch, mv_frame) for t in d])
                    okx = np.array([_ok_axis(ox + int(t), x0, tx0, tx1, cw, mv_frame) for t in d])
                    mby = np.array([mvd_bits(4 * (oy + int(t))) for t in d]); mbx = np.array([mvd_bits(4 * (ox + int(t))) for t in d])
                    rate = (lam * (mby[:, None] + mbx[None, :] + ref_bins(k, n))) >> 4
                    costs = [q[:, :, j] + rate for j in range(4)] + [q.sum(axis=2) + rate]
                    for j in range(5):
                        cc = np.where(oky[:, None] & okx[None, :], costs[j], BIG)
                        flat = int(np.argmin(cc))
                        if cc.flat[flat] == BIG:
                            continue                                                             # (no admissible candidate in this window)
                        key = (int(cc.flat[flat]), k, wi, flat, ox + flat % W - R, oy + flat // W - R)
                        if best[j] is None or key < best[j]:
                            best[j] = key
                        if wi == 0 and (best0[j] is None or key < best0[j]):
                            best0[j] = key
            split = (lam * SPLIT_BITS >> 4) + sum(best[j][0] for j in range(4)) < best[4][0]
            cost[by, bx] = [best[j][0] for j in range(5)]; cost_zero[by, bx] = [best0[j][0] for j in range(5)]
            for qy in range(2):
                for qx in range(2):
                    key = best[qy * 2 + qx] if split else best[4]
                    sl = (slice(y0 // 8 + qy * 2, y0 // 8 + qy * 2 + 2), slice(x0 // 8 + qx * 2, x0 // 8 + qx * 2 + 2))
                    log2[sl] = 4 if split else 5
                    mv[sl] = (key[4] * 4, key[5] * 4)
                    rf[sl] = key[1]
    if detail is not None:
        detail.update(early=early, cost=cost, cost_zero=cost_zero, second=second)
    return log2, mv, rf, centres
