"""numpy restatement of the integer motion search of "uvgx multi-reference v1" (lp-refs) -- k_me over n references.

Per 32x32 block of the coded picture:
  * me-early-termination: SAD of the block against the co-located block of reference 0 <= 64 * lambda_q4 -> one 32x32 unit, zero vector, reference 0;
  * else every reference k < n and every integer displacement (dx, dy) in [-R, R]^2 that keeps the block (plus 4 rows / columns on an odd
    displacement) inside its tile -- and, with mv-constraint, inside the picture (margin only with frametilemargin) -- is a candidate with
    cost = SAD + ((lambda_q4 * (mvd_bits(4 dx) + mvd_bits(4 dy) + ref_bins(k, n))) >> 4), SAD over each 16x16 quarter and over the whole block,
    reference samples outside the picture clamped to its edge;
  * each quarter and the whole block take the minimum of (cost, k, (dy + R) * W + dx + R); the block splits into four 16x16 units when
    (lambda_q4 * 8 >> 4) + the quarters' costs < the whole block's cost.
With n = 1 this is the single-reference search of oracle/hevc_enc.c me_block32() (subme 0, intra-in-P off): tests/test_lp_refs_host.py pins it there.
Returns per 8x8 block: log2 (uint8), mv (int16 x 2, quarter samples), ref (uint8)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_BITS = 8


def _lambda_table():
    text = open(os.path.join(ROOT, "kvazzup_amd", "csrc", "hevc_tables.h")).read()
    body = re.search(r"kLambdaQ4\[52\]\s*=\s*\{([^}]*)\}", text).group(1)
    return [int(v) for v in body.replace("\n", " ").split(",") if v.strip()]


LAMBDA_Q4 = _lambda_table()


def mvd_bits(q):
    a = abs(int(q))
    if a == 0:
        return 1
    if a == 1:
        return 3
    x, k, ln = a - 2, 1, 0
    while x >= (1 << k):
        x -= 1 << k
        k += 1
        ln += 1
    return 2 + ln + 1 + k + 1


def ref_bins(k, n):
    if n <= 1:
        return 0
    return k + 1 if k < n - 1 else n - 1


def _tile_bounds(first, n_ctb, parts, idx_ctb):
    """[start, end) in samples of the uniform tile (6.5.1) holding CTB idx_ctb, with `parts` tiles over n_ctb CTBs"""
    if parts <= 1:
        return 0, n_ctb * 64
    starts = [(i * n_ctb) // parts for i in range(parts + 1)]
    for i in range(parts):
        if starts[i] <= idx_ctb < starts[i + 1]:
            return starts[i] * 64, starts[i + 1] * 64
    raise AssertionError


def search(src, refs, qp, me_range, tile_rows=1, tile_cols=1, mv_frame=0, me_early=1):
    """src: (ch, cw) uint8 luma of the picture (coded size, a multiple of 64); refs: list of n (ch, cw) uint8 planes searched for references 0 .. n - 1."""
    src = np.asarray(src, dtype=np.int32)
    ch, cw = src.shape
    n = len(refs)
    R, W = me_range, 2 * me_range + 1
    lam = LAMBDA_Q4[qp]
    nby, nbx = ch // 32, cw // 32
    # quarter SADs of every block for every candidate and reference: [k, dyi, dxi, by, bx, quarter]
    sads = np.zeros((n, W, W, nby, nbx, 4), dtype=np.int64)
    for k, ref in enumerate(refs):
        pad = np.pad(np.asarray(ref, dtype=np.int32), R, mode="edge")
        for dyi in range(W):
            for dxi in range(W):
                shifted = pad[dyi:dyi + ch, dxi:dxi + cw]
                d = np.abs(src - shifted).reshape(nby, 2, 16, nbx, 2, 16).sum(axis=(2, 5))      # [by, qy, bx, qx]
                sads[k, dyi, dxi] = d.transpose(0, 2, 1, 3).reshape(nby, nbx, 4)
    # rate and admissibility per (k, candidate), per block (the tile bounds depend on the block)
    d = np.arange(W) - R
    mb = np.array([mvd_bits(4 * v) for v in d])
    log2 = np.zeros((ch // 8, cw // 8), np.uint8)
    mv = np.zeros((ch // 8, cw // 8, 2), np.int16)
    rf = np.zeros((ch // 8, cw // 8), np.uint8)
    r0 = np.asarray(refs[0], dtype=np.int32)
    for by in range(nby):
        for bx in range(nbx):
            x0, y0 = bx * 32, by * 32
            b8 = (slice(y0 // 8, y0 // 8 + 4), slice(x0 // 8, x0 // 8 + 4))
            if me_early and np.abs(src[y0:y0 + 32, x0:x0 + 32] - r0[y0:y0 + 32, x0:x0 + 32]).sum() <= 64 * lam:
                log2[b8] = 5
                continue
            ty0, ty1 = _tile_bounds(0, ch // 64, tile_rows, y0 // 64)
            tx0, tx1 = _tile_bounds(0, cw // 64, tile_cols, x0 // 64)

            def ok_axis(v, p0, lo, hi, size):
                m = 4 if v & 1 else 0
                if (lo > 0 and p0 + v - m < lo) or (hi < size and p0 + v + 32 + m > hi):
                    return False
                if mv_frame:
                    mm = 4 if (mv_frame == 2 and (v & 1)) else 0
                    if p0 + v - mm < 0 or p0 + v + 32 + mm > size:
                        return False
                return True
            oky = np.array([ok_axis(v, y0, ty0, ty1, ch) for v in d])
            okx = np.array([ok_axis(v, x0, tx0, tx1, cw) for v in d])
            best = [None] * 5
            for k in range(n):
                rate = (lam * (mb[:, None] + mb[None, :] + ref_bins(k, n))) >> 4      # [dyi, dxi]
                q = sads[k, :, :, by, bx, :]                                            # [dyi, dxi, 4]
                costs = [q[:, :, j] + rate for j in range(4)] + [q.sum(axis=2) + rate]
                for j in range(5):
                    c = np.where(oky[:, None] & okx[None, :], costs[j], np.iinfo(np.int64).max)
                    flat = int(np.argmin(c))                                            # first minimum: lowest candidate index
                    key = (int(c.flat[flat]), k, flat)
                    if best[j] is None or key < best[j]:
                        best[j] = key
            split = (lam * SPLIT_BITS >> 4) + sum(best[j][0] for j in range(4)) < best[4][0]
            for qy in range(2):
                for qx in range(2):
                    _, k, cand = best[qy * 2 + qx] if split else best[4]
                    sl = (slice(y0 // 8 + qy * 2, y0 // 8 + qy * 2 + 2), slice(x0 // 8 + qx * 2, x0 // 8 + qx * 2 + 2))
                    log2[sl] = 4 if split else 5
                    mv[sl] = ((cand % W - R) * 4, (cand // W - R) * 4)
                    rf[sl] = k
    return log2, mv, rf
