"""Concealment v3, the statement of record: what stands in for a reference picture that never arrived when the decoder is asked for mode 3
(kvzx_decoder_set_concealment; csrc/decoder.h, csrc/conceal_kernels.hip) -- the source picture concealment v2 would copy, moved block by block along its own
motion, continued to the missing picture's order count.  Plain numpy over pyhevc.Picture's mv / ref_idx / ref_poc / ref_lt, and a pyhevc.Decoder whose
missing_ref applies it: the second decoder the HIP decoder is held to in mode 3 (the checker, oracle/, stays at v2).  Test infrastructure.

The rule, all integer, >> arithmetic; p = order count of the missing picture, S = the source (order count s) v2's rule picks:
 1. block vectors: per 16x16 luma block B of the coded picture the motion of the 4x4 block at B's top-left corner in S, list 0 if that list predicts it, else
    list 1; zero when that block is intra, when the picture the vector points into (order count r) was a long-term reference then, when S is a stand-in (it has
    no motion) or when td = 0; else scaled as 8.5.3.2.12 scales a vector, td = clip3(-128, 127, s - r), tb = clip3(-128, 127, p - s)
 2. neighbour test: B keeps its vector only if at least two of its four edge neighbours inside the grid carry a vector of step 1 within 4 quarter samples of it in
    both components; else zero
 3. fetch, whole samples, clipped to the coded plane: luma by ((vx + 2) >> 2, (vy + 2) >> 2), B's 8x8 chroma by ((vx + 4) >> 3, (vy + 4) >> 3)"""
import numpy as np

import pyhevc


def clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def scale(mv, td, tb):
    """8.5.3.2.12's scaling of one vector component (td != 0)"""
    tx = (16384 + (abs(td) >> 1)) // abs(td) * (1 if td > 0 else -1)       # (the division truncates)
    f = clip3(-4096, 4095, (tb * tx + 32) >> 6)
    q = f * mv
    a = (abs(q) + 127) >> 8
    return clip3(-32768, 32767, a if q >= 0 else -a)


def block_vectors(src, p):
    """step 1: [h16][w16][x, y] in quarter samples"""
    h16, w16 = (src.h + 15) // 16, (src.w + 15) // 16
    v = np.zeros((h16, w16, 2), np.int64)
    tb = clip3(-128, 127, p - src.poc)
    for by in range(h16):
        for bx in range(w16):
            y4, x4 = by * 4, bx * 4
            L = 0 if src.ref_idx[y4, x4, 0] >= 0 else 1
            if src.ref_idx[y4, x4, L] < 0 or src.ref_lt[y4, x4, L]:
                continue
            td = clip3(-128, 127, src.poc - int(src.ref_poc[y4, x4, L]))
            if td == 0:
                continue
            v[by, bx] = [scale(int(src.mv[y4, x4, L, k]), td, tb) for k in (0, 1)]
    return v


def neighbour_test(v):
    """step 2: reads the field of step 1, not its own results"""
    h16, w16 = v.shape[:2]
    out = np.zeros_like(v)
    for by in range(h16):
        for bx in range(w16):
            near = 0
            for ny, nx in ((by, bx - 1), (by, bx + 1), (by - 1, bx), (by + 1, bx)):
                if 0 <= ny < h16 and 0 <= nx < w16 and abs(int(v[ny, nx, 0] - v[by, bx, 0])) <= 4 and abs(int(v[ny, nx, 1] - v[by, bx, 1])) <= 4:
                    near += 1
            if near >= 2:
                out[by, bx] = v[by, bx]
    return out


def displacements(v):
    """whole-sample displacements per block: luma dx, dy, chroma dx, dy (what kvzx_decoder_debug_copy "standin_mv" reads back)"""
    return np.concatenate([(v + 2) >> 2, (v + 4) >> 3], axis=2).astype(np.int16)


def fetch(planes, disp):
    """step 3: the three planes moved by the table"""
    out = []
    for c, src in enumerate(planes):
        n, k = (16, 0) if c == 0 else (8, 2)
        H, W = src.shape
        dst = np.empty_like(src)
        for by in range(disp.shape[0]):
            for bx in range(disp.shape[1]):
                y0, x0 = by * n, bx * n
                y1, x1 = min(y0 + n, H), min(x0 + n, W)
                rows = np.clip(np.arange(y0, y1) + int(disp[by, bx, k + 1]), 0, H - 1)
                cols = np.clip(np.arange(x0, x1) + int(disp[by, bx, k]), 0, W - 1)
                dst[y0:y1, x0:x1] = src[np.ix_(rows, cols)]
        out.append(dst)
    return out


def stand_in(src, p):
    """(planes, displacement table) of the stand-in for order count p made of picture src"""
    disp = displacements(neighbour_test(block_vectors(src, p)))
    return fetch(src.planes, disp), disp


class Decoder(pyhevc.Decoder):
    """tests/pyhevc.py's decoder in concealment mode 3; stand_ins: order count, source's order count (None: grey), planes and table of every stand-in made, in order"""

    def __init__(self, tabs):
        super().__init__(tabs)
        self.stand_ins = []

    def missing_ref(self, sps, poc, is_lt):
        pic = super().missing_ref(sps, poc, is_lt)                 # v2's: the source's copy, or grey; marked, filed, counted
        cands = [p for p in self.pre_refs if not getattr(p, "fresh", False) and p is not pic]
        disp = np.zeros(((sps["h"] + 15) // 16, (sps["w"] + 15) // 16, 4), np.int16)
        src = None
        if cands:
            src = min(cands, key=lambda p: (abs(p.poc - poc), p.poc))        # (v2's choice, unchanged)
            planes, disp = stand_in(src, poc)
            for dst, pl in zip(pic.planes, planes):
                dst[:] = pl
        self.stand_ins.append({"poc": poc, "au": getattr(self, "au", None), "src_poc": None if src is None else src.poc, "src_is_stand_in": src is not None and getattr(src, "stand_in", False),
                               "list1_blocks": 0 if src is None else int(((src.ref_idx[::4, ::4, 0] < 0) & (src.ref_idx[::4, ::4, 1] >= 0)).sum()),
                               "planes": [pl.astype(np.uint8) for pl in pic.planes], "disp": disp})
        pic.stand_in = True
        return pic


def decode(aus, tabs):
    """the access units through the mode-3 decoder: (pictures in output order, the decoder)"""
    d = Decoder(tabs)
    for d.au, au in enumerate(aus):                                # (stand_ins[k]["au"]: the access unit that asked for it)
        for nal in pyhevc.split_nals(au):
            d.decode_nal(nal)
    return d.flush(), d
