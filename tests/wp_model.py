"""Python restatement of "uvgx weighted prediction v1" (kvazaar.h weightp): the luma statistics, the candidate weights, the check,
the sample prediction (steps 1-4) and pred_weight_table() (step 6).  Python integers and numpy throughout; no arithmetic is shared with the product.

A picture here is its visible luma plane, (height, width) uint8.  record() is what the encoder's debug_all()["wp"] holds for a P picture: per reference of
list 0 (flag, w, o), (0, 64, 0) past the active references."""
import math

import numpy as np

MAX_REFS = 4
PLAIN = (0, 64, 0)


def clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


# ---- 1. statistics
def moments(y):
    """(m, v): the mean in 1 / 256 and the variance in 1 / 65536 of the visible samples; a variance the rounding of m takes below zero is 0"""
    y = np.asarray(y)
    n = int(y.size)
    s1 = int(y.astype(np.int64).sum())
    s2 = int((y.astype(np.int64) ** 2).sum())
    return moments_of_sums(s1, s2, n)


def moments_of_sums(s1, s2, n):
    m = (256 * s1 + n // 2) // n
    q = (256 * s2 + n // 2) // n
    return m, max(256 * q - m * m, 0)


# ---- 2. candidate weights
def candidate(mc, vc, mr, vr):
    """(w, o, is a candidate) of a picture with moments (mc, vc) against a reference with (mr, vr)"""
    w = 64
    if vc != 0 and vr != 0:
        w = clip3(16, 127, (math.isqrt((16384 * vc) // vr) + 1) >> 1)
    o = clip3(-128, 127, (64 * mc - w * mr + 8192) >> 14)
    return w, o, abs(w - 64) >= 2 or o != 0


# ---- 4. sample prediction
def sample(s, w, o):
    """a full sample of a weighted reference; s: int or array"""
    return np.clip(((np.asarray(s, dtype=np.int64) * w + 32) >> 6) + o, 0, 255)


def pred14(p, w, o):
    """8.5.3.3.4.3, luma_log2_weight_denom 6, on the 14-bit intermediate"""
    return np.clip(((np.asarray(p, dtype=np.int64) * w + 2048) >> 12) + o, 0, 255)


# ---- 3. the check
def check(cur, ref, w, o):
    """(plain, weighted) sums of absolute differences over the samples at (4i, 4j)"""
    c = np.asarray(cur)[::4, ::4].astype(np.int64)
    r = np.asarray(ref)[::4, ::4].astype(np.int64)
    return int(np.abs(c - r).sum()), int(np.abs(c - sample(r, w, o)).sum())


def decide(cur, ref):
    """(flag, w, o) of picture `cur` against the input picture `ref`"""
    w, o, cand = candidate(*moments(cur), *moments(ref))
    if not cand:
        return PLAIN
    plain, wt = check(cur, ref, w, o)
    return (1, w, o) if 16 * wt < 15 * plain else PLAIN


def record(inputs, t, dists):
    """the record of P picture t of the clip `inputs` (visible luma planes) whose references lie dists[k] pictures back"""
    return [decide(inputs[t], inputs[t - d]) for d in dists] + [PLAIN] * (MAX_REFS - len(dists))


def search_plane(plane, rec):
    """what the integer search reads of a reference with record entry rec = (flag, w, o): plane: the (coded) plane it would have read otherwise"""
    return sample(plane, rec[1], rec[2]).astype(np.uint8) if rec[0] else np.asarray(plane, dtype=np.uint8)


# ---- 6. syntax
def _ue(v):
    b = bin(v + 1)[2:]
    return "0" * (len(b) - 1) + b


def _se(v):
    return _ue(2 * v - 1 if v > 0 else -2 * v)


def pred_weight_table(rec, nact):
    """the bits of pred_weight_table() for the first nact entries of a record, as a string of 0 / 1"""
    bits = _ue(6) + _se(0)
    bits += "".join("1" if rec[k][0] else "0" for k in range(nact))
    bits += "0" * nact
    for k in range(nact):
        if rec[k][0]:
            bits += _se(rec[k][1] - 64) + _se(rec[k][2])
    return bits


# ---- the brightness changes of the issue's table, applied to the luma of an I420 clip
def change(frames, w, h, kind):
    """kind: "none", "offset" (-6 levels per picture), "gain" (-3/64 per picture), "flash" (+8 levels on every fourth picture)"""
    out = []
    for t, fr in enumerate(frames):
        fr = np.array(fr, dtype=np.uint8, copy=True)
        y = fr[:w * h].astype(np.int64)
        if kind == "offset":
            y = y - 6 * t
        elif kind == "gain":
            y = (y * (64 - 3 * t) + 32) >> 6
        elif kind == "flash":
            y = y + (8 if t % 4 == 3 else 0)
        else:
            assert kind == "none", kind
        fr[:w * h] = np.clip(y, 0, 255).astype(np.uint8)
        out.append(fr)
    return out
