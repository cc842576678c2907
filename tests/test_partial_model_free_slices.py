"""CPU: the rules of partial pictures v1 for pictures of free slices on the model of tests/partial_model.py alone -- properties of the statement of record itself, on
streams of its own (the product is held to the model in tests/test_partial_pictures.py and tests/test_gpu_partial_pictures.py): a first segment lost with an independent one
behind it, a middle independent segment lost, a dependent segment dragged along, two separate gaps in one picture; synthesiser slices=3, with and without WPP,
lf_across 0 and 2, 72x56 with coding tree blocks of 16 and 32 (partial last column and row) and 64x64 with 16.  The losses are chosen from the streams' own segment
tables."""
import functools

import numpy as np
import pytest

import deckit
import enckit
import orc
import partial_model as pm

CASES = [(72, 56, 4, 0, 0, 21), (72, 56, 4, 1, 2, 22), (72, 56, 5, 1, 0, 23), (64, 64, 4, 0, 2, 24), (64, 64, 4, 1, 0, 25)]


@functools.lru_cache(maxsize=None)
def case(w, h, ctb, wpp, lf, seed):
    g = orc.OracleGen(w, h, seed=seed, slices=3, wpp=wpp, ctb_log2=ctb, lf_across=lf, tile_rows=1, tile_cols=1, gop=0, b_slices=0, tmvp=1, sao=1, intra_period=16)
    aus = [g.picture() for _ in range(7)]
    g.close()
    return aus, pm.segment_table(aus)


def patterns(table):
    """losses by pattern, each on a picture of its own behind the first: {pattern: {access unit: (lost VCL units)}}"""
    out = {}
    for t, segs in enumerate(table):
        if t == 0 or len(segs) < 3:
            continue
        indep = [k for k, s in enumerate(segs) if k > 0 and not s[1]]
        if indep and indep[0] == 1:
            out.setdefault("first segment lost with an independent one behind it", {t: (0,)})
        mid = [k for k in indep if k < len(segs) - 1]
        if mid:
            out.setdefault("a middle independent segment lost", {t: (mid[0],)})
        if len(indep) >= 2 and indep[-1] - indep[0] >= 2:
            out.setdefault("two separate gaps in one picture", {t: (indep[0], indep[-1])})
        dep = [k for k, s in enumerate(segs) if s[1] and k + 1 < len(segs) and segs[k + 1][1]]
        if dep:
            out.setdefault("a middle dependent segment lost that drags later dependents with it", {t: (dep[0],)})
    return out


def test_every_pattern_occurs_in_the_case_table():
    seen = set()
    for c in CASES:
        seen |= set(patterns(case(*c)[1]))
    assert seen == {"first segment lost with an independent one behind it", "a middle independent segment lost", "two separate gaps in one picture",
                    "a middle dependent segment lost that drags later dependents with it"}, seen


@pytest.mark.parametrize("c", CASES)
def test_the_model_keeps_what_arrived(c):
    w, h, ctb, wpp, lf, seed = c
    aus, table = case(*c)
    whole = {(p["cvs"], p["poc"]): p for p in deckit.python_pictures(aus)}
    for what, lost in patterns(table).items():
        for mode in (2, 3):
            pics, d = pm.decode([au for _, au in pm.cut(aus, lost)], deckit.tabs(), mode)
            assert len(pics) == len(aus) and d.damage, what
            first = d.damage[0]
            assert 0 < first["missing"] < first["total"], what
            if what.startswith("first"):
                assert first["runs"][0][0] == 0
            if what.startswith("two"):
                assert len(first["runs"]) >= 2
            if what.startswith("a middle dependent"):
                (t, (k,)), = lost.items()
                assert first["missing"] > (table[t][k + 1][2] - table[t][k][2]), "the dependent segment behind the lost one was decoded"
            got = enckit.planes(next(p for p in pics if (p["cvs"], p["poc"]) == (first["cvs"], first["poc"]))["i420"], w, h)
            intact = enckit.planes(whole[(first["cvs"], first["poc"])]["i420"], w, h)
            n, wc = 1 << ctb, -(-w >> ctb)
            far = np.ones((h, w), bool)
            for a, cnt in first["runs"]:
                for b in range(a, a + cnt):
                    y0, x0 = (b // wc) * n, (b % wc) * n
                    far[max(0, y0 - 8):y0 + n + 8, max(0, x0 - 8):x0 + n + 8] = False
            if not first["src_damaged"] and far.any():
                assert np.array_equal(got[0][far], intact[0][far]), "%s, mode %d: a received sample far from what is missing differs from the intact decode" % (what, mode)
