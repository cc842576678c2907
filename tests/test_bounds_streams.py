"""Streams at the bounds of the syntax (tests/bounds_cases.py): the checker's decoder (oracle/hevc_dec.c) and the decoder written from the standard's text
(tests/pyhevc.py, Python integers: the unbounded-precision statement of 8.6.2 - 8.6.4 and 8.5.3.3.4) must agree on every picture bit for bit before the HIP decoder
is held to either (tests/test_gpu_bounds_streams.py), and every row must hold what it is there for.  CPU only."""
import numpy as np
import pytest

import bounds_cases
import orc
import pyhevc
from deckit import tabs


def decode_both(aus):
    od = orc.OracleDecoder()
    want = []
    for au in aus:
        want += od.decode_au(au)
    want += od.flush()
    od.close()
    pd = pyhevc.Decoder(tabs())
    for au in aus:
        pd.decode(au)
    return want, pd.flush(), pd.seen


@pytest.mark.parametrize("r", bounds_cases.ROWS, ids=lambda r: r["id"])
def test_checker_and_python_decoder_agree_at_the_bounds(r):
    aus = bounds_cases.stream(r)
    assert max(len(au) for au in aus) <= 4 * r["w"] * r["h"] + (1 << 20)           # (OracleGen.buf: the densest rows take about a byte per sample)
    want, got, seen = decode_both(aus)
    assert len(want) == len(got) == r["pictures"]
    for k, (a, b) in enumerate(zip(want, got)):
        assert (a["width"], a["height"], a["poc"]) == (b["width"], b["height"], b["poc"]) and (a["width"], a["height"]) == (r["w"], r["h"]), k
        d = np.nonzero(a["i420"] != b["i420"])[0]
        assert d.size == 0, "picture %d: %d samples differ, first at %d" % (k, d.size, d[0])
    missing = [k for k in r["seen"] if seen[k] <= 0]
    assert not missing, "the stream holds none of %r; it holds %r" % (missing, {k: v for k, v in sorted(seen.items()) if v})


def test_switched_off_the_bounds_draw_nothing():
    """sat_levels, edge_mvd and edge_weights at 0 and at -1 take nothing from the random sequence: the stream is byte for byte the one without the fields"""
    kw = dict(seed=77, density=45, num_refs=4, tmvp=1, sign_hiding=1, transform_skip=1, weighted=60, b_slices=50, gop=4, tq_bypass=15, scaling_lists=4)
    streams = []
    for off in (None, 0, -1):
        extra = {} if off is None else dict(sat_levels=off, edge_mvd=off, edge_weights=off)
        g = orc.OracleGen(200, 136, **kw, **extra)
        streams.append([g.picture() for _ in range(6)])
        g.close()
    assert streams[0] == streams[1] == streams[2]
    g = orc.OracleGen(200, 136, **kw, sat_levels=35, edge_mvd=20, edge_weights=1)
    assert [g.picture() for _ in range(6)] != streams[0]
    g.close()


@pytest.mark.parametrize("w,h,ctb_log2", [(16, 200, 4), (32, 136, 5), (64, 200, 6)])
def test_saturating_coding_tree_units_stay_within_their_size_limit(w, h, ctb_log2):
    """7.4.9.x: a coding tree unit takes 5/3 of its raw size at most.  In a picture one coding tree block wide under WPP every substream is one unit, so the entry
    points state each unit's size; with every residual block asked to saturate, the synthesiser's running estimate is all that keeps them inside.  The estimate admits
    saturating blocks up to the raw size and leaves 2/3 of it (8 bits per luma sample) to what follows: an empirical margin (oracle/hevc_gen.c sat_fits), held here
    on these one-block-wide pictures only, and from its other side by test_the_ordinary_draw_stays_inside_the_margin_left_to_it."""
    g = orc.OracleGen(w, h, seed=5, ctb_log2=ctb_log2, wpp=1, sat_levels=100, density=45, intra_in_p=30, tq_bypass=20, transform_skip=1, slices=0, tile_rows=1)
    aus = [g.picture() for _ in range(4)]
    g.close()
    want, got, seen = decode_both(aus)
    assert all(np.array_equal(a["i420"], b["i420"]) for a, b in zip(want, got)) and len(want) == len(got) == 4
    raw_bits = 12 << (2 * ctb_log2)
    print("largest coding tree unit: %d bits, raw size %d, limit %d" % (8 * seen["substream_bytes_max"], raw_bits, raw_bits * 5 // 3))
    assert seen["level_big"] > 0 and 8 * seen["substream_bytes_max"] <= raw_bits * 5 // 3


@pytest.mark.parametrize("w,h,ctb_log2", [(16, 200, 4), (32, 136, 5), (64, 200, 6)])
def test_the_ordinary_draw_stays_inside_the_margin_left_to_it(w, h, ctb_log2):
    """sat_fits leaves 8 bits per luma sample of a coding tree unit to the ordinary syntax: no unit of the ordinary draw, at twice the density any row uses, takes more
    (measured: 3.9 bits per sample at CTB 16, 2.0 at 32, 1.5 at 64)"""
    worst = 0
    for seed in (1, 2, 3):
        g = orc.OracleGen(w, h, seed=seed, ctb_log2=ctb_log2, wpp=1, density=90, intra_in_p=30, tq_bypass=20, transform_skip=1, slices=0, tile_rows=1)
        aus = [g.picture() for _ in range(4)]
        g.close()
        pd = pyhevc.Decoder(tabs())
        for au in aus:
            pd.decode(au)
        worst = max(worst, 8 * pd.seen["substream_bytes_max"])
    print("largest ordinary coding tree unit: %.2f bits per luma sample" % (worst / (1 << (2 * ctb_log2))))
    assert worst <= 8 << (2 * ctb_log2)


def test_levels_stay_inside_their_range():
    """TransCoeffLevel is -32768 .. 32767: +32768 is never written, not by a coded sign and not by a hidden one (pyhevc.Decoder.raw_levels: the levels as parsed, before any clip)"""
    g = orc.OracleGen(136, 72, seed=9, sat_levels=60, sign_hiding=1, tq_bypass=20, transform_skip=1)
    aus = [g.picture() for _ in range(3)]
    g.close()
    pd = pyhevc.Decoder(tabs())
    pd.raw_levels = []
    for au in aus:
        pd.decode(au)
    lo, hi = min(pd.raw_levels), max(pd.raw_levels)
    assert lo == -32768 and hi == 32767, (lo, hi)
