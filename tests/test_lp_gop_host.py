"""CPU side of "uvgx low-delay GOP v1" (kvazaar.h lp-gop): the option's parsing, the statement tests/lp_gop_model.py held to the
tables and properties the design states, the slice segment headers with each picture's reference picture set read back (host build: tests/hostcheck) --
and, with the option off, byte equality of every header with the encoder of before (tests/golden/tmvp_off_access_units.json) --, and the merge / AMVP
derivation of hevc_core.h with a table of POC distances against pyhevc's SliceDecoder on random motion fields whose references are the model's sets."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import hc
import lp_gop_model as M
import lp_gop_stream
import pyhevc
from cases import FORMS, GDN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. config_parse
def test_config_parse_lp_gop():
    from kvazzup_amd import _native
    if not os.path.exists(_native.library_path()):
        _native.build_library()
    api = _native.load_library().kvz_api_get(8).contents
    cfg = api.config_alloc()
    api.config_init(cfg)
    ok = lambda k, v: api.config_parse(cfg, k.encode(), v.encode())
    assert cfg.contents.lp_gop == 0
    for v, want in (("1", 1), ("0", 0), ("true", 1), ("false", 0), ("1", 1)):
        assert ok("lp-gop", v) == 1 and cfg.contents.lp_gop == want, v
    for bad in ("2", "x", "-1"):
        assert ok("lp-gop", bad) == 0 and cfg.contents.lp_gop == 1, bad
    for preset in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"):
        api.config_init(cfg)
        assert ok("preset", preset) == 1 and cfg.contents.lp_gop == 0, preset
        assert ok("lp-gop", "1") == 1 and ok("preset", preset) == 1 and cfg.contents.lp_gop == 1, preset
    # the gop string: parsed as ever, whatever lp-gop says, and never the switch
    api.config_init(cfg)
    assert (cfg.contents.gop_len, cfg.contents.gop_lp_ref_depth, cfg.contents.gop_lp_temporal_layers) == (0, 1, 1)
    for v, want in (("lp-g4d3t1", (4, 3, 1)), ("lp-g8d4t1", (8, 4, 1)), ("lp-g1d1t1", (1, 1, 1)), ("lp-g32d2t2", (32, 2, 2)), ("lp-g4d7t1", (4, 7, 1))):
        assert ok("gop", v) == 1, v
        assert (cfg.contents.gop_len, cfg.contents.gop_lp_ref_depth, cfg.contents.gop_lp_temporal_layers) == want and cfg.contents.lp_gop == 0, v
    assert ok("gop", "0") == 1 and cfg.contents.gop_len == 0
    for bad in ("8", "16", "lp-g0d1t1", "lp-g33d1t1", "lp-g4d0t1", "lp-g4d3t0", "lp-g4d3", "b4"):
        assert ok("gop", bad) == 0, bad
    api.config_destroy(cfg)


# ---- 2. the model
def test_model_tables():
    assert [M.layer(t, 4, 3) for t in range(1, 9)] == [3, 2, 3, 1, 3, 2, 3, 1]
    assert [M.layer(t, 8, 4) for t in range(1, 9)] == [4, 3, 4, 2, 4, 3, 4, 1]
    assert all(M.layer(t, g, 1) == 1 for g in (1, 4, 8) for t in range(1, 40))
    assert [M.picture_qp(32, t, 4, 3) for t in range(0, 6)] == [32, 35, 34, 35, 33, 35]
    assert M.picture_qp(50, 1, 4, 3) == 51 and M.picture_qp(51, 4, 4, 3) == 51 and M.picture_qp(0, 0, 4, 3) == 0
    want3 = {1: [0], 2: [1, 0], 3: [2, 1, 0], 4: [3, 2, 0], 5: [4, 3, 0], 6: [5, 4, 3], 7: [6, 5, 4], 8: [7, 6, 4], 9: [8, 7, 4], 10: [9, 8, 7],
             11: [10, 9, 8], 12: [11, 10, 8], 13: [12, 11, 8]}
    for t, s in want3.items():
        assert M.ref_pocs(t, 4, 3) == s, t
    want2 = {1: [0], 2: [1, 0], 3: [2, 0], 4: [3, 0], 5: [4, 0], 6: [5, 4], 7: [6, 4], 8: [7, 4], 9: [8, 4], 10: [9, 8], 11: [10, 8], 12: [11, 8], 13: [12, 8]}
    for t, s in want2.items():
        assert M.ref_pocs(t, 4, 2) == s, t
    assert M.ref_dists(9, 4, 3) == [1, 2, 5] and M.ref_dists(5, 4, 2) == [1, 5]


@pytest.mark.parametrize("g", [1, 2, 3, 4, 5, 6, 8, 12, 16, 32])
def test_model_properties(g):
    for n in (1, 2, 3, 4):
        assert M.check_properties(g, n, 200)
    if 2 <= g <= 6:                                     # the key picture is within reach from every position
        for t in range(2, 100):
            assert ((t - 2) // g) * g in M.ref_pocs(t, g, 2), (g, t)


# ---- 3. headers
@pytest.mark.parametrize("gdn", GDN)
@pytest.mark.parametrize("form", FORMS)
def test_headers_carry_the_model(gdn, form):
    g, d, n = gdn
    wpp, tr, tc, sl = form
    period = 2 * g + 3
    for tmvp, sao in ((0, 0), (1, 1)):
        for pic in M.structure(period, 2 * period, g, d, n, 32):
            t = pic["poc"]
            au = hc.access_unit(256, 192, t, lp=n, tmvp=tmvp, sao=sao, wpp=wpp, tr=tr, tc=tc, slices=sl, qp_delta=pic["qp"] - 32, dists=pic["dists"])
            nals = pyhevc.split_nals(au)
            sps = pyhevc.parse_sps(pyhevc.unescape(nals[1]))
            pps = pyhevc.parse_pps(pyhevc.unescape(nals[2]))
            assert lp_gop_stream.sps_dpb(pyhevc.unescape(nals[1])) == max(n, 1) + 1
            assert pps["nref_default"] == max(n, 1)
            heads = lp_gop_stream.slice_headers(au, sps, pps)
            assert heads and heads[0]["first"] == 1
            for f in heads:
                if f["dependent"]:
                    continue
                assert f["qp"] == pic["qp"]
                if pic["idr"]:
                    assert f["nal"] == 19 and f["type"] == 2
                    continue
                assert f["nal"] == 1 and f["type"] == 1 and f["poc"] == t and f["rps_in_header"]
                assert f["rps"] == [(p - t, 1) for p in pic["refs"]], (gdn, t, f["rps"])
                assert f["nact"] == len(pic["refs"]) == min(max(n, 1), t)
                assert f["tmvp"] == (1 if tmvp and t != 1 else 0)
    # the parameter sets are those of lp-refs alone
    on = pyhevc.split_nals(hc.access_unit(256, 192, 0, lp=n, tmvp=0, sao=0, wpp=wpp, tr=tr, tc=tc, slices=sl, qp_delta=0, dists=()))
    off = pyhevc.split_nals(hc.access_unit(256, 192, 0, lp=n, tmvp=0, sao=0, wpp=wpp, tr=tr, tc=tc, slices=sl))
    assert on[:3] == off[:3]


def test_headers_with_the_option_off_are_unchanged():
    """without a table every access unit's headers are byte for byte the ones of the encoder before the option (digests from an earlier hevc_headers.h)"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "tmvp_off_access_units.json")))
    assert len(gold["cases"]) == 700
    for *args, digest in gold["cases"]:
        w, h, lp, sao, wpp, tr, tc, sl, poc = args
        au = hc.access_unit(w, h, poc, lp=lp, tmvp=0, sao=sao, wpp=wpp, tr=tr, tc=tc, slices=sl)
        assert hashlib.sha256(au).hexdigest()[:16] == digest, args


# ---- 4. merge / AMVP with a distance table against pyhevc's derivation
def _col_picture(poc, intra, mv, ref, dists):
    p = hc.col_picture(poc, intra, mv, ref)
    up = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)
    p.ref_poc[:, :, 0] = poc - np.asarray(dists, np.int32)[up(ref).astype(np.int32)]
    return p


def _col_record(intra, mv, ref, dists):
    rec = hc.col_record(intra, mv, ref)
    rec[..., 2] = np.where(intra[::2, ::2] != 0, 0, np.asarray(dists, np.int16)[ref[::2, ::2].astype(np.int32)])
    return np.ascontiguousarray(rec)


def _tab(dists):
    return sum(d << (8 * k) for k, d in enumerate(dists))


def _run(seed, g, n, poc, seen, pairs):
    rng = random.Random(0x60B0 + seed)
    cw, ch = rng.choice(((256, 128), (192, 192), (320, 128), (128, 256)))
    tr, tc = rng.choice(((1, 1), (2, 1), (1, 2), (2, 2)))
    dists, cdists = M.ref_dists(poc, g, n), M.ref_dists(poc - 1, g, n)
    nref, ncol = len(dists), len(cdists)
    log2, intra, mv, ref, cbf = hc.motion_field(rng, cw, ch, nref)
    _, cintra, cmv, cref, _ = hc.motion_field(rng, cw, ch, ncol, p_intra=0.2)
    same = np.array([[rng.random() < 0.5 for _ in range(cw // 8)] for _ in range(ch // 8)])
    cmv = np.where((same & (cintra == 0))[..., None], mv, cmv).astype(np.int16)
    col = _col_record(cintra, cmv, cref, cdists)
    stub = hc.MotionStub(cw, ch, tr, tc, nref, intra, mv, ref, _col_picture(poc - 1, cintra, cmv, cref, cdists), poc)
    stub.refs = [[stub.refs[0][0]] + [hc.Ref(poc - dists[k]) for k in range(1, nref)], []]
    a = [np.ascontiguousarray(x) for x in (log2, intra, mv, ref, cbf)]
    for y in range(0, ch, 8):
        for x in range(0, cw, 8):
            l = int(log2[y // 8, x // 8])
            if intra[y // 8, x // 8] or (x | y) & ((1 << l) - 1):
                continue
            nn = 1 << l
            merge, amvp, sig = hc.cands(cw, ch, tr, tc, nref, a, x, y, l, col=col, tab=_tab(dists))
            want_m = [(c[0], c[1], c[2]) for c in stub.merge_candidates(x, y, nn, x, y, nn, nn, 0, 0)]
            assert [tuple(merge[3 * k:3 * k + 3]) for k in range(5)] == want_m, (seed, x, y)
            r = int(ref[y // 8, x // 8])
            want_a = [tuple(c) for c in stub.amvp_candidates(x, y, nn, x, y, nn, nn, 0, 0, r)]
            assert [tuple(amvp[2 * k:2 * k + 2]) for k in range(2)] == want_a, (seed, x, y, r)
            own = (int(mv[y // 8, x // 8, 0]), int(mv[y // 8, x // 8, 1]))
            first = next((k for k, c in enumerate(want_m) if c == own + (r,)), None)
            if first is not None:
                assert sig[0] & 2 and sig[1] == first
            else:
                assert sig[0] == 0 and (own[0] - sig[3], own[1] - sig[4]) == want_a[sig[2]]
            # what came up: a spatial neighbour of another reference whose vector AMVP scales (td != tb), a temporal candidate with td != tb
            seen["cus"] += 1
            hit = False
            nb = [(x - 1, y + nn), (x - 1, y + nn - 1), (x + nn, y - 1), (x + nn - 1, y - 1), (x - 1, y - 1)]
            A = [(xn, yn) for xn, yn in nb[:2] if stub.pb_avail(x, y, nn, x, y, nn, nn, 0, xn, yn) and stub.pic.ref_idx[yn >> 2, xn >> 2, 0] >= 0]
            B = [(xn, yn) for xn, yn in nb[2:] if stub.pb_avail(x, y, nn, x, y, nn, nn, 0, xn, yn) and stub.pic.ref_idx[yn >> 2, xn >> 2, 0] >= 0]
            for grp in ((A,) if A else (B,)):
                if grp and not any(int(stub.pic.ref_idx[yn >> 2, xn >> 2, 0]) == r for xn, yn in grp):
                    rn = int(stub.pic.ref_idx[grp[0][1] >> 2, grp[0][0] >> 2, 0])
                    if dists[rn] != dists[r]:
                        hit = True
                        pairs.add((dists[rn], dists[r]))
            xc, yc = ((x + nn // 2) >> 4), ((y + nn // 2) >> 4)
            td = int(col[yc, xc, 2])
            if stub.temporal(x, y, nn, nn, 0, r) is not None and td not in (0, dists[r]):
                hit = True
            seen["scaled"] += hit


def test_merge_and_amvp_with_a_distance_table_match_pyhevc():
    seen, pairs = {"cus": 0, "scaled": 0}, set()
    seed = 0
    for g, n in ((4, 3), (4, 2), (4, 4), (3, 4), (8, 3), (2, 2)):
        for poc in range(2, 2 * g + 3):
            _run(seed, g, n, poc, seen, pairs)
            seed += 1
    assert seen["scaled"] * 4 >= seen["cus"], seen
    # every pair of different distances that g4, n = 3 can put into one picture's list came up as (neighbour's, own) in a spatial scaling
    want = set()
    for t in range(2, 40):
        d = M.ref_dists(t, 4, 3)
        want |= {(a, b) for a in d for b in d if a != b}
    assert want <= pairs, sorted(want - pairs)


def test_sequential_table_is_the_derivation_without_one():
    """a table that says k + 1 gives what the entry gives without a table"""
    rng = random.Random(11)
    cw, ch, nref = 256, 128, 3
    log2, intra, mv, ref, cbf = hc.motion_field(rng, cw, ch, nref)
    _, cintra, cmv, cref, _ = hc.motion_field(rng, cw, ch, nref)
    col = hc.col_record(cintra, cmv, cref)
    a = [np.ascontiguousarray(x) for x in (log2, intra, mv, ref, cbf)]
    for y in range(0, ch, 8):
        for x in range(0, cw, 8):
            l = int(log2[y // 8, x // 8])
            if intra[y // 8, x // 8] or (x | y) & ((1 << l) - 1):
                continue
            o1 = hc.cands(cw, ch, 1, 1, nref, a, x, y, l, col=col, tab=_tab([1, 2, 3]))
            o2 = hc.cands(cw, ch, 1, 1, nref, a, x, y, l, col=col)
            assert all(np.array_equal(p, q) for p, q in zip(o1, o2)), (x, y)
