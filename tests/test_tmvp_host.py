"""CPU side of "tmvp" (temporal motion vector prediction): the option's parsing, the parameter sets and slice segment headers with
the temporal flags read back bit by bit and with tests/pyhevc.py, byte equality of every header with tmvp off against what the encoder wrote before the
option existed (tests/golden/tmvp_off_access_units.json), and the merge / AMVP derivation of hevc_core.h with a collocated record (host build:
tests/hostcheck) against pyhevc's SliceDecoder.merge_candidates / amvp_candidates / temporal on random motion fields."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import hc
import pyhevc
from cases import FORMS
from hc import col_record, motion_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. config_parse
@pytest.fixture(scope="module")
def api():
    from kvazzup_amd import _native
    if not os.path.exists(_native.library_path()):
        _native.build_library()
    lib = _native.load_library()
    return lib.kvz_api_get(8).contents


def test_config_parse_tmvp(api):
    cfg = api.config_alloc()
    api.config_init(cfg)
    ok = lambda k, v: api.config_parse(cfg, k.encode(), v.encode())
    assert cfg.contents.tmvp_enable == 0                                  # default off (Kvazaar's is on)
    for v, want in (("1", 1), ("0", 0), ("true", 1), ("false", 0), ("1", 1)):
        assert ok("tmvp", v) == 1 and cfg.contents.tmvp_enable == want, v
    for bad in ("2", "x", "yes please", "-1"):
        assert ok("tmvp", bad) == 0, bad
    for preset in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"):
        api.config_init(cfg)
        assert ok("preset", preset) == 1 and cfg.contents.tmvp_enable == 0, preset
        assert ok("tmvp", "1") == 1 and ok("preset", preset) == 1 and cfg.contents.tmvp_enable == 1, preset     # no preset switches it off either
    api.config_destroy(cfg)


# ---- 2. parameter sets and slice segment headers
def test_headers_with_tmvp_off_are_unchanged():
    """every access unit's headers with tmvp=0 are byte for byte the ones of the encoder before the option (digests from the parent's hevc_headers.h)"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "tmvp_off_access_units.json")))
    assert len(g["cases"]) == 700
    for *args, digest in g["cases"]:
        w, h, lp, sao, wpp, tr, tc, sl, poc = args
        au = hc.access_unit(w, h, poc, lp=lp, tmvp=0, sao=sao, wpp=wpp, tr=tr, tc=tc, slices=sl)
        assert hashlib.sha256(au).hexdigest()[:16] == digest, args


def slice_headers(au, sps, pps, lp, sao):
    """(first, dependent, fields) of every slice segment NAL unit of an access unit, read as 7.3.6.1 lays them out for this encoder's tool set"""
    out = []
    for nal in pyhevc.split_nals(au):
        t = (nal[0] >> 1) & 63
        if t not in (1, 19):
            continue
        idr = t == 19
        r = pyhevc.Bits(pyhevc.unescape(nal)[2:])
        first = r.u(1)
        if idr:
            r.u(1)
        assert r.ue() == 0
        dependent = 0
        if not first:
            if pps["dep"]:
                dependent = r.u(1)
            wc, hc = -(-sps["w"] >> 6), -(-sps["h"] >> 6)
            r.u(max(1, (wc * hc - 1).bit_length()))
        f = {}
        if not dependent:
            f["type"] = r.ue()
            f["tmvp"] = 0
            f["nact"] = pps["nref_default"]
            if not idr:
                f["poc"] = r.u(8)
                assert r.u(1) == 1
                if lp > 1:
                    r.u((lp - 1).bit_length())
                if sps["tmvp"]:
                    f["tmvp"] = r.u(1)
            if sao:
                assert r.u(2) == 3
            if not idr:
                if r.u(1):
                    f["nact"] = r.ue() + 1
                f["col_idx"] = r.ue() if (f["tmvp"] and f["nact"] > 1) else None
                assert r.ue() == 0                                  # five_minus_max_num_merge_cand
            assert r.se() == 0                                      # slice_qp_delta
            assert r.u(1) == 1                                      # slice_loop_filter_across_slices_enabled_flag
        if pps["tiles"] or pps["wpp"]:
            n = r.ue()
            if n:
                ln = r.ue() + 1
                assert all(r.u(ln) + 1 == 2 for _ in range(n))      # the 2-byte substreams the host build gives every segment
        assert r.u(1) == 1                                          # alignment_bit_equal_to_one
        r.align()
        out.append((first, dependent, f))
    return out


@pytest.mark.parametrize("lp", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("form", FORMS)
def test_tmvp_headers(lp, form):
    wpp, tr, tc, sl = form
    for sao in (0, 1):
        for poc in range(0, 7):
            au = hc.access_unit(256, 192, poc, lp=lp, tmvp=1, sao=sao, wpp=wpp, tr=tr, tc=tc, slices=sl)
            nals = pyhevc.split_nals(au)
            sps = pyhevc.parse_sps(pyhevc.unescape(nals[1]))
            pps = pyhevc.parse_pps(pyhevc.unescape(nals[2]))
            assert sps["tmvp"] == 1
            heads = slice_headers(au, sps, pps, lp, sao)
            assert heads and heads[0][0] == 1
            n = max(lp, 1)
            for first, dep, f in heads:
                if dep:
                    continue
                if poc == 0:
                    assert f["type"] == 2 and "poc" not in f
                    continue
                assert f["type"] == 1 and f["poc"] == poc
                assert f["nact"] == min(n, poc)
                # the collocated picture is ref_idx_l0 0, the previous picture: no temporal candidates when that is the IDR picture
                assert f["tmvp"] == (poc != 1), (poc, f)
                assert f["col_idx"] == (0 if (poc != 1 and f["nact"] > 1) else None), (poc, f)
    # the off stream's SPS says 0
    au = hc.access_unit(256, 192, 0, lp=lp, tmvp=0, sao=0, wpp=wpp, tr=tr, tc=tc, slices=sl)
    assert pyhevc.parse_sps(pyhevc.unescape(pyhevc.split_nals(au)[1]))["tmvp"] == 0


# ---- 3. merge / AMVP with the temporal candidate against pyhevc's derivation
@pytest.mark.parametrize("seed", range(16))
def test_merge_and_amvp_with_temporal_candidates_match_pyhevc(seed):
    rng = random.Random(0x7E40 + seed)
    cw, ch = rng.choice(((256, 128), (192, 192), (320, 128), (128, 256)))
    tr, tc = rng.choice(((1, 1), (2, 1), (1, 2), (2, 2)))
    lp = 1 + seed % 4                                   # lp-refs 1 .. 4
    poc = rng.randrange(2, 7)                           # the picture; the collocated one is poc - 1 (never the IDR picture: tmvp is on)
    nref, ncol = min(lp, poc), min(lp, poc - 1)
    log2, intra, mv, ref, cbf = motion_field(rng, cw, ch, nref)
    _, cintra, cmv, cref, _ = motion_field(rng, cw, ch, ncol, p_intra=0.2)
    # the collocated picture's vectors: often the current picture's own (a steady pan), so that the temporal candidate can win
    same = np.array([[rng.random() < 0.5 for _ in range(cw // 8)] for _ in range(ch // 8)])
    cmv = np.where((same & (cintra == 0))[..., None], mv, cmv).astype(np.int16)
    col = col_record(cintra, cmv, cref)
    stub = hc.MotionStub(cw, ch, tr, tc, nref, intra, mv, ref, hc.col_picture(poc - 1, cintra, cmv, cref), poc)
    a = [np.ascontiguousarray(x) for x in (log2, intra, mv, ref, cbf)]
    seen = {"merge_t": 0, "amvp_t": 0, "scaled": 0, "br_out_row": 0, "br_out_pic": 0, "col_intra": 0, "n16": 0, "n32": 0, "merged_t": 0}
    for y in range(0, ch, 8):
        for x in range(0, cw, 8):
            l = int(log2[y // 8, x // 8])
            if intra[y // 8, x // 8] or (x | y) & ((1 << l) - 1):
                continue
            n = 1 << l
            merge, amvp, sig = hc.cands(cw, ch, tr, tc, nref, a, x, y, l, col=col)
            want_m = [(c[0], c[1], c[2]) for c in stub.merge_candidates(x, y, n, x, y, n, n, 0, 0)]
            assert [tuple(merge[3 * k:3 * k + 3]) for k in range(5)] == want_m, (seed, x, y)
            r = int(ref[y // 8, x // 8])
            want_a = [tuple(c) for c in stub.amvp_candidates(x, y, n, x, y, n, n, 0, 0, r)]
            assert [tuple(amvp[2 * k:2 * k + 2]) for k in range(2)] == want_a, (seed, x, y, r)
            own = (int(mv[y // 8, x // 8, 0]), int(mv[y // 8, x // 8, 1]))
            first = next((k for k, c in enumerate(want_m) if (c[0], c[1], c[2]) == own + (r,)), None)
            if first is not None:
                assert sig[0] & 2 and sig[1] == first
            else:
                assert sig[0] == 0 and (own[0] - sig[3], own[1] - sig[4]) == want_a[sig[2]]
            # what came up: a temporal candidate in either list, a scaled one, bottom-right positions that do not count, intra collocated blocks
            t0, tr_ = stub.temporal(x, y, n, n, 0, 0), stub.temporal(x, y, n, n, 0, r)
            seen["n16"] += l == 4
            seen["n32"] += l == 5
            seen["merge_t"] += t0 is not None
            seen["merged_t"] += t0 is not None and first is not None and want_m[first] == t0 + (0,)
            seen["amvp_t"] += tr_ is not None and tr_ in want_a
            xb, yb = x + n, y + n
            seen["br_out_row"] += yb < ch and (yb >> 6) != (y >> 6)
            seen["br_out_pic"] += xb >= cw or yb >= ch
            xc, yc = ((x + n // 2) >> 4), ((y + n // 2) >> 4)
            seen["col_intra"] += int(col[yc, xc, 2] == 0)
            if tr_ is not None and int(col[yc, xc, 2]) not in (0, r + 1):
                seen["scaled"] += 1
    for k in ("merge_t", "amvp_t", "br_out_row", "br_out_pic", "col_intra", "n16", "n32", "merged_t"):
        assert seen[k] > 0, (seed, k, seen)
    if nref > 1 or ncol > 1:
        assert seen["scaled"] > 0, seen


@pytest.mark.parametrize("seed", range(4))
def test_no_record_keeps_the_derivation_of_before(seed):
    """without a collocated record the lists are pyhevc's with slice_temporal_mvp_enabled_flag 0 (what test_lp_refs_host pins for the encoder of before)"""
    rng = random.Random(seed)
    cw, ch, nref = 256, 128, 1 + seed
    log2, intra, mv, ref, cbf = motion_field(rng, cw, ch, nref)
    stub = hc.MotionStub(cw, ch, 1, 1, nref, intra, mv, ref, None, 9)
    a = [np.ascontiguousarray(x) for x in (log2, intra, mv, ref, cbf)]
    for y in range(0, ch, 8):
        for x in range(0, cw, 8):
            l = int(log2[y // 8, x // 8])
            if intra[y // 8, x // 8] or (x | y) & ((1 << l) - 1):
                continue
            n = 1 << l
            merge, amvp, sig = hc.cands(cw, ch, 1, 1, nref, a, x, y, l)
            assert [tuple(merge[3 * k:3 * k + 3]) for k in range(5)] == [c[:3] for c in stub.merge_candidates(x, y, n, x, y, n, n, 0, 0)]
            assert [tuple(amvp[2 * k:2 * k + 2]) for k in range(2)] == [tuple(c) for c in stub.amvp_candidates(x, y, n, x, y, n, n, 0, 0, int(ref[y // 8, x // 8]))]


def test_picture_restatement_files_the_record():
    """ht_picture (what the GPU test restates k_inter_signal with) files the record col_record describes and derives what hc_cands derives"""
    rng = random.Random(5)
    cw, ch, nref = 192, 128, 2
    log2, intra, mv, ref, cbf = motion_field(rng, cw, ch, nref)
    _, cintra, cmv, cref, _ = motion_field(rng, cw, ch, 2)
    col = col_record(cintra, cmv, cref)
    a = [np.ascontiguousarray(x) for x in (log2, intra, mv, ref, cbf)]
    flags, midx, mvp, mvd, out = hc.picture(cw, ch, 1, 1, nref, a, col=col)
    assert np.array_equal(out, col_record(intra, mv, ref))
    for y in range(0, ch, 8):
        for x in range(0, cw, 8):
            l = int(log2[y // 8, x // 8])
            if intra[y // 8, x // 8]:
                continue
            merge, amvp, sig = hc.cands(cw, ch, 1, 1, nref, a, x & ~((1 << l) - 1), y & ~((1 << l) - 1), l, col=col)
            i = (y // 8, x // 8)
            assert (flags[i], midx[i], mvp[i], mvd[i][0], mvd[i][1]) == tuple(sig), (x, y)
