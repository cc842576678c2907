"""CPU side of "uvgx weighted prediction v1" (kvazaar.h weightp): the option's parsing; the statement functions of hevc_core.h (host
build: tests/hostcheck) against the restatement tests/wp_model.py -- random statistics, the extremes, every sample value under every weight --; access units whose
slice headers carry pred_weight_table(), read back by tests/pyhevc.py and decoded by the checker's decoder; and, with the field off, byte equality of every
header with the encoder of before (tests/golden/tmvp_off_access_units.json)."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import hc
import orc
import pyhevc
import wp_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. config_parse
def test_config_parse_weightp():
    from kvazzup_amd import _native
    if not os.path.exists(_native.library_path()):
        _native.build_library()
    api = _native.load_library().kvz_api_get(8).contents
    cfg = api.config_alloc()
    api.config_init(cfg)
    ok = lambda k, v: api.config_parse(cfg, k.encode(), v.encode())
    assert cfg.contents.weightp == 0
    for v, want in (("1", 1), ("0", 0), ("1", 1)):
        assert ok("weightp", v) == 1 and cfg.contents.weightp == want, v
    for bad in ("2", "x", "-1", "", "true"):
        assert ok("weightp", bad) == 0 and cfg.contents.weightp == 1, bad
    for preset in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"):
        api.config_init(cfg)
        assert ok("preset", preset) == 1 and cfg.contents.weightp == 0, preset
        assert ok("weightp", "1") == 1 and ok("preset", preset) == 1 and cfg.contents.weightp == 1, preset
    # the field lies behind lp_gop: the options before it keep their places
    api.config_init(cfg)
    assert ok("lp-gop", "1") == 1 and ok("me-coarse", "64") == 1 and cfg.contents.weightp == 0 and cfg.contents.lp_gop == 1 and cfg.contents.me_coarse == 64
    api.config_destroy(cfg)


# ---- 2. the statement against the model
def test_isqrt():
    rng = random.Random(5)
    vals = [0, 1, 2, 3, 4, 15, 16, 17, (1 << 32) - 1, 1 << 32, (1 << 44) + 12345, (1 << 62) - 1, 1 << 62, (1 << 64) - 1]
    vals += [rng.getrandbits(rng.randrange(1, 64)) for _ in range(2000)] + [k * k + d for k in (3, 255, 65535, 4194303) for d in (-1, 0, 1)]
    import math
    for v in vals:
        assert hc.lib().hw_isqrt(v) == math.isqrt(v), v


def test_moments_and_candidates_match_the_model():
    rng = random.Random(0x77E1)
    stats = []
    for _ in range(3000):                                   # random pictures' sums: a mean, a spread, a size
        n = rng.choice((16 * 16, 320 * 192, 1920 * 1080, 7680 * 4320, rng.randrange(256, 1 << 25)))
        mean, sd = rng.uniform(0, 255), rng.choice((0.0, 0.3, 2.0, 20.0, 70.0)) * rng.random()
        s1 = min(255 * n, max(0, int(mean * n)))
        s2 = min(255 * s1, max(-(-s1 * s1 // n), int((mean * mean + sd * sd) * n)))      # (between the flat picture's and the two-level picture's)
        stats.append((s1, s2, n))
    # the extremes: flat pictures (v = 0), 8K of 255s, black, one bright sample, half black / half white
    n8k = 7680 * 4320
    stats += [(255 * n8k, 255 * 255 * n8k, n8k), (0, 0, n8k), (255, 255 * 255, n8k), (255 * (n8k // 2), 255 * 255 * (n8k // 2), n8k), (128 * 4096, 128 * 128 * 4096, 4096),
              (3 * 1000 + 1, 9 * 1000 + 1, 1000 + 1), (100 * 777 + 1, 100 * 100 * 777 + 201, 777)]
    mom = []
    for s1, s2, n in stats:
        got = hc.wp_moments(s1, s2, n)
        assert got == M.moments_of_sums(s1, s2, n), (s1, s2, n)
        assert got[1] >= 0
        mom.append(got)
    assert hc.wp_moments(255 * n8k, 255 * 255 * n8k, n8k) == (65280, 0)
    assert any(v == 0 for _, v in mom) and any(v > 0 for _, v in mom)
    seen = set()
    pairs = [(rng.choice(mom), rng.choice(mom)) for _ in range(20000)]
    # both clamps of w and of o, v = 0 on either side, an exact tie at the candidate threshold
    pairs += [((100 * 256, 1 << 20), (100 * 256, 1)), ((100 * 256, 1), (100 * 256, 1 << 20)), ((255 * 256, 100), (0, 100)), ((0, 100), (255 * 256, 100)),
              ((50 * 256, 0), (60 * 256, 500)), ((50 * 256, 500), (60 * 256, 0)), ((50 * 256, 0), (50 * 256, 0)), ((100 * 256, 4096), (100 * 256, 4096)),
              ((100 * 256, 4356), (100 * 256, 4096)), ((100 * 256 + 128, 4096), (100 * 256, 4096)), ((100 * 256 + 127, 4096), (100 * 256, 4096))]
    for (mc, vc), (mr, vr) in pairs:
        got = hc.wp_candidate(mc, vc, mr, vr)
        assert got == M.candidate(mc, vc, mr, vr), (mc, vc, mr, vr)
        w, o, _ = got
        seen |= {("w", w) if w in (16, 64, 127) else None, ("o", o) if o in (-128, 127) else None, "cand" if got[2] else "plain"}
    assert {("w", 16), ("w", 127), ("w", 64), ("o", -128), ("o", 127), "cand", "plain"} <= seen, seen
    for cand in (0, 1):
        for plain, wt in ((0, 0), (16, 15), (16, 14), (1600, 1499), (1600, 1500), (1 << 40, (1 << 40) - (1 << 37)), (5, 100)):
            assert hc.lib().hw_accept(cand, plain, wt) == int(bool(cand) and 16 * wt < 15 * plain)


def test_sample_prediction_matches_the_formulas():
    s = np.arange(256)
    for w in range(16, 128):
        for o in (-128, -77, -6, -1, 0, 1, 8, 50, 127):
            want = np.clip(((s * w + 32) >> 6) + o, 0, 255)
            got = np.array([hc.lib().hw_sample(int(v), w, o) for v in s])
            assert np.array_equal(got, want) and np.array_equal(M.sample(s, w, o), want), (w, o)
    # the 14-bit form: at whole vectors (p = 64 s) the sample formula; in between, 8.5.3.3.4.3 (-8192 + ... + 8192 covers what the filters can give)
    rng = random.Random(3)
    for w in (16, 17, 63, 64, 65, 100, 127):
        for o in (-128, -6, 0, 9, 127):
            assert all(hc.lib().hw_pred14(64 * int(v), w, o) == hc.lib().hw_sample(int(v), w, o) for v in s)
            for p in [rng.randrange(-2048, 18432) for _ in range(400)] + [-2048, -1, 0, 1, 16383, 18431]:
                want = min(255, max(0, ((p * w + 2048) >> 12) + o))
                assert hc.lib().hw_pred14(p, w, o) == want == int(M.pred14(p, w, o)), (p, w, o)
    assert all(hc.lib().hw_pred14(p, 64, 0) == min(255, max(0, (p + 32) >> 6)) for p in range(-2048, 18432, 7))      # (64, 0) is the prediction without weights


def test_decision_on_pictures_matches_the_model():
    """hw_decide composes sums, moments, candidate, check and verdict as the kernels do; the model on the same pictures, sizes that are no multiple of 4 or 16 too"""
    rng = np.random.default_rng(11)
    kinds = {"w": 0, "p": 0}
    for w, h in ((320, 192), (322, 190), (200, 120), (64, 64)):
        base = orc.synth_frame(0, 1234, w, h, 1)[:w * h].reshape(h, w).astype(np.int64)
        for f in (lambda y: y, lambda y: y - 6, lambda y: y + 8, lambda y: (y * 61 + 32) >> 6, lambda y: (y * 80 + 32) >> 6, lambda y: y + rng.integers(-40, 41, y.shape),
                  lambda y: (y * 40 >> 6) + 90, lambda y: np.full_like(y, 77), lambda y: y + 1):
            cur = np.clip(f(base), 0, 255).astype(np.uint8)
            for a, b in ((cur, base.astype(np.uint8)), (base.astype(np.uint8), cur)):
                pitch = (w + 63) & ~63
                pa, pb = np.zeros((h, pitch), np.uint8), np.zeros((h, pitch), np.uint8)
                pa[:, :w], pb[:, :w] = a, b
                pa[:, w:], pb[:, w:] = 201, 3                # (what lies beside the visible samples must not count)
                out = np.zeros(3, np.int32)
                hc.lib().hw_decide(pa.ctypes.data, pb.ctypes.data, w, h, pitch, out.ctypes.data)
                assert tuple(int(v) for v in out) == M.decide(a, b), (w, h)
                kinds["w" if out[0] else "p"] += 1
    assert kinds["w"] >= 20 and kinds["p"] >= 8, kinds


# ---- 3. syntax
def _header_bits(au, nal_index):
    nal = pyhevc.split_nals(au)[nal_index]
    rbsp = pyhevc.unescape(nal)[2:]
    return "".join(format(b, "08b") for b in rbsp)


@pytest.mark.parametrize("nact", [1, 2, 3, 4])
def test_slice_headers_carry_the_table(nact):
    rng = random.Random(nact)
    recs = [[(0, 64, 0)] * 4, [(1, 127, -128)] * 4, [(1, 16, 127)] * 4, [(1, 63, 0), (0, 64, 0), (1, 64, -1), (1, 70, 5)]]
    recs += [[((1, rng.randrange(16, 128), rng.randrange(-128, 128)) if rng.random() < 0.6 else (0, 64, 0)) for _ in range(4)] for _ in range(12)]
    for rec in recs:
        for wpp, tr, tc, sl in ((1, 1, 1, 0), (0, 1, 1, 0), (0, 2, 2, 2), (1, 1, 1, 1)):
            on = hc.access_unit(256, 192, nact, lp=4, weightp=1, wts=rec, wpp=wpp, tr=tr, tc=tc, slices=sl)
            off = hc.access_unit(256, 192, nact, lp=4, weightp=0, wts=None, wpp=wpp, tr=tr, tc=tc, slices=sl)
            non, noff = pyhevc.split_nals(on), pyhevc.split_nals(off)
            assert non[0] == noff[0] and non[1] == noff[1]                       # VPS and SPS are unchanged
            pps = pyhevc.parse_pps(pyhevc.unescape(non[2]))
            assert pps["weighted_pred"] == 1 and pps["weighted_bipred"] == 0 and pyhevc.parse_pps(pyhevc.unescape(noff[2]))["weighted_pred"] == 0
            table = M.pred_weight_table(rec, nact)
            assert len(M.pred_weight_table([(0, 64, 0)] * 4, nact)) == 6 + 2 * nact <= 14
            for k in range(3, len(non)):
                a, b = _header_bits(on, k), _header_bits(off, k)
                dependent = sl == 1 and k > 3
                if dependent:
                    assert a == b                                                # a dependent slice segment carries no table
                    continue
                # the header with the option is the header without it with the table spliced in (in front of five_minus_max_num_merge_cand)
                assert any(a[:i] == b[:i] and a[i:i + len(table)] == table and _header_from(a, i + len(table)) == _header_from(b, i) for i in range(8, len(b))), (rec, k)


PAYLOAD = "1010010110000000"                                # the host build's placeholder substream, 0xa5 0x80


def _header_from(bits, start):
    """the header's bits from `start` up to its rbsp trailing bits: they end where the first substream begins, at a byte boundary"""
    k = next(i for i in range((start + 7) // 8 * 8, len(bits), 8) if bits[i:i + 16] == PAYLOAD)
    return bits[start:k].rstrip("0")[:-1]


def _payloads(w, h, n, frames):
    """(idr?, poc, the slice data) of a stream of the checker's encoder without WPP: what lies behind the header the host build writes for the same picture"""
    oe = orc.OracleEncoder(w, h, qp=32, period=64, me_range=8, wpp=0)
    oe.set_option("lp-refs", n)
    out = []
    try:
        for t, fr in enumerate(frames):
            au = oe.encode(fr)
            nal = [x for x in pyhevc.split_nals(au) if (x[0] >> 1) & 63 in (1, 19)]
            assert len(nal) == 1
            rbsp = pyhevc.unescape(nal[0])
            mine = pyhevc.split_nals(hc.access_unit(w, h, t, lp=n, weightp=0, wts=None, payload=b"", write_ps=0, wpp=0))[0]
            hdr = pyhevc.unescape(mine)[:-2]                                      # (the placeholder substream's two bytes)
            assert rbsp.startswith(hdr), t                                        # the host build's header is the checker's
            out.append((t, bytes(rbsp[len(hdr):]), oe.recon()))
    finally:
        oe.close()
    return out


def test_access_units_decode_with_the_weights_put_in():
    """A stream of the checker's encoder (lp-refs 4: pictures with 1, 2, 3 and 4 references) under new headers from the host build: weighted_pred_flag and a
    table per P picture.  tests/pyhevc.py reads back the weights put in; it and the checker's decoder make the same pictures of the stream -- the reconstruction
    of before where every flag is 0, another picture where a reference is weighted."""
    from deckit import tabs
    w, h, n = 128, 64, 4
    frames = [orc.synth_frame(0, 0x5EED0000, w, h, t) for t in range(5)]
    pay = _payloads(w, h, n, frames)
    recs = {1: [(1, 70, -9), M.PLAIN, M.PLAIN, M.PLAIN], 2: [M.PLAIN, (1, 16, 127), M.PLAIN, M.PLAIN], 3: [(1, 127, -128), M.PLAIN, (1, 60, 3), M.PLAIN],
            4: [(1, 65, 0), (1, 64, -1), (1, 63, 1), (1, 90, -40)]}
    for weighted in (False, True):
        dec, od = pyhevc.Decoder(tabs()), orc.OracleDecoder()
        try:
            for t, data, rec_plain in pay:
                rec = recs[t] if weighted and t else [M.PLAIN] * 4
                au = hc.access_unit(w, h, t, lp=n, weightp=1, wts=rec if t else None, payload=data, write_ps=int(t == 0), wpp=0)
                dec.decode(au)
                if t:
                    ld, cd, wp = dec.last_sh["wp"]
                    nact = min(n, t)
                    assert (ld, cd) == (6, 6) and len(wp) == 1 and len(wp[0]) == nact
                    for k in range(nact):
                        assert wp[0][k][0] == (rec[k][1], rec[k][2]) and wp[0][k][1] == (64, 0) and wp[0][k][2] == (64, 0), (t, k, wp[0][k])
                got = od.decode_au(au, t)
                assert len(got) == 1
                mine = dec.flush()[-1]["i420"]
                assert np.array_equal(got[0]["i420"], mine), "picture %d: the checker's decoder and pyhevc differ" % t
                if not weighted or t == 0:
                    assert np.array_equal(mine, rec_plain), t
                else:
                    assert not np.array_equal(mine[:w * h], rec_plain[:w * h]), t
        finally:
            od.close()


def test_headers_with_the_field_off_are_the_parents_bytes():
    """StreamParams::weightp 0 (with or without a PicWeights handed over): every access unit's headers are byte for byte the ones of the encoder before the option
    (digests from an earlier hevc_headers.h)"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "tmvp_off_access_units.json")))
    assert len(gold["cases"]) == 700
    some = [(1, 99, -3)] * 4
    for i, (*args, digest) in enumerate(gold["cases"]):
        w, h, lp, sao, wpp, tr, tc, sl, poc = args
        au = hc.access_unit(w, h, poc, lp=lp, weightp=0, wts=some if i & 1 else None, sao=sao, wpp=wpp, tr=tr, tc=tc, slices=sl)
        assert hashlib.sha256(au).hexdigest()[:16] == digest, args
