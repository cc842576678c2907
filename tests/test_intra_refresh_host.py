"""CPU side of "uvgx intra refresh v1" (kvazaar.h intra-refresh): the option's parsing; the statement functions of hevc_core.h (host build:
tests/hostcheck) against the restatement tests/ir_model.py -- every coded width 64 .. 4096 under every N --; the access units: with the option off the bytes of
before (tests/golden/tmvp_off_access_units.json), with it on one more NAL unit in a cycle's first picture, the recovery point SEI, which the decoder's host
half (tests/parser_probe.py), the checker's decoder and tests/pyhevc.py pass over."""
import hashlib
import json
import os

import numpy as np
import pytest

import hc
import ir_model as M
import orc
import pyhevc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def nal_type(nal):
    return (nal[0] >> 1) & 63


# ---- 1. config_parse
def test_config_parse_intra_refresh():
    from kvazzup_amd import _native
    if not os.path.exists(_native.library_path()):
        _native.build_library()
    api = _native.load_library().kvz_api_get(8).contents
    cfg = api.config_alloc()
    api.config_init(cfg)
    ok = lambda k, v: api.config_parse(cfg, k.encode(), v.encode())
    assert cfg.contents.intra_refresh == 0
    for v in [2, 3, 30, 60, 254, 255, 0, 17]:
        assert ok("intra-refresh", str(v)) == 1 and cfg.contents.intra_refresh == v, v
    for bad in ("1", "256", "-1", "x", "", "true", "4096"):
        assert ok("intra-refresh", bad) == 0 and cfg.contents.intra_refresh == 17, bad
    for preset in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"):
        api.config_init(cfg)
        assert ok("preset", preset) == 1 and cfg.contents.intra_refresh == 0, preset
        assert ok("intra-refresh", "30") == 1 and ok("preset", preset) == 1 and cfg.contents.intra_refresh == 30, preset
    # the field lies behind weightp: the options before it keep their places
    api.config_init(cfg)
    assert ok("weightp", "1") == 1 and ok("lp-gop", "1") == 1 and cfg.contents.intra_refresh == 0 and cfg.contents.weightp == 1 and cfg.contents.lp_gop == 1
    api.config_destroy(cfg)


# ---- 2. the statement against the model
def test_every_schedule_matches_the_model_and_covers_the_picture():
    sched = np.zeros(2 * 254, np.int32)
    bands = np.zeros(2 * 256, np.int32)
    for cw in range(64, 4097, 64):
        hc.lib().hi_schedules(cw, sched.ctypes.data)
        for N in range(2, 256):
            m, n = int(sched[2 * (N - 2)]), int(sched[2 * (N - 2) + 1])
            assert (m, n) == (M.step(cw, N), M.cycle(cw, N)), (cw, N)
            assert 1 <= n <= N and m >= 1, (cw, N, m, n)
            assert hc.lib().hi_bands(cw, N, bands.ctypes.data) == n
            got = [(int(bands[2 * j]), int(bands[2 * j + 1])) for j in range(n)]
            assert got == [M.band(cw, N, j) for j in range(n)], (cw, N)
            # the bands of a cycle cover [0, cw): they start at 0, end at cw, and each starts inside the one before
            assert got[0][0] == 0 and got[-1][1] == cw, (cw, N, got)
            for j in range(n):
                s, e = got[j]
                assert s == 32 * m * j and s % 32 == 0 and s < e <= cw, (cw, N, j)
                if j + 1 < n:
                    # consecutive bands overlap by exactly 16 (the right edge alone is cut by the picture)
                    assert e == s + 32 * m + 16 and got[j + 1][0] + 16 == e and e < cw, (cw, N, j)
                else:
                    assert e == cw
    # the sizes the GPU tests run, by hand
    assert (M.step(320, 5), M.cycle(320, 5)) == (2, 5) and (M.step(320, 10), M.cycle(320, 10)) == (1, 10)
    assert (M.step(256, 8), M.cycle(256, 8)) == (1, 8) and (M.step(640, 4), M.cycle(640, 4)) == (5, 4)
    assert [M.band(320, 5, j) for j in range(5)] == [(0, 80), (64, 144), (128, 208), (192, 272), (256, 320)]


def test_positions_restart_behind_idr_pictures_and_cycles():
    for cw, N in ((320, 5), (320, 10), (256, 8), (640, 4), (1920, 30), (1920, 60), (3840, 255), (64, 2)):
        n = M.cycle(cw, N)
        for poc in range(1, 3 * n + 2):
            assert hc.lib().hi_position(cw, N, poc) == M.position(cw, N, poc) == (poc - 1) % n
        assert M.record(cw, N, 0) == [-1, 0, 0, n] and M.record(cw, N, 1)[0] == 0 and M.record(cw, N, n + 1)[0] == 0 and M.record(cw, N, n)[2] == cw


def test_quarters_bound_and_last_column_match_the_model():
    seen = set()
    for cw, N in ((320, 5), (320, 10), (256, 8), (640, 4), (1920, 30)):
        n = M.cycle(cw, N)
        for j in range(n):
            s, e = M.band(cw, N, j)
            for x0 in range(0, cw, 32):
                q = hc.lib().hi_forced_quarters(x0, s, e)
                assert q == M.forced_quarters(x0, s, e) and q in (0, 5, 15), (cw, N, j, x0, q)
                seen.add(q)
                clean = bool(hc.lib().hi_clean_block(x0, s, j))
                assert clean == M.clean_block(x0, s, j)
                if clean:
                    assert q == 0 and hc.lib().hi_mvx_max(x0, s) == M.mvx_max(x0, s) >= 0      # the zero vector is always admissible
                assert not (q and clean)
                for nb in (8, 16):
                    for xb in range(x0, x0 + 32, nb):
                        assert bool(hc.lib().hi_last_column(xb, nb, e, cw)) == M.last_column(xb, nb, e, cw)
            # the columns of the forced quarters are the band
            cols = sorted({x0 + 16 * (k & 1) for x0 in range(0, cw, 32) for k in range(4) if (M.forced_quarters(x0, s, e) >> k) & 1})
            assert cols == list(range(s, e, 16)), (cw, N, j)
    assert seen == {0, 5, 15}


# ---- 3. syntax
def test_recovery_point_sei_is_the_models():
    for cnt in list(range(0, 255)) + [1000, 32767]:
        rbsp = hc.recovery_sei(cnt)
        assert rbsp == M.recovery_point_sei(cnt), cnt
        assert M.parse_recovery_point(rbsp) == (cnt, 1, 0), cnt


def test_access_units_with_the_option_off_are_the_parents_bytes():
    """recovery -1 (the option off, or a picture that starts no cycle): every access unit is byte for byte the one of the encoder before the option (digests from an
    earlier hevc_headers.h)"""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "tmvp_off_access_units.json")))
    assert len(gold["cases"]) == 700
    for *args, digest in gold["cases"]:
        w, h, lp, sao, wpp, tr, tc, sl, poc = args
        au = hc.access_unit(w, h, poc, recovery=-1, lp=lp, sao=sao, wpp=wpp, tr=tr, tc=tc, slices=sl)
        assert hashlib.sha256(au).hexdigest()[:16] == digest, args


@pytest.mark.parametrize("cfg", [dict(), dict(sao=1), dict(wpp=0), dict(slices=1), dict(weightp=1)], ids=["plain", "sao", "nowpp", "slices", "weightp"])
def test_a_cycles_first_picture_gains_the_sei_and_nothing_else(cfg):
    w, h, N = 320, 192, 5
    n = M.cycle(320, N)
    for poc in range(0, 2 * n + 2):
        for ps in (0, 1):
            off = pyhevc.split_nals(hc.access_unit(w, h, poc, recovery=-1, write_ps=ps, **cfg))
            first = poc >= 1 and M.position(320, N, poc) == 0
            on = pyhevc.split_nals(hc.access_unit(w, h, poc, recovery=n - 1 if first else -1, write_ps=ps, **cfg))
            if not first:
                assert on == off
                continue
            assert len(on) == len(off) + 1
            k = 3 * ps                                          # behind the parameter sets, in front of the first slice segment
            assert on[:k] == off[:k] and on[k + 1:] == off[k:] and nal_type(on[k]) == 39 and on[k][1] == 1
            assert M.parse_recovery_point(pyhevc.unescape(on[k])[2:]) == (n - 1, 1, 0)


def test_the_three_parsers_pass_over_the_sei():
    """a stream of the checker's encoder with the recovery point SEI put in front of the slices of pictures 1 and 4: the decoder's host half parses the same
    pictures, the checker's decoder and tests/pyhevc.py decode the same pictures as without it"""
    import parser_probe
    from deckit import tabs
    w, h, nf = 128, 64, 6
    oe = orc.OracleEncoder(w, h, qp=32, period=64, me_range=8)
    aus, recs = [], []
    for t in range(nf):
        aus.append(oe.encode(orc.synth_frame(0, 1234, w, h, t)))
        recs.append(oe.recon())
    oe.close()
    sei = b"\x00\x00\x00\x01" + bytes([39 << 1, 1]) + hc.recovery_sei(2)
    with_sei = []
    for t, au in enumerate(aus):
        nals = list(orc.split_nals(au))
        if t in (1, 4):
            k = next(i for i, x in enumerate(nals) if nal_type(pyhevc.split_nals(x)[0]) in (1, 19))
            nals.insert(k, sei)
        with_sei.append(b"".join(nals))
    assert sum(len(a) for a in with_sei) == sum(len(a) for a in aus) + 2 * len(sei)
    plain = parser_probe.probe([x for au in aus for x in orc.split_nals(au)], 1)
    got = parser_probe.probe([x for au in with_sei for x in orc.split_nals(au)], 1)
    assert got == plain and got["pictures"] == nf
    od, dec = orc.OracleDecoder(), pyhevc.Decoder(tabs())
    try:
        for t, au in enumerate(with_sei):
            a = od.decode_au(au, t)
            assert len(a) == 1 and np.array_equal(a[0]["i420"], recs[t]), t
            dec.decode(au)
        pics = dec.flush()
        assert len(pics) == nf and all(np.array_equal(p["i420"], recs[t]) for t, p in enumerate(pics))
    finally:
        od.close()


# ---- 4. the control of the recovery test, on the CPU
def test_without_the_option_a_lost_picture_stays_in_the_pictures():
    """what the option is for, measured on the checker's encoder and decoder (no option there: this is the encoder of before): the benchmark clip at 320x192, qp 32,
    access unit 4 of 16 lost -- eleven pictures later the decoded picture still differs from the reconstruction in thousands of luma samples, all over its width"""
    w, h = 320, 192
    oe = orc.OracleEncoder(w, h, qp=32, period=64, me_range=8)
    aus, recs = [], []
    for t in range(16):
        aus.append(oe.encode(orc.synth_frame(0, 1234, w, h, t)))
        recs.append(oe.recon())
    oe.close()
    od = orc.OracleDecoder()
    try:
        for t, au in enumerate(aus):
            if t != 4:
                got = od.decode_au(au, t)
        assert od.concealed() == 1
    finally:
        od.close()
    diff = got[0]["i420"][:w * h].reshape(h, w) != recs[15][:w * h].reshape(h, w)
    print("luma samples that differ in picture 15: %d, in %d of %d columns" % (int(diff.sum()), int(diff.any(axis=0).sum()), w))
    assert diff.sum() > 7000 and diff.any(axis=0).sum() > 300
