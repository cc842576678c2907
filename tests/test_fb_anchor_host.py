"""CPU side of "uvgx loss feedback v2" (kvazaar.h fb_anchor): the option's parsing; the fb_anchor_* functions of hevc_core.h (host build:
tests/hostcheck/anchor.cpp, compiled here into pytest's temporary directory) against the statement of record tests/fb_anchor_model.py -- the anchor rule over every
small case, MaxDpbSize at and around its thresholds, the step through a record with the reference bit --; and the parameter sets and slice segment headers the
host build of hevc_headers.h writes with kept pictures, read back by tests/pyhevc.py."""
import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import fb_anchor_model as A
import fb_model as M
import hc
import pyhevc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ha(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("anchor") / "libanchor.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "hostcheck", "anchor.cpp")], check=True)
    L = C.CDLL(so)
    I, P = C.c_int, C.c_void_p
    for name, res, args in (("ha_max_dpb", I, [I, I]), ("ha_level", I, [I, I]), ("ha_pick", I, [I] * 5), ("ha_kept", I, [I, I]), ("ha_used", I, [I, I]),
                            ("ha_info", None, [P, P, P, I, P]), ("ha_step", None, [P, I, I, P, P, I, I]), ("ha_access_unit", I, [I] * 7 + [P, I])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


# ---- 1. config_parse
def test_config_parse_fb_anchor():
    from kvazzup_amd import _native
    if not os.path.exists(_native.library_path()):
        _native.build_library()
    api = _native.load_library().kvz_api_get(8).contents
    cfg = api.config_alloc()
    api.config_init(cfg)
    ok = lambda k, v: api.config_parse(cfg, k.encode(), v.encode())
    assert cfg.contents.fb_anchor == 0
    for v in (2, 3, 4, 5, 6, 7, 0, 4):
        assert ok("fb-anchor", str(v)) == 1 and cfg.contents.fb_anchor == v, v
    for bad in ("1", "8", "-1", "x", "", "on", "64"):
        assert ok("fb-anchor", bad) == 0 and cfg.contents.fb_anchor == 4, bad
    for preset in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"):
        api.config_init(cfg)
        assert ok("preset", preset) == 1 and cfg.contents.fb_anchor == 0, preset
        assert ok("fb-anchor", "5") == 1 and ok("preset", preset) == 1 and cfg.contents.fb_anchor == 5, preset
    # the field is appended behind loss_feedback: the options before it keep their places
    api.config_init(cfg)
    assert ok("loss-feedback", "9") == 1 and ok("scenecut", "6") == 1 and cfg.contents.fb_anchor == 0 and cfg.contents.loss_feedback == 9 and cfg.contents.scenecut == 6
    assert ok("fb-anchor", "3") == 1 and cfg.contents.loss_feedback == 9 and cfg.contents.scenecut == 6 and cfg.contents.fb_anchor == 3
    api.config_destroy(cfg)


# ---- 2. the anchor rule, every small case
def test_the_anchor_rule_matches_the_model(ha):
    """every clean point c, every non-empty set of up to three pending POCs (the rule reads their least and their age; sets of the same least and oldest agree),
    every heal picture t <= 12, K in 0, 2 .. 7, H in K .. 8 and two rings shorter than the delay"""
    n = v2 = 0
    for t in range(1, 13):
        pend = [s for k in (1, 2, 3) for s in itertools.combinations(range(0, t), k)]
        for c in range(0, t):
            for K in (0, 2, 3, 4, 5, 6, 7):
                for H in sorted({max(K, 1), 8, 3, 1}):
                    for p in pend:
                        want = A.anchor(c, p, t, K, H)
                        got = ha.ha_pick(c, min(p), t, K, H)
                        assert got == (-1 if want is None else want), (c, p, t, K, H, got, want)
                        n += 1
                        v2 += want is not None
    assert v2 > 1000 and n - v2 > 1000, (n, v2)
    # the cases the statement names: in time; too late; in front of the clean point; the IDR picture itself lost
    assert ha.ha_pick(0, 3, 6, 4, 8) == 2 and ha.ha_pick(0, 3, 8, 4, 8) == -1 and ha.ha_pick(6, 2, 9, 4, 8) == -1 and ha.ha_pick(0, 0, 2, 4, 8) == -1
    assert ha.ha_pick(6, 7, 9, 4, 8) == 6                       # the anchor may be the clean point itself


def test_the_kept_set_matches_the_model(ha):
    for K in (2, 3, 4, 7):
        for t in range(1, 13):
            for a in [None] + [x for x in range(max(0, t - K), t - 1)]:
                da = 0 if a is None else t - a
                got = [(-j, ha.ha_used(j, da)) for j in range(1, ha.ha_kept(t, K) + 1)]
                assert got == A.rps(t, K, a), (K, t, a, got)


# ---- 3. MaxDpbSize
def test_max_dpb_size_matches_a42(ha):
    sizes = [(1920, 1088), (3840, 2176), (1280, 768), (320, 320), (128, 64), (8192, 4352)]
    # ... and the coded sizes (multiples of 64) on both sides of each threshold of each level: 1/4, 1/2, 3/4 of MaxLumaPs and MaxLumaPs itself
    for ps in A.MAX_LUMA_PS.values():
        for num in (1, 2, 3, 4):
            for cw in (1024, 2048, 4096, 8192):
                ch = (ps * num // 4) // cw // 64 * 64           # the tallest picture of this width at or under the threshold
                sizes += [(cw, c) for c in (ch - 64, ch, ch + 64) if c >= 64]
    seen = set()
    for cw, ch in sizes:
        if cw * ch > 35651584:
            continue
        assert ha.ha_level(cw, ch) == A.level_idc(cw, ch), (cw, ch)
        assert ha.ha_max_dpb(cw, ch) == A.max_dpb_size(cw, ch), (cw, ch)
        seen.add(A.max_dpb_size(cw, ch))
    assert seen == {6, 8, 12, 16}, seen
    # the sizes the statement names: 1080p and 2160p keep five pictures at the most, 1280x768 and smaller seven
    assert A.max_dpb_size(1920, 1088) == 6 and A.max_dpb_size(3840, 2176) == 6 and A.max_dpb_size(1280, 768) >= 8
    assert A.k_allowed(1920, 1088, 5, 8) and not A.k_allowed(1920, 1088, 6, 8) and A.k_allowed(3840, 2176, 5, 8) and not A.k_allowed(3840, 2176, 6, 8)
    assert A.k_allowed(1280, 768, 7, 8) and A.k_allowed(320, 320, 7, 7) and not A.k_allowed(320, 320, 7, 6) and not A.k_allowed(320, 320, 1, 8) and not A.k_allowed(320, 320, 8, 8)


# ---- 4. the step with the reference bit
def record(rng, cw, ch, p_ref1):
    log2, intra, mv, _, _ = hc.motion_field(rng, cw, ch, 1, 0.12)
    ref = np.zeros(intra.shape, dtype=np.uint8)
    for by in range(ch // 16):                                  # a quarter has one reference
        for bx in range(cw // 16):
            if rng.random() < p_ref1:
                ref[2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = 1
    ref[np.asarray(intra) != 0] = 0
    return np.ascontiguousarray(mv), np.ascontiguousarray(intra), np.ascontiguousarray(log2), ref


def c_step(ha, prev, rec, cw, ch, filt, bad):
    mv, intra, log2, ref = rec
    info = np.zeros(intra.shape, dtype=np.uint8)
    ha.ha_info(intra.ctypes.data, log2.ctypes.data, ref.ctypes.data, intra.size, info.ctypes.data)
    assert np.array_equal((info & A.REF1) != 0, (ref != 0) & (intra == 0))
    d = np.ascontiguousarray(prev, dtype=np.uint8).copy()
    ha.ha_step(d.ctypes.data, cw, ch, mv.ctypes.data, info.ctypes.data, int(filt), int(bad))
    return d


@pytest.mark.parametrize("cw,ch", [(64, 64), (320, 320)])
@pytest.mark.parametrize("bad", [0, 1])
def test_step_with_the_reference_bit_matches_the_model(ha, cw, ch, bad):
    rng = random.Random(cw * 7 + bad)
    hit = 0
    for trial in range(4 if cw > 64 else 24):
        rec = record(rng, cw, ch, (0.0, 0.3, 0.6, 1.0)[trial % 4])
        prev = (np.array([[rng.random() < (0.0, 0.05, 0.3)[trial % 3] for _ in range(cw // 8)] for _ in range(ch // 8)])).astype(np.uint8)
        for filt in (0, 1):
            want = A.step(prev, rec, cw, ch, filt, bad)
            got = c_step(ha, prev, rec, cw, ch, filt, bad)
            assert np.array_equal(got, want), (trial, filt, int((got != want).sum()))
            if not rec[3].any():                                # no reference-1 cell: v1's step
                assert np.array_equal(want, M.step(prev, rec[:3], cw, ch, filt))
            elif not filt:                                      # a reference-1 cell is in S exactly where the anchor is bad
                r1 = (rec[3] != 0) & (rec[1] == 0)
                assert np.array_equal(want[r1] != 0, np.full(int(r1.sum()), bool(bad)))
                hit += int(r1.sum())
    assert hit > 0


# ---- 5. headers
def au(ha, w, h, K, lp, poc, da, ps):
    buf = np.empty(1 << 16, np.uint8)
    n = ha.ha_access_unit(w, h, K, lp, poc, da, ps, buf.ctypes.data, len(buf))
    assert n > 0
    return bytes(buf[:n])


@pytest.mark.parametrize("K", [2, 4, 7])
def test_headers_carry_the_kept_set(ha, K):
    w, h = 320, 320
    hd = A.Headers()
    sh, rps, poc, idr = hd.read(au(ha, w, h, K, 0, 0, 0, 1))
    assert idr and hd.dpb == K and hd.pps["nref_default"] == 1 and len(hd.sps["rps"]) == 1
    vps = [n for n in pyhevc.split_nals(au(ha, w, h, K, 0, 0, 0, 1)) if (n[0] >> 1) & 63 == 32][0]
    for t in range(1, 11):
        # an ordinary picture
        sh, rps, poc, idr = hd.read(au(ha, w, h, K, 0, t, 0, 0))
        assert not idr and poc == t and rps == A.rps(t, K) and sh["nref"] == 1, (t, rps, sh["nref"])
        assert [u for _, u in rps] == [1] + [0] * (min(K, t) - 1)
        # a v2 heal picture with every anchor the set holds
        for a in range(max(0, t - K), t - 1):
            sh, rps, poc, idr = hd.read(au(ha, w, h, K, 0, t, t - a, 0))
            assert poc == t and rps == A.rps(t, K, a) and sh["nref"] == A.active_refs(a) == 2, (t, a, rps, sh["nref"])
            assert [t + d for d, u in rps if u] == [t - 1, a] and sh["list_entry"] == [None, None]
    assert pyhevc.unescape(vps)      # (the VPS states the same buffer: checked against the SPS's bytes below)
    r = pyhevc.Bits(pyhevc.unescape(vps))
    r.u(16), r.u(4), r.u(2), r.u(6)
    max_sub = r.u(3)
    r.u(1), r.u(16)
    pyhevc.parse_ptl(r, max_sub)
    r.u(1)
    assert r.ue() == K


def test_with_k_0_the_bytes_are_those_of_the_writer_of_before(ha):
    for w, h in ((320, 320), (1920, 1080)):
        for poc in range(0, 4):
            assert au(ha, w, h, 0, 1, poc, 0, 1) == hc.access_unit(w, h, poc, lp=1), (w, h, poc)
            assert au(ha, w, h, 0, 0, poc, 0, int(poc == 0)) == hc.access_unit(w, h, poc, lp=0, write_ps=int(poc == 0)), (w, h, poc)
    # ... and with K on, everything behind the slice header's set and count is the same: the slice data of an ordinary picture does not move
    a, b = au(ha, 320, 320, 4, 0, 1, 0, 0), au(ha, 320, 320, 0, 0, 1, 0, 0)
    assert a != b and len(pyhevc.split_nals(a)) == len(pyhevc.split_nals(b))
