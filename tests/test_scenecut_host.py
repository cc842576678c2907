"""CPU side of "uvgx scene cut v1" (kvazaar.h scenecut): the option's parsing; the statement functions of hevc_core.h (host build:
tests/hostcheck/scenecut.cpp, compiled here into pytest's temporary directory) against the restatement tests/scenecut_model.py -- random and edge inputs, the
ties of every threshold, whole quarter pictures with their corner blocks --; which pictures are examined; and the model's margin on every clip the GPU tests
(tests/test_gpu_scenecut.py) use."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import enckit
import scenecut_model as M
import wp_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scenecut") / "libscenecut.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "hostcheck", "scenecut.cpp")], check=True)
    L = C.CDLL(so)
    I, P, LL, U = C.c_int, C.c_void_p, C.c_longlong, C.c_uint
    for name, res, args in (("hs_reach", I, [I]), ("hs_visible_blocks", None, [I, I, P]), ("hs_mean_shift", I, [LL, LL, LL]), ("hs_ref_sample", I, [I, I]),
                            ("hs_block_mean", I, [I]), ("hs_is_new", I, [U, U]), ("hs_verdict", I, [I, I]), ("hs_examined", I, [I, I, I]),
                            ("hs_blocks", None, [P, P] + [I] * 6 + [P])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def _blocks(hs, qc, qp, width, height, rq, d):
    bw, bh = M.visible_blocks(width, height)
    out = np.zeros((bh, bw, 2), dtype=np.uint32)
    qc, qp = np.ascontiguousarray(qc, dtype=np.uint8), np.ascontiguousarray(qp, dtype=np.uint8)
    hs.hs_blocks(qc.ctypes.data, qp.ctypes.data, qc.shape[1], qc.shape[0], width, height, rq, d, out.ctypes.data)
    return out


# ---- 1. config_parse
def test_config_parse_scenecut():
    from kvazzup_amd import _native
    if not os.path.exists(_native.library_path()):
        _native.build_library()
    api = _native.load_library().kvz_api_get(8).contents
    cfg = api.config_alloc()
    api.config_init(cfg)
    ok = lambda k, v: api.config_parse(cfg, k.encode(), v.encode())
    assert cfg.contents.scenecut == 0
    for v in (1, 8, 255, 0, 40):
        assert ok("scenecut", str(v)) == 1 and cfg.contents.scenecut == v, v
    for bad in ("256", "-1", "x", "", "on", "1e2", "99999999999999999999"):
        assert ok("scenecut", bad) == 0 and cfg.contents.scenecut == 40, bad
    for preset in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"):
        api.config_init(cfg)
        assert ok("preset", preset) == 1 and cfg.contents.scenecut == 0, preset
        assert ok("scenecut", "8") == 1 and ok("preset", preset) == 1 and cfg.contents.scenecut == 8, preset
    # the field lies behind intra_refresh: the options before it keep their places
    api.config_init(cfg)
    assert ok("intra-refresh", "6") == 1 and ok("weightp", "1") == 1 and cfg.contents.scenecut == 0 and cfg.contents.intra_refresh == 6 and cfg.contents.weightp == 1
    assert ok("scenecut", "3") == 1 and cfg.contents.intra_refresh == 6 and cfg.contents.scenecut == 3
    api.config_destroy(cfg)


# ---- 2. the scalar statement functions against the model
def test_mean_shift_matches_the_model(hs):
    rng = random.Random(0x5CE1)
    cases = [(0, 0, 1), (0, 255, 1), (255, 0, 1), (10, 11, 2), (11, 10, 2), (0, 1, 2), (1, 0, 2), (5, 8, 2), (8, 5, 2), (0, 3, 2), (0, 5, 2)]      # exact halves either side of zero
    n8k = (16384 // 4) ** 2
    cases += [(255 * n8k, 0, n8k), (0, 255 * n8k, n8k), (128 * n8k, 128 * n8k + n8k // 2, n8k), (128 * n8k, 128 * n8k + n8k // 2 + 1, n8k), (128 * n8k, 128 * n8k + n8k // 2 - 1, n8k)]
    for _ in range(20000):
        n = rng.choice((16 * 16, 80 * 48, 480 * 270, rng.randrange(1, 1 << 24)))
        cases.append((rng.randrange(0, 255 * n + 1), rng.randrange(0, 255 * n + 1), n))
    for _ in range(2000):                                   # numerators around the multiples of 2n, negative ones among them
        n = rng.randrange(1, 5000)
        k, e = rng.randrange(-200, 201), rng.choice((-1, 0, 1))
        sp = 255 * n
        sc = sp + (2 * n * k - n + e) // 2 if (2 * n * k - n + e) % 2 == 0 else sp + k * n
        if 0 <= sc <= 255 * n * 2:
            cases.append((sc, sp, n))
    neg = 0
    for sc, sp, n in cases:
        want = M.mean_shift_of_sums(sc, sp, n)
        assert hs.hs_mean_shift(sc, sp, n) == want, (sc, sp, n)
        neg += 2 * (sc - sp) + n < 0
    assert neg > 1000                                      # (negative numerators were covered)
    assert M.mean_shift_of_sums(0, 3, 2) == -1 and M.mean_shift_of_sums(0, 1, 2) == 0 and M.mean_shift_of_sums(0, 5, 2) == -2      # floor, not truncation


def test_thresholds_and_small_functions(hs):
    rng = random.Random(3)
    for A in (0, 1, 500, 16320 - 129, 16320):
        assert hs.hs_is_new(A + 128, A) == 0 and hs.hs_is_new(A + 129, A) == 1 and not M.is_new(A + 128, A) and M.is_new(A + 129, A)
    for _ in range(5000):
        S, A = rng.randrange(0, 16321), rng.randrange(0, 16321)
        assert bool(hs.hs_is_new(S, A)) == bool(M.is_new(S, A)), (S, A)
    for n_b in (1, 2, 4, 59, 60, 104, 2040, 2041):
        for n_new in range(0, n_b + 1):
            assert bool(hs.hs_verdict(n_new, n_b)) == M.verdict(n_new, n_b), (n_new, n_b)
    assert hs.hs_verdict(30, 60) == 0 and hs.hs_verdict(31, 61) == 1 and hs.hs_verdict(31, 60) == 1      # 2 n_new = n_b, = n_b + 1
    for mc, want in ((0, 8), (64, 16), (128, 32), (256, 64)):
        assert hs.hs_reach(mc) == want == M.reach(mc)
    for p in range(256):
        for d in (-255, -41, -1, 0, 1, 8, 255):
            assert hs.hs_ref_sample(p, d) == min(255, max(0, p + d))
    for s in (0, 31, 32, 95, 96, 64 * 255):
        assert hs.hs_block_mean(s) == (s + 32) >> 6


def test_block_counts(hs):
    for (w, h), n in (((64, 64), 4), ((320, 192), 60), ((416, 240), 104), ((1920, 1080), 2040), ((16, 16), 1), ((1928, 1090), 61 * 35)):
        out = (C.c_int * 2)()
        hs.hs_visible_blocks(w, h, out)
        assert (out[0], out[1]) == M.visible_blocks(w, h) and out[0] * out[1] == n, (w, h)
        cw, ch = M.coded_size(w, h)
        assert 32 * out[0] <= cw and 32 * out[1] <= ch     # every block lies inside the quarter picture


def test_examined(hs):
    for N in (0, 1, 2, 8, 255):
        for period in (0, 1, 4, 64):
            for since in range(0, 300):
                periodic = since == 0 or (period > 0 and since % period == 0)
                want = N >= 1 and not periodic and since >= N
                assert bool(hs.hs_examined(since, N, int(periodic))) == want == M.examined(since, N, periodic), (N, period, since)
    # the clips of the GPU tests, by the model's plan: period 4, a cut at 6, N 2; period 64, a cut at 3, N 8
    w, h = 320, 192
    idr = [t for t, (_, _, i) in enumerate(M.run(M.luma_planes(M.cut_clip(w, h, 16, 6), w, h), w, h, 2, 4)) if i]
    assert idr == [0, 4, 6, 10, 14]
    got = M.run(M.luma_planes(M.cut_clip(w, h, 12, 3), w, h), w, h, 8, 64)
    assert [t for t, (_, _, i) in enumerate(got) if i] == [0] and [t for t, (r, _, _) in enumerate(got) if r["examined"]] == [8, 9, 10, 11]


# ---- 3. sc_block_stat against the model on whole quarter pictures
@pytest.mark.parametrize("size", [(64, 64), (320, 192)])
@pytest.mark.parametrize("rq", [8, 16])
def test_block_stat_matches_the_model(hs, size, rq):
    w, h = size
    planes = M.luma_planes(M.cut_clip(w, h, 4, 2), w, h)
    rng = np.random.default_rng(w + rq)
    noise = rng.integers(0, 256, planes[0].shape, dtype=np.uint8)
    edge = np.zeros_like(planes[0]); edge[:, ::2] = 255                # saturating content: the clip of sc_ref_sample on both ends
    pairs = [(planes[1], planes[0], None), (planes[2], planes[1], None), (noise, planes[0], None), (planes[0], noise, 37), (edge, edge[:, ::-1], -90), (edge, edge, 255)]
    seen_new = seen_old = 0
    for cur, prev, d in pairs:
        qc, qp = M.quarter(cur), M.quarter(prev)
        d = M.mean_shift(qc, qp, w, h) if d is None else d
        want = M.blocks(qc, qp, w, h, rq, d)
        got = _blocks(hs, qc, qp, w, h, rq, d)
        assert got.shape == want.shape
        bad = np.argwhere(got.astype(np.int64) != want)
        assert not len(bad), "%d entries differ, first (row, column, S / A) %s: host %s, model %s" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        new = M.is_new(want[..., 0], want[..., 1])
        seen_new += int(new.sum()); seen_old += int((~new).sum())
        corners = [(0, 0), (0, -1), (-1, 0), (-1, -1)]      # the corner blocks were compared (the window's clamping)
        assert all(got[c][0] == want[c][0] for c in corners)
    assert seen_new > 0 and seen_old > 0


def test_quarter_matches_the_product(hs):
    import hc
    w, h = 320, 192
    plane = M.luma_planes(M.bench_clip(w, h, 1), w, h)[0]
    q = np.zeros((plane.shape[0] // 4, plane.shape[1] // 4), dtype=np.uint8)
    hc.lib().hc_quarter(np.ascontiguousarray(plane).ctypes.data, plane.shape[1], plane.shape[0], q.ctypes.data)
    assert np.array_equal(q, M.quarter(plane))


# ---- 4. the model's margin on every clip the GPU tests use (compare() asserts it; here also which side each pair lies on)
def _verdicts(frames, w, h, me_coarse=0):
    planes = M.luma_planes(frames, w, h)
    return [M.compare(planes[t], planes[t - 1], w, h, me_coarse)[0] for t in range(1, len(planes))]


@pytest.mark.parametrize("size", [(64, 64), (320, 192), (416, 240)])
def test_margin_cut_clips(size):
    w, h = size
    recs = _verdicts(M.cut_clip(w, h, 7, 4), w, h)
    assert [r["cut"] for r in recs] == [0, 0, 0, 1, 0, 0], recs
    if size == (320, 192):
        assert [r["cut"] for r in _verdicts(M.cut_clip(w, h, 7, 4), w, h, me_coarse=64)] == [0, 0, 0, 1, 0, 0]
        assert [r["cut"] for r in _verdicts(M.cut_clip(w, h, 10, 5), w, h)] == [0, 0, 0, 0, 1, 0, 0, 0, 0]
        assert [r["cut"] for r in _verdicts(M.cut_clip(w, h, 16, 6), w, h)] == [0] * 5 + [1] + [0] * 9


def test_margin_1080p_pair():
    w, h = 1920, 1080
    f = M.cut_clip(w, h, 2, 1)
    rec = _verdicts(f, w, h)[0]
    assert rec["cut"] == 1 and rec["n_b"] == 2040, rec


def test_margin_clips_without_a_cut():
    w, h, n = 320, 192, 10
    bench = M.bench_clip(w, h, n)
    clips = {"bench": bench, "pan": enckit.pan(w, h, n)}
    for kind in ("offset", "gain", "flash"):
        clips[kind] = wp_model.change(bench, w, h, kind)
    for name, frames in clips.items():
        recs = _verdicts(frames, w, h)
        assert not any(r["cut"] for r in recs), (name, recs)
    assert any(r["d"] <= -5 for r in _verdicts(clips["offset"], w, h))      # (the mean shift is what absorbs the step)
