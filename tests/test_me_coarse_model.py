"""CPU: "uvgx coarse-to-fine search v1" (kvazaar.h me-coarse) -- the option, the numpy statement tests/me_coarse_model.py, and the
device code's arithmetic built for the host (tests/hostcheck) against that statement."""
import ctypes as C
import os

import numpy as np
import pytest

import hc
import lp_refs_model
import me_coarse_model
import pan_content

# ---- C1: the option
@pytest.fixture(scope="module")
def lib():
    from kvazzup_amd import _native
    if not os.path.exists(_native.library_path()):
        _native.build_library()
    return _native.load_library()


def test_config_parse_me_coarse(lib):
    api = lib.kvz_api_get(8).contents
    cfg = api.config_alloc()
    try:
        assert api.config_init(cfg) == 1
        assert cfg.contents.me_coarse == 0
        ok = lambda k, v: api.config_parse(cfg, k.encode(), v.encode())
        for v in (64, 128, 256, 0):
            assert ok("me-coarse", str(v)) == 1 and cfg.contents.me_coarse == v, v
        assert ok("me-coarse", "128") == 1
        for v in ("32", "100", "-1", "x"):
            assert ok("me-coarse", v) == 0 and cfg.contents.me_coarse == 128, v
        assert api.config_init(cfg) == 1 and cfg.contents.me_coarse == 0
        for p in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"):
            assert ok("preset", p) == 1 and cfg.contents.me_coarse == 0, p
    finally:
        api.config_destroy(cfg)


# ---- C2: the model with the coarse stage off is lp_refs_model.search
def _synth_refs(kind, w, h, frames):
    import orc
    fr = [orc.synth_frame(kind, 0x5EED0000, w, h, t)[:w * h].reshape(h, w) for t in range(frames)]
    return fr


@pytest.mark.parametrize("cfg", [
    dict(w=256, h=128, n=2, R=8, me_early=1, kind=0, frames=5),
    dict(w=192, h=128, n=4, R=6, me_early=0, kind=2, frames=6, qp=37),
    dict(w=256, h=256, n=4, R=8, me_early=1, kind=0, frames=6, tiles="2x2", mv_frame=2),
])
def test_model_without_the_coarse_stage_is_the_lp_refs_model(cfg):
    w, h, n, R, qp = cfg["w"], cfg["h"], cfg["n"], cfg["R"], cfg.get("qp", 32)
    tc, tr = [int(v) for v in cfg.get("tiles", "1x1").split("x")]
    fr = _synth_refs(cfg["kind"], w, h, cfg["frames"])
    t = cfg["frames"] - 1
    refs = [fr[t - 1 - k] for k in range(n)]
    kw = dict(tile_rows=tr, tile_cols=tc, mv_frame=cfg.get("mv_frame", 0), me_early=cfg["me_early"])
    a = lp_refs_model.search(fr[t], refs, qp, R, **kw)
    b = me_coarse_model.search(fr[t], refs, qp, R, me_coarse=0, **kw)
    for x, y in zip(a, b[:3]):
        assert np.array_equal(x, y)
    assert not b[3].any()


# ---- C3: the model on the pan clip
PANS = [((72, -40), 128, 170), ((-100, 24), 128, 176), ((9, 150), 256, 133), ((200, 0), 256, 156)]


def _pan_pair(v):
    f = pan_content.luma_frames(640, 384, 3, v[0], v[1])
    return f[2], f[1]


@pytest.mark.parametrize("v,reach,count", PANS)
def test_model_finds_the_pan(v, reach, count):
    w, h, qp, R = 640, 384, 32, 16
    cur, ref = _pan_pair(v)
    det = {}
    log2, mv, rf, cen = me_coarse_model.search(cur, [ref], qp, R, me_early=1, me_coarse=reach, refs_in=[ref], detail=det)
    inside = pan_content.interior(w, h, v[0], v[1])
    assert int(inside.sum()) == count
    assert not det["early"].any()
    want = np.array([4 * v[0], 4 * v[1]], np.int16)
    bad = [(by, bx, y8, x8, mv[y8, x8].tolist()) for by, bx in np.argwhere(inside) for y8 in range(by * 4, by * 4 + 4) for x8 in range(bx * 4, bx * 4 + 4)
           if not np.array_equal(mv[y8, x8], want)]
    assert not bad, "%d 8x8 units of interior blocks do not carry the pan, first %s" % (len(bad), bad[:4])
    assert (det["cost"] <= det["cost_zero"]).all()


def test_reach_is_what_the_option_says():
    v = (9, 150)
    cur, ref = _pan_pair(v)
    log2, mv, rf, cen = me_coarse_model.search(cur, [ref], 32, 16, me_early=1, me_coarse=128, refs_in=[ref])
    inside = pan_content.interior(640, 384, v[0], v[1])
    hit = [(by, bx) for by, bx in np.argwhere(inside) if (mv[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] == np.array([36, 600], np.int16)).all(axis=2).any()]
    assert not hit, hit
    assert np.abs(cen).max() <= 128


# ---- C4: the device code's arithmetic, built for the host, against the model
def _random_pictures(rng, w, h, n, shift):
    """n pictures of smoothed noise, each the previous one displaced by `shift` plus fresh noise: the search has something to find and ties to break"""
    big = rng.integers(0, 256, (h + 2 * 300, w + 2 * 300)).astype(np.int32)
    big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) >> 2
    out = []
    for t in range(n):
        y, x = 300 + t * shift[1], 300 + t * shift[0]
        out.append(np.clip(big[y:y + h, x:x + w] + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8))
    return out


@pytest.mark.parametrize("cfg", [
    dict(w=256, h=192, n=1, R=8, reach=64, shift=(-37, 22), me_early=1),
    dict(w=256, h=256, n=3, R=6, reach=64, shift=(18, -29), me_early=0, tiles=(2, 2), mv_frame=2, qp=27),
    dict(w=320, h=192, n=2, R=16, reach=128, shift=(90, 5), me_early=0, mv_frame=1, qp=40),
    dict(w=256, h=128, n=2, R=8, reach=256, shift=(0, 0), me_early=1, tiles=(2, 1)),
])
def test_host_build_of_the_device_arithmetic_matches_the_model(cfg):
    L = hc.lib()
    rng = np.random.default_rng(0xC0A25E + cfg["w"] + cfg["reach"])
    w, h, n, R, reach, qp = cfg["w"], cfg["h"], cfg["n"], cfg["R"], cfg["reach"], cfg.get("qp", 32)
    tc, tr = cfg.get("tiles", (1, 1))
    mvf = cfg.get("mv_frame", 0)
    pics = _random_pictures(rng, w, h, n + 1, cfg["shift"])
    cur, refs = pics[n], [pics[n - 1 - k] for k in range(n)]
    recs = [np.clip(r.astype(np.int32) + rng.integers(-3, 4, r.shape), 0, 255).astype(np.uint8) for r in refs]     # what the fine stage searches (reconstructions)
    det = {}
    log2, mv, rf, cen = me_coarse_model.search(cur, recs, qp, R, tile_rows=tr, tile_cols=tc, mv_frame=mvf, me_early=cfg["me_early"], me_coarse=reach,
                                               refs_in=refs, detail=det)
    lam = lp_refs_model.LAMBDA_Q4[qp]
    q = np.zeros((h // 4, w // 4), np.uint8)
    qs = []
    for p in [cur] + refs:
        p = np.ascontiguousarray(p)
        L.hc_quarter(p.ctypes.data, w, h, q.ctypes.data)
        assert np.array_equal(q, me_coarse_model.quarter(p))
        qs.append(q.copy())
    got_c = np.zeros((4, h // 32, w // 32, 2), np.int16)
    for k in range(n):
        L.hc_coarse(qs[0].ctypes.data, qs[1 + k].ctypes.data, w, h, reach // 4, lam, tr, tc, mvf, got_c[k].ctypes.data)
    assert np.array_equal(got_c[:n], cen.astype(np.int16))
    cur_c = np.ascontiguousarray(cur)
    planes = (C.c_void_p * 4)(*[np.ascontiguousarray(r).ctypes.data for r in recs] + [None] * (4 - n))
    recs = [np.ascontiguousarray(r) for r in recs]
    planes = (C.c_void_p * 4)(*([r.ctypes.data for r in recs] + [None] * (4 - n)))
    g_log2 = np.zeros((h // 8, w // 8), np.uint8); g_ref = np.zeros((h // 8, w // 8), np.uint8); g_mv = np.zeros((h // 8, w // 8, 2), np.int16)
    g_early = np.zeros((h // 32, w // 32), np.uint8)
    L.hc_fine(cur_c.ctypes.data, planes, got_c.ctypes.data, w, h, n, R, reach // 4, lam, tr, tc, mvf, cfg["me_early"], g_log2.ctypes.data, g_mv.ctypes.data, g_ref.ctypes.data, g_early.ctypes.data)
    assert np.array_equal(g_early.astype(bool), det["early"])
    assert np.array_equal(g_log2, log2) and np.array_equal(g_ref, rf) and np.array_equal(g_mv, mv)
    if cfg["shift"] != (0, 0):
        assert det["second"].any() and np.abs(mv).max() > 4 * R, "the case does not leave the zero window"
