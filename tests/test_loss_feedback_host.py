"""CPU side of "uvgx loss feedback v1" (kvazaar.h loss_feedback): the option's parsing; the statement functions of hevc_core.h (host build:
tests/hostcheck/feedback.cpp, compiled here into pytest's temporary directory) against the statement of record tests/fb_model.py -- seed, step and block records
on random motion fields and on the edge cases --; the model's own properties; and the check of the claim: on the checker's encoder's pictures, decoded with a
loss by tests/partial_model.py and the checker's decoder, every cell in which a decoder's picture differs from the reconstruction lies inside the model's map."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import deckit
import enckit
import fb_model as M
import hc
import orc
import partial_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(256, 128), (320, 320), (200, 120)]


def coded(w, h):
    return max(128, (w + 63) & ~63), (h + 63) & ~63


@pytest.fixture(scope="module")
def hf(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("feedback") / "libfeedback.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "hostcheck", "feedback.cpp")], check=True)
    L = C.CDLL(so)
    I, P = C.c_int, C.c_void_p
    for name, res, args in (("hf_seed", None, [P, I, I, I, I, I]), ("hf_step", None, [P, I, I, P, P, I]), ("hf_info", None, [P, P, I, I, P]),
                            ("hf_blocks", None, [P, I, I, I, P]), ("hf_reach", I, [I])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


# ---- the host build's calls in the model's vocabulary
def c_seed(hf, cw, ch, reports, filt):
    d = np.zeros((ch // 8, cw // 8), dtype=np.uint8)
    for first, count in reports:
        hf.hf_seed(d.ctypes.data, cw, ch, first, count, int(filt))
    return d


def c_step(hf, prev, record, cw, ch, filt, clean=False):
    mv, intra, log2 = (np.ascontiguousarray(a) for a in record)
    info = np.zeros(intra.shape, dtype=np.uint8)
    hf.hf_info(intra.ctypes.data, log2.ctypes.data, intra.size, int(clean), info.ctypes.data)
    d = np.ascontiguousarray(prev, dtype=np.uint8).copy()
    hf.hf_step(d.ctypes.data, cw, ch, mv.ctypes.data, info.ctypes.data, int(filt))
    return d


def c_blocks(hf, d, cw, ch, me_range):
    out = np.zeros((ch // 32, cw // 32, 2), dtype=np.uint8)
    d = np.ascontiguousarray(d, dtype=np.uint8)
    hf.hf_blocks(d.ctypes.data, cw, ch, me_range, out.ctypes.data)
    return out


def record(rng, cw, ch, p_intra=0.12):
    log2, intra, mv, _, _ = hc.motion_field(rng, cw, ch, 1, p_intra)
    return mv, intra, log2


def random_map(rng, cw, ch, p):
    return (np.array([[rng.random() < p for _ in range(cw // 8)] for _ in range(ch // 8)])).astype(np.uint8)


# ---- 1. config_parse
def test_config_parse_loss_feedback():
    from kvazzup_amd import _native
    if not os.path.exists(_native.library_path()):
        _native.build_library()
    api = _native.load_library().kvz_api_get(8).contents
    cfg = api.config_alloc()
    api.config_init(cfg)
    ok = lambda k, v: api.config_parse(cfg, k.encode(), v.encode())
    assert cfg.contents.loss_feedback == 0
    for v in (1, 8, 64, 0, 17):
        assert ok("loss-feedback", str(v)) == 1 and cfg.contents.loss_feedback == v, v
    for bad in ("65", "-1", "x", "", "on", "1e1", "99999999999999999999"):
        assert ok("loss-feedback", bad) == 0 and cfg.contents.loss_feedback == 17, bad
    for preset in ("ultrafast", "superfast", "veryfast", "faster", "fast", "medium", "slow", "slower", "veryslow", "placebo"):
        api.config_init(cfg)
        assert ok("preset", preset) == 1 and cfg.contents.loss_feedback == 0, preset
        assert ok("loss-feedback", "8") == 1 and ok("preset", preset) == 1 and cfg.contents.loss_feedback == 8, preset
    # the field is appended: the options before it keep their places
    api.config_init(cfg)
    assert ok("scenecut", "6") == 1 and ok("input-format", "yuyv") == 1 and cfg.contents.loss_feedback == 0 and cfg.contents.scenecut == 6 and cfg.contents.input_format == 3
    assert ok("loss-feedback", "3") == 1 and cfg.contents.scenecut == 6 and cfg.contents.input_format == 3 and cfg.contents.loss_feedback == 3
    api.config_destroy(cfg)


# ---- 2. the statement functions against the model
@pytest.mark.parametrize("w,h", SIZES)
def test_seed_matches_the_model(hf, w, h):
    cw, ch = coded(w, h)
    n = (cw // 64) * (ch // 64)
    for filt in (0, 1):
        for reports in ([(0, 1)], [(n - 1, 1)], [(1, 3)], [(0, n)], [(0, -1)], [(2, 0)], [(0, 1), (n - 2, 2)], [(cw // 64, cw // 64)]):
            assert np.array_equal(c_seed(hf, cw, ch, reports, filt), M.seed(cw, ch, reports, filt)), (filt, reports)
    assert not c_seed(hf, cw, ch, [], 1).any()


@pytest.mark.parametrize("w,h", SIZES)
def test_step_and_block_records_match_the_model_on_random_motion(hf, w, h):
    cw, ch = coded(w, h)
    rng = random.Random(0xFB00 + w)
    for trial in range(6):
        filt = trial & 1
        d = random_map(rng, cw, ch, (0.02, 0.1, 0.4)[trial % 3])
        for _ in range(3):                                   # three pictures in a row: the map of one is the input of the next
            rec = record(rng, cw, ch, p_intra=(0.12, 0.5)[trial >= 4])
            want = M.step(d, rec, cw, ch, filt)
            assert np.array_equal(c_step(hf, d, rec, cw, ch, filt), want), (trial, filt)
            d = want
            for R in (1, 8, 16, 32):
                assert np.array_equal(c_blocks(hf, d, cw, ch, R), M.block_records(d, cw, ch, R)), (trial, R)


@pytest.mark.parametrize("w,h", SIZES)
def test_edge_cases_match_the_model(hf, w, h):
    cw, ch = coded(w, h)
    gh, gw = ch // 8, cw // 8
    rng = random.Random(0xED6E)
    empty, full = np.zeros((gh, gw), np.uint8), np.ones((gh, gw), np.uint8)
    rec = record(rng, cw, ch)
    for filt in (0, 1):
        # an empty map and a full map
        assert not c_step(hf, empty, rec, cw, ch, filt).any() and not M.step(empty, rec, cw, ch, filt).any()
        assert np.array_equal(c_step(hf, full, rec, cw, ch, filt), M.step(full, rec, cw, ch, filt))
        for R in (4, 16):
            assert np.array_equal(c_blocks(hf, empty, cw, ch, R), M.block_records(empty, cw, ch, R))
            assert np.array_equal(c_blocks(hf, full, cw, ch, R), M.block_records(full, cw, ch, R))
        # vectors leaving the picture on every side: the corner cells are read through the clamp
        for mvx, mvy in ((-4 * cw, 0), (4 * cw, 0), (0, -4 * ch), (0, 4 * ch), (-4 * cw - 3, 4 * ch + 1), (32767, -32768), (-32768, 32767)):
            mv = np.zeros((gh, gw, 2), np.int16)
            mv[..., 0], mv[..., 1] = mvx, mvy
            inter = (mv, np.zeros((gh, gw), np.uint8), np.full((gh, gw), 4, np.uint8))
            for cy, cx in ((0, 0), (0, gw - 1), (gh - 1, 0), (gh - 1, gw - 1)):
                d = empty.copy()
                d[cy, cx] = 1
                assert np.array_equal(c_step(hf, d, inter, cw, ch, filt), M.step(d, inter, cw, ch, filt)), (mvx, mvy, cy, cx)
        # an intra chain along a whole row: 16x16 intra units from edge to edge, one inter cell at the left end reads the damage -- the whole row follows
        intra = np.zeros((gh, gw), np.uint8)
        intra[2:4, 2:] = 1
        log2 = np.full((gh, gw), 4, np.uint8)
        chain = (np.zeros((gh, gw, 2), np.int16), intra, log2)
        d = empty.copy()
        d[2, 1] = 1
        got = c_step(hf, d, chain, cw, ch, filt)
        assert np.array_equal(got, M.step(d, chain, cw, ch, filt))
        assert got[2:4, 2:].all(), "the chain did not reach the end of the row"
    assert [hf.hf_reach(c) for c in (0, 4, 32, 0xff)] == [0, 4, 32, 0] == [M.reach_of(c) for c in (0, 4, 32, 0xff)]


# ---- 3. the model's properties
def test_model_properties():
    cw, ch = 256, 128
    gh, gw = ch // 8, cw // 8
    rng = random.Random(0x9807)
    for trial in range(8):
        filt = trial & 1
        rec = record(rng, cw, ch, p_intra=0.3)
        a = random_map(rng, cw, ch, 0.05)
        b = a | random_map(rng, cw, ch, 0.05)
        sa, sb = M.step(a, rec, cw, ch, filt), M.step(b, rec, cw, ch, filt)
        assert not M.step(np.zeros((gh, gw), np.uint8), rec, cw, ch, filt).any(), "no damage in, damage out"
        assert not (sa & ~sb & 1).any(), "not monotone in the input map"
        assert not M.step(b, rec, cw, ch, filt, clean=True).any(), "an IDR record left damage"
        for R in (4, 16, 32):
            blk = M.block_records(sb, cw, ch, R)
            # the zero vector is admissible for every free quarter: a free quarter holds no cell of the map, and reads nothing else with the zero vector
            for by in range(ch // 32):
                for bx in range(cw // 32):
                    for k in range(4):
                        if not (blk[by, bx, 0] >> k) & 1:
                            qy, qx = 2 * by + (k >> 1), 2 * bx + (k & 1)
                            assert not sb[2 * qy:2 * qy + 2, 2 * qx:2 * qx + 2].any()
                    assert M.vector_within((0, 0), blk[by, bx, 1])
                    assert blk[by, bx, 1] == M.ZERO_ONLY or blk[by, bx, 1] in {min(R, 8 * k - 4) for k in range(1, R // 8 + 3)}, (R, blk[by, bx, 1])      # min(me-range, d - 4) at a distance d = 8 k
    # a vector at the reach reads no cell of the map: every free quarter moved by (+-r, +-r) full samples, and by the largest fraction inside, stays clean
    d = random_map(rng, cw, ch, 0.03)
    blk = M.block_records(d, cw, ch, 32)
    for by in range(ch // 32):
        for bx in range(cw // 32):
            r = M.reach_of(blk[by, bx, 1])
            for k in range(4):
                if (blk[by, bx, 0] >> k) & 1:
                    continue
                for cy in range(2):
                    for cx in range(2):
                        X, Y = 4 * bx + 2 * (k & 1) + cx, 4 * by + 2 * (k >> 1) + cy
                        for mx, my in ((4 * r, 4 * r), (-4 * r, 4 * r), (4 * r, -4 * r), (-4 * r, -4 * r), (4 * r - 1, 1 - 4 * r) if r else (0, 0)):
                            assert not M.inter_reads(d, cw, ch, X, Y, mx, my), (bx, by, k, mx, my)


def test_heal_map_folds_reports_and_fills_past_the_ring():
    cw, ch = 256, 128
    rng = random.Random(0x600D)
    recs = {k: record(rng, cw, ch) for k in range(1, 12)}
    one = M.heal_map(cw, ch, recs, [(3, 0, 2)], 6, 8, 1)
    two = M.heal_map(cw, ch, recs, [(3, 0, 2), (4, 5, 1)], 6, 8, 1)
    assert not (one & ~two & 1).any() and (two != one).any()
    assert np.array_equal(two, M.heal_map(cw, ch, recs, [(4, 5, 1), (3, 0, 2)], 6, 8, 1))
    still = (np.zeros((ch // 8, cw // 8, 2), np.int16), np.zeros((ch // 8, cw // 8), np.uint8), np.full((ch // 8, cw // 8), 5, np.uint8))
    stills = {k: still for k in range(1, 12)}
    assert M.heal_map(cw, ch, stills, [(2, 0, 1)], 11, 8, 0).all(), "a report H + 1 pictures back did not fill the map"
    assert np.array_equal(M.heal_map(cw, ch, stills, [(3, 0, 1)], 11, 8, 0), M.seed(cw, ch, [(0, 1)], 0)), "a report H pictures back: a still picture keeps the seed"
    assert np.array_equal(M.heal_map(cw, ch, recs, [(5, 1, 1)], 6, 8, 1), M.seed(cw, ch, [(1, 1)], 1))      # one picture late: the seed itself


# ---- 4. the check of the claim: the map covers what a decoder gets wrong
W = H = 320
LOST = 2


@functools.lru_cache(maxsize=None)
def checker_stream(dx, dy):
    oe = enckit.oracle_encoder(W, H, qp=30, period=64, me_range=16, subme=2, sao=1, slices=1, opts=(("intra-in-p", 1),))
    out = []
    try:
        for f in enckit.pan(W, H, 8, dx, dy):
            au = oe.encode(f)
            d = oe.debug()
            out.append((au, oe.recon().copy(), (d["cu_mv"].copy(), d["cu_intra"].copy(), d["cu_log2"].copy())))
    finally:
        oe.close()
    return out


def differing_cells(a, b):
    """the cells in which two I420 pictures differ in any plane"""
    out = np.zeros((H // 8, W // 8), dtype=bool)
    for pa, pb, n in zip(enckit.planes(a, W, H), enckit.planes(b, W, H), (8, 4, 4)):
        d = pa != pb
        out |= d.reshape(d.shape[0] // n, n, d.shape[1] // n, n).any(axis=(1, 3))
    return out


def damaged_pictures(dx, dy, loss, mode):
    st = checker_stream(dx, dy)
    aus = [au for au, _, _ in st]
    rows = H // 64
    assert all(len(pm.vcl_indices(au)) == rows for au in aus)
    if loss == "whole":
        od = orc.OracleDecoder()
        try:
            pics = [f for t, au in enumerate(aus) if t != LOST for f in od.decode_au(au, t)] + od.flush()
            assert od.concealed() > 0
        finally:
            od.close()
        return {p["poc"]: p["i420"] for p in pics}, [(0, -1)]
    row = rows - 1 if loss == "last" else 3
    pics, d = pm.decode([au for _, au in pm.cut(aus, {LOST: (row,)})], deckit.tabs(), mode)
    assert len(d.damage) == 1 and d.damage[0]["poc"] == LOST
    return {p["poc"]: p["i420"] for p in pics}, d.damage[0]["runs"]


@pytest.mark.parametrize("loss,mode", [("last", 2), ("last", 3), ("row3", 2), ("row3", 3), ("whole", 0)])
@pytest.mark.parametrize("dx,dy", [(12, -6), (4, 6)])
def test_the_map_covers_what_a_decoder_gets_wrong(dx, dy, loss, mode):
    st = checker_stream(dx, dy)
    pics, runs = damaged_pictures(dx, dy, loss, mode)
    d = M.seed(W, H, runs, 1)
    for k in range(LOST, len(st)):
        if k > LOST:
            d = M.step(d, st[k][2], W, H, 1)
        if k not in pics:                                # (the access unit that never arrived)
            continue
        diff = differing_cells(pics[k], st[k][1])
        outside = diff & (d == 0)
        print("(%d, %d) %s mode %d picture %d: %d cells differ, %d in the map of %d, %d outside" % (dx, dy, loss, mode, k, diff.sum(), int((d != 0).sum()), d.size, outside.sum()))
        assert not outside.any(), "picture %d: %d cells differ outside the map, first (row, column) %s" % (k, outside.sum(), np.argwhere(outside)[0].tolist())
        if k == LOST + 1:
            assert diff.any(), "the picture behind the loss does not differ: the case shows nothing"
        if loss == "last" and k == LOST + 3:
            assert (d != 0).sum() <= 0.8 * d.size, "%d of %d cells are in the map three pictures after the loss" % ((d != 0).sum(), d.size)
