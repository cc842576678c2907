"""The interleaved host arithmetic coder (entropy_host.h cabac_play_rows_host<K>, EntropyHost with K lanes) against the coder that codes
one substream at a time (cabac_play_tokens_host): identical substream bytes and bin counts for K = 1..4.  CPU only."""
import ctypes as C
import functools

import numpy as np
import pytest

import hc
import hcr
import orc

LANES = (1, 2, 3, 4)
BYPASS, TERM = 0x8000, 0xC000


@functools.lru_cache(maxsize=None)
def picture_tokens(w, h, t):
    """tokens of picture t (0: IDR, 2: P) of the oracle encoder's synthetic clip, cut into CTUs -> (tokens, count, offset, wc, hc)"""
    oe = orc.OracleEncoder(w, h, qp=32, period=64, me_range=16)
    for i in range(t + 1):
        oe.encode(orc.synth_frame(0, 0x5EED0000, w, h, i))
    dbg = oe.debug()
    f, hold = hc.make_frame(dbg, w, h, 32)
    L = hc.lib()
    tok = np.zeros(8 << 20, dtype=np.uint16)
    n = L.hc_picture_tokens(C.byref(f), tok.ctypes.data, len(tok))
    assert 0 < n < len(tok)
    tok = tok[:n].copy()
    # a CTU ends with end_of_slice_segment_flag (a terminating bin), at the end of a WPP row followed by end_of_subset_one_bit
    term = (tok & 0xC000) == 0xC000
    ends = np.nonzero(term & ~np.append(term[1:], False))[0] + 1
    wc, hcn = dbg["coded_w"] // 64, dbg["coded_h"] // 64
    assert len(ends) == wc * hcn
    offset = np.concatenate(([0], ends[:-1])).astype(np.uint32)
    count = np.diff(np.concatenate(([0], ends))).astype(np.int32)
    return tok, count, offset, wc, hcn


def same_for_all_lanes(code):
    ref = code(1)
    assert len(ref[0]) >= 1 and ref[1] > 0
    for k in LANES[1:]:
        got = code(k)
        assert len(got[0]) == len(ref[0])
        for r, (a, b) in enumerate(zip(got[0], ref[0])):
            assert a == b, "lanes %d: substream %d differs" % (k, r)
        assert got[1] == ref[1], "lanes %d: bins %d, expected %d" % (k, got[1], ref[1])
    return ref


@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160)], ids=["1080p", "2160p"])
@pytest.mark.parametrize("t", [0, 2], ids=["idr", "p"])
@pytest.mark.parametrize("wpp,tile_rows,tile_cols", [(1, 1, 1), (0, 1, 1), (0, 2, 2), (1, 2, 2)], ids=["wpp", "single", "tiles2x2", "wpp-tiles2x2"])
def test_picture(size, t, wpp, tile_rows, tile_cols):
    tok, count, offset, wc, hcn = picture_tokens(size[0], size[1], t)
    rows, _ = same_for_all_lanes(lambda k: hcr.code_picture(k, tok, count, offset, wc, hcn, wpp, tile_rows, tile_cols, init_type=0 if t == 0 else 1))
    assert len(rows) == (hcn * tile_cols if wpp else tile_rows * tile_cols)


@pytest.mark.parametrize("wpp", [1, 0])
def test_one_ctu_wide_tiles(wpp):
    tok, count, offset, wc, hcn = picture_tokens(1920, 1080, 2)
    assert wc == 30
    # 20 tile columns over 30 CTUs: ten of them one CTU wide (their WPP rows all start from the initial contexts)
    rows, _ = same_for_all_lanes(lambda k: hcr.code_picture(k, tok, count, offset, wc, hcn, wpp, 1, 20))
    assert len(rows) == (hcn * 20 if wpp else 20)


@pytest.mark.parametrize("wpp,tile_rows,row0,nrows", [(1, 4, 0, 9), (1, 4, 9, 8), (1, 4, 17, 17), (0, 4, 0, 17), (0, 4, 17, 17)])
def test_band(wpp, tile_rows, row0, nrows):
    tok, count, offset, wc, hcn = picture_tokens(3840, 2160, 2)
    same_for_all_lanes(lambda k: hcr.code_band(k, tok, count, offset, wc, hcn, wpp, tile_rows, row0, nrows))


@pytest.mark.parametrize("threads", [1, 4])
def test_unequal_rows(threads):
    """rows of very unequal length: one row all bypass tokens, one row without a token, one row eight times the rest"""
    tok, count, offset, wc, hcn = picture_tokens(1920, 1080, 2)
    rng = np.random.default_rng(7)
    parts, cnt = [], np.zeros(wc * hcn, dtype=np.int32)
    for cy in range(hcn):
        for cx in range(wc):
            i = cy * wc + cx
            base = tok[offset[i]:offset[i] + count[i]]
            if cy == 3:
                base = (BYPASS | (rng.integers(0, 16, len(base)) << 10) | rng.integers(0, 1024, len(base))).astype(np.uint16)
            elif cy == 5:
                base = base[:0]
            elif cy == 8:
                base = np.tile(base, 8)
            parts.append(base)
            cnt[i] = len(base)
    t2 = np.concatenate(parts).astype(np.uint16)
    off = np.concatenate(([0], np.cumsum(cnt)[:-1])).astype(np.uint32)
    assert cnt.sum() >= 16000                      # (the pool path; the serial one is below)
    same_for_all_lanes(lambda k: hcr.code_picture(k, t2, cnt, off, wc, hcn, 1, threads=threads))
    # a still picture: few tokens, coded on the calling thread
    small = np.minimum(cnt, 12).astype(np.int32)
    small[5 * wc:6 * wc] = 0
    assert small.sum() < 16000
    same_for_all_lanes(lambda k: hcr.code_picture(k, t2, small, off, wc, hcn, 1, threads=threads))


def random_tokens(rng, n, p_bypass, p_term):
    u = rng.random(n)
    regular = (rng.integers(0, 154, n) << 1) | rng.integers(0, 2, n)
    nbits = rng.integers(0, 16, n)
    # bypass values: half of them all ones (long runs of 0xff in the coder's low register, carried through by cabac_write_out)
    val = np.where(rng.random(n) < 0.5, (1 << (nbits + 1)) - 1, rng.integers(0, 1 << 16, n) & ((1 << (nbits + 1)) - 1))
    bypass = BYPASS | (nbits << 10) | (val & 0x3FF)
    term = TERM | rng.integers(0, 2, n)
    return np.where(u < p_term, term, np.where(u < p_term + p_bypass, bypass, regular)).astype(np.uint16)


@pytest.mark.parametrize("seed", range(6))
def test_random_streams(seed):
    rng = np.random.default_rng(seed)
    nsub = int(rng.integers(1, 12))
    subs = []
    for _ in range(nsub):
        runs = []
        for _ in range(int(rng.integers(0, 8))):
            runs.append(random_tokens(rng, int(rng.integers(0, 3000)), p_bypass=float(rng.random()), p_term=float(rng.random()) * 0.1))
        subs.append(runs)
    ctx0 = rng.integers(0, 126, (nsub, hcr.CTX_COUNT)).astype(np.uint8)
    ref = hcr.play(0, subs, ctx0)
    for k in LANES:
        assert hcr.play(k, subs, ctx0) == ref, "lanes %d" % k


def test_carry_through_ff_runs():
    """streams dense in all-ones bypass values: cabac_write_out buffers runs of 0xff bytes until a byte without them (or a carry) settles them"""
    rng = np.random.default_rng(99)
    subs = []
    for s in range(7):
        runs = []
        for _ in range(20):
            r = random_tokens(rng, 400, p_bypass=0.9, p_term=0.02)
            runs.append(r)
        subs.append(runs)
    ctx0 = np.tile(np.arange(hcr.CTX_COUNT, dtype=np.uint8) % 126, (len(subs), 1))
    ref = hcr.play(0, subs, ctx0)
    assert sum(b.count(b"\xff\xff\xff") for b, _ in ref) > 10
    for k in LANES:
        assert hcr.play(k, subs, ctx0) == ref, "lanes %d" % k
