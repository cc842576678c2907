"""CPU side of "tmvp" (temporal motion vector prediction): the option's parsing, the parameter sets and slice segment headers with
the temporal flags read back bit by bit and with tests/pyhevc.py, byte equality of every header with tmvp off against what the encoder wrote before the
option existed (tests/golden/tmvp_off_access_units.json), and the merge / AMVP derivation of hevc_core.h with a collocated record (host build:
tests/hosttmvp) against pyhevc's SliceDecoder.merge_candidates / amvp_candidates / temporal on random motion fields."""
import ctypes as C
import fcntl
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import pyhevc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def ht():
    global _LIB
    if _LIB is None:
        d = os.path.join(ROOT, "tests", "hosttmvp")
        with open(os.path.join(d, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.run(["make", "-s", "-C", d], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(d, "build", "libhosttmvp.so"))
        P = C.c_void_p
        L.ht_access_unit.argtypes = [C.c_int] * 10 + [P, C.c_int]
        L.ht_cands.argtypes = [C.c_int] * 5 + [P] * 6 + [C.c_int] * 3 + [P] * 3
        L.ht_picture.argtypes = [C.c_int] * 5 + [P] * 6 + [P] * 5
        _LIB = L
    return _LIB


def access_unit(w, h, lp, tmvp, sao, wpp, tr, tc, slices, poc):
    buf = np.zeros(1 << 16, np.uint8)
    n = ht().ht_access_unit(w, h, lp, tmvp, sao, wpp, tr, tc, slices, poc, buf.ctypes.data, len(buf))
    assert n > 0
    return bytes(buf[:n])


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
FORMS = ((1, 1, 1, 0), (1, 1, 1, 1), (0, 2, 2, 2), (1, 2, 1, 2), (0, 1, 1, 0))     # (wpp, tile rows, tile columns, slices): WPP, slices=wpp, tiles 2x2 with slices=tiles, ...


def test_headers_with_tmvp_off_are_unchanged():
    """every access unit's headers with tmvp=0 are byte for byte the ones of the encoder before the option (digests from the parent's hevc_headers.h)"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "tmvp_off_access_units.json")))
    assert len(g["cases"]) == 700
    for *args, digest in g["cases"]:
        w, h, lp, sao, wpp, tr, tc, sl, poc = args
        au = access_unit(w, h, lp, 0, sao, wpp, tr, tc, sl, poc)
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
                assert all(r.u(ln) + 1 == 2 for _ in range(n))      # the 2-byte substreams hosttmvp gives every segment
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
            au = access_unit(256, 192, lp, 1, sao, wpp, tr, tc, sl, poc)
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
    au = access_unit(256, 192, lp, 0, 0, wpp, tr, tc, sl, 0)
    assert pyhevc.parse_sps(pyhevc.unescape(pyhevc.split_nals(au)[1]))["tmvp"] == 0


# ---- 3. merge / AMVP with the temporal candidate against pyhevc's derivation
class _Pic:
    pass


class _Ref:
    def __init__(self, poc):
        self.poc, self.is_lt = poc, False


def _col_picture(poc, intra, mv, ref):
    """pyhevc's view of the collocated picture: list-0 motion per 4x4 block, intra blocks with no list"""
    p = _Pic()
    p.poc, p.is_lt = poc, False
    h4, w4 = intra.shape[0] * 2, intra.shape[1] * 2
    up = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)
    p.mv = np.zeros((h4, w4, 2, 2), np.int32)
    p.mv[:, :, 0, :] = up(mv)
    p.ref_idx = np.full((h4, w4, 2), -1, np.int32)
    p.ref_idx[:, :, 0] = np.where(up(intra) != 0, -1, up(ref).astype(np.int32))
    p.ref_poc = np.zeros((h4, w4, 2), np.int32)
    p.ref_poc[:, :, 0] = poc - 1 - up(ref).astype(np.int32)
    p.ref_lt = np.zeros((h4, w4, 2), np.int32)
    return p


def col_record(intra, mv, ref):
    """the record a picture files (hevc_core.h ColMv): its top-left 8x8 unit's motion for every 16x16 block, distance 0 for intra"""
    i, m, r = intra[::2, ::2], mv[::2, ::2], ref[::2, ::2]
    rec = np.zeros(i.shape + (4,), np.int16)
    rec[..., 0] = np.where(i != 0, 0, m[..., 0])
    rec[..., 1] = np.where(i != 0, 0, m[..., 1])
    rec[..., 2] = np.where(i != 0, 0, r.astype(np.int16) + 1)
    return np.ascontiguousarray(rec)


class _Stub:
    """the state pyhevc.SliceDecoder's merge / AMVP / temporal derivations read, filled from one motion field and the collocated picture's"""
    merge_candidates = pyhevc.SliceDecoder.merge_candidates
    amvp_candidates = pyhevc.SliceDecoder.amvp_candidates
    pb_avail = pyhevc.SliceDecoder.pb_avail
    avail = pyhevc.SliceDecoder.avail
    zaddr = pyhevc.SliceDecoder.zaddr
    motion = pyhevc.SliceDecoder.motion
    temporal = pyhevc.SliceDecoder.temporal
    scale = staticmethod(pyhevc.SliceDecoder.scale)

    def __init__(self, cw, ch, tr, tc, nref, intra, mv, ref, col, poc):
        self.w, self.h, self.ctb_log2, self.ctb, self.wc = cw, ch, 6, 64, cw // 64
        rows, cols = ch // 64, cw // 64
        self.tile_of_row = [next(i for i in range(tr) if (i * rows) // tr <= y < ((i + 1) * rows) // tr) for y in range(rows)]
        self.tile_of_col = [next(i for i in range(tc) if (i * cols) // tc <= x < ((i + 1) * cols) // tc) for x in range(cols)]
        self.ctb_slice = [-1] * (rows * cols)
        self.sps = {"min_cb": 3}
        self.pps = {"par_mrg": 2}
        self.cu_pred = intra.astype(np.int32)
        self.pic = _Pic()
        self.pic.mv = np.zeros((ch // 4, cw // 4, 2, 2), np.int32)
        self.pic.mv[:, :, 0, :] = np.repeat(np.repeat(mv, 2, 0), 2, 1)
        self.pic.ref_idx = np.full((ch // 4, cw // 4, 2), -1, np.int32)
        self.pic.ref_idx[:, :, 0] = np.repeat(np.repeat(ref, 2, 0), 2, 1)
        self.refs = [[col if (k == 0 and col is not None) else _Ref(poc - 1 - k) for k in range(nref)], []]
        self.sh = {"poc": poc, "max_merge": 5, "b": False, "nref": nref, "tmvp": col is not None, "col_idx": 0, "col_l0": 1}


def motion_field(rng, cw, ch, nref, p_intra=0.12):
    """a random quadtree of 32x32 / 16x16 / 8x8 units: some intra, vectors from a small set (so that neighbours and collocated blocks often agree), random references"""
    b8h, b8w = ch // 8, cw // 8
    log2 = np.zeros((b8h, b8w), np.uint8); intra = np.zeros_like(log2); ref = np.zeros_like(log2); cbf = np.zeros_like(log2)
    mv = np.zeros((b8h, b8w, 2), np.int16)
    pool = [(0, 0), (4, 0), (-8, 4), (12, -4), (4, 0), (3, -1), (-33, 17), (100, -60), (8, 0), (-2, 6)]
    for y in range(0, ch, 32):
        for x in range(0, cw, 32):
            l = rng.choice((5, 4, 4, 3))
            for yy in range(y, y + 32, 1 << l):
                for xx in range(x, x + 32, 1 << l):
                    s = (slice(yy // 8, (yy + (1 << l)) // 8), slice(xx // 8, (xx + (1 << l)) // 8))
                    log2[s] = l
                    intra[s] = rng.random() < p_intra
                    mv[s] = pool[rng.randrange(len(pool))] if rng.random() < 0.8 else (rng.randrange(-300, 300), rng.randrange(-150, 150))
                    ref[s] = rng.randrange(nref)
                    cbf[s] = rng.random() < 0.5
    mv[intra != 0] = 0
    return log2, intra, mv, ref, cbf


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
    stub = _Stub(cw, ch, tr, tc, nref, intra, mv, ref, _col_picture(poc - 1, cintra, cmv, cref), poc)
    merge = np.zeros(15, np.int32); amvp = np.zeros(4, np.int32); sig = np.zeros(5, np.int32)
    a = [np.ascontiguousarray(x) for x in (log2, intra, mv, ref, cbf)]
    seen = {"merge_t": 0, "amvp_t": 0, "scaled": 0, "br_out_row": 0, "br_out_pic": 0, "col_intra": 0, "n16": 0, "n32": 0, "merged_t": 0}
    for y in range(0, ch, 8):
        for x in range(0, cw, 8):
            l = int(log2[y // 8, x // 8])
            if intra[y // 8, x // 8] or (x | y) & ((1 << l) - 1):
                continue
            n = 1 << l
            ht().ht_cands(cw, ch, tr, tc, nref, *[v.ctypes.data for v in a], col.ctypes.data, x, y, l, merge.ctypes.data, amvp.ctypes.data, sig.ctypes.data)
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
    """without a collocated record the lists are pyhevc's with slice_temporal_mvp_enabled_flag 0 (what tests/hostrefs pins for the encoder of before)"""
    rng = random.Random(seed)
    cw, ch, nref = 256, 128, 1 + seed
    log2, intra, mv, ref, cbf = motion_field(rng, cw, ch, nref)
    stub = _Stub(cw, ch, 1, 1, nref, intra, mv, ref, None, 9)
    merge = np.zeros(15, np.int32); amvp = np.zeros(4, np.int32); sig = np.zeros(5, np.int32)
    a = [np.ascontiguousarray(x) for x in (log2, intra, mv, ref, cbf)]
    for y in range(0, ch, 8):
        for x in range(0, cw, 8):
            l = int(log2[y // 8, x // 8])
            if intra[y // 8, x // 8] or (x | y) & ((1 << l) - 1):
                continue
            n = 1 << l
            ht().ht_cands(cw, ch, 1, 1, nref, *[v.ctypes.data for v in a], None, x, y, l, merge.ctypes.data, amvp.ctypes.data, sig.ctypes.data)
            assert [tuple(merge[3 * k:3 * k + 3]) for k in range(5)] == [c[:3] for c in stub.merge_candidates(x, y, n, x, y, n, n, 0, 0)]
            assert [tuple(amvp[2 * k:2 * k + 2]) for k in range(2)] == [tuple(c) for c in stub.amvp_candidates(x, y, n, x, y, n, n, 0, 0, int(ref[y // 8, x // 8]))]


def test_picture_restatement_files_the_record():
    """ht_picture (what the GPU test restates k_inter_signal with) files the record col_record describes and derives what ht_cands derives"""
    rng = random.Random(5)
    cw, ch, nref = 192, 128, 2
    log2, intra, mv, ref, cbf = motion_field(rng, cw, ch, nref)
    _, cintra, cmv, cref, _ = motion_field(rng, cw, ch, 2)
    col = col_record(cintra, cmv, cref)
    b8 = (ch // 8, cw // 8)
    flags = np.zeros(b8, np.uint8); midx = np.zeros(b8, np.uint8); mvp = np.zeros(b8, np.uint8); mvd = np.zeros(b8 + (2,), np.int16)
    out = np.zeros((ch // 16, cw // 16, 4), np.int16)
    a = [np.ascontiguousarray(x) for x in (log2, intra, mv, ref, cbf)]
    ht().ht_picture(cw, ch, 1, 1, nref, *[v.ctypes.data for v in a], col.ctypes.data, flags.ctypes.data, midx.ctypes.data, mvp.ctypes.data, mvd.ctypes.data, out.ctypes.data)
    assert np.array_equal(out, col_record(intra, mv, ref))
    merge = np.zeros(15, np.int32); amvp = np.zeros(4, np.int32); sig = np.zeros(5, np.int32)
    for y in range(0, ch, 8):
        for x in range(0, cw, 8):
            l = int(log2[y // 8, x // 8])
            if intra[y // 8, x // 8]:
                continue
            ht().ht_cands(cw, ch, 1, 1, nref, *[v.ctypes.data for v in a], col.ctypes.data, x & ~((1 << l) - 1), y & ~((1 << l) - 1), l,
                          merge.ctypes.data, amvp.ctypes.data, sig.ctypes.data)
            i = (y // 8, x // 8)
            assert (flags[i], midx[i], mvp[i], mvd[i][0], mvd[i][1]) == tuple(sig), (x, y)
