"""CPU: the checker's statement of "me-coarse"  and "lp-gop" (section 9d), oracle/hevc_enc.c, held to what states them independently.

* Off is off: with me-coarse 0 and without lp-gop the checker writes the bytes of the checker opened without the options.  That shows the zero values inert
  inside this build; that the bytes are those of the checker BEFORE it learned the options -- me_block32's key is now cost << 17 | k << 14 | window << 13 |
  candidate for every configuration -- is what the untouched recorded digests guard (tests/test_oracle_lp_refs_tmvp.py, tests/golden/oracle_streams.json,
  the parser digests, the golden streams), not this test.
* Its two-level integer search equals tests/me_coarse_model.py entry for entry -- cu_log2, cu_mv, cu_ref and the centres --, with vectors beyond 32 samples.
* The structure of its lp-gop streams, read from the stream alone, and its own report equal tests/lp_gop_model.py.
* Its search under lp-gop equals tests/lp_refs_model.search() handed the model's reference planes and the picture's QP.
* Every stream decodes to its reconstruction in oracle/hevc_dec.c (MD5 SEI checked) and, for the small sizes, in tests/pyhevc.py.
* Recorded digests (tests/golden/me_coarse_lp_gop_access_units.json) hold the statement still."""
import hashlib
import json
import os

import numpy as np
import pytest

import enckit
import lp_gop_model as M
import lp_gop_stream
import lp_refs_model
import me_coarse_model
import occluder_content
import orc
import pan_content
import pyhevc
from cases import GDN, LP_REFS_SEARCH as REFS_SEARCH, ME_COARSE_SEARCH as COARSE_SEARCH, ORACLE_GUARD as GUARD
from enckit import ROI as _ROI, SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _padded(fr, w, h):
    """the padded input luma plane the encoder codes: the last column and row repeated up to the coded size (a multiple of 64, at least 128 wide)"""
    cw, ch = max(128, (w + 63) & ~63), (h + 63) & ~63
    return np.pad(fr[:w * h].reshape(h, w), ((0, ch - h), (0, cw - w)), mode="edge")


def test_options_are_checked():
    e = orc.OracleEncoder(256, 128)
    for name, bad in (("me-coarse", 32), ("me-coarse", 512), ("me-coarse", -64), ("lp-gop-d", 7), ("lp-gop-d", 0), ("lp-gop-g", -1), ("lp-gop", 2)):
        with pytest.raises(ValueError):
            e.set_option(name, bad)
    e.set_option("lp-gop-g", 4)
    with pytest.raises(ValueError):                   # the switch with a g and no d: refused, as with d > 6
        e.set_option("lp-gop", 1)
    e.set_option("lp-refs", 3)
    e.set_lp_gop(4, 3)
    e.set_option("me-coarse", 64)
    e.set_option("lp-refs", 2)                        # (changed again before the first picture: the ring follows)
    e.encode(orc.synth_frame(0, SEED, 256, 128, 0))
    for name, v in (("me-coarse", 128), ("lp-gop", 0), ("lp-gop-g", 8), ("lp-gop-d", 2)):
        with pytest.raises(ValueError):               # after the first picture
            e.set_option(name, v)
    e.close()


# ---- 1. off is off: the guard cases of tests/test_oracle_lp_refs_tmvp.py
@pytest.mark.parametrize("cfg", GUARD, ids=[str(i) for i in range(len(GUARD))])
@pytest.mark.parametrize("n", [None, 3])
def test_off_is_the_checker_of_before(cfg, n):
    """the options at 0 against the same build without them (the parent's bytes: the recorded digests, see the module docstring)"""
    w, h = 320, 256
    frames = enckit.frames(cfg.get("kind", 0), w, h, cfg.get("frames", 5))
    kw = dict(qp=30, me_range=12, period=4, **cfg["kw"])
    base = enckit.oracle_encoder(w, h, n, opts=cfg.get("opts", ()), **kw)
    want = [base.encode(f) for f in frames]
    base.close()
    # me-coarse 0; the gop string without the switch; the switch without a string; both off
    for coarse, gop in ((0, None), (None, (4, 3, 0)), (None, (0, 3, 1)), (0, (8, 4, 0))):
        e = enckit.oracle_encoder(w, h, n, None, coarse, gop, opts=cfg.get("opts", ()), **kw)
        got = [e.encode(f) for f in frames]
        d = e.debug()
        assert got == want, (coarse, gop, [a == b for a, b in zip(got, want)])
        assert "me_coarse" not in d and d["lp_gop"]["active"] == 0 and d["lp_gop"]["layer"] == 0
        e.close()


# ---- 2. the two-level integer search against the numpy statement (subme 0): the rows of tests/test_gpu_me_coarse.py SEARCH below 1080p
SEARCH = [c for c in COARSE_SEARCH if c.get("w", 640) <= 640]


@pytest.mark.parametrize("cfg", SEARCH, ids=[str(i) for i in range(len(SEARCH))])
def test_coarse_search_matches_the_model(cfg):
    w, h, n, R, qp, reach = cfg.get("w", 640), cfg.get("h", 384), cfg.get("n", 1), cfg.get("R", 16), cfg.get("qp", 32), cfg["reach"]
    tc, tr = [int(v) for v in cfg.get("tiles", "1x1").split("x")]
    me_early = cfg.get("me_early", 1)
    nf = cfg.get("frames", 3)
    frames = enckit.frames(cfg.get("kind", 0), w, h, nf) if cfg["clip"] == "moving" else pan_content.clip(w, h, nf, *cfg["clip"])
    e = enckit.oracle_encoder(w, h, n, 0, reach, opts=(("me-source", cfg.get("me_source", 0)),), qp=qp, me_range=R, me_early=me_early, tile_rows=tr, tile_cols=tc,
             mv_frame=cfg.get("mv_frame", 0), wpp=0 if tc * tr > 1 else 1)
    srcs, recs, longest, seconds = [], [], 0, 0
    for t, fr in enumerate(frames):
        e.encode(fr)
        d = e.debug()
        srcs.append(_padded(fr, w, h)); recs.append(d["rec0"])
        if t == 0:
            assert "me_coarse" not in d
            continue
        nact = min(n, t)
        refs_in = [srcs[t - 1 - k] for k in range(nact)]
        refs = refs_in if cfg.get("me_source") else [recs[t - 1 - k] for k in range(nact)]
        det = {}
        log2, mv, rf, cen = me_coarse_model.search(srcs[t], refs, qp, R, tile_rows=tr, tile_cols=tc, mv_frame=cfg.get("mv_frame", 0), me_early=me_early,
                                                   me_coarse=reach, refs_in=refs_in, detail=det)
        for name, a, b in (("cu_log2", log2, d["cu_log2"]), ("cu_ref", rf, d["cu_ref"]), ("cu_mv", mv, d["cu_mv"])):
            bad = np.argwhere(np.asarray(a != b))
            assert not len(bad), "picture %d: %s differs at %d entries, first %s (model %s checker %s)" % (
                t, name, len(bad), bad[0].tolist(), a[tuple(bad[0][:a.ndim])], b[tuple(bad[0][:b.ndim])])
        for k in range(4):                            # every block's centre (the checker also states those of blocks that terminate early), zeros beyond m
            want = cen[k].astype(np.int16) if k < nact else np.zeros_like(d["me_coarse"][k])
            bad = np.argwhere((want != d["me_coarse"][k]).any(axis=2))
            assert not len(bad), "picture %d reference %d: centres differ at %d blocks, first %s" % (t, k, len(bad), bad[0].tolist())
        longest = max(longest, int(np.abs(d["cu_mv"].astype(np.int32)).max()))
        seconds += int(det["second"].sum())
    e.close()
    if cfg["clip"] != "moving" and max(abs(cfg["clip"][0]), abs(cfg["clip"][1])) > 32:
        assert longest > 4 * 32, "no vector longer than 32 samples: the case does not leave the old window (longest %d quarter samples)" % longest
        assert seconds > 0


# ---- 3. the structure of lp-gop streams: from the stream alone, and the checker's own report
@pytest.mark.parametrize("period", [5, 12, 13])
@pytest.mark.parametrize("gdn", GDN)
def test_structure_matches_the_model(gdn, period):
    g, d, n = gdn
    w, h, qp, nf = 128, 64, 30, 2 * period + 3
    e = enckit.oracle_encoder(w, h, n, 0, None, (g, d), qp=qp, me_range=8, period=period)
    want = M.structure(period, nf, g, d, n, qp)
    sps = pps = None
    for i, fr in enumerate(enckit.frames(0, w, h, nf)):
        au = e.encode(fr)
        nals = pyhevc.split_nals(au)
        if (nals[0][0] >> 1) & 63 == 32:
            sps, pps = pyhevc.parse_sps(pyhevc.unescape(nals[1])), pyhevc.parse_pps(pyhevc.unescape(nals[2]))
            assert lp_gop_stream.sps_dpb(pyhevc.unescape(nals[1])) == n + 1 and pps["nref_default"] == n
        heads = [f for f in lp_gop_stream.slice_headers(au, sps, pps) if not f["dependent"]]
        assert heads, i
        m = want[i]
        for f in heads:
            assert f["nal"] == (19 if m["idr"] else 1) and f["qp"] == m["qp"], (i, f, m)
            if not m["idr"]:
                assert f["poc"] == m["poc"] and f["rps_in_header"] and f["nact"] == len(m["refs"]), (i, f, m)
                assert f["rps"] == [(p - m["poc"], 1) for p in m["refs"]], (i, f, m)
        dd = e.debug()
        gp = dd["lp_gop"]
        assert dd["poc"] == m["poc"] and bool(dd["is_intra"]) == m["idr"]
        assert gp["active"] == 1 and gp["qp"] == m["qp"] and gp["layer"] == m["layer"] and gp["dists"] == m["dists"], (i, gp, m)
    e.close()


def test_parameter_sets_are_those_of_lp_refs_alone():
    w, h = 128, 64
    fr = orc.synth_frame(0, SEED, w, h, 0)
    for n in (1, 3):
        a, b = enckit.oracle_encoder(w, h, n, 1, qp=30), enckit.oracle_encoder(w, h, n, 1, None, (4, 3), qp=30)
        na, nb = orc.split_nals(a.encode(fr)), orc.split_nals(b.encode(fr))
        assert na[:3] == nb[:3] and na == nb          # VPS, SPS, PPS -- and the IDR picture, which keeps Q
        a.close(); b.close()


# ---- 4. the search under lp-gop against the model: tests/test_gpu_lp_refs.py SEARCH on the blink clip
@pytest.mark.parametrize("cfg", REFS_SEARCH, ids=[str(i) for i in range(len(REFS_SEARCH))])
def test_lp_gop_search_matches_the_model(cfg):
    w, h, n, R, qp = cfg["w"], cfg["h"], cfg["n"], cfg["R"], cfg.get("qp", 32)
    g, d, nf = 4, 3, 7
    tc, tr = [int(v) for v in cfg.get("tiles", "1x1").split("x")]
    e = enckit.oracle_encoder(w, h, n, 0, None, (g, d), opts=(("me-source", cfg.get("me_source", 0)),), qp=qp, me_range=R, me_early=cfg["me_early"], tile_rows=tr, tile_cols=tc,
             mv_frame=cfg.get("mv_frame", 0))
    frames = occluder_content.blink_clip(w, h, nf, kind=cfg["kind"])
    y0, y1, x0, x1 = occluder_content.region(w, h)
    recs, far = [], 0
    for t, fr in enumerate(frames):
        e.encode(fr)
        recs.append(e.recon())
        if t == 0:
            continue
        dd = e.debug()
        dists = M.ref_dists(t, g, n)
        assert dd["lp_gop"]["dists"] == dists and dd["lp_gop"]["qp"] == M.picture_qp(qp, t, g, d)
        src = frames if cfg.get("me_source") else recs
        refs = [src[t - k][:w * h].reshape(h, w) for k in dists]
        log2, mv, rf = lp_refs_model.search(fr[:w * h].reshape(h, w), refs, M.picture_qp(qp, t, g, d), R, tile_rows=tr, tile_cols=tc, mv_frame=cfg.get("mv_frame", 0),
                                            me_early=cfg["me_early"])
        for name, a, b in (("cu_log2", log2, dd["cu_log2"]), ("cu_ref", rf, dd["cu_ref"]), ("cu_mv", mv, dd["cu_mv"])):
            bad = np.argwhere(np.asarray(a != b))
            assert not len(bad), "picture %d: %s differs at %d entries, first %s (model %s checker %s)" % (
                t, name, len(bad), bad[0].tolist(), a[tuple(bad[0][:a.ndim])], b[tuple(bad[0][:b.ndim])])
        if max(dists) > n:
            k = dists.index(max(dists))
            assert t - max(dists) == ((t - 2) // g) * g                      # the far reference is the key picture
            far += int((dd["cu_ref"][y0 // 8:y1 // 8, x0 // 8:x1 // 8] == k).sum())
    e.close()
    assert far > 0, "no block chose the key picture at a distance beyond lp-refs"


# ---- 5. the checker's own closed loop over the tool set; pan: a pan clip (vx, vy) beyond the zero window, else synthetic moving content
CLOSED = [
    # me-coarse alone
    dict(coarse=128, pan=(72, -40)), dict(coarse=128, pan=(-72, 40), kw=dict(subme=2)), dict(coarse=128, pan=(40, 72), kw=dict(subme=4, sao=1)),
    dict(coarse=64, pan=(-40, -52), n=3, tmvp=1), dict(coarse=128, pan=(72, -40), kw=dict(subme=2), opts=(("intra-in-p", 1),)),
    dict(coarse=128, pan=(-72, 40), kw=dict(wpp=0, tile_rows=2, tile_cols=2)), dict(coarse=128, pan=(72, 40), kw=dict(wpp=0, tile_rows=2, tile_cols=2, slices=2)),
    dict(coarse=128, pan=(-72, -40), kw=dict(slices=1)), dict(coarse=128, pan=(72, -40), kw=dict(bitrate=400000), frames=8),
    dict(coarse=128, pan=(-72, 40), kw=dict(bitrate=400000, rc_bands=4, sao=1), frames=8), dict(coarse=128, pan=(72, 40), kw=dict(vaq=6)),
    dict(coarse=128, pan=(72, 40), kw=dict(qp_in_cu=1), roi=True), dict(coarse=128, pan=(-72, -40), opts=(("lossless", 1),)),
    dict(coarse=128, pan=(72, -40), opts=(("scaling-list", 1),)), dict(coarse=128, pan=(-40, -72), opts=(("rdoq", 1), ("signhide", 1))),
    dict(coarse=256, pan=(230, 0), kw=dict(subme=4)), dict(coarse=256, pan=(0, 260), kw=dict(subme=2), opts=(("me-source", 1),)),
    # lp-gop alone
    dict(gop=(4, 3), n=3), dict(gop=(4, 3), n=1, tmvp=1), dict(gop=(4, 3), n=4, tmvp=1, kw=dict(subme=2, sao=1)), dict(gop=(8, 4), n=3, tmvp=1, frames=14),
    dict(gop=(3, 2), n=4, tmvp=1), dict(gop=(1, 1), n=2, tmvp=1), dict(gop=(4, 3), n=3, tmvp=1, kw=dict(period=5), frames=14),
    dict(gop=(4, 3), n=3, kw=dict(subme=4), opts=(("intra-in-p", 2),), kind=2), dict(gop=(4, 3), n=3, opts=(("rdoq", 1), ("signhide", 1))),
    dict(gop=(4, 3), n=3, kw=dict(bitrate=400000)), dict(gop=(4, 3), n=3, tmvp=1, kw=dict(bitrate=400000, rc_bands=4, sao=1)),
    dict(gop=(4, 3), n=3, kw=dict(vaq=6)), dict(gop=(4, 3), n=2, kw=dict(qp_in_cu=1), roi=True), dict(gop=(4, 3), n=3, opts=(("lossless", 1),)),
    dict(gop=(4, 3), n=4, opts=(("scaling-list", 1),)), dict(gop=(4, 3), n=3, kw=dict(wpp=0, tile_rows=2, tile_cols=2)),
    dict(gop=(4, 3), n=4, kw=dict(wpp=0, tile_rows=2, tile_cols=2, slices=2)), dict(gop=(4, 3), n=2, tmvp=1, kw=dict(slices=1)),
    dict(gop=(4, 3), n=3, tmvp=1, kw=dict(qp=50)), dict(gop=(8, 4), n=3, kw=dict(qp=49)), dict(gop=(4, 3), n=2, kw=dict(qp=0), frames=6),
    dict(gop=(4, 3), n=4, tmvp=1, opts=(("me-source", 1),)),
    # both
    dict(coarse=128, gop=(4, 3), n=3, pan=(44, -36), w=384, h=256), dict(coarse=128, gop=(4, 3), n=3, tmvp=1, pan=(-44, 36), w=384, h=256, opts=(("me-source", 1),)),
    dict(coarse=64, gop=(4, 3), n=3, tmvp=1, pan=(40, 36), kw=dict(subme=2, sao=1), opts=(("me-source", 1), ("intra-in-p", 1))),
    dict(coarse=64, gop=(3, 2), n=4, tmvp=1, pan=(-36, 40), kw=dict(bitrate=400000, rc_bands=4, subme=4)),
    # the smallest: tests/pyhevc.py too
    dict(coarse=64, pan=(44, -36), w=256, h=128, kw=dict(me_range=8, subme=2), frames=4, pyhevc=True),
    dict(gop=(4, 3), n=3, w=128, h=64, kw=dict(me_range=8), blink=True, frames=7, pyhevc=True),
    dict(gop=(4, 3), n=2, tmvp=1, w=128, h=64, kw=dict(me_range=8), blink=True, frames=7, pyhevc=True),
    dict(coarse=64, gop=(4, 3), n=3, tmvp=1, pan=(36, -40), w=130, h=70, kw=dict(me_range=8, subme=4), frames=7, pyhevc=True),
]


def _clip(cfg, w, h, nf):
    if cfg.get("pan"):
        return pan_content.clip(w, h, nf, *cfg["pan"])
    if cfg.get("blink"):
        return occluder_content.blink_clip(w, h, nf)
    return enckit.frames(cfg.get("kind", 0), w, h, nf)


@pytest.mark.parametrize("cfg", CLOSED, ids=[str(i) for i in range(len(CLOSED))])
def test_closed_loop(cfg):
    w, h = cfg.get("w", 320), cfg.get("h", 192)
    nf = cfg.get("frames", 10 if cfg.get("gop") else 6)
    kw = dict(dict(qp=32, me_range=12), **cfg.get("kw", {}))
    e = enckit.oracle_encoder(w, h, cfg.get("n"), cfg.get("tmvp"), cfg.get("coarse"), cfg.get("gop"), opts=(("hash", 2),) + tuple(cfg.get("opts", ())), **kw)
    if cfg.get("roi"):
        e.set_roi(*_ROI)
    od = orc.OracleDecoder()
    pairs, longest, clipped = [], 0, 0
    for t, f in enumerate(_clip(cfg, w, h, nf)):
        au = e.encode(f)
        rec = e.recon()
        d = e.debug()
        if not d["is_intra"]:
            longest = max(longest, int(np.abs(d["cu_mv"].astype(np.int32)).max()))
            clipped += d["lp_gop"]["qp"] == 51
        pairs.append((au, rec))
        got = od.decode_au(au, t)
        assert len(got) == 1 and np.array_equal(got[0]["i420"], rec), "picture %d: oracle/hevc_dec.c differs from the reconstruction" % t
    checked, bad = od.hash_stats()
    assert checked == nf and bad == 0, (checked, bad)
    od.close(); e.close()
    if cfg.get("pan"):
        assert longest > 4 * 32, "the case does not leave the old window"
    if cfg.get("gop") and kw["qp"] >= 49:
        assert clipped > 0, "no picture's QP was clipped at 51"
    if cfg.get("pyhevc"):
        from deckit import tabs
        dec = pyhevc.Decoder(tabs())
        for au, _ in pairs:
            dec.decode(au)
        pics = dec.flush()
        assert len(pics) == nf
        for t, p in enumerate(pics):
            assert np.array_equal(p["i420"], pairs[t][1]), "picture %d: tests/pyhevc.py differs" % t


def test_closed_loop_decodes_scaled_amvp():
    """a stream in which adjacent inter CUs hold references of different distance with a non-merged CU among them (counted from the debug arrays): the decoder
    scales a neighbour's vector by the true POC distances (8.5.3.2.7) to read the vector differences the checker's encoder wrote"""
    w, h, g, d, n = 320, 192, 4, 3, 3
    e = enckit.oracle_encoder(w, h, n, 1, None, (g, d), qp=22, me_range=12, me_early=0)
    od = orc.OracleDecoder()
    count = 0
    for t, fr in enumerate(enckit.frames(2, w, h, 10)):
        au = e.encode(fr)
        got = od.decode_au(au, t)
        assert len(got) == 1 and np.array_equal(got[0]["i420"], e.recon()), t
        if t < 2:
            continue
        dd = e.debug()
        dist = np.asarray(M.ref_dists(t, g, n) + [0] * 4)[dd["cu_ref"].astype(np.int32)]
        inter, amvp = dd["cu_intra"] == 0, (dd["cu_flags"] & 2) == 0
        for a, b in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
            count += int((inter[a] & inter[b] & (dist[a] != dist[b]) & (amvp[a] | amvp[b])).sum())
    od.close(); e.close()
    assert count > 0, "no non-merged CU beside a CU with a reference of another distance"


def test_long_mvd_strings():
    """me-coarse 256 on a pan past 230 samples with subme 4: mvd components of more than 10 bins are coded, and the stream decodes"""
    w, h = 640, 384
    e = enckit.oracle_encoder(w, h, None, None, 256, qp=32, me_range=16, subme=4)
    od = orc.OracleDecoder()
    longest = 0
    for t, fr in enumerate(pan_content.clip(w, h, 3, 236, -3)):
        au = e.encode(fr)
        got = od.decode_au(au, t)
        assert len(got) == 1 and np.array_equal(got[0]["i420"], e.recon()), t
        d = e.debug()
        if t:
            amvp = (d["cu_intra"] == 0) & ((d["cu_flags"] & 2) == 0)
            longest = max(longest, max(lp_refs_model.mvd_bits(int(v)) for v in np.abs(d["cu_mvd"][amvp].astype(np.int32)).max(axis=0)))
    od.close(); e.close()
    assert longest > 10, longest


# ---- 6. recorded digests
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "me_coarse_lp_gop_access_units.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("idx", range(len(_golden())))
def test_recorded_digests(idx):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_me_coarse_lp_gop_digests as mk
    case = _golden()[idx]
    got = mk.digests(dict(case["config"], opts=[tuple(o) for o in case["config"]["opts"]]))
    for t, want in enumerate(case["frames"]):
        assert got[t] == want, (idx, t)
    assert len(got) == len(case["frames"])
