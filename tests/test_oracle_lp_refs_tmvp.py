"""CPU: the checker's statement of "lp-refs"  and "tmvp" (section 9b), oracle/hevc_enc.c.

* With lp-refs 0 / 1 and tmvp 0 the checker writes the bytes of the checker opened without the options.
* Its integer search over n references equals the numpy restatement tests/lp_refs_model.py.
* Every stream it writes decodes to its reconstruction in oracle/hevc_dec.c (MD5 SEI checked) and, for the small sizes, in tests/pyhevc.py.
* tmvp changes the bits and never the pictures.
* Its merge / AMVP decisions equal the host build of the product's derivation (tests/hostcheck ht_picture) fed the checker's own fields.
* Recorded digests (tests/golden/lp_refs_tmvp_access_units.json) hold the statement still."""
import hashlib
import json
import os

import numpy as np
import pytest

import edge_content as ec
import enckit
import hc
import lp_refs_model
import orc
from cases import ORACLE_GUARD as GUARD
from enckit import SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_are_checked():
    e = orc.OracleEncoder(256, 128)
    for name, bad in (("lp-refs", 5), ("lp-refs", -1), ("tmvp", 2)):
        with pytest.raises(ValueError):
            e.set_option(name, bad)
    e.set_option("lp-refs", 4)
    e.set_option("lp-refs", 2)                        # (changed again before the first picture: the ring follows)
    e.encode(orc.synth_frame(0, SEED, 256, 128, 0))
    with pytest.raises(ValueError):                   # after the first picture the parameter sets are out
        e.set_option("lp-refs", 3)
    e.close()


# ---- 1. guard: lp-refs 0 / 1 and tmvp 0 are the checker of before, byte for byte


@pytest.mark.parametrize("cfg", GUARD, ids=[str(i) for i in range(len(GUARD))])
def test_one_reference_and_tmvp_off_are_the_checker_of_before(cfg):
    w, h = 320, 256
    frames = enckit.frames(cfg.get("kind", 0), w, h, cfg.get("frames", 5))
    kw = dict(qp=30, me_range=12, period=4, **cfg["kw"])
    base = enckit.oracle_encoder(w, h, opts=cfg.get("opts", ()), **kw)
    want = [base.encode(f) for f in frames]
    base.close()
    for n, tmvp in ((0, 0), (1, 0), (1, None), (None, 0)):
        e = enckit.oracle_encoder(w, h, n, tmvp, opts=cfg.get("opts", ()), **kw)
        got = [e.encode(f) for f in frames]
        assert got == want, (n, tmvp, [a == b for a, b in zip(got, want)])
        assert not e.debug()["cu_ref"].any()
        e.close()


# ---- 2. the integer search against the numpy restatement (subme 0, intra-in-P off)
SEARCH = [
    dict(w=256, h=128, n=2, R=8, me_early=1, kind=0, frames=5),
    dict(w=256, h=192, n=3, R=8, me_early=0, kind=0, frames=6, qp=27),
    dict(w=192, h=128, n=4, R=6, me_early=0, kind=2, frames=6, qp=37),
    dict(w=256, h=128, n=4, R=8, me_early=1, kind=0, frames=6, tmvp=1),
    dict(w=256, h=256, n=4, R=8, me_early=1, kind=0, frames=6, tiles=(2, 2), mv_frame=2),
    dict(w=256, h=256, n=3, R=8, me_early=0, kind=0, frames=5, tiles=(2, 2), mv_frame=1),
    dict(w=256, h=128, n=3, R=8, me_early=0, kind=0, frames=5, me_source=1),
    dict(w=256, h=128, n=2, R=6, me_early=1, kind=0, frames=7, me_source=1, period=4),
    dict(w=256, h=192, n=4, R=8, me_early=0, pattern="cut_black_white", frames=5),
    dict(w=256, h=192, n=3, R=8, me_early=0, pattern="cut_runs", frames=7, me_source=1),
    dict(w=256, h=192, n=3, R=8, me_early=1, pattern="cut_runs", frames=7, me_source=1),
]


@pytest.mark.parametrize("cfg", SEARCH, ids=[str(i) for i in range(len(SEARCH))])
def test_integer_search_matches_the_model(cfg):
    w, h, n, R, qp = cfg["w"], cfg["h"], cfg["n"], cfg["R"], cfg.get("qp", 32)
    tc, tr = cfg.get("tiles", (1, 1))
    period = cfg.get("period", 64)
    e = enckit.oracle_encoder(w, h, n, cfg.get("tmvp", 0), opts=(("me-source", cfg.get("me_source", 0)),), qp=qp, me_range=R, me_early=cfg["me_early"],
             tile_rows=tr, tile_cols=tc, mv_frame=cfg.get("mv_frame", 0), period=period)
    if cfg.get("pattern") == "cut_runs":              # three black pictures, three white ones, ...: the first of a run has only the other colour behind it
        frames = [ec.cut_black_white(w, h, (t // 3) % 2, ec.SEED) for t in range(cfg["frames"])]
    elif cfg.get("pattern"):
        frames = [ec.PATTERNS[cfg["pattern"]](w, h, t, ec.SEED) for t in range(cfg["frames"])]
    else:
        frames = enckit.frames(cfg["kind"], w, h, cfg["frames"])
    recs, older = [], 0
    for t, fr in enumerate(frames):
        e.encode(fr)
        d = e.debug()
        recs.append(d["rec0"])
        poc = t % period
        if poc == 0:
            continue
        nact = min(n, poc)
        src = [f[:w * h].reshape(h, w) for f in frames] if cfg.get("me_source") else recs
        refs = [src[t - 1 - k] for k in range(nact)]
        log2, mv, rf = lp_refs_model.search(fr[:w * h].reshape(h, w), refs, qp, R, tile_rows=tr, tile_cols=tc, mv_frame=cfg.get("mv_frame", 0),
                                            me_early=cfg["me_early"])
        for name, a, b in (("cu_log2", log2, d["cu_log2"]), ("cu_ref", rf, d["cu_ref"]), ("cu_mv", mv, d["cu_mv"])):
            bad = np.argwhere(np.asarray(a != b))
            assert not len(bad), "picture %d: %s differs at %d entries, first %s (model %s checker %s)" % (
                t, name, len(bad), bad[0].tolist(), a[tuple(bad[0][:a.ndim])], b[tuple(bad[0][:b.ndim])])
        older += int((d["cu_ref"] > 0).sum())
        if cfg.get("pattern") == "cut_runs":
            # (me-source: the search looks at the input pictures, exactly 0 or 255) the first picture of a run: every candidate of every reference
            # ties on the SAD (each quarter's is 65280), the rate makes the zero vector of reference 0 the cheapest; inside a run
            # reference 0 is an exact match
            assert not d["cu_ref"].any(), t
            if t % 3 == 0:
                assert (d["cu_log2"] == 5).all() and not d["cu_mv"].any(), t
    if not cfg.get("pattern"):
        assert older > 0, "no block chose an older reference"


# ---- 3. the checker's own closed loop
CLOSED = [
    dict(n=2), dict(n=3), dict(n=4),
    dict(n=3, kw=dict(subme=1)), dict(n=4, kw=dict(subme=4, sao=1)),
    dict(n=3, kw=dict(subme=2), opts=(("intra-in-p", 1),)), dict(n=4, opts=(("intra-in-p", 2),), kind=2),
    dict(n=4, kw=dict(subme=2, sao=1), opts=(("me-source", 1), ("intra-in-p", 1))),
    dict(n=3, kw=dict(wpp=0, tile_rows=2, tile_cols=2)), dict(n=4, kw=dict(wpp=0, tile_rows=2, tile_cols=2, slices=2)), dict(n=2, kw=dict(slices=1)),
    dict(n=2, kw=dict(period=1)), dict(n=3, kw=dict(period=4), frames=9), dict(n=4, kw=dict(period=5), frames=11),
    dict(n=3, kw=dict(bitrate=400000), frames=9), dict(n=4, kw=dict(bitrate=400000, rc_bands=4, sao=1), frames=9),
    dict(n=3, opts=(("rdoq", 1), ("signhide", 1))), dict(n=3, kw=dict(vaq=6)), dict(n=2, kw=dict(qp_in_cu=1), roi=True),
    dict(n=3, opts=(("lossless", 1),)), dict(n=4, opts=(("scaling-list", 1),)), dict(n=2, kw=dict(deblock=0)),
    dict(n=3, kw=dict(mv_frame=1)), dict(n=4, kw=dict(mv_frame=2, tile_rows=2, tile_cols=2)), dict(n=4, kind=2, kw=dict(qp=22, me_early=0)),
    dict(n=3, w=128, h=64, pyhevc=True), dict(n=4, w=130, h=70, kw=dict(subme=4), pyhevc=True), dict(n=2, w=16, h=16, pyhevc=True, frames=5),
]
CLOSED_CASES = [dict(c, tmvp=tm) for c in CLOSED for tm in (0, 1)]


@pytest.mark.parametrize("cfg", CLOSED_CASES, ids=[str(i) for i in range(len(CLOSED_CASES))])
def test_closed_loop(cfg):
    w, h = cfg.get("w", 320), cfg.get("h", 192)
    nf = cfg.get("frames", 7)
    kw = dict(dict(qp=32, me_range=12), **cfg.get("kw", {}))
    e = enckit.oracle_encoder(w, h, cfg["n"], cfg["tmvp"], opts=(("hash", 2),) + tuple(cfg.get("opts", ())), **kw)
    if cfg.get("roi"):
        e.set_roi(4, 3, (np.arange(12, dtype=np.int8) % 7 - 3).astype(np.int8))
    od = orc.OracleDecoder()
    pairs = []
    for t, f in enumerate(enckit.frames(cfg.get("kind", 0), w, h, nf)):
        au = e.encode(f)
        rec = e.recon()
        pairs.append((au, rec))
        got = od.decode_au(au, t)
        assert len(got) == 1 and np.array_equal(got[0]["i420"], rec), "picture %d: oracle/hevc_dec.c differs from the reconstruction" % t
    checked, bad = od.hash_stats()
    assert checked == nf and bad == 0, (checked, bad)
    od.close(); e.close()
    if cfg.get("pyhevc"):
        import pyhevc
        from deckit import tabs
        dec = pyhevc.Decoder(tabs())
        for au, _ in pairs:
            dec.decode(au)
        pics = dec.flush()
        assert len(pics) == nf
        for t, p in enumerate(pics):
            assert np.array_equal(p["i420"], pairs[t][1]), "picture %d: tests/pyhevc.py differs" % t


# ---- 4. tmvp changes the bits, not the pictures
@pytest.mark.parametrize("n,kw,opts", [(1, {}, ()), (3, dict(subme=4), (("intra-in-p", 1),)), (4, dict(tile_rows=2, tile_cols=2, sao=1, period=4), ()),
                                       (2, dict(subme=2), (("me-source", 1), ("rdoq", 1)))])
def test_tmvp_changes_bits_not_pictures(n, kw, opts):
    w, h, nf = 320, 256, 7
    frames = enckit.pan(w, h, nf)
    runs = {}
    for tmvp in (0, 1):
        e = enckit.oracle_encoder(w, h, n, tmvp, opts=opts, **dict(dict(qp=30, me_range=12), **kw))
        runs[tmvp] = [(e.encode(f), e.recon()) for f in frames]
        e.close()
    for t in range(nf):
        assert np.array_equal(runs[0][t][1], runs[1][t][1]), "picture %d: tmvp changed the reconstruction" % t
    differ = [a[0] != b[0] for a, b in zip(runs[0], runs[1])]
    assert any(differ[2:]), "tmvp changed no access unit on a pan"


# ---- 5. two statements of the signalling agree: the checker's decisions == the host build of hevc_core.h's, fed the checker's fields
SIGNAL = [dict(n=1), dict(n=2, kw=dict(period=4, subme=4)), dict(n=3, opts=(("intra-in-p", 2),)), dict(n=4, kw=dict(tile_rows=2, tile_cols=2, wpp=0)),
          dict(n=4, kw=dict(subme=2), opts=(("me-source", 1),)), dict(n=3, w=130, h=70, kw=dict(subme=4)), dict(n=3, pan=True, kw=dict(subme=2))]


@pytest.mark.parametrize("cfg", SIGNAL, ids=[str(i) for i in range(len(SIGNAL))])
@pytest.mark.parametrize("tmvp", [0, 1])
def test_signalling_matches_the_host_derivation(cfg, tmvp):
    w, h, n = cfg.get("w", 320), cfg.get("h", 192), cfg["n"]
    kw = dict(dict(qp=30, me_range=12), **cfg.get("kw", {}))
    period = kw.get("period", 64)
    e = enckit.oracle_encoder(w, h, n, tmvp, opts=cfg.get("opts", ()), **kw)
    frames = enckit.pan(w, h, 8) if cfg.get("pan") else enckit.frames(0, w, h, 8)
    prev, checked, temporal = None, 0, 0
    for t, fr in enumerate(frames):
        e.encode(fr)
        d = e.debug()
        cw, ch = d["coded_w"], d["coded_h"]
        poc = t % period
        col = hc.col_record(d["cu_intra"], d["cu_mv"], d["cu_ref"]) if poc else None
        if poc:
            nact = min(max(n, 1), poc)
            use = prev if (tmvp and poc >= 2) else None
            a = [d[k] for k in ("cu_log2", "cu_intra", "cu_mv", "cu_ref", "cu_cbf")]
            want = {}
            want["flags"], want["midx"], want["mvp"], wmvd, _ = hc.picture(cw, ch, kw.get("tile_rows", 1), kw.get("tile_cols", 1), nact, a, col=use)
            inter = d["cu_intra"] == 0
            for name, got, exp in (("cu_flags", d["cu_flags"], want["flags"]), ("cu_merge_idx", d["cu_merge_idx"], want["midx"]),
                                   ("cu_mvp_idx", d["cu_mvp_idx"], want["mvp"]), ("cu_mvd", d["cu_mvd"], wmvd)):
                bad = np.argwhere(inter & (np.any(got != exp, axis=-1) if got.ndim == 3 else (got != exp)))
                assert not len(bad), "picture %d: %s differs at %d units, first %s" % (t, name, len(bad), bad[0].tolist())
            checked += int(inter.sum())
            if use is not None:
                f0 = {}
                f0["flags"], f0["midx"], f0["mvp"], _, _ = hc.picture(cw, ch, kw.get("tile_rows", 1), kw.get("tile_cols", 1), nact, a)
                temporal += int((inter & ((f0["flags"] != want["flags"]) | (f0["midx"] != want["midx"]) | (f0["mvp"] != want["mvp"]))).sum())
        prev = col
    assert checked > 0
    if tmvp:
        assert temporal > 0, "no decision used a temporal candidate"


# ---- 6. recorded digests
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "lp_refs_tmvp_access_units.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("idx", range(len(_golden())))
def test_recorded_digests(idx):
    case = _golden()[idx]
    c = case["config"]
    e = enckit.oracle_encoder(c["w"], c["h"], opts=[tuple(o) for o in c["opts"]], **c["enc"])
    for t, want in enumerate(case["frames"]):
        au = e.encode(orc.synth_frame(c["kind"], c["seed"], c["w"], c["h"], t))
        got = {"au_bytes": len(au), "au_md5": hashlib.md5(au).hexdigest(), "recon_md5": hashlib.md5(e.recon().tobytes()).hexdigest()}
        assert got == want, (idx, t)
    e.close()
