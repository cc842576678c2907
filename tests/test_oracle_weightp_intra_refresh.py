"""CPU: the checker's statement of "weightp"  and "intra-refresh" (section 9f), oracle/hevc_enc.c, held to what states them independently.

* Off is off: with both options at 0 the checker writes the bytes of the checker opened without them.  That shows the zero values inert inside this build; that
  the bytes are those of the checker BEFORE it learned the options is what the untouched recorded digests guard (tests/golden/oracle_streams.json, the parser
  digests, me_coarse_lp_gop_access_units.json, the golden streams), not this test.
* weightp: its record equals tests/wp_model.py record() entry for entry, and at subme 0 its search equals tests/lp_refs_model.search() handed the model's
  search planes.
* intra-refresh: its pictures have the structure tests/ir_model.py check_structure() asks of the HIP encoder's, with every rule exercised.
* Every stream decodes to its reconstruction in oracle/hevc_dec.c (MD5 SEI checked) and, at 128x64, in tests/pyhevc.py.
* The recovery property of section 9f, on the checker's own refreshed stream in the checker's decoder.
* Recorded digests (tests/golden/weightp_intra_refresh_access_units.json) hold the statement still."""
import json
import os

import numpy as np
import pytest

import enckit
import ir_model as IR
import lp_gop_model
import lp_refs_model
import orc
import pan_content
import pyhevc
import wp_model as WP
from cases import ORACLE_GUARD as GUARD
from enckit import SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("none", "offset", "gain", "flash")
# references per P picture, lp-gop (g, d) or None, me-source: the setups of tests/test_gpu_weightp.py
SETUPS = {"one": (1, None, 0), "three": (3, None, 0), "one-src": (1, None, 1), "gop-src": (3, (4, 3), 1)}
# (width, height, N) of tests/test_gpu_intra_refresh.py and the smallest picture: B = 4, m = 2, n = 2
IR_SIZES = [(320, 192, 5), (320, 192, 10), (200, 120, 8), (640, 384, 4), (128, 64, 2)]


def _cw(w):
    return max(128, (w + 63) & ~63)


# ---- option checks
def test_options_are_checked():
    fr = orc.synth_frame(0, SEED, 256, 128, 0)
    e = orc.OracleEncoder(256, 128)
    for name, bad in (("weightp", 2), ("weightp", -1), ("intra-refresh", 1), ("intra-refresh", 256), ("intra-refresh", -2)):
        with pytest.raises(ValueError):
            e.set_option(name, bad)
    e.set_option("weightp", 1); e.set_option("intra-refresh", 255); e.set_option("intra-refresh", 2); e.set_option("weightp", 0); e.set_option("weightp", 1)
    for name, v in (("lossless", 1), ("lp-refs", 2), ("lp-refs", 4), ("lp-gop", 1), ("tmvp", 1), ("me-coarse", 64), ("intra-chain", 0)):
        with pytest.raises(ValueError):               # set behind the option that is not stated with it
            e.set_option(name, v)
    e.set_option("lp-refs", 1); e.set_option("tmvp", 0); e.set_option("me-coarse", 0); e.set_option("intra-chain", 1)      # (the allowed values stay allowed)
    e.encode(fr)
    for name, v in (("weightp", 0), ("intra-refresh", 0), ("intra-refresh", 8)):
        with pytest.raises(ValueError):               # after the first picture
            e.set_option(name, v)
    e.close()
    # ... and the other way round: the option set behind what it is not stated with
    for opts, kw, name in (((("lossless", 1),), {}, "weightp"), ((("lossless", 1),), {}, "intra-refresh"), ((("lp-refs", 2),), {}, "intra-refresh"),
                           ((("lp-gop-g", 4), ("lp-gop-d", 3), ("lp-gop", 1)), {}, "intra-refresh"), ((("tmvp", 1),), {}, "intra-refresh"),
                           ((("me-coarse", 64),), {}, "intra-refresh"), ((("intra-chain", 0),), {}, "intra-refresh"),
                           ((), dict(tile_rows=2, wpp=0), "intra-refresh"), ((), dict(tile_cols=2, wpp=0), "intra-refresh")):
        e = enckit.oracle_encoder(256, 128, opts=opts, **kw)
        with pytest.raises(ValueError):
            e.set_option(name, 8 if name == "intra-refresh" else 1)
        e.close()


# ---- 1. off is off
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
    e = enckit.oracle_encoder(w, h, n, opts=tuple(cfg.get("opts", ())) + (("weightp", 0), ("intra-refresh", 0)), **kw)
    got = [e.encode(f) for f in frames]
    d = e.debug()
    e.close()
    assert got == want, [a == b for a, b in zip(got, want)]
    assert "wp" not in d and "ir" not in d


# ---- 2. weightp: the record and the integer search against the models
def _wp_clip(kind, w, h, n):
    """the benchmark clip (synth kind 0, seed 1234) with the change `kind` on its luma, and its visible luma planes"""
    frames = WP.change([orc.synth_frame(0, 1234, w, h, t) for t in range(n)], w, h, kind)
    return frames, [f[:w * h].reshape(h, w) for f in frames]


@pytest.mark.parametrize("setup", sorted(SETUPS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", [(320, 192), (200, 120)])
def test_weightp_record_and_search_match_the_models(size, kind, setup):
    w, h = size
    n, gop, me_source = SETUPS[setup]
    qp, R, nf = 32, 6, 7
    frames, ys = _wp_clip(kind, w, h, nf)
    e = enckit.oracle_encoder(w, h, n, 0, None, gop, opts=(("me-source", me_source), ("weightp", 1)), qp=qp, me_range=R)
    recs, weighted0 = [], 0
    for t, fr in enumerate(frames):
        e.encode(fr)
        recs.append(e.recon())
        d = e.debug()
        got = [tuple(int(v) for v in r) for r in d["wp"]]
        if t == 0:
            assert got == [WP.PLAIN] * 4
            continue
        dists = lp_gop_model.ref_dists(t, gop[0], n) if gop else list(range(1, min(n, t) + 1))
        want = WP.record(ys, t, dists)
        assert got == want, (t, got, want)
        weighted0 += got[0][0]
        if w == 320:                                    # (coded size = visible size: the planes the search reads are the visible ones)
            planes = frames if me_source else recs
            refs = [WP.search_plane(planes[t - k][:w * h].reshape(h, w), want[i]) for i, k in enumerate(dists)]
            pqp = lp_gop_model.picture_qp(qp, t, gop[0], gop[1]) if gop else qp
            log2, mv, rf = lp_refs_model.search(ys[t], refs, pqp, R)
            for name, a, b in (("cu_log2", log2, d["cu_log2"]), ("cu_ref", rf, d["cu_ref"]), ("cu_mv", mv, d["cu_mv"])):
                bad = np.argwhere(np.asarray(a != b))
                assert not len(bad), "picture %d: %s differs at %d entries, first %s (model %s checker %s)" % (
                    t, name, len(bad), bad[0].tolist(), a[tuple(bad[0][:a.ndim])], b[tuple(bad[0][:b.ndim])])
    e.close()
    if kind in ("offset", "gain"):                      # the coverage: a silent "never weighted" (or "always") fails
        assert weighted0 == nf - 1, (kind, weighted0)
    if kind == "none":
        assert weighted0 == 0


# ---- 3. intra-refresh: the structure of the checker's own pictures
def _ir_clip(w, h, n):
    return [orc.synth_frame(0, 1234, w, h, t) for t in range(n)]


STRUCT = [(s, 1) for s in IR_SIZES] + [(IR_SIZES[0], 0), (IR_SIZES[0], 2)]


@pytest.mark.parametrize("size,ip", STRUCT, ids=["%dx%d-N%d-ip%d" % (s + (ip,)) for s, ip in STRUCT])
def test_intra_refresh_pictures_have_the_structure(size, ip):
    w, h, N = size
    cw = _cw(w)
    e = enckit.oracle_encoder(w, h, opts=(("intra-in-p", ip), ("intra-refresh", N)), qp=32, me_range=8, subme=2)
    total = {}
    for t, fr in enumerate(_ir_clip(w, h, 2 * IR.cycle(cw, N) + 4)):
        e.encode(fr)
        for k, v in IR.check_structure(e.debug(), t, cw, N, ip).items():
            total[k] = total.get(k, 0) + v
    e.close()
    assert total["band"] > 0 and total["clean"] > 0 and total["last"] > 0 and total["excluded_matter"] > 0, total


def test_intra_refresh_bound_decides_vectors_on_a_pan():
    """content moving right to left: a clean block's match lies to its right, in what the reference picture has not cleaned.  The option changes such vectors"""
    w, h, N = 320, 192, 5
    frames = pan_content.clip(w, h, IR.cycle(w, N) + 2, 6, 0)
    mvs = []
    for on in (0, N):
        e = enckit.oracle_encoder(w, h, opts=(("intra-refresh", on),), qp=32, me_range=8, subme=2)
        out = []
        for t, fr in enumerate(frames):
            e.encode(fr)
            d = e.debug()
            if on:
                IR.check_structure(d, t, w, N, 0)
            out.append(d)
        e.close()
        mvs.append(out)
    changed = 0
    for t in range(1, len(frames)):
        j, s, _, _ = IR.record(w, N, t)
        if j >= 1:
            inter = (mvs[0][t]["cu_intra"][:, :s // 8] == 0) & (mvs[1][t]["cu_intra"][:, :s // 8] == 0)
            changed += int((inter & (mvs[0][t]["cu_mv"][:, :s // 8] != mvs[1][t]["cu_mv"][:, :s // 8]).any(axis=2)).sum())
    assert changed > 0


# ---- 4. the checker's own closed loop over the tool set: oracle/hevc_dec.c with the MD5 SEI, the 128x64 streams in tests/pyhevc.py too
CLOSED = [
    dict(change="offset", opts=(("weightp", 1),)), dict(change="gain", kw=dict(subme=2), opts=(("weightp", 1),)), dict(change="flash", kw=dict(subme=4, sao=1), opts=(("weightp", 1),)),
    dict(change="gain", n=3, tmvp=1, kw=dict(subme=2), opts=(("weightp", 1),)), dict(change="offset", n=2, kw=dict(subme=2), opts=(("weightp", 1), ("intra-in-p", 1), ("me-source", 1))),
    dict(change="flash", n=3, kw=dict(wpp=0, tile_rows=2, tile_cols=2, slices=2, subme=2), opts=(("weightp", 1),)), dict(change="offset", kw=dict(slices=1, subme=2), w=200, h=120, opts=(("weightp", 1),)),
    dict(change="gain", kw=dict(bitrate=400000, rc_bands=4, subme=2), opts=(("weightp", 1), ("rdoq", 1), ("signhide", 1))), dict(change="flash", n=2, coarse=64, w=384, h=256, opts=(("weightp", 1),)),
    dict(change="gain", n=3, tmvp=1, gop=(4, 3), kw=dict(subme=2), opts=(("weightp", 1),)), dict(change="none", n=2, kw=dict(subme=2), opts=(("weightp", 1),)),
    dict(N=5), dict(N=5, kw=dict(subme=4, sao=1)), dict(N=5, kw=dict(subme=2), opts=(("rdoq", 1), ("signhide", 1))), dict(N=5, change="offset", kw=dict(subme=2), opts=(("weightp", 1),)),
    dict(N=5, kw=dict(subme=2), opts=(("me-source", 1), ("intra-in-p", 1))), dict(N=5, kw=dict(bitrate=400000, rc_bands=4, subme=2)), dict(N=5, kw=dict(slices=1, subme=2)),
    dict(N=5, kw=dict(subme=4), opts=(("intra-in-p", 0),)), dict(N=5, kw=dict(subme=2), opts=(("intra-in-p", 2), ("rdoq", 1))), dict(N=5, kw=dict(period=4, subme=2), opts=(("intra-in-p", 1),)),
    dict(N=5, kw=dict(period=0)), dict(N=10), dict(N=8, w=200, h=120, kw=dict(subme=2, sao=1)), dict(N=4, w=640, h=384, kw=dict(subme=2)), dict(N=5, kw=dict(wpp=0, subme=2)),
    dict(N=5, kw=dict(deblock=0), opts=(("intra-in-p", 1),)), dict(N=255, kw=dict(subme=2)),
    dict(N=2, w=128, h=64, kw=dict(me_range=8, subme=2), pyhevc=True), dict(N=2, w=128, h=64, kw=dict(me_range=8, sao=1), opts=(("intra-in-p", 2),), pyhevc=True),
    dict(change="offset", n=2, w=128, h=64, kw=dict(me_range=8), opts=(("weightp", 1),), frames=5, pyhevc=True),
    dict(change="gain", w=128, h=64, kw=dict(me_range=8, subme=2), opts=(("weightp", 1),), frames=5, pyhevc=True),
]


@pytest.mark.parametrize("cfg", CLOSED, ids=[str(i) for i in range(len(CLOSED))])
def test_closed_loop(cfg):
    w, h, N = cfg.get("w", 320), cfg.get("h", 192), cfg.get("N", 0)
    nf = cfg.get("frames", min(2 * IR.cycle(_cw(w), N) + 4, 14) if N else 8)
    kw = dict(dict(qp=32, me_range=12 if not N else 8), **cfg.get("kw", {}))
    opts = (("hash", 2),) + tuple(cfg.get("opts", ())) + ((("intra-refresh", N),) if N else ())
    e = enckit.oracle_encoder(w, h, cfg.get("n"), cfg.get("tmvp"), cfg.get("coarse"), cfg.get("gop"), opts=opts, **kw)
    od = orc.OracleDecoder()
    pairs, weighted, seis = [], 0, 0
    for t, f in enumerate(WP.change(_ir_clip(w, h, nf), w, h, cfg.get("change", "none"))):
        au = e.encode(f)
        rec = e.recon()
        d = e.debug()
        weighted += int(d["wp"][0][0]) if "wp" in d else 0
        sei = [n for n in pyhevc.split_nals(au) if (n[0] >> 1) & 63 == 39]
        if N:                                           # only a cycle's first picture carries the recovery point SEI, in front of its first slice segment
            assert len(sei) == (1 if d["ir"][0] == 0 else 0), t
            if sei:
                assert bytes(pyhevc.unescape(sei[0])[2:]) == IR.recovery_point_sei(d["ir"][3] - 1)
                assert (pyhevc.split_nals(au)[0][0] >> 1) & 63 == 39
                seis += 1
        else:
            assert not sei
        pairs.append((au, rec))
        got = od.decode_au(au, t)
        assert len(got) == 1 and np.array_equal(got[0]["i420"], rec), "picture %d: oracle/hevc_dec.c differs from the reconstruction" % t
    checked, bad = od.hash_stats()
    assert checked == nf and bad == 0, (checked, bad)
    od.close(); e.close()
    if N:
        assert seis >= 1
    if cfg.get("change", "none") != "none":
        assert weighted >= 2, weighted
    if cfg.get("pyhevc"):
        from deckit import tabs
        dec = pyhevc.Decoder(tabs())
        for au, _ in pairs:
            dec.decode(au)
        pics = dec.flush()
        assert len(pics) == nf
        for t, p in enumerate(pics):
            assert np.array_equal(p["i420"], pairs[t][1]), "picture %d: tests/pyhevc.py differs" % t


# ---- 5. recovery: one access unit lost, the checker's decoder
@pytest.mark.parametrize("where", ["before-a-cycle", "mid-cycle"])
def test_a_lost_picture_is_healed_by_the_next_cycle(where):
    """Left of e_j - 4 every picture of the first cycle that begins after the loss is the encoder's, and every picture behind that cycle entirely (DESIGN.md
    section 9f, "why it is exact"); the same clip and loss without the option still differ there"""
    w, h, N = 320, 192, 5
    n = IR.cycle(w, N)
    lost = n if where == "before-a-cycle" else 1 + n // 2
    frames = _ir_clip(w, h, 2 * n + 4)

    def stream(on):
        e = enckit.oracle_encoder(w, h, opts=(("intra-in-p", 1),) + ((("intra-refresh", on),) if on else ()), qp=32, me_range=8, subme=2, sao=1)
        out = [(e.encode(f), e.recon()) for f in frames]
        e.close()
        return out

    def decode(pairs):
        od = orc.OracleDecoder()
        got = []
        for t, (au, _) in enumerate(pairs):
            if t != lost:
                got += od.decode_au(au, t)
        got += od.flush()
        assert od.concealed() > 0
        od.close()
        return {f["pts"]: f["i420"] for f in got}

    pairs = stream(N)
    got = decode(pairs)
    assert sorted(got) == [t for t in range(len(pairs)) if t != lost]
    assert not np.array_equal(got[lost + 1], pairs[lost + 1][1])              # (the loss does damage: the test is about something)
    for t in range(n + 1, len(pairs)):
        j, s, e_, _ = IR.record(w, N, t)
        lim = w if (t > 2 * n or e_ == w) else min(w, e_ - 4)
        for c, (a, b) in enumerate(zip(enckit.planes(got[t], w, h), enckit.planes(pairs[t][1], w, h))):
            k = lim if c == 0 else lim // 2
            assert np.array_equal(a[:, :k], b[:, :k]), "picture %d (position %d, band [%d, %d)), plane %d: %d samples differ left of column %d" % (
                t, j, s, e_, c, int((a[:, :k] != b[:, :k]).sum()), k)
    plain = stream(0)
    got = decode(plain)
    assert not np.array_equal(got[2 * n][:w * h], plain[2 * n][1][:w * h])
    assert not np.array_equal(got[len(plain) - 1][:w * h], plain[-1][1][:w * h])


# ---- 6. recorded digests
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "weightp_intra_refresh_access_units.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("idx", range(len(_golden())))
def test_recorded_digests(idx):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_weightp_intra_refresh_digests as mk
    case = _golden()[idx]
    got = mk.digests(dict(case["config"], opts=[tuple(o) for o in case["config"]["opts"]]))
    for t, want in enumerate(case["frames"]):
        assert got[t] == want, (idx, t)
    assert len(got) == len(case["frames"])
