"""GPU: "tmvp" (temporal motion vector prediction) -- merge and AMVP candidates from the previous picture's motion.

tmvp changes how motion is signalled, never which motion is chosen: k_me and k_subpel price a vector by mvd_bits() of the vector itself, not of its
difference to a predictor, and nothing after k_inter_signal reads the signalling but the tokenizer.  So at a constant QP the reconstruction with tmvp=1
is the reconstruction with tmvp=0, picture for picture, whatever else is switched on.  What breaks the equality is a bitrate: the picture-level rate
control follows the access units' sizes, which tmvp changes (the in-picture steps of rc-algorithm follow the levels' cost, which it does not change).
Those cases are held to the closed loop only: every reconstruction equals what the checker's decoder (md5 SEI verified), the HIP decoder (synchronous
and frame-threaded) and, for the small cases, tests/pyhevc.py make of the stream.  (The checker's encoder states tmvp itself: tests/test_gpu_lp_refs_oracle.py holds the HIP
encoder to it bit for bit, the bitrate cases included.)"""
import numpy as np
import pytest

import enckit
import hc
import orc
from hc import col_record


# ---- 4 + 5. the same pictures as without tmvp, and the closed loop
CASES = [
    dict(), dict(owf=2), dict(owf=6),
    dict(opts=(("lp-refs", 2),)), dict(opts=(("lp-refs", 3),), owf=2), dict(opts=(("lp-refs", 4),), owf=6),
    dict(opts=(("wpp", 0), ("tiles", "2x2"))), dict(opts=(("tiles", "2x2"), ("slices", "tiles"), ("wpp", 0), ("lp-refs", 3))),
    dict(opts=(("slices", "wpp"), ("lp-refs", 2))),
    dict(opts=(("intra-in-p", 1), ("subme", 4))), dict(opts=(("intra-in-p", 2), ("lp-refs", 4)), kind=2),
    dict(opts=(("subme", 4), ("sao", "full")), owf=2), dict(opts=(("me-source", 1), ("subme", 2), ("intra-in-p", 1), ("lp-refs", 3)), owf=6),
    dict(opts=(("period", 8), ("lp-refs", 3)), frames=19), dict(opts=(("period", 8),), owf=6, frames=19),
    dict(opts=(("gpu-entropy", 1), ("lp-refs", 2))), dict(opts=(("gpu-entropy", 1),), owf=2),
    dict(opts=(("preset", "veryfast"),), owf=2),
    dict(bitrate=400000, opts=(("lp-refs", 3),)), dict(bitrate=400000, opts=(("rc-algorithm", "lambda"), ("sao", "full"))),
    dict(sei=True, opts=(("lp-refs", 2), ("period", 8)), frames=10),
    dict(w=128, h=64, opts=(("lp-refs", 3), ("me-range", 8)), pyhevc=True, frames=6),
    dict(w=192, h=128, pan=True, opts=(("period", 4), ("intra-in-p", 1)), pyhevc=True, frames=6),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CASES, ids=[str(i) for i in range(len(CASES))])
def test_same_pictures_and_closed_loop(gpu, cfg):
    w, h = cfg.get("w", 320), cfg.get("h", 192)
    owf = cfg.get("owf", 0)
    br = cfg.get("bitrate", 0)
    opts = (("owf", owf), ("me-range", 12)) + tuple(cfg.get("opts", ())) + ((("bitrate", br),) if br else ())
    fields = dict(({"target_bitrate": br} if br else {}), **({"hash": 2} if cfg.get("sei") else {}))
    n = cfg.get("frames", 9)
    frames = enckit.pan(w, h, n) if cfg.get("pan") else enckit.frames(cfg.get("kind", 0), w, h, n)
    runs = {}
    for tmvp in (0, 1):
        ge = enckit.encoder(w, h, opts + (("tmvp", tmvp),), fields=fields or None)
        runs[tmvp] = enckit.encode_all(ge, frames, owf)
        ge.close()
    if not br:
        for t in range(n):
            assert np.array_equal(runs[0][t][1], runs[1][t][1]), "picture %d: tmvp changed the reconstruction" % t
    assert any(a[0] != b[0] for a, b in zip(runs[0], runs[1])), "tmvp changed no access unit"
    enckit.closed_loop(runs[1], sei=cfg.get("sei", False), pyhevc_too=cfg.get("pyhevc", False), frame_threaded=True)


# ---- 6. the decisions against the host derivation, the record against the picture's fields
DECISIONS = [
    dict(lp=1), dict(lp=3, opts=(("intra-in-p", 2),)), dict(lp=4, opts=(("tiles", "2x2"), ("wpp", 0))), dict(lp=2, opts=(("period", 4), ("subme", 4))),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", DECISIONS, ids=[str(i) for i in range(len(DECISIONS))])
def test_decisions_match_the_host_derivation(gpu, cfg):
    w, h, lp = 320, 192, cfg["lp"]
    opts = dict(cfg.get("opts", ()))
    period = int(opts.get("period", 64))
    tc, tr = [int(v) for v in opts.get("tiles", "1x1").split("x")]
    ge = enckit.encoder(w, h, (("me-range", 12), ("lp-refs", lp), ("tmvp", 1)) + tuple(cfg.get("opts", ())))
    cw, ch = ge.coded_size()
    frames = enckit.frames(0, w, h, 9)
    prev_col = None
    temporal_used = 0
    try:
        for t, fr in enumerate(frames):
            ge.encode(fr)
            poc = t % period
            if poc == 0:
                prev_col = None
                continue
            d = ge.debug_all()
            mvd = ge.debug("cu_mvd", np.int16, (ch // 8, cw // 8, 2))
            col = ge.debug("col", np.int16, (ch // 16, cw // 16, 4))
            assert np.array_equal(col, col_record(d["cu_intra"], d["cu_mv"], d["cu_ref"])), "picture %d: the collocated record" % t
            nact = min(max(lp, 1), poc)
            a = [d[k] for k in ("cu_log2", "cu_intra", "cu_mv", "cu_ref", "cu_cbf")]
            use = prev_col if poc >= 2 else None
            want = {}
            want["flags"], want["midx"], want["mvp"], wmvd, _ = hc.picture(cw, ch, tr, tc, nact, a, col=use)
            inter = d["cu_intra"] == 0
            for name, got, exp in (("cu_flags", d["cu_flags"], want["flags"]), ("cu_merge_idx", d["cu_merge_idx"], want["midx"]),
                                   ("cu_mvp_idx", d["cu_mvp_idx"], want["mvp"]), ("cu_mvd", mvd, wmvd)):
                bad = np.argwhere(inter & (np.any(got != exp, axis=-1) if got.ndim == 3 else (got != exp)))
                assert not len(bad), "picture %d: %s differs at %d units, first %s" % (t, name, len(bad), bad[0].tolist())
            if use is not None:
                f0 = {}
                f0["flags"], f0["midx"], f0["mvp"], _, _ = hc.picture(cw, ch, tr, tc, nact, a)
                temporal_used += int((inter & ((f0["flags"] != want["flags"]) | (f0["midx"] != want["midx"]) | (f0["mvp"] != want["mvp"]))).sum())
            prev_col = col
    finally:
        ge.close()
    assert temporal_used > 0


# ---- 7. exercised: a pan, where every block moves like its collocated block
@pytest.mark.gpu
def test_pan_uses_the_temporal_candidates(gpu):
    w, h = 320, 192
    ge = enckit.encoder(w, h, (("me-range", 12), ("tmvp", 1), ("qp", 30)))
    cw, ch = ge.coded_size()
    frames = enckit.pan(w, h, 6)
    prev_col, merged_t, amvp_t, inter_cus = None, 0, 0, 0
    try:
        for t, fr in enumerate(frames):
            ge.encode(fr)
            if t == 0:
                continue
            d = ge.debug_all()
            col = ge.debug("col", np.int16, (ch // 16, cw // 16, 4))
            if t >= 2:
                a = [d[k] for k in ("cu_log2", "cu_intra", "cu_mv", "cu_ref", "cu_cbf")]
                f0, i0, p0, _, _ = hc.picture(cw, ch, 1, 1, 1, a)
                inter = d["cu_intra"] == 0
                inter_cus += int(inter.sum())
                # merged where the derivation without the temporal candidate could not merge, or merged elsewhere: the temporal candidate
                merged_t += int((inter & (d["cu_flags"] & 2 != 0) & ((f0 & 2 == 0) | (i0 != d["cu_merge_idx"]))).sum())
                amvp_t += int((inter & (d["cu_flags"] == 0) & (p0 != d["cu_mvp_idx"])).sum())
            prev_col = col
    finally:
        ge.close()
    assert prev_col is not None and merged_t + amvp_t > 0, (merged_t, amvp_t, inter_cus)


# ---- 8. the default is off, byte for byte; band mode refuses it
@pytest.mark.gpu
def test_explicit_off_is_the_default(gpu):
    w, h = 320, 192
    frames = enckit.frames(0, w, h, 6)
    for opts in ((), (("lp-refs", 3), ("owf", 2), ("sao", "full"))):
        owf = int(dict(opts).get("owf", 0))
        a = enckit.encoder(w, h, opts)
        ra = enckit.encode_all(a, frames, owf)
        a.close()
        b = enckit.encoder(w, h, opts + (("tmvp", 0),))
        rb = enckit.encode_all(b, frames, owf)
        b.close()
        assert [x[0] for x in ra] == [x[0] for x in rb]


@pytest.mark.gpu
def test_band_mode_refuses_tmvp(gpu, capfd):
    from kvazzup_amd.codec import Encoder
    with pytest.raises(RuntimeError):
        Encoder(256, 256, options=(("tmvp", 1), ("tiles", "1x2"), ("band-row0", 0), ("band-rows", 2)))
    assert "tmvp" in capfd.readouterr().err


# ---- 9. the public path: KvazaarFilter with the custom parameter, the wire adapter, OpenHEVCFilter
@pytest.mark.gpu
def test_filter_chain_with_tmvp(gpu):
    from kvazzup_amd.pipeline import Pipeline
    w, h, nf = 320, 192, 8
    pl = Pipeline(w, h, settings={"video/QP": 30, "video/Intra": 64}, custom=(("me-range", 12), ("tmvp", 1)))
    od = orc.OracleDecoder()
    try:
        for f in enckit.frames(0, w, h, nf):
            pl.push(f)
        assert pl.wait(nf, 60000)
        for t in range(nf):
            au, pts = pl.pop_encoded()
            assert pts == t
            want = od.decode_au(au, t)
            d = pl.pop_decoded()
            assert len(want) == 1 and np.array_equal(d["i420"], want[0]["i420"]), "picture %d" % t
        st = pl.stats()
        assert st["encoded_pictures"] == nf and st["decoded_pictures"] == nf and st["dropped"] == 0
    finally:
        pl.close(); od.close()
