"""GPU: "uvgx coarse-to-fine search v1" (kvazaar.h me-coarse) -- a coarse search on quarter-resolution input pictures gives every 32x32
block and reference a centre, and k_me searches a second window around it.

T1: absent and with me-coarse=0 the encoder writes what the checker writes (the checker opened without the option: it stands for the encoder of before; with the option it states the feature itself, tests/test_gpu_coarse_gop_oracle.py).
T2: cu_log2 / cu_mv / cu_ref and the centres equal the numpy statement tests/me_coarse_model.py, every P picture.
T3: closed loop -- every reconstruction is what the checker's decoder and the HIP decoder make of the stream -- over the tool set, with vectors that leave the picture.
T4: what it buys on the pan clip; T5: through the filter chain; T6: band mode refuses it."""
import numpy as np
import pytest

import enckit
import me_coarse_model
import orc
import pan_content
from cases import ME_COARSE_CLOSED as CLOSED, ME_COARSE_SEARCH as SEARCH
from enckit import SEED


def _clip(name, w, h, n):
    if name == "moving":
        return [orc.synth_frame(0, SEED, w, h, t) for t in range(n)]
    if name == "flat":
        return pan_content.flat_clip(w, h, n)
    return pan_content.clip(w, h, n, name[0], name[1])


# ---- T1 guard
GUARD = [dict(n=1), dict(n=1, subme=2, sao=1, intra_in_p=1), dict(n=1, tiles=(2, 2), owf=3, me_source=1, wpp=0), dict(n=3, tmvp=1)]


@pytest.mark.gpu
@pytest.mark.parametrize("clip", ["moving", (36, -20)], ids=["moving", "pan"])
@pytest.mark.parametrize("cfg", GUARD, ids=["plain", "subme2_sao_intra_in_p1", "tiles2x2_owf3_me_source1", "lp_refs3_tmvp1"])
def test_off_is_the_encoder_of_before(gpu, cfg, clip):
    w, h, nf = 320, 192, 5
    c = dict(dict(w=w, h=h, R=12), **cfg)
    frames = _clip(clip, w, h, nf)
    oe = enckit.checker(w, h, c)
    want = []
    for f in frames:
        au = oe.encode(f)
        want.append((au, oe.recon()))
    oe.close()
    tc, tr = c.get("tiles", (1, 1))
    base = (("qp", 32), ("period", 64), ("me-range", 12), ("wpp", c.get("wpp", 1)), ("tiles", "%dx%d" % (tc, tr)), ("sao", "full" if c.get("sao") else "off"),
            ("subme", c.get("subme", 0)), ("intra-in-p", c.get("intra_in_p", 0)), ("me-source", c.get("me_source", 0)), ("owf", c.get("owf", 0)),
            ("lp-refs", c["n"]), ("tmvp", c.get("tmvp", 0)))
    for extra in ((), (("me-coarse", 0),)):
        ge = enckit.encoder(w, h, base + extra)
        got = enckit.encode_all(ge, frames, c.get("owf", 0))
        if extra:
            assert "me_coarse" not in ge.debug_all()
        ge.close()
        for t in range(nf):
            assert got[t][0] == want[t][0], "picture %d (%s): access unit differs from the checker's, %d vs %d bytes" % (t, extra, len(got[t][0]), len(want[t][0]))
            assert np.array_equal(got[t][1], want[t][1]), "picture %d (%s): reconstruction differs from the checker's" % (t, extra)


# ---- T2 search = model


def _sid(c):
    return "_".join("%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in sorted(c.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SEARCH, ids=[_sid(c) for c in SEARCH])
def test_search_matches_the_model(gpu, cfg):
    w, h, n, R, qp, reach = cfg.get("w", 640), cfg.get("h", 384), cfg.get("n", 1), cfg.get("R", 16), cfg.get("qp", 32), cfg["reach"]
    tiles = cfg.get("tiles", "1x1"); tc, tr = [int(v) for v in tiles.split("x")]
    me_early = cfg.get("me_early", 1)
    opts = (("qp", qp), ("me-range", R), ("subme", 0), ("me-early-termination", "on" if me_early else "off"), ("me-source", cfg.get("me_source", 0)),
            ("mv-constraint", ("none", "frame", "frametilemargin")[cfg.get("mv_frame", 0)]), ("lp-refs", n), ("me-coarse", reach))
    opts += ((("tiles", tiles), ("wpp", 0)) if tiles != "1x1" else ())
    nf = cfg.get("frames", 3)
    if cfg["clip"] == "moving":
        frames = [orc.synth_frame(cfg.get("kind", 0), SEED, w, h, t) for t in range(nf)]
    else:
        frames = pan_content.clip(w, h, nf, *cfg["clip"])
    ge = enckit.encoder(w, h, opts)
    srcs, recs = [], []
    longest = 0
    try:
        for t, fr in enumerate(frames):
            ge.encode(fr)
            d = ge.debug_all()
            srcs.append(d["src0"]); recs.append(d["rec0"])                     # the padded input plane and the coded reconstruction plane
            if t == 0:
                continue
            nact = min(n, t)
            refs_in = [srcs[t - 1 - k] for k in range(nact)]
            refs = refs_in if cfg.get("me_source") else [recs[t - 1 - k] for k in range(nact)]
            det = {}
            log2, mv, rf, cen = me_coarse_model.search(srcs[t], refs, qp, R, tile_rows=tr, tile_cols=tc, mv_frame=cfg.get("mv_frame", 0), me_early=me_early,
                                                       me_coarse=reach, refs_in=refs_in, detail=det)
            for name, a, b in (("cu_log2", log2, d["cu_log2"]), ("cu_ref", rf, d["cu_ref"]), ("cu_mv", mv, d["cu_mv"])):
                bad = np.argwhere(np.asarray(a != b))
                assert not len(bad), "picture %d: %s differs at %d entries, first %s (model %s gpu %s)" % (t, name, len(bad), bad[0].tolist(), a[tuple(bad[0][:a.ndim])], b[tuple(bad[0][:b.ndim])])
            searched = ~det["early"]
            for k in range(nact):
                bad = np.argwhere((cen[k].astype(np.int16) != d["me_coarse"][k]).any(axis=2) & searched)
                assert not len(bad), "picture %d reference %d: centres differ at %d blocks, first %s (model %s gpu %s)" % (t, k, len(bad), bad[0].tolist(), cen[k][tuple(bad[0])], d["me_coarse"][k][tuple(bad[0])])
            longest = max(longest, int(np.abs(d["cu_mv"].astype(np.int32)).max()))
    finally:
        ge.close()
    if cfg["clip"] != "moving" and max(abs(cfg["clip"][0]), abs(cfg["clip"][1])) > 32:
        assert longest > 4 * 32, "no vector longer than 32 samples: the case does not leave the old window (longest %d quarter samples)" % longest


# ---- T3 closed loop over the tool set


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CLOSED, ids=[str(i) for i in range(len(CLOSED))])
def test_closed_loop_decodes_to_the_reconstruction(gpu, cfg):
    w, h = 640, 384
    owf = cfg.get("owf", 0)
    opts = (("owf", owf), ("me-range", 16), ("qp", 32), ("me-coarse", cfg.get("reach", 128))) + tuple(cfg.get("opts", ()))
    br = cfg.get("bitrate", 0)
    if br:
        opts += (("bitrate", br),)
    fields = dict(cfg.get("fields", {}), **({"target_bitrate": br} if br else {}))
    ge = enckit.encoder(w, h, opts, fields=fields or None)
    frames = pan_content.clip(w, h, cfg.get("frames", 6), *cfg["pan"])
    pairs = enckit.encode_all(ge, frames, owf)
    d = ge.debug_all()
    ge.close()
    if not br and "lossless" not in dict(cfg.get("opts", ())):
        assert int(np.abs(d["cu_mv"].astype(np.int32)).max()) > 4 * 32, "the case does not leave the old window"
    enckit.closed_loop(pairs, sei=cfg.get("sei", False))


@pytest.mark.gpu
def test_closed_loop_small_case_also_matches_pyhevc(gpu):
    w, h = 256, 128
    ge = enckit.encoder(w, h, (("me-range", 8), ("me-coarse", 64), ("subme", 2)))
    pairs = enckit.encode_all(ge, pan_content.clip(w, h, 4, 44, -36))
    d = ge.debug_all()
    ge.close()
    assert int(np.abs(d["cu_mv"].astype(np.int32)).max()) > 4 * 32
    enckit.closed_loop(pairs, pyhevc_too=True)


# ---- T4 what it buys
@pytest.mark.gpu
@pytest.mark.parametrize("subme", [0, 2])
def test_pan_costs_fewer_bytes(gpu, subme):
    w, h, nf = 640, 384, 8
    frames = pan_content.clip(w, h, nf, 72, -40)
    res = {}
    for mc in (0, 128):
        ge = enckit.encoder(w, h, (("qp", 32), ("me-range", 16), ("subme", subme), ("me-coarse", mc)))
        pairs = enckit.encode_all(ge, frames)
        ge.close()
        res[mc] = (sum(len(au) for au, _ in pairs[1:]), np.mean([enckit.psnr_y(rec, frames[t], w * h) for t, (_, rec) in enumerate(pairs) if t]))
    print("me-coarse 0: %d bytes of P pictures, %.3f dB; 128: %d bytes, %.3f dB" % (res[0] + res[128]))
    assert res[128][0] < res[0][0], res
    assert res[128][1] >= res[0][1] - 0.1, res


@pytest.mark.gpu
def test_flat_clip_does_not_change(gpu):
    w, h = 640, 384
    frames = _clip("flat", w, h, 5)
    out = []
    for mc in (0, 128):
        ge = enckit.encoder(w, h, (("qp", 32), ("me-coarse", mc)))
        out.append(enckit.encode_all(ge, frames))
        ge.close()
    for (a, ra), (b, rb) in zip(*out):
        assert a == b and np.array_equal(ra, rb)


# ---- T5 the public path
@pytest.mark.gpu
def test_filter_chain_with_me_coarse(gpu):
    from kvazzup_amd.pipeline import Pipeline
    w, h, nf = 640, 384, 6
    pl = Pipeline(w, h, settings={"video/QP": 32, "video/Intra": 64}, custom=(("me-coarse", 128),))
    od = orc.OracleDecoder()
    try:
        for f in pan_content.clip(w, h, nf, 72, -40):
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


# ---- T6 band mode refuses it
@pytest.mark.gpu
def test_band_mode_refuses_me_coarse(gpu, capfd):
    from kvazzup_amd.codec import Encoder
    with pytest.raises(RuntimeError):
        Encoder(256, 256, options=(("me-coarse", 64), ("tiles", "1x2"), ("band-row0", 0), ("band-rows", 2)))
    assert "band mode" in capfd.readouterr().err
