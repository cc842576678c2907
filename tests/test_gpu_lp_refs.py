"""GPU: "uvgx multi-reference v1" (kvazaar.h lp-refs) -- P pictures that refer to up to four previous pictures.

Here the feature is held to three things: with lp-refs 0 / 1 the encoder is the one-reference encoder byte for byte; the integer search equals
the numpy restatement tests/lp_refs_model.py (itself pinned to the checker by tests/test_lp_refs_host.py); and every picture's reconstruction
equals what the checker's decoder and the library's HIP decoder make of the stream (closed loop).  The checker's encoder states lp-refs itself,
and tests/test_gpu_lp_refs_oracle.py (run_case of tests/enckit.py) holds the HIP encoder to it bit for bit."""
import numpy as np
import pytest

import enckit
import orc
import lp_refs_model
from cases import LP_REFS_CLOSED as CLOSED, LP_REFS_SEARCH as SEARCH
from enckit import SEED


# ---- 1. guard: lp-refs 0 and 1 are the one-reference encoder
@pytest.mark.gpu
@pytest.mark.parametrize("opts", [(), (("subme", 2), ("sao", "full"), ("intra-in-p", 1)), (("tiles", "2x2"), ("owf", 3), ("me-source", 1))])
def test_lp_refs_0_and_1_are_the_one_reference_encoder(gpu, opts):
    w, h = 320, 192
    frames = enckit.frames(0, w, h, 5)
    owf = dict(opts).get("owf", 0)
    base = enckit.encoder(w, h, opts)
    want = enckit.encode_all(base, frames, owf)
    base.close()
    for n in (0, 1):
        ge = enckit.encoder(w, h, (("lp-refs", n),) + opts)
        got = enckit.encode_all(ge, frames, owf)
        ge.close()
        for t in range(len(frames)):
            assert got[t][0] == want[t][0] and np.array_equal(got[t][1], want[t][1]), (n, t)


# ---- 2. the integer search against the numpy restatement


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SEARCH)
def test_integer_search_matches_the_model(gpu, cfg):
    w, h, n, R, qp = cfg["w"], cfg["h"], cfg["n"], cfg["R"], cfg.get("qp", 32)
    tiles = cfg.get("tiles", "1x1"); tc, tr = [int(v) for v in tiles.split("x")]
    opts = (("qp", qp), ("me-range", R), ("subme", 0), ("me-early-termination", "on" if cfg["me_early"] else "off"), ("me-source", cfg.get("me_source", 0)),
            ("mv-constraint", ("none", "frame", "frametilemargin")[cfg.get("mv_frame", 0)])) + ((("tiles", tiles),) if tiles != "1x1" else ())
    ge = enckit.encoder(w, h, (("lp-refs", n),) + opts)
    frames = enckit.frames(cfg["kind"], w, h, cfg["frames"])
    recs = []
    try:
        for t, fr in enumerate(frames):
            au, rec = ge.encode(fr)
            recs.append(rec)
            if t == 0:
                continue
            d = ge.debug_all()
            nact = min(n, t)
            src = (frames if cfg.get("me_source") else recs)
            refs = [src[t - 1 - k][:w * h].reshape(h, w) for k in range(nact)]
            log2, mv, rf = lp_refs_model.search(fr[:w * h].reshape(h, w), refs, qp, R, tile_rows=tr, tile_cols=tc, mv_frame=cfg.get("mv_frame", 0), me_early=cfg["me_early"])
            for name, a, b in (("cu_log2", log2, d["cu_log2"]), ("cu_ref", rf, d["cu_ref"]), ("cu_mv", mv, d["cu_mv"])):
                bad = np.argwhere(np.asarray(a != b))
                assert not len(bad), "picture %d: %s differs at %d entries, first %s (model %s gpu %s)" % (t, name, len(bad), bad[0].tolist(), a[tuple(bad[0][:a.ndim])], b[tuple(bad[0][:b.ndim])])
            if nact > 1:
                assert d["cu_ref"].max() > 0 or cfg["kind"] == 1, "no block chose an older reference"
    finally:
        ge.close()


# ---- 3. closed loop over the tool set


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CLOSED, ids=[str(i) for i in range(len(CLOSED))])
def test_closed_loop_decodes_to_the_reconstruction(gpu, cfg):
    w, h = cfg.get("w", 320), cfg.get("h", 192)
    owf = int(dict(cfg.get("opts", ())).get("owf", cfg.get("owf", 0)))
    opts = (("owf", owf), ("me-range", 12)) + tuple(cfg.get("opts", ()))
    br = cfg.get("bitrate", 0)
    if br:
        opts += (("bitrate", br),)
    fields = dict(cfg.get("fields", {}), **({"target_bitrate": br} if br else {}))
    ge = enckit.encoder(w, h, (("lp-refs", cfg["n"]),) + opts, fields=fields or None)
    if cfg.get("roi"):
        import ctypes as C
        deltas = (np.arange(12, dtype=np.int8) % 7 - 3).astype(np.int8)
        ge._roi = deltas
        for pic in ge.pics:
            pic.contents.roi.width, pic.contents.roi.height = 4, 3
            pic.contents.roi.roi_array = deltas.ctypes.data_as(C.POINTER(C.c_int8))
    frames = enckit.frames(cfg.get("kind", 0), w, h, cfg.get("frames", 8))
    pairs = enckit.encode_all(ge, frames, owf)
    ge.close()
    enckit.closed_loop(pairs, sei=cfg.get("sei", False))


@pytest.mark.gpu
def test_closed_loop_smallest_case_also_matches_pyhevc(gpu):
    w, h = 128, 64
    ge = enckit.encoder(w, h, (("lp-refs", 3), ("me-range", 8)))
    pairs = enckit.encode_all(ge, enckit.frames(0, w, h, 5))
    ge.close()
    enckit.closed_loop(pairs, pyhevc_too=True)


@pytest.mark.gpu
def test_closed_loop_1080p_three_references(gpu):
    w, h = 1920, 1080
    ge = enckit.encoder(w, h, (("lp-refs", 3), ("preset", "veryfast")))
    pairs = enckit.encode_all(ge, enckit.frames(0, w, h, 8))
    ge.close()
    enckit.closed_loop(pairs)


# ---- 4. the benefit: picture t repeats picture t - 2
def _alternating(w, h, n):
    a = orc.synth_frame(2, SEED, w, h, 0)
    b = orc.synth_frame(0, SEED ^ 0x1234, w, h, 3)
    return [a if t % 2 == 0 else b for t in range(n)]


@pytest.mark.gpu
def test_two_alternating_scenes_use_the_older_reference(gpu):
    w, h, nf = 320, 192, 8
    frames = _alternating(w, h, nf)
    sizes = {}
    for n in (1, 2):
        ge = enckit.encoder(w, h, (("lp-refs", n), ("qp", 30)))
        sz, refs = [], []
        for t, f in enumerate(frames):
            au, _ = ge.encode(f)
            sz.append(len(au))
            if n == 2 and t >= 2:
                d = ge.debug_all()
                inter = d["cu_intra"] == 0
                refs.append((d["cu_ref"][inter] == 1).mean())
        ge.close()
        sizes[n] = sz
        if n == 2:
            assert min(refs) >= 0.9, refs
    p1, p2 = sum(sizes[1][2:]), sum(sizes[2][2:])
    assert p2 * 2 <= p1, (sizes[1], sizes[2])


# ---- 5. the public path: KvazaarFilter with the custom parameter, the wire adapter, OpenHEVCFilter
@pytest.mark.gpu
def test_filter_chain_with_three_references(gpu):
    from kvazzup_amd.pipeline import Pipeline
    w, h, nf = 320, 192, 8
    pl = Pipeline(w, h, settings={"video/QP": 30, "video/Intra": 64}, custom=(("me-range", 12), ("lp-refs", 3)))
    od = orc.OracleDecoder()
    try:
        clip = enckit.frames(0, w, h, nf)
        for f in clip:
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


# ---- 6. band mode refuses more than one reference
@pytest.mark.gpu
def test_band_mode_refuses_lp_refs(gpu, capfd):
    from kvazzup_amd.codec import Encoder
    with pytest.raises(RuntimeError):
        Encoder(256, 256, options=(("lp-refs", 2), ("tiles", "1x2"), ("band-row0", 0), ("band-rows", 2)))
    assert "band mode" in capfd.readouterr().err
