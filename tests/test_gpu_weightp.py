"""GPU: "uvgx weighted prediction v1" (kvazaar.h weightp) -- explicit weighted prediction of luma for brightness changes.

The feature is held to: every picture's record (flag, w, o per reference) equals tests/wp_model.py on the same input pictures; the integer search equals
tests/lp_refs_model.search() handed the model's search planes; every reconstruction equals what the checker's decoder, the library's HIP decoder and (the
smallest case) tests/pyhevc.py make of the stream; on an unchanged clip the reconstructions are the option-off encoder's and an access unit grows by the
table alone; on a clip that darkens the option saves bits.  The clips are the benchmark's synthetic clip with the changes of wp_model.change()."""
import numpy as np
import pytest

import enckit
from cases import WEIGHTP_CLOSED as CLOSED
import lp_gop_model
import lp_refs_model
import orc
import wp_model as M

KINDS = ("none", "offset", "gain", "flash")
# references per P picture, lp-gop (g, d) or None, me-source
SETUPS = {"one": (1, None, 0), "three": (3, None, 0), "one-src": (1, None, 1), "gop-src": (3, (4, 3), 1)}
ON = (("weightp", 1),)


def _record(ge):
    """the delivered picture's (flag, w, o) per reference"""
    return [tuple(int(v) for v in r) for r in ge.debug("wp", np.int32, (4, 3))]


def _clip(kind, w, h, n):
    """the benchmark clip (synth kind 0, seed 1234) with the change `kind` on its luma"""
    frames = M.change([orc.synth_frame(0, 1234, w, h, t) for t in range(n)], w, h, kind)
    return frames, [f[:w * h].reshape(h, w) for f in frames]


# ---- 1. the record and the integer search against the models
@pytest.mark.gpu
@pytest.mark.parametrize("setup", sorted(SETUPS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", [(320, 192), (640, 384)])
def test_record_and_search_match_the_models(gpu, size, kind, setup):
    w, h = size
    n, gop, me_source = SETUPS[setup]
    qp, R, nf = 32, 6, 7
    opts = (("qp", qp), ("me-range", R), ("subme", 0), ("lp-refs", n), ("me-source", me_source))
    if gop:
        opts += (("gop", "lp-g%dd%dt1" % gop), ("lp-gop", 1))
    frames, ys = _clip(kind, w, h, nf)
    ge = enckit.encoder(w, h, ON + opts)
    recs, weighted0 = [], 0
    try:
        for t, fr in enumerate(frames):
            au, rec = ge.encode(fr)
            recs.append(rec)
            d = ge.debug_all()
            got = [tuple(int(v) for v in r) for r in d["wp"]]
            if t == 0:
                assert got == [M.PLAIN] * 4
                continue
            dists = lp_gop_model.ref_dists(t, gop[0], n) if gop else list(range(1, min(n, t) + 1))
            want = M.record(ys, t, dists)
            assert got == want, (t, got, want)
            weighted0 += got[0][0]
            if w == 320:                                    # the search, on the planes the model makes of the planes the search would have read
                planes = frames if me_source else recs
                refs = [M.search_plane(planes[t - k][:w * h].reshape(h, w), want[i]) for i, k in enumerate(dists)]
                pqp = lp_gop_model.picture_qp(qp, t, gop[0], gop[1]) if gop else qp
                log2, mv, rf = lp_refs_model.search(ys[t], refs, pqp, R)
                for name, a, b in (("cu_log2", log2, d["cu_log2"]), ("cu_ref", rf, d["cu_ref"]), ("cu_mv", mv, d["cu_mv"])):
                    bad = np.argwhere(np.asarray(a != b))
                    assert not len(bad), "picture %d: %s differs at %d entries, first %s (model %s gpu %s)" % (t, name, len(bad), bad[0].tolist(), a[tuple(bad[0][:a.ndim])], b[tuple(bad[0][:b.ndim])])
    finally:
        ge.close()
    # the coverage: a silent "never weighted" (or "always") fails
    if kind in ("offset", "gain"):
        assert weighted0 == nf - 1, (kind, weighted0)
    if kind == "none":
        assert weighted0 == 0


# ---- 2. closed loop over the tool set (the rows: tests/cases.py WEIGHTP_CLOSED; tests/test_gpu_weightp_ir_oracle.py holds every one of them to the checker)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CLOSED, ids=[str(i) for i in range(len(CLOSED))])
def test_closed_loop_decodes_to_the_reconstruction(gpu, cfg):
    w, h, owf, br = cfg.get("w", 320), cfg.get("h", 192), cfg.get("owf", 0), cfg.get("bitrate", 0)
    opts = (("owf", owf), ("me-range", 12)) + tuple(cfg.get("opts", ())) + ((("bitrate", br),) if br else ())
    ge = enckit.encoder(w, h, ON + opts, fields={"target_bitrate": br} if br else None)
    frames, _ = _clip(cfg["kind"], w, h, 8)
    out = enckit.encode_all(ge, frames, owf, per_picture=_record)
    ge.close()
    weighted = sum(r[0][0] for _, _, r in out)
    assert (weighted == 0) if cfg["kind"] == "none" else (weighted >= 2), weighted      # (the streams exercise the weighted paths, the last one the plain path under the flag)
    enckit.closed_loop([(au, rec) for au, rec, _ in out])


@pytest.mark.gpu
def test_closed_loop_smallest_case_also_matches_pyhevc(gpu):
    w, h = 128, 64
    for kind, extra in (("offset", (("lp-refs", 2),)), ("gain", (("subme", 2),))):
        ge = enckit.encoder(w, h, ON + (("me-range", 8),) + extra)
        frames, _ = _clip(kind, w, h, 5)
        out = enckit.encode_all(ge, frames, per_picture=_record)
        ge.close()
        assert sum(r[0][0] for _, _, r in out) >= 2
        enckit.closed_loop([(au, rec) for au, rec, _ in out], pyhevc_too=True)


# ---- 3. an unchanged clip: the reconstructions of the encoder without the option, access units longer by the table alone
@pytest.mark.gpu
@pytest.mark.parametrize("opts", [(), (("lp-refs", 4), ("subme", 2), ("sao", "full"), ("tmvp", 1)), (("tiles", "2x2"), ("slices", "tiles"), ("owf", 3), ("me-source", 1), ("lp-refs", 3))])
def test_unchanged_clip_costs_the_table_alone(gpu, opts):
    import pyhevc
    w, h = 320, 192
    frames, _ = _clip("none", w, h, 7)
    owf = dict(opts).get("owf", 0)
    runs = []
    for on in (0, 1):
        ge = enckit.encoder(w, h, (("weightp", on), ("me-range", 12)) + tuple(opts))
        runs.append(enckit.encode_all(ge, frames, owf, per_picture=_record if on else None))
        ge.close()
    for t in range(len(frames)):
        off_au, off_rec = runs[0][t]
        on_au, on_rec, rec = runs[1][t]
        assert rec == [M.PLAIN] * 4, (t, rec)
        assert np.array_equal(on_rec, off_rec), t
        segments = sum(1 for nal in pyhevc.split_nals(on_au) if (nal[0] >> 1) & 63 in (1, 19))      # (slices=tiles: four independent segments; no dependent ones here)
        assert len(off_au) <= len(on_au) <= len(off_au) + 3 * segments, (t, len(on_au), len(off_au))
        if t == 0:
            assert on_au != off_au                          # (the PPS says weighted_pred_flag)


# ---- 4. the benefit, direction only: a 1080p clip that darkens by six levels a picture
@pytest.mark.gpu
def test_1080p_offset_clip_takes_fewer_bits(gpu):
    w, h = 1920, 1080
    frames, _ = _clip("offset", w, h, 5)
    bits = []
    for on in (0, 1):
        ge = enckit.encoder(w, h, (("weightp", on), ("qp", 32), ("me-range", 16)))
        aus = [ge.encode(fr, want_recon=False)[0] for fr in frames]
        if on:
            assert int(ge.debug("wp", np.int32, (4, 3))[0][0]) == 1      # (the last picture's record)
        ge.close()
        bits.append(8 * sum(len(a) for a in aus[1:]))
    print("1080p offset clip, bits of the four P pictures: option off %d, on %d" % tuple(bits))
    assert bits[1] < bits[0], bits


# ---- 5. what encoder_open refuses
@pytest.mark.gpu
@pytest.mark.parametrize("opts", [(("tiles", "1x2"), ("band-row0", 0), ("band-rows", 2)), (("lossless", 1),)])
def test_encoder_open_refuses(gpu, capfd, opts):
    from kvazzup_amd.codec import Encoder
    with pytest.raises(RuntimeError):
        Encoder(256, 256, options=(("weightp", 1),) + opts)
    assert "weightp" in capfd.readouterr().err
