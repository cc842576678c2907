"""GPU: "uvgx low-delay GOP v1" (kvazaar.h lp-gop) -- gop=lp-g<g>d<d>t1 taking effect: QP layers and key-picture references.

The feature is held to four things: every stream's structure, read from the stream alone, is the one tests/lp_gop_model.py states; the integer search equals
tests/lp_refs_model.search() handed the model's reference planes and the picture's QP; every reconstruction equals what the checker's decoder, the library's
HIP decoder and (a subset) tests/pyhevc.py make of the stream; and the gop string without the switch, or the switch without the string, changes nothing.  The checker's encoder states
the option itself (oracle/hevc_enc.c "lp-gop"); tests/test_gpu_coarse_gop_oracle.py holds the HIP encoder to it bit for bit."""
import numpy as np
import pytest

import enckit
import lp_gop_model as M
import lp_gop_stream
import lp_refs_model
import occluder_content
import pyhevc
from cases import GDN, LP_GOP_ROWS as ROWS, LP_REFS_SEARCH as SEARCH


def _gop(g, d, n, on=1):
    return (("lp-refs", n), ("gop", "lp-g%dd%dt1" % (g, d)), ("lp-gop", on))


# ---- 1. the structure, from the stream alone
@pytest.mark.gpu
@pytest.mark.parametrize("period", [5, 12, 13])       # (13: a multiple of no g above -- the count restarts at the IDR picture for every row)
@pytest.mark.parametrize("gdn", GDN)
def test_structure_from_the_stream(gpu, gdn, period):
    g, d, n = gdn
    w, h, qp, nf = 128, 64, 30, 2 * period + 3
    ge = enckit.encoder(w, h, _gop(g, d, n) + (("period", period), ("qp", qp), ("me-range", 8)))
    want = M.structure(period, nf, g, d, n, qp)
    sps = pps = None
    try:
        for i, fr in enumerate(enckit.frames(0, w, h, nf)):
            au, _ = ge.encode(fr)
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
            # what the encoder says it planned: kvz_frame_info and debug_all()
            assert ge.info["qp"] == m["qp"] and ge.info["poc"] == m["poc"]
            gp = ge.debug_all()["lp_gop"]
            assert gp["active"] == 1 and gp["qp"] == m["qp"] and gp["layer"] == m["layer"] and gp["dists"] == m["dists"], (i, gp, m)
            if not m["idr"]:
                assert ge.info["ref_list"] == m["refs"], (i, ge.info, m)
    finally:
        ge.close()


# ---- 2. the integer search against the model
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SEARCH)
def test_integer_search_matches_the_model(gpu, cfg):
    w, h, n, R, qp = cfg["w"], cfg["h"], cfg["n"], cfg["R"], cfg.get("qp", 32)
    g, d, nf = 4, 3, 7
    tiles = cfg.get("tiles", "1x1"); tc, tr = [int(v) for v in tiles.split("x")]
    opts = (("qp", qp), ("me-range", R), ("subme", 0), ("me-early-termination", "on" if cfg["me_early"] else "off"), ("me-source", cfg.get("me_source", 0)),
            ("mv-constraint", ("none", "frame", "frametilemargin")[cfg.get("mv_frame", 0)])) + ((("tiles", tiles),) if tiles != "1x1" else ())
    ge = enckit.encoder(w, h, _gop(g, d, n) + opts)
    # background that pictures 1 .. 4 cover and picture 5 shows again: only the key picture (POC 0, five pictures back) holds it
    frames = occluder_content.blink_clip(w, h, nf, kind=cfg["kind"])
    y0, y1, x0, x1 = occluder_content.region(w, h)
    recs, far = [], 0
    try:
        for t, fr in enumerate(frames):
            au, rec = ge.encode(fr)
            recs.append(rec)
            if t == 0:
                continue
            dd = ge.debug_all()
            dists = M.ref_dists(t, g, n)
            assert dd["lp_gop"]["dists"] == dists
            src = (frames if cfg.get("me_source") else recs)
            refs = [src[t - k][:w * h].reshape(h, w) for k in dists]
            log2, mv, rf = lp_refs_model.search(fr[:w * h].reshape(h, w), refs, M.picture_qp(qp, t, g, d), R, tile_rows=tr, tile_cols=tc, mv_frame=cfg.get("mv_frame", 0), me_early=cfg["me_early"])
            for name, a, b in (("cu_log2", log2, dd["cu_log2"]), ("cu_ref", rf, dd["cu_ref"]), ("cu_mv", mv, dd["cu_mv"])):
                bad = np.argwhere(np.asarray(a != b))
                assert not len(bad), "picture %d: %s differs at %d entries, first %s (model %s gpu %s)" % (t, name, len(bad), bad[0].tolist(), a[tuple(bad[0][:a.ndim])], b[tuple(bad[0][:b.ndim])])
            if max(dists) > n:
                k = dists.index(max(dists))
                assert t - max(dists) == ((t - 2) // g) * g                      # the far reference is the key picture
                far += int((dd["cu_ref"][y0 // 8:y1 // 8, x0 // 8:x1 // 8] == k).sum())
        assert far > 0, "no block chose the key picture at a distance beyond lp-refs"
    finally:
        ge.close()


# ---- 3. closed loop over the tool set


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ROWS, ids=[str(i) for i in range(len(ROWS))])
def test_closed_loop_decodes_to_the_reconstruction(gpu, cfg):
    w, h = cfg.get("w", 320), cfg.get("h", 192)
    owf = int(dict(cfg.get("opts", ())).get("owf", cfg.get("owf", 0)))
    opts = (("owf", owf), ("me-range", 12)) + tuple(cfg.get("opts", ()))
    br = cfg.get("bitrate", 0)
    if br:
        opts += (("bitrate", br),)
    fields = dict(cfg.get("fields", {}), **({"target_bitrate": br} if br else {}))
    ge = enckit.encoder(w, h, _gop(cfg.get("g", 4), cfg.get("d", 3), cfg["n"]) + opts, fields=fields or None)
    if cfg.get("roi"):
        import ctypes as C
        deltas = (np.arange(12, dtype=np.int8) % 7 - 3).astype(np.int8)
        ge._roi = deltas
        for pic in ge.pics:
            pic.contents.roi.width, pic.contents.roi.height = 4, 3
            pic.contents.roi.roi_array = deltas.ctypes.data_as(C.POINTER(C.c_int8))
    frames = enckit.frames(cfg.get("kind", 0), w, h, cfg.get("frames", 10))
    pairs = enckit.encode_all(ge, frames, owf)
    ge.close()
    enckit.closed_loop(pairs, sei=cfg.get("sei", False))


@pytest.mark.gpu
def test_closed_loop_smallest_case_also_matches_pyhevc(gpu):
    w, h = 128, 64
    for n, extra in ((3, ()), (2, (("tmvp", 1),))):
        ge = enckit.encoder(w, h, _gop(4, 3, n) + (("me-range", 8),) + extra)
        pairs = enckit.encode_all(ge, occluder_content.blink_clip(w, h, 7))
        ge.close()
        enckit.closed_loop(pairs, pyhevc_too=True)


@pytest.mark.gpu
def test_closed_loop_decodes_scaled_amvp(gpu):
    """a stream in which adjacent inter CUs hold references of different distance with a non-merged CU among them (counted from debug_all()): the decoders
    scale a neighbour's vector by the true POC distances (8.5.3.2.7) to read its vector differences"""
    w, h, g, d, n = 320, 192, 4, 3, 3
    ge = enckit.encoder(w, h, _gop(g, d, n) + (("qp", 22), ("me-range", 12), ("me-early-termination", "off"), ("tmvp", 1)))
    frames = enckit.frames(2, w, h, 10)
    pairs, count = [], 0
    for t, fr in enumerate(frames):
        au, rec = ge.encode(fr)
        pairs.append((au, rec))
        if t < 2:
            continue
        dd = ge.debug_all()
        dist = np.asarray(M.ref_dists(t, g, n) + [0] * 4)[dd["cu_ref"].astype(np.int32)]
        inter, amvp = dd["cu_intra"] == 0, (dd["cu_flags"] & 2) == 0
        for a, b in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
            count += int((inter[a] & inter[b] & (dist[a] != dist[b]) & (amvp[a] | amvp[b])).sum())
    ge.close()
    assert count > 0, "no non-merged CU beside a CU with a reference of another distance"
    enckit.closed_loop(pairs, pyhevc_too=False)


@pytest.mark.gpu
def test_closed_loop_1080p(gpu):
    w, h = 1920, 1080
    ge = enckit.encoder(w, h, _gop(4, 3, 3) + (("preset", "veryfast"), ("tmvp", 1)))
    pairs = enckit.encode_all(ge, enckit.frames(0, w, h, 10))
    ge.close()
    enckit.closed_loop(pairs)


# ---- 4. off is off
@pytest.mark.gpu
@pytest.mark.parametrize("opts", [(("lp-refs", 3),), (("lp-refs", 2), ("subme", 2), ("sao", "full"), ("tmvp", 1), ("intra-in-p", 1)), (("tiles", "2x2"), ("owf", 3), ("me-source", 1), ("lp-refs", 4), ("period", 5))])
def test_the_string_alone_and_the_switch_alone_change_nothing(gpu, opts):
    from kvazzup_amd.codec import Encoder
    w, h = 320, 192
    frames = enckit.frames(0, w, h, 9)
    owf = dict(opts).get("owf", 0)

    def run(extra, gop_default=True):
        from kvazzup_amd import codec
        keep = codec.DEFAULT_OPTIONS
        if not gop_default:                             # (the wrapper passes uvgComm's gop string by default: the baseline is a run with neither option)
            codec.DEFAULT_OPTIONS = tuple(kv for kv in keep if kv[0] != "gop")
        try:
            ge = Encoder(w, h, options=tuple(opts) + extra)
        finally:
            codec.DEFAULT_OPTIONS = keep
        assert not ge.rejected, ge.rejected
        out = enckit.encode_all(ge, frames, owf)
        ge.close()
        return out
    want = run((), gop_default=False)
    assert want[1][0] == run((("lp-gop", 1),), gop_default=False)[1][0]
    for extra in ((("gop", "0"),), (("gop", "lp-g4d3t1"), ("lp-gop", 0)), (("gop", "lp-g4d3t1"),), (("gop", "0"), ("lp-gop", 1))):
        got = run(extra)
        for t in range(len(frames)):
            assert got[t][0] == want[t][0] and np.array_equal(got[t][1], want[t][1]), (extra, t)


# ---- 5. what encoder_open refuses
@pytest.mark.gpu
@pytest.mark.parametrize("opts,word", [((("gop", "lp-g4d3t2"),), "sub-layers"), ((("gop", "lp-g4d7t1"),), "1 .. 6"),
                                       ((("gop", "lp-g4d3t1"), ("tiles", "1x2"), ("band-row0", 0), ("band-rows", 2)), "band mode")])
def test_encoder_open_refuses(gpu, capfd, opts, word):
    from kvazzup_amd.codec import Encoder
    with pytest.raises(RuntimeError):
        Encoder(256, 256, options=(("lp-gop", 1),) + opts)
    assert word in capfd.readouterr().err
