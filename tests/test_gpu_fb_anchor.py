"""GPU: "uvgx loss feedback v2" (kvazaar.h fb-anchor) -- a reported loss healed from a kept picture, the anchor.

The feature is held to: after a lost row segment or a lost access unit reported in time, the decoders have the encoder's pictures in all three planes from the v2
heal picture on, while the same loss without the report still differs; the heal picture's map and block records equal the model, every cell of a forced quarter is
an intra unit or refers to the anchor and at least one does refer to it, every other cell keeps v1's reach on the previous picture; the v2 heal picture's access
unit is smaller than v1's for the same report; a report that comes too late for an anchor gets v1's heal picture decision for decision; without a report every
reconstruction and every byte of slice data is that of fb-anchor=0; a later report that reaches behind an earlier heal picture's anchor takes that picture's
reference-1 cells for damaged; pipeline shapes, the tool set, and what encoder_open refuses.

The decoders: the library's HIP decoder with partial pictures (concealment modes 2 and 3), tests/partial_model.py, and the checker's decoder.  The checker's
decoder refuses an access unit that lost slice segments (error -1), so it takes the loss itself where a whole access unit is lost, and decodes the complete stream
of the row-segment cases (the closed loop: a v2 heal picture's two references and every kept set are read as the encoder meant them).

Clip: enckit.pan(320, 320, 10, 3, -2) -- over the anchor's distance of 4 pictures the motion is (12, -8), inside me-range 16.  qp 30."""
import functools

import numpy as np
import pytest

import deckit
import enckit
import fb_anchor_model as A
import fb_model as M
import ir_model
import orc
import partial_model as pm
import pyhevc

H, K = 8, 4
W = HT = 320
R = 16
N = 10
LOST, HEAL = 3, 6
BASE = (("qp", 30), ("period", 64), ("slices", "wpp"), ("subme", 2), ("sao", "full"), ("intra-in-p", 1), ("me-range", R))
FB = (("loss-feedback", H), ("fb-anchor", K))
REPORT = [(LOST, 15, 10)]      # row 3 of picture 3 is lost and takes the dependent segment of row 4 with it: what the receiver's damage log says
ARRAYS = ("cu_mv", "cu_intra", "cu_log2", "cu_ref")


def run(opts, frames, reports=None, owf=0, fields=None, want=(), times=False, w=W, h=HT):
    """the clip through the HIP encoder; reports = {t: [(poc, first, count)]} are made in front of picture t's encode call.  -> per picture (access unit,
    reconstruction, {"fb", "fba": the picture's records, "refs": kvz_frame_info.ref_list, the arrays named in `want`, "times": kernel_times of the picture})"""
    ge = enckit.encoder(w, h, tuple(opts) + (("owf", owf),), fields=fields)
    cw, ch = ge.coded_size()
    b8 = (ch // 8, cw // 8)
    shapes = {"cu_mv": (np.int16, b8 + (2,)), "cu_intra": (np.uint8, b8), "cu_log2": (np.uint8, b8), "cu_ref": (np.uint8, b8), "fb_map": (np.uint8, b8),
              "fb_blk": (np.uint8, (ch // 32, cw // 32, 2))}
    o = dict(opts)
    out = []
    try:
        if times:
            ge.set_profiling(1)
        for t in range(len(frames) + owf + 1):
            for r in (reports or {}).get(t, ()):
                got = ge.report_damage(*r)
                assert got == 1, "report_damage%r returned %d" % (tuple(r), got)
            au, rec = ge.encode(frames[t] if t < len(frames) else None)
            if au:
                d = {"fb": [int(v) for v in ge.debug("fb", np.int32, (4,))] if o.get("loss-feedback") else [0, 0, 0, 0],
                     "fba": [int(v) for v in ge.debug("fb_anchor", np.int32, (4,))] if o.get("fb-anchor") else [0, 0, 0, 0], "refs": list(ge.info["ref_list"])}
                for k in want:
                    d[k] = ge.debug(k, *shapes[k])
                if times:
                    d["times"] = ge.kernel_times(reset=True)
                out.append((au, rec, d))
    finally:
        ge.close()
    assert len(out) == len(frames), "%d pictures in, %d access units out" % (len(frames), len(out))
    return out


def differs(a, b):
    return not np.array_equal(a, b)


def hip_decode(arrives, mode=2):
    """{time stamp: i420} of what arrives [(t, access unit)], and the decoder's damage log"""
    from kvazzup_amd.codec import Decoder
    gd = Decoder(concealment=mode, partial_pictures=True)
    try:
        got = [f for t, au in arrives for f in gd.decode_au(au, t)] + gd.drain()
        log = gd.damage_log()
    finally:
        gd.close()
    return {f["pts"]: f["i420"] for f in got}, log


def model_decode(arrives, mode=2):
    return {p["poc"]: p["i420"] for p in pm.decode([au for _, au in arrives], deckit.tabs(), mode)[0]}


def checker_decode(arrives):
    od = orc.OracleDecoder()
    try:
        got = [f for t, au in arrives for f in od.decode_au(au, t)] + od.flush()
        assert od.concealed() > 0
    finally:
        od.close()
    return {f["pts"]: f["i420"] for f in got}


def starts_with_recovery_point(au):
    nals = pyhevc.split_nals(au)
    return (nals[0][0] >> 1) & 63 == 39 and bytes(pyhevc.unescape(nals[0])[2:]) == ir_model.recovery_point_sei(0)


def same_planes(name, pics, pairs, ts):
    for t in ts:
        for c, (a, b) in enumerate(zip(enckit.planes(pics[t], W, HT), enckit.planes(pairs[t][1], W, HT))):
            assert np.array_equal(a, b), "%s, picture %d, plane %d: %d samples differ" % (name, t, c, int((a != b).sum()))


@functools.lru_cache(maxsize=None)
def clip():
    return tuple(enckit.pan(W, HT, N, 3, -2))


def records(pairs, ts):
    return {k: tuple(pairs[k][2][n] for n in ARRAYS) for k in ts}


def heal_in_time(opts, owf=0, fields=None, modes=(2,), lost=None, want=(), reports_at=HEAL):
    """case 1's loss and report on the options: the run without the report, what arrives of it, the run with the receiver's own log handed in before picture
    `reports_at`, and the decoders' pictures of what then arrives"""
    lost = lost or {LOST: (3,)}
    plain = run(opts, clip(), owf=owf, fields=fields)
    assert all(len(pm.vcl_indices(p[0])) == HT // 64 for p in plain)
    arrives = pm.cut([p[0] for p in plain[:reports_at]], lost)
    _, log = hip_decode(arrives, modes[0])
    pairs = run(opts, clip(), {reports_at: log}, owf=owf, fields=fields, want=want)
    assert [p[0] for p in pairs[:reports_at]] == [p[0] for p in plain[:reports_at]], "a report changed a picture in front of the heal picture"
    arrives = arrives + [(t, pairs[t][0]) for t in range(reports_at, N)]
    decoded = [("the HIP decoder, mode %d" % m, hip_decode(arrives, m)[0]) for m in modes] + [("tests/partial_model.py, mode %d" % m, model_decode(arrives, m)) for m in modes]
    return plain, log, pairs, decoded


# ---- 1. a lost row segment, reported in time
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [2, 3])
def test_a_lost_row_segment_is_healed_from_the_anchor(gpu, mode):
    plain, log, pairs, decoded = heal_in_time(BASE + FB, modes=(mode,), want=ARRAYS + ("fb_map", "fb_blk"))
    assert log == REPORT, log
    for name, pics in decoded:
        for t in range(LOST, HEAL):
            assert differs(pics[t], pairs[t][1]), "%s, picture %d: the loss does no damage" % (name, t)
        same_planes(name, pics, pairs, range(HEAL, N))
    if mode == 2:
        # the control: the same loss without the report still differs; and the complete stream through the checker's decoder and the HIP decoder
        got, _ = hip_decode(pm.cut([p[0] for p in plain], {LOST: (3,)}), mode)
        assert differs(got[HEAL], plain[HEAL][1]) and differs(got[9], plain[9][1])
        enckit.closed_loop([(au, rec) for au, rec, _ in pairs])
    # structure
    d = pairs[HEAL][2]
    cw, ch = W, HT
    want_map = A.heal_map(cw, ch, records(pairs, range(1, HEAL)), {}, log, HEAL, H, 1)
    assert np.array_equal(want_map, M.heal_map(cw, ch, {k: v[:3] for k, v in records(pairs, range(1, HEAL)).items()}, log, HEAL, H, 1))
    assert np.array_equal(d["fb_map"], want_map), "%d cells of the map differ from the model" % int((d["fb_map"] != want_map).sum())
    want_blk = M.block_records(want_map, cw, ch, R)
    assert np.array_equal(d["fb_blk"], want_blk)
    assert 0 < want_map.sum() < want_map.size
    ref1 = 0
    for by in range(ch // 32):
        for bx in range(cw // 32):
            forced, code = int(want_blk[by, bx, 0]), int(want_blk[by, bx, 1])
            for k in range(4):
                cells = (slice(4 * by + 2 * (k >> 1), 4 * by + 2 * (k >> 1) + 2), slice(4 * bx + 2 * (k & 1), 4 * bx + 2 * (k & 1) + 2))
                f = (forced >> k) & 1
                for mv, intra, ref in zip(d["cu_mv"][cells].reshape(-1, 2), d["cu_intra"][cells].ravel(), d["cu_ref"][cells].ravel()):
                    assert A.cell_allowed(f, intra, ref, mv, code), "block (%d, %d) quarter %d (forced %d): intra %d, reference %d, vector %s, reach code %d" % (bx, by, k, f, intra, ref, mv.tolist(), code)
                ref1 += int(f and not d["cu_intra"][cells].any() and d["cu_ref"][cells].all())
    forced_q = sum(bin(int(v)).count("1") for v in want_blk[..., 0].ravel())
    print("v2 heal picture: %d damaged cells of %d, %d forced quarters of %d, %d of them inter units on the anchor" % (int(want_map.sum()), want_map.size, forced_q, (cw // 16) * (ch // 16), ref1))
    assert ref1 >= 1, "no forced quarter is an inter unit on the anchor: the clip shows nothing"
    assert d["fb"] == [1, 1, int(want_map.sum()), forced_q]
    assert d["fba"] == [1, LOST - 1, HEAL - (LOST - 1), ref1], d["fba"]
    assert [p[2]["fba"][0] for p in pairs] == [int(t == HEAL) for t in range(N)] and [p[2]["fb"][0] for p in pairs] == [int(t == HEAL) for t in range(N)]
    assert d["refs"] == [HEAL - 1, LOST - 1] and all(p[2]["refs"] == ([t - 1] if t else []) for t, p in enumerate(pairs) if t != HEAL), [p[2]["refs"] for p in pairs]
    assert all(not p[2]["cu_ref"].any() for t, p in enumerate(pairs) if t != HEAL)
    assert [starts_with_recovery_point(p[0]) for p in pairs] == [t == HEAL for t in range(N)]
    hd = A.Headers()
    for t, p in enumerate(pairs):
        sh, rps, poc, idr = hd.read(p[0])
        assert idr == (t == 0) and poc == t and (idr or (rps == A.rps(t, K, LOST - 1 if t == HEAL else None) and sh["nref"] == (2 if t == HEAL else 1))), (t, rps, sh["nref"])
    assert hd.dpb == K


# ---- 2. a lost access unit
@pytest.mark.gpu
def test_a_lost_access_unit_is_healed_from_the_anchor_alone(gpu):
    pairs = run(BASE + FB, clip(), {HEAL: [(LOST, 0, -1)]}, want=ARRAYS)
    arrives = [(t, p[0]) for t, p in enumerate(pairs) if t != LOST]
    d = pairs[HEAL][2]
    quarters = (W // 16) * (HT // 16)
    assert d["fb"][:2] == [1, 1] and d["fb"][3] == quarters, d["fb"]      # every quarter is forced
    assert d["fba"][:3] == [1, LOST - 1, HEAL - LOST + 1] and d["refs"] == [HEAL - 1, LOST - 1], (d["fba"], d["refs"])
    assert (d["cu_intra"].astype(bool) | (d["cu_ref"] == 1)).all(), "the heal picture holds a reference-0 cell"
    assert d["fba"][3] >= 1 and d["fba"][3] == int(((d["cu_intra"] == 0) & (d["cu_ref"] == 1))[::2, ::2].sum())
    assert starts_with_recovery_point(pairs[HEAL][0])
    for name, got in (("the checker's decoder", checker_decode(arrives)), ("the HIP decoder", hip_decode(arrives)[0]), ("tests/partial_model.py", model_decode(arrives))):
        assert differs(got[LOST + 1], pairs[LOST + 1][1]), name
        same_planes(name, got, pairs, range(HEAL, N))


# ---- 3. it is cheaper
@pytest.mark.gpu
@pytest.mark.parametrize("ip", [0, 1])
def test_the_v2_heal_picture_is_smaller_than_v1s(gpu, ip):
    base = tuple(o for o in BASE if o[0] != "intra-in-p") + (("intra-in-p", ip),)
    v2 = run(base + FB, clip(), {HEAL: REPORT}, times=True)
    v1 = run(base + (("loss-feedback", H), ("fb-anchor", 0)), clip(), {HEAL: REPORT}, times=True)      # the behaviour of before: the thing measured against
    assert v2[HEAL][2]["fba"][0] == 1 and v1[HEAL][2]["fb"][0] == 1 and v1[HEAL][2]["refs"] == [HEAL - 1]
    ny = W * HT
    size = lambda p: len(p[HEAL][0])
    print("intra-in-p %d: heal picture v2 %d bytes, Y-PSNR %.2f dB; v1 %d bytes, Y-PSNR %.2f dB; the picture before: %d bytes" % (
        ip, size(v2), enckit.psnr_y(v2[HEAL][1], clip()[HEAL], ny), size(v1), enckit.psnr_y(v1[HEAL][1], clip()[HEAL], ny), len(v1[HEAL - 1][0])))
    assert size(v2) < size(v1), "the v2 heal picture has %d bytes, v1's %d" % (size(v2), size(v1))
    if ip == 0:
        stage = lambda p: [p[HEAL][2]["times"][k][1] for k in ("k_intra_analyse<P>", "k_intra_recon<P>")]
        assert stage(v2) == [0, 0], "intra-in-p 0: the v2 heal picture launched an intra-in-P stage %s" % stage(v2)
        assert min(stage(v1)) >= 1, "intra-in-p 0: v1's heal picture launched no intra-in-P stage %s" % stage(v1)
        assert not v2[HEAL][2]["times"]["k_me"][1] == 0


# ---- 4. too late for an anchor
@pytest.mark.gpu
def test_a_report_too_late_for_an_anchor_gets_v1s_heal_picture(gpu):
    late = 8                                             # the anchor, picture 2, lies 6 pictures back: K = 4 does not keep it
    want = ("cu_mv", "cu_intra")
    v2 = run(BASE + FB, clip(), {late: REPORT}, want=want)
    v1 = run(BASE + (("loss-feedback", H),), clip(), {late: REPORT}, want=want)
    assert [p[2]["fb"][0] for p in v2] == [int(t == late) for t in range(N)] and not any(p[2]["fba"][0] for p in v2) and v2[late][2]["refs"] == [late - 1]
    assert v2[late][2]["fb"][3] > 0
    for t, (a, b) in enumerate(zip(v2, v1)):
        assert np.array_equal(a[1], b[1]), "picture %d: the reconstruction differs from fb-anchor=0's" % t
        assert a[2]["fb"] == b[2]["fb"], (t, a[2]["fb"], b[2]["fb"])
        assert np.array_equal(a[2]["cu_intra"], b[2]["cu_intra"]) and np.array_equal(a[2]["cu_mv"], b[2]["cu_mv"]), "picture %d: the decisions differ from fb-anchor=0's" % t


# ---- 5. no report
def vcl_nals(au):
    return [n for n in pyhevc.split_nals(au) if ((n[0] >> 1) & 63) < 32]


@pytest.mark.gpu
def test_without_a_report_the_slice_data_is_that_of_fb_anchor_0(gpu):
    on = run(BASE + FB, clip())
    off = run(BASE + (("loss-feedback", H),), clip())
    hd, hd0 = A.Headers(), A.Headers()
    for t, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a[1], b[1]), "picture %d: the reconstruction differs with the option on" % t
        na, nb = vcl_nals(a[0]), vcl_nals(b[0])
        assert len(na) == len(nb) and na[1:] == nb[1:], "picture %d: a dependent slice segment differs" % t
        # the first segment: the header states the kept set and is a byte or two longer; the slice data behind it is the same bytes
        sh, rps, poc, idr = hd.read(a[0])
        hd0.read(b[0])
        assert len(hd.data) > 0 and hd.data == hd0.data, "picture %d: the first segment's slice data differs (%d and %d bytes)" % (t, len(hd.data), len(hd0.data))
        assert (na[0] == nb[0]) if t == 0 else 0 <= len(na[0]) - len(nb[0]) <= 2, "picture %d: first segments of %d and %d bytes" % (t, len(na[0]), len(nb[0]))
        assert idr == (t == 0) and (idr or (rps == A.rps(t, K) and len(rps) == min(K, t) and [u for _, u in rps] == [1] + [0] * (len(rps) - 1) and sh["nref"] == 1)), (t, rps)
    assert hd.dpb == K and all(p[2]["fb"] == [0, 0, 0, 0] and p[2]["fba"] == [0, 0, 0, 0] for p in on)
    enckit.closed_loop([(au, rec) for au, rec, _ in on], pyhevc_too=True)


# ---- 6. a report that reaches behind an earlier heal picture's anchor
@pytest.mark.gpu
def test_a_report_behind_an_earlier_anchor_takes_its_cells_for_damaged(gpu):
    second = 9
    lost = {2: (1, 2), LOST: (3,)}
    plain = run(BASE + FB, clip())
    _, log = hip_decode(pm.cut([p[0] for p in plain[:HEAL]], lost))
    assert [r for r in log if r[0] == LOST] == REPORT and len(log) == 2 and log[0][0] == 2, log
    early, later = [r for r in log if r[0] == LOST], [r for r in log if r[0] == 2]
    pairs = run(BASE + FB, clip(), {HEAL: early, second: later}, want=ARRAYS + ("fb_map",))
    assert [p[2]["fb"][0] for p in pairs] == [int(t in (HEAL, second)) for t in range(N)]
    assert pairs[HEAL][2]["fba"][:3] == [1, 2, 4] and pairs[second][2]["fba"] == [0, 0, 0, 0] and pairs[second][2]["refs"] == [second - 1]      # a = 1 < c = 6: v1's heal picture
    want_map = A.heal_map(W, HT, records(pairs, range(3, second)), {HEAL: 2}, later, second, H, 1)
    got_map = pairs[second][2]["fb_map"]
    assert np.array_equal(got_map, want_map), "%d cells of the map differ from the model" % int((got_map != want_map).sum())
    r1 = (pairs[HEAL][2]["cu_ref"] == 1) & (pairs[HEAL][2]["cu_intra"] == 0)
    ignored = A.heal_map(W, HT, records(pairs, range(3, second)), {}, later, second, H, 1)
    assert r1.any() and int(want_map.sum()) > int(ignored.sum()), "the anchor flag adds no cell: the case shows nothing"
    arrives = pm.cut([p[0] for p in pairs], lost)
    for name, got in (("the HIP decoder", hip_decode(arrives)[0]), ("tests/partial_model.py", model_decode(arrives))):
        assert differs(got[second - 1], pairs[second - 1][1]), "%s: picture %d is whole, the anchor was not damaged" % (name, second - 1)
        same_planes(name, got, pairs, range(second, N))


# ---- 7. pipeline shapes
SHAPES = [dict(owf=3), dict(owf=2, pre=(("preset", "veryfast"),))]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SHAPES, ids=["owf3", "veryfast-owf2"])
def test_pipeline_shapes(gpu, cfg):
    plain, log, pairs, decoded = heal_in_time(cfg.get("pre", ()) + BASE + FB, owf=cfg["owf"])
    assert log == REPORT and pairs[HEAL][2]["fba"][:3] == [1, 2, 4] and pairs[HEAL][2]["fba"][3] >= 1, (log, pairs[HEAL][2]["fba"])
    for name, pics in decoded:
        assert any(differs(pics[t], pairs[t][1]) for t in range(LOST, HEAL)), name
        same_planes(name, pics, pairs, range(HEAL, N))
    enckit.closed_loop([(au, rec) for au, rec, _ in pairs])


# ---- 8. the tool set
TOOLS = [dict(opts=(("rdoq", 1), ("signhide", 1))), dict(opts=(("deblock", 0), ("sao", "off"))), dict(opts=(("rc-algorithm", "lambda"),), bitrate=600000), dict(opts=(("vaq", 8),))]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", TOOLS, ids=["rdoq-signhide", "no-filters", "bitrate", "vaq"])
def test_tool_set(gpu, cfg):
    br = cfg.get("bitrate", 0)
    opts = BASE + tuple(cfg["opts"]) + ((("bitrate", br),) if br else ()) + FB
    plain, log, pairs, decoded = heal_in_time(opts, fields={"target_bitrate": br} if br else None)
    assert pairs[HEAL][2]["fba"][:3] == [1, 2, 4] and pairs[HEAL][2]["fba"][3] >= 1, pairs[HEAL][2]["fba"]
    for name, pics in decoded:
        assert any(differs(pics[t], pairs[t][1]) for t in range(LOST, HEAL)), name
        same_planes(name, pics, pairs, [t for t in range(N) if not LOST <= t < HEAL])
    enckit.closed_loop([(au, rec) for au, rec, _ in pairs])


# ---- 9. what encoder_open refuses, and what report_damage returns
REFUSED = [dict(fields={"fb_anchor": 1}), dict(fields={"fb_anchor": 8}), dict(fields={"fb_anchor": -2}), dict(opts=(("loss-feedback", 4), ("fb-anchor", 5))), dict(opts=(("loss-feedback", 0), ("fb-anchor", 4))),
           dict(opts=(("fb-anchor", 6),), size=(1920, 1088)), dict(opts=(("fb-anchor", 6),), size=(3840, 2176)), dict(opts=(("weightp", 1),)),
           # what loss-feedback refuses
           dict(opts=(("lp-refs", 2),)), dict(opts=(("gop", "lp-g4d3t1"), ("lp-gop", 1))), dict(opts=(("tmvp", 1),)), dict(opts=(("me-coarse", 64),)), dict(opts=(("tiles", "2x1"),)),
           dict(opts=(("tiles", "1x2"), ("wpp", 0))), dict(opts=(("band-row0", 0), ("band-rows", 2))), dict(opts=(("lossless", 1),)), dict(opts=(("intra-chain", 0),)), dict(opts=(("intra-refresh", 8),))]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_encoder_open_refuses(gpu, capfd, cfg):
    from kvazzup_amd.codec import Encoder
    w, h = cfg.get("size", (256, 256))
    with pytest.raises(RuntimeError):
        Encoder(w, h, options=FB + tuple(cfg.get("opts", ())), fields=cfg.get("fields"))
    assert "fb-anchor" in capfd.readouterr().err


@pytest.mark.gpu
def test_the_largest_k_a_size_allows_opens(gpu):
    for (w, h), k in (((1280, 768), 7), ((1920, 1088), 5)):
        ge = enckit.encoder(w, h, (("loss-feedback", H), ("fb-anchor", k)))
        ge.close()


@pytest.mark.gpu
def test_report_damage_returns_what_it_did(gpu):
    w, h = 320, 192
    frames = enckit.pan(w, h, 2, 4, 2)
    ge = enckit.encoder(w, h, (("qp", 32),) + FB)
    try:
        assert ge.report_damage(0, 0, -1) == 2          # nothing has been coded
        for f in frames:
            ge.encode(f)
        n = (w // 64) * (h // 64)
        assert [ge.report_damage(1, a, c) for a, c in ((-1, 1), (n, 1), (n - 1, 2), (0, n + 1))] == [0, 0, 0, 0]
        assert ge.report_damage(-1, 0, 1) == 0 and ge.report_damage(2, 0, 1) == 2
        assert ge.report_damage(1, n - 1, 1) == 1 and ge.report_damage(0, 0, n) == 1
    finally:
        ge.close()
