"""GPU: "uvgx loss feedback v1" (kvazaar.h loss-feedback) -- the receiver's loss report handed to the encoder, and the heal picture behind it.

The feature is held to: a decoder that lost a CTU row's segment, or a whole access unit, has the encoder's pictures in all three planes from the heal picture on
-- the library's HIP decoder with partial pictures, tests/partial_model.py and the checker's decoder -- while the same loss without the report still differs; the
heal picture's map and block records equal tests/fb_model.py run over the encoder's own motion fields, every forced quarter is intra and every vector keeps its
block's reach; reports of every age up to and past the ring; with the option on and no report the stream is the option-off stream byte for byte; the closed loop
over the tool set with a heal picture inside; and what encoder_open and report_damage refuse.  Pan clips (tests/enckit.py), qp 30 - 32."""
import functools

import numpy as np
import pytest

import deckit
import enckit
import fb_model as M
import ir_model
import orc
import partial_model as pm
import pyhevc

H = 8
BASE = (("qp", 30), ("period", 64), ("slices", "wpp"), ("subme", 2), ("sao", "full"), ("intra-in-p", 1), ("me-range", 16))


def _coded(w, h):
    return max(128, (w + 63) & ~63), (h + 63) & ~63


def run(w, h, opts, frames, reports=None, owf=0, fields=None, want=(), expect=1):
    """the clip through the HIP encoder; reports = {t: [(poc, first, count)]} are made in front of picture t's encode call.  -> [(access unit, reconstruction,
    {"fb": the picture's record} + the arrays named in `want`)]"""
    ge = enckit.encoder(w, h, tuple(opts) + (("owf", owf),), fields=fields)
    cw, ch = ge.coded_size()
    shapes = {"cu_mv": (np.int16, (ch // 8, cw // 8, 2)), "cu_intra": (np.uint8, (ch // 8, cw // 8)), "cu_log2": (np.uint8, (ch // 8, cw // 8)),
              "fb_map": (np.uint8, (ch // 8, cw // 8)), "fb_blk": (np.uint8, (ch // 32, cw // 32, 2))}
    out = []
    try:
        for t in range(len(frames) + owf + 1):
            for r in (reports or {}).get(t, ()):
                got = ge.report_damage(*r)
                assert got == expect, "report_damage%r returned %d" % (tuple(r), got)
            au, rec = ge.encode(frames[t] if t < len(frames) else None)
            if au:
                d = {"fb": [int(v) for v in ge.debug("fb", np.int32, (4,))]} if dict(opts).get("loss-feedback") else {"fb": [0, 0, 0, 0]}
                for k in want:
                    d[k] = ge.debug(k, *shapes[k])
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


# ---- 1. heal, partial loss
W1 = H1 = 320
LOST, HEAL = 3, 6


@functools.lru_cache(maxsize=None)
def clip1():
    return tuple(enckit.pan(W1, H1, 10, 12, -6))


@functools.lru_cache(maxsize=None)
def head1():
    """pictures 0 .. 5 (no report has been made: every run shares them), row 3's segment of picture 3 cut"""
    pairs = run(W1, H1, BASE + (("loss-feedback", H),), clip1()[:HEAL])
    aus = [au for au, _, _ in pairs]
    assert all(len(pm.vcl_indices(au)) == H1 // 64 for au in aus)
    return pairs, pm.cut(aus, {LOST: (3,)})


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [2, 3])
def test_a_lost_row_segment_is_healed_by_the_picture_behind_the_report(gpu, mode):
    head, arrives = head1()
    _, log = hip_decode(arrives, mode)
    assert log == [(LOST, 15, 10)], log                  # row 3 is lost and takes the dependent segment of row 4 with it
    pairs = run(W1, H1, BASE + (("loss-feedback", H),), clip1(), {HEAL: log}, want=("fb_blk",))
    assert [p[0] for p in pairs[:HEAL]] == [p[0] for p in head[:HEAL]], "a report changed a picture in front of the heal picture"
    arrives = arrives + [(t, pairs[t][0]) for t in range(HEAL, 10)]
    got, _ = hip_decode(arrives, mode)
    model = {p["poc"]: p["i420"] for p in pm.decode([au for _, au in arrives], deckit.tabs(), mode)[0]}
    for name, pics in (("the HIP decoder", got), ("tests/partial_model.py", model)):
        for t in range(LOST, HEAL):
            assert differs(pics[t], pairs[t][1]), "%s, picture %d: the loss does no damage" % (name, t)
        for t in range(HEAL, 10):
            for c, (a, b) in enumerate(zip(enckit.planes(pics[t], W1, H1), enckit.planes(pairs[t][1], W1, H1))):
                assert np.array_equal(a, b), "%s, mode %d, picture %d, plane %d: %d samples differ" % (name, mode, t, c, int((a != b).sum()))
    fb, blk = pairs[HEAL][2]["fb"], pairs[HEAL][2]["fb_blk"]
    assert [p[2]["fb"][0] for p in pairs] == [int(t == HEAL) for t in range(10)] and fb[1] == 1
    assert starts_with_recovery_point(pairs[HEAL][0]) and not any(starts_with_recovery_point(p[0]) for t, p in enumerate(pairs) if t != HEAL)
    print("heal picture: %d damaged cells of %d, %d forced quarters of %d, %d of %d blocks without one" % (fb[2], blk.shape[0] * blk.shape[1] * 16, fb[3], blk.shape[0] * blk.shape[1] * 4,
                                                                                                              int((blk[..., 0] == 0).sum()), blk.shape[0] * blk.shape[1]))
    assert fb[3] >= 1 and fb[3] == sum(bin(int(v)).count("1") for v in blk[..., 0].ravel())
    assert (blk[..., 0] == 0).sum() * 4 >= blk.shape[0] * blk.shape[1], "fewer than 25 % of the 32x32 blocks have no forced quarter"
    if mode == 2:
        # the control: the same run without the report still differs
        plain = run(W1, H1, BASE + (("loss-feedback", H),), clip1())
        got, _ = hip_decode(head1()[1] + [(t, plain[t][0]) for t in range(HEAL, 10)], mode)
        assert differs(got[HEAL], plain[HEAL][1]) and differs(got[9], plain[9][1])


# ---- 2. heal, lost access unit
@pytest.mark.gpu
def test_a_lost_access_unit_is_healed_by_a_picture_of_forced_quarters(gpu):
    pairs = run(W1, H1, BASE + (("loss-feedback", H),), clip1(), {HEAL: [(LOST, 0, -1)]})
    arrives = [(t, p[0]) for t, p in enumerate(pairs) if t != LOST]
    fb = pairs[HEAL][2]["fb"]
    assert fb[:2] == [1, 1] and fb[2] > 0 and fb[3] == (W1 // 16) * (H1 // 16), fb      # every quarter is forced
    assert starts_with_recovery_point(pairs[HEAL][0])
    for name, got in (("the checker's decoder", checker_decode(arrives)), ("the HIP decoder", hip_decode(arrives)[0])):
        assert differs(got[LOST + 1], pairs[LOST + 1][1]), name
        for t in range(HEAL, 10):
            assert np.array_equal(got[t], pairs[t][1]), "%s, picture %d: %d samples differ" % (name, t, int((got[t] != pairs[t][1]).sum()))


# ---- 3. structure against the model
STRUCT = [(w, h, ip) for w, h in ((320, 320), (200, 120), (640, 384)) for ip in (0, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,ip", STRUCT, ids=["%dx%d-ip%d" % s for s in STRUCT])
def test_the_heal_picture_has_the_structure_the_model_asks_for(gpu, w, h, ip):
    cw, ch = _coded(w, h)
    R, n, t = 16, 2, 5
    nctb = (cw // 64) * (ch // 64)
    report = (n, cw // 64 if ch > 64 * 2 else 1, cw // 64 if ch > 64 * 2 else 1)      # the second CTU row; two rows only: one block
    opts = (("qp", 32), ("period", 64), ("subme", 2), ("sao", "full"), ("intra-in-p", ip), ("me-range", R), ("loss-feedback", H))
    pairs = run(w, h, opts, enckit.pan(w, h, t + 1, 12, -6), {t: [report]}, want=("cu_mv", "cu_intra", "cu_log2", "fb_map", "fb_blk"))
    assert report[1] + report[2] <= nctb
    recs = {k: (pairs[k][2]["cu_mv"], pairs[k][2]["cu_intra"], pairs[k][2]["cu_log2"]) for k in range(1, t)}
    d = pairs[t][2]
    want_map = M.heal_map(cw, ch, recs, [report], t, H, 1)
    assert np.array_equal(d["fb_map"], want_map), "%d cells of the map differ from the model" % int((d["fb_map"] != want_map).sum())
    want_blk = M.block_records(want_map, cw, ch, R)
    assert np.array_equal(d["fb_blk"], want_blk)
    assert d["fb"] == [1, 1, int(want_map.sum()), sum(bin(int(v)).count("1") for v in want_blk[..., 0].ravel())]
    assert 0 < want_map.sum() < want_map.size
    on_bound = 0
    for by in range(ch // 32):
        for bx in range(cw // 32):
            forced, code = int(want_blk[by, bx, 0]), int(want_blk[by, bx, 1])
            for k in range(4):
                cells = (slice(4 * by + 2 * (k >> 1), 4 * by + 2 * (k >> 1) + 2), slice(4 * bx + 2 * (k & 1), 4 * bx + 2 * (k & 1) + 2))
                if (forced >> k) & 1:
                    assert d["cu_intra"][cells].all(), "block (%d, %d) quarter %d is forced and not intra" % (bx, by, k)
                    continue
                for mv, intra in zip(d["cu_mv"][cells].reshape(-1, 2), d["cu_intra"][cells].ravel()):
                    if not intra:
                        assert M.vector_within(mv, code), "block (%d, %d) quarter %d: vector %s beyond the reach code %d" % (bx, by, k, mv.tolist(), code)
                        on_bound += int(code == M.ZERO_ONLY or (code < R and max(abs(int(mv[0])), abs(int(mv[1]))) == 4 * code))
            if ip == 0 and forced == 0:
                assert not d["cu_intra"][4 * by:4 * by + 4, 4 * bx:4 * bx + 4].any(), "intra-in-p 0: an intra unit outside the forced quarters"
    assert on_bound >= 1, "no block sits on its bound or at the zero-only code"
    enckit.closed_loop([(au, rec) for au, rec, _ in pairs])


# ---- 4. delays and the ring
W4, H4 = 320, 192
OPTS4 = (("qp", 32), ("period", 64), ("slices", "wpp"), ("subme", 2), ("sao", "full"), ("intra-in-p", 1), ("me-range", 16), ("loss-feedback", H))


@pytest.mark.gpu
@pytest.mark.parametrize("late", [1, 2, 7, H, H + 1])
def test_a_report_of_any_age_heals(gpu, late):
    n, t = 2, 2 + late
    frames = enckit.pan(W4, H4, t + 2, 4, 2)
    pairs = run(W4, H4, OPTS4, frames, {t: [(n, 5, 10)]})
    arrives = pm.cut([p[0] for p in pairs], {n: (1,)})
    got, log = hip_decode(arrives)
    assert log == [(n, 5, 10)]
    fb = pairs[t][2]["fb"]
    assert fb[0] == 1 and [p[2]["fb"][0] for p in pairs].count(1) == 1
    quarters = (W4 // 16) * (H4 // 16)
    print("report %d pictures late: %d of %d quarters forced" % (late, fb[3], quarters))
    assert (fb[3] == quarters) if late == H + 1 else (0 < fb[3] < quarters if late <= 2 else fb[3] > 0), "late %d: %d of %d quarters forced" % (late, fb[3], quarters)
    assert differs(got[t - 1], pairs[t - 1][1])
    for k in range(t, len(frames)):
        assert np.array_equal(got[k], pairs[k][1]), "report %d pictures late, picture %d: %d samples differ" % (late, k, int((got[k] != pairs[k][1]).sum()))


@pytest.mark.gpu
def test_two_reports_fold_into_one_heal_picture(gpu):
    frames = enckit.pan(W4, H4, 8, 4, 2)
    pairs = run(W4, H4, OPTS4, frames, {5: [(2, 10, 5), (3, 5, 10)]})
    got, log = hip_decode(pm.cut([p[0] for p in pairs], {2: (2,), 3: (1,)}))
    assert log == [(2, 10, 5), (3, 5, 10)]
    assert [p[2]["fb"][:2] for p in pairs] == [[int(t == 5), 2 * int(t == 5)] for t in range(8)]
    assert differs(got[4], pairs[4][1])
    for k in range(5, 8):
        assert np.array_equal(got[k], pairs[k][1]), "picture %d: %d samples differ" % (k, int((got[k] != pairs[k][1]).sum()))


@pytest.mark.gpu
def test_a_report_from_before_the_last_idr_picture_is_void(gpu):
    frames = enckit.pan(W4, H4, 8, 4, 2)
    opts = tuple(o for o in OPTS4 if o[0] != "period") + (("period", 4),)
    plain = run(W4, H4, opts, frames)
    void = run(W4, H4, opts, frames, {6: [(3, 0, -1)]}, expect=2)      # pictures 4 (the IDR picture) and 5 have been coded: POC 3 lies in front of them
    assert [(au, rec.tobytes()) for au, rec, _ in void] == [(au, rec.tobytes()) for au, rec, _ in plain]
    assert all(p[2]["fb"] == [0, 0, 0, 0] for p in void)


# ---- 5. on, and no report: the option-off encoder's stream byte for byte
ROWS5 = [(("preset", p), ("owf", owf)) for p in ("ultrafast", "veryfast") for owf in (0, 2, 6)] + [(("me-source", 1), ("subme", 2), ("intra-in-p", 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS5, ids=["-".join(str(v) for kv in r for v in kv) for r in ROWS5])
def test_without_a_report_no_byte_changes(gpu, row):
    w, h = 320, 192
    frames = enckit.frames(0, w, h, 8)
    owf = dict(row).get("owf", 0)
    opts = tuple(o for o in row if o[0] != "owf") + (("qp", 32),)
    off = run(w, h, opts, frames, owf=owf)
    on = run(w, h, opts + (("loss-feedback", H),), frames, owf=owf)
    for t, (a, b) in enumerate(zip(off, on)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), "picture %d differs with the option on" % t
    assert all(p[2]["fb"] == [0, 0, 0, 0] for p in on)


# ---- 6. the closed loop with a heal picture inside
CLOSED = [dict(opts=(("subme", 4), ("sao", "full"))), dict(opts=(("weightp", 1), ("subme", 2))), dict(opts=(("rc-algorithm", "lambda"),), bitrate=600000),
          dict(opts=(("vaq", 8),)), dict(opts=(("rdoq", 1), ("signhide", 1))), dict(opts=(("intra-in-p", 0), ("subme", 2))), dict(opts=(("intra-in-p", 2), ("sao", "full"))),
          dict(opts=(("me-source", 1), ("subme", 2), ("intra-in-p", 1))), dict(opts=(("me-source", 1), ("intra-in-p", 0))), dict(opts=(("subme", 2),), owf=0), dict(opts=(("subme", 2), ("sao", "full")), owf=2),
          dict(opts=(("subme", 2),), owf=6), dict(opts=(("scenecut", 2), ("subme", 2)), cut=True), dict(opts=(("subme", 2), ("sao", "full"), ("intra-in-p", 1)), threaded=True)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CLOSED, ids=[str(i) for i in range(len(CLOSED))])
def test_closed_loop_with_a_heal_picture_inside(gpu, cfg):
    w, h = 320, 192
    frames = enckit.pan(w, h, 9, 4, 2)
    if cfg.get("cut"):                                    # a scene cut at the picture behind the report: the IDR picture voids it
        import scenecut_model
        frames = list(scenecut_model.cut_clip(w, h, 9, 5))
    br = cfg.get("bitrate", 0)
    opts = (("qp", 32), ("me-range", 16), ("loss-feedback", H)) + tuple(cfg["opts"]) + ((("bitrate", br),) if br else ())
    pairs = run(w, h, opts, frames, {5: [(2, 3, 4)]}, owf=cfg.get("owf", 0), fields={"target_bitrate": br} if br else None)
    heals = [t for t, p in enumerate(pairs) if p[2]["fb"][0]]
    if cfg.get("cut"):
        assert any((n[0] >> 1) & 63 in (19, 20) for n in pyhevc.split_nals(pairs[5][0])), "the picture behind the report is no IDR picture: the row shows nothing"
        assert heals == [] and not any(starts_with_recovery_point(p[0]) for p in pairs)
    else:
        assert heals == [5] and pairs[5][2]["fb"][3] > 0 and starts_with_recovery_point(pairs[5][0])      # (the report is made when five pictures have been handed in, whatever is still in flight)
    enckit.closed_loop([(au, rec) for au, rec, _ in pairs], frame_threaded=bool(cfg.get("threaded")))


# ---- 7. what encoder_open and report_damage refuse
REFUSED = [(("lp-refs", 2),), (("gop", "lp-g4d3t1"), ("lp-gop", 1)), (("tmvp", 1),), (("me-coarse", 64),), (("tiles", "2x1"),), (("tiles", "1x2"), ("wpp", 0)),
           (("tiles", "1x2"), ("band-row0", 0), ("band-rows", 2)), (("band-row0", 0), ("band-rows", 2)), (("lossless", 1),), (("intra-chain", 0),), (("intra-refresh", 8),)]


@pytest.mark.gpu
@pytest.mark.parametrize("opts", REFUSED, ids=["-".join(str(v) for kv in o for v in kv) for o in REFUSED])
def test_encoder_open_refuses(gpu, capfd, opts):
    from kvazzup_amd.codec import Encoder
    with pytest.raises(RuntimeError):
        Encoder(256, 256, options=(("loss-feedback", H),) + opts)
    assert "loss-feedback" in capfd.readouterr().err


@pytest.mark.gpu
def test_report_damage_refuses(gpu):
    w, h = 320, 192
    frames = enckit.pan(w, h, 2, 4, 2)
    for on in (0, H):
        ge = enckit.encoder(w, h, (("qp", 32),) + ((("loss-feedback", on),) if on else ()))
        try:
            if on:
                assert ge.report_damage(0, 0, -1) == 2          # nothing has been coded
            for f in frames:
                ge.encode(f)
            if not on:
                assert ge.report_damage(1, 0, 1) == 0 and ge.report_damage(1, 0, -1) == 0
            else:
                n = (w // 64) * (h // 64)
                assert [ge.report_damage(1, a, c) for a, c in ((-1, 1), (n, 1), (n - 1, 2), (0, n + 1))] == [0, 0, 0, 0]
                assert ge.report_damage(-1, 0, 1) == 0 and ge.report_damage(2, 0, 1) == 2
                assert ge.report_damage(1, n - 1, 1) == 1 and ge.report_damage(0, 0, n) == 1
        finally:
            ge.close()
