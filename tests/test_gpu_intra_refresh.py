"""GPU: "uvgx intra refresh v1" (kvazaar.h intra-refresh) -- a band of intra units walks across the P pictures and heals what a lost
picture left behind, without an IDR picture.

The feature is held to: every picture's schedule equals tests/ir_model.py; every cell of the band is intra, every vector of a clean block keeps the bound, every
forced unit on the band's last unit column keeps to the modes that read no above-right samples; every reconstruction equals what the checker's decoder, the
library's HIP decoder and (the smallest case) tests/pyhevc.py make of the stream, over the tool set; and the point of it: with an access unit dropped, the
pictures of the first cycle that begins after the loss are the encoder's left of the band's end, every later picture entirely -- in both decoders -- while the
same clip and loss without the option still differ there.  The clip is the benchmark's synthetic clip, qp 32; each run has an IDR picture and 2 n + 3 P pictures."""
import functools

import numpy as np
import pytest

import enckit
from cases import INTRA_REFRESH_CLOSED as CLOSED
import ir_model as M
from ir_model import check_structure as _check_structure
import orc
import pyhevc

QP, RANGE = 32, 8
# (width, height, N): m = 2, n = 5; m = 1, n = 10; coded 256 wide, visible narrower, n = 8; m = 5, n = 4
SIZES = [(320, 192, 5), (320, 192, 10), (200, 120, 8), (640, 384, 4)]
IDS = ["%dx%d-N%d" % s for s in SIZES]


def _cw(w):
    return (w + 63) & ~63


def _opts(N):
    return (("qp", QP), ("me-range", RANGE), ("intra-refresh", N))


@functools.lru_cache(maxsize=None)
def _clip(w, h, n):
    return tuple(orc.synth_frame(0, 1234, w, h, t) for t in range(n))


def _npics(w, N):
    return 2 * M.cycle(_cw(w), N) + 4 if N else 0


@functools.lru_cache(maxsize=None)
def _stream(w, h, N, opts=(), npics=0):
    """(access unit, reconstruction) of the clip's pictures under intra-refresh=N (0: without the option), owf 0"""
    ge = enckit.encoder(w, h, _opts(N) + opts)
    out = enckit.encode_all(ge, _clip(w, h, npics or _npics(w, N)))
    ge.close()
    return out


# ---- 1. structure
# every size at intra-in-p 1; the first size at 0 (the band's units are the only intra units) and 2 (8x8 units) as well
STRUCT = [(s, 1) for s in SIZES] + [(SIZES[0], 0), (SIZES[0], 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("size,ip", STRUCT, ids=["%s-ip%d" % ("%dx%d-N%d" % s, ip) for s, ip in STRUCT])
def test_every_picture_has_the_structure_the_statement_asks_for(gpu, size, ip):
    w, h, N = size
    cw = _cw(w)
    ge = enckit.encoder(w, h, _opts(N) + (("intra-in-p", ip), ("subme", 2)))
    total = {}
    try:
        for t, fr in enumerate(_clip(w, h, _npics(w, N))):
            ge.encode(fr)
            for k, v in _check_structure(ge.debug_all(), t, cw, N, ip).items():
                total[k] = total.get(k, 0) + v
    finally:
        ge.close()
    assert total["band"] > 0 and total["clean"] > 0 and total["last"] > 0 and total["excluded_matter"] > 0, total


@pytest.mark.gpu
def test_the_bound_bites_on_a_pan(gpu):
    """content moving right to left: a block's match lies to its right in the reference picture.  Without the option clean blocks beside the band point into it;
    with the option none does, on the same pictures"""
    import pan_content
    w, h, N = 320, 192, 5
    n = M.cycle(w, N)
    frames = pan_content.clip(w, h, n + 2, 6, 0)
    counts = []
    for on in (0, N):
        from kvazzup_amd.codec import Encoder
        ge = Encoder(w, h, options=(("qp", QP), ("me-range", RANGE), ("subme", 2)) + ((("intra-refresh", on),) if on else ()))
        assert not ge.rejected
        beyond = 0
        try:
            for t, fr in enumerate(frames):
                ge.encode(fr)
                d = ge.debug_all()
                j, s, e, _ = M.record(w, N, t)
                if on:
                    _check_structure(d, t, w, N, 0)
                for x0 in range(0, s if j >= 1 else 0, 32):
                    inter = d["cu_intra"][:, x0 // 8:x0 // 8 + 4] == 0
                    beyond += int((inter & (4 * (x0 + 32) + d["cu_mv"][:, x0 // 8:x0 // 8 + 4, 0].astype(np.int64) > 4 * s)).sum())
        finally:
            ge.close()
        counts.append(beyond)
    assert counts[0] >= 1 and counts[1] == 0, counts


# ---- 2. closed loop over the tool set (the rows: tests/cases.py INTRA_REFRESH_CLOSED; tests/test_gpu_weightp_ir_oracle.py holds every one of them to the checker)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CLOSED, ids=[str(i) for i in range(len(CLOSED))])
def test_closed_loop_decodes_to_the_reconstruction(gpu, cfg):
    w, h, N = cfg.get("size", SIZES[0])
    owf, br = cfg.get("owf", 0), cfg.get("bitrate", 0)
    opts = (("owf", owf),) + tuple(cfg.get("opts", ())) + ((("bitrate", br),) if br else ())
    frames = list(_clip(w, h, _npics(w, N)))
    if cfg.get("change"):
        import wp_model
        frames = wp_model.change(frames, w, h, cfg["change"])
    ge = enckit.encoder(w, h, _opts(N) + opts, fields={"target_bitrate": br} if br else None)
    pairs, irs = [], []
    try:
        for t in range(len(frames) + owf + 1):
            au, rec = ge.encode(frames[t] if t < len(frames) else None)
            if au:
                pairs.append((au, rec))
                irs.append([int(v) for v in ge.debug("ir", np.int32, (4,))])
    finally:
        ge.close()
    assert len(pairs) == len(frames)
    period = dict(opts).get("period", 64)
    assert irs == [M.record(_cw(w), N, t % period) for t in range(len(frames))]      # (period 4: the cycle restarts behind every IDR picture)
    # only a cycle's first picture carries the SEI
    for t, (au, _) in enumerate(pairs):
        sei = [n for n in pyhevc.split_nals(au) if (n[0] >> 1) & 63 == 39]
        assert len(sei) == (1 if irs[t][0] == 0 else 0), t
        if sei:
            assert bytes(pyhevc.unescape(sei[0])[2:]) == M.recovery_point_sei(irs[t][3] - 1)
    enckit.closed_loop(pairs)


@pytest.mark.gpu
def test_closed_loop_smallest_case_also_matches_pyhevc(gpu):
    w, h, N = 128, 64, 2                                        # B = 4, m = 2, n = 2
    for extra in ((("subme", 2),), (("intra-in-p", 2), ("sao", "full"))):
        pairs = _stream(w, h, N, extra)
        assert len(pairs) == 2 * M.cycle(w, N) + 4
        enckit.closed_loop(pairs, pyhevc_too=True)


# ---- 3. recovery
def _decode_with_a_loss(aus, lost, which):
    """{time stamp: i420} of the stream without access unit `lost`, from the checker's decoder or the HIP decoder"""
    if which == "checker":
        dec = orc.OracleDecoder()
    else:
        from kvazzup_amd.codec import Decoder
        dec = Decoder()
    got = []
    try:
        for t, au in enumerate(aus):
            if t != lost:
                got += dec.decode_au(au, t)
        got += dec.flush() if which == "checker" else dec.drain()
        if which == "checker":
            assert dec.concealed() > 0
    finally:
        dec.close()
    return {f["pts"]: f["i420"] for f in got}


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["before-a-cycle", "mid-cycle"])
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_a_lost_picture_is_healed_by_the_next_cycle(gpu, size, where):
    """One access unit dropped; the tool set of a call above `ultrafast` (fractional vectors, SAO, free intra units).  Left of e_j - 4 every picture of the next cycle
    is the encoder's: deblocking the band's end against the dirty side reaches three columns and, through the horizontal edges' decisions, a fourth; SAO would add a
    fifth (this test found column e_j - 5 differing in one or two samples a picture), which is why k_sao<false, true> leaves luma SAO off in the coding tree blocks at
    the band's end"""
    w, h, N = size
    cw, n = _cw(w), M.cycle(_cw(w), N)
    opts = (("subme", 2), ("sao", "full"), ("intra-in-p", 1))
    pairs = _stream(w, h, N, opts)
    lost = n if where == "before-a-cycle" else 1 + n // 2       # the first cycle's last picture / a picture in its middle; the second cycle is poc n + 1 .. 2 n
    assert M.record(cw, N, lost)[0] == (n - 1 if where == "before-a-cycle" else n // 2)
    for which in ("checker", "hip"):
        got = _decode_with_a_loss([au for au, _ in pairs], lost, which)
        assert sorted(got) == [t for t in range(len(pairs)) if t != lost]
        assert not np.array_equal(got[lost + 1], pairs[lost + 1][1])          # (the loss does damage: the test is about something)
        for t in range(n + 1, len(pairs)):
            j, s, e, _ = M.record(cw, N, t)
            whole = t > 2 * n or e == cw
            lim = w if whole else min(w, e - 4)
            for c, (a, b) in enumerate(zip(enckit.planes(got[t], w, h), enckit.planes(pairs[t][1], w, h))):
                k = lim if c == 0 else lim // 2
                assert np.array_equal(a[:, :k], b[:, :k]), "%s decoder, picture %d (position %d, band [%d, %d)), plane %d: %d samples differ left of column %d, first column %d" % (
                    which, t, j, s, e, c, int((a[:, :k] != b[:, :k]).sum()), k, int(np.flatnonzero((a[:, :k] != b[:, :k]).any(axis=0))[0]))
    # the control: the same clip and loss without the option still differs where the refreshed stream is whole
    plain = _stream(w, h, 0, opts, len(pairs))
    got = _decode_with_a_loss([au for au, _ in plain], lost, "checker")
    assert not np.array_equal(got[2 * n][:w * h], plain[2 * n][1][:w * h])
    assert not np.array_equal(got[len(pairs) - 1][:w * h], plain[-1][1][:w * h])


# ---- 4. what encoder_open refuses
REFUSED = [(("lp-refs", 2),), (("lp-refs", 4),), (("gop", "lp-g4d3t1"), ("lp-gop", 1)), (("tmvp", 1),), (("me-coarse", 64),), (("tiles", "2x1"),), (("tiles", "1x2"), ("wpp", 0)),
           (("tiles", "1x2"), ("band-row0", 0), ("band-rows", 2)), (("lossless", 1),), (("intra-chain", 0),)]


@pytest.mark.gpu
@pytest.mark.parametrize("opts", REFUSED, ids=["-".join(str(v) for kv in o for v in kv) for o in REFUSED])
def test_encoder_open_refuses(gpu, capfd, opts):
    from kvazzup_amd.codec import Encoder
    with pytest.raises(RuntimeError):
        Encoder(256, 256, options=(("intra-refresh", 8),) + opts)
    assert "intra-refresh" in capfd.readouterr().err
