"""GPU side of tests/test_partial_pictures.py: the HIP decoder with partial pictures on (kvzx_decoder_set_partial_pictures; csrc/decoder.h "Partial pictures v1",
csrc/conceal_kernels.hip k_dec_fill_ctbs) against the model of tests/partial_model.py -- every picture it hands out bit for bit, in concealment modes 2 and 3,
synchronous and with frame threads; the damage it reports; the table of displacements; two decoders at once, where the submission layer launches the pictures.
What v1 builds is Kvazaar's row form (WPP, a dependent slice segment per CTB row) and any cut of a one-tile picture WITHOUT WPP into slices (free slices); the streams and their losses are tests/partial_cases.py's, and the CPU test
asserts what each of them brings.  With the option on and nothing lost the decoder still equals the checker."""
import functools

import numpy as np
import pytest

import deckit
import partial_cases as pc

THREADS = [1, 3, 8]
MODES = [2, 3]


def compare(got, pics, what):
    assert len(got) == len(pics), "%s: %d pictures from the HIP decoder, %d from the model" % (what, len(got), len(pics))
    for k, (a, b) in enumerate(zip(got, pics)):
        assert (a["width"], a["height"]) == (b["width"], b["height"])
        if not np.array_equal(a["i420"], b["i420"]):
            d = np.flatnonzero(a["i420"] != b["i420"])
            w, h = b["width"], b["height"]
            pytest.fail("%s, picture %d in output order (POC %d): %d samples differ, first at %d (%s)"
                        % (what, k, b["poc"], len(d), d[0], "Y x=%d y=%d" % (d[0] % w, d[0] // w) if d[0] < w * h else "chroma"))


def hold_to_the_model(name, mode, threads):
    from kvazzup_amd.codec import Decoder
    w, h, _, arrives = pc.stream(name)
    pics, model = pc.model(name, mode)
    assert any(0 < d["missing"] < d["total"] for d in model.damage), "no picture of %s is damaged" % name
    gd = Decoder(threads=threads, frame_threads=True, concealment=mode, partial_pictures=True) if threads > 1 else Decoder(concealment=mode, partial_pictures=True)
    got, tables = [], []
    try:
        for k, (t, au) in enumerate(arrives):
            n = len(gd.damage_log())
            got += gd.decode_au(au, t)
            if threads == 1 and mode == 3 and len(gd.damage_log()) > n:        # (one picture at a time: a damaged picture closed by this access unit has been filled)
                tables.append(gd.fill_mv(w, h).copy())
        got += gd.drain()
        log = gd.damage_log()
    finally:
        gd.close()
    compare(got, pics, "%s, mode %d, %d threads" % (name, mode, threads))
    # the damage: the log in decoding order, and what every picture handed out says of itself
    assert log == [(d["poc"], a, n) for d in model.damage for a, n in d["runs"]]
    by = {(d["cvs"], d["poc"]): d for d in model.damage}
    for a, b in zip(got, pics):
        d = by.get((b["cvs"], b["poc"]))
        assert (a["missing_ctbs"], a["total_ctbs"]) == ((d["missing"], d["total"]) if d else (0, a["total_ctbs"])) and a["total_ctbs"] > 0, "POC %d: %r" % (b["poc"], a.get("missing_ctbs"))
    return tables, model


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", pc.NAMES)
def test_rows_lost_on_the_way(gpu, name, mode, threads):
    tables, model = hold_to_the_model(name, mode, threads)
    if threads == 1 and mode == 3:
        # (a damaged picture that closes when the stream ends is filled inside drain(): its table is not among these)
        want = [d["disp"] for d in model.damage]
        assert tables and len(tables) <= len(want)
        for k, t in enumerate(tables):
            assert np.array_equal(t, want[k]), "damaged picture %d: the displacement table differs at %d entries" % (k, int((t != want[k]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(pc.FREE))
def test_free_slices_without_wpp_with_segments_lost(gpu, name, mode, threads):
    """gaps anywhere in a one-tile picture: a first segment lost with an independent one behind it, a middle independent one, a dependent one that drags its
    successors along, the last one, two gaps in one picture (what each stream brings: tests/test_partial_pictures.py); missing blocks in the middle of a row, received
    blocks behind missing ones"""
    hold_to_the_model(name, mode, threads)


@pytest.mark.parametrize("name", list(pc.ENCODED))
def test_under_a_pan_the_fill_moves_and_some_fetch_leaves_the_picture(name):
    """CPU, what the two cases are there for: mode 3 on the encoder's own slices=wpp streams: row 0 stays, rows 1-2 come from the picture before along its motion"""
    _, model = pc.model(name, 3)
    first = model.damage[0]
    assert first["runs"] == [(5, 10)] and (first["disp"] != 0).any() and first["leaves"]


@pytest.mark.gpu
def test_two_decoders_at_once(gpu, monkeypatch):
    """two different damaged streams side by side: the submission layer launches their pictures (the fill comes before them), each equals its model.  Low-delay
    streams: the pictures come out in the order they went in, so the model's pictures take the time stamps of what arrived"""
    import kvazzup_amd.codec as codec
    monkeypatch.setattr(codec, "Decoder", functools.partial(codec.Decoder, partial_pictures=True))
    streams = []
    for name, mode, threads in (("72x56_ctb16_sao_tmvp", 3, 3), ("64x64_ctb16_irap", 2, 1)):
        arrives, pics = pc.stream(name)[3], pc.model(name, mode)[0]
        assert len(arrives) == len(pics)
        streams.append({"aus": arrives, "want": [dict(p, pts=t) for p, (t, _) in zip(pics, arrives)], "threads": threads, "concealment": mode})
    st = deckit.together(streams)
    assert st["pictures"] > 0, "the submission layer launched nothing: %r" % (st,)


@pytest.mark.gpu
def test_option_on_and_nothing_lost_equals_the_checker(gpu, monkeypatch):
    import kvazzup_amd.codec as codec
    monkeypatch.setattr(codec, "Decoder", functools.partial(codec.Decoder, partial_pictures=True))
    deckit.run_stream(72, 56, 6, seed=3, slices=1, wpp=1, ctb_log2=4, sao=1, tmvp=1)
    deckit.run_stream(192, 128, 5, seed=61, slices=3, wpp=1)
    deckit.run_stream(64, 64, 8, threads=3, frame_threads=True, seed=7, slices=1, wpp=1, ctb_log2=4, gop=4, b_slices=50)


@pytest.mark.gpu
def test_the_setter_and_an_intact_picture(gpu):
    from kvazzup_amd.codec import Decoder
    aus = pc.stream("64x64_ctb16_irap")[2]
    d = Decoder()
    try:
        assert gpu.kvzx_decoder_set_partial_pictures(d.h, 1) and gpu.kvzx_decoder_set_partial_pictures(d.h, 0) and gpu.kvzx_decoder_set_partial_pictures(d.h, 1)
        assert not gpu.kvzx_decoder_set_band(d.h, 0, 1)                   # no band form ...
        assert gpu.kvzx_decoder_set_partial_pictures(d.h, 0) and gpu.kvzx_decoder_set_band(d.h, 0, 1) and not gpu.kvzx_decoder_set_partial_pictures(d.h, 1)      # ... either way round
        assert gpu.kvzx_decoder_set_band(d.h, 0, 0) and gpu.kvzx_decoder_set_partial_pictures(d.h, 1)
        d.partial_pictures = True
        out = d.decode_au(aus[0], 0)
        assert len(out) == 1 and out[0]["missing_ctbs"] == 0 and out[0]["total_ctbs"] == 16
        assert not gpu.kvzx_decoder_set_partial_pictures(d.h, 0) and not gpu.kvzx_decoder_set_partial_pictures(d.h, 1)      # after the first picture
        assert d.damage_log() == []
    finally:
        d.close()
    with pytest.raises(ValueError):
        Decoder(partial_pictures=True, concealment=4)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_through_the_filter_chain(gpu, mode):
    """KvazaarFilter' with video/Slices = 1 and WPP -> a wire that loses every fourth slice segment (uvgx/wireLossSegmentEvery; never one of an IRAP picture) ->
    OpenHEVCFilter' with uvgx/partialPictures = 1: the pictures are the model's.  320x192 is three CTU rows, a segment each: in turn a first segment goes (the picture
    is lost whole, its other segments are rejected), a middle one (rows 1-2 are filled), a last one (row 2 is filled)"""
    import enckit
    import orc
    import partial_model as pm
    from kvazzup_amd.pipeline import Pipeline
    w, h, frames, period, every = 320, 192, 14, 16, 4
    pl = Pipeline(w, h, settings={"video/QP": 30, "video/Intra": period, "video/Slices": 1, "video/WPP": 1, "uvgx/wireLossSegmentEvery": every, "uvgx/partialPictures": 1,
                                  "uvgx/concealment": mode}, custom=(("me-range", 16),))
    try:
        for f in enckit.pan(w, h, frames, 3, 1):
            assert pl.push_host_paced(np.ascontiguousarray(f), max_backlog=4)
        assert pl.wait(frames - 3, 60000)                           # (pictures 2, 6 and 10 lose their first segment and never come out)
        seen, arrived = 0, []
        for t in range(frames):                                     # (the harness's rule, applied to the access units as they left the encoder)
            au, pts = pl.pop_encoded()
            assert pts == t
            nals = orc.split_nals(au)
            irap = any(16 <= ((n[4] >> 1) & 63) <= 23 for n in nals)
            keep = []
            for n in nals:
                if ((n[4] >> 1) & 63) < 32 and not irap:
                    seen += 1
                    if seen % every == 0:
                        continue
                keep.append(n)
            arrived.append((t, b"".join(keep), ((keep[-1][4] >> 1) & 63) < 32 and any(((n[4] >> 1) & 63) < 32 and (n[6] & 0x80) for n in keep)))
        pics, d = pm.decode([au for _, au, _ in arrived], deckit.tabs(), mode)
        stamps = [t for t, _, first in arrived if first]            # (a picture whose first segment arrived comes out)
        assert len(pics) == len(stamps) == frames - 3 and d.rejected and len(d.damage) >= 4 and any(x["missing"] == 10 for x in d.damage) and any(x["missing"] == 5 for x in d.damage)
        for t, want in zip(stamps, pics):
            got = pl.pop_decoded()
            # (no word on time stamps: the filter, like the one it restates, pairs pictures with the NAL units that went in, one by one, and a picture is three of them here)
            assert got is not None and np.array_equal(got["i420"], want["i420"]), "picture %d" % t
    finally:
        pl.close()
