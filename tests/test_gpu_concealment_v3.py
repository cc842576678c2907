"""GPU side of tests/test_concealment_v3.py: the HIP decoder in concealment mode 3 (kvzx_decoder_set_concealment; csrc/decoder.h, csrc/conceal_kernels.hip) against the
model decoder of tests/conceal_model.py -- every picture it hands out bit for bit, the wrong ones behind a loss included, and the stand-ins themselves with their
displacement tables (kvzx_decoder_debug_copy "standin" / "standin_mv").  The checker stays at v2: a decoder that is not asked for mode 3 still equals it.

Not here: a first loss without a source (a grey stand-in).  The reference pictures a picture finds always include the last IRAP picture, which is never lost in
these streams and cannot be (nothing decodes without it), so no stream of the kits gets there; mode 3 fills a grey stand-in with v2's own memset."""
import functools

import numpy as np
import pytest

import conceal_model as cm
import deckit
import enckit
import orc
from nalkit import lossy

THREADS = [1, 3, 8]


def pan_stream(refs, dx, dy, lose):
    """the checker's encoder on a 192x128 pan with lp-refs, access units `lose` lost: [(time stamp, access unit)]"""
    w, h = 192, 128
    e = enckit.oracle_encoder(w, h, n=refs, qp=30, subme=2)
    aus = [e.encode(f) for f in enckit.pan(w, h, 9, dx, dy)]
    e.close()
    return w, h, [(t, a) for t, a in enumerate(aus) if t not in lose]


@functools.lru_cache(maxsize=None)
def case(kind, *args):
    """(w, h, the access units that arrive, the model decoder's pictures, the model decoder): made once, shared by the thread counts"""
    if kind == "pan":
        w, h, cut = pan_stream(*args)
    else:
        w, h, seed, n = args
        cut = lossy(seed, n=n, w=w, h=h)[0]
    pics, d = cm.decode([au for _, au in cut], deckit.tabs())
    assert d.stand_ins, "nothing was concealed"
    return w, h, cut, pics, d


def hold_to_the_model(w, h, cut, pics, model, threads):
    from kvazzup_amd.codec import Decoder
    gd = Decoder(threads=threads, frame_threads=True, concealment=3) if threads > 1 else Decoder(concealment=3)
    got = []
    try:
        for k, (t, au) in enumerate(cut):
            got += gd.decode_au(au, t)
            mine = [s for s in model.stand_ins if s["au"] == k]
            if threads == 1 and mine:                               # (one picture at a time: the stand-in filled last is this access unit's last)
                planes, mv = gd.standin(w, h)
                assert np.array_equal(mv, mine[-1]["disp"]), "access unit %d: the displacement table differs at %d entries" % (k, int((mv != mine[-1]["disp"]).sum()))
                for c in range(3):
                    assert np.array_equal(planes[c], mine[-1]["planes"][c]), "access unit %d: plane %d of the stand-in differs at %d samples" % (k, c, int((planes[c] != mine[-1]["planes"][c]).sum()))
        got += gd.drain()
    finally:
        gd.close()
    assert len(got) == len(cut) == len(pics), "%d access units arrived: %d pictures from the HIP decoder, %d from the model" % (len(cut), len(got), len(pics))
    for k, (a, b) in enumerate(zip(got, pics)):
        assert (a["width"], a["height"]) == (b["width"], b["height"])
        if not np.array_equal(a["i420"], b["i420"]):
            d = np.flatnonzero(a["i420"] != b["i420"])
            pytest.fail("picture %d in output order: %d samples differ, first at %d" % (k, len(d), d[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("refs,dx,dy,lose", [(1, 12, -6, (3,)), (3, 12, -6, (3,)), (1, -9, 5, (3,)), (3, -9, 5, (3,)), (3, -9, 5, (3, 4)), (1, 3, 1, (3, 4, 6))])
def test_a_pan_with_pictures_lost(gpu, refs, dx, dy, lose, threads):
    """vectors that leave the picture on every side; with lp-refs 3 blocks that point further back than one picture (td != tb); two losses in a row (tb = 2)"""
    w, h, cut, pics, d = case("pan", refs, dx, dy, lose)
    assert any((s["disp"] != 0).any() for s in d.stand_ins), "no stand-in moved"
    hold_to_the_model(w, h, cut, pics, d, threads)


# seeds of nalkit.lossy by what they bring (found with the model decoder): 1, 5, 7 B pictures, a stand-in earlier in output order than its source (tb < 0) and
# blocks predicted from list 1 only; 6, 10 long-term reference pictures; 8 one reference picture, 7 and 11 four; 11 a stand-in made from a stand-in
@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("w,h,seed,n", [(64, 64, 1, 26), (64, 64, 5, 26), (64, 64, 6, 26), (64, 64, 7, 26), (64, 64, 8, 26), (64, 64, 10, 26), (64, 64, 11, 26),
                                        (72, 56, 4, 20), (72, 56, 5, 20), (72, 56, 6, 20), (416, 240, 3, 12), (416, 240, 4, 12)])
def test_streams_of_the_synthesiser_with_pictures_lost(gpu, w, h, seed, n, threads):
    """72x56: the last block column and row are partial (8 samples)"""
    hold_to_the_model(*case("lossy", w, h, seed, n), threads)


def test_the_seeds_bring_what_they_are_there_for():
    """CPU: the properties the seeds above were chosen for"""
    st = {seed: case("lossy", 64, 64, seed, 26)[4].stand_ins for seed in (1, 5, 6, 11)}
    assert any(s["poc"] < s["src_poc"] for s in st[1] + st[5])            # tb < 0
    assert any(s["list1_blocks"] for s in st[1] + st[5])                  # blocks that only list 1 predicts
    assert all((s["disp"] != 0).any() for s in st[6])                     # every stand-in of the long-term stream moved
    assert any(s["src_is_stand_in"] for s in st[11])                      # a stand-in as the source of the next
    assert any((s["disp"] != 0).any() for s in case("lossy", 72, 56, 4, 20)[4].stand_ins)


@pytest.mark.gpu
def test_the_setter(gpu):
    from kvazzup_amd.codec import Decoder
    cut = case("lossy", 64, 64, 8, 26)[2]
    d = Decoder()
    try:
        assert not d.set_concealment(4) and not d.set_concealment(0) and not d.set_concealment(1)
        assert d.set_concealment(3) and d.set_concealment(2) and d.set_concealment(3)
        assert not gpu.kvzx_decoder_set_band(d.h, 0, 1)                   # no band form of mode 3 ...
        assert d.set_concealment(2) and gpu.kvzx_decoder_set_band(d.h, 0, 1) and not d.set_concealment(3)      # ... either way round
        assert gpu.kvzx_decoder_set_band(d.h, 0, 0) and d.set_concealment(3)
        d.decode_au(cut[0][1], 0)
        assert not d.set_concealment(2) and not d.set_concealment(3)      # after the first picture
    finally:
        d.close()
    with pytest.raises(ValueError):
        Decoder(concealment=4)


@pytest.mark.gpu
def test_without_the_keyword_the_decoder_still_equals_the_checker(gpu):
    deckit.run(lossy(6, n=26)[0], 1)
    deckit.run(lossy(5, n=26)[0], 3)


@pytest.mark.gpu
def test_through_the_filter_chain(gpu):
    """KvazaarFilter' -> a wire that loses every fourth access unit -> OpenHEVCFilter' with uvgx/concealment = 3: the pictures are the model decoder's"""
    from kvazzup_amd.pipeline import Pipeline
    w, h, frames, period, every = 192, 128, 24, 16, 4
    pl = Pipeline(w, h, settings={"video/QP": 30, "video/Intra": period, "uvgx/wireLossEvery": every, "uvgx/concealment": 3}, custom=(("me-range", 16),))
    try:
        for f in enckit.pan(w, h, frames, 3, 1):
            assert pl.push_host_paced(np.ascontiguousarray(f), max_backlog=4)
        lost = (frames - len(range(0, frames, period))) // every
        assert lost >= 4 and pl.wait(frames - lost, 60000)
        seen, arrived = 0, []
        for t in range(frames):                                     # (the harness's rule, applied to the access units as they left the encoder)
            au, pts = pl.pop_encoded()
            assert pts == t
            if t % period != 0:
                seen += 1
                if seen % every == 0:
                    continue
            arrived.append((t, au))
        pics, d = cm.decode([au for _, au in arrived], deckit.tabs())
        assert len(pics) == len(arrived) == frames - lost and any((s["disp"] != 0).any() for s in d.stand_ins)
        for (t, _), want in zip(arrived, pics):
            got = pl.pop_decoded()
            assert got["pts"] == t and np.array_equal(got["i420"], want["i420"]), "picture %d" % t
    finally:
        pl.close()
