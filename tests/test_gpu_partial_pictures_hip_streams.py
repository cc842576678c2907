"""GPU: partial pictures v1 on the HIP encoder's OWN slices=wpp streams (tests/test_gpu_partial_pictures.py takes the checker's encoder for its pan cases so that the
CPU tests can share them) -- the pan clip at 320x192, three CTU rows, lp-refs 1 and 3, row 1's segment of pictures 3 and 4 lost: row 0 stays, rows 1-2 are filled; the
decoder against tests/partial_model.py bit for bit in concealment modes 2 and 3, synchronous and with frame threads.  And the take-back of a picture whose last
segment ended early (Decoder::take_back_job closes the rows of its ColMotion again): frame threads, tmvp, WPP, free slices, against the checker."""
import functools

import numpy as np
import pytest

import deckit
import enckit
import partial_model as pm
from test_gpu_partial_pictures import compare


@functools.lru_cache(maxsize=None)
def hip_stream(refs, dx, dy):
    w, h = 320, 192
    ge = enckit.encoder(w, h, (("qp", 30), ("period", 64), ("slices", "wpp"), ("lp-refs", refs), ("subme", 2), ("me-range", 16)))
    try:
        aus = [au for au, _ in enckit.encode_all(ge, enckit.pan(w, h, 7, dx, dy))]
    finally:
        ge.close()
    assert all(len(pm.vcl_indices(au)) == 3 for au in aus)
    return w, h, pm.cut(aus, {3: (1,), 4: (1,)})


@functools.lru_cache(maxsize=None)
def model(refs, dx, dy, mode):
    return pm.decode([au for _, au in hip_stream(refs, dx, dy)[2]], deckit.tabs(), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("refs,dx,dy", [(1, 12, -6), (3, 10, -5)])
def test_the_encoders_own_row_segments(gpu, refs, dx, dy, mode, threads):
    from kvazzup_amd.codec import Decoder
    w, h, arrives = hip_stream(refs, dx, dy)
    pics, d = model(refs, dx, dy, mode)
    assert [x["runs"] for x in d.damage] == [[(5, 10)], [(5, 10)]]
    if mode == 3:
        assert (d.damage[0]["disp"] != 0).any() and d.damage[0]["leaves"], "no displacement, or no fetch that leaves the picture"
    gd = Decoder(threads=threads, frame_threads=True, concealment=mode, partial_pictures=True) if threads > 1 else Decoder(concealment=mode, partial_pictures=True)
    try:
        got = [f for t, au in arrives for f in gd.decode_au(au, t)] + gd.drain()
        if threads == 1 and mode == 3:
            assert np.array_equal(gd.fill_mv(w, h), d.damage[-1]["disp"])
        assert gd.damage_log() == [(x["poc"], 5, 10) for x in d.damage]
    finally:
        gd.close()
    compare(got, pics, "lp-refs %d, mode %d, %d threads" % (refs, mode, threads))


def take_backs(gd):
    import ctypes as C
    n = C.c_uint32(0)
    assert gd.lib.kvzx_decoder_debug_copy(gd.h, b"take_backs", C.byref(n), 4)
    return n.value


@pytest.mark.gpu
def test_pictures_taken_back_from_a_frame_worker_keep_their_rows_closed(gpu):
    """free slices with WPP and temporal prediction under frame threads: a picture whose segments cover it row by row is submitted, found to end early and taken back
    (asserted: the decoder counts them); the next picture's parser must wait for its SECOND parse row by row -- the pictures are the checker's"""
    import orc
    from kvazzup_amd.codec import Decoder
    taken = 0
    for ctb, seed in ((6, 68), (5, 60), (5, 88), (4, 61)):       # (the first three: streams in which the synchronous decoder takes a picture back too -- found on the CPU)
        g = orc.OracleGen(192, 128, seed=seed, slices=3, wpp=1, tmvp=1, ctb_log2=ctb, intra_period=16, gop=0, b_slices=0, tile_rows=1, tile_cols=1)
        aus = [g.picture() for _ in range(8)]
        g.close()
        od, gd = orc.OracleDecoder(), Decoder(threads=4, frame_threads=True)
        try:
            want = [f for t, au in enumerate(aus) for f in od.decode_au(au, t)] + od.flush()
            got = [f for t, au in enumerate(aus) for f in gd.decode_au(au, t)] + gd.drain()
            taken += take_backs(gd)
        finally:
            gd.close()
            od.close()
        assert len(got) == len(want) == 8, "seed %d: %d pictures, %d from the checker" % (seed, len(got), len(want))
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a["i420"], b["i420"]), "seed %d, picture %d" % (seed, k)
    print("pictures taken back:", taken)
    assert taken > 0, "no picture of these streams was taken back: the test guards nothing"
