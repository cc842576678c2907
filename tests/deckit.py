"""Decoders side by side: a stream through the checker's decoder (oracle/), the Python decoder (tests/pyhevc.py) and the HIP decoder, the pictures compared bit
for bit.  What the decoder tests and the soak scripts under tools/ share.  Test infrastructure; every assert says what it saw (pytest rewrites asserts in test
modules only)."""
import numpy as np
import pytest

import orc
import pyhevc
from orc import table


def tabs():
    """the normative tables pyhevc.Decoder takes, read from the checker"""
    return {"range_lps": table(1, np.uint8, (64, 4)), "trans_lps": table(2, np.uint8, (64,)), "trans_mps": table(13, np.uint8, (64,)),
            "dct": table(0, np.int8, (32, 32)).astype(int), "dst": table(5, np.int8, (4, 4)).astype(int),
            "luma_filter": table(11, np.int8, (4, 8)).astype(int), "chroma_filter": table(12, np.int8, (8, 4)).astype(int),
            "beta": table(6, np.uint8, (52,)).astype(int), "tc": table(7, np.uint8, (54,)).astype(int),
            "intra_angle": table(9, np.int8, (35,)).astype(int), "inv_angle": table(10, np.int16, (35,)).astype(int)}


def python_pictures(aus):
    """the pictures tests/pyhevc.py makes of the access units, in output order"""
    d = pyhevc.Decoder(tabs())
    for au in aus:
        for nal in pyhevc.split_nals(au):
            d.decode_nal(nal)
    return d.flush()


PLAIN = dict(num_refs=1, tmvp=0, amp=0, sao=0, strong_intra=1, sign_hiding=0, transform_skip=0, cabac_init=0, wpp=1, tile_rows=1, uniform_tiles=1,
             th_depth_inter=0, th_depth_intra=0, qp_delta=0, chroma_qp_offsets=0, deblock_mode=0, par_mrg_level=2, intra_in_p=0, all_part_modes=0,
             chroma_modes=0, nxn_intra=0, max_cu_log2=5, min_cu_log2=3, big_mvd=0)


def run_stream(w, h, pictures, threads=1, frame_threads=False, **cfg):
    """`pictures` access units of the synthesiser (options cfg) through the checker and the HIP decoder: every picture bit for bit"""
    from kvazzup_amd.codec import Decoder
    g = orc.OracleGen(w, h, **cfg)
    od = orc.OracleDecoder()
    gd = Decoder(threads=threads, frame_threads=frame_threads) if frame_threads else Decoder()
    refs, got, pocs = [], [], []
    try:
        reorder = g.config.get("gop", 0) > 1              # (pictures come out in POC order, later than they go in)
        for t in range(pictures):
            au = g.picture()
            r = od.decode_au(au, t)
            assert reorder or len(r) == 1, "access unit %d: the checker handed out %d pictures; config %r" % (t, len(r), g.config)
            refs += [f["i420"] for f in r]
            pocs += [f["poc"] for f in r]
            got += gd.decode_au(au, t)
        refs += [f["i420"] for f in od.flush()]
        if frame_threads or reorder or g.config.get("slices") == 3:      # (free slices: a picture is closed by what follows it in the stream)
            got += gd.drain()
        assert len(got) == pictures and len(refs) == pictures, "%d pictures in: %d from the HIP decoder, %d from the checker; config %r" % (pictures, len(got), len(refs), g.config)
        for t in range(pictures):
            assert got[t]["width"] == w and got[t]["height"] == h, "picture %d: the HIP decoder says %dx%d, the stream is %dx%d" % (t, got[t]["width"], got[t]["height"], w, h)
            if not np.array_equal(got[t]["i420"], refs[t]):
                d = np.flatnonzero(got[t]["i420"] != refs[t])
                plane = "Y" if d[0] < w * h else "C"
                pytest.fail("picture %d: %d samples differ, first at %d (%s, x=%d y=%d); config %r"
                            % (t, len(d), d[0], plane, d[0] % w, d[0] // w, g.config))
    finally:
        gd.close()
        od.close()
        g.close()


def both(cut, pts, threads=1, frame_threads=False):
    """the access units `cut` (time stamps `pts`) through the checker and the product: the pictures must agree, in order"""
    from kvazzup_amd.codec import Decoder
    od = orc.OracleDecoder()
    gd = Decoder(threads=threads, frame_threads=frame_threads) if frame_threads else Decoder()
    want, got = [], []
    try:
        for p, au in zip(pts, cut):
            want += od.decode_au(au, p)
            got += gd.decode_au(au, p)
        want += od.flush()
        got += gd.drain()
        assert [f["pts"] for f in got] == [f["pts"] for f in want], "time stamps: the HIP decoder %r, the checker %r" % ([f["pts"] for f in got], [f["pts"] for f in want])
        for a, b in zip(got, want):
            assert (a["width"], a["height"]) == (b["width"], b["height"]), "time stamp %d: the HIP decoder says %dx%d, the checker %dx%d" % (a["pts"], a["width"], a["height"], b["width"], b["height"])
            if not np.array_equal(a["i420"], b["i420"]):
                d = np.flatnonzero(a["i420"] != b["i420"])
                pytest.fail("picture with time stamp %d: %d samples differ, first at %d" % (a["pts"], len(d), d[0]))
    finally:
        gd.close()
        od.close()
    return [f["pts"] for f in want]


def run(cut, threads, must_conceal=True):
    """a stream with access units lost, [(time stamp, access unit)], through the checker and the HIP decoder: the same pictures, the wrong ones too"""
    from kvazzup_amd.codec import Decoder
    od = orc.OracleDecoder()
    gd = Decoder(threads=threads, frame_threads=True) if threads > 1 else Decoder()
    want, got = [], []
    try:
        for t, au in cut:
            want += od.decode_au(au, t)
            got += gd.decode_au(au, t)
        want += od.flush()
        got += gd.drain()
        assert od.concealed() > 0 or not must_conceal, "the checker concealed nothing: no reference picture was lost"
    finally:
        gd.close()
        od.close()
    assert [f["pts"] for f in got] == [f["pts"] for f in want], "time stamps: the HIP decoder %r, the checker %r" % ([f["pts"] for f in got], [f["pts"] for f in want])
    assert len(got) == len(cut) or not must_conceal, "%d access units arrived, %d pictures came out" % (len(cut), len(got))
    for a, b in zip(got, want):
        if not np.array_equal(a["i420"], b["i420"]):
            d = np.flatnonzero(a["i420"] != b["i420"])
            pytest.fail("picture with time stamp %d: %d samples differ, first at %d" % (a["pts"], len(d), d[0]))
