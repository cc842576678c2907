"""Decoders side by side: a stream through the checker's decoder (oracle/), the Python decoder (tests/pyhevc.py) and the HIP decoder, the pictures compared bit
for bit.  What the decoder tests and the soak scripts under tools/ share.  Test infrastructure; every assert says what it saw (pytest rewrites asserts in test
modules only)."""
import ctypes as C
import threading
import time

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


def batch_stats(lib, reset=False):
    """the submission layer's counters on device 0 (kvzx_batch_stats): batches launched, the pictures in them, batches by size, and per batched kernel the profiled
    time, launches and pictures"""
    lib.kvzx_batch_stats.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
    b, p = C.c_uint64(), C.c_uint64()
    sizes, ms, ln, fr = (C.c_uint64 * 9)(), (C.c_double * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
    k = lib.kvzx_batch_stats(0, C.byref(b), C.byref(p), sizes, ms, ln, fr, int(reset))
    return {"batches": b.value, "pictures": p.value, "sizes": list(sizes), "ms": list(ms)[:k], "launches": list(ln)[:k], "frames": list(fr)[:k]}


def together(streams, hold=False):
    """Several decoders open at once on the device, each on a Python thread of its own (the filter threads of a call): what the submission layer (csrc/batch.h)
    launches together must be, decoder by decoder, that decoder's expected pictures bit for bit.  A stream is a dict: `aus` [(pts, access unit)]; `want` its
    pictures in output order, made on the CPU beforehand; `threads` (1: synchronous, more: frame threads); `concealment` None or 3; `start_after` None or (index
    of another stream, k) -- the decoder is opened once that one has handed in k access units: a peer joins; `close_early` -- it closes as soon as its stream has
    ended: a peer leaves.  hold: the layer is held while the threads queue what they can, then released, so that full batches leave.  Every other decoder
    stays open until the layer's statistics have been read (a decoder left alone launches for itself); they are returned."""
    from kvazzup_amd.codec import Decoder
    n = len(streams)
    decs, out, err, handed = [None] * n, [None] * n, [None] * n, [0] * n
    step = threading.Condition()

    def open_decoder(k):
        s = streams[k]
        threads = s.get("threads", 1)
        kw = {"concealment": s["concealment"]} if s.get("concealment") else {}
        decs[k] = Decoder(threads=threads, frame_threads=True, **kw) if threads > 1 else Decoder(**kw)

    def work(k):
        s = streams[k]
        try:
            if s.get("start_after"):
                other, count = s["start_after"]
                with step:
                    step.wait_for(lambda: handed[other] >= count)
                open_decoder(k)
            got = []
            for pts, au in s["aus"]:
                got += decs[k].decode_au(au, pts)
                with step:
                    handed[k] += 1
                    step.notify_all()
            got += decs[k].drain()
            out[k] = got
            if s.get("close_early"):
                decs[k].close()
        except Exception as e:          # noqa: BLE001 -- re-raised by the asserting thread
            err[k] = e
        finally:
            with step:
                handed[k] = float("inf")          # (whoever waits for this decoder goes on, whatever became of it)
                step.notify_all()

    try:
        for k in range(n):
            if not streams[k].get("start_after"):
                open_decoder(k)
        lib = next(d for d in decs if d is not None).lib
        lib.kvzx_batch_hold.argtypes = [C.c_int, C.c_int]
        batch_stats(lib, reset=True)
        ths = [threading.Thread(target=work, args=(k,)) for k in range(n)]
        if hold:
            lib.kvzx_batch_hold(0, 1)
        try:
            for t in ths:
                t.start()
            if hold:
                time.sleep(1.0)                   # every decoder has queued what its ring lets it queue and waits for its first picture
        finally:
            lib.kvzx_batch_hold(0, 0)
            for t in ths:
                t.join()
        st = batch_stats(lib)
    finally:
        for d in decs:
            if d is not None:
                d.close()
    for e in err:
        if e is not None:
            raise e
    for k, s in enumerate(streams):
        got, want = out[k], s["want"]
        assert len(got) == len(want), "decoder %d: %d access units in, %d pictures out, %d expected" % (k, len(s["aus"]), len(got), len(want))
        assert [f["pts"] for f in got] == [f["pts"] for f in want], "decoder %d: time stamps %r, expected %r" % (k, [f["pts"] for f in got], [f["pts"] for f in want])
        for t, (a, b) in enumerate(zip(got, want)):
            assert (a["width"], a["height"]) == (b["width"], b["height"]), "decoder %d, picture %d: the HIP decoder says %dx%d, expected %dx%d" % (k, t, a["width"], a["height"], b["width"], b["height"])
            if not np.array_equal(a["i420"], b["i420"]):
                d = np.flatnonzero(a["i420"] != b["i420"])
                w, h = b["width"], b["height"]
                at = (d[0] % w, d[0] // w) if d[0] < w * h else ((d[0] - w * h) % (w // 2), (d[0] - w * h) % (w * h // 4) // (w // 2))
                pytest.fail("decoder %d (%dx%d, threads %d), picture %d (time stamp %d): %d samples differ, first at %d (%s, x=%d y=%d); %d decoders%s"
                            % (k, w, h, s.get("threads", 1), t, a["pts"], len(d), d[0], "Y" if d[0] < w * h else "C", at[0], at[1], n, ", held" if hold else ""))
    return st
