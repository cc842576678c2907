"""GPU: the benchmark's pipeline at the benchmark's settings (tools/benchkit/stream.py run_stream / multi_stream), whole intra periods against the checker's encoder.

The timed path hands the encoder pictures that lie in device memory and stay there untouched (push_device_paced, input-hold=1), keeps six pictures in flight in
the encoder (video/OWF 6: its eight working sets in rotation), parses with 32 frame threads and leaves the decoded pictures in device memory
(uvgx/decoderDownload 0).  Here that very pipeline runs at 416x240, where the checker's encoder follows it through two whole periods: every one of the 130 access
units equals the checker's, IDR pictures fall at 0, 64 and 128, nothing is dropped, and the checker's decoder makes the checker's reconstruction of every access
unit.  Then the default-mode leg (preset veryfast at a bitrate, the search on the input picture) and three such pipelines at once in one process, each against
its own checker stream (held inputs and the decoders' shared submission layer together).  The settings are read from bench.py and tools/benchkit, not restated.
tests/test_gpu_configs.py test_config1_long_run_two_idrs runs the same length at 1080p, where the checker's encoder is followed for three pictures only."""
import functools
import os
import sys
import threading

import numpy as np
import pytest

import devkit
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench                                                    # noqa: E402
from tools.benchkit.workloads import CLIP_FRAMES, PERIOD, WORKLOADS, stream_seed      # noqa: E402

W, H, N = 416, 240, 2 * PERIOD + 2
CFG = WORKLOADS["1080p"]["cfg_index"]


@functools.lru_cache(maxsize=None)
def _bench_args():
    """bench.py's own defaults (a plain `bench.py` run)"""
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        return bench.parse_args()
    finally:
        sys.argv = argv


def _frame_threads(streams=1):
    a = _bench_args()
    return max(1, a.decoder_frame_threads or 32) if streams == 1 else max(2, min(32, 32 // streams))      # (run_stream's D; multi_stream's)


DEFAULT_MODE = {"video/Preset": "veryfast", "video/bitrate": 1000000}      # (bench.py default_mode_leg's settings)


def _pipeline(default_mode=False, streams=1):
    """the pipeline run_stream's make(keep, download=False) builds (multi_stream's with streams > 1), kept outputs"""
    from kvazzup_amd.pipeline import Pipeline
    a = _bench_args()
    D = _frame_threads(streams)
    st = {"video/QP": 32, "video/Intra": PERIOD, "video/VPS": 1, "uvgx/gpu": 0, "uvgx/decoderDownload": 0,
          "video/OWF": a.owf, "video/OPENHEVC_threads": D, "video/OH_parallelization": "Frame" if D > 1 else "Slice"}
    if streams > 1:
        st["video/kvzThreads"] = 4
    custom = (("me-range", a.me_range), ("gpu", 0)) + bench.RESIDENT
    if default_mode:
        st.update(DEFAULT_MODE)
        custom += (("me-source", "1"),)
    return Pipeline(W, H, settings=st, custom=custom, loopback=True, keep_outputs=True)


@functools.lru_cache(maxsize=None)
def _host_clip(seed):
    return tuple(orc.synth_frame(0, seed, W, H, t) for t in range(CLIP_FRAMES))


@functools.lru_cache(maxsize=None)
def _want(seed, default_mode=False, n=N):
    """[(access unit, reconstruction)] of the checker's encoder over the n pictures the pipeline is fed (the clip cycled, as the benchmark cycles it)"""
    a = _bench_args()
    clip = _host_clip(seed)
    if default_mode:
        br = DEFAULT_MODE["video/bitrate"]
        oe = orc.OracleEncoder(W, H, qp=32, period=PERIOD, me_range=a.me_range, sao=1, subme=2, bitrate=br, rc_bands=4)
        oe.set_option("intra-in-p", 1); oe.set_option("rc-delay", min(a.owf, 6) + 1); oe.set_option("me-source", 1)      # (as tests/test_gpu_configs.py test_default_mode_pipelined...)
    else:
        oe = orc.OracleEncoder(W, H, qp=32, period=PERIOD, me_range=a.me_range)
    od = orc.OracleDecoder()
    out = []
    try:
        for t in range(n):
            au = oe.encode(clip[t % CLIP_FRAMES])
            rec = oe.recon()
            pics = od.decode_au(au, t)
            assert len(pics) == 1 and np.array_equal(pics[0]["i420"], rec), "picture %d: the checker's decoder does not make the checker's reconstruction" % t
            out.append((au, rec))
    finally:
        oe.close(); od.close()
    return tuple(out)


def _device_clip(lib, seed):
    bufs = devkit.synth_clip(lib, 0, seed & 0xFFFFFFFF, W, H, CLIP_FRAMES)
    return bufs


def _run(pl, bufs, n=N):
    """push n pictures as run_stream's run() does, flush, wait; returns the access units [(bytes, pts)]"""
    while pl.pushed < n:
        assert pl.push_device_paced(bufs[pl.pushed % CLIP_FRAMES].ptr, 6, 120000), "pipeline stalled: %r" % (pl.stats(),)
    pl.flush()
    assert pl.wait(n, 120000), "pipeline did not deliver %d pictures: %r" % (n, pl.stats())
    aus = []
    while True:
        a = pl.pop_encoded()
        if a is None:
            break
        aus.append(a)
    return aus


def _check(pl, aus, want, what=""):
    n = len(want)
    st = pl.stats()
    assert st["decoded_pictures"] == n and st["dropped"] == 0 and st["encoded_pictures"] == n and st["encoder_inputs_discarded"] == 0, (what, st)
    assert [pts for _, pts in aus] == list(range(n)), what
    assert [t for t in range(n) if (aus[t][0][4] >> 1) == 32] == list(range(0, n, PERIOD)), what      # access units that start with a VPS
    for t in range(n):
        assert aus[t][0] == want[t][0], "%saccess unit %d has %d bytes, the checker's encoder makes %d" % (what, t, len(aus[t][0]), len(want[t][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["headline", "default-mode"])
def test_timed_path_gives_the_checkers_stream(gpu, mode):
    a = _bench_args()
    assert (a.owf, _frame_threads(), a.me_range, PERIOD, bench.RESIDENT) == (6, 32, 16, 64, (("input-hold", "1"),))      # (what the issue at hand was written against)
    seed = stream_seed(CFG, 0)
    n = N
    want = _want(seed, mode == "default-mode", n)
    pl = _pipeline(mode == "default-mode")
    bufs = _device_clip(pl.lib, seed)
    try:
        if mode == "headline":
            host = _host_clip(seed)
            for t in range(CLIP_FRAMES):
                assert np.array_equal(bufs[t].download(), host[t]), "picture %d of the device clip differs from the checker's clip" % t
        aus = _run(pl, bufs, n)
        _check(pl, aus, want)
    finally:
        pl.close()
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_three_timed_paths_at_once(gpu):
    K, n = 3, N
    seeds = [stream_seed(CFG, k) for k in range(K)]
    wants = [_want(s, False, n) for s in seeds]                  # (one after the other: the checker keeps state between calls that two encoders at once would share)
    pls = [_pipeline(streams=K) for _ in range(K)]
    clips = [_device_clip(pls[0].lib, s) for s in seeds]
    got, errors = [None] * K, []
    gate = threading.Barrier(K)

    def body(k):
        try:
            gate.wait()
            got[k] = _run(pls[k], clips[k], n)
        except BaseException as e:                               # noqa: BLE001
            gate.abort()
            errors.append((k, e))
    try:
        ths = [threading.Thread(target=body, args=(k,)) for k in range(K)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errors, errors
        for k in range(K):
            _check(pls[k], got[k], wants[k], "stream %d: " % k)
    finally:
        for pl in pls:
            pl.close()
        for c in clips:
            for b in c:
                b.free()
