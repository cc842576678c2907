"""GPU: the two promises of the encoder's device entry point (kvzx_encoder_encode_device, kvazaar.h input-hold) -- the way the benchmark's pictures go in.

input-hold off: "the caller may reuse its input buffer when this returns".  ONE device buffer serves the whole run and the next picture is written into it
the moment encode_device returns; the stream must still be the checker's.
input-hold=1: the caller leaves a picture unchanged until its access unit has come back, and the call returns without waiting for the input stage (owf >= 2: the
picture is read later, on the submitter thread).  Once with a buffer per picture that is never written again, once with a ring of owf + 2 buffers in which a
buffer is rewritten only after its picture's access unit has come back -- how the benchmark cycles its clip.

Every run -- and the host entry beside them -- gives the checker's encoder's access units and reconstructions for all 20 pictures, over the tools that read the
input picture behind the input stage or read an earlier input picture, at owf 0, 2 and 6.  Every check is an equality.  (input-hold with a packed input-format
stays refused: tests/test_gpu_input_formats.py.)"""
import functools

import numpy as np
import pytest

import devkit
import enckit
import orc
from kvazzup_amd import synth

SEED = enckit.SEED
W, H, N, CUT = 416, 240, 20, 7
BASE = (("qp", 32), ("period", 8), ("me-range", 16))
ORACLE = dict(qp=32, period=8, me_range=16)

# opts: the HIP encoder's; okw / oopts / n / tmvp / coarse: the checker's (enckit.oracle_encoder); cut: the scene-cut clip, whose cut makes an IDR picture from
# which the period counts anew -- the checker codes the pictures from the cut on as a stream of their own
SETS = {
    "plain": dict(),
    "me-source-subme2": dict(opts=(("me-source", 1), ("subme", 2)), okw=dict(subme=2), oopts=(("me-source", 1),)),
    "weightp": dict(opts=(("weightp", 1),), oopts=(("weightp", 1),)),
    "scenecut": dict(opts=(("scenecut", 2),), cut=CUT),
    "me-coarse64": dict(opts=(("me-coarse", 64),), coarse=64),
    "sao": dict(opts=(("sao", "full"),), okw=dict(sao=1)),
    "lp-refs3-tmvp": dict(opts=(("lp-refs", 3), ("tmvp", 1)), n=3, tmvp=1),
}


@functools.lru_cache(maxsize=None)
def _clip(cut=None):
    if cut is None:
        return tuple(synth.frame(synth.MOVING, SEED, W, H, t) for t in range(N))
    return tuple(synth.scene_cut_frame(SEED, W, H, t, cut) for t in range(N))


@functools.lru_cache(maxsize=None)
def _want(name):
    """[(access unit, reconstruction)] of the checker's encoder for the option set"""
    c = SETS[name]
    frames = _clip(c.get("cut"))
    out = []
    for first, last in ((0, c["cut"]), (c["cut"], N)) if c.get("cut") else ((0, N),):
        oe = enckit.oracle_encoder(W, H, n=c.get("n"), tmvp=c.get("tmvp"), coarse=c.get("coarse"), opts=c.get("oopts", ()), **dict(ORACLE, **c.get("okw", {})))
        try:
            for t in range(first, last):
                au = oe.encode(frames[t])
                out.append((au, oe.recon()))
        finally:
            oe.close()
    if c.get("cut"):
        idr = [t for t, (au, _) in enumerate(out) if (au[4] >> 1) == 32]          # (vps-period 1: parameter sets lead every IDR picture)
        assert idr == [0, c["cut"], c["cut"] + 8], idr
    return tuple(out)


def _recon(ge):
    ny = W * H
    rec = np.empty(ny * 3 // 2, dtype=np.uint8)
    assert ge.lib.kvzx_encoder_download_recon(ge.enc, rec.ctypes.data, rec.ctypes.data + ny, rec.ctypes.data + ny + ny // 4), "kvzx_encoder_download_recon failed"
    return rec


def _run_device(opts, frames, owf, bufs, hold):
    """the clip through encode_device.  bufs: the device buffers, picture t lies in bufs[t % len(bufs)]; a buffer that serves several pictures is rewritten
    as soon as the contract allows: the moment the call returns (hold off), or once the access unit of the picture it held has come back (hold on)"""
    ge = enckit.encoder(W, H, opts + (("owf", owf),) + ((("input-hold", 1),) if hold else ()))
    out = []
    try:
        for t in range(min(len(bufs), N)):
            bufs[t].upload(frames[t])
        for t in range(N):
            au = ge.encode_device(bufs[t % len(bufs)].ptr)
            nxt = t + 1
            if nxt < N and nxt >= len(bufs):                # the next picture's buffer holds picture nxt - len(bufs)
                if hold:
                    assert len(out) + bool(au) > nxt - len(bufs), "picture %d's access unit has not come back behind call %d: the ring is too short for the test" % (nxt - len(bufs), t)
                bufs[nxt % len(bufs)].upload(frames[nxt])
            if au:
                out.append((au, _recon(ge)))
        while len(out) < N:
            au = ge.encode_device(None)
            assert au, "the flush returned nothing with %d of %d access units out" % (len(out), N)
            out.append((au, _recon(ge)))
    finally:
        ge.close()
    return out


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for t, ((au, rec), (au_w, rec_w)) in enumerate(zip(got, want)):
        assert au == au_w, "%s: access unit %d has %d bytes, the checker's %d" % (what, t, len(au), len(au_w))
        assert np.array_equal(rec, rec_w), "%s: reconstruction %d differs from the checker's (%d samples)" % (what, t, int((rec != rec_w).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("owf", [0, 2, 6])
@pytest.mark.parametrize("name", sorted(SETS))
def test_device_entry_keeps_both_promises(gpu, name, owf):
    c = SETS[name]
    frames = _clip(c.get("cut"))
    assert all(not np.array_equal(frames[t], frames[t + 1]) for t in range(N - 1))      # (a picture read late would be another picture)
    want = _want(name)
    opts = BASE + tuple(c.get("opts", ()))
    ge = enckit.encoder(W, H, opts + (("owf", owf),))
    try:
        host = enckit.encode_all(ge, frames, owf)
    finally:
        ge.close()
    _same(host, want, "host entry")
    lib = ge.lib
    bufs = [devkit.DeviceBuffer(lib, W * H * 3 // 2) for _ in range(N)]
    try:
        one = _run_device(opts, frames, owf, bufs[:1], hold=False)
        _same(one, want, "input-hold off, one buffer rewritten behind every call")
        own = _run_device(opts, frames, owf, bufs, hold=True)
        _same(own, want, "input-hold=1, a buffer per picture")
        ring = _run_device(opts, frames, owf, bufs[:owf + 2], hold=True)
        _same(ring, want, "input-hold=1, a ring of %d buffers" % (owf + 2))
    finally:
        for b in bufs:
            b.free()
    for run in (one, own, ring):
        assert [au for au, _ in run] == [au for au, _ in host]
