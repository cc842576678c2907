"""GPU: "input-format" (kvazaar.h) -- the encoder takes packed RGB32 / YUYV pictures and converts them in its input stage.

The feature is held to: the working set's padded source planes equal tests/input_model.py's padded() -- the reference's converter, then edge replication --
sample for sample, for random and synthetic pictures through the host and the device entry point, at sizes that pad in neither, one and both directions and at
1080p; the access units and reconstructions equal those of an i420 encoder with the same options fed the converted pictures, byte for byte, over presets, owf and
the options that read the input pictures; the same once through the filter graph with loop-back decode; what encoder_open and the entry points refuse; and
input-format=i420 changes no byte.  Every check is an equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import enckit
import input_model as M
from kvazzup_amd import synth

SEED = enckit.SEED
BASE = (("qp", 32), ("me-range", 8), ("vps-period", 1))
SIZES = [(64, 64), (72, 40), (320, 192), (416, 240)]       # no padding; pads to 128x64, width % 16 != 0, chroma width 36; whole CTUs; pads in both directions
PLANES = ("src0", "src1", "src2")


class DeviceBuffer:
    """a packed picture in device memory, through the library's own helpers"""

    def __init__(self, lib, data):
        lib.kvzx_harness_alloc.restype = C.c_void_p
        lib.kvzx_harness_alloc.argtypes = [C.c_int, C.c_size_t]
        lib.kvzx_harness_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.kvzx_harness_free.argtypes = [C.c_void_p]
        self.lib = lib
        data = np.ascontiguousarray(data, dtype=np.uint8)
        self.ptr = lib.kvzx_harness_alloc(0, data.nbytes)
        assert self.ptr and lib.kvzx_harness_upload(self.ptr, data.ctypes.data, data.nbytes)
        lib.kvzx_harness_sync(0)

    def free(self):
        self.lib.kvzx_harness_free(self.ptr)


@functools.lru_cache(maxsize=None)
def _clip(w, h, n, cut=None):
    """the benchmark's moving clip (cut: its scene-cut form), I420"""
    if cut is None:
        return tuple(synth.frame(synth.MOVING, SEED, w, h, t) for t in range(n))
    return tuple(synth.scene_cut_frame(SEED, w, h, t, cut) for t in range(n))


def _packed(fmt, i420, w, h):
    return synth.to_yuyv(i420, w, h) if fmt == "yuyv" else synth.to_rgb32(i420, w, h)


@functools.lru_cache(maxsize=None)
def _packed_clip(fmt, w, h, n, cut=None):
    return tuple(_packed(fmt, f, w, h) for f in _clip(w, h, n, cut))


def _planes_equal(ge, want, what):
    cw, ch = ge.coded_size()
    assert (cw, ch) == (want[0].shape[1], want[0].shape[0]), (cw, ch, want[0].shape)
    for c, name in enumerate(PLANES):
        got = ge.debug(name, np.uint8, want[c].shape)
        bad = np.argwhere(got != want[c])
        assert not len(bad), "%s: %s differs at %d samples, first (row, column) %s: GPU %d, statement %d" % (
            what, name, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[c][tuple(bad[0])])


# ---- 1. the padded planes against the statement
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_padded_planes_equal_the_statement(gpu, fmt, size):
    w, h = size
    pictures = {"random": M.random_packed(fmt, 11, w, h), "synth": _packed(fmt, _clip(w, h, 2)[1], w, h)}
    ge = enckit.encoder(w, h, BASE + (("input-format", fmt), ("period", 1)))
    bufs = []
    try:
        for name, pic in pictures.items():
            want = M.padded(fmt, pic, w, h)
            au, _ = ge.encode_packed(pic, want_recon=False)
            assert au
            _planes_equal(ge, want, "%s picture, host entry" % name)
            bufs.append(DeviceBuffer(ge.lib, pic))
            au, _ = ge.encode_packed_device(bufs[-1].ptr, want_recon=False)
            assert au
            _planes_equal(ge, want, "%s picture, device entry" % name)
    finally:
        ge.close()
        for b in bufs:
            b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_padded_planes_equal_the_statement_1080p(gpu, fmt):
    w, h = 1920, 1080                                      # the grid's last workgroups; 1080 -> 1088
    pic = M.random_packed(fmt, 12, w, h)
    ge = enckit.encoder(w, h, BASE + (("input-format", fmt),))
    buf = DeviceBuffer(ge.lib, pic)
    try:
        au, _ = ge.encode_packed_device(buf.ptr, want_recon=False)
        assert au
        _planes_equal(ge, M.padded(fmt, pic, w, h), "1080p")
    finally:
        ge.close()
        buf.free()


# ---- 2. the invariant: the stream and the reconstructions are those of an i420 encoder fed the converted pictures
def _run_i420(w, h, opts, frames, owf, fields=None):
    ge = enckit.encoder(w, h, opts, fields=fields)
    try:
        return enckit.encode_all(ge, frames, owf)
    finally:
        ge.close()


def _run_packed(w, h, opts, fmt, pictures, owf, fields=None):
    ge = enckit.encoder(w, h, opts + (("input-format", fmt),), fields=fields)
    out = []
    try:
        for t in range(len(pictures) + owf + 1):
            au, rec = ge.encode_packed(pictures[t] if t < len(pictures) else None)
            if au:
                out.append((au, rec))
    finally:
        ge.close()
    assert len(out) == len(pictures), "%d pictures in, %d access units out" % (len(pictures), len(out))
    return out


def _same(got, want):
    assert len(got) == len(want)
    for t, ((au, rec), (au_w, rec_w)) in enumerate(zip(got, want)):
        assert au == au_w, "access unit %d: %d bytes, the i420 encoder fed the converted picture makes %d" % (t, len(au), len(au_w))
        assert np.array_equal(rec, rec_w), "reconstruction %d differs from the i420 encoder's (%d samples)" % (t, int((rec != rec_w).sum()))


INVARIANT = {
    "ultrafast-owf0": dict(opts=(("preset", "ultrafast"),)),
    "ultrafast-owf2": dict(opts=(("preset", "ultrafast"),), owf=2),
    "veryfast-owf0": dict(opts=(("preset", "veryfast"),)),
    "veryfast-owf2": dict(opts=(("preset", "veryfast"),), owf=2),
    "src-subme2": dict(opts=(("me-source", 1), ("subme", 2))),
    "scenecut": dict(opts=(("scenecut", 1),), cut=4),
    "weightp": dict(opts=(("weightp", 1),)),
    "me-coarse64": dict(opts=(("me-coarse", 64),)),
    "bitrate-lambda": dict(opts=(("bitrate", 400000), ("rc-algorithm", "lambda")), fields={"target_bitrate": 400000}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INVARIANT))
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_stream_equals_the_i420_encoders(gpu, fmt, name):
    w, h, n = 416, 240, 8
    c = INVARIANT[name]
    owf = c.get("owf", 0)
    opts = BASE + (("period", 64), ("owf", owf)) + tuple(c["opts"])
    pictures = _packed_clip(fmt, w, h, n, c.get("cut"))
    converted = [M.convert(fmt, p, w, h) for p in pictures]
    want = _run_i420(w, h, opts, converted, owf, c.get("fields"))
    if c.get("cut"):
        assert sum(((au[4] >> 1) & 63) == 32 for au, _ in want) == 2, "the clip's cut did not make an IDR picture"      # (vps-period 1: parameter sets lead every IDR picture)
    _same(_run_packed(w, h, opts, fmt, pictures, owf, c.get("fields")), want)


@pytest.mark.gpu
@pytest.mark.parametrize("owf", [0, 2])
def test_page_locked_pictures_give_the_same_stream(gpu, owf):
    """a packed picture that starts a page-locked kvz_picture is read where it lies (owf 2: handed to the submitter thread); one kvz_picture per picture, none written again"""
    w, h, n, fmt = 416, 240, 8, "rgb32"
    opts = BASE + (("period", 64), ("owf", owf))
    pictures = _packed_clip(fmt, w, h, n)
    want = _run_i420(w, h, opts, [M.convert(fmt, p, w, h) for p in pictures], owf)
    ge = enckit.encoder(w, h, opts + (("input-format", fmt),))
    pics = [ge.api.picture_alloc(w, 3 * h) for _ in range(n)]          # (w * 3h * 3 / 2 + 64 bytes each: room for w * h * 4)
    out = []
    try:
        assert all(pics)
        for t in range(n + owf + 1):
            view = None
            if t < n:
                view = np.frombuffer((C.c_uint8 * pictures[t].nbytes).from_address(pics[t].contents.fulldata_buf), dtype=np.uint8)
                view[:] = pictures[t]
            au, rec = ge.encode_packed(view)
            if au:
                out.append((au, rec))
    finally:
        ge.close()
        for p in pics:
            ge.api.picture_free(p)
    _same(out, want)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_pipeline_with_loop_back_decode(gpu, fmt):
    from kvazzup_amd.pipeline import Pipeline
    w, h, n = 416, 240, 8
    pictures = _packed_clip(fmt, w, h, n)
    want = _run_i420(w, h, (("me-range", 16),), [M.convert(fmt, p, w, h) for p in pictures], 0)
    pl = Pipeline(w, h, settings={"video/QP": 32, "video/Intra": 64, "uvgx/inputFormat": fmt}, custom=(("me-range", 16),))
    try:
        for t in range(n):
            assert pl.push_packed(pictures[t], fmt, t)
            assert pl.wait(t + 1, 60000), pl.stats()
        aus = [pl.pop_encoded() for _ in range(n)]
        dec = [pl.pop_decoded() for _ in range(n)]
    finally:
        pl.close()
    for t in range(n):
        assert aus[t] is not None and dec[t] is not None, t
        assert aus[t][0] == want[t][0], "access unit %d differs from the i420 encoder's" % t
        assert np.array_equal(dec[t]["i420"], want[t][1]), "decoded picture %d differs from the reconstruction" % t


@pytest.mark.gpu
def test_pipeline_takes_a_device_picture(gpu):
    from kvazzup_amd.pipeline import Pipeline
    w, h, fmt = 72, 40, "yuyv"
    pic = _packed_clip(fmt, w, h, 1)[0]
    want = _run_i420(w, h, (("me-range", 16),), [M.convert(fmt, pic, w, h)], 0)
    pl = Pipeline(w, h, settings={"video/QP": 32, "video/Intra": 64, "uvgx/inputFormat": fmt}, custom=(("me-range", 16),), loopback=False)
    buf = DeviceBuffer(pl.lib, pic)
    try:
        assert pl.push_packed(buf.ptr, fmt, 0, device=True)
        assert pl.wait(1, 60000), pl.stats()
        assert pl.pop_encoded()[0] == want[0][0]
    finally:
        pl.close()
        buf.free()


# ---- 3. what is refused
def _open_fails(w, h, opts, capfd, say):
    from kvazzup_amd.codec import Encoder
    with pytest.raises(RuntimeError):
        Encoder(w, h, options=opts)
    assert say in capfd.readouterr().err


@pytest.mark.gpu
def test_encoder_open_refuses_input_hold(gpu, capfd):
    _open_fails(256, 256, (("input-format", "yuyv"), ("input-hold", 1)), capfd, "input-hold")


@pytest.mark.gpu
def test_encoder_open_refuses_band_mode(gpu, capfd):
    _open_fails(256, 256, (("input-format", "rgb32"), ("tiles", "1x2"), ("band-row0", 0), ("band-rows", 2)), capfd, "band mode")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["rgb32", "rgb32-sse41"])
def test_encoder_open_refuses_rgb32_width(gpu, capfd, fmt):
    _open_fails(70, 64, (("input-format", fmt),), capfd, "multiple of 4")


@pytest.mark.gpu
def test_yuyv_takes_a_width_that_is_no_multiple_of_8(gpu):
    w, h, fmt = 70, 42, "yuyv"                             # a lane straddles the picture's right edge
    pic = M.random_packed(fmt, 13, w, h)
    ge = enckit.encoder(w, h, BASE + (("input-format", fmt),))
    try:
        au, _ = ge.encode_packed(pic, want_recon=False)
        assert au
        _planes_equal(ge, M.padded(fmt, pic, w, h), "70x42")
    finally:
        ge.close()


@pytest.mark.gpu
def test_i420_entry_points_refuse_a_packed_encoder(gpu):
    w, h = 64, 64
    ge = enckit.encoder(w, h, BASE + (("input-format", "yuyv"),))
    frame = _clip(w, h, 1)[0]
    buf = DeviceBuffer(ge.lib, frame)
    n, au = C.c_uint32(0), np.empty(1 << 20, dtype=np.uint8)
    try:
        with pytest.raises(RuntimeError):
            ge.encode(frame)                               # encoder_encode(kvz_picture): a kvz_picture carries planes
        with pytest.raises(RuntimeError):
            ge.encode_device(buf.ptr)
        ny = w * h
        assert ge.lib.kvzx_encoder_encode_host(ge.enc, frame.ctypes.data, frame.ctypes.data + ny, frame.ctypes.data + ny + ny // 4, au.ctypes.data, au.size, C.byref(n), None) == 0
        assert ge.lib.kvzx_encoder_pending(ge.enc) == 0
        out, _ = ge.encode_packed(_packed("yuyv", frame, w, h))      # ... and the encoder is none the worse for it
        assert out
    finally:
        ge.close()
        buf.free()


@pytest.mark.gpu
def test_packed_entry_points_refuse_an_i420_encoder(gpu):
    w, h = 64, 64
    ge = enckit.encoder(w, h, BASE)
    pic = _packed("rgb32", _clip(w, h, 1)[0], w, h)
    buf = DeviceBuffer(ge.lib, pic)
    n, au = C.c_uint32(0), np.empty(1 << 20, dtype=np.uint8)
    try:
        assert ge.lib.kvzx_encoder_encode_packed_host(ge.enc, pic.ctypes.data, au.ctypes.data, au.size, C.byref(n), None) == 0
        assert ge.lib.kvzx_encoder_encode_packed_device(ge.enc, buf.ptr, au.ctypes.data, au.size, C.byref(n), None) == 0
        assert ge.lib.kvzx_encoder_pending(ge.enc) == 0
    finally:
        ge.close()
        buf.free()


@pytest.mark.gpu
def test_config_parse_knows_the_formats(gpu):
    from kvazzup_amd.codec import Encoder
    ge = Encoder(64, 64, options=(("input-format", "nv12"),))
    try:
        assert ge.rejected == ["input-format"] and int(ge.cfg.contents.input_format) == 0
        for k, fmt in enumerate(("i420",) + M.FORMATS):
            assert ge.api.config_parse(ge.cfg, b"input-format", fmt.encode()) == 1 and int(ge.cfg.contents.input_format) == k
        for bad in (b"", b"nv12", b"RGB32", b"1"):
            assert ge.api.config_parse(ge.cfg, b"input-format", bad) == 0
    finally:
        ge.close()


# ---- 4. input-format=i420 is the option-less encoder
@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["ultrafast", "veryfast"])
def test_explicit_i420_changes_no_byte(gpu, preset):
    w, h, n = 416, 240, 6
    opts = BASE + (("preset", preset), ("period", 64))
    frames = _clip(w, h, n)
    _same(_run_i420(w, h, opts + (("input-format", "i420"),), frames, 0), _run_i420(w, h, opts, frames, 0))
