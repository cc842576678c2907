"""GPU: the decoder's device-resident output (Decoder(download=False), kvzx_decoder_output_device) -- the path the benchmark times -- held to the checker's decoder.

1. Geometry: the planes handed out are the checker's picture at sizes without a crop window and with one in both directions, pitch = the padded coded width,
   synchronously, with frame threads and with the crop window switched off; the decoder's own consumer of those planes (kvzx_decoder_output_rgb32_device)
   gives the reference's conversion of the checker's picture.
2. Lifetime (include/kvazzup_amd.h kvzx_decoder_set_output_hold): a picture handed out equals the checker's when it is handed out, after each of the next n calls
   that begin a picture and immediately before the (n + 1)-th, for every thread count at which the decoder's GPU queue has another depth and n = 1, 2 (the
   default, left unset) and 8; on the HIP encoder's streams (one reference and four), a stream with B pictures in groups and one with long-term reference pictures.
   In the drain every end-of-sequence call moves the ring on by one picture as a picture's first NAL unit does, and counts like one.
   Beside it, so that the comparison cannot pass emptily: consecutive pictures differ in every plane, buffers are handed out again, and a picture whose hold ran
   out IS found overwritten later -- the test would see an early overwrite.

Every check is an equality.  No pointer is read after its decoder has been closed; the streams keep one picture size, so no buffer is released under the test."""
import functools

import numpy as np
import pytest

import devkit
import enckit
import orc
import refcolor

SEED = enckit.SEED
EOS = bytes([0, 0, 0, 1, 36 << 1, 1])


# ---- the streams and the checker's pictures, made once
def _checked(aus):
    """(access units, the checker's pictures in output order); consecutive pictures differ in every plane"""
    od = orc.OracleDecoder()
    want = []
    try:
        for t, au in enumerate(aus):
            want += od.decode_au(au, t)
        want += od.flush()
    finally:
        od.close()
    assert len(want) == len(aus), "the checker's decoder returned %d pictures of %d" % (len(want), len(aus))
    w, h = want[0]["width"], want[0]["height"]
    for t in range(1, len(want)):
        a, b = enckit.planes(want[t - 1]["i420"], w, h), enckit.planes(want[t]["i420"], w, h)
        assert all(not np.array_equal(a[c], b[c]) for c in range(3)), "pictures %d and %d of the checker's output share a plane: an overwrite by the next picture would not show" % (t - 1, t)
    return tuple(aus), tuple(p["i420"] for p in want), w, h


@functools.lru_cache(maxsize=None)
def _hip_stream(w, h, n, refs=1):
    """the HIP encoder's stream of the moving clip, period 8"""
    ge = enckit.encoder(w, h, (("qp", 32), ("period", 8), ("me-range", 16)) + ((("lp-refs", refs), ("tmvp", 1)) if refs > 1 else ()))
    try:
        out = enckit.encode_all(ge, enckit.frames(0, w, h, n))
    finally:
        ge.close()
    return _checked([au for au, _ in out])


@functools.lru_cache(maxsize=None)
def _checker_stream(w, h, n):
    """the checker's encoder's stream of the moving clip (sizes the HIP encoder does not take), period 4"""
    oe = orc.OracleEncoder(w, h, qp=30, period=4, me_range=8)
    try:
        return _checked([oe.encode(f) for f in enckit.frames(0, w, h, n)])
    finally:
        oe.close()


GEN = {"b-pictures": dict(seed=21, gop=4, b_slices=60, num_refs=3, tmvp=1, long_term=0),            # groups of four, decoded 4 2 1 3: pictures wait for their turn and leave in POC order
       "long-term": dict(seed=22, gop=0, b_slices=0, num_refs=2, long_term=1, intra_period=32)}     # references older than the ring of buffers is long


@functools.lru_cache(maxsize=None)
def _gen_stream(name, n=56):
    kw = dict(intra_period=8, density=40, wpp=1, slices=0, tile_rows=1, tile_cols=1, ctb_log2=6, open_gop=0, hidden_pics=0, temporal_layers=0, scaling_lists=0)
    kw.update(GEN[name])
    g = orc.OracleGen(416, 240, **kw)
    try:
        return _checked([g.picture() for _ in range(n)])
    finally:
        g.close()


def _stream(name):
    if name == "hip":
        return _hip_stream(416, 240, 80)
    if name == "hip-refs4":
        return _hip_stream(416, 240, 80, 4)
    return _gen_stream(name)


def _begins_picture(nal):
    """a slice segment NAL unit with first_slice_segment_in_pic_flag"""
    return len(nal) > 6 and (nal[4] >> 1) <= 31 and bool(nal[6] & 0x80)


class Handed:
    def __init__(self, index, planes, pitches):
        self.index, self.planes, self.pitches, self.age = index, planes, pitches, 0


def _read(gd, p, w, h):
    return devkit.download_i420(gd.lib, p.planes, p.pitches, w, h)


# ---- 1. geometry
def _geometry_stream(w, h):
    return _hip_stream(w, h, 10) if (w % 8 == 0 and h % 8 == 0) else _checker_stream(w, h, 10)


def _decode_all(gd, aus, per_picture):
    """every NAL unit, then the drain; per_picture(index, what decode_nal returned) behind every call that hands a picture out.  Returns the number handed out"""
    got = 0
    for t, au in enumerate(aus):
        for nal in orc.split_nals(au):
            f = gd.decode_nal(nal, t)
            if f is not None:
                per_picture(got, f)
                got += 1
    misses = 0
    while misses <= gd.threads + 1:
        f = gd.decode_nal(EOS)
        if f is not None:
            per_picture(got, f)
            got += 1
            misses = 0
        else:
            misses += 1
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("size", [(320, 192), (130, 70), (416, 240)])
def test_device_planes_are_the_checkers_picture(gpu, size, threads):
    from kvazzup_amd.codec import Decoder
    w, h = size
    aus, want, ww, wh = _geometry_stream(w, h)
    assert (ww, wh) == (w, h)
    pw = (w + 63) & ~63
    cropped = (w % 8 != 0 or h % 8 != 0) or pw != w
    variant = "simd" if w % 16 == 0 else "c"              # (variant 0: what the reference's filter picks for the width)
    gd = Decoder(threads=threads, frame_threads=threads > 1, download=False)
    rgb = devkit.DeviceBuffer(gd.lib, w * h * 4)

    def check(i, f):
        assert (f["width"], f["height"]) == (w, h), f
        planes, pitches = gd.output_device()
        assert pitches == [pw, pw // 2, pw // 2], "picture %d: pitches %s, the padded coded width is %d" % (i, pitches, pw)
        got = devkit.download_i420(gd.lib, planes, pitches, w, h)
        assert np.array_equal(got, want[i]), "picture %d differs from the checker's (%d samples)" % (i, int((got != want[i]).sum()))
        if cropped:
            rgb.upload(np.full(w * h * 4, 0x5A, np.uint8))
            assert gd.output_rgb32_device(rgb.ptr, 0)
            out = rgb.download()
            ref = refcolor.restatement(variant, want[i], w, h)
            assert np.array_equal(out, ref), "picture %d: the conversion in device memory differs from the reference's of the checker's picture (%d bytes)" % (i, int((out != ref).sum()))
    try:
        assert _decode_all(gd, aus, check) == len(aus)
    finally:
        gd.close()
        rgb.free()


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [1, 4])
def test_device_planes_without_cropping(gpu, threads):
    """libOpenHevcSetNoCropping: the planes start at the coded picture's corner; the checker's picture is its top left part"""
    from kvazzup_amd.codec import Decoder
    w, h = 130, 70
    aus, want, _, _ = _checker_stream(w, h, 10)
    cw, ch, pw = (w + 63) & ~63, (h + 63) & ~63, (w + 63) & ~63      # (the checker's encoder codes whole 64x64 coding tree blocks and crops)
    gd = Decoder(threads=threads, frame_threads=threads > 1, download=False, no_cropping=True)

    def check(i, f):
        assert (f["width"], f["height"]) == (cw, ch), f
        planes, pitches = gd.output_device()
        assert pitches == [pw, pw // 2, pw // 2], (i, pitches)
        for c, ref in enumerate(enckit.planes(want[i], w, h)):
            got = devkit.download_plane(gd.lib, planes[c], pitches[c], cw >> (c > 0), ch >> (c > 0))
            assert np.array_equal(got[:ref.shape[0], :ref.shape[1]], ref), "picture %d, plane %d differs from the checker's" % (i, c)
    try:
        assert _decode_all(gd, aus, check) == len(aus)
    finally:
        gd.close()


# ---- 2. lifetime
WATCH = 48      # calls a picture is looked at behind its hold, for the overwrite that must come


def _run_lifetime(name, threads, hold):
    from kvazzup_amd.codec import Decoder
    aus, want, w, h = _stream(name)
    gd = Decoder(threads=threads, frame_threads=threads > 1, download=False)
    if hold != 2:
        gd.set_output_hold(hold)                           # (2 is the default and stays unset)
    held, expired, addresses, overwritten = [], [], [], []
    got = 0

    def compare(p, when):
        pic = _read(gd, p, w, h)
        assert np.array_equal(pic, want[p.index]), "%s, %d frame threads, hold %d: picture %d %s differs from the checker's (%d samples): its buffer was written inside its hold" % (
            name, threads, hold, p.index, when, int((pic != want[p.index]).sum()))

    def call(nal, pts, counts):
        nonlocal got, held
        if counts:
            for p in held:
                compare(p, "before the call that begins picture number %d behind it" % (p.age + 1))
        f = gd.decode_nal(nal, pts)
        if counts:
            for p in held + expired:
                p.age += 1
            expired.extend(p for p in held if p.age > hold)
            held = [p for p in held if p.age <= hold]
        if f is not None:
            assert (f["width"], f["height"]) == (w, h), f
            planes, pitches = gd.output_device()
            held.append(Handed(got, planes, pitches))
            addresses.append(planes[0])
            got += 1
        for p in held:
            compare(p, "%d picture(s) behind the call that handed it out" % p.age)
        for p in list(expired):                            # (live memory: the decoder is open and the picture size has not changed)
            if not np.array_equal(_read(gd, p, w, h), want[p.index]):
                overwritten.append((p.index, p.age))
                expired.remove(p)
            elif p.age > hold + WATCH:
                expired.remove(p)

    try:
        for t, au in enumerate(aus):
            for nal in orc.split_nals(au):
                call(nal, t, _begins_picture(nal))
        misses = 0
        while misses <= threads + 1:
            before = got
            call(EOS, 0, True)
            misses = 0 if got > before else misses + 1
    finally:
        gd.close()
    assert got == len(aus), "%d pictures handed out of %d" % (got, len(aus))
    assert len(set(addresses)) < got, "every picture had a buffer of its own (%d addresses): nothing was handed out twice" % len(set(addresses))
    assert overwritten, "no picture was ever found overwritten behind its hold: the comparison could not have seen an early overwrite"
    assert min(age for _, age in overwritten) > hold
    return overwritten


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [1, 2, 8])
@pytest.mark.parametrize("threads", [1, 3, 4, 12, 24, 32])
def test_handed_out_pictures_stay_for_their_hold(gpu, threads, hold):
    _run_lifetime("hip", threads, hold)


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [2, 8])
def test_handed_out_pictures_stay_with_four_references(gpu, hold):
    _run_lifetime("hip-refs4", 32, hold)


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [2, 8])
@pytest.mark.parametrize("threads", [1, 32])
@pytest.mark.parametrize("name", sorted(GEN))
def test_handed_out_pictures_stay_in_foreign_streams(gpu, name, threads, hold):
    _run_lifetime(name, threads, hold)
