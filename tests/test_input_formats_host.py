"""CPU: the statement of the encoder's packed input formats (tests/input_model.py, "input-format") -- yuyv_to_yuv420_c against the
reference's own object code where build() has made it, the RGB statements against theirs, the padding by edge replication, and the test-picture helpers of
kvazzup_amd.synth."""
import numpy as np
import pytest

import input_model as M
import refcolor
from kvazzup_amd import synth

SIZES = [(16, 2), (72, 40), (416, 240)]

needs_ref = pytest.mark.skipif(not refcolor.available(), reason="oracle/_ref/libyuvconversions_ref.so has not been built (no reference tree)")


@needs_ref
@pytest.mark.parametrize("size", SIZES)
def test_yuyv_statement_equals_the_reference_object_code(size):
    w, h = size
    for seed in (1, 2):
        src = M.random_yuyv(seed, w, h)
        want = M.reference_yuyv(src, w, h)
        assert want is not None, "the reference library does not export %s" % M.YUYV_SYM
        assert np.array_equal(M.yuyv_to_i420(src, w, h), want)


@needs_ref
@pytest.mark.parametrize("fmt", ["rgb32", "rgb32-sse41"])
@pytest.mark.parametrize("size", [(16, 2), (72, 40)])
def test_rgb_statements_equal_the_reference_object_code(fmt, size):
    w, h = size
    src = refcolor.random_rgb32(3, w, h)
    assert np.array_equal(M.convert(fmt, src, w, h), refcolor.reference_rgb2yuv("c" if fmt == "rgb32" else "sse41", src, w, h))


def test_yuyv_statement_by_hand():
    # 4x2: Y0 U Y1 V per pixel pair; chroma means (0 + 255) // 2 = 127, (255 + 254) // 2 = 254, (1 + 2) // 2 = 1, (7 + 7) // 2 = 7
    src = np.array([10, 0, 11, 255, 12, 1, 13, 7,
                    20, 255, 21, 254, 22, 2, 23, 7], dtype=np.uint8)
    assert M.yuyv_to_i420(src, 4, 2).tolist() == [10, 11, 12, 13, 20, 21, 22, 23, 127, 1, 254, 7]


def test_pad_replicates_each_plane_by_itself():
    w, h = 72, 40
    i420 = refcolor.random_i420(5, w, h)
    Y, U, V = M.pad(i420, w, h)
    assert Y.shape == (64, 128) and U.shape == V.shape == (32, 64)
    assert np.array_equal(Y[:h, :w].reshape(-1), i420[:w * h])
    assert (Y[:h, w:] == Y[:h, w - 1:w]).all() and (Y[h:] == Y[h - 1]).all()
    assert (U[:h // 2, w // 2:] == U[:h // 2, w // 2 - 1:w // 2]).all() and (V[h // 2:] == V[h // 2 - 1]).all()
    assert M.coded_size(64, 64) == (128, 64) and M.coded_size(1920, 1080) == (1920, 1088)


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_padded_is_convert_then_pad(fmt):
    w, h = 72, 40
    src = M.random_packed(fmt, 7, w, h)
    got = M.padded(fmt, src, w, h)
    want = M.pad(M.convert(fmt, src, w, h), w, h)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    if fmt == "rgb32-sse41":                                # the flip comes first: the coded picture's bottom rows repeat the SOURCE picture's top row
        top = refcolor.restatement_rgb2yuv("sse41", src, w, h)[:w * h].reshape(h, w)[h - 1]
        assert (got[0][h:, :w] == top).all()


def test_synth_helpers_build_packed_pictures():
    w, h = 72, 40
    f = synth.frame(synth.MOVING, 0x5EED0000, w, h, 3)
    rgb, yuyv = synth.to_rgb32(f, w, h), synth.to_yuyv(f, w, h)
    assert rgb.dtype == np.uint8 and rgb.size == M.packed_bytes("rgb32", w, h) and yuyv.dtype == np.uint8 and yuyv.size == M.packed_bytes("yuyv", w, h)
    assert np.array_equal(rgb, synth.to_rgb32(f, w, h)) and np.array_equal(yuyv, synth.to_yuyv(f, w, h))      # deterministic
    back = M.yuyv_to_i420(yuyv, w, h)
    assert np.array_equal(back[:w * h], f[:w * h])          # luma travels as it is
    assert np.abs(back[w * h:].astype(int) - f[w * h:].astype(int)).max() <= 1      # chroma: c and c ^ 1 average to c or c - 1
    assert len(np.unique(rgb.reshape(-1, 4)[:, :3], axis=0)) > 100       # a picture, not a constant
