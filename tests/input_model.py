"""Statement of the encoder's input stage for packed pictures ("input-format", kvazaar.h), in numpy: what the reference's converters make of
an RGB32 or YUYV picture (the RGB statements are tests/refcolor.py's; yuyv_to_yuv420_c, src/media/processing/yuvconversions.cpp:800-834, is stated here), and that
picture padded to the coded size by edge replication, which is what k_pad_input makes of an I420 picture.  padded() is what the working set's source planes must
hold after k_input_rgb32 / k_input_yuyv.  Test infrastructure only."""
import ctypes as C

import numpy as np

import refcolor

FORMATS = ("rgb32", "rgb32-sse41", "yuyv")
YUYV_SYM = "_Z16yuyv_to_yuv420_cPhS_tt"          # yuyv_to_yuv420_c(uint8_t *, uint8_t *, uint16_t, uint16_t), yuvconversions.h


def packed_bytes(fmt, w, h):
    return w * h * (2 if fmt == "yuyv" else 4)


def yuyv_to_i420(yuyv, w, h):
    """luma copied; a chroma sample is the truncating mean of the two rows' samples"""
    p = np.asarray(yuyv, dtype=np.uint8).reshape(h, w // 2, 4).astype(np.uint16)
    y = p[..., 0::2].reshape(h, w)
    u = (p[0::2, :, 1] + p[1::2, :, 1]) // 2
    v = (p[0::2, :, 3] + p[1::2, :, 3]) // 2
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint8)


def reference_yuyv(yuyv, w, h, fill=0x5A):
    """the reference's own object code (oracle/_ref, refcolor.available()); None when the library does not export the function"""
    lib = C.CDLL(refcolor.REF_SO)
    try:
        fn = getattr(lib, YUYV_SYM)
    except AttributeError:
        return None
    fn.restype = None
    src = np.ascontiguousarray(yuyv, dtype=np.uint8)
    out = np.full(w * h * 3 // 2, fill, dtype=np.uint8)
    fn(src.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint16(w), C.c_uint16(h))
    return out


def convert(fmt, packed, w, h):
    """the packed I420 picture the reference's converter of `fmt` makes"""
    if fmt == "yuyv":
        return yuyv_to_i420(packed, w, h)
    return refcolor.restatement_rgb2yuv("c" if fmt == "rgb32" else "sse41", packed, w, h)


def coded_size(w, h):
    return max(128, (w + 63) & ~63), (h + 63) & ~63


def pad(i420, w, h):
    """the three coded planes of an I420 picture: every sample beyond the picture takes the nearest sample inside, per plane"""
    cw, ch = coded_size(w, h)
    ny = w * h
    src = (i420[:ny].reshape(h, w), i420[ny:ny + ny // 4].reshape(h // 2, w // 2), i420[ny + ny // 4:].reshape(h // 2, w // 2))
    return tuple(np.pad(p, ((0, (ch >> (c > 0)) - p.shape[0]), (0, (cw >> (c > 0)) - p.shape[1])), mode="edge") for c, p in enumerate(src))


def padded(fmt, packed, w, h):
    return pad(convert(fmt, packed, w, h), w, h)


def random_yuyv(seed, w, h):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, w * h * 2, dtype=np.uint8)
    a[:16] = 0                     # extremes: the first eight pixels black-and-zero chroma, the last eight all 255
    a[-16:] = 255
    if h >= 2:                     # ... and a chroma pair 0 / 255 and 255 / 254 across the first two rows (the mean truncates)
        a[17], a[w * 2 + 17], a[19], a[w * 2 + 19] = 0, 255, 255, 254
    return a


def random_packed(fmt, seed, w, h):
    return random_yuyv(seed, w, h) if fmt == "yuyv" else refcolor.random_rgb32(seed, w, h)
