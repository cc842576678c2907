"""weightp ("uvgx weighted prediction v1") on the GPU: what weightp=1 costs and buys against the same encoder without it, at 1080p and
2160p, presets ultrafast and veryfast (wpp, period 64, qp 32), on the benchmark clip and on that clip with a brightness change applied to its luma
(tests/wp_model.change: offset -6 levels per picture, gain -3/64 per picture, +8 levels on every fourth picture).  Option off is the reference of every ratio.

  quality  owf 0: bits per P picture, luma PSNR over the P pictures and how many P pictures were weighted against reference 0
  rate     encoder pictures/s of a clip resident in device memory (kvzx_encoder_encode_device, input-hold, owf 2), one warm-up pass; off and on alternate
           inside this one command, two rounds
  trace    `--trace KIND PRESET ON [HEIGHT]`: encodes the clip once and nothing else -- the program for a kernel-trace run of its own, e.g.
           rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure/weightp_ab.py --trace none ultrafast 1
           (the times of k_wp_stats, k_wp_decide, k_wp_check and k_wp_plane come from that run's kernel statistics)

usage: python tools/measure/weightp_ab.py [out.txt] [--quick] [--rate-only]      (one JSON object per line, also appended to out.txt; --quick: 1080p only)"""
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import orc  # noqa: E402
import wp_model  # noqa: E402
from kvazzup_amd import _native  # noqa: E402
from kvazzup_amd.codec import Encoder  # noqa: E402

LIB = _native.load_library()
NF = 13
KINDS = ("none", "offset", "gain", "flash")
SIZES = ((1920, 1080), (3840, 2160))
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = ARGS[0] if ARGS and "--trace" not in sys.argv else None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def opts(preset, on, owf):
    return (("preset", preset), ("threads", 8), ("owf", owf), ("wpp", 1), ("qp", 32), ("period", 64), ("me-range", 16), ("weightp", on))


def make_clip(kind, w, h, nf=NF):
    return wp_model.change([orc.synth_frame(0, 1234, w, h, t) for t in range(nf)], w, h, kind)


def quality(frames, w, h, options, on):
    e = Encoder(w, h, options=options)
    assert not e.rejected, e.rejected
    ny = w * h
    bits, psnr, weighted = [], [], 0
    for t, f in enumerate(frames):
        au, rec = e.encode(f)
        if t == 0:
            continue
        bits.append(8 * len(au))
        mse = np.mean((rec[:ny].astype(np.float64) - f[:ny]) ** 2)
        psnr.append(10 * np.log10(255 ** 2 / max(mse, 1e-9)))
        if on:
            weighted += int(e.debug("wp", np.int32, (4, 3))[0][0])
    e.close()
    return int(np.mean(bits)), round(float(np.mean(psnr)), 3), weighted


def upload(frames):
    """the clip into device memory through the library's own helpers"""
    import ctypes as C
    LIB.kvzx_harness_alloc.restype = C.c_void_p
    LIB.kvzx_harness_alloc.argtypes = [C.c_int, C.c_size_t]
    LIB.kvzx_harness_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    LIB.kvzx_harness_free.argtypes = [C.c_void_p]
    dev = []
    for f in frames:
        f = np.ascontiguousarray(f)
        d = LIB.kvzx_harness_alloc(0, f.nbytes)
        assert d and LIB.kvzx_harness_upload(d, f.ctypes.data, f.nbytes)
        dev.append(C.c_void_p(d))
    LIB.kvzx_harness_sync(0)
    return dev


def rate(dev, w, h, preset, on, passes=3):
    e = Encoder(w, h, options=opts(preset, on, 2) + (("input-hold", 1),))
    assert not e.rejected, e.rejected
    for d in dev:
        e.encode_device(d)
    t0 = time.perf_counter()
    k = 0
    for _ in range(passes):
        for d in dev:
            e.encode_device(d)
            k += 1
    for _ in range(3):
        e.encode_device(None)
    dt = time.perf_counter() - t0
    e.close()
    return k / dt


def trace(kind, preset, on, height="1080"):
    w, h = (1920, 1080) if int(height) == 1080 else (3840, 2160)
    frames = make_clip(kind, w, h)
    e = Encoder(w, h, options=opts(preset, int(on), 0))
    for f in frames:
        e.encode(f, want_recon=False)
    e.close()


def main():
    if "--trace" in sys.argv:
        i = sys.argv.index("--trace")
        return trace(*sys.argv[i + 1:i + 5])
    rate_only = "--rate-only" in sys.argv
    for w, h in (SIZES[:1] if "--quick" in sys.argv else SIZES):
        for kind in KINDS:
            frames = make_clip(kind, w, h)
            for preset in (() if rate_only else ("ultrafast", "veryfast")):
                ref = None
                for on in (0, 1):
                    bits, psnr, weighted = quality(frames, w, h, opts(preset, on, 0), on)
                    ref = ref or bits
                    emit({"what": "quality", "size": "%dx%d" % (w, h), "clip": kind, "preset": preset, "weightp": on, "bits_per_p": bits, "psnr_y": psnr,
                          "weighted_p_pictures": weighted, "of": len(frames) - 1, "bits_vs_off_percent": round(100.0 * (bits - ref) / ref, 2)})
            dev = upload(frames)
            for preset in ("ultrafast", "veryfast"):
                for rnd in range(2):
                    for on in (0, 1):
                        emit({"what": "rate", "size": "%dx%d" % (w, h), "clip": kind, "preset": preset, "round": rnd, "weightp": on, "fps": round(rate(dev, w, h, preset, on), 1)})
            for d in dev:
                LIB.kvzx_harness_free(d)


if __name__ == "__main__":
    main()
