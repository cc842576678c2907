"""lp-gop ("uvgx low-delay GOP v1") on the GPU: what gop=lp-g4d3t1 with lp-gop=1 costs and buys against the same encoder without it,
at 1080p, presets ultrafast and veryfast (wpp, period 64), on the benchmark clip, a panning clip and a clip with an occluder passing over a still textured
background (tests/occluder_content.py).  Pairs: {lp-refs=3} against {lp-refs=3, gop=lp-g4d3t1, lp-gop=1}, and the same with lp-refs=1 (QP layers alone).

  quality  owf 0, qp 27 / 32 / 37 / 42: bits per P picture and luma PSNR over the P pictures.  The option moves QP, so the pair is compared as a BD-rate over
           the four points (cubic fit of log rate over PSNR, integrated over the PSNR range both curves cover): negative = fewer bits at equal PSNR
  rc       uvgComm's default mode (veryfast, 1 Mbit/s, rc-algorithm lambda): bits per picture and PSNR of the pair at the same target bitrate
  rate     encoder pictures/s of a clip resident in device memory (kvzx_encoder_encode_device, input-hold, owf 2), one warm-up pass; the settings alternate
           inside this one command
  trace    `--trace CLIP PRESET N ON`: encodes the clip once and nothing else -- the program for a kernel-trace run of its own, e.g.
           rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure/lp_gop_ab.py --trace occluder veryfast 3 1
           (the time of k_inter_signal with the table comes from that run's kernel statistics)

usage: python tools/measure/lp_gop_ab.py [out.txt] [--quick]      (one JSON object per line, also appended to out.txt; --quick: veryfast, lp-refs 3, no rate; --rate-only: the rate part alone)"""
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import occluder_content  # noqa: E402
import orc  # noqa: E402
import pan_content  # noqa: E402
from kvazzup_amd import _native  # noqa: E402
from kvazzup_amd.codec import Encoder  # noqa: E402

LIB = _native.load_library()

W, H, NF = 1920, 1080, 33
QPS = (27, 32, 37, 42)
GOP = "lp-g4d3t1"
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = ARGS[0] if ARGS and "--trace" not in sys.argv else None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def opts(preset, n, on, owf, qp=32):
    return (("preset", preset), ("threads", 8), ("owf", owf), ("wpp", 1), ("qp", qp), ("period", 64), ("lp-refs", n), ("gop", GOP), ("lp-gop", on))


def make_clip(name, nf=NF):
    if name == "bench":
        return [orc.synth_frame(0, 0x5EED0000, W, H, t) for t in range(nf)]
    if name == "pan":
        return pan_content.clip(W, H, nf, 12, -6)
    return occluder_content.passing_clip(W, H, nf)


def quality(frames, options, fields=None):
    e = Encoder(W, H, options=options, fields=fields)
    assert not e.rejected, e.rejected
    ny = W * H
    bits, psnr = [], []
    for t, f in enumerate(frames):
        au, rec = e.encode(f)
        if t == 0:
            continue
        bits.append(8 * len(au))
        mse = np.mean((rec[:ny].astype(np.float64) - f[:ny]) ** 2)
        psnr.append(10 * np.log10(255 ** 2 / max(mse, 1e-9)))
    e.close()
    return int(np.mean(bits)), round(float(np.mean(psnr)), 3)


def bd_rate(a, b):
    """Bjontegaard delta rate of curve b against curve a, per cent; each a list of (bits, psnr)"""
    (ra, pa), (rb, pb) = [(np.log([r for r, _ in c]), np.array([p for _, p in c])) for c in (a, b)]
    fa, fb = np.polyfit(pa, ra, 3), np.polyfit(pb, rb, 3)
    lo, hi = max(pa.min(), pb.min()), min(pa.max(), pb.max())
    if hi <= lo:
        return None
    ia, ib = np.polyint(fa), np.polyint(fb)
    avg = ((np.polyval(ib, hi) - np.polyval(ib, lo)) - (np.polyval(ia, hi) - np.polyval(ia, lo))) / (hi - lo)
    return round(float((np.exp(avg) - 1) * 100), 2)


def upload(frames):
    """the clip into device memory through the library's own helpers (no tensor library in the process: one that ships its own HIP runtime would replace the system's)"""
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


def rate(dev, preset, n, on, passes=2):
    e = Encoder(W, H, options=opts(preset, n, on, 2) + (("input-hold", 1),))
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


def trace(clip, preset, n, on):
    frames = make_clip(clip, 13)
    e = Encoder(W, H, options=opts(preset, int(n), int(on), 0) + (("tmvp", 1),))
    for f in frames:
        e.encode(f, want_recon=False)
    e.close()


def main():
    if "--trace" in sys.argv:
        i = sys.argv.index("--trace")
        return trace(*sys.argv[i + 1:i + 5])
    quick = "--quick" in sys.argv
    rate_only = "--rate-only" in sys.argv
    presets = ("veryfast",) if quick else ("ultrafast", "veryfast")
    depths = (3,) if quick else (3, 1)
    for clip in ("bench", "pan", "occluder"):
        frames = make_clip(clip)
        for preset in (() if rate_only else presets):
            for n in depths:
                curves = {0: [], 1: []}
                for qp in QPS:
                    for on in (0, 1):
                        bits, psnr = quality(frames, opts(preset, n, on, 0, qp))
                        curves[on].append((bits, psnr))
                        emit({"what": "quality", "clip": clip, "preset": preset, "lp_refs": n, "lp_gop": on, "qp": qp, "bits_per_p": bits, "psnr_y": psnr})
                emit({"what": "bd_rate", "clip": clip, "preset": preset, "lp_refs": n, "bd_rate_percent": bd_rate(curves[0], curves[1])})
        for on in (() if rate_only else (0, 1)):
            o = opts("veryfast", 3, on, 0) + (("bitrate", 1000000), ("rc-algorithm", "lambda"))
            bits, psnr = quality(frames, o, fields={"target_bitrate": 1000000})
            emit({"what": "rc", "clip": clip, "preset": "veryfast", "bitrate": 1000000, "lp_refs": 3, "lp_gop": on, "bits_per_p": bits, "psnr_y": psnr})
        if not quick:
            dev = upload(frames)
            for preset in presets:
                for rnd in range(2):
                    for n in depths:
                        for on in (0, 1):
                            emit({"what": "rate", "clip": clip, "preset": preset, "round": rnd, "lp_refs": n, "lp_gop": on, "fps": round(rate(dev, preset, n, on), 1)})
            for d in dev:
                LIB.kvzx_harness_free(d)


if __name__ == "__main__":
    main()
