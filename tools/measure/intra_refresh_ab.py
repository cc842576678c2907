"""intra-refresh ("uvgx intra refresh v1") on the GPU: what a call pays for healing losses without IDR pictures.  1080p (and 2160p with
--2160), presets ultrafast and veryfast (wpp, qp 32, me-range 16), the benchmark's synthetic clip, 128 pictures:

  period=64                       an IDR picture every 64 pictures, no refresh (what uvgComm sends today)
  period=0 intra-refresh=30       one IDR picture, then a band of intra units that crosses the picture in 30 P pictures
  period=0 intra-refresh=60       ... in 60

  quality  owf 0: mean bits per picture, the largest access unit over the mean access unit (what the option is for), luma PSNR
  rate     encoder pictures/s of the clip resident in device memory (kvzx_encoder_encode_device, input-hold, owf 2), one warm-up pass
  trace    `--trace PRESET CONFIG [HEIGHT]` (CONFIG 0 / 1 / 2 as listed above): encodes the clip once and nothing else -- the program for a kernel-trace run of its
           own, e.g.  rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure/intra_refresh_ab.py --trace ultrafast 1
           (the chain is k_me, k_intra_analyse<P>, k_inter_recon, k_intra_recon<P>: their times come from that run's kernel statistics)

usage: python tools/measure/intra_refresh_ab.py [out.txt] [--2160] [--pictures N]      (one JSON object per line, also appended to out.txt)"""
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import orc  # noqa: E402
from kvazzup_amd import _native  # noqa: E402
from kvazzup_amd.codec import Encoder  # noqa: E402

LIB = _native.load_library()
CONFIGS = ((("period", 64),), (("period", 0), ("intra-refresh", 30)), (("period", 0), ("intra-refresh", 60)))
ARGV = list(sys.argv[1:])
NF = 128
if "--pictures" in ARGV:
    i = ARGV.index("--pictures")
    NF = int(ARGV[i + 1])
    del ARGV[i:i + 2]
ARGS = [a for a in ARGV if not a.startswith("--")]
OUT = ARGS[0] if ARGS and "--trace" not in ARGV else None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def opts(preset, config, owf):
    return (("preset", preset), ("threads", 8), ("owf", owf), ("wpp", 1), ("qp", 32), ("me-range", 16)) + CONFIGS[config]


def name(config):
    return " ".join("%s=%s" % kv for kv in CONFIGS[config])


def quality(frames, w, h, preset, config):
    e = Encoder(w, h, options=opts(preset, config, 0))
    assert not e.rejected, e.rejected
    ny = w * h
    sizes, psnr = [], []
    for f in frames:
        au, rec = e.encode(f)
        sizes.append(len(au))
        mse = np.mean((rec[:ny].astype(np.float64) - f[:ny]) ** 2)
        psnr.append(10 * np.log10(255 ** 2 / max(mse, 1e-9)))
    e.close()
    mean = float(np.mean(sizes))
    return {"bits_per_picture": int(8 * mean), "largest_over_mean_au": round(max(sizes) / mean, 2), "largest_p_over_mean_au": round(max(sizes[1:]) / mean, 2), "psnr_y": round(float(np.mean(psnr)), 3)}


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


def rate(dev, w, h, preset, config):
    e = Encoder(w, h, options=opts(preset, config, 2) + (("input-hold", 1),))
    assert not e.rejected, e.rejected
    for d in dev:
        e.encode_device(d)
    t0 = time.perf_counter()
    for d in dev:
        e.encode_device(d)
    for _ in range(3):
        e.encode_device(None)
    dt = time.perf_counter() - t0
    e.close()
    return len(dev) / dt


def trace(preset, config, height="1080"):
    w, h = (1920, 1080) if int(height) == 1080 else (3840, 2160)
    e = Encoder(w, h, options=opts(preset, int(config), 0))
    for t in range(NF):
        e.encode(orc.synth_frame(0, 1234, w, h, t), want_recon=False)
    e.close()


def main():
    if "--trace" in ARGV:
        i = ARGV.index("--trace")
        return trace(*ARGV[i + 1:i + 4])
    for w, h in ((1920, 1080),) + (((3840, 2160),) if "--2160" in ARGV else ()):
        frames = [orc.synth_frame(0, 1234, w, h, t) for t in range(NF)]
        dev = upload(frames)
        for preset in ("ultrafast", "veryfast"):
            for config in range(len(CONFIGS)):
                d = {"size": "%dx%d" % (w, h), "pictures": NF, "preset": preset, "config": name(config)}
                d.update(quality(frames, w, h, preset, config))
                d["fps"] = [round(rate(dev, w, h, preset, config), 1) for _ in range(2)]
                emit(d)
        for d in dev:
            LIB.kvzx_harness_free(d)


if __name__ == "__main__":
    main()
