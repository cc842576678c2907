"""me-coarse ("uvgx coarse-to-fine search v1") on the GPU: what a coarse reach of 128 / 256 samples costs and buys against the search
of before (me-coarse 0), at 1080p and 2160p, on the benchmark clip and on a panning clip, presets ultrafast and veryfast (owf 2, wpp, QP 32, period 64).

  rate     encoder pictures/s of a clip resident in device memory (kvzx_encoder_encode_device, input-hold), one warm-up pass; the settings alternate
           (0, 128, 256, 0, 128, 256) inside this one command
  quality  owf 0: bits per P picture, luma PSNR of the reconstruction, and the share of 32x32 blocks whose reference-0 centre lies outside the zero window
           (an upper bound of the blocks that search a second window: blocks that terminate early use no centre)
  trace    `--trace SIZE CLIP PRESET REACH`: encodes the clip once and nothing else -- the program for a kernel-trace run of its own, e.g.
           rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure/me_coarse_ab.py --trace 1080p pan veryfast 128
           (times of k_luma_quarter, k_me_coarse and k_me come from that run's kernel statistics)

usage: python tools/measure/me_coarse_ab.py [out.txt] [--quick]      (one JSON object per line, also appended to out.txt; --quick: 1080p only)"""
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import orc  # noqa: E402
import pan_content  # noqa: E402
from kvazzup_amd.codec import Encoder  # noqa: E402

SIZES = {"1080p": (1920, 1080, 32), "2160p": (3840, 2160, 16)}
PRESETS = ("ultrafast", "veryfast")
REACH = (0, 128, 256)
PAN = (72, -40)
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = ARGS[0] if ARGS and "--trace" not in sys.argv else None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def opts(preset, reach, owf):
    return (("preset", preset), ("threads", 8), ("owf", owf), ("wpp", 1), ("qp", 32), ("period", 64), ("me-coarse", reach))


def make_clip(name, w, h, nf):
    if name == "bench":
        return [orc.synth_frame(0, 0x5EED0000, w, h, t) for t in range(nf)]
    return pan_content.clip(w, h, nf, *PAN)


def rate(w, h, dev, preset, reach, passes=3):
    """pictures/s over `passes` passes of the resident clip behind one warm-up pass (the clip restarts: every pass begins with a large change, the same for every setting)"""
    e = Encoder(w, h, options=opts(preset, reach, 2) + (("input-hold", 1),))
    assert not e.rejected, e.rejected
    for d in dev:
        e.encode_device(d.data_ptr())
    t0 = time.perf_counter()
    n = 0
    for _ in range(passes):
        for d in dev:
            e.encode_device(d.data_ptr())
            n += 1
    for _ in range(3):
        e.encode_device(None)
    dt = time.perf_counter() - t0
    e.close()
    return n / dt


def quality(w, h, frames, preset, reach):
    e = Encoder(w, h, options=opts(preset, reach, 0))
    assert not e.rejected, e.rejected
    ny = w * h
    bits, psnr, far = [], [], []
    rng = int(e.cfg.contents.me_range)
    for t, f in enumerate(frames):
        au, rec = e.encode(f)
        if t == 0:
            continue
        bits.append(8 * len(au))
        mse = np.mean((rec[:ny].astype(np.float64) - f[:ny]) ** 2)
        psnr.append(10 * np.log10(255 ** 2 / max(mse, 1e-9)))
        if reach:
            c = np.abs(e.debug_all()["me_coarse"][0].astype(np.int32))
            far.append(float(((c[..., 0] > rng - 4) | (c[..., 1] > rng - 4)).mean()))
    e.close()
    return {"bits_per_p": int(np.mean(bits)), "psnr_y": round(float(np.mean(psnr)), 3), "far_centre_share": round(float(np.mean(far)), 4) if far else 0.0}


def trace(size, clip, preset, reach):
    w, h, nf = SIZES[size]
    frames = make_clip(clip, w, h, min(nf, 12))
    e = Encoder(w, h, options=opts(preset, int(reach), 0))
    for f in frames:
        e.encode(f, want_recon=False)
    e.close()


def main():
    if "--trace" in sys.argv:
        i = sys.argv.index("--trace")
        return trace(*sys.argv[i + 1:i + 5])
    import torch
    sizes = ("1080p",) if "--quick" in sys.argv else tuple(SIZES)
    for size in sizes:
        w, h, nf = SIZES[size]
        for clip in ("bench", "pan"):
            frames = make_clip(clip, w, h, nf)
            dev = [torch.from_numpy(f).cuda() for f in frames]
            torch.cuda.synchronize()
            for preset in PRESETS:
                for rnd in range(2):
                    for reach in REACH:
                        emit({"what": "rate", "size": size, "clip": clip, "preset": preset, "round": rnd, "me_coarse": reach, "fps": round(rate(w, h, dev, preset, reach), 1)})
                for reach in REACH:
                    emit(dict({"what": "quality", "size": size, "clip": clip, "preset": preset, "me_coarse": reach}, **quality(w, h, frames[:8], preset, reach)))
            del dev


if __name__ == "__main__":
    main()
