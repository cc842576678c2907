"""lp-refs ("uvgx multi-reference v1") on the GPU: what n = 2..4 references cost against one, at 1080p and 2160p, presets ultrafast and veryfast with uvgComm's
settings (kvazaarfilter.cpp: owf 2, wpp, QP 32, period 64, gop lp-g4d3t1 -- which has no effect -- and lp-refs as the custom parameter).

  rate     encode + decode frames/s of a resident clip (pictures generated up front, host input, the HIP decoder behind the encoder in the same loop);
           base (lp-refs 0) and change runs alternate, two rounds
  kernels  owf 0, profiling on: encoder kernel times per P picture (k_me is the n-reference search) and the decoder's kernel time per picture
  quality  bits per P picture and luma PSNR of the reconstruction, computed on the host

usage: python tools/measure/lp_refs_rate.py [out.txt]      (one JSON object per line, also appended to out.txt)"""
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import orc  # noqa: E402
from kvazzup_amd.codec import Decoder, Encoder  # noqa: E402

SIZES = ((1920, 1080, 48), (3840, 2160, 24))
PRESETS = ("ultrafast", "veryfast")
REFS = (0, 2, 3, 4)
OUT = sys.argv[1] if len(sys.argv) > 1 else None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def opts(preset, n, owf):
    return (("preset", preset), ("threads", 8), ("owf", owf), ("wpp", 1), ("qp", 32), ("period", 64), ("lp-refs", n))


def rate(w, h, frames, preset, n):
    e, d = Encoder(w, h, options=opts(preset, n, 2)), Decoder()
    e.encode(frames[0], want_recon=False)                    # (warm-up: first picture, parameter sets)
    t0 = time.perf_counter()
    done = 0
    for f in frames[1:] + [None] * 3:
        au, _ = e.encode(f, want_recon=False)
        if au:
            d.decode_au(au, done)
            done += 1
    dt = time.perf_counter() - t0
    e.close(); d.close()
    return done / dt


def kernels_and_quality(w, h, frames, preset, n):
    e, d = Encoder(w, h, options=opts(preset, n, 0)), Decoder()
    e.set_profiling(True); d.set_profiling(True)
    bits, psnr = [], []
    ny = w * h
    for t, f in enumerate(frames):
        au, rec = e.encode(f)
        d.decode_au(au, t)
        if t == 0:
            e.kernel_times(); d.kernel_times()               # (the IDR picture left out)
            continue
        bits.append(8 * len(au))
        mse = np.mean((rec[:ny].astype(np.float64) - f[:ny]) ** 2)
        psnr.append(10 * np.log10(255 ** 2 / max(mse, 1e-9)))
    ke, kd = e.kernel_times(), d.kernel_times()
    e.close(); d.close()
    np_ = len(frames) - 1
    enc = {k: round(v[0] / np_ * 1e3, 1) for k, v in ke.items() if v[1]}
    dec_total = round(sum(v[0] for v in kd.values()) / np_ * 1e3, 1)
    return {"enc_us_per_picture": enc, "dec_kernel_us_per_picture": dec_total, "bits_per_p": int(np.mean(bits)), "psnr_y": round(float(np.mean(psnr)), 3)}


def main():
    for w, h, nf in SIZES:
        frames = [orc.synth_frame(0, 0x5EED0001, w, h, t) for t in range(nf)]
        for preset in PRESETS:
            for rnd in range(2):
                for n in REFS[1:]:
                    for m in (0, n):                         # base, change, base, change ...
                        emit({"what": "rate", "size": "%dx%d" % (w, h), "preset": preset, "round": rnd, "lp_refs": m, "fps": round(rate(w, h, frames, preset, m), 1)})
            for n in REFS:
                emit(dict({"what": "kernels", "size": "%dx%d" % (w, h), "preset": preset, "lp_refs": n}, **kernels_and_quality(w, h, frames[:12], preset, n)))


if __name__ == "__main__":
    main()
