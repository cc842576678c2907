"""tmvp (temporal motion vector prediction) on the GPU: what it saves in bits, and what it costs in k_inter_signal.

  bits     access-unit bits of the P pictures with tmvp=0 and tmvp=1 on the same clip, and whether the reconstructions are equal (they are at a constant
           QP: tmvp changes the signalling only).  Configurations: the benchmark's clip and settings (uvgx-synth-v1, preset ultrafast, QP 32, period 64) at
           1080p and 2160p; the same with lp-refs 3; uvgComm's default mode (preset veryfast, 1 Mbit/s), where rate control turns the saving into a
           lower mean QP; and a pan of the same texture (every block moves like its collocated block)
  encode   encode a 1080p clip with the given tmvp value and nothing else -- the program to run under `rocprofv3 --kernel-trace --stats -- ...` once per value

usage: python tools/measure/tmvp_bits.py bits [out.txt]       (one JSON object per line, also appended to out.txt)
       python tools/measure/tmvp_bits.py encode <0|1> [pictures]"""
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import orc  # noqa: E402
from kvazzup_amd.codec import Encoder  # noqa: E402

SEED = 0x5EED0000
BASE = (("preset", "ultrafast"), ("threads", 8), ("owf", 2), ("wpp", 1), ("qp", 32), ("period", 64))
CONFIGS = [
    ("bench", BASE, 0),
    ("bench+lp-refs3", BASE + (("lp-refs", 3),), 0),
    ("default_mode", (("preset", "veryfast"), ("threads", 8), ("owf", 2), ("wpp", 1), ("period", 64)), 1000000),
]


def clip(w, h, n, pan=False):
    if not pan:
        return [orc.synth_frame(0, SEED, w, h, t) for t in range(n)]
    big = orc.synth_frame(0, SEED, 2 * w, 2 * h, 0)
    Y, U, V = big[:4 * w * h].reshape(2 * h, 2 * w), big[4 * w * h:5 * w * h].reshape(h, w), big[5 * w * h:].reshape(h, w)
    out = []
    for t in range(n):
        x0, y0 = w // 2 - 4 * t, h // 2 - 2 * t
        out.append(np.concatenate([Y[y0:y0 + h, x0:x0 + w].ravel(), U[y0 // 2:y0 // 2 + h // 2, x0 // 2:x0 // 2 + w // 2].ravel(),
                                   V[y0 // 2:y0 // 2 + h // 2, x0 // 2:x0 // 2 + w // 2].ravel()]).astype(np.uint8))
    return out


def run(w, h, frames, opts, bitrate, tmvp):
    fields = {"target_bitrate": bitrate} if bitrate else None
    e = Encoder(w, h, options=opts + (("tmvp", tmvp),) + ((("bitrate", bitrate),) if bitrate else ()), fields=fields)
    assert not e.rejected, e.rejected
    owf = int(dict(opts).get("owf", 0))
    bits, qps, recs = [], [], []
    for t in range(len(frames) + owf + 1):
        au, rec = e.encode(frames[t] if t < len(frames) else None)
        if au:
            bits.append(8 * len(au)); recs.append(rec); qps.append(int(e.info["qp"]))
    e.close()
    return bits, recs, qps


def bits(out):
    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")
    for w, h, n in ((1920, 1080, 64), (3840, 2160, 32)):
        frames = clip(w, h, n)
        for name, opts, br in CONFIGS:
            if br and w > 1920:
                continue
            (b0, r0, q0), (b1, r1, q1) = run(w, h, frames, opts, br, 0), run(w, h, frames, opts, br, 1)
            same = all(np.array_equal(a, b) for a, b in zip(r0, r1))
            ny = w * h
            psnr = lambda recs: round(float(np.mean([10 * np.log10(255 ** 2 / max(np.mean((r[:ny].astype(np.float64) - f[:ny]) ** 2), 1e-9)) for r, f in zip(recs[1:], frames[1:])])), 3)
            p0, p1 = sum(b0[1:]), sum(b1[1:])
            emit({"what": name, "size": "%dx%d" % (w, h), "pictures": n, "p_bits_tmvp0": p0, "p_bits_tmvp1": p1, "saving_pct": round(100.0 * (p0 - p1) / p0, 2),
                  "same_reconstruction": same, "psnr_y_tmvp0": psnr(r0), "psnr_y_tmvp1": psnr(r1),
                  "mean_qp_tmvp0": round(float(np.mean(q0[1:])), 2), "mean_qp_tmvp1": round(float(np.mean(q1[1:])), 2)})
    w, h, n = 1920, 1080, 32
    frames = clip(w, h, n, pan=True)
    (b0, r0, _), (b1, r1, _) = run(w, h, frames, BASE, 0, 0), run(w, h, frames, BASE, 0, 1)
    emit({"what": "pan", "size": "%dx%d" % (w, h), "pictures": n, "p_bits_tmvp0": sum(b0[1:]), "p_bits_tmvp1": sum(b1[1:]),
          "saving_pct": round(100.0 * (sum(b0[1:]) - sum(b1[1:])) / sum(b0[1:]), 2), "same_reconstruction": all(np.array_equal(a, b) for a, b in zip(r0, r1))})


def encode(tmvp, n):
    w, h = 1920, 1080
    frames = clip(w, h, n)
    run(w, h, frames, BASE, 0, tmvp)


if __name__ == "__main__":
    if sys.argv[1] == "bits":
        bits(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        encode(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 64)
