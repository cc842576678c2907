"""What one open encoder holds of the device's memory, and how long opening and closing one takes.  Per configuration: free device memory
(torch.cuda.mem_get_info) before the open, the drop across the open (after three pictures, so that the host-picture ring and the reconstruction sink's event
exist), and free memory after the close against the start.  The list is gone through twice: the first pass also loads each configuration's kernels and fills the
stream pool, which stay with the process; the second pass shows what an encoder itself leaves behind.  Then `--reopen N`: N times create + destroy of the 1080p default encoder, ms each.
Which library: KVAZZUP_AMD_LIBRARY (kvazzup_amd/_native.py), so that two builds can be run alternately from one script.
    python tools/measure/enc_footprint.py [--reopen 10] [--label NAME]"""
import argparse
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
import orc  # noqa: E402
from kvazzup_amd.codec import Encoder  # noqa: E402

W, H = 1920, 1080
RC = (("bitrate", 1000000), ("rc-algorithm", "lambda"))
CONFIGS = [
    ("bench-1080p", (("owf", 6), ("me-range", 16), ("input-hold", 1)), None),                                   # bench.py's headline encoder
    ("uvgcomm-defaults", (("preset", "veryfast"), ("owf", 2)) + RC, {"target_bitrate": 1000000}),               # SAO + per-CTU QP + rate control, the side chain with them
    ("all-intra", (("period", 1), ("owf", 6)), None),
    ("lp-refs4-tmvp-coarse-weightp-scenecut", (("lp-refs", 4), ("tmvp", 1), ("me-coarse", 128), ("weightp", 1), ("scenecut", 40), ("owf", 2)), None),
    ("entropy-gpu", (("gpu-entropy", 1), ("owf", 6)), None),
]


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reopen", type=int, default=0)
    ap.add_argument("--label", default=os.environ.get("KVAZZUP_AMD_LIBRARY", "in-tree library"))
    a = ap.parse_args()
    frames = [orc.synth_frame(0, 0x5EED0001, W, H, t) for t in range(3)]
    torch.cuda.init()
    e = Encoder(W, H, options=(("owf", 0),)); e.encode(frames[0]); e.close()       # the runtime's own first allocations (code objects, streams) are not an encoder's
    for npass, (name, opts, fields) in [(p, c) for p in (1, 2) for c in CONFIGS]:
        f0 = free_bytes()
        e = Encoder(W, H, options=opts, fields=fields)
        assert not e.rejected, e.rejected
        for f in frames:
            e.encode(f)
        f1 = free_bytes()
        while e.encode(None)[0] is not None:
            pass
        e.close()
        f2 = free_bytes()
        print("%s | pass %d %s | free before %d | held while open %d bytes (%.1f MiB) | free after close - before %+d" % (a.label, npass, name, f0, f0 - f1, (f0 - f1) / 2 ** 20, f2 - f0), flush=True)
    if a.reopen:
        ms = []
        for _ in range(a.reopen):
            t0 = time.perf_counter()
            e = Encoder(W, H, options=(("preset", "veryfast"), ("owf", 2)) + RC, fields={"target_bitrate": 1000000})
            e.close()
            ms.append((time.perf_counter() - t0) * 1e3)
        print("%s | create + destroy x%d (uvgcomm-defaults, 1080p) ms: %s | median %.1f" % (a.label, a.reopen, " ".join("%.1f" % v for v in ms), sorted(ms)[len(ms) // 2]), flush=True)


if __name__ == "__main__":
    main()
