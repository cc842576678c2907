#!/usr/bin/env python3
"""tools/measure/standin_time.py: what filling one stand-in costs on the GPU -- concealment v2's device-to-device copy against v3's k_dec_standin
(csrc/conceal_kernels.hip) -- at 1080p: a pan coded by the HIP encoder, access units lost, each fill between two HIP events (set_profiling; debug_copy
"standin_ms").  Two access units lost per run, so two fills: the first includes whatever the first launch of the kernel costs the host (its code object is
loaded then), the second does not.  Single measurements, of a path that runs once per lost picture.  GPU box:
    python tools/measure/standin_time.py >> profiles/concealment_v3.txt"""
import ctypes as C
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
import numpy as np  # noqa: E402

from kvazzup_amd import synth  # noqa: E402
from kvazzup_amd.codec import Decoder, Encoder  # noqa: E402

w, h, n, lost = 1920, 1080, 9, (3, 6)
big = synth.frame(synth.MOVING, 0x5EED0000, 2 * w, 2 * 1088, 0)
Y, U, V = big[:4 * w * 1088].reshape(2 * 1088, 2 * w), big[4 * w * 1088:5 * w * 1088].reshape(1088, w), big[5 * w * 1088:].reshape(1088, w)
e = Encoder(w, h, options=(("qp", 30), ("me-range", 16)))
aus = []
for t in range(n):
    x0, y0 = w // 2 - 6 * t, 544 - 2 * t                    # a pan of (6, 2) samples a picture
    f = np.concatenate([Y[y0:y0 + h, x0:x0 + w].ravel(), U[y0 // 2:y0 // 2 + h // 2, x0 // 2:x0 // 2 + w // 2].ravel(), V[y0 // 2:y0 // 2 + h // 2, x0 // 2:x0 // 2 + w // 2].ravel()])
    aus.append(e.encode(f.astype(np.uint8))[0])
e.close()
print("# fill of a stand-in at %dx%d, HIP events around it: the first and the second of a decoder (tools/measure/standin_time.py); single measurements" % (w, h))
for mode in (2, 3):
    d = Decoder(concealment=mode)
    d.set_profiling(1)
    took = []
    for t, au in enumerate(aus):
        if t in lost:
            continue
        d.decode_au(au, t)
        if t - 1 in lost:
            ms = C.c_float(-1)
            took.append(ms.value * 1000.0 if d.lib.kvzx_decoder_debug_copy(d.h, b"standin_ms", C.byref(ms), 4) else float("nan"))
    moved = ""
    if mode == 3:
        mv = d.standin(w, h)[1]
        moved = ", %d of %d blocks moved" % (int((mv != 0).any(axis=2).sum()), mv.shape[0] * mv.shape[1])
    print("concealment %d: %s %s us%s" % (mode, "hipMemcpy device to device (v2's copy)" if mode == 2 else "k_dec_standin", " / ".join("%.1f" % v for v in took), moved))
    d.close()
