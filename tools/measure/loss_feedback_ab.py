"""loss-feedback ("uvgx loss feedback v1") on the GPU: what healing a reported loss in one picture costs and buys.  1080p, presets
ultrafast and veryfast (slices=wpp, qp 32, me-range 16), the benchmark's synthetic clip, 64 pictures, period 0.

  heal     a loss at picture 20 -- one CTU row's segment (with the dependent segments behind it: what a receiver then reports), and the last four rows -- reported
           3 pictures later: bytes and luma PSNR of the heal picture (picture 23), of the same picture forced to an IDR picture (period=23), and of the same
           picture of a stream that is never told; the heal picture's damaged cells and forced quarters; and the stream's bytes over the 64 pictures against
           intra-refresh=30 over the same pictures.  The receiver is exact from the heal picture on (tests/test_gpu_loss_feedback.py holds that); with
           intra-refresh=30 it is exact when the pass that began after the loss is complete, at most 59 pictures later
  rate     encoder pictures/s of the clip resident in device memory (kvzx_encoder_encode_device, input-hold, owf 2), option off / on without a report / on with
           a report every 16 pictures
  times    owf 0 with profiling on: the kernel times per picture kind (the record writer rides behind every chain; the map kernels run on heal pictures only and
           are read from a kernel-trace run of `--trace PRESET`, which encodes the heal clip once and nothing else)

With `--anchor K` the same case for fb-anchor=K ("uvgx loss feedback v2") and nothing else: the v2 heal picture and its run beside v1's,
the never-told and the IDR one; the heal picture's kernel times beside v1's; pictures/s with the option on and no report against loss-feedback alone; and the
memory the kept pictures take.

usage: python tools/measure/loss_feedback_ab.py [out.txt] [--pictures N] [--anchor K]      (one JSON object per line, also appended to out.txt)"""
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import orc  # noqa: E402
from kvazzup_amd.codec import Encoder  # noqa: E402

ARGV = list(sys.argv[1:])
NF = 64
if "--pictures" in ARGV:
    i = ARGV.index("--pictures")
    NF = int(ARGV[i + 1])
    del ARGV[i:i + 2]
ANCHOR = 0
if "--anchor" in ARGV:
    i = ARGV.index("--anchor")
    ANCHOR = int(ARGV[i + 1])
    del ARGV[i:i + 2]
ARGS = [a for a in ARGV if not a.startswith("--")]
OUT = ARGS[0] if ARGS and "--trace" not in ARGV else None
W, H = 1920, 1080
WC, HC = (W + 63) // 64, (H + 63) // 64
LOST, HEAL, HIST = 20, 23, 8


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def opts(preset, owf, extra):
    return (("preset", preset), ("threads", 8), ("owf", owf), ("wpp", 1), ("slices", "wpp"), ("qp", 32), ("me-range", 16), ("period", 0)) + tuple(extra)


def psnr(a, b):
    mse = np.mean((a[:W * H].astype(np.float64) - b[:W * H].astype(np.float64)) ** 2)
    return round(float(10 * np.log10(255.0 ** 2 / mse)), 2) if mse else 99.0


def encode(frames, preset, extra, report=None):
    """[(bytes, luma PSNR)] per picture, the heal picture's record (fb-anchor: and its anchor record behind it)"""
    e = Encoder(W, H, options=opts(preset, 0, extra))
    assert not e.rejected, e.rejected
    out, fb = [], None
    for t, f in enumerate(frames):
        if report and t == HEAL:
            assert e.report_damage(*report) == 1
        au, rec = e.encode(f)
        out.append((len(au), psnr(rec, f)))
        if report and t == HEAL:
            fb = [int(v) for v in e.debug("fb", np.int32, (4,))]
            if dict(extra).get("fb-anchor"):
                fb += [int(v) for v in e.debug("fb_anchor", np.int32, (4,))]
    e.close()
    return out, fb


def run_psnr(pics):
    return round(sum(p for _, p in pics) / len(pics), 2)


def anchor_heal(frames, preset):
    """fb-anchor: the one-CTU-row case, v2 against v1, never told and IDR"""
    report = (LOST, 8 * WC, (HC - 8) * WC)
    plain, _ = encode(frames, preset, ())
    idr, _ = encode(frames, preset, (("period", HEAL),))
    v1, fb1 = encode(frames, preset, (("loss-feedback", HIST),), report)
    v2, fb2 = encode(frames, preset, (("loss-feedback", HIST), ("fb-anchor", ANCHOR)), report)
    row = lambda pics: {"heal_picture_bytes": pics[HEAL][0], "heal_picture_psnr_y": pics[HEAL][1], "run_bytes": sum(b for b, _ in pics), "run_psnr_y": run_psnr(pics)}
    emit({"measure": "anchor heal", "preset": preset, "fb-anchor": ANCHOR, "report": list(report), "v2": row(v2), "v1": row(v1), "never_told": row(plain), "idr_at_heal": row(idr),
          "v2_record": dict(zip(("heal", "reports", "cells", "forced_quarters", "v2", "anchor", "da", "quarters_on_the_anchor"), fb2)), "v1_forced_quarters": fb1[3], "quarters": (WC * 4) * (HC * 4)})


def anchor_times(frames, preset):
    for name, extra in (("v1", (("loss-feedback", HIST),)), ("v2", (("loss-feedback", HIST), ("fb-anchor", ANCHOR)))):
        e = Encoder(W, H, options=opts(preset, 0, extra))
        e.set_profiling(1)
        for t, f in enumerate(frames[:HEAL + 1]):
            if t == HEAL:
                assert e.report_damage(LOST, 8 * WC, (HC - 8) * WC) == 1
                e.kernel_times(reset=True)
            e.encode(f, want_recon=False)
        emit({"measure": "anchor times", "preset": preset, "picture": "heal, " + name, "ms": {k: round(v[0], 4) for k, v in e.kernel_times(reset=True).items() if v[1]}})
        e.close()


def anchor_rate(dev, preset):
    for name, extra in (("loss-feedback alone", (("loss-feedback", HIST),)), ("fb-anchor=%d, no report" % ANCHOR, (("loss-feedback", HIST), ("fb-anchor", ANCHOR)))):
        e = Encoder(W, H, options=opts(preset, 2, (("input-hold", 1),) + extra))
        assert not e.rejected, e.rejected
        best = 0.0
        for rep in range(4):                             # (the first pass warms up)
            t0 = time.perf_counter()
            for d in dev:
                e.encode_device(d)
            for _ in range(3):
                e.encode_device(None)
            if rep:
                best = max(best, len(dev) / (time.perf_counter() - t0))
        e.close()
        emit({"measure": "anchor rate", "preset": preset, "config": name, "pictures_per_s": round(best, 1)})


def heal(frames, preset):
    plain, _ = encode(frames, preset, ())
    idr, _ = encode(frames, preset, (("period", HEAL),))
    ir, _ = encode(frames, preset, (("intra-refresh", 30),))
    for what, report in (("one CTU row and the segments behind it", (LOST, 8 * WC, (HC - 8) * WC)), ("the last four rows", (LOST, (HC - 4) * WC, 4 * WC))):
        on, fb = encode(frames, preset, (("loss-feedback", HIST),), report)
        emit({"measure": "heal", "preset": preset, "lost": what, "report": list(report), "heal_picture": {"bytes": on[HEAL][0], "psnr_y": on[HEAL][1]},
              "same_picture_untold": {"bytes": plain[HEAL][0], "psnr_y": plain[HEAL][1]}, "same_picture_idr": {"bytes": idr[HEAL][0], "psnr_y": idr[HEAL][1]},
              "damaged_cells": fb[2], "cells": (WC * 8) * (HC * 8), "forced_quarters": fb[3], "quarters": (WC * 4) * (HC * 4),
              "stream_bytes": {"untold": sum(b for b, _ in plain), "healed": sum(b for b, _ in on), "idr_at_heal": sum(b for b, _ in idr), "intra-refresh=30": sum(b for b, _ in ir)},
              "pictures_until_exact": {"loss-feedback": HEAL - LOST, "intra-refresh=30": "30 .. 59 (the pass that begins after the loss)"}})


def upload(frames):
    """the clip into device memory through the library's own helpers"""
    import ctypes as C
    from kvazzup_amd import _native
    lib = _native.load_library()
    lib.kvzx_harness_alloc.restype = C.c_void_p
    lib.kvzx_harness_alloc.argtypes = [C.c_int, C.c_size_t]
    lib.kvzx_harness_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    dev = []
    for f in frames:
        f = np.ascontiguousarray(f)
        d = lib.kvzx_harness_alloc(0, f.nbytes)
        assert d and lib.kvzx_harness_upload(d, f.ctypes.data, f.nbytes)
        dev.append(C.c_void_p(d))
    return dev


def rate(dev, preset):
    for name, extra, every in (("off", (), 0), ("on, no report", (("loss-feedback", HIST),), 0), ("on, a report every 16 pictures", (("loss-feedback", HIST),), 16)):
        e = Encoder(W, H, options=opts(preset, 2, (("input-hold", 1),) + extra))
        assert not e.rejected, e.rejected
        best = 0.0
        for rep in range(4):                             # (the first pass warms up)
            t0 = time.perf_counter()
            for t, d in enumerate(dev):
                if every and t % every == every - 1:
                    assert e.report_damage(max(rep * len(dev) + t - 3, 0), 8 * WC, WC) == 1
                e.encode_device(d)
            for _ in range(3):
                e.encode_device(None)
            if rep:
                best = max(best, len(dev) / (time.perf_counter() - t0))
        e.close()
        emit({"measure": "rate", "preset": preset, "config": name, "pictures_per_s": round(best, 1)})


def times(frames, preset):
    e = Encoder(W, H, options=opts(preset, 0, (("loss-feedback", HIST),)))
    e.set_profiling(1)
    for t, f in enumerate(frames[:32]):
        if t == HEAL:
            assert e.report_damage(LOST, 8 * WC, WC) == 1
            e.kernel_times(reset=True)
        e.encode(f, want_recon=False)
        if t == HEAL:
            emit({"measure": "times", "preset": preset, "picture": "heal", "ms": {k: round(v[0], 4) for k, v in e.kernel_times(reset=True).items() if v[1]}})
    k = e.kernel_times(reset=True)
    emit({"measure": "times", "preset": preset, "picture": "P pictures behind it, mean", "ms": {n: round(v[0] / v[1], 4) for n, v in k.items() if v[1]}})
    e.close()


def main():
    frames = [orc.synth_frame(0, 0x5EED0000, W, H, t) for t in range(NF)]
    if "--trace" in ARGV:
        encode(frames[:32], ARGV[ARGV.index("--trace") + 1], (("loss-feedback", HIST),), (LOST, 8 * WC, WC))
        return
    if ANCHOR:
        cw, ch = WC * 64, HC * 64
        emit({"measure": "anchor memory", "fb-anchor": ANCHOR, "kept_reconstructions_bytes": (ANCHOR - 1) * cw * ch * 3 // 2, "cu_ref_bytes": 8 * (cw // 8) * (ch // 8)})
        dev = upload(frames)
        for preset in ("ultrafast", "veryfast"):
            anchor_heal(frames, preset)
            anchor_times(frames, preset)
            anchor_rate(dev, preset)
        return
    dev = upload(frames)
    for preset in ("ultrafast", "veryfast"):
        heal(frames, preset)
        times(frames, preset)
        rate(dev, preset)


if __name__ == "__main__":
    main()
