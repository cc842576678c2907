"""input-format on the GPU: what converting RGB32 / YUYV pictures in the encoder's input stage saves the host, and what the fused kernel costs.
1080p, preset ultrafast (wpp, qp 32, me-range 16, period 64, threads 8):

  host     process CPU time per picture and pictures/s at owf 2, N pictures of the benchmark's clip as RGB32 (kvazzup_amd.synth.to_rgb32), three paths:
             a  the reference's arithmetic on the CPU (its own object code from oracle/_ref where that has been built, else the numpy statement), then the
                I420 picture through encoder_encode
             b  kvzx_rgb32_to_yuv420 (upload, convert, download), then the I420 picture through encoder_encode -- the device route of before
             c  kvzx_encoder_encode_packed_host on an input-format encoder
           and, for the price of 4 (2) bytes a sample on the copy engine instead of 1.5:  i420 = pre-converted I420 pictures through encoder_encode,  yuyv = path c
  kernel   k_input_rgb32 against k_rgb32_to_i420 + k_pad_input on the same picture, resident in device memory, owf 0, five alternated rounds: the encoders'
           kernel_times (the input stage's id) of a packed and of an i420 encoder, and the free-standing converter between event pairs of the same kind
           (kvzx_rgb32_to_yuv420_device_timed); achieved GB/s of the fused kernels (4 w h or 2 w h read + 1.5 cw ch written) against the HBM peak.
           PASS MARK: the fused kernel's median does not exceed the median of the pair's sums

usage: python tools/measure/input_format_ab.py [out.txt] [--pictures N]      (one JSON object per line, also appended to out.txt)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import input_model  # noqa: E402
import orc  # noqa: E402
import refcolor  # noqa: E402
from kvazzup_amd import _native, synth  # noqa: E402
from kvazzup_amd.codec import Encoder  # noqa: E402

LIB = _native.load_library()
W, H, SEED, CLIP = 1920, 1080, 1234, 16
ARGV = list(sys.argv[1:])
NF = 200
if "--pictures" in ARGV:
    i = ARGV.index("--pictures")
    NF = int(ARGV[i + 1])
    del ARGV[i:i + 2]
OUT = ARGV[0] if ARGV else None
LIB.kvzx_harness_alloc.restype = C.c_void_p
LIB.kvzx_harness_alloc.argtypes = [C.c_int, C.c_size_t]
LIB.kvzx_harness_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
LIB.kvzx_harness_free.argtypes = [C.c_void_p]
LIB.kvzx_harness_hbm_peak_gbs.restype = C.c_double
LIB.kvzx_harness_hbm_peak_gbs.argtypes = [C.c_int]
LIB.kvzx_rgb32_to_yuv420.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
LIB.kvzx_rgb32_to_yuv420_device_timed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def opts(owf, fmt=None):
    return (("preset", "ultrafast"), ("threads", 8), ("owf", owf), ("wpp", 1), ("qp", 32), ("me-range", 16), ("period", 64)) + ((("input-format", fmt),) if fmt else ())


def cpu_convert(variant):
    """rgb32 -> I420 on the CPU with the reference's arithmetic: its object code when there, else numpy"""
    if refcolor.available():
        return "reference object code", lambda p: refcolor.reference_rgb2yuv(variant, p, W, H)
    return "numpy statement", lambda p: refcolor.restatement_rgb2yuv(variant, p, W, H)


def run(e, feed, pictures, n, owf):
    """n pictures through feed(picture) -> access unit or None, then the pictures in flight; CPU seconds of the process and wall seconds"""
    got = 0
    c0, t0 = time.process_time(), time.perf_counter()
    for t in range(n):
        got += bool(feed(pictures[t % len(pictures)]))
    for _ in range(owf + 1):
        got += bool(feed(None))
    c1, t1 = time.process_time(), time.perf_counter()
    assert got == n, (got, n)
    return c1 - c0, t1 - t0


def host_paths(rgb, yuyv, i420):
    owf = 2
    for fmt, variant, vnum in (("rgb32", "c", 1), ("rgb32-sse41", "sse41", 2)):
        how, conv = cpu_convert(variant)
        tmp = np.empty(W * H * 3 // 2, dtype=np.uint8)

        def device_route(p):
            assert LIB.kvzx_rgb32_to_yuv420(p.ctypes.data, tmp.ctypes.data, W, H, vnum)
            return tmp

        paths = (("a", None, lambda e: (lambda p: e.encode(None if p is None else conv(p), want_recon=False)[0]), how + ", then encoder_encode"),
                 ("b", None, lambda e: (lambda p: e.encode(None if p is None else device_route(p), want_recon=False)[0]), "kvzx_rgb32_to_yuv420, then encoder_encode"),
                 ("c", fmt, lambda e: (lambda p: e.encode_packed(p, want_recon=False)[0]), "kvzx_encoder_encode_packed_host"))
        for name, f, make, what in paths:
            e = Encoder(W, H, options=opts(owf, f))
            assert not e.rejected, e.rejected
            feed = make(e)
            run(e, feed, rgb, 8, owf)                      # warm-up: buffers, page-locking
            cpu, wall = run(e, feed, rgb, NF, owf)
            e.close()
            emit({"measure": "host", "format": fmt, "path": name, "what": what, "pictures": NF, "owf": owf, "cpu_ms_per_picture": round(1e3 * cpu / NF, 3),
                  "pictures_per_s": round(NF / wall, 1)})
    for name, f, pictures in (("i420", None, i420), ("yuyv", "yuyv", yuyv)):
        e = Encoder(W, H, options=opts(owf, f))
        assert not e.rejected, e.rejected
        feed = (lambda p: e.encode_packed(p, want_recon=False)[0]) if f else (lambda p: e.encode(p, want_recon=False)[0])
        run(e, feed, pictures, 8, owf)
        cpu, wall = run(e, feed, pictures, NF, owf)
        e.close()
        emit({"measure": "host", "format": name, "path": "c" if f else "pre-converted", "pictures": NF, "owf": owf, "cpu_ms_per_picture": round(1e3 * cpu / NF, 3),
              "pictures_per_s": round(NF / wall, 1)})


def upload(a):
    a = np.ascontiguousarray(a)
    d = LIB.kvzx_harness_alloc(0, a.nbytes)
    assert d and LIB.kvzx_harness_upload(d, a.ctypes.data, a.nbytes)
    return d


def stage_us(e, feed, dptr, n):
    """mean time of the input stage's kernel over n profiled pictures, microseconds"""
    e.kernel_times(reset=True)
    for _ in range(n):
        assert feed(dptr)
    ms, k = e.kernel_times(reset=True)["k_pad_input"]
    assert k == n, (k, n)
    return 1e3 * ms / k


def kernel_times(rgb0, yuyv0, i4200):
    n, rounds = 20, 5
    cw, ch = input_model.coded_size(W, H)
    peak = LIB.kvzx_harness_hbm_peak_gbs(0)
    d_rgb, d_yuyv, d_i420, d_tmp = upload(rgb0), upload(yuyv0), upload(i4200), upload(i4200)
    enc = {}
    for key, fmt in (("i420", None), ("rgb32", "rgb32"), ("rgb32-sse41", "rgb32-sse41"), ("yuyv", "yuyv")):
        e = Encoder(W, H, options=opts(0, fmt) + (("period", 1),))      # (every picture intra: nothing of the previous picture runs beside the input stage)
        assert not e.rejected, e.rejected
        e.set_profiling(1)
        enc[key] = e
    feed_i420 = lambda d: enc["i420"].encode_device(d)
    ms = (C.c_float * n)()
    for fmt, variant in (("rgb32", 1), ("rgb32-sse41", 2)):
        feed = lambda d, e=enc[fmt]: e.encode_packed_device(d, want_recon=False)[0]
        stage_us(enc[fmt], feed, d_rgb, 4); stage_us(enc["i420"], feed_i420, d_i420, 4)      # warm-up
        fused, conv, pad = [], [], []
        for r in range(rounds):
            fused.append(stage_us(enc[fmt], feed, d_rgb, n))
            assert LIB.kvzx_rgb32_to_yuv420_device_timed(d_rgb, d_tmp, W, H, variant, n, ms)
            conv.append(1e3 * sum(ms) / n)
            pad.append(stage_us(enc["i420"], feed_i420, d_tmp, n))
        sums = [a + b for a, b in zip(conv, pad)]
        f_med, s_med = statistics.median(fused), statistics.median(sums)
        gb = (4 * W * H + 1.5 * cw * ch) / 1e9
        emit({"measure": "kernel", "format": fmt, "k_input_rgb32_us": [round(v, 2) for v in fused], "k_rgb32_to_i420_us": [round(v, 2) for v in conv],
              "k_pad_input_us": [round(v, 2) for v in pad], "pair_sum_us": [round(v, 2) for v in sums], "fused_median_us": round(f_med, 2),
              "pair_median_us": round(s_med, 2), "pass": bool(f_med <= s_med), "fused_gb_s": round(gb / (f_med * 1e-6), 1), "hbm_peak_gb_s": round(peak, 1),
              "fraction_of_peak": round(gb / (f_med * 1e-6) / peak, 4) if peak else None})
    feed = lambda d: enc["yuyv"].encode_packed_device(d, want_recon=False)[0]
    stage_us(enc["yuyv"], feed, d_yuyv, 4)
    y = [stage_us(enc["yuyv"], feed, d_yuyv, n) for _ in range(rounds)]
    gb = (2 * W * H + 1.5 * cw * ch) / 1e9
    emit({"measure": "kernel", "format": "yuyv", "k_input_yuyv_us": [round(v, 2) for v in y], "median_us": round(statistics.median(y), 2),
          "gb_s": round(gb / (statistics.median(y) * 1e-6), 1), "hbm_peak_gb_s": round(peak, 1),
          "fraction_of_peak": round(gb / (statistics.median(y) * 1e-6) / peak, 4) if peak else None})
    for e in enc.values():
        e.close()
    for d in (d_rgb, d_yuyv, d_i420, d_tmp):
        LIB.kvzx_harness_free(d)


def main():
    i420 = [orc.synth_frame(0, SEED, W, H, t) for t in range(CLIP)]
    rgb = [synth.to_rgb32(f, W, H) for f in i420]
    yuyv = [synth.to_yuyv(f, W, H) for f in i420]
    emit({"measure": "setup", "size": [W, H], "pictures": NF, "clip": CLIP, "cpu_conversion": cpu_convert("c")[0], "cpus": len(os.sched_getaffinity(0))})
    kernel_times(rgb[0], yuyv[0], i420[0])
    host_paths(rgb, yuyv, i420)


if __name__ == "__main__":
    main()
