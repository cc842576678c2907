"""scenecut ("uvgx scene cut v1") on the GPU: what an IDR picture at a scene cut buys and what the host's wait for the verdict costs.
1080p, presets ultrafast and veryfast (wpp, qp 32, me-range 16, period 64), scenecut off against scenecut=8:

  cut      64 pictures of the scene-cut clip (kvazzup_amd.synth.scene_cut_frame, the cut at picture 20), owf 0: bytes and luma PSNR of the cut picture and of the
           eight pictures behind it, total bytes and mean luma PSNR of the stream, which pictures are IDR pictures
  rate     encoder pictures/s on the benchmark's clip (no cut in it: the wait is all the option does) resident in device memory
           (kvzx_encoder_encode_device, input-hold), at owf 2 and owf 0, one warm-up pass, two rounds
  trace    `--trace PRESET`: encodes the scene-cut clip once with scenecut=8 and nothing else -- the program for a kernel-trace run of its own, e.g.
           rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure/scenecut_ab.py --trace ultrafast      (k_sc_sum, k_sc_blocks, k_sc_decide)

usage: python tools/measure/scenecut_ab.py [out.txt] [--pictures N]      (one JSON object per line, also appended to out.txt)"""
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
W, H, CUT, SEED, N_ON = 1920, 1080, 20, 1234, 8
ARGV = list(sys.argv[1:])
NF = 64
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


def opts(preset, scenecut, owf):
    return (("preset", preset), ("threads", 8), ("owf", owf), ("wpp", 1), ("qp", 32), ("me-range", 16), ("period", 64), ("scenecut", scenecut))


def cut_frame(t):
    """kvazzup_amd.synth.scene_cut_frame through the checker's generator (the same clip, tests/test_synth*.py): from the cut on the mirror image of another clip"""
    if t < CUT:
        return orc.synth_frame(0, SEED, W, H, t)
    f = orc.synth_frame(0, SEED ^ 0x00C0FFEE, W, H, t + 400)
    ny = W * H
    y = f[:ny].reshape(H, W)[::-1, ::-1]
    u = f[ny:ny + ny // 4].reshape(H // 2, W // 2)[::-1, ::-1]
    v = f[ny + ny // 4:].reshape(H // 2, W // 2)[::-1, ::-1]
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint8)


def at_the_cut(frames, preset, scenecut):
    e = Encoder(W, H, options=opts(preset, scenecut, 0))
    assert not e.rejected, e.rejected
    ny = W * H
    sizes, psnr, idr = [], [], []
    for t, f in enumerate(frames):
        au, rec = e.encode(f)
        sizes.append(len(au))
        mse = np.mean((rec[:ny].astype(np.float64) - f[:ny]) ** 2)
        psnr.append(10 * np.log10(255 ** 2 / max(mse, 1e-9)))
        if e.info["nal_unit_type"] == 19:
            idr.append(t)
    e.close()
    behind = slice(CUT + 1, CUT + 9)
    return {"idr_pictures": idr, "cut_bytes": sizes[CUT], "cut_psnr_y": round(float(psnr[CUT]), 3), "behind8_bytes": int(sum(sizes[behind])),
            "behind8_psnr_y": round(float(np.mean(psnr[behind])), 3), "total_bytes": int(sum(sizes)), "psnr_y": round(float(np.mean(psnr)), 3)}


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


def rate(dev, preset, scenecut, owf):
    e = Encoder(W, H, options=opts(preset, scenecut, owf) + (("input-hold", 1),))
    assert not e.rejected, e.rejected
    for d in dev:
        e.encode_device(d)
    t0 = time.perf_counter()
    for d in dev:
        e.encode_device(d)
    for _ in range(owf + 1):
        e.encode_device(None)
    dt = time.perf_counter() - t0
    e.close()
    return len(dev) / dt


def trace(preset):
    e = Encoder(W, H, options=opts(preset, N_ON, 0))
    for t in range(NF):
        e.encode(cut_frame(t), want_recon=False)
    e.close()


def main():
    if "--trace" in ARGV:
        return trace(ARGV[ARGV.index("--trace") + 1])
    cut = [cut_frame(t) for t in range(NF)]
    for preset in ("ultrafast", "veryfast"):
        for scenecut in (0, N_ON):
            d = {"what": "cut", "size": "%dx%d" % (W, H), "pictures": NF, "cut_at": CUT, "preset": preset, "scenecut": scenecut}
            d.update(at_the_cut(cut, preset, scenecut))
            emit(d)
    dev = upload([orc.synth_frame(0, SEED, W, H, t) for t in range(NF)])
    for preset in ("ultrafast", "veryfast"):
        for owf in (2, 0):
            d = {"what": "rate", "size": "%dx%d" % (W, H), "pictures": NF, "preset": preset, "owf": owf}
            for scenecut in (0, N_ON):
                d["fps_scenecut_%d" % scenecut] = [round(rate(dev, preset, scenecut, owf), 1) for _ in range(2)]
            emit(d)
    for d in dev:
        LIB.kvzx_harness_free(d)


if __name__ == "__main__":
    main()
