"""Case tables that more than one test module runs.  A table one module uses stays in that module.  Test infrastructure."""
import random

# (wpp, tile rows, tile columns, slices) of the header tests: WPP, slices=wpp, tiles 2x2 with slices=tiles, ...
FORMS = ((1, 1, 1, 0), (1, 1, 1, 1), (0, 2, 2, 2), (1, 2, 1, 2), (0, 1, 1, 0))

# lp-gop's (g, d, lp-refs n): the headers on the CPU, the checker's structure and the HIP encoder's are held to the same ones
GDN = ((4, 3, 1), (4, 3, 2), (4, 3, 3), (4, 3, 4), (8, 4, 3), (3, 2, 4), (1, 1, 2))


def drawn(seed):
    """(w, h, the synthesiser's options) of "everything at once", drawn from the seed"""
    r = random.Random(1000 + seed)
    ctb = r.choice((6, 6, 5, 4))
    min_cb = r.choice([3, 3, 4] + ([5] if ctb >= 5 else []))
    sizes = [(416, 240), (352, 288), (192, 128), (640, 352), (128, 128)] if min_cb > 3 else [(416, 240), (352, 288), (200, 136), (648, 360), (64, 64)]
    w, h = r.choice(sizes)
    if min_cb == 5 and (w % 32 or h % 32):
        w, h = 192, 128
    layout = r.choice(("one", "free", "free", "tiles", "tile_slices"))
    kw = dict(ctb_log2=ctb, min_cb_log2=min_cb, cip=r.choice((0, 0, 1)), pcm=r.choice((0, 0, 15)), lf_across=r.choice((0, 1, 2)), intra_in_p=r.choice((10, 30, 50)))
    if layout == "free":
        kw["slices"] = 3
    elif layout == "tiles":
        kw.update(slices=0, tile_rows=r.choice((2, 3)), tile_cols=r.choice((1, 2, 3)))
    elif layout == "tile_slices":
        kw.update(slices=2, tile_rows=2, tile_cols=r.choice((1, 2)), wpp=0)
    else:
        kw["slices"] = 0
    if r.random() < 0.4 and layout in ("one", "free"):
        kw.update(long_term=1, gop=0, b_slices=0, intra_period=20)
    return w, h, kw


# ---- lp-refs (tests/test_gpu_lp_refs.py); lp-gop runs the same searches and closed loops under its structure, the checker its own search on them
LP_REFS_SEARCH = [
    dict(w=256, h=128, n=2, R=8, me_early=1, kind=0, frames=5),
    dict(w=256, h=192, n=3, R=8, me_early=0, kind=0, frames=6, qp=27),
    dict(w=192, h=128, n=4, R=6, me_early=0, kind=2, frames=6, qp=37),
    dict(w=256, h=256, n=4, R=8, me_early=1, kind=0, frames=6, tiles="2x2", mv_frame=2),
    dict(w=256, h=128, n=3, R=8, me_early=0, kind=0, frames=5, me_source=1),
]

LP_REFS_CLOSED = [
    dict(n=2), dict(n=3), dict(n=4),
    dict(n=3, opts=(("wpp", 0), ("tiles", "2x2"))),
    dict(n=2, opts=(("slices", "wpp"),)),
    dict(n=4, opts=(("tiles", "2x2"), ("slices", "tiles"), ("wpp", 0))),
    dict(n=3, owf=1), dict(n=4, owf=3), dict(n=4, owf=6, opts=(("period", 5),)), dict(n=2, owf=6, opts=(("period", 1),)),
    dict(n=3, opts=(("period", 5),)), dict(n=4, opts=(("period", 64),), frames=12),
    dict(n=3, opts=(("subme", 2),)), dict(n=4, opts=(("subme", 4), ("sao", "full"))),
    dict(n=3, opts=(("rdoq", 1), ("signhide", 1))),
    dict(n=3, opts=(("intra-in-p", 1), ("subme", 2))), dict(n=4, opts=(("intra-in-p", 2),), kind=2),
    dict(n=3, bitrate=400000), dict(n=3, bitrate=400000, opts=(("rc-algorithm", "lambda"), ("sao", "full"))),
    dict(n=2, opts=(("set-qp-in-cu", 1),), roi=True), dict(n=3, opts=(("vaq", 6),)),
    dict(n=3, opts=(("lossless", 1),)), dict(n=4, opts=(("scaling-list", "default"),)),
    dict(n=3, opts=(("gpu-entropy", 1),)), dict(n=4, opts=(("gpu-entropy", 1), ("owf", 2))),
    dict(n=3, fields={"hash": 2}, sei=True),                        # md5 SEI (the wrapper sets kvz_config.hash itself)
    dict(n=4, opts=(("me-source", 1), ("subme", 2), ("intra-in-p", 1), ("sao", "full")), owf=3),
    dict(n=2, opts=(("deblock", 0),)),
    dict(n=4, kind=2, opts=(("qp", 22), ("me-early-termination", "off"))),
]


# ---- me-coarse (tests/test_gpu_me_coarse.py); the checker runs the searches, the parity test every closed-loop row
ME_COARSE_SEARCH = [
    dict(clip=(72, -40), reach=128),
    dict(clip=(-100, 24), reach=128, me_source=1),
    dict(clip=(9, 150), reach=256),
    dict(clip=(200, 0), reach=256, R=8),
    dict(clip=(-44, -52), reach=64, n=3, frames=5),
    dict(clip=(72, -40), reach=128, n=3, me_source=1, frames=4),
    dict(clip=(-60, 36), reach=64, tiles="2x2"),
    dict(clip=(50, 70), reach=128, mv_frame=2, tiles="2x2"),
    dict(clip=(-72, 40), reach=128, mv_frame=2),
    dict(clip="moving", reach=128, me_early=1, frames=4),
    dict(clip="moving", reach=64, me_early=0, kind=2, n=3, frames=4, R=8),
    dict(clip=(72, -40), reach=128, me_early=0),
    dict(clip=(40, 28), reach=64, w=1920, h=1080, frames=2),
]

ME_COARSE_CLOSED = [
    dict(pan=(72, -40)), dict(pan=(-72, 40), opts=(("subme", 2),)), dict(pan=(40, 72), opts=(("subme", 4), ("sao", "full"))),
    dict(pan=(-40, -72), opts=(("rdoq", 1), ("signhide", 1))),
    dict(pan=(72, -40), opts=(("intra-in-p", 1), ("subme", 2))), dict(pan=(-100, 24), opts=(("intra-in-p", 2),)),
    dict(pan=(72, 40), opts=(("lp-refs", 2),)), dict(pan=(-72, -40), opts=(("lp-refs", 3), ("tmvp", 1))), dict(pan=(20, -90), opts=(("lp-refs", 4), ("subme", 2), ("tmvp", 1))),
    dict(pan=(72, -40), opts=(("tmvp", 1),)),
    dict(pan=(-72, 40), opts=(("tiles", "2x2"), ("wpp", 0))), dict(pan=(72, 40), opts=(("tiles", "2x2"), ("slices", "tiles"), ("wpp", 0))), dict(pan=(-72, -40), opts=(("slices", "wpp"),)),
    dict(pan=(72, -40), opts=(("wpp", 0),)),
    dict(pan=(72, -40), owf=1), dict(pan=(-72, 40), owf=3), dict(pan=(40, -72), owf=6, opts=(("period", 5),), frames=12),
    dict(pan=(72, -40), bitrate=400000), dict(pan=(-72, 40), bitrate=400000, opts=(("rc-algorithm", "lambda"), ("sao", "full"))),
    dict(pan=(72, 40), opts=(("vaq", 6),)), dict(pan=(-72, -40), opts=(("lossless", 1),)), dict(pan=(72, -40), opts=(("scaling-list", "default"),)),
    dict(pan=(-72, 40), opts=(("gpu-entropy", 1),)), dict(pan=(72, 40), fields={"hash": 2}, sei=True), dict(pan=(-72, -40), opts=(("deblock", 0),)),
    dict(pan=(230, 0), reach=256), dict(pan=(-9, -150), reach=256, opts=(("subme", 2), ("lp-refs", 2))), dict(pan=(0, 260), reach=256, opts=(("me-source", 1), ("subme", 2))),
    dict(pan=(-250, 120), reach=256, opts=(("sao", "full"), ("tmvp", 1))),
    dict(pan=(60, -36), reach=64, opts=(("me-source", 1), ("subme", 2), ("intra-in-p", 1), ("sao", "full")), owf=3),
]


# ---- lp-gop (tests/test_gpu_lp_gop.py): the closed loops of lp-refs under the structure and these; the parity test runs every row
LP_GOP_EXTRA = [
    dict(n=3, opts=(("tmvp", 1),)), dict(n=4, opts=(("tmvp", 1), ("subme", 2), ("sao", "full")), owf=3), dict(n=2, opts=(("tmvp", 1), ("slices", "wpp"))),
    dict(n=3, opts=(("me-coarse", 128),), w=384, h=256), dict(n=3, opts=(("me-coarse", 128), ("me-source", 1), ("tmvp", 1)), w=384, h=256, owf=2),
    dict(n=3, opts=(("me-source", 1),)), dict(n=4, opts=(("me-source", 1), ("tmvp", 1)), w=200, h=120),
    dict(n=3, opts=(("tmvp", 1),), w=328, h=184, frames=12), dict(n=3, opts=(("qp", 50), ("tmvp", 1))),
    dict(n=3, opts=(("tmvp", 1),), g=8, d=4, frames=14), dict(n=4, opts=(("tmvp", 1),), g=3, d=2, frames=10), dict(n=2, opts=(("tmvp", 1),), g=1, d=1),
    dict(n=1, opts=(("tmvp", 1),)), dict(n=3, opts=(("tmvp", 1), ("period", 5)), owf=6, frames=14),
]
LP_GOP_ROWS = LP_REFS_CLOSED + LP_GOP_EXTRA


# ---- the checker's own guard: an option at 0 is the checker of before (tests/test_oracle_lp_refs_tmvp.py, tests/test_oracle_me_coarse_lp_gop.py)
ORACLE_GUARD = [dict(kw=dict()), dict(kw=dict(subme=4)), dict(kw=dict(), opts=(("intra-in-p", 2),), kind=2),
         dict(kw=dict(tile_rows=2, tile_cols=2, slices=2, sao=1)), dict(kw=dict(bitrate=300000, rc_bands=4), frames=8),
         dict(kw=dict(subme=2), opts=(("me-source", 1), ("intra-in-p", 1)))]


# ---- weightp (tests/test_gpu_weightp.py: closed loops on the benchmark clip with wp_model.change(kind), 320x192 unless the row says otherwise, me-range 12, 8 pictures)
# and intra-refresh (tests/test_gpu_intra_refresh.py: size = (w, h, N), 2 n + 4 pictures); tests/test_gpu_weightp_ir_oracle.py holds every row to the checker
WEIGHTP_CLOSED = [
    dict(kind="offset"), dict(kind="gain", opts=(("subme", 2),)), dict(kind="flash", opts=(("subme", 4), ("sao", "full"))),
    dict(kind="gain", opts=(("lp-refs", 3), ("tmvp", 1), ("subme", 2))), dict(kind="offset", opts=(("lp-refs", 2), ("intra-in-p", 1), ("subme", 2), ("me-source", 1))),
    dict(kind="offset", opts=(("tiles", "2x2"), ("wpp", 0), ("lp-refs", 3))), dict(kind="flash", opts=(("tiles", "2x2"), ("slices", "tiles"), ("subme", 2))),
    dict(kind="gain", owf=3, opts=(("lp-refs", 4), ("subme", 2), ("sao", "full"), ("me-source", 1))), dict(kind="offset", owf=3, opts=(("period", 4),)),
    dict(kind="offset", bitrate=400000, opts=(("rc-algorithm", "lambda"), ("subme", 2))), dict(kind="gain", bitrate=400000, opts=(("rc-algorithm", "lambda"), ("rdoq", 1))),
    dict(kind="flash", w=384, h=256, opts=(("me-coarse", 64), ("lp-refs", 2))), dict(kind="gain", opts=(("rdoq", 1), ("signhide", 1), ("subme", 4))),
    dict(kind="offset", opts=(("rdoq", 1),)), dict(kind="gain", opts=(("lp-refs", 3), ("gop", "lp-g4d3t1"), ("lp-gop", 1), ("tmvp", 1), ("subme", 2))),
    dict(kind="offset", w=200, h=120, opts=(("subme", 2), ("slices", "wpp"))), dict(kind="none", opts=(("subme", 2), ("lp-refs", 2))),
]

INTRA_REFRESH_CLOSED = [
    dict(), dict(opts=(("subme", 2),)), dict(opts=(("subme", 4), ("sao", "full"))), dict(opts=(("rdoq", 1), ("signhide", 1), ("subme", 2))),
    dict(opts=(("weightp", 1), ("subme", 2)), change="offset"), dict(opts=(("me-source", 1), ("subme", 2), ("intra-in-p", 1))),
    dict(bitrate=400000, opts=(("rc-algorithm", "lambda"), ("subme", 2))), dict(owf=3, opts=(("subme", 2), ("sao", "full"), ("me-source", 1))),
    dict(opts=(("slices", "wpp"), ("subme", 2))), dict(opts=(("intra-in-p", 0), ("subme", 4))), dict(opts=(("intra-in-p", 1), ("sao", "full"))),
    dict(opts=(("intra-in-p", 2), ("subme", 2), ("rdoq", 1))), dict(opts=(("period", 4), ("subme", 2), ("intra-in-p", 1))), dict(owf=3, opts=(("period", 4),)),
    dict(size=(320, 192, 10), opts=(("preset", "veryfast"),)), dict(size=(200, 120, 8), opts=(("subme", 2), ("sao", "full"))), dict(size=(640, 384, 4), opts=(("subme", 2),)),
    dict(opts=(("wpp", 0), ("subme", 2))), dict(opts=(("deblock", 0), ("intra-in-p", 1))),
]
