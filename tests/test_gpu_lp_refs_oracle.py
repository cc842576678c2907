"""GPU parity for "lp-refs"  and "tmvp" (section 9b): the HIP encoder against the CPU checker (oracle/hevc_enc.c), which
states both features itself.  For every picture of every case: the access unit equals the checker's byte for byte, the reconstruction and the
CABAC bin count equal the checker's, and the HIP decoder turns the access unit into exactly that reconstruction.  On a mismatch the message names
the first stage that differs (decisions, then levels, then samples).

These cases hold to the checker what the closed-loop tests (tests/test_gpu_lp_refs.py, tests/test_gpu_tmvp.py) can only hold to "decodable": the
reference each CU searches, refines and predicts from, the intra-in-P choice priced with reference bins, rate control, SAO and VAQ on pictures
with several references, the temporal candidates on coded pictures."""
import ctypes as C

import numpy as np
import pytest

import edge_content as ec
import orc

SEED = 0x5EED0000


def _checker(w, h, c):
    tc, tr = c.get("tiles", (1, 1))
    oe = orc.OracleEncoder(w, h, qp=c.get("qp", 32), period=c.get("period", 64), me_range=c.get("R", 12), wpp=c.get("wpp", 1), deblock=c.get("deblock", 1),
                           bitrate=c.get("bitrate", 0), tile_rows=tr, tile_cols=tc, qp_in_cu=int(bool(c.get("roi"))), sao=c.get("sao", 0),
                           mv_frame=c.get("mv_frame", 0), vaq=c.get("vaq", 0), me_early=c.get("me_early", 1), subme=c.get("subme", 0),
                           rc_bands=4 if c.get("rc_lambda") else 0, slices=c.get("slices", 0))
    owf = c.get("owf", 0)
    if c.get("bitrate") and owf >= 3:
        oe.set_option("rc-delay", owf + 1)            # the controller books picture t - (pictures in flight + 1), as encoder.hip does
    oe.set_option("lp-refs", c["n"])
    oe.set_option("tmvp", c.get("tmvp", 0))
    if c.get("coarse"):                               # "me-coarse"  and "lp-gop" with the gop string's g, d (section 9d): tests/test_gpu_coarse_gop_oracle.py
        oe.set_option("me-coarse", c["coarse"])
    if c.get("gop"):
        oe.set_lp_gop(*c["gop"])
    for name, key in (("intra-in-p", "intra_in_p"), ("rdoq", "rdoq"), ("signhide", "signhide"), ("me-source", "me_source"), ("hash", "hash"),
                      ("scaling-list", "scaling_list"), ("lossless", "lossless")):     # (lossless last: it switches tools off)
        if c.get(key):
            oe.set_option(name, c[key])
    return oe


def _hip(w, h, c):
    from kvazzup_amd.codec import Encoder
    tc, tr = c.get("tiles", (1, 1))
    br = c.get("bitrate", 0)
    o = ((("preset", c["preset"]),) if c.get("preset") else ()) + (
        ("qp", c.get("qp", 32)), ("period", c.get("period", 64)), ("me-range", c.get("R", 12)), ("wpp", c.get("wpp", 1)), ("deblock", c.get("deblock", 1)),
        ("tiles", "%dx%d" % (tc, tr)), ("sao", "full" if c.get("sao") else "off"), ("subme", c.get("subme", 0)), ("intra-in-p", c.get("intra_in_p", 0)),
        ("rdoq", c.get("rdoq", 0)), ("signhide", c.get("signhide", 0)), ("me-source", c.get("me_source", 0)), ("owf", c.get("owf", 0)),
        ("mv-constraint", ("none", "frame", "frametilemargin")[c.get("mv_frame", 0)]), ("me-early-termination", "on" if c.get("me_early", 1) else "off"),
        ("slices", ("none", "wpp", "tiles")[c.get("slices", 0)]), ("gpu-entropy", c.get("gpu_entropy", 0)), ("set-qp-in-cu", int(bool(c.get("roi")))),
        ("lp-refs", c["n"]), ("tmvp", c.get("tmvp", 0)))
    o += ((("vaq", c["vaq"]),) if c.get("vaq") else ()) + ((("bitrate", br),) if br else ()) + ((("rc-algorithm", "lambda"),) if c.get("rc_lambda") else ())
    o += ((("scaling-list", "default"),) if c.get("scaling_list") else ()) + ((("lossless", 1),) if c.get("lossless") else ())
    o += ((("me-coarse", c["coarse"]),) if c.get("coarse") else ()) + ((("gop", "lp-g%dd%dt1" % tuple(c["gop"])), ("lp-gop", 1)) if c.get("gop") else ())
    fields = dict(({"target_bitrate": br} if br else {}), **({"hash": c["hash"]} if c.get("hash") else {}))
    ge = Encoder(w, h, options=o, fields=fields or None)
    assert not ge.rejected, ge.rejected
    return ge


def _first_stage(do, dg):
    """the first stage at which the checker's picture (do) and the HIP encoder's (dg) differ, in the order the encoder decides them"""
    inter = (do["cu_intra"] == 0)
    intra = ~inter
    m = do.get("m")                                     # active references of the picture (run_case)
    if "me_coarse" in do and "me_coarse" in dg:         # the coarse stage's centres of the active references (the library's array keeps what an earlier picture left beyond them)
        a, b = np.asarray(do["me_coarse"])[:m], np.asarray(dg["me_coarse"])[:m]
        bad = np.argwhere((a != b).any(axis=-1))
        if len(bad):
            i = tuple(bad[0])
            return "first stage that differs: me_coarse (centres) at %d blocks, first (reference, block row, column) %s: checker %s, HIP %s" % (len(bad), list(i), a[i], b[i])
    if "lp_gop" in do and "lp_gop" in dg:
        for k in ("layer", "qp", "dists"):              # the layer and the QP, then the reference distances
            if do["lp_gop"][k] != dg["lp_gop"][k]:
                return "first stage that differs: lp_gop %s: checker %s, HIP %s" % (k, do["lp_gop"][k], dg["lp_gop"][k])
    order = [("cu_log2", None), ("cu_intra", None), ("cu_intra_mode", intra), ("cu_ref", inter), ("cu_mv", inter), ("cu_flags", inter),
             ("cu_merge_idx", inter), ("cu_mvp_idx", inter), ("cu_mvd", inter), ("cu_cbf", None), ("coef0", None), ("coef1", None), ("coef2", None),
             ("predeblock0", None), ("predeblock1", None), ("predeblock2", None), ("bs_v", None), ("bs_h", None), ("rec0", None), ("rec1", None), ("rec2", None)]
    for k, mask in order:
        if k not in do or k not in dg:
            continue
        a, b = np.asarray(do[k]), np.asarray(dg[k])
        if a.shape != b.shape:
            return "%s: shapes %s vs %s" % (k, a.shape, b.shape)
        if mask is not None:
            a, b = a[mask], b[mask]
        bad = np.argwhere(a != b)
        if len(bad):
            i = tuple(bad[0])
            where = ("(8x8 block %s)" % (np.argwhere(mask)[bad[0][0]].tolist(),)) if mask is not None else "(at %s)" % (list(i),)
            return "first stage that differs: %s at %d entries, first %s: checker %s, HIP %s" % (k, len(bad), where, a[i[:a.ndim]], b[i[:b.ndim]])
    return "no stage-level difference found (entropy coding / slice headers?)"


def _frames(c):
    w, h, nf = c["w"], c["h"], c.get("frames", 5)
    if c.get("pattern"):
        return [ec.PATTERNS[c["pattern"]](w, h, t, ec.SEED) for t in range(nf)]
    if c.get("clip") == "alternating":                 # picture t repeats picture t - 2: the older reference wins
        a = orc.synth_frame(2, SEED, w, h, 0)
        b = orc.synth_frame(0, SEED ^ 0x1234, w, h, 3)
        return [a if t % 2 == 0 else b for t in range(nf)]
    if c.get("clip") == "pan":
        from test_gpu_tmvp import _pan
        return _pan(w, h, nf)
    if c.get("pan"):                                   # a global pan of (vx, vy) samples a picture (tests/pan_content.py)
        import pan_content
        return pan_content.clip(w, h, nf, *c["pan"])
    if c.get("clip") == "blink":                       # a background that is covered for four pictures and shown again (tests/occluder_content.py)
        import occluder_content
        return occluder_content.blink_clip(w, h, nf, kind=c.get("kind", 0))
    return [orc.synth_frame(c.get("kind", 0), c.get("seed", SEED), w, h, t) for t in range(nf)]


def run_case(c, check=None):
    """check(want): conditions on the checker's pictures [(access unit, debug arrays)] alone -- that the case exercises its subject -- before the HIP encoder runs"""
    from kvazzup_amd.codec import Decoder
    w, h, owf = c["w"], c["h"], c.get("owf", 0)
    frames = _frames(c)
    oe = _checker(w, h, c)
    roi = None
    if c.get("roi"):
        roi = c["roi"]
        oe.set_roi(*roi)
    want = []
    for f in frames:
        au = oe.encode(f)
        d = oe.debug()
        d["recon"] = oe.recon()
        d["m"] = 0 if d["is_intra"] else min(max(c["n"], 1), d["poc"])
        want.append((au, d))
    oe.close()
    if check:
        check(want)
    ge = _hip(w, h, c)
    gd = Decoder()
    try:
        t = 0
        for i in range(len(frames) + owf):
            if i < len(frames):
                if roi:
                    p = ge.pic.contents
                    p.roi.width, p.roi.height = roi[0], roi[1]
                    p.roi.roi_array = roi[2].ctypes.data_as(C.POINTER(C.c_int8))
                au, rec = ge.encode(frames[i])
            else:
                au, rec = ge.encode(None)
            if au is None:
                continue
            au_o, d = want[t]
            what = "picture %d (%s, m = %d)" % (t, "I" if d["is_intra"] else "P", d["m"])
            if au != au_o or not np.array_equal(rec, d["recon"]):
                pytest.fail("%s: access unit %d vs %d bytes (checker / HIP), equal=%s, reconstruction equal=%s; %s" % (
                    what, len(au_o), len(au), au == au_o, np.array_equal(rec, d["recon"]), _first_stage(d, _hip_debug(ge))))
            assert ge.last_bins() == d["bins"], (what, ge.last_bins(), d["bins"])
            got = gd.decode_au(au, t)
            assert len(got) == 1 and np.array_equal(got[0]["i420"], rec), "%s: the HIP decoder differs from the reconstruction" % what
            t += 1
        assert t == len(frames), t
    finally:
        ge.close()
        gd.close()


def _hip_debug(ge):
    d = ge.debug_all()
    cw, ch = ge.coded_size()
    d["cu_mvd"] = ge.debug("cu_mvd", np.int16, (ch // 8, cw // 8, 2))
    return d


# ---- the cases of tests/test_gpu_lp_refs.py CLOSED and tests/test_gpu_tmvp.py CASES the checker expresses, each with tmvp 0 and 1
_ROI = (4, 3, (np.arange(12, dtype=np.int8) % 7 - 3).astype(np.int8))
TOOLS = [
    dict(n=2), dict(n=3), dict(n=4),
    dict(n=3, subme=1), dict(n=2, subme=2), dict(n=3, subme=3), dict(n=4, subme=4, sao=1),
    dict(n=3, intra_in_p=1, subme=2), dict(n=4, intra_in_p=2, kind=2),
    dict(n=3, me_source=1, subme=2, intra_in_p=1, owf=3), dict(n=4, me_source=1, subme=2, intra_in_p=1, sao=1, owf=6),
    dict(n=3, wpp=0, tiles=(2, 2)), dict(n=4, wpp=0, tiles=(2, 2), slices=2), dict(n=2, slices=1),
    dict(n=2, owf=6, period=1), dict(n=3, period=4, frames=9), dict(n=4, owf=6, period=5, frames=11), dict(n=3, period=8, frames=12),
    dict(n=3, bitrate=400000, frames=9), dict(n=3, bitrate=400000, rc_lambda=1, sao=1, frames=9), dict(n=4, bitrate=400000, rc_lambda=1, owf=3, frames=10),
    dict(n=3, sao=1), dict(n=3, rdoq=1, signhide=1), dict(n=3, vaq=6), dict(n=2, roi=_ROI), dict(n=3, lossless=1), dict(n=4, scaling_list=1),
    dict(n=3, gpu_entropy=1), dict(n=4, gpu_entropy=1, owf=2), dict(n=3, hash=2), dict(n=2, deblock=0),
    dict(n=3, mv_frame=1), dict(n=4, mv_frame=2, tiles=(2, 2)),
    dict(n=4, kind=2, qp=22, me_early=0),
]
TOOL_CASES = [dict(c, tmvp=tm) for c in TOOLS for tm in (0, 1)]


def _id(c):
    return "_".join("%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else ("" if k == "roi" else v))
                    for k, v in sorted(c.items()) if k not in ("w", "h"))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", TOOL_CASES, ids=[_id(c) for c in TOOL_CASES])
def test_tools_match_the_checker(gpu, cfg):
    run_case(dict(dict(w=320, h=192, frames=6), **cfg))


# ---- sizes that are not multiples of 64 (the TMVP bottom-right rule reads the coded picture's edge), and the 1080p preset case
SIZES = [dict(w=130, h=70, n=3, tmvp=1, R=8, frames=5), dict(w=130, h=70, n=4, tmvp=1, R=8, subme=4, kind=2, frames=5),
         dict(w=702, h=394, n=3, tmvp=1, frames=4), dict(w=702, h=394, n=2, tmvp=1, intra_in_p=2, subme=2, frames=4),
         dict(w=16, h=16, n=4, tmvp=1, R=8, frames=6), dict(w=192, h=128, n=3, tmvp=1, clip="pan", period=4, intra_in_p=1, frames=7),
         dict(w=1920, h=1080, n=3, tmvp=1, preset="veryfast", R=16, sao=1, subme=2, intra_in_p=1, me_source=1, frames=3)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SIZES, ids=[_id(dict(c, size="%dx%d" % (c["w"], c["h"]))) for c in SIZES])
def test_sizes_match_the_checker(gpu, cfg):
    run_case(cfg)


# ---- full-range content (tests/edge_content.py): in the cut every candidate of every reference ties -- reference 0 and the lowest candidate win
EDGE = [dict(pattern=p, n=n, tmvp=n - 3, w=256, h=192, R=16, qp=q, frames=5)
        for p, q in (("cut_black_white", 32), ("hard_edges", 32), ("binary_noise", 22), ("near_black", 51)) for n in (3, 4)]
EDGE += [dict(pattern="cut_black_white", n=4, tmvp=1, w=256, h=192, R=16, qp=32, frames=5, intra_in_p=2),
         dict(clip="alternating", n=2, tmvp=1, w=320, h=192, qp=30, frames=8), dict(clip="alternating", n=3, w=320, h=192, qp=30, subme=2, intra_in_p=1, frames=8)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", EDGE, ids=[_id(c) for c in EDGE])
def test_edge_content_matches_the_checker(gpu, cfg):
    run_case(cfg)


# ---- a seeded sweep: everything test_gpu_encoder.py's test_random_tool_combinations_match_oracle draws, plus lp-refs 2..4 and tmvp 0 / 1
def sweep_case(seed):
    rng = np.random.default_rng(5000 + seed)
    w, h = int(rng.integers(8, 60)) * 8, int(rng.integers(8, 48)) * 8
    hc = (h + 63) // 64
    c = dict(w=w, h=h, qp=int(rng.integers(8, 46)), period=int(rng.choice([1, 2, 3, 5, 64])), R=int(rng.choice([1, 4, 8, 16, 32])),
             wpp=int(rng.integers(0, 2)), deblock=int(rng.integers(0, 2)), sao=int(rng.integers(0, 2)), bitrate=int(rng.choice([0, 0, 0, 150000, 2000000])),
             mv_frame=int(rng.choice([0, 0, 1, 2])), vaq=int(rng.choice([0, 0, 3, 12])), me_early=int(rng.integers(0, 2)))
    tr = int(rng.integers(1, min(hc, 3) + 1))
    qp_in_cu = int(rng.integers(0, 2))
    c["owf"] = int(rng.choice([0, 1, 2, 3, 5]))
    c["kind"] = int(rng.choice([0, 2]))
    c["seed"] = 77 + seed
    c["subme"] = int(rng.choice([0, 0, 2, 4]))
    tc = int(rng.choice([1, 1, 2])) if w >= 256 else 1
    c["tiles"] = (tc, tr)
    c.update(intra_in_p=int(rng.integers(0, 3)), rdoq=int(rng.integers(0, 2)), signhide=int(rng.integers(0, 2)))
    c["lossless"] = int(rng.integers(0, 4) == 0)
    c["me_source"] = int(rng.integers(0, 2))
    c["n"] = int(rng.integers(2, 5))
    c["tmvp"] = int(rng.integers(0, 2))
    if qp_in_cu or c["vaq"]:
        rw, rh = int(rng.integers(1, 6)), int(rng.integers(1, 5))
        c["roi"] = (rw, rh, np.ascontiguousarray(rng.integers(-14, 15, rw * rh), dtype=np.int8))
    c["frames"] = (9 if c["owf"] < 3 else 12) if c["bitrate"] else 6
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_tool_combinations_with_references_match_the_checker(gpu, seed):
    run_case(sweep_case(seed))
