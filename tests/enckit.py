"""What the encoder tests share: the HIP encoder opened and run over a clip, the clips, the closed loop through the decoders, and the HIP encoder held to the
checker's picture by picture (run_case).  Plain functions; a feature's test module builds its option tuple and calls these.  Test infrastructure; every assert
says what it saw (pytest rewrites asserts in test modules only)."""
import ctypes as C

import numpy as np
import pytest

import edge_content as ec
import orc

SEED = 0x5EED0000


# ---- the encoder and the clips
def encoder(w, h, opts=(), fields=None):
    """the HIP encoder with the options, none of them rejected"""
    from kvazzup_amd.codec import Encoder
    ge = Encoder(w, h, options=tuple(opts), fields=fields)
    assert not ge.rejected, "the encoder rejected %r" % (ge.rejected,)
    return ge


def encode_all(ge, frames, owf=0, per_picture=None):
    """(access unit, reconstruction) of every picture, the pictures in flight flushed; per_picture(ge), read behind each delivered picture, is appended to its tuple"""
    out = []
    for t in range(len(frames) + owf + 1):
        au, rec = ge.encode(frames[t] if t < len(frames) else None)
        if au:
            out.append((au, rec) + ((per_picture(ge),) if per_picture else ()))
    assert len(out) == len(frames), "%d pictures in, %d access units out" % (len(frames), len(out))
    return out


def oracle_encoder(w, h, n=None, tmvp=None, coarse=None, gop=None, opts=(), **kw):
    """the checker's encoder with lp-refs n, tmvp, me-coarse and lp-gop (g, d) set where given, then the named options"""
    e = orc.OracleEncoder(w, h, **kw)
    if n is not None:
        e.set_option("lp-refs", n)
    if tmvp is not None:
        e.set_option("tmvp", tmvp)
    if coarse is not None:
        e.set_option("me-coarse", coarse)
    if gop is not None:
        e.set_lp_gop(*gop)
    for name, value in opts:
        e.set_option(name, value)
    return e


def frames(kind, w, h, n, seed=SEED):
    return [orc.synth_frame(kind, seed, w, h, t) for t in range(n)]


def pan(w, h, n, dx=4, dy=2):
    """a textured picture moving (dx, dy) samples per picture: every block's motion is its collocated block's"""
    big = orc.synth_frame(0, SEED, 2 * w, 2 * h, 0)
    Y = big[:4 * w * h].reshape(2 * h, 2 * w)
    U = big[4 * w * h:5 * w * h].reshape(h, w)
    V = big[5 * w * h:].reshape(h, w)
    out = []
    for t in range(n):
        x0, y0 = w // 2 - dx * t, h // 2 - dy * t
        out.append(np.concatenate([Y[y0:y0 + h, x0:x0 + w].ravel(), U[y0 // 2:y0 // 2 + h // 2, x0 // 2:x0 // 2 + w // 2].ravel(),
                                   V[y0 // 2:y0 // 2 + h // 2, x0 // 2:x0 // 2 + w // 2].ravel()]).astype(np.uint8))
    return out


def planes(i420, w, h):
    ny = w * h
    return i420[:ny].reshape(h, w), i420[ny:ny + ny // 4].reshape(h // 2, w // 2), i420[ny + ny // 4:].reshape(h // 2, w // 2)


def psnr_y(a, b, n):
    mse = np.mean((a[:n].astype(np.float64) - b[:n].astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse)


# ---- the closed loop
def closed_loop(pairs, sei=False, pyhevc_too=False, frame_threaded=False):
    """every reconstruction of pairs = [(access unit, reconstruction)] == the checker's decoder's picture == the HIP decoder's picture; sei: the checker verified
    every picture's hash SEI; frame_threaded: the frame-threaded HIP decoder too; pyhevc_too: tests/pyhevc.py too.  On a mismatch the first picture and which decoder"""
    from kvazzup_amd.codec import Decoder
    od, gd = orc.OracleDecoder(), Decoder()
    gf = Decoder(threads=4, frame_threads=True) if frame_threaded else None
    try:
        for t, (au, rec) in enumerate(pairs):
            a = od.decode_au(au, t)
            assert len(a) == 1, "picture %d: the checker's decoder returned %d pictures" % (t, len(a))
            assert np.array_equal(a[0]["i420"], rec), "picture %d: the checker's decoder differs from the encoder's reconstruction (%d samples)" % (t, int((a[0]["i420"] != rec).sum()))
            b = gd.decode_au(au, t)
            assert len(b) == 1, "picture %d: the HIP decoder returned %d pictures" % (t, len(b))
            assert np.array_equal(b[0]["i420"], rec), "picture %d: the HIP decoder differs from the encoder's reconstruction (%d samples)" % (t, int((b[0]["i420"] != rec).sum()))
        if sei:
            checked, bad = od.hash_stats()
            assert checked == len(pairs) and bad == 0, "the checker's decoder verified %d hash SEI messages of %d pictures, %d bad" % (checked, len(pairs), bad)
        if gf:
            got = []
            for t, (au, _) in enumerate(pairs):
                got += gf.decode_au(au, t)
            got += gf.drain()
            assert len(got) == len(pairs), "the frame-threaded HIP decoder returned %d pictures of %d" % (len(got), len(pairs))
            for t, p in enumerate(got):
                assert np.array_equal(p["i420"], pairs[t][1]), "picture %d: the frame-threaded HIP decoder differs (%d samples)" % (t, int((p["i420"] != pairs[t][1]).sum()))
    finally:
        od.close(); gd.close()
        if gf:
            gf.close()
    if pyhevc_too:
        import pyhevc
        from deckit import tabs
        dec = pyhevc.Decoder(tabs())
        for au, _ in pairs:
            dec.decode(au)
        pics = dec.flush()
        assert len(pics) == len(pairs), "tests/pyhevc.py returned %d pictures of %d" % (len(pics), len(pairs))
        for t, p in enumerate(pics):
            assert np.array_equal(p["i420"], pairs[t][1]), "picture %d: tests/pyhevc.py differs (%d samples)" % (t, int((p["i420"] != pairs[t][1]).sum()))


def diagnose(dbg_o, dbg_g):
    """where the checker's picture (debug()) and the HIP encoder's (debug_all()) first differ, stage by stage: for a failing test's message"""
    msgs = []
    for k in ("cu_log2", "cu_intra", "cu_intra_mode", "cu_mv", "cu_cbf", "cu_flags"):
        a, b = dbg_o[k], dbg_g[k]
        if k == "cu_mv":
            m = (dbg_o["cu_intra"] == 0)
            a, b = a[m], b[m]
        if k == "cu_intra_mode":
            m = dbg_o["cu_intra"] == 1
            a, b = a[m], b[m]
        if not np.array_equal(a, b):
            bad = np.argwhere(np.asarray(a != b))
            msgs.append("%s differs at %d entries, first %s (oracle %s gpu %s)" % (k, len(bad), bad[0].tolist(), a[tuple(bad[0])] if a.ndim == bad.shape[1] else "?", b[tuple(bad[0])] if b.ndim == bad.shape[1] else "?"))
    for c in range(3):
        a, b = dbg_o["rec%d" % c], dbg_g["rec%d" % c]
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            msgs.append("rec%d differs at %d samples, first (y,x)=%s" % (c, len(bad), bad[0].tolist()))
    return "; ".join(msgs) if msgs else "no stage-level difference found (entropy coding / assembly?)"


# ---- the HIP encoder against the checker, picture by picture; a case is a dict in the vocabulary of checker() / hip()


def checker(w, h, c):
    """the checker's encoder for case c"""
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
    if c.get("weightp"):                              # "weightp"  and "intra-refresh" N (section 9f): tests/test_gpu_weightp_ir_oracle.py
        oe.set_option("weightp", c["weightp"])
    if c.get("intra_refresh"):
        oe.set_option("intra-refresh", c["intra_refresh"])
    for name, key in (("intra-in-p", "intra_in_p"), ("rdoq", "rdoq"), ("signhide", "signhide"), ("me-source", "me_source"), ("hash", "hash"),
                      ("scaling-list", "scaling_list"), ("lossless", "lossless")):     # (lossless last: it switches tools off)
        if c.get(key):
            oe.set_option(name, c[key])
    return oe


def hip(w, h, c):
    """the HIP encoder for case c"""
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
    o += ((("weightp", c["weightp"]),) if c.get("weightp") else ()) + ((("intra-refresh", c["intra_refresh"]),) if c.get("intra_refresh") else ())
    fields = dict(({"target_bitrate": br} if br else {}), **({"hash": c["hash"]} if c.get("hash") else {}))
    return encoder(w, h, o, fields=fields or None)


def first_stage(do, dg):
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
    for k in ("wp", "ir"):                              # weightp's record (flag, w, o per reference), then intra-refresh's (j, s, e, n): in front of every decision
        if k in do and k in dg:
            a, b = np.asarray(do[k]).tolist(), np.asarray(dg[k]).tolist()
            if a != b:
                return "first stage that differs: %s (the record): checker %s, HIP %s" % (k, a, b)
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


def case_frames(c):
    w, h = c["w"], c["h"]
    fr = _case_clip(c)
    if c.get("change"):                                # a brightness change on the luma of whatever clip the case names (tests/wp_model.py change())
        import wp_model
        fr = wp_model.change(fr, w, h, c["change"])
    return fr


def _case_clip(c):
    w, h, nf = c["w"], c["h"], c.get("frames", 5)
    if c.get("pattern"):
        return [ec.PATTERNS[c["pattern"]](w, h, t, ec.SEED) for t in range(nf)]
    if c.get("clip") == "alternating":                 # picture t repeats picture t - 2: the older reference wins
        a = orc.synth_frame(2, SEED, w, h, 0)
        b = orc.synth_frame(0, SEED ^ 0x1234, w, h, 3)
        return [a if t % 2 == 0 else b for t in range(nf)]
    if c.get("clip") == "pan":
        return pan(w, h, nf)
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
    frames = case_frames(c)
    oe = checker(w, h, c)
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
    ge = hip(w, h, c)
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
                    what, len(au_o), len(au), au == au_o, np.array_equal(rec, d["recon"]), first_stage(d, hip_debug(ge))))
            assert ge.last_bins() == d["bins"], "%s: %d bins, the checker counts %d" % (what, ge.last_bins(), d["bins"])
            got = gd.decode_au(au, t)
            assert len(got) == 1 and np.array_equal(got[0]["i420"], rec), "%s: the HIP decoder differs from the reconstruction" % what
            t += 1
        assert t == len(frames), "%d pictures in, %d access units out" % (len(frames), t)
    finally:
        ge.close()
        gd.close()


def hip_debug(ge):
    d = ge.debug_all()
    cw, ch = ge.coded_size()
    d["cu_mvd"] = ge.debug("cu_mvd", np.int16, (ch // 8, cw // 8, 2))
    return d


_NAMES = {"subme": "subme", "rdoq": "rdoq", "signhide": "signhide", "intra-in-p": "intra_in_p", "lp-refs": "n", "tmvp": "tmvp", "wpp": "wpp", "period": "period",
          "vaq": "vaq", "lossless": "lossless", "gpu-entropy": "gpu_entropy", "deblock": "deblock", "me-source": "me_source", "qp": "qp", "owf": "owf",
          "me-coarse": "coarse", "weightp": "weightp", "intra-refresh": "intra_refresh"}


def case_from_opts(opts, fields=None):
    """a row's kvazaar options in the vocabulary of checker() / hip(); an option without a mapping is an error, not a dropped row"""
    c = {}
    for k, v in opts:
        if k in _NAMES:
            c[_NAMES[k]] = int(v)
        elif k == "sao":
            c["sao"] = int(v == "full")
        elif k == "tiles":
            c["tiles"] = tuple(int(x) for x in v.split("x"))
        elif k == "slices":
            c["slices"] = {"none": 0, "wpp": 1, "tiles": 2}[v]
        elif k == "rc-algorithm":
            c["rc_lambda"] = int(v == "lambda")
        elif k == "scaling-list":
            c["scaling_list"] = int(v == "default")
        elif k == "me-early-termination":
            c["me_early"] = int(v == "on")
        elif k == "preset":
            c["preset"] = v                           # (hip() states every tool a preset touches after it, so the checker's options are the case's)
        elif k == "gop":
            g, d = v[len("lp-g"):-len("t1")].split("d")
            assert v == "lp-g%sd%st1" % (g, d), v
            c["gop"] = (int(g), int(d))
        elif k == "lp-gop":
            assert int(v) == 1, v                     # (the switch: the numbers come with "gop")
        elif k == "set-qp-in-cu":
            pass                                      # (checker() / hip() switch it on with the ROI map)
        else:
            raise KeyError("no checker mapping for option %s" % k)
    for k, v in (fields or {}).items():
        if k != "hash":
            raise KeyError(k)
        c["hash"] = v
    return c


ROI = (4, 3, (np.arange(12, dtype=np.int8) % 7 - 3).astype(np.int8))


def case_id(c):
    return "_".join("%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else ("" if k == "roi" else v))
                    for k, v in sorted(c.items()) if k not in ("w", "h"))


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
