"""GPU parity for "weightp"  and "intra-refresh" (section 9f): the HIP encoder against the CPU checker (oracle/hevc_enc.c), which states
both options itself.  For every picture of every case: the access unit equals the checker's byte for byte, the reconstruction and the CABAC bin count equal
the checker's, and the HIP decoder turns the access unit into exactly that reconstruction (run_case of tests/enckit.py).  On a mismatch the message names the
first stage that differs: the record of weights, the band, then the decisions, levels and samples.

These cases hold to the checker what the models (tests/wp_model.py: the record and the integer search at subme 0; tests/ir_model.py: the schedule and three
structural rules) and the closed loops (tests/test_gpu_weightp.py, tests/test_gpu_intra_refresh.py: "decodable") cannot: the fractional refinement priced on the
weighted prediction, levels and cbf of the weighted reconstruction, merge / AMVP / skip under weights, the choice between weighted and plain references, the
intra-in-P price against a weighted inter cost, SAO, rate control and the bin count of weighted pictures; the intra mode of every forced unit, the vector of
every clean block, the free quarters of a partially forced block, SAO's parameters beside the CTB column it leaves off, rate control with a band in every picture.

Every row of cases.WEIGHTP_CLOSED and cases.INTRA_REFRESH_CLOSED is a case here through enckit.case_from_opts(); none has a checker gap.  Each case also
states, on the checker's output alone, that it exercises its subject (coverage())."""
import numpy as np
import pytest

import enckit
import ir_model as IR
import scenecut_model
import wp_model as WP
from cases import INTRA_REFRESH_CLOSED as IR_ROWS, WEIGHTP_CLOSED as WP_ROWS
from enckit import ROI as _ROI, case_from_opts, case_id as _id, run_case, sweep_case


def _cw(w):
    return max(128, (w + 63) & ~63)


def coverage(c):
    """what the checker's pictures of case c must contain for the case to exercise its subject; returns run_case's check"""
    def check(want):
        if c.get("sweep"):                              # (a drawn case promises nothing: period 1 has no P picture at all)
            return
        w, h = c["w"], c["h"]
        pics = [d for _, d in want]
        if c.get("weightp"):
            weighted = frac = mixed = sat = rejected = 0
            for t, d in enumerate(pics):
                flags = [int(r[0]) for r in d["wp"]]
                if d["is_intra"]:
                    assert not any(flags)
                    continue
                weighted += any(flags)
                inter = d["cu_intra"] == 0
                on = np.asarray(flags, dtype=bool)[d["cu_ref"].astype(np.int32)]
                frac += int((inter & on & ((d["cu_mv"] & 3) != 0).any(axis=2)).sum())
                if flags[0] and d["m"] >= 2 and not flags[1]:
                    mixed += int((inter & on).any() and (inter & ~on).any())
                if flags[0]:                            # reference 0's search plane: the samples the whole-vector form clips
                    _, wk, ok = (int(v) for v in d["wp"][0])
                    prev = pics[t - 1]["rec0"].astype(np.int64)
                    un = ((prev * wk + 32) >> 6) + ok
                    sat += int(((un < 0) | (un > 255)).sum())
                    assert np.array_equal(WP.search_plane(pics[t - 1]["rec0"], d["wp"][0]), np.clip(un, 0, 255))
                else:                                   # a candidate the check refused?
                    y0, y1 = (f[:w * h].reshape(h, w) for f in (c["_frames"][t], c["_frames"][t - 1]))
                    rejected += int(WP.candidate(*WP.moments(y0), *WP.moments(y1))[2])
            if "expect_weighted" in c:
                assert weighted == c["expect_weighted"], "%d weighted pictures, the case expects %d" % (weighted, c["expect_weighted"])
            elif c.get("change", "none") == "none":
                assert weighted == 0, "%d weighted pictures on an unchanged clip" % weighted
            else:
                assert weighted >= 2, "%d weighted pictures on a changed clip" % weighted
                if c.get("subme") and c.get("expect_frac", 1):
                    assert frac > 0, "no fractional vector on a weighted reference"
            if c.get("expect_mixed"):
                assert mixed > 0, "no picture with flags (1, 0, ..) whose CUs refer to both kinds of reference"
            if c.get("expect_saturated"):
                assert sat > 0, "no sample of a search plane is clipped at 0 or 255"
            if c.get("expect_rejected"):
                assert rejected > 0, "no candidate that the check refuses"
            if c.get("expect_flat"):                    # v = 0 gives w = 64, and the offset reaches the ends of its range
                recs = [tuple(int(v) for v in d["wp"][0]) for d in pics if not d["is_intra"]]
                assert all(r[1] == 64 for r in recs) and any(r[2] in (-128, 127) for r in recs), recs
        if c.get("intra_refresh"):
            total = {}
            for d in pics:
                for k, v in IR.check_structure(d, d["poc"], _cw(w), c["intra_refresh"], c.get("intra_in_p", 0)).items():
                    total[k] = total.get(k, 0) + v
            assert all(total[k] > 0 for k in ("band", "clean", "last", "excluded_matter")), total
            if c.get("expect_bound"):                   # some clean block's vector is another one without the option
                off = dict(c, intra_refresh=0)
                oe = enckit.checker(w, h, off)
                changed = 0
                for f, d in zip(c["_frames"], pics):
                    oe.encode(f)
                    o = oe.debug()
                    if not d["is_intra"] and d["ir"][0] >= 1:
                        s8 = d["ir"][1] // 8
                        both = (d["cu_intra"][:, :s8] == 0) & (o["cu_intra"][:, :s8] == 0)
                        changed += int((both & (d["cu_mv"][:, :s8] != o["cu_mv"][:, :s8]).any(axis=2)).sum())
                oe.close()
                assert changed > 0, "the bound decides no clean block's vector"
    return check


def run(c):
    c["_frames"] = enckit.case_frames(c)                # (the input pictures, for the conditions that need them; run_case makes its own)
    run_case(c, coverage(c))


# ---- every row of cases.WEIGHTP_CLOSED: the benchmark clip (synth kind 0, seed 1234) under wp_model.change(kind), me-range 12, 8 pictures
def _wp_case(r):
    c = dict(w=r.get("w", 320), h=r.get("h", 192), R=12, qp=32, n=1, kind=0, seed=1234, frames=8, change=r["kind"], weightp=1, owf=r.get("owf", 0))
    if r.get("bitrate"):
        c["bitrate"] = r["bitrate"]
    c.update(case_from_opts(r.get("opts", ())))
    return c


WP_CASES = [_wp_case(r) for r in WP_ROWS]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", WP_CASES, ids=[str(i) for i in range(len(WP_CASES))])
def test_weightp_rows_match_the_checker(gpu, cfg):
    run(dict(cfg))


# ---- every row of cases.INTRA_REFRESH_CLOSED: the benchmark clip, QP 32, me-range 8; a cycle and what follows it, twelve pictures at the most
def _ir_case(r):
    w, h, N = r.get("size", (320, 192, 5))
    c = dict(w=w, h=h, R=8, qp=32, n=1, kind=0, seed=1234, frames=min(2 * IR.cycle(_cw(w), N) + 4, 12), intra_refresh=N, owf=r.get("owf", 0))
    if r.get("bitrate"):
        c["bitrate"] = r["bitrate"]
    if r.get("change"):
        c["change"] = r["change"]
    c.update(case_from_opts(r.get("opts", ())))
    return c


IR_CASES = [_ir_case(r) for r in IR_ROWS]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", IR_CASES, ids=[str(i) for i in range(len(IR_CASES))])
def test_intra_refresh_rows_match_the_checker(gpu, cfg):
    run(dict(cfg))


# ---- what the rows do not reach
def _wp(**kw):
    return dict(dict(w=320, h=192, R=12, qp=32, n=1, kind=0, seed=1234, frames=8, weightp=1, change="offset", subme=2), **kw)


def _ir(**kw):
    return dict(dict(w=320, h=192, R=8, qp=32, n=1, kind=0, seed=1234, frames=8, intra_refresh=5), **kw)


MORE = [
    # weightp under lp-gop g8d4 with four references and tmvp: the weights of references at distances up to 7
    _wp(n=4, tmvp=1, gop=(8, 4), change="gain", frames=12),
    # the intra-in-P price against a weighted inter cost, where quarters lie near the price (QP 27)
    _wp(qp=27, intra_in_p=1), _wp(qp=27, intra_in_p=2, change="gain"),
    # rate control v1 and v2 on weighted pictures, synchronous and with three pictures in flight
    _wp(bitrate=400000, frames=12), _wp(bitrate=400000, owf=3, frames=12, change="gain"),
    _wp(bitrate=400000, rc_lambda=1, frames=12, change="gain"), _wp(bitrate=400000, rc_lambda=1, owf=3, sao=1, frames=12),
    # VAQ and an ROI map; the arithmetic coder on the GPU; the default scaling lists; an independent slice (and a table) per tile
    _wp(vaq=6), _wp(roi=_ROI, qp=40, change="gain"), _wp(gpu_entropy=1, change="gain"), _wp(scaling_list=1), _wp(tiles=(2, 2), slices=2, wpp=0, change="gain"),
    # the flash: picture 4 refers to a weighted picture 3 and plain pictures 2 and 1
    _wp(n=3, change="flash", frames=9, expect_mixed=1), _wp(n=3, tmvp=1, change="flash", frames=9, subme=4, sao=1, expect_mixed=1),
    # intra-refresh: intra-in-p 0 / 1 / 2 x subme 0 / 2 / 4
] + [_ir(intra_in_p=ip, subme=sm) for ip in (0, 1, 2) for sm in (0, 2, 4)] + [
    _ir(rdoq=1, signhide=1, subme=2), _ir(bitrate=400000, subme=2, frames=12), _ir(bitrate=400000, rc_lambda=1, subme=2, sao=1, frames=12),
    _ir(me_source=1, subme=2, intra_in_p=1), _ir(weightp=1, change="offset", subme=2, sao=1),
    # a pan right to left: a clean block's match lies in what the reference picture has not cleaned, so the bound decides vectors
    _ir(pan=(6, 0), subme=2, expect_bound=1), _ir(pan=(6, 0), subme=4, intra_in_p=1, sao=1, expect_bound=1),
    # the shortest and the longest cycle; a coded picture wider than the visible one; the cycle restarting behind IDR pictures, and never
    _ir(intra_refresh=2, subme=2), _ir(intra_refresh=255, subme=2, frames=12), _ir(w=200, h=120, intra_refresh=8, subme=2, sao=1, frames=12),
    _ir(period=4, subme=2, intra_in_p=1, frames=10), _ir(period=0, subme=2, frames=9),
    _ir(w=128, h=64, intra_refresh=2, subme=2, intra_in_p=2, sao=1),
    # 1080p, three pictures each
    _wp(w=1920, h=1080, R=16, frames=3), _ir(w=1920, h=1080, R=16, intra_refresh=30, subme=2, sao=1, intra_in_p=1, frames=3),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", MORE, ids=[_id(dict(c, size="%dx%d" % (c["w"], c["h"]))) for c in MORE])
def test_more_cases_match_the_checker(gpu, cfg):
    run(dict(cfg))


# ---- full-range content (tests/edge_content.py) under a change of brightness, 256x192.  near_black darkening and hard_edges under a gain: samples of the search
# plane are clipped at 0 and 255, and so is the prediction (Clip1).  cut_black_white: flat pictures, v = 0 gives w = 64 and the offset reaches +-128's ends.
# binary_noise: pictures that share nothing -- the moments give a candidate and the check refuses it, every picture plain under the flag.  No refinement leaves the
# whole vector on these patterns (flat pictures tie and the centre wins; the edges and the noise move by whole samples or not at all), at any QP and subme: the
# fractional candidates are priced on clipped predictions and lose, so these cases are exempt from "a fractional vector on a weighted reference" (expect_frac 0)
EDGE = [dict(pattern="near_black", change="offset", expect_saturated=1), dict(pattern="hard_edges", change="gain", expect_saturated=1),
        dict(pattern="cut_black_white", change="offset", expect_flat=1), dict(pattern="binary_noise", change="gain", qp=22, expect_weighted=0, expect_rejected=1),
        dict(pattern="hard_edges", change="gain", n=3, tmvp=1, subme=0, expect_saturated=1), dict(pattern="near_black", change="offset", subme=4, sao=1, qp=22, expect_saturated=1)]
EDGE = [dict(dict(w=256, h=192, R=16, qp=32, n=1, weightp=1, subme=2, frames=6, expect_frac=0), **c) for c in EDGE]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", EDGE, ids=[_id(c) for c in EDGE])
def test_edge_content_matches_the_checker(gpu, cfg):
    run(dict(cfg))


# ---- both options under scenecut=2: the cut's IDR picture restarts the weights' history and the cycle.  The checker knows no scene cuts: it codes the pictures
# in front of the cut as one stream and the pictures from the cut on as a fresh one (tests/test_gpu_scenecut.py pins the plain encoder the same way)
@pytest.mark.gpu
def test_both_options_under_scenecut_match_the_checker(gpu):
    w, h, n, cut = 320, 192, 11, 5
    c = dict(w=w, h=h, R=8, qp=32, n=1, subme=2, sao=1, weightp=1, intra_refresh=5, period=0)
    frames = scenecut_model.cut_clip(w, h, n, cut)
    want = []
    for part in (frames[:cut], frames[cut:]):
        oe = enckit.checker(w, h, c)
        for f in part:
            au = oe.encode(f)
            want.append((au, oe.recon(), oe.debug()))
        oe.close()
    assert [d["ir"][0] for _, _, d in want] == [-1, 0, 1, 2, 3, -1, 0, 1, 2, 3, 4]
    ge = enckit.encoder(w, h, (("qp", 32), ("period", 0), ("me-range", 8), ("subme", 2), ("sao", "full"), ("weightp", 1), ("intra-refresh", 5), ("scenecut", 2)))
    try:
        for t, f in enumerate(frames):
            au, rec = ge.encode(f)
            if au != want[t][0] or not np.array_equal(rec, want[t][1]):
                pytest.fail("picture %d: access unit %d vs %d bytes (checker / HIP), equal=%s, reconstruction equal=%s; %s" % (
                    t, len(want[t][0]), len(au), au == want[t][0], np.array_equal(rec, want[t][1]), enckit.first_stage(dict(want[t][2], m=1), enckit.hip_debug(ge))))
            assert ge.last_bins() == want[t][2]["bins"], t
    finally:
        ge.close()


# ---- a seeded sweep: sweep_case of tests/enckit.py with weightp (and a change) or intra-refresh N drawn on top; the tools an option is not stated with at
# their allowed values
def wp_ir_sweep_case(seed):
    c = sweep_case(seed)
    rng = np.random.default_rng(9000 + seed)
    c["lossless"] = 0
    c["sweep"] = 1
    if seed % 2 == 0:
        c["weightp"] = 1
        c["change"] = str(rng.choice(["offset", "gain", "flash", "none"]))
    else:
        c["intra_refresh"] = int(rng.choice([2, 3, 5, 8, 255]))
        c.update(n=1, tmvp=0, tiles=(1, 1))
        if int(rng.integers(0, 2)):
            c["weightp"] = 1
            c["change"] = str(rng.choice(["offset", "gain"]))
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_tool_combinations_with_the_options_match_the_checker(gpu, seed):
    run(wp_ir_sweep_case(seed))
