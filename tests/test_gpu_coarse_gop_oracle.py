"""GPU parity for "me-coarse"  and "lp-gop" (section 9d): the HIP encoder against the CPU checker (oracle/hevc_enc.c), which states
both features itself.  For every picture of every case: the access unit equals the checker's byte for byte, the reconstruction and the CABAC bin count
equal the checker's, and the HIP decoder turns the access unit into exactly that reconstruction (run_case of tests/enckit.py).  On a mismatch
the message names the first stage that differs: the coarse centres, the layer / QP, the reference distances, then the decisions, levels and samples.

These cases hold to the checker what the models (tests/me_coarse_model.py, tests/lp_gop_model.py: the integer search at subme 0, the structure) and the closed
loops (tests/test_gpu_me_coarse.py, tests/test_gpu_lp_gop.py: "decodable") cannot: fractional refinement around vectors up to +-288 samples with the rate of long
differences, the merge / AMVP choice among neighbours scaled by true POC distances, every consumer of the picture's QP (lambda in the search, the refinement,
the intra-in-P price, RDOQ, SAO; the chroma QP; VAQ / ROI targets; rate control v2's start), rate control v1 under the layer offsets, and the bin count of
pictures with mvd strings beyond 10 bins.

Every row of test_gpu_me_coarse.py CLOSED and of test_gpu_lp_gop.py ROWS (CLOSED + EXTRA) is a case here through case_from_opts(); none has a checker gap.
Each case also states, on the checker's output alone, that it exercises its subject (coverage())."""
import numpy as np
import pytest

import lp_gop_model as M
import lp_refs_model
from cases import LP_GOP_ROWS as GOP_ROWS, ME_COARSE_CLOSED as COARSE_ROWS
from enckit import ROI as _ROI, case_from_opts, case_id as _id, run_case, sweep_case

def coverage(c):
    """what the checker's pictures of case c must contain for the case to exercise its subject; returns run_case's check"""
    def check(want):
        n = max(c["n"], 1)
        longest = far = could = mvd = 0
        for _, d in want:
            if d["is_intra"]:
                continue
            inter = d["cu_intra"] == 0
            longest = max(longest, int(np.abs(d["cu_mv"].astype(np.int32)[inter]).max(initial=0)))
            amvp = inter & ((d["cu_flags"] & 2) == 0)
            if amvp.any():
                mvd = max(mvd, max(lp_refs_model.mvd_bits(int(v)) for v in np.abs(d["cu_mvd"].astype(np.int32)[amvp]).max(axis=0)))
            if c.get("gop"):
                g = c["gop"][0]
                dists = d["lp_gop"]["dists"]
                assert dists == M.ref_dists(d["poc"], g, n), (d["poc"], dists)
                if max(dists) > n:
                    could += 1
                    far += int((inter & (d["cu_ref"] == dists.index(max(dists)))).sum())
        if c.get("pan") and max(abs(c["pan"][0]), abs(c["pan"][1])) > 32 and c.get("coarse") and not all(d["is_intra"] for _, d in want):
            assert longest > 4 * 32, "no vector beyond 32 samples (longest %d quarter samples)" % longest
        if c.get("gop") and n >= 2 and could and c.get("expect_far", 1):
            assert far > 0, "no CU refers to the key picture at a distance beyond lp-refs"
        if c.get("expect_mvd"):
            assert mvd > 10, "no mvd component of more than 10 bins (longest %d)" % mvd
        if c.get("expect_intra_p"):
            assert any((not d["is_intra"]) and d["lp_gop"]["layer"] > 1 and d["cu_intra"].any() for _, d in want), "no intra unit in a P picture above layer 1"
        if c.get("expect_clip"):
            assert any((not d["is_intra"]) and d["lp_gop"]["qp"] == 51 and c["qp"] + d["lp_gop"]["layer"] > 51 for _, d in want), "no picture's QP was clipped"
    return check


def run(c):
    run_case(c, coverage(c))


# ---- the rows of tests/test_gpu_me_coarse.py CLOSED: 640x384, me-range 16, QP 32, a pan beyond the zero window
def _coarse_case(r):
    c = dict(w=640, h=384, R=16, qp=32, n=1, coarse=r.get("reach", 128), pan=r["pan"], frames=r.get("frames", 6), owf=r.get("owf", 0))
    if r.get("bitrate"):
        c["bitrate"] = r["bitrate"]
    c.update(case_from_opts(r.get("opts", ()), r.get("fields")))
    return c


COARSE_CASES = [_coarse_case(r) for r in COARSE_ROWS]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", COARSE_CASES, ids=[str(i) for i in range(len(COARSE_CASES))])
def test_me_coarse_rows_match_the_checker(gpu, cfg):
    run(cfg)


# ---- the rows of tests/test_gpu_lp_gop.py ROWS: 320x192, me-range 12, g4d3 unless the row says otherwise
def _gop_case(r):
    c = dict(w=r.get("w", 320), h=r.get("h", 192), R=12, n=r["n"], gop=(r.get("g", 4), r.get("d", 3)), frames=r.get("frames", 10), kind=r.get("kind", 0), owf=r.get("owf", 0))
    if r.get("bitrate"):
        c["bitrate"] = r["bitrate"]
    if r.get("roi"):
        c["roi"] = _ROI
    c.update(case_from_opts(r.get("opts", ()), r.get("fields")))
    return c


GOP_CASES = [_gop_case(r) for r in GOP_ROWS]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", GOP_CASES, ids=[str(i) for i in range(len(GOP_CASES))])
def test_lp_gop_rows_match_the_checker(gpu, cfg):
    run(cfg)


# ---- what the rows above do not reach
G43 = (4, 3)
MORE = [
    # both options with lp-refs 3, tmvp, me-source, subme 2, intra-in-P, SAO, three pictures in flight
    dict(w=384, h=256, R=12, n=3, tmvp=1, coarse=128, gop=G43, pan=(44, -36), me_source=1, subme=2, intra_in_p=1, sao=1, owf=3, frames=10),
    dict(w=384, h=256, R=12, n=4, tmvp=1, coarse=64, gop=(8, 4), pan=(-40, 44), subme=4, rdoq=1, signhide=1, frames=11),
    # constant-QP edges: the clip at 51 (49 + layers 3 / 4 of g8d4, 50 + layer 2), QP 0; the count restarting at the IDR picture (period 5 / 13)
    dict(w=320, h=192, n=3, gop=(8, 4), qp=49, period=13, frames=16, expect_clip=1), dict(w=320, h=192, n=2, tmvp=1, gop=(8, 4), qp=50, period=5, frames=12, expect_clip=1),
    dict(w=320, h=192, n=4, tmvp=1, gop=(3, 2), qp=50, period=13, subme=2, frames=15, expect_clip=1), dict(w=320, h=192, n=3, gop=(3, 2), qp=49, period=5, sao=1, frames=12),
    dict(w=320, h=192, n=2, tmvp=1, gop=(1, 1), qp=50, period=5, frames=8), dict(w=320, h=192, n=3, tmvp=1, gop=(8, 4), qp=0, period=13, frames=15),
    dict(w=320, h=192, n=4, gop=(3, 2), qp=0, period=5, subme=2, intra_in_p=1, frames=8), dict(w=320, h=192, n=2, gop=(1, 1), qp=0, frames=5),
    # rate control v1 and v2 with the layer offset on top of a moving QP, synchronous and with three pictures in flight
    dict(w=320, h=192, n=3, tmvp=1, gop=G43, bitrate=400000, frames=14), dict(w=320, h=192, n=3, tmvp=1, gop=G43, bitrate=150000, owf=3, frames=14),
    dict(w=320, h=192, n=3, tmvp=1, gop=G43, bitrate=400000, rc_lambda=1, sao=1, frames=14), dict(w=320, h=192, n=4, gop=G43, bitrate=150000, rc_lambda=1, owf=3, subme=2, frames=14),
    # the intra-in-P price under the layer offset: at QP 27 quarters lie between the price with the picture's lambda and with the base QP's (chosen on the
    # checker: these rows change when its price takes the base QP's lambda, the rows with intra-in-p above mostly do not)
    dict(w=320, h=192, n=3, tmvp=1, gop=G43, qp=27, intra_in_p=1, frames=10, expect_intra_p=1), dict(w=320, h=192, n=3, tmvp=1, gop=(8, 4), qp=27, intra_in_p=1, subme=2, frames=10, expect_intra_p=1),
    # VAQ and an ROI map: the targets take the picture's QP
    dict(w=320, h=192, n=3, tmvp=1, gop=G43, vaq=12, subme=2, frames=10), dict(w=320, h=192, n=3, tmvp=1, gop=(8, 4), roi=_ROI, qp=45, sao=1, frames=10),
    # me-coarse at sizes that are not multiples of 64 (of 32 in the quarter picture): the coarse stage's edge clamp, a second window that leaves the picture
    dict(w=130, h=70, R=8, n=1, coarse=64, pan=(36, -40), subme=2, frames=4), dict(w=130, h=70, R=8, n=3, tmvp=1, coarse=128, pan=(-60, 36), subme=4, frames=5),
    dict(w=702, h=394, R=16, n=1, coarse=128, pan=(72, -40), frames=3), dict(w=702, h=394, R=12, n=2, tmvp=1, coarse=256, pan=(-150, 90), subme=2, intra_in_p=2, frames=4),
    dict(w=200, h=120, R=8, n=2, coarse=64, gop=G43, pan=(40, 36), me_source=1, frames=6),
    # the longest mvd strings: the bin count is the point
    dict(w=640, h=384, R=16, n=1, coarse=256, pan=(236, -3), subme=4, frames=3, expect_mvd=1), dict(w=640, h=384, R=16, n=2, tmvp=1, coarse=256, pan=(-3, 250), subme=4, frames=4, expect_mvd=1),
    # 1080p
    dict(w=1920, h=1080, n=3, tmvp=1, preset="veryfast", R=16, sao=1, subme=2, intra_in_p=1, me_source=1, gop=G43, coarse=64, frames=4),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", MORE, ids=[_id(dict(c, size="%dx%d" % (c["w"], c["h"]))) for c in MORE])
def test_more_cases_match_the_checker(gpu, cfg):
    run(cfg)


# ---- full-range content (tests/edge_content.py) with me-coarse 128: in the cut every candidate of both windows ties -- the zero window and the lowest candidate win
EDGE = [dict(pattern=p, n=n, tmvp=n - 2, w=256, h=192, R=16, qp=q, coarse=128, frames=5)
        for p, q in (("cut_black_white", 32), ("hard_edges", 32), ("binary_noise", 22), ("near_black", 51)) for n in (1, 3)]
# (with lp-gop the cut reaches the key picture at distances 4 and 5, but no CU can refer to it: the pictures are constant black or white, every reference of the
# other colour ties on the SAD, one of the same colour is an exact match at any distance, and the rate then gives reference 0 or the nearer one -- so this
# case states that the tie goes to the lower reference, and is exempt from the key-picture condition)
EDGE += [dict(pattern="cut_black_white", n=3, tmvp=1, w=256, h=192, R=16, qp=32, coarse=128, gop=G43, intra_in_p=2, frames=7, expect_far=0)]
for _c in EDGE:
    _c["tmvp"] = max(_c["tmvp"], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", EDGE, ids=[_id(c) for c in EDGE])
def test_edge_content_matches_the_checker(gpu, cfg):
    run(cfg)


# ---- a seeded sweep: sweep_case of tests/enckit.py plus me-coarse, lp-gop and the content drawn from the generator
def coarse_gop_sweep_case(seed):
    c = sweep_case(seed)
    rng = np.random.default_rng(7000 + seed)
    coarse = int(rng.choice([0, 64, 128]))
    gop = (None, (4, 3), (8, 4), (3, 2))[int(rng.integers(0, 4))]
    if coarse:
        c["coarse"] = coarse
    if gop:
        c["gop"] = gop
        c["frames"] = c["frames"] + 4
    if int(rng.integers(0, 2)):                        # a pan, else the moving content sweep_case drew
        v = int(rng.integers(34, 60))
        c["pan"] = (v * int(rng.choice([-1, 1])), int(rng.integers(-40, 41)))
    # (the intra periods sweep_case draws, 1 .. 5 and 64, and its six to sixteen pictures mostly end a GOP before a key picture lies beyond lp-refs, and
    # nothing steers the drawn content towards it: the sweep does not promise such a CU -- the cases above do.  What coverage() asks of every case, the
    # distances of the model and a vector beyond the zero window on a pan with P pictures, holds here too)
    c["expect_far"] = 0
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_tool_combinations_with_both_options_match_the_checker(gpu, seed):
    run(coarse_gop_sweep_case(seed))
