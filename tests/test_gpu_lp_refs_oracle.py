"""GPU parity for "lp-refs"  and "tmvp" (section 9b): the HIP encoder against the CPU checker (oracle/hevc_enc.c), which
states both features itself.  For every picture of every case: the access unit equals the checker's byte for byte, the reconstruction and the
CABAC bin count equal the checker's, and the HIP decoder turns the access unit into exactly that reconstruction.  On a mismatch the message names
the first stage that differs (decisions, then levels, then samples).

These cases hold to the checker what the closed-loop tests (tests/test_gpu_lp_refs.py, tests/test_gpu_tmvp.py) can only hold to "decodable": the
reference each CU searches, refines and predicts from, the intra-in-P choice priced with reference bins, rate control, SAO and VAQ on pictures
with several references, the temporal candidates on coded pictures."""
import pytest

from enckit import ROI as _ROI, case_id as _id, run_case, sweep_case


# ---- the cases of tests/test_gpu_lp_refs.py CLOSED and tests/test_gpu_tmvp.py CASES the checker expresses, each with tmvp 0 and 1
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
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_tool_combinations_with_references_match_the_checker(gpu, seed):
    run_case(sweep_case(seed))
