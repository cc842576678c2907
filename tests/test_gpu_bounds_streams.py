"""The HIP decoder at the bounds of the syntax (tests/bounds_cases.py; the checker and tests/pyhevc.py agree on every row: tests/test_bounds_streams.py): levels of
+-32767 and -32768 behind the longest escape codes through the parser's clip, the 32-bit and 64-bit dequantisers at QP 0 and 51 with and without scaling lists, the
16-bit clip between the inverse transform's stages and the MFMA / dot2 stage sums on coefficients that all pull one way, such levels as the residual of
transquant-bypass and transform-skip blocks; vector differences at the ends of their range, vectors folded across +-2^15 and reference blocks 8192 samples outside the
picture; weights, offsets and denominators at their ends on samples of 0 and 255; pictures smaller than a coding tree block, one coding tree block wide under WPP, and
tiles of one coding tree block.  Every picture is the checker's bit for bit."""
import pytest

import batch_cases as bc
import bounds_cases
from deckit import run_stream, together


@pytest.mark.gpu
@pytest.mark.parametrize("r", bounds_cases.ROWS, ids=lambda r: r["id"])
def test_bounds_row(gpu, r):
    run_stream(r["w"], r["h"], r["pictures"], **r["cfg"])


@pytest.mark.gpu
@pytest.mark.parametrize("r", [r for r in bounds_cases.ROWS if r["frames"]], ids=lambda r: r["id"])
def test_bounds_row_with_four_frame_threads(gpu, r):
    run_stream(r["w"], r["h"], r["pictures"], threads=4, frame_threads=True, **r["cfg"])


@pytest.mark.gpu
def test_a_saturating_stream_beside_an_ordinary_one_in_the_submission_layer(gpu):
    """two decoders, held so that their pictures leave in the same launches: a batched launch shares no dequantiser or transform assumption across pictures"""
    sat = bounds_cases.BY_ID["levels-sizes-inter"]
    streams = [bc.gen(sat["w"], sat["h"], sat["cfg"], sat["pictures"]),
               bc.gen(200, 136, dict(seed=5, num_refs=2, tmvp=1, sao=1, intra_in_p=20), 4)]
    st = together(streams, hold=True)
    assert st["pictures"] == bc.total(streams) and sum(st["sizes"][2:]) >= 1, st
