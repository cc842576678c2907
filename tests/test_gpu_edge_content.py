"""GPU parity on full-range, saturating content (tests/edge_content.py): ±255 residuals over whole blocks, all-tie motion
search, 0/255 reference samples, reconstructions and filters that only stay in [0, 255] through their clip.  For every
picture of every case: the HIP encoder's access unit equals the checker's byte for byte, its reconstruction and bin count
equal the checker's, and the HIP decoder turns the access unit into exactly that reconstruction."""
import numpy as np
import pytest

import edge_content as ec
import orc
from enckit import diagnose as _diagnose


def _first_difference(a, b, w, h):
    for name, pa, pb in zip(("Y", "Cb", "Cr"), ec.planes(a, w, h), ec.planes(b, w, h)):
        if not np.array_equal(pa, pb):
            bad = np.argwhere(pa != pb)
            y, x = bad[0].tolist()
            return "%s differs at %d samples, first (y,x)=(%d,%d): %d vs %d" % (name, len(bad), y, x, pa[y, x], pb[y, x])
    return "equal"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_edge_content_matches_oracle(gpu, case):
    from kvazzup_amd.codec import Decoder, Encoder
    w, h = case["w"], case["h"]
    kw, sets, hip = ec.codec_options(case)
    oe = orc.OracleEncoder(w, h, **kw)
    for name, value in sets:
        oe.set_option(name, value)
    ge = Encoder(w, h, options=hip)
    assert not ge.rejected, ge.rejected
    gd = Decoder()
    try:
        for t in range(case["frames"]):
            frame = ec.frame(case, t)
            au_o = oe.encode(frame)
            au_g, rec_g = ge.encode(frame)
            dbg_o = oe.debug()
            rec_o = oe.recon()
            what = "picture %d (%s)" % (t, "I" if dbg_o["is_intra"] else "P")
            if au_o != au_g or not np.array_equal(rec_g, rec_o):
                pytest.fail("%s: AU %d vs %d bytes, equal=%s; reconstruction: %s; %s" % (
                    what, len(au_o), len(au_g), au_o == au_g, _first_difference(rec_o, rec_g, w, h), _diagnose(dbg_o, ge.debug_all())))
            assert ge.last_bins() == dbg_o["bins"], what
            if case.get("lossless"):
                assert np.array_equal(rec_g, frame), what
            got = gd.decode_au(au_g, t)
            assert len(got) == 1, (what, len(got))
            if not np.array_equal(got[0]["i420"], rec_o):
                pytest.fail("%s: HIP decoder output differs from the reconstruction: %s" % (what, _first_difference(rec_o, got[0]["i420"], w, h)))
    finally:
        ge.close()
        gd.close()
        oe.close()
