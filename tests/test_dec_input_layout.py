"""The decoder's input block (kvazzup_amd/csrc/dec_frame.h DecInputLayout) against a restatement of the formulas it replaced.

Before the layout had one statement the fixed part was a chain of members of the decoder (decoder.h):

    off_region()  = (pw / 4) * (ph / 4) * sizeof(B4Rec)
    off_ctu()     = off_region() + (pw / 32) * (ph / 32) * sizeof(TuRange)
    nctb()        = (pw >> ctbl) * (ph >> ctbl)
    off_tile()    = off_ctu() + nctb() * sizeof(TuRange)
    off_sao()     = (off_tile() + nctb() + 15) & ~15
    off_scaling() = (off_sao() + nctb() * sizeof(SaoParams) + 63) & ~63
    off_wt()      = (off_scaling() + KVZ_SCALING_BYTES + 63) & ~63
    off_frame()   = (off_wt() + 32 * sizeof(DecWt) + 63) & ~63
    off_nb()      = (off_frame() + sizeof(DecFrame) + 15) & ~15
    fixed_bytes() = (off_nb() + nctb() + 15) & ~15

and the variable part was spelled out by the uploader (decoder.hip launch_gpu; the parser and the probe had copies):

    tu_off  = fixed_bytes()
    lev_off = (tu_off + ntu * sizeof(DecTu) + 15) & ~15
    x_off   = (lev_off + nlev * sizeof(uint32_t) + 15) & ~15
    i_off   = (x_off + (bi ? b4x.size() * sizeof(B4L1) : 0) + 15) & ~15
    bytes   = ctbl < 6 ? i_off + ntu * sizeof(uint32_t) : (bi ? x_off + b4x.size() * sizeof(B4L1) : lev_off + nlev * sizeof(uint32_t))

The struct sizes come from the host library, not from this file."""
import pytest

import hc

SIZES = [(64, 64), (192, 128), (1920, 1088), (3840, 2176)]
COUNTS = [(0, 0, 0), (1, 1, 1), (7, 13, 5), (40000, 160000, 9000)]


def up(v, a):
    return (v + a - 1) & ~(a - 1)


def restated(pw, ph, ctbl, ntu, nlev, nb4x, bi, z):
    o = {}
    o["region"] = (pw // 4) * (ph // 4) * z["B4Rec"]
    o["ctu"] = o["region"] + (pw // 32) * (ph // 32) * z["TuRange"]
    nctb = (pw >> ctbl) * (ph >> ctbl)
    o["tile"] = o["ctu"] + nctb * z["TuRange"]
    o["sao"] = up(o["tile"] + nctb, 16)
    o["scaling"] = up(o["sao"] + nctb * z["SaoParams"], 64)
    o["wt"] = up(o["scaling"] + z["scaling"], 64)
    o["frame"] = up(o["wt"] + 32 * z["DecWt"], 64)
    o["nb"] = up(o["frame"] + z["DecFrame"], 16)
    fixed = up(o["nb"] + nctb, 16)
    o["tus"] = fixed
    o["lev"] = up(o["tus"] + ntu * z["DecTu"], 16)
    o["b4x"] = up(o["lev"] + nlev * 4, 16)
    o["index"] = up(o["b4x"] + (nb4x * z["B4L1"] if bi else 0), 16)
    nbytes = o["index"] + ntu * 4 if ctbl < 6 else (o["b4x"] + nb4x * z["B4L1"] if bi else o["lev"] + nlev * 4)
    # what every part holds and the alignment it is placed on (1: packed behind its predecessor)
    parts = [("records", 0, o["region"], 1), ("region", o["region"], (pw // 32) * (ph // 32) * z["TuRange"], 1), ("ctu", o["ctu"], nctb * z["TuRange"], 1),
             ("tile", o["tile"], nctb, 1), ("sao", o["sao"], nctb * z["SaoParams"], 16), ("scaling", o["scaling"], z["scaling"], 64),
             ("wt", o["wt"], 32 * z["DecWt"], 64), ("frame", o["frame"], z["DecFrame"], 64), ("nb", o["nb"], nctb, 16),
             ("tus", o["tus"], ntu * z["DecTu"], 16), ("lev", o["lev"], nlev * 4, 16), ("b4x", o["b4x"], nb4x * z["B4L1"] if bi else 0, 16),
             ("index", o["index"], ntu * 4 if ctbl < 6 else 0, 16)]
    return o, fixed, nbytes, parts


@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "%d-%d-%d" % c)
@pytest.mark.parametrize("ctbl", [4, 5, 6])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_layout_is_the_restatement(size, ctbl, counts, bi):
    (pw, ph), (ntu, nlev, nb4x) = size, counts
    got, fixed, nbytes, z = hc.input_layout(pw, ph, ctbl, ntu, nlev, nb4x, bi)
    want, want_fixed, want_bytes, parts = restated(pw, ph, ctbl, ntu, nlev, nb4x, bi, z)
    assert got == want
    assert fixed == want_fixed
    assert nbytes == want_bytes
    end = 0
    for name, off, size_, align in parts:
        at = 0 if name == "records" else got[name]
        assert at == off and at % align == 0, (name, at, off, align)
        assert at >= end, "%s at %d begins inside its predecessor, which ends at %d" % (name, at, end)
        end = at + size_
        assert end <= nbytes or size_ == 0, "%s ends at %d, the upload at %d" % (name, end, nbytes)
    last = max(off + n for _, off, n, _ in parts if n)
    assert 0 <= nbytes - last < 16, "the upload (%d bytes) ends with the last part present (%d), rounded up to 16 at the most" % (nbytes, last)
