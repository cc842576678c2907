"""The edge-content patterns (tests/edge_content.py) on the CPU: the checker's closed loop on every case the GPU file runs,
and checks that each pattern still reaches the bound it was written for -- so that a later edit cannot quietly turn one
into harmless content."""
import functools

import numpy as np
import pytest

import edge_content as ec
import orc

BY_ID = {ec.case_id(c): c for c in ec.CASES}


@functools.lru_cache(maxsize=None)
def _oracle_run(cid):
    """the checker's encoder and decoder on one case: per picture (source, encoder debug, reconstruction, decoded pictures)"""
    c = BY_ID[cid]
    w, h = c["w"], c["h"]
    kw, sets, _ = ec.codec_options(c)
    oe = orc.OracleEncoder(w, h, **kw)
    for name, value in sets:
        oe.set_option(name, value)
    od = orc.OracleDecoder()
    out = []
    for t in range(c["frames"]):
        src = ec.frame(c, t)
        au = oe.encode(src)
        out.append((src, oe.debug(), oe.recon(), [f["i420"] for f in od.decode_au(au, t)]))
    oe.close()
    od.close()
    return out


def _run(cid):
    assert cid in BY_ID, "%s is no longer in the case matrix" % cid
    return _oracle_run(cid)


@pytest.mark.parametrize("cid", list(BY_ID))
def test_checker_closed_loop(cid):
    """the checker's decoder returns exactly the checker encoder's reconstruction, picture by picture: a GPU mismatch on
    this content is the HIP code's, not the reference's"""
    c = BY_ID[cid]
    for t, (src, dbg, rec, dec) in enumerate(_run(cid)):
        assert len(dec) == 1 and np.array_equal(dec[0], rec), t
        if c.get("lossless"):
            assert np.array_equal(rec, src), t


def test_patterns_are_deterministic_i420():
    for name, f in ec.PATTERNS.items():
        for w, h in ((256, 192), (130, 70)):
            a = f(w, h, 1, ec.SEED)
            assert a.dtype == np.uint8 and a.shape == (w * h + 2 * (w // 2) * (h // 2),), name
            assert np.array_equal(a, f(w, h, 1, ec.SEED)), name


@pytest.mark.parametrize("name", ec.FULL_RANGE)
def test_every_plane_holds_0_and_255(name):
    w, h = (130, 70) if name == "edge_column" else (256, 192)
    pics = [ec.planes(ec.PATTERNS[name](w, h, t, ec.SEED), w, h) for t in range(3)]
    for p in range(3):
        vals = np.concatenate([pic[p].reshape(-1) for pic in pics])
        assert vals.min() == 0 and vals.max() == 255, (name, "YUV"[p])


def test_chroma_is_full_range_or_flat():
    w, h = 256, 192
    for name in ("checker", "hard_edges", "near_black", "binary_noise"):
        y, cb, cr = ec.planes(ec.PATTERNS[name](w, h, 2, ec.SEED), w, h)
        assert np.array_equal(cr.astype(int), 255 - cb.astype(int)), name
    for name in ("checker_flat_chroma", "hard_edges_flat_chroma"):
        full = ec.PATTERNS[name[:-len("_flat_chroma")]](w, h, 2, ec.SEED)
        flat = ec.PATTERNS[name](w, h, 2, ec.SEED)
        assert np.array_equal(flat[:w * h], full[:w * h]) and (flat[w * h:] == 128).all(), name


def test_near_black_and_near_white_stay_near():
    w, h = 256, 192
    for t in range(4):
        yb, cbb, crb = ec.planes(ec.near_black(w, h, t, ec.SEED), w, h)
        yw, cbw, crw = ec.planes(ec.near_white(w, h, t, ec.SEED), w, h)
        assert yb.max() <= 12 and cbb.max() <= 12 and crb.min() >= 243
        assert yw.min() >= 243 and cbw.min() >= 243 and crw.max() <= 12
        assert yb.min() == 0 and yw.max() == 255


@pytest.mark.parametrize("cid", ["cut_black_white_256x192_qp0", "cut_white_black_256x192_qp0"])
def test_cut_p_pictures_are_all_inter_with_full_residual(cid):
    """every P picture of the cut is coded inter against a reference that is exactly the other extreme: the residual is
    ±255 at every sample, each 16x16 quarter's SAD is 65280 for every candidate (all tie), and every unit codes it"""
    c = BY_ID[cid]
    w, h = c["w"], c["h"]
    run = _run(cid)
    for t in range(1, c["frames"]):
        src, dbg, rec, _ = run[t]
        ref = run[t - 1][2]
        assert not dbg["is_intra"] and (dbg["cu_intra"] == 0).all(), t
        diff = src.astype(int) - ref.astype(int)
        assert (np.abs(diff) == 255).all() and len(np.unique(np.sign(diff[:w * h]))) == 1, t
        sad = np.abs(diff[:w * h]).reshape(h // 16, 16, w // 16, 16).sum(axis=(1, 3))
        assert (sad == 65280).all(), t
        assert (dbg["cu_cbf"] == 7).all(), t
    signs = {int(np.sign(run[t][0][0].astype(int) - run[t - 1][2][0].astype(int))) for t in range(1, c["frames"])}
    assert signs == {-1, 1}          # both +255 and -255 (the byte split's high byte -1)


@pytest.mark.parametrize("cid", ["cut_black_white_256x192_qp32_intra_in_p2", "cut_black_white_256x192_qp51_intra_in_p2"])
def test_cut_with_intra_in_p_codes_intra_units(cid):
    for t, (src, dbg, rec, _) in enumerate(_run(cid)):
        if t:
            assert not dbg["is_intra"] and dbg["cu_intra"].any(), t


def test_checker_energy_sits_at_the_highest_frequency():
    """at QP 0 the checkerboard's I picture puts its largest coefficients at the last position of the transform blocks"""
    src, dbg, rec, _ = _run("checker_256x192_qp0")[0]
    for plane, n in ((0, 8), (1, 4), (2, 4)):
        co = np.abs(dbg["coef%d" % plane].astype(int))
        hh, ww = co.shape
        folded = co.reshape(hh // n, n, ww // n, n).sum(axis=(0, 2))
        assert folded.argmax() == n * n - 1, plane


def test_binary_noise_at_qp0_has_large_levels():
    """dense full-range residual at QP 0: levels far past the Rice escape (the longest coeff_abs_level_remaining codes)"""
    for t, (src, dbg, rec, _) in enumerate(_run("binary_noise_256x192_qp0")):
        assert np.abs(dbg["coef0"].astype(int)).max() > 1000, t
        if t:
            assert not dbg["is_intra"]


@pytest.mark.parametrize("cid", ["near_black_256x192_qp51", "near_black_256x192_qp51_sao1_subme4"])
def test_near_black_reconstruction_reaches_0(cid):
    for t, (src, dbg, rec, _) in enumerate(_run(cid)):
        for p, plane in enumerate(ec.planes(rec, 256, 192)[:2]):
            assert plane.min() == 0, (t, p)


@pytest.mark.parametrize("cid", ["near_white_256x192_qp51", "near_white_256x192_qp51_sao1_subme4"])
def test_near_white_reconstruction_reaches_255(cid):
    for t, (src, dbg, rec, _) in enumerate(_run(cid)):
        for p, plane in enumerate(ec.planes(rec, 256, 192)[:2]):
            assert plane.max() == 255, (t, p)


def test_cut_reconstruction_at_qp51_reaches_0():
    """the flat black I picture at QP 51 reconstructs to a ripple around 0: its troughs are clipped"""
    src, dbg, rec, _ = _run("cut_black_white_256x192_qp51")[0]
    y = rec[:256 * 192]
    assert src[:256 * 192].max() == 0 and y.min() == 0 and y.max() > 0


@pytest.mark.parametrize("cid", ["hard_edges_256x192_qp32", "hard_edges_256x192_qp32_sao1_subme4", "hard_edges_256x192_qp51_sao1_subme4"])
def test_hard_edges_use_fractional_chroma_vectors(cid):
    """3 luma samples per picture is 1.5 chroma samples: inter units whose chroma prediction is the 4-tap filter over 0/255 steps"""
    for t, (src, dbg, rec, _) in enumerate(_run(cid)):
        if t:
            inter = dbg["cu_intra"] == 0
            assert (dbg["cu_mv"][inter][:, 0] % 8 != 0).any(), t


def test_hard_edges_with_subme_at_qp51_use_quarter_sample_luma_vectors():
    run = _run("hard_edges_256x192_qp51_sao1_subme4")
    assert any((dbg["cu_mv"][dbg["cu_intra"] == 0] % 4 != 0).any() for _, dbg, _, _ in run[1:])


@pytest.mark.parametrize("cid", ["edge_column_130x70_qp32", "edge_column_702x394_qp51"])
def test_edge_column_is_padded_into_the_coded_area(cid):
    c = BY_ID[cid]
    src, dbg, rec, _ = _run(cid)[0]
    assert dbg["coded_w"] > c["w"] and dbg["coded_h"] > c["h"]
    y = ec.planes(src, c["w"], c["h"])[0]
    assert (y[:, -1] == 255).all() and (y[-1, :] == 255).all() and y[:-1, :-1].max() == 0


def test_half_checker_ctu_variances_span_their_range():
    y = ec.planes(ec.half_checker(256, 192, 0, ec.SEED), 256, 192)[0].astype(float)
    var = y.reshape(3, 64, 4, 64).var(axis=(1, 3))
    assert var.max() >= 255.0 ** 2 / 4 and var.min() == 0
    assert "half_checker_256x192_qp32_vaq8" in BY_ID


def test_1080p_cut_codes_32x32_transforms():
    """the whole-picture 1080p case: the cut's P picture is all 32x32 units with a residual in every plane (the MFMA 32x32 transform)"""
    run = _run("cut_then_noise_1920x1080_qp22")
    dbg = run[1][1]
    assert not dbg["is_intra"] and (dbg["cu_log2"] == 5).all() and (dbg["cu_cbf"] == 7).all()
    assert np.abs(dbg["coef0"].astype(int)).max() > 1000
