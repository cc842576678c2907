"""Reads what "lp-gop"  writes into a stream back out of it, for tests/test_lp_gop_host.py and tests/test_gpu_lp_gop.py: the DPB size
of the SPS and, of every independent slice segment header, the POC, the reference picture set, the active reference count and SliceQpY -- as 7.3.6.1 lays
them out for this encoder's tool set, with tests/pyhevc.py's bit reader and parsers."""
import pyhevc


def sps_dpb(rbsp):
    """sps_max_dec_pic_buffering_minus1 + 1 of the highest sub-layer (pyhevc.parse_sps reads past it)"""
    r = pyhevc.Bits(rbsp)
    r.u(16)
    r.u(4)
    max_sub = r.u(3)
    r.u(1)
    pyhevc.parse_ptl(r, max_sub)
    r.ue()
    assert r.ue() == 1
    r.ue(); r.ue()
    if r.u(1):
        for _ in range(4):
            r.ue()
    r.ue(); r.ue(); r.ue()
    present = r.u(1)
    dpb = None
    for _ in range(0 if present else max_sub, max_sub + 1):
        dpb = r.ue() + 1
        r.ue(); r.ue()
    return dpb


def slice_headers(au, sps, pps):
    """per slice segment NAL unit of the access unit: dict(nal, first, dependent) and, for independent segments, type, poc, rps [(delta, used)],
    rps_in_header, nact, tmvp, qp (SliceQpY)"""
    out = []
    for nal in pyhevc.split_nals(au):
        t = (nal[0] >> 1) & 63
        if t not in (1, 19):
            continue
        idr = t == 19
        r = pyhevc.Bits(pyhevc.unescape(nal)[2:])
        f = {"nal": t, "first": r.u(1), "dependent": 0}
        if idr:
            r.u(1)
        assert r.ue() == 0
        if not f["first"]:
            if pps["dep"]:
                f["dependent"] = r.u(1)
            wc, hc = -(-sps["w"] >> 6), -(-sps["h"] >> 6)
            r.u(max(1, (wc * hc - 1).bit_length()))
        if not f["dependent"]:
            f["type"] = r.ue()
            f["tmvp"] = 0
            f["nact"] = pps["nref_default"]
            f["rps"] = []
            if not idr:
                f["poc"] = r.u(sps["poc_bits"])
                f["rps_in_header"] = not r.u(1)
                n = len(sps["rps"])
                if f["rps_in_header"]:
                    f["rps"] = pyhevc.parse_st_rps(r, n, n, sps["rps"])
                else:
                    f["rps"] = sps["rps"][r.u((n - 1).bit_length()) if n > 1 else 0]
                assert sps["lt"] is None
                if sps["tmvp"]:
                    f["tmvp"] = r.u(1)
            if sps["sao"]:
                assert r.u(2) == 3
            if not idr:
                if r.u(1):
                    f["nact"] = r.ue() + 1
                if f["tmvp"] and f["nact"] > 1:
                    assert r.ue() == 0                              # collocated_ref_idx
                assert r.ue() == 0                                  # five_minus_max_num_merge_cand
            f["qp"] = pps["init_qp"] + r.se()
        out.append(f)
    return out
