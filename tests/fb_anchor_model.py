""""uvgx loss feedback v2" (kvazaar.h fb_anchor): the statement of record, on top of tests/fb_model.py (v1, which stays as it is).  The device
and host arithmetic (the fb_anchor_* functions of kvazzup_amd/csrc/hevc_core.h, the reference-bit kernels of fb_kernels.hip, the header writers of hevc_headers.h)
is held to this file by tests/test_fb_anchor_host.py and tests/test_gpu_fb_anchor.py.

K = fb-anchor: the encoder and every decoder keep the K pictures before the current one.  H = loss-feedback.  POCs count from the last IDR picture (POC 0).  A
v2 heal picture t has two references: index 0 = picture t - 1, index 1 = the ANCHOR a, da = t - a pictures back.  A RECORD here is (mv, intra, log2, ref): v1's
record and per cell the reference index of its vector."""
import numpy as np

import fb_model as M
import pyhevc

# ---- A.4.2: the decoded picture buffer
MAX_LUMA_PS = {123: 2228224, 153: 8912896, 183: 35651584}      # level 4.1, 5.1, 6.1 (Table A.8): the levels the encoder writes


def level_idc(cw, ch):
    """the level the stream states for its coded size (hevc_headers.h level_idc_for)"""
    px = cw * ch
    return 123 if px <= 2228224 else 153 if px <= 8912896 else 183


def max_dpb_size(cw, ch):
    """MaxDpbSize (A-2) with maxDpbPicBuf = 6"""
    px, ps = cw * ch, MAX_LUMA_PS[level_idc(cw, ch)]
    if px <= ps >> 2:
        return 16
    if px <= ps >> 1:
        return 12
    if px <= (3 * ps) >> 2:
        return 8
    return 6


def k_allowed(cw, ch, K, H):
    """what encoder_open takes: the K kept pictures and the current one fit the buffer, and a report the anchor answers lies within the ring of H records"""
    return K == 0 or (2 <= K <= 7 and 1 <= H and K <= H and K + 1 <= max_dpb_size(cw, ch))


# ---- the anchor
def anchor(c, pending, t, K, H):
    """the anchor's POC of heal picture t, or None: v1's heal picture.  c: the POC of the most recent IDR or heal picture; pending: the POCs of the reports
    pending when picture t is planned"""
    n0 = min(pending)
    a = n0 - 1
    if K >= 2 and a >= c and a >= 0 and t - a <= K and all(t - n <= H for n in pending):
        return a
    return None


def rps(t, K, a=None):
    """P picture t's reference picture set [(delta POC, used by the picture)]: min(K, t) pictures, each one further back; t - 1 is used, and the anchor"""
    return [(-j, int(j == 1 or (a is not None and t - j == a))) for j in range(1, min(K, t) + 1)]


def active_refs(a):
    return 1 if a is None else 2


# ---- later reports stepping through a v2 heal picture's record
REF1 = 0x10      # the record's info byte: the cell's vector refers to reference 1


def step(prev, record, cw, ch, filt, anchor_bad):
    """D_(k-1) -> D_k through picture k's record (mv, intra, log2, ref).  A reference-1 cell read picture k's anchor: it is in S where the report names a picture
    at or before that anchor (anchor_bad) and never otherwise; every other cell is v1's"""
    gh, gw = ch // 8, cw // 8
    mv, intra, log2, ref = record
    s = np.zeros((gh, gw), dtype=np.uint8)
    for cy in range(gh):
        for cx in range(gw):
            if intra[cy, cx]:
                continue
            if ref[cy, cx]:
                s[cy, cx] = 1 if anchor_bad else 0
            elif M.inter_reads(prev, cw, ch, cx, cy, mv[cy, cx, 0], mv[cy, cx, 1]):
                s[cy, cx] = 1
    cells = [(int(cy), int(cx)) for cy, cx in np.argwhere(np.asarray(intra) != 0)]
    changed = bool(s.any())
    while changed:
        changed = False
        for cy, cx in cells:
            if not s[cy, cx] and M.intra_reads(s, cw, ch, cx, cy, log2[cy, cx]):
                s[cy, cx] = 1
                changed = True
    return M.dilate(s) if filt else s


def heal_map(cw, ch, records, anchors, reports, t, H, filt):
    """D' of heal picture t as fb_model.heal_map, with records = {poc: (mv, intra, log2, ref)} and anchors = {poc: anchor POC} of the v2 heal pictures among them"""
    gh, gw = ch // 8, cw // 8
    oldest = min(r[0] for r in reports)
    if t - oldest > H:
        return np.ones((gh, gw), dtype=np.uint8)
    d = np.zeros((gh, gw), dtype=np.uint8)
    for k in range(oldest, t):
        if k > oldest:
            d = step(d, records[k], cw, ch, filt, k in anchors and oldest <= anchors[k])
        d |= M.seed(cw, ch, [(f, c) for n, f, c in reports if n == k], filt)
    return d


# ---- what a v2 heal picture's cells may be (the map and the block records are v1's: fb_model.block_records)
def cell_allowed(forced, intra, ref, mv, code):
    """a forced quarter's cell is an intra unit (the ordinary gate) or refers to the anchor; a free quarter's cell is an intra unit or refers to the previous picture
    with its vector within the block's reach"""
    if intra:
        return True
    return ref == 1 if forced else (ref == 0 and M.vector_within(mv, code))


# ---- reading what a stream says (tests/pyhevc.py)
def sps_dpb(nal):
    """sps_max_dec_pic_buffering_minus1 of an SPS NAL unit"""
    r = pyhevc.Bits(pyhevc.unescape(nal))
    r.u(16)
    r.u(4)
    max_sub = r.u(3)
    r.u(1)
    pyhevc.parse_ptl(r, max_sub)
    r.ue(), r.ue(), r.ue(), r.ue()                     # id, chroma format, width, height
    if r.u(1):
        r.ue(), r.ue(), r.ue(), r.ue()
    r.ue(), r.ue(), r.ue()                             # bit depths, log2_max_poc_lsb - 4
    r.u(1)
    return r.ue()


class Headers:
    """the parameter sets and slice segment headers of a stream's access units, one call each"""
    def __init__(self):
        self.sps, self.pps, self.dpb = None, None, None
        self.dec = pyhevc.Decoder(None)
        self.data = b""      # the slice data of the segment read last: the RBSP behind its header (entry points and alignment included in the header)

    def read(self, au):
        """-> (slice header dict, the picture's set [(delta, used)], POC, IDR picture?) of the access unit's first slice segment"""
        for nal in pyhevc.split_nals(au):
            t = (nal[0] >> 1) & 63
            if t == 33:
                self.sps, self.dpb = pyhevc.parse_sps(pyhevc.unescape(nal)), sps_dpb(nal)
            elif t == 34:
                self.pps = pyhevc.parse_pps(pyhevc.unescape(nal))
            elif t <= 21:
                r = pyhevc.Bits(pyhevc.unescape(nal))
                r.u(16)
                assert r.u(1) == 1
                idr = t in (19, 20)
                if 16 <= t <= 23:
                    r.u(1)
                r.ue()
                self.dec.no_rasl_out = idr
                sh, rps_, poc = self.dec.slice_header_body(r, self.sps, self.pps, t, idr)
                if self.pps["tiles"] or self.pps["wpp"]:
                    n = r.ue()
                    if n:
                        ln = r.ue() + 1
                        r.u(ln * n)
                assert not self.pps["sh_ext"]
                r.u(1)
                r.align()
                self.data = pyhevc.unescape(nal)[r.pos >> 3:]
                if not idr:
                    self.dec.prev_poc_tid0 = poc
                else:
                    self.dec.prev_poc_tid0 = 0
                return sh, rps_, poc, idr
        raise ValueError("no slice segment in the access unit")
