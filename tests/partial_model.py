"""Partial pictures v1, the statement of record beside csrc/decoder.h: what the decoder makes of a picture that lost slice segments when it is asked to keep
what arrived (kvzx_decoder_set_partial_pictures).  tests/pyhevc.py decodes segment by segment already (SliceDecoder.run_segment starts at any address, lf_ok is
the one question both loop filters ask); this module wraps it with the rule and holds the loss helper.  The second decoder the HIP decoder is held to with the
option on -- the checker, oracle/, stays at today's behaviour.  Test infrastructure.

The rule (one-tile pictures; total = the picture's coding tree blocks, next = where the decoded part ends so far, 0 at first):
 1. segments are taken in arrival order inside an access unit, a = the segment's address.  a < next: ignored.  Independent: decoded, [next, a) is missing when
    a > next.  Dependent: decoded only if a == next, next > 0 and block a - 1 was decoded; else dropped, next unchanged -- a lost segment takes every following
    dependent one with it, up to the next independent one.  After a decoded segment next = a + the blocks it coded.  The picture ends when next == total or when
    something arrives that can only belong to the next access unit; then [next, total) is missing.  No segment decoded: a lost picture, v2 / v3 as ever.  A segment
    that does not parse is corruption: the exception pyhevc raises goes up as ever.
 2. a non-first segment joins the open picture if nal_unit_type and PPS match (an independent one: its picture order count too) and a >= next; else the open
    picture is closed as damaged and an independent segment opens a picture from its own header, [0, a) missing; a dependent one without a picture is rejected.
 3. a missing block has no coding units, is available to nothing, files no motion, has no edges; its boundary is closed to both loop filters (lf_ok).
 4. its samples: S = v2's choice for the damaged picture's own order count among the reference pictures the DPB held when the picture arrived (stand-ins made for
    this picture excluded; nearest, of two the earlier); an IRAP picture that starts a coded video sequence: the held picture decoded last; none: 128.  Mode 2:
    S's samples at the same place; mode 3: conceal_model's stand-in for (S, the damaged picture's order count) restricted to the missing blocks.
 5. the damaged picture is an ordinary picture: output in its turn, kept as a reference.

Decoder.damage files, per damaged picture in decoding order: poc, cvs, runs [(first block, count)], missing, total, src (S, a pyhevc.Picture; None: grey), src_poc,
src_damaged, disp (mode 3's table, zeros in mode 2), irap, b, leaves (some fetch of a missing block reads outside the coded picture)."""

import numpy as np

import conceal_model as cm
import pyhevc


class _Slice(pyhevc.SliceDecoder):
    """a picture opened by a segment that is not its first: the one step of finish_header_and_decode that cannot be reached by subclassing -- its run_segment(.., 0, 0)"""

    def run_segment(self, data, starts, address, dependent):
        if self.dec._open_at is not None:
            address, self.dec._open_at = self.dec._open_at, None
        return super().run_segment(data, starts, address, dependent)


def runs_of(blocks):
    """sorted block addresses -> [(first, count)]"""
    out = []
    for a in blocks:
        if out and out[-1][0] + out[-1][1] == a:
            out[-1][1] += 1
        else:
            out.append([a, 1])
    return [tuple(r) for r in out]


class Decoder(cm.Decoder):
    def __init__(self, tabs, mode=2):
        super().__init__(tabs)
        self.mode, self.damage, self.next, self.open, self.rejected = mode, [], 0, None, 0
        self._open_at = None

    # ---- v2 / v3 for pictures lost whole, as ever
    def missing_ref(self, sps, poc, is_lt):
        if self.mode == 3:
            return super().missing_ref(sps, poc, is_lt)
        pic = pyhevc.Decoder.missing_ref(self, sps, poc, is_lt)
        pic.stand_in = True
        return pic

    # ---- NAL level: what can only belong to the next access unit closes the picture under way
    def decode_nal(self, nal):
        t = (nal[0] >> 1) & 63
        if self.cur is not None and 32 <= t <= 40 and t != 38:
            self.close_damaged()
        super().decode_nal(nal)

    def flush(self):
        if self.cur is not None:
            self.close_damaged()
        return super().flush()

    def _opened(self, nal_type, pps, sps):
        """a picture is under way: what a further segment must match, and S (rule 4), chosen now"""
        sl = self.cur
        irap = 16 <= nal_type <= 23
        cands = [p for p in self.pre_refs if not getattr(p, "fresh", False)]
        if irap and self.no_rasl_out:
            real = [p for p in cands if not getattr(p, "stand_in", False)]
            src = real[-1] if real else None
        else:
            src = min(cands, key=lambda p: (abs(p.poc - sl.sh["poc"]), p.poc)) if cands else None
        self.open = {"nal_type": nal_type, "pps": pps["id"], "sps": sps, "src": src, "tid": self.tid, "irap": irap}
        self._track()

    def _track(self):
        sl = self.cur
        if sl is not None:
            self.next = max(i for i, s in enumerate(sl.ctb_slice) if s != -1) + 1
            if self.next >= sl.wc * sl.hc:
                self.close_damaged()                               # (it reaches the picture's end with a gap behind it: run_segment counted fewer blocks than the picture has)

    def decode_slice(self, nal, nal_type):
        rbsp = pyhevc.unescape(nal)
        r = pyhevc.Bits(rbsp)
        r.u(16)
        irap, idr = 16 <= nal_type <= 23, nal_type in (19, 20)
        first = r.u(1)
        if irap:
            no_prior = r.u(1)
        pps = self.pps[r.ue()]
        sps = self.sps[pps["sps"]]
        if first or pps["tile_rows"] > 1 or pps["tile_cols"] > 1:
            if first and self.cur is not None:
                self.close_damaged()
            super().decode_slice(nal, nal_type)                    # (a first segment, and pictures with tiles: pyhevc's own way, unchanged)
            if first and self.cur is not None:
                self._opened(nal_type, pps, sps)
            return
        if (nal_type in (8, 9) and self.skip_rasl) or (self.cvs == 0 and not irap):
            return
        dependent = r.u(1) if pps["dep"] else 0
        wc, hc = -(-sps["w"] >> sps["ctb"]), -(-sps["h"] >> sps["ctb"])
        address = r.u(max(1, (wc * hc - 1).bit_length()))
        sh = rps = poc = None
        if not dependent:
            sh, rps, poc = self.slice_header_body(r, sps, pps, nal_type, idr)
        sl = self.cur
        if sl is not None:
            joins = (self.open["nal_type"], self.open["pps"]) == (nal_type, pps["id"]) and (dependent or poc == sl.sh["poc"])
            if joins and address < self.next:
                return                                             # rule 1: a duplicate, or out of order
            if not joins:
                self.close_damaged()
                sl = None
        if sl is None:
            if dependent:
                self.rejected += 1                                 # rule 2: without its picture (the product answers DEC_ERR_INVALID, as ever)
                return
            # rule 2: an independent segment opens a picture from its own header; what a first segment decides (8.1.3, C.5.2.2) is decided here
            self.no_rasl_out = idr or nal_type in (16, 17, 18) or (irap and (self.cvs == 0 or self.after_eos))
            if irap:
                self.skip_rasl = self.no_rasl_out
                self.drop_prior = bool(no_prior) and nal_type != 21 and self.cvs > 0 and not self.after_eos
            self.skipping = False
            self._open_at, keep = address, pyhevc.SliceDecoder
            pyhevc.SliceDecoder = _Slice
            try:
                self.finish_header_and_decode(r, rbsp, nal, nal_type, idr, 1, 0, 0, sps, pps, sh, rps, poc)
            finally:
                pyhevc.SliceDecoder, self._open_at = keep, None
            if self.cur is not None:
                self._opened(nal_type, pps, sps)
            return
        if dependent:
            if not (address == self.next and self.next > 0 and sl.ctb_slice[address - 1] != -1):
                return                                             # rule 1: its predecessor is gone
            sh, poc = dict(sl.sh), sl.sh["poc"]
        self.finish_header_and_decode(r, rbsp, nal, nal_type, idr, 0, dependent, address, sps, pps, sh, rps, poc)
        self._track()

    # ---- rules 3-5
    def close_damaged(self):
        sl, op = self.cur, self.open
        total = sl.wc * sl.hc
        missing = [a for a in range(total) if sl.ctb_slice[a] == -1]
        sps, poc = op["sps"], sl.sh["poc"]
        tid, self.tid = self.tid, op["tid"]
        try:
            if not missing:
                self.picture_done(sl, sps, op["nal_type"])
                return
            miss, log2, wc, whole = set(missing), sl.ctb_log2, sl.wc, sl.lf_ok

            def lf_ok(xq, yq, xp, yp):
                cq, cp = (yq >> log2) * wc + (xq >> log2), (yp >> log2) * wc + (xp >> log2)
                return False if cq != cp and (cq in miss or cp in miss) else whole(xq, yq, xp, yp)
            sl.lf_ok = lf_ok
            sl.loop_filters()
            src = op["src"]
            disp = np.zeros(((sl.h + 15) // 16, (sl.w + 15) // 16, 4), np.int16)
            moved = None
            if src is not None:
                moved = [pl for pl in src.planes]
                if self.mode == 3 and not getattr(src, "stand_in", False):
                    moved, disp = cm.stand_in(src, poc)
            for a in missing:
                cx, cy = a % wc, a // wc
                for c, pl in enumerate(sl.pic.planes):
                    s = sl.ctb >> (1 if c else 0)
                    y0, x0 = cy * s, cx * s
                    pl[y0:y0 + s, x0:x0 + s] = 128 if moved is None else moved[c][y0:y0 + s, x0:x0 + s]
            sl.pic.damaged = True
            self.damage.append({"poc": poc, "cvs": self.cvs, "runs": runs_of(missing), "missing": len(missing), "total": total, "au": getattr(self, "au", None),
                                "src": src, "src_poc": None if src is None else src.poc, "src_damaged": bool(getattr(src, "damaged", False)), "disp": disp,
                                "irap": op["irap"], "b": bool(sl.sh["b"]),
                                "leaves": False if moved is None else fetch_leaves(disp, missing, sl)})
            self.picture_done(sl, sps, op["nal_type"], filtered=True)
        finally:
            self.tid = tid
            self.cur = None


def fetch_leaves(disp, missing, sl):
    """does some fetch of a missing block read outside the coded picture (and get clamped)?"""
    per = sl.ctb >> 4
    for a in missing:
        cx, cy = a % sl.wc, a // sl.wc
        for by in range(cy * per, min((cy + 1) * per, disp.shape[0])):
            for bx in range(cx * per, min((cx + 1) * per, disp.shape[1])):
                dx, dy = int(disp[by, bx, 0]), int(disp[by, bx, 1])
                if bx * 16 + dx < 0 or by * 16 + dy < 0 or bx * 16 + 15 + dx >= sl.w or by * 16 + 15 + dy >= sl.h:
                    return True
    return False


def decode(aus, tabs, mode=2):
    """the access units (what arrived of them) through the model: (pictures in output order, the decoder)"""
    d = Decoder(tabs, mode)
    for d.au, au in enumerate(aus):
        for nal in pyhevc.split_nals(au):
            d.decode_nal(nal)
    return d.flush(), d


# ---- the loss helper: which NAL units of a stream never arrive
def vcl_indices(au):
    return [k for k, n in enumerate(pyhevc.split_nals(au)) if ((n[0] >> 1) & 63) < 32]


def cut(aus, lost):
    """lost: {access unit: the VCL NAL units of it that are lost, counted from 0 among its VCL units}; an access unit that keeps no VCL unit is lost whole.
    -> [(index, what arrives of the access unit)]"""
    out = []
    for t, au in enumerate(aus):
        nals, gone = pyhevc.split_nals(au), lost.get(t, ())
        vcl = vcl_indices(au)
        if gone and len(set(gone)) >= len(vcl):
            continue
        drop = {vcl[k] for k in gone}
        out.append((t, b"".join(b"\x00\x00\x00\x01" + bytes(n) for k, n in enumerate(nals) if k not in drop)))
    return out


def segment_table(aus):
    """per access unit its VCL NAL units as (first_slice_segment_in_pic_flag, dependent_slice_segment_flag, slice_segment_address)"""
    sps, pps, out = {}, {}, []
    for au in aus:
        row = []
        for n in pyhevc.split_nals(au):
            t = (n[0] >> 1) & 63
            if t == 33:
                s = pyhevc.parse_sps(pyhevc.unescape(n)); sps[s["id"]] = s
            elif t == 34:
                p = pyhevc.parse_pps(pyhevc.unescape(n)); pps[p["id"]] = p
            elif t < 32:
                r = pyhevc.Bits(pyhevc.unescape(n)); r.u(16)
                first = r.u(1)
                if 16 <= t <= 23:
                    r.u(1)
                p = pps[r.ue()]; s = sps[p["sps"]]
                dep = addr = 0
                if not first:
                    dep = r.u(1) if p["dep"] else 0
                    wc, hc = -(-s["w"] >> s["ctb"]), -(-s["h"] >> s["ctb"])
                    addr = r.u(max(1, (wc * hc - 1).bit_length()))
                row.append((first, dep, addr))
        out.append(row)
    return out
