"""ctypes bindings of tests/hostcheck, the one host build of the product's serial code (hevc_core.h, hevc_headers.h, entropy_host.h): lib() is the only loader,
and the wrappers the CPU tests of the encoder options share live here.  Test infrastructure."""
import ctypes as C
import fcntl
import os
import subprocess
import numpy as np

import pyhevc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


class HcFrame(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("cw", "ch", "width", "height", "qp", "is_intra", "poc", "wpp", "deblock", "fps_num", "fps_den", "write_ps")] + \
               [(n, C.c_void_p) for n in ("cu_log2", "cu_intra", "cu_flags", "cu_merge_idx", "cu_mvp_idx", "cu_intra_mode", "cu_cbf", "cu_mv", "cu_mvd")] + \
               [("coef", C.c_void_p * 3)]


class AccessUnit(C.Structure):
    """hostcheck/syntax.cpp HcAccessUnit"""
    _fields_ = [(n, C.c_int32) for n in ("w", "h", "lp_refs", "tmvp", "sao", "wpp", "tile_rows", "tile_cols", "slices", "weightp", "poc", "qp_delta", "write_ps", "nrefs")] + \
               [("dist", C.c_int8 * 4), ("wts", C.c_void_p), ("recovery", C.c_int32), ("payload", C.c_void_p), ("payload_len", C.c_int32)]


def _declare(L):
    I, P, U64, I64, D, LONG = C.c_int, C.c_void_p, C.c_uint64, C.c_int64, C.c_double, C.c_long
    sig = {
        # hostcheck.cpp
        "hc_table": (I, [I, P]), "hc_inter_signal": (None, [P]), "hc_encode_au": (I, [P, P, I, P]), "hc_encode_au_tokens": (I, [P, P, I, P]),
        "hc_intra_uses": (U64, [I, I, I]), "hc_intra_predict": (None, [P, P, I, I, I, P]), "hc_deblock": (None, [P] * 4),
        "hc_quant": (I, [I] * 4), "hc_dequant": (I, [I] * 3), "hc_mvd_bits": (I, [I]),
        "hc_bench_play_tokens": (D, [P, LONG, I, I]), "hc_picture_tokens": (LONG, [P, P, LONG]),
        # syntax.cpp
        "hr_header": (I, [I] * 4 + [P, I]), "hi_recovery_sei": (I, [I, P, I]), "hc_access_unit": (I, [P, P, I]),
        # motion.cpp
        "hc_cands": (None, [I] * 5 + [P] * 6 + [C.c_uint32] + [I] * 3 + [P] * 3), "ht_picture": (None, [I] * 5 + [P] * 6 + [P] * 5),
        "hr_ref_idx_tokens": (I, [I, I, P, I]),
        # statements.cpp
        "hc_quarter": (None, [P, I, I, P]), "hc_coarse": (None, [P, P] + [I] * 7 + [P]), "hc_fine": (None, [P, P, P] + [I] * 10 + [P] * 4),
        "hw_moments": (None, [U64] * 3 + [P]), "hw_isqrt": (C.c_uint32, [U64]), "hw_candidate": (None, [I64] * 4 + [P]), "hw_accept": (I, [I, U64, U64]),
        "hw_sample": (I, [I] * 3), "hw_pred14": (I, [I] * 3), "hw_decide": (None, [P, P, I, I, I, P]),
        "hi_step": (I, [I, I]), "hi_cycle": (I, [I, I]), "hi_band": (None, [I] * 3 + [P]), "hi_position": (I, [I] * 3), "hi_forced_quarters": (I, [I] * 3),
        "hi_clean_block": (I, [I] * 3), "hi_mvx_max": (I, [I, I]), "hi_last_column": (I, [I] * 4), "hi_schedules": (None, [I, P]), "hi_bands": (I, [I, I, P]),
        "hd_input_layout": (None, [I] * 3 + [U64] * 3 + [I, P, P]), "he_layout": (None, [I] * 3 + [P]),
        # coder.cpp
        "hcr_play": (I, [I, P, P, P, I, P, P, I, P, P]), "hcr_code_picture": (I, [I, I, P, P, P] + [I] * 7 + [P, I, P, I, P]),
        "hcr_code_band": (I, [I, I, P, P, P] + [I] * 8 + [P, I, P, I, P]), "hcr_bench": (D, [P, LONG, I, I, I]),
        # order.cpp
        "ho_new": (P, []), "ho_free": (None, [P]), "ho_submitted": (U64, [P] + [I] * 5 + [P, I, P]), "ho_mark": (None, [P]), "ho_restore": (None, [P]), "ho_discarded": (I, [P, U64]),
        "ho_sequence_ended": (None, [P]), "ho_idle": (I, [P]), "ho_completed": (None, [P, U64] + [I] * 4), "ho_next": (I, [P, I, P]), "ho_drain": (None, [P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args


def lib():
    """the one host library of the tests: built (under a lock: pytest -n workers reach this at once, and a half-linked library must not be loaded) and loaded once"""
    global _LIB
    if _LIB is None:
        d = os.path.join(ROOT, "tests", "hostcheck")
        with open(os.path.join(d, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.run(["make", "-s", "-C", d], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(d, "build", "libhostcheck.so"))
        _declare(L)
        _LIB = L
    return _LIB


def make_frame(dbg, width, height, qp, wpp=1, deblock=1, fps=(30, 1), write_ps=1):
    """dbg: dict of numpy arrays as produced by orc.OracleEncoder.debug(); arrays are kept alive in the returned holder"""
    hold = {k: np.ascontiguousarray(v).copy() for k, v in dbg.items() if isinstance(v, np.ndarray)}
    if "cu_mvd" not in hold:
        hold["cu_mvd"] = np.zeros_like(hold["cu_mv"])
    f = HcFrame()
    f.cw, f.ch, f.width, f.height, f.qp = dbg["coded_w"], dbg["coded_h"], width, height, qp
    f.is_intra, f.poc, f.wpp, f.deblock, f.fps_num, f.fps_den, f.write_ps = dbg["is_intra"], dbg["poc"], wpp, deblock, fps[0], fps[1], write_ps
    for n in ("cu_log2", "cu_intra", "cu_flags", "cu_merge_idx", "cu_mvp_idx", "cu_intra_mode", "cu_cbf", "cu_mv", "cu_mvd"):
        setattr(f, n, hold[n].ctypes.data)
    for c in range(3):
        f.coef[c] = hold["coef%d" % c].ctypes.data
    return f, hold


def encode_au(f):
    out = np.empty(f.cw * f.ch * 3 + (1 << 16), dtype=np.uint8)
    bins = C.c_ulonglong()
    n = lib().hc_encode_au(C.byref(f), out.ctypes.data, len(out), C.byref(bins))
    assert n > 0, "hc_encode_au: %d" % n
    return bytes(out[:n]), bins.value


def encode_au_tokens(f):
    out = np.empty(f.cw * f.ch * 3 + (1 << 16), dtype=np.uint8)
    nt = C.c_ulonglong()
    n = lib().hc_encode_au_tokens(C.byref(f), out.ctypes.data, len(out), C.byref(nt))
    assert n > 0, "hc_encode_au_tokens: %d" % n
    return bytes(out[:n]), nt.value


# ---- syntax (hostcheck/syntax.cpp)
def header(which, n, poc=0, sao=0):
    """the bare RBSP of the VPS (0), SPS (1), PPS (2) or the slice segment header of picture `poc` (3) with lp-refs n"""
    buf = np.zeros(512, np.uint8)
    k = lib().hr_header(which, n, poc, sao, buf.ctypes.data, len(buf))
    assert k > 0, "hr_header(%d, %d, %d, %d): %d" % (which, n, poc, sao, k)
    return bytes(buf[:k])


def recovery_sei(cnt):
    """the RBSP of the recovery point SEI with recovery_poc_cnt `cnt`"""
    buf = np.zeros(64, np.uint8)
    n = lib().hi_recovery_sei(cnt, buf.ctypes.data, len(buf))
    assert n > 0, "hi_recovery_sei(%d): %d" % (cnt, n)
    return bytes(buf[:n])


def access_unit(w, h, poc, lp=0, tmvp=0, sao=0, wpp=1, tr=1, tc=1, slices=0, weightp=0, qp_delta=0, write_ps=1, dists=(), wts=None, recovery=-1, payload=b""):
    """The access unit of picture `poc` (0: the IDR picture) as assemble_access_unit writes it.  dists: lp-gop's references (none: no PicRefs handed over);
    wts: weightp's [reference](flag, w, o) (None: no PicWeights); recovery: the SEI's recovery_poc_cnt (-1: no SEI); payload: the one substream (wpp 0, one
    tile), else a 2-byte placeholder per substream."""
    a = AccessUnit(w, h, lp, tmvp, sao, wpp, tr, tc, slices, weightp, poc, qp_delta, write_ps, len(dists))
    a.dist[:] = list(dists) + [0] * (4 - len(dists))
    wa = None if wts is None else np.ascontiguousarray(np.asarray(wts, np.int32).reshape(12))
    pl = np.frombuffer(bytes(payload) or b"\0", np.uint8)
    a.wts, a.recovery, a.payload, a.payload_len = None if wa is None else wa.ctypes.data, recovery, pl.ctypes.data, len(payload)
    buf = np.empty(1 << 20, np.uint8)
    n = lib().hc_access_unit(C.byref(a), buf.ctypes.data, len(buf))
    assert n > 0, "hc_access_unit(%dx%d, poc %d): %d" % (w, h, poc, n)
    return bytes(buf[:n])


# ---- motion (hostcheck/motion.cpp)
def motion_field(rng, cw, ch, nref, p_intra=0.12):
    """a random quadtree of 32x32 / 16x16 / 8x8 units: some intra, vectors from a small set (so that neighbours and collocated blocks often agree), random references"""
    b8h, b8w = ch // 8, cw // 8
    log2 = np.zeros((b8h, b8w), np.uint8); intra = np.zeros_like(log2); ref = np.zeros_like(log2); cbf = np.zeros_like(log2)
    mv = np.zeros((b8h, b8w, 2), np.int16)
    pool = [(0, 0), (4, 0), (-8, 4), (12, -4), (4, 0), (3, -1), (-33, 17), (100, -60), (8, 0), (-2, 6)]
    for y in range(0, ch, 32):
        for x in range(0, cw, 32):
            l = rng.choice((5, 4, 4, 3))
            for yy in range(y, y + 32, 1 << l):
                for xx in range(x, x + 32, 1 << l):
                    s = (slice(yy // 8, (yy + (1 << l)) // 8), slice(xx // 8, (xx + (1 << l)) // 8))
                    log2[s] = l
                    intra[s] = rng.random() < p_intra
                    mv[s] = pool[rng.randrange(len(pool))] if rng.random() < 0.8 else (rng.randrange(-300, 300), rng.randrange(-150, 150))
                    ref[s] = rng.randrange(nref)
                    cbf[s] = rng.random() < 0.5
    mv[intra != 0] = 0
    return log2, intra, mv, ref, cbf


def col_record(intra, mv, ref):
    """the record a picture files (hevc_core.h ColMv): its top-left 8x8 unit's motion for every 16x16 block, distance 0 for intra"""
    i, m, r = intra[::2, ::2], mv[::2, ::2], ref[::2, ::2]
    rec = np.zeros(i.shape + (4,), np.int16)
    rec[..., 0] = np.where(i != 0, 0, m[..., 0])
    rec[..., 1] = np.where(i != 0, 0, m[..., 1])
    rec[..., 2] = np.where(i != 0, 0, r.astype(np.int16) + 1)
    return np.ascontiguousarray(rec)


# what hc.cands is held to: tests/pyhevc.py's derivation on the same motion field
class Pic:
    pass


class Ref:
    def __init__(self, poc):
        self.poc, self.is_lt = poc, False


def col_picture(poc, intra, mv, ref):
    """pyhevc's view of the collocated picture: list-0 motion per 4x4 block, intra blocks with no list"""
    p = Pic()
    p.poc, p.is_lt = poc, False
    h4, w4 = intra.shape[0] * 2, intra.shape[1] * 2
    up = lambda a: np.repeat(np.repeat(a, 2, 0), 2, 1)
    p.mv = np.zeros((h4, w4, 2, 2), np.int32)
    p.mv[:, :, 0, :] = up(mv)
    p.ref_idx = np.full((h4, w4, 2), -1, np.int32)
    p.ref_idx[:, :, 0] = np.where(up(intra) != 0, -1, up(ref).astype(np.int32))
    p.ref_poc = np.zeros((h4, w4, 2), np.int32)
    p.ref_poc[:, :, 0] = poc - 1 - up(ref).astype(np.int32)
    p.ref_lt = np.zeros((h4, w4, 2), np.int32)
    return p


class MotionStub:
    """the state pyhevc.SliceDecoder's merge / AMVP / temporal derivations read, filled from one motion field and the collocated picture's"""
    merge_candidates = pyhevc.SliceDecoder.merge_candidates
    amvp_candidates = pyhevc.SliceDecoder.amvp_candidates
    pb_avail = pyhevc.SliceDecoder.pb_avail
    avail = pyhevc.SliceDecoder.avail
    zaddr = pyhevc.SliceDecoder.zaddr
    motion = pyhevc.SliceDecoder.motion
    temporal = pyhevc.SliceDecoder.temporal
    scale = staticmethod(pyhevc.SliceDecoder.scale)

    def __init__(self, cw, ch, tr, tc, nref, intra, mv, ref, col, poc):
        self.w, self.h, self.ctb_log2, self.ctb, self.wc = cw, ch, 6, 64, cw // 64
        rows, cols = ch // 64, cw // 64
        self.tile_of_row = [next(i for i in range(tr) if (i * rows) // tr <= y < ((i + 1) * rows) // tr) for y in range(rows)]
        self.tile_of_col = [next(i for i in range(tc) if (i * cols) // tc <= x < ((i + 1) * cols) // tc) for x in range(cols)]
        self.ctb_slice = [-1] * (rows * cols)
        self.sps = {"min_cb": 3}
        self.pps = {"par_mrg": 2}
        self.cu_pred = intra.astype(np.int32)
        self.pic = Pic()
        self.pic.mv = np.zeros((ch // 4, cw // 4, 2, 2), np.int32)
        self.pic.mv[:, :, 0, :] = np.repeat(np.repeat(mv, 2, 0), 2, 1)
        self.pic.ref_idx = np.full((ch // 4, cw // 4, 2), -1, np.int32)
        self.pic.ref_idx[:, :, 0] = np.repeat(np.repeat(ref, 2, 0), 2, 1)
        self.refs = [[col if (k == 0 and col is not None) else Ref(poc - 1 - k) for k in range(nref)], []]
        self.sh = {"poc": poc, "max_merge": 5, "b": False, "nref": nref, "tmvp": col is not None, "col_idx": 0, "col_l0": 1}


def _field(field):
    """(log2, intra, mv, ref, cbf) -> contiguous arrays (kept alive by the caller of this) of the element types the library reads"""
    return [np.ascontiguousarray(a, t) for a, t in zip(field, (np.uint8, np.uint8, np.int16, np.uint8, np.uint8))]


def cands(cw, ch, tr, tc, nref, field, x0, y0, cl, col=None, tab=0):
    """-> (merge[15], amvp[4], sig[5]) of the inter CU at (x0, y0) of size 1 << cl; field = (log2, intra, mv, ref, cbf); col: the collocated record, tab: the
    POC distances, byte k = reference k (0: k + 1).  motion.cpp hc_cands says which product code each combination reaches."""
    a = _field(field)
    merge, amvp, sig = np.zeros(15, np.int32), np.zeros(4, np.int32), np.zeros(5, np.int32)
    lib().hc_cands(cw, ch, tr, tc, nref, *[v.ctypes.data for v in a], None if col is None else col.ctypes.data, tab, x0, y0, cl,
                   merge.ctypes.data, amvp.ctypes.data, sig.ctypes.data)
    return merge, amvp, sig


def picture(cw, ch, tr, tc, nref, field, col=None):
    """the signalling of every 8x8 unit of a picture and the record it files -> (flags, merge_idx, mvp_idx, mvd, col_out)"""
    a = _field(field)
    b8 = (ch // 8, cw // 8)
    flags, midx, mvp, mvd = np.zeros(b8, np.uint8), np.zeros(b8, np.uint8), np.zeros(b8, np.uint8), np.zeros(b8 + (2,), np.int16)
    out = np.zeros((ch // 16, cw // 16, 4), np.int16)
    lib().ht_picture(cw, ch, tr, tc, nref, *[v.ctypes.data for v in a], None if col is None else col.ctypes.data, flags.ctypes.data, midx.ctypes.data,
                     mvp.ctypes.data, mvd.ctypes.data, out.ctypes.data)
    return flags, midx, mvp, mvd, out


# ---- statements (hostcheck/statements.cpp)
def wp_moments(s1, s2, n):
    out = np.zeros(2, np.int64)
    lib().hw_moments(s1, s2, n, out.ctypes.data)
    return int(out[0]), int(out[1])


def wp_candidate(mc, vc, mr, vr):
    out = np.zeros(3, np.int32)
    lib().hw_candidate(mc, vc, mr, vr, out.ctypes.data)
    return int(out[0]), int(out[1]), bool(out[2])


LAYOUT_PARTS = ("region", "ctu", "tile", "sao", "scaling", "wt", "frame", "nb", "tus", "lev", "b4x", "index")
LAYOUT_SIZES = ("B4Rec", "TuRange", "SaoParams", "scaling", "DecWt", "DecFrame", "DecTu", "B4L1")


def input_layout(pw, ph, ctb_log2, ntu, nlev, nb4x, bi):
    """dec_frame.h DecInputLayout -> ({part: offset}, fixed_bytes, upload_bytes, {struct: size})"""
    out, sizes = np.zeros(14, np.uint64), np.zeros(8, np.uint64)
    lib().hd_input_layout(pw, ph, ctb_log2, ntu, nlev, nb4x, int(bi), out.ctypes.data, sizes.ctypes.data)
    return dict(zip(LAYOUT_PARTS, map(int, out[:12]))), int(out[12]), int(out[13]), dict(zip(LAYOUT_SIZES, map(int, sizes)))


ENC_LAYOUT = ("cw", "ch", "rows", "npx", "nb8", "n16", "nctu", "plane0", "plane1", "cu_bytes", "cu_mv", "col", "mc_q", "mc_centres", "sc_blocks", "sync", "edge_col", "edge_row",
              "me_block", "intra_scratch", "intra_order", "trace", "tok_cap", "tok_buf", "tok_count", "tok_seg", "tok_list", "tok_dense_cap", "stage_cap", "out_cap",
              "ctx_save", "sub", "me_cand_off", "ip_arrive_off", "ip_scratch_off", "ic16_off", "ic32_off", "im8_off", "im16_off", "im32_off", "edge_col_off1", "edge_col_off2")


def enc_layout(width, height, band_rows=0):
    """enc_layout.h EncLayout -> {name: count, cap or offset}; "edge_col_off" / "edge_row_off": the three planes' offsets, "cu_off": the seven CU arrays'"""
    out = np.zeros(52, np.uint64)
    lib().he_layout(width, height, band_rows, out.ctypes.data)
    d = dict(zip(ENC_LAYOUT, map(int, out[:42])))
    d["edge_col_off"] = [0, d.pop("edge_col_off1"), d.pop("edge_col_off2")]
    d["edge_row_off"] = [int(v) for v in out[42:45]]
    d["cu_off"] = [int(v) for v in out[45:52]]
    return d
