"""ctypes bindings of tests/hostcheck/coder.cpp (host build of the product's arithmetic coder, entropy_host.h).  Test infrastructure."""
import ctypes as C
import numpy as np
from hc import lib

CTX_COUNT = 154


def play(lanes, subs, ctx0):
    """subs: list of substreams, each a list of uint16 token arrays (runs); ctx0: (nsub, CTX_COUNT) uint8.  -> [(bytes, bins)]"""
    runs = [np.asarray(r, dtype=np.uint16) for s in subs for r in s]
    tok = np.ascontiguousarray(np.concatenate(runs) if runs else np.zeros(1, np.uint16))
    run_len = np.array([len(r) for r in runs] or [0], dtype=np.int32)
    run_first = np.cumsum([0] + [len(s) for s in subs]).astype(np.int32)
    nsub = len(subs)
    cap = 2 * max([sum(len(r) for r in s) for s in subs] + [0]) + 64
    out = np.zeros(nsub * cap, dtype=np.uint8)
    ln = np.zeros(nsub, dtype=np.int32)
    bins = np.zeros(nsub, dtype=np.uint32)
    ctx0 = np.ascontiguousarray(ctx0, dtype=np.uint8)
    lib().hcr_play(lanes, tok.ctypes.data, run_len.ctypes.data, run_first.ctypes.data, nsub, ctx0.ctypes.data, out.ctypes.data, cap,
                   ln.ctypes.data, bins.ctypes.data)
    return [(bytes(out[k * cap:k * cap + ln[k]]), int(bins[k])) for k in range(nsub)]


def _rows(n, out, cap, ln, bins):
    assert n >= 0, "the coder filed more substreams, or longer ones, than the buffers hold (%d)" % n
    return [bytes(out[k * cap:k * cap + ln[k]]) for k in range(n)], bins.value


def code_picture(lanes, tok, count, offset, wc, hc, wpp, tile_rows=1, tile_cols=1, init_type=1, qp=32, threads=4):
    cap = 2 * int(count.max(initial=0)) * wc * hc + 64
    maxs = hc * tile_cols * max(tile_rows, 1) + 1
    out = np.zeros(maxs * cap, dtype=np.uint8)
    ln = np.zeros(maxs, dtype=np.int32)
    bins = C.c_ulonglong()
    n = lib().hcr_code_picture(threads, lanes, tok.ctypes.data, count.ctypes.data, offset.ctypes.data, wc, hc, int(wpp), tile_rows, tile_cols,
                               init_type, qp, out.ctypes.data, cap, ln.ctypes.data, maxs, C.byref(bins))
    return _rows(n, out, cap, ln, bins)


def code_band(lanes, tok, count, offset, wc, hc, wpp, tile_rows, row0, nrows, init_type=1, qp=32, threads=4):
    cap = 2 * int(count.max(initial=0)) * wc * hc + 64
    maxs = hc + 1
    out = np.zeros(maxs * cap, dtype=np.uint8)
    ln = np.zeros(maxs, dtype=np.int32)
    bins = C.c_ulonglong()
    n = lib().hcr_code_band(threads, lanes, tok.ctypes.data, count.ctypes.data, offset.ctypes.data, wc, hc, int(wpp), tile_rows, init_type, qp,
                            row0, nrows, out.ctypes.data, cap, ln.ctypes.data, maxs, C.byref(bins))
    return _rows(n, out, cap, ln, bins)
