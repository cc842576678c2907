"""The streams tests/test_partial_pictures.py (CPU) and tests/test_gpu_partial_pictures.py share: pictures in Kvazaar's row form -- WPP, a dependent slice segment per
CTB row -- with segments lost on the way, and what tests/partial_model.py makes of them.  The losses are chosen here, on the CPU, with the model; what every
case brings is asserted by the CPU test.  Test infrastructure."""
import functools

import deckit
import enckit
import orc
import partial_model as pm

# synthesiser streams (oracle/hevc_gen.c, slices = 1 with WPP): name -> (w, h, pictures, generator options, losses {access unit: lost VCL units})
#  72x56: the last CTB column and row are 8 samples wide (CTB 16 and 32); 64x64 CTB 16 four full rows; 416x240 CTB 64 seven by four, the last row 48 samples
SYNTH = {
    "72x56_ctb16_sao_tmvp": (72, 56, 9, dict(seed=3, ctb_log2=4, tmvp=1, sao=1, intra_in_p=30, gop=0, b_slices=0), {1: (1,), 3: (3,), 4: (2,), 6: (0, 1, 2, 3), 7: (1,)}),
    "72x56_ctb32": (72, 56, 8, dict(seed=5, ctb_log2=5, tmvp=1, sao=0, gop=0, b_slices=0, num_refs=2), {2: (1,), 3: (1,), 6: (1,)}),
    "64x64_ctb16_b": (64, 64, 10, dict(seed=7, ctb_log2=4, tmvp=1, sao=1, gop=4, b_slices=50, intra_period=16), {2: (2,), 3: (1,), 5: (3,), 7: (2, 3)}),
    "64x64_ctb16_irap": (64, 64, 9, dict(seed=9, ctb_log2=4, tmvp=0, sao=1, lf_across=2, intra_period=4, gop=0, b_slices=0), {2: (1,), 4: (2,), 8: (1,)}),
    "416x240_ctb64": (416, 240, 8, dict(seed=4, ctb_log2=6, tmvp=1, sao=1, intra_in_p=30, gop=0, b_slices=0), {2: (2,), 5: (1, 2)}),
}
# the checker's encoder with slices=wpp on the pan clip at 320x192 (three CTB rows): (lp-refs, pan) ; row 1's segment of pictures 3 and 4 lost: row 0 stays, rows 1-2 are filled
ENCODED = {"pan_refs1": (1, (12, -6)), "pan_refs3": (3, (10, -5))}
NAMES = list(SYNTH) + list(ENCODED)
# pictures of FREE slices, without and with WPP (synthesiser slices = 3: independent slices and dependent segments that begin at any coding tree block): name -> (w, h, pictures,
# generator options); the losses are drawn from the stream's own segment table, one pattern per access unit (free_losses).  72x56 with CTB 64 is 2 x 1 blocks.
FREE = {
    "free_72x56_ctb16": (72, 56, 9, dict(seed=21, ctb_log2=4, lf_across=0, tmvp=1, sao=1, gop=0, b_slices=0, intra_period=16)),
    "free_64x64_ctb16_lf2": (64, 64, 9, dict(seed=24, ctb_log2=4, lf_across=2, tmvp=1, sao=1, gop=0, b_slices=0, intra_period=16)),
    "free_72x56_ctb32": (72, 56, 9, dict(seed=26, ctb_log2=5, lf_across=2, tmvp=1, sao=1, intra_in_p=30, gop=0, b_slices=0, intra_period=16)),
    "free_72x56_ctb64": (72, 56, 9, dict(seed=27, ctb_log2=6, lf_across=0, tmvp=0, sao=1, gop=0, b_slices=0, intra_period=16)),
    "free_416x240_ctb64_b": (416, 240, 8, dict(seed=28, ctb_log2=6, lf_across=0, tmvp=1, sao=1, intra_in_p=30, gop=4, b_slices=50, intra_period=16)),
    "free_wpp_72x56_ctb16_lf2": (72, 56, 9, dict(wpp=1, seed=22, ctb_log2=4, lf_across=2, tmvp=1, sao=1, gop=0, b_slices=0, intra_period=16)),
    "free_wpp_72x56_ctb32": (72, 56, 9, dict(wpp=1, seed=23, ctb_log2=5, lf_across=0, tmvp=1, sao=1, intra_in_p=30, gop=0, b_slices=0, intra_period=16)),
    "free_wpp_64x64_ctb16": (64, 64, 9, dict(wpp=1, seed=25, ctb_log2=4, lf_across=0, tmvp=1, sao=1, gop=0, b_slices=0, intra_period=16)),
    "free_wpp_416x240_ctb64_b": (416, 240, 8, dict(wpp=1, seed=29, ctb_log2=6, lf_across=2, tmvp=1, sao=1, intra_in_p=30, gop=4, b_slices=50, intra_period=16)),
}
PATTERNS = ("first segment lost with an independent one behind it", "a middle independent segment lost", "two separate gaps in one picture",
            "a middle dependent segment lost that drags later dependents with it", "last segment lost")


def free_losses(table):
    """{pattern: (access unit, lost VCL units)}: for every pattern the first access unit behind the first that has it and carries no other pattern yet"""
    out, used = {}, set()
    for t, segs in enumerate(table):
        if t == 0 or len(segs) < 2:
            continue
        indep = [k for k, s in enumerate(segs) if k > 0 and not s[1]]
        mid = [k for k in indep if k < len(segs) - 1]
        dep = [k for k, s in enumerate(segs) if k > 0 and s[1] and k + 1 < len(segs) and segs[k + 1][1]]
        have = {PATTERNS[0]: (0,) if indep and indep[0] == 1 else None, PATTERNS[1]: (mid[0],) if mid else None,
                PATTERNS[2]: (indep[0], indep[-1]) if len(indep) >= 2 and indep[-1] - indep[0] >= 2 else None, PATTERNS[3]: (dep[0],) if dep else None,
                PATTERNS[4]: (len(segs) - 1,)}
        for p in PATTERNS:
            if p not in out and have[p] is not None and t not in used:
                out[p] = (t, have[p])
                used.add(t)
    return out


@functools.lru_cache(maxsize=None)
def stream(name):
    """(w, h, every access unit, [(time stamp, what arrives of the access unit)])"""
    if name in FREE:
        w, h, n, kw = FREE[name]
        g = orc.OracleGen(w, h, slices=3, tile_rows=1, tile_cols=1, **dict(dict(wpp=0), **kw))
        aus = [g.picture() for _ in range(n)]
        g.close()
        lost = {t: v for t, v in free_losses(pm.segment_table(aus)).values()}
    elif name in SYNTH:
        w, h, n, kw, lost = SYNTH[name]
        g = orc.OracleGen(w, h, slices=1, wpp=1, tile_rows=1, tile_cols=1, **kw)
        aus = [g.picture() for _ in range(n)]
        g.close()
    else:
        refs, (dx, dy) = ENCODED[name]
        w, h, lost = 320, 192, {3: (1,), 4: (1,)}
        e = enckit.oracle_encoder(w, h, n=refs, qp=30, subme=2, slices=1)
        aus = [e.encode(f) for f in enckit.pan(w, h, 7, dx, dy)]
        e.close()
    return w, h, aus, pm.cut(aus, lost)


def ctb_of(name):
    return 1 << ((FREE.get(name) or SYNTH.get(name) or (0, 0, 0, dict(ctb_log2=6)))[3]["ctb_log2"])


@functools.lru_cache(maxsize=None)
def model(name, mode):
    """(the model's pictures in output order, the model decoder) of what arrives"""
    return pm.decode([au for _, au in stream(name)[3]], deckit.tabs(), mode)


# ---- the product's host half on these streams (kvzx_decoder_set_parse_only with partial pictures on): run as a CHILD process with a time limit -- a parser thread
# left waiting for a coding tree block that never comes is then a failure, not a stuck suite
def probe(name, threads, option=1, nals=None, blocks=None):
    """{"log": [[poc, first, count]], "layouts": per damaged picture its "partial_layout" rows [missing, ctu_tile, ctu_nb, blocks], "digest"}"""
    import ctypes as C
    import numpy as np
    import parser_probe
    lib = parser_probe._lib()
    lib.kvzx_decoder_set_partial_pictures.argtypes = [C.c_void_p, C.c_int]
    lib.kvzx_decoder_damage_log.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    lib.kvzx_decoder_debug_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    if nals is None:
        nals = [n for _, au in stream(name)[3] for n in orc.split_nals(au)]
    h = lib.libOpenHevcInit(1, 2)
    assert lib.kvzx_decoder_set_parse_only(h, threads) == 1 and lib.kvzx_decoder_set_partial_pictures(h, option) == 1 and lib.libOpenHevcStartDecoder(h) == 0
    if blocks is None and name is not None:
        pw, ph = stream(name)[:2]
        blocks = -(-pw // ctb_of(name)) * -(-ph // ctb_of(name))
    layouts, seen, total = [], 0, blocks or 0
    try:
        for t, n in enumerate(list(nals) + [bytes([0, 0, 0, 1, 36 << 1, 1])]):
            rc = lib.libOpenHevcDecode(h, n, len(n), t)
            assert rc == 0, "NAL %d: libOpenHevcDecode returned %d (error %d)" % (t, rc, lib.kvzx_decoder_last_error(h))
            k = lib.kvzx_decoder_damage_log(h, None, 0)
            if k > seen:
                seen = k
                assert total, "a damaged picture, and the caller did not say how many blocks a picture has"
                lay = np.zeros((total, 4), np.uint8)
                assert lib.kvzx_decoder_debug_copy(h, b"partial_layout", lay.ctypes.data, lay.nbytes)
                layouts.append(lay.tolist())
        buf = (C.c_int32 * (3 * max(seen, 1)))()
        assert lib.kvzx_decoder_damage_log(h, buf, seen) == seen
        out = (C.c_uint64 * 5)()
        lib.kvzx_decoder_parse_probe_stats(h, out, None)
    finally:
        lib.libOpenHevcClose(h)
    return {"log": [list(buf[3 * i:3 * i + 3]) for i in range(seen)], "layouts": layouts, "digest": "%016x" % out[3], "pictures": int(out[0])}


if __name__ == "__main__":
    import json
    import sys
    sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
    if sys.argv[1].startswith("digest:"):                       # a stream of tests/parser_probe.py with nothing lost and the option on
        import parser_probe
        name = sys.argv[1][7:]
        nals = dict(parser_probe.golden_cases())[name] if name.startswith("golden_") else parser_probe.encoded_case(name)
        print(json.dumps(probe(None, int(sys.argv[2]), nals=nals)))
    elif sys.argv[1].startswith("file:"):                       # a committed stream with its losses in it (tests/golden/partial/): file:<name>:<blocks a picture>
        _, fname, blocks = sys.argv[1].split(":")
        data = open(__import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "partial", fname), "rb").read()
        print(json.dumps(probe(None, int(sys.argv[2]), nals=orc.split_nals(data), blocks=int(blocks))))
    else:
        print(json.dumps(probe(sys.argv[1], int(sys.argv[2]))))
