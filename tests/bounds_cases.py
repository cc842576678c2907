"""The table of streams at the bounds of the syntax: coefficient levels at +-32767 / -32768 and the longest escape codes, vector differences at the ends of their
range and vectors that fold across +-2^15 (8.5.3.2.6), prediction weights, offsets and denominators at their ends on saturated pictures, and pictures smaller than
a coding tree block.  Written by the stream synthesiser (oracle/hevc_gen.c: sat_levels, edge_mvd, edge_weights).  tests/test_bounds_streams.py holds the checker's
decoder and tests/pyhevc.py to each other on every row (CPU), tests/test_gpu_bounds_streams.py the HIP decoder to the checker.

A row: `id`, picture size `w` x `h`, `pictures`, `frames` (the GPU test also runs it with four frame threads), the synthesiser's options `cfg`, and `seen`: the
counters of pyhevc.Decoder.seen that must be above zero -- the stream holds what the row is there for.  Seeds and percentages were picked on the CPU until that held.

Counters (tests/pyhevc.py): level_big |level| >= 32766, level_m32768, esc14_rice<r> an escape code with a suffix of 14 bits at Rice parameter r,
dequant_clip_flat / dequant_clip_lists a scaled coefficient beyond 16 bits (m = 16 / scaling lists), stage1_clip_<4|8|16|32|dst> a first-stage intermediate beyond 16
bits, rec_clip0 / rec_clip255 a reconstructed sample clipped, level_big_bypass / level_big_tskip such a level in a transquant-bypass / transform-skip block,
level_big_<luma|chroma>_qp<n> such a level scaled at QP n, slice_qp_<n> a slice with SliceQpY n,
mvd_end a vector difference at an end of its range, mv_wrap a component folded, mv_wrap_near folded by one to four (mvp + mvd just across +-2^15), mv_at_end within four
of the end without folding, pb_outside a prediction block wholly outside the reference picture,
<w|o|denom>_<lo|hi>_<uni|bi> a luma weight delta / offset / denominator at an end in a uni- / bi-predicted block, c<w|o|denom>_... the same for chroma."""

LEVELS = ("level_big", "level_m32768", "rec_clip0", "rec_clip255")
ESCAPES = tuple("esc14_rice%d" % r for r in range(5))
STAGES = ("stage1_clip_4", "stage1_clip_8", "stage1_clip_16", "stage1_clip_32", "stage1_clip_dst")
VECTORS = ("mvd_end", "mv_wrap", "mv_wrap_near", "mv_at_end", "pb_outside")
C_W = ("cw_lo_uni", "cw_hi_uni")
W_UNI = tuple("%s_%s_uni" % (a, b) for a in ("w", "o", "denom") for b in ("lo", "hi"))
W_BI = tuple("%s_%s_bi" % (a, b) for a in ("w", "o", "denom") for b in ("lo", "hi"))


def at_qp(qp):
    """saturating luma levels scaled at the very QP the row names (qp_delta = 0: every coding unit sits at SliceQpY)"""
    return ("slice_qp_%d" % qp, "level_big_luma_qp%d" % qp)


def row(id, w=200, h=136, pictures=4, frames=False, seen=(), **cfg):
    cfg.setdefault("seed", 1)
    return dict(id=id, w=w, h=h, pictures=pictures, frames=frames, seen=tuple(seen), cfg=cfg)


SMALL = dict(wpp=1, sao=1, intra_in_p=30, tmvp=1, num_refs=2, big_mvd=1)
ALL_ON = dict(sat_levels=20, edge_mvd=10, edge_weights=1, weighted=60, b_slices=50, gop=4, scaling_lists=4, tq_bypass=15, transform_skip=1, sign_hiding=1, sao=1,
              qp_delta=2)

ROWS = (
    # ---- levels, flat quantiser (m = 16): the 32-bit dequantisers at both ends of the QP range, the clip to 16 bits, the stage sums
    [row("levels-qp%d" % qp, qp=qp, qp_delta=0, sat_levels=35, seed=seed, seen=LEVELS + ESCAPES + ("dequant_clip_flat", "stage1_clip_4", "stage1_clip_8", "stage1_clip_16") + at_qp(qp))
     for qp, seed in ((0, 61), (26, 61), (51, 61))]
    # ---- drifting QP
    + [row("levels-qp-drift", qp_delta=4, chroma_qp_offsets=1, sat_levels=35, seed=3, frames=True, seen=LEVELS + ("dequant_clip_flat",))]
    # ---- every transform size: 4 (DCT and DST) .. 32
    + [row("levels-sizes-intra", max_cu_log2=6, th_depth_inter=2, th_depth_intra=2, nxn_intra=1, intra_period=1, sat_levels=35, seed=4, seen=LEVELS + STAGES),
       row("levels-sizes-inter", max_cu_log2=6, th_depth_inter=2, th_depth_intra=2, nxn_intra=1, intra_in_p=20, sat_levels=35, seed=5, seen=LEVELS + STAGES)]
    # ---- scaling lists: m = 1 .. 255, the 64-bit product at QP 51
    + [row("levels-lists%d-qp%d" % (sl, qp), scaling_lists=sl, qp=qp, qp_delta=0, sat_levels=35, seed=seed, seen=LEVELS + ("dequant_clip_lists",) + at_qp(qp))
       for sl, qp, seed in ((2, 51, 61), (2, 0, 61), (4, 51, 61), (4, 0, 61))]
    # ---- transform skip, transquant bypass (with sign hiding: a bypass unit hides no sign)
    + [row("levels-tskip", transform_skip=1, sat_levels=35, seed=7, seen=LEVELS + ("level_big_tskip",)),
       row("levels-bypass35", tq_bypass=35, sign_hiding=1, sat_levels=35, seed=8, frames=True, seen=LEVELS + ("level_big_bypass",)),
       row("levels-bypass100", tq_bypass=100, sign_hiding=1, sat_levels=35, seed=9, frames=True, seen=("level_big", "level_m32768", "rec_clip0", "rec_clip255", "level_big_bypass"))]
    # ---- smaller coding tree blocks: the size limit of a coding tree unit bites
    + [row("levels-ctb%d" % (1 << c), ctb_log2=c, sat_levels=35, seed=10, seen=LEVELS) for c in (5, 4)]
    # ---- vectors
    + [row("vectors-refs1", edge_mvd=20, num_refs=1, tmvp=1, seed=11, pictures=5, frames=True, seen=VECTORS),
       row("vectors-refs4", edge_mvd=20, num_refs=4, tmvp=1, seed=12, pictures=5, frames=True, seen=VECTORS),
       row("vectors-b", edge_mvd=20, num_refs=4, tmvp=1, b_slices=70, gop=4, seed=13, pictures=5, frames=True, seen=VECTORS),
       row("vectors-tiles", edge_mvd=20, num_refs=2, tmvp=1, tile_cols=2, tile_rows=2, seed=14, pictures=5, seen=VECTORS)]
    # ---- weights on saturated pictures
    + [row("weights-p", edge_weights=1, weighted=100, sat_levels=25, num_refs=3, seed=51, pictures=5, seen=W_UNI + C_W + ("rec_clip0", "rec_clip255")),
       row("weights-b", edge_weights=1, weighted=100, sat_levels=25, num_refs=3, b_slices=70, gop=4, seed=52, pictures=5, frames=True, seen=W_UNI + W_BI + C_W + ("rec_clip0", "rec_clip255"))]
    # ---- small pictures: a side below the coding tree block, below the interpolation filter's reach; 6 pictures, so that P pictures predict from the padding
    + [row("small-%dx%d-ctb%d" % (w, h, 1 << c), w=w, h=h, pictures=6, ctb_log2=c, seed=17 + c, **SMALL)
       for (w, h) in ((16, 16), (16, 24), (24, 16), (40, 40), (56, 72), (16, 200), (328, 16), (64, 200), (32, 136)) for c in (6, 5, 4)]
    # ---- one coding tree block wide, several rows, WPP: every row starts from initialised contexts (9.3.1: the block above-right does not exist)
    + [row("column-%dx%d-ctb%d" % (w, h, 1 << c), w=w, h=h, pictures=6, ctb_log2=c, seed=31, cabac_init=1, sat_levels=10, **SMALL) for (w, h, c) in ((16, 200, 4), (32, 136, 5), (64, 200, 6))]
    # ---- every tile one coding tree block
    + [row("tiles-%dx%d-wpp%d-lf%d" % (w, h, wpp, lf), w=w, h=h, pictures=6, ctb_log2=4, tile_cols=tc, tile_rows=tr, lf_across=lf, seed=33, **dict(SMALL, wpp=wpp))
       for (w, h, tc, tr) in ((48, 48, 3, 3), (64, 32, 4, 2)) for wpp in (0, 1) for lf in (0, 1)]
    # ---- everything at once
    + [row("all-ctb%d" % (1 << c), ctb_log2=c, seed=41, pictures=5, frames=True, seen=("level_big", "mvd_end", "mv_wrap"), **ALL_ON) for c in (6, 5, 4)]
)

BY_ID = {r["id"]: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def stream(r):
    """the access units of a row"""
    import orc
    g = orc.OracleGen(r["w"], r["h"], **r["cfg"])
    try:
        return [g.picture() for _ in range(r["pictures"])]
    finally:
        g.close()
