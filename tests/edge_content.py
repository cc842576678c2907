"""Full-range, saturating picture content for the edge-content tests (numpy only).

The synthetic clips of the other tests (orc.synth_frame kinds 0/1/2) keep luma in [16, 235] and chroma well inside
[0, 255], or are uniform noise that lines nothing up.  Every pattern here is built to drive one exactness argument of the
kernels to its bound: ±255 residuals over whole blocks, 0/255 reference samples, reconstructions that would leave
[0, 255] without their clip.  Each pattern is a function (w, h, t, seed) -> packed I420 uint8.

Chroma is full range: Cb is the luma pattern on the chroma grid and Cr = 255 - Cb, so one plane sits at 0 where the
other sits at 255.  flat_chroma(pattern) is the variant with both chroma planes at 128.

CASES is the case matrix shared by test_edge_content.py (the checker's closed loop, CPU) and test_gpu_edge_content.py
(HIP encoder and decoder against the checker); codec_options() turns a case into the options of both encoders.
"""
import numpy as np


def _i420(y, cb, cr=None):
    y = np.asarray(y, dtype=np.uint8)
    cb = np.asarray(cb, dtype=np.uint8)
    cr = (255 - cb).astype(np.uint8) if cr is None else np.asarray(cr, dtype=np.uint8)
    return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])


def _full(plane_fn, w, h, t, seed):
    """luma from plane_fn(w, h, t, seed, 1), Cb from the same pattern on the chroma grid, Cr = 255 - Cb"""
    return _i420(plane_fn(w, h, t, seed, 1), plane_fn(w // 2, h // 2, t, seed, 2))


def planes(i420, w, h):
    """(Y, Cb, Cr) views of a packed I420 picture"""
    ny, nc = w * h, (w // 2) * (h // 2)
    return (i420[:ny].reshape(h, w), i420[ny:ny + nc].reshape(h // 2, w // 2), i420[ny + nc:].reshape(h // 2, w // 2))


def flat_chroma(pattern):
    """the same luma with both chroma planes flat at 128"""
    def f(w, h, t, seed):
        out = pattern(w, h, t, seed).copy()
        out[w * h:] = 128
        return out
    f.__name__ = pattern.__name__ + "_flat_chroma"
    f.__doc__ = "%s with chroma flat at 128: the luma bounds alone" % pattern.__name__
    return f


# -- the patterns

def cut_black_white(w, h, t, seed):
    """0, then 255, then 0 again, ...: every P picture is a full cut.  Its residual is +255 (or -255) at every sample, every
    16x16 quarter of every motion candidate has SAD exactly 65280 (the limit of the 16-bit v_qsad accumulators), so all
    candidates tie; the largest DC coefficients; a residual of -255 is the byte split's high byte -1."""
    v = 255 if t % 2 else 0
    return _i420(np.full((h, w), v), np.full((h // 2, w // 2), v))


def cut_white_black(w, h, t, seed):
    """255, then 0, then 255, ...: cut_black_white the other way round (the first P picture's residual is -255 everywhere)"""
    return cut_black_white(w, h, t + 1, seed)


def _checker_plane(w, h, t, seed, sub, moving):
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y + (t if moving else 0)) & 1) * 255


def checker(w, h, t, seed):
    """1-sample 0/255 checkerboard, the same in every picture: the highest-frequency coefficients of every transform size,
    the intra SATD near the bound of its f16 matrix-core arithmetic (|H.d| up to 2040), deblocking decisions on maximal
    activity.  Chroma is the checkerboard on the chroma grid."""
    return _full(lambda w, h, t, s, sub: _checker_plane(w, h, t, s, sub, False), w, h, t, seed)


def checker_moving(w, h, t, seed):
    """the checkerboard moved one sample per picture: every P picture is the inverse of its reference picture at the
    zero vector (residual ±255 alternating at every sample) and matches it exactly one sample away"""
    return _full(lambda w, h, t, s, sub: _checker_plane(w, h, t, s, sub, True), w, h, t, seed)


def _binary_noise_plane(w, h, t, seed, sub):
    rng = np.random.default_rng([seed, t, sub])
    return rng.integers(0, 2, (h, w)) * 255


def binary_noise(w, h, t, seed):
    """fresh 0/255 noise in each picture: no motion vector matches, dense ±255 residuals, the longest
    coeff_abs_level_remaining escape codes at QP 0"""
    return _full(_binary_noise_plane, w, h, t, seed)


def _near_black_plane(w, h, t, seed, sub):
    """low-amplitude texture in 0..12 moving one luma sample per picture: 8x8 blocks of random levels plus ±1 grain"""
    blocks = np.random.default_rng([seed]).integers(0, 13, ((h * sub) // 8 + 2, (w * sub) // 8 + 4))     # (the same blocks on both grids)
    tex = np.kron(blocks, np.ones((8 // sub, 8 // sub), dtype=np.int64))
    tex = np.clip(tex + np.random.default_rng([seed, sub]).integers(-1, 2, tex.shape), 0, 12)
    dx = t // sub
    return tex[:h, dx:dx + w]


def near_black(w, h, t, seed):
    """texture in 0..12 with slow motion (Cr in 243..255): at QP 40-51 reconstruction, deblocking and SAO corrections
    that would leave [0, 255] without their clip; SAO band offsets in bands 0-3 (and 28-31 in Cr)"""
    return _full(_near_black_plane, w, h, t, seed)


def near_white(w, h, t, seed):
    """near_black turned over: luma in 243..255, Cb in 243..255 and Cr in 0..12"""
    return _i420(255 - _near_black_plane(w, h, t, seed, 1), 255 - _near_black_plane(w // 2, h // 2, t, seed, 2))


def _hard_edges_plane(w, h, t, seed, sub):
    """0/255 cells 11x9 luma samples wide, off the block grid, moving 3 luma samples per picture to the right and 1 up
    (on the chroma grid: 1.5 and 0.5 samples, evaluated at the chroma sample positions)"""
    y, x = np.mgrid[0:h, 0:w]
    lx = x * sub - 3 * t
    ly = y * sub + t
    return (((lx // 11) + (ly // 9)) & 1) * 255


def hard_edges(w, h, t, seed):
    """0/255 steps moving 3 samples per picture: overshoot of the 8-tap luma and 4-tap chroma interpolation filters that
    only the clip removes (with subme), the intra DC and angular boundary filters with 0/255 reference samples"""
    return _full(_hard_edges_plane, w, h, t, seed)


def edge_column(w, h, t, seed):
    """a 0 picture whose last column and last row are 255 (chroma alike; Cr the other way round): at sizes that are not
    multiples of the CTU the input padding copies the extreme values into the coded area"""
    def plane(w, h):
        p = np.zeros((h, w), dtype=np.int64)
        p[:, -1] = 255
        p[-1, :] = 255
        return p
    return _i420(plane(w, h), plane(w // 2, h // 2))


def half_checker(w, h, t, seed):
    """the left half the 1-sample checkerboard, the right half flat 128: CTU variances at both ends of their range, so
    the adaptive QP offsets of vaq hit their clamp"""
    def plane(w, h):
        p = _checker_plane(w, h, 0, seed, 1, False)
        p[:, (w // 2) & ~31:] = 128
        return p
    return _i420(plane(w, h), plane(w // 2, h // 2))


def cut_then_noise(w, h, t, seed):
    """black, white, then binary noise: the full cut and the dense ±255 residual in one short clip"""
    return cut_black_white(w, h, t, seed) if t < 2 else binary_noise(w, h, t, seed)


checker_flat_chroma = flat_chroma(checker)
hard_edges_flat_chroma = flat_chroma(hard_edges)

PATTERNS = {f.__name__: f for f in (cut_black_white, cut_white_black, checker, checker_moving, binary_noise, near_black, near_white,
                                    hard_edges, edge_column, half_checker, cut_then_noise, checker_flat_chroma, hard_edges_flat_chroma)}
# the patterns whose every plane holds both 0 and 255 over the first pictures of a clip
FULL_RANGE = ("cut_black_white", "cut_white_black", "checker", "checker_moving", "binary_noise", "hard_edges", "edge_column", "half_checker", "cut_then_noise")

SEED = 0xED6E0000


# -- the case matrix

def _case(pattern, w=256, h=192, frames=3, qp=32, **opts):
    return dict(pattern=pattern, w=w, h=h, frames=frames, qp=qp, **opts)


CASES = (
    # ultrafast defaults at QP 0 / 32 / 51 on every pattern at 256x192
    [_case(p, qp=q) for p in ("cut_black_white", "cut_white_black", "checker", "checker_moving", "binary_noise", "near_black", "near_white",
                              "hard_edges", "edge_column", "checker_flat_chroma", "hard_edges_flat_chroma") for q in (0, 32, 51)]
    # fractional motion (8-tap / 4-tap MC and their clip) and SAO
    + [_case(p, qp=q, frames=4, subme=4, sao=1) for p in ("hard_edges", "near_black", "near_white") for q in (32, 51)]
    # rdoq + sign hiding: the zero-out and the parity fix on maximal levels
    + [_case(p, qp=q, rdoq=1, signhide=1) for p in ("checker", "binary_noise") for q in (0, 22)]
    # lossless: ±255 residuals coded sample by sample
    + [_case(p, lossless=1) for p in ("cut_black_white", "binary_noise")]
    # the default scaling lists at QP 0
    + [_case(p, qp=0, scaling_list=1) for p in ("cut_white_black", "checker")]
    # intra units in P pictures at the cut
    + [_case("cut_black_white", qp=q, frames=4, intra_in_p=2) for q in (32, 51)]
    # vaq: CTU variances at both ends, delta QP at its clamp
    + [_case("half_checker", qp=q, vaq=8) for q in (22, 32)]
    # the GPU arithmetic coder on the longest escape codes
    + [_case("binary_noise", qp=0, gpu_entropy=1)]
    # tiles with WPP
    + [_case("checker_moving", qp=22, tiles=(2, 2))]
    # padding of sizes that are not multiples of 64
    + [_case("edge_column", w=130, h=70, qp=32), _case("edge_column", w=702, h=394, qp=51)]
    # the whole-picture path at 1080p: 32x32 transforms on the matrix cores
    + [_case("cut_then_noise", w=1920, h=1080, qp=22)]
)


def case_id(c):
    extra = "_".join("%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in sorted(c.items())
                     if k not in ("pattern", "w", "h", "frames", "qp"))
    return "%s_%dx%d_qp%d%s" % (c["pattern"], c["w"], c["h"], c["qp"], "_" + extra if extra else "")


def frame(c, t):
    return PATTERNS[c["pattern"]](c["w"], c["h"], t, SEED)


def codec_options(c):
    """(OracleEncoder keyword arguments, OracleEncoder.set_option pairs, HIP Encoder options) of a case"""
    tc, tr = c.get("tiles", (1, 1))
    kw = dict(qp=c["qp"], period=64, me_range=16, wpp=1, tile_rows=tr, tile_cols=tc, sao=c.get("sao", 0), vaq=c.get("vaq", 0), subme=c.get("subme", 0))
    tools = (("intra-in-p", "intra_in_p"), ("rdoq", "rdoq"), ("signhide", "signhide"), ("scaling-list", "scaling_list"), ("lossless", "lossless"))
    sets = [(name, c[key]) for name, key in tools if c.get(key)]          # (only what a case switches on, lossless last: it switches tools off)
    hip = (("qp", c["qp"]), ("period", 64), ("me-range", 16), ("wpp", 1), ("sao", "full" if kw["sao"] else "off"), ("subme", kw["subme"]))
    hip += tuple((name, "default" if name == "scaling-list" else v) for name, v in sets)
    if (tc, tr) != (1, 1):
        hip += (("tiles", "%dx%d" % (tc, tr)),)
    if kw["vaq"]:
        hip += (("vaq", kw["vaq"]),)
    if c.get("gpu_entropy"):
        hip += (("gpu-entropy", 1),)
    return kw, sets, hip
