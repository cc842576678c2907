"""The streams of tests/test_gpu_batch_foreign.py -- several decoders open at once, foreign streams of every kind through the device's submission layer
(kvazzup_amd/csrc/batch.h) -- and what each is there for; tests/test_batch_foreign_cases.py holds the tables to that on the CPU.  Every stream is a dict
deckit.together takes: `aus` [(pts, access unit)], `want` the checker's pictures in output order (conceal_model's for a decoder in concealment mode 3), made here
on the CPU, and beside them `w`, `h`, the generator's `config` (None: the checker's encoder) and what the builders counted.  Builders are cached and their
results shared: nobody changes them, a case takes `dict(stream, threads=...)`.  Test infrastructure."""
import functools

import cases
import conceal_model
import deckit
import nalkit
import orc
import pyhevc

SEED = 31

# (a) eight forms, eight pictures each: (w, h, the synthesiser's options; None: the checker's encoder, the plain Kvazaar peer)
PLAIN = dict(qp=30, period=4, me_range=8, sao=1, subme=2)
FORMS = (
    (208, 144, dict(b_slices=70, gop=4, tmvp=1, num_refs=2, weighted=50, list_mod=50, sao=1)),
    (200, 136, dict(ctb_log2=4, min_cb_log2=4, intra_in_p=30, sao=1, slices=0)),
    (208, 144, dict(ctb_log2=5, wpp=0, tile_rows=2, tile_cols=2, slices=2, lf_across=2, intra_in_p=30, sao=1)),
    (208, 144, dict(slices=3, pcm=15, lf_across=1, intra_in_p=40, sao=1)),
    (208, 144, dict(scaling_lists=4, tq_bypass=20, intra_in_p=20, slices=0)),
    (64, 64, dict(long_term=1, num_refs=3, tmvp=1, gop=0, b_slices=0, intra_period=20, slices=0)),
    (24, 16, dict(slices=0, intra_in_p=30)),
    (320, 192, None),
)
B_SLICES, CTB16, TILES, PCM, SCALING, LONG_TERM, TINY, KVAZAAR = range(8)

CIP = (64, 64, dict(seed=3, cip=1, intra_in_p=8, slices=0, sao=1, intra_period=6))
ALL_INTRA = (352, 288, dict(intra_period=1, nxn_intra=1, slices=0))
LOSSY = ((5, 3, None), (6, 1, None), (11, 1, 3))          # (seed of nalkit.lossy, threads, concealment mode)
LOSSY_SPARE = (1, 5, 6, 7, 10)                            # where the mode-3 seed moves when its stand-ins do not move


def expected(aus):
    """the checker's decoder on [(pts, access unit)]: (its pictures in output order, how many reference pictures it had to replace)"""
    od = orc.OracleDecoder()
    try:
        want = []
        for pts, au in aus:
            want += od.decode_au(au, pts)
        want += od.flush()
        return want, od.concealed()
    finally:
        od.close()


@functools.lru_cache(maxsize=None)
def generated(w, h, n, seed, opts):
    """n pictures of the synthesiser; opts: its options as sorted items"""
    g = orc.OracleGen(w, h, seed=seed, **dict(opts))
    try:
        aus = [(t, g.picture()) for t in range(n)]
        config = dict(g.config)
    finally:
        g.close()
    want, _ = expected(aus)
    return dict(w=w, h=h, aus=aus, want=want, config=config)


def gen(w, h, kw, n, seed=SEED):
    kw = dict(kw)
    seed = kw.pop("seed", seed)
    return generated(w, h, n, seed, tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def kvazaar(repeats=1):
    """eight pictures of the synthetic clip through the checker's encoder, the access units `repeats` times in a row (each run opens with an IDR picture)"""
    w, h = FORMS[KVAZAAR][:2]
    e = orc.OracleEncoder(w, h, **PLAIN)
    try:
        once = [e.encode(orc.synth_frame(0, SEED, w, h, t)) for t in range(8)]
    finally:
        e.close()
    aus = list(enumerate(once * repeats))
    want, _ = expected(aus)
    return dict(w=w, h=h, aus=aus, want=want, config=None)


def form(k, n=8, seed=SEED):
    w, h, kw = FORMS[k]
    return kvazaar() if kw is None else gen(w, h, kw, n, seed)


class _Kinds(pyhevc.Decoder):
    """tests/pyhevc.py's decoder, noting per picture whether it holds inter and intra blocks"""

    def __init__(self, tabs):
        super().__init__(tabs)
        self.kinds = []

    def picture_done(self, sl, *a, **kw):
        used = sl.pic.ref_idx >= 0
        self.kinds.append(("I" if (~used).all(axis=2).any() else "") + ("P" if used.any() else ""))
        return super().picture_done(sl, *a, **kw)


@functools.lru_cache(maxsize=None)
def cip_stream():
    """... and `kinds`, per picture in decoding order "I", "P" or "IP": one with both is launched by its own decoder (Decoder::launch_gpu), the others by the
    submission layer; `mixed` counts the former"""
    w, h, kw = CIP
    s = dict(gen(w, h, kw, 12))
    d = _Kinds(deckit.tabs())
    for _, au in s["aus"]:
        for nal in pyhevc.split_nals(au):
            d.decode_nal(nal)
    s["kinds"] = d.kinds
    s["mixed"] = d.kinds.count("IP")
    return s


@functools.lru_cache(maxsize=None)
def lossy_stream(seed, concealment=None):
    """nalkit.lossy(seed, n=26) at 64x64: `concealed` the reference pictures the checker replaced; mode 3: the pictures are conceal_model's (their time stamps the
    checker's -- the mode changes samples, not the order), `moved` its stand-ins with a displacement"""
    cut, _, lose = nalkit.lossy(seed, n=26)
    want, concealed = expected(cut)
    s = dict(w=64, h=64, aus=cut, want=want, config=None, concealed=concealed, lost=len(lose))
    if concealment == 3:
        pics, d = conceal_model.decode([au for _, au in cut], deckit.tabs())
        assert len(pics) == len(want), "%d pictures from the model decoder, %d from the checker" % (len(pics), len(want))
        s["want"] = [dict(p, pts=c["pts"]) for p, c in zip(pics, want)]
        s["moved"] = sum(1 for x in d.stand_ins if (x["disp"] != 0).any())
    return s


@functools.lru_cache(maxsize=None)
def mode3_seed():
    """LOSSY's seed for concealment mode 3, or the first spare one whose stand-ins move"""
    for seed in (LOSSY[2][0],) + LOSSY_SPARE:
        if lossy_stream(seed, 3)["moved"]:
            return seed
    raise AssertionError("no seed of nalkit.lossy gives a stand-in that moves")


# ---- the cases: lists of streams with how each decoder runs
def eight_forms():
    """(a) decoders alternate between synchronous and four frame threads"""
    return [dict(form(k), threads=(1, 4)[k & 1]) for k in range(len(FORMS))]


def ten_decoders():
    """(b) two more than a batch holds"""
    return eight_forms() + [dict(form(TINY, seed=SEED + 1), threads=1), dict(form(LONG_TERM, seed=SEED + 1), threads=4)]


def cip_hop():
    """(c) a decoder that changes between the submission layer and its own launches beside two that stay"""
    return [dict(cip_stream(), threads=1), dict(form(CTB16, n=12), threads=4), dict(form(TINY, n=12), threads=1)]


def everything_plan(group):
    """(d) four consecutive seeds of cases.drawn, group 0 .. 11: [(seed, w, h, options, pictures, threads)], as tests/test_gpu_everything.py runs them one by one"""
    out = []
    for seed in range(4 * group + 1, 4 * group + 5):
        w, h, kw = cases.drawn(seed)
        out.append((seed, w, h, kw, 12 if kw.get("long_term") else 6, 3 if seed & 1 else 1))
    return out


def everything(group):
    return [dict(gen(w, h, kw, n, seed), threads=threads) for seed, w, h, kw, n, threads in everything_plan(group)]


def lost_pictures():
    """(e) three decoders that conceal, one of them in mode 3, beside a clean one"""
    out = []
    for seed, threads, mode in LOSSY:
        out.append(dict(lossy_stream(mode3_seed() if mode == 3 else seed, mode), threads=threads, concealment=mode))
    return out + [dict(kvazaar(3), threads=1)]


def join_and_leave():
    """(f) a frame-threaded decoder alone on its two chains; two peers come and go"""
    w, h, kw = ALL_INTRA
    return [dict(gen(w, h, kw, 12), threads=4),
            dict(form(LONG_TERM), threads=1, start_after=(0, 3), close_early=True),
            dict(form(TINY), threads=1, start_after=(0, 8), close_early=True)]


def total(streams):
    return sum(len(s["want"]) for s in streams)
