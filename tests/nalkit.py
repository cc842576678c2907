"""Streams of the synthesiser cut, renamed and thinned the way a splicer or a lossy wire does it: what the random access and lost picture tests, on the CPU and on
the GPU, and the soak scripts under tools/ share.  Test infrastructure."""
import orc


EOS = bytes([0, 0, 0, 1, 36 << 1, 1])                   # an end of sequence NAL unit


def nal_type(nal):
    i = 0
    while nal[i] == 0:
        i += 1
    return (nal[i + 1] >> 1) & 63


def vcl_type(au):
    return next(t for t in (nal_type(n) for n in orc.split_nals(au)) if t < 32)


def rename(au, old, new):
    """the access unit with its slice NAL units of type `old` called `new` (the type sits in bits 1..6 of the header's first byte)"""
    out = bytearray()
    for n in orc.split_nals(au):
        n = bytearray(n)
        i = 0
        while n[i] == 0:
            i += 1
        if (n[i + 1] >> 1) & 63 == old:
            n[i + 1] = (n[i + 1] & 0x81) | (new << 1)
        out += n
    return bytes(out)


def rasl_of(types, k):
    """indices of the RASL pictures that belong to the CRA picture at index k"""
    out = []
    for i in range(k + 1, len(types)):
        if 16 <= types[i] <= 23:
            break
        if types[i] in (8, 9):
            out.append(i)
    return out


def discard_prior(au):
    """the access unit with no_output_of_prior_pics_flag = 1 in its IDR / BLA slice NAL units (the second bit of the slice segment header)"""
    out = bytearray()
    for n in orc.split_nals(au):
        n = bytearray(n)
        i = 0
        while n[i] == 0:
            i += 1
        if 16 <= (n[i + 1] >> 1) & 63 <= 20:
            n[i + 3] |= 0x40
        out += n
    return bytes(out)


def tid_of(au):
    """TemporalId of the access unit's slice NAL units"""
    for n in orc.split_nals(au):
        i = 0
        while n[i] == 0:
            i += 1
        if (n[i + 1] >> 1) & 63 < 32:
            return (n[i + 2] & 7) - 1
    raise ValueError("no slice")


def layered(seed, n=26, w=64, h=64, **kw):
    cfg = dict(gop=(2, 4, 8)[seed % 3], temporal_layers=1, open_gop=seed & 1, intra_period=24, b_slices=50, num_refs=1 + seed % 4, tmvp=1)
    cfg.update(kw)
    g = orc.OracleGen(w, h, seed=seed, **cfg)
    aus = [g.picture() for _ in range(n)]
    g.close()
    return aus


def lossy(seed, n=26, w=64, h=64, every=5, **extra):
    """(access units with some lost, how many were lost): never the first picture, never an IDR or CRA picture"""
    kw = dict(intra_period=12, num_refs=1 + seed % 4, tmvp=1)
    if seed & 1:
        kw.update(gop=(2, 4, 8)[seed % 3], b_slices=50)
    else:
        kw.update(long_term=(seed >> 1) & 1)
    kw.update(extra)
    g = orc.OracleGen(w, h, seed=seed, **kw)
    aus = [g.picture() for _ in range(n)]
    g.close()
    types = [vcl_type(a) for a in aus]
    lose = [i for i in range(1, n) if types[i] not in (19, 21) and i % every == 2]
    return [(i, a) for i, a in enumerate(aus) if i not in lose], aus, lose
