""""uvgx low-delay GOP v1" (kvazaar.h lp-gop): the statement of record of what gop=lp-g<g>d<d>t1 with lp-gop=1 makes of a stream.

t is a picture's POC (pictures since the last IDR picture, the IDR picture itself 0), g / d the numbers of the gop string, n = max(1, lp-refs).
Key pictures are the pictures with t % g == 0.  A P picture lies on one of d QP layers (the key picture on layer 1) and is coded at QP + layer; it refers
to the previous picture, then to the most recent key picture within reach, then to the pictures before the previous one -- min(n, t) pictures in all,
in list 0 by increasing distance.  The search itself is tests/lp_refs_model.search() handed the reference planes in that order."""

REACH = 7          # the oldest picture a P picture can refer to: what the encoder's working sets still hold of it (kSets - 1)


def is_key(t, g):
    return t % g == 0


def layer(t, g, d):
    """QP layer 1 .. d of P picture t >= 1"""
    assert t >= 1 and g >= 1 and d >= 1
    pos = ((t - 1) % g) + 1
    mod = [g] + [1 << (d - 1 - i) for i in range(1, d)]
    l = 1
    while l < d and pos % mod[l - 1] != 0:
        l += 1
    return l


def picture_qp(q, t, g, d):
    """QP of picture t when it would have had q without the option: IDR pictures keep q"""
    return q if t == 0 else max(0, min(51, q + layer(t, g, d)))


def ref_pocs(t, g, n):
    """POCs of the references of P picture t in list 0 order (increasing distance)"""
    assert t >= 1
    n = max(1, n)
    m = min(n, t)
    s = [t - 1]
    if m >= 2:
        k = ((t - 2) // g) * g                       # the most recent key picture <= t - 2
        if t - k <= REACH:
            s.append(k)
    back = 2
    while len(s) < m:
        assert back <= REACH
        if t - back not in s:
            s.append(t - back)
        back += 1
    return sorted(s, reverse=True)


def ref_dists(t, g, n):
    """POC distances of the references, list 0 order"""
    return [t - p for p in ref_pocs(t, g, n)]


def check_properties(g, n, pictures=200):
    """what section 9d promises of every set: its size, its reach, and that a picture's reference picture set is its reference set -- nothing kept for later"""
    prev = set()
    for t in range(1, pictures):
        s = ref_pocs(t, g, n)
        assert len(s) == len(set(s)) == min(max(1, n), t), (g, n, t, s)
        assert s[0] == t - 1 and all(0 <= p < t for p in s), (g, n, t, s)
        assert max(t - p for p in s) <= REACH, (g, n, t, s)
        assert set(s) <= prev | {t - 1}, (g, n, t, s, prev)
        if g == 1 or n <= 1:
            assert s == [t - 1 - k for k in range(len(s))], (g, n, t, s)
        prev = set(s)
    return True


def structure(period, pictures, g, d, n, qp):
    """per picture of a stream with intra period `period` (0: the first picture only): dict(idr, poc, qp, layer, refs (POCs), dists)"""
    out = []
    t = 0
    for i in range(pictures):
        idr = i == 0 or (period > 0 and i % period == 0)
        t = 0 if idr else t + 1
        if idr:
            out.append(dict(idr=True, poc=0, qp=qp, layer=0, refs=[], dists=[]))
        else:
            out.append(dict(idr=False, poc=t, qp=picture_qp(qp, t, g, d), layer=layer(t, g, d), refs=ref_pocs(t, g, n), dists=ref_dists(t, g, n)))
    return out
