""""uvgx intra refresh v1" (kvazaar.h intra-refresh) restated in Python: the schedule, the forced quarters, the vector bound, the mode
rule, the recovery point SEI, and check_structure(): one coded picture held to these rules.  hevc_core.h's ir_* functions (host build: tests/hostcheck) and the HIP encoder are held to it.  All integer.

cw = coded width (a multiple of 64), B = cw / 32 block columns, N = 2 .. 255 the number of P pictures a cycle may take.
  m = ceil(B / N)   block columns a picture advances
  n = ceil(B / m)   pictures of a cycle (n <= N)
  s_j = 32 m j,  e_j = min(cw, s_j + 32 m + 16):  the band of position j is the luma columns [s_j, e_j)
A cycle begins at the first P picture behind an IDR picture and again behind position n - 1; IDR pictures belong to no cycle."""

import numpy as np

# modes (bit m: mode m) whose prediction reads above-right samples, per luma block size (hevc_core.h intra_uses_above_right, cidx 0)
ABOVE_RIGHT = {3: 0x7F8000001, 4: 0x7F9F80001}


def step(cw, N):
    B = cw // 32
    return -(-B // N)


def cycle(cw, N):
    B = cw // 32
    return -(-B // step(cw, N))


def band(cw, N, j):
    """[s_j, e_j)"""
    m = step(cw, N)
    s = 32 * m * j
    return s, min(cw, s + 32 * m + 16)


def position(cw, N, poc):
    """position in its cycle of the P picture `poc` pictures behind its IDR picture (poc >= 1)"""
    return (poc - 1) % cycle(cw, N)


def record(cw, N, poc):
    """what debug_copy("ir") says of a picture: [j, s_j, e_j, n]; an IDR picture (poc 0): [-1, 0, 0, n]"""
    n = cycle(cw, N)
    if poc == 0:
        return [-1, 0, 0, n]
    j = position(cw, N, poc)
    s, e = band(cw, N, j)
    return [j, s, e, n]


def forced_quarters(x0, s, e):
    """bit k: the 16x16 quarter k (raster of 2 x 2) of the 32x32 block at x0 lies in the band"""
    q = 0
    for k in range(4):
        x = x0 + 16 * (k & 1)
        if s <= x and x + 16 <= e:
            q |= 1 << k
    return q


def clean_block(x0, s, j):
    return j >= 1 and x0 + 32 <= s


def mvx_max(x0, s):
    """a clean block and its quarters keep every vector to 4 (x0 + 32) + mvx <= 4 s (quarter samples)"""
    return 4 * (s - x0 - 32)


def last_column(xb, nb, e, cw):
    """a forced unit of size nb at xb on the band's last unit column"""
    return xb + nb == e and e < cw


def recovery_point_sei(cnt):
    """the RBSP of the prefix SEI NAL unit: payload type 6, recovery_poc_cnt = cnt as se(v), exact_match_flag 1, broken_link_flag 0"""
    v = 2 * cnt - 1 if cnt > 0 else -2 * cnt
    x, ln = v + 1, (v + 1).bit_length() - 1
    bits = "0" * ln + format(x, "b") + "1" + "0"
    if len(bits) % 8:
        bits += "1"
        bits += "0" * (-len(bits) % 8)
    payload = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    return bytes([6, len(payload)]) + payload + b"\x80"


def parse_recovery_point(rbsp):
    """(recovery_poc_cnt, exact_match_flag, broken_link_flag) of an SEI RBSP that holds one recovery point message and nothing else"""
    assert rbsp[0] == 6 and rbsp[1] == len(rbsp) - 3 and rbsp[-1] == 0x80, rbsp.hex()
    bits = "".join(format(b, "08b") for b in rbsp[2:-1])
    z = bits.index("1")
    v = int(bits[z:2 * z + 1], 2) - 1
    pos = 2 * z + 1
    cnt = (v + 1) // 2 if v & 1 else -(v // 2)
    exact, broken = int(bits[pos]), int(bits[pos + 1])
    rest = bits[pos + 2:]
    assert rest == "" or (rest[0] == "1" and set(rest[1:]) <= {"0"}), rest
    return cnt, exact, broken


# ---- a coded picture against the rules (the HIP encoder: tests/test_gpu_intra_refresh.py; the checker: tests/test_oracle_weightp_intra_refresh.py)
def avail(x, y, xn, yn, cw):
    """z-scan availability of the sample (xn, yn) for the block at (x, y): one slice, no tiles, 64x64 coding tree blocks, 8x8 granularity"""
    if xn < 0 or yn < 0 or xn >= cw:
        return False
    if (xn >> 6, yn >> 6) != (x >> 6, y >> 6):
        return (yn >> 6, xn >> 6) < (y >> 6, x >> 6)
    z = lambda a, b: sum((((a >> 3) >> k) & 1) << (2 * k) | (((b >> 3) >> k) & 1) << (2 * k + 1) for k in range(3))
    return z(xn & 63, yn & 63) < z(x & 63, y & 63)


def check_structure(d, poc, cw, N, free):
    """one picture's debug arrays (the HIP encoder's debug_all() or the checker's debug()) against the statement; returns how many cells it looked at per rule"""
    seen = {"band": 0, "clean": 0, "last": 0, "excluded_matter": 0}
    assert d["ir"] == record(cw, N, poc), (poc, d["ir"])
    if poc == 0:
        return seen
    j, s, e, _ = d["ir"]
    intra, log2, mode, mv = d["cu_intra"], d["cu_log2"], d["cu_intra_mode"], d["cu_mv"]
    rows = intra.shape[0]
    band = intra[:, s // 8:e // 8]
    assert band.all(), "picture %d: %d cells of the band [%d, %d) are not intra" % (poc, int((band == 0).sum()), s, e)
    seen["band"] += band.size
    assert set(np.unique(log2[:, s // 8:e // 8])) <= ({4} if free < 2 else {3, 4})
    if not free:
        outside = np.concatenate([intra[:, :s // 8], intra[:, e // 8:]], axis=1)
        assert not outside.any(), "picture %d: intra-in-p=0 and %d intra cells outside the band" % (poc, int(outside.sum()))
    if j >= 1:
        for x0 in range(0, s, 32):
            assert clean_block(x0, s, j)
            blk_mv, blk_in = mv[:, x0 // 8:x0 // 8 + 4, 0].astype(np.int64), intra[:, x0 // 8:x0 // 8 + 4]
            bad = (blk_in == 0) & (4 * (x0 + 32) + blk_mv > 4 * s)
            assert not bad.any(), "picture %d: a clean block at x0 = %d has a vector beyond the bound (mvx %d, limit %d)" % (poc, x0, int(blk_mv[bad].max()), mvx_max(x0, s))
            seen["clean"] += int((blk_in == 0).sum())
    if e < cw:
        cx = e // 8 - 1
        for cy in range(rows):
            l2 = int(log2[cy, cx]); nb = 1 << l2
            xb, yb = e - nb, (cy * 8) & ~(nb - 1)
            assert last_column(xb, nb, e, cw)
            seen["last"] += 1
            if avail(xb, yb, xb + nb, yb - 1, cw):
                seen["excluded_matter"] += 1
                assert not (ABOVE_RIGHT[l2] >> int(mode[cy, cx])) & 1, "picture %d: the unit at (%d, %d) size %d takes mode %d, which reads above-right samples" % (poc, xb, yb, nb, int(mode[cy, cx]))
    return seen
