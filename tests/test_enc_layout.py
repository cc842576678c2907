"""The encoder's array lengths and partitions (kvazzup_amd/csrc/enc_layout.h EncLayout) against a restatement of the expressions they replaced.

Before the layout had one statement, Encoder::init spelled every length out where it allocated (most of them twice, the clear repeating the allocation), and
point_me_block, point_chain, picture_frame and debug_copy cut the partitioned arrays up by formulas of their own.  restated() below copies those expressions
from that encoder.hip, with the line each stood on; nothing in it calls the library.  (a) every count and cap is the restatement's; (b) the parts of every
partitioned array are disjoint, in order and inside the allocation, ip_scratch lies on a multiple of 8 bytes and the counter arrays are multiples of 16 bytes --
the check the separate formulas never had."""
import pytest

import hc

# width, height, band rows: the smallest picture the ABI takes (coded 128x64, the floor), the small test size, 1080p, 8K, and a band of an 8K picture
CASES = [(16, 16, 0), (192, 128, 0), (1920, 1080, 0), (7680, 4320, 0), (7680, 4320, 17)]
REFS = 4      # hevc_core.h KVZ_MAX_LP_REFS


def restated(width, height, band_rows):
    cw, ch = (width + 63) & ~63, (height + 63) & ~63                          # encoder.hip:122
    if cw < 128:                                                              # :123
        cw = 128
    rows = ch // 64                                                           # :124
    npx = cw * ch; nb8 = npx // 64                                            # :141
    nctu = (cw // 64) * rows                                                  # :180, :223
    n16 = (cw // 16) * (ch // 16)                                             # :279
    o = dict(cw=cw, ch=ch, rows=rows, npx=npx, nb8=nb8, n16=n16, nctu=nctu)
    o["plane0"], o["plane1"] = npx, npx // 4                                  # :144  c ? npx / 4 : npx
    o["cu_bytes"] = nb8 * 7                                                   # :150
    o["cu_mv"] = nb8 * 2                                                      # :151  nb8 * 2 * sizeof(int16_t)
    o["col"] = nb8 // 4                                                       # :154  nb8 / 4 * sizeof(ColMv)
    o["mc_q"] = npx // 16                                                     # :155
    o["mc_centres"] = REFS * (nb8 // 16) * 2                                  # :158  KVZ_MAX_LP_REFS * (nb8 / 16) * 2 * sizeof(int16_t)
    o["sc_blocks"] = ((width + 31) // 32) * ((height + 31) // 32) * 2         # :173-174  bw * bh * 2 * sizeof(uint32_t); hevc_core.h:224 sc_visible_blocks
    o["sync"] = (rows * (cw // 64) * 3 + 2 + 3) & ~3                          # :209, :278, :282
    o["edge_col"] = nctu * 128                                                # :211, :293  nctu * 128 * sizeof(uint32_t)
    o["edge_row"] = nctu * 32                                                 # :212, :294  nctu * 32 * 8 bytes
    o["me_block"] = n16 + 2 + n16 // 4 + n16 // 4 + (n16 // 4) * 40           # :279, :282
    o["intra_scratch"] = nb8 * 4 + nb8 + nb8 // 4 + nb8 + nb8 // 4 + nb8 // 16 + 64      # :221
    wc, nr = cw // 64, band_rows if band_rows > 0 else rows                   # :287
    o["intra_order"] = sum(1 for d in range(wc + 2 * nr) for cy in range(nr) if 0 <= d - 2 * cy < wc)      # :289  order.size()
    o["trace"] = rows * (cw // 64) * 72                                       # :296
    o["tok_cap"] = 49152                                                      # :224
    o["tok_buf"] = nctu * o["tok_cap"]                                        # :225
    o["tok_count"] = nctu * 2                                                 # :226
    o["tok_seg"] = nctu * 16 * 17 * 2                                         # :227
    o["tok_list"] = 1 + nctu * 16 * 4                                         # :229
    o["tok_dense_cap"] = min(nctu * o["tok_cap"], 1 << 27)                    # :231-232
    o["stage_cap"] = min(o["tok_dense_cap"] * 2 + 256 * rows, 0xfff00000)     # :235
    o["out_cap"] = min(cw * ch * 3 + 4096, o["stage_cap"])                    # :236
    o["ctx_save"] = 40 * rows                                                 # :246
    o["sub"] = 3 * rows                                                       # :250
    o["me_cand_off"] = n16                                                    # :26   f.me_cand = block + n16
    o["ip_arrive_off"] = n16 + 1 + n16 // 4                                   # :27   f.ip_arrive = f.me_cand + 1 + n16 / 4
    o["ip_scratch_off"] = (n16 + 1 + n16 // 4 + n16 // 4 + 1) & ~1            # :27
    o["ic16_off"] = nb8 * 4                                                   # :320  p += nb8 * 4
    o["ic32_off"] = o["ic16_off"] + nb8                                       # :320  p += nb8
    o["im8_off"] = o["ic32_off"] + nb8 // 4                                   # :320  p += nb8 / 4
    o["im16_off"] = o["im8_off"] + nb8                                        # :321  p += nb8
    o["im32_off"] = o["im16_off"] + nb8 // 4                                  # :321  p += nb8 / 4
    o["edge_col_off"] = [0, nctu * 64, nctu * 96]                             # :35
    o["edge_row_off"] = [0, nctu * 16, nctu * 24]                             # :36
    o["cu_off"] = [i * nb8 for i in range(7)]                                 # :729-730, :1333
    return o


def parts_of(o):
    """(array, its length, [(part, offset, length)]) in the array's own elements.  The parts' lengths are what their users index (hevc_core.h EncFrame): a progress
    word per luma row of a CTU and per chroma row of either plane, a word of four samples per four columns; me_cand [0] a count, [1 ..] the 32x32 blocks;
    ip_scratch 20 64-bit words a 32x32 block; the intra scratch's cost words (4 bytes) and mode bytes per 8x8, 16x16 and 32x32 block"""
    n16, nb8, nctu = o["n16"], o["nb8"], o["nctu"]
    return [
        ("me_block", o["me_block"], [("me_cost16", 0, n16), ("me_cand", o["me_cand_off"], 1 + n16 // 4), ("ip_arrive", o["ip_arrive_off"], n16 // 4),
                                     ("ip_scratch", o["ip_scratch_off"], (n16 // 4) * 20 * 2)]),
        ("edge_col", o["edge_col"], [("y", o["edge_col_off"][0], nctu * 64), ("cb", o["edge_col_off"][1], nctu * 32), ("cr", o["edge_col_off"][2], nctu * 32)]),
        ("edge_row", o["edge_row"], [("y", o["edge_row_off"][0], nctu * 16), ("cb", o["edge_row_off"][1], nctu * 8), ("cr", o["edge_row_off"][2], nctu * 8)]),
        ("intra_scratch", o["intra_scratch"], [("ic8", 0, nb8 * 4), ("ic16", o["ic16_off"], nb8 // 4 * 4), ("ic32", o["ic32_off"], nb8 // 16 * 4),
                                               ("im8", o["im8_off"], nb8), ("im16", o["im16_off"], nb8 // 4), ("im32", o["im32_off"], nb8 // 16)]),
        ("cu_bytes", o["cu_bytes"], [("cu%d" % i, o["cu_off"][i], nb8) for i in range(7)]),
    ]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_band%d" % c)
def test_counts_and_caps_are_the_restatement(case):
    got, want = hc.enc_layout(*case), restated(*case)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_band%d" % c)
def test_parts_are_disjoint_in_order_and_inside(case):
    got = hc.enc_layout(*case)
    for name, total, parts in parts_of(got):
        end = 0
        for part, off, n in parts:
            assert n > 0, (name, part)
            assert off >= end, "%s: %s at %d begins inside its predecessor, which ends at %d" % (name, part, off, end)
            end = off + n
        assert end <= total, "%s: its last part ends at %d, the array at %d" % (name, end, total)
    assert got["ip_scratch_off"] * 4 % 8 == 0, "ip_scratch (64-bit words) at byte %d of its block" % (got["ip_scratch_off"] * 4)
    assert got["sync"] * 4 % 16 == 0, "the progress counters are %d bytes, k_picture_begin clears 16 at a time" % (got["sync"] * 4)
    assert got["sync"] >= got["nctu"] * 3 + 2, "a counter per CTU and plane, the ticket word and the word behind it"
