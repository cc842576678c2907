// kvazzup_amd/csrc/enc_layout.h -- how long every encoder array is whose length is a formula, and where the parts lie in the arrays that are cut up, stated
// ONCE: Encoder::init allocates by it, point_me_block / point_chain / picture_frame / debug_copy point by it.  Host only, no HIP.  Counts are ELEMENTS of the
// array's type (given with each), offsets are elements from the array's start.  Which of the arrays an encoder has is its options' business (encoder.hip).
#pragma once
#include <stddef.h>
#include "hevc_core.h"

namespace kvzx {

struct EncLayout {
  int width, height, band_rows;      // the picture; band_rows > 0: this instance codes that many CTU rows of it
  EncLayout(int w = 0, int h = 0, int band = 0) : width(w), height(h), band_rows(band) {}
  static size_t least(size_t a, size_t b) { return a < b ? a : b; } static int most(int a, int b) { return a > b ? a : b; }
  int cw = most(128, (width + 63) & ~63), ch = (height + 63) & ~63, rows = ch / 64, wc = cw / 64;      // coded size (multiples of 64, at least 128 wide), its CTU rows and columns
  size_t npx = (size_t)cw * ch, nb8 = npx / 64, n16 = (size_t)(cw / 16) * (ch / 16), nctu = (size_t)wc * rows;      // luma samples (a chroma plane: npx / 4), 8x8 blocks (one byte each in a CU array), 16x16 blocks, CTUs (the per-CTU arrays)
  size_t plane(int c) const { return c ? npx / 4 : npx; }
  // per working set: the seven CU byte arrays back to back (log2 | intra | flags | merge_idx | mvp_idx | intra_mode | cbf), cu_mv / cu_mvd (i16), ColMv per 16x16, the quarter picture (u8), me-coarse's centres (i16 [reference][32x32 block][2]); scenecut's (S, A) per visible 32x32 block (u32)
  size_t cu_bytes = nb8 * 7, cu_mv = nb8 * 2, col = nb8 / 4, mc_q = npx / 16, mc_centres = (size_t)KVZ_MAX_LP_REFS * (nb8 / 16) * 2, sc_blocks = sc_pairs(width, height);
  size_t cu_off(int i) const { return (size_t)i * nb8; }
  static size_t sc_pairs(int w, int h) { int bw, bh; sc_visible_blocks(w, h, &bw, &bh); return (size_t)bw * bh * 2; }
  // one intra chain: a progress counter per CTU and plane, the ticket counter of k_intra_recon's workgroups and the P pictures' "has intra units" word (u32; a multiple of
  // 16 bytes: k_picture_begin zeroes it in 16-byte pieces), and per plane the CTUs' right columns (u32) and bottom rows (u64)
  size_t sync = (nctu * 3 + 2 + 3) & ~(size_t)3, edge_col = nctu * 128, edge_row = nctu * 32;
  size_t edge_col_off(int c) const { return c == 0 ? 0 : nctu * (c == 1 ? 64 : 96); } size_t edge_row_off(int c) const { return c == 0 ? 0 : nctu * (c == 1 ? 16 : 24); }
  // the me-source block (u32): me_cost16 (n16) | me_cand (1 + n16 / 4) | ip_arrive (n16 / 4) | ip_scratch ([n16 / 4][20] u64, 8-byte aligned)
  size_t me_cand_off = n16, ip_arrive_off = me_cand_off + 1 + n16 / 4, ip_scratch_off = (ip_arrive_off + n16 / 4 + 1) & ~(size_t)1, me_block = n16 + 2 + n16 / 4 + n16 / 4 + (n16 / 4) * 40;
  // intra scratch (bytes): ic8 (nb8 u32) | ic16 (nb8 / 4 u32) | ic32 (nb8 / 16 u32) | im8 (nb8) | im16 (nb8 / 4) | im32 (nb8 / 16)
  size_t ic16_off = nb8 * 4, ic32_off = ic16_off + nb8, im8_off = ic32_off + nb8 / 4, im16_off = im8_off + nb8, im32_off = im16_off + nb8 / 4, intra_scratch = im32_off + nb8 / 16 + 64;
  size_t intra_order = (size_t)wc * (band_rows > 0 ? band_rows : rows), trace = nctu * 72;      // u32: the CTUs of the rows this instance codes; u64: KVAZZUP_AMD_INTRA_TRACE
  // tokenizer: tokens per CTU slot (worst case of a 64x64 CTU is ~43k), the slots (u16), two sets of cursors that take turns (k_tok_compact), [ctu][unit][piece] {offset, length},
  // the P pictures' (unit, role) list; the dense tokens a picture may have, the GPU coder's staging bytes and the access unit's (twice the raw picture: a larger access unit is
  // not a picture this encoder makes); the GPU coder's 40 context words and {offset, length, bins} per substream row (u32)
  int tok_cap = 49152;
  size_t tok_buf = nctu * tok_cap, tok_count = nctu * 2, tok_seg = nctu * 16 * 17 * 2, tok_list = 1 + nctu * 16 * 4;
  size_t tok_dense_cap = least(tok_buf, (size_t)1 << 27), stage_cap = least(tok_dense_cap * 2 + 256 * (size_t)rows, 0xfff00000u), out_cap = least(npx * 3 + 4096, stage_cap);
  size_t ctx_save = (size_t)40 * rows, sub = (size_t)3 * rows;
};

}  // namespace kvzx
