// tests/hostcheck/statements.cpp -- host build of the statement functions the kernels share through hevc_core.h, for the CPU tests that hold them to the numpy
// restatements: me-coarse's arithmetic (me_*: the quarter sample, the coarse stage's cost, key and centre, the admissibility rule, the second-window rule and
// the fine stage's candidate order; the loops around them are plain C++ here, the kernels' are lanes and LDS windows; tests/me_coarse_model.py), weightp's
// (wp_*; tests/wp_model.py) and intra-refresh's (ir_*; tests/ir_model.py); and of the decoder's input-block layout (dec_frame.h DecInputLayout;
// tests/test_dec_input_layout.py) and the encoder's array lengths and partitions (enc_layout.h EncLayout; tests/test_enc_layout.py).  Test infrastructure.
#include <cstring>
#include "../../kvazzup_amd/csrc/hevc_core.h"
#include "../../kvazzup_amd/csrc/dec_frame.h"
#include "../../kvazzup_amd/csrc/enc_layout.h"

using namespace kvzx;

namespace {
inline int px(const uint8_t *p, int w, int h, int x, int y) { return p[(size_t)clip3(0, h - 1, y) * w + clip3(0, w - 1, x)]; }
}

extern "C" {

void hc_quarter(const uint8_t *src, int cw, int ch, uint8_t *q)
{
  for (int y = 0; y < ch / 4; y++) for (int x = 0; x < cw / 4; x++) q[(size_t)y * (cw / 4) + x] = (uint8_t)me_quarter_sample(src + (size_t)4 * y * cw + 4 * x, cw);
}

// the centres [32x32 block][2] of one reference: cur_q, ref_q = quarter pictures (cw / 4 x ch / 4)
void hc_coarse(const uint8_t *cur_q, const uint8_t *ref_q, int cw, int ch, int rq, int lam, int tile_rows, int tile_cols, int mv_frame, int16_t *centres)
{
  const int qw = cw / 4, qh = ch / 4, wq = 2 * rq + 1;
  for (int by = 0; by < ch / 32; by++)
    for (int bx = 0; bx < cw / 32; bx++) {
      int ty0, ty1, tx0, tx1;
      me_tile_span(ch >> 6, tile_rows, by >> 1, true, &ty0, &ty1);
      me_tile_span(cw >> 6, tile_cols, bx >> 1, false, &tx0, &tx1);
      unsigned long long best = ~0ull;
      for (int dyi = 0; dyi < wq; dyi++)
        for (int dxi = 0; dxi < wq; dxi++) {
          if (!me_axis_ok(4 * (dyi - rq), by * 32, ty0, ty1, ch, mv_frame) || !me_axis_ok(4 * (dxi - rq), bx * 32, tx0, tx1, cw, mv_frame)) continue;
          uint32_t sad = 0;
          for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++) sad += (uint32_t)iabs((int)cur_q[(size_t)(by * 8 + y) * qw + bx * 8 + x] - px(ref_q, qw, qh, bx * 8 + x + dxi - rq, by * 8 + y + dyi - rq));
          const unsigned long long key = me_coarse_key(sad, dxi, dyi, rq, (uint32_t)lam);
          if (key < best) best = key;
        }
      int cx, cy;
      me_coarse_centre(best, rq, &cx, &cy);
      centres[2 * (by * (cw / 32) + bx)] = (int16_t)cx; centres[2 * (by * (cw / 32) + bx) + 1] = (int16_t)cy;
    }
}

// the fine stage of a whole picture: refs[k] = the plane searched for reference k, centres [4][block][2] as hc_coarse filed them
void hc_fine(const uint8_t *src, const uint8_t *const *refs, const int16_t *centres, int cw, int ch, int nref, int R, int rq, int lam, int tile_rows, int tile_cols,
             int mv_frame, int me_early, uint8_t *log2, int16_t *mv, uint8_t *rf, uint8_t *early)
{
  const int W = 2 * R + 1, nblk = (cw / 32) * (ch / 32);
  (void)rq;
  for (int by = 0; by < ch / 32; by++)
    for (int bx = 0; bx < cw / 32; bx++) {
      const int x0 = bx * 32, y0 = by * 32, blk = by * (cw / 32) + bx;
      auto put = [&](int qy, int qx, int l2, int mx, int my, int r) {
        for (int y = 0; y < 2; y++) for (int x = 0; x < 2; x++) { const int i = (y0 / 8 + qy * 2 + y) * (cw / 8) + x0 / 8 + qx * 2 + x; log2[i] = (uint8_t)l2; mv[2 * i] = (int16_t)mx; mv[2 * i + 1] = (int16_t)my; rf[i] = (uint8_t)r; }
      };
      early[blk] = 0;
      if (me_early) {
        uint32_t s0 = 0;
        for (int y = 0; y < 32; y++) for (int x = 0; x < 32; x++) s0 += (uint32_t)iabs((int)src[(size_t)(y0 + y) * cw + x0 + x] - (int)refs[0][(size_t)(y0 + y) * cw + x0 + x]);
        if (s0 <= 64u * (uint32_t)lam) { early[blk] = 1; for (int q = 0; q < 4; q++) put(q >> 1, q & 1, 5, 0, 0, 0); continue; }
      }
      int ty0, ty1, tx0, tx1;
      me_tile_span(ch >> 6, tile_rows, by >> 1, true, &ty0, &ty1);
      me_tile_span(cw >> 6, tile_cols, bx >> 1, false, &tx0, &tx1);
      unsigned long long best[5] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
      for (int it = 0; it < 2 * nref; it++) {
        const int k = it >> 1, win = it & 1;
        int ox = 0, oy = 0;
        if (win) { ox = centres[2 * (k * nblk + blk)]; oy = centres[2 * (k * nblk + blk) + 1]; if (!me_second_window(ox, oy, R)) continue; }
        for (int dyi = 0; dyi < W; dyi++)
          for (int dxi = 0; dxi < W; dxi++) {
            const int dx = ox + dxi - R, dy = oy + dyi - R;
            if (!me_axis_ok(dy, y0, ty0, ty1, ch, mv_frame) || !me_axis_ok(dx, x0, tx0, tx1, cw, mv_frame)) continue;
            uint32_t sq[4] = {0, 0, 0, 0};
            for (int y = 0; y < 32; y++) for (int x = 0; x < 32; x++) sq[(y >> 4) * 2 + (x >> 4)] += (uint32_t)iabs((int)src[(size_t)(y0 + y) * cw + x0 + x] - px(refs[k], cw, ch, x0 + x + dx, y0 + y + dy));
            const uint32_t rate = ((uint32_t)lam * (uint32_t)(mvd_bits(dx * 4) + mvd_bits(dy * 4) + ref_bins(k, nref))) >> 4;
            for (int q = 0; q < 4; q++) { const unsigned long long key = me_fine_key(sq[q] + rate, k, win, dyi * W + dxi); if (key < best[q]) best[q] = key; }
            const unsigned long long key = me_fine_key(sq[0] + sq[1] + sq[2] + sq[3] + rate, k, win, dyi * W + dxi);
            if (key < best[4]) best[4] = key;
          }
      }
      const uint32_t pen = ((uint32_t)lam * 8u) >> 4;
      const bool split = pen + (uint32_t)(best[0] >> 17) + (uint32_t)(best[1] >> 17) + (uint32_t)(best[2] >> 17) + (uint32_t)(best[3] >> 17) < (uint32_t)(best[4] >> 17);
      for (int q = 0; q < 4; q++) {
        const unsigned long long key = split ? best[q] : best[4];
        const int k = (int)((key >> 14) & 7), win = (int)((key >> 13) & 1), ci = (int)(key & 0x1fff);
        const int cx = win ? centres[2 * (k * nblk + blk)] : 0, cy = win ? centres[2 * (k * nblk + blk) + 1] : 0;
        put(q >> 1, q & 1, split ? 4 : 5, (cx + ci % W - R) * 4, (cy + ci / W - R) * 4, k);
      }
    }
}

void hw_moments(uint64_t s1, uint64_t s2, uint64_t n, int64_t *mv) { wp_moments(s1, s2, n, &mv[0], &mv[1]); }
uint32_t hw_isqrt(uint64_t v) { return wp_isqrt(v); }
// out = {w, o, candidate}
void hw_candidate(int64_t mc, int64_t vc, int64_t mr, int64_t vr, int32_t *out) { int w, o; out[2] = wp_candidate(mc, vc, mr, vr, &w, &o) ? 1 : 0; out[0] = w; out[1] = o; }
int hw_accept(int cand, uint64_t plain, uint64_t wt) { return wp_accept(cand != 0, plain, wt) ? 1 : 0; }
int hw_sample(int s, int w, int o) { return wp_sample(s, w, o); }
int hw_pred14(int p, int w, int o) { return wp_pred14(p, w, o); }

// the whole decision of picture `cur` against input picture `ref` (planes of `pitch` bytes a row, width x height visible) as the kernels compose it: sums, moments,
// candidate, check, verdict.  out = {flag, w, o}
void hw_decide(const uint8_t *cur, const uint8_t *ref, int width, int height, int pitch, int32_t *out)
{
  uint64_t s[2][2] = {{0, 0}, {0, 0}};
  const uint8_t *pl[2] = {cur, ref};
  for (int k = 0; k < 2; k++)
    for (int y = 0; y < height; y++) for (int x = 0; x < width; x++) { const uint64_t v = pl[k][(size_t)y * pitch + x]; s[k][0] += v; s[k][1] += v * v; }
  int64_t m[2], v[2];
  for (int k = 0; k < 2; k++) wp_moments(s[k][0], s[k][1], (uint64_t)width * height, &m[k], &v[k]);
  int w, o;
  const bool cand = wp_candidate(m[0], v[0], m[1], v[1], &w, &o);
  uint64_t plain = 0, wt = 0;
  for (int y = 0; y < height; y += 4) for (int x = 0; x < width; x += 4) {
    const int c = cur[(size_t)y * pitch + x], r = ref[(size_t)y * pitch + x];
    plain += (uint64_t)iabs(c - r); wt += (uint64_t)iabs(c - wp_sample(r, w, o));
  }
  const bool on = wp_accept(cand, plain, wt);
  out[0] = on ? 1 : 0; out[1] = on ? w : 64; out[2] = on ? o : 0;
}

int hi_step(int cw, int N) { return ir_step(cw, N); }
int hi_cycle(int cw, int N) { return ir_cycle(cw, N); }
// out = {s_j, e_j}
void hi_band(int cw, int N, int j, int32_t *out) { out[0] = ir_band_start(cw, N, j); out[1] = ir_band_end(cw, N, j); }
int hi_position(int cw, int N, int poc) { return ir_position(cw, N, poc); }
int hi_forced_quarters(int x0, int s, int e) { return ir_forced_quarters(x0, s, e); }
int hi_clean_block(int x0, int s, int j) { return ir_clean_block(x0, s, j) ? 1 : 0; }
int hi_mvx_max(int x0, int s) { return ir_mvx_max(x0, s); }
int hi_last_column(int xb, int nb, int e, int cw) { return ir_last_column(xb, nb, e, cw) ? 1 : 0; }
// every schedule of a coded width in one call: out[2 (N - 2)] = m, out[2 (N - 2) + 1] = n for N = 2 .. 255
void hi_schedules(int cw, int32_t *out) { for (int N = 2; N <= 255; N++) { out[2 * (N - 2)] = ir_step(cw, N); out[2 * (N - 2) + 1] = ir_cycle(cw, N); } }
// the bands of one cycle: out[2 j] = s_j, out[2 j + 1] = e_j for j < ir_cycle(cw, N); returns the cycle's length
int hi_bands(int cw, int N, int32_t *out) { const int n = ir_cycle(cw, N); for (int j = 0; j < n; j++) { out[2 * j] = ir_band_start(cw, N, j); out[2 * j + 1] = ir_band_end(cw, N, j); } return n; }

// ---- the decoder's input block (dec_frame.h DecInputLayout).  out[0..11] = the parts' offsets in block order (region table, CTB table, tile ids, SAO parameters,
// scaling factors, weights, frame descriptor, neighbour map, transform blocks, level words, second vectors, index list), out[12] = fixed_bytes(),
// out[13] = upload_bytes(); sizes = {B4Rec, TuRange, SaoParams, KVZ_SCALING_BYTES, DecWt, DecFrame, DecTu, B4L1}: what a restatement needs of the product's structs
void hd_input_layout(int pw, int ph, int ctb_log2, uint64_t ntu, uint64_t nlev, uint64_t nb4x, int bi, uint64_t *out, uint64_t *sizes)
{
  const DecInputLayout l(pw, ph, ctb_log2, (size_t)ntu, (size_t)nlev, (size_t)nb4x, bi != 0);
  const size_t o[14] = {l.region_off, l.ctu_off, l.tile_off, l.sao_off, l.scaling_off, l.wt_off, l.frame_off, l.nb_off, l.tu_off, l.lev_off, l.x_off, l.i_off, l.fixed_bytes(), l.upload_bytes()};
  const size_t z[8] = {sizeof(B4Rec), sizeof(TuRange), sizeof(SaoParams), KVZ_SCALING_BYTES, sizeof(DecWt), sizeof(DecFrame), sizeof(DecTu), sizeof(B4L1)};
  for (int i = 0; i < 14; i++) out[i] = o[i];
  for (int i = 0; i < 8; i++) sizes[i] = z[i];
}

// ---- the encoder's arrays (enc_layout.h EncLayout) of a width x height encoder, band_rows > 0: a band of that many CTU rows.  out[0..41], in the order of
// tests/hc.py ENC_LAYOUT: the coded size, the counts (elements of each array's type), the caps, and the offsets of the parts of the arrays that are cut up;
// out[42..44] the three planes' edge-row offsets, out[45..51] the seven CU arrays' offsets
void he_layout(int width, int height, int band_rows, uint64_t *out)
{
  const EncLayout l(width, height, band_rows);
  const size_t o[42] = {(size_t)l.cw, (size_t)l.ch, (size_t)l.rows, l.npx, l.nb8, l.n16, l.nctu, l.plane(0), l.plane(1), l.cu_bytes, l.cu_mv, l.col, l.mc_q, l.mc_centres,
                        l.sc_blocks, l.sync, l.edge_col, l.edge_row, l.me_block, l.intra_scratch, l.intra_order, l.trace, (size_t)l.tok_cap, l.tok_buf, l.tok_count, l.tok_seg,
                        l.tok_list, l.tok_dense_cap, l.stage_cap, l.out_cap, l.ctx_save, l.sub,
                        l.me_cand_off, l.ip_arrive_off, l.ip_scratch_off, l.ic16_off, l.ic32_off, l.im8_off, l.im16_off, l.im32_off, l.edge_col_off(1), l.edge_col_off(2)};
  for (int i = 0; i < 42; i++) out[i] = o[i];
  for (int c = 0; c < 3; c++) out[42 + c] = l.edge_row_off(c);
  for (int i = 0; i < 7; i++) out[45 + i] = l.cu_off(i);
}

}
