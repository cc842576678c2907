// tests/hostcoarse/hostcoarse.cpp -- host build of the arithmetic the kernels of "uvgx coarse-to-fine search v1" (me-coarse) share
// through hevc_core.h: the quarter sample, the coarse stage's cost, key and centre, the admissibility rule, the second-window rule and the fine stage's
// candidate order.  The loops around them are plain C++ here (the kernels' are lanes and LDS windows); tests/test_me_coarse_model.py holds the result to
// the numpy statement tests/me_coarse_model.py.  Test infrastructure.
#include <cstring>
#include "../../kvazzup_amd/csrc/hevc_core.h"

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

}
