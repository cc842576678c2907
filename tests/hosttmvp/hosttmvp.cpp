// tests/hosttmvp/hosttmvp.cpp -- host build of what "tmvp" adds to the product's serial code, for tests/test_tmvp_host.py: the parameter sets and slice
// segment headers with temporal motion vector prediction (hevc_headers.h) and the merge / AMVP candidate lists with a collocated record (hevc_core.h).
// Test infrastructure.
#include <cstring>
#include <vector>
#include "../../kvazzup_amd/csrc/hevc_core.h"
#include "../../kvazzup_amd/csrc/hevc_headers.h"

using namespace kvzx;

extern "C" {

// The access unit of a picture `poc` pictures after its IDR picture (poc 0: the IDR picture), parameter sets first, with one 2-byte substream per CTU row
// (wpp) or tile: Annex B bytes -> out; returns their count, -1 when cap is too small or the substreams do not fit the tiling.
int ht_access_unit(int w, int h, int lp_refs, int tmvp, int sao, int wpp, int tile_rows, int tile_cols, int slices, int poc, uint8_t *out, int cap)
{
  StreamParams s{};
  s.cw = (w + 63) & ~63; s.ch = (h + 63) & ~63; s.width = w; s.height = h; s.qp = 32; s.wpp = wpp; s.deblock = 1; s.fps_num = 30; s.fps_den = 1;
  s.sao = sao; s.lp_refs = lp_refs; s.tmvp = tmvp; s.tile_rows = tile_rows; s.tile_cols = tile_cols; s.slices = slices;
  const int hc = s.ch / 64;
  int nsub = 0;
  for (int tr = 0; tr < tile_rows; tr++) nsub += (wpp ? tile_row_first(hc, tile_rows, tr + 1) - tile_row_first(hc, tile_rows, tr) : 1) * tile_cols;
  std::vector<std::vector<uint8_t>> rows((size_t)nsub, std::vector<uint8_t>{0xa5, 0x80});
  std::vector<uint8_t> au;
  if (!assemble_access_unit(au, s, poc == 0, poc, true, rows, nsub)) return -1;
  if ((int)au.size() > cap) return -1;
  memcpy(out, au.data(), au.size());
  return (int)au.size();
}

// The motion field of a P picture (per 8x8 block log2 3..5, intra, mv (x, y), ref, cbf; a tile grid) and the previous picture's collocated record
// (col: ColMv per 16x16 block, NULL: none).  For the inter CU at (x0, y0) of size 1 << log2: merge[5][3] = the merge candidates (mvx, mvy, ref) with nref
// active references, amvp[2][2] = the AMVP candidates for the CU's own reference, sig[5] = the signalling {flags, merge_idx, mvp_idx, mvdx, mvdy}.
void ht_cands(int cw, int ch, int tile_rows, int tile_cols, int nref, const uint8_t *log2, const uint8_t *intra, const int16_t *mv, const uint8_t *ref,
              const uint8_t *cbf, const int16_t *col, int x0, int y0, int cl, int32_t *merge, int32_t *amvp, int32_t *sig)
{
  EncFrame f;
  memset(&f, 0, sizeof(f));
  f.cw = cw; f.ch = ch; f.b8w = cw / 8; f.b8h = ch / 8; f.tile_rows = tile_rows; f.tile_cols = tile_cols; f.chp = pack_height(ch, tile_rows, tile_cols);
  f.cu_log2 = const_cast<uint8_t *>(log2); f.cu_intra = const_cast<uint8_t *>(intra); f.cu_mv = const_cast<int16_t *>(mv); f.cu_cbf = const_cast<uint8_t *>(cbf);
  f.cu_ref = const_cast<uint8_t *>(ref); f.nref = nref;
  const ColMv *cr = reinterpret_cast<const ColMv *>(col);
  FrameMvView v{f};
  const int n = 1 << cl;
  const FiveNb q = five_neighbours(v, f.cw, f.chp, x0, y0, n);
  const ColMv cb = col_block(cr, cw, ch, x0, y0, n);
  const NbMv t0 = temporal_cand(cb, 0), tr = temporal_cand(cb, ref[b8idx(f, x0, y0)]);
  int cmx[5], cmy[5], cref[5], px[2], py[2];
  merge_cand_list(q, cmx, cmy, cref, nref, cr ? &t0 : nullptr);
  amvp_cand_list(q, px, py, ref[b8idx(f, x0, y0)], cr ? &tr : nullptr);
  for (int k = 0; k < 5; k++) { merge[3 * k] = cmx[k]; merge[3 * k + 1] = cmy[k]; merge[3 * k + 2] = cref[k]; }
  for (int k = 0; k < 2; k++) { amvp[2 * k] = px[k]; amvp[2 * k + 1] = py[k]; }
  const CuSignal r = decide_signalling_values(v, f.cw, f.chp, x0, y0, cl, nref, cr);
  sig[0] = r.flags; sig[1] = r.midx; sig[2] = r.mvp; sig[3] = r.mvdx; sig[4] = r.mvdy;
}

// decide_signalling_values for every 8x8 unit of a picture, as k_inter_signal<TMVP> runs it (col NULL: k_inter_signal<false>), and the collocated record
// the picture files (col_out: ColMv per 16x16 block): what the GPU test restates the kernel's exported arrays with
void ht_picture(int cw, int ch, int tile_rows, int tile_cols, int nref, const uint8_t *log2, const uint8_t *intra, const int16_t *mv, const uint8_t *ref,
                const uint8_t *cbf, const int16_t *col, uint8_t *flags, uint8_t *midx, uint8_t *mvp, int16_t *mvd, int16_t *col_out)
{
  EncFrame f;
  memset(&f, 0, sizeof(f));
  f.cw = cw; f.ch = ch; f.b8w = cw / 8; f.b8h = ch / 8; f.tile_rows = tile_rows; f.tile_cols = tile_cols; f.chp = pack_height(ch, tile_rows, tile_cols);
  f.cu_log2 = const_cast<uint8_t *>(log2); f.cu_intra = const_cast<uint8_t *>(intra); f.cu_mv = const_cast<int16_t *>(mv); f.cu_cbf = const_cast<uint8_t *>(cbf);
  f.cu_ref = const_cast<uint8_t *>(ref); f.nref = nref;
  FrameMvView v{f};
  for (int y = 0; y < ch; y += 8)
    for (int x = 0; x < cw; x += 8) {
      const int g = b8idx(f, x, y), cl = log2[g], n = 1 << cl;
      if (!intra[g]) {
        const CuSignal r = decide_signalling_values(v, f.cw, f.chp, x & ~(n - 1), y & ~(n - 1), cl, nref > 1 ? nref : 1, reinterpret_cast<const ColMv *>(col));
        flags[g] = (uint8_t)r.flags; midx[g] = (uint8_t)r.midx; mvp[g] = (uint8_t)r.mvp; mvd[2 * g] = (int16_t)r.mvdx; mvd[2 * g + 1] = (int16_t)r.mvdy;
      }
      if (!((x | y) & 15)) {
        int16_t *c = col_out + 4 * ((y >> 4) * (cw >> 4) + (x >> 4));
        c[0] = intra[g] ? 0 : mv[2 * g]; c[1] = intra[g] ? 0 : mv[2 * g + 1]; c[2] = intra[g] ? 0 : (int16_t)(ref[g] + 1); c[3] = 0;
      }
    }
}

}
