// tests/hostcheck/motion.cpp -- host build of the product's motion signalling (hevc_core.h) for the CPU tests of lp-refs, tmvp and lp-gop: the merge / AMVP
// candidate lists with n references, a collocated record and a table of POC distances, the signalling of a whole picture, ref_idx_l0's bins.
// Test infrastructure.
#include <cstring>
#include "../../kvazzup_amd/csrc/hevc_core.h"

using namespace kvzx;

// The motion field of a P picture: per 8x8 block log2 (3..5), intra, mv (x, y), ref, cbf; a tile grid; nref active references.
static EncFrame frame_of(int cw, int ch, int tile_rows, int tile_cols, int nref, const uint8_t *log2, const uint8_t *intra, const int16_t *mv, const uint8_t *ref,
                         const uint8_t *cbf)
{
  EncFrame f;
  memset(&f, 0, sizeof(f));
  f.cw = cw; f.ch = ch; f.b8w = cw / 8; f.b8h = ch / 8; f.tile_rows = tile_rows; f.tile_cols = tile_cols; f.chp = pack_height(ch, tile_rows, tile_cols);
  f.cu_log2 = const_cast<uint8_t *>(log2); f.cu_intra = const_cast<uint8_t *>(intra); f.cu_mv = const_cast<int16_t *>(mv); f.cu_cbf = const_cast<uint8_t *>(cbf);
  f.cu_ref = const_cast<uint8_t *>(ref); f.nref = nref;
  return f;
}

// the two lists of the inter CU at (x0, y0) under the distances `dist`: temporal candidates only with a record
template <typename D>
static void cand_lists(const EncFrame &f, const ColMv *cr, D dist, int x0, int y0, int cl, int32_t *merge, int32_t *amvp)
{
  FrameMvView v{f};
  const int n = 1 << cl, own = f.cu_ref[b8idx(f, x0, y0)];
  const FiveNb q = five_neighbours(v, f.cw, f.chp, x0, y0, n);
  const ColMv cb = col_block(cr, f.cw, f.ch, x0, y0, n);
  const NbMv t0 = temporal_cand(cb, 0, dist), tr = temporal_cand(cb, own, dist);
  int cmx[5], cmy[5], cref[5], px[2], py[2];
  merge_cand_list(q, cmx, cmy, cref, f.nref, cr ? &t0 : nullptr);
  amvp_cand_list(q, px, py, own, cr ? &tr : nullptr, dist);
  for (int k = 0; k < 5; k++) { merge[3 * k] = cmx[k]; merge[3 * k + 1] = cmy[k]; merge[3 * k + 2] = cref[k]; }
  for (int k = 0; k < 2; k++) { amvp[2 * k] = px[k]; amvp[2 * k + 1] = py[k]; }
}

extern "C" {

// For the inter CU at (x0, y0) of size 1 << cl of the motion field (frame_of): merge[5][3] = the merge candidates (mvx, mvy, ref) with nref active references,
// amvp[2][2] = the AMVP candidates for the CU's own reference, sig[5] = the signalling the encoder derives {flags, merge_idx, mvp_idx, mvdx, mvdy}.
// col: the previous picture's collocated record (ColMv per 16x16 block), NULL: none.  tab: the references' POC distances (byte k: reference k;
// EncFrame::ref_dist), 0: none, reference k is k + 1 pictures back.  Which product code each caller pins:
//   no col, no tab (test_lp_refs_host, test_tmvp_host's "no record"): SeqDist by default and decide_signalling_values(f, x0, y0, cl), the EncFrame overload;
//   col, no tab (test_tmvp_host, test_lp_gop_host's "sequential table"): SeqDist, temporal_cand(cb, ref) and decide_signalling_values(v, .., nref, col);
//   tab (test_lp_gop_host): TabDist{tab} throughout and f.ref_dist = tab.
void hc_cands(int cw, int ch, int tile_rows, int tile_cols, int nref, const uint8_t *log2, const uint8_t *intra, const int16_t *mv, const uint8_t *ref,
              const uint8_t *cbf, const int16_t *col, uint32_t tab, int x0, int y0, int cl, int32_t *merge, int32_t *amvp, int32_t *sig)
{
  EncFrame f = frame_of(cw, ch, tile_rows, tile_cols, nref, log2, intra, mv, ref, cbf);
  const ColMv *cr = reinterpret_cast<const ColMv *>(col);
  FrameMvView v{f};
  CuSignal r;
  if (tab) {
    f.ref_dist = tab;
    const TabDist dist{tab};
    cand_lists(f, cr, dist, x0, y0, cl, merge, amvp);
    r = decide_signalling_values(v, f.cw, f.chp, x0, y0, cl, nref, cr, dist);
  } else {
    cand_lists(f, cr, SeqDist(), x0, y0, cl, merge, amvp);
    r = cr ? decide_signalling_values(v, f.cw, f.chp, x0, y0, cl, nref, cr) : decide_signalling_values(f, x0, y0, cl);
  }
  sig[0] = r.flags; sig[1] = r.midx; sig[2] = r.mvp; sig[3] = r.mvdx; sig[4] = r.mvdy;
}

// decide_signalling_values for every 8x8 unit of a picture, as k_inter_signal<TMVP> runs it (col NULL: k_inter_signal<false>), and the collocated record
// the picture files (col_out: ColMv per 16x16 block): what the GPU test restates the kernel's exported arrays with
void ht_picture(int cw, int ch, int tile_rows, int tile_cols, int nref, const uint8_t *log2, const uint8_t *intra, const int16_t *mv, const uint8_t *ref,
                const uint8_t *cbf, const int16_t *col, uint8_t *flags, uint8_t *midx, uint8_t *mvp, int16_t *mvd, int16_t *col_out)
{
  const EncFrame f = frame_of(cw, ch, tile_rows, tile_cols, nref, log2, intra, mv, ref, cbf);
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

// ref_idx_l0's bins (hevc_core.h enc_ref_idx) as tokens: returns their count
int hr_ref_idx_tokens(int r, int nref, uint16_t *out, int cap)
{
  TokOut t; t.tabs = nullptr; t.p = out; t.n = 0; t.cap = cap;
  enc_ref_idx(t, r, nref);
  return t.n;
}

}
