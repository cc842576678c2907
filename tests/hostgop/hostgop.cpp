// tests/hostgop/hostgop.cpp -- host build of what "lp-gop"  adds to the product's serial code, for tests/test_lp_gop_host.py: slice
// segment headers that carry the picture's reference picture set (hevc_headers.h PicRefs) and the merge / AMVP candidate lists with a table of POC
// distances (hevc_core.h TabDist).  Test infrastructure.
#include <cstring>
#include <vector>
#include "../../kvazzup_amd/csrc/hevc_core.h"
#include "../../kvazzup_amd/csrc/hevc_headers.h"

using namespace kvzx;

extern "C" {

// The access unit of a picture `poc` pictures after its IDR picture (poc 0: the IDR picture), parameter sets first, with one 2-byte substream per CTU row
// (wpp) or tile, coded at init QP + qp_delta.  nrefs > 0: the picture's references, dist[k] pictures back (the option on); 0: the option off.
// Annex B bytes -> out; returns their count, -1 when cap is too small or the substreams do not fit the tiling.
int hg_access_unit(int w, int h, int lp_refs, int tmvp, int sao, int wpp, int tile_rows, int tile_cols, int slices, int poc, int qp_delta, int nrefs,
                   const int8_t *dist, uint8_t *out, int cap)
{
  StreamParams s{};
  s.cw = (w + 63) & ~63; s.ch = (h + 63) & ~63; s.width = w; s.height = h; s.qp = 32; s.wpp = wpp; s.deblock = 1; s.fps_num = 30; s.fps_den = 1;
  s.sao = sao; s.lp_refs = lp_refs; s.tmvp = tmvp; s.tile_rows = tile_rows; s.tile_cols = tile_cols; s.slices = slices;
  const int hc = s.ch / 64;
  int nsub = 0;
  for (int tr = 0; tr < tile_rows; tr++) nsub += (wpp ? tile_row_first(hc, tile_rows, tr + 1) - tile_row_first(hc, tile_rows, tr) : 1) * tile_cols;
  std::vector<std::vector<uint8_t>> rows((size_t)nsub, std::vector<uint8_t>{0xa5, 0x80});
  std::vector<uint8_t> au;
  PicRefs pr; pr.n = nrefs; for (int k = 0; k < 4; k++) pr.dist[k] = k < nrefs ? dist[k] : 0;
  if (!assemble_access_unit(au, s, poc == 0, poc, true, rows, nsub, qp_delta, nrefs > 0 ? &pr : nullptr)) return -1;
  if ((int)au.size() > cap) return -1;
  memcpy(out, au.data(), au.size());
  return (int)au.size();
}

// As tests/hosttmvp's ht_cands, with the references' POC distances in `tab` (byte k: reference k; EncFrame::ref_dist): for the inter CU at (x0, y0) of size
// 1 << cl, merge[5][3] = the merge candidates (mvx, mvy, ref), amvp[2][2] = the AMVP candidates for the CU's own reference, sig[5] = {flags, merge_idx,
// mvp_idx, mvdx, mvdy}.  col: the previous picture's record (ColMv per 16x16 block, dist = the true POC distance), NULL: none.
void hg_cands(int cw, int ch, int tile_rows, int tile_cols, int nref, const uint8_t *log2, const uint8_t *intra, const int16_t *mv, const uint8_t *ref,
              const uint8_t *cbf, const int16_t *col, uint32_t tab, int x0, int y0, int cl, int32_t *merge, int32_t *amvp, int32_t *sig)
{
  EncFrame f;
  memset(&f, 0, sizeof(f));
  f.cw = cw; f.ch = ch; f.b8w = cw / 8; f.b8h = ch / 8; f.tile_rows = tile_rows; f.tile_cols = tile_cols; f.chp = pack_height(ch, tile_rows, tile_cols);
  f.cu_log2 = const_cast<uint8_t *>(log2); f.cu_intra = const_cast<uint8_t *>(intra); f.cu_mv = const_cast<int16_t *>(mv); f.cu_cbf = const_cast<uint8_t *>(cbf);
  f.cu_ref = const_cast<uint8_t *>(ref); f.nref = nref; f.ref_dist = tab;
  const ColMv *cr = reinterpret_cast<const ColMv *>(col);
  const TabDist dist{tab};
  FrameMvView v{f};
  const int n = 1 << cl, own = ref[b8idx(f, x0, y0)];
  const FiveNb q = five_neighbours(v, f.cw, f.chp, x0, y0, n);
  const ColMv cb = col_block(cr, cw, ch, x0, y0, n);
  const NbMv t0 = temporal_cand(cb, 0, dist), tr = temporal_cand(cb, own, dist);
  int cmx[5], cmy[5], cref[5], px[2], py[2];
  merge_cand_list(q, cmx, cmy, cref, nref, cr ? &t0 : nullptr);
  amvp_cand_list(q, px, py, own, cr ? &tr : nullptr, dist);
  for (int k = 0; k < 5; k++) { merge[3 * k] = cmx[k]; merge[3 * k + 1] = cmy[k]; merge[3 * k + 2] = cref[k]; }
  for (int k = 0; k < 2; k++) { amvp[2 * k] = px[k]; amvp[2 * k + 1] = py[k]; }
  const CuSignal r = decide_signalling_values(v, f.cw, f.chp, x0, y0, cl, nref, cr, dist);
  sig[0] = r.flags; sig[1] = r.midx; sig[2] = r.mvp; sig[3] = r.mvdx; sig[4] = r.mvdy;
}

}
