// tests/hostrefs/hostrefs.cpp -- host build of what "lp-refs" adds to the product's serial code, for tests/test_lp_refs_host.py: the parameter sets and
// slice header with n references (hevc_headers.h) and the reference-aware merge / AMVP candidate lists (hevc_core.h).  Test infrastructure.
#include <cstring>
#include <vector>
#include "../../kvazzup_amd/csrc/hevc_core.h"
#include "../../kvazzup_amd/csrc/hevc_headers.h"

using namespace kvzx;

extern "C" {

// which: 0 VPS, 1 SPS, 2 PPS, 3 the slice segment header of a picture `poc` pictures after its IDR picture (poc 0: the IDR picture itself).  RBSP
// bytes (no NAL unit header, no emulation prevention) -> out; returns their count, or -1 when cap is too small.
int hr_header(int which, int lp_refs, int poc, int sao, uint8_t *out, int cap)
{
  StreamParams s{};
  s.cw = 256; s.ch = 128; s.width = 256; s.height = 128; s.qp = 32; s.wpp = 1; s.deblock = 1; s.fps_num = 30; s.fps_den = 1; s.sao = sao; s.lp_refs = lp_refs;
  BitWriter w;
  if (which == 0) write_vps(w, s);
  else if (which == 1) write_sps(w, s);
  else if (which == 2) write_pps(w, s);
  else { std::vector<uint32_t> entries(1, 7u); write_slice_header(w, s, poc == 0, poc, entries); }
  const std::vector<uint8_t> &d = w.data();
  if ((int)d.size() > cap) return -1;
  memcpy(out, d.data(), d.size());
  return (int)d.size();
}

// The motion field of a P picture: per 8x8 block log2 (3..5), intra, mv (x, y), ref; a tile grid.  For the inter CU at (x0, y0) of size 1 << log2:
// merge[5][3] = the merge candidates (mvx, mvy, ref) with nref active references, amvp[2][2] = the AMVP candidates for the CU's own reference;
// sig[5] = the signalling the encoder derives {flags, merge_idx, mvp_idx, mvdx, mvdy}.
void hr_cands(int cw, int ch, int tile_rows, int tile_cols, int nref, const uint8_t *log2, const uint8_t *intra, const int16_t *mv, const uint8_t *ref,
              const uint8_t *cbf, int x0, int y0, int cl, int32_t *merge, int32_t *amvp, int32_t *sig)
{
  EncFrame f;
  memset(&f, 0, sizeof(f));
  f.cw = cw; f.ch = ch; f.b8w = cw / 8; f.b8h = ch / 8; f.tile_rows = tile_rows; f.tile_cols = tile_cols; f.chp = pack_height(ch, tile_rows, tile_cols);
  f.cu_log2 = const_cast<uint8_t *>(log2); f.cu_intra = const_cast<uint8_t *>(intra); f.cu_mv = const_cast<int16_t *>(mv); f.cu_cbf = const_cast<uint8_t *>(cbf);
  f.cu_ref = const_cast<uint8_t *>(ref); f.nref = nref;
  FrameMvView v{f};
  const int n = 1 << cl;
  const FiveNb q = five_neighbours(v, f.cw, f.chp, x0, y0, n);
  int cmx[5], cmy[5], cref[5], px[2], py[2];
  merge_cand_list(q, cmx, cmy, cref, nref);
  amvp_cand_list(q, px, py, ref[b8idx(f, x0, y0)]);
  for (int k = 0; k < 5; k++) { merge[3 * k] = cmx[k]; merge[3 * k + 1] = cmy[k]; merge[3 * k + 2] = cref[k]; }
  for (int k = 0; k < 2; k++) { amvp[2 * k] = px[k]; amvp[2 * k + 1] = py[k]; }
  const CuSignal r = decide_signalling_values(f, x0, y0, cl);
  sig[0] = r.flags; sig[1] = r.midx; sig[2] = r.mvp; sig[3] = r.mvdx; sig[4] = r.mvdy;
}

// ref_idx_l0's bins (hevc_core.h enc_ref_idx) as tokens: returns their count
int hr_ref_idx_tokens(int r, int nref, uint16_t *out, int cap)
{
  TokOut t; t.tabs = nullptr; t.p = out; t.n = 0; t.cap = cap;
  enc_ref_idx(t, r, nref);
  return t.n;
}

}
