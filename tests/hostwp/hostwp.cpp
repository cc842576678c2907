// tests/hostwp/hostwp.cpp -- host build of what "weightp"  adds to the product's serial code, for tests/test_weightp_host.py: the statement
// functions of hevc_core.h (wp_moments, wp_candidate, wp_accept, wp_sample, wp_pred14) and the headers that carry the weights (hevc_headers.h PicWeights).
// Test infrastructure.
#include <cstring>
#include <vector>
#include "../../kvazzup_amd/csrc/hevc_core.h"
#include "../../kvazzup_amd/csrc/hevc_headers.h"

using namespace kvzx;

extern "C" {

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

// The access unit of a picture `poc` pictures after its IDR picture (poc 0: the IDR picture), parameter sets first when write_ps, coded at init QP + qp_delta.
// weightp: StreamParams::weightp; wts (weightp, a P picture): [reference][flag, w, o], NULL: no PicWeights handed over.  nrefs > 0: lp-gop's table as in
// tests/hostgop.  payload: the one substream's bytes (wpp 0, one tile) when payload_len > 0, else a 2-byte substream per CTU row (wpp) or tile.
// Annex B bytes -> out; returns their count, -1 when cap is too small or the substreams do not fit the tiling.
int hw_access_unit(int w, int h, int lp_refs, int tmvp, int sao, int wpp, int tile_rows, int tile_cols, int slices, int poc, int qp_delta, int nrefs,
                   const int8_t *dist, int weightp, const int32_t *wts, const uint8_t *payload, int payload_len, int write_ps, uint8_t *out, int cap)
{
  StreamParams s{};
  s.cw = (w + 63) & ~63; s.ch = (h + 63) & ~63;
  s.width = w; s.height = h; s.qp = 32; s.wpp = wpp; s.deblock = 1; s.fps_num = 30; s.fps_den = 1;
  s.sao = sao; s.lp_refs = lp_refs; s.tmvp = tmvp; s.tile_rows = tile_rows; s.tile_cols = tile_cols; s.slices = slices; s.weightp = weightp;
  const int hc = s.ch / 64;
  int nsub = 0;
  for (int tr = 0; tr < tile_rows; tr++) nsub += (wpp ? tile_row_first(hc, tile_rows, tr + 1) - tile_row_first(hc, tile_rows, tr) : 1) * tile_cols;
  std::vector<std::vector<uint8_t>> rows((size_t)nsub, std::vector<uint8_t>{0xa5, 0x80});
  if (payload_len > 0) { if (nsub != 1) return -1; rows[0].assign(payload, payload + payload_len); }
  std::vector<uint8_t> au;
  PicRefs pr; pr.n = nrefs; for (int k = 0; k < 4; k++) pr.dist[k] = k < nrefs ? dist[k] : 0;
  PicWeights pw{};
  if (wts) for (int k = 0; k < 4; k++) { pw.flag[k] = (int8_t)wts[3 * k]; pw.w[k] = (int16_t)wts[3 * k + 1]; pw.o[k] = (int16_t)wts[3 * k + 2]; }
  if (!assemble_access_unit(au, s, poc == 0, poc, write_ps != 0, rows, nsub, qp_delta, nrefs > 0 ? &pr : nullptr, wts ? &pw : nullptr)) return -1;
  if ((int)au.size() > cap) return -1;
  memcpy(out, au.data(), au.size());
  return (int)au.size();
}

}
