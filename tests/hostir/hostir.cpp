// tests/hostir/hostir.cpp -- host build of what "intra-refresh"  adds to the product's serial code, for tests/test_intra_refresh_host.py: the
// statement functions of hevc_core.h (ir_step .. ir_last_column) and the access unit with the recovery point SEI (hevc_headers.h).  Test infrastructure.
#include <cstring>
#include <vector>
#include "../../kvazzup_amd/csrc/hevc_core.h"
#include "../../kvazzup_amd/csrc/hevc_headers.h"

using namespace kvzx;

extern "C" {

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

// the RBSP of the recovery point SEI NAL unit; returns its length
int hi_recovery_sei(int cnt, uint8_t *out, int cap)
{
  BitWriter w;
  write_recovery_point_sei(w, cnt);
  if ((int)w.data().size() > cap) return -1;
  memcpy(out, w.data().data(), w.data().size());
  return (int)w.data().size();
}

// The access unit of a picture `poc` pictures after its IDR picture (poc 0: the IDR picture), parameter sets first when write_ps; recovery >= 0: the recovery point
// SEI with that recovery_poc_cnt in front of the slices, -1: none.  Substreams as in tests/hostwp: `payload` (wpp 0, one tile) or a 2-byte placeholder per
// CTU row (wpp) or tile.  Annex B bytes -> out; returns their count, -1 when cap is too small or the substreams do not fit the tiling.
int hi_access_unit(int w, int h, int lp_refs, int sao, int wpp, int tile_rows, int tile_cols, int slices, int weightp, int poc, int qp_delta, int recovery,
                   const uint8_t *payload, int payload_len, int write_ps, uint8_t *out, int cap)
{
  StreamParams s{};
  s.cw = (w + 63) & ~63; s.ch = (h + 63) & ~63;
  s.width = w; s.height = h; s.qp = 32; s.wpp = wpp; s.deblock = 1; s.fps_num = 30; s.fps_den = 1;
  s.sao = sao; s.lp_refs = lp_refs; s.tile_rows = tile_rows; s.tile_cols = tile_cols; s.slices = slices; s.weightp = weightp;
  const int hc = s.ch / 64;
  int nsub = 0;
  for (int tr = 0; tr < tile_rows; tr++) nsub += (wpp ? tile_row_first(hc, tile_rows, tr + 1) - tile_row_first(hc, tile_rows, tr) : 1) * tile_cols;
  std::vector<std::vector<uint8_t>> rows((size_t)nsub, std::vector<uint8_t>{0xa5, 0x80});
  if (payload_len > 0) { if (nsub != 1) return -1; rows[0].assign(payload, payload + payload_len); }
  std::vector<uint8_t> au;
  if (!assemble_access_unit(au, s, poc == 0, poc, write_ps != 0, rows, nsub, qp_delta, nullptr, nullptr, recovery)) return -1;
  if ((int)au.size() > cap) return -1;
  memcpy(out, au.data(), au.size());
  return (int)au.size();
}

}
