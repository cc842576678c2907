// tests/hostcheck/syntax.cpp -- host build of the product's header writers (hevc_headers.h) for the CPU tests of the encoder options: bare parameter sets and
// slice segment headers, whole access units with every per-picture value assemble_access_unit takes, the recovery point SEI.  Test infrastructure.
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

// the RBSP of the recovery point SEI NAL unit; returns its length
int hi_recovery_sei(int cnt, uint8_t *out, int cap)
{
  BitWriter w;
  write_recovery_point_sei(w, cnt);
  if ((int)w.data().size() > cap) return -1;
  memcpy(out, w.data().data(), w.data().size());
  return (int)w.data().size();
}

// One access unit: the StreamParams fields the tests set, then the picture's values (tests/hc.py mirrors the struct; a new encoder option is one more field).
struct HcAccessUnit {
  int32_t w, h, lp_refs, tmvp, sao, wpp, tile_rows, tile_cols, slices, weightp;
  int32_t poc, qp_delta, write_ps;
  int32_t nrefs; int8_t dist[4];     // lp-gop: the picture's references, dist[k] pictures back; nrefs 0: no PicRefs handed over
  const int32_t *wts;                // weightp, a P picture: [reference][flag, w, o]; NULL: no PicWeights handed over
  int32_t recovery;                  // intra-refresh: recovery_poc_cnt of the recovery point SEI in front of the slices, -1: none
  const uint8_t *payload; int32_t payload_len;
};

// The access unit of a picture `poc` pictures after its IDR picture (poc 0: the IDR picture), parameter sets first when write_ps, coded at init QP + qp_delta.
// payload: the one substream's bytes (wpp 0, one tile) when payload_len > 0, else a 2-byte substream per CTU row (wpp) or tile.
// Annex B bytes -> out; returns their count, -1 when cap is too small or the substreams do not fit the tiling.
int hc_access_unit(const HcAccessUnit *a, uint8_t *out, int cap)
{
  StreamParams s{};
  s.cw = (a->w + 63) & ~63; s.ch = (a->h + 63) & ~63;
  s.width = a->w; s.height = a->h; s.qp = 32; s.wpp = a->wpp; s.deblock = 1; s.fps_num = 30; s.fps_den = 1;
  s.sao = a->sao; s.lp_refs = a->lp_refs; s.tmvp = a->tmvp; s.tile_rows = a->tile_rows; s.tile_cols = a->tile_cols; s.slices = a->slices; s.weightp = a->weightp;
  const int hc = s.ch / 64;
  int nsub = 0;
  for (int tr = 0; tr < a->tile_rows; tr++) nsub += (a->wpp ? tile_row_first(hc, a->tile_rows, tr + 1) - tile_row_first(hc, a->tile_rows, tr) : 1) * a->tile_cols;
  std::vector<std::vector<uint8_t>> rows((size_t)nsub, std::vector<uint8_t>{0xa5, 0x80});
  if (a->payload_len > 0) { if (nsub != 1) return -1; rows[0].assign(a->payload, a->payload + a->payload_len); }
  std::vector<uint8_t> au;
  PicRefs pr; pr.n = a->nrefs; for (int k = 0; k < 4; k++) pr.dist[k] = k < a->nrefs ? a->dist[k] : 0;
  PicWeights pw{};
  if (a->wts) for (int k = 0; k < 4; k++) { pw.flag[k] = (int8_t)a->wts[3 * k]; pw.w[k] = (int16_t)a->wts[3 * k + 1]; pw.o[k] = (int16_t)a->wts[3 * k + 2]; }
  if (!assemble_access_unit(au, s, a->poc == 0, a->poc, a->write_ps != 0, rows, nsub, a->qp_delta, a->nrefs > 0 ? &pr : nullptr, a->wts ? &pw : nullptr, a->recovery)) return -1;
  if ((int)au.size() > cap) return -1;
  memcpy(out, au.data(), au.size());
  return (int)au.size();
}

}
