// tests/hostcheck/anchor.cpp -- host build of fb-anchor's statement functions (hevc_core.h fb_anchor_*; "uvgx loss feedback v2") and of the
// header writers with kept pictures (hevc_headers.h) for tests/test_fb_anchor_host.py, which holds them to the statement of record tests/fb_anchor_model.py.
// Built by that test on its own (g++, into pytest's temporary directory), as feedback.cpp is.  The step's loop is what k_fb_step_ref does with one workgroup.
// Test infrastructure.
#include <cstddef>
#include <cstring>
#include <vector>
#include "../../kvazzup_amd/csrc/hevc_core.h"
#include "../../kvazzup_amd/csrc/hevc_headers.h"

using namespace kvzx;

extern "C" {

int ha_max_dpb(int cw, int ch) { return fb_anchor_max_dpb(cw, ch); }
int ha_level(int cw, int ch) { return level_idc_for(cw, ch); }
int ha_pick(int c, int n0, int t, int K, int H) { return fb_anchor_pick(c, n0, t, K, H); }
int ha_kept(int t, int K) { return fb_anchor_kept(t, K); }
int ha_used(int back, int da) { return fb_anchor_used(back, da) ? 1 : 0; }

// a record's info bytes: fb_info() and the reference bit of the inter cells (k_fb_record_ref)
void ha_info(const uint8_t *intra, const uint8_t *log2, const uint8_t *ref, int n, uint8_t *info)
{
  for (int i = 0; i < n; i++) info[i] = (uint8_t)(fb_info(intra[i], log2[i]) | (!intra[i] && ref[i] ? KVZ_FB_REF1 : 0));
}

// map: D of the picture before -> D of the v2 heal picture whose record (mv [cell][2], info [cell]) is given (k_fb_step_ref)
void ha_step(uint8_t *map, int cw, int ch, const int16_t *mv, const uint8_t *info, int dilate, int anchor_bad)
{
  const int gw = cw / 8, gh = ch / 8, n = gw * gh;
  std::vector<uint8_t> tmp((size_t)n);
  for (int i = 0; i < n; i++) {
    if (!(info[i] & (KVZ_FB_CLEAN | 1)) && (info[i] & KVZ_FB_REF1)) { tmp[i] = fb_anchor_cell(info[i], anchor_bad) ? 1 : 0; continue; }
    tmp[i] = (!(info[i] & (KVZ_FB_CLEAN | 1)) && fb_inter_cell(map, cw, ch, i % gw, i / gw, mv[2 * i], mv[2 * i + 1])) ? 1 : 0;
  }
  for (bool changed = true; changed;) {
    changed = false;
    for (int i = 0; i < n; i++)
      if ((info[i] & 1) && !(info[i] & KVZ_FB_CLEAN) && !tmp[i] && fb_intra_cell(tmp.data(), cw, ch, i % gw, i / gw, (info[i] >> 1) & 7)) { tmp[i] = 1; changed = true; }
  }
  for (int i = 0; i < n; i++) map[i] = (dilate ? fb_dilated(tmp.data(), gw, gh, i % gw, i / gw) : tmp[i] != 0) ? 1 : 0;
}

// the access unit of picture `poc` (0: the IDR picture) of a w x h stream with fb-anchor K, parameter sets in front when write_ps, one two-byte placeholder per
// substream: the references as Encoder::hand_off states them -- K 0: no PicRefs; else the kept set of fb_anchor_kept() entries, the previous picture active and,
// da > 0, the anchor da pictures back.  lp_refs: as hc_access_unit's (K 0: the writer of before).  Returns the length, or -1
int ha_access_unit(int w, int h, int K, int lp_refs, int poc, int da, int write_ps, uint8_t *out, int cap)
{
  StreamParams s{};
  s.cw = (w + 63) & ~63; s.ch = (h + 63) & ~63;
  s.width = w; s.height = h; s.qp = 32; s.wpp = 1; s.deblock = 1; s.fps_num = 30; s.fps_den = 1; s.lp_refs = lp_refs; s.fb_anchor = K;
  const int nsub = s.ch / 64;
  std::vector<std::vector<uint8_t>> rows((size_t)nsub, std::vector<uint8_t>{0xa5, 0x80});
  std::vector<uint8_t> au;
  PicRefs pr{}; pr.n = da > 0 ? 2 : 1; pr.dist[0] = 1; pr.dist[1] = (int8_t)da; pr.kept = fb_anchor_kept(poc, K);
  if (!assemble_access_unit(au, s, poc == 0, poc, write_ps != 0, rows, nsub, 0, K && poc > 0 ? &pr : nullptr, nullptr, -1)) return -1;
  if ((int)au.size() > cap) return -1;
  memcpy(out, au.data(), au.size());
  return (int)au.size();
}

}
