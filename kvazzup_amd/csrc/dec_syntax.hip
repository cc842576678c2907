// kvazzup_amd/csrc/dec_syntax.hip -- see dec_syntax.h.  The decoder's header syntax: profile / tier / level, short-term reference picture sets, scaling lists,
// VPS / SPS / PPS, the slice segment header's self-contained parts and its tail.  No Decoder member is touched here and no HIP header is needed: host code only.
#include <cstring>
#include "dec_syntax.h"

namespace kvzx {

static bool skip_ptl(BitReader &r, int max_sub_layers_minus1)
{
  r.get(8); r.get(32); r.get(4); r.get(32); r.get(11); r.get(1); r.get(8);
  int pp[8], lp[8];
  for (int i = 0; i < max_sub_layers_minus1; i++) { pp[i] = r.get(1); lp[i] = r.get(1); }
  if (max_sub_layers_minus1 > 0) for (int i = max_sub_layers_minus1; i < 8; i++) r.get(2);
  for (int i = 0; i < max_sub_layers_minus1; i++) { if (pp[i]) { r.get(32); r.get(32); r.get(24); } if (lp[i]) r.get(8); }
  return !r.err;
}

// st_ref_pic_set(idx) (7.3.7, 7.4.8): explicit or predicted from an earlier set
bool parse_st_rps(BitReader &r, int idx, int num_in_sps, const StRps *all, StRps &out)
{
  out = StRps();
  int inter = 0;
  if (idx != 0) inter = r.get(1);
  if (inter) {
    int delta_idx = 1;
    if (idx == num_in_sps) delta_idx = (int)r.ue() + 1;
    if (delta_idx > idx) return false;
    const StRps &ref = all[idx - delta_idx];
    const int sign = r.get(1), absd = (int)r.ue() + 1, drps = (1 - 2 * sign) * absd, nd = ref.n_neg + ref.n_pos;
    int used[17], use_delta[17];
    for (int j = 0; j <= nd; j++) { used[j] = r.get(1); use_delta[j] = 1; if (!used[j]) use_delta[j] = r.get(1); }
    int s0[16], u0[16], s1[16], u1[16], n0 = 0, n1 = 0;
    const int *rs0 = ref.dpoc, *rs1 = ref.dpoc + ref.n_neg; const uint8_t *unused = nullptr; (void)unused;
    for (int j = ref.n_pos - 1; j >= 0; j--) { const int d = rs1[j] + drps; if (d < 0 && use_delta[ref.n_neg + j] && n0 < 16) { s0[n0] = d; u0[n0++] = used[ref.n_neg + j]; } }
    if (drps < 0 && use_delta[nd] && n0 < 16) { s0[n0] = drps; u0[n0++] = used[nd]; }
    for (int j = 0; j < ref.n_neg; j++) { const int d = rs0[j] + drps; if (d < 0 && use_delta[j] && n0 < 16) { s0[n0] = d; u0[n0++] = used[j]; } }
    for (int j = ref.n_neg - 1; j >= 0; j--) { const int d = rs0[j] + drps; if (d > 0 && use_delta[j] && n1 < 16) { s1[n1] = d; u1[n1++] = used[j]; } }
    if (drps > 0 && use_delta[nd] && n1 < 16) { s1[n1] = drps; u1[n1++] = used[nd]; }
    for (int j = 0; j < ref.n_pos; j++) { const int d = rs1[j] + drps; if (d > 0 && use_delta[ref.n_neg + j] && n1 < 16) { s1[n1] = d; u1[n1++] = used[ref.n_neg + j]; } }
    if (n0 + n1 > 16) return false;
    out.n_neg = n0; out.n_pos = n1;
    for (int j = 0; j < n0; j++) { out.dpoc[j] = s0[j]; out.used[j] = (uint8_t)u0[j]; }
    for (int j = 0; j < n1; j++) { out.dpoc[n0 + j] = s1[j]; out.used[n0 + j] = (uint8_t)u1[j]; }
  } else {
    const int nneg = (int)r.ue(), npos = (int)r.ue();
    if (nneg > 16 || npos > 16 || nneg + npos > 16 || r.err) return false;
    out.n_neg = nneg; out.n_pos = npos;
    int prev = 0;
    for (int j = 0; j < nneg; j++) { prev -= (int)r.ue() + 1; out.dpoc[j] = prev; out.used[j] = (uint8_t)r.get(1); }
    prev = 0;
    for (int j = 0; j < npos; j++) { prev += (int)r.ue() + 1; out.dpoc[nneg + j] = prev; out.used[nneg + j] = (uint8_t)r.get(1); }
  }
  return !r.err;
}

// ------------------------------------------------------------------------------------------ scaling lists (7.3.4, 7.4.5)
// scaling_list_data(): every list either the default one, a copy of an earlier list of its size, or 16 / 64 entries in diagonal scan order
static bool parse_scaling_list_data(BitReader &r, ScalingLists &sl)
{
  const ScanTabs &st = scan_tabs();
  for (int s = 0; s < 4; s++)
    for (int m = 0; m < (s == 3 ? 2 : 6); m++) {
      if (!r.get(1)) {
        const uint32_t delta = r.ue();
        if (delta > (uint32_t)m) return false;
        if (delta == 0) scaling_default_one(sl, s, m);
        else { memcpy(sl.m[s][m], sl.m[s][m - (int)delta], 64); if (s >= 2) sl.dc[s - 2][m] = sl.dc[s - 2][m - (int)delta]; }
      } else {
        int next = 8;
        if (s >= 2) { const int dc = r.se(); if (dc < -7 || dc > 247) return false; next = dc + 8; sl.dc[s - 2][m] = (uint8_t)next; }
        const int l2 = s == 0 ? 2 : 3, n = 1 << l2;
        for (int i = 0; i < n * n; i++) {
          const int d = r.se();
          if (d < -128 || d > 127) return false;
          next = (next + d + 256) & 255;
          if (!next) return false;
          sl.m[s][m][st.y[0][l2][i] * n + st.x[0][l2][i]] = (uint8_t)next;      // diagonal scan position i -> (x, y)
        }
      }
      if (r.err) return false;
    }
  return true;
}
static std::shared_ptr<const std::vector<uint8_t>> build_scaling(const ScalingLists &sl)
{
  auto out = std::make_shared<std::vector<uint8_t>>((size_t)KVZ_SCALING_BYTES);
  scaling_factors(sl, out->data());
  return out;
}

// ------------------------------------------------------------------------------------------ parameter sets (7.3.2)
int parse_vps(BitReader &r, VpsTiming &t)                      // VPS: only the timing information is used
{
  r.get(4); r.get(2); r.get(6); int msl = r.get(3); r.get(1); r.get(16);
  if (!skip_ptl(r, msl)) return DEC_ERR_INVALID;
  int oi = r.get(1);
  for (int k = oi ? 0 : msl; k <= msl; k++) { r.ue(); r.ue(); r.ue(); }
  int max_layer_id = r.get(6); int nls = r.ue() + 1;
  if (nls > 1024) return DEC_ERR_INVALID;
  for (int a = 1; a < nls; a++) for (int b = 0; b <= max_layer_id; b++) r.get(1);
  if (r.get(1)) { t.present = true; t.fps_den = r.get(32); t.fps_num = r.get(32); }
  return r.err ? DEC_ERR_INVALID : 0;
}

int parse_sps(BitReader &r, DecSps &s, int &id)                // SPS (7.3.2.2)
{
  r.get(4); int msl = r.get(3); r.get(1);
  if (!skip_ptl(r, msl)) return DEC_ERR_INVALID;
  id = r.ue(); if (id > 15) return DEC_ERR_INVALID;
  if (r.ue() != 1) return DEC_ERR_UNSUPPORTED;   // 4:2:0 only
  s.width = r.ue(); s.height = r.ue();
  if (r.get(1)) {
    const uint32_t cl = r.ue(), cr = r.ue(), ct = r.ue(), cb = r.ue();
    if (cl > 8192 || cr > 8192 || ct > 8192 || cb > 8192) return DEC_ERR_INVALID;
    s.crop_l = 2 * (int)cl; s.crop_r = 2 * (int)cr; s.crop_t = 2 * (int)ct; s.crop_b = 2 * (int)cb;
  }
  if (r.ue() != 0 || r.ue() != 0) return DEC_ERR_UNSUPPORTED;   // 8 bit only
  s.log2_max_poc_lsb = r.ue() + 4;
  if (s.log2_max_poc_lsb > 16) return DEC_ERR_INVALID;
  int oi = r.get(1);
  for (int k = oi ? 0 : msl; k <= msl; k++) { r.ue(); s.num_reorder = r.ue(); r.ue(); }      // (max_dec_pic_buffering, max_num_reorder_pics, max_latency_increase: the highest sub-layer's stay)
  if (s.num_reorder < 0 || s.num_reorder > 15) return DEC_ERR_INVALID;
  int log2_min_cb = r.ue() + 3, diff_cb = r.ue(), log2_min_tb = r.ue() + 2, diff_tb = r.ue();
  s.th_depth_inter = r.ue(); s.th_depth_intra = r.ue();
  if (r.get(1)) {                                             // scaling_list_enabled_flag: the default lists, or sps_scaling_list_data
    ScalingLists sl = scaling_defaults();
    if (r.get(1) && !parse_scaling_list_data(r, sl)) return DEC_ERR_INVALID;
    s.scaling = build_scaling(sl);
  }
  s.amp = r.get(1); s.sao = r.get(1);
  if (r.get(1)) {                                               // pcm_enabled_flag
    s.pcm_depth[0] = (int)r.get(4) + 1; s.pcm_depth[1] = (int)r.get(4) + 1;
    s.pcm_min_log2 = (int)r.ue() + 3; s.pcm_max_log2 = s.pcm_min_log2 + (int)r.ue(); s.pcm_no_filter = r.get(1);
    if (r.err || s.pcm_depth[0] > 8 || s.pcm_depth[1] > 8 || s.pcm_min_log2 < log2_min_cb || s.pcm_max_log2 > imin(5, log2_min_cb + diff_cb)) return DEC_ERR_INVALID;
  }
  if (r.err) return DEC_ERR_INVALID;
  // coding geometry: CTB 64 (what Kvazaar always writes), 32 or 16 (round 6: other encoders); coding blocks from 8 (Kvazaar), 16 or 32 up; transform blocks 4 .. min(32, CTB)
  if (log2_min_cb < 3 || log2_min_cb > 5 || diff_cb < 0 || diff_cb > 3) return DEC_ERR_INVALID;
  s.ctb_log2 = log2_min_cb + diff_cb; s.min_cb_log2 = log2_min_cb;
  if (s.ctb_log2 < 4 || s.ctb_log2 > 6 || log2_min_tb != 2 || diff_tb != imin(3, s.ctb_log2 - 2) || s.th_depth_inter > 4 || s.th_depth_intra > 4)
    return DEC_ERR_UNSUPPORTED;
  s.num_st_rps = r.ue();
  if (s.num_st_rps > 64) return DEC_ERR_INVALID;
  for (int k = 0; k < s.num_st_rps; k++) if (!parse_st_rps(r, k, s.num_st_rps, s.st_rps, s.st_rps[k])) return DEC_ERR_INVALID;
  if (r.get(1)) {                                               // long_term_ref_pics_present_flag: candidates by POC LSBs
    s.num_lt_sps = (int)r.ue();
    if (s.num_lt_sps > 32) return DEC_ERR_INVALID;
    for (int k = 0; k < s.num_lt_sps; k++) { s.lt_lsb_sps[k] = (uint16_t)r.get(s.log2_max_poc_lsb); s.lt_used_sps[k] = (uint8_t)r.get(1); }
  }
  s.tmvp = r.get(1);
  s.strong_intra = r.get(1);
  if (r.get(1)) {                                               // VUI: timing only
    if (r.get(1)) { if (r.get(8) == 255) { r.get(16); r.get(16); } }
    if (r.get(1)) r.get(1);
    if (r.get(1)) { r.get(4); if (r.get(1)) r.get(24); }
    if (r.get(1)) { r.ue(); r.ue(); }
    r.get(3);
    if (r.get(1)) { r.ue(); r.ue(); r.ue(); r.ue(); }
    if (r.get(1)) { s.fps_den = r.get(32); s.fps_num = r.get(32); }
  }
  if (r.err) return DEC_ERR_INVALID;
  // sizes: multiples of the minimum coding block; the upper bound is the encoder's (and keeps every index inside 32 bits)
  if ((s.width & ((1 << s.min_cb_log2) - 1)) || (s.height & ((1 << s.min_cb_log2) - 1))) return DEC_ERR_INVALID;      // (7.4.3.2.1: multiples of MinCbSizeY)
  if ((s.width & 7) || (s.height & 7) || s.width < 16 || s.height < 16 || s.width > 16384 || s.height > 16384) return DEC_ERR_UNSUPPORTED;
  if (s.crop_l + s.crop_r >= s.width || s.crop_t + s.crop_b >= s.height) return DEC_ERR_INVALID;
  s.valid = true;
  return 0;
}

int parse_pps(BitReader &r, DecPps &p, int &id)                // PPS (7.3.2.3)
{
  id = r.ue(); p.sps_id = r.ue();
  if (id > 63 || p.sps_id > 15) return DEC_ERR_INVALID;
  int dep = r.get(1); p.output_flag_present = r.get(1); p.extra_header_bits = r.get(3); p.sign_hiding = r.get(1);
  p.cabac_init_present = r.get(1);
  p.num_ref_idx_default = (int)r.ue() + 1; p.num_ref_idx1_default = (int)r.ue() + 1;
  p.init_qp = 26 + r.se();
  if (p.init_qp < 0 || p.init_qp > 51) return DEC_ERR_INVALID;
  int cip = r.get(1); p.tskip = r.get(1); p.cu_qp_delta = r.get(1);
  if (p.cu_qp_delta) { p.qp_delta_depth = r.ue(); if (p.qp_delta_depth > 3) return DEC_ERR_INVALID; }
  p.cb_qp_offset = r.se(); p.cr_qp_offset = r.se(); p.slice_chroma_offsets = r.get(1);
  int wp = r.get(1), wbp = r.get(1), tqb = r.get(1), tiles = r.get(1);
  p.wpp = r.get(1);
  if (r.err || p.num_ref_idx_default > 15 || p.num_ref_idx1_default > 15 || p.cb_qp_offset < -12 || p.cb_qp_offset > 12 || p.cr_qp_offset < -12 || p.cr_qp_offset > 12) return DEC_ERR_INVALID;
  p.dependent_slices = dep;
  p.cip = cip;                                                 // constrained_intra_pred_flag: the kernels' business (reference samples of blocks that are not intra-coded do not count)
  p.weighted_pred = wp; p.weighted_bipred = wbp;
  p.tq_bypass = tqb;
  if (tiles) {                                                 // supported: the level limits of 20 columns x 22 rows (A.4.2); loop filter across tiles on
    const int cols = r.ue() + 1, rows = r.ue() + 1; p.uniform_tiles = r.get(1);
    if (cols > 20 || rows > 22) return DEC_ERR_UNSUPPORTED;
    if (!p.uniform_tiles) {
      for (int k = 0; k < cols - 1; k++) { p.col_width[k] = (int)r.ue() + 1; if (p.col_width[k] > 1024) return DEC_ERR_INVALID; }
      for (int k = 0; k < rows - 1; k++) { p.row_height[k] = (int)r.ue() + 1; if (p.row_height[k] > 1024) return DEC_ERR_INVALID; }
    }
    p.across_tiles = r.get(1);                                 // loop_filter_across_tiles_enabled_flag (Kvazaar writes 0: its tiles are filtered one by one)
    p.tile_rows = rows; p.tile_cols = cols;
  }
  p.loop_filter_across_slices = r.get(1);
  p.deblock_control = r.get(1);
  if (p.deblock_control) {
    p.deblock_override = r.get(1);
    p.deblock_disabled = r.get(1);
    if (!p.deblock_disabled) { p.beta_offset_div2 = r.se(); p.tc_offset_div2 = r.se(); }
  }
  if (r.get(1)) {                                              // pps_scaling_list_data: instead of the SPS's lists
    ScalingLists sl = scaling_defaults();
    if (!parse_scaling_list_data(r, sl)) return DEC_ERR_INVALID;
    p.scaling = build_scaling(sl);
  }
  p.lists_mod = r.get(1);                                       // lists_modification_present_flag
  p.par_mrg_level = (int)r.ue() + 2;
  p.header_extension = r.get(1);
  if (r.err || p.par_mrg_level > 6 || p.beta_offset_div2 < -6 || p.beta_offset_div2 > 6 || p.tc_offset_div2 < -6 || p.tc_offset_div2 > 6) return DEC_ERR_INVALID;
  p.valid = true;
  return 0;
}

// ------------------------------------------------------------------------------------------ slice segment header (7.3.6)
// long-term reference pictures (7.3.6.1): candidates of the SPS by index, then explicit ones; DeltaPocMsbCycleLt accumulates inside each group (7-52)
static int parse_lt_refs(BitReader &r, const DecSps &s, LtRefs &lt)
{
  const int n_sps = s.num_lt_sps > 0 ? (int)r.ue() : 0, n_pics = (int)r.ue();
  if (r.err || n_sps < 0 || n_sps > s.num_lt_sps || n_pics < 0 || n_sps + n_pics > 16) return DEC_ERR_INVALID;
  lt.n = n_sps + n_pics;
  int bits = 0; while ((1 << bits) < s.num_lt_sps) bits++;
  for (int k = 0; k < lt.n; k++) {
    if (k < n_sps) { const int idx = bits ? (int)r.get(bits) : 0; if (idx >= s.num_lt_sps) return DEC_ERR_INVALID; lt.lsb[k] = s.lt_lsb_sps[idx]; lt.used[k] = s.lt_used_sps[idx] != 0; }
    else { lt.lsb[k] = (int)r.get(s.log2_max_poc_lsb); lt.used[k] = r.get(1) != 0; }
    lt.msb[k] = r.get(1) != 0;
    const int delta = lt.msb[k] ? (int)r.ue() : 0;
    if (delta < 0 || delta > (1 << 20) || lt.cycle[k ? k - 1 : 0] > (1 << 24)) return DEC_ERR_INVALID;
    lt.cycle[k] = delta + ((k == 0 || k == n_sps) ? 0 : lt.cycle[k - 1]);
  }
  if (r.err) return DEC_ERR_INVALID;
  return 0;
}

// NumPicTotalCurr = the set's used pictures, short-term and long-term
static int parse_ref_list_mods(BitReader &r, const StRps &rps, const LtRefs &lt, SliceHdr &sh)
{
  int total = 0;
  for (int k = 0; k < rps.n_neg + rps.n_pos; k++) total += rps.used[k] ? 1 : 0;
  for (int k = 0; k < lt.n; k++) total += lt.used[k] ? 1 : 0;
  if (total > 1) {
    int bits = 0; while ((1 << bits) < total) bits++;
    for (int l = 0; l < (sh.is_b ? 2 : 1); l++) {
      sh.list_mod[l] = (uint8_t)r.get(1);
      if (sh.list_mod[l]) for (int i = 0; i < (l ? sh.num_ref_idx1 : sh.num_ref_idx); i++) { const int e = r.get(bits); if (e >= total) return DEC_ERR_INVALID; sh.list_entry[l][i] = (uint8_t)e; }
    }
  }
  return 0;
}

// pred_weight_table() (7.3.6.3; one layer: every entry's picture differs from the current one, so every flag is there) and 7.4.7.3
static int parse_pred_weight_table(BitReader &r, SliceHdr &sh)
{
  sh.weighted = true;
  const int ld = (int)r.ue(), cd = ld + r.se();
  if (ld < 0 || ld > 7 || cd < 0 || cd > 7) return DEC_ERR_INVALID;
  sh.wt_log2[0] = (uint8_t)ld; sh.wt_log2[1] = (uint8_t)cd;
  for (int k = 0; k < 32; k++) { sh.wt[k].w[0] = (int16_t)(1 << ld); sh.wt[k].w[1] = sh.wt[k].w[2] = (int16_t)(1 << cd); sh.wt[k].o[0] = sh.wt[k].o[1] = sh.wt[k].o[2] = 0; }
  for (int l = 0; l < (sh.is_b ? 2 : 1); l++) {
    const int n = l ? sh.num_ref_idx1 : sh.num_ref_idx;
    uint32_t lf = 0, cf = 0;
    for (int i = 0; i < n; i++) lf |= (uint32_t)r.get(1) << i;
    for (int i = 0; i < n; i++) cf |= (uint32_t)r.get(1) << i;
    for (int i = 0; i < n; i++) {
      DecWt &e = sh.wt[l * 16 + i];
      if ((lf >> i) & 1) {
        const int dw = r.se(), lo = r.se();
        if (dw < -128 || dw > 127 || lo < -128 || lo > 127) return DEC_ERR_INVALID;
        e.w[0] = (int16_t)((1 << ld) + dw); e.o[0] = (int16_t)lo;
      }
      if ((cf >> i) & 1) for (int j = 0; j < 2; j++) {
        const int dw = r.se(), dof = r.se();
        if (dw < -128 || dw > 127 || dof < -512 || dof > 511) return DEC_ERR_INVALID;
        const int w = (1 << cd) + dw;
        e.w[1 + j] = (int16_t)w; e.o[1 + j] = (int16_t)clip3(-128, 127, 128 + dof - ((128 * w) >> cd));
      }
    }
  }
  if (r.err) return DEC_ERR_INVALID;
  for (int k = 0; k < 32; k++) { const DecWt &e = sh.wt[k]; if (e.w[0] != (1 << ld) || e.w[1] != (1 << cd) || e.w[2] != (1 << cd) || e.o[0] || e.o[1] || e.o[2]) sh.wt_explicit |= 1u << k; }
  return 0;
}

static int parse_deblock_override(BitReader &r, const DecPps &p, SliceHdr &sh)
{
  sh.deblock_disabled = p.deblock_disabled; sh.beta_offset_div2 = p.beta_offset_div2; sh.tc_offset_div2 = p.tc_offset_div2;
  if (p.deblock_override && r.get(1)) {
    sh.deblock_disabled = r.get(1);
    if (!sh.deblock_disabled) { sh.beta_offset_div2 = r.se(); sh.tc_offset_div2 = r.se(); }
    if (sh.beta_offset_div2 < -6 || sh.beta_offset_div2 > 6 || sh.tc_offset_div2 < -6 || sh.tc_offset_div2 > 6) return DEC_ERR_INVALID;
  }
  return 0;
}

int parse_slice_header_rest(BitReader &r, const DecSps &s, const DecPps &p, bool idr, int prev_poc, bool no_rasl, SliceHdr &sh, StRps &rps, LtRefs &lt, bool &across_slices)
{
  if (p.output_flag_present) sh.no_output = r.get(1) == 0;
  if (!idr) {
    const int lsb = r.get(s.log2_max_poc_lsb), max_lsb = 1 << s.log2_max_poc_lsb;
    const int prev_lsb = prev_poc & (max_lsb - 1), prev_msb = prev_poc - prev_lsb;
    int msb = prev_msb;
    if (lsb < prev_lsb && prev_lsb - lsb >= max_lsb / 2) msb = prev_msb + max_lsb;
    else if (lsb > prev_lsb && lsb - prev_lsb > max_lsb / 2) msb = prev_msb - max_lsb;
    if (no_rasl) msb = 0;
    sh.poc = msb + lsb;
    if (r.get(1)) {
      int idx = 0, bits = 0; while ((1 << bits) < s.num_st_rps) bits++;
      if (s.num_st_rps == 0) return DEC_ERR_INVALID;
      if (bits) idx = r.get(bits);
      if (idx >= s.num_st_rps) return DEC_ERR_INVALID;
      rps = s.st_rps[idx];
    } else if (!parse_st_rps(r, s.num_st_rps, s.num_st_rps, s.st_rps, rps)) return DEC_ERR_INVALID;
    if (s.num_lt_sps >= 0) if (const int rc = parse_lt_refs(r, s, lt)) return rc;
    if (s.tmvp) sh.tmvp = r.get(1);
  }
  if (s.sao) { sh.sao_luma = r.get(1); sh.sao_chroma = r.get(1); }
  sh.num_ref_idx = p.num_ref_idx_default; sh.num_ref_idx1 = sh.is_b ? p.num_ref_idx1_default : 0;
  if (!sh.is_intra) {
    if (r.get(1)) { sh.num_ref_idx = (int)r.ue() + 1; if (sh.is_b) sh.num_ref_idx1 = (int)r.ue() + 1; }
    if (sh.num_ref_idx < 1 || sh.num_ref_idx > 15 || (sh.is_b && (sh.num_ref_idx1 < 1 || sh.num_ref_idx1 > 15))) return DEC_ERR_INVALID;
    if (p.lists_mod) if (const int rc = parse_ref_list_mods(r, rps, lt, sh)) return rc;      // ref_pic_lists_modification()
    if (sh.is_b) sh.mvd_l1_zero = r.get(1);
    if (p.cabac_init_present) sh.cabac_init_flag = r.get(1);
    if (sh.tmvp) {
      if (sh.is_b) sh.collocated_from_l0 = r.get(1);
      const int n = sh.collocated_from_l0 ? sh.num_ref_idx : sh.num_ref_idx1;
      if (n > 1) { sh.collocated_ref_idx = r.ue(); if (sh.collocated_ref_idx < 0 || sh.collocated_ref_idx >= n) return DEC_ERR_INVALID; }
    }
    if (sh.is_b ? p.weighted_bipred : p.weighted_pred) if (const int rc = parse_pred_weight_table(r, sh)) return rc;
    sh.max_merge = 5 - (int)r.ue();
    if (sh.max_merge < 1 || sh.max_merge > 5) return DEC_ERR_INVALID;
  }
  sh.slice_qp = p.init_qp + r.se();
  if (sh.slice_qp < 0 || sh.slice_qp > 51) return DEC_ERR_INVALID;
  sh.cb_qp_offset = p.cb_qp_offset; sh.cr_qp_offset = p.cr_qp_offset;
  if (p.slice_chroma_offsets) { sh.cb_qp_offset += r.se(); sh.cr_qp_offset += r.se(); }
  if (sh.cb_qp_offset < -12 || sh.cb_qp_offset > 12 || sh.cr_qp_offset < -12 || sh.cr_qp_offset > 12) return DEC_ERR_INVALID;
  if (const int rc = parse_deblock_override(r, p, sh)) return rc;
  across_slices = p.loop_filter_across_slices != 0;
  if (p.loop_filter_across_slices && (!sh.deblock_disabled || sh.sao_luma || sh.sao_chroma)) across_slices = r.get(1) != 0;
  return 0;
}

// tile boundaries (6.5.1) for this picture size
int tile_boundaries(DecPps &pp, int wc, int hc)
{
  if (pp.tile_rows > hc) return DEC_ERR_INVALID;
  pp.row_bd[0] = 0;
  for (int k = 0; k < pp.tile_rows; k++) {
    const int hgt = pp.uniform_tiles ? ((k + 1) * hc) / pp.tile_rows - (k * hc) / pp.tile_rows : (k < pp.tile_rows - 1 ? pp.row_height[k] : hc - pp.row_bd[k]);
    if (hgt < 1) return DEC_ERR_INVALID;
    pp.row_bd[k + 1] = pp.row_bd[k] + hgt;
  }
  if (pp.row_bd[pp.tile_rows] != hc) return DEC_ERR_INVALID;
  if (pp.tile_cols > wc) return DEC_ERR_INVALID;
  pp.col_bd[0] = 0;
  for (int k = 0; k < pp.tile_cols; k++) {
    const int wid = pp.uniform_tiles ? ((k + 1) * wc) / pp.tile_cols - (k * wc) / pp.tile_cols : (k < pp.tile_cols - 1 ? pp.col_width[k] : wc - pp.col_bd[k]);
    if (wid < 1) return DEC_ERR_INVALID;
    pp.col_bd[k + 1] = pp.col_bd[k] + wid;
  }
  if (pp.col_bd[pp.tile_cols] != wc) return DEC_ERR_INVALID;
  return 0;
}

// an independent slice of a picture under way: the same slice parameters as the first (what this decoder keeps per picture; inside one tile a slice may have its own SliceQpY)
bool same_slice_params(const SliceHdr &sh, const SliceHdr &a, bool tiles)
{
  return !(sh.is_intra != a.is_intra || sh.is_b != a.is_b || sh.num_ref_idx1 != a.num_ref_idx1 || sh.mvd_l1_zero != a.mvd_l1_zero || sh.collocated_from_l0 != a.collocated_from_l0 || sh.poc != a.poc || sh.tmvp != a.tmvp || sh.collocated_ref_idx != a.collocated_ref_idx || sh.sao_luma != a.sao_luma ||
      sh.sao_chroma != a.sao_chroma || sh.num_ref_idx != a.num_ref_idx || sh.cabac_init_flag != a.cabac_init_flag || sh.max_merge != a.max_merge ||
      (sh.slice_qp != a.slice_qp && tiles) || sh.cb_qp_offset != a.cb_qp_offset || sh.cr_qp_offset != a.cr_qp_offset || sh.deblock_disabled != a.deblock_disabled ||
      sh.beta_offset_div2 != a.beta_offset_div2 || sh.tc_offset_div2 != a.tc_offset_div2 ||
      memcmp(sh.list_mod, a.list_mod, 2) || memcmp(sh.list_entry, a.list_entry, sizeof(sh.list_entry)) ||
      sh.wt_explicit != a.wt_explicit || sh.weighted != a.weighted || (sh.weighted && (memcmp(sh.wt, a.wt, sizeof(sh.wt)) || sh.wt_log2[0] != a.wt_log2[0] || sh.wt_log2[1] != a.wt_log2[1])));
}

int parse_segment_tail(BitReader &r, bool entry_points, bool header_extension, std::vector<uint32_t> &entry, size_t &hdr)
{
  if (entry_points) {
    const int nep = r.ue();
    if (nep < 0 || nep > 1024) return DEC_ERR_INVALID;
    if (nep > 0) { int bits = r.ue() + 1; if (bits > 32) return DEC_ERR_INVALID; for (int k = 0; k < nep; k++) entry.push_back(r.get(bits) + 1); }
  }
  if (header_extension) { const int n = r.ue(); if (n > 256) return DEC_ERR_INVALID; for (int k = 0; k < n; k++) r.get(8); }
  if (!r.get(1)) return DEC_ERR_INVALID;                         // byte_alignment()
  while (r.pos & 7) r.get(1);
  if (r.err) return DEC_ERR_INVALID;
  hdr = r.pos >> 3;
  return 0;
}

// Substream starts inside the unescaped slice data (starts[0] = base: where the segment's bytes will lie).  entry_point offsets count bytes of the NAL
// unit payload INCLUDING emulation prevention bytes (7.4.7.1); epb[] holds, for every removed
// byte, how many unescaped payload bytes preceded it.
std::vector<size_t> substream_starts(const std::vector<uint32_t> &entry, const std::vector<size_t> &epb, size_t hdr, size_t base)
{
  std::vector<size_t> starts(1, base);
  size_t esc = hdr;                                            // escaped offset of the slice data in the payload
  for (size_t k = 0; k < epb.size(); k++) if (epb[k] < hdr) esc++;
  for (uint32_t e : entry) {
    esc += e;
    size_t removed = 0;
    for (size_t k = 0; k < epb.size(); k++) if (epb[k] + k < esc) removed++;     // epb k sits at escaped offset epb[k] + k
    starts.push_back(base + esc - removed - hdr);
  }
  return starts;
}

}  // namespace kvzx
