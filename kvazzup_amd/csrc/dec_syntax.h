// kvazzup_amd/csrc/dec_syntax.h -- the decoder's header syntax (H.265 7.3.1 - 7.3.6): bits to plain structs.  Parameter sets, the self-contained parts of
// the slice segment header, tile boundaries, entry points.  Nothing here knows the Decoder (decoder.h): every function takes a BitReader and plain structs and
// returns 0 or the error code the decoder hands on.  Plain C++17, no HIP: `g++ -std=c++17 -fsyntax-only -x c++ dec_syntax.hip` passes.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <memory>
#include <vector>
#include "hevc_core.h"
#include "dec_frame.h"
#include "scaling_tables.h"

namespace kvzx {

enum { DEC_ERR_INVALID = -1, DEC_ERR_UNSUPPORTED = -2, DEC_ERR_GPU = -3, DEC_ERR_HASH = -4, DEC_SEG_ENDS_EARLY = -100 /* internal: PicJob::ambiguous_end */ };      // (-4: a decoded picture hash SEI did not match, libOpenHevcSetCheckMD5)

// ------------------------------------------------------------------------------------------ bits
struct BitReader {
  const uint8_t *p; size_t n, pos = 0; bool err = false;
  BitReader(const uint8_t *b, size_t len) : p(b), n(len) {}
  uint32_t bit() { if (pos >= n * 8) { err = true; pos++; return 0; } uint32_t b = (p[pos >> 3] >> (7 - (pos & 7))) & 1; pos++; return b; }
  uint32_t get(int k) { uint32_t v = 0; for (int i = 0; i < k; i++) v = (v << 1) | bit(); return v; }
  // (at most 30 leading zeros: the value stays below 2^31, so that every `(int)r.ue()` and `r.ue() + 1` below is a non-negative int and the callers' upper-bound
  // checks are range checks -- a 32-bit code word used to come out as a NEGATIVE index that passed `id > 63`; found by tools/fuzz_parser.py under ASan)
  uint32_t ue() { int z = 0; while (!bit()) { if (++z > 30 || err) { err = true; return 0; } } return z ? ((1u << z) - 1) + get(z) : 0; }
  int32_t se() { uint32_t k = ue(); return (k & 1) ? (int32_t)((k + 1) >> 1) : -(int32_t)(k >> 1); }
};

inline int ctbs_in(int size, int ctb_log2) { return (size + (1 << ctb_log2) - 1) >> ctb_log2; }      // a picture dimension in coding tree blocks

// short-term reference picture set (7.4.8): negative deltas first (closest first), then positive ones
struct StRps { int n_neg = 0, n_pos = 0; int dpoc[16]; uint8_t used[16]; };

struct DecSps {
  bool valid = false;
  int width = 0, height = 0;          // coded size
  int crop_r = 0, crop_b = 0, crop_l = 0, crop_t = 0;   // luma samples
  int log2_max_poc_lsb = 8;
  int num_st_rps = 0; StRps st_rps[65];
  uint32_t fps_num = 0, fps_den = 0;
  int num_reorder = 0;                // sps_max_num_reorder_pics of the highest sub-layer: pictures that may precede a picture in decoding order and follow it in output order
  int strong_intra = 0, sao = 0, tmvp = 0, amp = 0, th_depth_inter = 0, th_depth_intra = 0;
  int ctb_log2 = 6;                   // CtbLog2SizeY: 6 (every Kvazaar stream), 5 or 4 (round 6: other encoders' streams); transform blocks 4 .. min(32, CTB)
  int min_cb_log2 = 3;                // MinCbLog2SizeY: 3 (every Kvazaar stream), 4 or 5
  int wc() const { return ctbs_in(width, ctb_log2); }      // the picture in coding tree blocks
  int hc() const { return ctbs_in(height, ctb_log2); }
  int num_lt_sps = -1; uint16_t lt_lsb_sps[32] = {}; uint8_t lt_used_sps[32] = {};      // long_term_ref_pics_present_flag (-1: not set): the SPS's candidates
  int pcm_depth[2] = {0, 0}, pcm_min_log2 = 0, pcm_max_log2 = 0, pcm_no_filter = 0;      // pcm_enabled_flag: PcmBitDepthY / C (0: no PCM), Log2MinIpcmCbSizeY .. Log2MaxIpcmCbSizeY, pcm_loop_filter_disabled_flag
  // scaling_list_enabled_flag: the scaling factors (dec_frame.h KVZ_SCALING_BYTES) of the SPS's lists -- the default ones (Tables 7-5 / 7-6) without
  // sps_scaling_list_data; NULL: flat.  What uvgComm's "scaling list" checkbox switches on in a peer's Kvazaar (kvazaarfilter.cpp:235-242).
  std::shared_ptr<const std::vector<uint8_t>> scaling;
};
struct DecPps {
  bool valid = false;
  int sps_id = 0;
  int sign_hiding = 0, cabac_init_present = 0, num_ref_idx_default = 1, num_ref_idx1_default = 1, init_qp = 26, tskip = 0;
  int dependent_slices = 0;
  int cu_qp_delta = 0, qp_delta_depth = 0, cb_qp_offset = 0, cr_qp_offset = 0, slice_chroma_offsets = 0;
  int weighted_pred = 0, weighted_bipred = 0, lists_mod = 0;
  int output_flag_present = 0, extra_header_bits = 0, header_extension = 0;
  int wpp = 0, tile_rows = 1, row_bd[34];   // tile row i covers CTB rows [row_bd[i], row_bd[i + 1]); filled at slice time when uniform
  int tile_cols = 1, col_bd[34];            // tile column j covers CTB columns [col_bd[j], col_bd[j + 1])
  int uniform_tiles = 1, row_height[33], col_width[33];
  int deblock_control = 0, deblock_override = 0, deblock_disabled = 0, beta_offset_div2 = 0, tc_offset_div2 = 0, loop_filter_across_slices = 1, across_tiles = 1, cip = 0;
  int par_mrg_level = 2;
  int tq_bypass = 0;                                   // transquant_bypass_enabled_flag (a peer's Kvazaar with `lossless`, kvazaarfilter.cpp:244)
  std::shared_ptr<const std::vector<uint8_t>> scaling; // pps_scaling_list_data: these factors instead of the SPS's
};

struct SliceHdr {
  bool is_intra = false, is_b = false; int poc = 0;
  bool no_output = false;                                              // pic_output_flag = 0: decoded and kept as a reference, never handed out
  int num_ref_idx1 = 0, mvd_l1_zero = 0, collocated_from_l0 = 1;      // B slices: num_ref_idx_l1_active, mvd_l1_zero_flag, collocated_from_l0_flag
  int tmvp = 0, collocated_ref_idx = 0, sao_luma = 0, sao_chroma = 0, num_ref_idx = 1, cabac_init_flag = 0, max_merge = 5;
  int slice_qp = 26, cb_qp_offset = 0, cr_qp_offset = 0;      // offsets: PPS + slice
  int deblock_disabled = 0, beta_offset_div2 = 0, tc_offset_div2 = 0;
  uint8_t list_mod[2] = {0, 0}, list_entry[2][16] = {};      // ref_pic_lists_modification() (7.3.6.2): entries of the temporary lists (8.3.4)
  bool weighted = false; uint8_t wt_log2[2] = {0, 0}; DecWt wt[32] = {};
  uint32_t wt_explicit = 0;                                        // bit list * 16 + index: the entry's weights or offsets differ from the defaults (with the defaults the explicit formulas ARE the default ones)      // pred_weight_table() (7.3.6.3) as derived by 7.4.7.3: entry list * 16 + index
};

// the slice header's long-term entries (7.3.6.1): POC LSBs, used_by_curr_pic_lt_flag, delta_poc_msb_present_flag, DeltaPocMsbCycleLt
struct LtRefs { int n = 0, lsb[16] = {}, cycle[16] = {}; bool used[16] = {}, msb[16] = {}; };

inline const CoreTabs *host_tabs()               // (function-local statics: initialised once, thread-safe -- parse workers race to the first call)
{
  static const CoreTabs t = [] { CoreTabs t; for (int i = 0; i < 64; i++) core_tabs_fill_entry(t, i); return t; }();
  return &t;
}

// scan position -> (x, y) for the three scans and block sizes 1..8 (H.265 6.5.3-6.5.5)
struct ScanTabs { uint8_t x[3][4][64], y[3][4][64], inv[3][4][64], sigk[3][5][16]; };   // sigk[scan][prev_csbf, 4 = 4x4 block][scan position k] = context pattern; inv[scan][log2 of the grid][y << log2 | x] = scan position
inline const ScanTabs &scan_tabs()
{
  static const ScanTabs t = [] {
    ScanTabs t;
    const CoreTabs *ct = host_tabs();
    for (int sc = 0; sc < 3; sc++) for (int l2 = 0; l2 < 4; l2++) for (int i = 0; i < (1 << (2 * l2)); i++) {
      int x, y; scan_pos(ct, sc, l2, i, x, y); t.x[sc][l2][i] = (uint8_t)x; t.y[sc][l2][i] = (uint8_t)y; t.inv[sc][l2][(y << l2) | x] = (uint8_t)i;
    }
    for (int sc = 0; sc < 3; sc++) for (int k = 0; k < 16; k++) {
      for (int pc = 0; pc < 4; pc++) t.sigk[sc][pc][k] = ct->sigpat[pc][ct->pos4[sc][k]];
      t.sigk[sc][4][k] = ct->ctxmap4x4[ct->pos4[sc][k]];
    }
    return t;
  }();
  return t;
}

bool parse_st_rps(BitReader &r, int idx, int num_in_sps, const StRps *all, StRps &out);
// parameter sets: 0, or the error code; the caller stores what came out (`id`: which table entry)
struct VpsTiming { bool present = false; uint32_t fps_num = 0, fps_den = 0; };
int parse_vps(BitReader &r, VpsTiming &t);
int parse_sps(BitReader &r, DecSps &s, int &id);
int parse_pps(BitReader &r, DecPps &p, int &id);
// the slice segment header of an independent slice behind slice_type, up to the entry points (7.3.6.1); prev_poc: prevTid0Pic's (8.3.1), no_rasl: NoRaslOutputFlag
int parse_slice_header_rest(BitReader &r, const DecSps &s, const DecPps &p, bool idr, int prev_poc, bool no_rasl, SliceHdr &sh, StRps &rps, LtRefs &lt, bool &across_slices);
int tile_boundaries(DecPps &pp, int wc, int hc);                 // 6.5.1: fills row_bd / col_bd of the picture's copy of its PPS
bool same_slice_params(const SliceHdr &sh, const SliceHdr &a, bool tiles);
// the header's tail: entry points (when the PPS has them), header extension, byte_alignment(); `hdr`: the header's length in bytes
int parse_segment_tail(BitReader &r, bool entry_points, bool header_extension, std::vector<uint32_t> &entry, size_t &hdr);
std::vector<size_t> substream_starts(const std::vector<uint32_t> &entry, const std::vector<size_t> &epb, size_t hdr, size_t base);

}  // namespace kvzx
