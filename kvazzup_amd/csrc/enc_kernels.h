// kvazzup_amd/csrc/enc_kernels.h -- launch wrappers of the encoder kernels (each defined in the file of its kernel: enc_kernels.hip, recon_kernels.hip, loop_kernels.hip, ...)
#pragma once
#include <hip/hip_runtime.h>
#include "hevc_core.h"
namespace kvzx {
void launch_pad_input(const uint8_t *in, int w, int h, uint8_t *dy, uint8_t *du, uint8_t *dv, int cw, int ch, hipStream_t st);   // packed I420 -> padded planes
void launch_me(const EncFrame &f, hipStream_t st);
void launch_luma_quarter(const uint8_t *src, uint8_t *q, int cw, int ch, hipStream_t st);      // me-coarse: the quarter picture of a padded luma plane
void launch_me_coarse(const EncFrame &f, hipStream_t st);                                        // me-coarse: the centres of a P picture's blocks, per reference
void launch_subpel(const EncFrame &f, hipStream_t st);     // k_subpel: fractional-sample refinement of the searched vectors (f.subme > 0)
void launch_inter_recon(const EncFrame &f, hipStream_t st);
void launch_inter_signal(const EncFrame &f, hipStream_t st);
void launch_intra_analyse(const EncFrame &f, hipStream_t st);
void launch_intra_recon(const EncFrame &f, hipStream_t st);
void launch_deblock(const EncFrame &f, hipStream_t st);
void launch_vaq(const EncFrame &f, int vaq, int *act, int *sum, hipStream_t st);   // VAQ: f.ctu_qt holds ROI deltas on entry, target QPs on exit
void launch_sao(const EncFrame &f, hipStream_t st);        // SAO decision + filter: f.rec (deblocked) -> f.sao_out, parameters -> f.sao
void launch_qp_resolve(const EncFrame &f, hipStream_t st);  // per-CTU QP: first coded CU, QpY, delta (no-op without a QP map)
void launch_deblock_v(const EncFrame &f, hipStream_t st);   // vertical edges of the band
void launch_deblock_h(const EncFrame &f, hipStream_t st, int part = 0);   // part: 0 all horizontal edges of the band, 1 the inner ones, 2 its two boundary edges
void launch_tokenize(const EncFrame &f, hipStream_t st);    // k_tokenize: bins of every CTU into its slot, pieces in completion order
void launch_tok_compact(const EncFrame &f, hipStream_t st); // k_tok_compact: coding order restored, dense copy to host-mapped memory
// rate control v2 (rc_kernels.hip; the groups of CTU rows themselves: k_inter_recon's RC form, EncFrame::rc)
void launch_picture_begin(RcState *rc, uint32_t bits3, int slot3, int have3, int8_t *ctu_qt, const int8_t *roi, int nctu, int qp, int vaq, hipStream_t st,
                          void *zero_a = nullptr, size_t bytes_a = 0, void *zero_b = nullptr, size_t bytes_b = 0);      // head of a picture's chain: rate control state (rc != NULL) and the per-CTU target QPs (ctu_qt != NULL) in one launch
// "weightp" (wp_kernels.hip)
struct WpArgs {
  const unsigned long long *partial; int nblk;        // k_wp_stats' partial sums {S1, S2} of the picture, wp_stat_blocks(height) pairs
  long long n;                                       // width * height
  int64_t *stat;                                     // the picture's {m, v} (wp_moments), kept with its working set
  const int64_t *stat_ref[KVZ_MAX_LP_REFS];          // ... and those of its references' input pictures
  const uint8_t *in_ref[KVZ_MAX_LP_REFS];            // the references' padded input luma planes
  int nref;                                          // 0: an intra picture -- the moments only
  int32_t *cand; unsigned long long *acc;            // scratch: [reference][candidate, w, o] and the check's [reference][plain, weighted]
  int32_t *rec, *rec_host;                           // the record [reference][flag, w, o]: device memory / the slot's host-mapped copy
};
struct WpPlaneArgs { const int32_t *rec; const uint8_t *from[KVZ_MAX_LP_REFS]; uint8_t *to[KVZ_MAX_LP_REFS]; };
int wp_stat_blocks(int height);
void launch_wp_stats(const uint8_t *src, int cw, int width, int height, unsigned long long *partial, hipStream_t st);
void launch_wp_decide(const WpArgs &a, int phase, hipStream_t st);      // phase 0: moments, candidates; phase 1: the record
void launch_wp_check(const WpArgs &a, const uint8_t *cur, int cw, int width, int height, hipStream_t st);
void launch_wp_plane(const WpPlaneArgs &a, int nref, int cw, int ch, hipStream_t st);      // the references' search planes
// "scenecut" (sc_kernels.hip)
struct ScArgs {
  const uint8_t *qc, *qp;                            // the quarter pictures of this input picture and of the previous one (k_luma_quarter), qw x qh samples
  int qw, qh, vw, vh;                                // ... of which vw x vh are visible
  int bw, bh, rq;                                    // sc_visible_blocks, sc_reach
  unsigned long long *sum_c; const unsigned long long *sum_p;   // the sums over the visible quarter samples, kept with the pictures' working sets
  uint32_t *blocks;                                  // [block, raster][S, A] of the picture last examined
  uint32_t *n_new;                                   // counter of new blocks: zero between pictures (k_sc_decide leaves it so)
  int32_t *rec, *rec_host;                           // the record {examined, n_new, n_b, d, cut}: device memory / the slot's host-mapped copy
};
void launch_sc_sum(const ScArgs &a, hipStream_t st);      // every picture: sum_c (zero before the launch) += the visible samples of qc
void launch_sc_blocks(const ScArgs &a, hipStream_t st);   // an examined picture: (S, A) of every block, n_new
void launch_sc_decide(const ScArgs &a, hipStream_t st);   // ... and its record
// "loss-feedback" (fb_kernels.hip)
struct FbArgs {
  int gw, gh;                                        // the cell grid: coded width / 8, coded height / 8
  const int16_t *cu_mv; const uint8_t *cu_intra, *cu_log2;   // k_fb_record: the working set's final arrays; clean: the record of an IDR picture, KVZ_FB_CLEAN (the statement's; the engine files none, it never steps through one)
  int clean;
  int16_t *rec_mv; uint8_t *rec_info;                // one picture's record in the ring: [cell][2] vectors, [cell] fb_info (written by k_fb_record, read by k_fb_step)
  uint8_t *map, *tmp;                                // the map being taken to the heal picture, and a step's scratch, one byte a cell
  int first, count, dilate;                          // k_fb_seed: the reported coding tree blocks; dilate: deblocking or SAO is on
  int me_range; uint8_t *blk; int32_t *stat;         // k_fb_blocks: the block records [32x32 block][2] and the slot's host-mapped record {heal, reports, cells, forced quarters}
};
// "fb-anchor" (DESIGN.md section 9j): what the kernels of a v2 heal picture's record take on top -- an argument block of their own, so that the kernels of before
// keep theirs.  cu_ref: k_fb_record_ref files the cell's reference index into the info byte (KVZ_FB_REF1), k_fb_refs counts; anchor_bad: k_fb_step_ref -- the
// record's reference-1 cells are in S (the report reaches that picture's anchor) or never are
struct FbRefArgs : FbArgs { const uint8_t *cu_ref; int anchor_bad; };
void launch_fb_record(const FbArgs &a, hipStream_t st);   // every P picture with the option on, behind its chain
void launch_fb_seed(const FbArgs &a, hipStream_t st);     // a heal picture: one report into the map
void launch_fb_step(const FbArgs &a, hipStream_t st);     // ... the map through one picture's record
void launch_fb_blocks(const FbArgs &a, hipStream_t st);   // ... the block records and the counts
void launch_fb_record_ref(const FbRefArgs &a, hipStream_t st);   // fb-anchor, a v2 heal picture: its record with the reference bit
void launch_fb_step_ref(const FbRefArgs &a, hipStream_t st);     // ... a later heal picture: the map through that record
void launch_fb_refs(const FbRefArgs &a, hipStream_t st);         // ... behind its decisions: the quarters coded from reference 1 into stat[7]
// k_cabac_rows (cabac_kernels.hip): the arithmetic coder proper on the GPU, one wave per substream
struct CabacRowsArgs {
  const uint16_t *tok; const int32_t *count; const uint32_t *off;   // dense tokens (device): CTU i has count[i] tokens at tok + off[i]
  uint8_t *stage; uint32_t stage_cap;     // device: every substream codes into a range reserved for its worst case
  uint8_t *out; uint32_t out_cap;         // host-mapped: the finished substreams, dense, in completion order
  uint32_t *cursors;                      // device {staging bytes reserved, output bytes reserved}: zero before the launch (k_tok_compact)
  uint32_t *sub_off, *sub_len, *sub_bins; // host-mapped, per substream of the launch: byte range in `out`, bins coded; sub_len == ~0u: did not fit
  uint32_t *ctx_save, *ctx_ready;         // device [CTU rows][40] context words after the row's second CTU, [CTU rows] generation of that copy
  uint32_t gen;                           // generation of this launch (differs from the previous launch with the same arrays)
  uint32_t *err;                          // device error flags (64: a row waited for its upper neighbour in vain)
  int wc, hc, wpp, tile_rows, init_type, qp, first_sub;
};
void launch_cabac_rows(const CabacRowsArgs &a, int nsub, hipStream_t st);
}  // namespace kvzx
