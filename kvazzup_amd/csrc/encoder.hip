// kvazzup_amd/csrc/encoder.hip -- see encoder.h
#include <chrono>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "encoder.h"
#include "enc_kernels.h"
#include "stream_pool.h"
#include "scaling_tables.h"
#include "pic_hash.h"

namespace kvzx {

// Events that only order this library's streams among themselves (never waited for or queried by the host): no system-scope fence when they complete --
// the default makes every record write back and invalidate the caches for the host's benefit, a bubble of its own in a chain of 10-50 us kernels.
static const unsigned kDeviceEvent = hipEventDisableTiming | hipEventDisableSystemFence;

#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { if (error) *error = std::string(#expr) + ": " + hipGetErrorString(e_); return false; } } while (0)
#define HIP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fprintf(stderr, "kvazzup_amd: %s failed: %s\n", #expr, hipGetErrorString(e_)); return false; } } while (0)

// the me-source block of one working set, or the shared one: k_me's 16x16 costs, the candidate list with the intra pricing's arrival counters and scratch
static void point_me_block(EncFrame &f, const EncLayout &L, uint32_t *block)
{
  f.me_cost16 = block; f.me_cand = block + L.me_cand_off;
  f.ip_arrive = block + L.ip_arrive_off; f.ip_scratch = (uint64_t *)(block + L.ip_scratch_off);
}

// the arrays of one intra chain: progress counters, and per plane the CTUs' right columns and bottom rows
static void point_chain(EncFrame &f, const EncLayout &L, const EncChain &c)
{
  f.sync = c.sync;
  for (int p = 0; p < 3; p++) { f.edge_col[p] = c.edge_col + L.edge_col_off(p); f.edge_row[p] = c.edge_row + L.edge_row_off(p); }
}

// ... allocated and cleared (tagged words: generation 0 = never written); SAO: the chain's work picture too
bool Encoder::build_chain(EncChain &c, std::string *error)
{
  HIP_OK(mem_.dev(&c.sync, lay_.sync, true)); HIP_OK(mem_.dev(&c.edge_col, lay_.edge_col, true)); HIP_OK(mem_.dev(&c.edge_row, lay_.edge_row, true));
  if (cfg_.sao) for (int p = 0; p < 3; p++) HIP_OK(mem_.dev(&c.work[p], lay_.plane(p)));
  return true;
}

Encoder *Encoder::create(const EncoderConfig &cfg, std::string *error)
{
  Encoder *e = new Encoder();
  if (!e->init(cfg, error)) { delete e; return nullptr; }
  return e;
}

bool Encoder::init(const EncoderConfig &cfg_in, std::string *error)
{
  EncoderConfig cfg = cfg_in;
  if (cfg.vaq > 0) cfg.qp_in_cu = 1;                       // the deltas travel as cu_qp_delta
  if (cfg.lossless) { cfg.deblock = 0; cfg.sao = 0; cfg.rdoq = 0; cfg.signhide = 0; cfg.bitrate = 0; cfg.rc_bands = 0; }      // (oracle/hevc_enc.c "lossless")
  if (cfg.bitrate <= 0 || cfg.band_rows > 0) cfg.rc_bands = 0;
  if (cfg.rc_bands > 8) cfg.rc_bands = 8;                  // (RcState::acc)
  if ((cfg.slices == 1 && !cfg.wpp) || (cfg.slices == 2 && cfg.tile_rows * cfg.tile_cols < 2) || (cfg.slices == 1 && cfg.tile_cols > 1) || cfg.slices < 0 || cfg.slices > 2) cfg.slices = 0;
  if (cfg.band_rows > 0) cfg.intra_in_p = 0;               // (intra-in-P runs behind the whole picture's inter reconstruction: not in band mode, where a picture is coded in parts by several instances)
  if (cfg.rc_bands > 0) cfg.qp_in_cu = 1;                  // ... and so do the steps of rate control v2
  if (cfg.band_rows > 0) cfg.me_source = 0;                // (a band's search window reaches into the neighbouring bands' rows: the halo carries reconstruction rows, not source rows)
  if (cfg.lp_refs < 1 || cfg.lp_refs > KVZ_MAX_LP_REFS) { if (error) *error = "lp-refs out of range (0 .. 4)"; return false; }
  if (cfg.lp_refs > 1 && cfg.band_rows > 0) { if (error) *error = "lp-refs >= 2 is not available in band mode (the halo exchange carries one reference picture's rows)"; return false; }
  if (cfg.tmvp && cfg.band_rows > 0) { if (error) *error = "tmvp is not available in band mode"; return false; }
  if (cfg.lp_gop && cfg.gop_g >= 1) {                      // "lp-gop" with a gop=lp-g<g>d<d>t<t> string; without the string the option has nothing to say
    if (cfg.band_rows > 0) { if (error) *error = "lp-gop is not available in band mode (the halo exchange carries one reference picture's rows)"; return false; }
    if (cfg.gop_t > 1) { if (error) *error = "lp-gop: temporal sub-layers (gop=lp-g..d..t2 and more) are not implemented, only t1"; return false; }
    if (cfg.gop_d < 1 || cfg.gop_d > 6) { if (error) *error = "lp-gop: the gop string's d (QP layers) must be 1 .. 6"; return false; }
  }
  if (cfg.me_coarse != 0 && cfg.me_coarse != 64 && cfg.me_coarse != 128 && cfg.me_coarse != 256) { if (error) *error = "me-coarse must be 0, 64, 128 or 256"; return false; }
  if (cfg.me_coarse && cfg.band_rows > 0) { if (error) *error = "me-coarse is not available in band mode (the halo exchange carries a few rows)"; return false; }
  if (cfg.weightp && cfg.band_rows > 0) { if (error) *error = "weightp is not available in band mode (a band's encoder sees a part of the picture, the weights are the whole picture's)"; return false; }
  if (cfg.weightp && cfg.lossless) { if (error) *error = "weightp is not available with lossless"; return false; }
  if (cfg.scenecut < 0 || cfg.scenecut > 255) { if (error) *error = "scenecut must be 0 .. 255"; return false; }
  if (cfg.scenecut && cfg.band_rows > 0) { if (error) *error = "scenecut is not available in band mode (a band's encoder sees a part of the picture, the verdict is the whole picture's)"; return false; }
  if (cfg.input_format != KVZ_INPUT_I420) {                // "input-format" 
    const char *why = nullptr;
    if (cfg.input_format != KVZ_INPUT_RGB32 && cfg.input_format != KVZ_INPUT_RGB32_SSE41 && cfg.input_format != KVZ_INPUT_YUYV) why = "input-format must be i420, rgb32, rgb32-sse41 or yuyv";
    else if (cfg.input_hold) why = "input-format other than i420 is not available with input-hold (held pictures are I420)";
    else if (cfg.band_rows > 0) why = "input-format other than i420 is not available in band mode";
    else if (cfg.input_format != KVZ_INPUT_YUYV && (cfg.width & 3)) why = "input-format rgb32 / rgb32-sse41 needs a width that is a multiple of 4";
    if (why) { if (error) *error = why; return false; }
  }
  if (cfg.intra_refresh) {                                 // "uvgx intra refresh v1" ("not covered")
    const char *why = nullptr;
    if (cfg.intra_refresh < 2 || cfg.intra_refresh > 255) why = "intra-refresh must be 0 or 2 .. 255";
    else if (cfg.lp_refs >= 2) why = "intra-refresh is not available with lp-refs >= 2 (a clean block may refer to the previous picture only)";
    else if (cfg.lp_gop) why = "intra-refresh is not available with lp-gop";
    else if (cfg.tmvp) why = "intra-refresh is not available with tmvp (a temporal candidate is read from a picture the decoder may have concealed)";
    else if (cfg.me_coarse) why = "intra-refresh is not available with me-coarse";
    else if (cfg.tile_rows != 1 || cfg.tile_cols != 1) why = "intra-refresh is not available with tiles";
    else if (cfg.band_rows > 0) why = "intra-refresh is not available in band mode";
    else if (cfg.lossless) why = "intra-refresh is not available with lossless";
    else if (!cfg.intra_chain) why = "intra-refresh is not available with intra-chain=0";
    if (why) { if (error) *error = why; return false; }
    // intra-in-p = 0: the working sets and launches of intra-in-P are brought up for the band alone (16x16 units, as at level 1); outside it nothing is priced
    ir_free_ = cfg.intra_in_p != 0;
    if (!cfg.intra_in_p) cfg.intra_in_p = 1;
  }
  if (cfg.loss_feedback) {                                 // "uvgx loss feedback v1" ("refused")
    const char *why = nullptr;
    if (cfg.loss_feedback < 0 || cfg.loss_feedback > 64) why = "loss-feedback must be 0 .. 64";
    else if (cfg.lp_refs >= 2) why = "loss-feedback is not available with lp-refs >= 2 (the map follows one reference)";
    else if (cfg.lp_gop) why = "loss-feedback is not available with lp-gop";
    else if (cfg.tmvp) why = "loss-feedback is not available with tmvp (a temporal candidate is read from a picture the decoder may have got wrong)";
    else if (cfg.me_coarse) why = "loss-feedback is not available with me-coarse";
    else if (cfg.tile_rows != 1 || cfg.tile_cols != 1) why = "loss-feedback is not available with tiles";
    else if (cfg.band_rows > 0) why = "loss-feedback is not available in band mode";
    else if (cfg.lossless) why = "loss-feedback is not available with lossless";
    else if (!cfg.intra_chain) why = "loss-feedback is not available with intra-chain=0";
    else if (cfg.intra_refresh) why = "loss-feedback is not available with intra-refresh (both own the forced quarters)";
    if (why) { if (error) { *error = why; if (cfg.fb_anchor) *error += "; fb-anchor rests on loss-feedback"; } return false; }
  }
  if (cfg.fb_anchor) {                                     // "uvgx loss feedback v2" ("refused"; what loss-feedback refuses is refused above)
    const char *why = nullptr;
    const EncLayout sz(cfg.width, cfg.height, 0);
    if (cfg.fb_anchor < 2 || cfg.fb_anchor > kMaxRefDist) why = "fb-anchor must be 0 or 2 .. 7";
    else if (!cfg.loss_feedback) why = "fb-anchor needs loss-feedback (the anchor answers a loss report)";
    else if (cfg.fb_anchor > cfg.loss_feedback) why = "fb-anchor must not exceed loss-feedback (a report the anchor answers lies within the ring of records)";
    else if (cfg.fb_anchor + 1 > fb_anchor_max_dpb(sz.cw, sz.ch)) why = "fb-anchor: the kept pictures and the current one exceed MaxDpbSize of the coded size at its level (1920x1088, 3840x2176: at most 5)";
    else if (cfg.weightp) why = "fb-anchor is not available with weightp";
    if (why) { if (error) *error = why; return false; }
  }

  const char *prio = getenv("KVAZZUP_AMD_PRIO"); if (!prio || strlen(prio) < 4) prio = "hnnn";   // main, tokenizer, input, decoder: the chain the next picture waits for is the urgent one (+6 % at 1080p; any explicit priority also gives the stream a hardware queue of its own)

  if (cfg.width < 16 || cfg.height < 16 || (cfg.width & 1) || (cfg.height & 1) || cfg.width > 16384 || cfg.height > 16384) {
    if (error) *error = "unsupported picture size"; return false;
  }
  if (cfg.qp < 0 || cfg.qp > 51 || cfg.me_range < 1 || cfg.me_range > 32) { if (error) *error = "qp or me-range out of range"; return false; }
  if (cfg.tile_cols < 1) cfg.tile_cols = 1;
  if (cfg.tile_rows < 1 || cfg.tile_rows > (cfg.height + 63) / 64 || cfg.tile_rows > 22 || cfg.tile_cols > 20 || cfg.tile_cols > (cfg.width + 63) / 64 || (cfg.band_rows > 0 && cfg.tile_cols > 1)) {
    if (error) *error = "tile grid out of range (at most 20 x 22 tiles, none smaller than a CTU; band mode: full-width tile rows)"; return false;
  }
  if (cfg.tile_cols > 1) cfg.entropy_gpu = 0;                // (k_cabac_rows runs full-width substreams)
  if (cfg.band_rows > 0) {
    const int hc = (cfg.height + 63) / 64, T = cfg.tile_rows;
    const bool ok = cfg.band_row0 >= 0 && cfg.band_row0 + cfg.band_rows <= hc && tile_row_starts_at(hc, T, cfg.band_row0) &&
                    tile_row_ends_at(hc, T, cfg.band_row0 + cfg.band_rows - 1) && !cfg.sao && cfg.vaq == 0;
    if (!ok) { if (error) *error = "a band must consist of whole tile rows (and SAO and VAQ are not available in band mode)"; return false; }
  }
  if (cfg.band_rows > 0) cfg.entropy_gpu = 0;               // (band mode hands its substreams to the caller from the host pool)
  if (cfg.band_rows > 0) cfg.hash = 0;                      // (a band encoder holds a part of the picture only)
  cfg_ = cfg;
  qp_cur_ = cfg.qp;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg.device) {
    if (error) *error = "no usable HIP device (this library has no CPU fallback)"; return false;
  }
  HIP_OK(hipSetDevice(cfg.device));
  lay_ = EncLayout(cfg.width, cfg.height, cfg.band_rows); const EncLayout &L = lay_;
  cw_ = L.cw; ch_ = L.ch; rows_ = L.rows;
  // pictures in flight behind the one being submitted (output lag).  Rate control books picture t - 3 before picture t: lag <= 2.  Beyond
  // 3 the gain is buffering: while an intra picture's chain holds the main stream (1.6 ms at 1080p, ten picture intervals) the coder threads
  // work off the pictures queued before it (1080p, host-bound: owf 3 -> 4 measured +4 %; more changes nothing).  The GPU arithmetic coder
  // is a longer stage than the host pool (a substream is one serial chain) and profits from up to 8.
  // With a bitrate the controller books picture t - rc_delay_ before picture t, rc_delay_ = pictures in flight + 1 (3 .. 7: the size ring holds eight):
  // a pipelined encoder then decides exactly like a synchronous one with the same delay (oracle/hevc_enc.c rate_control, "rc-delay").
  depth_ = cfg.owf >= 3 ? (cfg.bitrate == 0 ? (cfg.owf > kMaxDepth ? kMaxDepth : cfg.owf) : (cfg.owf > 6 ? 6 : cfg.owf)) : (cfg.owf >= 2 ? 2 : (cfg.owf == 1 ? 1 : 0));
  rc_delay_ = cfg.bitrate > 0 && depth_ + 1 > 3 && cfg.band_rows == 0 ? depth_ + 1 : 3;
  // the picture being written, the lp_refs pictures before it, and the depth_ pictures in flight in front of it -- none of whose references may be
  // overwritten (the oldest, t - depth_, reads t - depth_ - lp_refs); + 1 (at least): an intra picture is written ahead of its turn, beside the P pictures
  // in front of it, which still read theirs
  // (lp-gop with several references: a key picture stays a reference for up to kMaxRefDist pictures)
  // (fb-anchor K: the K pictures behind the current one stay, as every decoder keeps them)
  const int keep = cfg.fb_anchor ? cfg.fb_anchor : (cfg.lp_gop && cfg.gop_g > 1 && cfg.lp_refs > 1 ? kMaxRefDist : cfg.lp_refs);
  nrec_ = depth_ + 1 + keep < 2 + keep ? 2 + keep : depth_ + 1 + keep;
  prio_[0] = prio[0]; prio_[1] = prio[1]; prio_[2] = prio[2];
  HIP_OK(stream_acquire(&stream_, cfg.device, 'M', prio_[0]));
  for (int c = 0; c < 3; c++) {
    for (int k = 0; k < kSets; k++) HIP_OK(mem_.dev(&src_[k][c], L.plane(c)));
    for (int b = 0; b < nrec_; b++) HIP_OK(mem_.dev(&rec_[b][c], L.plane(c), true));
    for (int k = 0; k < kSets; k++) HIP_OK(mem_.dev(&coef_[k][c], L.plane(c), true));
  }
  for (int k = 0; k < kSets; k++) {
    HIP_OK(mem_.dev(&cu_bytes_[k], L.cu_bytes, true));
    HIP_OK(mem_.dev(&cu_mv_[k], L.cu_mv, true)); HIP_OK(mem_.dev(&cu_mvd_[k], L.cu_mv, true));
    if (cfg.lp_refs > 1 || cfg.fb_anchor) HIP_OK(mem_.dev(&cu_ref_[k], L.nb8, true));      // (fb-anchor: a v2 heal picture's frame alone points at it)
    if (cfg.tmvp) HIP_OK(mem_.dev(&col_[k], L.col, true));
    if (cfg.me_coarse || cfg.scenecut) HIP_OK(mem_.dev(&mc_q_[k], L.mc_q, true));
    if (cfg.scenecut) HIP_OK(mem_.dev(&sc_sum_[k], 1, true));
    if (cfg.me_coarse) HIP_OK(mem_.dev(&mc_centres_[k], L.mc_centres, true));
    if (cfg.weightp) { HIP_OK(mem_.dev(&wp_partial_[k], (size_t)wp_stat_blocks(cfg.height) * 2)); HIP_OK(mem_.dev(&wp_stat_[k], 2, true)); HIP_OK(mem_.dev(&wp_rec_[k], 3 * KVZ_MAX_LP_REFS, true)); }
    HIP_OK(mem_.event(&ev_tok_done_[k], kDeviceEvent));
  }
  if (cfg.weightp) {
    HIP_OK(mem_.dev(&wp_cand_, 3 * KVZ_MAX_LP_REFS)); HIP_OK(mem_.dev(&wp_acc_, 2 * KVZ_MAX_LP_REFS));
    for (int r = 0; r < cfg.lp_refs; r++) HIP_OK(mem_.dev(&wp_plane_[r], L.npx));
  }
  if (cfg.scenecut) {
    HIP_OK(mem_.dev(&sc_blocks_, L.sc_blocks, true)); HIP_OK(mem_.dev(&sc_count_, 1, true)); HIP_OK(mem_.dev(&sc_rec_, 5, true));
    HIP_OK(mem_.event(&ev_sc_, hipEventDisableTiming));      // (the host reads what k_sc_decide wrote into host-mapped memory: an event with its system fence)
  }
  if (cfg.qp_in_cu) {
    for (int k = 0; k < kSets; k++) {
      HIP_OK(mem_.dev(&ctu_qt_[k], L.nctu)); HIP_OK(mem_.dev(&ctu_qy_[k], L.nctu)); HIP_OK(mem_.dev(&ctu_delta_[k], L.nctu)); HIP_OK(mem_.dev(&ctu_first_[k], L.nctu));
      HIP_OK(mem_.pinned(&h_ctu_qt_[k], L.nctu, hipHostMallocDefault)); HIP_OK(mem_.dev(&ctu_roi_[k], L.nctu));
    }
    if (cfg.vaq > 0) { HIP_OK(mem_.dev(&vaq_act_, L.nctu)); HIP_OK(mem_.dev(&vaq_sum_, 1)); }
  }
  if (cfg.sao) for (int k = 0; k < kSets; k++) HIP_OK(mem_.dev(&sao_[k], L.nctu));
  if (cfg.rc_bands > 0) HIP_OK(mem_.dev(&rc_state_, 1, true));
  HIP_OK(stream_acquire(&stream_tok_, cfg.device, 'T', prio_[1]));
  HIP_OK(stream_acquire(&stream_in_, cfg.device, 'I', prio_[2]));
  for (int k = 0; k < kSets; k++) HIP_OK(mem_.event(&ev_src_free_[k], kDeviceEvent));
  HIP_OK(mem_.event(&ev_signalled_, kDeviceEvent));
  // the intra pictures' own stream: where the chain shares nothing with the P pictures' kernels (no SAO work picture, no intra units in P pictures
  // -- they use the same progress counters --, no per-CTU QP upload, no row groups) and pictures are queued ahead at all
  // (round 4: SAO, intra units in P pictures, per-CTU QPs and the row groups of rate control v2 no longer keep it on the main stream -- the side chain has its own
  // progress counters, edge columns and SAO work picture; VAQ still does: its activity scratch is shared)
  // (not when every picture is an intra picture: then the chains ARE the main stream's work, and the next picture's analysis belongs beside them on the
  // input stream, not behind them -- all-intra 1080p 940 -> 1 300 frames/s)
  idr_side_ = depth_ >= 2 && cfg.vaq == 0 && cfg.band_rows == 0 && cfg.intra_period != 1;
  // Every picture an intra picture (BASELINE configs[0]): no picture depends on another, and one chain keeps a few dozen compute units busy for 0.7 ms --
  // the pictures ALTERNATE between the main stream with its arrays and a second stream with the side chain's (round 5: all-intra 1080p was bound by
  // one chain after the other, 1 / (0.67 + 0.03 ms)).  The second stream is one of its own here: the input stream carries every picture's analysis.
  all_intra_alt_ = depth_ >= 2 && cfg.vaq == 0 && cfg.band_rows == 0 && cfg.intra_period == 1;
  if (!build_chain(chain_, error)) return false;
  if (idr_side_ || all_intra_alt_) {
    if (!build_chain(chain_idr_, error)) return false;
    // ... which is the INPUT stream: the pictures behind an intra picture need it anyway, so their input stages lose nothing by queueing behind
    // its chain, and a further stream would share a hardware queue with one that matters (HIP spreads a priority level's streams over four;
    // measured with a stream of its own: no gain at the default level, half the rate at any other)
    if (all_intra_alt_) HIP_OK(stream_acquire(&stream_idr_, cfg.device, 'X', prio_[0])); else stream_idr_ = stream_in_;
    HIP_OK(mem_.event(&ev_idr_done_, kDeviceEvent));
  }
  HIP_OK(mem_.dev(&intra_scratch_, L.intra_scratch));
  HIP_OK(mem_.dev(&tok_buf_, L.tok_buf)); HIP_OK(mem_.dev(&tok_count_, L.tok_count, true));
  HIP_OK(mem_.dev(&tok_seg_, L.tok_seg, true));            // (all "no tokens": the list form of k_tokenize writes only the entries that have some; k_tok_compact zeroes behind itself)
  if (cfg.band_rows == 0) HIP_OK(mem_.dev(&tok_list_, L.tok_list, true));      // (unit, role) pairs with something to say, P pictures (hevc_core.h EncFrame::tok_list)
  spin_wait_ = getenv("KVAZZUP_AMD_SPIN") != nullptr;
  nslots_ = depth_ + 1;
  for (int i = 0; i < nslots_; i++) {
    Slot &sl = slot_[i];
    if (cfg.entropy_gpu) {
      HIP_OK(mem_.dev(&sl.g_tok, L.tok_dense_cap)); HIP_OK(mem_.dev(&sl.g_count, L.nctu)); HIP_OK(mem_.dev(&sl.g_off, L.nctu));
      sl.d_tok_dense = sl.g_tok; sl.d_tok_count = sl.g_count; sl.d_tok_off = sl.g_off;
      HIP_OK(mem_.dev(&sl.g_stage, L.stage_cap));
      HIP_OK(mem_.dev(&sl.g_cursors, 2, true)); HIP_OK(mem_.dev(&sl.g_ctx_save, L.ctx_save)); HIP_OK(mem_.dev(&sl.g_ctx_ready, (size_t)rows_, true));
      HIP_OK(mem_.pinned(&sl.h_out, L.out_cap, hipHostMallocMapped, &sl.d_out)); HIP_OK(mem_.pinned(&sl.h_sub, L.sub, hipHostMallocMapped, &sl.d_sub));
      HIP_OK(stream_acquire(&sl.ent_stream, cfg.device, 'E', 'l'));           // (streams of one priority level share that level's hardware queues: the long coder kernels get the lowest level to themselves)
      HIP_OK(mem_.event(&sl.tok_ev, hipEventDisableTiming));
    } else {
      HIP_OK(mem_.pinned(&sl.h_tok_dense, L.tok_dense_cap, hipHostMallocMapped, &sl.d_tok_dense));
      HIP_OK(mem_.pinned(&sl.h_tok_count, L.nctu, hipHostMallocMapped, &sl.d_tok_count)); HIP_OK(mem_.pinned(&sl.h_tok_off, L.nctu, hipHostMallocMapped, &sl.d_tok_off));
    }
    HIP_OK(mem_.pinned(&sl.h_err, 1, hipHostMallocMapped, &sl.d_err)); *sl.h_err = 0;
    if (cfg.weightp) {
      HIP_OK(mem_.pinned(&sl.h_wp, 3 * KVZ_MAX_LP_REFS, hipHostMallocMapped, &sl.d_wp));
      for (int r = 0; r < KVZ_MAX_LP_REFS; r++) { sl.h_wp[3 * r] = 0; sl.h_wp[3 * r + 1] = 64; sl.h_wp[3 * r + 2] = 0; }
    }
    if (cfg.loss_feedback) {
      const int nfb = cfg.fb_anchor ? 8 : 4;
      HIP_OK(mem_.pinned(&sl.h_fb, nfb, hipHostMallocMapped, &sl.d_fb));
      for (int i = 0; i < nfb; i++) sl.h_fb[i] = 0;
    }
    if (cfg.scenecut) {
      HIP_OK(mem_.pinned(&sl.h_sc, 5, hipHostMallocMapped, &sl.d_sc));
      for (int i = 0; i < 5; i++) sl.h_sc[i] = 0;
    }
    HIP_OK(mem_.event(&sl.done, hipEventDisableTiming)); HIP_OK(mem_.event(&sl.rec_done, hipEventDisableTiming));
  }
  HIP_OK(mem_.event(&in_done_, kDeviceEvent));
  if (cfg.intra_in_p || cfg.loss_feedback) HIP_OK(mem_.dev(&me_cost16_, L.me_block, true));      // k_me's inter cost per 16x16 block (intra-in-P; loss-feedback with intra-in-p=0: the heal pictures')
  if (cfg.loss_feedback) {                                 // (encoder.h fb_rec_mv_)
    HIP_OK(mem_.dev(&fb_rec_mv_, (size_t)cfg.loss_feedback * L.nb8 * 2, true)); HIP_OK(mem_.dev(&fb_rec_info_, (size_t)cfg.loss_feedback * L.nb8, true));
    HIP_OK(mem_.event(&ev_fb_me_, kDeviceEvent));
    if (cfg.fb_anchor) fb_rec_anchor_.assign((size_t)cfg.loss_feedback, -1);
    HIP_OK(mem_.dev(&fb_map_, L.nb8, true)); HIP_OK(mem_.dev(&fb_tmp_, L.nb8, true)); HIP_OK(mem_.dev(&fb_blk_, L.nb8 / 16 * 2, true));
  }
  me_ahead_ = cfg.me_source != 0;
  if (me_ahead_ && cfg.intra_in_p)                         // (encoder.h me_block_: one block of these and one array of progress counters per working set)
    for (int k = 0; k < kSets; k++) { HIP_OK(mem_.dev(&me_block_[k], L.me_block, true)); HIP_OK(mem_.dev(&sync_set_[k], L.sync, true)); }
  {
    // dispatch order of the intra reconstruction's workgroups: the CTUs of the rows this instance codes, by anti-diagonal cx + 2 cy
    const int wc = cw_ / 64, r0 = cfg.band_rows > 0 ? cfg.band_row0 : 0, nr = cfg.band_rows > 0 ? cfg.band_rows : rows_;
    std::vector<uint32_t> order;
    for (int d = 0; d < wc + 2 * nr; d++) for (int cy = 0; cy < nr; cy++) { const int cx = d - 2 * cy; if (cx >= 0 && cx < wc) order.push_back((uint32_t)((r0 + cy) * wc + cx)); }
    HIP_OK(mem_.dev(&intra_order_, L.intra_order));
    HIP_OK(hipMemcpy(intra_order_, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice));
  }
  HIP_OK(mem_.dev(&err_, 1, true));
  if (getenv("KVAZZUP_AMD_INTRA_TRACE")) HIP_OK(mem_.dev(&trace_, L.trace, true));
  int eth = cfg.entropy_threads;
  if (const char *e = getenv("KVAZZUP_AMD_ENTROPY_THREADS")) eth = atoi(e) < 1 ? 1 : atoi(e);     // tuning knob (containers with a small CPU quota)
  if (cfg.entropy_gpu) { entropy_ = nullptr; entropy2_ = nullptr; }
  else if (cfg.owf >= 2 && eth >= 4) {                        // two pictures side by side, half the threads each
    entropy_ = new EntropyHost((eth + 1) / 2 < rows_ ? (eth + 1) / 2 : rows_);
    entropy2_ = new EntropyHost(eth / 2 < rows_ ? eth / 2 : rows_);
  } else entropy_ = new EntropyHost(eth < rows_ ? eth : rows_);

  if (cfg.scaling_list) {                                 // `scaling-list default`: the default lists' factors, once
    uint8_t tab[KVZ_SCALING_BYTES];
    scaling_factors(scaling_defaults(), tab);
    HIP_OK(mem_.dev(&d_scaling_, KVZ_SCALING_BYTES)); HIP_OK(hipMemcpy(d_scaling_, tab, KVZ_SCALING_BYTES, hipMemcpyHostToDevice));
  }
  // what every picture's frame starts from (picture_frame)
  EncFrame &b = base_;
  b.cw = cw_; b.ch = ch_; b.b8w = cw_ / 8; b.b8h = ch_ / 8;
  b.tile_rows = cfg.tile_rows; b.tile_cols = cfg.tile_cols; b.chp = pack_height(ch_, cfg.tile_rows, cfg.tile_cols);
  b.row0 = cfg.band_rows > 0 ? cfg.band_row0 : 0; b.nrows = cfg.band_rows > 0 ? cfg.band_rows : 0;
  b.range = cfg.me_range; b.scaling = d_scaling_; b.intra_chain = cfg.intra_chain;
  b.lossless = cfg.lossless; b.rdoq = cfg.rdoq; b.signhide = cfg.signhide; b.intra_p = cfg.intra_in_p;
  if (cfg.intra_in_p) point_me_block(b, L, me_cost16_);      // (loss-feedback with intra-in-p=0: a heal picture's frame alone points at it)
  b.wpp = cfg.wpp; b.mv_frame = cfg.mv_frame; b.me_early = cfg.me_early; b.satd = cfg.satd; b.subme = cfg.subme; b.slices = cfg.slices;
  uint8_t *p = intra_scratch_;
  b.ic8 = (uint32_t *)p; b.ic16 = (uint32_t *)(p + L.ic16_off); b.ic32 = (uint32_t *)(p + L.ic32_off); b.im8 = p + L.im8_off; b.im16 = p + L.im16_off; b.im32 = p + L.im32_off;
  b.tok_buf = tok_buf_; b.tok_cap = L.tok_cap; b.tok_seg = tok_seg_; b.tok_list = tok_list_; b.tok_dense_cap = (uint32_t)L.tok_dense_cap;
  point_chain(b, L, chain_);
  b.err = err_; b.trace = trace_; b.intra_order = intra_order_;
  // (a synchronous encoder: the cap that keeps the search from holding every wave slot protects nobody -- 185 -> 142 us of an intra picture's encoding delay
  // at 1080p; band mode keeps the cap)
  b.analyse_alone = depth_ < 2 && cfg.band_rows == 0 ? 1 : 0;
  // (two pictures' chains side by side: two anti-diagonals of workgroups each -- all-intra 2 030 -> 2 110 frames/s; a lone chain is 2.5 % slower with two,
  // 670 -> 687 us: profiles/r05_intra_diags.txt)
  b.chain_diags = all_intra_alt_ ? 2 : 0;

  sp_.cw = cw_; sp_.ch = ch_; sp_.width = cfg.width; sp_.height = cfg.height; sp_.qp = cfg.qp; sp_.wpp = cfg.wpp; sp_.tile_rows = cfg.tile_rows; sp_.tile_cols = cfg.tile_cols; sp_.qp_in_cu = cfg.qp_in_cu; sp_.sao = cfg.sao; sp_.slices = cfg.slices; sp_.signhide = cfg.signhide; sp_.scaling_list = cfg.scaling_list; sp_.tq_bypass = cfg.lossless;
  sp_.lp_refs = cfg.lp_refs > 1 ? cfg.lp_refs : 0;
  sp_.tmvp = cfg.tmvp;
  sp_.weightp = cfg.weightp;
  sp_.fb_anchor = cfg.fb_anchor;
  sp_.deblock = cfg.deblock; sp_.fps_num = cfg.fps_num; sp_.fps_den = cfg.fps_den;
  HIP_OK(hipStreamSynchronize(stream_));
  HIP_OK(hipDeviceSynchronize());
  tok_deferred_ = depth_ >= 2 && cfg.sao && !cfg.entropy_gpu && cfg.band_rows == 0 && cfg.owf <= kSets - 1;
  HIP_OK(hipDeviceSynchronize());                        // (every clear above ran on the null stream: done before anything is queued on the encoder's non-blocking streams)
  if (tok_deferred_) tok_thread_ = std::thread([this] { name_this_thread("kvzx-enc-tok"); tok_launcher(); });
  if (depth_ >= 2) { bg_[0] = std::thread([this] { name_this_thread("kvzx-enc-bg0"); background(0); }); if (entropy2_) bg_[1] = std::thread([this] { name_this_thread("kvzx-enc-bg1"); background(1); }); }
  if (depth_ >= 2 && cfg.band_rows == 0) sub_thread_ = std::thread([this] { name_this_thread("kvzx-enc-sub"); submitter(); });
  return true;
}

namespace { struct Tick { std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } }; }

Encoder::~Encoder()
{
  if (getenv("KVAZZUP_AMD_TRACE")) fprintf(stderr, "kvazzup_amd encoder thread ms: submit %.1f  wait_gpu %.1f  arith %.1f  assemble %.1f  wait_input %.1f  (pictures %ld)\n", t_submit_, t_wait_, t_arith_, t_asm_, t_in_, collected_);
  auto stop = [](std::mutex &m, bool &quit, std::condition_variable &cv) { { std::lock_guard<std::mutex> l(m); quit = true; } cv.notify_all(); };
  stop(sm_, squit_, scv_); if (sub_thread_.joinable()) sub_thread_.join();
  stop(tm_, tquit_, tcv_); if (tok_thread_.joinable()) tok_thread_.join();           // (what it still had queued has gone to the workers)
  stop(bm_, bquit_, bcv_); for (auto &t : bg_) if (t.joinable()) t.join();
  for (hipStream_t st : {stream_, stream_idr_ != stream_in_ ? stream_idr_ : nullptr, stream_tok_, stream_in_}) if (st) hipStreamSynchronize(st);
  for (Slot &sl : slot_) { if (sl.ent_stream) hipStreamSynchronize(sl.ent_stream); if (sl.sink_done) hipEventSynchronize(sl.sink_done); }      // (the coders' streams; the copies into the caller's pictures)
  mem_.release();
  delete entropy_; delete entropy2_;
  for (Slot &sl : slot_) stream_release(sl.ent_stream, cfg_.device, 'E', 'l');
  stream_release(stream_rec_, cfg_.device, 'R', 'n');
  stream_release(stream_tok_, cfg_.device, 'T', prio_[1]);
  stream_release(stream_in_, cfg_.device, 'I', prio_[2]);
  if (stream_idr_ && stream_idr_ != stream_in_) stream_release(stream_idr_, cfg_.device, 'X', prio_[0]);
  stream_release(stream_, cfg_.device, 'M', prio_[0]);
}

void Encoder::timed(KernelId id, hipStream_t st, const std::function<void()> &launch) { timed_slot(*cur_slot_, prof_now_, id, st, launch); }
void Encoder::timed_slot(Slot &sl, bool prof, KernelId id, hipStream_t st, const std::function<void()> &launch)
{
  if (!prof) { launch(); return; }
  if (sl.ev_used == sl.ev.size()) {
    EvPair p; mem_.event(&p.a, hipEventDefault); mem_.event(&p.b, hipEventDefault); p.id = id; sl.ev.push_back(p);
  }
  EvPair &p = sl.ev[sl.ev_used++]; p.id = id;
  hipEventRecord(p.a, st);
  launch();
  hipEventRecord(p.b, st);
}

void Encoder::get_kernel_times(double *ms, uint64_t *launches, bool reset)
{
  std::lock_guard<std::mutex> l(stat_m_);
  for (int i = 0; i < K_COUNT; i++) { if (ms) ms[i] = k_ms_[i]; if (launches) launches[i] = k_n_[i]; }
  if (reset) for (int i = 0; i < K_COUNT; i++) { k_ms_[i] = 0; k_n_[i] = 0; }
}

// encode = submit the picture's kernels, then finish ("collect") the oldest picture in flight.  With
// owf == 0 that is the picture just submitted; with owf >= 1 it is the previous one, whose arithmetic
// coding on the host then runs while the GPU works on the new picture.
// Host picture in: the copy engine moves it into device buffer k = t mod kInRing on the input stream while earlier pictures' kernels
// run; the input stage of picture t (stream_in_) follows that copy.  The ring is longer than the pictures that can be in flight, so the
// buffer's previous reader (the input stage of picture t - kInRing) has long finished and the copy command carries no dependency: the copy
// engine takes it at once.  (A copy waiting inside the engine's queue holds up every copy behind it, the decoder's included; the input
// kernel reading the host picture itself across PCIe -- tried -- slows the kernels running beside it 2-10x, tools/measure/pcie_copy_vs_kernels.hip.)
// Nothing here waits on the calling thread except a staging buffer coming free (callers without page-locked planes).
bool Encoder::upload_and_submit(const uint8_t *y, const uint8_t *u, const uint8_t *v, bool pinned)
{
  const size_t ny = (size_t)cfg_.width * cfg_.height, bytes = input_bytes();
  const bool packed = cfg_.input_format != KVZ_INPUT_I420;
  const int k = (int)(in_count_++ % kInRing);
  // The copy rides on the input stream itself, ahead of the picture's input kernel.  HIP spreads the streams of one priority level over four
  // hardware queues, and at the default level those are taken (tokenizer, input, decoder, decoder transfers): a fifth stream there shares a
  // queue with one of them and is serialised behind that stream's event waits (measured: the input stream behind the tokenizer's, 3700 instead
  // of 5200 frames/s at 1080p); a stream at the lowest level has a queue to itself and measured no better for the encoder alone, worse with
  // the decoder beside it.
  if (!d_in_[k]) {
    HIP_CHECK(mem_.dev(&d_in_[k], bytes));
    HIP_CHECK(mem_.event(&ev_h2d_[k], hipEventDisableTiming)); HIP_CHECK(mem_.event(&ev_pad_[k], hipEventDisableTiming));
  }
  const uint8_t *src = y;
  if (!pinned) {
    if (!h_in_[k]) HIP_CHECK(mem_.pinned(&h_in_[k], bytes, hipHostMallocDefault));
    if (h2d_pending_[k]) { Tick tk; HIP_CHECK(hipEventSynchronize(ev_h2d_[k])); h2d_pending_[k] = false; t_in_ += tk.ms(); }   // the staging buffer's last upload
    if (packed) memcpy(h_in_[k], y, bytes);
    else { memcpy(h_in_[k], y, ny); memcpy(h_in_[k] + ny, u, ny / 4); memcpy(h_in_[k] + ny + ny / 4, v, ny / 4); }
    src = h_in_[k];
  }
  if (pad_pending_[k]) {                             // d_in_[k]'s last reader: done long ago, normally
    if (hipEventQuery(ev_pad_[k]) != hipSuccess) HIP_CHECK(hipStreamWaitEvent(stream_in_, ev_pad_[k], 0));
    pad_pending_[k] = false;
  }
  HIP_CHECK(hipMemcpyAsync(d_in_[k], src, bytes, hipMemcpyHostToDevice, stream_in_));
  HIP_CHECK(hipEventRecord(ev_h2d_[k], stream_in_)); h2d_pending_[k] = true;
  { Tick tk; if (!submit(d_in_[k], k)) return false; t_submit_ += tk.ms(); }
  in_pending_ = false;                               // (nobody but this ring reads d_in_[k])
  return true;
}

size_t Encoder::input_bytes() const { return kvzx::input_bytes(cfg_.input_format, cfg_.width, cfg_.height); }

bool Encoder::encode_host(const uint8_t *y, const uint8_t *u, const uint8_t *v, EncodedPicture *out, bool pinned)
{
  const size_t ny = (size_t)cfg_.width * cfg_.height;
  out->valid = false; out->au.clear();
  if (cfg_.input_format != KVZ_INPUT_I420) return false;      // (a packed encoder takes encode_packed_host)
  return host_picture(y, u, v, out, pinned && u == y + ny && v == u + ny / 4);
}

bool Encoder::encode_packed_host(const uint8_t *packed, EncodedPicture *out, bool pinned)
{
  out->valid = false; out->au.clear();
  if (cfg_.input_format == KVZ_INPUT_I420 || !packed) return false;
  return host_picture(packed, nullptr, nullptr, out, pinned);
}

bool Encoder::host_picture(const uint8_t *y, const uint8_t *u, const uint8_t *v, EncodedPicture *out, bool pinned)
{
  HIP_CHECK(hipSetDevice(cfg_.device));
  if (pinned && sub_thread_.joinable()) return enqueue(y, true, out);
  drain_submitter();
  accepted_++;
  roi_sub_ = roi_; roi_sub_w_ = roi_w_; roi_sub_h_ = roi_h_;
  for (int c = 0; c < 3; c++) { sink_sub_[c] = sink_[c]; sink_[c] = nullptr; }
  tl("up0", submitted_);
  if (!upload_and_submit(y, u, v, pinned)) { accepted_--; return false; }
  tl("sub1", submitted_ - 1);
  return pending() > depth_ ? collect(out) : true;
}

bool Encoder::encode_device(const uint8_t *d_i420, EncodedPicture *out)
{
  out->valid = false; out->au.clear();
  return cfg_.input_format == KVZ_INPUT_I420 && device_picture(d_i420, out);      // (a packed encoder takes encode_packed_device)
}

bool Encoder::encode_packed_device(const uint8_t *d_packed, EncodedPicture *out)
{
  out->valid = false; out->au.clear();
  // (the RGB32 kernels read 16 bytes at a time: rows are multiples of 16 bytes, the picture must start at one)
  if (cfg_.input_format == KVZ_INPUT_I420 || !d_packed || (cfg_.input_format != KVZ_INPUT_YUYV && (((uintptr_t)d_packed) & 15))) return false;
  return device_picture(d_packed, out);
}

bool Encoder::device_picture(const uint8_t *d_i420, EncodedPicture *out)
{
  HIP_CHECK(hipSetDevice(cfg_.device));
  if (cfg_.input_hold && sub_thread_.joinable()) return enqueue(d_i420, false, out);
  drain_submitter();
  accepted_++;
  roi_sub_ = roi_; roi_sub_w_ = roi_w_; roi_sub_h_ = roi_h_;
  { Tick tk; if (!submit(d_i420, -1)) { accepted_--; return false; } t_submit_ += tk.ms(); }
  bool ok = true;
  if (pending() > depth_) ok = collect(out);
  // the caller may reuse its input buffer when this returns (the pad kernel is first in the picture's queue,
  // and by now it has had the whole host coding stage of the previous picture to run)
  if (in_pending_) { Tick tk; HIP_CHECK(hipEventSynchronize(in_done_)); in_pending_ = false; t_in_ += tk.ms(); }
  return ok;
}

// owf >= 2: hand the picture to the submitter thread, then finish the oldest picture in flight if the pipeline is full
bool Encoder::enqueue(const uint8_t *src, bool host, EncodedPicture *out)
{
  tl("enq", accepted_);
  SubmitJob j; j.src = src; j.host = host; j.roi = roi_; j.roi_w = roi_w_; j.roi_h = roi_h_; j.slot = (int)(accepted_ % nslots_);
  for (int c = 0; c < 3; c++) { j.sink[c] = sink_[c]; sink_[c] = nullptr; }
  { std::lock_guard<std::mutex> l(bm_); slot_[j.slot].ready = false; slot_[j.slot].ok = true; }
  accepted_++;
  { std::lock_guard<std::mutex> l(sm_); sq_.push_back(std::move(j)); }
  scv_.notify_one();
  return pending() > depth_ ? collect(out) : true;
}

void Encoder::submitter()
{
  hipSetDevice(cfg_.device);
  for (;;) {
    SubmitJob j;
    {
      std::unique_lock<std::mutex> l(sm_);
      sbusy_ = false; scv_.notify_all();
      scv_.wait(l, [&] { return squit_ || !sq_.empty(); });
      if (squit_ || sq_.empty()) return;               // (closing: what is still queued reads caller pictures that may be gone -- it is dropped, nobody collects it)
      j = std::move(sq_.front()); sq_.pop_front(); sbusy_ = true;
    }
    const long before = submitted_;
    roi_sub_.swap(j.roi); roi_sub_w_ = j.roi_w; roi_sub_h_ = j.roi_h;
    for (int c = 0; c < 3; c++) sink_sub_[c] = j.sink[c];
    tl("sub0", submitted_);
    const size_t ny = (size_t)cfg_.width * cfg_.height;
    bool ok;
    if (j.host) ok = upload_and_submit(j.src, j.src + ny, j.src + ny + ny / 4, true);
    else { Tick tk; ok = submit(j.src, -1); t_submit_ += tk.ms(); in_pending_ = false; }
    tl("sub1", submitted_ - 1);
    if (!ok) {                                       // nothing was queued for this picture: its slot reports the failure
      if (submitted_ == before) submitted_++;        // (the slots are numbered by pictures accepted: a picture that failed still took its turn)
      { std::lock_guard<std::mutex> l(bm_); slot_[j.slot].ok = false; slot_[j.slot].ready = true; }
      bcv_.notify_all();
    }
  }
}

// a synchronous call after asynchronous ones: everything handed over so far has been queued on the GPU
void Encoder::drain_submitter()
{
  if (!sub_thread_.joinable()) return;
  std::unique_lock<std::mutex> l(sm_);
  scv_.wait(l, [&] { return sq_.empty() && !sbusy_; });
}

bool Encoder::flush(EncodedPicture *out)
{
  out->valid = false; out->au.clear();
  if (!pending()) return true;
  HIP_CHECK(hipSetDevice(cfg_.device));
  return collect(out);
}

bool Encoder::poll(EncodedPicture *out)
{
  out->valid = false; out->au.clear();
  if (!pending()) return true;
  Slot &sl = slot_[collected_ % nslots_];
  if (depth_ >= 2) { std::lock_guard<std::mutex> l(bm_); if (!sl.ready) return true; }
  else {
    HIP_CHECK(hipSetDevice(cfg_.device));
    if (sub_thread_.joinable()) drain_submitter();
    if (hipEventQuery(sl.done) != hipSuccess || hipEventQuery(sl.rec_done) != hipSuccess) return true;
  }
  return collect(out);
}

void Encoder::set_roi(int w, int h, const int8_t *map)
{
  roi_.clear(); roi_w_ = roi_h_ = 0;
  if (w > 0 && h > 0 && map) { roi_.assign(map, map + (size_t)w * h); roi_w_ = w; roi_h_ = h; }
}

// target QP of every CTU of the picture being submitted (set set_): host map -> pinned -> device, on stream_
// Per-CTU quantiser targets (cu_qp_delta): target = clip(picture QP + ROI delta), with VAQ the device adds its own delta.  The ROI deltas of the picture's map
// (kvz_picture.roi, spread over the CTU grid here) go up on `st` -- the INPUT stream, ahead of the event the main stream waits for anyway -- and only when
// the picture brings a map; the targets themselves are written by the kernel at the head of the picture's chain (k_picture_begin).  Nothing is copied on
// the main stream: a 510-byte copy there cost every picture of uvgComm's default mode a ~28 us bubble.
bool Encoder::stage_roi(hipStream_t st)
{
  roi_dev_ = nullptr;
  if (!cfg_.qp_in_cu || roi_sub_.empty()) return true;
  const int wc = cw_ / 64, hc = rows_;
  int8_t *h = h_ctu_qt_[set_];
  for (int cy = 0; cy < hc; cy++) for (int cx = 0; cx < wc; cx++)
    h[cy * wc + cx] = (int8_t)clip3(-12, 12, (int)roi_sub_[(size_t)(cy * roi_sub_h_ / hc) * roi_sub_w_ + (cx * roi_sub_w_ / wc)]);
  HIP_CHECK(hipMemcpyAsync(ctu_roi_[set_], h, (size_t)wc * hc, hipMemcpyHostToDevice, st));
  roi_dev_ = ctu_roi_[set_];
  return true;
}
// generation of the picture's intra chain launch (the tag of the edge-column words, kernel_common.h IntraNeighbours): 1 .. 2^24 - 1; when the counter
// wraps, both arrays go back to "never written" on the streams that use them
uint32_t Encoder::next_chain_gen()
{
  if (++chain_gen_ >= (1u << 24)) {
    const size_t col = lay_.edge_col * sizeof(uint32_t), row = lay_.edge_row * sizeof(unsigned long long);
    hipMemsetAsync(chain_.edge_col, 0, col, stream_); hipMemsetAsync(chain_.edge_row, 0, row, stream_);
    if (chain_idr_.edge_col) { hipMemsetAsync(chain_idr_.edge_col, 0, col, stream_idr_); hipMemsetAsync(chain_idr_.edge_row, 0, row, stream_idr_); }
    chain_gen_ = 1;
  }
  return chain_gen_;
}

bool Encoder::picture_begin(const EncFrame &f, hipStream_t qt_stream, EncFrame *fold, bool zero)
{
  const bool have = frame_idx_ >= rc_delay_;
  const uint32_t bits3 = have ? 8u * rc_bytes_[(frame_idx_ - rc_delay_) & 7] : 0u;
  const int slot3 = (frame_idx_ - rc_delay_) & 7, n = (cw_ / 64) * rows_;
  int8_t *qt = cfg_.qp_in_cu ? ctu_qt_[set_] : nullptr;
  if (fold && qt_stream == stream_ && cfg_.vaq == 0) {
    fold->pb_on = (rc_state_ || qt) ? 1 : 0; fold->pb_rc = rc_state_; fold->pb_qt = qt; fold->pb_roi = roi_dev_; fold->pb_bits3 = bits3; fold->pb_nctu = n;
    fold->pb_slot3 = (int8_t)slot3; fold->pb_have3 = have ? 1 : 0;
    return true;
  }
  // (an intra picture, `zero`: the launch also takes the chain's two arrays back to zero -- the ticket counter's array with the "has intra units" word of the
  // P pictures behind it, which no P picture has pending while an intra picture starts on these arrays, and the CU cbf bits)
  void *za = zero ? (void *)f.sync : nullptr, *zb = zero ? (void *)f.cu_cbf : nullptr;
  const size_t na = zero ? sizeof(uint32_t) * lay_.sync : 0, nb = zero ? (size_t)f.b8w * f.b8h : 0;
  if (qt_stream == stream_) launch_picture_begin(rc_state_, bits3, slot3, have ? 1 : 0, qt, roi_dev_, n, f.qp, cfg_.vaq > 0 ? 1 : 0, stream_, za, na, zb, nb);
  else {
    // an intra picture on its side stream: the rate control state is updated in PICTURE ORDER on the main stream (between the P pictures' row groups, which
    // run there), the picture's own per-CTU targets on its own stream
    launch_picture_begin(rc_state_, bits3, slot3, have ? 1 : 0, nullptr, nullptr, 0, f.qp, 0, stream_);
    launch_picture_begin(nullptr, 0, 0, 0, qt, roi_dev_, n, f.qp, 0, qt_stream, za, na, zb, nb);
  }
  if (cfg_.qp_in_cu && cfg_.vaq > 0) launch_vaq(f, cfg_.vaq, vaq_act_, vaq_sum_, stream_);          // (reads f.qp, f.src and f.ctu_qt; the source is padded: stream_ waits for in_done_)
  return true;
}

// picture-level rate control: the statement of record is rate_control() in oracle/hevc_enc.c
void Encoder::rate_control()
{
  if (cfg_.bitrate <= 0 || frame_idx_ < rc_delay_) return;
  const int64_t T = ((int64_t)cfg_.bitrate * cfg_.fps_den) / (cfg_.fps_num > 0 ? cfg_.fps_num : 1);
  const int64_t trend = (int64_t)8 * rc_bytes_[(frame_idx_ - rc_delay_) & 7] - T;
  rc_debt_ += trend;
  int step = 0;
  if (rc_debt_ > 4 * T && trend > 0) step = rc_debt_ > 16 * T ? 2 : 1;
  if (rc_debt_ < -4 * T && trend < 0) step = rc_debt_ < -16 * T ? -2 : -1;
  qp_cur_ = clip3(10, 51, qp_cur_ + step);
}

// What is decided for a picture before anything is queued: its working set, intra picture or not (POC), its QP (rate control; lp-gop: + the layer), its
// references, where its chain runs
Encoder::Plan Encoder::plan(int set)
{
  Plan p;
  set_ = set;
  const int period = cfg_.intra_period;
  p.intra = (frame_idx_ == 0) || (period > 0 && (frame_idx_ % period) == 0);
  // scenecut: the period counts from the last IDR picture, wherever a cut put it (poc_ + 1 pictures back; without a cut that is the count above), and the
  // picture sc_stage found to be a cut is one
  if (cfg_.scenecut) p.intra = (frame_idx_ == 0) || (period > 0 && ((poc_ + 1) % period) == 0) || sc_cut_;
  if (p.intra) poc_ = 0; else poc_++;
  rate_control();
  // the references: the min(lp-refs, pictures since the IDR picture) pictures before this one ...
  p.qp = qp_cur_;
  p.nref = p.intra || poc_ < 1 ? 1 : (poc_ < cfg_.lp_refs ? poc_ : cfg_.lp_refs);
  if (gop_on() && !p.intra) {
    // ... or "uvgx low-delay GOP v1" (statement of record: tests/lp_gop_model.py): the QP layer -- the controller's own state is not told about the offset --, and
    // the previous picture, the most recent key picture within reach, then the pictures before the previous one; list 0 holds them by increasing distance
    const int g = cfg_.gop_g, d = cfg_.gop_d, pos = ((poc_ - 1) % g) + 1;
    int layer = 1;
    while (layer < d && pos % (layer == 1 ? g : 1 << (d - layer)) != 0) layer++;
    p.layer = layer; p.qp = clip3(0, 51, qp_cur_ + layer);
    int n = 0; int8_t set[KVZ_MAX_LP_REFS];
    set[n++] = 1;
    if (p.nref >= 2) { const int key = ((poc_ - 2) / g) * g; if (poc_ - key <= kMaxRefDist) set[n++] = (int8_t)(poc_ - key); }
    for (int back = 2; n < p.nref; back++) { bool have = false; for (int k = 0; k < n; k++) have |= set[k] == back; if (!have) set[n++] = (int8_t)back; }
    for (int k = 0; k < n; k++) { int j = k; const int8_t v = set[k]; for (; j > 0 && set[j - 1] > v; j--) set[j] = set[j - 1]; set[j] = v; }
    for (int k = 0; k < KVZ_MAX_LP_REFS; k++) p.dist[k] = k < n ? set[k] : 1;
  }
  if (cfg_.intra_refresh && !p.intra) {                     // intra-refresh: a cycle begins behind the IDR picture and again behind each cycle's last picture
    p.ir_j = ir_position(cw_, cfg_.intra_refresh, poc_);
    p.ir_s = ir_band_start(cw_, cfg_.intra_refresh, p.ir_j); p.ir_e = ir_band_end(cw_, cfg_.intra_refresh, p.ir_j);
  }
  p.ahead = me_ahead_ && !p.intra;
  if (cfg_.loss_feedback) {
    // loss-feedback: the reports made since the last picture was planned turn this P picture into their heal picture; an IDR picture heals everything and
    // voids them.  Under me-source the heal picture's search waits for the picture before it on the main stream (the map comes from that picture's record)
    // and still reads the previous input picture; no other picture changes its place
    std::lock_guard<std::mutex> l(fbm_);
    fb_heal_.clear();
    if (p.intra) { fb_q_.clear(); fb_clean_ = 0; }
    else if (!fb_q_.empty()) {
      fb_heal_.swap(fb_q_); p.fb = true; p.ahead = false;
      // fb-anchor: the picture before the oldest reported one is the anchor when it is kept and not in front of the clean point (fb_anchor_pick) -- the heal
      // picture's references are then the previous picture and the anchor; otherwise it is v1's heal picture in every decision
      if (cfg_.fb_anchor) {
        int n0 = poc_;
        for (const FbReport &r : fb_heal_) n0 = r.poc < n0 ? r.poc : n0;
        const int a = fb_anchor_pick(fb_clean_, n0, poc_, cfg_.fb_anchor, cfg_.loss_feedback);
        if (a >= 0) { p.fb_da = poc_ - a; p.nref = 2; p.dist[0] = 1; p.dist[1] = (int8_t)p.fb_da; }
      }
      fb_clean_ = poc_;
    }
  }
  // the stream this picture's chain runs on: an intra picture's own (encoder.h stream_idr_), else the main stream -- behind the last intra picture's chain
  p.side = p.intra && (idr_side_ || (all_intra_alt_ && (frame_idx_ & 1)));
  p.ms = p.side ? stream_idr_ : stream_;
  return p;
}

// The frame every kernel of the planned picture gets: base_ with the working set set_, the arrays of the chain it runs on, the set's me-source block, its
// references, the slot's outputs, and its QP, POC and tokenizer cursors.  Reads the encoder's state and changes none of it.
EncFrame Encoder::picture_frame(const Plan &p, const Slot &sl, uint32_t chain_gen) const
{
  EncFrame f = base_;
  const int k = set_;
  uint8_t *cu = cu_bytes_[k];
  for (int c = 0; c < 3; c++) { f.coef[c] = coef_[k][c]; f.src[c] = src_[k][c]; }
  f.cu_log2 = cu; f.cu_intra = cu + lay_.cu_off(1); f.cu_flags = cu + lay_.cu_off(2); f.cu_merge_idx = cu + lay_.cu_off(3);
  f.cu_mvp_idx = cu + lay_.cu_off(4); f.cu_intra_mode = cu + lay_.cu_off(5); f.cu_cbf = cu + lay_.cu_off(6);
  f.cu_mv = cu_mv_[k]; f.cu_mvd = cu_mvd_[k];
  f.cu_ref = cfg_.fb_anchor && !p.fb_da ? nullptr : cu_ref_[k];      // NULL with one reference (fb-anchor: every picture but a v2 heal picture)
  f.sao = sao_[k];                                    // NULL without SAO
  f.ctu_qt = ctu_qt_[k]; f.ctu_qy = ctu_qy_[k]; f.ctu_delta = ctu_delta_[k]; f.ctu_first = ctu_first_[k];     // all NULL without qp_in_cu
  f.qp = p.qp; f.qpc = kChromaQp[p.qp]; f.lambda_q4 = kLambdaQ4[p.qp];
  f.is_intra = p.intra; f.poc = poc_;
  for (int c = 0; c < 3; c++) { f.rec[c] = cfg_.sao ? chain_.work[c] : rec_[cur_idx_][c]; f.sao_out[c] = rec_[cur_idx_][c]; f.ref[c] = rec_[ref_idx_][c]; }
  // me-source: the search looks at the previous input picture (still in its working set: the set is not padded into again before kSets - 1 more pictures have
  // gone through the input stream, behind this picture's k_me), and what the search and the intra pricing behind it write is the set's own
  f.me_ref = me_ahead_ && !p.intra ? src_[prev_set_][0] : f.ref[0];      // (a heal picture is not ahead and searches the previous input picture all the same)
  // lp-refs: reference r is the picture p.dist[r] before this one (the plan: r + 1, or lp-gop's table) -- ring slot cur_idx_ - p.dist[r]; the search
  // looks at its reconstruction or (me-source) at its input picture, which is still in the working set it was padded into (set_ - p.dist[r]: a set is padded
  // into again kSets pictures later, behind this picture's search on the input stream)
  if (f.cu_ref) {
    f.nref = p.nref;
    for (int r = 0; r < KVZ_MAX_LP_REFS; r++) {
      const int back = r < f.nref ? p.dist[r] : 1, slot = (cur_idx_ + nrec_ - back) % nrec_;
      for (int c = 0; c < 3; c++) f.refs[r][c] = rec_[slot][c];
      f.me_refs[r] = p.ahead || (p.fb_da && me_ahead_) ? src_[(k + kSets - back) % kSets][0] : f.refs[r][0];      // (a v2 heal picture is not ahead and searches the input pictures all the same)
    }
  }
  if ((gop_on() && !p.intra) || p.fb_da) f.ref_dist = (uint32_t)(uint8_t)p.dist[0] | (uint32_t)(uint8_t)p.dist[1] << 8 | (uint32_t)(uint8_t)p.dist[2] << 16 | (uint32_t)(uint8_t)p.dist[3] << 24;
  // tmvp: the previous picture -- set k - 1 -- filed its record on the tokenizer's stream, where this picture's k_inter_signal reads it; right after the IDR
  // picture (which files none) the slice says slice_temporal_mvp_enabled_flag = 0 (hevc_headers.h slice_tmvp) and nothing is read
  // me-coarse: the quarter picture of this set's input and of the sets that hold input pictures t - p.dist[r] (written on the input stream, where the coarse stage
  // reads them), and the set's centres
  if (cfg_.me_coarse) {                               // (scenecut alone keeps quarter pictures too: they are sc_stage's, no frame points at them)
    f.mc_rq = cfg_.me_coarse / 4; f.mc_q = mc_q_[k]; f.mc_centres = mc_centres_[k];
    const int nr = f.cu_ref ? f.nref : 1;
    for (int r = 0; r < KVZ_MAX_LP_REFS; r++) f.mc_qrefs[r] = mc_q_[(k + kSets - (r < nr ? p.dist[r] : 1)) % kSets];
  }
  if (p.ir_e) { f.ir_j = p.ir_j; f.ir_s = p.ir_s; f.ir_e = p.ir_e; f.ir_free = ir_free_ ? 1 : 0; }      // intra-refresh: the picture's band
  if (p.fb) {                                          // loss-feedback: a heal picture -- its block records; intra-in-p = 0: the intra-in-P stages for the forced quarters alone
    f.fb_heal = 1; f.fb_blk = fb_blk_; f.ir_free = cfg_.intra_in_p ? 1 : 0;
    if (!cfg_.intra_in_p && !p.fb_da) { f.intra_p = 1; point_me_block(f, lay_, me_cost16_); }      // (a v2 heal picture forces no quarter intra: no intra stage is brought up for it)
  }
  if (wp_rec_[k] && !p.intra) f.wp = wp_rec_[k];       // weightp: the record k_wp_decide writes on the input stream, in front of everything that reads it
  if (col_[k] && !p.intra) { f.col_out = col_[k]; f.col_prev = poc_ >= 2 ? col_[(k + kSets - 1) % kSets] : nullptr; }
  if (p.ahead && me_block_[k]) { point_me_block(f, lay_, me_block_[k]); f.sync = sync_set_[k]; }
  f.tok_dense = sl.d_tok_dense; f.tok_count_out = sl.d_tok_count; f.tok_off_out = sl.d_tok_off; f.err_out = sl.d_err; f.ent_cursors = sl.g_cursors;
  f.tok_cursor = (uint32_t *)tok_count_ + (size_t)(frame_idx_ & 1) * lay_.nctu; f.tok_cursor_next = (uint32_t *)tok_count_ + (size_t)((frame_idx_ + 1) & 1) * lay_.nctu;
  f.chain_gen = chain_gen;
  if (p.side) {                                       // beside the P pictures still on the main stream: nothing of theirs is touched
    point_chain(f, lay_, chain_idr_);
    f.me_cand = nullptr;                              // (me_cand NULL: the picture's deblocking kernel leaves the P pictures' candidate list and "has intra units" word alone)
    if (cfg_.sao) for (int c = 0; c < 3; c++) f.rec[c] = chain_idr_.work[c];
  }
  return f;
}

bool Encoder::submit(const uint8_t *d_i420, int in_ring)
{
  Slot &sl = slot_[submitted_ % nslots_];
  cur_slot_ = &sl;
  prof_now_ = profiling_ && (frame_idx_ % prof_every_) == 0;
  // Three HIP streams per picture t.
  //   stream_in_:  input padding into source set t & 1 -- runs while stream_ still works on picture t - 1.
  //   stream_:     motion search / intra decisions, reconstruction, deblocking: the chain picture t + 1 depends on.
  //   stream_tok_: merge/AMVP signalling, tokenizer, compaction, which only feed the host; they read set t & 1 of the
  //                level / CU arrays while stream_ already fills the other set for t + 1.
  // scenecut: whether the picture is an IDR picture may depend on the picture itself -- the head of its input stage runs, and an examined picture's verdict is
  // waited for, before anything is planned
  if (cfg_.scenecut && !sc_stage((int)(submitted_ % kSets), d_i420, in_ring)) return false;
  const Plan p = plan((int)(submitted_ % kSets));
  const EncFrame f = picture_frame(p, sl, next_chain_gen());
  if (all_intra_alt_) idr_pending_ = false;                 // (alternating intra pictures: the main stream's next picture has nothing to do with the side stream's last)
  if (!p.side && idr_pending_) { HIP_CHECK(hipStreamWaitEvent(stream_, ev_idr_done_, 0)); idr_pending_ = false; }
  return input_stage(f, p, d_i420, in_ring) && chain_stage(f, p) && hand_off(f, p, sl, in_ring);
}

// stream_in_, the head of the input stage: the picture padded into its working set, and its quarter picture where an option keeps one
bool Encoder::pad_stage(int set, const uint8_t *d_i420, int in_ring)
{
  if (src_busy_[set]) { HIP_CHECK(hipStreamWaitEvent(stream_in_, ev_src_free_[set], 0)); src_busy_[set] = false; }   // the last picture that used this set (t - kSets) has been reconstructed
  // input-format: a packed picture is converted in the pass that pads it, under the input stage's kernel id
  if (cfg_.input_format == KVZ_INPUT_I420) timed(K_PAD, stream_in_, [&] { launch_pad_input(d_i420, cfg_.width, cfg_.height, src_[set][0], src_[set][1], src_[set][2], cw_, ch_, stream_in_); });
  else {
    bool ok = true;
    timed(K_PAD, stream_in_, [&] { ok = launch_input_packed(cfg_.input_format, d_i420, cfg_.width, cfg_.height, src_[set][0], src_[set][1], src_[set][2], cw_, ch_, stream_in_); });
    if (!ok) return false;
  }
  if (in_ring >= 0) { HIP_CHECK(hipEventRecord(ev_pad_[in_ring], stream_in_)); pad_pending_[in_ring] = true; }
  // me-coarse, scenecut: every picture's quarter picture (an intra picture's is searched by / compared with the P picture behind it)
  if (mc_q_[set]) launch_luma_quarter(src_[set][0], mc_q_[set], cw_, ch_, stream_in_);      // (no kernel id of its own: the profile's keys are the default encoder's)
  return true;
}

// the host's wait for an event of its own stream, as finish_slot waits for a slot's
bool Encoder::wait_event(hipEvent_t e)
{
  if (depth_ >= 2 && !spin_wait_) return nap_until([&] { hipError_t r = hipEventQuery(e); return r == hipSuccess ? 1 : (r == hipErrorNotReady ? 0 : -1); });
  HIP_CHECK(hipEventSynchronize(e));
  return true;
}

// scenecut, the input stream, in front of plan(): the picture padded, its quarter picture and that picture's sum (every picture: the next one is compared with
// it); a picture sc_examined() names: the blocks against the previous input picture's quarter picture (the previous working set's, written on this stream),
// the record -- and the feature's one wait on the host, for the verdict plan() needs.  A picture that is not examined waits for nothing; its record is
// written here.
bool Encoder::sc_stage(int set, const uint8_t *d_i420, int in_ring)
{
  if (!pad_stage(set, d_i420, in_ring)) return false;
  const int prev = (set + kSets - 1) % kSets, period = cfg_.intra_period;
  const int since = frame_idx_ == 0 ? 0 : poc_ + 1;         // pictures behind the last IDR picture
  const bool periodic = frame_idx_ == 0 || (period > 0 && since % period == 0);
  ScArgs a{};
  a.qc = mc_q_[set]; a.qp = mc_q_[prev]; a.qw = cw_ / 4; a.qh = ch_ / 4; a.vw = (cfg_.width + 3) / 4; a.vh = (cfg_.height + 3) / 4;
  sc_visible_blocks(cfg_.width, cfg_.height, &a.bw, &a.bh); a.rq = sc_reach(cfg_.me_coarse);
  a.sum_c = sc_sum_[set]; a.sum_p = sc_sum_[prev]; a.blocks = sc_blocks_; a.n_new = sc_count_; a.rec = sc_rec_; a.rec_host = cur_slot_->d_sc;
  HIP_CHECK(hipMemsetAsync(sc_sum_[set], 0, sizeof(unsigned long long), stream_in_));
  launch_sc_sum(a, stream_in_);
  volatile int32_t *h = cur_slot_->h_sc;
  sc_cut_ = false;
  if (!sc_examined(since, cfg_.scenecut, periodic)) { h[0] = 0; h[1] = 0; h[2] = a.bw * a.bh; h[3] = 0; h[4] = 0; return true; }
  launch_sc_blocks(a, stream_in_);
  launch_sc_decide(a, stream_in_);
  HIP_CHECK(hipEventRecord(ev_sc_, stream_in_));
  if (!wait_event(ev_sc_)) return false;                    // (the time counts as submit time: KVAZZUP_AMD_TRACE)
  sc_cut_ = h[0] == 1 && h[4] != 0;
  return true;
}

// stream_in_: the picture padded into its set, and what needs the source pictures only; in_done_ behind it
bool Encoder::input_stage(const EncFrame &f, const Plan &p, const uint8_t *d_i420, int in_ring)
{
  if (!cfg_.scenecut && !pad_stage(set_, d_i420, in_ring)) return false;      // (scenecut: sc_stage has queued it)
  // weightp: every picture's luma statistics (an intra picture's are its successors' reference's), and a P picture's weights -- from input pictures alone,
  // whatever me-source says, like the coarse stage below
  if (cfg_.weightp && !wp_stage(f, p, *cur_slot_)) return false;
  // The tokenizer of the set's previous picture must be done with the set's CU arrays before this picture writes them: the INPUT stream waits for it (the
  // event is long past when it gets there), so that the main stream's one wait for in_done_ says both -- a wait of its own in front of every picture's chain
  // cost the chain a barrier packet, a few microseconds with nothing running.
  if (tok_pending_[set_]) { HIP_CHECK(hipStreamWaitEvent(stream_in_, ev_tok_done_[set_], 0)); tok_pending_[set_] = false; }
  if (p.intra) {
    // The intra decisions need the source picture only: they run on the input stream, beside what is left of picture t - 1 on the main stream.
    timed(K_INTRA_ANALYSE, stream_in_, [&] { launch_intra_analyse(f, stream_in_); });
  }
  // me-coarse: the coarse stage needs input pictures only, so it runs here whatever me-source says -- beside the chains of the pictures in front, and behind the
  // wait above (the centres are the set's own: its previous picture's k_me has long read them); in_done_ covers it for a k_me on the main stream
  if (f.mc_rq && !p.intra) launch_me_coarse(f, stream_in_);
  if (p.ahead) {
    // "uvgx search pipelining v1": the search needs the two input pictures only, the pricing of its expensive quarters as intra blocks the search and the source --
    // both run HERE, on the input stream, beside what the main stream still has of the pictures in front (k_me 31-34 us and k_intra_analyse<P> 19-24 us at
    // 1080p leave the chain the next picture waits for; the head of the chain, when there is one, is a launch of its own on the main stream)
    const EncFrame fs = f.wp ? wp_search_frame(f, p, stream_in_) : f;      // weightp: the search reads the references' weighted planes
    timed(K_ME, stream_in_, [&] { launch_me(fs, stream_in_); });
    if (f.intra_p) timed(K_INTRA_ANALYSE_P, stream_in_, [&] { launch_intra_analyse(f, stream_in_); });
  }
  if (!stage_roi(stream_in_)) return false;
  HIP_CHECK(hipEventRecord(in_done_, stream_in_)); in_pending_ = true;
  return true;
}

// the picture's chain on p.ms: decisions, reconstruction, loop filters; ev_src_free_ behind it
bool Encoder::chain_stage(const EncFrame &f, const Plan &p)
{
  const hipStream_t ms = p.ms;
  HIP_CHECK(hipStreamWaitEvent(ms, in_done_, 0));      // (measured by leaving it out: 8 of the ~28 us between a picture's last kernel and the next one's first; the rest is the record behind k_sao that two other streams wait for)
  EncFrame fm = f;                                               // (the picture's first kernel may carry the head of the chain)
  if (p.intra) { if (!picture_begin(f, ms, nullptr, true)) return false; }
  else if (!picture_begin(f, ms, p.ahead && cfg_.subme == 0 ? nullptr : &fm)) return false;      // (the search ahead on the input stream: the chain's head rides in k_subpel, or is a launch of its own without one)
  if (p.intra) {
    timed(K_INTRA_RECON, ms, [&] { launch_intra_recon(f, ms); });
  } else {
    if (p.fb && !fb_stage(f, p, *cur_slot_)) return false;        // loss-feedback: the heal picture's map and block records, behind the chain of the picture before
    if (!p.ahead) { const EncFrame fs = f.wp ? wp_search_frame(fm, p, stream_) : fm; timed(K_ME, stream_, [&] { launch_me(fs, stream_); }); }      // (weightp: the planes are made of reconstructions here, so on this stream)
    // loss-feedback under me-source: the one search that reads an input picture (t - 1's, in its working set) from the MAIN stream.  That set's free event was
    // recorded behind t - 1's chain, in front of this read, so the input stream -- which pads a later picture into the set -- waits for the search itself
    if (p.fb && me_ahead_) { HIP_CHECK(hipEventRecord(ev_fb_me_, stream_)); HIP_CHECK(hipStreamWaitEvent(stream_in_, ev_fb_me_, 0)); }
    // intra-in-P: quarters whose inter cost is high are priced as intra blocks and may become intra units (the launch leaves at once where none is)
    if (f.intra_p && !p.ahead) timed(K_INTRA_ANALYSE_P, stream_, [&] { launch_intra_analyse(f, stream_); });
    if (cfg_.subme > 0) timed(K_SUBPEL, stream_, [&] { launch_subpel(p.ahead ? fm : f, stream_); });
    if (rc_state_) {
      // rate control v2: the CTU rows in groups inside the one launch, the next group's QP decided on the device from the levels of the groups before
      EncFrame fb = f;
      fb.rc = rc_state_; fb.rc_nb = cfg_.rc_bands < rows_ ? cfg_.rc_bands : rows_; fb.rc_slot = frame_idx_ & 7;
      fb.rc_target = ((long long)cfg_.bitrate * cfg_.fps_den) / (cfg_.fps_num > 0 ? cfg_.fps_num : 1);
      timed(K_INTER_RECON, stream_, [&] { launch_inter_recon(fb, stream_); });
    } else
    timed(K_INTER_RECON, stream_, [&] { launch_inter_recon(f, stream_); });
    // ... and are reconstructed behind every inter unit (their reference samples may lie in inter units anywhere around them)
    if (f.intra_p) timed(K_INTRA_RECON_P, stream_, [&] { launch_intra_recon(f, stream_); });
    if (f.intra_p && !cfg_.deblock) { HIP_CHECK(hipMemsetAsync(f.me_cand, 0, sizeof(uint32_t), stream_)); HIP_CHECK(hipMemsetAsync(f.sync + rows_ * (cw_ / 64) * 3 + 1, 0, sizeof(uint32_t), stream_)); }      // (k_deblock_tile does it otherwise)
  }
  launch_qp_resolve(f, ms);                                      // per-CTU QP: which CU carries the delta, QpY for deblocking
  if (cfg_.fb_anchor && !p.fb_da) HIP_CHECK(hipMemsetAsync(cu_ref_[set_], 0, lay_.nb8, ms));      // fb-anchor: one reference -- debug_copy("cu_ref") says so (no kernel of the picture reads the array)
  if (p.fb_da) {                                                 // fb-anchor: the v2 heal picture's count of quarters on the anchor (the decisions are final)
    FbRefArgs a{};
    a.gw = cw_ / 8; a.gh = ch_ / 8; a.cu_intra = f.cu_intra; a.cu_ref = f.cu_ref; a.stat = cur_slot_->d_fb;
    launch_fb_refs(a, ms);
  }
  // levels, cbf and motion of the picture are final: the tokenizer's stream may start.  With SAO it waits for the filter anyway (the CTUs' SAO parameters
  // are coded) -- then no event is recorded in the middle of the chain (an event between two kernels of a stream costs the chain ~7 us)
  if (!cfg_.sao) HIP_CHECK(hipEventRecord(ev_signalled_, ms));
  if (cfg_.deblock) timed(K_DEBLOCK, ms, [&] { launch_deblock(f, ms); });
  if (cfg_.sao) timed(K_SAO, ms, [&] { launch_sao(f, ms); });      // (ONE event behind the chain's last kernel says "SAO done" and "the set is free": every record in the chain is a packet the next picture waits behind)
  // loss-feedback: a P picture's record into its place in the ring -- vectors and intra decisions are final.  An IDR picture files none: fb_stage never steps
  // through one (a report from in front of it is void), and its chain may run on the side stream, beside a heal picture that still reads the ring
  if (cfg_.loss_feedback && !p.intra) {
    FbRefArgs a{};
    a.gw = cw_ / 8; a.gh = ch_ / 8; a.cu_mv = f.cu_mv; a.cu_intra = f.cu_intra; a.cu_log2 = f.cu_log2; a.clean = 0;
    const size_t place = (size_t)(frame_idx_ % cfg_.loss_feedback);
    a.rec_mv = fb_rec_mv_ + place * lay_.nb8 * 2; a.rec_info = fb_rec_info_ + place * lay_.nb8;
    if (cfg_.fb_anchor) fb_rec_anchor_[place] = p.fb_da ? poc_ - p.fb_da : -1;
    if (p.fb_da) { a.cu_ref = f.cu_ref; launch_fb_record_ref(a, ms); }      // fb-anchor: a v2 heal picture's record carries the reference bit
    else launch_fb_record(a, ms);
  }
  // Last reader of this set on the main stream: k_sao reads the source picture for its statistics, deblocking the CU records.
  // Input padding and intra analysis of the next picture with this set (input stream) overwrite both and wait for this event.
  HIP_CHECK(hipEventRecord(ev_src_free_[set_], ms)); src_busy_[set_] = true;
  if (p.side) { HIP_CHECK(hipEventRecord(ev_idr_done_, ms)); idr_pending_ = true; }
  return true;
}

// loss-feedback, the main stream, in front of the heal picture's search: the map starts empty at the oldest reported picture, takes that picture's reports
// (k_fb_seed), then goes through the record of every picture up to the one before the heal picture (k_fb_step), taking the later pictures' reports on the way;
// a report from further back than the ring reaches makes the map full.  Then the block records.  The pictures since the last IDR picture have the POCs
// 0 .. poc_ one after the other, so the picture with POC k lies poc_ - k pictures back.
bool Encoder::fb_stage(const EncFrame &f, const Plan &p, Slot &sl)
{
  (void)p;
  const int H = cfg_.loss_feedback, t = poc_;
  FbRefArgs a{};
  a.gw = cw_ / 8; a.gh = ch_ / 8; a.map = fb_map_; a.tmp = fb_tmp_; a.dilate = cfg_.deblock || cfg_.sao ? 1 : 0;
  a.me_range = f.range; a.blk = fb_blk_; a.stat = sl.d_fb;
  int oldest = t;
  for (const FbReport &r : fb_heal_) oldest = r.poc < oldest ? r.poc : oldest;
  if (t - oldest > H) HIP_CHECK(hipMemsetAsync(fb_map_, 1, lay_.nb8, stream_));
  else {
    HIP_CHECK(hipMemsetAsync(fb_map_, 0, lay_.nb8, stream_));
    for (int k = oldest; k < t; k++) {
      if (k > oldest) {
        const size_t place = (size_t)((frame_idx_ - (t - k)) % H);
        a.rec_mv = fb_rec_mv_ + place * lay_.nb8 * 2; a.rec_info = fb_rec_info_ + place * lay_.nb8;
        // fb-anchor: picture k was a v2 heal picture -- its reference-1 cells read its anchor, which is wrong only where the report reaches it
        if (cfg_.fb_anchor && fb_rec_anchor_[place] >= 0) { a.anchor_bad = oldest <= fb_rec_anchor_[place] ? 1 : 0; launch_fb_step_ref(a, stream_); }
        else launch_fb_step(a, stream_);
      }
      for (const FbReport &r : fb_heal_) if (r.poc == k) { a.first = r.first; a.count = r.count; launch_fb_seed(a, stream_); }
    }
  }
  launch_fb_blocks(a, stream_);
  return true;
}

int Encoder::report_damage(int32_t poc, int first_ctb, int count)
{
  if (!cfg_.loss_feedback || poc < 0) return 0;
  if (count > 0 && (first_ctb < 0 || (long long)first_ctb + count > (long long)lay_.nctu)) return 0;
  drain_submitter();                                        // (owf >= 2: everything handed in so far has been planned -- the next picture is the heal picture)
  if (frame_idx_ == 0 || poc > poc_) return 2;              // the picture lies in front of the last IDR picture (or nothing has been coded): nothing to heal
  std::lock_guard<std::mutex> l(fbm_);
  fb_q_.push_back(FbReport{poc, first_ctb, count});
  return 1;
}

// weightp, the input stream: the picture's statistics; a P picture: candidate weights against every reference's input picture (the set it was padded into, as
// me-source's planes), the check, and the record -- into the set's device copy and the slot's host-mapped one.  Nothing waits for the host.
bool Encoder::wp_stage(const EncFrame &f, const Plan &p, const Slot &sl)
{
  const int k = set_;
  launch_wp_stats(src_[k][0], cw_, cfg_.width, cfg_.height, wp_partial_[k], stream_in_);
  WpArgs a{};
  a.partial = wp_partial_[k]; a.nblk = wp_stat_blocks(cfg_.height); a.n = (long long)cfg_.width * cfg_.height; a.stat = wp_stat_[k];
  a.nref = p.intra ? 0 : (f.cu_ref ? f.nref : 1);
  for (int r = 0; r < a.nref; r++) { const int ks = (k + kSets - p.dist[r]) % kSets; a.stat_ref[r] = wp_stat_[ks]; a.in_ref[r] = src_[ks][0]; }
  a.cand = wp_cand_; a.acc = wp_acc_; a.rec = wp_rec_[k]; a.rec_host = sl.d_wp;
  launch_wp_decide(a, 0, stream_in_);
  if (p.intra) return true;
  launch_wp_check(a, src_[k][0], cw_, cfg_.width, cfg_.height, stream_in_);
  launch_wp_decide(a, 1, stream_in_);
  return true;
}

// weightp: the planes the integer search reads -- the plane it would have read of every reference (f.me_ref / f.me_refs: reconstruction or, me-source, input
// picture) through wp_sample with the reference's (w, o), a copy where the reference is not weighted
EncFrame Encoder::wp_search_frame(const EncFrame &f, const Plan &p, hipStream_t st)
{
  (void)p;
  EncFrame fs = f;
  const int nref = f.cu_ref ? f.nref : 1;
  WpPlaneArgs a{};
  a.rec = f.wp;
  for (int r = 0; r < nref; r++) { a.from[r] = f.cu_ref ? f.me_refs[r] : f.me_ref; a.to[r] = wp_plane_[r]; }
  launch_wp_plane(a, nref, cw_, ch_, st);
  fs.me_ref = wp_plane_[0];
  if (f.cu_ref) for (int r = 0; r < KVZ_MAX_LP_REFS; r++) fs.me_refs[r] = wp_plane_[r < nref ? r : 0];
  return fs;
}

// the picture handed on: tokenizer, GPU arithmetic coder, copy of the reconstruction into the caller's picture, the slot to the workers
bool Encoder::hand_off(const EncFrame &f, const Plan &p, Slot &sl, int in_ring)
{
  const hipStream_t ms = p.ms;
  sl.set = set_;
  if (tok_deferred_) { sl.f_tok = f; sl.prof = prof_now_; }          // (encoder.h tok_deferred_: the launcher thread makes these launches when the chain is done)
  else if (!launch_tokenizer(sl, f, p.intra, true, prof_now_)) return false;
  tok_pending_[set_] = true;
  // the slot is complete when both streams are: the tokens (stream_tok_) and the reconstruction (stream_)
  if (cfg_.entropy_gpu) {
    // arithmetic coding on the slot's own stream, behind the compaction: the coders of several pictures run side by side
    HIP_CHECK(hipEventRecord(sl.tok_ev, stream_tok_));
    HIP_CHECK(hipStreamWaitEvent(sl.ent_stream, sl.tok_ev, 0));
    const int nsub = cfg_.wpp ? rows_ : cfg_.tile_rows;
    CabacRowsArgs a;
    a.tok = sl.g_tok; a.count = sl.g_count; a.off = sl.g_off; a.stage = sl.g_stage; a.stage_cap = (uint32_t)lay_.stage_cap; a.out = sl.d_out; a.out_cap = (uint32_t)lay_.out_cap;
    a.cursors = sl.g_cursors; a.sub_off = sl.d_sub; a.sub_len = sl.d_sub + rows_; a.sub_bins = sl.d_sub + 2 * rows_;
    a.ctx_save = sl.g_ctx_save; a.ctx_ready = sl.g_ctx_ready; a.gen = ++sl.gen; a.err = err_;
    a.wc = cw_ / 64; a.hc = rows_; a.wpp = cfg_.wpp; a.tile_rows = cfg_.tile_rows; a.init_type = p.intra ? 0 : 1; a.qp = f.qp; a.first_sub = 0;
    timed(K_CABAC_ROWS, sl.ent_stream, [&] { launch_cabac_rows(a, nsub, sl.ent_stream); });
    HIP_CHECK(hipEventRecord(sl.done, sl.ent_stream));
  } else if (!tok_deferred_) HIP_CHECK(hipEventRecord(sl.done, stream_tok_));      // (tok_deferred_: launch_tokenizer records it)
  // reconstruction final: with SAO the tokenizer's stream waited for the filter -- the chain's last kernel --, so sl.done already says it (and a record the
  // host can inspect ends with a system-scope fence: one fewer at the end of every picture's chain)
  if (!cfg_.sao) HIP_CHECK(hipEventRecord(sl.rec_done, ms));
  sl.has_sink = false;
  if (sink_sub_[0] && in_ring >= 0) {                      // (host pictures only: set_recon_sink)
    // the reconstruction is final behind the chain's last kernel: rec_done, with SAO the event behind the filter
    if (!stream_rec_) HIP_CHECK(stream_acquire(&stream_rec_, cfg_.device, 'R', 'n'));
    if (!sl.sink_done) HIP_CHECK(mem_.event(&sl.sink_done, hipEventDisableTiming));
    HIP_CHECK(hipStreamWaitEvent(stream_rec_, cfg_.sao ? ev_src_free_[set_] : sl.rec_done, 0));
    for (int c = 0; c < 3; c++) {
      const int pw = c ? cfg_.width / 2 : cfg_.width, ph = c ? cfg_.height / 2 : cfg_.height, cp = c ? cw_ / 2 : cw_;
      if (pw == cp) HIP_CHECK(hipMemcpyAsync(sink_sub_[c], rec_[cur_idx_][c], (size_t)pw * ph, hipMemcpyDeviceToHost, stream_rec_));
      else HIP_CHECK(hipMemcpy2DAsync(sink_sub_[c], (size_t)pw, rec_[cur_idx_][c], (size_t)cp, (size_t)pw, (size_t)ph, hipMemcpyDeviceToHost, stream_rec_));
    }
    HIP_CHECK(hipEventRecord(sl.sink_done, stream_rec_));
    sl.has_sink = true;
  }
  sink_sub_[0] = sink_sub_[1] = sink_sub_[2] = nullptr;
  sl.pic_idx = submitted_; sl.poc = poc_; sl.intra = p.intra; sl.rec_idx = cur_idx_; sl.qp = f.qp; sl.write_ps = false;
  if (sl_gop_timeline(p)) { char w[12]; snprintf(w, sizeof(w), "g%dq%02dd%d%d%d%d", p.layer, f.qp, p.nref > 0 ? p.dist[0] : 0, p.nref > 1 ? p.dist[1] : 0, p.nref > 2 ? p.dist[2] : 0, p.nref > 3 ? p.dist[3] : 0); tl(w, submitted_); }      // KVAZZUP_AMD_TIMELINE, lp-gop: a P picture's layer, QP and reference distances as a record "g<layer>q<QP>d<four distances, 0 = none>"
  if (sl.h_fb) { sl.h_fb[0] = p.fb ? 1 : 0; sl.h_fb[1] = p.fb ? (int32_t)fb_heal_.size() : 0; if (!p.fb) { sl.h_fb[2] = 0; sl.h_fb[3] = 0; } }      // (a heal picture's counts: k_fb_blocks)
  sl.ir[0] = p.ir_j; sl.ir[1] = p.ir_s; sl.ir[2] = p.ir_e; sl.ir[3] = cfg_.intra_refresh ? ir_cycle(cw_, cfg_.intra_refresh) : 0;
  sl.layer = p.layer; sl.nref = (gop_on() || cfg_.fb_anchor) && !p.intra ? p.nref : 0; for (int r = 0; r < KVZ_MAX_LP_REFS; r++) sl.dist[r] = r < sl.nref ? p.dist[r] : 0;
  sl.kept = cfg_.fb_anchor && !p.intra ? fb_anchor_kept(poc_, cfg_.fb_anchor) : 0;      // fb-anchor: every P picture lists the pictures it keeps
  if (sl.h_fb && cfg_.fb_anchor) { sl.h_fb[4] = p.fb_da ? 1 : 0; sl.h_fb[5] = p.fb_da ? poc_ - p.fb_da : 0; sl.h_fb[6] = p.fb_da; if (!p.fb_da) sl.h_fb[7] = 0; }      // (a v2 heal picture's count: k_fb_refs)
  if (p.intra) {
    sl.write_ps = (intra_count_ == 0) || (cfg_.vps_period > 0 && (intra_count_ % cfg_.vps_period) == 0);
    intra_count_++;
  }
  frame_idx_++; prev_set_ = set_;
  ref_idx_ = cur_idx_; cur_idx_ = (cur_idx_ + 1) % nrec_;      // rec_[ref_idx_] holds the picture just submitted
  submitted_++;
  if (tok_deferred_) {
    { std::lock_guard<std::mutex> l(bm_); sl.ready = false; }
    { std::lock_guard<std::mutex> l(tm_); tq_.push_back((int)((submitted_ - 1) % nslots_)); }
    tcv_.notify_all();
  } else if (depth_ >= 2) {
    { std::lock_guard<std::mutex> l(bm_); sl.ready = false; bq_.push_back((int)((submitted_ - 1) % nslots_)); }
    bcv_.notify_all();
  }
  return true;
}

// the tokenizer's three launches of one picture (stream_tok_) and the events behind them
bool Encoder::launch_tokenizer(Slot &sl, const EncFrame &f, bool intra, bool wait_on_stream, bool prof)
{
  if (wait_on_stream) HIP_CHECK(hipStreamWaitEvent(stream_tok_, cfg_.sao ? ev_src_free_[sl.set] : ev_signalled_, 0));
  if (!intra) timed_slot(sl, prof, K_INTER_SIGNAL, stream_tok_, [&] { launch_inter_signal(f, stream_tok_); });
  timed_slot(sl, prof, K_TOKENIZE, stream_tok_, [&] { launch_tokenize(f, stream_tok_); });
  timed_slot(sl, prof, K_TOK_COMPACT, stream_tok_, [&] { launch_tok_compact(f, stream_tok_); });
  HIP_CHECK(hipEventRecord(ev_tok_done_[sl.set], stream_tok_));
  if (tok_deferred_) HIP_CHECK(hipEventRecord(sl.done, stream_tok_));
  return true;
}

// encoder.h tok_deferred_: pictures in submission order -- wait (on the host, in naps) for the picture's chain, launch its tokenizer, hand the slot to the workers
void Encoder::tok_launcher()
{
  hipSetDevice(cfg_.device);
  for (;;) {
    int idx;
    { std::unique_lock<std::mutex> l(tm_); tcv_.wait(l, [&] { return tquit_ || !tq_.empty(); }); if (tq_.empty()) return; idx = tq_.front(); tq_.pop_front(); }
    Slot &sl = slot_[idx];
    hipEvent_t e = ev_src_free_[sl.set];                   // recorded behind the chain's last kernel (k_sao); not recorded again before this picture has been collected (owf < kSets)
    const bool chain_ok = nap_until([&] { hipError_t r = hipEventQuery(e); return r == hipSuccess ? 1 : (r == hipErrorNotReady ? 0 : -1); });
    tl("tok0", sl.pic_idx);
    // (a failed query -- device fault, the chain's last kernel failed -- means the CU and SAO arrays are not final: the picture fails like one whose
    // tokenizer could not be launched, finish_slot never codes what the slot held)
    sl.tok_failed = !chain_ok || !launch_tokenizer(sl, sl.f_tok, sl.intra, false, sl.prof);
    if (sl.tok_failed) fprintf(stderr, chain_ok ? "kvazzup_amd: the tokenizer of picture %ld could not be launched\n" : "kvazzup_amd: the kernels of picture %ld failed; it is not entropy coded\n", sl.pic_idx);
    { std::lock_guard<std::mutex> l(bm_); bq_.push_back(idx); }
    bcv_.notify_all();
  }
}

bool Encoder::collect(EncodedPicture *out)
{
  Slot &sl = slot_[collected_ % nslots_];
  tl("col0", collected_);
  struct OnExit { long p; ~OnExit() { tl("col1", p); } } on_exit_{collected_};
  collected_++;
  bool ok;
  if (depth_ >= 2) {
    Tick tk;
    std::unique_lock<std::mutex> l(bm_);
    bcv_.wait(l, [&] { return sl.ready; });
    t_wait_ += tk.ms();
    ok = sl.ok;
    std::swap(*out, sl.result);
  } else ok = finish_slot(sl, out);
  out_idx_ = sl.rec_idx; out_set_ = sl.set;
  out_gop_[0] = gop_on(); out_gop_[1] = out->layer; out_gop_[2] = out->qp; out_gop_[3] = out->nref; for (int r = 0; r < KVZ_MAX_LP_REFS; r++) out_gop_[4 + r] = out->dist[r];
  memcpy(out_wp_, out->wp, sizeof(out_wp_));
  memcpy(out_ir_, out->ir, sizeof(out_ir_));
  memcpy(out_sc_, out->sc, sizeof(out_sc_));
  memcpy(out_fb_, out->fb, sizeof(out_fb_));
  memcpy(out_fba_, out->fba, sizeof(out_fba_));
  rc_bytes_[(collected_ - 1) & 7] = (uint32_t)out->au.size();   // (collected_ - 1 = index of this picture)
  return ok;
}

// owf >= 2: pictures are finished here, in submission order, while the calling thread keeps launching kernels
void Encoder::background(int worker)
{
  hipSetDevice(cfg_.device);
  for (;;) {
    int idx;
    { std::unique_lock<std::mutex> l(bm_); bcv_.wait(l, [&] { return bquit_ || !bq_.empty(); }); if (bq_.empty()) return; idx = bq_.front(); bq_.pop_front(); }
    Slot &sl = slot_[idx];
    tl("bg0", sl.pic_idx);
    const bool ok = finish_slot(sl, &sl.result, worker);
    tl("bg1", sl.pic_idx);
    { std::lock_guard<std::mutex> l(bm_); sl.ok = ok; sl.ready = true; }
    bcv_.notify_all();
  }
}

bool Encoder::finish_slot(Slot &sl, EncodedPicture *out, int worker)
{
  out->valid = false; out->au.clear(); out->recon_delivered = false;
  // (whatever way this function is left: the copy into the caller's reconstruction picture is not in flight any more -- the caller frees it on failure)
  struct SinkGuard { Slot &s; ~SinkGuard() { if (s.has_sink) { hipEventSynchronize(s.sink_done); s.has_sink = false; } } } sink_guard_{sl};
  if (sl.tok_failed) { sl.tok_failed = false; return false; }
  {
    Tick tk;
    if (depth_ >= 2 && !spin_wait_) {          // background worker: naps between queries (see nap_until)
      auto q = [&](hipEvent_t e) { return nap_until([&] { hipError_t r = hipEventQuery(e); return r == hipSuccess ? 1 : (r == hipErrorNotReady ? 0 : -1); }); };
      if (!q(sl.done) || !q(sl.rec_done)) return false;
    } else { HIP_CHECK(hipEventSynchronize(sl.done)); HIP_CHECK(hipEventSynchronize(sl.rec_done)); }
    if (depth_ < 2) t_wait_ += tk.ms();
  }
  if (*sl.h_err) { fprintf(stderr, "kvazzup_amd: device error flags 0x%x (8/16/32: token buffer overflow)\n", *sl.h_err); return false; }
  if (sl.ev_used) {
    std::lock_guard<std::mutex> l(stat_m_);
    for (size_t i = 0; i < sl.ev_used; i++) {
      float ms = 0; hipEventElapsedTime(&ms, sl.ev[i].a, sl.ev[i].b);
      k_ms_[sl.ev[i].id] += ms; k_n_[sl.ev[i].id]++;
    }
    sl.ev_used = 0;
  }
  tl("gpudone", sl.pic_idx);
  // ---- serial half of entropy coding: host threads turn the bins into the WPP substreams
  const int nsub = (cfg_.wpp ? rows_ : cfg_.tile_rows) * cfg_.tile_cols;
  uint64_t bins = 0;
  Tick tk_ar;
  std::vector<std::vector<uint8_t>> &rows_out = worker ? rows_out2_ : rows_out_;
  if (cfg_.entropy_gpu) {
    // the substreams were coded on the GPU (k_cabac_rows) and lie in the slot's host-mapped buffer
    rows_out.resize((size_t)nsub);
    const uint32_t *off = sl.h_sub, *len = sl.h_sub + rows_, *nb = sl.h_sub + 2 * rows_;
    for (int k = 0; k < nsub; k++) {
      if (len[k] == ~0u || (size_t)off[k] + len[k] > lay_.out_cap) { fprintf(stderr, "kvazzup_amd: substream %d was not coded (token or output buffer overflow)\n", k); return false; }
      rows_out[(size_t)k].assign(sl.h_out + off[k], sl.h_out + off[k] + len[k]);
      bins += nb[k];
    }
  } else {
    for (int i = 0, n = (cw_ / 64) * rows_; i < n; i++) if (sl.h_tok_count[i] < 0) { fprintf(stderr, "kvazzup_amd: token array overflow (CTU %d)\n", i); return false; }
    EntropyHost *coder = worker ? entropy2_ : entropy_;
    coder->code_picture(sl.h_tok_dense, sl.h_tok_count, sl.h_tok_off, cw_ / 64, rows_, cfg_.wpp != 0, cfg_.tile_rows, sl.intra ? 0 : 1, sl.qp, rows_out, &bins, cfg_.tile_cols);
  }
  const double ar = tk_ar.ms();
  tl("arith", sl.pic_idx);
  if (profiling_ && !cfg_.entropy_gpu) { std::lock_guard<std::mutex> l(stat_m_); k_ms_[K_HOST_ARITH] += ar; k_n_[K_HOST_ARITH]++; }
  { std::lock_guard<std::mutex> l(stat_m_); t_arith_ += ar; }
  // ---- access unit assembly (host): parameter sets with IDR pictures, then the slice NAL
  out->valid = true; out->poc = sl.poc; out->qp = sl.qp; out->is_intra = sl.intra; out->bins = bins;
  out->layer = sl.layer; out->nref = sl.nref; for (int r = 0; r < KVZ_MAX_LP_REFS; r++) out->dist[r] = sl.dist[r];
  PicRefs pr; pr.n = sl.nref; pr.kept = sl.kept; for (int r = 0; r < KVZ_MAX_LP_REFS; r++) pr.dist[r] = sl.dist[r];      // lp-gop: the slice headers carry the picture's reference picture set
  memcpy(out->ir, sl.ir, sizeof(out->ir));
  if (sl.h_sc) memcpy(out->sc, sl.h_sc, sizeof(out->sc));      // scenecut: the record, final since the picture was submitted
  if (sl.h_fb) for (int i = 0; i < 4; i++) out->fb[i] = sl.h_fb[i];      // loss-feedback: the record, final with the picture's chain
  if (sl.h_fb && cfg_.fb_anchor) for (int i = 0; i < 4; i++) out->fba[i] = sl.h_fb[4 + i];
  int recovery = cfg_.intra_refresh && !sl.intra && sl.ir[0] == 0 ? sl.ir[3] - 1 : -1;      // intra-refresh: a cycle's first picture says when the pass is complete
  if (sl.h_fb && sl.h_fb[0]) recovery = 0;                 // loss-feedback: the heal picture is itself the recovery point
  PicWeights pw{};                                         // weightp: the record k_wp_decide left in the slot (final long before the tokens are)
  for (int r = 0; r < KVZ_MAX_LP_REFS; r++) {
    const bool on = cfg_.weightp && !sl.intra && sl.h_wp[3 * r] != 0;
    pw.flag[r] = on ? 1 : 0; pw.w[r] = (int16_t)(on ? sl.h_wp[3 * r + 1] : 64); pw.o[r] = (int16_t)(on ? sl.h_wp[3 * r + 2] : 0);
    out->wp[3 * r] = pw.flag[r]; out->wp[3 * r + 1] = pw.w[r]; out->wp[3 * r + 2] = pw.o[r];
  }
  bool assembled;
  { Tick tk; assembled = assemble_access_unit(out->au, sp_, sl.intra, sl.poc, sl.write_ps, rows_out, nsub, sl.qp - cfg_.qp, sl.nref ? &pr : nullptr, cfg_.weightp ? &pw : nullptr, recovery); const double a = tk.ms(); std::lock_guard<std::mutex> l(stat_m_); t_asm_ += a; }
  if (!assembled) { fprintf(stderr, "kvazzup_amd: %d substreams do not fit the tile grid\n", nsub); out->valid = false; return false; }
  out->recon_delivered = false;
  if (sl.has_sink) {                                       // the reconstruction's copy into the caller's picture: queued at submission, long done by now
    tl("rec0", sl.pic_idx);
    HIP_CHECK(hipEventSynchronize(sl.sink_done));
    tl("rec1", sl.pic_idx);
    sl.has_sink = false; out->recon_delivered = true;
  }
  if (cfg_.hash) {
    // decoded picture hash SEI: the picture's reconstruction (coded size, after the loop filters) comes down once more for it -- a
    // verification aid, not part of the hot path (uvgComm sets hash = none).  The ring entry is not written again before this picture is output.
    const size_t npx = (size_t)cw_ * ch_;
    std::vector<uint8_t> pic(npx * 3 / 2);
    const uint8_t *pl[3] = {pic.data(), pic.data() + npx, pic.data() + npx + npx / 4};
    const size_t pitch[3] = {(size_t)cw_, (size_t)cw_ / 2, (size_t)cw_ / 2};
    for (int c = 0; c < 3; c++) HIP_CHECK(hipMemcpy(const_cast<uint8_t *>(pl[c]), rec_[sl.rec_idx][c], c ? npx / 4 : npx, hipMemcpyDeviceToHost));
    const std::vector<uint8_t> payload = picture_hash_payload(cfg_.hash == 2 ? 0 : 2, pl, pitch, cw_, ch_);
    BitWriter sei;
    sei.put(132, 8); sei.put((uint32_t)payload.size(), 8);
    sei.bytes(payload.data(), payload.size());
    sei.trailing();
    append_nal(out->au, 40, sei.data().data(), sei.data().size());      // SUFFIX_SEI_NUT
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------------
// Band mode: this encoder codes CTU rows [row0, row0 + nrows) of every picture; its neighbours (other processes /
// GPUs) code the rest.  Everything up to deblocking is confined to the band by the tile rules; deblocking across the
// band's boundaries needs the neighbour's boundary rows, which arrive through the halo blocks.
// ---------------------------------------------------------------------------------------------------------------
bool Encoder::band_picture_setup()
{
  HIP_CHECK(hipSetDevice(cfg_.device));
  cur_slot_ = &slot_[0];
  prof_now_ = false;
  // rate control: every band's encoder runs the same controller on the same access-unit sizes (band_report_au), so all of them
  // arrive at the same QP without talking to each other
  if (cfg_.bitrate > 0 && frame_idx_ >= 3 && !(rc_known_ & (1u << ((frame_idx_ - 3) & 7)))) {
    fprintf(stderr, "kvazzup_amd: band mode with rate control: the size of access unit %d has not been reported (kvzx_encoder_band_report_au)\n", frame_idx_ - 3);
    return false;
  }
  const Plan p = plan(0);
  if (frame_idx_ >= 3) rc_known_ &= ~(1u << ((frame_idx_ - 3) & 7));
  band_f_ = picture_frame(p, slot_[0], 0);                 // (chain_gen: band_phase1)
  for (int c = 0; c < 3; c++) band_f_.sao_out[c] = nullptr;          // (no SAO in band mode)
  return true;
}

// band mode: the size of a finished access unit (picture index = count of pictures before it), for the rate controller
void Encoder::band_report_au(long picture, uint32_t bytes) { rc_bytes_[picture & 7] = bytes; rc_known_ |= 1u << (picture & 7); }

bool Encoder::band_phase1(const uint8_t *d_i420)
{
  if (cfg_.band_rows <= 0 || !d_i420) return false;
  if (!band_picture_setup()) return false;
  roi_sub_ = roi_; roi_sub_w_ = roi_w_; roi_sub_h_ = roi_h_;
  if (!stage_roi(stream_) || !picture_begin(band_f_, stream_)) return false;
  band_f_.chain_gen = next_chain_gen();                   // (drawn behind the picture's head: the clears of a wrap keep their place)
  const EncFrame &f = band_f_;
  launch_pad_input(d_i420, cfg_.width, cfg_.height, src_[0][0], src_[0][1], src_[0][2], cw_, ch_, stream_);
  if (f.is_intra) {
    launch_intra_analyse(f, stream_);
    HIP_CHECK(hipMemsetAsync(chain_.sync, 0, sizeof(uint32_t) * (rows_ * (cw_ / 64) * 3 + 1), stream_));
    HIP_CHECK(hipMemsetAsync(f.cu_cbf + (size_t)f.row0 * 8 * f.b8w, 0, (size_t)f.b8w * 8 * band_rows(f), stream_));
    launch_intra_recon(f, stream_);
  } else {
    launch_me(f, stream_);
    if (cfg_.subme > 0) launch_subpel(f, stream_);
    launch_inter_recon(f, stream_);
    launch_inter_signal(f, stream_);
  }
  launch_qp_resolve(f, stream_);
  if (cfg_.deblock) launch_deblock_v(f, stream_);
  HIP_CHECK(hipStreamSynchronize(stream_));
  return true;
}

// one halo block: [luma 4 rows | Cb 2 rows | Cr 2 rows | cu_log2 | cu_intra | cu_cbf (one 8x8 row each) | cu_mv (one 8x8 row)]
size_t Encoder::halo_bytes() const { return (size_t)cw_ * 4 + (size_t)(cw_ / 2) * 2 * 2 + (size_t)(cw_ / 8) * 3 + (size_t)(cw_ / 8) * 4; }

bool Encoder::band_export_halo(uint8_t *d_up, uint8_t *d_down)
{
  const EncFrame &f = band_f_;
  const int Y0 = f.row0 * 64, Y1 = (f.row0 + band_rows(f)) * 64, b8w = f.b8w, cw2 = cw_ / 2;
  for (int side = 0; side < 2; side++) {
    uint8_t *dst = side ? d_down : d_up;
    if (!dst) continue;
    const int y = side ? Y1 - 4 : Y0, b8y = side ? Y1 / 8 - 1 : Y0 / 8;        // first luma row of the 4-row strip; CU row
    size_t o = 0;
    HIP_CHECK(hipMemcpyAsync(dst + o, f.rec[0] + (size_t)y * cw_, (size_t)cw_ * 4, hipMemcpyDeviceToDevice, stream_)); o += (size_t)cw_ * 4;
    for (int c = 1; c < 3; c++) { HIP_CHECK(hipMemcpyAsync(dst + o, f.rec[c] + (size_t)(y / 2) * cw2, (size_t)cw2 * 2, hipMemcpyDeviceToDevice, stream_)); o += (size_t)cw2 * 2; }
    const uint8_t *arr[3] = {f.cu_log2, f.cu_intra, f.cu_cbf};
    for (int k = 0; k < 3; k++) { HIP_CHECK(hipMemcpyAsync(dst + o, arr[k] + (size_t)b8y * b8w, (size_t)b8w, hipMemcpyDeviceToDevice, stream_)); o += (size_t)b8w; }
    HIP_CHECK(hipMemcpyAsync(dst + o, f.cu_mv + (size_t)b8y * b8w * 2, (size_t)b8w * 4, hipMemcpyDeviceToDevice, stream_));
  }
  HIP_CHECK(hipStreamSynchronize(stream_));
  return true;
}

bool Encoder::band_import_halo(const uint8_t *d_from_up, const uint8_t *d_from_down)
{
  const EncFrame &f = band_f_;
  const int Y0 = f.row0 * 64, Y1 = (f.row0 + band_rows(f)) * 64, b8w = f.b8w, cw2 = cw_ / 2;
  for (int side = 0; side < 2; side++) {
    const uint8_t *src = side ? d_from_down : d_from_up;
    if (!src) continue;
    // from above: the neighbour's LAST rows land just above this band; from below: its FIRST rows just below
    const int y = side ? Y1 : Y0 - 4, b8y = side ? Y1 / 8 : Y0 / 8 - 1;
    if (y < 0 || y + 4 > ch_) return false;
    size_t o = 0;
    HIP_CHECK(hipMemcpyAsync(f.rec[0] + (size_t)y * cw_, src + o, (size_t)cw_ * 4, hipMemcpyDeviceToDevice, stream_)); o += (size_t)cw_ * 4;
    for (int c = 1; c < 3; c++) { HIP_CHECK(hipMemcpyAsync(f.rec[c] + (size_t)(y / 2) * cw2, src + o, (size_t)cw2 * 2, hipMemcpyDeviceToDevice, stream_)); o += (size_t)cw2 * 2; }
    uint8_t *arr[3] = {f.cu_log2, f.cu_intra, f.cu_cbf};
    for (int k = 0; k < 3; k++) { HIP_CHECK(hipMemcpyAsync(arr[k] + (size_t)b8y * b8w, src + o, (size_t)b8w, hipMemcpyDeviceToDevice, stream_)); o += (size_t)b8w; }
    HIP_CHECK(hipMemcpyAsync(f.cu_mv + (size_t)b8y * b8w * 2, src + o, (size_t)b8w * 4, hipMemcpyDeviceToDevice, stream_));
  }
  HIP_CHECK(hipStreamSynchronize(stream_));
  return true;
}

// Second phase in two halves, so that the halo exchange can run beside the first: (a) needs nothing from the neighbouring bands --
// the band's inner horizontal edges, the tokenizer, the host arithmetic coder (the tokens do not depend on deblocked samples) --
// and (b), after the halo rows have been imported, filters the two boundary edges and closes the picture.
bool Encoder::band_phase2a()
{
  if (cfg_.band_rows <= 0) return false;
  HIP_CHECK(hipSetDevice(cfg_.device));
  const EncFrame &f = band_f_;
  Slot &sl = slot_[0];
  if (cfg_.deblock) launch_deblock_h(f, stream_, 1);
  launch_tokenize(f, stream_); launch_tok_compact(f, stream_);
  HIP_CHECK(hipStreamSynchronize(stream_));
  if (*sl.h_err) { fprintf(stderr, "kvazzup_amd: device error flags 0x%x\n", *sl.h_err); return false; }
  const int wc = cw_ / 64;
  for (int i = f.row0 * wc; i < (f.row0 + band_rows(f)) * wc; i++) if (sl.h_tok_count[i] < 0) { fprintf(stderr, "kvazzup_amd: token array overflow (CTU %d)\n", i); return false; }
  band_bins_ = 0;
  entropy_->code_band(sl.h_tok_dense, sl.h_tok_count, sl.h_tok_off, wc, rows_, cfg_.wpp != 0, cfg_.tile_rows, f.is_intra ? 0 : 1, qp_cur_,
                      f.row0, band_rows(f), band_subs_, &band_bins_);
  band_coded_ = true;
  return true;
}

bool Encoder::band_phase2b(std::vector<std::vector<uint8_t>> *substreams, EncodedPicture *info)
{
  if (cfg_.band_rows <= 0 || !substreams || !band_coded_) return false;
  HIP_CHECK(hipSetDevice(cfg_.device));
  if (cfg_.deblock) { launch_deblock_h(band_f_, stream_, 2); HIP_CHECK(hipStreamSynchronize(stream_)); }
  substreams->swap(band_subs_);
  band_coded_ = false;
  if (info) { info->valid = true; info->poc = poc_; info->qp = qp_cur_; info->is_intra = band_f_.is_intra; info->bins = band_bins_; info->au.clear(); }
  frame_idx_++;
  if (band_f_.is_intra) intra_count_++;
  ref_idx_ = cur_idx_; cur_idx_ = (cur_idx_ + 1) % nrec_; out_idx_ = ref_idx_;
  return true;
}

bool Encoder::band_phase2(std::vector<std::vector<uint8_t>> *substreams, EncodedPicture *info) { return band_phase2a() && band_phase2b(substreams, info); }

// The picture last output: its reconstruction is complete (collect waited for the slot's events) and its ring entry is not written again
// before the next picture is submitted, so the copy goes on a stream of its own -- waiting on the main stream would wait for every
// picture queued behind this one (owf).
bool Encoder::download_recon(uint8_t *y, uint8_t *u, uint8_t *v)
{
  uint8_t *dst[3] = {y, u, v};
  HIP_CHECK(hipSetDevice(cfg_.device));
  if (!stream_rec_) HIP_CHECK(stream_acquire(&stream_rec_, cfg_.device, 'R', 'n'));
  if (pending() == 0) HIP_CHECK(hipStreamSynchronize(stream_));      // (band mode, debugging: nothing vouches for the picture but the main stream)
  for (int c = 0; c < 3; c++) {
    int w = c ? cfg_.width / 2 : cfg_.width, h = c ? cfg_.height / 2 : cfg_.height, pw = c ? cw_ / 2 : cw_;
    if (w == pw) HIP_CHECK(hipMemcpyAsync(dst[c], rec_[out_idx_][c], (size_t)w * h, hipMemcpyDeviceToHost, stream_rec_));
    else HIP_CHECK(hipMemcpy2DAsync(dst[c], (size_t)w, rec_[out_idx_][c], (size_t)pw, (size_t)w, (size_t)h, hipMemcpyDeviceToHost, stream_rec_));
  }
  HIP_CHECK(hipStreamSynchronize(stream_rec_));
  return true;
}

bool Encoder::debug_copy(const char *what, void *dst, size_t bytes)
{
  const void *src = nullptr; size_t have = 0;
  std::string w(what);
  static const char *names[7] = {"cu_log2", "cu_intra", "cu_flags", "cu_merge_idx", "cu_mvp_idx", "cu_intra_mode", "cu_cbf"};
  for (int i = 0; i < 7; i++) if (w == names[i]) { src = cu_bytes_[out_set_] + lay_.cu_off(i); have = lay_.nb8; }
  if (w == "lp_gop") { if (bytes > sizeof(out_gop_)) return false; memcpy(dst, out_gop_, bytes); return true; }      // (host values: no copy from the device)
  if (w == "ir") { if (!cfg_.intra_refresh || bytes > sizeof(out_ir_)) return false; memcpy(dst, out_ir_, bytes); return true; }      // (host values)
  if (w == "wp") { if (!cfg_.weightp || bytes > sizeof(out_wp_)) return false; memcpy(dst, out_wp_, bytes); return true; }      // (host values, as the slice headers said them)
  if (w == "scenecut") { if (!cfg_.scenecut || bytes > sizeof(out_sc_)) return false; memcpy(dst, out_sc_, bytes); return true; }      // (host values, as submit() read or wrote them)
  if (w == "fb") { if (!cfg_.loss_feedback || bytes > sizeof(out_fb_)) return false; memcpy(dst, out_fb_, bytes); return true; }      // (host values)
  if (w == "fb_anchor") { if (!cfg_.fb_anchor || bytes > sizeof(out_fba_)) return false; memcpy(dst, out_fba_, bytes); return true; }      // (host values)
  if (w == "fb_map" && fb_map_) { src = fb_map_; have = lay_.nb8; }      // (the heal picture last submitted: a synchronous copy, behind its kernels)
  if (w == "fb_blk" && fb_blk_) { src = fb_blk_; have = lay_.nb8 / 16 * 2; }
  if (w == "sc_blocks" && sc_blocks_) { src = sc_blocks_; have = lay_.sc_blocks * sizeof(uint32_t); }      // (the picture last examined: its kernels are done, submit() waited for them)
  if (w == "cu_mv") { src = cu_mv_[out_set_]; have = lay_.cu_mv * sizeof(int16_t); }
  if (w == "cu_mvd") { src = cu_mvd_[out_set_]; have = lay_.cu_mv * sizeof(int16_t); }
  if (w == "cu_ref") { src = cu_ref_[out_set_]; have = cu_ref_[out_set_] ? lay_.nb8 : 0; }
  if (w == "me_coarse") { src = mc_centres_[out_set_]; have = mc_centres_[out_set_] ? lay_.mc_centres * sizeof(int16_t) : 0; }
  if (w == "col") { src = col_[out_set_]; have = col_[out_set_] ? lay_.col * sizeof(ColMv) : 0; }
  if (w == "trace" && trace_) { src = trace_; have = lay_.trace * sizeof(unsigned long long); }
  for (int c = 0; c < 3; c++) {
    size_t n = lay_.plane(c);
    if (w == std::string("coef") + char('0' + c)) { src = coef_[out_set_][c]; have = n * 2; }
    if (w == std::string("rec") + char('0' + c)) { src = rec_[out_idx_][c]; have = n; }
    if (w == std::string("src") + char('0' + c)) { src = src_[out_set_][c]; have = n; }
  }
  if (!src || bytes > have) return false;
  HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return true;
}

}  // namespace kvzx
