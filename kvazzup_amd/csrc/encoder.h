// kvazzup_amd/csrc/encoder.h -- host engine of the HIP encoder: owns the device buffers and the
// HIP stream, runs the per-picture kernel pipeline and assembles the access unit.
// This is what sits behind kvz_api->encoder_open / encoder_encode / encoder_close
// (/root/reference/src/media/processing/kvazaarfilter.cpp:291,435-448,317).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "hevc_core.h"
#include "hevc_headers.h"
#include "entropy_host.h"
#include "enc_kernels.h"
#include "input_kernels.h"
#include "enc_layout.h"
#include "hip_owner.h"

namespace kvzx {

// K_HOST_ARITH is not a kernel: wall time of the host arithmetic-coding stage (entropy_host.h)
enum KernelId { K_PAD = 0, K_ME, K_INTER_RECON, K_INTER_SIGNAL, K_INTRA_ANALYSE, K_INTRA_RECON, K_DEBLOCK, K_TOKENIZE, K_HOST_ARITH, K_SAO, K_TOK_COMPACT, K_CABAC_ROWS, K_SUBPEL, K_INTRA_ANALYSE_P, K_INTRA_RECON_P, K_COUNT };      // (.._P: the intra units of a P picture, intra-in-p)

struct EncoderConfig {
  int width = 0, height = 0;
  int qp = 32, intra_period = 64, vps_period = 1;
  int me_range = 16;
  int fps_num = 30, fps_den = 1;
  int wpp = 1, deblock = 1;
  // Tile-row split of one picture over several encoder instances (one per GPU): this instance codes CTU
  // rows [band_row0, band_row0 + band_rows) only -- whole tiles -- through band_phase1 / halo exchange / band_phase2.
  int band_row0 = 0, band_rows = 0;   // band_rows == 0: the whole picture (normal operation)
  int tile_rows = 1;          // tile rows (kvazaar "tiles" CxR: R), uniform spacing, loop filter across tiles on
  int tile_cols = 1;          // tile columns (C); band mode needs 1
  int device = 0;
  int entropy_threads = 16;   // host threads of the arithmetic-coding stage
  int qp_in_cu = 0;           // kvazaar "set-qp-in-cu": cu_qp_delta_enabled_flag; a delta-QP map (set_roi, kvz_picture.roi) then gives every CTU its own QP
  int bitrate = 0;            // bits per second; 0 = constant QP, > 0 = "uvgx rate control v1" (oracle/hevc_enc.c rate_control())
  int slices = 0;             // kvazaar "slices": 1 = wpp (a dependent slice segment per CTU row; needs wpp), 2 = tiles (an independent slice per tile); one NAL unit per segment
  int lossless = 0;           // kvz_config.lossless: cu_transquant_bypass in every coding unit (no deblocking, SAO, RDOQ, sign hiding or rate control with it)
  int rc_bands = 0;           // with bitrate > 0: "uvgx rate control v2" -- a P picture's CTU rows are reconstructed in this many groups and the QP follows the level cost
                              // between them, on the device (rc_kernels.hip; statement rc_band_decide() in oracle/hevc_enc.c); 0 = picture level only (v1); implies qp_in_cu
  int satd = 1;               // intra mode search cost: 8x8 Hadamard sums (1) or SAD (0)
  int subme = 0;              // kvazaar "subme" 0..4: fractional-sample refinement of the searched vectors, "uvgx subme v1" (oracle/hevc_enc.c subme_refine())
  int me_early = 1;           // kvazaar "me-early-termination" (on / sensitive: 1, off: 0): static 32x32 blocks skip the motion search
  int vaq = 0;                // kvazaar "vaq" 1..20: "uvgx VAQ v1" (oracle/hevc_enc.c vaq_deltas()); implies qp_in_cu
  int mv_frame = 0;           // kvazaar "mv-constraint" frame / frametile (1), frametilemargin (2): vectors keep the block inside the picture
  int sao = 0;                // kvazaar "sao": sample adaptive offset, parameters by "uvgx SAO decision v1" (oracle/hevc_sao.c)
  int input_hold = 0;         // "input-hold" (extension): 1 = the caller leaves a DEVICE input picture unchanged until that picture's access unit has been returned --
                              // what the kvz_api contract already demands of host pictures (kvazaarfilter.cpp:76-88); encode_device then returns without waiting for the input stage
  int intra_chain = 1;        // "intra-chain": left-edge blocks / the above-right corner block of a CTU keep to the modes that do not read the neighbouring CTU's below-left / above-right samples (oracle/hevc_enc.c intra_analyse_size)
  int scaling_list = 0;       // kvazaar "scaling-list default": scaling_list_enabled_flag with the default lists (oracle/hevc_scaling.c); quantiser scale per position (qscale << 4) / m
  int rdoq = 0;               // kvazaar "rdoq": "uvgx RDOQ v1" -- sparse high-frequency coefficient groups are dropped when that is cheaper (oracle/hevc_transform.h orc_adjust_levels)
  int intra_in_p = 0;         // "intra-in-p" 0 / 1 (16x16 units only) / 2 (16x16 and 8x8): intra coding units in P pictures ("uvgx intra-in-P v1", oracle/hevc_enc.c me_block32); not in band mode
  int me_source = 0;          // "me-source" ("uvgx search pipelining v1", oracle/hevc_enc.c build_refpad): the integer search looks at the previous input picture; k_me (and k_intra_analyse<P>) of picture t + 1 then run on the input stream beside picture t's chain; not in band mode
  int signhide = 0;           // kvazaar "signhide": sign_data_hiding_enabled_flag; the quantiser makes the parity of every eligible coefficient group say the hidden sign
  int hash = 0;               // kvazaar "hash": 1 checksum, 2 md5 -- a decoded picture hash SEI (D.2.19) behind every picture's slices, from the reconstruction downloaded for it
  int entropy_gpu = 0;        // arithmetic coder: 1 = on the GPU (k_cabac_rows, cabac_kernels.hip), 0 = host thread pool (entropy_host.h); band mode always uses the host pool
  int lp_refs = 1;            // "lp-refs" (extension, "uvgx multi-reference v1"): references per P picture, 1..4 -- picture t refers to pictures
                              // t - 1 .. t - min(lp_refs, pictures since the IDR picture), all in list 0 (with lp_gop: the same count, chosen as lp_gop says); 1 = one reference (the encoder of before); not in band mode
  int me_coarse = 0;          // "me-coarse" (extension, "uvgx coarse-to-fine search v1"): 0 / 64 / 128 / 256 -- reach in full samples of the coarse search on quarter-resolution input pictures whose centres give k_me a second window; 0 = off (nothing allocated, nothing launched); not in band mode
  int lp_gop = 0;             // "lp-gop" (extension, "uvgx low-delay GOP v1"; statement of record: tests/lp_gop_model.py): 1 = the low-delay structure of
                              // gop=lp-g<gop_g>d<gop_d>t1 -- every gop_g-th picture after the IDR picture a key picture, P pictures at QP + layer (1 .. gop_d), and references
                              // that are the previous picture, the most recent key picture within kMaxRefDist pictures, then the pictures before (lp_refs in all); without effect
                              // while gop_g == 0 (no gop string, or gop=0); not in band mode, not with gop_t > 1 or gop_d > 6
  int gop_g = 0, gop_d = 1, gop_t = 1;   // the numbers of the gop string (kvz_config.gop_len, gop_lp_ref_depth, gop_lp_temporal_layers)
  int tmvp = 0;               // kvazaar "tmvp" (DESIGN.md section 9b): temporal motion vector prediction -- merge / AMVP candidates from the previous picture's motion
                              // (collocated_ref_idx 0); changes the signalling only, never the motion chosen; not in band mode
  int weightp = 0;            // "weightp" (extension, "uvgx weighted prediction v1"; restated in tests/wp_model.py): 1 = explicit weighted prediction of luma --
                              // per P picture and reference a weight and an offset from the two INPUT pictures' luma statistics, kept when a check on every fourth sample says
                              // they pay; the integer search reads weighted copies of its reference planes, k_subpel and k_inter_recon predict with the weights, the slice
                              // headers carry pred_weight_table(); 0 = off (nothing allocated, nothing launched); not in band mode, not with lossless
  int intra_refresh = 0;      // "intra-refresh" N (extension, "uvgx intra refresh v1"; restated in tests/ir_model.py): 0 = off; 2 .. 255 = a band of intra
                              // units walks across every P picture, one step a picture and at most N pictures a pass, and the blocks it has passed keep their vectors out of
                              // what it has not -- after one pass a decoder that lost a picture has the encoder's pictures again, without an IDR picture.  The first picture
                              // of a cycle carries a recovery point SEI.  Not with lp-refs >= 2, lp-gop, tmvp, me-coarse, tiles, band mode, lossless or intra-chain=0
  int scenecut = 0;           // "scenecut" N (extension, "uvgx scene cut v1"; restated in tests/scenecut_model.py): 0 = off; 1 .. 255 = an input picture
                              // at least N pictures behind the last IDR picture is compared with the previous input picture on their quarter pictures (mean shift, then per
                              // 8x8 block the best match against the block's own activity); when more than half of the blocks are new the picture is an IDR picture and
                              // the period counts from it.  The one option whose decision the host waits for: submit() of an examined picture waits for k_sc_decide on
                              // the input stream before it plans the picture.  Not in band mode
  int input_format = 0;       // "input-format" (extension; enum kvz_input_format): 0 = I420 pictures (the encoder of before); rgb32 / rgb32-sse41 / yuyv = PACKED pictures
                              // (encode_packed_host / _device), converted with the reference's arithmetic in the input stage -- k_input_rgb32 / k_input_yuyv (input_kernels.hip)
                              // write the working set's padded planes in k_pad_input's place, and everything behind them is as ever.  Not with input-hold, not in band mode
  int loss_feedback = 0;      // "loss-feedback" H (extension, "uvgx loss feedback v1"; statement of record: tests/fb_model.py): 0 = off; 1 .. 64 = the encoder
                              // keeps the motion records of its last H pictures and takes the receiver's loss reports (report_damage): the picture behind a report is a
                              // HEAL PICTURE -- a P picture whose 16x16 quarters are intra units wherever the reported error may have travelled along the motion since,
                              // and whose other blocks keep their vectors out of it; it carries a recovery point SEI.  Without a report no picture changes.  Not with
                              // lp-refs >= 2, lp-gop, tmvp, me-coarse, tiles, band mode, lossless, intra-chain=0 or intra-refresh
  int fb_anchor = 0;          // "fb-anchor" K (extension, "uvgx loss feedback v2"; statement of record: tests/fb_anchor_model.py): 0 = off; 2 .. 7 beside
                              // loss-feedback = H >= K: every P picture's slice header lists the K pictures before it, so that every decoder keeps them, and the ring of
                              // reconstructions keeps them too; a heal picture whose oldest report names picture n0 is then a V2 HEAL PICTURE when the anchor a = n0 - 1
                              // is at most K pictures back and not in front of the last IDR or heal picture: two references, the previous picture and the anchor, the
                              // quarters the error may have reached predicted from the anchor where v1 codes them as intra units.  Otherwise the heal picture is v1's.
                              // Not with weightp, K + 1 > MaxDpbSize of the coded size, and whatever loss-feedback refuses
  int owf = 0;                // kvazaar "owf": 0 = encode() returns its own picture; 1 = output lags one picture and the host
                              // coding of picture t overlaps the kernels of t + 1; >= 2 = output lags two pictures and the host
                              // coding runs on a background thread, so the calling thread only launches kernels
};

struct EncodedPicture {
  bool valid = false;         // false: nothing was output by this call (pipeline filling, owf >= 1)
  std::vector<uint8_t> au;
  int poc = 0, qp = 0; bool is_intra = false;
  int layer = 0, nref = 0; int8_t dist[KVZ_MAX_LP_REFS] = {0, 0, 0, 0};   // lp-gop, a P picture: its QP layer and its references' POC distances in list 0 order (nref 0: the option is off)
  int32_t wp[3 * KVZ_MAX_LP_REFS] = {0, 64, 0, 0, 64, 0, 0, 64, 0, 0, 64, 0};   // weightp: the picture's record [reference][flag, w, o]
  int32_t sc[5] = {0, 0, 0, 0, 0};  // scenecut: the picture's record {examined, n_new, n_b, d, cut}
  int32_t ir[4] = {-1, 0, 0, 0};  // intra-refresh: position j in the cycle (-1: an IDR picture, or the option is off), the band [s_j, e_j), the cycle's length n
  int32_t fb[4] = {0, 0, 0, 0};   // loss-feedback: {heal picture, reports folded into it, damaged cells of its map, forced quarters}
  int32_t fba[4] = {0, 0, 0, 0};  // fb-anchor: {v2 heal picture, the anchor's POC, its distance da, quarters coded from reference 1}
  uint64_t bins = 0;
  bool recon_delivered = false;   // the reconstruction has been copied into the planes given to set_recon_sink
};

// the arrays of one intra chain (Encoder::chain_, chain_idr_); work, SAO on: the picture up to deblocking (rec_[] then holds the filtered pictures)
struct EncChain { uint32_t *sync = nullptr, *edge_col = nullptr; unsigned long long *edge_row = nullptr; uint8_t *work[3] = {nullptr, nullptr, nullptr}; };

class Encoder {
 public:
  static Encoder *create(const EncoderConfig &cfg, std::string *error);
  ~Encoder();
  // picture as three host planes (stride = width).  pinned: the three planes lie back to back in page-locked memory (a kvz_picture from
  // picture_alloc) that the caller leaves alone until this picture's access unit has been returned (the kvz_api contract,
  // kvazaarfilter.cpp:76-88): the upload then reads the caller's picture itself, without a staging copy
  bool encode_host(const uint8_t *y, const uint8_t *u, const uint8_t *v, EncodedPicture *out, bool pinned = false);
  // picture as packed I420 in device memory (w*h*3/2 bytes)
  bool encode_device(const uint8_t *d_i420, EncodedPicture *out);
  // input-format other than i420: the picture as ONE packed block (input_bytes() long) in host / device memory; the I420 calls above fail on such an
  // encoder and these fail on an I420 encoder.  pinned: page-locked and left alone until the access unit has been returned, as for encode_host
  bool encode_packed_host(const uint8_t *packed, EncodedPicture *out, bool pinned = false);
  bool encode_packed_device(const uint8_t *d_packed, EncodedPicture *out);
  size_t input_bytes() const;            // bytes of one input picture in the encoder's format
  // owf >= 1: outputs the picture still in flight, if any (kvz_api encoder_encode with pic_in == NULL)
  bool flush(EncodedPicture *out);
  // like flush, but never waits: outputs the oldest picture in flight only if it has already been finished
  bool poll(EncodedPicture *out);
  // delta-QP map for the following pictures (kvz_picture.roi, kvazaarfilter.cpp:423-431): w x h int8 cells spread uniformly over
  // the picture, clamped to [-12, 12]; w == 0 removes it.  Needs cfg.qp_in_cu.  Statement: roi_targets() in oracle/hevc_enc.c.
  void set_roi(int w, int h, const int8_t *map);
  // loss-feedback: the receiver lost `count` coding tree blocks (64x64, raster order of the coded picture) from `first_ctb` of the most recently coded picture
  // with this POC; count <= 0: the whole picture.  1: accepted -- the next picture handed in is the heal picture (several reports fold into one); 2: void, an
  // IDR picture has been coded since; 0: refused (option off, range outside the picture).  A report older than H pictures counts as "everything damaged".
  // May be called from the thread that calls encode_*, between any two of its calls.
  int report_damage(int32_t poc, int first_ctb, int count);
  // ---- band mode (cfg.band_rows > 0); every call is synchronous.  Per picture: band_phase1, export the halos, exchange them
  // with the neighbouring bands' encoders (rank - 1 gets `up`, rank + 1 gets `down`), import theirs, band_phase2.
  void band_report_au(long picture, uint32_t bytes);              // rate control in band mode: size of the assembled access unit of picture `picture` (every band's encoder is told; needed before picture + 3 starts)
  bool band_phase1(const uint8_t *d_i420);                       // input, decisions, reconstruction, vertical-edge deblocking of the band
  size_t halo_bytes() const;                                     // size of one halo block
  bool band_export_halo(uint8_t *d_up, uint8_t *d_down);         // the band's first / last 4 luma + 2 x 2 chroma rows (vertical edges filtered) and CU records of its first / last 8x8 row
  bool band_import_halo(const uint8_t *d_from_up, const uint8_t *d_from_down);   // nullptr: no neighbour on that side
  // horizontal-edge deblocking (boundary edges included), tokenizer, arithmetic coding: one substream per CTU row (WPP) or tile of the band
  bool band_phase2(std::vector<std::vector<uint8_t>> *substreams, EncodedPicture *info);      // = band_phase2a + band_phase2b
  bool band_phase2a();                                            // what needs no halo: inner horizontal edges, tokenizer, arithmetic coder (may run beside the exchange, BEFORE band_import_halo)
  bool band_phase2b(std::vector<std::vector<uint8_t>> *substreams, EncodedPicture *info);     // after band_import_halo: the band's two boundary edges; hands out the substreams
  int rc_delay() const { return rc_delay_; }
  int pending() const { return (int)(accepted_ - collected_); }
  // pictures taken from the caller / pictures whose turn to be returned has come (also when collecting one FAILED): what the C ABI pairs its queues of source and
  // reconstruction pictures with (kvz_api.hip encoder_encode)
  long accepted_count() const { return accepted_; }
  long collected_count() const { return collected_; }
  // cropped reconstruction of the last coded picture -> host planes (stride = width)
  bool download_recon(uint8_t *y, uint8_t *u, uint8_t *v);
  // Where the reconstruction of the NEXT picture handed to encode_host goes (page-locked planes, width x height dense; kvz_api's pic_out): the copy is
  // queued behind the picture's chain when the picture is submitted and runs beside its tokenizer and arithmetic coder -- collect() returns when both
  // are done -- instead of as a synchronous download after the access unit is finished (0.13 ms of a 0.52 ms encoding delay at 1080p, 0.5 of 4.7 at 4K
  // with uvgComm's default OWF 0).  Call before encode_host; nullptr: no copy.
  void set_recon_sink(uint8_t *y, uint8_t *u, uint8_t *v) { sink_[0] = y; sink_[1] = u; sink_[2] = v; }
  // debug: copy an internal device array of the last coded picture to the host
  //   "cu_log2","cu_intra","cu_flags","cu_merge_idx","cu_mvp_idx","cu_intra_mode","cu_cbf" (b8 bytes),
  //   "lp_gop" (host values, 8 int32: option active, layer, QP, number of references, their four POC distances),
  //   "wp" (weightp; host values, 12 int32: [reference][flag, w, o] as the picture's slice headers say them -- an intra picture: 0, 64, 0 throughout),
  //   "ir" (intra-refresh; host values, 4 int32: position j in the cycle, the band's s_j and e_j, the cycle's length n -- an IDR picture: -1, 0, 0, n),
  //   "scenecut" (scenecut; 5 int32: the record {examined, n_new, n_b, d, cut} of the picture last output -- a picture that was not examined: 0, 0, n_b, 0, 0),
  //   "sc_blocks" (scenecut; n_b pairs of uint32: (S, A) of every block of the picture last EXAMINED, raster order),
  //   "fb" (loss-feedback; host values, 4 int32: {heal picture, reports folded, damaged cells, forced quarters} of the picture last output),
  //   "fb_anchor" (fb-anchor; host values, 4 int32: {v2 heal picture, the anchor's POC, its distance da, quarters coded from reference 1} of the picture last output),
  //   "fb_map" (loss-feedback; the map D' of the heal picture last submitted, one byte a cell), "fb_blk" (... its block records, two bytes per 32x32 block),
  //   "cu_mv" (b8 * 2 int16), "coef0..2" (int16 planes), "rec0..2" (coded planes), "src0..2", "col" (tmvp, a P picture: its collocated record, ColMv per 16x16), "me_coarse" (me-coarse, a P picture: the centres, int16 pairs [reference][32x32 block])
  bool debug_copy(const char *what, void *dst, size_t bytes);
  int coded_width() const { return cw_; }
  int coded_height() const { return ch_; }
  const EncoderConfig &config() const { return cfg_; }
  // every = 0: off; 1: every picture; n: every n-th picture (sampling keeps the event overhead out of the throughput)
  void set_profiling(int every) { profiling_ = every > 0; prof_every_ = every > 0 ? every : 1; }
  // accumulated kernel time (ms) and launch count per KernelId since the last reset
  void get_kernel_times(double *ms, uint64_t *launches, bool reset);
  const uint8_t *device_recon(int plane) const { return rec_[out_idx_][plane]; }   // picture last output
  hipStream_t stream() const { return stream_; }

 private:
  Encoder() {}
  bool init(const EncoderConfig &cfg, std::string *error);
  bool submit(const uint8_t *d_i420, int in_ring);   // in_ring >= 0: the picture is being uploaded into d_in_[in_ring] (encode_host)
  bool collect(EncodedPicture *out);
  struct Slot;
  // submit() in stages: plan (sets set_, POC, rate control), the picture's frame, then the input stage, its chain and the hand-off, in this order
  // side: the chain on stream_idr_; ahead: me-source search on the input stream; ms: the chain's stream; qp: the picture's QP (rate control's, plus the layer with
  // lp-gop); nref / dist: its references in list 0 order, dist[k] pictures back (k + 1 without lp-gop); layer: lp-gop's QP layer of a P picture, else 0
  struct Plan { bool intra = false, side = false, ahead = false; hipStream_t ms = nullptr; int qp = 0, layer = 0, nref = 1; int8_t dist[KVZ_MAX_LP_REFS] = {1, 2, 3, 4};
                int ir_j = -1, ir_s = 0, ir_e = 0;      // intra-refresh: the P picture's position in the cycle and its band (ir_e 0: none)
                bool fb = false;                        // loss-feedback: a heal picture (fb_heal_ has its reports)
                int fb_da = 0; };                       // fb-anchor: a v2 heal picture -- its anchor lies fb_da pictures back and is reference 1 (0: not one)
  bool gop_on() const { return cfg_.lp_gop && cfg_.gop_g >= 1; }
  bool sl_gop_timeline(const Plan &p) const { return gop_on() && !p.intra && Timeline::get().path; }
  Plan plan(int set);
  EncFrame picture_frame(const Plan &p, const Slot &sl, uint32_t chain_gen) const;
  bool input_stage(const EncFrame &f, const Plan &p, const uint8_t *d_i420, int in_ring);
  bool chain_stage(const EncFrame &f, const Plan &p);
  bool hand_off(const EncFrame &f, const Plan &p, Slot &sl, int in_ring);
  bool finish_slot(Slot &sl, EncodedPicture *out, int worker = 0);   // wait for the slot's kernels, arithmetic coding, access unit
  void background(int worker);
  void timed(KernelId id, hipStream_t st, const std::function<void()> &launch);

  EncoderConfig cfg_;
  int cw_ = 0, ch_ = 0, rows_ = 0;
  EncLayout lay_;                        // how long the arrays are and where their parts lie (enc_layout.h); cw_, ch_, rows_ are its
  HipOwner mem_;                         // every array and event below is a view of what it holds (init and the lazy sites); ~Encoder releases it explicitly, behind the last wait and in front of the streams' release
  hipStream_t stream_ = nullptr;
  EncFrame base_{};                      // what does not change from picture to picture: geometry, options, scratch, tokenizer buffers, the main chain's arrays (written by init only)
  // Host pictures (kvz_api->encoder_encode, kvazaarfilter.cpp:435-438): a ring of packed device buffers filled by the copy engine ahead of
  // each picture's input stage -- picture t + 1 travels over PCIe while the kernels of picture t run -- and, for callers whose planes are not
  // page-locked, a ring of pinned staging buffers (allocated on first use).  kInRing entries: more than the pictures that can be in flight
  // (owf <= kMaxDepth plus the submitter's hand), so a copy never waits in the copy engine's queue for its buffer's previous reader.
  static constexpr int kInRing = 20;
  uint8_t *d_in_[kInRing] = {};          // packed input (device)
  uint8_t *h_in_[kInRing] = {};          // pinned host staging
  hipEvent_t ev_h2d_[kInRing] = {}, ev_pad_[kInRing] = {}; bool pad_pending_[kInRing] = {}, h2d_pending_[kInRing] = {};
  long in_count_ = 0;
  hipStream_t stream_rec_ = nullptr;     // download of reconstructions the caller asks for (encoder_encode's pic_out)
  // Per-picture working sets (padded source planes, level planes, CU arrays, per-CTU QP arrays, SAO parameters): kSets of them take turns, so the
  // host can queue kSets - 1 pictures' kernels ahead of the one the GPU is working on without waiting for a set to come free (with two sets
  // the input stage of picture t waited for the reconstruction of t - 2, and the calling thread with it: the main stream ran dry between pictures)
  static constexpr int kSets = 8;
  uint8_t *src_[kSets][3] = {};         // padded source planes
  // reconstruction ring: the picture being coded, its reference(s) (lp-refs; lp-gop: every picture a later one may still refer to), and (owf >= 2) the one still waiting to be output
  static constexpr int kMaxDepth = 16;    // pictures in flight behind the one being submitted (owf), at most
  static constexpr int kMaxRefDist = kSets - 1;   // lp-gop: the oldest picture a P picture refers to -- its input picture, quarter picture and collocated record are still in a working set
  static constexpr int kRecRing = kMaxDepth + 2 + kMaxRefDist;
  uint8_t *rec_[kRecRing][3] = {};
  bool spin_wait_ = false;      // KVAZZUP_AMD_SPIN: poll the GPU instead of napping between queries
  int rc_delay_ = 3;            // rate control: pictures between a picture and the access unit size booked before it (3 .. 7)
  int nrec_ = 3;                // reconstruction ring: the picture being written, its reference, and the ones whose output is still owed (owf)
  int cur_idx_ = 0, ref_idx_ = 2, out_idx_ = 2;
  // What the tokenizer reads (levels and CU records) is the working set's too: picture t is tokenised on the second stream
  // from its set while the kernels of the pictures behind it fill the others.
  int16_t *coef_[kSets][3] = {};
  uint8_t *cu_bytes_[kSets] = {};          // 7 byte arrays back to back (EncLayout::cu_off)
  int16_t *cu_mv_[kSets] = {}, *cu_mvd_[kSets] = {};
  uint8_t *cu_ref_[kSets] = {};            // lp-refs >= 2: ref_idx_l0 per 8x8 block (EncFrame::cu_ref)
  uint8_t *mc_q_[kSets] = {}; int16_t *mc_centres_[kSets] = {};      // me-coarse (the quarter picture: also scenecut): the quarter picture of the set's input picture and the centres of the set's picture [reference][32x32 block] (EncFrame::mc_*)
  ColMv *col_[kSets] = {};                 // tmvp: the collocated record of the set's picture (EncFrame::col_out), which the next picture reads (col_prev)
  int set_ = 0, out_set_ = 0;
  int32_t out_gop_[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // debug_copy("lp_gop") of the picture last output
  int32_t out_ir_[4] = {-1, 0, 0, 0};               // debug_copy("ir") of the picture last output
  bool ir_free_ = true;                             // intra-refresh with intra-in-p=0: false -- the intra-in-P stages run for the band alone
  // loss-feedback (fb_kernels.hip): the ring of the last H pictures' records (picture i in place i % H), the map and its scratch, the heal picture's block
  // records; the reports wait in fb_q_ (under fbm_) until plan() takes them for the next P picture (fb_heal_) or an IDR picture voids them
  struct FbReport { int32_t poc; int first, count; };
  int16_t *fb_rec_mv_ = nullptr; uint8_t *fb_rec_info_ = nullptr, *fb_map_ = nullptr, *fb_tmp_ = nullptr, *fb_blk_ = nullptr;
  std::mutex fbm_; std::vector<FbReport> fb_q_, fb_heal_;
  hipEvent_t ev_fb_me_ = nullptr;                   // me-source: behind a heal picture's search on the main stream, which reads the previous input picture; the input stream waits for it
  int32_t out_fb_[4] = {0, 0, 0, 0};                // debug_copy("fb") of the picture last output
  // fb-anchor: the clean point c -- the POC of the most recent IDR or heal picture --, and per place of the ring the anchor's POC of the v2 heal picture filed
  // there (-1: the record holds no reference-1 cell)
  int fb_clean_ = 0; std::vector<int> fb_rec_anchor_;
  int32_t out_fba_[4] = {0, 0, 0, 0};               // debug_copy("fb_anchor") of the picture last output
  bool fb_stage(const EncFrame &f, const Plan &p, Slot &sl);   // main stream, in front of a heal picture's search: seeds, steps, block records
  // weightp (wp_kernels.hip): per working set the input picture's partial sums, its moments {m, v} and the picture's record; one set of scratch (candidates, the
  // check's sums) and of search planes -- their writers and readers follow one another on one stream (the input stream; the planes without me-source: the main stream)
  unsigned long long *wp_partial_[kSets] = {}; int64_t *wp_stat_[kSets] = {}; int32_t *wp_rec_[kSets] = {};
  int32_t *wp_cand_ = nullptr; unsigned long long *wp_acc_ = nullptr; uint8_t *wp_plane_[KVZ_MAX_LP_REFS] = {};
  int32_t out_wp_[3 * KVZ_MAX_LP_REFS] = {0, 64, 0, 0, 64, 0, 0, 64, 0, 0, 64, 0};   // debug_copy("wp") of the picture last output
  bool wp_stage(const EncFrame &f, const Plan &p, const Slot &sl);   // input stream: statistics of the picture; a P picture: candidates, check, record
  EncFrame wp_search_frame(const EncFrame &f, const Plan &p, hipStream_t st);   // the search planes of f's references built on `st`; returns f with me_ref / me_refs pointing at them
  // scenecut (sc_kernels.hip): per working set the sum over the input picture's visible quarter samples (its quarter picture is mc_q_, me-coarse's); one array of
  // (S, A) pairs, one counter and one device record -- an examination is over, the host has waited for it, before the next one is queued
  unsigned long long *sc_sum_[kSets] = {}; uint32_t *sc_blocks_ = nullptr, *sc_count_ = nullptr; int32_t *sc_rec_ = nullptr; hipEvent_t ev_sc_ = nullptr;
  bool sc_cut_ = false;                             // the verdict on the picture being submitted (sc_stage), read by plan()
  int32_t out_sc_[5] = {0, 0, 0, 0, 0};             // debug_copy("scenecut") of the picture last output
  bool pad_stage(int set, const uint8_t *d_i420, int in_ring);   // input stream: the picture padded into the set, its quarter picture (me-coarse, scenecut)
  bool sc_stage(int set, const uint8_t *d_i420, int in_ring);    // pad_stage, the picture's sum; an examined picture: blocks, record, and the wait for it -- before plan()
  bool wait_event(hipEvent_t e);                    // on the host, as finish_slot waits: naps between queries in a pipelined encoder, polling with KVAZZUP_AMD_SPIN
  char prio_[3] = {'h', 'n', 'n'};                      // priority levels of the main, tokenizer and input streams (stream_pool.h keys)
  std::vector<int8_t> roi_; int roi_w_ = 0, roi_h_ = 0;           // as set by the caller (set_roi)
  std::vector<int8_t> roi_sub_; int roi_sub_w_ = 0, roi_sub_h_ = 0;   // the map of the picture being submitted (it travels with the picture to the submitter thread)
  int8_t *ctu_qt_[kSets] = {}, *ctu_qy_[kSets] = {}, *ctu_delta_[kSets] = {}; uint8_t *ctu_first_[kSets] = {};   // per set
  int8_t *h_ctu_qt_[kSets] = {};   // pinned staging of the picture's ROI deltas, one per CTU
  int8_t *ctu_roi_[kSets] = {};    // ... and their device copies (uploaded on the input stream when the picture brings a map)
  bool stage_roi(hipStream_t st);  // the picture's ROI deltas -> ctu_roi_[set_] on `st`; roi_dev_ = that array or NULL (no map)
  const int8_t *roi_dev_ = nullptr;
  int *vaq_act_ = nullptr, *vaq_sum_ = nullptr; // VAQ: activity of every CTU, its sum over the picture
  uint32_t next_chain_gen();
  bool picture_begin(const EncFrame &f, hipStream_t qt_stream, EncFrame *fold = nullptr, bool zero = false);     // fold: a P picture without VAQ -- the work rides in the picture's k_me launch (EncFrame::pb_*) instead of a launch of its own   // launch_picture_begin: the rate control state on the main stream (picture order), the per-CTU targets on the picture's own stream (+ the VAQ kernels)
  int qp_cur_ = 0; int64_t rc_debt_ = 0; uint32_t rc_bytes_[8] = {0, 0, 0, 0, 0, 0, 0, 0}; uint32_t rc_known_ = 0;   // rate control state (calling thread)
  void rate_control();
  RcState *rc_state_ = nullptr;                 // rate control v2: device-side state
  bool band_picture_setup();
  EncFrame band_f_{};                    // band mode: the frame of the picture between band_phase1 and band_phase2b
  hipStream_t stream_tok_ = nullptr;     // signalling decisions, tokenizer, compaction
  hipStream_t stream_in_ = nullptr;      // input padding (runs ahead of the previous picture's kernels)
  hipEvent_t ev_src_free_[kSets] = {}; bool src_busy_[kSets] = {};
  SaoParams *sao_[kSets] = {};            // per CTU, one array per set

  // An intra picture depends on no other picture: its chain (1.6 ms at 1080p, twenty picture intervals) is queued on a stream of its own the moment the
  // picture is accepted, beside the P pictures in front of it that the main stream is still working through; the next P picture waits for ev_idr_done_.
  hipStream_t stream_idr_ = nullptr; hipEvent_t ev_idr_done_ = nullptr; bool idr_pending_ = false, idr_side_ = false, all_intra_alt_ = false;
  // ... with its own copies of what the P pictures' kernels also use while it runs beside them (round 4: the side chain also with SAO, intra units in P
  // pictures, per-CTU QPs and rate control v2 -- uvgComm's default mode): progress counters + ticket word, the CTUs' edge columns and rows, the SAO work picture
  EncChain chain_, chain_idr_; uint32_t chain_gen_ = 0;      // the main stream's; the side chain's (idr_side_ || all_intra_alt_, else empty)
  bool build_chain(EncChain &c, std::string *error);
  hipEvent_t ev_signalled_ = nullptr, ev_tok_done_[kSets] = {}; bool tok_pending_[kSets] = {};
  uint8_t *intra_scratch_ = nullptr;
  uint8_t *d_scaling_ = nullptr;          // scaling-list default: KVZ_SCALING_BYTES scaling factors
  uint16_t *tok_buf_ = nullptr; int32_t *tok_count_ = nullptr; uint32_t *tok_seg_ = nullptr; uint32_t *tok_list_ = nullptr;
  std::vector<std::vector<uint8_t>> band_subs_; uint64_t band_bins_ = 0; bool band_coded_ = false;   // band mode: between phase 2a and 2b
  // me-source: k_me and k_intra_analyse<P> of the pictures ahead run on the input stream while the main stream is still in an earlier picture's chain, so what
  // they write -- the 16x16 costs, the candidate list, the quarters' scratch, the P pictures' progress counters with the "has intra units" word -- exists per working set
  bool me_ahead_ = false; uint32_t *me_block_[kSets] = {}; uint32_t *sync_set_[kSets] = {}; int prev_set_ = 0;
  uint32_t *me_cost16_ = nullptr; uint32_t *intra_order_ = nullptr; uint32_t *err_ = nullptr; unsigned long long *trace_ = nullptr;
  // one slot per picture in flight: the host-visible results of its kernels and what collect() needs to finish it
  struct EvPair { hipEvent_t a, b; KernelId id; };
  struct Slot {
    uint16_t *h_tok_dense = nullptr, *d_tok_dense = nullptr; int32_t *h_tok_count = nullptr, *d_tok_count = nullptr;   // host-mapped pinned
    uint32_t *h_tok_off = nullptr, *d_tok_off = nullptr;
    uint32_t *h_err = nullptr, *d_err = nullptr;
    int32_t *h_wp = nullptr, *d_wp = nullptr;            // weightp: the picture's record as k_wp_decide left it (host-mapped: the slice headers are written from it)
    int32_t *h_sc = nullptr, *d_sc = nullptr;            // scenecut: the picture's record as k_sc_decide left it (host-mapped: submit() reads the verdict from it) or, not examined, as submit() wrote it
    // GPU arithmetic coder (cfg.entropy_gpu): dense tokens stay in device memory (d_tok_dense .. d_tok_off point there), the coder runs on the slot's own
    // stream -- a substream is a ~0.1-1 ms serial chain, so several pictures' coders must be able to run side by side
    uint16_t *g_tok = nullptr; int32_t *g_count = nullptr; uint32_t *g_off = nullptr;
    uint8_t *g_stage = nullptr; uint32_t *g_cursors = nullptr, *g_ctx_save = nullptr, *g_ctx_ready = nullptr;
    uint8_t *h_out = nullptr, *d_out = nullptr; uint32_t *h_sub = nullptr, *d_sub = nullptr;   // host-mapped: substream bytes; [3][nsub] offset, length, bins
    hipStream_t ent_stream = nullptr; hipEvent_t tok_ev = nullptr; uint32_t gen = 0;
    hipEvent_t done = nullptr, rec_done = nullptr;       // tokens / substreams delivered (stream_tok_ / ent_stream) / reconstruction final (stream_)
    hipEvent_t sink_done = nullptr; bool has_sink = false; // set_recon_sink: the reconstruction's copy into the caller's picture (stream_rec_)
    int poc = 0, rec_idx = 0, set = 0, qp = 0; bool intra = false, write_ps = false; long pic_idx = 0;
    int32_t *h_fb = nullptr, *d_fb = nullptr;            // loss-feedback: the picture's record {heal, reports, cells, forced quarters} (host-mapped: k_fb_blocks writes the counts); fb-anchor: four more words, {v2 heal, anchor POC, da, quarters from reference 1} (k_fb_refs writes the count)
    int kept = 0;                                        // fb-anchor: entries of the P picture's reference picture set (nref of them used)
    int32_t ir[4] = {-1, 0, 0, 0};                         // intra-refresh: what debug_copy("ir") says of the picture; ir[0] == 0: its access unit starts with the recovery point SEI
    int layer = 0, nref = 0; int8_t dist[KVZ_MAX_LP_REFS] = {0, 0, 0, 0};   // lp-gop (nref 0: off): what the slice header's reference picture set and debug_copy("lp_gop") say
    std::vector<EvPair> ev; size_t ev_used = 0;
    EncodedPicture result; bool ready = false, ok = true;   // owf >= 2: filled by the background thread
    EncFrame f_tok{}; bool prof = false, tok_failed = false;                    // tok_deferred_: what the tokenizer's launches need, kept until the launcher thread makes them
  };
  Slot slot_[kMaxDepth + 2]; Slot *cur_slot_ = nullptr; int nslots_ = 1, depth_ = 0;
  std::thread bg_[2]; std::mutex bm_; std::condition_variable bcv_; std::deque<int> bq_; bool bquit_ = false;
  // SAO (owf 2..7): the tokenizer of a picture needs the filter's parameters, i.e. the END of the picture's chain.  An event on the main stream that another
  // stream is already waiting for costs the stream's next kernel -- the next picture's k_me -- 12-25 us; one that only the host looks at costs 1-2 us
  // (tools/measure/record_after_writer.hip).  So a thread of its own watches the chains' events and launches a picture's tokenizer when its chain is done.
  bool tok_deferred_ = false; std::thread tok_thread_; std::mutex tm_; std::condition_variable tcv_; std::deque<int> tq_; bool tquit_ = false;
  void tok_launcher();
  bool launch_tokenizer(Slot &sl, const EncFrame &f, bool intra, bool wait_on_stream, bool prof);
  void timed_slot(Slot &sl, bool prof, KernelId id, hipStream_t st, const std::function<void()> &launch);
  std::mutex stat_m_;
  long submitted_ = 0, collected_ = 0, accepted_ = 0;    // pictures whose kernels have been queued / whose access unit has been returned / taken from the caller
  // owf >= 2: the output lags anyway, so the calling thread (uvgComm's encoder filter thread) only hands the picture over; a submitter thread makes the
  // ~20 HIP calls that queue its copy and kernels (~0.1 ms per picture, which at 1080p was most of what that thread had time for).  Applies where the
  // input stays valid without the call waiting for it: page-locked host pictures (contract) and device pictures with input-hold.
  struct SubmitJob { const uint8_t *src = nullptr; bool host = false; std::vector<int8_t> roi; int roi_w = 0, roi_h = 0; int slot = 0; uint8_t *sink[3] = {nullptr, nullptr, nullptr}; };
  uint8_t *sink_[3] = {nullptr, nullptr, nullptr}, *sink_sub_[3] = {nullptr, nullptr, nullptr};      // as set by the caller / of the picture being submitted
  std::thread sub_thread_; std::mutex sm_; std::condition_variable scv_; std::deque<SubmitJob> sq_; bool squit_ = false, sbusy_ = false;
  void submitter();
  void drain_submitter();
  bool enqueue(const uint8_t *src, bool host, EncodedPicture *out);
  bool upload_and_submit(const uint8_t *y, const uint8_t *u, const uint8_t *v, bool pinned);      // (a packed format: y is the whole picture)
  bool host_picture(const uint8_t *y, const uint8_t *u, const uint8_t *v, EncodedPicture *out, bool pinned);      // what encode_host and encode_packed_host share
  bool device_picture(const uint8_t *d_in, EncodedPicture *out);
  hipEvent_t in_done_ = nullptr; bool in_pending_ = false;   // input picture consumed (staging buffer / caller's device buffer reusable)
  // owf >= 2: two background workers, each with its own coder pool, finish two pictures side by side (the substreams of one
  // picture start one after the other -- WPP context hand-over -- so one picture alone cannot keep the pool busy)
  EntropyHost *entropy_ = nullptr, *entropy2_ = nullptr;
  std::vector<std::vector<uint8_t>> rows_out_, rows_out2_;
  int frame_idx_ = 0, poc_ = 0, intra_count_ = 0;
  bool profiling_ = false, prof_now_ = false; int prof_every_ = 1;
  double t_submit_ = 0, t_wait_ = 0, t_arith_ = 0, t_asm_ = 0, t_in_ = 0;   // encoder-thread time split (KVAZZUP_AMD_TRACE)
  double k_ms_[K_COUNT] = {0}; uint64_t k_n_[K_COUNT] = {0};
  StreamParams sp_{};
};

}  // namespace kvzx
