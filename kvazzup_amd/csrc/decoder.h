// kvazzup_amd/csrc/decoder.h -- host engine of the HIP decoder behind libOpenHevc*
// (/root/reference/src/media/processing/openhevcfilter.cpp:36-56,145-146,195-199).
//
// Four parts: dec_syntax.{h,hip} turns header bits into plain structs (parameter sets, slice header parts; knows no Decoder), dec_parse.hip is the slice-data
// parser (parse_job / parse_substream), dec_output.h (over dec_order.h; knows no Decoder either) owns the output side -- the order pictures leave in, the copies that
// are handed out and how long they stay valid --, decoder.hip is everything between them: NAL dispatch, picture assembly, reference management, the job ring,
// buffers, launches, the ring's own output buffers.
//
// Division of labour: the host parses NAL units and runs CABAC decoding (bit-serial, one substream per CTU row or tile),
// which yields per-4x4 records (motion, edges, QpY), the transform blocks in decoding order and their non-zero levels
// (dec_frame.h); those go to the GPU in one copy and the GPU does everything that touches samples: motion compensation,
// intra prediction, dequantisation + inverse transforms, reconstruction, deblocking, SAO (dec_kernels.hip).
//
// Supported streams: what a Main-profile encoder in a video call produces and OpenHEVC would be asked to decode -- 8-bit 4:2:0,
// CTB 64 (Kvazaar's fixed geometry), 32 or 16 / minimum CB 8 (Kvazaar's), 16 or 32 / transform blocks 4..min(32, CTB), coded sizes that are multiples of 8, I, P and B
// slices (both reference lists, bi-prediction, pictures handed out in POC order), every CU size and partitioning (AMP included), intra CUs in P pictures, NxN intra, all chroma
// prediction modes, transform trees, several reference pictures (RPS in the SPS or the slice header, inter RPS prediction), long-term reference pictures,
// temporal motion vector prediction, merge levels, cu_qp_delta at any quantisation-group size, chroma QP offsets, sign data
// hiding, transform skip, scaling lists (default, SPS and PPS scaling_list_data), cu_transquant_bypass (lossless coding units), PCM coding units, constrained intra prediction, deblocking offsets /
// overrides, SAO, WPP, tile grids up to the level limit of 20 columns x 22 rows (uniform or
// explicit spacing; in-loop filtering across tile and slice boundaries on or off -- Kvazaar switches it off), pictures in several slice segments: the two ways Kvazaar cuts them (a dependent slice segment per CTU row with WPP, an
// independent slice per tile) and -- one-tile pictures -- segments that begin at ANY coding tree block, independent slices (own SliceQpY) and dependent
// segments mixed (an MTU per slice, N row groups: PicJob::ctb_cut).  Random access (8.1.3, C.5.2.2): decoding may begin at a CRA picture -- its RASL pictures are
// dropped, its RADL pictures decoded --, BLA pictures and end of sequence NAL units start a coded video sequence, pic_output_flag = 0 keeps a picture in,
// no_output_of_prior_pics_flag discards what still waits (dec_order.h).  Rejected with a negative return value (kvzx_decoder_last_error): several slices
// inside a tile of a picture with tiles, slices of one picture that differ in more than SliceQpY and the loop filter flag,
// > 255 slices in a picture.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include "hevc_core.h"
#include "dec_syntax.h"
#include "dec_output.h"
#include "host_pool.h"
#include "dec_frame.h"
#include "dec_kernels.h"
#include "batch.h"

namespace kvzx {

// DK_HOST_PARSE is not a kernel: wall time of the host CABAC parsing stage
enum { PM_INTER = 0, PM_INTRA = 1, PM_SKIP = 2, PM_NONE = 255 };      // PicJob::pred_mode
enum DecKernelId { DK_INTER = 0, DK_INTRA, DK_DEBLOCK, DK_HOST_PARSE, DK_SAO, DK_INTRA_P, DK_COUNT };      // (DK_INTRA_P: the intra blocks of a picture that also has inter blocks)

// worker threads that parse whole pictures concurrently (frame threading)
class FrameWorkers {
 public:
  explicit FrameWorkers(int n) { for (int i = 0; i < n; i++) t_.emplace_back([this] { name_this_thread("kvzx-parse"); run(); }); }
  ~FrameWorkers() { { std::lock_guard<std::mutex> l(m_); quit_ = true; } cv_.notify_all(); for (auto &t : t_) t.join(); }
  void submit(std::function<void()> f) { { std::lock_guard<std::mutex> l(m_); q_.push_back(std::move(f)); } cv_.notify_one(); }
 private:
  void run()
  {
    for (;;) {
      std::function<void()> f;
      { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [this] { return quit_ || !q_.empty(); }); if (q_.empty()) return; f = std::move(q_.front()); q_.pop_front(); }
      f();
    }
  }
  std::vector<std::thread> t_; std::mutex m_; std::condition_variable cv_; std::deque<std::function<void()>> q_; bool quit_ = false;
};

// motion of a decoded picture as later pictures see it for temporal prediction (8.5.3.2.8): one entry per 16x16 luma block, the
// motion of its top-left 4x4.  Written by the picture's parser row by row, read by the parsers of following pictures (which may
// run concurrently under frame threading: row_done[] orders them).
struct ColMotion {
  struct Mv { int16_t mv[2][2]; int32_t ref_poc[2]; uint8_t used; uint8_t lt; uint8_t pad[2]; };      // per list: vector, POC of the picture it points into; used: bit L = list L predicts the block (0: intra); lt: bit L = that picture was a long-term reference picture then (8.5.3.2.9)
  int w16 = 0, h16 = 0, hc = 0, poc = 0;
  std::vector<Mv> mv;
  std::unique_ptr<std::atomic<uint8_t>[]> row_done;      // per CTU row
  std::unique_ptr<std::atomic<uint8_t>[]> row_cols;      // tile columns of the row that have been parsed (row_done follows the last one)
  int cols = 1;
};

// motion of a decoded picture as concealment v3 reads it (Decoder, below): one entry per 16x16 luma block of the coded picture (the last column and row may be
// partial), the motion of its top-left 4x4 -- list 0's when that list predicts the block, else list 1's.  Filled by the picture's parser row by row, and only in
// mode 3; read when a stand-in is filled from the picture, by which time the parse has finished (fill_concealed).  A plain array: no ordering state.
struct ConcealMotion {
  struct E { int16_t mv[2]; int32_t ref_poc; uint8_t lt, none, pad[2]; };      // vector (quarter samples), POC of the picture it points into, that picture was a long-term reference then, none: intra / not parsed
  int w16 = 0, h16 = 0;
  std::vector<E> e;
};

class Decoder {
 public:
  explicit Decoder(int device) : device_(device), outp_(device) {}
  // what stands in for a reference picture that never arrived: 2 = a copy of the nearest reference picture (default), 3 = that picture moved along its own motion
  // ("Concealment v2" / "v3" below); before the first picture, and 3 not in band mode.  false: refused
  bool set_concealment(int mode) { if ((mode != 2 && mode != 3) || !jobs_.empty() || (mode == 3 && band_nrows_ > 0)) return false; conceal_mode_ = mode; return true; }
  int concealment() const { return conceal_mode_; }
  // "Partial pictures v1" (below): a picture that lost slice segments keeps the coding tree blocks that arrived; off by default; before the first picture, not in band mode.  false: refused
  bool set_partial_pictures(bool on) { if (!jobs_.empty() || (on && band_nrows_ > 0)) return false; partial_ = on; return true; }
  bool partial_pictures() const { return partial_; }
  // the runs of missing coding tree blocks of every damaged picture so far, in decoding order: (POC, first block, count) triples; -> the number of triples there are
  int damage_log(int32_t *triples, int cap) const { const int n = (int)(damage_log_.size() / 3); for (int i = 0; triples && i < n && i < cap; i++) memcpy(triples + 3 * i, &damage_log_[(size_t)3 * i], 3 * sizeof(int32_t)); return n; }
  // frame threading: up to n pictures are parsed concurrently while one more is reconstructed on the GPU; the output is delayed by n pictures
  // (libOpenHevcInit(nb_threads, OH_THREAD_FRAME / OH_THREAD_FRAMESLICE)); call before the first picture
  void set_frame_threads(int n) { if (jobs_.empty()) frame_threads_ = n < 1 ? 1 : (n > 32 ? 32 : n); }
  int frame_threads() const { return frame_threads_; }
  ~Decoder();
  bool start(std::string *error);           // checks the HIP device; no CPU fallback
  // One NAL unit (with or without start code).  <0 error/unsupported, 0 nothing to output, 1 picture ready.
  int decode_nal(const uint8_t *data, size_t len, int64_t pts);
  bool get_picture(DecodedPicture *out);   // the picture announced by the last decode_nal() == 1
  void set_download(bool on) { download_ = on; }
  // Test / measurement hook, never a decoding mode: the host half alone -- NAL units, parameter sets, slice headers and the CABAC slice-data parser run,
  // nothing is allocated on or sent to a device, no picture ever comes out (decode_nal returns 0 for every picture).  What the parser produced is
  // summarised by parse_probe_stats: pictures, transform blocks, level words, a 64-bit FNV-1a digest over every picture's records / tables / blocks /
  // levels (the bytes launch_gpu would upload, fixed part minus the descriptor) and the time spent in parse_job.  CPU tests pin the parser's output with it
  // (tests/test_parser_probe.py); tools/measure/parse_rate.py times the parser where there is no GPU.
  bool set_parse_only() { if (jobs_.empty() && !started_) parse_only_ = true; return parse_only_; }      // (false: declined -- the decoder has been started)
  struct ProbeStats { uint64_t pictures = 0, tus = 0, levels = 0, digest = 0xcbf29ce484222325ull, bins = 0; double parse_ms = 0; };
  ProbeStats parse_probe_stats() const { return probe_; }
  // device-resident output (set_download(false)): the planes handed out stay untouched while the next `n` pictures are begun
  // (they may be read as reference pictures, never written); default 2.  alloc_slot keeps the promise for the ring's buffers, DecOutput for owned copies
  void set_output_hold(int n) { outp_.set_hold(n < 1 ? 1 : (n > 8 ? 8 : n)); }
  void set_profiling(int every) { profiling_ = every > 0; prof_every_ = every > 0 ? every : 1; }   // n: every n-th picture
  void set_parse_threads(int n) { if (!pool_) parse_threads_ = n < 1 ? 1 : n; }
  void get_kernel_times(double *ms, uint64_t *launches, bool reset);
  bool debug_copy(const char *what, void *dst, size_t bytes);
  int last_error() const { return last_error_; }
  // libOpenHevcSetCheckMD5: decoded picture hash SEI messages (MD5 or checksum) are compared with the pictures as decoded here
  void set_check_hash(bool on) { check_hash_ = on; }
  // libOpenHevcSetTemporalLayer_id: the highest temporal sub-layer that is decoded -- slice NAL units with a higher TemporalId are dropped (nothing of the layers below
  // predicts from them, 8.1.3 sub-bitstream extraction).  OpenHEVC's default is 7 (everything); uvgComm passes 0 (openhevcfilter.cpp:54), and its own sender codes one layer.
  void set_no_cropping(bool on) { no_crop_ = on; }      // libOpenHevcSetNoCropping: pictures are handed out at their coded size, the conformance window is not applied
  void set_max_temporal_id(int t) { max_tid_ = t < 0 ? 0 : (t > 7 ? 7 : t); }
  void hash_stats(int *checked, int *mismatch) const { if (checked) *checked = hash_checked_; if (mismatch) *mismatch = hash_mismatch_; }
  void flush() {}
  int pending() const { return (int)(job_head_ - job_tail_) + (gpu_job_ ? 1 : 0) + (int)gpu_q_.size(); }

  // ---- per-picture state shared with the slice-data parser (dec_parse.hip)
  // one per substream.  Two cache lines each: the rows of a picture are parsed side by side, every one appending to ITS vectors all the time -- the
  // vectors' headers of neighbouring rows do not share a cache line.  (What limits the row-parallel parse is WPP itself: a unit can start when its left neighbour
  // and the unit above-right are done, and a picture takes as long as the heaviest path through that graph.  The benchmark's moving objects are a few very heavy
  // units stacked over several rows -- ten of a 1080p P picture's 510 units hold a quarter of its parse -- and the heaviest path is two thirds of the whole: 1.4-1.6x
  // at best with any number of threads, tools/measure/wpp_critical_path.py, profiles/r06_wpp_critical_path.txt; seventeen rows end 55 us apart, owf0_timeline.py.)
  struct alignas(128) SubOut { std::vector<uint32_t> levels; std::vector<DecTu> tus; int rc = 0; };
  struct alignas(64) Progress { std::atomic<int> v{0}; char pad[60]; };   // one cache line per row: no false sharing between pollers
  // everything one picture needs between its slice header and its reconstruction
  struct PicJob {
    std::vector<uint8_t> rbsp; size_t data_off = 0, data_len = 0;
    std::vector<size_t> sub_start;
    // slice segments (a picture in several NAL units): whether a segment ends with this CTU row (always for the last row); where, inside a
    // substream that spans several rows (no WPP), a new segment's data starts at this row (SIZE_MAX: the row continues the stream)
    std::vector<uint8_t> seg_end_row; std::vector<size_t> row_restart;
    // the picture's substreams in decoding order: CTB rows [cy0, cy1) x columns [cx0, cx1) of one tile (one row with WPP), the tile's first row and id;
    // with tile columns: whether a slice segment ends with substream k (seg_end_row is per CTU row and only used without tile columns)
    struct SubGeom { int cy0, cy1, cx0, cx1, tile_cy0, tile_cy1, tc; };
    std::vector<SubGeom> geom; std::vector<uint8_t> seg_end_sub;
    // FREE slices (round 6; one tile): slice segments that begin at any coding tree block, independent slices inside the tile -- what an encoder that cuts
    // slices by bytes or block counts sends.  Per coding tree block (raster): ctb_cut bit 0 an independent slice begins here, bit 1 a dependent segment,
    // bit 2 a segment ENDS with this block; ctb_data: where the beginning segment's bytes start in rbsp; ctb_slice: the block's slice (counted from 0; it
    // also rides in ctu_tile[] for the kernels' availability tests); slice_qps: SliceQpY by slice; ds_saved: the context states a segment left behind at the
    // end of a CTB row (WPP: the next row's parser may need them, 9.3.1).  All empty: one slice, or Kvazaar's slices (whole rows / whole tiles).
    std::vector<uint8_t> ctb_cut, ctb_slice; std::vector<size_t> ctb_data; std::vector<int8_t> slice_qps; std::vector<uint8_t> ds_saved;
    // a one-tile picture submitted because its segments COVER it row by row: whether the last one really ends with the picture is not in any header.  The parser
    // says so when it does not (DEC_SEG_ENDS_EARLY), and the synchronous decoder then takes the picture back and waits for the rest of its access unit (submit_job).
    bool ambiguous_end = false;
    // some boundary inside the picture is closed to the in-loop filters (loop_filter_across_tiles_enabled_flag = 0 with tiles; a slice with
    // slice_loop_filter_across_slices_enabled_flag = 0): lf_slices = the picture's independent slices (first block, flag)
    bool lf_restricted = false; std::vector<std::pair<int, uint8_t>> lf_slices;
    struct Undo { int poc = 0, prev_poc = 0; bool is_ref = false, used = false, seen_irap = false; long decode_idx = 0; std::shared_ptr<ColMotion> motion; std::shared_ptr<ConcealMotion> cmotion; OrderMark order; bool standin = false; } undo;      // what submit_job changed
    SliceHdr sh; std::shared_ptr<const DecSps> sps; DecPps pps;  // (a later SPS / PPS NAL may replace the table entry while this picture is still being parsed: the job keeps the SPS it was coded with alive, the PPS by value)
    int64_t pts = 0; int crop[4] = {0, 0, 0, 0}; uint32_t fps_num = 0, fps_den = 0;
    int slot = 0;                                                // picture buffer this picture is reconstructed into
    int cvs = 0;                                                 // the coded video sequence it belongs to (output order)
    uint64_t serial = 0;                                         // number in decoding order
    // (mode 3: the stand-in's and the source's picture order counts and the source's motion, taken when the source is chosen)
    struct Conceal { int first, second; int poc = 0, src_poc = 0; std::shared_ptr<const ConcealMotion> motion; Conceal(int buf, int src) : first(buf), second(src) {} };
    // partial pictures v1: the runs (first coding tree block, count) that never arrived -- the parser gives them records that make every kernel do nothing, fill_missing
    // their samples; the source picture S chosen when the picture's first segment arrived (buffer or -1: grey, its order count, its motion for mode 3 -- NULL: a stand-in)
    bool scan_gaps = false;      // one tile, without WPP or as free slices: the parser itself finds what is missing (dec_parse.hip parse_substream; miss_map, a byte per block) and parse_job files the runs here
    std::vector<uint8_t> miss_map; std::vector<int> row_seg_start;      // (row_seg_start: WPP, per CTB row the address of the segment that goes on into it through an entry point, -1: none)
    std::vector<std::pair<int, int>> missing; int fill_src = -1, fill_src_poc = 0; std::shared_ptr<const ConcealMotion> fill_motion;
    std::vector<Conceal> conceal;                                // (buffer, source buffer or -1): buffers that stand in for reference pictures that never arrived, filled before this picture's kernels (launch_gpu)
    bool starts_cvs = false, discard_prior = false;              // NoRaslOutputFlag (8.1.3); ... and no_output_of_prior_pics_flag in force (C.5.2.2)
    int nref = 0; int ref_poc[16]; uint8_t ref_slot[16];        // RefPicList0
    int nref1 = 0; int ref_poc1[16]; uint8_t ref_slot1[16];     // RefPicList1 (B slices)
    uint8_t ref_buf[KVZ_DEC_MAX_REFS] = {};                     // ref_slot / ref_slot1 name entries of the kernels' table (B4Rec::slot, DecFrame::ref); ref_buf: the picture buffer (dpb_) behind each entry
    uint8_t ref_lt[16] = {}, ref_lt1[16] = {};                  // the entry is a long-term reference picture (8.3.2: no vector scaling, 8.5.3.2.7 / 8.5.3.2.9)
    bool no_backward = true;                                     // NoBackwardPredFlag (8.5.3.2.9): no entry of either list follows the picture in output order
    // B slices: the two-list motion of every 4x4 block as the parser's own derivations read it (merge, AMVP); what the kernels need of it goes
    // into the B4Rec (the first used list's vector and picture) and, for bi-predicted blocks (B4_BI), the second vector here
    struct MvF { int16_t mv[2][2]; int8_t ref[2]; };
    std::vector<MvF> mvf; std::vector<B4L1> b4x; std::atomic<int> any_bi{0};
    // One picture at a time (uvgComm's default "Slice" threading): a CTU row's 4x4 records go up as soon as the row is parsed, beside the parsing of the rows
    // below -- the megabyte (4K: four) of records is then on the device when the parse ends, and what submit_job uploads is the tables, transform blocks and
    // levels.  early_dst: the input buffer this picture will be launched from (nullptr: no early upload); early_rows: rows whose copy was queued.
    uint8_t *early_dst = nullptr; std::atomic<int> early_rows{0};
    std::shared_ptr<ColMotion> col, own;                         // collocated picture's motion (NULL: no temporal candidates); this picture's
    std::shared_ptr<ConcealMotion> cown;                         // this picture's motion for concealment v3 (NULL in mode 2)
    // the pinned input block (dec_frame.h) and the host views into it
    uint8_t *h_in = nullptr; size_t h_in_cap = 0; size_t ntu = 0, nlev = 0;
    DecInputLayout lay;                                          // where everything lies in it: the fixed part from prepare_jobs, the whole of it once parse_job has counted the picture's blocks
    B4Rec *b4 = nullptr; TuRange *region = nullptr, *ctu = nullptr; uint8_t *ctu_tile = nullptr; SaoParams *sao = nullptr;
    // host-only syntax state per 4x4: prediction mode (0 inter, 1 intra, 2 skip, 255 not decoded yet), coding quadtree depth, intra mode
    std::vector<uint8_t> pred_mode, ct_depth, intra_mode;
    std::vector<SubOut> subs; std::vector<uint8_t> wpp_saved;
    std::unique_ptr<Progress[]> row_progress; int row_progress_n = 0;
    alignas(64) bool any_intra = false; bool any_inter = false;        // (set by the rows' parsers: a line of their own, written once -- the parsers test before they store)
    alignas(64) bool across_slices = true;
    std::atomic<int> state{0}; int rc = 0; double parse_ms = 0;
    hipEvent_t done = nullptr;                                   // recorded behind the picture's last kernel
    std::atomic<int> launched{1};                                // 0 while the picture waits in the device's submission layer (batch.h): `done` has not been recorded yet
    std::vector<uint8_t> expect_hash;                            // payload of the picture's decoded picture hash SEI (libOpenHevcSetCheckMD5), empty: none
    long launch_idx = 0;                                         // count of pictures launched before this one
    hipEvent_t dl_done = nullptr; int dl_buf = -1;               // download mode: the picture's copy into host buffer dl_buf, queued behind `done` on the download stream
    struct EvPair { hipEvent_t a, b; int id; }; std::vector<EvPair> ev; size_t ev_used = 0;     // kernel timing (set_profiling)
    PicJob() {}
    PicJob(const PicJob &) {}                                  // (vector<PicJob> construction only)
  };
  // ---- tile-row split of ONE stream over several decoders, one per GPU (the decoding side of kvazzup_amd/tilesplit.py): this decoder
  // reconstructs CTU rows [row0, row0 + nrows) only -- whole tile rows of a stream whose motion vectors stay inside their tiles (what the
  // split ENCODER writes) -- and deblocking across the band's boundaries goes through two small exchanges with the neighbouring decoders.
  // Synchronous decoder only (one frame thread), no SAO, no temporal motion prediction.  Per picture: decode_nal (returns 0: the band is
  // reconstructed) -> band_export(0) -> [to rank + 1 / from rank - 1] -> band_import(0) -> band_deblock -> band_export(1) ->
  // [to rank - 1 / from rank + 1] -> band_import(1) -> band_finish (the picture is the output; its band's rows are valid).
  bool set_band(int row0, int nrows) { if ((conceal_mode_ == 3 || partial_) && nrows > 0) return false; if (jobs_.empty()) { band_row0_ = row0; band_nrows_ = nrows; } return true; }      // (false: refused -- concealment v3 and partial pictures have no band form)
  size_t band_halo_bytes() const { return (size_t)pw_ * 8; }
  bool band_export(int stage, uint8_t *d_buf);     // stage 0: this band's LAST four luma rows (+ chroma) before deblocking and their 4x4 records, for the band below; stage 1: the four rows above this band, final, for the band above
  bool band_import(int stage, const uint8_t *d_buf);   // stage 0: from the band above, into the rows above this band; stage 1: from the band below, this band's last four rows, final
  bool band_ready() const { return band_nrows_ > 0 && gpu_job_ != nullptr; }     // a picture's band is reconstructed and waits for the exchange
  bool band_deblock();
  int band_finish();
  int pw() const { return pw_; }
  int ph() const { return ph_; }

 private:
  bool ensure_buffers(int w, int h, int ctb_log2);
  void free_buffers();
  int decode_slice(const uint8_t *rbsp, size_t len, int nal_type, int64_t pts);
  size_t unescape(const uint8_t *data, size_t len); int decode_parameter_set(int nal_type, BitReader &r);
  int hash_sei(const uint8_t *rbsp, size_t len);
  int verify_hash(const PicJob &job, const std::vector<uint8_t> &want);
  bool check_hash_ = false; int hash_checked_ = 0, hash_mismatch_ = 0;
  int parse_job(PicJob &job, bool row_parallel);
  int parse_substream(PicJob &job, int sub, const uint8_t *data, size_t len, SubOut &out);
  int close_open_picture();
  int close_free_picture(PicJob &job);
  void take_back_job(PicJob &job); void file_damage(const PicJob &job); std::vector<uint8_t> layout_of(const PicJob &job) const; std::vector<uint8_t> damaged_layout_; uint32_t take_backs_ = 0;
  // ---- a picture arriving in several slice segment NAL units: its job is filled segment by segment and submitted with the last one.  Everything that is known
  // about the picture being assembled lives in ONE value, reset by assignment when a picture is opened (open_job).
  // FreeSeg: the slice segments as they arrived (one tile), kept beside the row bookkeeping of Kvazaar's forms, which is dropped the moment a segment turns up
  // that those forms do not have (OpenPicture::free) -- the picture is then put together from this list when the access unit ends.
  // LfSlice: in-loop filtering across slice and tile boundaries -- the picture's independent slices (first coding tree block, slice_loop_filter_across_
  // slices_enabled_flag) in every form a picture's slices come in; note_lf_restrictions turns them (and the PPS's tile flag) into PicJob::lf_restricted / the map
  // the parser's last step writes for the kernels (DecFrame::ctu_nb)
  struct FreeSeg { int address; bool dependent; int slice_qp; std::vector<size_t> subs; };
  struct LfSlice { int address; bool across; };
  struct OpenPicture {
    bool active = false, guessed_one_row = false, free = false, irap = false;
    int subs = 0, rows = 0, pps_id = 0, nal_type = 0;      // progress in substreams (tile columns) / CTB rows; what a further segment must match
    bool cur_dependent = false; int cur_qp = 26;           // the segment at hand: dependent?  SliceQpY of its slice
    std::vector<FreeSeg> segs; std::vector<LfSlice> lf;
  } asm_;
  bool free_stream_ = false;                               // per STREAM: its pictures come in free slices (append_segment)
  void note_lf_restrictions(PicJob &job);
  int finish_oldest();
  void drop_pending();
  // (the tables per coding tree block -- transform-block range, tile id, SAO parameters -- and the intra chains' arrays have one entry per CTB of the stream's size: ctbl_ = CtbLog2SizeY)
  size_t nctb() const { return (size_t)(pw_ >> ctbl_) * (ph_ >> ctbl_); }
  bool prepare_jobs(int w, int h, int ctb_log2);      // the new size takes effect; every ring entry: input block with a zeroed fixed part (PicJob::lay), per-4x4 syntax state
  bool grow_job_input(PicJob &job, size_t bytes);
  void bind_job(PicJob &job);
  // launch_gpu and its stages (decoder.hip), in the order they run; the `batched` / second-chain decisions between them are launch_gpu's own
  struct ChainSet; int launch_gpu(PicJob &job);
  int fill_concealed(PicJob &job); int fill_missing(PicJob &job); uint8_t *input_buffer(PicJob &job, int ib);
  DecFrame picture_frame(PicJob &job, const DecInputLayout &lay, const ChainSet &cs, uint8_t *d_in) const;
  bool upload(PicJob &job, const DecInputLayout &lay, uint8_t *d_in, int ib, bool batched);
  int post_to_batcher(PicJob &job, const DecFrame &f, uint8_t *d_in, int ib); int launch_self(PicJob &job, const DecFrame &f, uint8_t *d_in, int ib, bool alt);
  template <class F> bool each_buffer_used(const PicJob &job, F &&visit);      // the picture's own buffer and both lists' buffers
  int complete_gpu(PicJob &job);
  int alloc_slot(); struct DpbPic; bool alloc_picture(DpbPic &p);
  void sync_main();                       // everything this decoder has submitted has run (the submission layer's queue included)
  bool batch_attached_ = false, batch_used_ = false;

  int device_; bool started_ = false;
  bool parse_only_ = false; ProbeStats probe_; void probe_book(PicJob &job, double ms);
  hipStream_t stream_up_ = nullptr; hipEvent_t up_done_[9] = {};   // upload of the next picture's input block beside the current picture's kernels
  hipStream_t stream_ = nullptr, stream_dl_ = nullptr;       // reconstruction; download of finished pictures (behind the picture's event, beside the next picture's kernels)
  std::shared_ptr<const DecSps> sps_[16]; DecPps pps_[64]; uint32_t vps_fps_num_ = 0, vps_fps_den_ = 0;
  int w_ = 0, h_ = 0, pw_ = 0, ph_ = 0; int ctbl_ = 6;      // ctbl_: CtbLog2SizeY of the active sequence (the padded size stays a multiple of 64: the kernels that tile the picture do so in 64x64 / 32x32 pieces whatever the CTB)
  std::vector<PicJob> jobs_; int frame_threads_ = 1; long job_head_ = 0, job_tail_ = 0;
  int submit_job(PicJob &job, int nal_type, bool irap);
  int submit_closed(PicJob &job, int rc);                  // close_open_picture: submit, keep the error for last_error, stash a picture that came out
  // decode_slice's steps (decoder.hip), in the order of 7.3.6.1 / 8.1.3 / 8.3.2; SliceCtx: what they hand on to each other
  struct SliceCtx;
  bool slice_front(SliceCtx &c, int &rc);
  void sequence_state(const SliceCtx &c);
  int apply_rps_and_build_lists(SliceCtx &c);
  PicJob &open_job(const SliceCtx &c, const DecPps &pp, int slot);
  int append_segment_tiles(PicJob &job, const SliceCtx &c, int address);
  int append_segment(PicJob &job, const SliceCtx &c, const DecPps &pp, int address);
  // the output side (dec_output.h): what decode_nal does not hand out where it lies in the ring (out_) is offered -- copied -- and comes back in its turn
  DecOutput outp_; int cvs_ = 0;
  bool offer_output(bool in_turn) { if (!outp_.completed(out_, in_turn, download_, stream_dl_ ? stream_dl_ : stream_)) return false; pic_ready_ = false; return true; }
  int decode_nal_inner(const uint8_t *data, size_t len, int64_t pts, int &nal_type);
  std::unique_ptr<FrameWorkers> workers_;
  // decoded picture buffer: slot = device planes + what reference marking needs
  struct DpbPic { uint8_t *plane[3] = {nullptr, nullptr, nullptr}; int poc = 0; bool is_ref = false, used = false, is_lt = false, standin = false;      // is_lt: marked "used for long-term reference" (8.3.2)
                  long decode_idx = -1000; std::shared_ptr<ColMotion> motion; std::shared_ptr<ConcealMotion> cmotion;      // (cmotion: concealment v3's record, NULL in mode 2 and for a stand-in)
                  hipEvent_t last_dl = nullptr;      // download mode: the copy of the picture last reconstructed here (a later picture's kernels wait for it before they write the buffer)
                  hipEvent_t last_use = nullptr; bool last_use_alt = false; };      // (two chains, below: the last picture that read or wrote the buffer, and the stream it ran on)
  // More buffers than a picture can have reference pictures: beside those (15 at most, 7.4.3.2.1) the ring holds the pictures handed out and still promised
  // untouched (kvzx_decoder_set_output_hold: up to 8), the pictures launched behind them (kMaxGpuDepth), the picture at hand and the one a fill reads (avoid_slot_).
  // Buffers past the first six are allocated when first taken.  The kernels' table (DecFrame::ref) has KVZ_DEC_MAX_REFS entries: entry k is buffer k, and a
  // reference picture that lies in a buffer past those takes, for that picture, an entry whose own buffer the picture does not refer to (PicJob::ref_buf).
  static constexpr int kMaxPics = 15 + 8 + 8 + 2 + 1;
  DpbPic dpb_[kMaxPics];
  // device side
  // Frame-threaded mode keeps up to gpu_depth_ pictures queued on the GPU (launched, not yet completed): a picture's way through upload, kernels
  // and the copy back to the host is ~0.2 ms at 1080p, and with only one picture launched ahead of the one being waited for the calling thread
  // sat out most of that for every picture.  The output lag stays `frame_threads` pictures: the parse ring gives up what the GPU queue takes.
  static constexpr int kMaxGpuDepth = 8;
  int gpu_depth_ = 1; std::deque<PicJob *> gpu_q_;
  uint8_t *d_in_[kMaxGpuDepth + 1] = {}; size_t d_in_cap_[kMaxGpuDepth + 1] = {};   // device copies of PicJob::h_in: the pictures in flight take turns
  // the arrays of ONE intra chain and the stream it runs on: resid = intra residuals between k_dec_intra_resid and k_dec_intra; work = pictures with SAO are reconstructed
  // and deblocked here, the filter writes into the picture buffer; edge_col / edge_row = k_dec_intra's tagged hand-off words (dec_frame.h); progress = its ticket counter
  struct ChainSet { hipStream_t stream = nullptr; uint32_t *progress = nullptr, *edge_col = nullptr; unsigned long long *edge_row = nullptr; int16_t *resid[3] = {nullptr, nullptr, nullptr}; uint8_t *work[3] = {nullptr, nullptr, nullptr}; };
  ChainSet chain_[2]; uint32_t chain_gen_ = 0;      // main (its stream is stream_) and second (below); the generation of the last launch of either
  // per CTB of S luma samples a side: S + 2 x S / 2 column words, a quarter as many row words.  (pw_ and ph_ are multiples of 64, so the column words of a picture
  // are a multiple of 128 -- what a 64x64 CTB has -- whatever the CTB size.)
  size_t edge_col_words() const { return nctb() * (size_t)(2 << ctbl_); } size_t edge_row_words() const { return edge_col_words() / 4; }
  bool build_chain(ChainSet &cs, hipStream_t clear_on); void free_chain(ChainSet &cs);      // allocates; clears on the stream that will use the set (NULL: the null stream -- only while nothing is queued anywhere, ensure_buffers)
  uint32_t *intra_order_ = nullptr, *err_ = nullptr; uint32_t *h_err_ = nullptr;
  // A picture without inter blocks depends on no other picture, and its chain (k_dec_intra: 0.55 ms at 1080p) keeps a few dozen compute units busy: with the
  // frame-threaded decoder such pictures ALTERNATE between the decoder's stream and a second one with chain arrays of its own, so that two chains run side by
  // side (an all-intra stream, BASELINE configs[0]: the decoder's rate was 1 / chain).  Pictures that read or overwrite a buffer last used on the other stream
  // wait for that picture's event.
  char alt_prio_ = 'n'; long intra_seq_ = 0; bool alt_failed_ = false;      // (chain_[1] is assigned in one piece by ensure_alt: its stream non-NULL = every array of the second chain exists)
  bool ensure_alt();
  // download mode: page-locked output buffers take turns -- one is what libOpenHevcGetOutput last handed out (valid until the next
  // decode call, openhevcfilter.cpp:218-229 copies at once), one receives the picture whose kernels are running, queued behind them on
  // the download stream at launch, so the copy over PCIe overlaps the next picture's kernels instead of stalling the calling thread
  static constexpr int kOutRing = 16;     // (pictures queued on the GPU + the one handed out + the one being launched + six the caller may still be copying out of: OpenHEVCFilter's output stage)
  uint8_t *h_out_[kOutRing] = {}; size_t h_out_cap_ = 0;
  void describe_output(const PicJob &job, DecodedPicture &o, int buf) const;
  int queue_download(PicJob &job);
  int start_ready_downloads();
  long launched_ = 0; int out_slot_ = 0;
  char prio_dl_ = 'n', prio_up_ = 'n';
  char prio_ = 'n';                                       // priority level of the main stream (stream_pool.h key)
  int band_row0_ = 0, band_nrows_ = 0; uint8_t *band_din_ = nullptr; DecFrame band_f_{};      // band mode: the picture between its reconstruction and band_finish
  double t_parse_max_ = 0;                // trace: the longest parse of one picture (an IDR), ms
  bool spin_wait_ = false;                // KVAZZUP_AMD_SPIN: poll the GPU instead of napping between queries
  PicJob *gpu_job_ = nullptr;             // picture whose kernels are in flight (frame-threaded mode)
  int prev_poc_ = 0, cur_tid_ = 0; bool seen_irap_ = false;
  int max_tid_ = 7; bool no_crop_ = false;
  bool after_eos_ = false;       // an end of sequence / end of bitstream NAL unit came: the next picture starts a coded video sequence (a CRA picture then has NoRaslOutputFlag = 1, 8.1.3)
  // Concealment v2: a picture the reference picture set says the current one predicts from is not there (its access unit was lost on the way): a buffer with its
  // picture order count stands in -- no motion, never output -- and decoding goes on.  Its samples: a copy of the reference picture nearest in output order among
  // those the DPB held when the current picture arrived (of two equally near the earlier one), mid-grey when there is none (libavcodec's generate_missing_ref always takes grey).
  // The checker follows the same rule (oracle/hevc_dec.c missing_ref).  The buffers wait here for the picture that needed them; its launch fills them.
  //
  // Concealment v3 (set_concealment(3); off by default, and with it off nothing below exists): the stand-in is the same source picture S (order count s), moved along
  // S's own motion continued to the missing picture's order count p.  All integer, >> arithmetic:
  //  1. Block vectors.  Per 16x16 luma block B of the coded picture: the motion of the 4x4 block at B's top-left corner in S, list 0 if that list predicts it, else
  //     list 1 (ConcealMotion).  Zero when that block is intra, when the picture the vector points into (order count r) was a long-term reference then, when S is
  //     itself a stand-in, or when td = 0; else td = clip3(-128, 127, s - r), tb = clip3(-128, 127, p - s) and the vector is scaled as 8.5.3.2.12 scales one:
  //     tx = (16384 + (|td| >> 1)) / td, f = clip3(-4096, 4095, (tb * tx + 32) >> 6), v = clip3(-32768, 32767, sign(f * mv) * ((|f * mv| + 127) >> 8)).
  //  2. Neighbour test.  B keeps v only if at least two of its four edge neighbours inside the block grid carry a vector of step 1 within 4 quarter samples of v in
  //     both components; else its vector is zero.
  //  3. Fetch, whole samples: luma (x, y) of B = S's luma at (clip(x + ((vx + 2) >> 2)), clip(y + ((vy + 2) >> 2))); B's 8x8 chroma samples = S's chroma at
  //     (clip(xc + ((vx + 4) >> 3)), clip(yc + ((vy + 4) >> 3))); clipped to the coded plane.
  // Steps 1 and 2 run on the host when the stand-in is filled (conceal_displacements: one row of four displacements per block), step 3 is k_dec_standin
  // (conceal_kernels.hip).  Everything else is v2's: no motion, never output, grey without a source.  The checker stays at v2; tests/conceal_model.py states v3.
  int conceal_ref(int poc, bool is_lt); std::vector<PicJob::Conceal> pending_conceal_; uint64_t concealed_ = 0;
  int conceal_mode_ = 2;
  static std::vector<int16_t> conceal_displacements(const ConcealMotion *m, int w16, int h16, int p, int s);      // [h16][w16][4]: luma dx, dy, chroma dx, dy
  int16_t *d_standin_tab_ = nullptr; size_t standin_tab_cap_ = 0;      // the table on the device, allocated with the first stand-in of mode 3
  int standin_slot_ = -1; std::vector<int16_t> standin_tab_;          // debug_copy "standin" / "standin_mv": the stand-in filled last and its table
  float standin_ms_ = -1;                                              // debug_copy "standin_ms": time of the last stand-in's fill (either mode; set_profiling only)
  // Partial pictures v1 (set_partial_pictures; off by default, and with it off nothing below exists).  The statement of record; tests/partial_model.py restates it on
  // tests/pyhevc.py, the product is held to that model (the checker stays at today's behaviour).  One-tile pictures; total = the picture's coding tree blocks, next = where
  // the decoded part ends so far (0 at first).
  //  1. Segments are taken in arrival order inside an access unit; a = the segment's address.  a < next: ignored.  Independent: decoded; a > next leaves [next, a) missing.
  //     Dependent: decoded only if a == next, next > 0 and block a - 1 was decoded -- else its predecessor is gone, with its CABAC state (9.3.1), header and neighbours: the
  //     segment is dropped, next stays; a lost segment takes every following dependent one with it, up to the next independent one.  After a decoded segment next = a + the
  //     blocks it coded.  The picture ends when next == total or when something arrives that can only belong to the next access unit; then [next, total) is missing.  A
  //     picture none of whose segments was decoded is a lost picture (v2 / v3 as ever); a segment that arrives and does not parse is corruption: the picture is dropped as ever.
  //  2. A non-first segment joins the open picture if nal_unit_type and PPS match (an independent one: slice_pic_order_cnt_lsb too) and a >= next.
  //  3. A missing block has no coding units, is available (6.4.1) to nothing, files no motion (a collocated block there gives no temporal candidate; ConcealMotion: none), has
  //     no edges, and its boundary is closed to both loop filters exactly as slice_loop_filter_across_slices_enabled_flag = 0 closes one (DecFrame::ctu_nb): no received
  //     sample depends on a concealed one, the seam is unfiltered on purpose.
  //  4. Its samples, three planes, clipped to the coded picture: S = v2's choice for the damaged picture's OWN order count among the reference pictures the DPB held when the
  //     picture arrived (no stand-in made for this picture; nearest, of two the earlier); an IRAP picture that starts a coded video sequence: the held picture decoded last;
  //     none: 128.  Mode 2: S's samples at the same place.  Mode 3: per 16x16 block v3's steps 1-3 scaled to the damaged picture's order count, the neighbour test over S's
  //     whole grid, zero where S is a stand-in or S's own block was missing.
  //  5. The damaged picture is output in its turn and kept as a reference; its hash SEI is neither compared nor counted; damage is reported beside it (DecodedPicture).
  // BUILT in v1, two forms.  (a) What a Kvazaar peer's slices=wpp sends -- WPP, a dependent segment per CTB row: a lost row's segment takes every later row with it, the rows
  // before it stay (append_segment drops what rule 1 drops, close_open_picture lays the tail out as missing; PicJob::missing is set before the parse).  (b) One-tile pictures
  // in any other cut (Kvazaar's rows without WPP, free slices with or without WPP): gaps anywhere -- a first segment lost with an independent one behind it (slice_front: the segment opens the picture
  // from its own header), a middle independent or dependent one, two gaps, the tail.  The picture is put together like a picture of free slices when its access unit ends
  // (close_free_picture) and the PARSER finds the gaps (PicJob::scan_gaps, parse_substream): a segment that ends before the next one's address
  // leaves what lies between missing, a dependent successor is skipped with its bytes, an independent one takes up decoding; a missing block gets the slice byte 255, which
  // no decoded slice has (255 slices at most then).  With WPP a row thread learns from the row above whether it begins inside a gap and publishes its progress over skipped
  // blocks too (parse_substream says how).  Pictures with tiles keep today's behaviour -- dropped whole, then concealed (DESIGN.md section 9.3 "Not covered").
  // Where: parse_job gives the missing rows their records (nothing waits on them, their progress and ColMotion rows are published), fill_missing runs k_dec_fill_ctbs into the
  // picture's buffer BEHIND the picture's last kernel and before anything later is launched, on a drained device like fill_concealed -- whoever launched the picture (batch.h).
  bool partial_ = false; int cur_fill_src_ = -1, avoid_slot_ = -1;      // (cur_fill_src_: S of the picture whose first segment is being read; avoid_slot_: alloc_slot leaves S's buffer alone for it)
  void choose_fill_source(int poc, bool last_decoded, const std::vector<int> &fresh);
  std::vector<int32_t> damage_log_;
  uint32_t *d_fill_ctbs_ = nullptr; size_t fill_ctbs_cap_ = 0; int16_t *d_fill_tab_ = nullptr; size_t fill_tab_cap_ = 0;      // the list and the table on the device, allocated with the first damaged picture
  std::vector<int16_t> fill_tab_;                                       // debug_copy "fill_mv": the table used last
  bool cur_discard_ = false;     // the picture whose headers are being read empties the buffer without output (decided with its first segment)
  bool cur_no_rasl_ = false;     // NoRaslOutputFlag of the picture whose slice headers are being read (decided with its first segment)
  bool skip_rasl_ = false;       // NoRaslOutputFlag of the last IRAP picture: the RASL pictures that belong to it refer to pictures that are not there -- their NAL units are dropped
  bool download_ = true, profiling_ = false, prof_now_ = false; int prof_every_ = 1;
  bool pic_ready_ = false; DecodedPicture out_;
  int last_error_ = 0;
  double t_nal_ = 0, t_wait_ = 0, t_stage_ = 0, t_api_ = 0, t_sync_ = 0;     // decoder-thread time split (KVAZZUP_AMD_TRACE)
  std::vector<uint8_t> rbsp_;
  std::vector<size_t> epb_;                // unescaped payload offset of every removed emulation prevention byte
  std::vector<size_t> sub_start_;          // start of every substream inside the unescaped slice data
  std::unique_ptr<OrderedPool> pool_; int parse_threads_ = 16; std::mutex pool_mutex_;   // (frame workers: one picture at a time on the row pool)
  PicJob *timed_job_ = nullptr;
  double k_ms_[DK_COUNT] = {0}; uint64_t k_n_[DK_COUNT] = {0};
  template <class F> void timed(int id, F &&launch, hipStream_t st = nullptr);
};

}  // namespace kvzx
