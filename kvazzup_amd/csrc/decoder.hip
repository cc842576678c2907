// kvazzup_amd/csrc/decoder.hip -- see decoder.h.  Host half of the decoder between the header syntax (dec_syntax.hip) and the slice-data parser
// (dec_parse.hip): NAL units, picture assembly from slice segments, reference picture management (H.265 8.1.3, 8.3, C.5.2), the job ring and its frame
// workers, buffers, launches (the sample work is dec_kernels.hip), output order, band mode, picture hashes.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "stream_pool.h"
#include "pic_hash.h"
#include "decoder.h"
#include "scaling_tables.h"

namespace kvzx {

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fprintf(stderr, "kvazzup_amd: %s failed: %s\n", #expr, hipGetErrorString(e_)); return false; } } while (0)

namespace {
struct Tick { std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } };
}  // namespace

// ------------------------------------------------------------------------------------------ lifecycle
// Pictures still being parsed by frame workers are waited for and dropped (close / resolution change).
void Decoder::drop_pending()
{
  if (gpu_job_ || !gpu_q_.empty()) { sync_main(); if (stream_dl_) hipStreamSynchronize(stream_dl_); }
  if (gpu_job_) { gpu_job_->ev_used = 0; gpu_job_->dl_buf = -1; gpu_job_ = nullptr; }
  for (PicJob *j : gpu_q_) { j->ev_used = 0; j->dl_buf = -1; }
  gpu_q_.clear();
  for (; job_tail_ != job_head_; job_tail_++) {
    PicJob &job = jobs_[(size_t)(job_tail_ % jobs_.size())];
    while (job.state.load(std::memory_order_acquire) != 2) std::this_thread::yield();
    job.state.store(0, std::memory_order_relaxed);
  }
}

void Decoder::sync_main()
{
  if (batch_used_) { DecBatcher::get(device_).drain(this); batch_used_ = false; }
  hipStreamSynchronize(stream_);
  if (chain_[1].stream) hipStreamSynchronize(chain_[1].stream);
}

Decoder::~Decoder()
{
  if (getenv("KVAZZUP_AMD_TRACE")) fprintf(stderr, "kvazzup_amd decoder thread ms: nal %.1f  wait_parse %.1f  stage %.1f  gpu_api %.1f  gpu_sync %.1f  longest parse %.2f  (pictures %ld)\n", t_nal_, t_wait_, t_stage_, t_api_, t_sync_, t_parse_max_, job_tail_);
  if (parse_only_) { for (auto &j : jobs_) free(j.h_in); return; }
  drop_pending();
  workers_.reset();
  if (stream_) sync_main();
  if (batch_attached_) { DecBatcher::get(device_).detach(); batch_attached_ = false; }
  if (h_err_ && *h_err_) fprintf(stderr, "kvazzup_amd: decoder device error flags 0x%x (last picture)\n", *h_err_);
  for (auto &j : jobs_) { for (auto &e : j.ev) { hipEventDestroy(e.a); hipEventDestroy(e.b); } if (j.done) hipEventDestroy(j.done); if (j.dl_done) hipEventDestroy(j.dl_done); }
  free_buffers();
  outp_.release();                                           // (before the streams go; the member's own destructor runs it once more and finds nothing)
  if (stream_dl_ != stream_up_) stream_release(stream_dl_, device_, 'L', 'l');
  stream_release(stream_up_, device_, 'U', prio_up_);
  for (auto &e : up_done_) if (e) hipEventDestroy(e);
  if (h_err_) hipHostFree(h_err_);
  if (chain_[1].stream) stream_release(chain_[1].stream, device_, 'E', alt_prio_);
  stream_release(stream_, device_, 'D', prio_);
}

bool Decoder::start(std::string *error)
{
  if (parse_only_) { frame_threads_ = 1; started_ = true; return true; }      // (set_parse_only: the host half alone, no device)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_) {
    if (error) *error = "no usable HIP device (this library has no CPU fallback)";
    return false;
  }
  HIP_TRY(hipSetDevice(device_));
  spin_wait_ = getenv("KVAZZUP_AMD_SPIN") != nullptr;
  {
    const char *prio = getenv("KVAZZUP_AMD_PRIO");
    prio_ = (prio && strlen(prio) >= 4) ? prio[3] : 'n';
    HIP_TRY(stream_acquire(&stream_, device_, 'D', prio_));        // (stream_pool.h: a re-created decoder gets its predecessor's streams)
    chain_[0].stream = stream_;
  }
  {
    const char *prio = getenv("KVAZZUP_AMD_PRIO");          // (letters 5 and 6: the download and the upload stream)
    prio_dl_ = (prio && strlen(prio) >= 5) ? prio[4] : 'n'; prio_up_ = (prio && strlen(prio) >= 6) ? prio[5] : 'n';
  }
  // ONE transfer stream: the input blocks go up and the finished pictures come down on it, all through the copy engine and none of them ever
  // waiting inside the queue (a download is only queued once its picture's kernels are known to be done).  HIP spreads the streams of a priority
  // level over four hardware queues; with encoder and decoder in one process every further stream shares a queue with one that matters.
  HIP_TRY(stream_acquire(&stream_up_, device_, 'U', prio_up_));
  stream_dl_ = stream_up_;
  if (const char *e = getenv("KVAZZUP_AMD_DL")) if (!strcmp(e, "own")) HIP_TRY(stream_acquire(&stream_dl_, device_, 'L', 'l'));   // experiment: downloads on a stream of their own at the lowest priority level (its own pool of hardware queues)
  for (auto &e : up_done_) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // the kernels' error word (a wavefront that gave up waiting ORs a flag in) lives in host memory the device writes straight into, like the
  // encoder's: looked at when a picture completes, no copy (a copy queued on the download stream waited behind the pictures' own downloads)
  HIP_TRY(hipHostMalloc(&h_err_, sizeof(uint32_t), hipHostMallocMapped));
  *h_err_ = 0;
  { void *dp = nullptr; HIP_TRY(hipHostGetDevicePointer(&dp, h_err_, 0)); err_ = (uint32_t *)dp; }
  DecBatcher::get(device_).attach(stream_); batch_attached_ = true;
  started_ = true;
  return true;
}

void Decoder::free_buffers()
{
  for (auto &j : jobs_) { if (j.h_in) hipHostFree(j.h_in); j.h_in = nullptr; j.h_in_cap = 0; j.col.reset(); j.own.reset(); j.cown.reset(); }
  hipFree(d_standin_tab_); d_standin_tab_ = nullptr; standin_tab_cap_ = 0; standin_slot_ = -1; standin_tab_.clear();
  hipFree(d_fill_ctbs_); d_fill_ctbs_ = nullptr; fill_ctbs_cap_ = 0; hipFree(d_fill_tab_); d_fill_tab_ = nullptr; fill_tab_cap_ = 0; fill_tab_.clear();
  if (stream_dl_) hipStreamSynchronize(stream_dl_);
  for (auto &p : h_out_) { if (p) outp_.retire_host(p); p = nullptr; }      // (freed kOutHold calls later)
  for (auto &p : d_in_) { hipFree(p); p = nullptr; } for (auto &c : d_in_cap_) c = 0;
  free_chain(chain_[0]); hipFree(intra_order_); intra_order_ = nullptr;
  if (chain_[1].stream) { hipStreamSynchronize(chain_[1].stream); free_chain(chain_[1]); stream_release(chain_[1].stream, device_, 'E', alt_prio_); chain_[1].stream = nullptr; }
  alt_failed_ = false;                                       // (another picture size: the second chain's arrays may fit now)
  for (auto &p : dpb_) { hipFree(p.plane[0]); p = DpbPic(); }      // (a buffer's three planes are one allocation)
  w_ = h_ = pw_ = ph_ = 0;
}

// the arrays of one intra chain (decoder.h ChainSet; the stream is the caller's).  Tagged words: generation 0 = never written
bool Decoder::build_chain(ChainSet &cs, hipStream_t clear_on)
{
  const size_t npx = (size_t)pw_ * ph_;
  auto cleared = [&](void *p, size_t bytes) { return clear_on ? hipMemsetAsync(p, 0, bytes, clear_on) : hipMemset(p, 0, bytes); };
  HIP_TRY(hipMalloc(&cs.progress, sizeof(uint32_t) * (3 * nctb() + 1))); HIP_TRY(cleared(cs.progress, sizeof(uint32_t) * (3 * nctb() + 1)));      // (+ k_dec_intra's ticket counter)
  HIP_TRY(hipMalloc(&cs.edge_col, edge_col_words() * sizeof(uint32_t))); HIP_TRY(cleared(cs.edge_col, edge_col_words() * sizeof(uint32_t)));
  HIP_TRY(hipMalloc(&cs.edge_row, edge_row_words() * 8)); HIP_TRY(cleared(cs.edge_row, edge_row_words() * 8));
  for (int c = 0; c < 3; c++) { HIP_TRY(hipMalloc(&cs.resid[c], sizeof(int16_t) * (c ? npx / 4 : npx))); HIP_TRY(hipMalloc(&cs.work[c], c ? npx / 4 : npx)); }
  return true;
}
void Decoder::free_chain(ChainSet &cs)
{
  hipFree(cs.progress); hipFree(cs.edge_col); hipFree(cs.edge_row); for (int c = 0; c < 3; c++) { hipFree(cs.resid[c]); hipFree(cs.work[c]); }
  cs = ChainSet{cs.stream};                                  // (the stream stays: its owner releases it)
}

// host views into a job's input block
void Decoder::bind_job(PicJob &job)
{
  uint8_t *p = job.h_in;
  job.b4 = (B4Rec *)p; job.region = (TuRange *)(p + job.lay.region_off); job.ctu = (TuRange *)(p + job.lay.ctu_off);
  job.ctu_tile = p + job.lay.tile_off; job.sao = (SaoParams *)(p + job.lay.sao_off);
}

// pinned input block of a job: at least `bytes`; the fixed part written so far is kept.  Called from the
// thread that owns the job (decoder thread at allocation, the job's parse worker later).
bool Decoder::grow_job_input(PicJob &job, size_t bytes)
{
  if (bytes <= job.h_in_cap) return true;
  const size_t cap = bytes + bytes / 2;
  uint8_t *p = nullptr;
  if (parse_only_) p = (uint8_t *)aligned_alloc(64, (cap + 63) & ~(size_t)63);      // (the host half alone: plain memory)
  else if (hipSetDevice(device_) != hipSuccess || hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) return false;
  if (!p) return false;
  if (job.h_in) {
    memcpy(p, job.h_in, job.lay.fixed_bytes() < job.h_in_cap ? job.lay.fixed_bytes() : job.h_in_cap);
    if (!parse_only_ && job.early_rows.load(std::memory_order_acquire) > 0) hipStreamSynchronize(stream_up_);      // (rows of records on their way up read the old block)
    if (parse_only_) free(job.h_in); else hipHostFree(job.h_in);
  }
  job.h_in = p; job.h_in_cap = cap;
  bind_job(job);
  return true;
}

bool Decoder::ensure_buffers(int w, int h, int ctb_log2)
{
  if (w == w_ && h == h_ && ctb_log2 == ctbl_) return true;
  // Resolution change (a new SPS took effect at this IRAP picture): what the ring still holds is completed now and queued -- the
  // following calls hand it out one picture at a time, as a software decoder's bumping process would -- before the buffers go
  while (!parse_only_ && w_ && (!gpu_q_.empty() || job_tail_ != job_head_)) {      // (a band decoder's picture between its reconstruction and band_finish -- gpu_job_ -- is not finish_oldest's to complete: drop_pending below lets it go)
    const int rc = finish_oldest();
    if (rc < 0 || (rc > 0 && pic_ready_ && !offer_output(false))) { drop_pending(); break; }
  }
  if (!parse_only_ && w_) outp_.drain();                                   // a new sequence follows: what waited for later pictures of the old one leaves in POC order, one picture per call
  if (parse_only_) {
    for (auto &j : jobs_) { free(j.h_in); j.h_in = nullptr; j.h_in_cap = 0; }
    if (jobs_.empty()) jobs_ = std::vector<PicJob>(3);
    gpu_depth_ = 1;
    if (!prepare_jobs(w, h, ctb_log2)) return false;
    for (auto &d : dpb_) { d = DpbPic(); d.plane[0] = (uint8_t *)(uintptr_t)64; }      // (never dereferenced: slots are only book-keeping here)
    seen_irap_ = false;
    return true;
  }
  drop_pending();
  sync_main();
  free_buffers();
  if (jobs_.empty()) {
    const char *e = getenv("KVAZZUP_AMD_DEC_GPU_DEPTH");
    gpu_depth_ = e ? atoi(e) : (frame_threads_ >= 4 ? (frame_threads_ >= 24 ? 8 : (frame_threads_ >= 12 ? 4 : 3)) : 1);      // (an intra picture's chain is ~1.5 ms at 1080p: ten picture intervals)
    if (gpu_depth_ > kMaxGpuDepth) gpu_depth_ = kMaxGpuDepth;
    if (gpu_depth_ > frame_threads_ - 1) gpu_depth_ = frame_threads_ - 1;
    if (gpu_depth_ < 1 || band_nrows_ > 0) gpu_depth_ = 1;
    jobs_ = std::vector<PicJob>((size_t)frame_threads_ + 2);   // the pictures being parsed and queued on the GPU (frame_threads_ of them), the one being handed out, the one being filled
  }
  if (!prepare_jobs(w, h, ctb_log2)) return false;
  h_out_cap_ = (size_t)pw_ * ph_ * 3 / 2;                // (allocated by the first picture that is downloaded)
  for (int i = 0; i <= gpu_depth_; i++) { d_in_cap_[i] = jobs_[0].lay.fixed_bytes() + (1 << 20); HIP_TRY(hipMalloc(&d_in_[i], d_in_cap_[i])); }
  if (!build_chain(chain_[0], nullptr)) return false; chain_gen_ = 0;
  {
    // dispatch order of k_dec_intra's workgroups: CTUs by anti-diagonal cx + 2 cy (every CTU a block depends on comes earlier)
    const int wc = ctbs_in(w_, ctbl_), hc = ctbs_in(h_, ctbl_);      // (the picture's coding tree blocks -- with CTBs smaller than 64 fewer than the padded size holds)
    std::vector<uint32_t> order;
    const int r0 = band_nrows_ > 0 ? band_row0_ : 0, nr = band_nrows_ > 0 ? band_nrows_ : hc;      // (band mode: this decoder's CTU rows)
    if (r0 < 0 || r0 + nr > hc) return false;
    for (int d = 0; d < wc + 2 * nr; d++) for (int cy = 0; cy < nr; cy++) { const int cx = d - 2 * cy; if (cx >= 0 && cx < wc) order.push_back((uint32_t)((r0 + cy) * wc + cx)); }
    HIP_TRY(hipMalloc(&intra_order_, sizeof(uint32_t) * order.size()));
    HIP_TRY(hipMemcpy(intra_order_, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice));
  }
  for (int s = 0; s < 6; s++) if (!alloc_picture(dpb_[s])) return false;
  seen_irap_ = false;
  HIP_TRY(hipDeviceSynchronize());                       // (the clears above ran on the null stream: done before anything is queued on the decoder's non-blocking streams)
  return true;
}

// a picture buffer for the picture about to be decoded: not a reference any more and, if it was output, output long enough ago
// Concealment v2 (decoder.h): the buffer that stands in for a reference picture that never arrived.  Marked like the real one would be; its samples are set when
// the picture that asked for it is launched (the GPU may still be reading the buffer's former picture for older pictures that are in flight).
int Decoder::conceal_ref(int poc, bool is_lt)
{
  const int s = alloc_slot();
  if (s < 0) return -1;
  DpbPic &d = dpb_[s];
  d.poc = poc; d.is_ref = true; d.used = true; d.is_lt = is_lt; d.standin = true; d.motion.reset(); d.cmotion.reset();      // (decode_idx stays: the buffer was old enough to be taken and is no picture anybody waits for -- free again the moment no set names it)
  pending_conceal_.emplace_back(s, -2);                           // (-2: the source is chosen once the reference picture set has been applied, decode_slice)
  if (concealed_++ < 3) fprintf(stderr, "kvazzup_amd: decoder: reference picture with POC %d never arrived -- the nearest reference picture (or a grey one) stands in\n", poc);
  return s;
}

// a picture buffer: Y | Cb | Cr back to back in one allocation (it goes to the host in ONE copy), mid-grey.  (The clear runs on the null stream, ordered with nothing on the decoder's non-blocking streams: the caller synchronises the device.)
bool Decoder::alloc_picture(DpbPic &p)
{
  const size_t npx = (size_t)pw_ * ph_;
  if (hipMalloc(&p.plane[0], npx * 3 / 2) != hipSuccess) { p.plane[0] = nullptr; return false; }
  p.plane[1] = p.plane[0] + npx; p.plane[2] = p.plane[1] + npx / 4;
  HIP_TRY(hipMemset(p.plane[0], 128, npx * 3 / 2));
  return true;
}
// the new picture size takes effect: every ring entry gets its input block for it (ensure_buffers)
bool Decoder::prepare_jobs(int w, int h, int ctb_log2)
{
  w_ = w; h_ = h; pw_ = (w + 63) & ~63; ph_ = (h + 63) & ~63; ctbl_ = ctb_log2;
  const size_t nb4 = (size_t)pw_ * ph_ / 16;
  for (auto &j : jobs_) {
    j.lay = DecInputLayout(pw_, ph_, ctbl_, 0, 0, 0, false);
    if (!grow_job_input(j, j.lay.fixed_bytes() + (1 << 16))) return false;
    memset(j.h_in, 0, j.lay.fixed_bytes());
    j.pred_mode.assign(nb4 / 4, PM_NONE); j.ct_depth.assign(nb4 / 4, 0); j.intra_mode.assign(nb4, 1);
  }
  return true;
}

int Decoder::alloc_slot()
{
  // A picture handed out stays untouched while `hold` further pictures are begun (kvzx_decoder_set_output_hold; dec_output.h).  The synchronous decoder launches picture q
  // in the call that begins it and hands picture p out in the call that began it: q may take p's buffer when q - p > hold.  With frame threads the call that
  // begins picture k hands out picture k - frame_threads_ and launches picture k - frame_threads_ + gpu_depth_: picture q is launched gpu_depth_ calls after the one
  // that handed out q - gpu_depth_, so it may take p's buffer when q - p > hold + gpu_depth_.
  const long margin = outp_.hold() + (frame_threads_ > 1 ? gpu_depth_ : 0);
  for (int s = 0; s < kMaxPics; s++) {
    DpbPic &p = dpb_[s];
    if (p.is_ref || s == avoid_slot_ || job_head_ - p.decode_idx <= margin) continue;
    if (!p.plane[0] && parse_only_) p.plane[0] = (uint8_t *)(uintptr_t)64;
    if (!p.plane[0]) { if (hipSetDevice(device_) != hipSuccess || !alloc_picture(p)) return -1; hipDeviceSynchronize(); }      // (a buffer is added kMaxPics - 6 times at most)
    return s;
  }
  return -1;
}

template <class F> void Decoder::timed(int id, F &&launch, hipStream_t st)
{
  if (!prof_now_) { launch(); return; }
  if (!st) st = stream_;
  PicJob &j = *timed_job_;
  if (j.ev_used == j.ev.size()) { PicJob::EvPair p; hipEventCreate(&p.a); hipEventCreate(&p.b); p.id = id; j.ev.push_back(p); }
  PicJob::EvPair &p = j.ev[j.ev_used++]; p.id = id;
  hipEventRecord(p.a, st); launch(); hipEventRecord(p.b, st);
}
// the second chain's stream and arrays (decoder.h chain_[1]), on first use
bool Decoder::ensure_alt()
{
  if (chain_[1].stream) return true;
  if (alt_failed_) return false;                             // (it did not fit once: the intra-only pictures keep to the one chain instead of trying again for every picture)
  if (hipSetDevice(device_) != hipSuccess) return false;
  // the second chain's priority level = its pool of hardware queues: the LOWEST level, where nothing else of this library lives (measured, all-intra 1080p with
  // the encoder's second chain at the main stream's level: second decoder chain at the default level 1 563 frames/s -- the level's four queues are taken by
  // tokenizer, input, decoder and transfers --, at the high level 1 681, at the low one 1 724; one chain each side: 1 279)
  { const char *e = getenv("KVAZZUP_AMD_DEC_ALT_PRIO"); alt_prio_ = e ? e[0] : 'l'; }
  // Everything is built in a local and handed to the member in one piece: chain_[1].stream != NULL is what launch_gpu takes for "the second chain exists", so a
  // half-built state (a failed allocation at 4K) must never be visible -- on any failure what was allocated is freed and the stream released.
  // (Cleared ON the stream that is about to use them: a clear on the null stream is ordered with nothing on a non-blocking stream -- the second chain's first picture had its hand-off words zeroed under its hands, every wait in it gave up: error flags 3)
  ChainSet cs;
  auto build = [&]() -> bool { HIP_TRY(stream_acquire(&cs.stream, device_, 'E', alt_prio_)); return build_chain(cs, cs.stream); };
  if (!build()) {
    if (cs.stream) hipStreamSynchronize(cs.stream);          // (a clear may be queued on it)
    free_chain(cs); stream_release(cs.stream, device_, 'E', alt_prio_); (void)hipGetLastError();      // (stream_release: nothing to do without a stream)
    alt_failed_ = true; return false;
  }
  chain_[1] = cs;
  return true;
}
void Decoder::get_kernel_times(double *ms, uint64_t *launches, bool reset)
{
  for (int i = 0; i < DK_COUNT; i++) { if (ms) ms[i] = k_ms_[i]; if (launches) launches[i] = k_n_[i]; }
  if (reset) for (int i = 0; i < DK_COUNT; i++) { k_ms_[i] = 0; k_n_[i] = 0; }
}

// ------------------------------------------------------------------------------------------ NAL units
// One picture out per call at most (the libOpenHevcDecode contract).  The fast path -- a sequence that does not reorder, nothing completed ahead of its turn -- hands
// out the ring's own buffer as complete_gpu described it: no copy, no event, no allocation.  Everything else goes through DecOutput (dec_output.h): the picture this
// call completed is copied and takes its place, and the next one in output order, if its turn has come, is handed out.
int Decoder::decode_nal(const uint8_t *data, size_t len, int64_t pts)
{
  outp_.begin_call();
  int nal_type = -1;
  const int rc = decode_nal_inner(data, len, pts, nal_type);
  if (rc < 0 || (outp_.idle() && !(pic_ready_ && out_.num_reorder > 0))) return rc;
  if (pic_ready_ && !offer_output(true)) return last_error_ = DEC_ERR_GPU;
  pic_ready_ = outp_.next((nal_type == 36 || nal_type == 37) && pending() == 0, out_);      // (EOS / EOB with nothing left in the pipeline: what still waits leaves, one per call)
  return pic_ready_ ? 1 : 0;
}

// emulation prevention bytes out (7.4.2; hevc_headers.h append_nal is the inverse): the bytes between zero bytes in one piece.  The payload behind the two
// header bytes goes to rbsp_, the removed bytes' places to epb_; returns the payload's length.
size_t Decoder::unescape(const uint8_t *data, size_t len)
{
  if (rbsp_.size() < len + 32) rbsp_.resize(len + 32);
  epb_.clear();
  size_t n = 0; int zeros = 0;
  for (size_t k = 2; k < len;) {
    if (zeros == 0) {
      const uint8_t *z = (const uint8_t *)memchr(data + k, 0, len - k);
      const size_t m = z ? (size_t)(z - (data + k)) : len - k;
      memcpy(rbsp_.data() + n, data + k, m); n += m; k += m;
      if (k >= len) break;
    }
    if (zeros >= 2 && data[k] == 3) { zeros = 0; epb_.push_back(n); k++; continue; }
    rbsp_[n++] = data[k]; zeros = data[k] == 0 ? zeros + 1 : 0; k++;
  }
  memset(rbsp_.data() + n, 0, 32);                          // (readers may look a few bytes past the end)
  return n;
}

// VPS / SPS / PPS: dec_syntax reads them, the tables are kept here
int Decoder::decode_parameter_set(int nal_type, BitReader &r)
{
  int id = 0, rc;
  if (nal_type == 32) {
    VpsTiming t;
    rc = parse_vps(r, t);
    if (t.present) { vps_fps_den_ = t.fps_den; vps_fps_num_ = t.fps_num; }      // (kept even when the NAL unit then turns out too short: the order this code has always had)
  } else if (nal_type == 33) {
    DecSps s;
    if (!(rc = parse_sps(r, s, id))) sps_[id] = std::make_shared<const DecSps>(s);      // (a new object: pictures still being parsed keep the one they were coded with)
  } else {
    DecPps p;
    if (!(rc = parse_pps(r, p, id))) pps_[id] = p;
  }
  return rc ? (last_error_ = rc) : 0;
}

int Decoder::decode_nal_inner(const uint8_t *data, size_t len, int64_t pts, int &nal_type)
{
  Tick tk_nal;
  struct Acc { double &d; Tick &t; double &w, &s, &a, &y; double w0, s0, a0, y0; ~Acc() { d += t.ms() - ((w - w0) + (s - s0) + (a - a0) + (y - y0)); } } acc_{t_nal_, tk_nal, t_wait_, t_stage_, t_api_, t_sync_, t_wait_, t_stage_, t_api_, t_sync_};
  pic_ready_ = false;
  if (!started_) return last_error_ = DEC_ERR_GPU;
  size_t i = 0;
  while (i + 2 < len && data[i] == 0) i++;
  if (i >= 2 && i < len && data[i] == 1) { data += i + 1; len -= i + 1; }
  if (len < 2 || (data[0] & 0x80)) return last_error_ = DEC_ERR_INVALID;      // EOS / EOB are header-only
  nal_type = (data[0] >> 1) & 0x3f; const int layer = ((data[0] & 1) << 5) | (data[1] >> 3);
  if (layer != 0) return 0;
  cur_tid_ = (data[1] & 7) - 1;
  if (nal_type < 32 && cur_tid_ > max_tid_) return 0;            // (set_max_temporal_id: a sub-layer the caller does not want)
  const size_t n = unescape(data, len);
  BitReader r(rbsp_.data(), n);
  // (partial pictures: a picture in the row form that is built -- one tile, WPP -- is closed here too, with what it has)
  const bool open_rows = partial_ && asm_.active && !jobs_.empty() && jobs_[(size_t)(job_head_ % jobs_.size())].pps.wpp && jobs_[(size_t)(job_head_ % jobs_.size())].pps.tile_rows == 1 && jobs_[(size_t)(job_head_ % jobs_.size())].pps.tile_cols == 1;
  if (asm_.active && (asm_.guessed_one_row || asm_.free || open_rows) && nal_type >= 32 && nal_type <= 40 && nal_type != 38) { const int rc = close_open_picture(); if (rc < 0) return rc; }   // (what can only open the next access unit, or end the sequence)
  if (nal_type >= 32 && nal_type <= 34) return decode_parameter_set(nal_type, r);
  if (nal_type == 36 || nal_type == 37) { outp_.begin_picture(); after_eos_ = true; outp_.sequence_ended(); int rc = finish_oldest(); if (rc < 0) last_error_ = rc; return rc; }   // EOS / EOB: drain one delayed picture; whatever picture follows starts a sequence
  if (nal_type == 40 && check_hash_) return hash_sei(rbsp_.data(), n);       // suffix SEI: decoded picture hash (libOpenHevcSetCheckMD5)
  if (nal_type > 31) return 0;                                    // AUD / other SEI / ...
  if (!(nal_type <= 9 || (nal_type >= 16 && nal_type <= 21))) return last_error_ = DEC_ERR_UNSUPPORTED;      // (reserved types)
  int rc = decode_slice(rbsp_.data(), n, nal_type, pts);
  if (rc < 0) last_error_ = rc;
  return rc;
}

// Decoded picture hash SEI (D.2.19, payload type 132) with libOpenHevcSetCheckMD5(h, 1): the message follows its picture's last slice
// segment.  Frame-threaded decoder: the picture is still in the ring -- the expected hashes travel with its job and are compared when the
// picture completes.  Synchronous decoder: the picture has just been output and still sits untouched in its buffer -- compared at once.
int Decoder::hash_sei(const uint8_t *rbsp, size_t len)
{
  BitReader r(rbsp, len);
  while (r.pos + 16 <= len * 8 && !r.err) {
    int type = 0, size = 0, b;
    do { b = (int)r.get(8); type += b; } while (b == 255 && !r.err);
    do { b = (int)r.get(8); size += b; } while (b == 255 && !r.err);
    if (r.err || r.pos + (size_t)size * 8 > len * 8) break;
    if (type != 132 || size < 1) { for (int k = 0; k < size; k++) r.get(8); continue; }
    std::vector<uint8_t> want((size_t)size);
    for (int k = 0; k < size; k++) want[(size_t)k] = (uint8_t)r.get(8);
    const int ht = want[0];
    if ((ht != 0 && ht != 2) || size != 1 + 3 * (ht == 0 ? 16 : 4)) continue;      // (CRC: not checked)
    if (job_head_ == 0) continue;
    PicJob &job = jobs_[(size_t)((job_head_ - 1) % (long)jobs_.size())];
    if (parse_only_) continue;
    if (!job.missing.empty()) continue;                     // (partial pictures: a damaged picture's hash is neither compared nor counted)
    if (frame_threads_ > 1 || band_nrows_ > 0) { job.expect_hash = std::move(want); continue; }
    const int rc = verify_hash(job, want);
    if (rc < 0) return last_error_ = rc;
  }
  return 0;
}

// the picture of `job` (complete on the device) against the hashes of its SEI message; the samples come down once more for it
int Decoder::verify_hash(const PicJob &job, const std::vector<uint8_t> &want)
{
  const size_t npx = (size_t)pw_ * ph_;
  std::vector<uint8_t> pic(npx * 3 / 2);
  if (hipSetDevice(device_) != hipSuccess || hipMemcpy(pic.data(), dpb_[job.slot].plane[0], pic.size(), hipMemcpyDeviceToHost) != hipSuccess) return DEC_ERR_GPU;
  const uint8_t *pl[3] = {pic.data(), pic.data() + npx, pic.data() + npx + npx / 4};
  const size_t pitch[3] = {(size_t)pw_, (size_t)pw_ / 2, (size_t)pw_ / 2};
  const std::vector<uint8_t> got = picture_hash_payload(want[0], pl, pitch, w_, h_);
  hash_checked_++;
  if (got != want) {
    hash_mismatch_++;
    fprintf(stderr, "kvazzup_amd: decoded picture hash mismatch (POC %d)\n", job.sh.poc);
    return DEC_ERR_HASH;
  }
  return 0;
}

// A picture whose last slice segment has not arrived when something that can only belong to the NEXT access unit turns up (a first slice
// segment, a parameter set, an access unit delimiter, a prefix SEI, the end of the sequence).  Either its first segment's extent was guessed
// wrong -- a one-tile picture without WPP whose PPS allows dependent slice segments is taken to begin with a one-row segment
// (append_segment), but the flag does not forbid whole pictures in one segment: then the segment IS the picture, it ends where its
// end_of_slice_segment_flag says and is submitted now, ahead of the NAL unit at hand -- or segments were lost and the picture is dropped,
// which must not pass unnoticed: the error code is left for kvzx_decoder_last_error and said once on stderr.
// A picture of free slices (append_segment) when its access unit has ended: every segment ends where the next begins, the last one with the picture.  What
// the parser needs per coding tree block -- which slice, whether a segment begins or ends there, where its bytes are -- is laid out here; the substreams
// stay what they are for any one-tile picture (a CTB row each with WPP, else the picture), a segment that begins inside one restarts the arithmetic decoder there.
int Decoder::close_free_picture(PicJob &job)
{
  const int wc = ctbs_in(w_, ctbl_), hc = ctbs_in(h_, ctbl_), total = wc * hc, n = (int)asm_.segs.size();
  const bool wpp = job.pps.wpp != 0;
  const bool headless = partial_ && n >= 1 && asm_.segs[0].address != 0 && !asm_.segs[0].dependent;      // (partial pictures: the picture's first segment never arrived)
  if (n < 1 || (asm_.segs[0].address != 0 && !headless) || asm_.segs[0].dependent) return DEC_ERR_INVALID;
  if (n == 1 && frame_threads_ == 1 && !headless) free_stream_ = false;      // (one segment: the stream may be back to whole pictures -- the synchronous decoder can afford to find out, submit_job take_back)
  if (n == 1 && !headless && !(partial_ && wpp && (int)asm_.segs[0].subs.size() < hc)) {      // (partial pictures with WPP: a single segment that holds fewer rows than the picture has lost its tail)
    // the whole picture in one segment: the layout of Kvazaar's forms -- nothing per coding tree block, the parser's availability tests as they were
    if ((int)asm_.segs[0].subs.size() != (wpp ? hc : 1)) return DEC_ERR_INVALID;
    job.ctb_cut.clear(); job.ctb_slice.clear(); job.ctb_data.clear(); job.slice_qps.clear();
    job.sub_start = asm_.segs[0].subs;
    job.seg_end_row.assign((size_t)hc, 0); job.seg_end_row[(size_t)hc - 1] = 1; job.row_restart.assign((size_t)hc, SIZE_MAX);
    job.seg_end_sub.assign(job.geom.size(), 0);
    return 0;
  }
  job.ctb_cut.assign((size_t)total, 0); job.ctb_slice.assign((size_t)total, 0); job.ctb_data.assign((size_t)total, SIZE_MAX); job.slice_qps.clear();
  job.sub_start.assign(wpp ? (size_t)hc : 1, SIZE_MAX);
  job.seg_end_row.assign((size_t)hc, 0); job.row_restart.assign((size_t)hc, SIZE_MAX);
  job.row_seg_start.assign((size_t)hc, -1);
  int slice = -1;
  for (int k = 0; k < n; k++) {
    const FreeSeg &sg = asm_.segs[(size_t)k];
    const int a = sg.address; int e = k + 1 < n ? asm_.segs[(size_t)k + 1].address : total;
    // (partial pictures with WPP: the entry points say how many rows the segment goes into -- it ends in the last of them at the latest; what lies between that row's end
    // and the next segment that arrived is missing whatever the parser finds)
    if (partial_ && wpp && a >= 0 && !sg.subs.empty() && (long)(a / wc + (int)sg.subs.size()) * wc < e) e = (a / wc + (int)sg.subs.size()) * wc;
    if (a < 0 || e <= a || e > total || sg.subs.empty()) return DEC_ERR_INVALID;
    if (!sg.dependent) { if (++slice > (partial_ ? 254 : 255)) return DEC_ERR_UNSUPPORTED; job.slice_qps.push_back((int8_t)sg.slice_qp); }      // (the kernels tell slices apart by a byte per block)
    job.ctb_cut[(size_t)a] |= sg.dependent ? 2 : 1; job.ctb_cut[(size_t)e - 1] |= 4; job.ctb_data[(size_t)a] = sg.subs[0];
    memset(job.ctb_slice.data() + a, slice, (size_t)(e - a));
    const int rows = (e - 1) / wc - a / wc + 1;
    if (wpp) {
      if ((int)sg.subs.size() != rows) return DEC_ERR_INVALID;      // (an entry point per CTB row the segment goes on into)
      for (int q = 0; q < rows; q++) if (q > 0 || a % wc == 0) { job.sub_start[(size_t)(a / wc + q)] = sg.subs[(size_t)q]; if (q > 0) job.row_seg_start[(size_t)(a / wc + q)] = a; }
    } else {
      if (sg.subs.size() != 1) return DEC_ERR_INVALID;
      if (k == 0) job.sub_start[0] = sg.subs[0];
    }
  }
  { size_t last = SIZE_MAX;      // (partial pictures with WPP: a row that lies in a gap has no bytes)
    for (size_t q = 0; q < job.sub_start.size(); q++) {
      if (job.sub_start[q] == SIZE_MAX) { if (partial_ && wpp) continue; return DEC_ERR_INVALID; }
      if (last != SIZE_MAX && job.sub_start[q] <= last) return DEC_ERR_INVALID;
      last = job.sub_start[q];
    }
    if (last == SIZE_MAX && !(partial_ && wpp)) return DEC_ERR_INVALID; }
  if (wpp) job.ds_saved.assign((size_t)hc * CTX_COUNT, 0);
  for (int cy = 0; cy < hc; cy++) memcpy(job.ctu_tile + (size_t)cy * wc, job.ctb_slice.data() + (size_t)cy * wc, (size_t)wc);      // (one tile: the byte the kernels compare between adjacent blocks is the slice's)
  job.sh.slice_qp = job.slice_qps[0];
  job.seg_end_sub.assign(job.geom.size(), 0);
  return 0;
}

// close_open_picture's three ways end alike: the picture is submitted (unless laying it out failed: rc < 0), an error is kept for kvzx_decoder_last_error --
// the NAL unit at hand is not to blame -- and a picture that comes out is stashed: handed out first, by the next call (the NAL unit at hand may produce one of its own)
int Decoder::submit_closed(PicJob &job, int rc)
{
  if (rc >= 0) rc = submit_job(job, asm_.nal_type, asm_.irap);
  if (rc < 0) { last_error_ = rc; return 0; }
  if (rc > 0 && pic_ready_ && !offer_output(false)) return last_error_ = DEC_ERR_GPU;
  return 0;
}

int Decoder::close_open_picture()
{
  if (!asm_.active) return 0;
  asm_.active = false;
  PicJob &old = jobs_[(size_t)(job_head_ % jobs_.size())];
  const int old_hc = ctbs_in(h_, ctbl_);
  if (asm_.free) {
    asm_.free = false;
    const int rc = close_free_picture(old);
    old.ambiguous_end = false;
    return submit_closed(old, rc);
  }
  if (asm_.guessed_one_row && asm_.rows == 1 && old_hc > 1) {
    asm_.guessed_one_row = false;
    old.seg_end_row[0] = 0; old.seg_end_row[(size_t)(old_hc - 1)] = 1;
    return submit_closed(old, 0);
  }
  if (partial_ && old.pps.wpp && old.pps.tile_rows == 1 && old.pps.tile_cols == 1 && band_nrows_ == 0 && asm_.rows > 0 && asm_.rows < old_hc) {
    // partial pictures v1 (decoder.h), Kvazaar's row form: with WPP the entry points say how many rows every segment holds -- rows [0, asm_.rows) arrived, the segment
    // of row asm_.rows was lost and took the dependent ones behind it along (append_segment dropped them): the tail is missing, the picture is kept
    const int wc = ctbs_in(w_, ctbl_);
    old.missing.assign(1, std::make_pair(asm_.rows * wc, (old_hc - asm_.rows) * wc));
    old.ambiguous_end = false;
    return submit_closed(old, 0);
  }
  if (old.pps.tile_rows == 1 && old.pps.tile_cols == 1 && band_nrows_ == 0 && asm_.segs.size() > 1) {
    // One tile, and the rows counted so far do not make the picture: they were counted on guesses -- without WPP no header says how far a segment reaches, a
    // dependent segment at a row's start was taken for that one row (the form Kvazaar's slices=wpp has WITH WPP).  The stream cuts its pictures as it likes after
    // all (it had looked like whole pictures again: close_free_picture's single-segment rule): the segments are all here, each ends where the next begins, the last
    // one with the picture.  If one was lost instead, the parser finds a segment ending early and the picture fails there.
    asm_.guessed_one_row = false;
    const int rc = close_free_picture(old);
    old.ambiguous_end = false;
    if (rc >= 0) free_stream_ = true;
    return submit_closed(old, rc);
  }
  last_error_ = DEC_ERR_INVALID;
  static bool said = false;
  if (!said) { said = true; fprintf(stderr, "kvazzup_amd: decoder dropped a picture whose slice segments did not complete before the next picture began\n"); }
  return 0;
}

// what decode_slice's steps hand on to each other: the reader and the NAL unit, the header as far as it is read, the lists apply_rps_and_build_lists builds
struct Decoder::SliceCtx {
  BitReader r; const uint8_t *rbsp; size_t len; int nal_type; int64_t pts; bool idr, irap;
  bool first_seg = false, opens = false, prior_flag = false, dependent = false; int pps_id = 0, seg_address = 0;      // prior_flag: no_output_of_prior_pics_flag
  const DecPps *p = nullptr; std::shared_ptr<const DecSps> sps; PicJob *open = nullptr;                  // open: the picture under way a further segment joins
  SliceHdr sh; StRps rps; LtRefs lt; bool across_slices = true;
  int nref = 0, ref_poc[16]; uint8_t ref_slot[16], ref_lt[16] = {};
  int nref1 = 0, ref_poc1[16]; uint8_t ref_slot1[16], ref_lt1[16] = {};
  bool no_backward = true;
  SliceCtx(const uint8_t *b, size_t n, int t, int64_t ts) : r(b, n), rbsp(b), len(n), nal_type(t), pts(ts), idr(t == 19 || t == 20), irap(t >= 16 && t <= 23) {}
};

// A picture may come in several slice segments, one NAL unit each -- the two ways a Kvazaar peer cuts them (uvgComm video/Slices,
// kvazaarfilter.cpp:205-215): a DEPENDENT slice segment per CTU row ("slices=wpp"), an independent slice per tile ("slices=tiles").
// Supported: segments that arrive in order and consist of whole CTU rows (WPP) or whole tiles; independent slices repeat the first
// one's header (the picture keeps one set of slice parameters).  The job is filled segment by segment and submitted with the last.
// slice_front: the header up to the segment address, and what it decides -- a RASL picture that is dropped, a segment without its picture, a picture that never got
// its last segment, a picture taken back from a frame worker, a stream that turns out to cut free slices.  false: decode_slice returns rc.
bool Decoder::slice_front(SliceCtx &c, int &rc)
{
  BitReader &r = c.r;
  c.first_seg = r.get(1) != 0;
  c.prior_flag = c.irap && r.get(1) != 0;
  if ((c.nal_type == 8 || c.nal_type == 9) && skip_rasl_) {
    // a RASL picture of an IRAP picture that starts a coded video sequence (8.1.3: decoding began there, or a splicer called it BLA, or an end of sequence
    // NAL unit precedes it): it predicts from pictures of the sequence before, which are not there -- not decoded, not output
    rc = (c.first_seg && asm_.active) ? close_open_picture() : 0;
    return false;
  }
  c.pps_id = r.ue();
  if (c.pps_id < 0 || c.pps_id > 63 || !pps_[c.pps_id].valid || !sps_[pps_[c.pps_id].sps_id] || !sps_[pps_[c.pps_id].sps_id]->valid) { rc = DEC_ERR_INVALID; return false; }
  c.p = &pps_[c.pps_id]; c.sps = sps_[c.p->sps_id];
  const DecPps &p = *c.p; const DecSps &s = *c.sps;
  if (!c.first_seg) {
    const int nctb = s.wc() * s.hc();
    int bits = 0; while ((1 << bits) < nctb) bits++;
    if (p.dependent_slices) c.dependent = r.get(1) != 0;
    c.seg_address = r.get(bits);
    if (!asm_.active && frame_threads_ > 1 && !parse_only_ && job_head_ > job_tail_ && c.pps_id == asm_.pps_id && c.nal_type == asm_.nal_type) {
      // frame threads: the picture this segment may belong to is with a worker -- submitted because its segments covered it row by row (PicJob::ambiguous_end).
      // The worker's verdict is waited for (a parse that ends early is a short one): "its last segment ends before the picture does" takes the picture back,
      // open again, and this segment joins it.
      PicJob &last = jobs_[(size_t)((job_head_ - 1) % jobs_.size())];
      if (last.ambiguous_end) {
        for (int st; (st = last.state.load(std::memory_order_acquire)) == 1;) futex_wait(last.state, st);
        if (last.state.load(std::memory_order_acquire) == 2 && last.rc == DEC_SEG_ENDS_EARLY) take_back_job(last);
      }
    }
    if (!asm_.active && p.tile_cols == 1 && p.tile_rows == 1 && (!c.dependent || c.seg_address % s.wc() != 0)) {
      // no picture is open, and this is no segment of Kvazaar's forms (a dependent segment per CTU row): the stream cuts its pictures into slices as it likes -- its
      // first picture went off as one segment (where a picture without WPP ends is not in its first segment's header).  From here on a picture of this stream is put
      // together from its segments when its access unit ends (append_segment, close_free_picture); this one is lost.
      free_stream_ = true;
    }
    if (asm_.active && partial_ && !c.dependent && p.tile_cols == 1 && p.tile_rows == 1 && band_nrows_ == 0 && (c.pps_id != asm_.pps_id || c.nal_type != asm_.nal_type)) {
      // (rule 2: an independent segment of ANOTHER picture -- the open one is closed with what it has)
      if ((rc = close_open_picture()) < 0) return false;
    }
    if (!asm_.active && partial_ && !c.dependent && p.tile_cols == 1 && p.tile_rows == 1 && band_nrows_ == 0) {
      // partial pictures v1, rule 2: an independent segment with no picture open opens one from its own header -- everything a first segment does; what lies in front of
      // its address is missing
      c.opens = true; c.open = nullptr;
      return true;
    }
    if (!asm_.active || c.pps_id != asm_.pps_id || c.nal_type != asm_.nal_type) { rc = DEC_ERR_INVALID; return false; }      // a segment without its picture's first one (lost), or of another picture
  } else if (asm_.active) {
    // the previous picture never got its last segment: close_open_picture() submits or drops it; this NAL unit -- a new picture -- is decoded normally
    rc = close_open_picture();
    if (rc < 0) return false;
  }
  c.open = c.first_seg ? nullptr : &jobs_[(size_t)(job_head_ % jobs_.size())];
  if (c.dependent && c.open->pps.tile_cols > 1) { asm_.active = false; rc = DEC_ERR_UNSUPPORTED; return false; }     // (with tile columns: whole pictures or slices of whole tiles)
  return true;
}

// 8.1.3 NoRaslOutputFlag: an IDR or BLA picture, or a CRA picture that is the first one decoded or follows an end of sequence NAL unit, starts a coded video
// sequence -- POC MSBs from zero, no reference picture survives, its RASL pictures are dropped.  (first_seg: an open picture has been closed above, seen_irap_ is current.)
void Decoder::sequence_state(const SliceCtx &c)
{
  cur_no_rasl_ = c.irap && (c.idr || c.nal_type <= 18 || !seen_irap_ || after_eos_); if (c.irap) skip_rasl_ = cur_no_rasl_;
  // C.5.2.2: an IDR or BLA picture that is not the first one empties the buffer WITHOUT output when its flag says so (a CRA picture gets here behind an end of
  // sequence NAL unit only, which has put out everything already)
  cur_discard_ = cur_no_rasl_ && c.prior_flag && c.nal_type != 21 && seen_irap_ && !after_eos_;
  after_eos_ = false;
}

// ---- reference picture set (8.3.2) and RefPicList0 / 1 (8.3.4): pictures not in the set stop being references; a picture the set needs and the buffer does not
// hold gets a stand-in (conceal_ref)
int Decoder::apply_rps_and_build_lists(SliceCtx &c)
{
  const SliceHdr &sh = c.sh; const StRps &rps = c.rps; const DecSps &s = *c.sps;
  cur_fill_src_ = avoid_slot_ = -1;
  if (partial_ && cur_no_rasl_) choose_fill_source(sh.poc, true, std::vector<int>());      // (before the sequence before lets go of its pictures)
  if (cur_no_rasl_) for (auto &d : dpb_) d.is_ref = false;         // (8.3.2; what a CRA or BLA picture's set names is for its RASL pictures)
  if (!c.idr) {
    int cand_slot[32], nc = 0, nbefore = 0;             // the used pictures: those before the current one in output order (nearest first), then those after it, then the long-term ones
    bool keep[kMaxPics] = {false};
    // the long-term entries first, among all reference pictures (8.3.2): by the POC's LSBs, or by the whole POC when delta_poc_msb_present_flag says how many LSB
    // cycles back -- what they name is a long-term reference picture from now on; the short-term entries name pictures among the rest
    int lt_slot[16], nl = 0;
    const int max_lsb = 1 << s.log2_max_poc_lsb;
    for (int k = 0; k < c.lt.n; k++) {
      const long long full = (long long)sh.poc - (long long)c.lt.cycle[k] * max_lsb - (sh.poc & (max_lsb - 1)) + c.lt.lsb[k];      // (64 bits: a hostile cycle count must not wrap into a POC that exists)
      int found = -1;
      for (int q = 0; q < kMaxPics; q++) if (dpb_[q].is_ref && dpb_[q].used && (c.lt.msb[k] ? dpb_[q].poc == full : (dpb_[q].poc & (max_lsb - 1)) == c.lt.lsb[k])) found = q;
      if (found < 0 && c.lt.used[k] && !sh.is_intra) {               // lost on the way: a grey picture stands in (known by its LSBs alone: the nearest POC before the current one that has them)
        long long at = full; if (!c.lt.msb[k]) { at = (long long)sh.poc - (sh.poc & (max_lsb - 1)) + c.lt.lsb[k]; if (at >= sh.poc) at -= max_lsb; }
        found = conceal_ref((int)at, true);
        if (found < 0) return DEC_ERR_INVALID;
      }
      if (found >= 0) { keep[found] = true; dpb_[found].is_lt = true; }
      if (c.lt.used[k]) { if (found < 0 && !sh.is_intra) return DEC_ERR_INVALID; if (found >= 0) lt_slot[nl++] = found; }
    }
    for (int k = 0; k < rps.n_neg + rps.n_pos; k++) {
      const int poc = sh.poc + rps.dpoc[k];
      int found = -1;
      for (int q = 0; q < kMaxPics; q++) if (dpb_[q].is_ref && dpb_[q].used && !dpb_[q].is_lt && dpb_[q].poc == poc) found = q;
      if (found < 0 && rps.used[k] && !sh.is_intra) {
        bool lt_has_it = false;                                  // (a long-term picture of that POC is no short-term entry's picture: that stays an error)
        for (int q = 0; q < kMaxPics; q++) lt_has_it |= dpb_[q].is_ref && dpb_[q].used && dpb_[q].is_lt && dpb_[q].poc == poc;
        if (!lt_has_it) found = conceal_ref(poc, false);
      }
      if (found >= 0) keep[found] = true;
      if (rps.used[k]) { if (found < 0 && !sh.is_intra) return DEC_ERR_INVALID; if (found >= 0 && nc < 16) { cand_slot[nc++] = found; if (k < rps.n_neg) nbefore = nc; } }      // a missing reference picture (lost access unit)
    }
    // stand-ins made above (conceal_ref): each a copy of the reference picture nearest in output order among those the DPB holds NOW, before this picture's set is
    // applied (with one reference picture per picture the set names the lost picture and nothing else), of two equally near the earlier one; no stand-in of this
    // same picture is a source.  (The source may be dropped by the set and become this picture's own buffer: the copy runs before the picture's kernels.)
    std::vector<int> fresh;
    for (const auto &pc : pending_conceal_) if (pc.second == -2) fresh.push_back(pc.first);
    if (partial_ && !cur_no_rasl_) choose_fill_source(sh.poc, false, fresh);
    for (auto &pc : pending_conceal_) if (pc.second == -2) {
      int best = -1;
      for (int q = 0; q < kMaxPics; q++) {
        if (!dpb_[q].is_ref || !dpb_[q].used || std::find(fresh.begin(), fresh.end(), q) != fresh.end()) continue;
        const long long dq = llabs((long long)dpb_[q].poc - dpb_[pc.first].poc), db = best < 0 ? 0 : llabs((long long)dpb_[best].poc - dpb_[pc.first].poc);
        if (best < 0 || dq < db || (dq == db && dpb_[q].poc < dpb_[best].poc)) best = q;
      }
      pc.second = best;                                            // (-1: none -- grey)
      if (conceal_mode_ == 3 && best >= 0) { pc.poc = dpb_[pc.first].poc; pc.src_poc = dpb_[best].poc; pc.motion = dpb_[best].cmotion; }      // (v3: the source's motion goes with the entry -- the buffer may be another picture's by the time it is filled; NULL: the source is a stand-in)
    }
    for (int q = 0; q < kMaxPics; q++) if (!keep[q]) dpb_[q].is_ref = false;
    if (!sh.is_intra) {
      const int nst = nc;                                 // (the short-term part of the temporary lists)
      for (int k = 0; k < nl && nc < 32; k++) cand_slot[nc++] = lt_slot[k];
      if (nc == 0 || nc > 16) return DEC_ERR_INVALID;
      // 8.3.4: RefPicList0 = before, after, long-term, repeated; RefPicList1 = after, before, long-term, repeated
      c.nref = sh.num_ref_idx;
      // (a modified list names entries of the temporary list; nc = NumPicTotalCurr here: a used picture that is missing ended the call above)
      for (int k = 0; k < c.nref; k++) {
        const int q = sh.list_mod[0] ? imin(sh.list_entry[0][k], nc - 1) : k % nc;
        c.ref_slot[k] = (uint8_t)cand_slot[q]; c.ref_lt[k] = (uint8_t)(q >= nst); c.ref_poc[k] = dpb_[c.ref_slot[k]].poc; if (c.ref_poc[k] > sh.poc) c.no_backward = false;
      }
      c.nref1 = sh.is_b ? sh.num_ref_idx1 : 0;
      const int nafter = nst - nbefore;
      for (int k = 0; k < c.nref1; k++) {
        const int q = sh.list_mod[1] ? imin(sh.list_entry[1][k], nc - 1) : k % nc;
        c.ref_slot1[k] = (uint8_t)cand_slot[q >= nst ? q : (q < nafter ? nbefore + q : q - nafter)]; c.ref_lt1[k] = (uint8_t)(q >= nst); c.ref_poc1[k] = dpb_[c.ref_slot1[k]].poc;
        if (c.ref_poc1[k] > sh.poc) c.no_backward = false;
      }
    }
  }
  return 0;
}

// ---- hand the picture to a parse job.  With frame threads (libOpenHevcInit thread_type FRAME / FRAMESLICE)
// up to `frame_threads_` pictures are parsed concurrently on worker threads and the output is delayed accordingly,
// like OpenHEVC's frame threading; temporal motion prediction makes a picture's parser follow the collocated
// picture's parser row by row (ColMotion::row_done).  The job's fields and the assembly state start afresh.
Decoder::PicJob &Decoder::open_job(const SliceCtx &c, const DecPps &pp, int slot)
{
  const SliceHdr &sh = c.sh; const DecSps &s = *c.sps;
  const int wc = s.wc(), hc = s.hc();
  PicJob &job = jobs_[(size_t)(job_head_ % jobs_.size())];
  job.rbsp.clear(); job.data_off = 0; job.data_len = 0; job.sub_start.clear(); job.expect_hash.clear();
  job.seg_end_row.assign((size_t)hc, 0); job.row_restart.assign((size_t)hc, SIZE_MAX);
  job.across_slices = c.across_slices;
  job.sh = sh; job.sps = c.sps; job.pps = pp; job.pts = c.pts;
  job.crop[0] = s.crop_l; job.crop[1] = s.crop_r; job.crop[2] = s.crop_t; job.crop[3] = s.crop_b;
  if (no_crop_) job.crop[0] = job.crop[1] = job.crop[2] = job.crop[3] = 0;
  job.fps_num = s.fps_num ? s.fps_num : vps_fps_num_; job.fps_den = s.fps_num ? s.fps_den : vps_fps_den_;
  job.slot = slot; job.nref = c.nref;
  outp_.begin_picture();                                         // (a picture has begun: dec_output.h)
  // the kernels' table of picture buffers (decoder.h dpb_): entry k is buffer k; a reference picture in a buffer past the table's end takes an entry whose own
  // buffer neither list names (the lists name 16 distinct pictures at most, apply_rps_and_build_lists) -- the records then name the picture by that entry
  uint8_t entry_of[kMaxPics];
  {
    bool taken[KVZ_DEC_MAX_REFS] = {false};
    for (int k = 0; k < KVZ_DEC_MAX_REFS; k++) job.ref_buf[k] = (uint8_t)k;
    for (int b = 0; b < kMaxPics; b++) entry_of[b] = (uint8_t)(b < KVZ_DEC_MAX_REFS ? b : 0xff);
    for (int k = 0; k < c.nref; k++) if (c.ref_slot[k] < KVZ_DEC_MAX_REFS) taken[c.ref_slot[k]] = true;
    for (int k = 0; k < c.nref1; k++) if (c.ref_slot1[k] < KVZ_DEC_MAX_REFS) taken[c.ref_slot1[k]] = true;
    auto place = [&](uint8_t buf) {
      if (entry_of[buf] != 0xff) return;
      int e = 0; while (e < KVZ_DEC_MAX_REFS - 1 && taken[e]) e++;
      taken[e] = true; entry_of[buf] = (uint8_t)e; job.ref_buf[e] = buf;
    };
    for (int k = 0; k < c.nref; k++) place(c.ref_slot[k]);
    for (int k = 0; k < c.nref1; k++) place(c.ref_slot1[k]);
  }
  for (int k = 0; k < 16; k++) { job.ref_poc[k] = k < c.nref ? c.ref_poc[k] : sh.poc; job.ref_slot[k] = k < c.nref ? entry_of[c.ref_slot[k]] : 0; job.ref_lt[k] = k < c.nref ? c.ref_lt[k] : 0; job.ref_lt1[k] = k < c.nref1 ? c.ref_lt1[k] : 0; }
  if (cur_no_rasl_) cvs_++;
  job.starts_cvs = cur_no_rasl_; job.discard_prior = cur_discard_;
  job.missing.clear(); job.fill_src = cur_fill_src_; job.fill_motion.reset();
  if (cur_fill_src_ >= 0) { job.fill_src_poc = dpb_[cur_fill_src_].poc; if (conceal_mode_ == 3) job.fill_motion = dpb_[cur_fill_src_].cmotion; }
  job.conceal = std::move(pending_conceal_); pending_conceal_.clear();                     // a new coded video sequence: its pictures follow ALL of the last one's in output order
  job.cvs = cvs_;
  job.nref1 = c.nref1; job.no_backward = c.no_backward;
  for (int k = 0; k < 16; k++) { job.ref_poc1[k] = k < c.nref1 ? c.ref_poc1[k] : sh.poc; job.ref_slot1[k] = k < c.nref1 ? entry_of[c.ref_slot1[k]] : 0; }
  job.col.reset();
  if (sh.tmvp && !sh.is_intra) job.col = dpb_[(sh.is_b && !sh.collocated_from_l0) ? c.ref_slot1[sh.collocated_ref_idx] : c.ref_slot[sh.collocated_ref_idx]].motion;      // 8.5.3.2.8
  job.any_bi.store(0, std::memory_order_relaxed);
  if (sh.is_b) {                                                 // two-list motion for the parser's derivations, second vectors for the kernels
    const size_t nb4 = (size_t)(pw_ / 4) * (ph_ / 4);
    PicJob::MvF none; memset(&none, 0, sizeof(none)); none.ref[0] = none.ref[1] = -1;
    job.mvf.assign(nb4, none);
    if (job.b4x.size() != nb4) job.b4x.assign(nb4, B4L1());
  } else if (sh.weighted) {                                      // a P slice with pred_weight_table(): the blocks' weight table entries
    const size_t nb4 = (size_t)(pw_ / 4) * (ph_ / 4);
    if (job.b4x.size() != nb4) job.b4x.assign(nb4, B4L1());
  }
  job.cown.reset();
  if (conceal_mode_ == 3) {                                      // concealment v3: the picture's motion per 16x16 block, should it become the source of a stand-in
    job.cown = std::make_shared<ConcealMotion>();
    job.cown->w16 = (s.width + 15) / 16; job.cown->h16 = (s.height + 15) / 16;
    ConcealMotion::E none; memset(&none, 0, sizeof(none)); none.none = 1;
    job.cown->e.assign((size_t)job.cown->w16 * job.cown->h16, none);
  }
  job.own.reset();
  if (s.tmvp) {                                                 // (only streams with temporal prediction ever read it)
    job.own = std::make_shared<ColMotion>();
    job.own->w16 = (s.width + 15) / 16; job.own->h16 = (s.height + 15) / 16; job.own->hc = hc; job.own->poc = sh.poc;
    job.own->mv.resize((size_t)job.own->w16 * job.own->h16);
    job.own->row_done.reset(new std::atomic<uint8_t>[(size_t)hc]);
    for (int k = 0; k < hc; k++) job.own->row_done[(size_t)k].store(0, std::memory_order_relaxed);
  }
  for (int cy = 0, t = 0; cy < hc; cy++) {
    while (cy >= pp.row_bd[t + 1]) t++;
    // the kernels only ever ask whether two ADJACENT CTUs (side by side, above, diagonal) lie in the same tile: (row mod 16, column mod 16)
    // tells adjacent tiles apart in one byte for any grid (a row-major index would need 20 x 22 = 440 values)
    for (int tc = 0; tc < pp.tile_cols; tc++) memset(job.ctu_tile + (size_t)cy * wc + pp.col_bd[tc], ((t & 15) << 4) | (tc & 15), (size_t)(pp.col_bd[tc + 1] - pp.col_bd[tc]));
  }
  // the substreams in decoding order (6.5.1 tile scan): tile after tile; with WPP every CTB row of a tile is one
  job.geom.clear();
  for (int tr = 0; tr < pp.tile_rows; tr++)
    for (int tc = 0; tc < pp.tile_cols; tc++) {
      PicJob::SubGeom g; g.tile_cy0 = pp.row_bd[tr]; g.tile_cy1 = pp.row_bd[tr + 1]; g.cx0 = pp.col_bd[tc]; g.cx1 = pp.col_bd[tc + 1]; g.tc = tc;
      if (pp.wpp) for (int cy = g.tile_cy0; cy < g.tile_cy1; cy++) { g.cy0 = cy; g.cy1 = cy + 1; job.geom.push_back(g); }
      else { g.cy0 = g.tile_cy0; g.cy1 = g.tile_cy1; job.geom.push_back(g); }
    }
  job.seg_end_sub.assign(job.geom.size(), 0);
  if (job.own) { job.own->cols = pp.tile_cols; job.own->row_cols.reset(new std::atomic<uint8_t>[(size_t)hc]); for (int k = 0; k < hc; k++) job.own->row_cols[(size_t)k].store(0, std::memory_order_relaxed); }
  job.rc = 0; job.any_intra = job.any_inter = false;
  job.ambiguous_end = false; job.lf_restricted = false; job.lf_slices.clear();
  job.ctb_cut.clear(); job.ctb_slice.clear(); job.ctb_data.clear(); job.slice_qps.clear();
  asm_ = OpenPicture();
  asm_.active = true; asm_.pps_id = c.pps_id; asm_.nal_type = c.nal_type; asm_.irap = c.irap; asm_.cur_qp = sh.slice_qp; asm_.lf.push_back(LfSlice{c.opens ? c.seg_address : 0, c.across_slices});
  return job;
}

int Decoder::decode_slice(const uint8_t *rbsp, size_t len, int nal_type, int64_t pts)
{
  SliceCtx c(rbsp, len, nal_type, pts);
  int rc = 0;
  if (!slice_front(c, rc)) return rc;
  const DecPps &p = *c.p; const DecSps &s = *c.sps; SliceHdr &sh = c.sh;
  if (c.dependent) {
    // 7.3.6.1: everything but the address and the entry points is taken over from the slice's first segment
    asm_.cur_dependent = true;
    return append_segment(*c.open, c, c.open->pps, c.seg_address);
  }
  for (int k = 0; k < p.extra_header_bits; k++) c.r.get(1);
  const int slice_type = c.r.ue();
  if (slice_type < 0 || slice_type > 2) return DEC_ERR_INVALID;
  sh.is_intra = slice_type == 2; sh.is_b = slice_type == 0;
  if (c.first_seg || c.opens) sequence_state(c);                            // (an open picture has been closed by slice_front: seen_irap_ is current)
  if ((rc = parse_slice_header_rest(c.r, s, p, c.idr, prev_poc_, cur_no_rasl_, sh, c.rps, c.lt, c.across_slices))) return rc;
  DecPps pp = p;                                                 // the picture's copy: tile boundaries for this picture size
  if ((rc = tile_boundaries(pp, s.wc(), s.hc()))) return rc;
  if (!c.first_seg && !c.opens && partial_ && pp.tile_cols == 1 && pp.tile_rows == 1 && sh.poc != c.open->sh.poc) {
    // partial pictures v1, rule 2: another picture's segment (its order count differs) -- the open picture is closed with what it has, this segment opens its own
    if ((rc = close_open_picture()) < 0) return rc;
    c.opens = true; c.open = nullptr; free_stream_ = true;
  }
  if (!c.first_seg && !c.opens) {
    // an independent slice of a picture under way
    if (!same_slice_params(sh, c.open->sh, pp.tile_cols > 1 || pp.tile_rows > 1)) return DEC_ERR_UNSUPPORTED;
    asm_.cur_dependent = false; asm_.cur_qp = sh.slice_qp;      // (inside one tile a slice may have its own SliceQpY: free slices, close_free_picture)
    asm_.lf.push_back(LfSlice{c.seg_address, c.across_slices});
    return append_segment(*c.open, c, pp, c.seg_address);
  }
  if (!sh.is_intra && !seen_irap_) return DEC_ERR_INVALID;       // nothing to predict from before the first random access point
  if (band_nrows_ > 0 && s.ctb_log2 != 6) return DEC_ERR_UNSUPPORTED;      // (the tile-row split hands over bands of 64-sample rows)
  if (p.cu_qp_delta && p.qp_delta_depth > s.ctb_log2 - s.min_cb_log2) return DEC_ERR_INVALID;      // (7.4.3.3.1: a quantisation group is no smaller than the minimum coding block)
  if (!ensure_buffers(s.width, s.height, s.ctb_log2)) return DEC_ERR_GPU;
  if ((rc = apply_rps_and_build_lists(c))) return rc;
  const int slot = alloc_slot();                                 // (partial pictures: not S's buffer, avoid_slot_ -- the fill reads it behind the picture's kernels)
  avoid_slot_ = -1;
  if (slot < 0) return DEC_ERR_GPU;
  return append_segment(open_job(c, pp, slot), c, pp, c.opens ? c.seg_address : 0);
}

// The slice data of one segment joins the picture's job: entry points (the segment's substreams: whole CTU rows with WPP, else whole
// tiles -- or, for a dependent segment without either, one run of CTU rows inside the current substream), then the bytes.  The last
// segment submits the job.  `r` stands behind the part of the slice segment header that precedes the entry points.
int Decoder::append_segment(PicJob &job, const SliceCtx &c, const DecPps &pp, int address)
{
  const DecPps &p = *c.p; const uint8_t *rbsp = c.rbsp; const size_t len = c.len; const int wc = c.sps->wc(), hc = c.sps->hc();
  BitReader r(rbsp, len); r.pos = c.r.pos;
  auto fail = [&](int rc) { asm_.active = false; return rc; };
  if (pp.tile_cols > 1) return append_segment_tiles(job, c, address);
  // One tile: a segment that Kvazaar's forms do not have -- one that begins inside a CTB row, an independent slice behind the picture's first -- makes the picture
  // (and the stream: free_stream_) one of FREE slices: its segments are only collected here; where each ends is where the next begins, and the picture is put
  // together when its access unit ends (close_free_picture).
  const bool one_tile = pp.tile_rows == 1;
  // (frame threads: a picture whose segments turn out not to reach its end is with a worker by then; it is taken back when the segment that shows as much arrives
  // -- decode_slice -- unless the ring has handed it on already.  A picture without WPP, whose first segment says nothing at all about how far it reaches, does not
  // take that chance: it always waits for the end of its access unit there -- the next NAL unit, one more picture of delay on top of the ring's; a picture that
  // then has ONE segment is parsed as ever, close_free_picture)
  const bool wait_always = one_tile && frame_threads_ > 1 && !p.wpp && band_nrows_ == 0 && !parse_only_;
  if (one_tile && !asm_.free && (wait_always || free_stream_ || (!asm_.segs.empty() && !asm_.cur_dependent) || address % wc != 0 || (!p.wpp && address != asm_.rows * wc))) {      // (without WPP no header says how many rows a segment has: one that begins elsewhere than guessed is no loss)
    if (band_nrows_ > 0) return fail(DEC_ERR_UNSUPPORTED);
    asm_.free = true;
    if (!wait_always) free_stream_ = true;
  }
  if (partial_ && !asm_.free && one_tile && p.wpp && asm_.cur_dependent && address % wc == 0 && address != asm_.rows * wc && address < wc * hc)
    return 0;      // partial pictures v1, rule 1: a dependent segment behind a gap (its predecessor is gone) or before `next` (a duplicate) is dropped, the picture stays open
  if (!asm_.free && address != asm_.rows * wc) return fail(address % wc ? DEC_ERR_UNSUPPORTED : DEC_ERR_INVALID);     // whole CTU rows, in order
  if (asm_.free && partial_ && !asm_.segs.empty() && address <= asm_.segs.back().address && address < wc * hc) return 0;      // (partial pictures, rule 1: a duplicate, or out of order -- ignored)
  if (asm_.free && (address >= wc * hc || (asm_.segs.empty() ? (address != 0 && !partial_) : address <= asm_.segs.back().address))) return fail(DEC_ERR_INVALID);
  std::vector<uint32_t> entry; size_t hdr = 0;
  if (const int rc = parse_segment_tail(r, p.wpp || p.tile_rows > 1, p.header_extension != 0, entry, hdr)) return fail(rc);
  // CTU rows the segment covers
  const int nss = (int)entry.size() + 1, row0 = asm_.rows;
  int rows = 0;
  bool mid_substream = false;                                    // no WPP, and the segment does not start a tile: it continues the tile's substream
  if (asm_.free) { if (nss > hc || (!p.wpp && nss != 1)) return fail(DEC_ERR_INVALID); }
  else if (p.wpp) rows = nss;
  else {
    int t = 0; while (t < pp.tile_rows && pp.row_bd[t] != row0) t++;
    if (t < pp.tile_rows) { if (t + nss > pp.tile_rows) return fail(DEC_ERR_INVALID); rows = pp.row_bd[t + nss] - row0; }
    else {
      // inside a tile: only a dependent segment can start here; how many rows it holds is not in its header -- one (the form the
      // synthesiser writes); a longer one fails at its first end_of_slice_segment_flag
      if (nss != 1) return fail(DEC_ERR_UNSUPPORTED);
      rows = 1; mid_substream = true;
    }
    if (!mid_substream && nss == 1 && pp.tile_rows == 1 && row0 == 0) {
      // one tile, no WPP: the first segment's length is unknown as well: the whole picture unless dependent segments follow
      rows = p.dependent_slices ? 1 : hc;
      asm_.guessed_one_row = p.dependent_slices != 0;
    } else if (!mid_substream && nss == 1 && p.dependent_slices) rows = 1;      // a tile begun by one row; the rest follows as dependent segments
  }
  if (!asm_.free && (rows < 1 || row0 + rows > hc)) return fail(DEC_ERR_INVALID);
  const size_t base = job.rbsp.size();
  if (hdr > len) return fail(DEC_ERR_INVALID);
  const std::vector<size_t> starts = substream_starts(entry, epb_, hdr, base);      // where the segment's substreams begin in job.rbsp
  job.rbsp.insert(job.rbsp.end(), rbsp + hdr, rbsp + len);
  job.data_off = 0; job.data_len = job.rbsp.size();
  if (one_tile) {
    if (asm_.segs.size() >= 1024) return fail(DEC_ERR_UNSUPPORTED);
    asm_.segs.push_back(FreeSeg{address, asm_.cur_dependent, asm_.cur_qp, starts});
  }
  if (asm_.free) return 0;                                       // (the access unit's end closes the picture: decode_nal_inner, close_open_picture)
  if (mid_substream) job.row_restart[(size_t)row0] = base;
  else job.sub_start.insert(job.sub_start.end(), starts.begin(), starts.end());
  asm_.rows = row0 + rows;
  job.seg_end_row[(size_t)(asm_.rows - 1)] = 1;
  if (asm_.rows < hc) return 0;                                  // more segments to come: no output for this NAL unit
  asm_.active = false;
  job.ambiguous_end = one_tile && band_nrows_ == 0;
  return submit_job(job, asm_.nal_type, asm_.irap);
}

// Tile columns: a slice segment is the whole picture or one or more whole tiles, in tile-scan order (independent slices; a Kvazaar
// peer's slices=tiles).  Progress is counted in substreams.
int Decoder::append_segment_tiles(PicJob &job, const SliceCtx &c, int address)
{
  const DecPps &p = *c.p; const uint8_t *rbsp = c.rbsp; const size_t len = c.len; const int wc = c.sps->wc();
  BitReader r(rbsp, len); r.pos = c.r.pos;
  auto fail = [&](int rc) { asm_.active = false; return rc; };
  const int nsub = (int)job.geom.size();
  if (asm_.subs >= nsub) return fail(DEC_ERR_INVALID);
  const PicJob::SubGeom &g0 = job.geom[(size_t)asm_.subs];
  if (g0.cy0 != g0.tile_cy0 || address != g0.cy0 * wc + g0.cx0) return fail(DEC_ERR_UNSUPPORTED);        // segments start where a tile starts
  std::vector<uint32_t> entry; size_t hdr = 0;
  if (const int rc = parse_segment_tail(r, true, p.header_extension != 0, entry, hdr)) return fail(rc);
  const int nss = (int)entry.size() + 1, last = asm_.subs + nss - 1;
  if (last >= nsub) return fail(DEC_ERR_INVALID);
  if (job.geom[(size_t)last].cy1 != job.geom[(size_t)last].tile_cy1) return fail(DEC_ERR_UNSUPPORTED);   // ... and end where one ends
  const size_t base = job.rbsp.size();
  if (hdr > len) return fail(DEC_ERR_INVALID);
  const std::vector<size_t> starts = substream_starts(entry, epb_, hdr, base);
  job.sub_start.insert(job.sub_start.end(), starts.begin(), starts.end());
  job.rbsp.insert(job.rbsp.end(), rbsp + hdr, rbsp + len);
  job.data_off = 0; job.data_len = job.rbsp.size();
  asm_.subs += nss;
  job.seg_end_sub[(size_t)last] = 1;
  if (asm_.subs < nsub) return 0;
  asm_.active = false;
  return submit_job(job, asm_.nal_type, asm_.irap);
}

// partial pictures: four bytes per coding tree block of a parsed picture -- missing, its ctu_tile byte, its ctu_nb byte (0xff: no map), min(255, transform blocks)
std::vector<uint8_t> Decoder::layout_of(const PicJob &job) const
{
  const int n = ctbs_in(w_, ctbl_) * ctbs_in(h_, ctbl_);
  std::vector<uint8_t> o((size_t)n * 4);
  for (int a = 0; a < n; a++) {
    bool miss = false; for (const auto &m : job.missing) miss |= a >= m.first && a < m.first + m.second;
    const uint32_t k = job.ctu[a].count & 0xffffffu;
    o[4 * (size_t)a] = miss; o[4 * (size_t)a + 1] = job.ctu_tile[a]; o[4 * (size_t)a + 2] = job.lf_restricted ? job.h_in[job.lay.nb_off + (size_t)a] : 0xff; o[4 * (size_t)a + 3] = (uint8_t)(k > 255 ? 255 : k);
  }
  return o;
}
// ... a damaged picture that has parsed: its runs join the log, in decoding order, and its layout is kept for debug_copy "partial_layout"
void Decoder::file_damage(const PicJob &job)
{
  if (job.missing.empty()) return;
  for (const auto &m : job.missing) { damage_log_.push_back(job.sh.poc); damage_log_.push_back(m.first); damage_log_.push_back(m.second); }
  damaged_layout_ = layout_of(job);
}

void Decoder::take_back_job(PicJob &job)
{
  DpbPic &d = dpb_[job.slot];
  d.poc = job.undo.poc; d.is_ref = job.undo.is_ref; d.used = job.undo.used; d.decode_idx = job.undo.decode_idx; d.motion = job.undo.motion; d.cmotion = job.undo.cmotion; prev_poc_ = job.undo.prev_poc; seen_irap_ = job.undo.seen_irap;
  outp_.restore(std::move(job.undo.order)); d.standin = job.undo.standin; take_backs_++;
  job.undo.motion.reset(); job.undo.cmotion.reset();
  // the parse that ended early has released every row of the picture's ColMotion (parse_job release_all) and counted its columns: the picture is parsed AGAIN when its
  // access unit has ended, and under frame threads the next picture's parser must wait for THAT parse, row by row -- the rows are closed again here (nobody holds the
  // ColMotion but this job: the buffer's entry has just gone back to what it was, and no later picture has been opened)
  if (job.own) for (int r = 0; r < job.own->hc; r++) { job.own->row_done[(size_t)r].store(0, std::memory_order_relaxed); if (job.own->row_cols) job.own->row_cols[(size_t)r].store(0, std::memory_order_relaxed); }
  job_head_--; job.state.store(0, std::memory_order_relaxed); job.rc = 0; job.early_dst = nullptr;
  asm_.active = true; asm_.free = free_stream_ = true;
}

// closed boundaries inside the picture?  (7.4.3.3.1 loop_filter_across_tiles_enabled_flag = 0 with more than one tile; 7.4.7.1 a slice with
// slice_loop_filter_across_slices_enabled_flag = 0 in a picture of several slices.)  The picture's slices go with the job; parse_job lays the map out.
void Decoder::note_lf_restrictions(PicJob &job)
{
  bool closed = (job.pps.tile_rows > 1 || job.pps.tile_cols > 1) && !job.pps.across_tiles;
  if (asm_.lf.size() > 1) for (const LfSlice &s : asm_.lf) closed |= !s.across;
  closed |= !job.missing.empty();                                // (partial pictures: the boundary of what is missing is closed)
  job.lf_restricted = closed && band_nrows_ == 0;
  job.lf_slices.clear();
  if (job.lf_restricted) for (const LfSlice &s : asm_.lf) job.lf_slices.emplace_back(s.address, (uint8_t)s.across);
}

int Decoder::submit_job(PicJob &job, int nal_type, bool irap)
{
  note_lf_restrictions(job);
  if (job.lf_slices.empty() && band_nrows_ > 0 && (job.pps.tile_rows > 1 || job.pps.tile_cols > 1) && !job.pps.across_tiles) return DEC_ERR_UNSUPPORTED;      // (the tile-row split exchanges halos FOR the filters)
  const SliceHdr &sh = job.sh;
  DpbPic &d = dpb_[job.slot];
  // (PicJob::ambiguous_end: when the picture's last segment ends before the picture does, more segments are to come -- everything is put back as it was before
  // the call and the picture is open again, as one of free slices; append_segment collects the rest, the end of the access unit closes it.  The synchronous decoder
  // knows at once; with frame threads the worker finds out and decode_slice looks when the next segment arrives.)
  job.undo.poc = d.poc; job.undo.prev_poc = prev_poc_; job.undo.is_ref = d.is_ref; job.undo.used = d.used; job.undo.seen_irap = seen_irap_; job.undo.decode_idx = d.decode_idx; job.undo.motion = d.motion; job.undo.cmotion = d.cmotion; job.undo.standin = d.standin;
  auto take_back = [&] { take_back_job(job); return 0; };
  job.scan_gaps = partial_ && band_nrows_ == 0 && (!job.pps.wpp || !job.ctb_cut.empty()) && job.pps.tile_rows == 1 && job.pps.tile_cols == 1;      // (one tile, without WPP or as free slices: the parser finds the gaps, parse_substream)
  d.poc = sh.poc; d.is_ref = true; d.used = true; d.is_lt = false; d.standin = false; d.decode_idx = job_head_; d.motion = job.own; d.cmotion = job.cown;
  if (cur_tid_ == 0 && (nal_type > 9 || ((nal_type & 1) && nal_type < 6))) prev_poc_ = sh.poc;   // prevTid0Pic (8.3.1): TemporalId 0, not RASL / RADL / sub-layer non-reference
  if (irap) seen_irap_ = true;
  job.undo.order = outp_.mark(); job.serial = outp_.submitted(sh.poc, job.sps->num_reorder, job.starts_cvs, job.discard_prior, sh.no_output);      // output bookkeeping in decoding order (C.5.2.2, C.5.2.3; dec_order.h)
  job_head_++;
  if (parse_only_) {
    auto t0 = std::chrono::steady_clock::now();
    job.rc = parse_job(job, parse_threads_ > 1);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (job.rc == DEC_SEG_ENDS_EARLY) return take_back();
    job_tail_ = job_head_;
    if (job.rc < 0) return job.rc;
    probe_book(job, ms);
    file_damage(job);      // (once the picture has parsed: rule 1, what does not parse is corruption and no damaged picture)
    return 0;
  }
  if (frame_threads_ == 1) {
    auto t0 = std::chrono::steady_clock::now();
    job.early_dst = nullptr; job.early_rows.store(0, std::memory_order_relaxed);
    {
      // (decoder.h PicJob::early_dst; the buffer is the one launch_gpu will pick -- nothing is launched between here and there)
      static const bool early_off = [] { const char *e = getenv("KVAZZUP_AMD_DEC_EARLY_UP"); return e && atoi(e) == 0; }();
      const int ib = (int)(launched_ % (gpu_depth_ + 1));
      if (!early_off && gpu_depth_ == 1 && band_nrows_ == 0 && job.pps.tile_cols == 1 && !job.lf_restricted && !job.scan_gaps && !(batch_attached_ && DecBatcher::get(device_).active()) && d_in_[ib] && d_in_cap_[ib] >= job.lay.fixed_bytes()) job.early_dst = d_in_[ib];      // (lf_restricted: parse_job's last step still changes records)
    }
    job.rc = parse_job(job, true);
    if (job.rc == DEC_SEG_ENDS_EARLY) { if (job.early_dst) hipStreamSynchronize(stream_up_); return take_back(); }
    if (profiling_) { k_ms_[DK_HOST_PARSE] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); k_n_[DK_HOST_PARSE]++; }
    job.state.store(2, std::memory_order_release);
  } else {
    job.state.store(1, std::memory_order_release);
    if (!workers_) workers_.reset(new FrameWorkers(frame_threads_));
    PicJob *jp = &job;
    workers_->submit([this, jp] {
      auto t0 = std::chrono::steady_clock::now();
      // a large picture (an intra picture: several milliseconds on one core, which the pictures behind it in the ring cannot
      // hide) has its substreams parsed side by side on the row pool; small ones stay on this worker
      bool rows = false;
      // (64 KB: a 4K intra picture at QP 32 is ~125 KB and ~10 ms on one core -- longer than the eleven pictures behind it in a ring
      // of twelve take -- a 1080p one ~37 KB and stays on its worker: at 1080p every core is busy anyway)
      static const size_t row_parse_bytes = [] { const char *e = getenv("KVAZZUP_AMD_ROWPARSE_KB"); return (size_t)(e ? atoi(e) : 64) << 10; }();
      if (jp->data_len > row_parse_bytes && pool_mutex_.try_lock()) rows = true;
      jp->rc = parse_job(*jp, rows);
      if (rows) pool_mutex_.unlock();
      jp->parse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      jp->state.store(2, std::memory_order_release);
      futex_wake_all(jp->state);
    });
  }
  if (job_head_ - job_tail_ < frame_threads_ - (gpu_depth_ - 1)) return 0;          // pipeline still filling: no output for this NAL
  return finish_oldest();
}

// set_parse_only: what launch_gpu would upload for this picture, folded into the running digest
void Decoder::probe_book(PicJob &job, double ms)
{
  if (const char *dump = getenv("KVAZZUP_AMD_PROBE_DUMP")) {      // (debugging aid: every picture's 4x4 records and intra modes, rows of pw / 4, appended to the file)
    if (FILE *fp = fopen(dump, "ab")) {
      const int32_t hdr[4] = {pw_ / 4, ph_ / 4, w_ / 4, h_ / 4};
      fwrite(hdr, sizeof(hdr), 1, fp); fwrite(job.b4, sizeof(B4Rec), (size_t)(pw_ / 4) * (ph_ / 4), fp); fwrite(job.intra_mode.data(), 1, (size_t)(pw_ / 4) * (ph_ / 4), fp);
      fclose(fp);
    }
  }
  uint64_t d = probe_.digest;
  auto fold = [&](const uint8_t *p, size_t n) { for (size_t i = 0; i < n; i++) { d ^= p[i]; d *= 0x100000001b3ull; } };
  fold(job.h_in, job.lay.scaling_off);                                        // records, region / CTU tables, tile ids, SAO parameters
  fold(job.h_in + job.lay.tu_off, job.ntu * sizeof(DecTu));
  fold(job.h_in + job.lay.lev_off, job.nlev * sizeof(uint32_t));
  probe_.digest = d; probe_.pictures++; probe_.tus += job.ntu; probe_.levels += job.nlev; probe_.parse_ms += ms;
}

// Waits for the oldest submitted picture to be parsed, reconstructs it on the GPU and makes it the output.
// Output stage.  Synchronous mode (frame_threads_ == 1): the picture just parsed is reconstructed and output.
// Frame-threaded mode: first the picture launched by the previous call is completed and becomes the output,
// then the oldest parsed picture is launched -- its kernels run while this thread goes on parsing headers.
int Decoder::finish_oldest()
{
  if (parse_only_) return 0;
  int rc_launch = 0;
  bool launched = false;
  if (job_head_ != job_tail_) {
    PicJob &job = jobs_[(size_t)(job_tail_ % jobs_.size())];
    job_tail_++;
    { Tick tk; for (int st; (st = job.state.load(std::memory_order_acquire)) != 2;) futex_wait(job.state, st); t_wait_ += tk.ms(); }
    job.state.store(0, std::memory_order_relaxed);
    if (frame_threads_ > 1 && profiling_) { k_ms_[DK_HOST_PARSE] += job.parse_ms; k_n_[DK_HOST_PARSE]++; }
    if (job.parse_ms > t_parse_max_) t_parse_max_ = job.parse_ms;
    // the next picture's kernels are queued BEFORE an earlier picture is waited for: the GPU goes from one to the other without
    // this thread's launch latency in between
    tl("dlaunch0", job.pts);
    rc_launch = job.rc < 0 ? (job.rc == DEC_SEG_ENDS_EARLY ? DEC_ERR_UNSUPPORTED : job.rc) : launch_gpu(job);      // (a picture whose last segment ended early and whose rest never came)
    // a picture that could not be parsed (damaged on the way) is never reconstructed: its buffer is no reference picture -- the pictures that name it find it
    // missing and get a stand-in (conceal_ref) instead of whatever the buffer held.  (Frame threads: pictures submitted before this was known keep the buffer.)
    if (job.rc >= 0) file_damage(job);      // (partial pictures: in decoding order, once the picture has parsed)
    if (job.rc < 0 && dpb_[job.slot].is_ref && dpb_[job.slot].poc == job.sh.poc && dpb_[job.slot].decode_idx == job_tail_ - 1) dpb_[job.slot].is_ref = false;
    tl("dlaunch1", job.pts);
    launched = rc_launch >= 0;
  }
  int produced = 0;
  { const int rc = start_ready_downloads(); if (rc < 0) return rc; }
  tl("ddl", 0);
  // frame-threaded mode: gpu_depth_ pictures stay queued on the GPU; a call that launches nothing (end of sequence / drain) takes one out
  if (!gpu_q_.empty() && (!launched || (int)gpu_q_.size() > gpu_depth_)) {
    PicJob *j = gpu_q_.front(); gpu_q_.pop_front();
    const int rc = complete_gpu(*j);
    tl("dcomplete", j->pts);
    if (rc < 0) return rc;
    produced = rc;
  }
  if (rc_launch < 0) return rc_launch;
  if (frame_threads_ == 1 && !gpu_q_.empty()) { PicJob *j = gpu_q_.front(); gpu_q_.pop_front(); const int rc = complete_gpu(*j); if (rc < 0) return rc; produced |= rc; }
  return produced;
}

// what libOpenHevcGetOutput / kvzx_decoder_output_device say about the picture of `job`; buf: its host buffer (download mode) or -1.
// The host buffer holds the picture buffer as it is -- coded size, Y | Cb | Cr back to back, pitch = coded width -- so that it comes down in one
// copy; the cropped picture is addressed through the plane pointers and pitches, as with any decoder's frame (openhevcfilter.cpp:209,224-227
// reads chroma row i/2 at pvU + i * (nUPitch / 2): the pitches are even).
void Decoder::describe_output(const PicJob &job, DecodedPicture &o, int buf) const
{
  o = DecodedPicture();
  o.coded_w = w_; o.coded_h = h_;
  o.width = w_ - job.crop[0] - job.crop[1]; o.height = h_ - job.crop[2] - job.crop[3];
  o.poc = job.sh.poc; o.pts = job.pts; o.is_intra = job.sh.is_intra; o.cvs = job.cvs; o.num_reorder = job.sps->num_reorder; o.serial = job.serial;
  o.fps_num = job.fps_num; o.fps_den = job.fps_den;
  for (const auto &m : job.missing) o.missing_ctbs += m.second;
  o.total_ctbs = ctbs_in(w_, ctbl_) * ctbs_in(h_, ctbl_);
  for (int c = 0; c < 3; c++) {
    const int pw = c ? pw_ / 2 : pw_, ox = c ? job.crop[0] / 2 : job.crop[0], oy = c ? job.crop[2] / 2 : job.crop[2];
    const size_t off = (size_t)oy * pw + ox;
    o.dev[c] = dpb_[job.slot].plane[c] + off; o.dev_pitch[c] = pw;
    if (buf >= 0) { o.host[c] = h_out_[buf] + (dpb_[job.slot].plane[c] - dpb_[job.slot].plane[0]) + off; o.host_pitch[c] = pw; }
  }
}

// The picture buffer of `job` -> host buffer job.dl_buf: one copy-engine transfer on the download stream.  Only called when the picture's
// kernels are KNOWN to have finished (the caller has seen job.done): the copy command then carries no dependency, the copy engine takes
// it at once and nothing waits inside a hardware queue.  (Copies that waited on an event in the stream were executed by the runtime as
// blit kernels, four per picture with a barrier each; a kernel that stores across PCIe -- tried too -- slows every kernel running beside it
// by a factor of two to ten, tools/measure/pcie_copy_vs_kernels.hip.  The copy engine disturbs nothing.)
int Decoder::queue_download(PicJob &job)
{
  job.dl_buf = (int)(job.launch_idx % kOutRing);
  if (!h_out_[job.dl_buf] && hipHostMalloc(&h_out_[job.dl_buf], h_out_cap_, hipHostMallocDefault) != hipSuccess) { h_out_[job.dl_buf] = nullptr; return DEC_ERR_GPU; }
  if (!job.dl_done && hipEventCreateWithFlags(&job.dl_done, hipEventDisableTiming) != hipSuccess) return DEC_ERR_GPU;
  // rows above the crop window are not needed, rows below the picture's last row neither: the copy covers the planes from the first to the last row used
  const size_t npx = (size_t)pw_ * ph_;
  const size_t used = npx + npx / 4 + (size_t)(pw_ / 2) * ((h_ + 1) / 2);             // up to the end of the last Cr row
  if (hipMemcpyAsync(h_out_[job.dl_buf], dpb_[job.slot].plane[0], used, hipMemcpyDeviceToHost, stream_dl_) != hipSuccess) return DEC_ERR_GPU;
  dpb_[job.slot].last_dl = job.dl_done;
  return hipEventRecord(job.dl_done, stream_dl_) == hipSuccess ? 0 : DEC_ERR_GPU;
}

// frame-threaded download mode: start the copy of every queued picture whose kernels have finished (oldest first).  (Queueing the copy at launch instead, behind
// the picture's event on the download stream, was measured in round 6 and HALVES the host-boundary rate -- 3 200 against 6 290 frames/s at 1080p, 1 060 against
// 1 995 at 4K: hipMemcpyAsync to the host behind an unresolved hipStreamWaitEvent holds the calling thread, 135 ms of launches instead of 22 per 384 pictures;
// profiles/r06_dl_at_launch_ab.txt.)
int Decoder::start_ready_downloads()
{
  if (!download_) return 0;
  for (PicJob *j : gpu_q_) {
    if (j->dl_buf >= 0) continue;
    if (!j->launched.load(std::memory_order_acquire)) break;      // (still in the submission layer's queue: its event has not been recorded)
    const hipError_t r = hipEventQuery(j->done);
    if (r == hipErrorNotReady) break;
    if (r != hipSuccess) return DEC_ERR_GPU;
    const int rc = queue_download(*j);
    if (rc < 0) return rc;
  }
  return 0;
}

int Decoder::complete_gpu(PicJob &job)
{
  {
    Tick tk;
    while (!job.launched.load(std::memory_order_acquire)) futex_wait(job.launched, 0);      // (batch.h: the submitter thread records job.done)
    auto wait = [&](hipEvent_t ev) {
      if (frame_threads_ > 1 && !spin_wait_)    // the output lags anyway: nap between queries instead of polling (see nap_until)
        return nap_until([&] { hipError_t r = hipEventQuery(ev); return r == hipSuccess ? 1 : (r == hipErrorNotReady ? 0 : -1); });
      return hipEventSynchronize(ev) == hipSuccess;
    };
    if (download_ && job.dl_buf < 0) {          // its copy has not been started yet (synchronous decoder; the GPU queue was short): kernels first
      if (!wait(job.done)) return DEC_ERR_GPU;
      const int rc = queue_download(job); if (rc < 0) return rc;
    }
    if (!wait(download_ ? job.dl_done : job.done)) return DEC_ERR_GPU;
    t_sync_ += tk.ms();
  }
  if (*h_err_) { fprintf(stderr, "kvazzup_amd: decoder device error flags 0x%x\n", *h_err_); return DEC_ERR_GPU; }
  if (!job.expect_hash.empty() && job.missing.empty()) {                  // libOpenHevcSetCheckMD5: the picture's hash SEI arrived while it was in the ring
    const std::vector<uint8_t> want = std::move(job.expect_hash); job.expect_hash.clear();
    const int rc = verify_hash(job, want);
    if (rc < 0) last_error_ = rc;                   // (the picture is still handed out: the application decides, as with OpenHEVC)
  }
  if (job.ev_used) {
    for (size_t i = 0; i < job.ev_used; i++) { float ms = 0; hipEventElapsedTime(&ms, job.ev[i].a, job.ev[i].b); k_ms_[job.ev[i].id] += ms; k_n_[job.ev[i].id]++; }
    job.ev_used = 0;
  }
  if (job.sh.no_output) { job.dl_buf = -1; return 0; }      // pic_output_flag = 0 (7.4.7.1): reconstructed -- later pictures predict from it -- and never handed out
  if (outp_.discarded(job.serial)) { job.dl_buf = -1; return 0; }      // (an IDR / BLA picture behind it said so: C.5.2.2)
  describe_output(job, out_, download_ ? job.dl_buf : -1);
  out_slot_ = job.slot;
  job.dl_buf = -1;
  pic_ready_ = true;
  return 1;
}

// ------------------------------------------------------------------------------------------ GPU reconstruction
// launch_gpu's stages, in the order they run.  fill_concealed: buffers that stand in for lost reference pictures (conceal_ref) -- grey, or a copy of the nearest
// picture -- BEFORE this picture's kernels and AFTER everything older has left the GPU: older pictures in flight may still read what the buffers held.  A loss is
// rare: the device is simply drained (pictures handed to the submission layer are launched first).
// Concealment v3, steps 1 and 2 (decoder.h): the source's motion per 16x16 block, continued from its order count s to the missing picture's p, kept where the
// neighbours agree -> per block the whole-sample displacements of luma (x, y) and chroma (x, y).  m = NULL: the source is a stand-in -- no motion, all zero.
std::vector<int16_t> Decoder::conceal_displacements(const ConcealMotion *m, int w16, int h16, int p, int s)
{
  std::vector<int16_t> tab((size_t)w16 * h16 * 4, 0);
  if (!m || m->w16 != w16 || m->h16 != h16) return tab;
  auto clip3 = [](long long lo, long long hi, long long v) { return (int)(v < lo ? lo : (v > hi ? hi : v)); };      // (64 bits: the difference of two order counts of a hostile stream)
  std::vector<int> v((size_t)w16 * h16 * 2, 0);
  const int tb = clip3(-128, 127, (long long)p - s);
  for (size_t b = 0; b < (size_t)w16 * h16; b++) {
    const ConcealMotion::E &e = m->e[b];
    const int td = clip3(-128, 127, (long long)s - e.ref_poc);
    if (e.none || e.lt || td == 0) continue;
    const int tx = (16384 + (abs(td) >> 1)) / td, f = clip3(-4096, 4095, (tb * tx + 32) >> 6);
    for (int k = 0; k < 2; k++) { const int q = f * e.mv[k], a = (abs(q) + 127) >> 8; v[2 * b + k] = clip3(-32768, 32767, q < 0 ? -a : a); }
  }
  for (int y = 0; y < h16; y++)
    for (int x = 0; x < w16; x++) {
      const size_t b = (size_t)y * w16 + x;
      const int vx = v[2 * b], vy = v[2 * b + 1];
      int agree = 0;
      auto near = [&](int nx, int ny) { if (nx < 0 || ny < 0 || nx >= w16 || ny >= h16) return; const size_t n = (size_t)ny * w16 + nx; agree += abs(v[2 * n] - vx) <= 4 && abs(v[2 * n + 1] - vy) <= 4; };
      near(x - 1, y); near(x + 1, y); near(x, y - 1); near(x, y + 1);
      if (agree < 2) continue;
      tab[4 * b] = (int16_t)((vx + 2) >> 2); tab[4 * b + 1] = (int16_t)((vy + 2) >> 2); tab[4 * b + 2] = (int16_t)((vx + 4) >> 3); tab[4 * b + 3] = (int16_t)((vy + 4) >> 3);
    }
  return tab;
}

int Decoder::fill_concealed(PicJob &job)
{
  const size_t npx = (size_t)pw_ * ph_;
  for (PicJob *j : gpu_q_) while (!j->launched.load(std::memory_order_acquire)) futex_wait(j->launched, 0);
  if (hipDeviceSynchronize() != hipSuccess) return DEC_ERR_GPU;
  // (unconditionally: headers run ahead of launches -- by now a LATER picture may have been given the buffer, which is fine, it launches after this one and
  // overwrites it; a list inherited from a header that failed names buffers that are still stand-ins or have become this picture's own)
  // (set_profiling: the fill itself -- v2's copy or v3's kernel -- between two events, debug_copy "standin_ms"; a loss is rare, the events are made here)
  hipEvent_t ev[2] = {nullptr, nullptr};
  auto stamp = [&](int k, hipStream_t st) { if (profiling_ && (ev[k] || hipEventCreate(&ev[k]) == hipSuccess)) hipEventRecord(ev[k], st); };
  auto elapsed = [&] { float ms = 0; if (profiling_ && ev[0] && ev[1] && hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) standin_ms_ = ms; };
  for (const auto &c : job.conceal) {
    uint8_t *dst = dpb_[c.first].plane[0], *src = c.second >= 0 ? dpb_[c.second].plane[0] : nullptr;
    if (conceal_mode_ == 3 && dst) {
      // v3 (decoder.h): steps 1 and 2 here -- the source's parse has finished, its picture was launched before this one --, the table goes up, step 3 is the kernel
      const int w16 = (w_ + 15) / 16, h16 = (h_ + 15) / 16;
      const bool moved = src && src != dst;
      standin_slot_ = c.first;
      standin_tab_ = moved ? conceal_displacements(c.motion.get(), w16, h16, c.poc, c.src_poc) : std::vector<int16_t>((size_t)w16 * h16 * 4, 0);
      if (moved) {
        const size_t bytes = standin_tab_.size() * sizeof(int16_t);
        if (bytes > standin_tab_cap_) { hipFree(d_standin_tab_); standin_tab_cap_ = 0; if (hipMalloc(&d_standin_tab_, bytes) != hipSuccess) { d_standin_tab_ = nullptr; return DEC_ERR_GPU; } standin_tab_cap_ = bytes; }
        if (hipMemcpy(d_standin_tab_, standin_tab_.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return DEC_ERR_GPU;
        stamp(0, stream_);
        launch_dec_standin(dpb_[c.first].plane, dpb_[c.second].plane, d_standin_tab_, w_, h_, pw_, stream_);
        stamp(1, stream_);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) return DEC_ERR_GPU;      // (the next entry overwrites the table)
        elapsed();
        continue;
      }
    }
    stamp(0, nullptr);
    if (dst && (src && src != dst ? hipMemcpy(dst, src, npx * 3 / 2, hipMemcpyDeviceToDevice) : hipMemset(dst, 128, npx * 3 / 2)) != hipSuccess) return DEC_ERR_GPU;
    stamp(1, nullptr); elapsed();
  }
  if (hipDeviceSynchronize() != hipSuccess) return DEC_ERR_GPU;
  for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
  job.conceal.clear(); return 0;
}
// Partial pictures v1, rule 4 (decoder.h): S for the picture whose first segment is being read -- conceal_ref's selection (apply_rps_and_build_lists) for the picture's own
// order count; last_decoded: an IRAP picture that starts a coded video sequence -- order counts of the sequence before do not compare, the held picture decoded last
void Decoder::choose_fill_source(int poc, bool last_decoded, const std::vector<int> &fresh)
{
  int best = -1;
  for (int q = 0; q < kMaxPics; q++) {
    if (!dpb_[q].is_ref || !dpb_[q].used || std::find(fresh.begin(), fresh.end(), q) != fresh.end()) continue;
    if (last_decoded) { if (!dpb_[q].standin && (best < 0 || dpb_[q].decode_idx > dpb_[best].decode_idx)) best = q; continue; }
    const long long dq = llabs((long long)dpb_[q].poc - poc), db = best < 0 ? 0 : llabs((long long)dpb_[best].poc - poc);
    if (best < 0 || dq < db || (dq == db && dpb_[q].poc < dpb_[best].poc)) best = q;
  }
  cur_fill_src_ = avoid_slot_ = best;      // (from here to the picture's own alloc_slot nothing takes S's buffer: not a stand-in made for this picture either -- conceal_ref)
}
// ... and its samples: the missing coding tree blocks of `job` from S into the picture's buffer (DecFrame::out), BEHIND the picture's last kernel -- k_dec_inter writes whole
// 32x32 regions, the SAO pass whole tiles, so nothing put there earlier would last -- and before any later picture is launched: the picture has been launched just now, by this
// decoder or by the submission layer (batch.h; its `launched` flag is waited for), the device is drained -- the picture and S are complete --, the kernel runs, and only then
// does launch_gpu return.  What the drain costs is what a lost picture's costs (fill_concealed): the GPU queue runs empty once -- the calling thread waits for the pictures in
// flight and for this one instead of going on parsing headers; a damaged picture is rare.
int Decoder::fill_missing(PicJob &job)
{
  while (!job.launched.load(std::memory_order_acquire)) futex_wait(job.launched, 0);
  if (hipDeviceSynchronize() != hipSuccess) return DEC_ERR_GPU;
  const int wc = ctbs_in(w_, ctbl_), total = wc * ctbs_in(h_, ctbl_);
  std::vector<uint32_t> list;
  for (const auto &m : job.missing) for (int k = 0; k < m.second; k++) if (m.first + k >= 0 && m.first + k < total) list.push_back((uint32_t)(m.first + k));
  if (list.empty()) return 0;
  if (list.size() * sizeof(uint32_t) > fill_ctbs_cap_) { hipFree(d_fill_ctbs_); fill_ctbs_cap_ = 0; if (hipMalloc(&d_fill_ctbs_, (size_t)total * sizeof(uint32_t)) != hipSuccess) { d_fill_ctbs_ = nullptr; return DEC_ERR_GPU; } fill_ctbs_cap_ = (size_t)total * sizeof(uint32_t); }
  if (hipMemcpy(d_fill_ctbs_, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return DEC_ERR_GPU;
  uint8_t *const *dst = dpb_[job.slot].plane;
  uint8_t *const *src = job.fill_src >= 0 && job.fill_src != job.slot && dpb_[job.fill_src].plane[0] ? dpb_[job.fill_src].plane : nullptr;
  const int16_t *d_tab = nullptr;
  const int w16 = (w_ + 15) / 16, h16 = (h_ + 15) / 16;
  fill_tab_.assign((size_t)w16 * h16 * 4, 0);
  if (conceal_mode_ == 3 && src) {
    fill_tab_ = conceal_displacements(job.fill_motion.get(), w16, h16, job.sh.poc, job.fill_src_poc);
    const size_t bytes = fill_tab_.size() * sizeof(int16_t);
    if (bytes > fill_tab_cap_) { hipFree(d_fill_tab_); fill_tab_cap_ = 0; if (hipMalloc(&d_fill_tab_, bytes) != hipSuccess) { d_fill_tab_ = nullptr; return DEC_ERR_GPU; } fill_tab_cap_ = bytes; }
    if (hipMemcpy(d_fill_tab_, fill_tab_.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return DEC_ERR_GPU;
    d_tab = d_fill_tab_;
  }
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (profiling_) for (auto &e : ev) if (hipEventCreate(&e) != hipSuccess) e = nullptr;
  if (ev[0]) hipEventRecord(ev[0], stream_);
  launch_dec_fill_ctbs(dst, src, d_tab, d_fill_ctbs_, (int)list.size(), ctbl_, w_, h_, pw_, stream_);
  if (ev[1]) hipEventRecord(ev[1], stream_);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) return DEC_ERR_GPU;
  if (ev[0] && ev[1]) { float ms = 0; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) standin_ms_ = ms; }      // (debug_copy "standin_ms": the last fill of either kind)
  for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
  return 0;
}
// The input block goes up on its own stream into one of gpu_depth_ + 1 device buffers: the gpu_depth_ pictures launched before this one may still be running
// (finish_oldest launches before it completes the oldest of them) and read the other buffers; the one before those has been completed, so this buffer is free.
// -> buffer `ib`, grown to hold this picture's block; NULL: no memory
uint8_t *Decoder::input_buffer(PicJob &job, int ib)
{
  const size_t bytes = job.lay.upload_bytes();
  if (bytes > d_in_cap_[ib]) {
    if (job.early_dst) { hipStreamSynchronize(stream_up_); job.early_dst = nullptr; }      // (the rows that went up early went into the buffer being replaced)
    hipFree(d_in_[ib]); d_in_cap_[ib] = bytes + bytes / 2;
    if (hipMalloc(&d_in_[ib], d_in_cap_[ib]) != hipSuccess) { d_in_[ib] = nullptr; d_in_cap_[ib] = 0; }
  }
  return d_in_[ib];
}
// The picture's kernel argument: the one place its fields are set.  Const apart from the scaling factors and weights, which it copies into the job's input block
// (they go up with it).  d_in: the device copy of that block, laid out by `lay`; cs: the chain the picture runs on.
DecFrame Decoder::picture_frame(PicJob &job, const DecInputLayout &lay, const ChainSet &cs, uint8_t *d_in) const
{
  DecFrame f; memset(&f, 0, sizeof(f));
  f.w = w_; f.h = h_; f.pw = pw_; f.ph = ph_; f.wc = (w_ + 63) / 64; f.hc = (h_ + 63) / 64;      // (wc, hc: the picture in 64x64 tiles -- what the region, deblocking and SAO grids are made of)
  f.ctb_log2 = ctbl_; f.cwc = (w_ + (1 << ctbl_) - 1) >> ctbl_; f.chc = (h_ + (1 << ctbl_) - 1) >> ctbl_;      // ... and in coding tree blocks: the intra chain's work units, the tile ids, the SAO parameters
  f.tu_index = lay.indexed ? (const uint32_t *)(d_in + lay.i_off) : nullptr;
  f.b4 = (const B4Rec *)d_in; f.b4x = lay.bi ? (const B4L1 *)(d_in + lay.x_off) : nullptr; f.region = (const TuRange *)(d_in + lay.region_off); f.ctu = (const TuRange *)(d_in + lay.ctu_off);
  f.ctu_tile = d_in + lay.tile_off; f.tus = (const DecTu *)(d_in + lay.tu_off); f.lev = (const uint32_t *)(d_in + lay.lev_off); f.ntu = (int)lay.ntu;
  const bool sao = job.sh.sao_luma || job.sh.sao_chroma;      // the picture is then built in the chain's work planes and filtered into its buffer
  for (int c = 0; c < 3; c++) { f.resid[c] = cs.resid[c]; f.rec[c] = sao ? cs.work[c] : dpb_[job.slot].plane[c]; f.out[c] = dpb_[job.slot].plane[c]; }
  for (int k = 0; k < KVZ_DEC_MAX_REFS; k++) for (int c = 0; c < 3; c++) f.ref[k][c] = dpb_[job.ref_buf[k]].plane[c];      // (entry k: buffer k, or a reference picture from past the table's end -- open_job)
  f.sao = sao ? (const SaoParams *)(d_in + lay.sao_off) : nullptr; f.ctu_nb = job.lf_restricted ? d_in + lay.nb_off : nullptr;
  { f.progress = cs.progress; f.intra_order = intra_order_; f.err = err_; const size_t nctu = (size_t)f.cwc * f.chc, S = (size_t)1 << ctbl_;
    f.edge_col[0] = cs.edge_col; f.edge_col[1] = cs.edge_col + nctu * S; f.edge_col[2] = cs.edge_col + nctu * (S + S / 2);      // per CTB: S words (luma), S / 2 (Cb), S / 2 (Cr)
    f.edge_row[0] = cs.edge_row; f.edge_row[1] = cs.edge_row + nctu * (S / 4); f.edge_row[2] = cs.edge_row + nctu * (S / 4 + S / 8); }
  if (job.any_intra) f.chain_gen = chain_gen_;
  f.cb_qp_offset = (int8_t)job.pps.cb_qp_offset; f.cr_qp_offset = (int8_t)job.pps.cr_qp_offset; f.beta_offset = (int8_t)(2 * job.sh.beta_offset_div2); f.tc_offset = (int8_t)(2 * job.sh.tc_offset_div2);
  f.intra_direct = job.any_inter ? 1 : 0;                 // (a picture with inter blocks: few (CTU, plane) pairs hold intra blocks)
  f.strong_intra = (uint8_t)job.sps->strong_intra; f.tiles = job.pps.tile_rows > 1 || job.pps.tile_cols > 1 || job.slice_qps.size() > 1 || !job.missing.empty();      // (missing blocks: a slice byte of their own -- no received block takes them for neighbours or waits for them)
  f.general = (uint8_t)(job.pps.tile_rows > 1 || job.pps.tile_cols > 1 || job.slice_qps.size() > 1 || !job.missing.empty() || job.sps->pcm_depth[0] != 0);
  f.cip = (uint8_t)(job.pps.cip && job.any_inter);      // (a picture without inter blocks: every neighbour is intra)
  f.tq_bypass = (uint8_t)(job.pps.tq_bypass || (job.sps->pcm_depth[0] && job.sps->pcm_no_filter));      // (units the loop filters keep out of: B4_BYPASS records)
  // scaling lists: the picture's factors (the PPS's lists when it carries any, else the SPS's) ride in the input block
  const std::vector<uint8_t> *sc = !job.sps->scaling ? nullptr : (job.pps.scaling ? job.pps.scaling.get() : job.sps->scaling.get());      // (scaling_list_enabled_flag = 0: a PPS's lists are not used)
  if (sc) { memcpy(job.h_in + lay.scaling_off, sc->data(), KVZ_SCALING_BYTES); f.scaling = d_in + lay.scaling_off; }
  if (job.sh.weighted && lay.bi) { memcpy(job.h_in + lay.wt_off, job.sh.wt, sizeof(job.sh.wt)); f.wt = (const DecWt *)(d_in + lay.wt_off); f.wt_log2[0] = job.sh.wt_log2[0]; f.wt_log2[1] = job.sh.wt_log2[1]; }
  if (band_nrows_ > 0) { f.row0 = band_row0_; f.nrows = band_nrows_; }
  return f;
}
// the block goes up, minus the records when every CTU row of them is there already (PicJob::early_dst: queued on this stream by the row parsers -- when all rows made it)
bool Decoder::upload(PicJob &job, const DecInputLayout &lay, uint8_t *d_in, int ib, bool batched)
{
  const size_t up_from = (!batched && job.early_dst && job.early_dst == d_in && job.early_rows.load(std::memory_order_acquire) == ctbs_in(h_, ctbl_)) ? lay.region_off : 0;
  job.early_dst = nullptr;
  if (hipMemcpyAsync(d_in + up_from, job.h_in + up_from, lay.upload_bytes() - up_from, hipMemcpyHostToDevice, stream_up_) != hipSuccess) return false;
  return hipEventRecord(up_done_[ib], stream_up_) == hipSuccess;
}
// Several decoders open on this device: the picture goes to the device's submission layer (batch.h), which launches the waiting pictures of all of them together;
// its descriptor travels inside the input block.
int Decoder::post_to_batcher(PicJob &job, const DecFrame &f, uint8_t *d_in, int ib)
{
  DecBatchItem it; it.f = f; it.d_f = (const DecFrame *)(d_in + job.lay.frame_off);
  it.inter = job.any_inter; it.intra = job.any_intra; it.deblock = !job.sh.deblock_disabled; it.sao = job.sh.sao_luma || job.sh.sao_chroma;
  it.wait0 = up_done_[ib]; it.wait1 = dpb_[job.slot].last_dl; dpb_[job.slot].last_dl = nullptr;
  it.done = job.done; it.launched = &job.launched; it.owner = this; it.profile = prof_now_;
  job.launched.store(0, std::memory_order_relaxed);
  DecBatcher::get(device_).submit(it); batch_used_ = true;
  return 0;
}
template <class F> bool Decoder::each_buffer_used(const PicJob &job, F &&visit)
{
  bool ok = visit(dpb_[job.slot]);
  for (int k = 0; ok && k < job.nref; k++) ok = visit(dpb_[job.ref_buf[job.ref_slot[k]]]);
  for (int k = 0; ok && k < job.nref1; k++) ok = visit(dpb_[job.ref_buf[job.ref_slot1[k]]]);
  return ok;
}
// One decoder: it launches for itself, frame by value, on the chain's stream.
int Decoder::launch_self(PicJob &job, const DecFrame &f, uint8_t *d_in, int ib, bool alt)
{
  const hipStream_t st = chain_[alt].stream;
  if (hipStreamWaitEvent(st, up_done_[ib], 0) != hipSuccess) return DEC_ERR_GPU;
  // the buffer the picture is built in: the copy to the host of the picture last reconstructed there (queued, maybe not yet run) comes first
  if (dpb_[job.slot].last_dl) { if (hipStreamWaitEvent(st, dpb_[job.slot].last_dl, 0) != hipSuccess) return DEC_ERR_GPU; dpb_[job.slot].last_dl = nullptr; }
  // two chains: whatever this picture writes (its buffer) or reads (its reference pictures) was last touched by a picture on the OTHER stream -> after that one
  if (chain_[1].stream && !each_buffer_used(job, [&](DpbPic &d) { return !(d.last_use && d.last_use_alt != alt) || hipStreamWaitEvent(st, d.last_use, 0) == hipSuccess; })) return DEC_ERR_GPU;
  if (job.any_inter) timed(DK_INTER, [&] { launch_dec_inter(f, st); }, st);
  if (job.any_intra) timed(job.any_inter ? DK_INTRA_P : DK_INTRA, [&] { launch_dec_intra_resid(f, st); launch_dec_intra(f, st); }, st);
  if (band_nrows_ > 0) { band_f_ = f; band_din_ = d_in; }       // deblocking follows the halo exchange (band_deblock)
  else if (!job.sh.deblock_disabled) timed(DK_DEBLOCK, [&] { launch_dec_deblock(f, st); }, st);
  if (f.sao) timed(DK_SAO, [&] { launch_dec_sao(f, st); }, st);
  if (hipEventRecord(job.done, st) != hipSuccess) return DEC_ERR_GPU;
  // (the picture's event now stands for the last use of its buffer and of every buffer it read; a job's event is recorded again only when its ring entry is
  // reused -- by a later picture, whose kernels are queued behind this one's on one of the two streams or wait for it through these same marks)
  each_buffer_used(job, [&](DpbPic &d) { d.last_use = job.done; d.last_use_alt = alt; return true; });
  return 0;
}
int Decoder::launch_gpu(PicJob &job)
{
  if (hipSetDevice(device_) != hipSuccess) return DEC_ERR_GPU;
  if (!job.conceal.empty()) { const int rc = fill_concealed(job); if (rc < 0) return rc; }
  prof_now_ = profiling_ && (launched_ % prof_every_) == 0; timed_job_ = &job; job.ev_used = 0;
  if (!job.done && hipEventCreateWithFlags(&job.done, hipEventDisableTiming) != hipSuccess) return DEC_ERR_GPU;
  Tick tk_api; const int ib = (int)(launched_ % (gpu_depth_ + 1));
  uint8_t *const d_in = input_buffer(job, ib); if (!d_in) return DEC_ERR_GPU;
  // which chain: a picture without inter blocks, every other one of them, with the frame-threaded decoder on its own (decoder.h chain_)
  DecBatcher &batcher = DecBatcher::get(device_);
  const bool batched = band_nrows_ == 0 && batch_attached_ && batcher.active() && !(job.pps.cip && job.any_inter && job.any_intra);      // (constrained intra prediction: the chain's own form, k_dec_intra_cip -- launched by this decoder itself)
  static const bool alt_off = getenv("KVAZZUP_AMD_DEC_ONE_CHAIN") != nullptr;
  bool alt = !alt_off && !batched && band_nrows_ == 0 && frame_threads_ > 1 && gpu_depth_ > 1 && job.any_intra && !job.any_inter && ((intra_seq_++) & 1);
  if (alt && !ensure_alt()) alt = false;
  if (job.any_intra && ++chain_gen_ >= (1u << 24)) {      // a generation of its own for every launch of a chain: 1 .. 2^24 - 1; at the wrap the hand-off words go back to "never written"
    sync_main();                                         // (everything this decoder has submitted has run: nothing reads the words while they are cleared)
    // (on the consuming stream: the decoder's streams are non-blocking, nothing would order the next chain behind a clear on the null stream)
    for (const ChainSet &c : chain_) if (c.stream && (hipMemsetAsync(c.edge_col, 0, edge_col_words() * sizeof(uint32_t), c.stream) != hipSuccess || hipMemsetAsync(c.edge_row, 0, edge_row_words() * 8, c.stream) != hipSuccess)) return DEC_ERR_GPU;
    chain_gen_ = 1;
  }
  if (band_nrows_ > 0) {      // a band starts and ends on tile boundaries of full-width tiles; no SAO, no temporal prediction (what the split encoder writes)
    bool ok = !(job.sh.sao_luma || job.sh.sao_chroma) && !job.sps->tmvp && job.pps.tile_cols == 1 && frame_threads_ == 1, top = false, bottom = false;
    for (int t = 0; t <= job.pps.tile_rows; t++) { top |= job.pps.row_bd[t] == band_row0_; bottom |= job.pps.row_bd[t] == band_row0_ + band_nrows_; }
    if (!ok || !top || !bottom) return DEC_ERR_UNSUPPORTED;
  }
  const DecFrame f = picture_frame(job, job.lay, chain_[alt], d_in);
  if (!batched && batch_used_) { batcher.drain(this); batch_used_ = false; }      // (the other decoder has just closed: what this one still has queued there comes first)
  if (batched && chain_[1].stream) hipStreamSynchronize(chain_[1].stream);      // (another decoder has opened: from here on the submission layer launches on the shared stream; the second chain's last pictures first)
  if (batched) memcpy(job.h_in + job.lay.frame_off, &f, sizeof(f));
  if (!upload(job, job.lay, d_in, ib, batched)) return DEC_ERR_GPU;
  job.dl_buf = -1; job.launch_idx = launched_;
  if (const int rc = batched ? post_to_batcher(job, f, d_in, ib) : launch_self(job, f, d_in, ib, alt); rc < 0) return rc;
  if (!job.missing.empty()) { const int rc = fill_missing(job); if (rc < 0) return rc; }      // (partial pictures: behind the picture's last kernel, before anything later is launched)
  t_api_ += tk_api.ms(); launched_++;
  if (band_nrows_ > 0) gpu_job_ = &job; else gpu_q_.push_back(&job);
  return 0;
}

// ---- band mode (tile-row split): halo blocks are [luma 4 rows | Cb 2 rows | Cr 2 rows | the 4x4 records of one unit row], pw_ * 8 bytes
bool Decoder::band_export(int stage, uint8_t *d_buf)
{
  if (band_nrows_ <= 0 || !gpu_job_ || !d_buf) return false;
  PicJob &job = *gpu_job_;
  const int y = stage == 0 ? (band_row0_ + band_nrows_) * 64 - 4 : band_row0_ * 64 - 4;     // first of the four luma rows
  if (y < 0 || y + 4 > ph_) return false;
  size_t o = 0;
  if (hipMemcpyAsync(d_buf + o, dpb_[job.slot].plane[0] + (size_t)y * pw_, (size_t)pw_ * 4, hipMemcpyDeviceToDevice, stream_) != hipSuccess) return false;
  o += (size_t)pw_ * 4;
  for (int c = 1; c < 3; c++) { if (hipMemcpyAsync(d_buf + o, dpb_[job.slot].plane[c] + (size_t)(y / 2) * (pw_ / 2), (size_t)pw_, hipMemcpyDeviceToDevice, stream_) != hipSuccess) return false; o += (size_t)pw_; }
  if (stage == 0 && hipMemcpyAsync(d_buf + o, band_din_ + (size_t)(y / 4) * (pw_ / 4) * sizeof(B4Rec), (size_t)(pw_ / 4) * sizeof(B4Rec), hipMemcpyDeviceToDevice, stream_) != hipSuccess) return false;
  return hipStreamSynchronize(stream_) == hipSuccess;
}
bool Decoder::band_import(int stage, const uint8_t *d_buf)
{
  if (band_nrows_ <= 0 || !gpu_job_ || !d_buf) return false;
  PicJob &job = *gpu_job_;
  const int y = stage == 0 ? band_row0_ * 64 - 4 : (band_row0_ + band_nrows_) * 64 - 4;
  if (y < 0 || y + 4 > ph_) return false;
  size_t o = 0;
  if (hipMemcpyAsync(dpb_[job.slot].plane[0] + (size_t)y * pw_, d_buf + o, (size_t)pw_ * 4, hipMemcpyDeviceToDevice, stream_) != hipSuccess) return false;
  o += (size_t)pw_ * 4;
  for (int c = 1; c < 3; c++) { if (hipMemcpyAsync(dpb_[job.slot].plane[c] + (size_t)(y / 2) * (pw_ / 2), d_buf + o, (size_t)pw_, hipMemcpyDeviceToDevice, stream_) != hipSuccess) return false; o += (size_t)pw_; }
  if (stage == 0 && hipMemcpyAsync(band_din_ + (size_t)(y / 4) * (pw_ / 4) * sizeof(B4Rec), d_buf + o, (size_t)(pw_ / 4) * sizeof(B4Rec), hipMemcpyDeviceToDevice, stream_) != hipSuccess) return false;
  return hipStreamSynchronize(stream_) == hipSuccess;
}
bool Decoder::band_deblock()
{
  if (band_nrows_ <= 0 || !gpu_job_) return false;
  if (!gpu_job_->sh.deblock_disabled) launch_dec_deblock(band_f_, stream_);
  return hipEventRecord(gpu_job_->done, stream_) == hipSuccess;
}
int Decoder::band_finish()
{
  if (band_nrows_ <= 0 || !gpu_job_) return 0;
  PicJob *j = gpu_job_; gpu_job_ = nullptr;
  if (hipEventRecord(j->done, stream_) != hipSuccess) return DEC_ERR_GPU;
  return complete_gpu(*j);
}

bool Decoder::get_picture(DecodedPicture *out)
{
  if (!pic_ready_) return false;
  *out = out_;
  return true;
}

bool Decoder::debug_copy(const char *what, void *dst, size_t bytes)
{
  if (!w_) return false;
  const size_t npx = (size_t)pw_ * ph_;
  std::string w(what);
  // concealment v3: the stand-in filled last (its buffer as it lies in memory: Y | Cb | Cr, pitch = the padded width) and its table of displacements
  if (w == "standin") { if (standin_slot_ < 0 || bytes > npx * 3 / 2) return false; return hipDeviceSynchronize() == hipSuccess && hipMemcpy(dst, dpb_[standin_slot_].plane[0], bytes, hipMemcpyDeviceToHost) == hipSuccess; }
  if (w == "standin_ms") { if (bytes != sizeof(float) || standin_ms_ < 0) return false; memcpy(dst, &standin_ms_, sizeof(float)); return true; }      // (either mode, with set_profiling: the last stand-in's fill, ms)
  if (w == "take_backs") { if (bytes != sizeof(uint32_t)) return false; memcpy(dst, &take_backs_, sizeof(uint32_t)); return true; }      // pictures taken back so far (take_back_job): what the tests of that path assert
  if (w == "fill_mv") { if (fill_tab_.empty() || bytes > fill_tab_.size() * sizeof(int16_t)) return false; memcpy(dst, fill_tab_.data(), bytes); return true; }      // partial pictures: the table used last
  if (w == "partial_layout") {
    // partial pictures: the layout (layout_of) of the damaged picture filed last; before the first one, of the picture parsed last (the synchronous and the parse-only
    // decoder: its parse has ended)
    std::vector<uint8_t> lay = damaged_layout_;
    if (lay.empty()) {
      if (job_head_ < 1) return false;
      const PicJob &job = jobs_[(size_t)((job_head_ - 1) % (long)jobs_.size())];
      if (job.state.load(std::memory_order_acquire) == 1 || !job.h_in) return false;
      lay = layout_of(job);
    }
    if (bytes != lay.size()) return false;
    memcpy(dst, lay.data(), bytes);
    return true;
  }
  if (w == "standin_mv") { if (standin_slot_ < 0 || bytes > standin_tab_.size() * sizeof(int16_t)) return false; memcpy(dst, standin_tab_.data(), bytes); return true; }
  for (int c = 0; c < 3; c++) {
    size_t n = c ? npx / 4 : npx;
    if (w == std::string("rec") + char('0' + c)) { if (bytes > n) return false; return hipMemcpy(dst, dpb_[out_slot_].plane[c], bytes, hipMemcpyDeviceToHost) == hipSuccess; }
  }
  return false;
}

}  // namespace kvzx
