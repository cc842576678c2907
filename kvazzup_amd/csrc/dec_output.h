// kvazzup_amd/csrc/dec_output.h -- the decoder's output side between "a picture's kernels have finished" and "the caller may no longer read the planes it was
// handed": the order pictures leave in (dec_order.h, plain C++) and, here, the storage of the pictures that cannot be handed out where they lie in the decoder's
// ring -- copies that own their samples, the pool their device memory comes from, and the two lifetime promises.  The statement of record for all of it.
//
// Promise 1, calls: frame memory handed out by get_picture stays valid while kOutHold further NAL units are decoded -- a caller may copy it out on a stage of its
// own (OpenHEVCFilter's output thread) -- also across a resolution change: the host output buffers and the owned pictures that such a change retires are only freed
// kOutHold calls later.  Promise 2, pictures (kvzx_decoder_set_output_hold; device-resident output): the planes handed out stay untouched while the next hold()
// pictures are begun -- pictures, not NAL units (an access unit may bring parameter sets, SEI messages, a delimiter): the calls that began a picture, and the EOS / EOB
// calls, which move the ring on by one picture like them.  An owned picture goes only when BOTH have run out; the ring's own buffers: Decoder::alloc_slot, by hold() too.
#pragma once
#include <hip/hip_runtime.h>
#include "dec_order.h"

namespace kvzx {

struct DecodedPicture {
  int width = 0, height = 0;          // cropped
  int coded_w = 0, coded_h = 0;
  const uint8_t *host[3] = {nullptr, nullptr, nullptr}; int host_pitch[3] = {0, 0, 0};
  const uint8_t *dev[3] = {nullptr, nullptr, nullptr}; int dev_pitch[3] = {0, 0, 0};
  int poc = 0; int64_t pts = 0; uint32_t fps_num = 0, fps_den = 0; bool is_intra = false;
  int cvs = 0, num_reorder = 0;       // coded video sequence the picture belongs to (a running count); its SPS's sps_max_num_reorder_pics
  uint64_t serial = 0;                // the picture's number in decoding order (dec_order.h: which waiting pictures an IDR / BLA picture discards)
  int missing_ctbs = 0, total_ctbs = 0;      // partial pictures: coding tree blocks of the picture that never arrived and were filled in (0: the picture is whole)
};

// a finished picture that owns its samples: one of a stream that reorders, or what is still in the frame-threaded ring when the stream changes its resolution --
// completed and kept like this until the following calls have handed it out (the decoder's own buffers are re-sized meanwhile)
struct OwnedPic {
  DecodedPicture pic;
  std::vector<uint8_t> host;          // download mode: the three planes back to back, pitches as in pic.host_pitch
  uint8_t *dev = nullptr; size_t dev_bytes = 0;      // one allocation holding the three planes, dense (pitch = width)
};

class DecOutput {
 public:
  static constexpr int kOutHold = 8;
  static constexpr size_t kOwnedPoolMax = 24;      // device buffers kept for the next picture of the same size
  explicit DecOutput(int device) : device_(device) {}
  DecOutput(const DecOutput &) = delete; DecOutput &operator=(const DecOutput &) = delete; ~DecOutput() { release(); }
  void set_hold(int n) { hold_ = n; } int hold() const { return hold_; }
  // ---- the two clocks: every decode call; every call that begins a picture or ends a sequence
  void begin_call() { calls_++; if (!retired_host_.empty() || !retired_.empty()) free_retired(false); } void begin_picture() { clock_++; }
  void retire_host(uint8_t *pinned) { retired_host_.emplace_back(calls_, pinned); }      // a page-locked output buffer the decoder gives up: freed kOutHold calls later
  // ---- order (dec_order.h); the copies of discarded pictures that had completed go back to the pool
  uint64_t submitted(int poc, int num_reorder, bool starts_cvs, bool discard_prior, bool no_output) { return order_.submitted(poc, num_reorder, starts_cvs, discard_prior, no_output, [this](OwnedPic &o) { recycle(o); }); }
  const OrderMark &mark() const { return order_.mark(); } void restore(OrderMark &&m) { order_.restore(std::move(m)); }
  bool discarded(uint64_t serial) const { return order_.discarded(serial); } void sequence_ended() { order_.sequence_ended(); }
  bool idle() const { return order_.idle(); } void drain() { order_.drain(); }
  // `pic` (complete on the device; what Decoder::describe_output said) is copied into storage of its own and takes its place in the order.  The device copy is
  // dense (pitch = width), so that device-resident consumers keep working across a re-allocation; it comes from the pool (a hipMalloc / hipFree per picture of a
  // reordering stream synchronised the whole device -- every other encoder and decoder of the process with it) and is made on `st`, the download stream, which
  // this thread waits for by event: the picture's kernels are complete, so the copies depend on nothing in another stream.
  bool completed(const DecodedPicture &pic, bool in_turn, bool download, hipStream_t st)
  {
    OwnedPic o; o.pic = pic;
    for (int c = 0; c < 3 && download; c++) o.host.insert(o.host.end(), pic.host[c], pic.host[c] + (size_t)pic.host_pitch[c] * (c ? pic.height / 2 : pic.height));      // plane after plane, pitch x rows each (next() rebuilds the pointers the same way)
    if (!(o.dev = alloc(o.dev_bytes = (size_t)pic.width * pic.height * 3 / 2))) return false;
    size_t off = 0; bool ok = true;
    for (int c = 0; c < 3 && ok; c++) {
      const int w = c ? pic.width / 2 : pic.width, h = c ? pic.height / 2 : pic.height;
      ok = hipMemcpy2DAsync(o.dev + off, (size_t)w, pic.dev[c], (size_t)pic.dev_pitch[c], (size_t)w, (size_t)h, hipMemcpyDeviceToDevice, st) == hipSuccess;
      o.pic.dev[c] = o.dev + off; o.pic.dev_pitch[c] = w; off += (size_t)w * h;
    }
    ok = ok && (ev_ || hipEventCreateWithFlags(&ev_, hipEventDisableTiming) == hipSuccess) && hipEventRecord(ev_, st) == hipSuccess && hipEventSynchronize(ev_) == hipSuccess;
    if (ok) order_.completed(std::move(o), OrderKey{pic.serial, pic.poc, pic.cvs, pic.num_reorder}, in_turn); else recycle(o);
    return ok;
  }
  // the next picture to hand out, one per call at most -> out, valid like any handed-out picture; the one handed out before it is retired (the caller may still be copying it out)
  bool next(bool flush, DecodedPicture &out)
  {
    OwnedPic p; size_t off = 0;
    if (!order_.next(flush, p)) return false;
    if (cur_.dev || !cur_.host.empty()) retired_.push_back(Retired{calls_, clock_, std::move(cur_)});
    cur_ = std::move(p); out = cur_.pic;
    for (int c = 0; c < 3 && !cur_.host.empty(); c++) { out.host[c] = cur_.host.data() + off; off += (size_t)out.host_pitch[c] * (c ? out.height / 2 : out.height); }
    return true;
  }
  // everything goes, whatever was promised (the decoder closes: before its streams are released)
  void release()
  {
    free_retired(true); order_.for_each([this](OwnedPic &o) { recycle(o); }); recycle(cur_); cur_ = OwnedPic(); drop_pool();      // (through the pool, which goes last)
    if (ev_) { hipEventDestroy(ev_); ev_ = nullptr; }
  }

 private:
  // the pool holds ONE size: when another one is asked for the stream has changed its resolution -- every pooled buffer of the old size goes at once (at 4K two dozen
  // of them are 288 MB).  An OwnedPic knows the size of its allocation, so a buffer never enters the pool under another one's.
  void drop_pool() { for (uint8_t *p : pool_) hipFree(p); pool_.clear(); }
  uint8_t *alloc(size_t bytes)
  {
    if (!pool_.empty() && pool_bytes_ == bytes) { uint8_t *p = pool_.front(); pool_.erase(pool_.begin()); return p; }
    drop_pool(); uint8_t *p = nullptr;
    return hipSetDevice(device_) == hipSuccess && hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
  }
  void recycle(OwnedPic &o)
  {
    if (o.dev && pool_.size() < kOwnedPoolMax && (pool_.empty() || pool_bytes_ == o.dev_bytes)) { pool_bytes_ = o.dev_bytes; pool_.push_back(o.dev); } else if (o.dev) hipFree(o.dev);
    o.dev = nullptr;
  }
  // a host buffer: kOutHold calls after its retirement; an owned picture: when both promises have run out (all: whatever was promised)
  void free_retired(bool all)
  {
    for (; !retired_host_.empty() && (all || calls_ - retired_host_.front().first > kOutHold); retired_host_.pop_front()) hipHostFree(retired_host_.front().second);
    for (; !retired_.empty() && (all || (calls_ - retired_.front().calls > kOutHold && clock_ - retired_.front().clock > hold_)); retired_.pop_front()) recycle(retired_.front().pic);
  }
  int device_, hold_ = 2; long calls_ = 0, clock_ = 0;
  OutputOrder<OwnedPic> order_; OwnedPic cur_;      // completed and not handed out yet; the one last handed out
  std::deque<std::pair<long, uint8_t *>> retired_host_;      // (call count at retirement, page-locked buffer)
  struct Retired { long calls, clock; OwnedPic pic; }; std::deque<Retired> retired_;
  std::vector<uint8_t *> pool_; size_t pool_bytes_ = 0; hipEvent_t ev_ = nullptr;
};

}  // namespace kvzx
