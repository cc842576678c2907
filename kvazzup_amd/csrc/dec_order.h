// kvazzup_amd/csrc/dec_order.h -- the decoder's output order (H.265 C.5.2) as this decoder applies it under frame threads: pure bookkeeping, no HIP, no
// picture memory -- the picture is an opaque payload P (dec_output.h: an OwnedPic; tests/hostcheck/order.cpp: its serial).  The statement of record.
//
// Two orders meet here.  DECODING order, at submit time (C.5.2.2, C.5.2.3): the pictures that are "needed for output" and have not had their turn, (serial, POC),
// bumped by the standard's counting rule.  The pictures themselves complete later (frame threads) and leave by the same rule; this list exists so that an IDR / BLA
// picture with no_output_of_prior_pics_flag discards exactly the pictures the standard's process would still hold at that instant, whatever the threads' timing.
// COMPLETION order: a stream whose SPS allows reordering (sps_max_num_reorder_pics > 0: B pictures in groups, Kvazaar gop=8) has its pictures handed on by POC --
// the smallest of those waiting once more than the SPS's count wait, all of a coded video sequence before the next one's first, the rest one per call when the
// stream ends.  A low-delay stream (the count is 0) with nothing queued never enters this: idle() is the decoder's fast path.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <deque>
#include <utility>
#include <vector>

namespace kvzx {

struct OrderKey { uint64_t serial; int poc, cvs, num_reorder; };      // number in decoding order, POC, coded video sequence (a running count), its SPS's sps_max_num_reorder_pics
using OrderMark = std::vector<std::pair<uint64_t, int>>;              // the decoding-order list as it was before a picture was submitted (mark / restore: a picture taken back)

template <class P> class OutputOrder {
 public:
  // ---- decoding order.  A picture is submitted: -> its serial.  starts_cvs: NoRaslOutputFlag (8.1.3); discard_prior: no_output_of_prior_pics_flag in force -- what still
  // waits is discarded: the ones that have completed go to drop(P &) for release, the others are found by discarded() when they complete
  template <class F> uint64_t submitted(int poc, int num_reorder, bool starts_cvs, bool discard_prior, bool no_output, F &&drop)
  {
    const uint64_t serial = ++serial_;
    auto bump = [&] { size_t b = 0; for (size_t i = 1; i < wait_.size(); i++) if (wait_[i].second < wait_[b].second) b = i; wait_.erase(wait_.begin() + (long)b); };
    if (starts_cvs) {
      if (discard_prior && !wait_.empty()) {
        for (const auto &v : wait_) discarded_.push_back(v.first);
        for (size_t i = 0; i < waiting_.size();) if (discarded(waiting_[i].key.serial)) { drop(waiting_[i].pic); waiting_.erase(waiting_.begin() + (long)i); } else i++;
        if (discarded_.size() > 64) discarded_.erase(discarded_.begin(), discarded_.end() - 64);
      }
      wait_.clear();
    } else while ((int)wait_.size() > num_reorder) bump();
    if (!no_output) { wait_.emplace_back(serial, poc); while ((int)wait_.size() > num_reorder) bump(); }
    return serial;
  }
  const OrderMark &mark() const { return wait_; } void restore(OrderMark &&m) { wait_ = std::move(m); }
  bool discarded(uint64_t serial) const { return std::find(discarded_.begin(), discarded_.end(), serial) != discarded_.end(); }      // (an IDR / BLA picture behind it said so: C.5.2.2)
  void sequence_ended() { wait_.clear(); }                           // EOS / EOB: everything that waits will have its turn
  // ---- completion order.  idle: nothing completed is queued -- a picture of a sequence that does not reorder may be handed out where it lies
  bool idle() const { return ready_.empty() && waiting_.empty(); }
  // A picture has completed.  A reordering sequence: it waits with its sequence and POC.  in_turn (the call that completed it hands out): a sequence that does not
  // reorder behind one that did -- everything still waiting precedes this picture: all of it becomes ready at once, in order, the picture behind it; every later
  // call, parameter sets included, hands one out, so the lag the old sequence needed drains instead of staying until the end of the stream.  Ahead of its turn (the
  // ring emptied at a resolution change, a picture closed by the next one's first NAL unit): it joins what waits, if anything does, and keeps its place by sequence.
  void completed(P pic, const OrderKey &key, bool in_turn)
  {
    if (key.num_reorder > 0) reorder_ = key.num_reorder;
    else if (in_turn) drain();
    if (key.num_reorder > 0 || !waiting_.empty()) waiting_.push_back(Waiting{std::move(pic), key}); else ready_.push_back(std::move(pic));
  }
  // the next picture to hand out, one per call at most; flush: the stream has ended (EOS / EOB with nothing left in the pipeline)
  bool next(bool flush, P &out) { if (ready_.empty() && !pop(flush)) return false; out = std::move(ready_.front()); ready_.pop_front(); return true; }
  void drain() { while (pop(true)) {} }                              // a new sequence follows (resolution change): what waited leaves in POC order, one picture per call
  template <class F> void for_each(F &&f) { for (auto &p : ready_) f(p); for (auto &w : waiting_) f(w.pic); }

 private:
  // C.5.2.4: of the waiting pictures of the oldest coded video sequence the one with the smallest POC becomes ready -- when more of them wait than may overtake a
  // picture, when a later sequence has begun, or when the stream is over
  bool pop(bool flush)
  {
    if (waiting_.empty()) return false;
    int first_cvs = waiting_.front().key.cvs, n = 0; size_t best = 0; bool later = false;
    for (const Waiting &w : waiting_) if (w.key.cvs < first_cvs) first_cvs = w.key.cvs;
    for (size_t i = 0; i < waiting_.size(); i++) {
      if (waiting_[i].key.cvs != first_cvs) { later = true; continue; }
      if (n++ == 0 || waiting_[i].key.poc < waiting_[best].key.poc) best = i;
    }
    if (!(flush || later || n > reorder_)) return false;
    ready_.push_back(std::move(waiting_[best].pic)); waiting_.erase(waiting_.begin() + (long)best);
    return true;
  }
  OrderMark wait_; std::vector<uint64_t> discarded_; uint64_t serial_ = 0;      // decoding order: (serial, POC) needed for output; the last 64 serials discarded
  struct Waiting { P pic; OrderKey key; }; std::deque<P> ready_; std::deque<Waiting> waiting_; int reorder_ = 0;      // completion order; the reordering sequence's count
};

}  // namespace kvzx
