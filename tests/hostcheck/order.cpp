// tests/hostcheck/order.cpp -- host build of the decoder's output-order rules (kvazzup_amd/csrc/dec_order.h: plain C++, no HIP) with payload = the picture's serial,
// for tests/test_output_order.py, which holds them to a restatement of C.5.2 as tests/pyhevc.py states it.  Test infrastructure.
#include <utility>
#include "../../kvazzup_amd/csrc/dec_order.h"

using namespace kvzx;

namespace { struct Order { OutputOrder<uint64_t> o; OrderMark mark; }; }

extern "C" {

void *ho_new() { return new Order; }
void ho_free(void *h) { delete (Order *)h; }
// -> the serial; dropped[0 .. *ndropped): the payloads of discarded pictures that had completed (cap entries at most are written)
uint64_t ho_submitted(void *h, int poc, int num_reorder, int starts_cvs, int discard_prior, int no_output, uint64_t *dropped, int cap, int *ndropped)
{
  int n = 0;
  const uint64_t s = ((Order *)h)->o.submitted(poc, num_reorder, starts_cvs != 0, discard_prior != 0, no_output != 0, [&](uint64_t &p) { if (n < cap) dropped[n] = p; n++; });
  *ndropped = n;
  return s;
}
void ho_mark(void *h) { ((Order *)h)->mark = ((Order *)h)->o.mark(); }
void ho_restore(void *h) { ((Order *)h)->o.restore(std::move(((Order *)h)->mark)); }
int ho_discarded(void *h, uint64_t serial) { return ((Order *)h)->o.discarded(serial) ? 1 : 0; }
void ho_sequence_ended(void *h) { ((Order *)h)->o.sequence_ended(); }
int ho_idle(void *h) { return ((Order *)h)->o.idle() ? 1 : 0; }
void ho_completed(void *h, uint64_t serial, int poc, int cvs, int num_reorder, int in_turn) { ((Order *)h)->o.completed(serial, OrderKey{serial, poc, cvs, num_reorder}, in_turn != 0); }
int ho_next(void *h, int flush, uint64_t *serial) { return ((Order *)h)->o.next(flush != 0, *serial) ? 1 : 0; }
void ho_drain(void *h) { ((Order *)h)->o.drain(); }

}
