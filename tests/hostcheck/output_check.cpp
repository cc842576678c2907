// tests/hostcheck/output_check.cpp -- kvazzup_amd/csrc/dec_output.h (the decoder's owned output copies, their pool, the two retirement clocks) on the CPU under
// AddressSanitizer and UBSan: a stand-alone program whose own malloc-backed functions stand in for the HIP calls the component makes.
// Build and run (make -C tests/hostcheck output_check):
//   hipcc -std=c++17 -g -O1 -Wall -Wno-unused-value -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer output_check.cpp -o build/output_check && build/output_check
// Test infrastructure; not part of libhostcheck.so, never loaded into Python, never run on a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include "../../kvazzup_amd/csrc/dec_output.h"

namespace {
std::set<void *> live_dev, live_host, live_ev;
int mallocs = 0, bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "output_check: line %d: %s\n", __LINE__, #c); bad++; } } while (0)
}

extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { *p = malloc(n ? n : 1); memset(*p, 0xa5, n); live_dev.insert(*p); mallocs++; return hipSuccess; }
hipError_t hipFree(void *p) { if (!p) return hipSuccess; if (!live_dev.erase(p)) { bad++; return hipErrorInvalidValue; } free(p); return hipSuccess; }
hipError_t hipHostFree(void *p) { if (!live_host.erase(p)) { bad++; return hipErrorInvalidValue; } free(p); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t w, size_t h, hipMemcpyKind, hipStream_t)
{
  for (size_t y = 0; y < h; y++) memcpy((uint8_t *)dst + y * dpitch, (const uint8_t *)src + y * spitch, w);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)malloc(8); live_ev.insert(*e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { return live_ev.count(e) ? hipSuccess : hipErrorInvalidValue; }
hipError_t hipEventSynchronize(hipEvent_t e) { return live_ev.count(e) ? hipSuccess : hipErrorInvalidValue; }
hipError_t hipEventDestroy(hipEvent_t e) { if (!live_ev.erase(e)) { bad++; return hipErrorInvalidValue; } free(e); return hipSuccess; }
}

namespace {
using namespace kvzx;
// a picture as Decoder::describe_output hands it over: the ring's planes (pitch > width), here a malloc each, exactly as large as the copies may read -- the device copy
// takes `width` bytes of every row, the host copy pitch x rows
struct Source {
  uint8_t *plane[3], *hplane[3]; DecodedPicture pic;
  Source(int w, int h, uint64_t serial, int poc, int cvs, int nr)
  {
    pic.width = w; pic.height = h; pic.serial = serial; pic.poc = poc; pic.cvs = cvs; pic.num_reorder = nr;
    for (int c = 0; c < 3; c++) {
      const int pw = (c ? w / 2 : w) + 24, ph = c ? h / 2 : h, cw = c ? w / 2 : w;
      plane[c] = (uint8_t *)malloc((size_t)pw * (ph - 1) + cw);
      for (int y = 0; y < ph; y++) for (int x = 0; x < cw; x++) plane[c][(size_t)y * pw + x] = (uint8_t)(serial * 7 + c * 50 + y * 3 + x);
      hplane[c] = (uint8_t *)calloc((size_t)pw, (size_t)ph);
      for (int y = 0; y < ph; y++) memcpy(hplane[c] + (size_t)y * pw, plane[c] + (size_t)y * pw, (size_t)cw);
      pic.dev[c] = plane[c]; pic.host[c] = hplane[c]; pic.dev_pitch[c] = pic.host_pitch[c] = pw;
    }
  }
  ~Source() { for (auto p : plane) free(p); for (auto p : hplane) free(p); }
};
// the picture handed out is the dense copy of its source, on the device side and (download) on the host side
void same(const DecodedPicture &o, const Source &s, bool download)
{
  EXPECT(o.serial == s.pic.serial && o.width == s.pic.width);
  for (int c = 0; c < 3; c++) {
    const int w = c ? o.width / 2 : o.width, h = c ? o.height / 2 : o.height;
    EXPECT(o.dev_pitch[c] == w && live_dev.count((void *)o.dev[0]));
    for (int y = 0; y < h; y++) {
      EXPECT(!memcmp(o.dev[c] + (size_t)y * w, s.plane[c] + (size_t)y * s.pic.dev_pitch[c], (size_t)w));
      if (download) EXPECT(o.host[c] != s.hplane[c] && !memcmp(o.host[c] + (size_t)y * o.host_pitch[c], s.plane[c] + (size_t)y * s.pic.host_pitch[c], (size_t)w));
    }
  }
}
// one picture of a sequence that does not reorder through the component: completed in its turn behind something queued, or ahead of its turn
uint64_t serial = 100;
bool put(DecOutput &out, int w, int h, bool in_turn, bool download) { serial++; Source s(w, h, serial, (int)serial, 1, 0); return out.completed(s.pic, in_turn, download, nullptr); }

void clocks(int hold)
{
  DecOutput out(0); out.set_hold(hold);
  DecodedPicture o;
  Source a(64, 32, 1, 0, 1, 0), b(64, 32, 2, 1, 1, 0);
  EXPECT(out.idle()); mallocs = 0;
  const uint64_t first = serial + 1;
  EXPECT(out.completed(a.pic, false, true, nullptr) && out.completed(b.pic, false, true, nullptr) && !out.idle() && mallocs == 2);
  EXPECT(out.next(false, o)); same(o, a, true);
  EXPECT(out.next(false, o)); same(o, b, true);               // a is retired at (calls 0, clock 0); b is the current picture
  EXPECT(!out.next(true, o) && out.idle());
  // promise 1 alone has run out: nine calls, no picture begun -- a's device copy is still held (the next copy finds no pooled buffer)
  for (int k = 0; k < DecOutput::kOutHold + 1; k++) out.begin_call();
  mallocs = 0; EXPECT(put(out, 64, 32, false, false) && mallocs == 1 && live_dev.size() == 3);
  // ... and promise 2 up to its last picture: still held; one more picture begun: the copy goes to the pool with the next call and is used again
  for (int k = 0; k < hold; k++) out.begin_picture();
  out.begin_call(); EXPECT(put(out, 64, 32, false, false) && mallocs == 2);
  out.begin_picture(); out.begin_call();
  EXPECT(put(out, 64, 32, false, false) && mallocs == 2 && live_dev.size() == 4);
  // the other way round: b retired now; pictures enough, calls too few
  EXPECT(out.next(false, o) && o.serial == first);
  for (int k = 0; k < hold + 1; k++) out.begin_picture();
  for (int k = 0; k < DecOutput::kOutHold; k++) out.begin_call();
  EXPECT(put(out, 64, 32, false, false) && mallocs == 3);
  out.begin_call(); EXPECT(put(out, 64, 32, false, false) && mallocs == 3);
  // a page-locked buffer the decoder gave up: freed with the ninth call after
  void *pinned = malloc(100); live_host.insert(pinned); out.retire_host((uint8_t *)pinned);
  for (int k = 0; k < DecOutput::kOutHold; k++) out.begin_call();
  EXPECT(live_host.size() == 1); out.begin_call(); EXPECT(live_host.empty());
}     // (destroyed with a current picture, ready pictures and a pool)

void pool_and_sizes()
{
  DecOutput out(0); out.set_hold(1);
  DecodedPicture o;
  // a full pool at one size: thirty pictures handed out and retired, both promises run out -- two dozen buffers are kept, the rest freed
  for (int k = 0; k < 30; k++) EXPECT(put(out, 48, 16, false, false));
  for (int k = 0; k < 30; k++) EXPECT(out.next(false, o));
  for (int k = 0; k < 10; k++) { out.begin_picture(); out.begin_call(); }
  EXPECT(live_dev.size() == DecOutput::kOwnedPoolMax + 1);        // (+ the current picture)
  mallocs = 0; for (int k = 0; k < 5; k++) EXPECT(put(out, 48, 16, false, false));
  EXPECT(mallocs == 0 && live_dev.size() == DecOutput::kOwnedPoolMax + 1);
  // another size with the pool (19 left) in use: every pooled buffer goes at once; the old size's pictures still queued stay valid and are freed, not pooled, later
  EXPECT(put(out, 80, 48, false, false) && mallocs == 1 && live_dev.size() == 1 + 5 + 1);
  for (int k = 0; k < 6; k++) EXPECT(out.next(false, o));
  EXPECT(o.width == 80);
  for (int k = 0; k < 10; k++) { out.begin_picture(); out.begin_call(); }
  EXPECT(live_dev.size() == 1 + 6);                                 // (the old size's copies met an empty pool and are kept -- until the new size asks again)
  EXPECT(put(out, 80, 48, false, false) && mallocs == 2 && live_dev.size() == 2);
}

void discarded_payloads()
{
  DecOutput out(0);
  DecodedPicture o;
  // a reordering sequence (two pictures may overtake one): three submitted -- the first has had its turn in decoding order when the third arrives --, two completed
  // and waiting, then an IDR picture with no_output_of_prior_pics_flag: the second's copy goes back to the pool, the first still leaves ahead of the new sequence
  const uint64_t s1 = out.submitted(1, 2, true, false, false), s2 = out.submitted(4, 2, false, false, false), s3 = out.submitted(2, 2, false, false, false);
  Source a(32, 16, s1, 1, 1, 2), b(32, 16, s2, 4, 1, 2);
  EXPECT(out.completed(a.pic, true, false, nullptr) && out.completed(b.pic, true, false, nullptr) && !out.next(false, o) && live_dev.size() == 2);
  const uint64_t s4 = out.submitted(0, 0, true, true, false);
  EXPECT(s4 == s3 + 1 && !out.discarded(s1) && out.discarded(s2) && out.discarded(s3) && !out.discarded(s4) && !out.idle() && live_dev.size() == 2);
  mallocs = 0; Source d(32, 16, s4, 0, 2, 0);
  EXPECT(out.completed(d.pic, false, false, nullptr) && mallocs == 0);      // (b's buffer, from the pool)
  EXPECT(out.next(false, o)); same(o, a, false);
  EXPECT(!out.next(false, o) && out.next(true, o)); same(o, d, false);      // (completed ahead of its turn behind pictures that waited: it leaves with the next picture of its sequence, or with the flush)
  EXPECT(out.idle());
}

void every_queue()
{
  DecOutput *out = new DecOutput(0);
  DecodedPicture o;
  for (int k = 0; k < 3; k++) EXPECT(put(*out, 64, 64, false, true));
  EXPECT(out->next(false, o) && out->next(false, o));               // one retired, one current, one ready
  const uint64_t s = out->submitted(8, 3, true, false, false);
  Source w(64, 64, s, 8, 2, 3);
  EXPECT(out->completed(w.pic, true, true, nullptr));                 // one waiting
  for (int k = 0; k < 12; k++) { out->begin_picture(); out->begin_call(); }      // the retired one is pooled
  EXPECT(out->next(false, o));                                       // ... and the next one retired
  void *pinned = malloc(64); live_host.insert(pinned); out->retire_host((uint8_t *)pinned);
  EXPECT(live_dev.size() == 4 && live_ev.size() == 1 && live_host.size() == 1);
  delete out;
  EXPECT(live_dev.empty() && live_ev.empty() && live_host.empty());
}
}  // namespace

int main()
{
  for (int hold : {1, 8}) { clocks(hold); EXPECT(live_dev.empty() && live_host.empty() && live_ev.empty()); }
  pool_and_sizes(); EXPECT(live_dev.empty() && live_ev.empty());
  discarded_payloads(); EXPECT(live_dev.empty() && live_ev.empty());
  every_queue();
  if (bad) { fprintf(stderr, "output_check: %d failed\n", bad); return 1; }
  printf("output_check: ok (both clocks at hold 1 and 8, pool reuse, a size change with the pool full, discarded payloads, destruction with pictures in every queue)\n");
  return 0;
}
