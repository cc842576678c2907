// tests/hostcheck/owner_check.cpp -- kvazzup_amd/csrc/hip_owner.h on the CPU under AddressSanitizer and UBSan: a stand-alone program whose own malloc-backed
// functions stand in for the HIP calls the owner makes, so that every hand-out, a failure midway, the release and a second release run without a device.
// Build and run (make -C tests/hostcheck owner_check):
//   hipcc -std=c++17 -g -O1 -Wall -Wno-unused-value -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer owner_check.cpp -o build/owner_check && build/owner_check
// Test infrastructure; not part of libhostcheck.so, never loaded into Python, never run on a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include "../../kvazzup_amd/csrc/hip_owner.h"

namespace {
std::set<void *> live_dev, live_host, live_ev;
int calls_left = -1;      // >= 0: that many more hand-outs succeed, the next one fails (once)
bool refuse() { if (calls_left < 0) return false; if (calls_left-- > 0) return false; return true; }
int bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "owner_check: line %d: %s\n", __LINE__, #c); bad++; } } while (0)
}

extern "C" {
hipError_t hipMalloc(void **p, size_t n) { if (refuse()) return hipErrorOutOfMemory; *p = malloc(n ? n : 1); memset(*p, 0xa5, n); live_dev.insert(*p); return hipSuccess; }
hipError_t hipMemset(void *p, int v, size_t n) { if (!live_dev.count(p)) return hipErrorInvalidValue; memset(p, v, n); return hipSuccess; }
hipError_t hipFree(void *p) { if (!p) return hipSuccess; if (!live_dev.erase(p)) { bad++; return hipErrorInvalidValue; } free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { if (refuse()) return hipErrorOutOfMemory; *p = malloc(n ? n : 1); live_host.insert(*p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) { if (!live_host.count(h)) return hipErrorInvalidValue; *d = h; return hipSuccess; }
hipError_t hipHostFree(void *p) { if (!live_host.erase(p)) { bad++; return hipErrorInvalidValue; } free(p); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { if (refuse()) return hipErrorOutOfMemory; *e = (hipEvent_t)malloc(8); live_ev.insert(*e); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { if (!live_ev.erase(e)) { bad++; return hipErrorInvalidValue; } free(e); return hipSuccess; }
}

int main()
{
  using kvzx::HipOwner;
  {
    HipOwner own;
    uint32_t *a = nullptr, *z = nullptr; uint8_t *b = nullptr; unsigned long long *none = nullptr;
    int32_t *h = nullptr, *d = nullptr; int8_t *plain = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    // some of each kind
    EXPECT(own.dev(&a, 100) == hipSuccess && a);
    EXPECT(own.dev(&z, 1000, true) == hipSuccess && z);
    for (int i = 0; i < 1000; i++) EXPECT(z[i] == 0);
    a[99] = 7; z[999] = 7;
    EXPECT(own.dev(&b, 33) == hipSuccess && b);
    EXPECT(own.dev(&none, 0, true) == hipSuccess);
    EXPECT(own.pinned(&h, 12, hipHostMallocMapped, &d) == hipSuccess && h && d == h);
    h[11] = 64;
    EXPECT(own.pinned(&plain, 510, hipHostMallocDefault) == hipSuccess && plain);
    EXPECT(own.event(&e0, hipEventDisableTiming) == hipSuccess && e0);
    EXPECT(own.event(&e1, hipEventDefault) == hipSuccess && e1);
    EXPECT(live_dev.size() == 4 && live_host.size() == 2 && live_ev.size() == 2);
    // a failure midway, of each kind: the error comes back, the pointer stays as it was, what was handed out before is still held
    uint16_t *f0 = nullptr, *f1 = nullptr; float *g = nullptr, *ga = nullptr;
    calls_left = 1;
    EXPECT(own.dev(&f0, 50, true) == hipSuccess && f0);
    EXPECT(own.dev(&f1, 50, true) == hipErrorOutOfMemory && !f1);
    calls_left = 0;
    EXPECT(own.pinned(&g, 5, hipHostMallocMapped, &ga) == hipErrorOutOfMemory && !g && !ga);
    calls_left = 0;
    EXPECT(own.event(&e2, hipEventDisableTiming) == hipErrorOutOfMemory && !e2);
    EXPECT(calls_left < 0);
    EXPECT(live_dev.size() == 5 && live_host.size() == 2 && live_ev.size() == 2);
    // ... and the owner goes on handing out afterwards (an encoder whose lazy site failed is still closed in the ordinary way)
    EXPECT(own.event(&e2, hipEventDisableTiming) == hipSuccess && e2);
    own.release();
    EXPECT(live_dev.empty() && live_host.empty() && live_ev.empty());
    own.release();                                   // again: nothing left to free
    EXPECT(bad == 0);
    // handed out after a release: held, and released by the destructor
    EXPECT(own.dev(&a, 10, true) == hipSuccess && own.event(&e0, 0) == hipSuccess);
    EXPECT(live_dev.size() == 1 && live_ev.size() == 1);
  }
  EXPECT(live_dev.empty() && live_host.empty() && live_ev.empty());
  if (bad) { fprintf(stderr, "owner_check: %d failed\n", bad); return 1; }
  printf("owner_check: ok (hand-outs of each kind, a refused hand-out of each kind, release, release again, destructor)\n");
  return 0;
}
