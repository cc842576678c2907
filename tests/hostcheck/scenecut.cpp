// tests/hostcheck/scenecut.cpp -- host build of scenecut's statement functions (hevc_core.h sc_*; "uvgx scene cut v1") for
// tests/test_scenecut_host.py, which holds them to the numpy restatement tests/scenecut_model.py.  Built by that test on its own (g++, into pytest's
// temporary directory) so that libhostcheck.so and its Makefile stay as they are; folding it into that library is a follow-up.  Test infrastructure.
#include <cstddef>
#include <cstring>
#include "../../kvazzup_amd/csrc/hevc_core.h"

using namespace kvzx;

extern "C" {

int hs_reach(int me_coarse) { return sc_reach(me_coarse); }
void hs_visible_blocks(int width, int height, int *out) { sc_visible_blocks(width, height, &out[0], &out[1]); }
int hs_mean_shift(long long sc, long long sp, long long n) { return sc_mean_shift(sc, sp, n); }
int hs_ref_sample(int p, int d) { return sc_ref_sample(p, d); }
int hs_block_mean(int sum) { return sc_block_mean(sum); }
int hs_is_new(unsigned S, unsigned A) { return sc_is_new(S, A) ? 1 : 0; }
int hs_verdict(int n_new, int n_b) { return sc_verdict(n_new, n_b) ? 1 : 0; }
int hs_examined(int since_idr, int N, int periodic) { return sc_examined(since_idr, N, periodic != 0) ? 1 : 0; }

// (S, A) of every visible block of a picture width x height whose quarter picture qc (qw x qh) is compared with qp shifted by d: out[block, raster][2]
void hs_blocks(const uint8_t *qc, const uint8_t *qp, int qw, int qh, int width, int height, int rq, int d, uint32_t *out)
{
  int bw, bh;
  sc_visible_blocks(width, height, &bw, &bh);
  for (int by = 0; by < bh; by++) for (int bx = 0; bx < bw; bx++) sc_block_stat(qc, qp, qw, qh, bx, by, rq, d, &out[2 * (by * bw + bx)], &out[2 * (by * bw + bx) + 1]);
}

}
