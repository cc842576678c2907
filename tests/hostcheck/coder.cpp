// tests/hostcheck/coder.cpp -- host build of the product's arithmetic coder (kvazzup_amd/csrc/entropy_host.h) for the CPU
// tests of the interleaved coder (tests/test_host_coder_rows.py) and its microbenchmark (tools/arith_bench.py).  Test infrastructure.
#include <chrono>
#include "../../kvazzup_amd/csrc/entropy_host.h"

using namespace kvzx;

static const CoreTabs &core_tabs()
{
  static CoreTabs t = [] { CoreTabs c; for (int i = 0; i < 64; i++) core_tabs_fill_entry(c, i); return c; }();
  return t;
}
static const HostCabacTabs &host_tabs() { static HostCabacTabs t; return t; }

static void play_rows(int lanes, HostSub *sub, int nsub)
{
  switch (lanes) {
    case 1: cabac_play_rows_host<1>(host_tabs(), &core_tabs(), sub, nsub); break;
    case 2: cabac_play_rows_host<2>(host_tabs(), &core_tabs(), sub, nsub); break;
    case 3: cabac_play_rows_host<3>(host_tabs(), &core_tabs(), sub, nsub); break;
    default: cabac_play_rows_host<4>(host_tabs(), &core_tabs(), sub, nsub); break;
  }
}

extern "C" {

// Substreams given directly: substream k is the runs [run_first[k], run_first[k + 1]) of run_len (tokens taken from `tok` one run after
// the other), starting from contexts ctx0 + k * CTX_COUNT.  lanes = 0: every substream through cabac_play_tokens_host() on its own (the
// reference), else cabac_play_rows_host<lanes>.  Substream k's bytes go to out + k * cap; len[k], bins[k] receive its byte and bin counts.
int hcr_play(int lanes, const uint16_t *tok, const int32_t *run_len, const int32_t *run_first, int nsub, const uint8_t *ctx0,
             uint8_t *out, int cap, int32_t *len, uint32_t *bins)
{
  std::vector<HostRun> runs((size_t)run_first[nsub]);
  for (size_t i = 0, o = 0; i < runs.size(); o += (size_t)run_len[i], i++) runs[i] = {tok + o, run_len[i]};
  std::vector<HostSub> sub((size_t)nsub);
  for (int k = 0; k < nsub; k++) {
    HostSub &s = sub[(size_t)k];
    s.run = runs.data() + run_first[k]; s.nrun = run_first[k + 1] - run_first[k]; s.ctx0 = ctx0 + (size_t)k * CTX_COUNT;
    s.out = out + (size_t)k * cap; s.cap = cap; s.len = -1; s.bins = 0;
  }
  if (lanes == 0) {
    for (HostSub &s : sub) {
      uint8_t ctx[CTX_COUNT]; memcpy(ctx, s.ctx0, CTX_COUNT);
      CabacEnc c; c.nbins = 0;
      cabac_start(c, s.out, s.cap, ctx, &core_tabs());
      for (int i = 0; i < s.nrun; i++) cabac_play_tokens_host(c, host_tabs(), s.run[i].tok, s.run[i].n);
      cabac_finish(c);
      s.len = c.pos; s.bins = c.nbins;
    }
  } else play_rows(lanes, sub.data(), nsub);
  for (int k = 0; k < nsub; k++) { len[k] = sub[(size_t)k].len; bins[k] = sub[(size_t)k].bins; }
  return 0;
}

// A whole picture through EntropyHost::code_picture (threads: its pool; lanes as set_lanes(), 1 = the per-substream coder).  Substream k's
// bytes go to out + k * cap, len[k] its length; returns the number of substreams (or -1: more than max_sub), *bins the picture's bins.
int hcr_code_picture(int threads, int lanes, const uint16_t *tokens, const int32_t *count, const uint32_t *offset, int wc, int hc, int wpp,
                     int tile_rows, int tile_cols, int init_type, int qp, uint8_t *out, int cap, int32_t *len, int max_sub, unsigned long long *bins)
{
  EntropyHost e(threads);
  e.set_lanes(lanes);
  std::vector<std::vector<uint8_t>> rows;
  uint64_t b = 0;
  e.code_picture(tokens, count, offset, wc, hc, wpp != 0, tile_rows, init_type, qp, rows, &b, tile_cols);
  if ((int)rows.size() > max_sub) return -1;
  for (size_t k = 0; k < rows.size(); k++) {
    len[k] = (int32_t)rows[k].size();
    if ((int)rows[k].size() > cap) return -1;
    memcpy(out + k * (size_t)cap, rows[k].data(), rows[k].size());
  }
  *bins = b;
  return (int)rows.size();
}

// The same for EntropyHost::code_band (the substreams of CTU rows [row0, row0 + nrows)).
int hcr_code_band(int threads, int lanes, const uint16_t *tokens, const int32_t *count, const uint32_t *offset, int wc, int hc, int wpp,
                  int tile_rows, int init_type, int qp, int row0, int nrows, uint8_t *out, int cap, int32_t *len, int max_sub, unsigned long long *bins)
{
  EntropyHost e(threads);
  e.set_lanes(lanes);
  std::vector<std::vector<uint8_t>> rows;
  uint64_t b = 0;
  e.code_band(tokens, count, offset, wc, hc, wpp != 0, tile_rows, init_type, qp, row0, nrows, rows, &b);
  if ((int)rows.size() > max_sub) return -1;
  for (size_t k = 0; k < rows.size(); k++) {
    len[k] = (int32_t)rows[k].size();
    if ((int)rows[k].size() > cap) return -1;
    memcpy(out + k * (size_t)cap, rows[k].data(), rows[k].size());
  }
  *bins = b;
  return (int)rows.size();
}

// Microbenchmark: ns per token of the coder on a picture's tokens cut into nsub substreams of equal length, one thread.  lanes = 0:
// cabac_play_tokens_host() substream after substream, else cabac_play_rows_host<lanes>.  Best of `reps`.
double hcr_bench(const uint16_t *tok, long n, int nsub, int reps, int lanes)
{
  std::vector<int32_t> run_len((size_t)nsub), run_first((size_t)nsub + 1);
  for (int k = 0; k <= nsub; k++) run_first[(size_t)k] = k;
  for (int k = 0; k < nsub; k++) run_len[(size_t)k] = (int32_t)(n * (k + 1) / nsub - n * k / nsub);
  std::vector<uint8_t> ctx0((size_t)nsub * CTX_COUNT);
  for (int k = 0; k < nsub; k++) cabac_init_contexts(&ctx0[(size_t)k * CTX_COUNT], 1, 32);
  const int cap = (int)(n / nsub + 1) * 2 + 64;
  std::vector<uint8_t> out((size_t)nsub * cap);
  std::vector<int32_t> len((size_t)nsub); std::vector<uint32_t> bins((size_t)nsub);
  double best = 1e30;
  for (int r = 0; r < reps; r++) {
    auto t0 = std::chrono::steady_clock::now();
    hcr_play(lanes, tok, run_len.data(), run_first.data(), nsub, ctx0.data(), out.data(), cap, len.data(), bins.data());
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    if (ns < best) best = ns;
  }
  return best / (double)n;
}

}  // extern "C"
