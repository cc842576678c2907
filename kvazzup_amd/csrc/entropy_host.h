// kvazzup_amd/csrc/entropy_host.h -- the serial half of entropy coding, on host threads.
//
// Binarisation and context selection -- everything in CABAC that can be done in parallel -- runs
// on the GPU (k_tokenize, enc_kernels.hip) and produces, per CTU, the list of bins in coding
// order as 16-bit tokens.  What is left is the arithmetic coder proper: one state machine per
// WPP substream (CTU row), each bin depending on the previous one.  A GPU lane does that at
// ~80 ns per bin; a host core at ~8 ns.  So the rows of a picture are coded here by a small pool
// of host threads (the reference's encoder does its CABAC on host threads too: Kvazaar's WPP
// worker pool behind kvz_api->encoder_encode, kvazaarfilter.cpp:176-194 "threads"/"wpp").
// Row r starts from the context states row r-1 had after its second CTU (H.265 9.3.2.2).
// Each thread codes several rows at once, interleaved bin by bin (cabac_play_rows_host): one row's chain leaves a core mostly idle.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <utility>
#include <vector>
#include "hevc_core.h"
#include "host_pool.h"

namespace kvzx {

// cabac_play_tokens() of hevc_core.h for the host: the same arithmetic with the coder's registers in locals (the context array is
// written through a byte pointer, which the compiler must assume to alias the coder's own fields: kept in the struct they are
// reloaded after every bin), the context update as one table look-up and the renormalisation shift from the leading-zero count.
struct HostCabacTabs {
  uint8_t next_mps[128], next_lps[128];     // context variable = pStateIdx << 1 | valMps
  uint8_t next[128][2];                     // the same, indexed by [variable][least probable symbol coded]
  uint8_t lps[128][4];                      // rangeTabLps by context variable and (range >> 6) & 3
  HostCabacTabs()
  {
    for (int s = 0; s < 128; s++) {
      const int st = s >> 1, mps = s & 1;
      next_mps[s] = (uint8_t)(((st < 62 ? st + 1 : st) << 1) | mps);
      next_lps[s] = (uint8_t)((kNextLps[st] << 1) | (st == 0 ? mps ^ 1 : mps));
      next[s][0] = next_mps[s]; next[s][1] = next_lps[s];
      for (int q = 0; q < 4; q++) lps[s][q] = kRangeLps[st][q];
    }
  }
};
inline void cabac_play_tokens_host(CabacEnc &c, const HostCabacTabs &T, const uint16_t *tok, int n)
{
  uint32_t low = c.low, range = c.range; int bits_left = c.bits_left;
  uint8_t *const ctx = c.ctx;
  uint32_t nbins = 0;
  auto spill = [&] { c.low = low; c.range = range; c.bits_left = bits_left; };
  auto fill = [&] { low = c.low; range = c.range; bits_left = c.bits_left; };
  for (int i = 0; i < n; i++) {
    const uint32_t t = tok[i];
    if (__builtin_expect(!(t & 0x8000u), 1)) {
      // both outcomes computed and selected (the bin values of sig / greater1 flags are close to coin flips for a branch predictor):
      // either way the new range is renormalised by its leading zeros
      const uint32_t ci = t >> 1, s = ctx[ci];
      const uint32_t lps = T.lps[s][(range >> 6) & 3];
      const uint32_t rmps = range - lps;
      const uint32_t isl = (t ^ s) & 1u;
      const uint32_t r = isl ? lps : rmps;
      const int nb = __builtin_clz(r) - 23;                               // r in [6, 510] -> [256, 510] (an MPS range is at least 128: one bit at most)
      nbins++;
      low = (low + (isl ? rmps : 0u)) << nb; range = r << nb; bits_left -= nb;
      ctx[ci] = T.next[s][isl];
      if (__builtin_expect(bits_left < 12, 0)) { spill(); cabac_write_out(c); fill(); }
    } else {
      spill();
      if (!(t & 0x4000u)) cabac_bypass_bits(c, t & 0x3ffu, (int)((t >> 10) & 15) + 1);
      else cabac_terminate(c, (int)(t & 1));
      fill();
    }
  }
  spill();
  c.nbins += nbins;
}

// The same coder over several substreams at once.  One substream is a chain of bins each waiting on the one before it (range ->
// rangeTabLps row -> subtract -> select -> leading zeros -> shift, and a context store forwarded to the next load of the same
// context): a wide core runs that chain with most of its issue width idle.  The substreams of a picture are independent once their
// starting contexts are known (EntropyHost::prepass_contexts), so K of them are interleaved in one loop, one token from each per
// step.  A lane's registers are locals of the loop; its contexts are a uint16_t copy (a byte store may alias anything, the coder's
// registers included, and would have them reloaded after every store -- with 8-bit contexts the interleaving gains nothing).  A lane
// that finishes its substream takes the next one not yet claimed; when none is left the loop goes on with K - 1 lanes.  The bytes
// and bin counts are those of cabac_play_tokens_host() on each substream alone (tests/test_host_coder_rows.py).
struct HostRun { const uint16_t *tok; int n; };           // the tokens of one CTU
struct HostSub {                                           // one substream for cabac_play_rows_host()
  const HostRun *run; int nrun;                            // its tokens, CTU after CTU
  const uint8_t *ctx0;                                     // contexts it starts from (CTX_COUNT)
  uint8_t *out; int cap;                                   // room for its bytes (two per token and 64 more)
  int len; uint32_t bins;                                  // out: bytes written, bins coded
};
namespace rows_detail {
struct Lane { uint32_t low, range; int bits_left; const uint16_t *p, *e; };     // what the bin loop keeps in registers
struct LaneMem {                                                                 // what it leaves in memory
  CabacEnc c;
  HostSub *s; const HostRun *run, *run_end;
  uint16_t ctx[CTX_COUNT];
};
struct Claim { HostSub *sub; int nsub, next; const CoreTabs *tabs; };
// Starts the next unclaimed substream with a token on the lane; false when none is left.  Substreams without tokens are finished here.
inline bool start_next(Lane &L, LaneMem &M, Claim &q)
{
  for (;;) {
    if (q.next >= q.nsub) return false;
    HostSub &s = q.sub[q.next++];
    M.s = &s; M.run = s.run; M.run_end = s.run + s.nrun;
    cabac_start(M.c, s.out, s.cap, nullptr, q.tabs);
    uint32_t ntok = 0;
    for (int i = 0; i < s.nrun; i++) ntok += (uint32_t)s.run[i].n;
    M.c.nbins = ntok;                     // every regular token is one bin; a bypass / terminate token corrects this by its own count less one
    for (int i = 0; i < CTX_COUNT; i++) M.ctx[i] = s.ctx0[i];
    while (M.run < M.run_end && M.run->n == 0) M.run++;
    if (M.run < M.run_end) { L.low = M.c.low; L.range = M.c.range; L.bits_left = M.c.bits_left; L.p = M.run->tok; L.e = L.p + M.run->n; return true; }
    cabac_finish(M.c); s.len = M.c.pos; s.bins = M.c.nbins;
  }
}
// The lane's current CTU is used up: on to its next CTU, else the substream is finished and the lane takes the next one.
__attribute__((noinline)) inline bool advance(Lane &L, LaneMem &M, Claim &q)
{
  while (++M.run < M.run_end)
    if (M.run->n) { L.p = M.run->tok; L.e = L.p + M.run->n; return true; }
  M.c.low = L.low; M.c.range = L.range; M.c.bits_left = L.bits_left;
  cabac_finish(M.c); M.s->len = M.c.pos; M.s->bins = M.c.nbins;
  return start_next(L, M, q);
}
template <int K> struct Rows {
  static void play(const HostCabacTabs &T, Lane *mem, LaneMem *m, Claim &q)
  {
    Lane l[K];
    for (int j = 0; j < K; j++) l[j] = mem[j];
    int dead = -1;
    // one token of lane j; false: the lane has neither tokens nor a substream left
    auto one = [&](auto J) __attribute__((always_inline)) -> bool {
      constexpr int j = decltype(J)::value;
      if (__builtin_expect(l[j].p == l[j].e, 0)) {
        Lane t = l[j];                                   // (the slow path works on a copy: l itself never has its address taken)
        const bool more = advance(t, m[j], q);
        l[j] = t;
        if (!more) { dead = j; return false; }
      }
      uint32_t low = l[j].low, range = l[j].range; int bits_left = l[j].bits_left;
      const uint32_t t = *l[j].p++;
      if (__builtin_expect(!(t & 0x8000u), 1)) {
        uint16_t *const ctx = m[j].ctx;
        const uint32_t ci = t >> 1, s = ctx[ci];
        const uint32_t lps = T.lps[s][(range >> 6) & 3];
        const uint32_t rmps = range - lps;
        const uint32_t isl = (t ^ s) & 1u;
        const uint32_t r = isl ? lps : rmps;
        const int nb = __builtin_clz(r) - 23;
        low = (low + (isl ? rmps : 0u)) << nb; range = r << nb; bits_left -= nb;
        ctx[ci] = T.next[s][isl];
        if (__builtin_expect(bits_left < 12, 0)) {
          CabacEnc &c = m[j].c;
          c.low = low; c.range = range; c.bits_left = bits_left; cabac_write_out(c); low = c.low; range = c.range; bits_left = c.bits_left;
        }
      } else {
        CabacEnc &c = m[j].c;
        c.low = low; c.range = range; c.bits_left = bits_left; c.nbins--;
        if (!(t & 0x4000u)) cabac_bypass_bits(c, t & 0x3ffu, (int)((t >> 10) & 15) + 1);
        else cabac_terminate(c, (int)(t & 1));
        low = c.low; range = c.range; bits_left = c.bits_left;
      }
      l[j].low = low; l[j].range = range; l[j].bits_left = bits_left;
      return true;
    };
    step(one, std::make_integer_sequence<int, K>{});
    // lane `dead` is done: the last lane moves into its place and the rest goes on with one lane fewer
    for (int j = 0; j < K; j++) mem[j] = l[j];
    if (dead != K - 1) { mem[dead] = mem[K - 1]; std::swap(m[dead], m[K - 1]); }
    Rows<K - 1>::play(T, mem, m, q);
  }
  template <class F, int... J> __attribute__((always_inline)) static void step(F &one, std::integer_sequence<int, J...>)
  {
    while ((one(std::integral_constant<int, J>{}) && ...)) {}
  }
};
template <> struct Rows<0> { static void play(const HostCabacTabs &, Lane *, LaneMem *, Claim &) {} };
}  // namespace rows_detail

template <int K> void cabac_play_rows_host(const HostCabacTabs &T, const CoreTabs *tabs, HostSub *sub, int nsub)
{
  using namespace rows_detail;
  static_assert(K >= 1 && K <= 4, "lanes");
  Lane mem[K]; LaneMem m[K];
  Claim q{sub, nsub, 0, tabs};
  int k = 0;
  while (k < K && start_next(mem[k], m[k], q)) k++;
  switch (k) {                                     // (fewer substreams with tokens than lanes)
    case 0: return;
    case 1: Rows<1>::play(T, mem, m, q); return;
    case 2: Rows<(K < 2 ? K : 2)>::play(T, mem, m, q); return;
    case 3: Rows<(K < 3 ? K : 3)>::play(T, mem, m, q); return;
    default: Rows<K>::play(T, mem, m, q); return;
  }
}

class EntropyHost {
 public:
  explicit EntropyHost(int max_threads) : pool_(max_threads) { for (int i = 0; i < 64; i++) core_tabs_fill_entry(tabs_, i); }
  // Codes one picture.  tokens: dense token array; CTU i has count[i] tokens starting at offset[i].
  // rows_out[r] receives the bytes of substream r (one per CTU row with WPP, else a single one).
  void code_picture(const uint16_t *tokens, const int32_t *count, const uint32_t *offset, int wc, int hc, bool wpp, int tile_rows, int init_type, int qp,
                    std::vector<std::vector<uint8_t>> &rows_out, uint64_t *bins, int tile_cols = 1)
  {
    tokens_ = tokens; count_ = count; offset_ = offset; wc_ = wc; hc_ = hc; wpp_ = wpp; tiles_ = tile_rows < 1 ? 1 : tile_rows; init_type_ = init_type; qp_ = qp;
    cols_ = tile_cols < 1 ? 1 : tile_cols;
    build_geometry();
    const int nsub = (int)geom_.size();
    rows_out.resize((size_t)nsub);
    rows_ = &rows_out;
    saved_.resize((size_t)hc * cols_ * CTX_COUNT);
    bins_.store(0);
    run_rows(nsub, 0);
    if (bins) *bins = bins_.load();
  }
  // The substreams of CTU rows [row0, row0 + nrows) only (whole tiles): rows_out[k] = substream of CTU row row0 + k with WPP,
  // else of the k-th tile of the band.  Arrays are indexed by picture CTU as in code_picture().
  void code_band(const uint16_t *tokens, const int32_t *count, const uint32_t *offset, int wc, int hc, bool wpp, int tile_rows, int init_type, int qp,
                 int row0, int nrows, std::vector<std::vector<uint8_t>> &rows_out, uint64_t *bins)
  {
    tokens_ = tokens; count_ = count; offset_ = offset; wc_ = wc; hc_ = hc; wpp_ = wpp; tiles_ = tile_rows < 1 ? 1 : tile_rows; init_type_ = init_type; qp_ = qp;
    cols_ = 1;                                       // (bands are whole tile rows of full-width tiles)
    build_geometry();
    const int first = wpp ? row0 : tile_row_of(hc, tiles_, row0);
    const int nsub = wpp ? nrows : tile_row_of(hc, tiles_, row0 + nrows - 1) - first + 1;
    all_rows_.resize((size_t)(wpp ? hc : tiles_));
    rows_ = &all_rows_;
    saved_.resize((size_t)hc * CTX_COUNT);
    bins_.store(0);
    run_rows(nsub, first);
    rows_out.resize((size_t)nsub);
    for (int k = 0; k < nsub; k++) rows_out[(size_t)k].swap(all_rows_[(size_t)(first + k)]);
    if (bins) *bins = bins_.load();
  }

 private:
  // A picture with very few tokens (a still scene: all skip) is coded by the calling thread, row after row: handing
  // few-microsecond rows to a pool costs more in wake-ups than the rows take.  Everything else goes to the pool, where row r
  // follows row r - 1 at a distance of two CTUs (a 1080p inter picture of the benchmark clip has some 100 000 tokens, 0.8 ms
  // of coding on one core).
  // WPP: the contexts every CTU row starts from (those of the row above after its second CTU) for ALL rows ahead of the coding, on the
  // calling thread: a context variable follows the bin values alone, not the arithmetic coder's registers, so the hand-over chain is a
  // replay of two CTUs' tokens per row through the state table (~10 us per 1080p picture).  The rows are then coded side by side
  // without ever waiting for each other (before: every row's thread spun until the row above had coded two CTUs -- a quarter of
  // the coder threads' CPU time went into that wait at 6000 frames/s).
  void prepass_contexts(int nsub, int first)
  {
    uint8_t ctx[CTX_COUNT];
    for (int k = 0; k < nsub; k++) {
      const Sub g = geom_[(size_t)(first + k)];
      if (g.cx1 - g.cx0 < 2) continue;                                   // (a one-CTU-wide tile: every row starts from the initial values)
      if (g.cy0 == g.tile_cy0) cabac_init_contexts(ctx, init_type_, qp_);
      else memcpy(ctx, &saved_[((size_t)(g.cy0 - 1) * cols_ + g.tc) * CTX_COUNT], CTX_COUNT);
      for (int cx = g.cx0; cx < g.cx0 + 2; cx++) {
        const size_t ctu = (size_t)g.cy0 * wc_ + cx;
        const uint16_t *tok = tokens_ + offset_[ctu];
        for (int i = 0, n = count_[ctu]; i < n; i++) {
          const uint32_t t = tok[i];
          if (t & 0x8000u) continue;                                     // bypass / terminating bins: no context
          const uint32_t ci = t >> 1, s = ctx[ci];
          ctx[ci] = ((t ^ s) & 1u) ? htabs_.next_lps[s] : htabs_.next_mps[s];
        }
      }
      memcpy(&saved_[((size_t)g.cy0 * cols_ + g.tc) * CTX_COUNT], ctx, CTX_COUNT);
    }
  }
  // Substreams are coded kLanes at a time, interleaved (cabac_play_rows_host): one pool task per kLanes substreams of similar token
  // counts (the longest first: the clip's heavy CTUs sit in a few rows), so that a task's lanes run out at about the same time.
  void run_rows(int nsub, int first)
  {
    if (wpp_) prepass_contexts(nsub, first);
    size_t ntok = 0;
    for (int i = 0; i < wc_ * hc_; i++) ntok += (size_t)count_[i];
    const int K = lanes_;
    if (K == 1 || nsub == 1) {
      if (ntok < 16000) { for (int k = 0; k < nsub; k++) code_row(first + k); }
      else pool_.run(nsub, [this, first](int k) { code_row(first + k); });
      return;
    }
    build_subs(nsub, first);
    if (ntok < 16000) { code_subs(K, 0, nsub); return; }
    const int k = pool_lanes(K, nsub, pool_.threads());
    pool_.run((nsub + k - 1) / k, [this, k, nsub](int t) { code_subs(k, t * k, (t + 1) * k < nsub ? (t + 1) * k : nsub); });
  }
  // Lanes per pool task: fewer, longer tasks save CPU time but lengthen the picture's coding when there are fewer tasks than threads
  // (4 lanes throughout: 1080p's 17 rows in 5 tasks on 8 threads, the coding of a picture took 190 us instead of 115, and the 2160p
  // line, which waits on it, lost 8 %).  Chosen: the lane count, at most max_k, with the shortest wall time in row-times -- rounds of
  // tasks times a task's length, K rows at kStep[K] each (tools/arith_bench.py: 1, 0.67, 0.59, 0.62 of a row coded alone) --
  // the larger one on a tie.
  static int pool_lanes(int max_k, int nsub, int threads)
  {
    static constexpr float kStep[5] = {0.f, 1.f, 0.67f, 0.59f, 0.62f};
    int best = 1; float best_t = 1e30f;
    for (int k = 1; k <= max_k; k++) {
      const int rounds = ((nsub + k - 1) / k + threads - 1) / threads;
      const float t = (float)rounds * (float)k * kStep[k];
      if (t <= best_t) { best = k; best_t = t; }
    }
    return best;
  }
 public:
  // lanes of the interleaved coder: kLanes, or KVAZZUP_AMD_ENTROPY_LANES in [1, 4] (A/B runs; 1 = one substream at a time)
  static constexpr int kLanes = 4;
  static int lanes()
  {
    static const int k = [] { const char *e = getenv("KVAZZUP_AMD_ENTROPY_LANES"); const int v = e ? atoi(e) : kLanes; return v < 1 ? 1 : v > 4 ? 4 : v; }();
    return k;
  }
  void set_lanes(int k) { lanes_ = k < 1 ? 1 : k > 4 ? 4 : k; }      // (tests)
 private:
  // the substreams [first, first + nsub) as runs of tokens with their starting contexts and output room, longest first in order_
  void build_subs(int nsub, int first)
  {
    runs_.clear(); subs_.resize((size_t)nsub); order_.resize((size_t)nsub);
    std::vector<size_t> run0((size_t)nsub + 1);
    std::vector<size_t> ntok((size_t)nsub);
    for (int k = 0; k < nsub; k++) {
      const Sub g = geom_[(size_t)(first + k)];
      run0[(size_t)k] = runs_.size(); ntok[(size_t)k] = 0;
      for (int cy = g.cy0; cy < g.cy1; cy++)
        for (int cx = g.cx0; cx < g.cx1; cx++) {
          const size_t ctu = (size_t)cy * wc_ + cx;
          if (count_[ctu] > 0) { runs_.push_back({tokens_ + offset_[ctu], count_[ctu]}); ntok[(size_t)k] += (size_t)count_[ctu]; }
        }
    }
    run0[(size_t)nsub] = runs_.size();
    cabac_init_contexts(init_ctx_, init_type_, qp_);
    for (int k = 0; k < nsub; k++) {
      const Sub g = geom_[(size_t)(first + k)];
      HostSub &s = subs_[(size_t)k];
      s.run = runs_.data() + run0[(size_t)k]; s.nrun = (int)(run0[(size_t)k + 1] - run0[(size_t)k]);
      // contexts as in code_row()
      const bool fresh = !wpp_ || g.cy0 == g.tile_cy0 || g.cx1 - g.cx0 < 2;
      s.ctx0 = fresh ? init_ctx_ : &saved_[((size_t)(g.cy0 - 1) * cols_ + g.tc) * CTX_COUNT];
      std::vector<uint8_t> &out = (*rows_)[(size_t)(first + k)];
      out.resize(ntok[(size_t)k] * 2 + 64);                  // a token never produces more than two bytes
      s.out = out.data(); s.cap = (int)out.size(); s.len = 0; s.bins = 0;
      order_[(size_t)k] = k;
    }
    std::stable_sort(order_.begin(), order_.end(), [&](int a, int b) { return ntok[(size_t)a] > ntok[(size_t)b]; });
    first_ = first;
  }
  // substreams order_[i0 .. i1) through one interleaved coder
  void code_subs(int K, int i0, int i1)
  {
    HostSub task[64];
    for (int i0b = i0; i0b < i1; i0b += 64) {                // (the serial path hands over all substreams of the picture)
      const int n = i1 - i0b < 64 ? i1 - i0b : 64;
      for (int i = 0; i < n; i++) task[i] = subs_[(size_t)order_[(size_t)(i0b + i)]];
      switch (K) {
        case 2: cabac_play_rows_host<2>(htabs_, &tabs_, task, n); break;
        case 3: cabac_play_rows_host<3>(htabs_, &tabs_, task, n); break;
        default: cabac_play_rows_host<4>(htabs_, &tabs_, task, n); break;
      }
      uint64_t bins = 0;
      for (int i = 0; i < n; i++) {
        const int k = order_[(size_t)(i0b + i)];
        (*rows_)[(size_t)(first_ + k)].resize((size_t)task[i].len);
        bins += task[i].bins;
      }
      bins_.fetch_add(bins);
    }
  }
  // the substreams in decoding order (6.5.1 tile scan: tile after tile; with WPP every CTU row of a tile is one)
  struct Sub { int cy0, cy1, cx0, cx1, tile_cy0, tc; };
  void build_geometry()
  {
    geom_.clear();
    for (int tr = 0; tr < tiles_; tr++)
      for (int tc = 0; tc < cols_; tc++) {
        Sub g; g.tile_cy0 = tile_row_first(hc_, tiles_, tr); g.cx0 = tile_col_first(wc_, cols_, tc); g.cx1 = tile_col_first(wc_, cols_, tc + 1); g.tc = tc;
        const int tile_cy1 = tile_row_first(hc_, tiles_, tr + 1);
        if (wpp_) for (int cy = g.tile_cy0; cy < tile_cy1; cy++) { g.cy0 = cy; g.cy1 = cy + 1; geom_.push_back(g); }
        else { g.cy0 = g.tile_cy0; g.cy1 = tile_cy1; geom_.push_back(g); }
      }
  }
  // substream r of the geometry list: a CTU row of a tile with WPP, else a tile
  void code_row(int r)
  {
    uint8_t ctx[CTX_COUNT];
    std::vector<uint8_t> &out = (*rows_)[(size_t)r];
    const Sub g = geom_[(size_t)r];
    size_t ntok = 0;
    for (int cy = g.cy0; cy < g.cy1; cy++) for (int cx = g.cx0; cx < g.cx1; cx++) ntok += (size_t)count_[(size_t)cy * wc_ + cx];
    out.resize(ntok * 2 + 64);                    // a token never produces more than two bytes
    CabacEnc c; c.nbins = 0;
    cabac_start(c, out.data(), (int)out.size(), ctx, &tabs_);
    // contexts: initialised at the first CTU of a tile (9.3.1), else (WPP) inherited from the row above inside the tile after its second
    // CTU -- when the tile is at least two CTUs wide
    const bool fresh = !wpp_ || g.cy0 == g.tile_cy0 || g.cx1 - g.cx0 < 2;
    if (fresh) cabac_init_contexts(ctx, init_type_, qp_);
    else {
      const size_t above = (size_t)(g.cy0 - 1) * cols_ + g.tc;                 // (prepass_contexts)
      memcpy(ctx, &saved_[above * CTX_COUNT], CTX_COUNT);
    }
    for (int cy = g.cy0; cy < g.cy1; cy++)
      for (int cx = g.cx0; cx < g.cx1; cx++) {
        const size_t ctu = (size_t)cy * wc_ + cx;
        cabac_play_tokens_host(c, htabs_, tokens_ + offset_[ctu], count_[ctu]);
      }
    cabac_finish(c);
    out.resize((size_t)c.pos);
    bins_.fetch_add(c.nbins);
  }

  OrderedPool pool_;
  CoreTabs tabs_;
  HostCabacTabs htabs_;
  const uint16_t *tokens_ = nullptr; const int32_t *count_ = nullptr; const uint32_t *offset_ = nullptr;
  int wc_ = 0, hc_ = 0, tiles_ = 1, cols_ = 1, init_type_ = 0, qp_ = 0; bool wpp_ = true;
  std::vector<Sub> geom_;
  std::vector<HostRun> runs_; std::vector<HostSub> subs_; std::vector<int> order_; int first_ = 0;     // (build_subs)
  uint8_t init_ctx_[CTX_COUNT];
  int lanes_ = lanes();
  std::vector<uint8_t> saved_;
  std::vector<std::vector<uint8_t>> *rows_ = nullptr;
  std::vector<std::vector<uint8_t>> all_rows_;
  std::atomic<uint64_t> bins_{0};
};

}  // namespace kvzx
