// kvazzup_amd/csrc/dec_parse.hip -- see decoder.h.  The decoder's slice-data parser (H.265 7.3.8, 9.3): the CABAC arithmetic decoder, SAO and residual
// syntax, the coding quadtree with merge / AMVP derivation (SliceParser), and the two Decoder members that drive it -- parse_substream (one CTU row or tile)
// and parse_job (a picture's substreams, then its input block).  ONE translation unit on purpose: every hot function keeps the inlining context it was tuned in.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "decoder.h"

namespace kvzx {

enum { PART_2Nx2N = 0, PART_2NxN, PART_Nx2N, PART_NxN, PART_2NxnU, PART_2NxnD, PART_nLx2N, PART_nRx2N };

namespace {

// ------------------------------------------------------------------------------------------ CABAC decoding (H.265 9.3.4.3)
// Arithmetic decoder with the offset kept scaled in a 64-bit register: value = offset << bits | next
// `bits` stream bits, so a renormalisation by n is just bits -= n and the stream is touched 32 bits at
// a time.  Context variable = pStateIdx << 1 | valMps with precomputed transitions.
// next[variable][LPS decoded], lps[variable][(range >> 6) & 3]; lpsn[variable][q] = the LPS range already renormalised (bits 0..8) | its shift << 16: an LPS
// range's renormalisation depends on the table entry alone, so it is looked up with it instead of counted (a leading-zero count, a subtraction and a shift
// less on the range's dependency chain); an MPS range (>= 128) is shifted by one at most
struct StateTabs { uint8_t next_mps[128], next_lps[128]; uint8_t next[128][2]; uint8_t lps[128][4]; uint32_t lpsn[128][4]; };
const StateTabs &state_tabs()               // (function-local statics: initialised once, thread-safe -- parse workers race to the first call)
{
  static const StateTabs t = [] {
    StateTabs t;
    for (int s = 0; s < 128; s++) {
      int st = s >> 1, mps = s & 1;
      t.next_mps[s] = (uint8_t)(((st < 62 ? st + 1 : st) << 1) | mps);
      t.next_lps[s] = (uint8_t)((kNextLps[st] << 1) | (st == 0 ? mps ^ 1 : mps));
      t.next[s][0] = t.next_mps[s]; t.next[s][1] = t.next_lps[s];
      for (int q = 0; q < 4; q++) { t.lps[s][q] = kRangeLps[st][q]; const int n = __builtin_clz((uint32_t)kRangeLps[st][q]) - 23; t.lpsn[s][q] = ((uint32_t)kRangeLps[st][q] << n) | ((uint32_t)n << 16) | ((uint32_t)kRangeLps[st][q] << 24); }
    }
    return t;
  }();
  return t;
}
// The decoder's registers apart from the context variables: a function that decodes many bins in a row (parse_residual) works on a LOCAL copy -- a local
// whose address never leaves the function lives in registers, while the members of an object reached through a reference are re-loaded and written back
// around every context store (measured on the parser alone, tools/measure/parse_rate.py: 11.3 -> see HISTORY.md ns per bin at 1080p / QP 32).
struct CabacRegs {
  const uint8_t *p = nullptr, *end = nullptr;                   // next unread byte, end of the substream; reads past `end` deliver zeros (a malformed NAL cannot walk off the buffer)
  uint64_t value = 0; int bits = 0;
  uint32_t range = 510; uint32_t past = 0;                      // 32-bit words fetched beyond the end
  const StateTabs *st = nullptr;
  uint16_t *ctx = nullptr;                                      // 16-bit entries: a byte store may alias anything; a uint16_t store cannot alias the fields above
  // (every member function is forced inline: one call with `this` would pin a local copy to the stack)
  static __attribute__((noinline)) uint32_t word_tail(const uint8_t *p, const uint8_t *end) { uint32_t w = 0; for (int i = 0; i < 4; i++) w = (w << 8) | (p + i < end ? p[i] : 0u); return w; }
  __attribute__((always_inline)) inline uint32_t word()
  {
    uint32_t w;
    if (__builtin_expect(p + 4 <= end, 1)) { memcpy(&w, p, 4); w = __builtin_bswap32(w); }
    else { w = word_tail(p, end); past++; }
    p += 4;
    return w;
  }
  __attribute__((always_inline)) inline void refill() { if (__builtin_expect(bits < 16, 0)) { value = (value << 32) | word(); bits += 32; } }
  bool overrun() const { return past > 3; }
  __attribute__((always_inline)) inline int bin(int ci)
  {
    // (both outcomes are computed and selected: the bin values of sig / greater1 flags are close to coin flips for a branch predictor)
    const uint32_t s = ctx[ci];
    const uint32_t e = st->lpsn[s][(range >> 6) & 3];     // LPS range: as it is (bits 24..31), renormalised (bits 0..8), its shift (bits 16..19)
    const uint32_t rmps = range - (e >> 24);
    const uint64_t scaled = (uint64_t)rmps << bits;
    const bool isl = value >= scaled;
    value -= isl ? scaled : 0;
    const uint32_t nm = (rmps >> 8) ^ 1u;                 // an MPS range is in [128, 510]: one shift when below 256
    range = isl ? (e & 0x1ffu) : (rmps << nm);
    bits -= (int)(isl ? ((e >> 16) & 15u) : nm);
    ctx[ci] = st->next[s][isl];
    refill();
    return (int)((s & 1u) ^ (uint32_t)isl);
  }
  __attribute__((always_inline)) inline int bypass()
  {
    bits--;
    const uint64_t scaled = (uint64_t)range << bits;
    int b = 0;
    if (value >= scaled) { value -= scaled; b = 1; }
    refill();
    return b;
  }
  // n bypass bins at once: they are the n-bit quotient of value by range << (bits - n) (binary long division, one step per
  // bin); refill() keeps bits >= 16, so up to 16 bins go in one division
  __attribute__((always_inline)) inline uint32_t bypass_bits(int n)
  {
    uint32_t v = 0;
    while (n > 0) {
      const int m = n > 16 ? 16 : n;
      if (m <= 2) { for (int i = 0; i < m; i++) v = (v << 1) | (uint32_t)bypass(); }
      else {
        bits -= m;
        const uint64_t scaled = (uint64_t)range << bits;
        const uint64_t q = value / scaled;
        value -= q * scaled;
        v = (v << m) | (uint32_t)(q & 0xffffu);
        refill();
      }
      n -= m;
    }
    return v;
  }
  __attribute__((always_inline)) inline int terminate()
  {
    range -= 2;
    if (value >= ((uint64_t)range << bits)) return 1;
    if (range < 256) { range <<= 1; bits--; }
    refill();
    return 0;
  }
};
struct CabacDec : CabacRegs {
  const uint8_t *buf = nullptr;                                 // the substream
  uint16_t ctx_store[CTX_COUNT];
  CabacDec() { ctx = ctx_store; }
  CabacDec(const CabacDec &) = delete;
  void load_ctx(const uint8_t *src) { for (int i = 0; i < CTX_COUNT; i++) ctx_store[i] = src[i]; }
  void save_ctx(uint8_t *dst) const { for (int i = 0; i < CTX_COUNT; i++) dst[i] = (uint8_t)ctx_store[i]; }
  void start(const uint8_t *b, size_t l)
  {
    buf = b; p = b; end = b + l; past = 0; st = &state_tabs(); range = 510; ctx = ctx_store;
    value = word(); bits = 32 - 9;
    refill();
  }
  // bytes from the start of the substream up to and including the byte holding the last consumed bit (after a terminating bin == 1:
  // 9.3.2.5 reads rbsp_trailing / alignment, i.e. the arithmetic codeword ends at the byte boundary after the 7 bits it consumed last)
  size_t bytes_consumed() const { const size_t consumed_bits = (size_t)(p - buf) * 8 - (size_t)bits; return (consumed_bits + 7) >> 3; }
};

std::atomic<long> g_yields{0};

// sao() of one CTU (7.3.8.3); `left` / `up`: the neighbours that may be merged from
void parse_sao(CabacDec &c, SaoParams &p, const SaoParams *left, const SaoParams *up, bool luma, bool chroma)
{
  memset(&p, 0, sizeof(p));
  if (left && c.bin(CTX_SAO_MERGE)) { p = *left; return; }
  if (up && c.bin(CTX_SAO_MERGE)) { p = *up; return; }
  for (int ci = 0; ci < 3; ci++) {
    if (!(ci ? chroma : luma)) continue;
    if (ci < 2) p.type[ci] = (uint8_t)(c.bin(CTX_SAO_TYPE) ? (c.bypass() ? 2 : 1) : 0);
    else { p.type[2] = p.type[1]; p.eo_class[2] = p.eo_class[1]; }
    if (!p.type[ci]) continue;
    int a[4];
    for (int i = 0; i < 4; i++) { a[i] = 0; while (a[i] < 7 && c.bypass()) a[i]++; }
    if (p.type[ci] == 1) {
      for (int i = 0; i < 4; i++) if (a[i] && c.bypass()) a[i] = -a[i];
      p.band_pos[ci] = (uint8_t)c.bypass_bits(5);
    } else {
      if (ci < 2) p.eo_class[ci] = (uint8_t)c.bypass_bits(2);
      a[2] = -a[2]; a[3] = -a[3];                                  // edge offsets: categories 1, 2 positive, 3, 4 negative
    }
    for (int i = 0; i < 4; i++) p.offset[ci][i] = (int8_t)a[i];
  }
}

// residual_coding() (7.3.8.11): appends (raster position << 16 | level) words; *tskip receives transform_skip_flag
// The two loops that decode most of a picture's bins, as functions of their own: inside parse_residual the compiler has no registers left for the decoder's
// (x86-64: sixteen for a function with thirty live values) and keeps them on the stack -- a store and a load on every bin's dependency chain; here they are
// the only live state.
__attribute__((noinline)) uint32_t sig_flag_run(CabacRegs &cr, const uint8_t *pk, int base, int k0)       // sig_coeff_flag of scan positions k0 .. 1
{
  CabacRegs c = cr;
  uint32_t sig = 0;
  for (int k = k0; k >= 1; k--) sig |= (uint32_t)c.bin(base + pk[k]) << k;
  cr.p = c.p; cr.value = c.value; cr.bits = c.bits; cr.range = c.range; cr.past = c.past;
  return sig;
}
// coeff_abs_level_greater1_flag of the first (up to eight) coefficients of a sub-block: bit j of the result = flag of coefficient j; *c1_io: greater1Ctx
__attribute__((noinline)) uint32_t greater1_run(CabacRegs &cr, int ctx_base, int n, int *c1_io)
{
  CabacRegs c = cr;
  uint32_t g = 0; int c1 = *c1_io;
  for (int j = 0; j < n; j++) {
    const int g1 = c.bin(ctx_base + c1);
    g |= (uint32_t)g1 << j;
    if (g1) c1 = 0; else if (c1 > 0 && c1 < 3) c1++;
  }
  *c1_io = c1;
  cr.p = c.p; cr.value = c.value; cr.bits = c.bits; cr.range = c.range; cr.past = c.past;
  return g;
}

__attribute__((always_inline)) inline bool parse_residual_regs(CabacRegs &c, int log2, int cidx, int scan_idx, bool sign_hiding, bool ts_enabled, int *tskip, std::vector<uint32_t> &out)
{
  const ScanTabs &S = scan_tabs();
  const int n = 1 << log2, sbl = log2 - 2, nsb = 1 << sbl;
  const uint8_t *SX = S.x[scan_idx][sbl], *SY = S.y[scan_idx][sbl], *PX = S.x[scan_idx][2], *PY = S.y[scan_idx][2];
  uint8_t csbf[8][8]; memset(csbf, 0, sizeof(csbf));
  *tskip = (ts_enabled && log2 == 2) ? c.bin(CTX_TS_FLAG + (cidx ? 1 : 0)) : 0;
  int pre[2];
  for (int d = 0; d < 2; d++) {
    int off, sh, mx = (log2 << 1) - 1, v = 0;
    if (cidx == 0) { off = 3 * (log2 - 2) + ((log2 - 1) >> 2); sh = (log2 + 1) >> 2; } else { off = 15; sh = log2 - 2; }
    while (v < mx && c.bin((d ? CTX_LAST_Y : CTX_LAST_X) + off + (v >> sh))) v++;
    pre[d] = v;
  }
  int lx = pre[0], ly = pre[1];
  if (lx > 3) { int nb = (lx >> 1) - 1; lx = (1 << nb) * (2 + (lx & 1)) + (int)c.bypass_bits(nb); }
  if (ly > 3) { int nb = (ly >> 1) - 1; ly = (1 << nb) * (2 + (ly & 1)) + (int)c.bypass_bits(nb); }
  if (scan_idx == 2) { int tt = lx; lx = ly; ly = tt; }
  if (lx >= n || ly >= n) return false;
  // the last significant coefficient as (sub-block, position inside it) in scan order: inverse scan tables
  const int last_sb = S.inv[scan_idx][sbl][((ly >> 2) << sbl) | (lx >> 2)], last_pos = S.inv[scan_idx][2][((ly & 3) << 2) | (lx & 3)];
  int c1 = 1;
  for (int i = last_sb; i >= 0; i--) {
    const int xs = SX[i], ys = SY[i];
    int right = (xs < nsb - 1) ? csbf[ys][xs + 1] : 0, below = (ys < nsb - 1) ? csbf[ys + 1][xs] : 0, infer_dc = 0;
    if (i < last_sb && i > 0) { csbf[ys][xs] = (uint8_t)c.bin(CTX_CSBF + ((right | below) ? 1 : 0) + (cidx ? 2 : 0)); infer_dc = 1; }
    else csbf[ys][xs] = 1;
    if (!csbf[ys][xs]) continue;
    uint32_t sig = 0;
    if (i == last_sb) sig |= 1u << last_pos;
    const int prev_csbf = right | (below << 1);
    // sig_coeff_flag contexts (9.3.4.2.5) from tables: pattern by the neighbouring sub-blocks' flags and the position inside
    // the sub-block, plus an offset that is constant over the sub-block
    const uint8_t *pk = S.sigk[scan_idx][log2 == 2 ? 4 : prev_csbf];
    const int sig_base = CTX_SIG + (cidx ? 27 : 0);
    const int sig_off = log2 == 2 ? 0 : (cidx == 0 ? ((i > 0 ? 3 : 0) + ((log2 == 3) ? ((scan_idx == 0) ? 9 : 15) : 21)) : ((log2 == 3) ? 9 : 12));
    {
      const int k0 = (i == last_sb) ? last_pos - 1 : 15;
      const int base = sig_base + sig_off;
      if (k0 >= 1) sig |= sig_flag_run(c, pk, base, k0);      // (position 0 apart: no per-flag conditions in that loop)
      if (k0 >= 0) {
        if (infer_dc && !(sig >> 1)) sig |= 1u;            // every other flag of a coded sub-block zero: inferred
        else sig |= (uint32_t)c.bin((i == 0 && log2 != 2) ? sig_base : base + pk[0]);      // (the DC coefficient of the block has its own context)
      }
    }
    if (!sig) continue;
    int ctx_set = (i > 0 && cidx == 0) ? 2 : 0;
    if (c1 == 0) ctx_set++;
    c1 = 1;
    int pos[16], lev[16], nsig = 0, g1idx = -1;
    for (uint32_t m = sig; m;) { const int k = 31 - __builtin_clz(m); pos[nsig++] = k; m &= ~(1u << k); }     // highest scan position first
    for (int j = 0; j < nsig; j++) lev[j] = 1;
    {
      const uint32_t g = greater1_run(c, CTX_GT1 + (cidx ? 16 : 0) + ctx_set * 4, nsig < 8 ? nsig : 8, &c1);
      if (g) { g1idx = __builtin_ctz(g); for (uint32_t m = g; m; m &= m - 1) lev[__builtin_ctz(m)] = 2; }
    }
    if (g1idx >= 0 && c.bin(CTX_GT2 + (cidx ? 4 : 0) + ctx_set)) lev[g1idx] = 3;
    // sign_data_hiding (7.3.8.11, 9.3.4.3): the sign of the sub-block's first coefficient in scan order is not sent when its
    // first and last significant positions are more than three apart; it follows from the parity of the sum of the levels
    const bool hidden = sign_hiding && (pos[0] - pos[nsig - 1] > 3);
    const int nsigns = hidden ? nsig - 1 : nsig;
    uint32_t signs = c.bypass_bits(nsigns) << (nsig - nsigns);
    int rice = 0, sum = 0;
    for (int j = 0; j < nsig; j++) {
      int base = (j < 8) ? ((j == g1idx) ? 3 : 2) : 1;
      if (lev[j] == base) {
        int prefix = 0;
        while (prefix < 32 && c.bypass()) prefix++;
        if (prefix - 3 + rice > 16) return false;              // (9.3.3.11: an 8-bit stream's escape suffix has at most 16 bits; anything longer is not a level, and the shifts below must not see it)
        int rem = prefix <= 3 ? (prefix << rice) + (int)c.bypass_bits(rice)
                              : (((1 << (prefix - 3)) + 3 - 1) << rice) + (int)c.bypass_bits(prefix - 3 + rice);
        lev[j] = base + rem;
        if (lev[j] > 3 * (1 << rice)) rice = imin(rice + 1, 4);
      }
      sum += lev[j];
    }
    if (hidden && (sum & 1)) signs |= 1u;
    const size_t o0 = out.size();
    out.resize(o0 + (size_t)nsig);                       // (one capacity check per sub-block instead of one per level)
    uint32_t *dst = out.data() + o0;
    for (int j = 0; j < nsig; j++) {
      const int v = ((signs >> (nsig - 1 - j)) & 1) ? -lev[j] : lev[j];
      const int xp = PX[pos[j]], yp = PY[pos[j]];
      dst[j] = (uint32_t)((((ys << 2) + yp) * n + (xs << 2) + xp) << 16) | ((uint32_t)clip3(-32768, 32767, v) & 0xffffu);
    }
    if (c.overrun()) return false;
  }
  return !c.overrun();
}

bool parse_residual(CabacDec &cd, int log2, int cidx, int scan_idx, bool sign_hiding, bool ts_enabled, int *tskip, std::vector<uint32_t> &out)
{
  CabacRegs c = cd;                                        // the decoder's registers in locals for the whole block (CabacRegs)
  const bool ok = parse_residual_regs(c, log2, cidx, scan_idx, sign_hiding, ts_enabled, tskip, out);
  static_cast<CabacRegs &>(cd) = c;
  return ok;
}

// ------------------------------------------------------------------------------------------ slice data (7.3.8) of one substream
struct MvCand { int mvx, mvy, ref_idx; };

struct SliceParser {
  Decoder::PicJob &job; Decoder::SubOut &out;
  const DecSps &sps; const DecPps &pps; const SliceHdr &sh;
  CabacDec c;
  const int w, h, b4w, b8w, ctbl, mincb, wc, hc;      // ctbl: CtbLog2SizeY; mincb: MinCbLog2SizeY (3, 4 or 5); wc, hc: the picture in coding tree blocks
  B4Rec *b4; uint8_t *pm, *ctd, *im;     // pm, ctd: per 8x8 (the minimum coding block); im: per 4x4 (NxN parts)
  int ref_y0 = -(1 << 30), ref_y1 = 1 << 30;                              // band mode: the luma rows of a reference picture this decoder holds (the picture's outer edges open)
  int tile_y0 = 0, tile_y1 = 1 << 30, tile_x0 = 0, tile_x1 = 1 << 30;    // luma rows / columns of the tile being parsed: nothing outside is available (other tiles may be parsed concurrently)
  const uint8_t *slice_of = nullptr; int cur_slice = 0;                  // pictures of several slices inside a tile (PicJob::ctb_slice): the slice of every coding tree block, the one being parsed
  int slice_qp = 26;                                                      // SliceQpY of the slice being parsed
  int err = 0;
  // quantisation (8.6.1)
  int qp_y = 0, qp_y_pred = 0, last_qp_y = 0, cu_qp_delta_val = 0, log2_qg = 6; bool qp_delta_coded = false;
  // coding unit being parsed
  int cu_pred_mode = 0, part_mode = 0, max_trafo_depth = 0, intra_modes[4] = {0, 0, 0, 0}, chroma_mode = 0; bool intra_split = false;
  uint32_t ctu_intra_mask = 0;

  SliceParser(Decoder::PicJob &j, Decoder::SubOut &o, int pw)
      : job(j), out(o), sps(*j.sps), pps(j.pps), sh(j.sh), w(j.sps->width), h(j.sps->height), b4w(pw / 4), b8w(pw / 8), ctbl(j.sps->ctb_log2), mincb(j.sps->min_cb_log2), wc(j.sps->wc()),
        hc(j.sps->hc()), b4(j.b4), pm(j.pred_mode.data()), ctd(j.ct_depth.data()), im(j.intra_mode.data())
  { log2_qg = ctbl - pps.qp_delta_depth; }

  inline int bi(int x, int y) const { return (y >> 2) * b4w + (x >> 2); }
  inline int b8(int x, int y) const { return (y >> 3) * b8w + (x >> 3); }
  // 6.4.1: inside the picture, inside the tile, in the same slice (slice_of: pictures with several slices inside a tile), already decoded.  "Already
  // decoded" is read off the prediction-mode array, which starts every picture as PM_NONE: in decoding order a block is marked
  // when its coding unit starts, and the WPP row hand-over (two CTUs behind the row above, parse_substream) guarantees that every
  // neighbour that precedes the current block in z-scan order has been parsed while none that follows it has been.
  inline bool avail(int, int, int xn, int yn) const
  {
    return xn >= tile_x0 && yn >= tile_y0 && xn < w && yn < h && yn < tile_y1 && xn < tile_x1 && pm[b8(xn, yn)] != PM_NONE && (!slice_of || slice_of[(yn >> ctbl) * wc + (xn >> ctbl)] == cur_slice);
  }
  // coding-unit wide values of the per-8x8 arrays
  void fill_cu8(uint8_t *arr, int x0, int y0, int n, int v)
  {
    const int cols = imin(n, w - x0) >> 3;
    for (int y = y0; y < y0 + n && y < h; y += 8) memset(arr + b8(x0, y), v, (size_t)cols);
  }
  void fill_u8(uint8_t *arr, int x0, int y0, int bw, int bh, int v)       // per-4x4 array
  {
    const int cols = imin(bw, w - x0) >> 2;
    for (int y = y0; y < y0 + bh && y < h; y += 4) memset(arr + bi(x0, y), v, (size_t)cols);
  }
  // one record for every 4x4 unit of a rectangle
  // cu_edges: the rectangle is a whole coding block -- its top row and left column get the coding block's edge flags in the same pass (a
  // read-modify-write of the column afterwards waits for every one of the stores just issued: it was the hottest line of the parser)
  bool cu_edges_done = false;
  int cu_bypass = 0;                                       // cu_transquant_bypass_flag of the coding unit being parsed
  void fill_recs(int x0, int y0, int bw, int bh, const B4Rec &r, bool cu_edges = false)
  {
    uint64_t v; memcpy(&v, &r, 8);
    const int cols = imin(bw, w - x0) >> 2;
    if (!cu_edges) { for (int y = y0; y < y0 + bh && y < h; y += 4) { uint64_t *p = (uint64_t *)&b4[bi(x0, y)]; for (int i = 0; i < cols; i++) p[i] = v; } return; }
    B4Rec e = r;
    e.flags |= B4_EDGE_V | B4_TU_V; uint64_t vl; memcpy(&vl, &e, 8);                    // first column
    e.flags = r.flags | B4_EDGE_H | B4_TU_H; uint64_t vt; memcpy(&vt, &e, 8);           // first row
    e.flags |= B4_EDGE_V | B4_TU_V; uint64_t vc; memcpy(&vc, &e, 8);                    // the corner
    for (int y = y0; y < y0 + bh && y < h; y += 4) {
      uint64_t *p = (uint64_t *)&b4[bi(x0, y)];
      const bool top = y == y0;
      if (cols > 0) p[0] = top ? vc : vl;
      for (int i = 1; i < cols; i++) p[i] = top ? vt : v;
    }
    cu_edges_done = true;
  }
  void emit_tu(const DecTu &td)
  {
    const int X = td.plane ? td.x * 2 : td.x, Y = td.plane ? td.y * 2 : td.y;
    if (ctbl == 6) {                                                 // (smaller CTBs: a region spans substreams that are parsed side by side, and parse_job builds region[] from the finished list anyway)
      TuRange &r = job.region[(Y >> 5) * (b4w >> 3) + (X >> 5)];      // (32x32 regions of the padded picture)
      if (!r.count) r.first = (uint32_t)out.tus.size();
      r.count++;
    }
    out.tus.push_back(td);
  }

  // ---------------------------------------------------------------- motion vector prediction (8.5.3.2)
  bool pb_avail(int xcb, int ycb, int ncbs, int xpb, int ypb, int npbw, int npbh, int part_idx, int xn, int yn) const
  {
    const bool same_cb = xcb <= xn && ycb <= yn && xcb + ncbs > xn && ycb + ncbs > yn;
    bool a;
    if (!same_cb) a = avail(xpb, ypb, xn, yn);
    else a = !((npbw << 1) == ncbs && (npbh << 1) == ncbs && part_idx == 1 && (ycb + npbh <= yn) && (xcb + npbw > xn));
    if (a && pm[b8(xn, yn)] == PM_INTRA) a = false;
    return a;
  }
  static bool same_motion(const B4Rec &a, const B4Rec &b) { return a.ref_idx == b.ref_idx && a.mvx == b.mvx && a.mvy == b.mvy; }

  // temporal candidate of list X (8.5.3.2.8, 8.5.3.2.9).  The collocated block may be bi-predicted (a B picture): of its two vectors the one of list X
  // counts when no reference picture of this slice follows it in output order, else the one of list collocated_from_l0_flag.
  inline int list_poc(int L, int idx) const { return L ? job.ref_poc1[idx & 15] : job.ref_poc[idx & 15]; }
  inline bool list_lt(int L, int idx) const { return (L ? job.ref_lt1[idx & 15] : job.ref_lt[idx & 15]) != 0; }      // the entry is a long-term reference picture
  static void scale_by(int &mvx, int &mvy, int td_, int tb_)
  {
    const int td = clip3(-128, 127, td_), tb = clip3(-128, 127, tb_);
    if (td == 0) return;
    const int tx = (16384 + (iabs(td) >> 1)) / td, dsf = clip3(-4096, 4095, (tb * tx + 32) >> 6);
    const int px = dsf * mvx, py = dsf * mvy;
    mvx = clip3(-32768, 32767, (px < 0 ? -1 : 1) * ((iabs(px) + 127) >> 8));
    mvy = clip3(-32768, 32767, (py < 0 ? -1 : 1) * ((iabs(py) + 127) >> 8));
  }
  bool temporal_mv(int xpb, int ypb, int npbw, int npbh, int X, int ref_idx, int &mvx, int &mvy)
  {
    ColMotion *col = job.col.get();
    if (!col) return false;
    const int cy = ypb >> ctbl;
    if (cy < col->hc) {                                  // the collocated picture may still be in the hands of its own parser (frame threads)
      std::atomic<uint8_t> &d = col->row_done[(size_t)cy];
      int spins = 0;
      while (!d.load(std::memory_order_acquire)) { if (++spins < 2000) __builtin_ia32_pause(); else std::this_thread::yield(); }
    }
    const int cand[2][2] = {{xpb + npbw, ypb + npbh}, {xpb + (npbw >> 1), ypb + (npbh >> 1)}};
    for (int k = 0; k < 2; k++) {
      int x = cand[k][0], y = cand[k][1];
      if (k == 0 && !((ypb >> ctbl) == (y >> ctbl) && y < h && x < w)) continue;      // bottom right: same CTB row, inside the picture
      x >>= 4; y >>= 4;
      if (x >= col->w16 || y >= col->h16) continue;
      const ColMotion::Mv &m = col->mv[(size_t)y * col->w16 + x];
      if (!m.used) continue;
      const int L = m.used == 2 ? 1 : (m.used == 1 ? 0 : (job.no_backward ? X : sh.collocated_from_l0));
      const bool cur_lt = list_lt(X, ref_idx);
      if ((((m.lt >> L) & 1) != 0) != cur_lt) continue;      // 8.5.3.2.9: one of the two reference pictures long-term, the other not: no candidate from this block
      const int col_diff = col->poc - m.ref_poc[L], cur_diff = sh.poc - list_poc(X, ref_idx);
      mvx = m.mv[L][0]; mvy = m.mv[L][1];
      if (!cur_lt && col_diff != cur_diff && col_diff != 0) scale_by(mvx, mvy, col_diff, cur_diff);      // (long-term: taken as it is)
      return true;
    }
    return false;
  }

  // `want`: the index the bitstream chose -- only cand[want] is read afterwards (merge_idx 0 with the left neighbour there, the common case of a
  // skipped CU, needs one look-up instead of five and the pruning)
  void merge_candidates(int xcb, int ycb, int ncbs, int xpb, int ypb, int npbw, int npbh, int part_idx, int pmode, MvCand *cand, int want)
  {
    const int lvl = pps.par_mrg_level;
    int n = 0;
    if (lvl > 2 && ncbs == 8) { xpb = xcb; ypb = ycb; npbw = npbh = ncbs; part_idx = 0; pmode = PART_2Nx2N; }
    auto par = [&](int xn, int yn) { return ((xpb >> lvl) == (xn >> lvl)) && ((ypb >> lvl) == (yn >> lvl)); };
    const int xa1 = xpb - 1, ya1 = ypb + npbh - 1, xb1 = xpb + npbw - 1, yb1 = ypb - 1, xb0 = xpb + npbw, yb0 = ypb - 1;
    const int xa0 = xpb - 1, ya0 = ypb + npbh, xb2 = xpb - 1, yb2 = ypb - 1;
    const bool part1 = part_idx == 1;
    const bool nbA1 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xa1, ya1) && !par(xa1, ya1) &&
                      !(part1 && (pmode == PART_Nx2N || pmode == PART_nLx2N || pmode == PART_nRx2N));
    if (want == 0 && nbA1) { const B4Rec &m = b4[bi(xa1, ya1)]; cand[0].mvx = m.mvx; cand[0].mvy = m.mvy; cand[0].ref_idx = m.ref_idx; return; }
    const bool nbB1 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xb1, yb1) && !par(xb1, yb1) &&
                      !(part1 && (pmode == PART_2NxN || pmode == PART_2NxnU || pmode == PART_2NxnD));
    const bool nbB0 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xb0, yb0) && !par(xb0, yb0);
    const bool nbA0 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xa0, ya0) && !par(xa0, ya0);
    const bool nbB2 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xb2, yb2) && !par(xb2, yb2);
    const B4Rec zero = B4Rec();
    const B4Rec &A1 = nbA1 ? b4[bi(xa1, ya1)] : zero, &B1 = nbB1 ? b4[bi(xb1, yb1)] : zero, &B0 = nbB0 ? b4[bi(xb0, yb0)] : zero;
    const B4Rec &A0 = nbA0 ? b4[bi(xa0, ya0)] : zero, &B2 = nbB2 ? b4[bi(xb2, yb2)] : zero;
    const bool avA1 = nbA1, avB1 = nbB1 && !(nbA1 && same_motion(A1, B1)), avB0 = nbB0 && !(nbB1 && same_motion(B1, B0));
    const bool avA0 = nbA0 && !(nbA1 && same_motion(A1, A0));
    const bool avB2 = nbB2 && !(nbA1 && same_motion(A1, B2)) && !(nbB1 && same_motion(B1, B2)) && ((int)avA0 + avA1 + avB0 + avB1 != 4);
    const int maxc = sh.max_merge;
    auto add = [&](const B4Rec &m) { if (n < maxc) { cand[n].mvx = m.mvx; cand[n].mvy = m.mvy; cand[n].ref_idx = m.ref_idx; n++; } };
    if (avA1) add(A1);
    if (avB1) add(B1);
    if (avB0) add(B0);
    if (avA0) add(A0);
    if (avB2) add(B2);
    if (n < maxc) { int tx, ty; if (temporal_mv(xpb, ypb, npbw, npbh, 0, 0, tx, ty)) { cand[n].mvx = tx; cand[n].mvy = ty; cand[n].ref_idx = 0; n++; } }
    for (int zi = 0; n < maxc; n++, zi++) { cand[n].mvx = cand[n].mvy = 0; cand[n].ref_idx = zi < sh.num_ref_idx ? zi : 0; }     // 8.5.3.2.5, P slices
  }

  void scale_mv(int &mvx, int &mvy, int ref_a, int ref_target) const
  {
    const int td = clip3(-128, 127, sh.poc - job.ref_poc[ref_a]), tb = clip3(-128, 127, sh.poc - job.ref_poc[ref_target]);
    if (td == 0) return;
    const int tx = (16384 + (iabs(td) >> 1)) / td, dsf = clip3(-4096, 4095, (tb * tx + 32) >> 6);
    const int px = dsf * mvx, py = dsf * mvy;
    mvx = clip3(-32768, 32767, (px < 0 ? -1 : 1) * ((iabs(px) + 127) >> 8));
    mvy = clip3(-32768, 32767, (py < 0 ? -1 : 1) * ((iabs(py) + 127) >> 8));
  }

  void amvp_candidates(int xcb, int ycb, int ncbs, int xpb, int ypb, int npbw, int npbh, int part_idx, int ref_idx, int cand[2][2])
  {
    const int xa[2] = {xpb - 1, xpb - 1}, ya[2] = {ypb + npbh, ypb + npbh - 1};                       // A0, A1
    const int xb[3] = {xpb + npbw, xpb + npbw - 1, xpb - 1}, yb[3] = {ypb - 1, ypb - 1, ypb - 1};     // B0, B1, B2
    bool avA[2], avB[3];
    for (int k = 0; k < 2; k++) avA[k] = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xa[k], ya[k]);
    for (int k = 0; k < 3; k++) avB[k] = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xb[k], yb[k]);
    const bool is_scaled = avA[0] || avA[1];
    bool flagA = false, flagB = false; int ax = 0, ay = 0, bx = 0, by = 0;
    const int target = job.ref_poc[ref_idx];
    const bool tlt = job.ref_lt[ref_idx & 15] != 0;          // (8.5.3.2.7 step 7: a vector into ANOTHER picture counts when that picture and the target are both long-term -- as it is -- or both short-term -- scaled)
    for (int k = 0; k < 2 && !flagA; k++) if (avA[k]) { const B4Rec &m = b4[bi(xa[k], ya[k])]; if (job.ref_poc[m.ref_idx & 15] == target) { flagA = true; ax = m.mvx; ay = m.mvy; } }
    for (int k = 0; k < 2 && !flagA; k++) if (avA[k]) { const B4Rec &m = b4[bi(xa[k], ya[k])]; if ((job.ref_lt[m.ref_idx & 15] != 0) != tlt) continue; flagA = true; ax = m.mvx; ay = m.mvy; if (!tlt) scale_mv(ax, ay, m.ref_idx & 15, ref_idx); }
    for (int k = 0; k < 3 && !flagB; k++) if (avB[k]) { const B4Rec &m = b4[bi(xb[k], yb[k])]; if (job.ref_poc[m.ref_idx & 15] == target) { flagB = true; bx = m.mvx; by = m.mvy; } }
    if (!is_scaled && flagB) { flagA = true; ax = bx; ay = by; }
    if (!is_scaled) {
      flagB = false;
      for (int k = 0; k < 3 && !flagB; k++) if (avB[k]) {
        const B4Rec &m = b4[bi(xb[k], yb[k])];
        if ((job.ref_lt[m.ref_idx & 15] != 0) != tlt) continue;
        flagB = true; bx = m.mvx; by = m.mvy;
        if (!tlt && job.ref_poc[m.ref_idx & 15] != target) scale_mv(bx, by, m.ref_idx & 15, ref_idx);
      }
    }
    int n = 0;
    if (flagA) { cand[n][0] = ax; cand[n][1] = ay; n++; }
    if (flagB && !(flagA && ax == bx && ay == by)) { cand[n][0] = bx; cand[n][1] = by; n++; }
    if (n < 2) { int tx, ty; if (temporal_mv(xpb, ypb, npbw, npbh, 0, ref_idx, tx, ty)) { cand[n][0] = tx; cand[n][1] = ty; n++; } }
    for (; n < 2; n++) cand[n][0] = cand[n][1] = 0;
  }

  // ---------------------------------------------------------------- B slices: the same derivations over two-list motion (job.mvf)
  typedef Decoder::PicJob::MvF MvF;
  MvF *mvf = nullptr;                                      // [ph / 4][pw / 4], B slices only
  static bool same_motion_b(const MvF &a, const MvF &b)
  {
    if (a.ref[0] != b.ref[0] || a.ref[1] != b.ref[1]) return false;
    if (a.ref[0] >= 0 && (a.mv[0][0] != b.mv[0][0] || a.mv[0][1] != b.mv[0][1])) return false;
    if (a.ref[1] >= 0 && (a.mv[1][0] != b.mv[1][0] || a.mv[1][1] != b.mv[1][1])) return false;
    return true;
  }
  // 8.5.3.2.2 - 8.5.3.2.5 for a B slice: spatial candidates, the temporal one for both lists, combined bi-predictive candidates, two-list zero candidates
  void merge_candidates_b(int xcb, int ycb, int ncbs, int xpb, int ypb, int npbw, int npbh, int part_idx, int pmode, MvF *cand)
  {
    const int lvl = pps.par_mrg_level;
    int n = 0;
    if (lvl > 2 && ncbs == 8) { xpb = xcb; ypb = ycb; npbw = npbh = ncbs; part_idx = 0; pmode = PART_2Nx2N; }
    auto par = [&](int xn, int yn) { return ((xpb >> lvl) == (xn >> lvl)) && ((ypb >> lvl) == (yn >> lvl)); };
    const int xa1 = xpb - 1, ya1 = ypb + npbh - 1, xb1 = xpb + npbw - 1, yb1 = ypb - 1, xb0 = xpb + npbw, yb0 = ypb - 1;
    const int xa0 = xpb - 1, ya0 = ypb + npbh, xb2 = xpb - 1, yb2 = ypb - 1;
    const bool part1 = part_idx == 1;
    const bool nbA1 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xa1, ya1) && !par(xa1, ya1) &&
                      !(part1 && (pmode == PART_Nx2N || pmode == PART_nLx2N || pmode == PART_nRx2N));
    const bool nbB1 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xb1, yb1) && !par(xb1, yb1) &&
                      !(part1 && (pmode == PART_2NxN || pmode == PART_2NxnU || pmode == PART_2NxnD));
    const bool nbB0 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xb0, yb0) && !par(xb0, yb0);
    const bool nbA0 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xa0, ya0) && !par(xa0, ya0);
    const bool nbB2 = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xb2, yb2) && !par(xb2, yb2);
    MvF zero; memset(&zero, 0, sizeof(zero)); zero.ref[0] = zero.ref[1] = -1;
    const MvF &A1 = nbA1 ? mvf[bi(xa1, ya1)] : zero, &B1 = nbB1 ? mvf[bi(xb1, yb1)] : zero, &B0 = nbB0 ? mvf[bi(xb0, yb0)] : zero;
    const MvF &A0 = nbA0 ? mvf[bi(xa0, ya0)] : zero, &B2 = nbB2 ? mvf[bi(xb2, yb2)] : zero;
    const bool avA1 = nbA1, avB1 = nbB1 && !(nbA1 && same_motion_b(A1, B1)), avB0 = nbB0 && !(nbB1 && same_motion_b(B1, B0));
    const bool avA0 = nbA0 && !(nbA1 && same_motion_b(A1, A0));
    const bool avB2 = nbB2 && !(nbA1 && same_motion_b(A1, B2)) && !(nbB1 && same_motion_b(B1, B2)) && ((int)avA0 + avA1 + avB0 + avB1 != 4);
    const int maxc = sh.max_merge;
    auto add = [&](const MvF &m) { if (n < maxc) cand[n++] = m; };
    if (avA1) add(A1);
    if (avB1) add(B1);
    if (avB0) add(B0);
    if (avA0) add(A0);
    if (avB2) add(B2);
    if (n < maxc) {
      int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
      const bool f0 = temporal_mv(xpb, ypb, npbw, npbh, 0, 0, x0, y0), f1 = temporal_mv(xpb, ypb, npbw, npbh, 1, 0, x1, y1);
      if (f0 || f1) {
        MvF &t = cand[n++];
        t.mv[0][0] = (int16_t)x0; t.mv[0][1] = (int16_t)y0; t.ref[0] = f0 ? 0 : -1;
        t.mv[1][0] = (int16_t)x1; t.mv[1][1] = (int16_t)y1; t.ref[1] = f1 ? 0 : -1;
      }
    }
    if (n > 1 && n < maxc) {                               // 8.5.3.2.4: list-0 motion of one candidate with list-1 motion of another (Table 8-7), unless they are one prediction
      static const uint8_t l0c[12] = {0, 1, 0, 2, 1, 2, 0, 3, 1, 3, 2, 3}, l1c[12] = {1, 0, 2, 0, 2, 1, 3, 0, 3, 1, 3, 2};
      const int norig = n;
      for (int comb = 0; comb < norig * (norig - 1) && n < maxc; comb++) {
        const MvF &p0 = cand[l0c[comb]], &p1 = cand[l1c[comb]];
        if (p0.ref[0] < 0 || p1.ref[1] < 0) continue;
        if (list_poc(0, p0.ref[0]) == list_poc(1, p1.ref[1]) && p0.mv[0][0] == p1.mv[1][0] && p0.mv[0][1] == p1.mv[1][1]) continue;
        MvF &t = cand[n++];
        t.mv[0][0] = p0.mv[0][0]; t.mv[0][1] = p0.mv[0][1]; t.ref[0] = p0.ref[0];
        t.mv[1][0] = p1.mv[1][0]; t.mv[1][1] = p1.mv[1][1]; t.ref[1] = p1.ref[1];
      }
    }
    const int nrefs = imin(sh.num_ref_idx, sh.num_ref_idx1);
    for (int zi = 0; n < maxc; n++, zi++) { MvF &t = cand[n]; memset(&t, 0, sizeof(t)); t.ref[0] = t.ref[1] = (int8_t)(zi < nrefs ? zi : 0); }
  }
  // 8.5.3.2.6 / 8.5.3.2.7 for list X of a B slice: a neighbour's vector into the target picture from either of its lists (its list X first), else any of
  // its vectors scaled by the ratio of the POC distances
  void amvp_candidates_b(int xcb, int ycb, int ncbs, int xpb, int ypb, int npbw, int npbh, int part_idx, int X, int ref_idx, int cand[2][2])
  {
    const int xa[2] = {xpb - 1, xpb - 1}, ya[2] = {ypb + npbh, ypb + npbh - 1};                       // A0, A1
    const int xb[3] = {xpb + npbw, xpb + npbw - 1, xpb - 1}, yb[3] = {ypb - 1, ypb - 1, ypb - 1};     // B0, B1, B2
    bool avA[2], avB[3];
    for (int k = 0; k < 2; k++) avA[k] = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xa[k], ya[k]);
    for (int k = 0; k < 3; k++) avB[k] = pb_avail(xcb, ycb, ncbs, xpb, ypb, npbw, npbh, part_idx, xb[k], yb[k]);
    const bool is_scaled = avA[0] || avA[1];
    bool flagA = false, flagB = false; int ax = 0, ay = 0, bx = 0, by = 0;
    const int target = list_poc(X, ref_idx), Y = X ^ 1;
    auto same_pic = [&](const MvF &m, int &vx, int &vy) {
      for (int L : {X, Y}) if (m.ref[L] >= 0 && list_poc(L, m.ref[L]) == target) { vx = m.mv[L][0]; vy = m.mv[L][1]; return true; }
      return false;
    };
    const bool tlt = list_lt(X, ref_idx);
    auto any_pic = [&](const MvF &m, int &vx, int &vy) {
      for (int L : {X, Y}) if (m.ref[L] >= 0 && list_lt(L, m.ref[L]) == tlt) {
        vx = m.mv[L][0]; vy = m.mv[L][1];
        const int poc = list_poc(L, m.ref[L]);
        if (!tlt && poc != target) scale_by(vx, vy, sh.poc - poc, sh.poc - target);
        return true;
      }
      return false;
    };
    for (int k = 0; k < 2 && !flagA; k++) if (avA[k]) flagA = same_pic(mvf[bi(xa[k], ya[k])], ax, ay);
    for (int k = 0; k < 2 && !flagA; k++) if (avA[k]) flagA = any_pic(mvf[bi(xa[k], ya[k])], ax, ay);
    for (int k = 0; k < 3 && !flagB; k++) if (avB[k]) flagB = same_pic(mvf[bi(xb[k], yb[k])], bx, by);
    if (!is_scaled && flagB) { flagA = true; ax = bx; ay = by; }
    if (!is_scaled) {
      flagB = false;
      for (int k = 0; k < 3 && !flagB; k++) if (avB[k]) flagB = any_pic(mvf[bi(xb[k], yb[k])], bx, by);
    }
    int n = 0;
    if (flagA) { cand[n][0] = ax; cand[n][1] = ay; n++; }
    if (flagB && !(flagA && ax == bx && ay == by)) { cand[n][0] = bx; cand[n][1] = by; n++; }
    if (n < 2) { int tx, ty; if (temporal_mv(xpb, ypb, npbw, npbh, X, ref_idx, tx, ty)) { cand[n][0] = tx; cand[n][1] = ty; n++; } }
    for (; n < 2; n++) cand[n][0] = cand[n][1] = 0;
  }
  int parse_ref_idx(int num_active)
  {
    int ref_idx = 0;
    const int mx = num_active - 1;
    while (ref_idx < mx && ref_idx < 2 && c.bin(CTX_REF_IDX + ref_idx)) ref_idx++;
    if (ref_idx == 2) while (ref_idx < mx && c.bypass()) ref_idx++;
    return ref_idx;
  }
  void parse_mvd(int &dx, int &dy)
  {
    const int g0x = c.bin(CTX_MVD_GT0), g0y = c.bin(CTX_MVD_GT0);
    const int g1x = g0x ? c.bin(CTX_MVD_GT1) : 0, g1y = g0y ? c.bin(CTX_MVD_GT1) : 0;
    dx = mvd_abs(g0x, g1x); if (g0x && c.bypass()) dx = -dx;
    dy = mvd_abs(g0y, g1y); if (g0y && c.bypass()) dy = -dy;
  }
  // prediction_unit() of a B slice (7.3.8.6): inter_pred_idc, a reference index / vector difference / predictor flag per used list
  void prediction_unit_b(int xcb, int ycb, int ncbs, int xp, int yp, int bw, int bh, int part_idx, bool skip, int *merge_out)
  {
    const int merge = skip ? 1 : c.bin(CTX_MERGE_FLAG);
    if (merge_out) *merge_out = merge;
    MvF m; memset(&m, 0, sizeof(m)); m.ref[0] = m.ref[1] = -1;
    if (merge) {
      int idx = 0;
      if (sh.max_merge > 1 && c.bin(CTX_MERGE_IDX)) { idx = 1; while (idx < sh.max_merge - 1 && c.bypass()) idx++; }
      MvF cand[5];
      merge_candidates_b(xcb, ycb, ncbs, xp, yp, bw, bh, part_idx, part_mode, cand);
      m = cand[idx];
      if (m.ref[0] >= 0 && m.ref[1] >= 0 && bw + bh == 12) { m.ref[1] = -1; m.mv[1][0] = m.mv[1][1] = 0; }      // 8x4 / 4x8 blocks are never bi-predicted
    } else {
      int idc;                                             // 0 PRED_L0, 1 PRED_L1, 2 PRED_BI (9.3.4.2: "both" is asked first, with the coding quadtree depth as context, unless the block is 8x4 / 4x8)
      if (bw + bh != 12 && c.bin(CTX_INTER_PRED_IDC + ctd[b8(xcb, ycb)])) idc = 2;
      else idc = c.bin(CTX_INTER_PRED_IDC + 4);
      for (int X = 0; X < 2; X++) {
        if (idc == 1 - X) continue;
        const int na = X ? sh.num_ref_idx1 : sh.num_ref_idx;
        const int ref_idx = na > 1 ? parse_ref_idx(na) : 0;
        int dx = 0, dy = 0;
        if (!(X == 1 && sh.mvd_l1_zero && idc == 2)) parse_mvd(dx, dy);
        const int mvp = c.bin(CTX_MVP_FLAG);
        if (ref_idx >= (X ? job.nref1 : job.nref)) { err = DEC_ERR_INVALID; return; }
        int cand[2][2];
        amvp_candidates_b(xcb, ycb, ncbs, xp, yp, bw, bh, part_idx, X, ref_idx, cand);
        m.mv[X][0] = (int16_t)(uint16_t)(cand[mvp][0] + dx); m.mv[X][1] = (int16_t)(uint16_t)(cand[mvp][1] + dy);      // 8.5.3.2.6: modulo 2^16
        m.ref[X] = (int8_t)ref_idx;
      }
    }
    if ((m.ref[0] < 0 && m.ref[1] < 0) || m.ref[0] >= job.nref || m.ref[1] >= job.nref1) { err = DEC_ERR_INVALID; return; }
    if (ref_y1 != (1 << 30) || ref_y0 != -(1 << 30)) { err = DEC_ERR_UNSUPPORTED; return; }      // (band mode is the split encoder's streams: P pictures)
    const int P = m.ref[0] >= 0 ? 0 : 1;                   // the list whose motion rides in the B4Rec
    const bool bi = m.ref[0] >= 0 && m.ref[1] >= 0;
    // explicit weights only where an entry the block uses differs from the defaults: ((p 2^d + 2^(d + 5)) >> (d + 6)) = (p + 32) >> 6 and the mean likewise
    const bool wtd = sh.weighted && (((m.ref[0] >= 0) && ((sh.wt_explicit >> m.ref[0]) & 1)) || ((m.ref[1] >= 0) && ((sh.wt_explicit >> (16 + m.ref[1])) & 1)));
    B4Rec r; r.mvx = m.mv[P][0]; r.mvy = m.mv[P][1]; r.ref_idx = m.ref[P]; r.flags = (uint8_t)((cu_bypass ? B4_BYPASS : 0) | (bi ? B4_BI : 0) | (wtd ? B4_WT : 0)); r.qp_y = (int8_t)qp_y;
    r.slot = P ? job.ref_slot1[m.ref[1]] : job.ref_slot[m.ref[0]];
    fill_recs(xp, yp, bw, bh, r, bw == ncbs && bh == ncbs);
    B4L1 x; x.mvx = m.mv[1][0]; x.mvy = m.mv[1][1]; x.slot = bi ? job.ref_slot1[m.ref[1]] : 0; x.pad[0] = (uint8_t)(P * 16 + m.ref[P]); x.pad[1] = (uint8_t)(bi ? 16 + m.ref[1] : 0); x.pad[2] = 0;
    const int cols = imin(bw, w - xp) >> 2;
    const bool ext = bi || wtd;                            // the block has an entry in b4x[]
    for (int y = yp; y < yp + bh && y < h; y += 4) { const int i0 = bi_(xp, y); for (int i = 0; i < cols; i++) { mvf[i0 + i] = m; if (ext) job.b4x[(size_t)(i0 + i)] = x; } }
    if (ext) if (!job.any_bi.load(std::memory_order_relaxed)) job.any_bi.store(1, std::memory_order_relaxed);
    if (bw != ncbs || bh != ncbs) {                          // prediction block edges inside the coding block (deblocking)
      for (int i = 0; i < bh && yp + i < h; i += 4) b4[bi_(xp, yp + i)].flags |= B4_EDGE_V;
      for (int i = 0; i < bw && xp + i < w; i += 4) b4[bi_(xp + i, yp)].flags |= B4_EDGE_H;
    }
  }
  inline int bi_(int x, int y) const { return (y >> 2) * b4w + (x >> 2); }      // (bi() under a name that does not collide with the local `bi`)

  int mvd_abs(int gt0, int gt1)
  {
    if (!gt0) return 0;
    if (!gt1) return 1;
    int k = 1, v = 0;
    while (k < 17 && c.bypass()) { v += 1 << k; k++; }           // (EG1 prefix: a vector difference fits 16 bits, 7.4.9.9 -- at most 15 ones follow the first order bit)
    if (k >= 17) { err = DEC_ERR_INVALID; return 0; }
    return v + (int)c.bypass_bits(k) + 2;
  }

  void prediction_unit(int xcb, int ycb, int ncbs, int xp, int yp, int bw, int bh, int part_idx, bool skip, int *merge_out)
  {
    if (sh.is_b) { prediction_unit_b(xcb, ycb, ncbs, xp, yp, bw, bh, part_idx, skip, merge_out); return; }
    const int merge = skip ? 1 : c.bin(CTX_MERGE_FLAG);
    if (merge_out) *merge_out = merge;
    int mvx, mvy, ref_idx = 0;
    if (merge) {
      int idx = 0;
      if (sh.max_merge > 1 && c.bin(CTX_MERGE_IDX)) { idx = 1; while (idx < sh.max_merge - 1 && c.bypass()) idx++; }
      MvCand cand[5];
      merge_candidates(xcb, ycb, ncbs, xp, yp, bw, bh, part_idx, part_mode, cand, idx);
      mvx = cand[idx].mvx; mvy = cand[idx].mvy; ref_idx = cand[idx].ref_idx;
    } else {
      if (sh.num_ref_idx > 1) {
        const int mx = sh.num_ref_idx - 1;
        while (ref_idx < mx && ref_idx < 2 && c.bin(CTX_REF_IDX + ref_idx)) ref_idx++;
        if (ref_idx == 2) while (ref_idx < mx && c.bypass()) ref_idx++;
      }
      const int g0x = c.bin(CTX_MVD_GT0), g0y = c.bin(CTX_MVD_GT0);
      const int g1x = g0x ? c.bin(CTX_MVD_GT1) : 0, g1y = g0y ? c.bin(CTX_MVD_GT1) : 0;
      int dx = mvd_abs(g0x, g1x); if (g0x && c.bypass()) dx = -dx;
      int dy = mvd_abs(g0y, g1y); if (g0y && c.bypass()) dy = -dy;
      const int mvp = c.bin(CTX_MVP_FLAG);
      int cand[2][2];
      amvp_candidates(xcb, ycb, ncbs, xp, yp, bw, bh, part_idx, ref_idx, cand);
      mvx = (int16_t)(uint16_t)(cand[mvp][0] + dx); mvy = (int16_t)(uint16_t)(cand[mvp][1] + dy);      // 8.5.3.2.6: modulo 2^16
    }
    if (ref_idx < 0 || ref_idx >= job.nref) { err = DEC_ERR_INVALID; ref_idx = 0; }
    if (ref_y1 != (1 << 30) || ref_y0 != -(1 << 30)) {        // band mode: the vector must stay inside this decoder's rows (luma 8-tap, chroma 4-tap windows)
      const int fy = mvy & 3, fc = mvy & 7;
      const int top = imin(yp + (mvy >> 2) - (fy ? 3 : 0), 2 * ((yp >> 1) + (mvy >> 3) - (fc ? 1 : 0)));
      const int bot = imax(yp + bh + (mvy >> 2) + (fy ? 4 : 0), 2 * ((yp >> 1) + (bh >> 1) + (mvy >> 3) + (fc ? 2 : 0)));
      if (top < ref_y0 || bot > ref_y1) err = DEC_ERR_UNSUPPORTED;
    }
    B4Rec r; r.mvx = (int16_t)mvx; r.mvy = (int16_t)mvy; r.ref_idx = (int8_t)ref_idx; r.flags = (uint8_t)((cu_bypass ? B4_BYPASS : 0) | ((sh.weighted && ((sh.wt_explicit >> ref_idx) & 1)) ? B4_WT : 0)); r.qp_y = (int8_t)qp_y; r.slot = job.ref_slot[ref_idx];
    fill_recs(xp, yp, bw, bh, r, bw == ncbs && bh == ncbs);
    if (r.flags & B4_WT) {                                       // explicit weights: the block's table entry rides where B pictures keep their second vectors
      B4L1 x; x.mvx = 0; x.mvy = 0; x.slot = 0; x.pad[0] = (uint8_t)ref_idx; x.pad[1] = x.pad[2] = 0;
      const int cols = imin(bw, w - xp) >> 2;
      for (int y = yp; y < yp + bh && y < h; y += 4) { const int i0 = bi(xp, y); for (int i = 0; i < cols; i++) job.b4x[(size_t)(i0 + i)] = x; }
      if (!job.any_bi.load(std::memory_order_relaxed)) job.any_bi.store(1, std::memory_order_relaxed);
    }
    if (bw != ncbs || bh != ncbs) {                          // prediction block edges inside the coding block (deblocking); the block's own are set by coding_unit
      for (int i = 0; i < bh && yp + i < h; i += 4) b4[bi(xp, yp + i)].flags |= B4_EDGE_V;
      for (int i = 0; i < bw && xp + i < w; i += 4) b4[bi(xp + i, yp)].flags |= B4_EDGE_H;
    }
  }

  // ---------------------------------------------------------------- transform tree (7.3.8.8 - 7.3.8.10)
  void transform_unit(int x0, int y0, int xbase, int ybase, int log2, int blk, int cbf_luma, int cbf_cb, int cbf_cr, int cbf_cb_parent, int cbf_cr_parent)
  {
    const bool intra = cu_pred_mode == PM_INTRA;
    const bool chroma_here = log2 > 2, chroma_parent = log2 == 2 && blk == 3;
    const int ccb = chroma_here ? cbf_cb : (chroma_parent ? cbf_cb_parent : 0), ccr = chroma_here ? cbf_cr : (chroma_parent ? cbf_cr_parent : 0);
    const bool cbf_chroma_any = log2 > 2 ? (cbf_cb || cbf_cr) : (cbf_cb_parent || cbf_cr_parent);
    if ((cbf_luma || cbf_chroma_any) && pps.cu_qp_delta && !qp_delta_coded) {
      int v = 0;
      while (v < 5 && c.bin(CTX_CU_QP_DELTA + (v ? 1 : 0))) v++;
      if (v == 5) { int k = 0; while (k < 16 && c.bypass()) { v += 1 << k; k++; } if (k >= 16) { err = DEC_ERR_INVALID; return; } v += (int)c.bypass_bits(k); }
      if (v && c.bypass()) v = -v;
      if (v < -26 || v > 25) { err = DEC_ERR_INVALID; return; }
      qp_delta_coded = true; cu_qp_delta_val = v;
      qp_y = (qp_y_pred + v + 52) % 52;
    }
    const int n = 1 << log2;
    DecTu td; td.pad = 0;
    const int lmode = intra ? im[bi(x0, y0)] : 0;
    if (intra || cbf_luma) {
      td.x = (uint16_t)x0; td.y = (uint16_t)y0; td.plane = 0; td.log2 = (uint8_t)log2; td.mode = (uint8_t)lmode; td.qp = (int8_t)qp_y;
      td.flags = (uint8_t)((intra ? TU_INTRA : 0) | ((intra && log2 == 2) ? TU_DST : 0) | (cu_bypass ? TU_BYPASS : 0));
      td.offset = (uint32_t)out.levels.size(); td.count = 0;
      if (cbf_luma) {
        int ts;
        if (!parse_residual(c, log2, 0, intra_scan_idx(intra, log2, 0, lmode), pps.sign_hiding != 0 && !cu_bypass, pps.tskip != 0 && !cu_bypass, &ts, out.levels)) { err = DEC_ERR_INVALID; return; }
        td.count = (uint16_t)(out.levels.size() - td.offset);
        if (ts) td.flags |= TU_TSKIP;
        for (int y = y0; y < y0 + n && y < h; y += 4) for (int x = x0; x < x0 + n && x < w; x += 4) b4[bi(x, y)].flags |= B4_NZ;
      }
      emit_tu(td);
      if (intra) ctu_intra_mask |= 1u;
    }
    if (chroma_here || chroma_parent) {
      const int cx = (chroma_here ? x0 : xbase) >> 1, cy = (chroma_here ? y0 : ybase) >> 1, clog2 = chroma_here ? log2 - 1 : 2;
      for (int ci = 1; ci <= 2; ci++) {
        const int cbf = ci == 1 ? ccb : ccr;
        if (!intra && !cbf) continue;
        td.x = (uint16_t)cx; td.y = (uint16_t)cy; td.plane = (uint8_t)ci; td.log2 = (uint8_t)clog2; td.mode = (uint8_t)chroma_mode;
        td.qp = (int8_t)kChromaQp[clip3(0, 57, qp_y + (ci == 1 ? sh.cb_qp_offset : sh.cr_qp_offset))];
        td.flags = (uint8_t)((intra ? TU_INTRA : 0) | (cu_bypass ? TU_BYPASS : 0));
        td.offset = (uint32_t)out.levels.size(); td.count = 0;
        if (cbf) {
          int ts;
          if (!parse_residual(c, clog2, ci, intra_scan_idx(intra, clog2, ci, chroma_mode), pps.sign_hiding != 0 && !cu_bypass, pps.tskip != 0 && !cu_bypass, &ts, out.levels)) { err = DEC_ERR_INVALID; return; }
          td.count = (uint16_t)(out.levels.size() - td.offset);
          if (ts) td.flags |= TU_TSKIP;
        }
        emit_tu(td);
        if (intra) ctu_intra_mask |= 1u << ci;
      }
    }
  }

  void transform_tree(int x0, int y0, int xbase, int ybase, int log2, int depth, int blk, int cbf_cb_parent, int cbf_cr_parent)
  {
    if (err) return;
    int split;
    if (log2 <= 5 && log2 > 2 && depth < max_trafo_depth && !(intra_split && depth == 0)) split = c.bin(CTX_SPLIT_TRANSFORM + 5 - log2);
    else {
      const bool inter_split = sps.th_depth_inter == 0 && cu_pred_mode == PM_INTER && part_mode != PART_2Nx2N && depth == 0;
      split = (log2 > imin(5, ctbl) || (intra_split && depth == 0) || inter_split) ? 1 : 0;      // (MaxTbLog2SizeY = min(5, CtbLog2SizeY): checked against the SPS)
    }
    int cbf_cb = 0, cbf_cr = 0;
    if (log2 > 2) {
      if (depth == 0 || cbf_cb_parent) cbf_cb = c.bin(CTX_CBF_CHROMA + depth);
      if (depth == 0 || cbf_cr_parent) cbf_cr = c.bin(CTX_CBF_CHROMA + depth);
    } else { cbf_cb = cbf_cb_parent; cbf_cr = cbf_cr_parent; }
    if (split) {
      if (log2 <= 2) { err = DEC_ERR_INVALID; return; }
      const int hh = 1 << (log2 - 1);
      transform_tree(x0, y0, x0, y0, log2 - 1, depth + 1, 0, cbf_cb, cbf_cr);
      transform_tree(x0 + hh, y0, x0, y0, log2 - 1, depth + 1, 1, cbf_cb, cbf_cr);
      transform_tree(x0, y0 + hh, x0, y0, log2 - 1, depth + 1, 2, cbf_cb, cbf_cr);
      transform_tree(x0 + hh, y0 + hh, x0, y0, log2 - 1, depth + 1, 3, cbf_cb, cbf_cr);
    } else {
      int cbf_luma = 1;
      if (cu_pred_mode == PM_INTRA || depth != 0 || cbf_cb || cbf_cr) cbf_luma = c.bin(CTX_CBF_LUMA + (depth == 0 ? 1 : 0));
      if (depth > 0) {                                     // transform block edges inside the coding block (deblocking)
        const int n = 1 << log2;
        for (int i = 0; i < n; i += 4) {
          if (y0 + i < h) b4[bi(x0, y0 + i)].flags |= B4_EDGE_V | B4_TU_V;
          if (x0 + i < w) b4[bi(x0 + i, y0)].flags |= B4_EDGE_H | B4_TU_H;
        }
      }
      transform_unit(x0, y0, xbase, ybase, log2, blk, cbf_luma, log2 > 2 ? cbf_cb : 0, log2 > 2 ? cbf_cr : 0, cbf_cb_parent, cbf_cr_parent);
    }
  }

  // ---------------------------------------------------------------- coding unit (7.3.8.5)
  void coding_unit(int x0, int y0, int log2cb, int depth)
  {
    const int n = 1 << log2cb;
    int skip = 0;
    cu_bypass = pps.tq_bypass ? c.bin(CTX_TQ_BYPASS) : 0;      // cu_transquant_bypass_flag (7.3.8.5: first in the coding unit)
    if (!sh.is_intra) {
      const int l = avail(x0, y0, x0 - 1, y0) && pm[b8(x0 - 1, y0)] == PM_SKIP, a = avail(x0, y0, x0, y0 - 1) && pm[b8(x0, y0 - 1)] == PM_SKIP;
      skip = c.bin(CTX_SKIP + l + a);
    }
    part_mode = PART_2Nx2N; intra_split = false; cu_edges_done = false;
    int rqt_root_cbf = 1, merge_2nx2n = 0;
    fill_cu8(ctd, x0, y0, n, depth);
    qp_y = (qp_y_pred + cu_qp_delta_val + 52) % 52;          // CuQpDeltaVal of the quantisation group so far
    if (skip) {
      cu_pred_mode = PM_INTER;
      fill_cu8(pm, x0, y0, n, PM_SKIP);
      prediction_unit(x0, y0, n, x0, y0, n, n, 0, true, nullptr);
      rqt_root_cbf = 0;
      if (!job.any_inter) job.any_inter = true;
    } else {
      cu_pred_mode = PM_INTRA;
      if (!sh.is_intra) cu_pred_mode = c.bin(CTX_PRED_MODE) ? PM_INTRA : PM_INTER;
      if (cu_pred_mode != PM_INTRA || log2cb == mincb) {
        if (cu_pred_mode == PM_INTRA) part_mode = c.bin(CTX_PART_MODE) ? PART_2Nx2N : PART_NxN;
        else if (c.bin(CTX_PART_MODE)) part_mode = PART_2Nx2N;
        else if (log2cb == mincb) {                          // 9.3.3.7 at the minimum size: 01 2NxN, 00 Nx2N at 8x8 (no NxN there); above it 01, 001, 000 = NxN
          if (c.bin(CTX_PART_MODE + 1)) part_mode = PART_2NxN;
          else if (log2cb == 3) part_mode = PART_Nx2N;
          else part_mode = c.bin(CTX_PART_MODE + 2) ? PART_Nx2N : PART_NxN;
        }
        else if (!sps.amp) part_mode = c.bin(CTX_PART_MODE + 1) ? PART_2NxN : PART_Nx2N;
        else {
          const int horiz = c.bin(CTX_PART_MODE + 1);
          if (c.bin(CTX_PART_MODE + 3)) part_mode = horiz ? PART_2NxN : PART_Nx2N;
          else { const int b = c.bypass(); part_mode = horiz ? (b ? PART_2NxnD : PART_2NxnU) : (b ? PART_nRx2N : PART_nLx2N); }
        }
      }
      fill_cu8(pm, x0, y0, n, cu_pred_mode);
      if (cu_pred_mode == PM_INTRA && part_mode == PART_2Nx2N && sps.pcm_depth[0] && log2cb >= sps.pcm_min_log2 && log2cb <= sps.pcm_max_log2 && c.terminate()) {
        // pcm_flag = 1 (7.3.8.5, 7.3.8.7): the arithmetic codeword has ended; zero bits to the byte boundary, the samples at their bit depths, and the arithmetic
        // decoder starts again behind them with the contexts as they are (9.3.2.5).  For the kernels the unit is an intra unit of one transform block per plane
        // whose "levels" ARE the samples (shifted up to 8 bits) -- the residual path of cu_transquant_bypass_flag -- over a prediction of zero (mode 35: none);
        // for its neighbours its mode is DC (8.4.2); pcm_loop_filter_disabled_flag keeps the loop filters off it the way the bypass flag does.
        const uint8_t *q = c.buf + c.bytes_consumed();
        const size_t need = ((size_t)n * n * sps.pcm_depth[0] + (size_t)n * n / 2 * sps.pcm_depth[1]) / 8;
        if (q > c.end || need > (size_t)(c.end - q)) { err = DEC_ERR_INVALID; return; }
        BitReader pr(q, need);
        for (int ci = 0; ci < 3; ci++) {
          const int shp = ci ? 1 : 0, m = n >> shp, depth = sps.pcm_depth[ci ? 1 : 0];
          DecTu td; td.pad = 0; td.x = (uint16_t)(x0 >> shp); td.y = (uint16_t)(y0 >> shp); td.plane = (uint8_t)ci; td.log2 = (uint8_t)(log2cb - shp); td.mode = 35; td.qp = 0;
          td.flags = (uint8_t)(TU_INTRA | TU_BYPASS); td.offset = (uint32_t)out.levels.size();
          for (int y = 0; y < m; y++)
            for (int x = 0; x < m; x++) { const uint32_t v = pr.get(depth) << (8 - depth); if (v) out.levels.push_back((uint32_t)((y * m + x) << 16) | v); }
          td.count = (uint16_t)(out.levels.size() - td.offset);
          emit_tu(td);
          ctu_intra_mask |= 1u << ci;
        }
        c.start(q + need, (size_t)(c.end - (q + need)));
        fill_u8(im, x0, y0, n, n, 1);
        B4Rec r; r.mvx = 0; r.mvy = 0; r.ref_idx = -1; r.flags = (uint8_t)((cu_bypass || sps.pcm_no_filter) ? B4_BYPASS : 0); r.qp_y = (int8_t)qp_y; r.slot = 0;
        fill_recs(x0, y0, n, n, r, true);
        if (!job.any_intra) job.any_intra = true;
        rqt_root_cbf = 0;
      } else
      if (cu_pred_mode == PM_INTRA) {
        intra_split = part_mode == PART_NxN;
        const int parts = intra_split ? 2 : 1, pb = n / parts;
        int prev[4], k = 0;
        for (int j = 0; j < parts * parts; j++) prev[j] = c.bin(CTX_PREV_INTRA);
        for (int j = 0; j < parts; j++)
          for (int i = 0; i < parts; i++, k++) {
            const int xp = x0 + i * pb, yp = y0 + j * pb;
            int ca = 1, cb = 1;                                   // 8.4.2 candidate modes
            if (avail(xp, yp, xp - 1, yp) && pm[b8(xp - 1, yp)] == PM_INTRA) ca = im[bi(xp - 1, yp)];
            if (avail(xp, yp, xp, yp - 1) && pm[b8(xp, yp - 1)] == PM_INTRA && (yp - 1) >= ((yp >> ctbl) << ctbl)) cb = im[bi(xp, yp - 1)];
            int cand[3];
            if (ca == cb) {
              if (ca < 2) { cand[0] = 0; cand[1] = 1; cand[2] = 26; }
              else { cand[0] = ca; cand[1] = 2 + ((ca + 29) % 32); cand[2] = 2 + ((ca - 2 + 1) % 32); }
            } else {
              cand[0] = ca; cand[1] = cb;
              cand[2] = (ca != 0 && cb != 0) ? 0 : ((ca != 1 && cb != 1) ? 1 : 26);
            }
            int mode;
            if (prev[k]) { int idx = 0; if (c.bypass()) { idx = 1; if (c.bypass()) idx = 2; } mode = cand[idx]; }
            else {
              mode = (int)c.bypass_bits(5);
              int t;
              if (cand[0] > cand[1]) { t = cand[0]; cand[0] = cand[1]; cand[1] = t; }
              if (cand[0] > cand[2]) { t = cand[0]; cand[0] = cand[2]; cand[2] = t; }
              if (cand[1] > cand[2]) { t = cand[1]; cand[1] = cand[2]; cand[2] = t; }
              for (int q = 0; q < 3; q++) if (mode >= cand[q]) mode++;
            }
            intra_modes[k] = mode;
            fill_u8(im, xp, yp, pb, pb, mode);
          }
        int icpm = 4;
        if (c.bin(CTX_CHROMA_MODE)) icpm = (int)c.bypass_bits(2);
        static const int cm[4] = {0, 26, 10, 1};
        if (icpm == 4) chroma_mode = intra_modes[0];
        else { chroma_mode = cm[icpm]; if (chroma_mode == intra_modes[0]) chroma_mode = 34; }
        B4Rec r; r.mvx = 0; r.mvy = 0; r.ref_idx = -1; r.flags = (uint8_t)(cu_bypass ? B4_BYPASS : 0); r.qp_y = (int8_t)qp_y; r.slot = 0;
        fill_recs(x0, y0, n, n, r, true);
        if (!job.any_intra) job.any_intra = true;
      } else {
        const int hh = n / 2, q = n / 4; int mf = 0;
        switch (part_mode) {
          case PART_2Nx2N: prediction_unit(x0, y0, n, x0, y0, n, n, 0, false, &merge_2nx2n); break;
          case PART_2NxN: prediction_unit(x0, y0, n, x0, y0, n, hh, 0, false, &mf); prediction_unit(x0, y0, n, x0, y0 + hh, n, hh, 1, false, &mf); break;
          case PART_Nx2N: prediction_unit(x0, y0, n, x0, y0, hh, n, 0, false, &mf); prediction_unit(x0, y0, n, x0 + hh, y0, hh, n, 1, false, &mf); break;
          case PART_2NxnU: prediction_unit(x0, y0, n, x0, y0, n, q, 0, false, &mf); prediction_unit(x0, y0, n, x0, y0 + q, n, n - q, 1, false, &mf); break;
          case PART_2NxnD: prediction_unit(x0, y0, n, x0, y0, n, n - q, 0, false, &mf); prediction_unit(x0, y0, n, x0, y0 + n - q, n, q, 1, false, &mf); break;
          case PART_nLx2N: prediction_unit(x0, y0, n, x0, y0, q, n, 0, false, &mf); prediction_unit(x0, y0, n, x0 + q, y0, n - q, n, 1, false, &mf); break;
          case PART_NxN:                                       // (a minimum coding block above 8 samples: four square prediction blocks in z-order)
            for (int k = 0; k < 4; k++) prediction_unit(x0, y0, n, x0 + (k & 1) * hh, y0 + (k >> 1) * hh, hh, hh, k, false, &mf);
            break;
          default: prediction_unit(x0, y0, n, x0, y0, n - q, n, 0, false, &mf); prediction_unit(x0, y0, n, x0 + n - q, y0, q, n, 1, false, &mf); break;     // nRx2N
        }
        if (!(part_mode == PART_2Nx2N && merge_2nx2n)) rqt_root_cbf = c.bin(CTX_RQT_ROOT_CBF);
        if (!job.any_inter) job.any_inter = true;
      }
    }
    if (err) return;
    if (!cu_edges_done) {                                  // coding block edges are transform and prediction edges (a block of one prediction block: written with its records)
      B4Rec *const r0 = &b4[bi(x0, y0)];
      const int rows = (imin(n, h - y0) + 3) >> 2, cols = (imin(n, w - x0) + 3) >> 2;
      for (int i = 0; i < rows; i++) r0[(size_t)i * b4w].flags |= B4_EDGE_V | B4_TU_V;
      for (int i = 0; i < cols; i++) r0[i].flags |= B4_EDGE_H | B4_TU_H;
    }
    const int qp_before = qp_y;
    if (rqt_root_cbf) {
      max_trafo_depth = cu_pred_mode == PM_INTRA ? sps.th_depth_intra + (intra_split ? 1 : 0) : sps.th_depth_inter;
      transform_tree(x0, y0, x0, y0, log2cb, 0, 0, 0, 0);
    }
    if (qp_y != qp_before)                                   // a cu_qp_delta arrived inside this unit: its QpY is the new one (8.6.1)
      for (int y = y0; y < y0 + n && y < h; y += 4) for (int x = x0; x < x0 + n && x < w; x += 4) b4[bi(x, y)].qp_y = (int8_t)qp_y;
    last_qp_y = qp_y;
  }

  void coding_quadtree(int x0, int y0, int log2cb, int depth)
  {
    if (err) return;
    const int n = 1 << log2cb;
    int split;
    if (x0 + n <= w && y0 + n <= h && log2cb > mincb) {
      const int l = avail(x0, y0, x0 - 1, y0) && ctd[b8(x0 - 1, y0)] > depth, a = avail(x0, y0, x0, y0 - 1) && ctd[b8(x0, y0 - 1)] > depth;
      split = c.bin(CTX_SPLIT_CU + l + a);
    } else split = log2cb > mincb;
    if (pps.cu_qp_delta && log2cb >= log2_qg) {            // a quantisation group starts here (7.3.8.4, 8.6.1)
      qp_delta_coded = false; cu_qp_delta_val = 0;
      int qa = last_qp_y, qb = last_qp_y;
      if (avail(x0, y0, x0 - 1, y0) && ((x0 - 1) >> ctbl) == (x0 >> ctbl)) qa = b4[bi(x0 - 1, y0)].qp_y;
      if (avail(x0, y0, x0, y0 - 1) && ((y0 - 1) >> ctbl) == (y0 >> ctbl)) qb = b4[bi(x0, y0 - 1)].qp_y;
      qp_y_pred = (qa + qb + 1) >> 1;
    }
    if (split) {
      const int hh = n >> 1;
      coding_quadtree(x0, y0, log2cb - 1, depth + 1);
      if (x0 + hh < w) coding_quadtree(x0 + hh, y0, log2cb - 1, depth + 1);
      if (y0 + hh < h) coding_quadtree(x0, y0 + hh, log2cb - 1, depth + 1);
      if (x0 + hh < w && y0 + hh < h) coding_quadtree(x0 + hh, y0 + hh, log2cb - 1, depth + 1);
    } else coding_unit(x0, y0, log2cb, depth);
  }
};

}  // namespace

// ------------------------------------------------------------------------------------------ slice data (7.3.8)
// One task per substream -- a CTU row with WPP, else a tile -- run by a pool of host threads.  With WPP row r follows row r-1
// at a distance of two CTUs: it starts from the context states saved after the second CTU of the row above and needs that row's
// records up to the above-right CTU.
int Decoder::parse_substream(PicJob &job, int sub, const uint8_t *data, size_t len, SubOut &out)
{
  SliceParser sp(job, out, pw_);
  tl("row0", sub);
  struct RowEnd { int s; ~RowEnd() { tl("row1", s); } } row_end_{sub};
  if (job.sh.is_b) sp.mvf = job.mvf.data();
  const int wc = sp.wc;
  const DecPps &pps = job.pps; const SliceHdr &sh = job.sh;
  const bool wpp = pps.wpp != 0;
  const PicJob::SubGeom g = job.geom[(size_t)sub];
  const int first_cy = g.cy0, ncy = g.cy1 - g.cy0, cx0 = g.cx0, cx1 = g.cx1, tw = cx1 - cx0, cols = pps.tile_cols;
  auto tile_starts_at = [&](int cy) { return cy == g.tile_cy0; };
  auto tile_ends_at = [&](int cy) { return cy + 1 == g.tile_cy1; };
  int seen_above = 0;                                  // last observed progress of the row above inside the tile (monotonic)
  auto wait_above = [&](int cy, int need) {            // CTUs of the tile's row cy-1 that must be complete
    if (!wpp || tile_starts_at(cy)) return true;       // nothing above inside the tile
    if (need > tw) need = tw;
    if (seen_above < need) {
      std::atomic<int> &p = job.row_progress[(size_t)(cy - 1) * cols + g.tc].v;
      int spins = 0;
      while ((seen_above = p.load(std::memory_order_acquire)) < need) {
        if (++spins < 2000) __builtin_ia32_pause(); else { g_yields.fetch_add(1, std::memory_order_relaxed); std::this_thread::yield(); }
      }
    }
    return seen_above < (1 << 29);                     // >= 1 << 29: that row failed
  };
  const int init_type = sh.is_intra ? 0 : (sh.is_b ? (sh.cabac_init_flag ? 1 : 2) : (sh.cabac_init_flag ? 2 : 1));      // 9.3.2.2: cabac_init_flag swaps the P and the B tables
  CabacDec &c = sp.c;
  // free slices (PicJob::ctb_cut; one tile): the slice of every coding tree block, its SliceQpY
  const bool free_slices = !job.ctb_cut.empty();
  // partial pictures v1, one tile (PicJob::scan_gaps): where a segment ends is known only here.  `skipping`: the blocks at hand belong to no decoded segment -- in front of
  // the first segment that arrived, or behind a segment that ended before the next one's address (the gap), a dependent successor included (its predecessor is gone: it is
  // skipped, with its bytes) -- until an INDEPENDENT segment begins.  A skipped block gets what makes every kernel do nothing there (rule 3), the slice byte 255 (no decoded
  // slice has it: close_free_picture) and a mark in job.miss_map; parse_job makes PicJob::missing of the marks.  Without WPP one thread walks the picture.  With WPP (free
  // slices; `data` is then the whole of the picture's bytes, every start of the arithmetic decoder names its own offset) a row learns from the row above whether it begins
  // inside a gap: an independent segment at its start decodes; a dependent one decodes if the last block of the row above was decoded (that row is waited for); a row that
  // continues a segment (an entry point) decodes if that segment's first block was decoded -- a block of the row above, waited for, or of a row further up, which the row
  // above has looked at before its own first block; a row without bytes skips.  A skipped block's progress is published like a decoded one's: nothing waits in vain.
  const bool scan = job.scan_gaps && cols == 1 && (!wpp || free_slices);
  bool skipping = false;
  size_t first_off = 0;                                   // scan with WPP: where this row's bytes begin in `data`
  if (scan && free_slices) {
    const int a0 = first_cy * wc + cx0;
    const uint8_t cut0 = job.ctb_cut[(size_t)a0];
    if (cut0 & 1) skipping = false;
    else if (a0 == 0) skipping = true;
    else if (cut0 & 2) { if (!wait_above(first_cy, tw)) return DEC_ERR_INVALID; skipping = job.miss_map[(size_t)a0 - 1] != 0; }
    else if (job.sub_start[(size_t)first_cy] == SIZE_MAX || job.row_seg_start[(size_t)first_cy] < 0) skipping = true;
    else {
      const int s0 = job.row_seg_start[(size_t)first_cy];
      if (!wait_above(first_cy, s0 / wc == first_cy - 1 ? imax(2, s0 % wc + 1) : 2)) return DEC_ERR_INVALID;
      skipping = job.miss_map[(size_t)s0] != 0;
    }
    if (wpp && !skipping) { first_off = job.sub_start[(size_t)first_cy]; if (first_off == SIZE_MAX || first_off >= len) return DEC_ERR_INVALID; }
  }
  c.start(data + first_off, len - first_off);
  sp.slice_qp = sh.slice_qp;
  if (free_slices) { sp.slice_of = job.ctb_slice.data(); sp.cur_slice = job.ctb_slice[(size_t)first_cy * wc + cx0]; sp.slice_qp = job.slice_qps[(size_t)sp.cur_slice]; }
  auto init_contexts = [&] { uint8_t init[CTX_COUNT]; cabac_init_contexts(init, init_type, sp.slice_qp); c.load_ctx(init); };
  // 9.3.1: the first CTB of a tile initialises the contexts; a WPP row takes them over from the row above after its second
  // CTB when that CTB exists (pictures one CTB wide: it does not, and the row initialises afresh) -- and is AVAILABLE: with free slices it may
  // belong to another slice; then a dependent segment that begins with this row goes on where the segment before it stopped (the end of the row
  // above), anything else initialises
  if (skipping) init_contexts();                        // (whatever: the next block decoded begins an independent slice)
  else if (!wpp || tile_starts_at(first_cy) || tw < 2) init_contexts();
  else if (scan && !wait_above(first_cy, 2)) return DEC_ERR_INVALID;      // (the row above may have found its second block missing: its slice byte is read below)
  else if (free_slices && job.ctb_slice[(size_t)(first_cy - 1) * wc + cx0 + 1] != sp.cur_slice) {
    if (job.ctb_cut[(size_t)first_cy * wc + cx0] & 2) {
      if (!wait_above(first_cy, tw)) return DEC_ERR_INVALID;
      c.load_ctx(&job.ds_saved[(size_t)(first_cy - 1) * CTX_COUNT]);
    } else init_contexts();
  } else {
    if (!wait_above(first_cy, 2)) return DEC_ERR_INVALID;
    c.load_ctx(&job.wpp_saved[((size_t)(first_cy - 1) * cols + g.tc) * CTX_COUNT]);
  }
  sp.last_qp_y = sp.slice_qp;                          // qPY_PREV at the start of a slice, a tile, a CTB row with WPP (8.6.1)
  sp.tile_y0 = g.tile_cy0 << ctbl_; sp.tile_y1 = g.tile_cy1 << ctbl_; sp.tile_x0 = cx0 << ctbl_; sp.tile_x1 = cx1 << ctbl_;
  if (band_nrows_ > 0) {
    if (band_row0_ > 0) sp.ref_y0 = band_row0_ * 64 - 4;
    if (band_row0_ + band_nrows_ < (h_ + 63) / 64) sp.ref_y1 = (band_row0_ + band_nrows_) * 64;
  }
  ColMotion *own = job.own.get();
  auto mark_missing = [&](int ctu) {
    const int per = 1 << (ctbl_ - 2), b4w = pw_ / 4, mx = ctu % wc, my = ctu / wc;
    B4Rec none; memset(&none, 0, sizeof(none)); none.ref_idx = -1;
    for (int k = 0; k < per; k++) for (int x = 0; x < per; x++) job.b4[(size_t)(my * per + k) * b4w + mx * per + x] = none;
    job.ctu_tile[ctu] = 255; if (free_slices) job.ctb_slice[(size_t)ctu] = 255;
    memset(&job.sao[ctu], 0, sizeof(SaoParams));
    job.miss_map[(size_t)ctu] = 1;
    if (wpp) job.row_progress[(size_t)(ctu / wc) * cols + g.tc].v.store(ctu % wc - cx0 + 1, std::memory_order_release);
  };
  for (int cy = first_cy; cy < first_cy + ncy; cy++) {
    if (cy > first_cy && job.row_restart[(size_t)cy] != SIZE_MAX) {
      // a dependent slice segment begins inside this substream: new arithmetic codeword, the contexts go on (9.3.1)
      const uint8_t *q = job.rbsp.data() + job.data_off + job.row_restart[(size_t)cy];
      if (q < data || q >= data + len) return DEC_ERR_INVALID;
      c.start(q, (size_t)(data + len - q));
    }
    for (int cx = cx0; cx < cx1; cx++) {
      if (!wait_above(cy, cx - cx0 + 2)) return DEC_ERR_INVALID;
      const int ctu = cy * wc + cx;
      const uint8_t cut = free_slices ? job.ctb_cut[(size_t)ctu] : 0;
      if (skipping) {
        if (!(cut & 1)) { mark_missing(ctu); continue; }
        skipping = false;                                  // an independent segment begins: decoding goes on
      }
      if (cut & 3) {
        // a slice segment begins with this block: its own arithmetic codeword (the substream's first block: started above); an independent slice is a new
        // slice for every availability rule, starts from the initial context states and from its own SliceQpY; a dependent one goes on with the states at hand
        if (cx != cx0 || cy != first_cy) {
          const uint8_t *q = job.rbsp.data() + job.data_off + job.ctb_data[(size_t)ctu];
          if (q < data || q >= data + len) return DEC_ERR_INVALID;
          c.start(q, (size_t)(data + len - q));
        }
        if (cut & 1) {
          sp.cur_slice = job.ctb_slice[(size_t)ctu]; sp.slice_qp = job.slice_qps[(size_t)sp.cur_slice];
          init_contexts();
          sp.last_qp_y = sp.slice_qp;
        }
      }
      const uint32_t tu0 = (uint32_t)out.tus.size();
      sp.ctu_intra_mask = 0;
      if (!pps.cu_qp_delta) { sp.qp_y_pred = sp.slice_qp; sp.cu_qp_delta_val = 0; }
      if (sh.sao_luma || sh.sao_chroma) {                  // sao() (7.3.8.3) opens the CTU
        SaoParams *s = &job.sao[ctu];
        const SaoParams *left = cx > cx0 ? s - 1 : nullptr, *up = (cy > 0 && !tile_starts_at(cy)) ? s - wc : nullptr;
        if (free_slices) { if (left && job.ctb_slice[(size_t)ctu - 1] != sp.cur_slice) left = nullptr; if (up && job.ctb_slice[(size_t)ctu - wc] != sp.cur_slice) up = nullptr; }      // (merging stays inside the slice)
        parse_sao(c, *s, left, up, sh.sao_luma != 0, sh.sao_chroma != 0);
      }
      // (measurement aid, tools/measure/wpp_critical_path.py: KVAZZUP_AMD_CTU_DUMP=<file> -- picture, row, column, nanoseconds of every coding tree unit's parse)
      static const char *const ctu_dump = getenv("KVAZZUP_AMD_CTU_DUMP");
      std::chrono::steady_clock::time_point ctu_t0;
      if (__builtin_expect(ctu_dump != nullptr, 0)) ctu_t0 = std::chrono::steady_clock::now();
      sp.coding_quadtree(cx << ctbl_, cy << ctbl_, ctbl_, 0);
      if (__builtin_expect(ctu_dump != nullptr, 0)) {
        const long ns = (long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - ctu_t0).count();
        static FILE *const fp = fopen(ctu_dump, "w"); static std::mutex m;
        if (fp) { std::lock_guard<std::mutex> l(m); fprintf(fp, "%d %d %d %ld\n", job.sh.poc, cy, cx, ns); fflush(fp); }
      }
      if (sp.err) return sp.err;
      if (c.overrun()) return DEC_ERR_INVALID;
      job.ctu[ctu].first = tu0;
      job.ctu[ctu].count = ((uint32_t)out.tus.size() - tu0) | (sp.ctu_intra_mask << 24);
      if (out.tus.size() - tu0 >= (1u << 24)) return DEC_ERR_INVALID;
      if (wpp && cx == cx0 + 1) c.save_ctx(&job.wpp_saved[((size_t)cy * cols + g.tc) * CTX_COUNT]);
      if (((cut & 4) || scan) && wpp && free_slices && cx == cx1 - 1) c.save_ctx(&job.ds_saved[(size_t)cy * CTX_COUNT]);      // (a segment ends with the row: what a dependent segment that begins the next row may have to go on with)
      if (wpp) job.row_progress[(size_t)cy * cols + g.tc].v.store(cx - cx0 + 1, std::memory_order_release);
      // end_of_slice_segment_flag: 1 exactly where the picture's slice segments end (decode_slice noted the rows; one segment: the
      // last CTU of the picture); inside a segment a substream ends with end_of_subset_one_bit
      const bool seg_last = free_slices ? (cut & 4) != 0 : cx == cx1 - 1 && (cols > 1 ? (cy == g.cy1 - 1 && job.seg_end_sub[(size_t)sub]) : job.seg_end_row[(size_t)cy] != 0);
      const int end = c.terminate();
      if (end != (seg_last ? 1 : 0)) {
        if (scan && end == 1 && !job.ambiguous_end) skipping = true;      // (partial pictures: it ends before the next segment's address -- what lies between never arrived)
        else return seg_last ? DEC_ERR_INVALID : (job.ambiguous_end ? DEC_SEG_ENDS_EARLY : DEC_ERR_UNSUPPORTED);      // (a segment that ends elsewhere: not whole CTU rows / tiles)
      }
      if (!skipping && !seg_last && cx == cx1 - 1 && (wpp || tile_ends_at(cy)) && !c.terminate()) return DEC_ERR_INVALID;   // end_of_subset_one_bit
    }
    if (job.early_dst) {
      // the row's 4x4 records are final (a coding unit writes inside its own CTU only): up they go, from whichever thread parsed the row
      const size_t rowb = (size_t)(4 << (ctbl_ - 4)) * (pw_ / 4) * sizeof(B4Rec), off = (size_t)cy * rowb;      // (a CTB row: CTB / 4 rows of records)
      if (hipSetDevice(device_) == hipSuccess && hipMemcpyAsync(job.early_dst + off, job.h_in + off, rowb, hipMemcpyHostToDevice, stream_up_) == hipSuccess)
        job.early_rows.fetch_add(1, std::memory_order_acq_rel);
    }
    const int per16 = 1 << (ctbl_ - 4);                     // 16x16 blocks a CTB is wide
    if (ConcealMotion *cm = job.cown.get()) {
      // concealment v3 (decoder.h): this CTB row's motion, should the picture become the source of a stand-in -- list 0's if that list predicts the block, else list 1's
      for (int y16 = cy * per16; y16 < (cy + 1) * per16 && y16 < cm->h16; y16++)
        for (int x16 = cx0 * per16; x16 < cx1 * per16 && x16 < cm->w16; x16++) {
          const size_t i4 = (size_t)(y16 * 4) * (pw_ / 4) + x16 * 4;
          const B4Rec &m = job.b4[i4];
          ConcealMotion::E &o = cm->e[(size_t)y16 * cm->w16 + x16];
          o.none = 1;
          if (m.ref_idx < 0) continue;                         // intra
          if (sh.is_b) {
            const PicJob::MvF &f = job.mvf[i4];
            const int L = f.ref[0] >= 0 ? 0 : 1;
            if (f.ref[L] < 0) continue;
            o.mv[0] = f.mv[L][0]; o.mv[1] = f.mv[L][1]; o.ref_poc = L ? job.ref_poc1[f.ref[L] & 15] : job.ref_poc[f.ref[L] & 15]; o.lt = (L ? job.ref_lt1 : job.ref_lt)[f.ref[L] & 15] ? 1 : 0;
          } else { o.mv[0] = m.mvx; o.mv[1] = m.mvy; o.ref_poc = job.ref_poc[m.ref_idx & 15]; o.lt = job.ref_lt[m.ref_idx & 15] ? 1 : 0; }
          o.none = 0;
        }
    }
    // this CTB row's motion (the tile's columns of it) as later pictures see it (one entry per 16x16 block)
    if (!own) continue;
    for (int y16 = cy * per16; y16 < (cy + 1) * per16 && y16 < own->h16; y16++)
      for (int x16 = cx0 * per16; x16 < cx1 * per16 && x16 < own->w16; x16++) {
        const size_t i4 = (size_t)(y16 * 4) * (pw_ / 4) + x16 * 4;
        const B4Rec &m = job.b4[i4];
        ColMotion::Mv &o = own->mv[(size_t)y16 * own->w16 + x16];
        memset(&o, 0, sizeof(o));
        if (m.ref_idx < 0) continue;                           // intra
        if (sh.is_b) {
          const PicJob::MvF &f = job.mvf[i4];
          for (int L = 0; L < 2; L++) if (f.ref[L] >= 0) { o.used |= (uint8_t)(1 << L); o.mv[L][0] = f.mv[L][0]; o.mv[L][1] = f.mv[L][1]; o.ref_poc[L] = L ? job.ref_poc1[f.ref[L] & 15] : job.ref_poc[f.ref[L] & 15]; if ((L ? job.ref_lt1 : job.ref_lt)[f.ref[L] & 15]) o.lt |= (uint8_t)(1 << L); }
        } else { o.used = 1; o.mv[0][0] = m.mvx; o.mv[0][1] = m.mvy; o.ref_poc[0] = job.ref_poc[m.ref_idx & 15]; o.lt = job.ref_lt[m.ref_idx & 15] ? 1 : 0; }
      }
    if (own->row_cols[(size_t)cy].fetch_add(1, std::memory_order_acq_rel) + 1 >= own->cols) own->row_done[(size_t)cy].store(1, std::memory_order_release);
  }
  return 0;
}

int Decoder::parse_job(PicJob &job, bool row_parallel)
{
  const uint8_t *data = job.rbsp.data() + job.data_off; const size_t len = job.data_len;
  const int wc = ctbs_in(w_, ctbl_), hc = ctbs_in(h_, ctbl_), nsub = (int)job.geom.size(), cols = job.pps.tile_cols;
  auto release_all = [&] { if (job.own) for (int r = 0; r < hc; r++) job.own->row_done[(size_t)r].store(1, std::memory_order_release); };   // never leave a later picture's parser waiting
  // partial pictures v1 (decoder.h): the coding tree blocks that never arrived.  What is built lays out whole trailing CTB rows of a one-tile picture with WPP: their
  // substreams have no bytes and are not parsed -- skip_row gives the row the records that make every kernel do nothing there and publishes it
  std::vector<uint8_t> miss;
  int nrecv = nsub;
  const bool scan_rows = job.scan_gaps && job.pps.wpp != 0 && !job.ctb_cut.empty();      // (free slices with WPP: rows may have no bytes, every row gets the whole of the picture's)
  if (job.scan_gaps) { job.missing.clear(); job.miss_map.assign((size_t)wc * hc, 0); }      // (the parser finds what is missing -- parse_substream; a picture parsed again starts afresh)
  if (!job.missing.empty()) {
    miss.assign((size_t)wc * hc, 0);
    if (job.missing.size() != 1 || !job.pps.wpp || cols != 1 || nsub != hc || band_nrows_ > 0) { release_all(); return DEC_ERR_INVALID; }
    const int a = job.missing[0].first, n = job.missing[0].second;
    if (a <= 0 || a % wc != 0 || a + n != wc * hc) { release_all(); return DEC_ERR_INVALID; }
    memset(miss.data() + a, 1, (size_t)n);
    nrecv = a / wc;
  }
  if ((int)job.sub_start.size() != nrecv) { release_all(); return DEC_ERR_INVALID; }
  for (int r = 0; r < nrecv; r++) if (job.sub_start[(size_t)r] >= len && !(scan_rows && job.sub_start[(size_t)r] == SIZE_MAX)) { release_all(); return DEC_ERR_INVALID; }
  if (scan_rows && (int)job.row_seg_start.size() != hc) { release_all(); return DEC_ERR_INVALID; }
  job.subs.resize((size_t)nsub);
  for (auto &r : job.subs) { r.levels.clear(); r.tus.clear(); r.rc = 0; }
  job.wpp_saved.resize((size_t)hc * cols * CTX_COUNT);
  if (!job.row_progress || job.row_progress_n < hc * cols) { job.row_progress.reset(new Progress[(size_t)hc * cols]); job.row_progress_n = hc * cols; }
  for (int r = 0; r < hc * cols; r++) job.row_progress[(size_t)r].v.store(0, std::memory_order_relaxed);
  memset(job.region, 0, (size_t)(pw_ / 32) * (ph_ / 32) * sizeof(TuRange));
  memset(job.ctu, 0, nctb() * sizeof(TuRange));
  memset(job.pred_mode.data(), PM_NONE, job.pred_mode.size());
  auto skip_row = [&](int cy) {
    // rule 3: no coding units (PM_NONE stays: available to nothing), no transform blocks (job.ctu stays zero), records that are intra to the inter kernel and carry no
    // edge, SAO off, a slice byte of their own, no motion filed (ColMotion: like intra; ConcealMotion: none, as open_job left it)
    const int per = 1 << (ctbl_ - 2), b4w = pw_ / 4;
    B4Rec none; memset(&none, 0, sizeof(none)); none.ref_idx = -1;
    for (int k = 0; k < per; k++) for (int x = 0; x < b4w; x++) job.b4[(size_t)(cy * per + k) * b4w + x] = none;
    memset(job.ctu_tile + (size_t)cy * wc, 255, (size_t)wc);
    memset(&job.sao[(size_t)cy * wc], 0, (size_t)wc * sizeof(SaoParams));
    job.subs[(size_t)cy].rc = 0;
    job.row_progress[(size_t)cy].v.store(wc, std::memory_order_release);
    if (ColMotion *own = job.own.get()) {
      const int per16 = 1 << (ctbl_ - 4);
      for (int y16 = cy * per16; y16 < (cy + 1) * per16 && y16 < own->h16; y16++) memset(&own->mv[(size_t)y16 * own->w16], 0, (size_t)own->w16 * sizeof(ColMotion::Mv));
      own->row_cols[(size_t)cy].store((uint8_t)own->cols, std::memory_order_release); own->row_done[(size_t)cy].store(1, std::memory_order_release);
    }
  };
  auto one = [&](int r) {
    if (r >= nrecv) { skip_row(job.geom[(size_t)r].cy0); return; }
    if (band_nrows_ > 0 && (job.geom[(size_t)r].cy0 < band_row0_ || job.geom[(size_t)r].cy1 > band_row0_ + band_nrows_)) { job.subs[(size_t)r].rc = 0; return; }   // another decoder's rows
    size_t start = job.sub_start[(size_t)r], end = (r + 1 < nrecv) ? job.sub_start[(size_t)r + 1] : len;
    if (scan_rows) { start = 0; end = len; }
    int rc = end > start ? parse_substream(job, r, data + start, end - start, job.subs[(size_t)r]) : DEC_ERR_INVALID;
    job.subs[(size_t)r].rc = rc;
    if (rc < 0 && job.pps.wpp) job.row_progress[(size_t)job.geom[(size_t)r].cy0 * cols + job.geom[(size_t)r].tc].v.store(1 << 30, std::memory_order_release);   // release any waiter
    if (rc < 0) release_all();
  };
  if (row_parallel && nsub > 1) {
    if (!pool_) {
      const char *e = getenv("KVAZZUP_AMD_PARSE_THREADS");
      if (e) parse_threads_ = atoi(e) < 1 ? 1 : atoi(e);
      else if (frame_threads_ > 1 && parse_threads_ > 8) parse_threads_ = 8;      // beside the frame workers: measured best at 4K (2231 against 2085 frames/s with 16)
      pool_.reset(new OrderedPool(parse_threads_));
    }
    pool_->run(nsub, one);
  } else {
    for (int r = 0; r < nsub; r++) one(r);              // frame-parallel mode: substreams in sequence on this worker
  }
  // the substreams' transform blocks and level words follow the fixed part of the job's input block; table entries and word
  // offsets become picture-wide
  size_t ntu = 0, nlev = 0;
  for (auto &r : job.subs) { if (r.rc < 0) return r.rc; ntu += r.tus.size(); nlev += r.levels.size(); }
  // The layout is decided HERE, once; everything behind the parser reads job.lay.  (bi: the second vectors ride behind the level words.  CTBs smaller than 64: a 32x32 region's transform
  // blocks are no run of the list any more -- CTB 16: four CTBs of two CTB rows, i.e. of two substreams --, the regions get a list of INDICES into it behind everything else, DecFrame::tu_index.)
  const bool bi = (job.sh.is_b || job.sh.weighted) && job.any_bi.load(std::memory_order_relaxed) != 0;
  const DecInputLayout lay = job.lay = DecInputLayout(pw_, ph_, ctbl_, ntu, nlev, job.b4x.size(), bi);
  if (!grow_job_input(job, lay.upload_bytes())) return DEC_ERR_GPU;
  if (bi) memcpy(job.h_in + lay.x_off, job.b4x.data(), lay.nb4x * sizeof(B4L1));
  DecTu *tus = (DecTu *)(job.h_in + lay.tu_off); uint32_t *lev = (uint32_t *)(job.h_in + lay.lev_off);
  size_t t = 0, l = 0;
  for (int r = 0; r < nsub; r++) {
    SubOut &so = job.subs[(size_t)r];
    const int cy0 = job.geom[(size_t)r].cy0, cy1 = job.geom[(size_t)r].cy1, cx0 = job.geom[(size_t)r].cx0, cx1 = job.geom[(size_t)r].cx1;
    if (t) {
      for (int cy = cy0; cy < cy1; cy++) {
        for (int cx = cx0; cx < cx1; cx++) if (job.ctu[cy * wc + cx].count & 0xffffffu) job.ctu[cy * wc + cx].first += (uint32_t)t;
        if (ctbl_ == 6) for (int ry = 2 * cy; ry < 2 * cy + 2; ry++) for (int rx = 2 * cx0; rx < 2 * cx1; rx++) { TuRange &g = job.region[ry * 2 * wc + rx]; if (g.count) g.first += (uint32_t)t; }
      }
    }
    for (DecTu td : so.tus) { td.offset += (uint32_t)l; tus[t++] = td; }
    if (!so.levels.empty()) memcpy(lev + l, so.levels.data(), so.levels.size() * sizeof(uint32_t));
    l += so.levels.size();
  }
  if (ctbl_ < 6) {
    const int rw = pw_ >> 5, nreg = rw * (ph_ >> 5);
    auto region_of = [&](const DecTu &d) { const int X = d.plane ? d.x * 2 : d.x, Y = d.plane ? d.y * 2 : d.y; return (Y >> 5) * rw + (X >> 5); };
    for (int g = 0; g < nreg; g++) { job.region[g].first = 0; job.region[g].count = 0; }
    for (size_t k = 0; k < ntu; k++) job.region[region_of(tus[k])].count++;
    uint32_t at = 0;
    for (int g = 0; g < nreg; g++) { job.region[g].first = at; at += job.region[g].count; job.region[g].count = 0; }
    uint32_t *idx = (uint32_t *)(job.h_in + lay.i_off);
    for (size_t k = 0; k < ntu; k++) { TuRange &g = job.region[region_of(tus[k])]; idx[g.first + g.count++] = (uint32_t)k; }      // (list order = decoding order inside a region)
  }
  job.ntu = ntu; job.nlev = nlev;
  if (job.scan_gaps) {      // gaps found by the parser: the runs, in raster order; their boundaries are closed like the row form's
    for (int a = 0; a < wc * hc; a++) if (job.miss_map[(size_t)a]) { if (!job.missing.empty() && job.missing.back().first + job.missing.back().second == a) job.missing.back().second++; else job.missing.emplace_back(a, 1); }
    if (!job.missing.empty()) { miss = job.miss_map; job.lf_restricted = true; }
  }
  if (job.lf_restricted) {
    // ---- closed slice / tile boundaries (PicJob::lf_restricted).  Every coding tree block's slice: the slices are runs of the DECODING order (tile after tile), so the
    // walk goes through the substreams' geometry; then per block which of its eight neighbours the in-loop filters may use -- not across a tile boundary when the
    // PPS says so, not across a slice boundary when the LATER of the two slices says so (its left and upper boundaries are the closed ones, 7.4.7.1).  SAO reads the
    // map; deblocking needs none: an edge on a closed boundary is no edge (8.7.2.3 filterEdgeFlag = 0), its marks come off the records here.
    const int n = wc * hc;
    std::vector<int> order((size_t)n, 0), slice((size_t)n, 0);
    {
      int ts = 0, cur = -1; size_t next = 0;
      for (const PicJob::SubGeom &g : job.geom)
        for (int cy = g.cy0; cy < g.cy1; cy++)
          for (int cx = g.cx0; cx < g.cx1; cx++) {
            const int a = cy * wc + cx;
            while (next < job.lf_slices.size() && job.lf_slices[next].first == a) { cur = (int)next; next++; }      // (a slice begins with this block)
            order[(size_t)a] = ts++; slice[(size_t)a] = cur < 0 ? 0 : cur;
          }
      if (next != job.lf_slices.size()) return DEC_ERR_INVALID;                      // (a slice that begins where no substream's walk comes by)
    }
    uint8_t *nb = job.h_in + lay.nb_off;
    const int per = 1 << (ctbl_ - 2), b4w = pw_ / 4;
    for (int cy = 0; cy < hc; cy++)
      for (int cx = 0; cx < wc; cx++) {
        const int c = cy * wc + cx; uint8_t m = 0xff;
        for (int dy = -1; dy <= 1; dy++)
          for (int dx = -1; dx <= 1; dx++) {
            const int nx = cx + dx, ny = cy + dy;
            if ((!dx && !dy) || nx < 0 || ny < 0 || nx >= wc || ny >= hc) continue;
            const int q = ny * wc + nx, later = order[(size_t)q] > order[(size_t)c] ? q : c;
            const bool closed = (job.ctu_tile[c] != job.ctu_tile[q] && !job.pps.across_tiles && job.ctb_cut.empty()) ||      // (free slices: the byte holds the slice, there is one tile)
                                (!miss.empty() && (miss[(size_t)c] || miss[(size_t)q])) ||                                     // (partial pictures: a missing block is closed on every side, and on the neighbours' side)
                                (!job.lf_slices.empty() && slice[(size_t)c] != slice[(size_t)q] && !job.lf_slices[(size_t)slice[(size_t)later]].second);
            const int k = (dy + 1) * 3 + (dx + 1);
            if (closed) m &= (uint8_t)~(1u << (k > 4 ? k - 1 : k));
          }
        nb[c] = m;
        if (!(m & (1u << 3))) for (int k = 0; k < per && (cy * per + k) * 4 < h_; k++) job.b4[(size_t)(cy * per + k) * b4w + cx * per].flags &= (uint8_t)~(B4_EDGE_V | B4_TU_V);      // W
        if (!(m & (1u << 1))) for (int k = 0; k < per && (cx * per + k) * 4 < w_; k++) job.b4[(size_t)(cy * per) * b4w + cx * per + k].flags &= (uint8_t)~(B4_EDGE_H | B4_TU_H);      // N
      }
  }
  return 0;
}

}  // namespace kvzx
