// kvazzup_amd/csrc/loop_kernels.hip -- CDNA4 (gfx950) kernels of the HEVC encoder hot path: per-CTU QP bookkeeping, deblocking, SAO
// (enc_kernels.hip has the introduction; the launch wrappers of these kernels are at the end).  Nothing here shares a helper of its own with the other two
// files, and no kernel's machine code was seen to depend on these being beside it.
//
// Launch geometry (coded size is a multiple of 64; DESIGN.md section 5 has the table with timings):
//   k_qp_first/chain  per-CTU QP bookkeeping (cu_qp_delta)
//   k_deblock_tile  one workgroup per 64x64 tile shifted by (-4, -4): vertical then horizontal edges in LDS
//                   (k_deblock_v / k_deblock_h: one thread per 4-sample edge segment, band mode of the tile-row split)
//   k_sao           one workgroup per CTU: statistics + decision and the filter
#include <hip/hip_runtime.h>
#include <type_traits>
#include "hevc_core.h"
#include "enc_kernels.h"
#include "kernel_common.h"

namespace kvzx {

// =============================================================================================
// Per-CTU QP (delta-QP map): after reconstruction, which CU of every CTU is the first with residual, and from that the
// QpY every CU ends up with (H.265 8.6.1, quantisation group = CTU: the prediction is the QpY of the previous CTU in
// decoding order, or the slice QP at the start of a tile and -- with WPP -- of a CTU row).  Statement: roi_resolve() in
// oracle/hevc_enc.c.
// =============================================================================================
__global__ __launch_bounds__(64) void k_qp_first(EncFrame f)                // one wave per CTU of the band
{
  const int wc = f.cw >> 6, ctu = blockIdx.x + f.row0 * wc, cx = ctu % wc, cy = ctu / wc, lane = threadIdx.x;
  int xi, yi; ctu_z_to_xy(lane, xi, yi);
  const int x = cx * 64 + xi * 8, y = cy * 64 + yi * 8, bi = b8idx(f, x, y), n = 1 << f.cu_log2[bi];
  const bool coded_origin = !((x | y) & (n - 1)) && f.cu_cbf[bi] != 0;
  const uint64_t m = __ballot(coded_origin);
  if (lane == 0) f.ctu_first[ctu] = (uint8_t)(m ? __builtin_ctzll(m) : 64);
}
__global__ __launch_bounds__(256) void k_qp_chain(EncFrame f)                // one thread per CTU of the band
{
  const int wc = f.cw >> 6, hc = f.ch >> 6, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= wc * band_rows(f)) return;
  const int ctu = t + f.row0 * wc, cx = ctu % wc, cy = ctu / wc;
  // QpY of the nearest CTU at or before this one in its chain that codes a delta; the chain runs in decoding order (tile scan) and
  // starts at the CTU row of the tile (WPP) or at the tile
  const int tc = tile_col_of(wc, f.tile_cols, cx), cx0 = tile_col_first(wc, f.tile_cols, tc), cx1 = tile_col_first(wc, f.tile_cols, tc + 1);
  const int first_cy = f.wpp ? cy : tile_row_first(hc, f.tile_rows, tile_row_of(hc, f.tile_rows, cy));
  int qy = f.qp, prev = f.qp; bool have = false, have_prev = false;
  for (int y = cy, x = cx; y >= first_cy && !have_prev; y--, x = cx1 - 1)
    for (; x >= cx0; x--) {
      const int c = y * wc + x;
      if (f.ctu_first[c] < 64) {
        if (c == ctu) { qy = f.ctu_qt[c]; have = true; }
        else { prev = f.ctu_qt[c]; have_prev = true; break; }
      }
    }
  (void)have_prev;
  if (!have) qy = prev;
  f.ctu_qy[ctu] = (int8_t)qy;
  f.ctu_delta[ctu] = (int8_t)(have ? qy - prev : 0);
}

// The two kernels above as ONE launch where the chain of a CTU never leaves its CTU row -- WPP (uvgComm's default, kvazaarfilter.cpp:194): the QpY prediction
// restarts with the slice QP at every CTU row of a tile.  A workgroup per CTU row: its waves find the rows' first coded units (one CTU per wave at a time), then
// a thread per CTU walks back along the row inside its tile.  Same results as k_qp_first + k_qp_chain (the launch is one of ten on a P picture's chain in
// uvgComm's default mode, each worth ~6 us whatever it does).
__global__ __launch_bounds__(256) void k_qp_rows(EncFrame f)
{
  __shared__ uint8_t first_s[256];                           // (a CTU row: at most 16384 / 64 CTUs)
  const int wc = f.cw >> 6, cy = blockIdx.x + f.row0, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int xi, yi; ctu_z_to_xy(lane, xi, yi);
  for (int cx = wave; cx < wc; cx += 4) {
    const int x = cx * 64 + xi * 8, y = cy * 64 + yi * 8, bi = b8idx(f, x, y), n = 1 << f.cu_log2[bi];
    const bool coded_origin = !((x | y) & (n - 1)) && f.cu_cbf[bi] != 0;
    const uint64_t m = __ballot(coded_origin);
    if (lane == 0) { const uint8_t v = (uint8_t)(m ? __builtin_ctzll(m) : 64); first_s[cx] = v; f.ctu_first[cy * wc + cx] = v; }
  }
  __syncthreads();
  for (int cx = threadIdx.x; cx < wc; cx += 256) {
    const int ctu = cy * wc + cx;
    const int tc = tile_col_of(wc, f.tile_cols, cx), cx0 = tile_col_first(wc, f.tile_cols, tc);
    int qy = f.qp, prev = f.qp; bool have = false;
    for (int x = cx; x >= cx0; x--) {
      if (first_s[x] < 64) {
        if (x == cx) { qy = f.ctu_qt[ctu]; have = true; }
        else { prev = f.ctu_qt[cy * wc + x]; break; }
      }
    }
    if (!have) qy = prev;
    f.ctu_qy[ctu] = (int8_t)qy;
    f.ctu_delta[ctu] = (int8_t)(have ? qy - prev : 0);
  }
}

// =============================================================================================
// Deblocking: all vertical edges of the picture, then (second launch) all horizontal edges
// =============================================================================================
// Both deblocking passes in one launch (whole pictures; the band mode of the tile-row split keeps the two kernels below: it
// exchanges halo rows between them).  A workgroup owns the 64x64 tile shifted by (-4, -4) against the CTU grid: every sample
// a vertical edge x = 64 tx + 8 e or a horizontal edge y = 64 ty + 8 e of this CTU can modify (three each side) or read (four)
// lies inside the tile, and the tiles partition the picture -- so the tile goes to LDS once, is filtered vertically, then
// horizontally on the vertically filtered samples (8.7.2: the whole picture's vertical edges come first), and goes back.
__global__ __launch_bounds__(256) void k_deblock_tile(EncFrame f)
{
  constexpr int P = 80, PC = 48;                           // LDS pitches: 68 (36) used, multiples of 16 so that the 16-byte pieces stay aligned
  __shared__ __attribute__((aligned(16))) uint8_t ty_[68 * P];
  __shared__ __attribute__((aligned(16))) uint8_t tc_[2][34 * PC];
  // the CU records of the tile's 8x8 cells and one ring around them (cells -1 .. 8 in both directions): everything the boundary
  // strength needs, fetched in one go beside the samples instead of per edge segment
  __shared__ uint8_t r_log2[100], r_intra[100], r_cbf[100], r_ref[100]; __shared__ uint32_t r_mv[100];
  const int tid = threadIdx.x, wc = f.cw >> 6, hc = f.ch >> 6;
  if (f.me_cand && blockIdx.x == 0 && tid == 0) { f.me_cand[0] = 0; f.sync[(size_t)3 * wc * hc + 1] = 0; }      // intra-in-P: the next picture's k_me starts its list of candidate blocks from nothing, its "has intra units" word from zero
  const int lin = xcd_contiguous((int)blockIdx.x, (int)gridDim.x), tx = lin % wc, tyi = lin / wc;
  const int X0 = tx * 64 - 4, Y0 = tyi * 64 - 4, CX0 = X0 >> 1, CY0 = Y0 >> 1, cw2 = f.cw >> 1;
  const int TW = tx == wc - 1 ? 68 : 64, TH = tyi == hc - 1 ? 68 : 64;
  if (tid < 100) {
    const int bx = tx * 8 - 1 + tid % 10, by = tyi * 8 - 1 + tid / 10;
    uint32_t l2 = 6, in = 0, cb = 0, mv = 0, rf = 0;
    if (bx >= 0 && by >= 0 && bx < f.b8w && by < f.b8h) {
      const int i = by * f.b8w + bx;
      l2 = f.cu_log2[i]; in = f.cu_intra[i]; cb = f.cu_cbf[i]; mv = *(const uint32_t *)&f.cu_mv[i * 2]; rf = (uint32_t)cu_ref_at(f, i);
    }
    r_log2[tid] = (uint8_t)l2; r_intra[tid] = (uint8_t)in; r_cbf[tid] = (uint8_t)cb; r_mv[tid] = mv; r_ref[tid] = (uint8_t)rf;
  }
  __syncthreads();
  auto cell = [&](int x, int y) { return ((y >> 3) - (tyi * 8 - 1)) * 10 + ((x >> 3) - (tx * 8 - 1)); };
  auto bs_of = [&](int cp, int cq) -> int {
    if (r_intra[cp] | r_intra[cq]) return 2;
    if ((r_cbf[cp] | r_cbf[cq]) & 1) return 1;
    if (r_ref[cp] != r_ref[cq]) return 1;                              // different reference pictures (lp-refs)
    const uint32_t a = r_mv[cp], b = r_mv[cq];
    if (iabs((int)(int16_t)(a & 0xffff) - (int)(int16_t)(b & 0xffff)) >= 4 || iabs((int)(int16_t)(a >> 16) - (int)(int16_t)(b >> 16)) >= 4) return 1;
    return 0;
  };
  // ---- boundary strengths of this thread's vertical and horizontal edge segment, from the records alone.  A tile none of whose
  // segments is filtered (still background: large units, equal vectors, no coefficients) leaves without touching a sample.
  int bsv = 0, bsh = 0, qpv = 0, qph = 0;
  if (tid < 8 * (TH / 4)) {
    const int x = tx * 64 + (tid & 7) * 8, y = Y0 + (tid >> 3) * 4;
    if (x > 0 && y >= 0) {
      const int cq = cell(x, y), cp = cq - 1;
      if ((x & ((1 << r_log2[cq]) - 1)) == 0) {
        bsv = bs_of(cp, cq);
        if (bsv) qpv = f.ctu_qy ? (cu_qpy(f, x - 1, y) + cu_qpy(f, x, y) + 1) >> 1 : f.qp;      // QpP and QpQ averaged (8.7.2.5.3)
      }
    }
  }
  if (tid < 8 * (TW / 4)) {
    const int y = tyi * 64 + (tid & 7) * 8, x = X0 + (tid >> 3) * 4;
    if (y > 0 && x >= 0) {
      const int cq = cell(x, y), cp = cq - 10;
      if ((y & ((1 << r_log2[cq]) - 1)) == 0) {
        bsh = bs_of(cp, cq);
        if (bsh) qph = f.ctu_qy ? (cu_qpy(f, x, y - 1) + cu_qpy(f, x, y) + 1) >> 1 : f.qp;
      }
    }
  }
  if (!__syncthreads_or(bsv | bsh)) return;
  // ---- tile in: 16-byte pieces (X0 is 4-byte aligned: dwordx4 with dword alignment), the last piece of a 68-wide row 4 bytes
  for (int i = tid; i < TH * 5; i += 256) {
    const int y = i / 5, k = i - y * 5, x = k * 16, gx = X0 + x, gy = Y0 + y;
    if (gy < 0 || x >= TW) continue;
    const uint8_t *g = &f.rec[0][(size_t)gy * f.cw + gx];
    if (k < 4) { if (gx >= 0) *(kv_u32x4 *)&ty_[y * P + x] = *(const kv_u32x4 *)g; else { kv_u32x4 v; v.x = 0; v.y = *(const uint32_t *)(g + 4); v.z = *(const uint32_t *)(g + 8); v.w = *(const uint32_t *)(g + 12); *(kv_u32x4 *)&ty_[y * P + x] = v; } }
    else *(uint32_t *)&ty_[y * P + x] = *(const uint32_t *)g;
  }
  // chroma: aligned dwords from two samples left of the tile (CX0 - 2 is a multiple of 4): sample x of the tile sits at LDS column x + 2
  for (int i = tid; i < 2 * (TH / 2) * 9; i += 256) {
    const int pl = i / ((TH / 2) * 9), r = i - pl * ((TH / 2) * 9), y = r / 9, k = r - y * 9, gx = CX0 - 2 + 4 * k, gy = CY0 + y;
    if (gy >= 0 && gx >= 0) *(uint32_t *)&tc_[pl][y * PC + 4 * k] = *(const uint32_t *)&f.rec[1 + pl][(size_t)gy * cw2 + gx];
  }
  __syncthreads();
  // ---- vertical edges: 8 edges x 16 (17) four-row segments
  if (bsv) {
    const int x = tx * 64 + (tid & 7) * 8, y = Y0 + (tid >> 3) * 4;
    deblock_luma_segment(&ty_[(y - Y0) * P + (x - X0)], 1, P, bsv, qpv);
    if (bsv == 2 && (x & 15) == 0) {
      const int o = ((y >> 1) - CY0) * PC + ((x >> 1) - CX0) + 2;
      deblock_chroma_segment(&tc_[0][o], 1, PC, 2, qpv);
      deblock_chroma_segment(&tc_[1][o], 1, PC, 2, qpv);
    }
  }
  __syncthreads();
  // ---- horizontal edges: 8 edges x 16 (17) four-column segments, on the vertically filtered samples
  if (bsh) {
    const int y = tyi * 64 + (tid & 7) * 8, x = X0 + (tid >> 3) * 4;
    deblock_luma_segment(&ty_[(y - Y0) * P + (x - X0)], P, 1, bsh, qph);
    if (bsh == 2 && (y & 15) == 0) {
      const int o = ((y >> 1) - CY0) * PC + ((x >> 1) - CX0) + 2;
      deblock_chroma_segment(&tc_[0][o], PC, 1, 2, qph);
      deblock_chroma_segment(&tc_[1][o], PC, 1, 2, qph);
    }
  }
  __syncthreads();
  // ---- tile out
  for (int i = tid; i < TH * 5; i += 256) {
    const int y = i / 5, k = i - y * 5, x = k * 16, gx = X0 + x, gy = Y0 + y;
    if (gy < 0 || x >= TW) continue;
    uint8_t *g = &f.rec[0][(size_t)gy * f.cw + gx];
    if (k < 4) {
      const kv_u32x4 v = *(const kv_u32x4 *)&ty_[y * P + x];
      if (gx >= 0) *(kv_u32x4 *)g = v; else { *(uint32_t *)(g + 4) = v.y; *(uint32_t *)(g + 8) = v.z; *(uint32_t *)(g + 12) = v.w; }
    } else *(uint32_t *)g = *(const uint32_t *)&ty_[y * P + x];
  }
  for (int i = tid; i < 2 * (TH / 2) * 9; i += 256) {
    const int pl = i / ((TH / 2) * 9), r = i - pl * ((TH / 2) * 9), y = r / 9, k = r - y * 9, gx = CX0 - 2 + 4 * k, gy = CY0 + y;
    if (gy < 0 || gx < 0) continue;
    uint8_t *g = &f.rec[1 + pl][(size_t)gy * cw2 + gx];
    const uint32_t v = *(const uint32_t *)&tc_[pl][y * PC + 4 * k];
    if (k == 0) *(uint16_t *)(g + 2) = (uint16_t)(v >> 16);                 // the first two bytes belong to the tile on the left
    else if (k == 8 && TW == 64) *(uint16_t *)g = (uint16_t)v;              // ... the last two to the tile on the right
    else *(uint32_t *)g = v;
  }
}

__global__ __launch_bounds__(256) void k_deblock_v(EncFrame f)
{
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  int ne = (f.cw >> 3) - 1, ns = band_rows(f) * 16;    // edges per row of segments, segment rows of the band
  if (t >= ne * ns) return;
  int x = ((t % ne) + 1) * 8, y = (t / ne) * 4 + f.row0 * 64;
  if (!is_cu_edge_v(f, x, y)) return;
  int bs = edge_bs(f, x - 1, y, x, y);
  if (!bs) return;
  const int qp = (cu_qpy(f, x - 1, y) + cu_qpy(f, x, y) + 1) >> 1;            // QpP and QpQ averaged (8.7.2.5.3)
  deblock_luma_segment(f.rec[0] + y * f.cw + x, 1, f.cw, bs, qp);
  if (bs == 2 && (x & 15) == 0) {
    int cw2 = f.cw >> 1;
    deblock_chroma_segment(f.rec[1] + (y >> 1) * cw2 + (x >> 1), 1, cw2, 2, qp);
    deblock_chroma_segment(f.rec[2] + (y >> 1) * cw2 + (x >> 1), 1, cw2, 2, qp);
  }
}
// part: 0 = every horizontal edge of the band, 1 = the edges inside it (they need nothing from the neighbouring bands), 2 = its two
// boundary edges (after the halo rows have arrived).  Horizontal edges lie 8 rows apart and change at most 3 rows on either side:
// the order in which they are filtered does not matter.
__global__ __launch_bounds__(256) void k_deblock_h(EncFrame f, int part)
{
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  // horizontal edges of the band: every 8 rows from its first row (when that is not the picture's) to its end (likewise);
  // the two boundary edges are filtered by both neighbours, each keeping its own side (halo rows hold the other's samples)
  const int ylo = imax(8, f.row0 * 64), yhi = imin(f.ch - 8, (f.row0 + band_rows(f)) * 64);
  int ns = f.cw >> 2, ne = (yhi - ylo) / 8 + 1;
  if (t >= ne * ns) return;
  int x = (t % ns) * 4, y = ylo + (t / ns) * 8;
  if (part) {
    const bool boundary = y == f.row0 * 64 || y == (f.row0 + band_rows(f)) * 64;
    if (boundary != (part == 2)) return;
  }
  if (!is_cu_edge_h(f, x, y)) return;
  int bs = edge_bs(f, x, y - 1, x, y);
  if (!bs) return;
  const int qp = (cu_qpy(f, x, y - 1) + cu_qpy(f, x, y) + 1) >> 1;
  deblock_luma_segment(f.rec[0] + y * f.cw + x, f.cw, 1, bs, qp);
  if (bs == 2 && (y & 15) == 0) {
    int cw2 = f.cw >> 1;
    deblock_chroma_segment(f.rec[1] + (y >> 1) * cw2 + (x >> 1), cw2, 1, 2, qp);
    deblock_chroma_segment(f.rec[2] + (y >> 1) * cw2 + (x >> 1), cw2, 1, 2, qp);
  }
}

// =============================================================================================
// Sample adaptive offset (8.7.3).  One workgroup per CTU: the deblocked CTU with a one-sample border goes to LDS for all
// three components.  Statistics against the source picture and "uvgx SAO decision v1" (statement of record:
// oracle/hevc_sao.c), parameters out, and the filtered CTU goes to the output picture.  (The decoder's SAO is dec_kernels.hip's.)
// =============================================================================================
#define KVZ_SAO_THREADS 1024   // (a CTU's workgroup is alone on its compute unit in uvgComm's default mode: four waves per SIMD hide what one wave waited for -- tools/sao_timeline.py)
struct SaoLds {
  // the deblocked CTU with a one-sample border, one padded picture per component: sample (x, y), x and y in -1 .. n, at
  // [(y + 1) * pitch + 4 + x]; pitch 72 / 40 keeps the CTB's own samples dword aligned
  alignas(4) uint8_t win[66 * 72];
  alignas(4) uint8_t winc[2][34 * 40];
  int en[3][4][5], es[3][4][5], bn[3][32][16], bs[3][32][16];      // (band statistics in 16 copies, by lane: neighbouring columns mostly fall into the same band, and LDS atomics on one address go one after the other)
  int eo_off[3][4][4], eo_dist[3][4][4], bo_off[3][32], bo_gain[3][32];
  int cand_dist[3][5], cand_bins[3][5], cand_band[3];
  SaoParams p;
};
__device__ __forceinline__ int sao_edge_idx(int c, int a, int b)
{
  const int e = 2 + ((c > a) - (c < a)) + ((c > b) - (c < b));
  return e == 2 ? 0 : (e < 2 ? e + 1 : e);
}
__device__ __forceinline__ int sao_rdiv(int a, int b) { return b == 0 ? 0 : (a >= 0 ? (2 * a + b) / (2 * b) : -((-2 * a + b) / (2 * b))); }
__device__ __forceinline__ int sao_off_bins(int o) { const int a = o < 0 ? -o : o; return a < 7 ? a + 1 : 7; }

// Statistics of one piece of a column of a CTB (ROWS rows from row ys of column x) with the 3 x 3 neighbourhood in registers.  Edge classes: four packed
// accumulators (see inside), reduced over the wave with DPP at the end -- one LDS atomic per wave and statistic.  Bands: runs of equal band index along the
// column are summed in registers and flushed when the band changes.  o8: the source samples of the piece (fetched by the caller long before).
template <int ROWS>
__device__ __forceinline__ void sao_stats_column(SaoLds &s, int c, const uint8_t *w, int pitch, int x, int ys, bool okh, int Y0, int ph, const int *o8, int tid)
{
  // the sign of a difference as med3(d, -1, 1); the edge index e = 2 + sign(c - a) + sign(c - b) is 0, 1 / 3, 4 for the categories 1, 2 / 3, 4 (2: none)
  auto sgn = [](int d) { return d > 1 ? 1 : (d < -1 ? -1 : d); };
  const uint8_t *col = w + 4 + x - 1;                                   // column x - 1 of window row 0 (= sample row -1)
  int r0[3], r1[3], r2[3];
  for (int k = 0; k < 3; k++) { r0[k] = col[ys * pitch + k]; r1[k] = col[(ys + 1) * pitch + k]; }
  // per class one 64-bit accumulator with four 16-bit fields, one per category: sum of (d + 256) + 2048 per sample -- the count rides above the sum
  // (ROWS <= 4: sum <= 4 * 511 < 2048)
  uint64_t acc[4] = {0, 0, 0, 0};
  int run_b = -1, run_n = 0, run_s = 0;
  int s_up = sgn(r1[1] - r0[1]);                                        // sign(c - above) of the row to come
#pragma unroll
  for (int j = 0; j < ROWS; j++) {
    const int y = ys + j;
    for (int k = 0; k < 3; k++) r2[k] = col[(y + 2) * pitch + k];
    const int v = r1[1], d = o8[j] - v, b = v >> 3;
    if (b != run_b) {
      if (run_n) { atomicAdd(&s.bn[c][run_b][tid & 15], run_n); atomicAdd(&s.bs[c][run_b][tid & 15], run_s); }
      run_b = b; run_n = 0; run_s = 0;
    }
    run_n++; run_s += d;
    const bool okv = Y0 + y - 1 >= 0 && Y0 + y + 1 < ph;
    const int s_dn = sgn(v - r2[1]);
    const int ea = okh ? 2 + sgn(v - r1[0]) + sgn(v - r1[2]) : 2, eb = okv ? 2 + s_up + s_dn : 2;
    const int ec = (okh && okv) ? 2 + sgn(v - r0[0]) + sgn(v - r2[2]) : 2, ed = (okh && okv) ? 2 + sgn(v - r0[2]) + sgn(v - r2[0]) : 2;
    const int ee[4] = {ea, eb, ec, ed};
    const uint32_t val = (uint32_t)(d + 256 + 2048);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e] += (uint64_t)(ee[e] == 2 ? 0u : val) << (16 * (ee[e] - (ee[e] > 2)));
    s_up = -s_dn;                                                       // the next row's sign(c - above)
    for (int k = 0; k < 3; k++) { r0[k] = r1[k]; r1[k] = r2[k]; }
  }
  if (run_n) { atomicAdd(&s.bn[c][run_b][tid & 15], run_n); atomicAdd(&s.bs[c][run_b][tid & 15], run_s); }
#pragma unroll
  for (int e = 0; e < 4; e++)
#pragma unroll
    for (int k = 1; k <= 4; k++) {
      // one reduction for both: the wave's count (<= 64 * ROWS) above bit 20, its biased sum (<= 64 * ROWS * 511) below
      const uint32_t fld = (uint32_t)(acc[e] >> (16 * (k - 1))) & 0xffffu, cnt = fld >> 11, sum = fld & 2047u;
      const uint32_t r = wave_sum_u32((cnt << 20) | sum), N = r >> 20, S = r & 0xfffffu;
      if ((tid & 63) == 0) { atomicAdd(&s.en[c][e][k], (int)N); atomicAdd(&s.es[c][e][k], (int)S - 256 * (int)N); }
    }
}

// IR (encoder, intra-refresh): the coding tree blocks that hold luma column ir_e - 5 leave luma SAO off.  Deblocking the band's end against what
// lies beyond it changes three columns left of it, and through the horizontal edges' decisions (taken per four columns) a fourth; an edge class of SAO would
// carry that one column further.  With luma SAO off there the columns < ir_e - 4 of a picture are what a decoder that lost a picture makes of them as well.  A
// form of its own: the launches without the option run the code of before.
template <bool IR = false>
__global__ __launch_bounds__(KVZ_SAO_THREADS) void k_sao(EncFrame f)
{
  __shared__ SaoLds s;
  const int tid = threadIdx.x, wc = f.cw >> 6, ctu = xcd_contiguous((int)blockIdx.x, (int)gridDim.x), cx = ctu % wc, cy = ctu / wc;
  unsigned long long *tr = (f.trace && tid == 0) ? f.trace + (size_t)wc * (f.ch >> 6) * 56 + (size_t)ctu * 16 : nullptr;      // (tools/sao_timeline.py)
#define SAO_STAMP(k) do { if (tr) tr[k] = wall_clock64(); } while (0)
  SAO_STAMP(0);
  constexpr int T = KVZ_SAO_THREADS;
  // the source samples of this thread's pieces of columns (sao_stats_column): in flight while the window is fetched
  const int lx = tid & 63, lys = (tid >> 6) * 4;                                         // luma: column lx, rows lys .. lys + 3
  const int cc = 1 + (tid >> 9), cxx = tid & 31, cys = ((tid & 511) >> 5) * 2;           // chroma component cc: column cxx, rows cys, cys + 1
  int o8l[4], o8c[2];
  const uint8_t *ol = f.src[0] + (size_t)(cy * 64 + lys) * f.cw + cx * 64 + lx, *oc = f.src[cc] + (size_t)(cy * 32 + cys) * (f.cw >> 1) + cx * 32 + cxx;
#pragma unroll
  for (int j = 0; j < 4; j++) o8l[j] = ol[(size_t)j * f.cw];
#pragma unroll
  for (int j = 0; j < 2; j++) o8c[j] = oc[(size_t)j * (f.cw >> 1)];
  // ---- window: the CTB's samples as dwords, the border ring byte by byte (clamped at the picture edges; those samples are
  // never used: a neighbour outside the picture switches the edge offset off)
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int sh = c ? 1 : 0, l2n = 6 - sh, n = 1 << l2n, pw = f.cw >> sh, ph = f.ch >> sh, X0 = cx * n, Y0 = cy * n;
    uint8_t *w = c ? s.winc[c - 1] : s.win; const int pitch = c ? 40 : 72;
    const uint8_t *src = f.rec[c];
#pragma unroll
    for (int i = tid; i < n * n / 4; i += T) {
      const int y = i >> (l2n - 2), x = (i & ((n >> 2) - 1)) * 4;
      *(uint32_t *)&w[(y + 1) * pitch + 4 + x] = *(const uint32_t *)&src[(size_t)(Y0 + y) * pw + X0 + x];
    }
    for (int q = tid; q < 4 * n + 4; q += T) {
      int x, y;
      if (q < n + 2) { x = q - 1; y = -1; } else if (q < 2 * n + 4) { x = q - (n + 2) - 1; y = n; }
      else if (q < 3 * n + 4) { x = -1; y = q - (2 * n + 4); } else { x = n; y = q - (3 * n + 4); }
      w[(y + 1) * pitch + 4 + x] = src[(size_t)clip3(0, ph - 1, Y0 + y) * pw + clip3(0, pw - 1, X0 + x)];
    }
  }
  for (int i = tid; i < (int)((sizeof(s.en) + sizeof(s.es) + sizeof(s.bn) + sizeof(s.bs)) / sizeof(int)); i += T) (&s.en[0][0][0])[i] = 0;
  __syncthreads();
  SAO_STAMP(1);
  // Statistics: sao_stats_column -- the luma CTB's columns in pieces of four rows over all 1024 threads, then both chroma CTBs' in pieces of two
  sao_stats_column<4>(s, 0, s.win, 72, lx, lys, cx * 64 + lx - 1 >= 0 && cx * 64 + lx + 1 < f.cw, cy * 64, f.ch, o8l, tid);
  sao_stats_column<2>(s, cc, s.winc[cc - 1], 40, cxx, cys, cx * 32 + cxx - 1 >= 0 && cx * 32 + cxx + 1 < (f.cw >> 1), cy * 32, f.ch >> 1, o8c, tid);
  __syncthreads();
  SAO_STAMP(2);
  if (tid < 48) {                                       // edge offsets: component x class x category
    const int c = tid >> 4, e = (tid >> 2) & 3, k = (tid & 3) + 1, N = s.en[c][e][k], S = s.es[c][e][k];
    int o = sao_rdiv(S, N);
    o = k <= 2 ? clip3(0, 7, o) : clip3(-7, 0, o);
    s.eo_off[c][e][k - 1] = o; s.eo_dist[c][e][k - 1] = N * o * o - 2 * o * S;
  } else if (tid >= 64 && tid < 160) {                  // band offsets: component x band
    const int c = (tid - 64) >> 5, b = (tid - 64) & 31;
    int N = 0, S = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { N += s.bn[c][b][k]; S += s.bs[c][b][k]; }
    const int o = clip3(-7, 7, sao_rdiv(S, N));
    s.bo_off[c][b] = o; s.bo_gain[c][b] = N * o * o - 2 * o * S;
  }
  __syncthreads();
  if (tid < 15) {                                       // candidates: component x [EO 0..3, BO]
    const int c = tid / 5, j = tid - c * 5;
    int dist = 0, bins = 0;
    if (j < 4) { for (int k = 0; k < 4; k++) { dist += s.eo_dist[c][j][k]; bins += sao_off_bins(s.eo_off[c][j][k]); } }
    else {
      int best = 0;
      for (int st = 0; st <= 28; st++) {
        const int g = s.bo_gain[c][st] + s.bo_gain[c][st + 1] + s.bo_gain[c][st + 2] + s.bo_gain[c][st + 3];
        if (st == 0 || g < dist) { dist = g; best = st; }
      }
      bins = 5;
      for (int k = 0; k < 4; k++) { const int o = s.bo_off[c][best + k]; bins += sao_off_bins(o) + (o != 0); }
      s.cand_band[c] = best;
    }
    s.cand_dist[c][j] = dist; s.cand_bins[c][j] = bins;
  }
  __syncthreads();
  SAO_STAMP(3);
  if (tid == 0) {
    const long long l2 = (long long)f.lambda_q4 * f.lambda_q4;
    int pick[2] = {0, 0};
    long long best = l2;
    for (int t = 1; t <= 5; t++) {
      const long long cost = 256LL * s.cand_dist[0][t - 1] + l2 * (2 + s.cand_bins[0][t - 1] + (t <= 4 ? 2 : 0));
      if (cost < best) { best = cost; pick[0] = t; }
    }
    if constexpr (IR) { if (f.ir_e < f.cw && cx == ((f.ir_e - 5) >> 6)) pick[0] = 0; }
    best = l2;
    for (int t = 1; t <= 5; t++) {
      const long long cost = 256LL * ((long long)s.cand_dist[1][t - 1] + s.cand_dist[2][t - 1]) + l2 * (2 + s.cand_bins[1][t - 1] + s.cand_bins[2][t - 1] + (t <= 4 ? 2 : 0));
      if (cost < best) { best = cost; pick[1] = t; }
    }
    SaoParams p;
    for (int c = 0; c < 3; c++) {
      const int t = pick[c ? 1 : 0];
      p.type[c] = t == 0 ? 0 : (t == 5 ? 1 : 2);
      p.eo_class[c] = (t >= 1 && t <= 4) ? (uint8_t)(t - 1) : 0;
      p.band_pos[c] = t == 5 ? (uint8_t)s.cand_band[c] : 0;
      for (int k = 0; k < 4; k++) p.offset[c][k] = (int8_t)(t == 0 ? 0 : (t == 5 ? s.bo_off[c][s.cand_band[c] + k] : s.eo_off[c][t - 1][k]));
    }
    s.p = p; f.sao[ctu] = p;
  }
  __syncthreads();
  SAO_STAMP(4);
  // ---- the filter: four samples of a row per thread, the rows above and below as 6-byte spans (samples x - 1 .. x + 4)
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int sh = c ? 1 : 0, l2n = 6 - sh, n = 1 << l2n, pw = f.cw >> sh, ph = f.ch >> sh, X0 = cx * n, Y0 = cy * n;
    const uint8_t *w = c ? s.winc[c - 1] : s.win; const int pitch = c ? 40 : 72;
    const int type = s.p.type[c], e = s.p.eo_class[c], bp = s.p.band_pos[c];
    int off[4];
    for (int k = 0; k < 4; k++) off[k] = s.p.offset[c][k];
#pragma unroll
    for (int q = tid; q < n * n / 4; q += T) {
      const int y = q >> (l2n - 2), x4 = (q & ((n >> 2) - 1)) * 4;
      const uint32_t *row = (const uint32_t *)&w[(y + 1) * pitch + x4];        // dword holding samples x4 - 4 .. x4 - 1
      uint32_t out = row[1];
      if (type == 1) {
        uint32_t o = 0;
        for (int i = 0; i < 4; i++) {
          const int v = (out >> (8 * i)) & 255, k = ((v >> 3) - bp) & 31;
          o |= (uint32_t)(k < 4 ? clip8(v + off[k]) : v) << (8 * i);
        }
        out = o;
      } else if (type == 2) {
        auto span = [&](const uint32_t *r) -> uint64_t { return ((uint64_t)r[0] >> 24) | ((uint64_t)r[1] << 8) | ((uint64_t)(r[2] & 255u) << 40); };
        const int dq = pitch >> 2;
        const uint64_t mid = span(row), up = span(row - dq), dn = span(row + dq);
        const bool okv = Y0 + y - 1 >= 0 && Y0 + y + 1 < ph;
        uint32_t o = 0;
        for (int i = 0; i < 4; i++) {
          const int v = (int)((mid >> (8 * (i + 1))) & 255);
          int a, b; bool ok;
          const bool okh = X0 + x4 + i - 1 >= 0 && X0 + x4 + i + 1 < pw;
          if (e == 0) { a = (int)((mid >> (8 * i)) & 255); b = (int)((mid >> (8 * (i + 2))) & 255); ok = okh; }
          else if (e == 1) { a = (int)((up >> (8 * (i + 1))) & 255); b = (int)((dn >> (8 * (i + 1))) & 255); ok = okv; }
          else if (e == 2) { a = (int)((up >> (8 * i)) & 255); b = (int)((dn >> (8 * (i + 2))) & 255); ok = okh && okv; }
          else { a = (int)((up >> (8 * (i + 2))) & 255); b = (int)((dn >> (8 * i)) & 255); ok = okh && okv; }
          const int k = ok ? sao_edge_idx(v, a, b) : 0;
          o |= (uint32_t)(k ? clip8(v + off[k - 1]) : v) << (8 * i);
        }
        out = o;
      }
      *(uint32_t *)&f.sao_out[c][(size_t)(Y0 + y) * pw + X0 + x4] = out;
    }
  }
  SAO_STAMP(5);
#undef SAO_STAMP
}

// =============================================================================================
// launch wrappers
// =============================================================================================
void launch_qp_resolve(const EncFrame &f, hipStream_t st)
{
  if (!f.ctu_qy) return;
  const int n = (f.cw / 64) * band_rows(f);
  if (f.wpp && f.cw / 64 <= 256) { hipLaunchKernelGGL(k_qp_rows, dim3(band_rows(f)), dim3(256), 0, st, f); return; }
  hipLaunchKernelGGL(k_qp_first, dim3(n), dim3(64), 0, st, f);
  hipLaunchKernelGGL(k_qp_chain, dim3((n + 255) / 256), dim3(256), 0, st, f);
}
void launch_deblock_v(const EncFrame &f, hipStream_t st)
{
  int nv = ((f.cw >> 3) - 1) * (band_rows(f) * 16);
  hipLaunchKernelGGL(k_deblock_v, dim3((nv + 255) / 256), dim3(256), 0, st, f);
}
void launch_deblock_h(const EncFrame &f, hipStream_t st, int part)
{
  const int ylo = imax(8, f.row0 * 64), yhi = imin(f.ch - 8, (f.row0 + band_rows(f)) * 64);
  int nh = (f.cw >> 2) * ((yhi - ylo) / 8 + 1);
  hipLaunchKernelGGL(k_deblock_h, dim3((nh + 255) / 256), dim3(256), 0, st, f, part);
}
void launch_deblock(const EncFrame &f, hipStream_t st)
{
  if (f.nrows > 0) { launch_deblock_v(f, st); launch_deblock_h(f, st, 0); return; }         // band of a tile-row split: two passes
  hipLaunchKernelGGL(k_deblock_tile, dim3((f.cw / 64) * (f.ch / 64)), dim3(256), 0, st, f);
}
void launch_sao(const EncFrame &f, hipStream_t st)
{
  if (f.ir_e) hipLaunchKernelGGL((k_sao<true>), dim3((f.cw / 64) * (f.ch / 64)), dim3(KVZ_SAO_THREADS), 0, st, f);      // intra-refresh: no luma SAO at the band's end
  else hipLaunchKernelGGL(k_sao<false>, dim3((f.cw / 64) * (f.ch / 64)), dim3(KVZ_SAO_THREADS), 0, st, f);
}

}  // namespace kvzx
