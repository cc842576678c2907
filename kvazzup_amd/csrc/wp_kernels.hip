// kvazzup_amd/csrc/wp_kernels.hip -- "uvgx weighted prediction v1" (weightp): what decides a P picture's luma weights and builds the
// planes its integer search reads.  Statement: the wp_* functions of hevc_core.h, restated in tests/wp_model.py.
//
//   k_wp_stats    every input picture: sum and sum of squares of the visible luma samples, one pair of partial sums per workgroup (four rows of the picture)
//   k_wp_decide   one workgroup.  Phase 0, behind k_wp_stats: the partial sums added up -> the picture's mean and variance (kept with its working set);
//                 a P picture: the candidate (w, o) of every reference from the two pictures' moments, the check's accumulators zeroed.
//                 Phase 1, behind k_wp_check: the verdicts -> the picture's record, in device memory (the kernels of its chain) and in the slot's
//                 host-mapped copy (the slice headers, written when the access unit is assembled)
//   k_wp_check    per candidate reference: sum |c - r| and sum |c - wp_sample(r)| over the samples at (4i, 4j) of the two input pictures
//   k_wp_plane    per reference: the search plane, wp_sample() of every sample of the plane the search would have read (a copy where the flag is 0)
//
// All four are streaming kernels over one luma plane or a sixteenth of it (2 MB at 1080p), 16 bytes per lane and access; every sum is an integer, so the order
// of the additions -- partial sums, atomics -- does not show in the result.  Everything here runs on the input stream, where the pictures follow one another.
#include <hip/hip_runtime.h>
#include "hevc_core.h"
#include "enc_kernels.h"
#include "kernel_common.h"

namespace kvzx {

namespace {

// sum of a value over the workgroup's waves (256 threads), valid in thread 0
__device__ __forceinline__ uint64_t block_sum(uint32_t v, uint32_t *part, int tid)
{
  v = wave_sum_u32(v);
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  const uint64_t r = (uint64_t)part[0] + part[1] + part[2] + part[3];
  __syncthreads();
  return r;
}
// the dword `k` of a 16-byte piece at sample x of a row `width` samples wide, samples past the row's end zeroed
__device__ __forceinline__ uint32_t visible(uint32_t d, int x, int k, int width)
{
  const int left = width - (x + 4 * k);
  return left >= 4 ? d : (left <= 0 ? 0u : d & (0xffffffffu >> (8 * (4 - left))));
}

}  // namespace

#define WP_ROWS 4       // rows of the picture per workgroup of k_wp_stats

__global__ __launch_bounds__(256) void k_wp_stats(const uint8_t *src, int cw, int width, int height, unsigned long long *partial)
{
  __shared__ uint32_t part[4];
  const int tid = threadIdx.x, y0 = blockIdx.x * WP_ROWS, wpr = (width + 15) >> 4;      // 16-byte pieces per row (cw is a multiple of 64: all inside the plane)
  uint32_t s1 = 0, s2 = 0;                                                              // per thread at most 16 x 1024 / 256 pieces of 16 samples: below 2^25
  for (int i = tid; i < WP_ROWS * wpr; i += 256) {
    const int r = i / wpr, x = (i - r * wpr) * 16, y = y0 + r;
    if (y >= height) break;
    const kv_u32x4 v = *reinterpret_cast<const kv_u32x4 *>(src + (size_t)y * cw + x);
    const uint32_t d[4] = {visible(v.x, x, 0, width), visible(v.y, x, 1, width), visible(v.z, x, 2, width), visible(v.w, x, 3, width)};
#pragma unroll
    for (int k = 0; k < 4; k++) { s1 = __builtin_amdgcn_sad_u8(d[k], 0u, s1); s2 = __builtin_amdgcn_udot4(d[k], d[k], s2, false); }
  }
  const uint64_t a = block_sum(s1, part, tid), b = block_sum(s2, part, tid);
  if (tid == 0) { partial[2 * blockIdx.x] = a; partial[2 * blockIdx.x + 1] = b; }
}

__global__ __launch_bounds__(256) void k_wp_decide(WpArgs a, int phase)
{
  __shared__ unsigned long long red[2];
  const int tid = threadIdx.x;
  if (phase == 0) {
    if (tid < 2) red[tid] = 0;
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    for (int i = tid; i < a.nblk; i += 256) { s1 += a.partial[2 * i]; s2 += a.partial[2 * i + 1]; }
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if ((tid & 63) == 0) { atomicAdd(&red[0], s1); atomicAdd(&red[1], s2); }
    __syncthreads();
    if (tid == 0) {
      int64_t m, v;
      wp_moments(red[0], red[1], (uint64_t)a.n, &m, &v);
      a.stat[0] = m; a.stat[1] = v;
      for (int r = 0; r < KVZ_MAX_LP_REFS; r++) {
        int w = 64, o = 0;
        const bool c = r < a.nref && wp_candidate(m, v, a.stat_ref[r][0], a.stat_ref[r][1], &w, &o);
        a.cand[3 * r] = c ? 1 : 0; a.cand[3 * r + 1] = w; a.cand[3 * r + 2] = o;
        a.acc[2 * r] = 0; a.acc[2 * r + 1] = 0;
      }
    }
  } else if (tid < KVZ_MAX_LP_REFS) {
    const bool on = wp_accept(a.cand[3 * tid] != 0, a.acc[2 * tid], a.acc[2 * tid + 1]);
    const int32_t f = on ? 1 : 0, w = on ? a.cand[3 * tid + 1] : 64, o = on ? a.cand[3 * tid + 2] : 0;
    a.rec[3 * tid] = f; a.rec[3 * tid + 1] = w; a.rec[3 * tid + 2] = o;
    a.rec_host[3 * tid] = f; a.rec_host[3 * tid + 1] = w; a.rec_host[3 * tid + 2] = o;
  }
}

#define WP_CHECK_ROWS 2       // sampled rows (4j) per workgroup of k_wp_check

// grid (sampled rows / WP_CHECK_ROWS, 1, references): a lane reads the 16-byte pieces of both pictures and takes the samples at their bytes 0, 4, 8, 12
__global__ __launch_bounds__(256) void k_wp_check(WpArgs a, const uint8_t *cur, int cw, int width, int height)
{
  __shared__ uint32_t part[4];
  const int tid = threadIdx.x, rf = blockIdx.z;
  if (!a.cand[3 * rf]) return;                                                          // (uniform: the whole launch of this reference leaves)
  const int w = a.cand[3 * rf + 1], o = a.cand[3 * rf + 2];
  const uint8_t *ref = a.in_ref[rf];
  const int wpr = (width + 15) >> 4, j0 = blockIdx.x * WP_CHECK_ROWS;
  uint32_t plain = 0, wt = 0;                                                           // per thread at most 2 x 64 / 256 pieces of 4 samples
  for (int i = tid; i < WP_CHECK_ROWS * wpr; i += 256) {
    const int r = i / wpr, x = (i - r * wpr) * 16, y = 4 * (j0 + r);
    if (y >= height) break;
    const kv_u32x4 c4 = *reinterpret_cast<const kv_u32x4 *>(cur + (size_t)y * cw + x), r4 = *reinterpret_cast<const kv_u32x4 *>(ref + (size_t)y * cw + x);
    const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w}, rr[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (x + 4 * k >= width) continue;
      const int cs = (int)(c[k] & 255u), rs = (int)(rr[k] & 255u);
      plain += (uint32_t)iabs(cs - rs); wt += (uint32_t)iabs(cs - wp_sample(rs, w, o));
    }
  }
  const uint64_t p = block_sum(plain, part, tid), q = block_sum(wt, part, tid);
  if (tid == 0) { atomicAdd(&a.acc[2 * rf], (unsigned long long)p); atomicAdd(&a.acc[2 * rf + 1], (unsigned long long)q); }
}

// grid (pieces of 16 samples / 256, 1, references) over the whole coded plane: the padding of a weighted plane is the weighted padding
__global__ __launch_bounds__(256) void k_wp_plane(WpPlaneArgs a, size_t npieces)
{
  const int rf = blockIdx.z;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npieces) return;
  const int32_t *rec = a.rec + 3 * rf;
  const int flag = rec[0], w = rec[1], o = rec[2];
  kv_u32x4 v = reinterpret_cast<const kv_u32x4 *>(a.from[rf])[i];
  if (flag) {
    uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t q = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) q |= (uint32_t)wp_sample((int)((d[k] >> (8 * b)) & 255u), w, o) << (8 * b);
      d[k] = q;
    }
    v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
  }
  reinterpret_cast<kv_u32x4 *>(a.to[rf])[i] = v;
}

int wp_stat_blocks(int height) { return (height + WP_ROWS - 1) / WP_ROWS; }
void launch_wp_stats(const uint8_t *src, int cw, int width, int height, unsigned long long *partial, hipStream_t st)
{
  hipLaunchKernelGGL(k_wp_stats, dim3(wp_stat_blocks(height)), dim3(256), 0, st, src, cw, width, height, partial);
}
void launch_wp_decide(const WpArgs &a, int phase, hipStream_t st) { hipLaunchKernelGGL(k_wp_decide, dim3(1), dim3(256), 0, st, a, phase); }
void launch_wp_check(const WpArgs &a, const uint8_t *cur, int cw, int width, int height, hipStream_t st)
{
  const int rows = (height + 3) / 4;
  hipLaunchKernelGGL(k_wp_check, dim3((rows + WP_CHECK_ROWS - 1) / WP_CHECK_ROWS, 1, a.nref), dim3(256), 0, st, a, cur, cw, width, height);
}
void launch_wp_plane(const WpPlaneArgs &a, int nref, int cw, int ch, hipStream_t st)
{
  const size_t npieces = (size_t)cw * ch / 16;
  hipLaunchKernelGGL(k_wp_plane, dim3((unsigned)((npieces + 255) / 256), 1, nref), dim3(256), 0, st, a, npieces);
}

}  // namespace kvzx
