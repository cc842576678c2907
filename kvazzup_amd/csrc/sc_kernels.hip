// kvazzup_amd/csrc/sc_kernels.hip -- "uvgx scene cut v1" (scenecut): what decides whether an input picture is a scene cut and
// becomes an IDR picture.  Statement: the sc_* functions of hevc_core.h, restated in tests/scenecut_model.py.
//
//   k_sc_sum      every input picture: the sum of the visible samples of its quarter picture (k_luma_quarter), kept with its working set
//   k_sc_blocks   an examined picture, one workgroup per visible 8x8 block of the quarter picture: the block's activity A around its mean and its best match S
//                 in the previous quarter picture shifted by the mean shift d, within +-rq samples; (S, A) filed, new blocks counted
//   k_sc_decide   one thread: the record {examined, n_new, n_b, d, cut} into device memory and the slot's host-mapped copy, the counter back to zero
//
// All sums are integers, so the order of the additions -- partial sums, atomics -- does not show in the result.  Everything here runs on the input stream,
// behind the picture's k_pad_input and k_luma_quarter; the host waits for k_sc_decide of an examined picture and for nothing else.
#include <hip/hip_runtime.h>
#include "hevc_core.h"
#include "enc_kernels.h"
#include "kernel_common.h"

namespace kvzx {

namespace {

// the dword `k` of a 16-byte piece at sample x of a row `width` samples wide, samples past the row's end zeroed
__device__ __forceinline__ uint32_t visible(uint32_t d, int x, int k, int width)
{
  const int left = width - (x + 4 * k);
  return left >= 4 ? d : (left <= 0 ? 0u : d & (0xffffffffu >> (8 * (4 - left))));
}
// four samples of the previous quarter picture, each through sc_ref_sample
__device__ __forceinline__ uint32_t shifted(uint32_t v, int d)
{
  uint32_t q = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) q |= (uint32_t)sc_ref_sample((int)((v >> (8 * b)) & 255u), d) << (8 * b);
  return q;
}

}  // namespace

#define SC_ROWS 8       // rows of the quarter picture per workgroup of k_sc_sum

// the quarter picture's rows are multiples of 16 samples (the coded width is a multiple of 64): every 16-byte piece lies inside the plane
__global__ __launch_bounds__(256) void k_sc_sum(ScArgs a)
{
  __shared__ uint32_t part[4];
  const int tid = threadIdx.x, y0 = blockIdx.x * SC_ROWS, wpr = (a.vw + 15) >> 4;
  uint32_t s = 0;                                                                       // per thread at most 8 x 256 / 256 pieces of 16 samples
  for (int i = tid; i < SC_ROWS * wpr; i += 256) {
    const int r = i / wpr, x = (i - r * wpr) * 16, y = y0 + r;
    if (y >= a.vh) break;
    const kv_u32x4 v = *reinterpret_cast<const kv_u32x4 *>(a.qc + (size_t)y * a.qw + x);
    s = __builtin_amdgcn_sad_u8(visible(v.x, x, 0, a.vw), 0u, s); s = __builtin_amdgcn_sad_u8(visible(v.y, x, 1, a.vw), 0u, s);
    s = __builtin_amdgcn_sad_u8(visible(v.z, x, 2, a.vw), 0u, s); s = __builtin_amdgcn_sad_u8(visible(v.w, x, 3, a.vw), 0u, s);
  }
  s = wave_sum_u32(s);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) atomicAdd(a.sum_c, (unsigned long long)part[0] + part[1] + part[2] + part[3]);
}

// One workgroup per block, as k_me_coarse: the block's window of the shifted previous quarter picture, (8 + 2 rq)^2 samples clamped to the picture's edge,
// sits in LDS -- rq and the picture's width are multiples of 4, so a word lies inside the picture or outside it as a whole.  A work item is a QUAD of
// horizontally adjacent candidates: v_qsad_pk_u16_u8 gives the four SADs of 4 samples of a row (an 8x8 SAD is at most 16 320: the u16 accumulators hold it).
#define SC_MAXRQ 64
#define SC_PITCH (2 * SC_MAXRQ + 12)          // bytes per window row: 8 + 2 rq samples, + 4 so the last quad's third word stays inside
__global__ __launch_bounds__(256) void k_sc_blocks(ScArgs a)
{
  __shared__ __attribute__((aligned(16))) uint8_t wbuf[(8 + 2 * SC_MAXRQ) * SC_PITCH];
  __shared__ uint32_t red;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int rq = a.rq, wq = 2 * rq + 1, wcols = 8 + 2 * rq, pitch = wcols + 4;
  const int qw = a.qw, qh = a.qh;
  const int d = sc_mean_shift((int64_t)*a.sum_c, (int64_t)*a.sum_p, (int64_t)a.vw * a.vh);
  if (tid == 0) red = ~0u;
  for (int i = tid; i < wcols * (pitch >> 2); i += nthreads) {
    const int wy = i / (pitch >> 2), wx = i - wy * (pitch >> 2);
    const int gy = clip3(0, qh - 1, by * 8 - rq + wy), gx = bx * 8 - rq + wx * 4;
    const uint8_t *row = a.qp + (size_t)gy * qw;
    uint32_t v;
    if (gx >= 0 && gx + 3 < qw) v = *reinterpret_cast<const uint32_t *>(row + gx);
    else v = (uint32_t)row[gx < 0 ? 0 : qw - 1] * 0x01010101u;
    *reinterpret_cast<uint32_t *>(&wbuf[wy * pitch + wx * 4]) = shifted(v, d);
  }
  uint32_t cur[16];                                              // the block: 8 rows of two words
  uint32_t sum = 0;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const uint32_t *c = reinterpret_cast<const uint32_t *>(a.qc + (size_t)(by * 8 + r) * qw + bx * 8);
    cur[2 * r] = c[0]; cur[2 * r + 1] = c[1];
    sum = __builtin_amdgcn_sad_u8(c[0], 0u, sum); sum = __builtin_amdgcn_sad_u8(c[1], 0u, sum);
  }
  __syncthreads();
  const int NQ = (wq + 3) >> 2;
  uint32_t best = ~0u;
  for (int item = tid; item < NQ * wq; item += nthreads) {
    const int dyi = item / NQ, q = item - dyi * NQ;
    const uint8_t *wbase = wbuf + dyi * pitch + 4 * q;
    uint64_t acc = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint32_t *wp = reinterpret_cast<const uint32_t *>(wbase + r * pitch);
      const uint32_t d0 = wp[0], d1 = wp[1], d2 = wp[2];
      acc = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)d1 << 32) | d0, cur[2 * r], acc);
      acc = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)d2 << 32) | d1, cur[2 * r + 1], acc);
    }
#pragma unroll
    for (int k4 = 0; k4 < 4; k4++) {
      const uint32_t s = (uint32_t)(acc >> (16 * k4)) & 0xffffu;
      if (4 * q + k4 < wq) best = s < best ? s : best;
    }
  }
  for (int o = 32; o > 0; o >>= 1) { const uint32_t v = __shfl_xor(best, o); best = v < best ? v : best; }
  if ((tid & 63) == 0) atomicMin(&red, best);
  __syncthreads();
  if (tid == 0) {
    const uint32_t m = (uint32_t)sc_block_mean((int)sum) * 0x01010101u;
    uint32_t act = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) act = __builtin_amdgcn_sad_u8(cur[i], m, act);
    const uint32_t S = red;
    uint32_t *out = a.blocks + 2 * ((size_t)by * a.bw + bx);
    out[0] = S; out[1] = act;
    if (sc_is_new(S, act)) atomicAdd(a.n_new, 1u);
  }
}

__global__ __launch_bounds__(64) void k_sc_decide(ScArgs a)
{
  if (threadIdx.x != 0) return;
  const int32_t n_new = (int32_t)*a.n_new, n_b = a.bw * a.bh;
  const int32_t d = sc_mean_shift((int64_t)*a.sum_c, (int64_t)*a.sum_p, (int64_t)a.vw * a.vh);
  const int32_t rec[5] = {1, n_new, n_b, d, sc_verdict(n_new, n_b) ? 1 : 0};
#pragma unroll
  for (int i = 0; i < 5; i++) { a.rec[i] = rec[i]; a.rec_host[i] = rec[i]; }
  *a.n_new = 0;
}

void launch_sc_sum(const ScArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_sc_sum, dim3((a.vh + SC_ROWS - 1) / SC_ROWS), dim3(256), 0, st, a); }
void launch_sc_blocks(const ScArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_sc_blocks, dim3(a.bw, a.bh), dim3(256), 0, st, a); }
void launch_sc_decide(const ScArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_sc_decide, dim3(1), dim3(64), 0, st, a); }

}  // namespace kvzx
