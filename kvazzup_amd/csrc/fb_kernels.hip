// kvazzup_amd/csrc/fb_kernels.hip -- "uvgx loss feedback v1" (loss-feedback): where a loss the receiver reported has travelled along the
// encoder's own motion, and what the heal picture does about it.  Statement: the fb_* functions of hevc_core.h, restated in tests/fb_model.py.
//
//   k_fb_record   every P picture with the option on, behind its chain: the picture's record -- per cell the final vector and fb_info() -- into its place in the ring
//   k_fb_seed     a heal picture, per report: the reported coding tree blocks' cells, dilated where a loop filter is on, OR-ed into the map
//   k_fb_step     ... per picture between the reported one and the heal picture: the map taken through that picture's record
//   k_fb_refs     fb-anchor, a v2 heal picture: how many quarters ended up as inter units on the anchor
//   k_fb_blocks   ... once: the map as one record per 32x32 block (fb_block_record) for k_me<.., FB> / k_subpel<.., FB>, and the picture's counts
// "uvgx loss feedback v2" (fb-anchor): k_fb_record_ref and k_fb_step_ref carry the reference bit of a v2 heal picture's cells.
//
// k_fb_seed, k_fb_step and k_fb_blocks are ONE workgroup each, looping over the cells: a step's intra units feed intra units, which is a fixed point with a
// barrier between its rounds, and the maps are small (1 600 cells at 320x320, 32 640 at 1080p).  They run on heal pictures only.  No kernel here waits for
// another workgroup or spins.
#include <hip/hip_runtime.h>
#include "hevc_core.h"
#include "enc_kernels.h"

namespace kvzx {

#define FB_THREADS 1024

__global__ __launch_bounds__(256) void k_fb_record(FbArgs a)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.gw * a.gh) return;
  if (a.clean) { a.rec_mv[2 * i] = 0; a.rec_mv[2 * i + 1] = 0; a.rec_info[i] = KVZ_FB_CLEAN; return; }
  a.rec_mv[2 * i] = a.cu_mv[2 * i]; a.rec_mv[2 * i + 1] = a.cu_mv[2 * i + 1];
  a.rec_info[i] = fb_info(a.cu_intra[i], a.cu_log2[i]);
}

// fb-anchor: a v2 heal picture's record -- an inter cell's reference index as KVZ_FB_REF1 beside fb_info().  A kernel of its own
__global__ __launch_bounds__(256) void k_fb_record_ref(FbRefArgs a)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.gw * a.gh) return;
  a.rec_mv[2 * i] = a.cu_mv[2 * i]; a.rec_mv[2 * i + 1] = a.cu_mv[2 * i + 1];
  a.rec_info[i] = (uint8_t)(fb_info(a.cu_intra[i], a.cu_log2[i]) | (!a.cu_intra[i] && a.cu_ref[i] ? KVZ_FB_REF1 : 0));
}

// map |= (the reported blocks' cells, dilated by one cell where a.dilate); tmp is scratch
__global__ __launch_bounds__(FB_THREADS) void k_fb_seed(FbArgs a)
{
  const int n = a.gw * a.gh;
  for (int i = threadIdx.x; i < n; i += FB_THREADS) a.tmp[i] = fb_seed_cell(a.gw * 8, i % a.gw, i / a.gw, a.first, a.count) ? 1 : 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += FB_THREADS)
    if (a.dilate ? fb_dilated(a.tmp, a.gw, a.gh, i % a.gw, i / a.gw) : a.tmp[i] != 0) a.map[i] = 1;
}

// map (D of the picture before) -> map (D of the record's picture): the inter cells into tmp, the intra units to their fixed point, the dilation
// RB (fb-anchor; k_fb_step_ref): the record is a v2 heal picture's -- a reference-1 cell read the anchor, not the picture before: it is in
// S where the report reaches the anchor (a.anchor_bad) and never otherwise (fb_anchor_cell)
template <bool RB, class A>
__device__ __forceinline__ void fb_step_body(const A &a)
{
  const int n = a.gw * a.gh, cw = a.gw * 8, ch = a.gh * 8;
  for (int i = threadIdx.x; i < n; i += FB_THREADS) {
    const uint8_t info = a.rec_info[i];
    if constexpr (RB) {
      if (!(info & (KVZ_FB_CLEAN | 1)) && (info & KVZ_FB_REF1)) { a.tmp[i] = fb_anchor_cell(info, a.anchor_bad) ? 1 : 0; continue; }
    }
    a.tmp[i] = (!(info & (KVZ_FB_CLEAN | 1)) && fb_inter_cell(a.map, cw, ch, i % a.gw, i / a.gw, a.rec_mv[2 * i], a.rec_mv[2 * i + 1])) ? 1 : 0;
  }
  __syncthreads();
  // (a round may see what another thread set in the same round: the set only grows, and what is set is reachable -- the fixed point is the same)
  for (;;) {
    int changed = 0;
    for (int i = threadIdx.x; i < n; i += FB_THREADS) {
      const uint8_t info = a.rec_info[i];
      if ((info & 1) && !(info & KVZ_FB_CLEAN) && !a.tmp[i] && fb_intra_cell(a.tmp, cw, ch, i % a.gw, i / a.gw, (info >> 1) & 7)) { a.tmp[i] = 1; changed = 1; }
    }
    if (!__syncthreads_or(changed)) break;
  }
  for (int i = threadIdx.x; i < n; i += FB_THREADS) a.map[i] = (a.dilate ? fb_dilated(a.tmp, a.gw, a.gh, i % a.gw, i / a.gw) : a.tmp[i] != 0) ? 1 : 0;
}

__global__ __launch_bounds__(FB_THREADS) void k_fb_step(FbArgs a) { fb_step_body<false>(a); }
__global__ __launch_bounds__(FB_THREADS) void k_fb_step_ref(FbRefArgs a) { fb_step_body<true>(a); }      // fb-anchor: a kernel of its own

// the heal picture's block records, and its counts {damaged cells, forced quarters} into stat[2], stat[3] (the slot's host-mapped record)
__global__ __launch_bounds__(FB_THREADS) void k_fb_blocks(FbArgs a)
{
  __shared__ uint32_t cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int n = a.gw * a.gh, bw = a.gw / 4, nb = bw * (a.gh / 4);
  uint32_t cells = 0, forced = 0;
  for (int i = threadIdx.x; i < n; i += FB_THREADS) cells += a.map[i] ? 1u : 0u;
  for (int b = threadIdx.x; b < nb; b += FB_THREADS) {
    uint8_t r[2];
    fb_block_record(a.map, a.gw, a.gh, b % bw, b / bw, a.me_range, r);
    a.blk[2 * b] = r[0]; a.blk[2 * b + 1] = r[1];
    forced += (uint32_t)__builtin_popcount(r[0]);
  }
  atomicAdd(&cnt[0], cells); atomicAdd(&cnt[1], forced);
  __syncthreads();
  if (threadIdx.x == 0) { a.stat[2] = (int32_t)cnt[0]; a.stat[3] = (int32_t)cnt[1]; }
}

// fb-anchor: the v2 heal picture's count of 16x16 quarters that are inter units on reference 1 (a quarter lies in one unit: its first cell says it), into stat[7]
__global__ __launch_bounds__(FB_THREADS) void k_fb_refs(FbRefArgs a)
{
  __shared__ uint32_t cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const int qw = a.gw / 2, nq = qw * (a.gh / 2);
  uint32_t c = 0;
  for (int q = threadIdx.x; q < nq; q += FB_THREADS) {
    const int i = (q / qw) * 2 * a.gw + (q % qw) * 2;
    c += (!a.cu_intra[i] && a.cu_ref[i]) ? 1u : 0u;
  }
  atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) a.stat[7] = (int32_t)cnt;
}

void launch_fb_record(const FbArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_fb_record, dim3((a.gw * a.gh + 255) / 256), dim3(256), 0, st, a); }
void launch_fb_record_ref(const FbRefArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_fb_record_ref, dim3((a.gw * a.gh + 255) / 256), dim3(256), 0, st, a); }
void launch_fb_seed(const FbArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_fb_seed, dim3(1), dim3(FB_THREADS), 0, st, a); }
void launch_fb_step(const FbArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_fb_step, dim3(1), dim3(FB_THREADS), 0, st, a); }
void launch_fb_step_ref(const FbRefArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_fb_step_ref, dim3(1), dim3(FB_THREADS), 0, st, a); }
void launch_fb_refs(const FbRefArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_fb_refs, dim3(1), dim3(FB_THREADS), 0, st, a); }
void launch_fb_blocks(const FbArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_fb_blocks, dim3(1), dim3(FB_THREADS), 0, st, a); }

}  // namespace kvzx
