// kvazzup_amd/csrc/recon_kernels.hip -- CDNA4 (gfx950) kernels of the HEVC encoder hot path: inter reconstruction and signalling, intra analysis,
// intra reconstruction (enc_kernels.hip has the introduction; the launch wrappers of these kernels are at the end).
//
// INTER AND INTRA RECONSTRUCTION STAY IN ONE FILE.  The machine code hipcc makes of k_intra_recon<ADJ = true, ..> depends on k_inter_recon being in its
// translation unit (both call adjust_block_lds; without k_inter_recon: other registers throughout, 300 lines more); likewise k_tokenize and the motion
// search in enc_kernels.hip.  Seen by compiling, not measured on a GPU: parting either pair is a performance change and wants a measurement.
//
// Launch geometry (coded size is a multiple of 64; DESIGN.md section 5 has the table with timings):
//   k_inter_recon   one workgroup per 32x32 block: MC, residual, DCT (32x32: MFMA i8), quant, dequant, IDCT, reconstruction
//                   (two forms: with fractional vectors -- subme > 0, separable LDS passes -- and without)
//   k_inter_signal  one thread per 16x16 block: merge / skip / AMVP signalling
//   k_intra_analyse one workgroup per 32x32 region: 35-mode search on source samples, cost = 8x8 Hadamard sums on the matrix cores
//                   (intra-satd, default) or SAD; work item = (16x16 tile, mode, kind) on one wave
//   k_intra_recon   four waves per (CTU, colour plane), one intra block per WAVE and no workgroup barrier in the chain (transforms on
//                   v_mfma_f32_16x16x16_f16, references over DPP / ds_bpermute); CTUs coupled by progress counters with 8x8 granularity
#include <hip/hip_runtime.h>
#include <type_traits>
#include "hevc_core.h"
#include "enc_kernels.h"
#include "kernel_common.h"

namespace kvzx {

// =============================================================================================
// Inter reconstruction of one 32x32 block (one 32x32 CU or four 16x16 CUs), one workgroup each
// =============================================================================================
__device__ __forceinline__ int ref_at(const uint8_t *p, int w, int h, int x, int y)
{
  return p[clip3(0, h - 1, y) * w + clip3(0, w - 1, x)];
}
// luma sample with the 8-tap filters of 8.5.3.3.3.1; mv in quarter samples (general path: fractional vectors)
__device__ __forceinline__ int mc_luma_sample(const uint8_t *p, int w, int h, int x, int y, int mvx, int mvy)
{
  int xf = mvx & 3, yf = mvy & 3, xi = x + (mvx >> 2), yi = y + (mvy >> 2), v;
  if (!xf && !yf) return ref_at(p, w, h, xi, yi);
  if (!yf) { v = 0; for (int i = 0; i < 8; i++) v += kLumaFilter[xf][i] * ref_at(p, w, h, xi + i - 3, yi); }
  else if (!xf) { v = 0; for (int i = 0; i < 8; i++) v += kLumaFilter[yf][i] * ref_at(p, w, h, xi, yi + i - 3); }
  else {
    v = 0;
    for (int j = 0; j < 8; j++) {
      int t = 0;
      for (int i = 0; i < 8; i++) t += kLumaFilter[xf][i] * ref_at(p, w, h, xi + i - 3, yi + j - 3);
      v += kLumaFilter[yf][j] * t;
    }
    v >>= 6;
  }
  return clip8((v + 32) >> 6);
}
// four luma samples (x .. x + 3, y) predicted with one vector, packed little-endian
__device__ __forceinline__ uint32_t mc_luma4(const uint8_t *p, int w, int h, int x, int y, int mvx, int mvy)
{
  if (((mvx | mvy) & 3) == 0) {
    const int xi = x + (mvx >> 2), yi = clip3(0, h - 1, y + (mvy >> 2));
    const uint8_t *row = p + (size_t)yi * w;
    if (xi >= 0 && xi + 3 < w) {
      const uint32_t *q = (const uint32_t *)(row + (xi & ~3));                 // planes are 4-byte aligned, w is a multiple of 64
      const uint32_t lo = q[0], hi = (xi & 3) ? q[1] : 0u;
      return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(xi & 3));
    }
    uint32_t v = 0;
    for (int i = 0; i < 4; i++) v |= (uint32_t)row[clip3(0, w - 1, xi + i)] << (8 * i);
    return v;
  }
  uint32_t v = 0;
  for (int i = 0; i < 4; i++) v |= (uint32_t)mc_luma_sample(p, w, h, x + i, y, mvx, mvy) << (8 * i);
  return v;
}

struct InterLds {
  alignas(16) int16_t A[1024], B[1024];
  alignas(16) int16_t M[2][KV_MATRIX_ENTRIES];
  alignas(16) uint8_t px[1024];            // prediction, then reconstruction: luma 32x32 raster; chroma 2 planes x 16x16
  alignas(16) uint8_t win[2][4][11 * 12];  // chroma reference windows: plane x 8x8 sub-block, 11 x 11 samples each
  uint32_t nz[2];
  int mv[4][2];
  uint8_t rf[4];                           // lp-refs: ref_idx of each quarter
  int intra_q[4];                          // intra-in-P: the 16x16 quarter is an intra unit
  int rc_qp, rc_last; uint32_t rc_part[4]; // rate control v2 inside the launch (k_inter_recon<.., RC>)
  alignas(16) int8_t M8[2][32 * 32];       // the 32-point matrix and its transpose as int8: MFMA B operands
  int rowsum[2][32];                       // sum over m of M8[.][j][m]
};
// fractional-sample luma interpolation (subme > 0), per 16x16 quadrant: the 23 x 23 reference window and the horizontally filtered
// rows (8.5.3.3.3.1).  Only the FRAC form of k_inter_recon has it: without these 8 KB eight workgroups fit a compute unit.
struct InterFracLds {
  alignas(16) uint8_t lwin[4][23 * 24];
  alignas(16) int ltmp[4][23 * 16];        // (32-bit on purpose: with int16 entries hipcc 7.2 mis-extends the upper halves of the packed loads)
};

// Level adjustment ("uvgx RDOQ v1" / sign data hiding, hevc_core.h adjust_group) of a block whose levels lie row-major in lev[n * n] and
// whose quantiser remainders lie in aux[n * n]: thread `t` of the block's threads takes the coefficient groups t, t + nthreads, ...
__device__ __forceinline__ void adjust_block_lds(int16_t *lev, const int16_t *aux, int n, int pitch, int scan_idx, int rdoq, int signhide, int t, int nthreads)
{
  const int nsb = n >> 2, ngroups = nsb * nsb;
  for (int gi = t; gi < ngroups; gi += nthreads) {
    const int xs = gi % nsb, ys = gi / nsb;
    int16_t lv[16]; uint16_t ax[16]; int at[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int xp = scan_idx == 0 ? kDiag4x[k] : (scan_idx == 1 ? (k & 3) : (k >> 2)), yp = scan_idx == 0 ? kDiag4y[k] : (scan_idx == 1 ? (k >> 2) : (k & 3));
      at[k] = ((ys << 2) + yp) * pitch + (xs << 2) + xp;
      lv[k] = lev[at[k]]; ax[k] = (uint16_t)aux[((ys << 2) + yp) * n + (xs << 2) + xp];
    }
    adjust_group(lv, ax, gi == 0, rdoq, signhide);
#pragma unroll
    for (int k = 0; k < 16; k++) lev[at[k]] = lv[k];
  }
}

// The four transform stages of `NTU` blocks of n = 1 << L2 held TU-major in s.A (the residual, row-major),
// NTU * XF<L2, OPL>::LANES == 256.  Levels go to `coef` for blocks that have any, *nz gets one bit per block.
// Ends with the reconstructed residual added into s.px.
//   px_index(tu, y, x) -> index of sample (x, y) of block tu in s.px;  coef_at(tu, y, x) -> its level in the plane
//   RC (rate control v2 inside the launch): qp_late() is called between the forward transform and the quantiser -- it waits for the QP if it has to --
//   and the cost of the levels (3 + 2 floor(log2 |level|) each) is added to `cost`
struct NoLateQp { __device__ int operator()() const { return 0; } };
__device__ __forceinline__ uint32_t rc_level_cost(int lv) { return lv ? 3u + 2u * (uint32_t)(31 - __builtin_clz((unsigned)iabs(lv))) : 0u; }
//   mtab: the scaling factors of this block size and plane for inter blocks (`scaling-list default`), NULL: flat
template <int L2, int OPL, bool RC = false, class PX, class CI, class QL = NoLateQp>
__device__ __forceinline__ void inter_transform(InterLds &s, int qp, uint32_t *nz, PX px_index, CI coef_at, int tid, int adj = 0, QL qp_late = QL(), uint32_t *cost = nullptr, const uint8_t *mtab0 = nullptr, int tu_per_plane = 1 << 30)
{
  constexpr int N = 1 << L2, G = XF<L2, OPL>::G, LPT = XF<L2, OPL>::LANES;
  const int tu = tid / LPT, l = tid % LPT, rp = l / G, g = l % G;
  const uint8_t *mtab = mtab0 ? mtab0 + (tu / tu_per_plane) * N * N : nullptr;      // (the chroma call holds Cb and Cr blocks: their matrices follow one another)
  int16_t *A = s.A + tu * N * N, *B = s.B + tu * N * N;
  const int16_t *Mf = s.M[0] + matrix_offset(L2);
  xf_stage<L2, OPL>(A, B, Mf, L2 - 1, rp, g);
  __syncthreads();
  {
    int acc[2][OPL], lv[2][OPL];
    xf_sums<L2, OPL>(B, Mf, rp, g, acc);
    if constexpr (RC) qp = qp_late();
    const int shift = L2 + 6, rnd = 1 << (shift - 1);
    bool any = false;
    if (adj) {
      // rdoq / signhide (bit 0 / bit 1 of adj): levels and quantiser remainders go to B and A in the block's own layout, a pass over the
      // 4x4 coefficient groups adjusts the levels (one thread per group), then every thread takes its levels back
      __syncthreads();                                           // (all threads are done reading B: xf_sums)
#pragma unroll
      for (int o = 0; o < OPL; o++)
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int c = clip3(-32768, 32767, (acc[e][o] + rnd) >> shift);
          uint16_t ax;
          B[(g * OPL + o) * N + 2 * rp + e] = (int16_t)quant_level_aux(c, qp, L2, 0, &ax, mtab ? mtab[(g * OPL + o) * N + 2 * rp + e] : 16);
          A[(g * OPL + o) * N + 2 * rp + e] = (int16_t)ax;
        }
      __syncthreads();
      adjust_block_lds(B, A, N, N, 0, adj & 1, adj & 2, l, LPT);
      __syncthreads();
#pragma unroll
      for (int o = 0; o < OPL; o++)
#pragma unroll
        for (int e = 0; e < 2; e++) lv[e][o] = B[(g * OPL + o) * N + 2 * rp + e];
      __syncthreads();                                           // (A still holds remainders other threads' groups have read: all done now)
    }
#pragma unroll
    for (int o = 0; o < OPL; o++)
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const int m = mtab ? mtab[(g * OPL + o) * N + 2 * rp + e] : 16;
        if (!adj) { int c = clip3(-32768, 32767, (acc[e][o] + rnd) >> shift); lv[e][o] = quant_level(c, qp, L2, 0, m); }
        any |= lv[e][o] != 0;
        if constexpr (RC) *cost += rc_level_cost(lv[e][o]);
        A[(2 * rp + e) * N + g * OPL + o] = (int16_t)dequant_coef(lv[e][o], qp, L2, m);     // transposed: [column][row]
      }
    if (any) atomicOr(nz, 1u << tu);
    __syncthreads();
    if ((*nz >> tu) & 1) {
#pragma unroll
      for (int o = 0; o < OPL; o++) *(uint32_t *)coef_at(tu, g * OPL + o, 2 * rp) = pack_i16(lv[0][o], lv[1][o]);   // row g*OPL+o, columns 2rp, 2rp+1
    }
  }
  const bool has = (*nz >> tu) & 1;
  const int16_t *Mt = s.M[1] + matrix_offset(L2);
  if (has) xf_stage<L2, OPL>(A, B, Mt, 7, rp, g);
  __syncthreads();
  if (has) {
    int acc[2][OPL];
    xf_sums<L2, OPL>(B, Mt, rp, g, acc);
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
      for (int o = 0; o < OPL; o++) {
        uint8_t *q = &s.px[px_index(tu, 2 * rp + e, g * OPL + o)];
        *q = (uint8_t)clip8(*q + ((acc[e][o] + 2048) >> 12));
      }
  }
  __syncthreads();
}

// The 32x32 luma block of a 32x32 CU: same contract as inter_transform<5, .>
template <bool RC = false, class QL = NoLateQp>
__device__ __forceinline__ void inter_transform_32(InterLds &s, int qp, uint32_t *nz, int16_t *coef, int cw, int tid, int adj = 0, QL qp_late = QL(), uint32_t *cost = nullptr, const uint8_t *mtab = nullptr)
{
  const int wave = tid >> 6, lane = tid & 63;
  const int j = (wave & 1) * 16 + (lane & 15), i0 = (wave >> 1) * 16 + (lane >> 4) * 4;   // result column, first of four result rows
  int lv[4];
  mfma_stage(s.A, s.B, s.M8[0], s.rowsum[0], 4, wave, lane);                               // forward rows (shift log2 n - 1)
  __syncthreads();
  {
    int acc[4];
    mfma_tile_sums(s.B, s.M8[0], s.rowsum[0], wave, lane, acc);                            // forward columns: coefficient (row j, columns i0 ..)
    if constexpr (RC) qp = qp_late();
    bool any = false;
    if (adj) {                                                                             // rdoq / signhide: see inter_transform
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int c = clip3(-32768, 32767, (acc[r] + 1024) >> 11);
        uint16_t ax;
        s.B[j * 32 + i0 + r] = (int16_t)quant_level_aux(c, qp, 5, 0, &ax, mtab ? mtab[j * 32 + i0 + r] : 16);
        s.A[j * 32 + i0 + r] = (int16_t)ax;
      }
      __syncthreads();
      adjust_block_lds(s.B, s.A, 32, 32, 0, adj & 1, adj & 2, tid, 256);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++) lv[r] = s.B[j * 32 + i0 + r];
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = mtab ? mtab[j * 32 + i0 + r] : 16;
      if (!adj) { const int c = clip3(-32768, 32767, (acc[r] + 1024) >> 11); lv[r] = quant_level(c, qp, 5, 0, m); }
      any |= lv[r] != 0;
      if constexpr (RC) *cost += rc_level_cost(lv[r]);
      s.A[(i0 + r) * 32 + j] = (int16_t)dequant_coef(lv[r], qp, 5, m);                     // transposed: [column][row]
    }
    if (any) atomicOr(nz, 1u);
  }
  __syncthreads();
  if (*nz & 1) *(uint2 *)&coef[(size_t)j * cw + i0] = make_uint2(pack_i16(lv[0], lv[1]), pack_i16(lv[2], lv[3]));
  const bool has = *nz & 1;
  if (has) mfma_stage(s.A, s.B, s.M8[1], s.rowsum[1], 7, wave, lane);                      // inverse columns
  __syncthreads();
  if (has) {
    int acc[4];
    mfma_tile_sums(s.B, s.M8[1], s.rowsum[1], wave, lane, acc);                            // inverse rows: residual (rows i0 .., column j)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      uint8_t *q = &s.px[(i0 + r) * 32 + j];
      *q = (uint8_t)clip8(*q + ((acc[r] + 2048) >> 12));
    }
  }
  __syncthreads();
}

// Rate control v2, the tail of a workgroup of k_inter_recon<.., RC>: its level cost joins its group's (one atomic: arrivals << 40 | cost), and the workgroup
// that completes the group decides for the next one (statement: rc_band_decide() in oracle/hevc_enc.c) -- prices the rows done against their share of the
// picture's target, moves the running QP step and publishes it -- the step of the group AFTER THE NEXT (round 4: one group of lag, so that no group waits
// for the one right in front of it) -- in RcState::decided: bits 0..3 the number of groups closed, bits 4 + 3 (g - 1) .. the step of group g, biased by 3.  The per-CTU QP array is left alone while workgroups may still read it: the workgroup that completes the LAST group applies
// every group's step to it (for k_qp_first / k_qp_chain, deblocking and k_intra_recon) and files the picture's cost for k_rc_begin of a later picture.
__device__ __forceinline__ int rc_word_step(uint32_t word, int grp) { return grp > 0 ? (int)((word >> (4 + 3 * (grp - 1))) & 7u) - 3 : 0; }
__device__ __forceinline__ void rc_group_done(const EncFrame &f, InterLds &s, int grp, uint32_t cost, int tid)
{
  RcState *rc = f.rc;
  const int rows = f.ch >> 6, wc = f.cw >> 6, nb = f.rc_nb;
  const int r0 = (grp * rows) / nb, r1 = ((grp + 1) * rows) / nb;
  cost = wave_sum_u32(cost);
  if ((tid & 63) == 0) s.rc_part[tid >> 6] = cost;
  __syncthreads();
  if (tid == 0) {
    const unsigned long long mine = (unsigned long long)s.rc_part[0] + s.rc_part[1] + s.rc_part[2] + s.rc_part[3];
    const unsigned long long old = atomicAdd(&rc->acc[grp * KVZ_RC_ACC_STRIDE], (1ull << 40) | mine);
    const bool last = (old >> 40) == (unsigned long long)((r1 - r0) * 2 * (f.cw >> 5)) - 1ull;
    uint32_t word = 0;
    if (last) {
      // The groups are processed in order: cost_sofar and the word are what the group before this one left -- whose workgroups this group did NOT wait
      // for (a group waits for the one before the last, see k_inter_recon), so the one thread that closes this group does (rarely long: that group
      // started earlier).
      if (grp > 0) { uint32_t spins = 0; while ((ld_l2_u32(&rc->decided) & 15u) < (uint32_t)grp) { __builtin_amdgcn_s_sleep(8); if (++spins > (1u << 22)) { atomicOr(f.err, 1u); break; } } }
      const uint32_t total = ld_l2_u32(&rc->cost_sofar) + (uint32_t)((old & ((1ull << 40) - 1)) + mine);
      word = ld_l2_u32(&rc->decided);
      if (grp + 1 < nb) {
        // the step of group grp + 2: the running step (that of group grp + 1, decided a group ago; groups 0 and 1: none) moved by what groups 0 .. grp cost
        if (grp == 0) word |= 3u << 4;                        // (group 1's step, biased: 0)
        if (grp + 2 < nb) {
          int off = rc_word_step(word, grp + 1);
          if (ld_l2_u32(&rc->ratio_valid)) {
            const unsigned long long est = ((unsigned long long)total * ld_l2_u32(&rc->ratio_q8)) >> 8, tgt = ((unsigned long long)f.rc_target * (unsigned long long)r1) / (unsigned long long)rows;
            if (est * 8 > tgt * 9) off++; else if (est * 8 < tgt * 7) off--;
            off = clip3(-3, 3, off);
          }
          word |= (uint32_t)(off + 3) << (4 + 3 * (grp + 1));
        }
        st_wt_u32(&rc->cost_sofar, total);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        word = (word & ~15u) | (uint32_t)(grp + 1);
        st_wt_u32(&rc->decided, word);
      } else { rc->cost[f.rc_slot] = total; rc->cost_valid[f.rc_slot] = 1; }
    }
    s.rc_last = (last && grp + 1 == nb) ? 1 : 0; s.rc_qp = (int)word;
  }
  __syncthreads();
  if (!s.rc_last) return;
  // every other workgroup of the launch is done: the steps go into the QP array
  const uint32_t word = (uint32_t)s.rc_qp;
  int8_t *qt = const_cast<int8_t *>(f.ctu_qt);
  for (int g = 1; g < nb; g++) {
    const int off = rc_word_step(word, g);
    if (off) for (int i = ((g * rows) / nb) * wc + tid; i < (((g + 1) * rows) / nb) * wc; i += 256) qt[i] = (int8_t)clip3(0, 51, (int)qt[i] + off);
  }
}

// The residual comes from the source picture, and the levels are written out (the decoder's reconstruction is dec_kernels.hip's).
// ADJ: rdoq / signhide -- a kernel of its own: the plain form fits eight workgroups per compute unit in 64 registers, and with the level adjustment compiled
// in it no longer did (159 registers spilled, 14 MB of scratch writes per 1080p launch, 23 -> 28 us -- found in the PMC pass, not in a test).
// RC (encoder, rate control v2): the CTU rows in f.rc_nb groups, the QP of a group decided by the last workgroup of the group before it.  Workgroups are
// dispatched in the order of their linear index (rows top to bottom here: no XCD permutation), so every workgroup of a group is resident or done when one of
// the next group starts to wait -- the wait cannot starve what it waits for (the intra chains' argument).
// LL: `lossless` (cu_transquant_bypass): the residual itself goes to the level planes, sample by sample, and the reconstruction is the source
// WP (encoder, weightp): luma of every quarter is predicted from its reference with that reference's (w, o) of the picture's record (f.wp) --
// wp_pred14 on the 14-bit intermediate, wp_sample at integer vectors; chroma as ever.  Forms of their own, at the register budget of the fractional forms --
// a wave less where the form of before already spills (rdoq / signhide: 4; rate control v2 with fractional vectors: 6), so that no weighted form uses scratch.
template <bool FRAC, bool ADJ = false, bool RC = false, bool LL = false, bool WP = false>
// waves per SIMD the fractional / rate-control forms are held to: 7 (72 registers, one spilled in the rate-control form) -- their 22 KB of LDS allow seven workgroups
// per compute unit, 78 registers only six; default mode 5 450-5 530 -> 5 580-5 660 frames/s, the launch 51.3 -> 49.3 us (profiles/r06_recon_waves_ab.txt).  The forms
// with the level-adjustment pass (ADJ: rdoq / signhide) keep 5: they spill at anything tighter.
#ifndef KVZ_RECON_WAVES
#define KVZ_RECON_WAVES 7
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((FRAC || ADJ || RC || WP) ? (ADJ ? (WP ? 4 : 5) : ((WP && RC && FRAC) ? KVZ_RECON_WAVES - 1 : KVZ_RECON_WAVES)) : 8))) void k_inter_recon(EncFrame f)
{
  __shared__ InterLds s;
  InterFracLds *fr = nullptr;
  if constexpr (FRAC) { __shared__ InterFracLds fr_s; fr = &fr_s; }
  const int tid = threadIdx.x;
  int bx_, by_;
  if (RC) { bx_ = (int)blockIdx.x; by_ = (int)blockIdx.y; } else xcd_block_2d(bx_, by_);
  const int x0 = bx_ * 32, y0 = by_ * 32 + f.row0 * 64;
  const int bi0 = b8idx(f, x0, y0);
  const bool split = f.cu_log2[bi0] != 5;                              // (four 16x16 units: with intra-in-P a quarter may also be an intra unit, 16x16 or four 8x8)
  const int cw2 = f.cw >> 1, ch2 = f.ch >> 1;
  int grp = 0;                                                         // RC: the group of CTU rows this block belongs to: rows [g * rows / nb, (g + 1) * rows / nb)
  if (RC) { const int rows = f.ch >> 6; while (grp + 1 < f.rc_nb && (y0 >> 6) >= ((grp + 1) * rows) / f.rc_nb) grp++; }
  int qp = ctu_quant_qp(f, x0, y0), qpc = kChromaQp[qp];             // the 32x32 block lies inside one CTU (RC, groups behind the first: before the group's step)
  uint32_t rc_cost = 0;
  // RC: called by the luma transform in front of its quantiser -- the CTU's QP once the group before this one has decided (rc_group_done): the word
  // that counts the decided groups carries their QP steps as well, so the wait costs one trip to memory
  auto qp_late = [&]() -> int {
    if (RC && grp > 1) {                                             // (groups 0 and 1 run at the picture's QP; group g's step was decided when group g - 2 closed)
      if (tid == 0) {
        uint32_t spins = 0, v;
        while (((v = ld_l2_u32(&f.rc->decided)) & 15u) + 1u < (uint32_t)grp) {
          __builtin_amdgcn_s_sleep(24);                                  // (~0.6 us: hundreds of workgroups poll this word, and the polls travel to memory)
          if (++spins > (1u << 22)) { atomicOr(f.err, 1u); break; }      // bounded spin: never hang the GPU
        }
        s.rc_qp = clip3(0, 51, qp + rc_word_step(v, grp));
      }
      __syncthreads();
      qp = s.rc_qp; qpc = kChromaQp[qp];
    }
    return qp;
  };
  const int adj = !ADJ ? 0 : ((f.rdoq ? 1 : 0) | (f.signhide ? 2 : 0));    // level adjustment behind the quantiser (hevc_core.h adjust_group)
  // matrices of the two block sizes in use (luma n, chroma n / 2): adjacent in the table
  if (split) load_matrices(s.M, 16, 64 + 256, tid, 256);
  else {
    load_matrices(s.M, 80, 256, tid, 256);                       // chroma 16-point matrices (dot2 path)
    if (tid >= 64 && tid < 192) ((uint4 *)s.M8)[tid - 64] = ((const uint4 *)g_xf.M8)[tid - 64];
    else if (tid >= 192 && tid < 208) ((uint4 *)s.rowsum)[tid - 192] = ((const uint4 *)g_xf.rowsum)[tid - 192];
  }
  if (tid < 2) s.nz[tid] = 0;
  if (tid < 4) {
    int bi = b8idx(f, x0 + (tid & 1) * 16, y0 + (tid >> 1) * 16);
    s.mv[tid][0] = f.cu_mv[bi * 2]; s.mv[tid][1] = f.cu_mv[bi * 2 + 1];
    s.rf[tid] = (uint8_t)cu_ref_at(f, bi);                            // lp-refs: the quarter's reference
    // intra-in-P: a quarter that is an intra unit gets no residual here (levels, cbf and reconstruction are k_intra_recon's, which runs behind this kernel)
    s.intra_q[tid] = (f.intra_p && split) ? f.cu_intra[bi] : 0;
  }
  __syncthreads();
  // ---- luma with fractional vectors (the encoder's with subme > 0): window -> LDS, horizontal pass -> LDS
  const bool anyfrac = FRAC && (((s.mv[0][0] | s.mv[0][1] | s.mv[1][0] | s.mv[1][1] | s.mv[2][0] | s.mv[2][1] | s.mv[3][0] | s.mv[3][1]) & 3) != 0);
  if (anyfrac) {
    for (int i = tid; i < 4 * 23 * 23; i += 256) {
      const int k = i / 529, r = i - k * 529, wy = r / 23, wx = r - wy * 23;
      const int gx = x0 + (k & 1) * 16 + (s.mv[k][0] >> 2) - 3 + wx, gy = y0 + (k >> 1) * 16 + (s.mv[k][1] >> 2) - 3 + wy;
      fr->lwin[k][wy * 24 + wx] = ref_plane(f, s.rf[k], 0)[(size_t)clip3(0, f.ch - 1, gy) * f.cw + clip3(0, f.cw - 1, gx)];
    }
    __syncthreads();
    for (int i = tid; i < 4 * 23 * 16; i += 256) {
      const int k = i / 368, r = i - k * 368, wy = r >> 4, c = r & 15, xf = s.mv[k][0] & 3;
      const uint8_t *wp = &fr->lwin[k][wy * 24 + c];
      int v = wp[3];
      if (xf) { v = 0; for (int t = 0; t < 8; t++) v += kLumaFilter[xf][t] * wp[t]; }
      fr->ltmp[k][wy * 16 + c] = v;
    }
    __syncthreads();
  }
  // ---- luma: prediction (four samples per thread), residual TU-major into s.A
  {
    const int y = tid >> 3, x = (tid & 7) * 4, k = (y >> 4) * 2 + (x >> 4);
    const int l2 = split ? 4 : 5, n = 1 << l2, tu = split ? k : 0;
    uint32_t p4 = 0;
    int wp_w = 64, wp_o = 0;
    if constexpr (WP) { const int32_t *rec = f.wp + 3 * s.rf[k]; wp_w = rec[1]; wp_o = rec[2]; }
    if (anyfrac) {                             // (block-uniform) separable 8-tap interpolation through LDS
      const int mvx = s.mv[k][0], mvy = s.mv[k][1], xf = mvx & 3, yf = mvy & 3;
      const int *tp = &fr->ltmp[k][(y & 15) * 16 + (x & 15)];
#pragma unroll 1
      for (int i = 0; i < 4; i++) {            // (kept rolled: the unrolled form came out wrong for the third and fourth sample with hipcc 7.2)
        int v;
        if (yf) {
          int a = 0;
          for (int j = 0; j < 8; j++) a += (int)kLumaFilter[yf][j] * tp[j * 16 + i];
          v = xf ? (a >> 6) : a;
        } else v = xf ? tp[3 * 16 + i] : tp[3 * 16 + i] * 64;
        p4 |= (uint32_t)(WP ? wp_pred14(v, wp_w, wp_o) : clip8((v + 32) >> 6)) << (8 * i);
      }
    } else {
      p4 = mc_luma4(ref_plane(f, s.rf[k], 0), f.cw, f.ch, x0 + x, y0 + y, s.mv[k][0], s.mv[k][1]);
      if constexpr (WP) {                      // (the encoder's vectors are whole here: without subme always, with it when no quarter has a fraction)
        uint32_t q4 = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) q4 |= (uint32_t)wp_sample((int)((p4 >> (8 * i)) & 255u), wp_w, wp_o) << (8 * i);
        p4 = q4;
      }
    }
    const size_t g = (size_t)(y0 + y) * f.cw + x0 + x;
    *(uint32_t *)&s.px[y * 32 + x] = p4;
    int16_t *A = s.A + (tu << (2 * l2));
    const int ty = y & (n - 1), tx = x & (n - 1);
    const uint32_t s4 = *(const uint32_t *)&f.src[0][g];
    int r[4];
    for (int i = 0; i < 4; i++) r[i] = s.intra_q[k] ? 0 : (int)((s4 >> (8 * i)) & 255) - (int)((p4 >> (8 * i)) & 255);
    if constexpr (LL) {
      *(uint2 *)&f.coef[0][g] = make_uint2(pack_i16(r[0], r[1]), pack_i16(r[2], r[3]));
      if (r[0] | r[1] | r[2] | r[3]) atomicOr(&s.nz[0], 1u << tu);
      if (!s.intra_q[k]) *(uint32_t *)&s.px[y * 32 + x] = s4;
    } else *(uint2 *)&A[ty * n + tx] = make_uint2(pack_i16(r[0], r[1]), pack_i16(r[2], r[3]));
  }
  // ---- chroma: reference windows of the eight 8x8 sub-blocks (plane x quadrant) -> LDS; mv in 1/8 samples
  auto chroma_windows = [&]() {
    for (int i = tid; i < 8 * 121; i += 256) {
      const int w8 = i / 121, r = i - w8 * 121, wy = r / 11, wx = r - wy * 11, pl = w8 >> 2, sub = w8 & 3, k = split ? sub : 0;
      const int xi = (x0 >> 1) + (sub & 1) * 8 + (s.mv[k][0] >> 3) + wx - 1, yi = (y0 >> 1) + (sub >> 1) * 8 + (s.mv[k][1] >> 3) + wy - 1;
      s.win[pl][sub][wy * 12 + wx] = ref_plane(f, s.rf[k], 1 + pl)[(size_t)clip3(0, ch2 - 1, yi) * cw2 + clip3(0, cw2 - 1, xi)];
    }
  };
  // RC: everything chroma reads from memory is fetched in front of the luma transform, where a workgroup may wait for its QP -- behind the wait it is on the
  // path from one group's decision to the next
  uint32_t src_c = 0;
  if (RC) {
    chroma_windows();
    src_c = *(const uint16_t *)&f.src[1 + (tid >> 7)][(size_t)((y0 >> 1) + ((tid >> 3) & 15)) * cw2 + (x0 >> 1) + (tid & 7) * 2];
  }
  {
    __syncthreads();
    auto px16 = [](int tu, int y, int x) { return ((tu >> 1) * 16 + y) * 32 + (tu & 1) * 16 + x; };
    const int cw = f.cw; int16_t *base = f.coef[0] + (size_t)y0 * cw + x0;
    auto ci16 = [=](int tu, int y, int x) { return base + (size_t)((tu >> 1) * 16 + y) * cw + (tu & 1) * 16 + x; };
    if constexpr (LL) { }
    else if (split) inter_transform<4, 2, RC>(s, qp, &s.nz[0], px16, ci16, tid, adj, qp_late, &rc_cost, f.scaling ? f.scaling + scaling_offset(4, 0, 1) : nullptr, 4);
    else inter_transform_32<RC>(s, qp, &s.nz[0], base, cw, tid, adj, qp_late, &rc_cost, f.scaling ? f.scaling + scaling_offset(5, 0, 1) : nullptr);
    *(uint32_t *)&f.rec[0][(size_t)(y0 + (tid >> 3)) * f.cw + x0 + (tid & 7) * 4] = *(const uint32_t *)&s.px[(tid >> 3) * 32 + (tid & 7) * 4];
  }
  if (!RC) chroma_windows();
  __syncthreads();                           // (also: every thread has copied its luma samples out of s.px)
  {
    // two samples per thread; the separable 4-tap form with the {0, 64, 0, 0} filter at fraction 0 covers every case of
    // 8.5.3.3.3.2 exactly: (64 * t) >> 6 == t
    const int pl = tid >> 7, y = (tid >> 3) & 15, x = (tid & 7) * 2, sub = (y >> 3) * 2 + (x >> 3), k = split ? sub : 0;
    const int xf = s.mv[k][0] & 7, yf = s.mv[k][1] & 7;
    const uint8_t *w = &s.win[pl][sub][(y & 7) * 12 + (x & 7)];
    int v0 = 0, v1 = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      int c[5];
#pragma unroll
      for (int i = 0; i < 5; i++) c[i] = w[j * 12 + i];
      int t0 = 0, t1 = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) { t0 += kChromaFilter[xf][i] * c[i]; t1 += kChromaFilter[xf][i] * c[i + 1]; }
      v0 += kChromaFilter[yf][j] * t0; v1 += kChromaFilter[yf][j] * t1;
    }
    const int p0 = clip8(((v0 >> 6) + 32) >> 6), p1 = clip8(((v1 >> 6) + 32) >> 6);
    *(uint16_t *)&s.px[pl * 256 + y * 16 + x] = (uint16_t)(p0 | (p1 << 8));
    const int cl2 = split ? 3 : 4, cn = 1 << cl2, tu = pl * (split ? 4 : 1) + (split ? sub : 0);
    const size_t g = (size_t)((y0 >> 1) + y) * cw2 + (x0 >> 1) + x;
    int16_t *A = s.A + (tu << (2 * cl2));
    const int ty = y & (cn - 1), tx = x & (cn - 1);
    const uint32_t s2 = RC ? src_c : *(const uint16_t *)&f.src[1 + pl][g];
    const uint32_t r2 = s.intra_q[sub] ? 0u : pack_i16((int)(s2 & 255) - p0, (int)(s2 >> 8) - p1);
    if constexpr (LL) {
      *(uint32_t *)&f.coef[1 + pl][g] = r2;
      if (r2) atomicOr(&s.nz[1], 1u << tu);
      if (!s.intra_q[sub]) *(uint16_t *)&s.px[pl * 256 + y * 16 + x] = (uint16_t)s2;
    } else *(uint32_t *)&A[ty * cn + tx] = r2;
  }
  __syncthreads();
  {
    auto px1 = [](int tu, int y, int x) { return tu * 256 + y * 16 + x; };
    auto px4 = [](int tu, int y, int x) { return (tu >> 2) * 256 + (((tu >> 1) & 1) * 8 + y) * 16 + (tu & 1) * 8 + x; };
    const size_t base = (size_t)(y0 >> 1) * cw2 + (x0 >> 1);
    int16_t *cb = f.coef[1] + base, *cr = f.coef[2] + base;
    auto ci1 = [=](int tu, int y, int x) { return (tu ? cr : cb) + (size_t)y * cw2 + x; };
    auto ci4 = [=](int tu, int y, int x) { return ((tu >> 2) ? cr : cb) + (size_t)(((tu >> 1) & 1) * 8 + y) * cw2 + (tu & 1) * 8 + x; };
    auto qpc_known = [&]() -> int { return qpc; };
    if constexpr (LL) { }
    else if (split) inter_transform<3, 1, RC>(s, qpc, &s.nz[1], px4, ci4, tid, adj, qpc_known, &rc_cost, f.scaling ? f.scaling + scaling_offset(3, 1, 1) : nullptr, 4);
    else inter_transform<4, 1, RC>(s, qpc, &s.nz[1], px1, ci1, tid, adj, qpc_known, &rc_cost, f.scaling ? f.scaling + scaling_offset(4, 1, 1) : nullptr, 1);
  }
  if (tid < 128) {
    const int pl = tid >> 6, y = (tid >> 2) & 15, x = (tid & 3) * 4;
    *(uint32_t *)&f.rec[1 + pl][(size_t)((y0 >> 1) + y) * cw2 + (x0 >> 1) + x] = *(const uint32_t *)&s.px[pl * 256 + y * 16 + x];
  }
  if (tid < 16) {
    int bx = tid & 3, by = tid >> 2, k = split ? ((by >> 1) * 2 + (bx >> 1)) : 0;
    int cbf = (int)((s.nz[0] >> k) & 1);
    if (split) cbf |= (int)((s.nz[1] >> k) & 1) << 1 | (int)((s.nz[1] >> (4 + k)) & 1) << 2;
    else cbf |= (int)(s.nz[1] & 1) << 1 | (int)((s.nz[1] >> 1) & 1) << 2;
    f.cu_cbf[b8idx(f, x0 + bx * 8, y0 + by * 8)] = (uint8_t)cbf;
  }
  if constexpr (RC) rc_group_done(f, s, grp, rc_cost, tid);
}

// One thread per 8x8 unit: it derives the signalling of the CU it lies in and writes its OWN five entries -- every unit of a CU (4 of a 16x16, 16 of a
// 32x32) derives the same values from the same few bytes (cache hits), so nobody loops over a CU's units storing single bytes and a wave's stores are
// consecutive.  In workgroups of 1024: the kernel is ~1 600 instructions of straight-line code that every wave runs once, and what it costs is FETCHING that
// code -- a launch that only reads the size byte and writes the entries takes 6.0 us (the floor), the derivation with the same threads in workgroups of 64
// (510 of them, a wave or two on every compute unit, each fetching the code for itself) 31 us, in workgroups of 256 13.8 - 21 us, 512 10.9, 1024 10.0
// (profiles/r05_inter_signal_variants.txt; one box, isolated).  Round 4's form (a thread per 16x16 block, 128 workgroups of 64): 22 us; staging the records
// in LDS, one workgroup per CTU: 28 - 32 us (twice the waves, a barrier) -- it was never the round trips to memory.
// TMVP ("tmvp"): the temporal candidates come from the previous picture's collocated record (f.col_prev, NULL right after the IDR
// picture), and the thread at each 16x16 origin files this picture's (f.col_out).  Both on the tokenizer's stream in picture order, which orders the write
// of picture t - 1 before the read of picture t, and the read of t before the write of t + kSets - 1 into the same set's record.  A separate
// instantiation: without tmvp the launch runs the code of before.
// GOP ("lp-gop"): the references' POC distances come from the picture's table (f.ref_dist) instead of ref_idx + 1 -- AMVP's spatial scaling,
// the temporal candidates and the record filed.  The table forms are instantiations of their own: the launches without the option run the code of before.
template <bool TMVP, bool GOP = false>
__global__ __launch_bounds__(1024) void k_inter_signal(EncFrame f)
{
  const int w8 = f.cw >> 3, h8 = band_rows(f) * 8;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < w8 * h8;
  const int x = valid ? (i % w8) * 8 : 0, y = valid ? (i / w8) * 8 + f.row0 * 64 : 0, g = b8idx(f, x, y);
  const int cl = f.cu_log2[g];
  const bool intra = f.cu_intra[g] != 0;                // an intra unit in a P picture (intra-in-P)
  int flags = 0;
  if (valid && !intra) {
    const int n = 1 << cl;
    CuSignal r;
    // (inlined on purpose: left to itself the compiler makes the longer TMVP derivation a call, with a 1 KB stack frame in scratch memory per thread)
    if constexpr (GOP) { FrameMvView v{f}; [[clang::always_inline]] r = decide_signalling_values(v, f.cw, f.chp, x & ~(n - 1), y & ~(n - 1), cl, f.cu_ref && f.nref > 1 ? f.nref : 1, TMVP ? f.col_prev : nullptr, TabDist{f.ref_dist}); }
    else if constexpr (TMVP) { FrameMvView v{f}; [[clang::always_inline]] r = decide_signalling_values(v, f.cw, f.chp, x & ~(n - 1), y & ~(n - 1), cl, f.cu_ref && f.nref > 1 ? f.nref : 1, f.col_prev); }
    else r = decide_signalling_values(f, x & ~(n - 1), y & ~(n - 1), cl);
    flags = r.flags;
    f.cu_flags[g] = (uint8_t)r.flags; f.cu_merge_idx[g] = (uint8_t)r.midx; f.cu_mvp_idx[g] = (uint8_t)r.mvp;
    *reinterpret_cast<uint32_t *>(&f.cu_mvd[g * 2]) = ((uint32_t)r.mvdx & 0xffffu) | ((uint32_t)r.mvdy << 16);
  }
  if constexpr (TMVP) {
    if (valid && !((x | y) & 15)) {
      ColMv c; c.mx = intra ? 0 : f.cu_mv[g * 2]; c.my = intra ? 0 : f.cu_mv[g * 2 + 1]; c.dist = intra ? 0 : (int16_t)(GOP ? TabDist{f.ref_dist}(cu_ref_at(f, g)) : cu_ref_at(f, g) + 1); c.pad = 0;
      f.col_out[(y >> 4) * (f.cw >> 4) + (x >> 4)] = c;
    }
  }
  // The tokenizer's work list (EncFrame::tok_list): of a P picture's 4 x units (unit, role) pairs nine in ten have nothing to say -- units inside a 32x32 coding
  // unit that starts elsewhere, colour components without residual -- and a wave each to find that out WAS k_tokenize's launch (32 640 waves at 1080p, 130 000
  // at 2160p).  The thread at a 16x16 unit's origin knows all of it: the unit's coding unit(s), this very thread's skip decision, the cbf bits (final: the
  // reconstruction is behind us).  Roles: 0 luma, 1 Cb, 2 Cr, 3 headers (and, for the CTU's last unit, its terminating bins).  One atomic per wave.
  if (f.tok_list) {
    uint32_t roles = 0;
    if (valid && !((x | y) & 15)) {
      const bool owner = !(cl == 5 && ((x | y) & 31));
      if (owner || ((x & 63) == 48 && (y & 63) == 48)) roles |= 8u;
      if (owner) {
        uint32_t cbf = 0;
        if (cl == 3) { cbf = f.cu_cbf[g] | f.cu_cbf[g + 1] | f.cu_cbf[g + w8] | f.cu_cbf[g + w8 + 1]; }      // four 8x8 coding units (intra units: never skipped)
        else if (!(flags & CU_SKIP)) cbf = f.cu_cbf[g];
        roles |= cbf & 7u;
      }
    }
    const int lane = threadIdx.x & 63, nr = __builtin_popcount(roles);
    int pre = nr;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(pre, o); if (lane >= o) pre += t; }
    const int total = __shfl(pre, 63);
    uint32_t base = 0;
    if (lane == 63 && total) base = atomicAdd(&f.tok_list[0], (uint32_t)total);
    base = (uint32_t)__shfl((int)base, 63);
    uint32_t o = base + (uint32_t)(pre - nr);
    const uint32_t unit = (uint32_t)((y >> 4) * (f.cw >> 4) + (x >> 4));
    for (uint32_t m = roles; m; m &= m - 1) f.tok_list[1 + o++] = (unit << 2) | (uint32_t)__builtin_ctz(m);
  }
}

// =============================================================================================
// Intra reconstruction.  Intra prediction of a block needs the reconstructed samples of its left /
// above neighbours, so inside one colour plane the blocks of a picture form a dependency chain:
// z-order inside a CTU, a two-CTU lag between CTU rows.  What is independent is the three colour
// planes (DM chroma uses the luma *mode*, not luma samples).  So: one WAVE per (CTU row, plane),
// launched as a 64-thread workgroup; nothing inside the chain ever waits for another wave, the
// steps of a block talk through LDS under wave-local barriers, and rows hand over through agent
// -scope progress counters (one per row and plane).  The CTU being coded, its borders, its source
// samples and its levels stay in LDS; global memory is touched once per CTU on the way in and out.
//
// Transforms: one primitive, P(X, T)[j][i] = sum_m X[i][m] * T[j][m] (rows of X times rows of T,
// result stored transposed), run four times -- forward rows, forward columns, inverse columns,
// inverse rows -- on int16 data with v_dot2_i32_i16.  A lane owns a pair of rows of X and OPL
// outputs of each, so the matrix rows it reads are shared by both rows and every LDS write is a
// packed pair.  Quantisation and dequantisation are the epilogue of the second forward stage, the
// reconstruction is the epilogue of the last inverse stage.
// =============================================================================================
#ifdef KVZ_PROF     // tools/intra_prof.py: cycle attribution inside the chain (never defined in the product build)
__shared__ long long g_prof[16];
#define PROF(k) do { if (threadIdx.x == 0) { long long t_ = clock64(); g_prof[k] += t_ - g_prof[15]; g_prof[15] = t_; } } while (0)
#else
#define PROF(k) do { } while (0)
#endif
struct IntraCtuLds {
  // The CTU being reconstructed with its borders, as one padded picture: row 0 = the sample row above the CTU
  // (above-left corner, above, above-right), column 15 = the sample column to its left, sample (x, y) of the
  // CTU at pic[(y + 1) * P + 16 + x], P = 16 + 2S.
  alignas(16) uint8_t pic[65 * 144];
  alignas(16) uint8_t src[64 * 64];          // source samples of the CTU
  alignas(16) int16_t lev[64 * 64];          // levels produced
  alignas(16) XfLaneF16 xf[4][64];           // matrix operands of the transform stages, per (transform, lane)
};

// =============================================================================================
// Intra analysis (IDR pictures): for every 8x8 and 16x16 block of a 32x32 region the SAD of all 35
// prediction modes against the SOURCE picture, predictions built from source neighbours (so nothing depends
// on reconstruction and the whole picture is searched in parallel); then the bottom-up split decision.  Intra
// coding units are 16x16 or 8x8 (Kvazaar's ultrafast shape; oracle/hevc_enc.c intra_decide() has the reason).
// The reference arrays of all 20 blocks are built once into LDS (scan order, as in the reconstruction
// kernel); a work item is (block, mode), one wave each: the mode is wave-uniform, 64 samples per step, the
// SAD is summed with DPP row operations.
// =============================================================================================

struct AnalyseLds {
  alignas(16) uint8_t src[32 * 32];
  // per block b (0..15: 8x8 raster, 16..19: 16x16 raster, 20: 32x32): unfiltered / filtered references, scan order, at
  // R[f][roff(b)]; sizes 33 / 65 / 129 entries
  alignas(16) uint8_t R[2][16 * 36 + 4 * 68 + 132];
  int dc[21];
  uint32_t cost[21][35];
  uint32_t bestc[21]; int bestm[21];
  int last;                                // intra-in-P: this workgroup is the last of its region's to arrive
  alignas(16) uint8_t srcT[32 * 32];       // src transposed (the horizontal modes' tiles: analyse_tile_satd)
  alignas(16) uint8_t ext[16][4 * 32];     // per wave: the reference samples of the item's block(s) as the array its mode walks along (analyse_tile_satd)
};
__device__ __forceinline__ int an_tile_of(int b) { return b < 16 ? (b >> 3) * 2 + ((b >> 1) & 1) : b - 16; }      // the 16x16 quarter block b (0..19) lies in
__device__ __forceinline__ int an_roff(int b) { return b < 16 ? b * 36 : (b < 20 ? 16 * 36 + (b - 16) * 68 : 16 * 36 + 4 * 68); }

template <int L2>
__device__ __forceinline__ uint32_t analyse_item(const AnalyseLds &s, int b, int bx, int by, int mode, int lane)
{
  constexpr int N = 1 << L2;
  const bool filt = intra_filter_needed(N, 0, mode);
  const uint8_t *R = s.R[filt ? 1 : 0] + an_roff(b);
  const int angle = kIntraAngle[mode], inv = kInvAngle[mode];
  const bool edge = N < 32, vert = mode >= 18, e2 = edge && (mode == 26 || mode == 10);
  const int dcv = s.dc[b];
  uint32_t sad = 0;
#pragma unroll
  for (int it = 0; it < N * N / 64; it++) {
    const int pxi = it * 64 + lane, y = pxi >> L2, x = pxi & (N - 1);
    int p;
    if (mode == 0) p = pred_planar<L2>(R, x, y);
    else if (mode == 1) p = pred_dc<L2>(R, edge, dcv, x, y);
    else p = pred_angular<L2>(R, vert, e2, angle, inv, x, y);
    sad += (uint32_t)iabs((int)s.src[(by + y) * 32 + bx + x] - p);
  }
  return wave_sum_u32(sad);
}

// SATD form of the search cost (f.satd): one item = (16x16 tile of the region, mode, kind) on one wave.  kind 0 predicts the tile as
// one 16x16 block, kind 1 as its four 8x8 blocks; either way the tile's difference to the source goes through the 8x8 Hadamard
// transform of each of its quadrants as ONE pair of matrix-core products: with H16 = H8 (+) H8 (block diagonal, entries +-1)
//   Y = D H16^T    (A = the differences, lane (g, c) = (lane >> 4, lane & 15) owns x = 4g .. 4g + 3 of row y = c)
//   Z = H16 Y      (B = Y, which the first product leaves in exactly the operand layout the second one reads)
// on v_mfma_f32_16x16x16_f16 -- exact: |D| <= 255, |Y| <= 2040 < 2^11, |Z| <= 16320.  q[k] = sum |Z| over quadrant k (raster).
__device__ __forceinline__ void analyse_tile_satd(AnalyseLds &s, int wave, int tile, int kind, int mode, int lane, uint32_t (&q)[4])
{
  const int g = lane >> 4, c = lane & 15, tx = (tile & 1) * 16, ty = (tile >> 1) * 16;
  int d[4];
  if (mode < 2) {
    // planar and DC (2 of 35 items): sample by sample
    const uint32_t s4 = *(const uint32_t *)&s.src[(ty + c) * 32 + tx + 4 * g];
    if (kind == 0) {
      const int b = 16 + tile;
      const uint8_t *R = s.R[intra_filter_needed(16, 0, mode) ? 1 : 0] + an_roff(b);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int x = 4 * g + r, y = c;
        const int p = mode == 0 ? pred_planar<4>(R, x, y) : pred_dc<4>(R, true, s.dc[b], x, y);
        d[r] = (int)((s4 >> (8 * r)) & 255u) - p;
      }
    } else {
      const int b = ((ty >> 3) + (c >> 3)) * 4 + (tx >> 3) + (g >> 1);
      const uint8_t *R = s.R[intra_filter_needed(8, 0, mode) ? 1 : 0] + an_roff(b);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int x = (4 * g + r) & 7, y = c & 7;
        const int p = mode == 0 ? pred_planar<3>(R, x, y) : pred_dc<3>(R, true, s.dc[b], x, y);
        d[r] = (int)((s4 >> (8 * r)) & 255u) - p;
      }
    }
  } else {
    // The 33 angular modes, all in the VERTICAL form: a horizontal mode predicts the transposed block from the left column the way a vertical mode predicts
    // the block from the row above (8.4.4.2.6 is symmetric in x and y), and the Hadamard cost of a transposed difference block is the cost of the block
    // (H D' H = (H D H)' for the symmetric H) -- so the tile is taken from the transposed copy of the source, and the quadrant sums q[1], q[2] change places
    // at the end.  Per item the wave first lays the block's reference samples out as the ONE array the mode walks along, ext[N + k] = ref[k] for
    // k = -N .. 2N + 1 (negative k: the other side's samples projected with the inverse angle), N bytes in front of the corner; then lane (g, c) -- row c,
    // samples 4g .. 4g + 3 -- needs ONE offset and ONE fraction (both depend on the row only), five consecutive bytes of ext (one aligned 8-byte read, a
    // byte shift) and four blends: no branch, no sign test per sample, no multiplication by the inverse angle outside the lay-out.
    const int ai = kAngInv.v[mode], angle = (int)(int16_t)(ai & 0xffff), inv = ai >> 16;
    const bool vert = mode >= 18, e2 = mode == 26 || mode == 10;
    const int sgn = vert ? 1 : -1;
    uint8_t *ext = s.ext[wave];
    const uint32_t s4 = vert ? *(const uint32_t *)&s.src[(ty + c) * 32 + tx + 4 * g] : *(const uint32_t *)&s.srcT[(tx + c) * 32 + ty + 4 * g];
    wave_sync();                                              // (the last item's reads of ext are done)
    int row, x0, N;
    const uint8_t *Rl, *el;                                   // the lane's block: its reference array, its ext
    if (kind == 0) {
      const uint8_t *R = s.R[intra_filter_needed(16, 0, mode) ? 1 : 0] + an_roff(16 + tile);
      const int k = lane - 16;
      const int idx = k >= 0 ? imin(k, 32) : imax(-((k * inv + 128) >> 8), -32);
      ext[lane] = R[32 + sgn * idx];
      row = c; x0 = 4 * g; N = 16; Rl = R; el = ext;
    } else {
      const uint8_t *R0 = s.R[intra_filter_needed(8, 0, mode) ? 1 : 0];
#pragma unroll
      for (int hh = 0; hh < 2; hh++) {
        const int e = lane + 64 * hh, slot = e >> 5, k = (e & 31) - 8;       // slot: the quadrant (sy', sx') of the tile as the lanes see it
        const int sx = vert ? (slot & 1) : (slot >> 1), sy = vert ? (slot >> 1) : (slot & 1);
        const uint8_t *R = R0 + an_roff(((ty >> 3) + sy) * 4 + (tx >> 3) + sx);
        const int idx = k >= 0 ? imin(k, 16) : imax(-((k * inv + 128) >> 8), -16);
        ext[e] = R[16 + sgn * idx];
      }
      const int slot = (c >> 3) * 2 + (g >> 1);
      const int sx = vert ? (slot & 1) : (slot >> 1), sy = vert ? (slot >> 1) : (slot & 1);
      row = c & 7; x0 = (4 * g) & 7; N = 8; Rl = R0 + an_roff(((ty >> 3) + sy) * 4 + (tx >> 3) + sx); el = ext + slot * 32;
    }
    wave_sync();
    const int t = (row + 1) * angle, fr = t & 31, j0 = N + x0 + (t >> 5) + 1;
    const uint32_t *w = (const uint32_t *)(el + (j0 & ~3));
    const uint32_t lo = w[0], hi = w[1];
    const uint32_t sh = (uint32_t)(j0 & 3);
    const uint32_t b03 = __builtin_amdgcn_alignbyte(hi, lo, sh), b4 = (hi >> (8 * sh)) & 255u;
    int B[5] = {(int)(b03 & 255u), (int)((b03 >> 8) & 255u), (int)((b03 >> 16) & 255u), (int)(b03 >> 24), (int)b4};
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int p = (32 * B[r] + fr * (B[r + 1] - B[r]) + 16) >> 5;
      d[r] = (int)((s4 >> (8 * r)) & 255u) - p;
    }
    if (e2 && x0 == 0) d[0] = (int)(s4 & 255u) - clip8(Rl[2 * N + sgn] + ((Rl[2 * N - sgn * (1 + row)] - Rl[2 * N]) >> 1));      // (8.4.4.2.6: the edge of the pure vertical / horizontal mode)
  }
  // H16[c][4g + r]: zero across the two 8x8 blocks, else the sign of the natural-ordered Hadamard matrix, (-1)^popcount(i & j)
  kv_f16x4 h;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int j = 4 * g + r;
    h[r] = ((c ^ j) & 8) ? (_Float16)0.f : ((__builtin_popcount((unsigned)(c & j & 7)) & 1) ? (_Float16)-1.f : (_Float16)1.f);
  }
  // Both products and the sum of magnitudes stay in floating point -- every value is an integer below 2^17, exact in f32, and Y (|y| <= 2040) is exact in
  // f16 --: the first product's result goes back in as packed halves (v_cvt_pkrtz: two per instruction, nothing to round), the magnitudes are source
  // modifiers of the adds, and ONE conversion per lane is left, after the lane sums (was 4 + 4 + 4 conversions and 8 integer abs steps per item: 154 -> 142 us).
  // (Tried and dropped: the 18 modes that never reach behind the corner reading their five reference bytes straight from R[] instead of laying out ext[] --
  // 142 -> 154 us: two code paths in the item loop cost more than the lay-out they save.)
  kv_f16x4 da;
#pragma unroll
  for (int r = 0; r < 4; r++) da[r] = (_Float16)(short)d[r];
  const kv_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const kv_f32x4 yf = __builtin_amdgcn_mfma_f32_16x16x16f16(da, h, zero, 0, 0, 0);
  typedef __fp16 kv_h2_ __attribute__((ext_vector_type(2)));
  const kv_h2_ y01 = __builtin_amdgcn_cvt_pkrtz(yf[0], yf[1]), y23 = __builtin_amdgcn_cvt_pkrtz(yf[2], yf[3]);
  struct { kv_h2_ lo, hi; } ypk = {y01, y23};
  const kv_f16x4 yb = __builtin_bit_cast(kv_f16x4, ypk);
  const kv_f32x4 zf = __builtin_amdgcn_mfma_f32_16x16x16f16(h, yb, zero, 0, 0, 0);
  float af = (__builtin_fabsf(zf[0]) + __builtin_fabsf(zf[1])) + (__builtin_fabsf(zf[2]) + __builtin_fabsf(zf[3]));
  // sums over the 8-lane groups (three DPP steps), then the two groups of each quadrant: output (u = 4g + r, v = c) lies in quadrant
  // (u >= 8) * 2 + (v >= 8)
  af += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, af), 0xB1, 0xf, 0xf, false));
  af += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, af), 0x4E, 0xf, 0xf, false));
  af += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, af), 0x141, 0xf, 0xf, false));
  const uint32_t a = (uint32_t)af;
  q[0] = (uint32_t)__builtin_amdgcn_readlane((int)a, 0) + (uint32_t)__builtin_amdgcn_readlane((int)a, 16);
  q[1] = (uint32_t)__builtin_amdgcn_readlane((int)a, 8) + (uint32_t)__builtin_amdgcn_readlane((int)a, 24);
  q[2] = (uint32_t)__builtin_amdgcn_readlane((int)a, 32) + (uint32_t)__builtin_amdgcn_readlane((int)a, 48);
  q[3] = (uint32_t)__builtin_amdgcn_readlane((int)a, 40) + (uint32_t)__builtin_amdgcn_readlane((int)a, 56);
  if (mode >= 2 && mode < 18) { const uint32_t t_ = q[1]; q[1] = q[2]; q[2] = t_; }      // (a horizontal mode's tile was transposed)
}

// PP = false: intra pictures.  PP = true ("uvgx intra-in-P v1"): launched behind k_me in a P picture; a region none of whose quarters'
// inter cost is above the gate leaves at once (nearly all of them), the others are analysed like an intra picture's and the quarters
// that come out cheaper as intra blocks are turned into intra units.
// IR (intra-refresh; with PP): the quarters k_me<.., true> sent with the cost 0xffffffff are the band's -- they pass the gate and the price
// comparison as they stand -- and a forced unit on the band's last unit column keeps to the modes that read no above-right samples (ir_last_column), beside
// the rules of intra-chain.  A form of its own: the launches without the option run the code of before.
template <bool PP, bool IR = false>
__global__ __launch_bounds__(PP ? 1024 : 256) void k_intra_analyse(EncFrame f)
{
  // (PP: few regions get past the gate, so what counts is how long ONE of them takes, not how many fit on the chip: sixteen waves share its items)
  constexpr int T = PP ? 1024 : 256, NW = T / 64;
  __shared__ AnalyseLds s;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (a scalar: item, mode, kind and tile of the search loops are wave-uniform, and the compiler cannot know)
  int bx_ = 0, by_ = 0;
  if (!PP) xcd_block_2d(bx_, by_);
  // PP: a fixed number of workgroups works through the list of blocks k_me found above the gate (f.me_cand); the first things they do is
  // zero what k_intra_recon<.., true> starts from: the progress counters of every CTU and the ticket counter behind them
  const uint32_t ncand = PP ? f.me_cand[0] : 1u;
  if (PP) for (uint32_t i = blockIdx.x * T + tid; i < 3u * (uint32_t)(f.cw >> 6) * (uint32_t)(f.ch >> 6) + 1u; i += gridDim.x * T) f.sync[i] = 0;      // (the word behind the ticket counter says whether the picture has an intra unit at all: set below, zeroed by k_deblock_tile)
  // PP: a work item is one QUARTER of a listed block (a quarter's 70 (size, mode) prices over sixteen waves are a third of the latency of the block's 280:
  // 43 -> 16 us for the launch); the quarters' workgroups leave their best prices in f.ip_scratch, and the last of a block's to arrive takes the decision
  for (uint32_t item = PP ? blockIdx.x : 0u; item < (PP ? 4u * ncand : 1u); item += PP ? gridDim.x : 1u) {
  const int mytile = PP ? (int)(item & 3u) : -1;
  const uint32_t ci = PP ? item >> 2 : 0u;
  auto mine = [&](int b) { return !PP || an_tile_of(b) == mytile; };
  if (PP) { __syncthreads(); const uint32_t r = f.me_cand[1 + ci]; bx_ = (int)(r % (uint32_t)(f.cw >> 5)); by_ = (int)(r / (uint32_t)(f.cw >> 5)); }      // (the barrier: LDS of the last item is free)
  const int X0 = bx_ * 32, Y0 = by_ * 32 + f.row0 * 64;
  uint32_t icost[4] = {0, 0, 0, 0}; bool cand[4] = {false, false, false, false};
  if (PP) {
    for (int k = 0; k < 4; k++) {
      icost[k] = f.me_cost16[((Y0 >> 4) + (k >> 1)) * (f.cw >> 4) + (X0 >> 4) + (k & 1)];
      cand[k] = icost[k] > (uint32_t)INTRA_P_GATE * (uint32_t)f.lambda_q4;
    }
    if (!cand[mytile]) continue;                                // (only the quarters above the gate are priced)
  }
  const uint8_t *src = f.src[0];
  if (tid < 256) *(uint32_t *)&s.src[tid * 4] = *(const uint32_t *)&src[(size_t)(Y0 + (tid >> 3)) * f.cw + X0 + (tid & 7) * 4];
  // ---- references of the 21 blocks from the source picture (8.4.4.2.2 substitution as an index clamp: the available
  // groups are contiguous in scan order; availability by picture bounds and z-scan order)
  for (int e = tid; e < 16 * 33 + 4 * 65; e += T) {
    int b, i, l2;
    if (e < 16 * 33) { b = e / 33; i = e - b * 33; l2 = 3; } else { int r = e - 16 * 33; b = 16 + r / 65; i = r % 65; l2 = 4; }
    if (!mine(b)) continue;
    const int n = 1 << l2, bi = b < 16 ? b : b - 16, nb = 32 >> l2;
    const int x0 = X0 + (bi % nb) * n, y0 = Y0 + (bi / nb) * n;
    const bool aL = avail64(f.cw, f.chp, x0, y0, x0 - 1, y0), aT = avail64(f.cw, f.chp, x0, y0, x0, y0 - 1);
    const bool aBL = aL && avail64(f.cw, f.chp, x0, y0, x0 - 1, y0 + n), aTR = aT && avail64(f.cw, f.chp, x0, y0, x0 + n, y0 - 1);
    const int lo = aBL ? 0 : (aL ? n : 2 * n + 1), hi = aTR ? 4 * n : (aT ? 3 * n : (aL ? 2 * n - 1 : -1));
    int v = 128;
    if (hi >= 0) {
      const int j = imin(imax(i, lo), hi);
      const int x = j < 2 * n ? x0 - 1 : x0 + j - 2 * n - 1, y = j < 2 * n ? y0 + 2 * n - 1 - j : y0 - 1;
      v = src[(size_t)y * f.cw + x];
    }
    s.R[0][an_roff(b) + i] = (uint8_t)v;
  }
  __syncthreads();
  // ---- filtered references (8.4.4.2.3) and DC values; the source block transposed (analyse_tile_satd)
  if (f.satd && tid < 256) {
    const uint32_t v = *(const uint32_t *)&s.src[tid * 4];
    const int y = tid >> 3, x = (tid & 7) * 4;
#pragma unroll
    for (int r = 0; r < 4; r++) s.srcT[(x + r) * 32 + y] = (uint8_t)(v >> (8 * r));
  }
  for (int e = tid; e < 16 * 33 + 4 * 65; e += T) {
    int b, i, l2;
    if (e < 16 * 33) { b = e / 33; i = e - b * 33; l2 = 3; } else { int r = e - 16 * 33; b = 16 + r / 65; i = r % 65; l2 = 4; }
    if (!mine(b)) continue;
    const int n = 1 << l2;
    const uint8_t *R = s.R[0] + an_roff(b);
    int fv = R[i];
    if (i != 0 && i != 4 * n) {
      const bool strong = n == 32 && iabs(R[2 * n] + R[4 * n] - 2 * R[3 * n]) < 8 && iabs(R[2 * n] + R[0] - 2 * R[n]) < 8;
      if (strong) { if (i != 2 * n) { int k = i < 2 * n ? 2 * n - i : i - 2 * n; fv = ((64 - k) * R[2 * n] + k * (i < 2 * n ? R[0] : R[4 * n]) + 32) >> 6; } }
      else fv = (R[i - 1] + 2 * R[i] + R[i + 1] + 2) >> 2;
    }
    s.R[1][an_roff(b) + i] = (uint8_t)fv;
  }
  if (tid < 20 && mine(tid)) {
    const int l2 = tid < 16 ? 3 : 4, n = 1 << l2;
    const uint8_t *R = s.R[0] + an_roff(tid);
    int a = n;
    for (int i = n; i <= 3 * n; i++) a += R[i];
    s.dc[tid] = (a - R[2 * n]) >> (l2 + 1);
  }
  __syncthreads();
  // ---- cost of every (block, mode): 8x8 Hadamard sums, (sum + 2) >> 2 per 8x8 block (oracle/hevc_enc.c satd_block()), or SADs
  if (f.satd) {
    const bool no8 = PP && f.intra_p == 1;                          // intra-in-p = 1: 16x16 intra units only -- the 8x8 blocks are not priced
    for (int j = wave; j < (PP ? (no8 ? 35 : 35 * 2) : 4 * 35 * 2); j += NW) {
      const int item = PP ? (no8 ? (j << 3) | (mytile << 1) : ((j >> 1) << 3) | (mytile << 1) | (j & 1)) : j;
      const int kind = item & 1, tile = (item >> 1) & 3, mode = item >> 3;
      uint32_t q[4];
      analyse_tile_satd(s, wave, tile, kind, mode, lane, q);
      if (lane == 0) {
        if (kind == 0) s.cost[16 + tile][mode] = ((q[0] + 2) >> 2) + ((q[1] + 2) >> 2) + ((q[2] + 2) >> 2) + ((q[3] + 2) >> 2);
        else {
          const int b0 = (tile >> 1) * 8 + (tile & 1) * 2;           // first of the tile's four 8x8 blocks (raster of 4 x 4)
          s.cost[b0][mode] = (q[0] + 2) >> 2; s.cost[b0 + 1][mode] = (q[1] + 2) >> 2; s.cost[b0 + 4][mode] = (q[2] + 2) >> 2; s.cost[b0 + 5][mode] = (q[3] + 2) >> 2;
        }
      }
    }
  } else
  for (int j = wave; j < (PP ? (f.intra_p == 1 ? 35 : 5 * 35) : 20 * 35); j += NW) {
    int b = j / 35; const int mode = j - b * 35;
    if (PP && f.intra_p == 1) b = 16 + mytile;
    else if (PP) b = b < 4 ? (mytile >> 1) * 8 + (mytile & 1) * 2 + (b >> 1) * 4 + (b & 1) : 16 + mytile;      // the quarter's four 8x8 blocks and its 16x16 block
    uint32_t c;
    if (b < 16) c = analyse_item<3>(s, b, (b & 3) * 8, (b >> 2) * 8, mode, lane);
    else c = analyse_item<4>(s, b, ((b - 16) & 1) * 16, ((b - 16) >> 1) * 16, mode, lane);
    if (lane == 0) s.cost[b][mode] = c;
  }
  __syncthreads();
  if (tid < 20 && mine(tid)) {
    uint32_t bc = 0xffffffffu; int bm = 0;
    uint64_t excl = 0;                                       // "intra-chain": modes this block may not take (statement: intra_analyse_size(), oracle/hevc_enc.c)
    if (f.intra_chain) {
      const int l2b = tid < 16 ? 3 : 4, nb_ = 1 << l2b, bib = tid < 16 ? tid : tid - 16, nbb = 32 >> l2b;
      const int xb = X0 + (bib % nbb) * nb_, yb = Y0 + (bib / nbb) * nb_;
      if ((yb & 63) == 0 && ((xb + nb_) & 63) == 0 && avail64(f.cw, f.chp, xb, yb, xb + nb_, yb - 1)) excl |= intra_uses_above_right(l2b, 0);      // the CTU's above-right corner block
      if ((xb & 63) == 0 && avail64(f.cw, f.chp, xb, yb, xb - 1, yb + nb_)) excl |= intra_uses_below_left(l2b, 0);                                  // a block on the CTU's left edge
    }
    if constexpr (IR) {
      const int l2b = tid < 16 ? 3 : 4, nb_ = 1 << l2b, bib = tid < 16 ? tid : tid - 16, nbb = 32 >> l2b;
      const int xb = X0 + (bib % nbb) * nb_, yb = Y0 + (bib / nbb) * nb_;
      if (ir_last_column(xb, nb_, f.ir_e, f.cw) && avail64(f.cw, f.chp, xb, yb, xb + nb_, yb - 1)) excl |= intra_uses_above_right(l2b, 0);      // beyond the band the reference picture is not clean yet
    }
    for (int m = 0; m < 35; m++) if (!((excl >> m) & 1) && s.cost[tid][m] < bc) { bc = s.cost[tid][m]; bm = m; }
    s.bestc[tid] = bc; s.bestm[tid] = bm;
    if (PP && cand[0] + cand[1] + cand[2] + cand[3] > 1) st_wt_u64(&f.ip_scratch[(size_t)ci * 20 + tid], (uint64_t)bc | ((uint64_t)bm << 32));      // for the block's other quarters
    const int l2 = tid < 16 ? 3 : 4, n = 1 << l2, bi = tid < 16 ? tid : tid - 16, nb = 32 >> l2;
    const int x0 = X0 + (bi % nb) * n, y0 = Y0 + (bi / nb) * n;
    const int bw = f.cw >> l2, ib = (y0 >> l2) * bw + (x0 >> l2);
    if (!PP) {
      if (l2 == 3) { f.im8[ib] = (uint8_t)bm; f.ic8[ib] = bc; }
      else { f.im16[ib] = (uint8_t)bm; f.ic16[ib] = bc; }
    }
  }
  if (PP && cand[0] + cand[1] + cand[2] + cand[3] > 1) {
    // the block's other quarters above the gate are other workgroups': the last one to arrive has everybody's prices (write-through stores, drained
    // before the count goes up; read past the caches) and decides -- nobody waits
    if (tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
      const bool last = atomicAdd(&f.ip_arrive[ci], 1u) == (uint32_t)(cand[0] + cand[1] + cand[2] + cand[3]) - 1u;
      if (last) f.ip_arrive[ci] = 0;                          // (for the next picture)
      s.last = last ? 1 : 0;
    }
    __syncthreads();
    if (!s.last) continue;
    if (tid < 20 && !mine(tid) && cand[an_tile_of(tid)]) { const uint64_t v = ld_l2_u64(&f.ip_scratch[(size_t)ci * 20 + tid]); s.bestc[tid] = (uint32_t)v; s.bestm[tid] = (int)(v >> 32); }
  }
  __syncthreads();
  // ---- bottom-up split decision for this 32x32 block: thread per 8x8 cell
  if (tid < 16) {
    const uint32_t pen = ((uint32_t)f.lambda_q4 * SPLIT_BITS) >> 4;
    bool split16[4], chosen = false;
    for (int k = 0; k < 4; k++) {
      uint32_t c8 = pen;
      for (int j = 0; j < 4; j++) c8 += s.bestc[((k >> 1) * 2 + (j >> 1)) * 4 + (k & 1) * 2 + (j & 1)];
      split16[k] = !(PP && f.intra_p == 1) && c8 < s.bestc[16 + k];
      if (PP) {                                                  // intra-in-P: the quarter goes intra when that is cheaper than what the search found
        const uint32_t cintra = (split16[k] ? c8 : s.bestc[16 + k]) + (((uint32_t)f.lambda_q4 * INTRA_P_BITS) >> 4);
        cand[k] = cand[k] && cintra < icost[k];
        chosen |= cand[k];
      }
    }
    const int bx = tid & 3, by = tid >> 2, k = (by >> 1) * 2 + (bx >> 1);
    const int i = ((Y0 >> 3) + by) * (f.cw >> 3) + (X0 >> 3) + bx;
    if (PP && chosen && tid == 0) f.sync[(size_t)3 * (f.cw >> 6) * (f.ch >> 6) + 1] = 1u;
    if (PP && !chosen) { }                                      // the block stays as the search left it
    else if (PP && !cand[k]) f.cu_log2[i] = 4;                  // an inter quarter beside an intra one: a 16x16 unit with the vector it has
    else {
      if (PP) { f.cu_mv[i * 2] = 0; f.cu_mv[i * 2 + 1] = 0; }
      int l2, mode;
      if (!split16[k]) { l2 = 4; mode = s.bestm[16 + k]; }
      else { l2 = 3; mode = s.bestm[tid]; }
      f.cu_log2[i] = (uint8_t)l2; f.cu_intra_mode[i] = (uint8_t)mode; f.cu_intra[i] = 1; f.cu_flags[i] = 0;
    }
  }
  }
}

// One plane of one CU on one wave (kernel_common.h "One intra block per WAVE"): block of n = 1 << L2 component samples.
// Returns whether the block has non-zero levels.
template <int L2, bool ADJ, bool LL = false>
__device__ __forceinline__ bool intra_block_wave(IntraCtuLds &s, IntraWaveScratch &ws, const IntraBlk &d, int cidx, int S, const QuantConst &q,
                                                 int lane, int adj, uint32_t *ecol, unsigned long long *erow, uint32_t gen, const uint8_t *mtab = nullptr)
{
  constexpr int N = 1 << L2;
  const int P = 16 + 2 * S, g = lane >> 4, c = lane & 15, rx = d.rx, ry = d.ry;
  const bool active = c < N && 4 * g < N;
  int pred[4], res[4] = {0, 0, 0, 0};
  wave_intra_predict<L2>(s.pic, P, ws, d, cidx == 0, lane, g, c, pred);
  if (active) {
    const uint32_t s4 = *(const uint32_t *)&s.src[(ry + c) * S + rx + 4 * g];
#pragma unroll
    for (int r = 0; r < 4; r++) res[r] = (int)((s4 >> (8 * r)) & 255u) - pred[r];
  }
  PROF(5);
  bool cbf;
  if constexpr (LL) {
    // cu_transquant_bypass (EncFrame.lossless): the levels ARE the residual, sample by sample, and the reconstruction is the source
    bool nzl = false;
    if (active) {
#pragma unroll
      for (int r = 0; r < 4; r++) { s.lev[(ry + c) * S + rx + 4 * g + r] = (int16_t)res[r]; nzl |= res[r] != 0; pred[r] += res[r]; }
    }
    cbf = __ballot(nzl) != 0;
  } else {
  // ---- forward rows, forward columns, quantiser; levels -> s.lev, dequantised coefficients stay in registers
  const XfLaneF16 &xl = s.xf[d.xf][lane];
  const kv_f16x4 ta = kv_h4(xl.ta), tb = kv_h4(xl.tb);
  int y[4], co[4], dq[4] = {0, 0, 0, 0};
  mfma16_data_a(res, ta, y);
#pragma unroll
  for (int r = 0; r < 4; r++) y[r] = (y[r] + (1 << (L2 - 2))) >> (L2 - 1);
  mfma16_data_b(ta, y, co);
  PROF(6);
  bool nz = false;
  if (ADJ) {
    // rdoq / signhide (bit 0 / bit 1): levels to s.lev, quantiser remainders to the wave's scratch, one lane per 4x4 coefficient group adjusts
    // the levels (hevc_core.h adjust_group), then every lane takes its levels back -- all inside the wave, no workgroup barrier
    if (active) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int cf = clip3(-32768, 32767, (co[r] + (1 << (L2 + 5))) >> (L2 + 6));
        const uint32_t a = (uint32_t)iabs(cf), prod = a * (uint32_t)(mtab ? (q.qscale << 4) / mtab[(4 * g + r) * N + c] : q.qscale);
        const int lvm = imin((int)((prod + (uint32_t)q.qoff) >> q.qshift), 32767);
        const int du = clip3(-256, 511, (int)(prod >> (q.qshift - 8)) - (lvm << 8));
        s.lev[(ry + 4 * g + r) * S + rx + c] = (int16_t)(cf < 0 ? -lvm : lvm);
        ws.tr[(4 * g + r) * N + c] = (int16_t)((du + 256) | (cf < 0 ? 0x8000 : 0));
      }
    }
    wave_sync();
    adjust_block_lds(&s.lev[ry * S + rx], ws.tr, N, S, intra_scan_idx(1, L2, cidx, d.mode), adj & 1, adj & 2, lane, 64);
    wave_sync();
    if (active) {
#pragma unroll
      for (int r = 0; r < 4; r++) { const int lv = s.lev[(ry + 4 * g + r) * S + rx + c]; nz |= lv != 0; dq[r] = mtab ? dequant_coef_qm(lv, q, mtab[(4 * g + r) * N + c]) : dequant_coef_q(lv, q); }
    }
    wave_sync();                                              // (ws.tr is free again for the inverse transform)
  } else if (active) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int cf = clip3(-32768, 32767, (co[r] + (1 << (L2 + 5))) >> (L2 + 6));
      const int lv = mtab ? quant_level_qm(cf, q, mtab[(4 * g + r) * N + c], nullptr) : quant_level_q(cf, q);
      nz |= lv != 0;
      dq[r] = mtab ? dequant_coef_qm(lv, q, mtab[(4 * g + r) * N + c]) : dequant_coef_q(lv, q);
      s.lev[(ry + 4 * g + r) * S + rx + c] = (int16_t)lv;
    }
  }
  cbf = __ballot(nz) != 0;
  PROF(7);
  if (cbf) {
    wave_inverse16(ws, tb, dq, g, c, res);
#pragma unroll
    for (int r = 0; r < 4; r++) pred[r] = clip8(pred[r] + res[r]);
  }
  }
  PROF(8);
  if (active) {
    const uint32_t o = (uint32_t)pred[0] | ((uint32_t)pred[1] << 8) | ((uint32_t)pred[2] << 16) | ((uint32_t)pred[3] << 24);
    *(uint32_t *)&s.pic[(ry + c + 1) * P + 16 + rx + 4 * g] = o;
    // what a neighbouring CTU's workgroup will read -- the CTU's last row (IB_EDGE) and last column (IB_EDGE_R) -- leaves at once, as self-validating
    // words nobody waits for (kernel_common.h IntraNeighbours); the CTU itself goes to the picture in full lines at the end
    if ((d.flags & IB_EDGE) && c == N - 1) st_wt_u64(erow + ((rx + 4 * g) >> 2), (unsigned long long)o | ((unsigned long long)gen << 32));      // the block's last row, four samples and the generation per word
    if ((d.flags & IB_EDGE_R) && g == (N >> 2) - 1) st_wt_u32(ecol + ry + c, (o >> 24) | (gen << 8));      // the block's last column, one sample and the generation per word
  }
  wave_sync();
  PROF(9);
  return cbf;
}

// One workgroup of KVZ_INTRA_WAVES waves per (CTU, colour plane).  The CTU's coding units form a list in z-order; a wave takes the
// next one, waits until the 8x8 units its reference samples lie in are final (kernel_common.h IntraChain: independent quadrants
// run side by side), reconstructs it and marks its units.  CTUs are coupled by the samples themselves: a CTU's right column and bottom
// row leave as tagged words (f.edge_col / f.edge_row, kernel_common.h IntraNeighbours) the moment the block that holds them is done, and a
// block of the neighbouring CTU polls exactly the words its MODE reads -- a CTU starts when the two or three blocks of its left and upper
// neighbours its first block reads are done, not when a counted prefix of them is.  (Rounds 2-3 published progress counters per CTU; the
// decoder's k_dec_intra still does, driven by the transform-block list.)
#ifndef KVZ_INTRA_WAVES
#define KVZ_INTRA_WAVES 8          // (measured at 1080p: 2 waves 1.58 ms, 4: 1.41, 8: 1.36 -- a wave that has just finished a block spends a microsecond on its bookkeeping before it can take the next)
#endif
// ADJ: rdoq / signhide -- a kernel of its own, so that the plain chain (every step of it is on the critical path) stays as it was.
// PP: the intra units of a P picture (intra-in-P), launched behind k_inter_recon: a CTU without intra units (nearly all) leaves at
// once; in the others the inter units count as finished from the start, the CTU picture in LDS starts as the inter
// reconstruction left it, and only the intra units' levels and cbf bits are written.
// SCAL: `scaling-list default` -- a form of its own for the same reason as ADJ (the per-position factors cost the plain chain 30 registers when they are a run-time branch)
// LL: `lossless` -- see intra_block_wave
template <bool ADJ, bool PP, bool SCAL = false, bool LL = false>
__global__ __launch_bounds__(64 * KVZ_INTRA_WAVES) void k_intra_recon(EncFrame f)
{
  constexpr int W = KVZ_INTRA_WAVES, T = 64 * W;
  __shared__ IntraCtuLds s;
  __shared__ IntraWaveScratch wss[W];
  __shared__ IntraChain ch;
  __shared__ IntraBlk blk[64];                              // the CTU's coding units in z-order
  __shared__ uint2 dep[64], cover[64];                      // per coding unit: units it waits for, units it finishes
  __shared__ uint32_t nblk_s, ticket_s;
  __shared__ uint8_t cu_cbf_s[64];
  // Workgroups are dispatched in blockIdx order and a picture has more of them than fit on the chip at once, so they are numbered
  // the way the wavefront advances (f.intra_order: by cx + 2 cy -- every CTU a block depends on comes earlier) instead of in raster
  // order, where the right ends of the upper rows would hold the slots the lower left needs.
  // ... and a workgroup does not belong to one (CTU, plane): the launch has only as many workgroups as the wavefront keeps busy (a few
  // anti-diagonals of CTUs), each taking the next (CTU, plane) in that order from a ticket counter when it is done with the last.
  // Whatever a workgroup waits for has a lower ticket, so it is held by a workgroup that runs or is finished.  The point is what the
  // OTHER kernels on the GPU get: a workgroup per (CTU, plane) parks 1500 waiting workgroups with 30 KB of LDS each on the chip for the
  // 1.6 ms the chain takes, and the decoder's (or, beside k_dec_intra, the encoder's) P pictures stand still until it is over.
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wc = f.cw >> 6;
  const uint32_t nticket = 3u * (uint32_t)wc * (uint32_t)band_rows(f);
  uint32_t *const ticket_ctr = f.sync + (size_t)3 * wc * (f.ch >> 6);
  if (PP && !ticket_ctr[1]) return;                         // no intra unit in this P picture (k_intra_analyse<true> says): nothing to do
  for (int i = tid; i < 4 * 64; i += T) ((uint4 *)s.xf)[i] = ((const uint4 *)g_xf16.t)[i];      // the transforms' matrix operands: once per workgroup, not per (CTU, plane)
  for (bool once = true;; once = false) {
  // (PP: a workgroup per (CTU, plane), in dispatch order -- nearly all of them find nothing to do, and a ticket would only add a round trip)
  if (PP) { if (!once) break; } else {
  __syncthreads();                                          // (everybody is done with the last (CTU, plane): LDS and the ticket word are free)
  if (tid == 0) ticket_s = atomicAdd(ticket_ctr, 1u);
  __syncthreads();
  }
  const uint32_t ticket = PP ? blockIdx.x : ticket_s;
  if (ticket >= nticket) break;
  const int c = (int)(ticket % 3u), ctu = (int)f.intra_order[ticket / 3u];
  const int row = ctu / wc, cx = ctu % wc;
#ifdef KVZ_PROF
  if (threadIdx.x == 0) { for (int k = 0; k < 15; k++) g_prof[k] = 0; g_prof[15] = clock64(); }
#endif
  const int adj = (f.rdoq ? 1 : 0) | (f.signhide ? 2 : 0);      // level adjustment behind the quantiser (hevc_core.h adjust_group)
  const int sh = c ? 1 : 0, S = 64 >> sh, pw = f.cw >> sh, P = 16 + 2 * S;
  uint64_t im = ~0ull;                                      // the CTU's 8x8 units (z-order) that belong to intra coding units
  if (PP) {
    int zx, zy; ctu_z_to_xy(lane, zx, zy);
    im = __ballot(f.cu_intra[b8idx(f, cx * 64 + zx * 8, row * 64 + zy * 8)] != 0);      // (every wave for itself: no barrier in front of the exit)
    if (!im) continue;                                      // (its samples are k_inter_recon's and final: the neighbours read them from the picture)
  }
  const int qpl = ctu_quant_qp(f, cx * 64, row * 64), qp = c ? kChromaQp[qpl] : qpl;
  const int hc = f.ch >> 6;
  IntraNeighbours nb;
  nb.nb_up = row > 0 && !tile_row_starts_at(hc, f.tile_rows, row); nb.nb_left = cx > 0 && !tile_col_starts_at(wc, f.tile_cols, cx);
  nb.nb_ur = nb.nb_up && cx + 1 < wc && !tile_col_starts_at(wc, f.tile_cols, cx + 1); nb.nb_ul = nb.nb_up && nb.nb_left;
  uint32_t *const ecol = f.edge_col[c] + (size_t)ctu * S;      // this CTU's right column for its right neighbour (IB_EDGE_R)
  nb.ecol_left = ecol - S; nb.gen = f.chain_gen;
  unsigned long long *const erow = f.edge_row[c] + (size_t)ctu * (S >> 2);     // this CTU's bottom row for the CTUs below (IB_EDGE)
  nb.erow_up = erow - (size_t)wc * (S >> 2); nb.erow_ur = nb.erow_up + (S >> 2); nb.erow_ul = nb.erow_up - (S >> 2);
  if (PP) {
    // which of the neighbours' edge units are intra units (kernel_common.h IntraBorders: the inter units around are final, nothing to wait for
    // there) -- lanes 0-7: the left CTU's right column, 8-15 / 16-23: the bottom rows of the upper / upper-right CTU, 24: the corner
    const int g = lane >> 3, u = lane & 7;
    int X = -1, Y = -1;
    if (g == 0 && nb.nb_left) { X = cx * 64 - 8; Y = row * 64 + u * 8; }
    else if (g == 1 && nb.nb_up) { X = cx * 64 + u * 8; Y = row * 64 - 8; }
    else if (g == 2 && nb.nb_ur) { X = (cx + 1) * 64 + u * 8; Y = row * 64 - 8; }
    else if (lane == 24 && nb.nb_ul) { X = cx * 64 - 8; Y = row * 64 - 8; }
    const uint64_t m = __ballot(X >= 0 && f.cu_intra[b8idx(f, X < 0 ? 0 : X, Y < 0 ? 0 : Y)] != 0);
    nb.il = (uint32_t)m & 0xffu; nb.iu = (uint32_t)(m >> 8) & 0xffu; nb.iur = (uint32_t)(m >> 16) & 0xffu; nb.iul = (uint32_t)(m >> 24) & 1u;
  }
  chain_init(ch, (uint32_t)~im, (uint32_t)(~im >> 32));
  // ---- everything the chain needs to know about the CTU's coding units, one lane per 8x8 unit (z-order), compacted into a list
  if (wave == 0) {
    int zx, zy; ctu_z_to_xy(lane, zx, zy);
    const int X = cx * 64 + zx * 8, Y = row * 64 + zy * 8, bi = b8idx(f, X, Y);
    const int l2 = f.cu_log2[bi], mode = f.cu_intra_mode[bi], n = 1 << (l2 - sh), nl = 1 << l2, su = nl >> 3;
    cu_cbf_s[lane] = 0;
    const bool start = (lane & (su * su - 1)) == 0 && ((im >> lane) & 1);
    const uint64_t starts = __ballot(start);
    const int k = __popcll(starts & ((1ull << lane) - 1ull));
    if (start) {
      const bool aL = avail64(f.cw, f.chp, X, Y, X - 1, Y), aT = avail64(f.cw, f.chp, X, Y, X, Y - 1);
      const bool aBL = aL && avail64(f.cw, f.chp, X, Y, X - 1, Y + nl), aTR = aT && avail64(f.cw, f.chp, X, Y, X + nl, Y - 1);
      IntraBlk d;
      d.rx = (uint8_t)((zx * 8) >> sh); d.ry = (uint8_t)((zy * 8) >> sh);
      // availability is decided per group of n samples (below-left, left, corner, above, above-right): each group lies in one block
      // of this block's size, which either precedes this block in z-order or does not; the available groups are contiguous
      d.lo = (uint8_t)(aBL ? 0 : (aL ? n : 2 * n + 1)); d.hi = (uint8_t)(aTR ? 4 * n : (aT ? 3 * n : (aL ? 2 * n - 1 : 0)));      // (nothing available: lo = 2n + 1 > hi = 0)
      d.mode = (uint8_t)mode; d.l2 = (uint8_t)(l2 - sh);
      d.flags = (uint8_t)((intra_filter_needed(n, c ? 1 : 0, mode) ? IB_FILT : 0) | ((zx == 0 || zy == 0) ? IB_BORDER : 0) | ((zy + su == 8) ? IB_EDGE : 0) | ((zx + su == 8) ? IB_EDGE_R : 0));
      d.xf = (uint8_t)((l2 - sh == 2 && c == 0) ? XF16_DST4 : l2 - sh - 1);
      d.angle = (int16_t)kIntraAngle[mode]; d.inv = (int16_t)kInvAngle[mode];
      d.zu = (uint16_t)lane; d.next = (uint16_t)(lane + su * su);
      blk[k] = d;
      dep[k] = chain_dependencies(zx, zy, su, ((intra_uses_below_left(l2 - sh, c ? 1 : 0) >> mode) & 1) != 0, ((intra_uses_above_right(l2 - sh, c ? 1 : 0) >> mode) & 1) != 0);
      cover[k] = chain_cover(lane, su);
    }
    if (lane == 0) nblk_s = (uint32_t)__popcll(starts);
  }
  const uint8_t *gsrc = f.src[c] + (size_t)(row * S) * pw + cx * S;
  uint8_t *plane = f.rec[c];
  uint8_t *grec = plane + (size_t)(row * S) * pw + cx * S;
  int16_t *gcoef = f.coef[c] + (size_t)(row * S) * pw + cx * S;
  for (int k = tid; k < S * S / 16; k += T) {
    int y = k / (S / 16), xq = k % (S / 16);
    *(uint4 *)&s.src[y * S + xq * 16] = *(const uint4 *)&gsrc[(size_t)y * pw + xq * 16];
    if (PP) *(uint4 *)&s.pic[(y + 1) * P + 16 + xq * 16] = *(const uint4 *)&grec[(size_t)y * pw + xq * 16];      // the CTU as k_inter_recon left it
  }
  if (f.trace && tid == 0) { unsigned long long *t = f.trace + ((size_t)ctu * 3 + c) * 8; t[0] = wall_clock64(); t[3] = 0; t[4] = 0; }
  __syncthreads();
  const int nblk = wave_uniform_int((int)nblk_s);         // (bounds the claim loop: uniform by construction, kernel_common.h chain_claim)
  const QuantConst q8 = quant_const(qp, 3 - sh, 1), q16 = quant_const(qp, 4 - sh, 1);      // (coding units are 8x8 or 16x16)
  IntraWaveScratch &ws = wss[wave];
  bool first = true;
  for (;;) {
    const int k = chain_claim(ch, lane);
    if (k >= nblk) break;
    PROF(1);                                                // claim
    const IntraBlk d = wave_uniform(&blk[k]);              // (wave-uniform: what is derived from it runs on the scalar unit)
    const uint2 dp = dep[k], cv = cover[k];
    // The neighbouring CTUs' samples this block reads come FIRST: they do not depend on this CTU's own blocks, so the memory round trip that fetches them
    // (and the poll, when the neighbour is not there yet) runs while the blocks in front of this one are still being coded, instead of behind them on the
    // chain's critical path -- three of the four blocks of a CTU's top row paid it there.  (A form that looks once and polls only when the block's turn has
    // come -- tried because a two-process run beside the test suite crawled, which turned out to have another cause -- is 6 % slower: 0.71 against 0.67 ms.)
    if (d.flags & IB_BORDER) {
      // the neighbouring CTUs are waited for only as far as the block's MODE reads them (hevc_core.h intra_uses_*): with "intra-chain" the left-edge blocks never
      // read the left CTU's below-left samples and the above-right CTU is not read at all
      const int n = 1 << d.l2;
      const int nl2 = ((intra_uses_below_left(d.l2, c) >> d.mode) & 1) ? 2 * n : n, nt2 = ((intra_uses_above_right(d.l2, c) >> d.mode) & 1) ? 2 * n : n;
      borders_need_wave(ch, nb, s.pic, P, plane, pw, cx, row, S, sh, 2 * S, d.rx, d.ry, n, f.err, lane, nl2, nt2);
    }
    PROF(2);                                                // neighbouring CTUs: waits and copies
    chain_wait_done(ch, make_uint2((uint32_t)__builtin_amdgcn_readfirstlane((int)dp.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)dp.y)), f.err, lane);
    PROF(3);                                                // waiting for the units of this CTU the block reads
    if (f.trace && first && k == 0 && lane == 0) f.trace[((size_t)ctu * 3 + c) * 8 + 1] = wall_clock64();
    first = false;
    bool cbf;
    switch (d.l2) {
      case 2: cbf = intra_block_wave<2, ADJ, LL>(s, ws, d, c, S, q8, lane, adj, ecol, erow, f.chain_gen, SCAL ? f.scaling + scaling_offset(2, c, 0) : nullptr); break;
      case 3: cbf = intra_block_wave<3, ADJ, LL>(s, ws, d, c, S, c ? q16 : q8, lane, adj, ecol, erow, f.chain_gen, SCAL ? f.scaling + scaling_offset(3, c, 0) : nullptr); break;
      default: cbf = intra_block_wave<4, ADJ, LL>(s, ws, d, c, S, q16, lane, adj, ecol, erow, f.chain_gen, SCAL ? f.scaling + scaling_offset(4, c, 0) : nullptr); break;
    }
    const uint2 cvu = make_uint2((uint32_t)__builtin_amdgcn_readfirstlane((int)cv.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)cv.y));
    chain_mark_done(ch, cvu, lane);
#ifndef KVZ_PROF
    if (f.trace && c == 0 && lane == 0 && k < 16) f.trace[(size_t)wc * (f.ch >> 6) * 56 + (size_t)ctu * 16 + k] = wall_clock64() | ((unsigned long long)d.l2 << 60);      // (tools/intra_timeline.py: when the luma blocks of the CTU were done)
#endif
    PROF(10);                                               // mark
#ifdef KVZ_PROF
    if (threadIdx.x == 0) g_prof[14] += 1;                   // blocks wave 0 did
#endif
    if (cbf && (int)d.zu + lane < (int)d.next) cu_cbf_s[d.zu + lane] = 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // the CTU's samples -> the picture, in whole lines (the chain itself stored only what neighbouring workgroups read; PP: the inter units' samples are what they were)
  for (int k = tid; k < S * S / 16; k += T) { const int y = k / (S / 16), xq = k % (S / 16); *(uint4 *)&grec[(size_t)y * pw + xq * 16] = *(const uint4 *)&s.pic[(y + 1) * P + 16 + xq * 16]; }
  for (int k = tid; k < S * S / 8; k += T) {
    int y = k / (S / 8), xq = k % (S / 8);
    if (PP && !((im >> kv_zunit8(((xq * 8) << sh) >> 3, (y << sh) >> 3)) & 1)) continue;       // (an inter unit's levels are k_inter_recon's)
    *(uint4 *)&gcoef[(size_t)y * pw + xq * 8] = *(const uint4 *)&s.lev[y * S + xq * 8];
  }
  if (tid < 64 && cu_cbf_s[tid]) {
    int zx, zy; ctu_z_to_xy(tid, zx, zy);
    const int bi = b8idx(f, cx * 64 + zx * 8, row * 64 + zy * 8);
    atomicOr((uint32_t *)(f.cu_cbf + (bi & ~3)), (1u << c) << (8 * (bi & 3)));   // the three planes own one bit each of the byte
  }
  if (f.trace && tid == 0) { unsigned long long *t = f.trace + ((size_t)ctu * 3 + c) * 8; t[2] = wall_clock64(); t[7] = (unsigned long long)nblk; }
#ifdef KVZ_PROF
  if (f.trace && tid == 0 && c == 0) for (int k = 0; k < 16; k++) f.trace[(size_t)wc * (f.ch >> 6) * 24 + (size_t)ctu * 16 + k] = (unsigned long long)g_prof[k];
#endif
  }
}

// =============================================================================================
// launch wrappers
// =============================================================================================
void launch_inter_recon(const EncFrame &f, hipStream_t st)
{
  const dim3 grid(f.cw / 32, band_rows(f) * 2);
  if (f.wp) {                                  // weightp: the weighted forms (never with lossless: the encoder refuses the pair)
    const int k = (f.rc ? 4 : 0) | ((f.rdoq || f.signhide) ? 2 : 0) | (f.subme > 0 ? 1 : 0);
    switch (k) {
      case 7: hipLaunchKernelGGL((k_inter_recon<true, true, true, false, true>), grid, dim3(256), 0, st, f); break;
      case 6: hipLaunchKernelGGL((k_inter_recon<false, true, true, false, true>), grid, dim3(256), 0, st, f); break;
      case 5: hipLaunchKernelGGL((k_inter_recon<true, false, true, false, true>), grid, dim3(256), 0, st, f); break;
      case 4: hipLaunchKernelGGL((k_inter_recon<false, false, true, false, true>), grid, dim3(256), 0, st, f); break;
      case 3: hipLaunchKernelGGL((k_inter_recon<true, true, false, false, true>), grid, dim3(256), 0, st, f); break;
      case 2: hipLaunchKernelGGL((k_inter_recon<false, true, false, false, true>), grid, dim3(256), 0, st, f); break;
      case 1: hipLaunchKernelGGL((k_inter_recon<true, false, false, false, true>), grid, dim3(256), 0, st, f); break;
      default: hipLaunchKernelGGL((k_inter_recon<false, false, false, false, true>), grid, dim3(256), 0, st, f); break;
    }
  } else if (f.rc) {                                  // rate control v2: the groups of CTU rows inside the one launch
    const int k = ((f.rdoq || f.signhide) ? 2 : 0) | (f.subme > 0 ? 1 : 0);
    if (k == 3) hipLaunchKernelGGL((k_inter_recon<true, true, true>), grid, dim3(256), 0, st, f);
    else if (k == 2) hipLaunchKernelGGL((k_inter_recon<false, true, true>), grid, dim3(256), 0, st, f);
    else if (k == 1) hipLaunchKernelGGL((k_inter_recon<true, false, true>), grid, dim3(256), 0, st, f);
    else hipLaunchKernelGGL((k_inter_recon<false, false, true>), grid, dim3(256), 0, st, f);
  } else if (f.rdoq || f.signhide) {
    if (f.subme > 0) hipLaunchKernelGGL((k_inter_recon<true, true>), grid, dim3(256), 0, st, f);
    else hipLaunchKernelGGL((k_inter_recon<false, true>), grid, dim3(256), 0, st, f);
  } else if (f.lossless) {
    if (f.subme > 0) hipLaunchKernelGGL((k_inter_recon<true, false, false, true>), grid, dim3(256), 0, st, f);
    else hipLaunchKernelGGL((k_inter_recon<false, false, false, true>), grid, dim3(256), 0, st, f);
  } else if (f.subme > 0) hipLaunchKernelGGL((k_inter_recon<true>), grid, dim3(256), 0, st, f);
  else hipLaunchKernelGGL((k_inter_recon<false>), grid, dim3(256), 0, st, f);     // integer vectors only
}
void launch_inter_signal(const EncFrame &f, hipStream_t st)
{
  const int n = (f.cw / 8) * (band_rows(f) * 8);
  if (f.ref_dist && f.col_out) hipLaunchKernelGGL((k_inter_signal<true, true>), dim3((n + 1023) / 1024), dim3(1024), 0, st, f);
  else if (f.ref_dist) hipLaunchKernelGGL((k_inter_signal<false, true>), dim3((n + 1023) / 1024), dim3(1024), 0, st, f);
  else if (f.col_out) hipLaunchKernelGGL(k_inter_signal<true>, dim3((n + 1023) / 1024), dim3(1024), 0, st, f);
  else hipLaunchKernelGGL(k_inter_signal<false>, dim3((n + 1023) / 1024), dim3(1024), 0, st, f);
}
void launch_intra_analyse(const EncFrame &f, hipStream_t st)
{
  // An intra picture's mode search is the one throughput-bound kernel of the pipeline: 2 040 independent workgroups at 1080p, all of them resident at once if
  // nothing stops them -- eight waves on every SIMD of the chip, i.e. EVERY wave slot, for the length of the launch, and whatever else is queued beside it
  // (the P pictures in front of an IDR, the other pictures' chains of an all-intra stream) cannot start a workgroup until one of the search's retires.  Dynamic
  // LDS it does not use caps it at kAnalysePerCu workgroups per compute unit (160 KB of LDS each), which leaves the other slots to everybody else.
  // Measured (profiles/r05_analyse_cap.txt; 4K, pipelined, worst launch of 504): k_me 948 -> 135 us, k_tok_compact 881 -> 59, k_inter_signal 540 -> 280 with a cap of 4;
  // the search itself 156 -> 173 us at 1080p (197 at 3); the encoder alone on an all-intra stream 2 450 -> 2 750 frames/s.  KVAZZUP_AMD_ANALYSE_PER_CU=0: no cap.
  static const int per_cu = getenv("KVAZZUP_AMD_ANALYSE_PER_CU") ? atoi(getenv("KVAZZUP_AMD_ANALYSE_PER_CU")) : 4;
  const size_t pad = per_cu > 1 && per_cu < 8 && !f.analyse_alone ? (size_t)(160 * 1024 / (per_cu + 1) + 1024 - 9264) & ~(size_t)255 : 0;
  if (f.is_intra) hipLaunchKernelGGL(k_intra_analyse<false>, dim3(f.cw / 32, band_rows(f) * 2), dim3(256), pad, st, f);
  else if (f.ir_e) hipLaunchKernelGGL((k_intra_analyse<true, true>), dim3(512), dim3(1024), 0, st, f);      // intra-refresh: the band's quarters are on the list whatever they cost
  else hipLaunchKernelGGL(k_intra_analyse<true>, dim3(512), dim3(1024), 0, st, f);       // intra-in-P, behind k_me: 512 workgroups (two per compute unit) share the candidate list, a quarter of a listed block at a time
}
void launch_intra_recon(const EncFrame &f, hipStream_t st)
{
  // as many workgroups as three anti-diagonals of the CTU wavefront hold, in three planes (k_intra_recon: tickets)
  static const int diags_env = getenv("KVAZZUP_AMD_INTRA_DIAGS") ? atoi(getenv("KVAZZUP_AMD_INTRA_DIAGS")) : -1;      // (measurement aid; 0: a workgroup per (CTU, plane))
  const int diags = diags_env >= 0 ? diags_env : (f.chain_diags ? f.chain_diags : 3);
  const int wc = f.cw / 64, nr = band_rows(f), diag = nr < (wc + 1) / 2 ? nr : (wc + 1) / 2, want = diags > 0 ? 3 * diags * diag + 32 : 3 * wc * nr;
  const dim3 grid(want < 3 * wc * nr ? want : 3 * wc * nr), block(64 * KVZ_INTRA_WAVES);
  const bool adj = f.rdoq || f.signhide;
  if (!f.is_intra) {                                                                                            // intra-in-P, behind k_inter_recon
    // (a workgroup per (CTU, plane) here: nearly all of them find no intra unit, and a workgroup that checks nine tickets in turn pays nine memory round trips)
    const dim3 all(3 * wc * nr);
    if (f.lossless) { hipLaunchKernelGGL((k_intra_recon<false, true, false, true>), all, block, 0, st, f); return; }
    if (f.scaling) { if (adj) hipLaunchKernelGGL((k_intra_recon<true, true, true>), all, block, 0, st, f); else hipLaunchKernelGGL((k_intra_recon<false, true, true>), all, block, 0, st, f); }
    else if (adj) hipLaunchKernelGGL((k_intra_recon<true, true>), all, block, 0, st, f); else hipLaunchKernelGGL((k_intra_recon<false, true>), all, block, 0, st, f);
    return;
  }
  if (f.lossless) hipLaunchKernelGGL((k_intra_recon<false, false, false, true>), grid, block, 0, st, f);
  else if (f.scaling) { if (adj) hipLaunchKernelGGL((k_intra_recon<true, false, true>), grid, block, 0, st, f); else hipLaunchKernelGGL((k_intra_recon<false, false, true>), grid, block, 0, st, f); }
  else if (adj) hipLaunchKernelGGL((k_intra_recon<true, false>), grid, block, 0, st, f);
  else hipLaunchKernelGGL((k_intra_recon<false, false>), grid, block, 0, st, f);
}

}  // namespace kvzx
