// kvazzup_amd/csrc/enc_kernels.hip -- CDNA4 (gfx950) kernels of the HEVC encoder hot path: motion search, tokenizer, input staging, VAQ.
//
// What the encoder's kernels replace: the work Kvazaar does inside kvz_api->encoder_encode
// (uvgComm's src/media/processing/kvazaarfilter.cpp:435-438): motion search, prediction,
// transform/quantisation, reconstruction, deblocking and CABAC.  The arithmetic is checked
// against oracle/ (tests/); the decisions follow "uvgx encoder algorithm v1" (oracle/hevc_enc.h).
// They are in three files, each with the launch wrappers (enc_kernels.h) of its kernels: this one, recon_kernels.hip (inter and intra reconstruction, signalling,
// intra analysis) and loop_kernels.hip (QP bookkeeping, deblocking, SAO).
//
// THE SEARCH AND THE TOKENIZER STAY IN ONE FILE.  The machine code hipcc makes of k_tokenize depends on k_me, k_luma_quarter and k_me_coarse being in its
// translation unit (without them: eight more basic blocks, a compare narrowed to 16 bits); likewise k_intra_recon<ADJ = true, ..> and k_inter_recon in
// recon_kernels.hip.  Seen by compiling, not measured on a GPU: parting either pair is a performance change and wants a measurement.
// tools/kernel_resources.py prints a digest of every kernel's instruction text; a move that changes none has changed no kernel.
//
// Launch geometry (coded size is a multiple of 64; DESIGN.md section 5 has the table with timings):
//   k_pad_input     packed I420 -> padded planes, sixteen samples per thread
//   k_vaq_stats/apply  per-CTU luma variance -> delta QP (vaq only)
//   k_me            one workgroup per 32x32 luma block (XCD-aware order): early termination on the co-located block, else the
//                   search window staged in LDS, v_qsad_pk_u16_u8 on quads x pairs of candidates, wave min of (cost << 13 | index)
//   k_tokenize      one wave per 16x16 unit (and colour component): binarisation + context selection -> bins as 16-bit tokens;
//   k_tok_compact   restores coding order per CTU, dense copy to host-mapped memory for the host arithmetic coder
// (the decoder's kernels live in dec_kernels.hip, the fractional-sample search in subpel_kernels.hip, rate control in rc_kernels.hip)
#include <hip/hip_runtime.h>
#include <type_traits>
#include "hevc_core.h"
#include "enc_kernels.h"
#include "kernel_common.h"

namespace kvzx {

// =============================================================================================
// Motion estimation
// =============================================================================================
#define ME_MAXR 32
#define ME_WPITCH 100      // bytes per window row in LDS: 32 + 2*32 = 96, + 4 so the 9th dword read stays inside

// Full search over (2R+1)^2 integer displacements for one 32x32 block, with the four 16x16 quarters
// kept apart.  The search window sits in LDS.  A work item is a QUAD of horizontally adjacent
// candidates times a PAIR of vertically adjacent ones: v_qsad_pk_u16_u8 produces the four SADs of a
// quad against four current samples in one instruction (16-bit accumulators: a 16x16 quarter sums
// to at most 65280), and each window row read from LDS serves both candidates of the pair.
// (Measured on MI355X: v_qsad_pk_u16_u8 issues at ~24 cycles per wave, v_sad_u8 at ~4.7; the quad form
// still wins because it needs no v_alignbyte to line the window up with the candidate.)
// MR (lp-refs, f.nref references): the window of every reference in turn, and the minimum over (reference, candidate) pairs of the 64-bit key
// cost << 16 | ref << 13 | candidate -- ties to the lower reference, then the lower candidate; cost includes ref_bins(ref).
// One reference: the 32-bit key cost << 13 | candidate (the same order).
// CO (me-coarse): per reference the zero window and, where k_me_coarse's centre lies outside it (me_second_window), a second window
// around that centre through the same LDS buffer; vectors are centre + displacement, rate and admissibility those of the whole vector; the 64-bit key
// me_fine_key(): cost << 17 | ref << 14 | window << 13 | candidate.
// IR (intra-refresh; one reference, no coarse stage: the encoder refuses the others): a block all of whose quarters lie in the picture's
// band is not searched -- its quarters go to k_intra_analyse<true, true> with the cost 0xffffffff, which passes the gate and beats every intra price; the block
// whose left quarters alone are forced is searched as ever (never left early) and joins the list as well; a clean block (left of the band, position >= 1)
// drops the candidates beyond ir_mvx_max.  A form of its own: the launches without the option run the code of before.
// FB (loss-feedback; one reference, no coarse stage): a heal picture's block reads its record (f.fb_blk, fb_block_record) where the IR form
// computes the band -- the forced quarters take the IR form's path, and every candidate beyond the record's reach in x or y is dropped (the zero vector never is).
// A form of its own as well.
// MR and FB together (fb-anchor, "uvgx loss feedback v2"; two references, 0 = the previous picture, 1 = the anchor): a v2 heal picture.  A
// quarter whose bit of the record's nibble is set is searched in reference 1 alone, over the whole window; a free quarter in reference 0 alone, within the
// record's reach.  The 32x32 key is admissible in reference 0 where the nibble is 0 and in reference 1 where it is 15; a mixed block is coded as its four
// quarters.  Early termination: nibble 0 as the FB form, nibble 15 against the anchor's co-located block (reference 1, zero vector), mixed none.  No quarter is
// sent to the intra path: the ordinary gate prices what the search found.  A form of its own as well.
template <bool MR, bool CO = false, bool IR = false, bool FB = false>
__global__ __launch_bounds__(256) void k_me(EncFrame f)
{
  constexpr bool FA = MR && FB;                                        // a v2 heal picture: forced quarters go to the anchor
  constexpr bool FQ = IR || (FB && !FA);                               // the block may have quarters forced intra
  using Key = typename std::conditional<MR || CO, unsigned long long, uint32_t>::type;
  constexpr int KS = CO ? 17 : (MR ? 16 : 13);                         // cost field's shift
  constexpr Key KMAX = ~(Key)0;
  __shared__ __attribute__((aligned(16))) uint8_t wbuf[(32 + 2 * ME_MAXR + 1) * ME_WPITCH + 16];
  __shared__ __attribute__((aligned(16))) uint32_t cur[32 * 8];
  __shared__ Key red[5];
  const int tid = threadIdx.x, nthreads = blockDim.x;
  int bx_, by_; xcd_block_2d(bx_, by_);
  const int x0 = bx_ * 32, y0 = by_ * 32 + f.row0 * 64;
  const int R = f.range, W = 2 * R + 1, WW = 32 + 2 * R;
  const uint8_t *ref = f.me_ref, *src = f.src[0];
  const uint32_t lam = (uint32_t)f.lambda_q4;
  if (f.pb_on && blockIdx.x == 0 && blockIdx.y == 0) picture_begin_body(f.pb_rc, f.pb_bits3, f.pb_slot3, f.pb_have3, f.pb_qt, f.pb_roi, f.pb_nctu, f.qp, 0, tid, nthreads);      // (nothing in this launch reads what it writes: k_inter_recon is the first)
  // the block itself, and (me-early-termination) its SAD against the co-located block of the reference: a block that differs
  // from it by no more than quantisation noise is coded unsplit with the zero vector, without a search
  if (tid == 0) red[0] = 0;
  int ir_forced = 0, ir_dx = 0x7fffffff;                               // IR: the block's forced quarters; a clean block's largest horizontal displacement in full samples
  if constexpr (IR) {
    ir_forced = ir_forced_quarters(x0, f.ir_s, f.ir_e);
    if (ir_clean_block(x0, f.ir_s, f.ir_j)) ir_dx = ir_mvx_max(x0, f.ir_s) >> 2;
  }
  int fb_r = 0;                                                        // FB: the block's reach in full samples
  if constexpr (FB) {
    const uint8_t *r = f.fb_blk + 2 * ((size_t)(y0 >> 5) * (f.cw >> 5) + (x0 >> 5));
    ir_forced = r[0]; fb_r = fb_reach(r[1]);
    if constexpr (FA) { if (ir_forced == 15) ref = f.me_refs[1]; }     // (early termination looks at the anchor's co-located block)
  }
  const int it0 = FA && ir_forced == 15 ? 1 : 0, it1 = FA && ir_forced == 0 ? 1 : 2;      // FA: the references the block's quarters are searched in
  if constexpr (FQ) {
    if (ir_forced == 15) {                                             // (the same for every thread, in front of the first barrier)
      if (tid < 16) {
        const int i = b8idx(f, x0 + (tid & 3) * 8, y0 + (tid >> 2) * 8);
        f.cu_log2[i] = 5; f.cu_intra[i] = 0; f.cu_mv[i * 2] = 0; f.cu_mv[i * 2 + 1] = 0;
        f.cu_mvp_idx[i] = 0;                             // mark for k_subpel: not searched
      }
      if (tid < 4) f.me_cost16[((y0 >> 4) + (tid >> 1)) * (f.cw >> 4) + (x0 >> 4) + (tid & 1)] = 0xffffffffu;
      if (tid == 0) f.me_cand[1 + atomicAdd(&f.me_cand[0], 1u)] = (uint32_t)((y0 >> 5) * (f.cw >> 5) + (x0 >> 5));
      return;
    }
  }
  __syncthreads();
  {
    uint32_t s0 = 0;
    for (int i = tid; i < 256; i += nthreads) {
      const size_t g = (size_t)(y0 + (i >> 3)) * f.cw + x0 + (i & 7) * 4;
      const uint32_t c = *reinterpret_cast<const uint32_t *>(src + g);
      cur[i] = c;
      if (f.me_early) s0 = __builtin_amdgcn_sad_u8(c, *reinterpret_cast<const uint32_t *>(ref + g), s0);
    }
    if (f.me_early) { s0 = wave_sum_u32(s0); if ((tid & 63) == 0) atomicAdd(&red[0], (Key)s0); }
  }
  __syncthreads();
  if (f.me_early && !(FQ && ir_forced) && !(FA && ir_forced != 0 && ir_forced != 15) && red[0] <= 64u * lam) {
    if (tid < 16) {
      const int i = b8idx(f, x0 + (tid & 3) * 8, y0 + (tid >> 2) * 8);
      f.cu_log2[i] = 5; f.cu_intra[i] = 0; f.cu_mv[i * 2] = 0; f.cu_mv[i * 2 + 1] = 0;
      f.cu_mvp_idx[i] = 0;                               // mark for k_subpel: not searched (k_inter_signal writes the real value later)
      if (MR) f.cu_ref[i] = FA && ir_forced == 15 ? 1 : 0;      // (the co-located block of reference 0; FA, every quarter forced: of the anchor)
    }
    if (f.intra_p && tid < 4) f.me_cost16[((y0 >> 4) + (tid >> 1)) * (f.cw >> 4) + (x0 >> 4) + (tid & 1)] = 0;      // never an intra candidate
    return;
  }
  Key best[5] = {KMAX, KMAX, KMAX, KMAX, KMAX};
  const int nr = MR ? f.nref : 1;
#pragma unroll 1
  for (int it = FA ? it0 : 0; it < (FA ? it1 : (CO ? 2 * nr : nr)); it++) {                    // (MR: one reference after the other through the same LDS window; CO: each reference's two windows)
  const int rf = CO ? it >> 1 : it, win = CO ? it & 1 : 0;
  int ox = 0, oy = 0;                                                  // the window's centre (CO, second window: k_me_coarse's)
  if constexpr (CO) {
    if (win) {
      const int16_t *c = f.mc_centres + 2 * ((size_t)rf * (f.cw >> 5) * (f.ch >> 5) + (size_t)(y0 >> 5) * (f.cw >> 5) + (x0 >> 5));
      ox = c[0]; oy = c[1];
      if (!me_second_window(ox, oy, R)) continue;                      // (the same for every thread of the workgroup)
    }
  }
  const uint8_t *refp = MR ? f.me_refs[rf] : ref;
  __syncthreads();                                                     // (red[] is about to be re-initialised; MR: the previous reference's window is done with)
  for (int i = tid; i < (WW + 1) * (ME_WPITCH / 4); i += nthreads) {   // four window samples per thread; columns >= WW and row WW are padding
    const int wy = i / (ME_WPITCH / 4), wx = (i - wy * (ME_WPITCH / 4)) * 4;
    const int gy = clip3(0, f.ch - 1, y0 + oy - R + wy), gx = x0 + ox - R + wx;
    const uint8_t *row = refp + (size_t)gy * f.cw;
    uint32_t v;
    if (gx >= 0 && gx + 7 < f.cw) {
      const uint32_t *q = (const uint32_t *)(row + (gx & ~3));
      v = __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(gx & 3));
    } else {
      v = 0;
      for (int k = 0; k < 4; k++) v |= (uint32_t)row[clip3(0, f.cw - 1, gx + k)] << (8 * k);
    }
    *(uint32_t *)&wbuf[wy * ME_WPITCH + wx] = v;
  }
  if (it == (FA ? it0 : 0) && tid < 5) red[tid] = KMAX;
  __syncthreads();
  const uint32_t rbins = MR ? (uint32_t)ref_bins(rf, nr) : 0u;
  // tile constraint (statement: me_block32() in oracle/hevc_enc.c): the displaced 32x32 block, plus 4 rows each side for
  // the chroma half-sample taps when the displacement is odd, stays inside its tile -- except across the picture's own edges
  int ty0 = 0, ty1 = f.ch, tx0 = 0, tx1 = f.cw;
  if (f.tile_rows > 1) {
    const int hc = f.ch >> 6, tr = tile_row_of(hc, f.tile_rows, y0 >> 6);
    ty0 = tile_row_first(hc, f.tile_rows, tr) * 64; ty1 = tile_row_first(hc, f.tile_rows, tr + 1) * 64;
  }
  if (f.tile_cols > 1) {                                       // ... and in x with tile columns
    const int wc = f.cw >> 6, tc = tile_col_of(wc, f.tile_cols, x0 >> 6);
    tx0 = tile_col_first(wc, f.tile_cols, tc) * 64; tx1 = tile_col_first(wc, f.tile_cols, tc + 1) * 64;
  }
  const int NQ = (W + 3) >> 2, NG = (W + 1) >> 1;
  for (int item = tid; item < NQ * NG; item += nthreads) {
    const int g = item / NQ, q = item - g * NQ, dy0 = 2 * g;
    uint64_t acc[2][4];                                          // [candidate of the pair][quarter]: four u16 sums, one per candidate of the quad
    const uint8_t *wbase = wbuf + dy0 * ME_WPITCH + 4 * q;
#pragma unroll
    for (int half = 0; half < 2; half++) {
      uint64_t al = 0, ar = 0, bl = 0, br = 0;                   // left / right quarter of this half, candidates A and B
#pragma unroll 1
      for (int rr = 0; rr < 17; rr++) {
        // window row dy0 + wr is row wr of candidate A (dy0) and row wr - 1 of candidate B (dy0 + 1); each half covers
        // the rows of both candidates that fall into its quarters: rows half*16 .. +15
        const int wr = half * 16 + rr;
        const uint32_t *wp = (const uint32_t *)(wbase + wr * ME_WPITCH);
        uint32_t d[9];
#pragma unroll
        for (int j = 0; j < 9; j++) d[j] = wp[j];
        uint64_t p[8];
#pragma unroll
        for (int j = 0; j < 8; j++) p[j] = ((uint64_t)d[j + 1] << 32) | d[j];
        if (rr < 16) {
          const uint32_t *c = &cur[wr * 8];
#pragma unroll
          for (int j = 0; j < 4; j++) { al = __builtin_amdgcn_qsad_pk_u16_u8(p[j], c[j], al); ar = __builtin_amdgcn_qsad_pk_u16_u8(p[j + 4], c[j + 4], ar); }
        }
        if (rr > 0) {
          const uint32_t *c = &cur[(wr - 1) * 8];
#pragma unroll
          for (int j = 0; j < 4; j++) { bl = __builtin_amdgcn_qsad_pk_u16_u8(p[j], c[j], bl); br = __builtin_amdgcn_qsad_pk_u16_u8(p[j + 4], c[j + 4], br); }
        }
      }
      acc[0][half * 2] = al; acc[0][half * 2 + 1] = ar; acc[1][half * 2] = bl; acc[1][half * 2 + 1] = br;
    }
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int dyi = dy0 + e;
      if (dyi >= W) continue;
      { const int dy = oy + dyi - R, m = (dy & 1) ? 4 : 0; if ((ty0 > 0 && y0 + dy - m < ty0) || (ty1 < f.ch && y0 + dy + 32 + m > ty1)) continue; }
      if (f.mv_frame) { const int dy = oy + dyi - R, my = (f.mv_frame == 2 && (dy & 1)) ? 4 : 0; if (y0 + dy - my < 0 || y0 + dy + 32 + my > f.ch) continue; }
      if constexpr (FB) { const int dy = oy + dyi - R; if ((!FA || rf == 0) && (dy > fb_r || dy < -fb_r)) continue; }      // within the record's reach (FA: reference 0)
      const int ry = mvd_bits((oy + dyi - R) * 4);
#pragma unroll
      for (int k4 = 0; k4 < 4; k4++) {
        const int dxi = 4 * q + k4;
        if (dxi >= W) continue;
        { const int dx = ox + dxi - R, m = (dx & 1) ? 4 : 0; if ((tx0 > 0 && x0 + dx - m < tx0) || (tx1 < f.cw && x0 + dx + 32 + m > tx1)) continue; }
        if (f.mv_frame) { const int dx = ox + dxi - R, mx = (f.mv_frame == 2 && (dx & 1)) ? 4 : 0; if (x0 + dx - mx < 0 || x0 + dx + 32 + mx > f.cw) continue; }
        if constexpr (IR) { if (ox + dxi - R > ir_dx) continue; }     // a clean block stays out of what the reference has not cleaned
        if constexpr (FB) { const int dx = ox + dxi - R; if ((!FA || rf == 0) && (dx > fb_r || dx < -fb_r)) continue; }
        const Key cand = CO ? (Key)me_fine_key(0u, rf, win, dyi * W + dxi) : ((Key)(dyi * W + dxi) | ((Key)rf << 13));
        const uint32_t rate = (lam * (uint32_t)(mvd_bits((ox + dxi - R) * 4) + ry + rbins)) >> 4;
        uint32_t sq[4];
#pragma unroll
        for (int k = 0; k < 4; k++) sq[k] = (uint32_t)(acc[e][k] >> (16 * k4)) & 0xffffu;
#pragma unroll
        for (int k = 0; k < 4; k++) { if (FA && ((ir_forced >> k) & 1) != rf) continue; best[k] = min(best[k], ((Key)(sq[k] + rate) << KS) | cand); }      // (FA: a quarter has one reference)
        best[4] = min(best[4], ((Key)(sq[0] + sq[1] + sq[2] + sq[3] + rate) << KS) | cand);      // (FA: one reference is searched where the nibble is 0 or 15; a mixed block never reads it)
      }
    }
  }
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
    Key v = best[k];
    if constexpr (MR || CO) { for (int o = 32; o > 0; o >>= 1) v = min(v, (Key)__shfl_xor((unsigned long long)v, o)); }
    else { for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o)); }
    if ((tid & 63) == 0) atomicMin(&red[k], v);
  }
  __syncthreads();
  if (tid < 16) {
    uint32_t pen = (lam * SPLIT_BITS) >> 4;
    uint32_t csplit = pen + (uint32_t)(red[0] >> KS) + (uint32_t)(red[1] >> KS) + (uint32_t)(red[2] >> KS) + (uint32_t)(red[3] >> KS);
    bool split = csplit < (uint32_t)(red[4] >> KS);
    if constexpr (FA) split = split || (ir_forced != 0 && ir_forced != 15);
    int bx = tid & 3, by = tid >> 2;                     // 8x8 block inside the 32x32 block
    int k = (by >> 1) * 2 + (bx >> 1);
    uint32_t ci = (uint32_t)(split ? red[k] : red[4]) & 0x1fff;
    int i = b8idx(f, x0 + bx * 8, y0 + by * 8);
    f.cu_log2[i] = split ? 4 : 5;
    f.cu_intra[i] = 0;
    f.cu_mvp_idx[i] = 1;                                 // mark for k_subpel: searched
    const int rsel = CO ? (int)(((split ? red[k] : red[4]) >> 14) & 7) : (MR ? (int)(((split ? red[k] : red[4]) >> 13) & 7) : 0);
    if (MR) f.cu_ref[i] = (uint8_t)rsel;
    int cx = 0, cy = 0;                                  // (CO: a candidate of the second window counts from the chosen reference's centre)
    if constexpr (CO) {
      if (((split ? red[k] : red[4]) >> 13) & 1) {
        const int16_t *c = f.mc_centres + 2 * ((size_t)rsel * (f.cw >> 5) * (f.ch >> 5) + (size_t)(y0 >> 5) * (f.cw >> 5) + (x0 >> 5));
        cx = c[0]; cy = c[1];
      }
    }
    f.cu_mv[i * 2] = (int16_t)((cx + (int)(ci % W) - R) * 4);
    f.cu_mv[i * 2 + 1] = (int16_t)((cy + (int)(ci / W) - R) * 4);
    // intra-in-P: the inter cost of the block's 16x16 quarters -- what the search found for a quarter, or a quarter of the 32x32 block's cost
    if constexpr (FQ) {                                  // a forced quarter: past the gate whatever the search found; ir_free 0 (intra-in-p 0): no other quarter is priced
      if (tid < 4) f.me_cost16[((y0 >> 4) + (tid >> 1)) * (f.cw >> 4) + (x0 >> 4) + (tid & 1)] =
        ((ir_forced >> tid) & 1) ? 0xffffffffu : (!f.ir_free ? 0u : (split ? (uint32_t)(red[tid] >> KS) : ((uint32_t)(red[4] >> KS) + 2) >> 2));
      if (tid == 0) {
        bool any = ir_forced != 0;
        if (f.ir_free) for (int k = 0; k < 4; k++) any |= (split ? (uint32_t)(red[k] >> KS) : ((uint32_t)(red[4] >> KS) + 2) >> 2) > (uint32_t)INTRA_P_GATE * lam;
        if (any) f.me_cand[1 + atomicAdd(&f.me_cand[0], 1u)] = (uint32_t)((y0 >> 5) * (f.cw >> 5) + (x0 >> 5));
      }
    } else {
    if (f.intra_p && tid < 4) f.me_cost16[((y0 >> 4) + (tid >> 1)) * (f.cw >> 4) + (x0 >> 4) + (tid & 1)] = split ? (uint32_t)(red[tid] >> KS) : ((uint32_t)(red[4] >> KS) + 2) >> 2;
    if (f.intra_p && tid == 0) {
      // ... and the block joins the list k_intra_analyse<P> works through when a quarter is above the gate (f.me_cand: count, then block indices)
      bool any = false;
      for (int k = 0; k < 4; k++) any |= (split ? (uint32_t)(red[k] >> KS) : ((uint32_t)(red[4] >> KS) + 2) >> 2) > (uint32_t)INTRA_P_GATE * lam;
      if (any) f.me_cand[1 + atomicAdd(&f.me_cand[0], 1u)] = (uint32_t)((y0 >> 5) * (f.cw >> 5) + (x0 >> 5));
    }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// "uvgx coarse-to-fine search v1" (me-coarse): the quarter picture and the coarse stage
// ---------------------------------------------------------------------------------------------
// Quarter picture of the padded luma plane: q(x, y) = (sum of the 4x4 samples at (4x, 4y) + 8) >> 4.  A thread reads four rows of 16 bytes and writes
// four quarter samples as one word; cw is a multiple of 64, so every access is aligned.
__global__ __launch_bounds__(256) void k_luma_quarter(const uint8_t *src, uint8_t *q, int cw, int ch)
{
  const int gx = blockIdx.x * 64 + threadIdx.x, gy = blockIdx.y * 4 + threadIdx.y;        // word gx of quarter row gy
  if (gx * 16 >= cw || gy * 4 >= ch) return;
  kv_u32x4 v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) v[k] = *reinterpret_cast<const kv_u32x4 *>(src + (size_t)(gy * 4 + k) * cw + gx * 16);
  uint32_t out = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t sum = 8;
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t w = j == 0 ? v[k].x : (j == 1 ? v[k].y : (j == 2 ? v[k].z : v[k].w)); sum = __builtin_amdgcn_sad_u8(w, 0u, sum); }
    out |= (sum >> 4) << (8 * j);
  }
  *reinterpret_cast<uint32_t *>(q + (size_t)gy * (cw >> 2) + gx * 4) = out;
}

// Coarse stage: one workgroup per (32x32 block, reference).  The block is 8x8 samples of the quarter picture; its window of the reference's quarter
// picture, (8 + 2 rq)^2 samples clamped to the picture's edge, sits in LDS.  A work item is a QUAD of horizontally adjacent candidates:
// v_qsad_pk_u16_u8 gives the four SADs of 4 samples of a row, two of them a row (an 8x8 SAD is at most 16 320: the u16 accumulators hold it).
// Minimum of me_coarse_key() -- cost << 16 | raster index of the candidate -- over the admissible candidates; the centre goes to mc_centres.
#define MEC_MAXRQ 64
#define MEC_PITCH (2 * MEC_MAXRQ + 12)        // bytes per window row: 8 + 2 rq samples, + 4 so the last quad's third word stays inside
__global__ __launch_bounds__(256) void k_me_coarse(EncFrame f)
{
  __shared__ __attribute__((aligned(16))) uint8_t wbuf[(8 + 2 * MEC_MAXRQ) * MEC_PITCH];
  __shared__ unsigned long long red;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int bx = blockIdx.x, by = blockIdx.y, rf = blockIdx.z;
  const int rq = f.mc_rq, wq = 2 * rq + 1, wcols = 8 + 2 * rq, pitch = wcols + 4;
  const int qw = f.cw >> 2, qh = f.ch >> 2, x0 = bx * 32, y0 = by * 32;
  const uint8_t *refq = f.mc_qrefs[rf];
  if (tid == 0) red = ~0ull;
  // the window: word wx of row wy is quarter-picture samples (8 bx - rq + 4 wx ..) of row 8 by - rq + wy; rq and the picture's width are multiples of 4,
  // so a word lies inside the picture or outside it as a whole
  for (int i = tid; i < wcols * (pitch >> 2); i += nthreads) {
    const int wy = i / (pitch >> 2), wx = i - wy * (pitch >> 2);
    const int gy = clip3(0, qh - 1, by * 8 - rq + wy), gx = bx * 8 - rq + wx * 4;
    const uint8_t *row = refq + (size_t)gy * qw;
    uint32_t v;
    if (gx >= 0 && gx + 3 < qw) v = *reinterpret_cast<const uint32_t *>(row + gx);
    else v = (uint32_t)row[gx < 0 ? 0 : qw - 1] * 0x01010101u;
    *reinterpret_cast<uint32_t *>(&wbuf[wy * pitch + wx * 4]) = v;
  }
  uint32_t cur[16];                                              // the block: 8 rows of two words
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const uint32_t *c = reinterpret_cast<const uint32_t *>(f.mc_q + (size_t)(by * 8 + r) * qw + bx * 8);
    cur[2 * r] = c[0]; cur[2 * r + 1] = c[1];
  }
  int ty0, ty1, tx0, tx1;
  me_tile_span(f.ch >> 6, f.tile_rows, y0 >> 6, true, &ty0, &ty1);
  me_tile_span(f.cw >> 6, f.tile_cols, x0 >> 6, false, &tx0, &tx1);
  __syncthreads();
  const uint32_t lam = (uint32_t)f.lambda_q4;
  const int NQ = (wq + 3) >> 2;
  unsigned long long best = ~0ull;
  for (int item = tid; item < NQ * wq; item += nthreads) {
    const int dyi = item / NQ, q = item - dyi * NQ;
    if (!me_axis_ok(4 * (dyi - rq), y0, ty0, ty1, f.ch, f.mv_frame)) continue;
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
      const int dxi = 4 * q + k4;
      if (dxi >= wq || !me_axis_ok(4 * (dxi - rq), x0, tx0, tx1, f.cw, f.mv_frame)) continue;
      const unsigned long long key = me_coarse_key((uint32_t)(acc >> (16 * k4)) & 0xffffu, dxi, dyi, rq, lam);
      best = key < best ? key : best;
    }
  }
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = __shfl_xor(best, o); best = v < best ? v : best; }
  if ((tid & 63) == 0) atomicMin(&red, best);
  __syncthreads();
  if (tid == 0) {
    int cx, cy;
    me_coarse_centre(red, rq, &cx, &cy);
    int16_t *c = f.mc_centres + 2 * ((size_t)rf * (f.cw >> 5) * (f.ch >> 5) + (size_t)by * (f.cw >> 5) + bx);
    c[0] = (int16_t)cx; c[1] = (int16_t)cy;
  }
}

// =============================================================================================
// Entropy coding, parallel half: one wave per 16x16 block turns its coding unit(s) into the list
// of CABAC bins in coding order (16-bit tokens, hevc_core.h TokOut).  The wave stages the per-CU
// records of the block and its left / above neighbours in LDS, lane 0 emits the (short) CU headers,
// and every transform block is tokenised by all lanes at once: one lane per 4x4 sub-block, whose
// only cross-sub-block dependency (the greater1 context set) is resolved from a ballot of
// "has a level > 1".  The serial arithmetic coder runs on host threads (entropy_host.h).
// =============================================================================================
struct TileView {
  const CuRec *tile;                 // [3][3] records: b8 (bx0 + tx, by0 + ty): the unit and its left / above neighbours
  int bx0, by0;
  __device__ CuRec at(int x, int y) const { return tile[((y >> 3) - by0) * 3 + ((x >> 3) - bx0)]; }
};

// The tokenizer's tables as constants of the code object (round 5; until then every wave computed them -- a dozen dependent loads from the constant tables,
// 2 us of a 17 us wave): CoreTabs as the host code has it, and the sig_coeff_flag context patterns by SCAN POSITION -- sigk[scan][pattern][k] =
// sigpat[pattern][pos4[scan][k]], pattern 4 = the 4x4 block's map -- so that a sub-block's sixteen patterns are one 16-byte LDS read.
struct alignas(16) TokTabs { uint8_t sigk[3][5][16]; };
constexpr CoreTabs make_core_tabs() { CoreTabs t{}; for (int i = 0; i < 64; i++) core_tabs_fill_entry(t, i); return t; }
constexpr TokTabs make_tok_tabs()
{
  const CoreTabs c = make_core_tabs();
  TokTabs t{};
  for (int sc = 0; sc < 3; sc++) for (int k = 0; k < 16; k++) {
    for (int pc = 0; pc < 4; pc++) t.sigk[sc][pc][k] = c.sigpat[pc][c.pos4[sc][k]];
    t.sigk[sc][4][k] = c.ctxmap4x4[c.pos4[sc][k]];
  }
  return t;
}
static __device__ const CoreTabs g_core_tabs = make_core_tabs();
static __device__ const TokTabs g_tok_tabs = make_tok_tabs();
static_assert(sizeof(CoreTabs) % 4 == 0 && sizeof(TokTabs) % 16 == 0, "copied by dwords / 16-byte words");

// A lane's 4x4 sub-block in registers: its sixteen levels in scan order as int16 pairs and the significance mask (bit k = scan position k).  Everything the
// tokenizer does with a sub-block -- two passes over its coefficients -- reads these eight registers with compile-time indices (the loops below are unrolled
// over the sixteen positions) instead of a dependent LDS read per coefficient and pass (round 4: 10 of a wave's 17.7 us, profiles/r04_tok_phases.txt).
struct SbRegs { uint32_t w[8]; uint32_t m; };
__device__ __forceinline__ int sb_level(const SbRegs &r, int k) { return (int)(int16_t)(uint16_t)(r.w[k >> 1] >> ((k & 1) * 16)); }      // k: a compile-time constant where it matters

template <bool KEEP_LDS>
__device__ __forceinline__ void digest_build_wave(const CoreTabs *t, TuDigest &d, const int16_t *lv, int stride, int log2, int scan_idx, int lane, SbRegs &sb)
{
  const int sbl = log2 - 2, nsb2 = 1 << (2 * sbl);
  d.csbf[lane] = 0;
  wave_sync();
  bool nz = false;
  sb.m = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) sb.w[k] = 0;
  if (lane < nsb2) {
    int xs, ys; scan_pos(t, scan_idx, sbl, lane, xs, ys);
    const int16_t *p = lv + (ys << 2) * stride + (xs << 2);
    uint2 r0 = *reinterpret_cast<const uint2 *>(p), r1 = *reinterpret_cast<const uint2 *>(p + stride);
    uint2 r2 = *reinterpret_cast<const uint2 *>(p + 2 * stride), r3 = *reinterpret_cast<const uint2 *>(p + 3 * stride);
    // the lane's 32 bytes of the digest's scratch: the sub-block in raster order, read back through the scan table in scan order
    uint2 *dst = reinterpret_cast<uint2 *>(&d.scan[lane * 16]);
    dst[0] = r0; dst[1] = r1; dst[2] = r2; dst[3] = r3;
    const uint8_t *pos = t->pos4[scan_idx];
    int v[16];
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { v[k] = d.scan[lane * 16 + pos[k]]; if (v[k]) m |= 1u << k; }
#pragma unroll
    for (int k = 0; k < 8; k++) sb.w[k] = ((uint32_t)v[2 * k] & 0xffffu) | ((uint32_t)v[2 * k + 1] << 16);
    if (KEEP_LDS) {                                        // (all reads of the raster form are done: the scan-order form takes its place for enc_subblock())
      uint32_t *d32 = reinterpret_cast<uint32_t *>(&d.scan[lane * 16]);
#pragma unroll
      for (int k = 0; k < 8; k++) d32[k] = sb.w[k];
    }
    sb.m = m;
    d.mask[lane] = (uint16_t)m;
    nz = m != 0;
    if (nz) d.csbf[ys * 8 + xs] = 1;
  }
  uint64_t sb64 = __ballot(nz);
  if (lane == 0) d.sbmask = sb64;
  wave_sync();
}

// subblock_g1_any() from registers: one of the sub-block's first eight coefficients in coding order has |level| > 1
__device__ __forceinline__ bool sb_g1_any(const SbRegs &r)
{
  bool any = false; int seen = 0;
#pragma unroll
  for (int k = 15; k >= 0; k--) if ((r.m >> k) & 1) { const int v = sb_level(r, k); if (seen < 8 && (v > 1 || v < -1)) any = true; seen++; }
  return any;
}

// enc_subblock() (hevc_core.h: the statement both forms follow, and the one the host tests drive) for a sub-block held in registers.  sk: the sixteen context
// patterns of the sub-block's scan positions (TokTabs::sigk row, four dwords).
template <class S>
__device__ __forceinline__ void enc_subblock_regs(S &c, const TuDigest &d, const SbRegs &r, const uint32_t (&sk)[4], int i, int last_sb, int last_pos, bool prev_g1, int log2, int cidx, int scan_idx, int sign_hiding)
{
  const int sbl = log2 - 2, nsb = 1 << sbl;
  int xs, ys; scan_pos(c.tabs, scan_idx, sbl, i, xs, ys);
  const int right = (xs < nsb - 1) ? d.csbf[ys * 8 + xs + 1] : 0;
  const int below = (ys < nsb - 1) ? d.csbf[(ys + 1) * 8 + xs] : 0;
  const uint32_t m = r.m;
  int coded = m != 0, infer_dc = 0;
  if (i < last_sb && i > 0) {
    cabac_bin(c, CTX_CSBF + ((right | below) ? 1 : 0) + (cidx ? 2 : 0), coded);
    infer_dc = 1;
  } else coded = 1;                        // inferred 1 for the last and the DC sub-block
  if (!coded) return;
  const int sigbase = CTX_SIG + (cidx ? 27 : 0);
  const int off = log2 == 2 ? 0 : (cidx == 0 ? ((i > 0 ? 3 : 0) + ((log2 == 3) ? ((scan_idx == 0) ? 9 : 15) : 21)) : ((log2 == 3) ? 9 : 12));
  const int start = (i == last_sb) ? last_pos - 1 : 15;
  if constexpr (sink_counts_only<S>::value) {
    if (start >= 0) c.n += start + 1 - ((infer_dc && (m >> 1) == 0) ? 1 : 0);
  } else {
#pragma unroll
    for (int k = 15; k >= 1; k--) if (k <= start) cabac_bin(c, sigbase + (int)((sk[k >> 2] >> ((k & 3) * 8)) & 0xffu) + off, (int)((m >> k) & 1));
    if (start >= 0 && !(infer_dc && (m >> 1) == 0))                 // (position 0: not sent when every other flag of a coded sub-block is zero; the block's DC coefficient has its own context)
      cabac_bin(c, sigbase + ((i == 0 && log2 != 2) ? 0 : (int)(sk[0] & 0xffu) + off), (int)(m & 1));
  }
  if (!m) return;
  int ctx_set = (i > 0 && cidx == 0) ? 2 : 0;
  if (prev_g1) ctx_set++;
  int c1 = 1, nsig = 0, g1idx = -1, g2 = 0;
  uint32_t signs = 0;
#pragma unroll
  for (int k = 15; k >= 0; k--) if ((m >> k) & 1) {
    const int v = sb_level(r, k), a = v < 0 ? -v : v;
    signs = (signs << 1) | (v < 0 ? 1u : 0u);
    if (nsig < 8) {
      const int g1 = a > 1;
      cabac_bin(c, CTX_GT1 + (cidx ? 16 : 0) + ctx_set * 4 + c1, g1);
      if (g1) { c1 = 0; if (g1idx < 0) { g1idx = nsig; g2 = a > 2; } }
      else if (c1 > 0 && c1 < 3) c1++;
    }
    nsig++;
  }
  if (g1idx >= 0) cabac_bin(c, CTX_GT2 + (cidx ? 4 : 0) + ctx_set, g2);
  if (sign_hiding && (31 - __builtin_clz(m)) - __builtin_ctz(m) > 3) cabac_bypass_bits(c, signs >> 1, nsig - 1);
  else cabac_bypass_bits(c, signs, nsig);
  int rice = 0, j = 0;
#pragma unroll
  for (int k = 15; k >= 0; k--) if ((m >> k) & 1) {
    const int v = sb_level(r, k), a = v < 0 ? -v : v;
    const int base = (j < 8) ? ((j == g1idx) ? 3 : 2) : 1;
    if (a >= base) {
      enc_abs_remaining(c, a - base, rice);
      if (a > 3 * (1 << rice)) rice = imin(rice + 1, 4);
    }
    j++;
  }
}

#define TOK_HDR_CAP 192        // split flags + CU header + last-position bins waiting for the piece they open
#define TOK_ARENA 512          // tokens of one piece staged in LDS (larger pieces are written straight to the slot)
#define TOK_PIECES 17          // pieces one unit can produce: 4 CUs x (header-only | one per coded component) + the CTU's terminating bins

// One wave per 16x16 luma block ("unit") and ROLE -- luma, Cb, Cr, and (round 5) the CU HEADERS on a wave of their own: the header bins are a serial
// walk on one lane (3.3 us), which the luma wave -- the longest one -- no longer carries in front of its transform block -- or, ALLC, one
// wave per unit that takes the roles in turn.  Every wave works on its own, with its own LDS state and no workgroup barrier
// (NW waves per workgroup: NW = 4, the units of a 32x32 quadrant, was measured and is no faster than NW = 1 -- the kernel is bound by
// the number of waves to start and by its longest waves, not by workgroup dispatch; more waves per SIMD is: six -- 79 registers, the
// most that needs no scratch memory; eight spill, 5 MB of extra traffic per 1080p picture -- 4K 73 -> 67 us, profiles/r02_tokenizer_timeline.txt).
// A unit owns the CU that starts at its origin (32x32 or
// 16x16) or the four 8x8 CUs inside it; units covered by a 32x32 CU that starts elsewhere emit
// nothing.  The tokens leave the unit in PIECES, four per CU in coding order: its header (split flags, CU header, cu_qp_delta; the CTU's SAO syntax in
// front of the first), then one per coded transform block (luma -- led by its last-position bins --, Cb, Cr); piece 16: the CTU's terminating bins.  For each piece the
// lanes first COUNT the tokens of their 4x4 sub-blocks (the emitters run with a zero-capacity
// sink), the piece reserves its place in the CTU's slot with one atomicAdd, and a second run of the
// emitters writes the tokens at their final offsets -- through a small LDS arena when the piece
// fits, which keeps the kernel at ~10 KB of LDS per wave.  k_tok_compact restores coding order
// from the (offset, length) table [ctu][unit][piece].
// waves per SIMD the register budget is cut for: six (80 registers) spilled eight of them once a sub-block's levels stayed in registers (round 5); five (102) holds all
#ifndef KVZ_TOK_WAVES
#define KVZ_TOK_WAVES 5
#endif
struct alignas(16) TokWave {
  TuDigest dg;
  TokTabs tk;
  CoreTabs tabs;
  CuRec tile[9];
  uint16_t hdr[TOK_HDR_CAP];
  uint16_t arena[TOK_ARENA];
  int hdr_n;
  uint32_t piece_off;
  uint32_t seg[TOK_PIECES][2];
};
// HDRW: the headers on a wave of their own (grid z = 4); else the luma wave carries them (z = 3).  REGS: a sub-block's levels in registers through both passes
// (enc_subblock_regs: sixteen exec-masked positions per pass) or in LDS (hevc_core.h enc_subblock: a dependent LDS read per significant level).  At 1080p the
// kernel is as long as its longest wave and both help (31 -> 27.7 -> 24.2 us); at 2160p it is bound by the number of waves and of instructions, and both cost
// (55 -> 60 -> 63 us): pictures of more than 16 384 units keep round 4's form.
// one (unit, role) of k_tokenize on one wave.  have_tabs: the wave's tables are in LDS already (the list form: a wave's second item and later)
template <bool ALLC, bool HDRW, bool REGS>
__device__ __forceinline__ void tok_unit(const EncFrame &f, TokWave &W, const int ux, const int uy, const int comp, const int lane, const bool have_tabs)
{
  CuRec *tile = W.tile; TuDigest &dg = W.dg; CoreTabs &tabs = W.tabs; uint16_t *hdr = W.hdr, *arena = W.arena;
  int &hdr_n = W.hdr_n; uint32_t &piece_off = W.piece_off; uint32_t (&seg)[TOK_PIECES][2] = W.seg;
  // comp: 0 luma, 1 Cb, 2 Cr, 3 the headers and the CTU's terminating bins (ALLC: 0 stands for all of them)
  const int wc = f.cw >> 6, hc = f.ch >> 6;
  const int hdr_comp = HDRW ? 3 : 0;
  const bool hdr_role = ALLC || comp == hdr_comp;
  const int cx = ux >> 2, cy = uy >> 2, ctu = cy * wc + cx;
  const int X0 = ux * 16, Y0 = uy * 16;
  int z4 = 0;                                          // z-order index of the unit inside its CTU
  for (int b = 0; b < 2; b++) z4 |= (((ux & 3) >> b) & 1) << (2 * b) | (((uy & 3) >> b) & 1) << (2 * b + 1);
  // Most waves of an inter picture have nothing to say (units inside a 32x32 CU that starts elsewhere, chroma of CUs without
  // chroma residual): they find that out from a few bytes and leave with their table entries zeroed.
  unsigned long long *tr = (f.trace && hdr_role && lane == 0 && (z4 == 0 || z4 == 15)) ? f.trace + (size_t)wc * hc * 32 + (size_t)ctu * 8 : nullptr;   // (tools/tok_timeline.py)
  if (tr) tr[z4 == 0 ? 5 : 6] = wall_clock64();
  // wave census (tools/tok_timeline.py): per class {left at once, header only, with residual} x {P, I}: waves and 10 ns ticks
  unsigned long long *census = f.trace ? f.trace + (size_t)wc * hc * 40 + (size_t)ctu * 16 + (f.is_intra ? 6 : 0) : nullptr;
  const unsigned long long t_begin = census ? wall_clock64() : 0;
  int wave_class = 1;
  // phases of a luma wave that codes ONE coding unit with residual (tools/tok_phases.py; a build with EXTRA=-DKVZ_TOK_PHASES -- nine time stamps
  // held in registers cost the kernel 88 scalar spills): ticks per phase summed per CTU, slot 15 counts the waves
#ifdef KVZ_TOK_PHASES
  unsigned long long *ph = (f.trace && comp == 0 && !f.is_intra) ? f.trace + (size_t)wc * hc * 56 + (size_t)ctu * 16 : nullptr;
  unsigned long long ph_t[9]; int ph_n = 0;
#define TOK_PH() do { if (ph && ph_n < 9) ph_t[ph_n++] = wall_clock64(); } while (0)
#define TOK_PH_SYNC() wave_sync()
#else
#define TOK_PH() do { } while (0)
#define TOK_PH_SYNC() do { } while (0)
#endif
  TOK_PH();
  // table entries this wave writes: piece 4k + 0 the header of CU k (and piece 16, the terminators): the header role; 4k + 1 + c: component c
  auto mine = [&](int piece) { return ALLC || ((piece == 16 || (piece & 3) == 0) ? hdr_comp : (piece & 3) - 1) == comp; };
  if (!(hdr_role && z4 == 15)) {
    const int g0 = (uy * 2) * f.b8w + ux * 2, l0 = f.cu_log2[g0];
    bool work = !(l0 == 5 && ((X0 | Y0) & 31));
    if (!ALLC && work && comp != hdr_comp) {              // a component's wave (that does not also carry the headers): one of the unit's CUs has residual of it
      bool c = false;
      if (lane < (l0 == 3 ? 4 : 1)) { const int g = g0 + (lane >> 1) * f.b8w + (lane & 1); c = !(f.cu_flags[g] & CU_SKIP) && ((f.cu_cbf[g] >> comp) & 1); }
      work = __ballot(c) != 0;
    }
    if (!work) {
      if (lane < TOK_PIECES && mine(lane)) { uint32_t *e = f.tok_seg + ((size_t)(ctu * 16 + z4) * TOK_PIECES + lane) * 2; e[0] = 0; e[1] = 0; }
      if (census && lane == 0) { atomicAdd(&census[0], 1ull); atomicAdd(&census[1], wall_clock64() - t_begin); }
      return;
    }
  }
  TOK_PH();                                                        // 1: the unit has something to say
  if (!have_tabs) {
    for (int i = lane; i < (int)(sizeof(CoreTabs) / 4); i += 64) reinterpret_cast<uint32_t *>(&tabs)[i] = reinterpret_cast<const uint32_t *>(&g_core_tabs)[i];
    if (lane < (int)(sizeof(TokTabs) / 16)) reinterpret_cast<uint4 *>(&W.tk)[lane] = reinterpret_cast<const uint4 *>(&g_tok_tabs)[lane];
  }
  if (lane < TOK_PIECES) { seg[lane][0] = 0; seg[lane][1] = 0; }
  if (lane == 0) hdr_n = 0;
  const int bx0 = ux * 2 - 1, by0 = uy * 2 - 1;
  if (lane < 9) {
    int bx = bx0 + lane % 3, by = by0 + lane / 3;
    CuRec r; r.log2 = 0; r.intra = 0; r.flags = 0; r.merge_idx = 0; r.mvp_idx = 0; r.intra_mode = 0; r.cbf = 0; r.ref = 0; r.mvdx = 0; r.mvdy = 0;
    if (bx >= 0 && by >= 0) {
      int g = by * f.b8w + bx;
      r.log2 = f.cu_log2[g]; r.intra = f.cu_intra[g]; r.flags = f.cu_flags[g]; r.merge_idx = f.cu_merge_idx[g];
      r.mvp_idx = f.cu_mvp_idx[g]; r.intra_mode = f.cu_intra_mode[g]; r.cbf = f.cu_cbf[g];
      r.mvdx = f.cu_mvd[g * 2]; r.mvdy = f.cu_mvd[g * 2 + 1]; r.ref = (uint8_t)cu_ref_at(f, g);
    }
    tile[lane] = r;
  }
  wave_sync();
  TOK_PH();                                                        // 2: tables and the 3 x 3 records in LDS
  uint16_t *slot = f.tok_buf + (size_t)ctu * f.tok_cap;
  int np = 0;                                          // piece being produced (wave-uniform): CU k, component c -> 4k + c; 16 = terminators
  // reserve `total` tokens of the CTU's slot for piece np; all lanes get the offset (or ~0u when the slot is full)
  auto reserve = [&](int total) -> uint32_t {
    if (lane == 0) {
      uint32_t o = atomicAdd(&f.tok_cursor[ctu], (uint32_t)total);
      if (o + (uint32_t)total > (uint32_t)f.tok_cap) { atomicOr(f.err, 16u); o = ~0u; }
      else { seg[np][0] = o; seg[np][1] = (uint32_t)total; }
      piece_off = o;
    }
    wave_sync();
    return piece_off;
  };
  TileView v; v.tile = tile; v.bx0 = bx0; v.by0 = by0;
  const int cl0 = v.at(X0, Y0).log2;
  const bool owner = !(cl0 == 5 && ((X0 | Y0) & 31));
  const int ncu = owner ? (cl0 == 3 ? 4 : 1) : 0;
  for (int k = 0; k < ncu; k++) {
    const int x0 = X0 + ((cl0 == 3) ? (k & 1) * 8 : 0), y0 = Y0 + ((cl0 == 3) ? (k >> 1) * 8 : 0);
    const CuRec cu = v.at(x0, y0);
    int z = 0;                                         // z-order index (8x8 units) of the CU origin inside the CTU
    for (int b = 0; b < 3; b++) z |= ((((x0 & 63) >> 3) >> b) & 1) << (2 * b) | ((((y0 & 63) >> 3) >> b) & 1) << (2 * b + 1);
    if (lane == 0 && hdr_role) {
      TokOut t; t.tabs = &tabs; t.p = hdr; t.n = 0; t.cap = TOK_HDR_CAP;
      if (f.sao && z4 == 0 && k == 0) {                 // coding_tree_unit() starts with sao()
        const bool hl = cx > 0 && !tile_col_starts_at(wc, f.tile_cols, cx), hu = cy > 0 && !tile_row_starts_at(hc, f.tile_rows, cy);
        enc_sao(t, f.sao[ctu], hl ? &f.sao[ctu - 1] : nullptr, hu ? &f.sao[ctu - wc] : nullptr);     // (read where they lie: a local copy indexed at run time would live in scratch memory)
      }
      enc_split_flags(v, t, f.cw, f.chp, x0, y0, z, cu.log2);
      enc_cu_header(v, t, f.cw, f.chp, f.is_intra != 0, x0, y0, cu, f.lossless != 0, f.cu_ref ? f.nref : 1);
      // the quantisation group's (= CTU's) delta QP goes with its first CU that has residual, right after the cbf flags
      if (f.ctu_qy && !(cu.flags & CU_SKIP) && cu.cbf && z == f.ctu_first[ctu]) enc_cu_qp_delta(t, f.ctu_delta[ctu]);
      hdr_n = t.n;
    }
    TOK_PH_SYNC(); TOK_PH();                                       // 3: lane 0 has the header bins
    if (hdr_role) {                                                 // the CU's header: piece 4k + 0
      np = 4 * k;
      wave_sync();
      const int hn = hdr_n > TOK_HDR_CAP ? TOK_HDR_CAP : hdr_n;
      if (hdr_n > TOK_HDR_CAP && lane == 0) atomicOr(f.err, 8u);
      const uint32_t o = reserve(hn);
      if (o != ~0u) for (int i = lane; i < hn; i += 64) slot[o + i] = hdr[i];
      wave_sync();
      if (lane == 0) hdr_n = 0;
      wave_sync();
    }
    const int cbf = (cu.flags & CU_SKIP) ? 0 : cu.cbf;          // wave-uniform
    for (int ci = (ALLC || comp == 3) ? 0 : comp; ci < (ALLC ? 3 : (comp == 3 ? 0 : comp + 1)); ci++) {   // the CU's transform blocks: luma, Cb, Cr (ALLC) or this wave's component (a wave that only carries headers: none)
      np = 4 * k + 1 + ci;
      if ((cbf >> ci) & 1) {
        wave_class = 2;
        const int l2 = ci ? cu.log2 - 1 : cu.log2, pw = ci ? (f.cw >> 1) : f.cw;
        const int px = ci ? (x0 >> 1) : x0, py = ci ? (y0 >> 1) : y0;
        const int scan = intra_scan_idx(cu.intra, l2, ci, cu.intra_mode);
        SbRegs sb;
        digest_build_wave<!REGS>(&tabs, dg, f.coef[ci] + py * pw + px, pw, l2, scan, lane, sb);   // ends with a barrier
        TOK_PH();                                                  // 4: digest
        const uint64_t sbm = dg.sbmask;
        const int last_sb = 63 - __builtin_clzll(sbm);
        const int last_pos = 31 - __builtin_clz((uint32_t)dg.mask[last_sb]);
        if (lane == 0) {
          TokOut t; t.tabs = &tabs; t.p = hdr; t.n = hdr_n; t.cap = TOK_HDR_CAP;
          int a, b; enc_last_pos(t, dg, l2, ci, scan, a, b);
          hdr_n = t.n;
        }
        // greater1 context-set carry: sub-block i inherits from the next non-empty sub-block above it
        const bool nzsb = (sbm >> lane) & 1;
        const bool g1 = nzsb && sb_g1_any(sb);
        const uint64_t g1m = __ballot(g1);
        bool prev_g1 = false;
        if (lane <= last_sb) {
          uint64_t above = (lane < 63) ? (sbm >> (lane + 1)) : 0;      // non-empty sub-blocks coded before this one
          if (above) { int j = lane + 1 + __builtin_ctzll(above); prev_g1 = (g1m >> j) & 1; }
        }
        // the sub-block's sixteen sig_coeff_flag context patterns: by the neighbouring sub-blocks' coded flags, or the 4x4 block's own map
        uint32_t sk[4] = {0, 0, 0, 0};
        if (lane <= last_sb) {
          const int sbl = l2 - 2, nsb = 1 << sbl;
          int xs, ys; scan_pos(&tabs, scan, sbl, lane, xs, ys);
          const int right = (xs < nsb - 1) ? dg.csbf[ys * 8 + xs + 1] : 0, below = (ys < nsb - 1) ? dg.csbf[(ys + 1) * 8 + xs] : 0;
          const uint4 q = *reinterpret_cast<const uint4 *>(W.tk.sigk[scan][l2 == 2 ? 4 : (right | (below << 1))]);
          sk[0] = q.x; sk[1] = q.y; sk[2] = q.z; sk[3] = q.w;
        }
        // pass 1: count
        int n_l = 0;
        if (lane <= last_sb) {
          TokCount t; t.tabs = &tabs; t.n = 0;
          if (REGS) enc_subblock_regs(t, dg, sb, sk, lane, last_sb, last_pos, prev_g1, l2, ci, scan, f.signhide);
          else enc_subblock(t, dg, lane, last_sb, last_pos, prev_g1, l2, ci, scan, f.signhide);
          n_l = t.n;
        }
        // offsets in coding order: sub-block last_sb first, then downwards
        int suffix = n_l;
        for (int o = 1; o < 64; o <<= 1) { int other = __shfl_down(suffix, o); if (lane + o < 64) suffix += other; }
        const int body = __shfl(suffix, 0);
        const int off = suffix - n_l;                                 // tokens of all sub-blocks with a higher index
        wave_sync();                                              // hdr_n of lane 0 visible
        const int hn = hdr_n > TOK_HDR_CAP ? TOK_HDR_CAP : hdr_n, total = hn + body;
        if (hdr_n > TOK_HDR_CAP && lane == 0) atomicOr(f.err, 8u);
        TOK_PH();                                                  // 5: last position, greater1 carry, count pass, offsets
        const uint32_t o = reserve(total);
        TOK_PH();                                                  // 6: place reserved
        if (o != ~0u) {
          const bool staged = total <= TOK_ARENA;
          uint16_t *dst = staged ? arena : slot + o;
          for (int i = lane; i < hn; i += 64) dst[i] = hdr[i];
          if (lane <= last_sb && n_l) {                               // pass 2: the same emitters, now writing at the final offsets
            TokOut t; t.tabs = &tabs; t.p = dst + hn + off; t.n = 0; t.cap = n_l;
            if (REGS) enc_subblock_regs(t, dg, sb, sk, lane, last_sb, last_pos, prev_g1, l2, ci, scan, f.signhide);
            else enc_subblock(t, dg, lane, last_sb, last_pos, prev_g1, l2, ci, scan, f.signhide);
          }
          if (staged) {
            wave_sync();
            for (int i = lane; i < total; i += 64) slot[o + i] = arena[i];
          }
        }
        wave_sync();
        TOK_PH();                                                  // 7: tokens written
        if (lane == 0) hdr_n = 0;
      }
      wave_sync();
    }
  }
  if (z4 == 15 && hdr_role) {                                       // the last unit of the CTU closes it
    const bool last = (cy == hc - 1 && cx == wc - 1);
    const bool row_end = tile_col_ends_at(wc, f.tile_cols, cx);                                   // last CTU of its row inside the tile
    const bool sub_end = row_end && (f.wpp || tile_row_ends_at(hc, f.tile_rows, cy));
    const bool seg_end = last || (row_end && (f.slices == 1 || (f.slices == 2 && tile_row_ends_at(hc, f.tile_rows, cy))));   // slice segments per CTU row / per tile
    const int n = 1 + ((sub_end && !seg_end) ? 1 : 0);
    wave_sync();
    np = 16;
    const uint32_t o = reserve(n);
    if (o != ~0u && lane == 0) {
      slot[o] = (uint16_t)(0xC000u | (seg_end ? 1u : 0u));          // end_of_slice_segment_flag
      if (n == 2) slot[o + 1] = 0xC001u;                            // end_of_subset_one_bit
    }
  }
  wave_sync();
  if (lane < TOK_PIECES && mine(lane)) {
    uint32_t *e = f.tok_seg + ((size_t)(ctu * 16 + z4) * TOK_PIECES + lane) * 2;
    e[0] = seg[lane][0]; e[1] = seg[lane][1];
  }
  TOK_PH();                                                        // 8: table entries out
#ifdef KVZ_TOK_PHASES
  if (ph && lane == 0 && ph_n == 9 && ncu == 1 && wave_class == 2) { for (int k = 0; k < 8; k++) atomicAdd(&ph[k], ph_t[k + 1] - ph_t[k]); atomicAdd(&ph[15], 1ull); }
#endif
#undef TOK_PH
#undef TOK_PH_SYNC
  if (tr && z4 == 15) tr[7] = wall_clock64();
  if (census && lane == 0) { atomicAdd(&census[wave_class * 2], 1ull); atomicAdd(&census[wave_class * 2 + 1], wall_clock64() - t_begin); }
}
// LIST (P pictures, whole pictures; round 6): the launch is a fixed number of waves that work off k_inter_signal's list of (unit, role) pairs with something to
// say (EncFrame::tok_list) instead of a wave per pair -- the pairs that are not listed keep the zero table entries k_tok_compact leaves behind.  The kernel was
// the time to start 32 640 waves (130 000 at 2160p) of which nine in ten left at once, plus its longest wave; now it is its longest wave.
template <bool ALLC, int NW, bool HDRW = true, bool REGS = true, bool LIST = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(REGS ? (LIST ? 3 : KVZ_TOK_WAVES) : 6))) void k_tokenize(EncFrame f)      // (the list form: few waves, each with work -- the registers it wants: at five waves per SIMD the item loop spilled 23)
{
  __shared__ TokWave tw[NW];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  TokWave &W = tw[wv];
  if constexpr (LIST) {
    const uint32_t count = f.tok_list[0], uw = (uint32_t)(f.cw >> 4);
    bool have = false;
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {
      const uint32_t v = f.tok_list[1 + it], unit = v >> 2;
      tok_unit<ALLC, HDRW, REGS>(f, W, (int)(unit % uw), (int)(unit / uw), (int)(v & 3u), lane, have);
      have = true;
      wave_sync();
    }
  } else {
    const int ux = NW == 4 ? blockIdx.x * 2 + (wv & 1) : blockIdx.x, uy = NW == 4 ? (blockIdx.y + f.row0 * 2) * 2 + (wv >> 1) : blockIdx.y + f.row0 * 4, comp = ALLC ? 0 : (int)blockIdx.z;
    tok_unit<ALLC, HDRW, REGS>(f, W, ux, uy, comp, lane, false);
  }
}

// one workgroup per CTU: the pieces of its 16 units in z-order, piece after piece -> the dense token array (CTUs in coding order)
// (tok_count_out[ctu] < 0 tells the host that the CTU did not fit or its table was inconsistent)
__global__ __launch_bounds__(256) void k_tok_compact(EncFrame f)
{
  constexpr int NSEG = 16 * TOK_PIECES;
  __shared__ uint32_t soff[NSEG], start[NSEG + 1], utot[17];
  __shared__ uint32_t wsum[4];
  const int first = f.row0 * (f.cw >> 6), ctu = blockIdx.x + first, tid = threadIdx.x;
  unsigned long long *tr = f.trace ? f.trace + (size_t)(f.cw >> 6) * (f.ch >> 6) * 32 + (size_t)ctu * 8 : nullptr;     // (tools/tok_timeline.py)
#define TC_STAMP(k) do { if (tr && tid == 0) tr[k] = wall_clock64(); } while (0)
  TC_STAMP(0);
  const uint32_t n = f.tok_cursor[ctu];
  // The CTU's place in the dense array: the tokens of all CTUs before it (every workgroup adds up the counts itself -- a few KB out of
  // L2 -- rather than queueing at one atomic counter: 2040 same-address atomics cost 25 ns each, which WAS this kernel's run time).
  // The next picture's cursors (the other of two arrays) go back to zero, and the device error word over to the host.
  uint32_t part = 0;
  for (int i = first + tid; i < ctu; i += 256) part += f.tok_cursor[i];
  part = wave_sum_u32(part);
  if ((tid & 63) == 0) wsum[tid >> 6] = part;
  if (tid == 0) { f.tok_cursor_next[ctu] = 0; if (blockIdx.x == 0) { *f.err_out = *f.err; if (f.ent_cursors) { f.ent_cursors[0] = 0; f.ent_cursors[1] = 0; } } }
  __syncthreads();
  const uint32_t base = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  TC_STAMP(1);
  // the CTU's table goes to LDS and back to zero in global memory: the next picture's tokenizer may be the list form, whose waves only write the entries of
  // the (unit, role) pairs that have something to say -- every other entry must read "no tokens"
  uint32_t *tab = f.tok_seg + (size_t)ctu * NSEG * 2;
  for (int i = tid; i < NSEG; i += 256) { const uint2 e = *reinterpret_cast<const uint2 *>(&tab[i * 2]); soff[i] = e.x; start[i] = e.y; *reinterpret_cast<uint2 *>(&tab[i * 2]) = make_uint2(0u, 0u); }        // start[] holds lengths for now
  if (f.tok_list && blockIdx.x == 0 && tid == 0) f.tok_list[0] = 0;      // (the list has been worked off: k_tokenize ran before this launch on the same stream)
  if (base + n > f.tok_dense_cap) { if (tid == 0) f.tok_count_out[ctu] = -1; return; }
  __syncthreads();
  TC_STAMP(2);
  if (tid < 16) { uint32_t a = 0; for (int p = 0; p < TOK_PIECES; p++) { uint32_t l = start[tid * TOK_PIECES + p]; start[tid * TOK_PIECES + p] = a; a += l; } utot[tid] = a; }
  __syncthreads();
  if (tid == 0) { uint32_t a = 0; for (int u = 0; u < 16; u++) { uint32_t t = utot[u]; utot[u] = a; a += t; } utot[16] = a; }
  __syncthreads();
  for (int i = tid; i < NSEG; i += 256) start[i] += utot[i / TOK_PIECES];
  if (tid == 0) start[NSEG] = utot[16];
  __syncthreads();
  const uint32_t total = start[NSEG];
  TC_STAMP(3);
  if (total != n) { if (tid == 0) f.tok_count_out[ctu] = -1; return; }
  const uint16_t *slot = f.tok_buf + (size_t)ctu * f.tok_cap;
  uint16_t *dst = f.tok_dense + base;
  int lo = 0;                                           // last segment with start <= i (empty segments share a start: take the last)
  for (uint32_t i = tid; i < n; i += 256) {
    if (start[lo + 1] <= i) {                           // past the segment of the previous round (long pieces: usually not)
      int hi = NSEG;
      while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (start[mid] <= i) lo = mid; else hi = mid; }
    }
    dst[i] = slot[soff[lo] + (i - start[lo])];
  }
  if (tid == 0) { f.tok_off_out[ctu] = base; f.tok_count_out[ctu] = (int32_t)n; }
  TC_STAMP(4);
#undef TC_STAMP
}

// =============================================================================================
// Input staging: packed I420 picture (w x h) -> coded planes padded to (cw x ch) by edge
// replication (what the oracle's load_input does)
// =============================================================================================
__global__ __launch_bounds__(256) void k_pad_input(const uint8_t *in, int w, int h, uint8_t *dy, uint8_t *du, uint8_t *dv, int cw, int ch)
{
  // A workgroup moves 1024 bytes x 16 rows: thread (x, q) the 16-byte piece x of rows 4q .. 4q + 3 -- four loads in flight, then four
  // stores.  blockIdx.y counts groups of 16 rows through luma, Cb, Cr (packed I420 input: Y, U, V planes back to back; the planes'
  // coded heights are multiples of 32, so a group never straddles two planes).
  int y0 = blockIdx.y * 16 + threadIdx.y * 4, plane = 0;
  if (y0 >= ch) { y0 -= ch; plane = 1; if (y0 >= ch / 2) { y0 -= ch / 2; plane = 2; } }
  const int pw = plane ? w / 2 : w, ph = plane ? h / 2 : h, pcw = plane ? cw / 2 : cw;
  const int x = (blockIdx.x * 64 + threadIdx.x) * 16;
  if (x >= pcw) return;
  const uint8_t *src = in + (plane == 0 ? 0 : (plane == 1 ? (size_t)w * h : (size_t)w * h + (size_t)(w / 2) * (h / 2)));
  uint8_t *dst = plane == 0 ? dy : (plane == 1 ? du : dv);
  kv_u32x4 v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint8_t *row = src + (size_t)imin(y0 + k, ph - 1) * pw;
    if (x + 16 <= pw && (((uintptr_t)(row + x)) & 3) == 0) v[k] = *reinterpret_cast<const kv_u32x4 *>(row + x);      // the common case: one 16-byte load
    else {                                                     // the picture's right edge (replicated) or an odd alignment: byte by byte
      uint32_t q[4] = {0, 0, 0, 0};
      for (int i = 0; i < 16; i++) q[i >> 2] |= (uint32_t)row[imin(x + i, pw - 1)] << (8 * (i & 3));
      v[k].x = q[0]; v[k].y = q[1]; v[k].z = q[2]; v[k].w = q[3];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) *reinterpret_cast<kv_u32x4 *>(dst + (size_t)(y0 + k) * pcw + x) = v[k];          // coded widths are multiples of 64: 16-byte aligned
}

// =============================================================================================
// Variance adaptive quantisation, "uvgx VAQ v1" (statement of record: vaq_deltas() in oracle/hevc_enc.c).
// k_vaq_stats: one workgroup per CTU -- sum and sum of squares of its 64x64 source luma samples, activity e = log2 of the
// variance in 1/16 steps, e to act[ctu] and into the picture's sum.  k_vaq_apply: the picture mean, the CTU's delta, and the
// target QP = clip(qp + clip(roi delta + vaq delta)) written over the ROI delta the host put into ctu_qt.
// =============================================================================================
__global__ __launch_bounds__(256) void k_vaq_stats(EncFrame f, int *act, int *sum)
{
  __shared__ uint32_t p1[4], p2[4];
  const int tid = threadIdx.x, wc = f.cw >> 6, cx = blockIdx.x % wc, cy = blockIdx.x / wc;
  const uint8_t *src = f.src[0] + (size_t)(cy * 64) * f.cw + cx * 64;
  uint32_t s1 = 0, s2 = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {                                     // 1024 dwords of the CTU, four per thread
    const int i = tid + 256 * k, y = i >> 4, x = (i & 15) * 4;
    const uint32_t v = *(const uint32_t *)&src[(size_t)y * f.cw + x];
#pragma unroll
    for (int b = 0; b < 4; b++) { const uint32_t px = (v >> (8 * b)) & 255u; s1 += px; s2 += px * px; }
  }
  s1 = wave_sum_u32(s1); s2 = wave_sum_u32(s2);
  if ((tid & 63) == 0) { p1[tid >> 6] = s1; p2[tid >> 6] = s2; }
  __syncthreads();
  if (tid == 0) {
    const uint32_t a = p1[0] + p1[1] + p1[2] + p1[3], b = p2[0] + p2[1] + p2[2] + p2[3];
    const uint64_t var = ((uint64_t)b * 4096 - (uint64_t)a * a) >> 24;
    const uint32_t v1 = (uint32_t)var + 1;
    const int l = 31 - __builtin_clz(v1), e = 16 * l + (int)(((v1 << 4) >> l) & 15);
    act[blockIdx.x] = e;
    atomicAdd(sum, e);
  }
}
__global__ __launch_bounds__(256) void k_vaq_apply(EncFrame f, int vaq, const int *act, const int *sum, int nctu)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nctu) return;
  const int mean = (int)(((long long)*sum + nctu / 2) / nctu);
  const int d = vaq * (act[i] - mean), delta = d >= 0 ? d / 48 : -((-d) / 48);
  int8_t *qt = const_cast<int8_t *>(f.ctu_qt);
  qt[i] = (int8_t)clip3(0, 51, f.qp + clip3(-12, 12, (int)qt[i] + delta));      // qt[i] holds the (clamped) ROI delta on entry
}

// =============================================================================================
// launch wrappers
// =============================================================================================
void launch_pad_input(const uint8_t *in, int w, int h, uint8_t *dy, uint8_t *du, uint8_t *dv, int cw, int ch, hipStream_t st)
{
  dim3 g((cw / 16 + 63) / 64, ch * 2 / 16);
  hipLaunchKernelGGL(k_pad_input, g, dim3(64, 4), 0, st, in, w, h, dy, du, dv, cw, ch);
}
void launch_luma_quarter(const uint8_t *src, uint8_t *q, int cw, int ch, hipStream_t st)
{
  hipLaunchKernelGGL(k_luma_quarter, dim3((cw / 16 + 63) / 64, (ch / 4 + 3) / 4), dim3(64, 4), 0, st, src, q, cw, ch);
}
void launch_me_coarse(const EncFrame &f, hipStream_t st)
{
  hipLaunchKernelGGL(k_me_coarse, dim3(f.cw / 32, f.ch / 32, f.nref > 1 ? f.nref : 1), dim3(256), 0, st, f);
}
void launch_me(const EncFrame &f, hipStream_t st)
{
  const int W = 2 * f.range + 1, items = ((W + 3) / 4) * ((W + 1) / 2);          // quads x pairs; R = 16: 153 items -> 192 threads
  const int threads = items >= 256 ? 256 : ((items + 63) / 64) * 64;
  if (f.mc_rq) {                                                                                                  // me-coarse: the form with the second window
    if (f.cu_ref) hipLaunchKernelGGL((k_me<true, true>), dim3(f.cw / 32, band_rows(f) * 2), dim3(threads), 0, st, f);
    else hipLaunchKernelGGL((k_me<false, true>), dim3(f.cw / 32, band_rows(f) * 2), dim3(threads), 0, st, f);
  }
  else if (f.cu_ref && f.fb_heal) hipLaunchKernelGGL((k_me<true, false, false, true>), dim3(f.cw / 32, band_rows(f) * 2), dim3(threads), 0, st, f);      // fb-anchor: a v2 heal picture (references: the previous picture and the anchor)
  else if (f.cu_ref) hipLaunchKernelGGL(k_me<true>, dim3(f.cw / 32, band_rows(f) * 2), dim3(threads), 0, st, f);     // lp-refs
  else if (f.fb_heal) hipLaunchKernelGGL((k_me<false, false, false, true>), dim3(f.cw / 32, band_rows(f) * 2), dim3(threads), 0, st, f);      // loss-feedback: a heal picture (one reference, no coarse stage)
  else if (f.ir_e) hipLaunchKernelGGL((k_me<false, false, true>), dim3(f.cw / 32, band_rows(f) * 2), dim3(threads), 0, st, f);     // intra-refresh (one reference, no coarse stage)
  else hipLaunchKernelGGL(k_me<false>, dim3(f.cw / 32, band_rows(f) * 2), dim3(threads), 0, st, f);
}
void launch_vaq(const EncFrame &f, int vaq, int *act, int *sum, hipStream_t st)
{
  const int nctu = (f.cw / 64) * (f.ch / 64);
  hipMemsetAsync(sum, 0, sizeof(int), st);
  hipLaunchKernelGGL(k_vaq_stats, dim3(nctu), dim3(256), 0, st, f, act, sum);
  hipLaunchKernelGGL(k_vaq_apply, dim3((nctu + 255) / 256), dim3(256), 0, st, f, vaq, (const int *)act, (const int *)sum, nctu);
}
void launch_tokenize(const EncFrame &f, hipStream_t st)
{
  // One wave per unit and colour component keeps the longest wave short: the kernel lasts as long as its slowest wave.  (One wave per unit that takes
  // the three components in turn was the faster form at 2160p while a wave that finds nothing to do cost what it did in round 1 -- 76 vs 137 us; with
  // today's early exit it is the slower one there as well: 66 vs 55 us per launch at 2160p, 51 vs 31 us at 1080p, a luma wave + a chroma wave per unit 60 /
  // 35 us -- and is kept for pictures beyond that, where nothing has been measured.)
  const int units = (f.cw / 16) * band_rows(f) * 4;
  // Measured (profiles/r06_tok_list_ab.txt, isolated): 2160p 49.1 against 56.9 us -- there the grid form is bound by the 130 000 waves it starts --, 1080p 27.4
  // against 24.1 us: there both forms last as long as their longest wave, and the list form's is the longer one (three waves per SIMD's worth of registers).
  // So: the list from 16 384 units on.  KVAZZUP_AMD_TOK_LIST=1 forces it everywhere (tests), =0 switches it off (A/B).
  static const int list_mode = [] { const char *e = getenv("KVAZZUP_AMD_TOK_LIST"); return e ? atoi(e) : -1; }();
  if (!f.is_intra && f.tok_list && f.nrows == 0 && units < 65536 && (list_mode > 0 || (list_mode < 0 && units > 16384))) {
    // the list form: as many waves as a picture of this size usually has pairs to say something about (half the units; a busier picture's waves take several)
    hipLaunchKernelGGL((k_tokenize<false, 1, true, true, true>), dim3(units / 2 < 256 ? 256 : units / 2), dim3(64), 0, st, f);
    return;
  }
  if (units >= 65536) hipLaunchKernelGGL((k_tokenize<true, 1>), dim3(f.cw / 16, band_rows(f) * 4), dim3(64), 0, st, f);
  else if (units > 16384) hipLaunchKernelGGL((k_tokenize<false, 1, false, false>), dim3(f.cw / 16, band_rows(f) * 4, 3), dim3(64), 0, st, f);     // (z: luma + headers, Cb, Cr)
  else hipLaunchKernelGGL((k_tokenize<false, 1, true>), dim3(f.cw / 16, band_rows(f) * 4, 4), dim3(64), 0, st, f);     // (z: luma, Cb, Cr, headers; tok_cursor is zero: the previous picture's k_tok_compact left it so)
}
void launch_tok_compact(const EncFrame &f, hipStream_t st)
{
  hipLaunchKernelGGL(k_tok_compact, dim3((f.cw / 64) * band_rows(f)), dim3(256), 0, st, f);
}

}  // namespace kvzx
