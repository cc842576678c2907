// kvazzup_amd/csrc/conceal_kernels.hip -- concealment v3, step 3 (decoder.h "Concealment v3"): the stand-in for a reference picture
// that never arrived is its source picture S moved block by block along S's own motion, whole samples, clipped to the coded plane.  The host has turned S's
// motion into one row of the table per 16x16 luma block -- luma dx, dy, chroma dx, dy (Decoder::conceal_displacements) --; this kernel only fetches:
//   luma   (x, y)   of block B = S's luma   at (clip(x + dx),   clip(y + dy))
//   chroma (xc, yc) of B's 8x8 = S's chroma at (clip(xc + dxc), clip(yc + dyc))
// One launch for the three planes.  A lane owns one ROW PIECE of one block: 16 luma samples, or 8 samples of Cb or Cr -- 16 + 8 + 8 = 32 lanes a block,
// neighbouring lanes the same row of neighbouring blocks.  A piece that lies inside the plane where it is read and where it is written moves as ONE load of 16 (8) bytes at whatever address the
// displacement gives -- global loads need no alignment on gfx950 -- and one aligned store; a piece that touches an edge goes byte by byte through the clamp.
// Pure streaming, 1.5 w h bytes read and written; no LDS, no scratch, nothing waits for another workgroup.  It runs once per lost picture, behind a drained
// device (Decoder::fill_concealed): nothing here is on the decoder's hot path.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dec_kernels.h"

namespace kvzx {

struct StandinPlanes { uint8_t *dst[3]; const uint8_t *src[3]; };

__device__ __forceinline__ int sd_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// (w, h): the coded picture; pitch: the luma planes' row length (chroma: half of it); w16 x h16 blocks; tab: four displacements per block
__global__ __launch_bounds__(256) void k_dec_standin(StandinPlanes pl, const short4 *__restrict__ tab, int w, int h, int pitch, int w16, int h16)
{
  // lanes run along a row of the picture: w16 consecutive lanes hold the same row piece (r) of the w16 blocks of a block row -- their stores are one run of
  // memory, their loads nearly so, and luma / chroma change only every w16 lanes
  const int t = blockIdx.x * 256 + threadIdx.x, bx = t % w16, q = t / w16, r = q & 31, by = q >> 5;
  if (by >= h16) return;
  const int b = by * w16 + bx;
  const short4 d = tab[b];
  const bool luma = r < 16;
  const int c = luma ? 0 : 1 + ((r - 16) >> 3);                         // the lane's plane
  const int n = luma ? 16 : 8;                                          // samples of a full piece
  const int W = luma ? w : w >> 1, H = luma ? h : h >> 1, P = luma ? pitch : pitch >> 1;
  const int x0 = bx * n, y = by * n + (luma ? r : (r & 7));
  if (y >= H) return;                                                   // (the last block row may be partial)
  const int sx = x0 + (luma ? d.x : d.z), sy = sd_clamp(y + (luma ? d.y : d.w), H - 1);
  const uint8_t *s = pl.src[c] + (size_t)sy * P;
  uint8_t *o = pl.dst[c] + (size_t)y * P + x0;
  if (x0 + n <= W && sx >= 0 && sx + n <= W) {                          // the piece inside the plane on both sides: one load, one store
    if (luma) { uint4 v; __builtin_memcpy(&v, s + sx, 16); *(uint4 *)o = v; }      // (o: x0 a multiple of 16, the pitch of 64, the plane 256-byte aligned)
    else { uint2 v; __builtin_memcpy(&v, s + sx, 8); *(uint2 *)o = v; }
    return;
  }
  const int m = W - x0 < n ? W - x0 : n;                                // (the last block column may be partial)
  for (int i = 0; i < m; i++) o[i] = s[sd_clamp(sx + i, W - 1)];
}

void launch_dec_standin(uint8_t *const dst[3], uint8_t *const src[3], const int16_t *d_tab, int w, int h, int pitch, hipStream_t st)
{
  StandinPlanes pl;
  for (int c = 0; c < 3; c++) { pl.dst[c] = dst[c]; pl.src[c] = src[c]; }
  const int w16 = (w + 15) / 16, h16 = (h + 15) / 16;
  const unsigned lanes = (unsigned)w16 * h16 * 32;
  hipLaunchKernelGGL(k_dec_standin, dim3((lanes + 255) / 256), dim3(256), 0, st, pl, (const short4 *)d_tab, w, h, pitch, w16, h16);
}

// ---- partial pictures v1 (decoder.h "Partial pictures"): k_dec_standin's work restricted to the coding tree blocks of a picture whose
// slice segments never arrived.  ctbs: their raster addresses (pitch cwc), n of them -- the grid is sized by what is missing, not by the picture.  A CTB of
// 16 << lg samples a side is (1 << lg)^2 blocks of 16x16, a block 32 row pieces as above; inside a CTB the lanes run along its rows (piece r of the 1 << lg
// blocks of a block row side by side).  tab: the table of the WHOLE block grid (pitch w16), NULL = no displacement (concealment mode 2); src[0] NULL = no
// source, mid-grey.  Same two forms of a piece, same clamp; no LDS, no scratch, nothing waits.
__global__ __launch_bounds__(256) void k_dec_fill_ctbs(StandinPlanes pl, const short4 *__restrict__ tab, const uint32_t *__restrict__ ctbs, int n, int lg, int cwc,
                                                       int w, int h, int pitch, int w16)
{
  const unsigned t = blockIdx.x * 256u + threadIdx.x, per_ctb = 32u << (2 * lg), m = t / per_ctb;
  if (m >= (unsigned)n) return;
  const unsigned q = t - m * per_ctb, ctb = ctbs[m];
  const int lbx = (int)(q & ((1u << lg) - 1)), r = (int)(q >> lg) & 31, lby = (int)(q >> (lg + 5));
  const int bx = (int)(ctb % (unsigned)cwc) * (1 << lg) + lbx, by = (int)(ctb / (unsigned)cwc) * (1 << lg) + lby;
  const bool luma = r < 16;
  const int c = luma ? 0 : 1 + ((r - 16) >> 3);
  const int n_ = luma ? 16 : 8;
  const int W = luma ? w : w >> 1, H = luma ? h : h >> 1, P = luma ? pitch : pitch >> 1;
  const int x0 = bx * n_, y = by * n_ + (luma ? r : (r & 7));
  if (x0 >= W || y >= H) return;                                        // (the last CTB column and row may be partial: blocks beyond the coded picture)
  uint8_t *o = pl.dst[c] + (size_t)y * P + x0;
  const int m_ = W - x0 < n_ ? W - x0 : n_;
  if (!pl.src[0]) { for (int i = 0; i < m_; i++) o[i] = 128; return; }
  short4 d = make_short4(0, 0, 0, 0);
  if (tab) d = tab[by * w16 + bx];
  const int sx = x0 + (luma ? d.x : d.z), sy = sd_clamp(y + (luma ? d.y : d.w), H - 1);
  const uint8_t *s = pl.src[c] + (size_t)sy * P;
  if (x0 + n_ <= W && sx >= 0 && sx + n_ <= W) {
    if (luma) { uint4 v; __builtin_memcpy(&v, s + sx, 16); *(uint4 *)o = v; }
    else { uint2 v; __builtin_memcpy(&v, s + sx, 8); *(uint2 *)o = v; }
    return;
  }
  for (int i = 0; i < m_; i++) o[i] = s[sd_clamp(sx + i, W - 1)];
}

// src NULL: grey.  d_ctbs / d_tab: device memory (Decoder::fill_missing puts them up beside the stand-in's table); dst: the picture's buffer, behind its last kernel
void launch_dec_fill_ctbs(uint8_t *const dst[3], uint8_t *const *src, const int16_t *d_tab, const uint32_t *d_ctbs, int n, int ctb_log2, int w, int h, int pitch, hipStream_t st)
{
  if (n < 1) return;
  StandinPlanes pl;
  for (int c = 0; c < 3; c++) { pl.dst[c] = dst[c]; pl.src[c] = src ? src[c] : nullptr; }
  const int lg = ctb_log2 - 4, cwc = (w + (1 << ctb_log2) - 1) >> ctb_log2;
  const unsigned lanes = (unsigned)n * (32u << (2 * lg));
  hipLaunchKernelGGL(k_dec_fill_ctbs, dim3((lanes + 255) / 256), dim3(256), 0, st, pl, (const short4 *)d_tab, d_ctbs, n, lg, cwc, w, h, pitch, (w + 15) / 16);
}

}  // namespace kvzx
