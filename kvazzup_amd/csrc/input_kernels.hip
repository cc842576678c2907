// kvazzup_amd/csrc/input_kernels.hip -- the encoder's input stage for pictures that are not I420 ("input-format"): a packed RGB32 or
// YUYV picture (w x h) in a ring slot -> the three coded planes of a working set (cw x ch, multiples of 64), converted and padded by edge replication in one
// pass.  What comes out is k_pad_input(convert(picture)) sample for sample, convert being
//   rgb32        rgb_to_yuv420_i_c      (the reference's src/media/processing/yuvconversions.cpp:770-797; color_kernels.hip k_rgb32_to_i420<false>)
//   rgb32-sse41  rgb_to_yuv420_i_sse41  (:634-767; k_rgb32_to_i420<true>: the picture comes out upside down)
//   yuyv         yuyv_to_yuv420_c       (:800-834: luma copied, a chroma sample the truncating mean of the two rows' samples)
// Padding replicates OUTPUT samples: a luma sample beyond the picture takes the nearest luma sample inside, a chroma sample the nearest chroma sample inside.
// So a lane clamps its output coordinates per plane and converts from the pixels those samples are made of; with the flipped variant the flip comes first
// (converted row y is made of source row h - 1 - y), then the padding.  Widths and heights are even (rgb32: width % 4 == 0), so a lane's 2 x 2 pixel blocks lie
// wholly inside or wholly outside the picture.
// Pure streaming, HBM bound: 4 w h (RGB32) or 2 w h (YUYV) bytes read, 1.5 cw ch written; no LDS, no scratch, nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "input_kernels.h"

namespace kvzx {

__device__ __forceinline__ int in_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// A lane owns 4 x 2 output luma samples and 2 chroma samples per plane: two 16-byte loads, two 4-byte luma stores, one 2-byte store per chroma plane.
// Lanes of the padding region load the picture's last pixel group / row pair and replicate from it.
template <bool SSE>
__global__ __launch_bounds__(256) void k_input_rgb32(const uint8_t *in, int w, int h, uint8_t *dy, uint8_t *du, uint8_t *dv, int cw, int ch)
{
  const int tx = blockIdx.x * blockDim.x + threadIdx.x, ty = blockIdx.y;
  if (tx * 4 >= cw || ty * 2 >= ch) return;
  const bool right = tx * 4 >= w, below = ty * 2 >= h;             // the lane lies in the padding
  const int sx = right ? w - 4 : tx * 4;                           // its pixel group
  const int p = below ? h / 2 - 1 : ty;                            // its row pair in the CONVERTED picture ...
  const int sp = SSE ? h / 2 - 1 - p : p;                          // ... and in the source picture
  const uint4 p0 = *(const uint4 *)(in + ((size_t)(2 * sp) * w + sx) * 4), p1 = *(const uint4 *)(in + ((size_t)(2 * sp + 1) * w + sx) * 4);
  const uint32_t px[2][4] = {{p0.x, p0.y, p0.z, p0.w}, {p1.x, p1.y, p1.z, p1.w}};
  int us[4], vs[4]; uint32_t y4[2];
#pragma unroll
  for (int i = 0; i < 4; i++) { us[i] = 0; vs[i] = 0; }
#pragma unroll
  for (int r = 0; r < 2; r++) {
    y4[r] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int b0 = px[r][i] & 255, b1 = (px[r][i] >> 8) & 255, b2 = (px[r][i] >> 16) & 255;
      if (SSE) {
        y4[r] |= (uint32_t)in_clamp255((76 * b2 + 150 * b1 + 29 * b0) >> 8) << (8 * i);
        us[i] += -43 * b2 - 84 * b1 + 127 * b0; vs[i] += 127 * b2 - 106 * b1 - 21 * b0;
      } else {
        y4[r] |= (uint32_t)(((76 * b0 + 150 * b1 + 29 * b2 + 128) >> 8) & 255) << (8 * i);
        us[i] += 127 * b0 - 84 * b1 - 43 * b2; vs[i] += -21 * b0 - 106 * b1 + 127 * b2;
      }
    }
    if (right) y4[r] = (y4[r] >> 24) * 0x01010101u;                // the picture's last column
  }
  int u0, u1, v0, v1;
  if (SSE) {
    int t[4], q[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { t[i] = in_clamp255((us[i] + 255 * 255) >> 9); q[i] = in_clamp255((vs[i] + 255 * 255) >> 9); }
    u0 = (t[0] + t[1]) >> 1; u1 = (t[2] + t[3]) >> 1; v0 = (q[0] + q[1]) >> 1; v1 = (q[2] + q[3]) >> 1;
  } else {
    u0 = ((us[0] + us[1] + 512) >> 10) + 128; u1 = ((us[2] + us[3] + 512) >> 10) + 128;
    v0 = ((vs[0] + vs[1] + 512) >> 10) + 128; v1 = ((vs[2] + vs[3] + 512) >> 10) + 128;
  }
  if (right) { u0 = u1; v0 = v1; }                                 // the picture's last chroma column
  // converted row 2p + r is made of source row 2sp + r (2sp + 1 - r when flipped); below the picture both output rows are converted row h - 1
  const int last = SSE ? 0 : 1;
  const uint32_t o0 = below ? y4[last] : y4[SSE ? 1 : 0], o1 = below ? y4[last] : y4[SSE ? 0 : 1];
  *(uint32_t *)(dy + (size_t)(2 * ty) * cw + tx * 4) = o0;
  *(uint32_t *)(dy + (size_t)(2 * ty + 1) * cw + tx * 4) = o1;
  *(uint16_t *)(du + (size_t)ty * (cw / 2) + tx * 2) = (uint16_t)((u0 & 255) | ((u1 & 255) << 8));
  *(uint16_t *)(dv + (size_t)ty * (cw / 2) + tx * 2) = (uint16_t)((v0 & 255) | ((v1 & 255) << 8));
}

// A lane owns 8 x 2 output luma samples and 4 chroma samples per plane: two 16-byte loads (Y0 U Y1 V ...), two 8-byte luma stores, one 4-byte store per chroma
// plane.  A lane that straddles the picture's right edge (width % 8 != 0), lies beyond it, or finds its rows at an odd alignment reads byte by byte from
// clamped coordinates.
__global__ __launch_bounds__(256) void k_input_yuyv(const uint8_t *in, int w, int h, uint8_t *dy, uint8_t *du, uint8_t *dv, int cw, int ch)
{
  const int tx = blockIdx.x * blockDim.x + threadIdx.x, ty = blockIdx.y;
  if (tx * 8 >= cw || ty * 2 >= ch) return;
  const bool below = ty * 2 >= h;
  const int p = below ? h / 2 - 1 : ty, ox = tx * 8;
  uint32_t ylo[2], yhi[2]; int us[4] = {0, 0, 0, 0}, vs[4] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const uint8_t *row = in + (size_t)(2 * p + r) * w * 2;
    uint32_t q[4];
    if (ox + 8 <= w && (((uintptr_t)(row + ox * 2)) & 15) == 0) {
      const uint4 v = *(const uint4 *)(row + ox * 2);
      q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int x0 = min(ox + 2 * c, w - 1), x1 = min(ox + 2 * c + 1, w - 1), cx = min(ox / 2 + c, w / 2 - 1);
        q[c] = (uint32_t)row[x0 * 2] | ((uint32_t)row[cx * 4 + 1] << 8) | ((uint32_t)row[x1 * 2] << 16) | ((uint32_t)row[cx * 4 + 3] << 24);
      }
    }
    ylo[r] = (q[0] & 255) | ((q[0] >> 8) & 0xFF00) | ((q[1] & 255) << 16) | ((q[1] << 8) & 0xFF000000u);
    yhi[r] = (q[2] & 255) | ((q[2] >> 8) & 0xFF00) | ((q[3] & 255) << 16) | ((q[3] << 8) & 0xFF000000u);
#pragma unroll
    for (int c = 0; c < 4; c++) { us[c] += (q[c] >> 8) & 255; vs[c] += q[c] >> 24; }
  }
  uint32_t u4 = 0, v4 = 0;
#pragma unroll
  for (int c = 0; c < 4; c++) { u4 |= (uint32_t)(us[c] >> 1) << (8 * c); v4 |= (uint32_t)(vs[c] >> 1) << (8 * c); }
  const int r0 = below ? 1 : 0;                                    // below the picture both output rows are its last row
  *(uint2 *)(dy + (size_t)(2 * ty) * cw + ox) = make_uint2(ylo[r0], yhi[r0]);
  *(uint2 *)(dy + (size_t)(2 * ty + 1) * cw + ox) = make_uint2(ylo[1], yhi[1]);
  *(uint32_t *)(du + (size_t)ty * (cw / 2) + tx * 4) = u4;
  *(uint32_t *)(dv + (size_t)ty * (cw / 2) + tx * 4) = v4;
}

size_t input_bytes(int format, int w, int h)
{
  const size_t n = (size_t)w * h;
  return format == KVZ_INPUT_I420 ? n * 3 / 2 : (format == KVZ_INPUT_YUYV ? n * 2 : n * 4);
}

// format: KVZ_INPUT_RGB32 / _RGB32_SSE41 (width % 4 == 0, `in` 16-byte aligned) or KVZ_INPUT_YUYV; w, h even; cw, ch multiples of 64 not below w, h
bool launch_input_packed(int format, const uint8_t *in, int w, int h, uint8_t *dy, uint8_t *du, uint8_t *dv, int cw, int ch, hipStream_t st)
{
  if (!in || w < 4 || h < 2 || (w & 1) || (h & 1) || cw < w || ch < h || (cw & 63) || (ch & 63)) return false;
  if (format == KVZ_INPUT_YUYV) {
    hipLaunchKernelGGL(k_input_yuyv, dim3((cw / 8 + 255) / 256, ch / 2), dim3(256), 0, st, in, w, h, dy, du, dv, cw, ch);
    return true;
  }
  if ((w & 3) || (((uintptr_t)in) & 15)) return false;
  const dim3 g((cw / 4 + 255) / 256, ch / 2);
  if (format == KVZ_INPUT_RGB32_SSE41) hipLaunchKernelGGL(k_input_rgb32<true>, g, dim3(256), 0, st, in, w, h, dy, du, dv, cw, ch);
  else if (format == KVZ_INPUT_RGB32) hipLaunchKernelGGL(k_input_rgb32<false>, g, dim3(256), 0, st, in, w, h, dy, du, dv, cw, ch);
  else return false;
  return true;
}

}  // namespace kvzx
