// The per-pixel pieces of the self-supervised loss that selfsup_loss.hip and selfsup_loss_weighted.hip share: the warp of the right
// image by the disparity (with the 0.9999 cover test), torch.abs' subgradient, and the edge-aware smoothness term with its gradient.
// One definition, so the weighted kernel's arithmetic per pixel is the plain kernel's.  DESIGN.md sections 4.5 and 4.5.1.
#pragma once
#include "common.h"

namespace ragmi {

// grid_sample(right, grid, bilinear, zeros, align_corners=False) at pixel (y, x) of grid = normalise(x - d, y) (loss.py:6-37), and
// the same sample of an all-ones image (the mask).  Index arithmetic in ATen's order and without contraction, so that the floor and
// the 0.9999 decision follow the reference's fp32 arithmetic.  est[c] = m * sample; dest[c] = d est[c] / d disp (m is piecewise
// constant: no gradient flows through it).  Returns m in {0, 1}.
template <int C>
__device__ __forceinline__ float warp_px(const float* __restrict__ rb, int64_t hw, int H, int W, int y, int x, float d,
                                         float (&est)[C], float (&dest)[C], float dxs_dd) {
#pragma clang fp contract(off)
  const float gx = 2.0f * ((float)x - d) / (float)(W - 1) - 1.0f;       // vgrid = grid - flow, scaled to [-1, 1] (align_corners=True)
  const float gy = 2.0f * (float)y / (float)(H - 1) - 1.0f;
  const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;                 // grid_sample's unnormalise, align_corners=False
  const float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  // taps are selected on the clamped integer corner (a NaN or huge disparity selects none); weights use the unclamped floor
  const int x0 = (int)fminf(fmaxf(fx, -2.f), (float)W + 1.f), y0 = (int)fminf(fmaxf(fy, -2.f), (float)H + 1.f);
  const float w_nw = (fx + 1.f - ix) * (fy + 1.f - iy);
  const float w_ne = (ix - fx) * (fy + 1.f - iy);
  const float w_sw = (fx + 1.f - ix) * (iy - fy);
  const float w_se = (ix - fx) * (iy - fy);
  const bool xin0 = x0 >= 0 && x0 < W, xin1 = x0 + 1 >= 0 && x0 + 1 < W;
  const bool yin0 = y0 >= 0 && y0 < H, yin1 = y0 + 1 >= 0 && y0 + 1 < H;
  const bool t_nw = yin0 && xin0, t_ne = yin0 && xin1, t_sw = yin1 && xin0, t_se = yin1 && xin1;
  float m = 0.f;
  if (t_nw) m += w_nw;
  if (t_ne) m += w_ne;
  if (t_sw) m += w_sw;
  if (t_se) m += w_se;
  m = m >= 0.9999f ? 1.f : 0.f;                                         // loss.py:34-35
  const int64_t o = (int64_t)y0 * W + x0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* p = rb + (int64_t)c * hw;
    const float v_nw = t_nw ? p[o] : 0.f, v_ne = t_ne ? p[o + 1] : 0.f;
    const float v_sw = t_sw ? p[o + W] : 0.f, v_se = t_se ? p[o + W + 1] : 0.f;
    float s = 0.f;
    if (t_nw) s += v_nw * w_nw;
    if (t_ne) s += v_ne * w_ne;
    if (t_sw) s += v_sw * w_sw;
    if (t_se) s += v_se * w_se;
    est[c] = s * m;
    // d sample / d ix (grid_sampler_2d_backward's gix, before its W/2 factor, which dxs_dd holds with d gx / d disp)
    const float g = (v_ne - v_nw) * (fy + 1.f - iy) + (v_se - v_sw) * (iy - fy);
    dest[c] = m * g * dxs_dd;
  }
  return m;
}

__device__ __forceinline__ float sgnf(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }   // torch.abs' subgradient: sign(0) = 0

// exp(-|mean_c(left[c, i] - left[c, j])|): the smoothness weight between neighbours i and j (loss.py:127-131)
template <int C>
__device__ __forceinline__ float edge_weight(const float* __restrict__ lb, int64_t hw, int64_t i, int64_t j) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) s += lb[c * hw + i] - lb[c * hw + j];
  return expf(-fabsf(s / (float)C));
}

// the pixel's smoothness term (edges to x+1 and y+1) and, with GRAD, d smooth_sum / d disp at the pixel (all four edges)
template <int C, bool GRAD>
__device__ __forceinline__ float smooth_px(const float* __restrict__ lb, const float* __restrict__ db, int64_t hw, int H, int W, int y,
                                           int x, float d, float& gsum) {
#pragma clang fp contract(off)                                          // the same rounding with and without GRAD, as the SSIM term
  const int64_t i = (int64_t)y * W + x;
  float f = 0.f;
  if (x < W - 1) {
    const float w = edge_weight<C>(lb, hw, i, i + 1), e = d - db[i + 1];
    f += fabsf(e) * w;
    if (GRAD) gsum += sgnf(e) * w;
  }
  if (y < H - 1) {
    const float w = edge_weight<C>(lb, hw, i, i + W), e = d - db[i + W];
    f += fabsf(e) * w;
    if (GRAD) gsum += sgnf(e) * w;
  }
  if (GRAD && x > 0) gsum -= sgnf(db[i - 1] - d) * edge_weight<C>(lb, hw, i - 1, i);
  if (GRAD && y > 0) gsum -= sgnf(db[i - W] - d) * edge_weight<C>(lb, hw, i - W, i);
  return f;
}

}  // namespace ragmi
