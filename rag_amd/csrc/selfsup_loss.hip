// Self-supervised training loss of the continual-adaptation mode (src_self/approaches/rag.py:266-278 with supervise=False):
// re_and_sm_loss (src_self/models/loss.py:112-141) = 0.85 SSIM_mean + 0.15 L1_mean of the right image warped by the disparity,
// plus 0.1 x an edge-aware smoothness term, and its gradient with respect to the disparity.  The reference builds it from two
// grid_samples, five avg_pool2d and a few dozen element-wise ATen ops (and their backward), and its warp() makes host tensors and
// copies them to the device at every call.  Here one thread owns one non-overlapping 3x3 SSIM block (avg_pool2d(kernel_size=3)
// strides by 3) for all channels and computes, in the same pass, its share of the three sums and the gradient of the total at its
// own pixels; a second one-workgroup kernel folds the per-workgroup partials, in the fixed order of reduce.h and without host
// synchronisation.  DESIGN.md section 4.5.
//
// The same kernel body, WEIGHTED, takes a per-pixel weight w [B, H, W] on the photometric terms (the left-right consistency weight
// of lr_check.hip; the reference's mean_l1(x, y, mask), src_self/models/loss.py:66-76, takes such a mask that its caller never
// supplies):
//   L1     = sum_{b,c,y,x} w |left - left_est| / (C sum w)
//   SSIM   = sum_{blocks,c} wb term / (C sum wb),   wb = avg_pool2d(w, 3): the mean of w over the block, term as in the plain form
//   smooth   unchanged and unweighted (it is what fills the occluded band)
//   total  = 0.85 SSIM + 0.15 L1 + 0.1 smooth,     and d total / d disp; w is a constant (no gradient flows to it).
// A term whose weights sum to 0 is 0 and so is its gradient (the reference form would give NaN, which a captured step would write into
// the weights).  The gradient needs 1 / sum w and 1 / sum wb at every pixel, so a fixed-order pre-pass (grid-stride partials in
// double, one-workgroup fold: reduce.h) leaves the two sums as two doubles on the device and the main kernel reads them: four
// launches, no host synchronisation, no atomics, no memset.  Both forms are one definition that parts only where w enters (the plain
// form never multiplies by a constant 1), so w = 1 gives the plain form's numbers.  DESIGN.md section 4.5.1.
#include "reduce.h"

namespace ragmi {

constexpr int SS_WG = 64;        // threads per workgroup of the main pass: one wave (B*(H/3)*(W/3) threads spread over many CUs)
constexpr int SS_FIN = 256;      // threads of the pre-pass workgroups and of both one-workgroup folds
constexpr int SS_PART = 3;       // partials per main slot (double): sum (wb) SSIM terms, sum (w) |left - left_est|, sum smoothness
constexpr int SS_PRE = 2;        // partials per pre-pass slot (double): sum w, sum w inside the 3x3 blocks
constexpr int SS_PRE_MAX = 256;  // at most this many pre-pass workgroups

struct SelfSupArgs {
  const float* left;     // [B, C, H, W]
  const float* right;    // [B, C, H, W]
  const float* disp;     // [B, H, W]
  float* unit_grad;      // [B, H, W] d total / d disp, or null
  int H, W, Hb, Wb;      // Hb, Wb: 3x3 SSIM blocks per column / row
  int64_t nthreads;      // B * Hb * Wb
  float dxs_dd;          // d xs / d disp = -W / (W - 1)
  float k_l1;            // plain: 0.15 / (B C H W)
  float k_ssim;          // plain: 0.85 / (B C Hb Wb)
  float k_sm;            // 0.1 / (B H W)
  // the weighted form's members, behind the plain form's
  const float* weight;   // [B, H, W]
  const double* wsum;    // [2] sum w, sum wb (written by the pre-pass)
  double c_l1;           // 0.15 / C: k_l1 = c_l1 / sum w
  double c_ssim;         // 0.85 / C: k_ssim = c_ssim / sum wb
};

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

// slots[s] = (sum w, sum of the w that lie inside a 3x3 block) over the pixels i = first, first + stride, ... of workgroup s.  I: the
// type of the pixel index (32-bit divisions where B H W allows them)
template <class I>
__global__ __launch_bounds__(SS_FIN) void selfsup_weight_sums_kernel(const float* __restrict__ weight, int64_t n, int H, int W, int Hb,
                                                                     int Wb, double* __restrict__ slots) {
  double v[SS_PRE] = {0.0, 0.0};
  const I stride = (I)gridDim.x * SS_FIN;
  for (I i = (I)blockIdx.x * SS_FIN + threadIdx.x; i < (I)n; i += stride) {
    const I row = i / (I)W;                                  // b * H + y
    const int x = (int)(i - row * (I)W), y = (int)(row % (I)H);
    const double w = weight[i];
    v[0] += w;
    if (y < 3 * Hb && x < 3 * Wb) v[1] += w;
  }
  const auto sum = block_tree_sum<SS_FIN>(v);
  if (threadIdx.x < SS_PRE) slots[(int64_t)blockIdx.x * SS_PRE + threadIdx.x] = sum[threadIdx.x];
}

// wsum[0] = sum w, wsum[1] = sum wb = (sum of w inside the blocks) / 9
__global__ __launch_bounds__(SS_FIN) void selfsup_weight_sums_finalize_kernel(const double* __restrict__ slots, int nslots,
                                                                              double* __restrict__ wsum) {
  double v[SS_PRE];
  gather_slots<SS_FIN>(slots, nslots, v);
  const auto sum = block_tree_sum<SS_FIN>(v);
  if (threadIdx.x == 0) {
    wsum[0] = sum[0];
    wsum[1] = sum[1] / 9.0;
  }
}

__device__ __forceinline__ double inv_or_zero(double s) { return s > 0.0 ? 1.0 / s : 0.0; }

// WEIGHTED parts from the plain form in seven places, each under `if constexpr`: the load of w, wb, the factors on the L1 and SSIM
// sums, kc, the L1 subgradient, and where k_l1 / k_ssim come from.  Everything else is one text for both.
template <int C, bool GRAD, bool WEIGHTED>
__global__ __launch_bounds__(SS_WG) void selfsup_loss_kernel(SelfSupArgs a, double* __restrict__ slots) {
  const int64_t t = (int64_t)blockIdx.x * SS_WG + threadIdx.x;
  float acc_ssim = 0.f, acc_l1 = 0.f, acc_sm = 0.f;
  if (t < a.nthreads) {
    const int H = a.H, W = a.W;
    const int64_t nblk = (int64_t)a.Hb * a.Wb, hw = (int64_t)H * W;
    const int64_t b = t / nblk;
    const int r = (int)(t - b * nblk), by = r / a.Wb, bx = r - by * a.Wb;
    const float* lb = a.left + b * C * hw;
    const float* rb = a.right + b * C * hw;
    const float* db = a.disp + b * hw;
    [[maybe_unused]] const float* wp = nullptr;
    if constexpr (WEIGHTED) wp = a.weight + b * hw;
    float* gb = GRAD ? a.unit_grad + b * hw : nullptr;
    float k_l1, k_ssim;
    if constexpr (WEIGHTED) {
      k_l1 = GRAD ? (float)(a.c_l1 * inv_or_zero(a.wsum[0])) : 0.f;
      k_ssim = GRAD ? (float)(a.c_ssim * inv_or_zero(a.wsum[1])) : 0.f;
    } else {
      k_l1 = a.k_l1;
      k_ssim = a.k_ssim;
    }
    const int y0 = 3 * by, x0 = 3 * bx;
    const int y1 = by == a.Hb - 1 ? H : y0 + 3, x1 = bx == a.Wb - 1 ? W : x0 + 3;   // the last block row / column owns the remainder

    // ---- the 3x3 SSIM block: x = left, y = left_est (loss.py:77-97)
    float lv[9][C], ev[9][C], dv[9][C], gs[9];
    [[maybe_unused]] float wv[WEIGHTED ? 9 : 1], wb;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int y = y0 + k / 3, x = x0 + k % 3;
      const int64_t i = (int64_t)y * W + x;
      const float d = db[i];
      if constexpr (WEIGHTED) wv[k] = wp[i];
      warp_px<C>(rb, hw, H, W, y, x, d, ev[k], dv[k], a.dxs_dd);
      float gsm = 0.f;
      acc_sm += smooth_px<C, GRAD>(lb, db, hw, H, W, y, x, d, gsm);
      gs[k] = gsm * a.k_sm;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        lv[k][c] = lb[c * hw + i];
        if constexpr (WEIGHTED) acc_l1 += wv[k] * fabsf(lv[k][c] - ev[k][c]);
        else acc_l1 += fabsf(lv[k][c] - ev[k][c]);
      }
    }
    if constexpr (WEIGHTED) {
#pragma clang fp contract(off)
      float sw = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) sw += wv[k];
      wb = sw / 9.f;                                                     // avg_pool2d(w, 3) at this block
    }
    constexpr float C1 = 1e-4f, C2 = 9e-4f;                              // 0.01**2, 0.03**2 (loss.py:84-85)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float mx, my, A, Bn, Cd, D, S, h;
      {
        // The term's value, without contraction: which products the compiler fuses into a following sum depends on what else uses
        // them, so the GRAD and the terms-only instantiation would otherwise round the same block differently (seen as one ulp of
        // the SSIM mean).  Unfused is also the reference's arithmetic: avg_pool2d, products and sums are separate ATen kernels.
#pragma clang fp contract(off)
        float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float x = lv[k][c], y = ev[k][c];
          sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
        }
        mx = sx / 9.f; my = sy / 9.f;
        const float vx = sxx / 9.f - mx * mx, vy = syy / 9.f - my * my, vxy = sxy / 9.f - mx * my;
        A = 2.f * mx * my + C1; Bn = 2.f * vxy + C2; Cd = mx * mx + my * my + C1; D = vx + vy + C2;
        S = (A * Bn) / (Cd * D);
        h = (1.f - S) / 2.f;
        if constexpr (WEIGHTED) acc_ssim += wb * fminf(fmaxf(h, 0.f), 1.f);      // the weighted product stays unfused too
      }
      if constexpr (!WEIGHTED) acc_ssim += fminf(fmaxf(h, 0.f), 1.f);
      if (GRAD) {
        // d term / d y_i = -1/2 dS/dy_i (clamp passes the gradient on the closed interval), with
        // dS/dy_i = 2/(9 Cd D) * (mx Bn + A (x_i - mx) - S (my D + Cd (y_i - my)));
        // WEIGHTED: d (wb term) / d y_i = -wb/2 dS/dy_i, and the L1 part carries the pixel's own w
        float kc;
        if constexpr (WEIGHTED) kc = (h >= 0.f && h <= 1.f) ? -(k_ssim * wb) / (9.f * Cd * D) : 0.f;
        else kc = (h >= 0.f && h <= 1.f) ? -k_ssim / (9.f * Cd * D) : 0.f;
        const float base = mx * Bn - S * my * D, SCd = S * Cd;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float dS = base + A * (lv[k][c] - mx) - SCd * (ev[k][c] - my);
          float ge;                                                          // d total / d left_est[c] at pixel k
          if constexpr (WEIGHTED) ge = kc * dS - (k_l1 * wv[k]) * sgnf(lv[k][c] - ev[k][c]);
          else ge = kc * dS - k_l1 * sgnf(lv[k][c] - ev[k][c]);
          gs[k] += ge * dv[k][c];
        }
      }
    }
    if (GRAD) {
#pragma unroll
      for (int k = 0; k < 9; ++k) gb[(int64_t)(y0 + k / 3) * W + x0 + k % 3] = gs[k];
    }

    // ---- remainder rows / columns of the last block row / column: L1 and smoothness only (outside avg_pool2d's windows)
    for (int y = y0; y < y1; ++y) {
      for (int x = (y < y0 + 3 ? x0 + 3 : x0); x < x1; ++x) {
        const int64_t i = (int64_t)y * W + x;
        const float d = db[i];
        [[maybe_unused]] float w;
        if constexpr (WEIGHTED) w = wp[i];
        float e[C], de[C];
        warp_px<C>(rb, hw, H, W, y, x, d, e, de, a.dxs_dd);
        float gsm = 0.f;
        acc_sm += smooth_px<C, GRAD>(lb, db, hw, H, W, y, x, d, gsm);
        float g = gsm * a.k_sm;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float l = lb[c * hw + i];
          if constexpr (WEIGHTED) {
            acc_l1 += w * fabsf(l - e[c]);
            if (GRAD) g -= (k_l1 * w) * sgnf(l - e[c]) * de[c];
          } else {
            acc_l1 += fabsf(l - e[c]);
            if (GRAD) g -= k_l1 * sgnf(l - e[c]) * de[c];
          }
        }
        if (GRAD) gb[i] = g;
      }
    }
  }
  // ---- per-workgroup partials in double, one slot per workgroup
  const double v[SS_PART] = {acc_ssim, acc_l1, acc_sm};
  const auto sum = block_tree_sum<SS_WG>(v);
  if (threadIdx.x < SS_PART) slots[(int64_t)blockIdx.x * SS_PART + threadIdx.x] = sum[threadIdx.x];
}

// out[0..3] = total, SSIM_mean, L1_mean, smoothness_mean (total = 0.85 SSIM + 0.15 L1 + 0.1 smoothness): the slots in a fixed order.
// Plain: the photometric sums times inv_ssim / inv_l1.  WEIGHTED: times inv_ssim = inv_l1 = 1 / C and 1 / wsum[1], 1 / wsum[0].
template <bool WEIGHTED>
__global__ __launch_bounds__(SS_FIN) void selfsup_loss_finalize_kernel(const double* __restrict__ slots, int64_t nslots,
                                                                       const double* __restrict__ wsum, double inv_ssim, double inv_l1,
                                                                       double inv_sm, float* __restrict__ out) {
  double v[SS_PART];
  gather_slots<SS_FIN>(slots, nslots, v);
  const auto sum = block_tree_sum<SS_FIN>(v);
  if (threadIdx.x == 0) {
    double ssim, l1;
    if constexpr (WEIGHTED) {
      // an all-zero weight: the term is 0 whatever its (then all-zero) numerator holds
      ssim = wsum[1] > 0.0 ? sum[0] * inv_ssim * inv_or_zero(wsum[1]) : 0.0;
      l1 = wsum[0] > 0.0 ? sum[1] * inv_l1 * inv_or_zero(wsum[0]) : 0.0;
    } else {
      ssim = sum[0] * inv_ssim;
      l1 = sum[1] * inv_l1;
    }
    const double sm = sum[2] * inv_sm;
    out[0] = (float)(0.85 * ssim + 0.15 * l1 + 0.1 * sm);
    out[1] = (float)ssim;
    out[2] = (float)l1;
    out[3] = (float)sm;
  }
}

__global__ __launch_bounds__(256) void selfsup_loss_bwd_kernel(const float* __restrict__ unit_grad, const float* __restrict__ gout,
                                                               float* __restrict__ grad, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) grad[i] = gout[0] * unit_grad[i];
}

template <int C, bool WEIGHTED>
static void launch_selfsup(const SelfSupArgs& a, unsigned nwg, double* slots, hipStream_t st) {
  if (a.unit_grad)
    hipLaunchKernelGGL((selfsup_loss_kernel<C, true, WEIGHTED>), dim3(nwg), dim3(SS_WG), 0, st, a, slots);
  else
    hipLaunchKernelGGL((selfsup_loss_kernel<C, false, WEIGHTED>), dim3(nwg), dim3(SS_WG), 0, st, a, slots);
}

static int64_t selfsup_slots(int B, int H, int W) { return ceil_div((int64_t)B * (H / 3) * (W / 3), SS_WG); }
static int selfsup_pre_slots(int B, int H, int W) { return grid_stride_slots((int64_t)B * H * W, SS_FIN, SS_PRE_MAX); }

// Both forward entry points: validate, fill the arguments and launch the pre-pass (WEIGHTED only), the main pass and the finalize.
// Workspace in doubles: plain, the main slots; WEIGHTED, wsum[2], the pre-pass slots, the main slots.
template <bool WEIGHTED>
static int selfsup_fwd(const void* left, const void* right, const void* disp, const void* weight, int B, int C, int H, int W, int dtype,
                       void* workspace, void* out, void* unit_grad, void* stream) {
  const char* name = WEIGHTED ? "selfsup_loss_weighted" : "selfsup_loss";
  RAGMI_REQUIRE(left && right && disp && (weight || !WEIGHTED) && workspace && out, RAGMI_EINVAL, "%s: null pointer", name);
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "%s: dtype %d not built (float32 only)", name, dtype);
  RAGMI_REQUIRE(C >= 1 && C <= 4, RAGMI_EUNSUPPORTED, "%s: C = %d not built (1..4)", name, C);
  RAGMI_REQUIRE(B > 0 && H >= 3 && W >= 3, RAGMI_EINVAL, "%s: bad size B=%d H=%d W=%d (H, W >= 3)", name, B, H, W);
  RAGMI_REQUIRE(aligned_to(workspace, 8), RAGMI_EINVAL, "%s: workspace not 8-byte aligned", name);
  const int64_t nslots = selfsup_slots(B, H, W);
  RAGMI_REQUIRE(nslots <= 0xffffffffLL, RAGMI_EINVAL, "%s: too many pixels", name);
  const int npre = WEIGHTED ? selfsup_pre_slots(B, H, W) : 0;
  double* wsum = WEIGHTED ? (double*)workspace : nullptr;
  double* pre = (double*)workspace + (WEIGHTED ? 2 : 0);
  double* slots = pre + (int64_t)npre * SS_PRE;
  SelfSupArgs a;
  a.left = (const float*)left; a.right = (const float*)right; a.disp = (const float*)disp; a.unit_grad = (float*)unit_grad;
  a.H = H; a.W = W; a.Hb = H / 3; a.Wb = W / 3;
  a.nthreads = (int64_t)B * a.Hb * a.Wb;
  const double n_img = (double)B * C * H * W, n_ssim = (double)B * C * a.Hb * a.Wb, n_px = (double)B * H * W;
  a.dxs_dd = (float)(-(double)W / (double)(W - 1));
  a.k_l1 = WEIGHTED ? 0.f : (float)(0.15 / n_img);
  a.k_ssim = WEIGHTED ? 0.f : (float)(0.85 / n_ssim);
  a.k_sm = (float)(0.1 / n_px);
  a.weight = (const float*)weight; a.wsum = wsum;
  a.c_l1 = 0.15 / (double)C;
  a.c_ssim = 0.85 / (double)C;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if constexpr (WEIGHTED) {
    const int64_t npx = (int64_t)B * H * W;
    if (npx + (int64_t)SS_PRE_MAX * SS_FIN < 0x7fffffffLL)     // the index and one stride past the end fit 32 bits
      hipLaunchKernelGGL(selfsup_weight_sums_kernel<uint32_t>, dim3((unsigned)npre), dim3(SS_FIN), 0, st, (const float*)weight, npx, H, W,
                         a.Hb, a.Wb, pre);
    else
      hipLaunchKernelGGL(selfsup_weight_sums_kernel<int64_t>, dim3((unsigned)npre), dim3(SS_FIN), 0, st, (const float*)weight, npx, H, W,
                         a.Hb, a.Wb, pre);
    hipLaunchKernelGGL(selfsup_weight_sums_finalize_kernel, dim3(1), dim3(SS_FIN), 0, st, (const double*)pre, npre, wsum);
  }
  switch (C) {
    case 1: launch_selfsup<1, WEIGHTED>(a, (unsigned)nslots, slots, st); break;
    case 2: launch_selfsup<2, WEIGHTED>(a, (unsigned)nslots, slots, st); break;
    case 3: launch_selfsup<3, WEIGHTED>(a, (unsigned)nslots, slots, st); break;
    default: launch_selfsup<4, WEIGHTED>(a, (unsigned)nslots, slots, st); break;
  }
  const double inv_c = 1.0 / (double)C;
  hipLaunchKernelGGL(selfsup_loss_finalize_kernel<WEIGHTED>, dim3(1), dim3(SS_FIN), 0, st, (const double*)slots, nslots,
                     (const double*)wsum, WEIGHTED ? inv_c : 1.0 / n_ssim, WEIGHTED ? inv_c : 1.0 / n_img, 1.0 / n_px, (float*)out);
  return check_launch(WEIGHTED ? "selfsup_loss_weighted_fwd" : "selfsup_loss_fwd");
}

}  // namespace ragmi

extern "C" int64_t ragmi_selfsup_loss_workspace_elems(int B, int H, int W) {
  if (B <= 0 || H < 3 || W < 3) return 0;
  return ragmi::selfsup_slots(B, H, W) * ragmi::SS_PART * 2;        // one double (two floats) per partial
}

// workspace, in doubles: wsum[2], the pre-pass slots, the main slots
extern "C" int64_t ragmi_selfsup_loss_weighted_workspace_elems(int B, int H, int W) {
  if (B <= 0 || H < 3 || W < 3) return 0;
  return (2 + (int64_t)ragmi::selfsup_pre_slots(B, H, W) * ragmi::SS_PRE + ragmi::selfsup_slots(B, H, W) * ragmi::SS_PART) * 2;
}

extern "C" int ragmi_selfsup_loss_fwd(const void* left, const void* right, const void* disp, int B, int C, int H, int W, int dtype,
                                      void* workspace, void* out, void* unit_grad, void* stream) {
  return ragmi::selfsup_fwd<false>(left, right, disp, nullptr, B, C, H, W, dtype, workspace, out, unit_grad, stream);
}

extern "C" int ragmi_selfsup_loss_weighted_fwd(const void* left, const void* right, const void* disp, const void* weight, int B, int C,
                                               int H, int W, int dtype, void* workspace, void* out, void* unit_grad, void* stream) {
  return ragmi::selfsup_fwd<true>(left, right, disp, weight, B, C, H, W, dtype, workspace, out, unit_grad, stream);
}

extern "C" int ragmi_selfsup_loss_bwd(const void* unit_grad, const void* gout, void* grad, int64_t n, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(unit_grad && gout && grad, RAGMI_EINVAL, "selfsup_loss_bwd: null pointer");
  RAGMI_REQUIRE(n > 0, RAGMI_EINVAL, "selfsup_loss_bwd: bad size");
  hipLaunchKernelGGL(selfsup_loss_bwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     (const float*)unit_grad, (const float*)gout, (float*)grad, n);
  return check_launch("selfsup_loss_bwd");
}

/* backward of ragmi_selfsup_loss_weighted_fwd's out[0]: the plain loss's scaling launch, grad[i] = gout[0] * unit_grad[i] */
extern "C" int ragmi_selfsup_loss_weighted_bwd(const void* unit_grad, const void* gout, void* grad, int64_t n, void* stream) {
  return ragmi_selfsup_loss_bwd(unit_grad, gout, grad, n, stream);
}
