// Self-supervised training loss of the continual-adaptation mode (src_self/approaches/rag.py:266-278 with supervise=False):
// re_and_sm_loss (src_self/models/loss.py:112-141) = 0.85 SSIM_mean + 0.15 L1_mean of the right image warped by the disparity,
// plus 0.1 x an edge-aware smoothness term, and its gradient with respect to the disparity.  The reference builds it from two
// grid_samples, five avg_pool2d and a few dozen element-wise ATen ops (and their backward), and its warp() makes host tensors and
// copies them to the device at every call.  Here one thread owns one non-overlapping 3x3 SSIM block (avg_pool2d(kernel_size=3)
// strides by 3) for all channels and computes, in the same pass, its share of the three sums and the gradient of the total at its
// own pixels; a second one-workgroup kernel folds the per-workgroup partials, in the fixed order of reduce.h and without host
// synchronisation.  DESIGN.md section 4.5.
#include "reduce.h"
#include "selfsup_common.h"

namespace ragmi {

constexpr int SS_WG = 64;        // threads per workgroup of the main pass: one wave (B*(H/3)*(W/3) threads spread over many CUs)
constexpr int SS_FIN = 256;      // threads of the finalize workgroup
constexpr int SS_PART = 3;       // partials per workgroup slot (double): sum SSIM terms, sum |left - left_est|, sum smoothness

struct SelfSupArgs {
  const float* left;     // [B, C, H, W]
  const float* right;    // [B, C, H, W]
  const float* disp;     // [B, H, W]
  float* unit_grad;      // [B, H, W] d total / d disp, or null
  int H, W, Hb, Wb;      // Hb, Wb: 3x3 SSIM blocks per column / row
  int64_t nthreads;      // B * Hb * Wb
  float dxs_dd;          // d xs / d disp = -W / (W - 1)
  float k_l1;            // 0.15 / (B C H W)
  float k_ssim;          // 0.85 / (B C Hb Wb)
  float k_sm;            // 0.1 / (B H W)
};

template <int C, bool GRAD>
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
    float* gb = GRAD ? a.unit_grad + b * hw : nullptr;
    const int y0 = 3 * by, x0 = 3 * bx;
    const int y1 = by == a.Hb - 1 ? H : y0 + 3, x1 = bx == a.Wb - 1 ? W : x0 + 3;   // the last block row / column owns the remainder

    // ---- the 3x3 SSIM block: x = left, y = left_est (loss.py:77-97)
    float lv[9][C], ev[9][C], dv[9][C], gs[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int y = y0 + k / 3, x = x0 + k % 3;
      const int64_t i = (int64_t)y * W + x;
      const float d = db[i];
      warp_px<C>(rb, hw, H, W, y, x, d, ev[k], dv[k], a.dxs_dd);
      float gsm = 0.f;
      acc_sm += smooth_px<C, GRAD>(lb, db, hw, H, W, y, x, d, gsm);
      gs[k] = gsm * a.k_sm;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        lv[k][c] = lb[c * hw + i];
        acc_l1 += fabsf(lv[k][c] - ev[k][c]);
      }
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
      }
      acc_ssim += fminf(fmaxf(h, 0.f), 1.f);
      if (GRAD) {
        // d term / d y_i = -1/2 dS/dy_i (clamp passes the gradient on the closed interval), with
        // dS/dy_i = 2/(9 Cd D) * (mx Bn + A (x_i - mx) - S (my D + Cd (y_i - my)))
        const float kc = (h >= 0.f && h <= 1.f) ? -a.k_ssim / (9.f * Cd * D) : 0.f;
        const float base = mx * Bn - S * my * D, SCd = S * Cd;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float dS = base + A * (lv[k][c] - mx) - SCd * (ev[k][c] - my);
          const float ge = kc * dS - a.k_l1 * sgnf(lv[k][c] - ev[k][c]);     // d total / d left_est[c] at pixel k
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
        float e[C], de[C];
        warp_px<C>(rb, hw, H, W, y, x, d, e, de, a.dxs_dd);
        float gsm = 0.f;
        acc_sm += smooth_px<C, GRAD>(lb, db, hw, H, W, y, x, d, gsm);
        float g = gsm * a.k_sm;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float l = lb[c * hw + i];
          acc_l1 += fabsf(l - e[c]);
          if (GRAD) g -= a.k_l1 * sgnf(l - e[c]) * de[c];
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

// out[0..3] = total, SSIM_mean, L1_mean, smoothness_mean (total = 0.85 SSIM + 0.15 L1 + 0.1 smoothness): the slots in a fixed order
__global__ __launch_bounds__(SS_FIN) void selfsup_loss_finalize_kernel(const double* __restrict__ slots, int64_t nslots, double inv_ssim,
                                                                       double inv_l1, double inv_sm, float* __restrict__ out) {
  double v[SS_PART];
  gather_slots<SS_FIN>(slots, nslots, v);
  const auto sum = block_tree_sum<SS_FIN>(v);
  if (threadIdx.x == 0) {
    const double ssim = sum[0] * inv_ssim, l1 = sum[1] * inv_l1, sm = sum[2] * inv_sm;
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

template <int C>
static void launch_selfsup(const SelfSupArgs& a, unsigned nwg, double* slots, hipStream_t st) {
  if (a.unit_grad)
    hipLaunchKernelGGL((selfsup_loss_kernel<C, true>), dim3(nwg), dim3(SS_WG), 0, st, a, slots);
  else
    hipLaunchKernelGGL((selfsup_loss_kernel<C, false>), dim3(nwg), dim3(SS_WG), 0, st, a, slots);
}

static int64_t selfsup_slots(int B, int H, int W) { return ceil_div((int64_t)B * (H / 3) * (W / 3), SS_WG); }

}  // namespace ragmi

extern "C" int64_t ragmi_selfsup_loss_workspace_elems(int B, int H, int W) {
  if (B <= 0 || H < 3 || W < 3) return 0;
  return ragmi::selfsup_slots(B, H, W) * ragmi::SS_PART * 2;        // one double (two floats) per partial
}

extern "C" int ragmi_selfsup_loss_fwd(const void* left, const void* right, const void* disp, int B, int C, int H, int W, int dtype,
                                      void* workspace, void* out, void* unit_grad, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(left && right && disp && workspace && out, RAGMI_EINVAL, "selfsup_loss: null pointer");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "selfsup_loss: dtype %d not built (float32 only)", dtype);
  RAGMI_REQUIRE(C >= 1 && C <= 4, RAGMI_EUNSUPPORTED, "selfsup_loss: C = %d not built (1..4)", C);
  RAGMI_REQUIRE(B > 0 && H >= 3 && W >= 3, RAGMI_EINVAL, "selfsup_loss: bad size B=%d H=%d W=%d (H, W >= 3)", B, H, W);
  RAGMI_REQUIRE(aligned_to(workspace, 8), RAGMI_EINVAL, "selfsup_loss: workspace not 8-byte aligned");
  const int64_t nslots = selfsup_slots(B, H, W);
  RAGMI_REQUIRE(nslots <= 0xffffffffLL, RAGMI_EINVAL, "selfsup_loss: too many pixels");
  SelfSupArgs a;
  a.left = (const float*)left; a.right = (const float*)right; a.disp = (const float*)disp; a.unit_grad = (float*)unit_grad;
  a.H = H; a.W = W; a.Hb = H / 3; a.Wb = W / 3;
  a.nthreads = (int64_t)B * a.Hb * a.Wb;
  const double n_img = (double)B * C * H * W, n_ssim = (double)B * C * a.Hb * a.Wb, n_px = (double)B * H * W;
  a.dxs_dd = (float)(-(double)W / (double)(W - 1));
  a.k_l1 = (float)(0.15 / n_img);
  a.k_ssim = (float)(0.85 / n_ssim);
  a.k_sm = (float)(0.1 / n_px);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* slots = (double*)workspace;
  switch (C) {
    case 1: launch_selfsup<1>(a, (unsigned)nslots, slots, st); break;
    case 2: launch_selfsup<2>(a, (unsigned)nslots, slots, st); break;
    case 3: launch_selfsup<3>(a, (unsigned)nslots, slots, st); break;
    default: launch_selfsup<4>(a, (unsigned)nslots, slots, st); break;
  }
  hipLaunchKernelGGL(selfsup_loss_finalize_kernel, dim3(1), dim3(SS_FIN), 0, st, (const double*)slots, nslots, 1.0 / n_ssim,
                     1.0 / n_img, 1.0 / n_px, (float*)out);
  return check_launch("selfsup_loss_fwd");
}

extern "C" int ragmi_selfsup_loss_bwd(const void* unit_grad, const void* gout, void* grad, int64_t n, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(unit_grad && gout && grad, RAGMI_EINVAL, "selfsup_loss_bwd: null pointer");
  RAGMI_REQUIRE(n > 0, RAGMI_EINVAL, "selfsup_loss_bwd: bad size");
  hipLaunchKernelGGL(selfsup_loss_bwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     (const float*)unit_grad, (const float*)gout, (float*)grad, n);
  return check_launch("selfsup_loss_bwd");
}
