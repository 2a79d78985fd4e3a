// The self-supervised loss of selfsup_loss.hip with a per-pixel weight w [B, H, W] on its photometric terms (the left-right
// consistency weight of lr_check.hip; the reference's mean_l1(x, y, mask), src_self/models/loss.py:66-76, takes such a mask that its
// caller never supplies):
//   L1     = sum_{b,c,y,x} w |left - left_est| / (C sum w)
//   SSIM   = sum_{blocks,c} wb term / (C sum wb),   wb = avg_pool2d(w, 3): the mean of w over the block, term as in selfsup_loss.hip
//   smooth   unchanged and unweighted (it is what fills the occluded band)
//   total  = 0.85 SSIM + 0.15 L1 + 0.1 smooth,     and d total / d disp; w is a constant (no gradient flows to it).
// A term whose weights sum to 0 is 0 and so is its gradient (the reference form would give NaN, which a captured step would write into
// the weights).  The gradient needs 1 / sum w and 1 / sum wb at every pixel, so a fixed-order pre-pass (grid-stride partials in
// double, one-workgroup fold: reduce.h) leaves the two sums as two doubles on the device and the main kernel reads them: four
// launches, no host synchronisation, no atomics, no memset.  Per pixel the arithmetic is selfsup_loss.hip's (selfsup_common.h), so
// w = 1 gives its numbers.  DESIGN.md section 4.5.1.
#include "reduce.h"
#include "selfsup_common.h"

namespace ragmi {

constexpr int SSW_WG = 64;        // threads per workgroup of the main pass, one 3x3 block per thread (as SS_WG)
constexpr int SSW_FIN = 256;      // threads of the pre-pass workgroups and of both one-workgroup folds
constexpr int SSW_PART = 3;       // partials per main slot (double): sum wb term, sum w |left - left_est|, sum smoothness
constexpr int SSW_PRE = 2;        // partials per pre-pass slot (double): sum w, sum w inside the 3x3 blocks
constexpr int SSW_PRE_MAX = 256;  // at most this many pre-pass workgroups

struct WSelfSupArgs {
  const float* left;     // [B, C, H, W]
  const float* right;    // [B, C, H, W]
  const float* disp;     // [B, H, W]
  const float* weight;   // [B, H, W]
  float* unit_grad;      // [B, H, W] d total / d disp, or null
  const double* wsum;    // [2] sum w, sum wb (written by the pre-pass)
  int H, W, Hb, Wb;      // Hb, Wb: 3x3 SSIM blocks per column / row
  int64_t nthreads;      // B * Hb * Wb
  float dxs_dd;          // d xs / d disp = -W / (W - 1)
  float k_sm;            // 0.1 / (B H W)
  double c_l1;           // 0.15 / C: k_l1 = c_l1 / sum w
  double c_ssim;         // 0.85 / C: k_ssim = c_ssim / sum wb
};

// slots[s] = (sum w, sum of the w that lie inside a 3x3 block) over the pixels i = first, first + stride, ... of workgroup s.  I: the
// type of the pixel index (32-bit divisions where B H W allows them)
template <class I>
__global__ __launch_bounds__(SSW_FIN) void selfsup_weight_sums_kernel(const float* __restrict__ weight, int64_t n, int H, int W, int Hb,
                                                                      int Wb, double* __restrict__ slots) {
  double v[SSW_PRE] = {0.0, 0.0};
  const I stride = (I)gridDim.x * SSW_FIN;
  for (I i = (I)blockIdx.x * SSW_FIN + threadIdx.x; i < (I)n; i += stride) {
    const I row = i / (I)W;                                  // b * H + y
    const int x = (int)(i - row * (I)W), y = (int)(row % (I)H);
    const double w = weight[i];
    v[0] += w;
    if (y < 3 * Hb && x < 3 * Wb) v[1] += w;
  }
  const auto sum = block_tree_sum<SSW_FIN>(v);
  if (threadIdx.x < SSW_PRE) slots[(int64_t)blockIdx.x * SSW_PRE + threadIdx.x] = sum[threadIdx.x];
}

// wsum[0] = sum w, wsum[1] = sum wb = (sum of w inside the blocks) / 9
__global__ __launch_bounds__(SSW_FIN) void selfsup_weight_sums_finalize_kernel(const double* __restrict__ slots, int nslots,
                                                                               double* __restrict__ wsum) {
  double v[SSW_PRE];
  gather_slots<SSW_FIN>(slots, nslots, v);
  const auto sum = block_tree_sum<SSW_FIN>(v);
  if (threadIdx.x == 0) {
    wsum[0] = sum[0];
    wsum[1] = sum[1] / 9.0;
  }
}

__device__ __forceinline__ double inv_or_zero(double s) { return s > 0.0 ? 1.0 / s : 0.0; }

template <int C, bool GRAD>
__global__ __launch_bounds__(SSW_WG) void selfsup_loss_weighted_kernel(WSelfSupArgs a, double* __restrict__ slots) {
  const int64_t t = (int64_t)blockIdx.x * SSW_WG + threadIdx.x;
  float acc_ssim = 0.f, acc_l1 = 0.f, acc_sm = 0.f;
  if (t < a.nthreads) {
    const int H = a.H, W = a.W;
    const int64_t nblk = (int64_t)a.Hb * a.Wb, hw = (int64_t)H * W;
    const int64_t b = t / nblk;
    const int r = (int)(t - b * nblk), by = r / a.Wb, bx = r - by * a.Wb;
    const float* lb = a.left + b * C * hw;
    const float* rb = a.right + b * C * hw;
    const float* db = a.disp + b * hw;
    const float* wp = a.weight + b * hw;
    float* gb = GRAD ? a.unit_grad + b * hw : nullptr;
    const float k_l1 = GRAD ? (float)(a.c_l1 * inv_or_zero(a.wsum[0])) : 0.f;
    const float k_ssim = GRAD ? (float)(a.c_ssim * inv_or_zero(a.wsum[1])) : 0.f;
    const int y0 = 3 * by, x0 = 3 * bx;
    const int y1 = by == a.Hb - 1 ? H : y0 + 3, x1 = bx == a.Wb - 1 ? W : x0 + 3;   // the last block row / column owns the remainder

    // ---- the 3x3 SSIM block: x = left, y = left_est (loss.py:77-97)
    float lv[9][C], ev[9][C], dv[9][C], gs[9], wv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int y = y0 + k / 3, x = x0 + k % 3;
      const int64_t i = (int64_t)y * W + x;
      const float d = db[i];
      wv[k] = wp[i];
      warp_px<C>(rb, hw, H, W, y, x, d, ev[k], dv[k], a.dxs_dd);
      float gsm = 0.f;
      acc_sm += smooth_px<C, GRAD>(lb, db, hw, H, W, y, x, d, gsm);
      gs[k] = gsm * a.k_sm;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        lv[k][c] = lb[c * hw + i];
        acc_l1 += wv[k] * fabsf(lv[k][c] - ev[k][c]);
      }
    }
    float wb;
    {
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
        // the term's value without contraction, as in selfsup_loss_kernel: both instantiations round a block the same way
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
        acc_ssim += wb * fminf(fmaxf(h, 0.f), 1.f);
      }
      if (GRAD) {
        // d (wb term) / d y_i = -wb/2 dS/dy_i, dS/dy_i as in selfsup_loss_kernel; the L1 part carries the pixel's own w
        const float kc = (h >= 0.f && h <= 1.f) ? -(k_ssim * wb) / (9.f * Cd * D) : 0.f;
        const float base = mx * Bn - S * my * D, SCd = S * Cd;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float dS = base + A * (lv[k][c] - mx) - SCd * (ev[k][c] - my);
          const float ge = kc * dS - (k_l1 * wv[k]) * sgnf(lv[k][c] - ev[k][c]);     // d total / d left_est[c] at pixel k
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
        const float d = db[i], w = wp[i];
        float e[C], de[C];
        warp_px<C>(rb, hw, H, W, y, x, d, e, de, a.dxs_dd);
        float gsm = 0.f;
        acc_sm += smooth_px<C, GRAD>(lb, db, hw, H, W, y, x, d, gsm);
        float g = gsm * a.k_sm;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float l = lb[c * hw + i];
          acc_l1 += w * fabsf(l - e[c]);
          if (GRAD) g -= (k_l1 * w) * sgnf(l - e[c]) * de[c];
        }
        if (GRAD) gb[i] = g;
      }
    }
  }
  // ---- per-workgroup partials in double, one slot per workgroup
  const double v[SSW_PART] = {acc_ssim, acc_l1, acc_sm};
  const auto sum = block_tree_sum<SSW_WG>(v);
  if (threadIdx.x < SSW_PART) slots[(int64_t)blockIdx.x * SSW_PART + threadIdx.x] = sum[threadIdx.x];
}

// out[0..3] = total, SSIM, L1, smoothness (total = 0.85 SSIM + 0.15 L1 + 0.1 smoothness): the slots in a fixed order
__global__ __launch_bounds__(SSW_FIN) void selfsup_loss_weighted_finalize_kernel(const double* __restrict__ slots, int64_t nslots,
                                                                                 const double* __restrict__ wsum, double inv_c,
                                                                                 double inv_sm, float* __restrict__ out) {
  double v[SSW_PART];
  gather_slots<SSW_FIN>(slots, nslots, v);
  const auto sum = block_tree_sum<SSW_FIN>(v);
  if (threadIdx.x == 0) {
    // an all-zero weight: the term is 0 whatever its (then all-zero) numerator holds
    const double ssim = wsum[1] > 0.0 ? sum[0] * inv_c * inv_or_zero(wsum[1]) : 0.0;
    const double l1 = wsum[0] > 0.0 ? sum[1] * inv_c * inv_or_zero(wsum[0]) : 0.0;
    const double sm = sum[2] * inv_sm;
    out[0] = (float)(0.85 * ssim + 0.15 * l1 + 0.1 * sm);
    out[1] = (float)ssim;
    out[2] = (float)l1;
    out[3] = (float)sm;
  }
}

template <int C>
static void launch_selfsup_weighted(const WSelfSupArgs& a, unsigned nwg, double* slots, hipStream_t st) {
  if (a.unit_grad)
    hipLaunchKernelGGL((selfsup_loss_weighted_kernel<C, true>), dim3(nwg), dim3(SSW_WG), 0, st, a, slots);
  else
    hipLaunchKernelGGL((selfsup_loss_weighted_kernel<C, false>), dim3(nwg), dim3(SSW_WG), 0, st, a, slots);
}

static int64_t ssw_slots(int B, int H, int W) { return ceil_div((int64_t)B * (H / 3) * (W / 3), SSW_WG); }
static int ssw_pre_slots(int B, int H, int W) { return grid_stride_slots((int64_t)B * H * W, SSW_FIN, SSW_PRE_MAX); }

}  // namespace ragmi

// workspace, in doubles: wsum[2], the pre-pass slots, the main slots
extern "C" int64_t ragmi_selfsup_loss_weighted_workspace_elems(int B, int H, int W) {
  if (B <= 0 || H < 3 || W < 3) return 0;
  return (2 + (int64_t)ragmi::ssw_pre_slots(B, H, W) * ragmi::SSW_PRE + ragmi::ssw_slots(B, H, W) * ragmi::SSW_PART) * 2;
}

extern "C" int ragmi_selfsup_loss_weighted_fwd(const void* left, const void* right, const void* disp, const void* weight, int B, int C,
                                               int H, int W, int dtype, void* workspace, void* out, void* unit_grad, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(left && right && disp && weight && workspace && out, RAGMI_EINVAL, "selfsup_loss_weighted: null pointer");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "selfsup_loss_weighted: dtype %d not built (float32 only)", dtype);
  RAGMI_REQUIRE(C >= 1 && C <= 4, RAGMI_EUNSUPPORTED, "selfsup_loss_weighted: C = %d not built (1..4)", C);
  RAGMI_REQUIRE(B > 0 && H >= 3 && W >= 3, RAGMI_EINVAL, "selfsup_loss_weighted: bad size B=%d H=%d W=%d (H, W >= 3)", B, H, W);
  RAGMI_REQUIRE(aligned_to(workspace, 8), RAGMI_EINVAL, "selfsup_loss_weighted: workspace not 8-byte aligned");
  const int64_t nslots = ssw_slots(B, H, W);
  RAGMI_REQUIRE(nslots <= 0xffffffffLL, RAGMI_EINVAL, "selfsup_loss_weighted: too many pixels");
  const int npre = ssw_pre_slots(B, H, W);
  double* wsum = (double*)workspace;
  double* pre = wsum + 2;
  double* slots = pre + (int64_t)npre * SSW_PRE;
  WSelfSupArgs a;
  a.left = (const float*)left; a.right = (const float*)right; a.disp = (const float*)disp; a.weight = (const float*)weight;
  a.unit_grad = (float*)unit_grad; a.wsum = wsum;
  a.H = H; a.W = W; a.Hb = H / 3; a.Wb = W / 3;
  a.nthreads = (int64_t)B * a.Hb * a.Wb;
  const double n_px = (double)B * H * W;
  a.dxs_dd = (float)(-(double)W / (double)(W - 1));
  a.k_sm = (float)(0.1 / n_px);
  a.c_l1 = 0.15 / (double)C;
  a.c_ssim = 0.85 / (double)C;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t npx = (int64_t)B * H * W;
  if (npx + (int64_t)SSW_PRE_MAX * SSW_FIN < 0x7fffffffLL)     // the index and one stride past the end fit 32 bits
    hipLaunchKernelGGL(selfsup_weight_sums_kernel<uint32_t>, dim3((unsigned)npre), dim3(SSW_FIN), 0, st, (const float*)weight, npx, H, W,
                       a.Hb, a.Wb, pre);
  else
    hipLaunchKernelGGL(selfsup_weight_sums_kernel<int64_t>, dim3((unsigned)npre), dim3(SSW_FIN), 0, st, (const float*)weight, npx, H, W,
                       a.Hb, a.Wb, pre);
  hipLaunchKernelGGL(selfsup_weight_sums_finalize_kernel, dim3(1), dim3(SSW_FIN), 0, st, (const double*)pre, npre, wsum);
  switch (C) {
    case 1: launch_selfsup_weighted<1>(a, (unsigned)nslots, slots, st); break;
    case 2: launch_selfsup_weighted<2>(a, (unsigned)nslots, slots, st); break;
    case 3: launch_selfsup_weighted<3>(a, (unsigned)nslots, slots, st); break;
    default: launch_selfsup_weighted<4>(a, (unsigned)nslots, slots, st); break;
  }
  hipLaunchKernelGGL(selfsup_loss_weighted_finalize_kernel, dim3(1), dim3(SSW_FIN), 0, st, (const double*)slots, nslots,
                     (const double*)wsum, 1.0 / (double)C, 1.0 / n_px, (float*)out);
  return check_launch("selfsup_loss_weighted_fwd");
}

/* backward of ragmi_selfsup_loss_weighted_fwd's out[0]: the plain loss's scaling launch, grad[i] = gout[0] * unit_grad[i] */
extern "C" int ragmi_selfsup_loss_weighted_bwd(const void* unit_grad, const void* gout, void* grad, int64_t n, void* stream) {
  return ragmi_selfsup_loss_bwd(unit_grad, gout, grad, n, stream);
}
