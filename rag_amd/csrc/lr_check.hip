// Left-right consistency of a stereo pair's two disparity maps, and the launch that builds the two-view batch they come from.
//
// ragmi_lr_stack_fwd writes out_left = [left ; mirror_x(right)] and out_right = [right ; mirror_x(left)]: sample i < B is the
// ordinary pair, sample i + B the pair seen from the right camera (mirrored along x it is again a legitimate left / right pair), so
// ONE forward of the 2B batch gives both views' disparities.  It only moves data; it is a kernel so that a captured step holds
// kernel nodes only (torch.cat / flip / copy_ may become memcpy nodes).
//
// ragmi_lr_check_fwd looks every pixel's disparity up in the other view (x - d, linear along the row) and marks the pixel
// consistent when the two agree within max(abs_tol, rel_tol |d|).  The partner row may be read mirrored and from another batch item
// ((b + partner_shift) mod B), so the stacked batch checks itself: the right-view disparity of sample i is the mirror of sample
// i +- B and is never materialised.  One thread owns one pixel; the consistent pixels are counted as integers per workgroup slot and
// a one-workgroup finalize folds each image's slots in the fixed order of reduce.h: no atomics, no memset, the same bits on every
// run.  A non-finite disparity or tap stays in its own pixel and is never used as an index.  DESIGN.md section 4.5.1.
#include <cmath>

#include "reduce.h"

namespace ragmi {

constexpr int LR_WG = 256;       // threads per workgroup of both kernels and of the finalize

__global__ __launch_bounds__(LR_WG) void lr_stack_kernel(const float* __restrict__ left, const float* __restrict__ right,
                                                         float* __restrict__ out_left, float* __restrict__ out_right, int B, int W,
                                                         int64_t chw, int64_t n) {
  // n = 2 * (2B * chw): the elements of out_left, then those of out_right
  const int64_t i = (int64_t)blockIdx.x * LR_WG + threadIdx.x;
  if (i >= n) return;
  const int64_t half = n / 2;
  const bool to_right = i >= half;
  const int64_t o = to_right ? i - half : i;               // offset inside the output
  const int64_t s = o / chw, r = o - s * chw;               // sample of the 2B batch, offset inside it
  const bool mirror = s >= B;
  const int64_t row = r / W;
  const int x = (int)(r - row * W);
  const int64_t src = (mirror ? s - B : s) * chw + row * W + (mirror ? W - 1 - x : x);
  // out_left: left, then mirrored right; out_right: right, then mirrored left
  const float v = (to_right != mirror) ? right[src] : left[src];
  (to_right ? out_right : out_left)[o] = v;
}

template <bool ERR>
__global__ __launch_bounds__(LR_WG) void lr_check_kernel(const float* __restrict__ disp, const float* __restrict__ partner, int B, int W,
                                                         int64_t hw, int partner_shift, int mirrored, float abs_tol, float rel_tol,
                                                         float occluded_weight, unsigned nwg, int* __restrict__ slots,
                                                         float* __restrict__ weight, float* __restrict__ err) {
#pragma clang fp contract(off)                              // the rule's arithmetic as written: products and sums round separately
  const int b = blockIdx.x / nwg;
  const int64_t p = (int64_t)(blockIdx.x - (unsigned)b * nwg) * LR_WG + threadIdx.x;     // pixel of image b
  int ok = 0;
  if (p < hw) {
    const int64_t y = p / W;
    const int x = (int)(p - y * W);
    const float d = disp[b * hw + p];
    const float xr = (float)x - d;
    const bool in_view = isfinite(d) && xr >= 0.f && xr <= (float)(W - 1);
    float e = INFINITY;
    if (in_view) {                                          // only here is xr an index: 0 <= x0 <= x1 <= W - 1
      const float x0f = floorf(xr);
      const int x0 = (int)x0f, x1 = min(x0 + 1, W - 1);
      const float f = xr - x0f;
      int pb = b + partner_shift;
      if (pb >= B) pb -= B;
      const float* prow = partner + pb * hw + y * W;
      const float p0 = prow[mirrored ? W - 1 - x0 : x0], p1 = prow[mirrored ? W - 1 - x1 : x1];
      const float dp = (1.f - f) * p0 + f * p1;
      e = fabsf(d - dp);
      if (!isfinite(e)) e = INFINITY;
    }
    ok = in_view && e <= fmaxf(abs_tol, rel_tol * fabsf(d));      // e = +inf fails; in view, d is finite
    weight[b * hw + p] = ok ? 1.f : occluded_weight;
    if (ERR) err[b * hw + p] = e;
  }
  const int v[1] = {ok};
  const auto sum = block_tree_sum<LR_WG>(v);
  if (threadIdx.x == 0) slots[blockIdx.x] = sum[0];
}

// valid[b] = float(double(consistent pixels of image b) / double(H W)); one workgroup walks the images
__global__ __launch_bounds__(LR_WG) void lr_check_finalize_kernel(const int* __restrict__ slots, int B, unsigned nwg, double hw,
                                                                  float* __restrict__ valid) {
  for (int b = 0; b < B; ++b) {
    long long v[1];
    gather_slots<LR_WG>(slots + (int64_t)b * nwg, nwg, v);
    const auto sum = block_tree_sum<LR_WG>(v);
    if (threadIdx.x == 0) valid[b] = (float)((double)sum[0] / hw);
    __syncthreads();                                        // the sums are read before the next image's tree reuses the LDS
  }
}

static int64_t lr_check_wgs(int H, int W) { return ceil_div((int64_t)H * W, LR_WG); }

}  // namespace ragmi

extern "C" int ragmi_lr_stack_fwd(const void* left, const void* right, void* out_left, void* out_right, int B, int C, int H, int W,
                                  void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(left && right && out_left && out_right, RAGMI_EINVAL, "lr_stack: null pointer");
  RAGMI_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, RAGMI_EINVAL, "lr_stack: bad size B=%d C=%d H=%d W=%d", B, C, H, W);
  const int64_t chw = (int64_t)C * H * W, n = 4 * (int64_t)B * chw;
  const int64_t nwg = ceil_div(n, LR_WG);
  RAGMI_REQUIRE(nwg <= 0x7fffffffLL, RAGMI_EINVAL, "lr_stack: too many elements");
  hipLaunchKernelGGL(lr_stack_kernel, dim3((unsigned)nwg), dim3(LR_WG), 0, static_cast<hipStream_t>(stream), (const float*)left,
                     (const float*)right, (float*)out_left, (float*)out_right, B, W, chw, n);
  return check_launch("lr_stack_fwd");
}

extern "C" int64_t ragmi_lr_check_workspace_elems(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 2) return 0;
  return (int64_t)B * ragmi::lr_check_wgs(H, W);            // one 32-bit count per workgroup
}

extern "C" int ragmi_lr_check_fwd(const void* disp, const void* partner, int B, int H, int W, int partner_shift, int mirrored,
                                  float abs_tol, float rel_tol, float occluded_weight, void* workspace, void* weight, void* err,
                                  void* valid, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(disp && partner && workspace && weight && valid, RAGMI_EINVAL, "lr_check: null pointer");
  RAGMI_REQUIRE(B >= 1 && H >= 1 && W >= 2, RAGMI_EINVAL, "lr_check: bad size B=%d H=%d W=%d (B, H >= 1, W >= 2)", B, H, W);
  RAGMI_REQUIRE(partner_shift >= 0 && partner_shift < B, RAGMI_EINVAL, "lr_check: partner_shift %d outside [0, %d)", partner_shift, B);
  RAGMI_REQUIRE(std::isfinite(abs_tol) && abs_tol >= 0.f && std::isfinite(rel_tol) && rel_tol >= 0.f, RAGMI_EINVAL,
                "lr_check: abs_tol and rel_tol must be finite and non-negative");
  RAGMI_REQUIRE(std::isfinite(occluded_weight) && occluded_weight >= 0.f && occluded_weight <= 1.f, RAGMI_EINVAL,
                "lr_check: occluded_weight must lie in [0, 1]");
  RAGMI_REQUIRE(aligned_to(workspace, 4), RAGMI_EINVAL, "lr_check: workspace not 4-byte aligned");
  const int64_t hw = (int64_t)H * W, nwg = lr_check_wgs(H, W);
  RAGMI_REQUIRE(B * nwg <= 0x7fffffffLL, RAGMI_EINVAL, "lr_check: too many pixels");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* slots = (int*)workspace;
  if (err)
    hipLaunchKernelGGL((lr_check_kernel<true>), dim3((unsigned)(B * nwg)), dim3(LR_WG), 0, st, (const float*)disp, (const float*)partner,
                       B, W, hw, partner_shift, mirrored != 0, abs_tol, rel_tol, occluded_weight, (unsigned)nwg, slots, (float*)weight,
                       (float*)err);
  else
    hipLaunchKernelGGL((lr_check_kernel<false>), dim3((unsigned)(B * nwg)), dim3(LR_WG), 0, st, (const float*)disp, (const float*)partner,
                       B, W, hw, partner_shift, mirrored != 0, abs_tol, rel_tol, occluded_weight, (unsigned)nwg, slots, (float*)weight,
                       (float*)nullptr);
  hipLaunchKernelGGL(lr_check_finalize_kernel, dim3(1), dim3(LR_WG), 0, st, (const int*)slots, B, (unsigned)nwg, (double)hw,
                     (float*)valid);
  return check_launch("lr_check_fwd");
}
