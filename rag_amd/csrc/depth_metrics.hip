// Loss + evaluation metrics of the monocular-depth eval loop (rag_depth/src/approaches/rag.py:440-489) as ONE pass over
// (depth_est, depth_gt): the masked pixels gt > 0 of the whole batch, as the reference gathers them.  silog_loss
// (utilstool/experiment.py:154-161) and compute_errors (approaches/rag.py:19-41) share their sums: with d = log est - log gt,
//   n, sum d, sum d^2, sum |gt - est| / gt, sum (gt - est)^2 / gt, sum (gt - est)^2, sum |log10 est - log10 gt|,
//   and the counts of max(gt/est, est/gt) < 1.25, 1.25^2, 1.25^3
// (log_rms's (log gt - log est)^2 is d^2, bit for bit).  Per-pixel terms are fp32 like the reference's arrays; the sums are double.
// Partials are reduced in the fixed order of reduce.h (an LDS tree per workgroup, then a one-workgroup finalize).  The reference
// does a boolean gather, a D2H copy and numpy per batch.
#include "reduce.h"

namespace ragmi {

constexpr int DM_WG = 256;       // threads per workgroup, main pass and finalize
constexpr int DM_NSUM = 10;      // sums per slot (order above)
constexpr int DM_MAXWG = 1024;   // workgroups of the main pass at most (grid-stride beyond)

__global__ __launch_bounds__(DM_WG) void depth_metrics_kernel(const float* __restrict__ est, const float* __restrict__ gt, int64_t n,
                                                              double* __restrict__ slots) {
  double v[DM_NSUM];
#pragma unroll
  for (int k = 0; k < DM_NSUM; ++k) v[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * DM_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * DM_WG) {
    const float g = gt[i];
    if (!(g > 0.f)) continue;
    const float e = est[i];
    const float d = logf(e) - logf(g);
    const float diff = g - e;
    const float sq = diff * diff;
    const float th = fmaxf(g / e, e / g);
    v[0] += 1.0;
    v[1] += d;
    v[2] += (double)(d * d);
    v[3] += fabsf(diff) / g;
    v[4] += sq / g;
    v[5] += sq;
    v[6] += fabsf(log10f(e) - log10f(g));
    v[7] += th < 1.25f ? 1.0 : 0.0;
    v[8] += th < 1.5625f ? 1.0 : 0.0;
    v[9] += th < 1.953125f ? 1.0 : 0.0;
  }
  const auto sum = block_tree_sum<DM_WG>(v);
  if (threadIdx.x < DM_NSUM) slots[(int64_t)blockIdx.x * DM_NSUM + threadIdx.x] = sum[threadIdx.x];
}

// out = silog_loss, then compute_errors: silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3
// saved (may be null): {n, mean d, sqrt(md2 - vf md^2)}, what silog_finalize_kernel (depth_train.hip) saves for silog_bwd_kernel, so
// out[0] is a training loss with ragmi_silog_loss_bwd as its backward.
// meter (may be null): the epoch's meter of search_epoch / search_eval (approaches/rag.py:401-427, 501-522) as 12 doubles, updated by
// this one thread after it stored `out`: meter[0..9] += the ten floats just stored (the reference adds per-batch floats; a batch with
// no valid pixel adds NaN, as numpy's mean of an empty selection does there), meter[10] += 1 (batches), meter[11] += n.
__global__ __launch_bounds__(DM_WG) void depth_metrics_finalize_kernel(const double* __restrict__ slots, int nslots, double variance_focus,
                                                                       float* __restrict__ out, double* __restrict__ saved,
                                                                       double* __restrict__ meter) {
  double v[DM_NSUM];
  gather_slots<DM_WG>(slots, nslots, v);
  const auto sum = block_tree_sum<DM_WG>(v);
  if (threadIdx.x == 0) {
    const double n = sum[0];                          // 0 masked pixels: every mean is 0/0 = NaN, as numpy's mean of an empty array
    const double md = sum[1] / n, md2 = sum[2] / n;
    const double sa = sqrt(md2 - variance_focus * md * md);
    out[0] = (float)(sa * 10.0);
    out[1] = (float)(sqrt(md2 - md * md) * 100.0);
    out[2] = (float)(sum[3] / n);
    out[3] = (float)(sum[6] / n);
    out[4] = (float)sqrt(sum[5] / n);
    out[5] = (float)(sum[4] / n);
    out[6] = (float)sqrt(md2);
    out[7] = (float)(sum[7] / n);
    out[8] = (float)(sum[8] / n);
    out[9] = (float)(sum[9] / n);
    if (saved) {
      saved[0] = n;
      saved[1] = md;
      saved[2] = sa;
    }
    if (meter) {
      for (int k = 0; k < DM_NSUM; ++k) meter[k] += (double)out[k];
      meter[10] += 1.0;
      meter[11] += n;
    }
  }
}

// the two launches of both entry points; `saved` / `meter` null: the finalize kernel stores `out` only
static int depth_metrics_launch(const void* est, const void* gt, long long n, float variance_focus, void* workspace, void* out10,
                                void* saved3, void* meter12, void* stream) {
  const int nslots = grid_stride_slots(n, DM_WG, DM_MAXWG);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(depth_metrics_kernel, dim3((unsigned)nslots), dim3(DM_WG), 0, st, (const float*)est, (const float*)gt, (int64_t)n,
                     (double*)workspace);
  hipLaunchKernelGGL(depth_metrics_finalize_kernel, dim3(1), dim3(DM_WG), 0, st, (const double*)workspace, nslots, (double)variance_focus,
                     (float*)out10, (double*)saved3, (double*)meter12);
  return check_launch("depth_metrics");
}

}  // namespace ragmi

extern "C" int ragmi_depth_metrics_workspace_elems(long long n) {
  using namespace ragmi;
  if (n <= 0) return 0;
  return grid_stride_slots(n, DM_WG, DM_MAXWG) * DM_NSUM * 2;        // one double (two floats) per partial
}

extern "C" int ragmi_depth_metrics_fwd(const void* est, const void* gt, long long n, float variance_focus, void* workspace, void* out10,
                                       int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(est && gt && workspace && out10, RAGMI_EINVAL, "depth_metrics: null pointer");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "depth_metrics: dtype %d not built (float32 only)", dtype);
  RAGMI_REQUIRE(n > 0, RAGMI_EINVAL, "depth_metrics: bad size %lld", n);
  RAGMI_REQUIRE(aligned_to(workspace, 8), RAGMI_EINVAL, "depth_metrics: workspace not 8-byte aligned");
  return depth_metrics_launch(est, gt, n, variance_focus, workspace, out10, nullptr, nullptr, stream);
}

extern "C" int ragmi_depth_metrics_meter_fwd(const void* est, const void* gt, long long n, float variance_focus, void* workspace,
                                             void* out10, void* saved3, void* meter12, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(est && gt && workspace && out10, RAGMI_EINVAL, "depth_metrics_meter: null pointer");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "depth_metrics_meter: dtype %d not built (float32 only)", dtype);
  RAGMI_REQUIRE(n > 0, RAGMI_EINVAL, "depth_metrics_meter: bad size %lld", n);
  RAGMI_REQUIRE(aligned_to(workspace, 8), RAGMI_EINVAL, "depth_metrics_meter: workspace not 8-byte aligned");
  RAGMI_REQUIRE(aligned_to(saved3, 8) && aligned_to(meter12, 8), RAGMI_EINVAL,
                "depth_metrics_meter: saved3 / meter12 not 8-byte aligned");
  return depth_metrics_launch(est, gt, n, variance_focus, workspace, out10, saved3, meter12, stream);
}
