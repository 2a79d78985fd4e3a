// Training the head's uncertainty: the adjoint of the statistics head (disp.hip, STATS = true) and the fused Laplace NLL loss.
//
// Adjoint.  With v_k the fine cost of a pixel, p = softmin(v), mu = sum p_k k, var = sum p_k (k - mu)^2, H = -sum p_k ln p_k,
// k* = argmax p, peak = p_k* and the cotangents (gmu, gV, gH, gP) of (disparity, variance, entropy, peak):
//   dL/dv_k = -p_k [ gmu (k - mu) + gV ((k - mu)^2 - var) - gH (ln p_k + H) - gP peak ] - [k = k*] gP peak
// Every term but the last is the softmax Jacobian applied to one per-sample function
//   f_k = gmu (k - mu) + gV (k - mu)^2 - gH ln p_k,     dL/dv_k = -p_k (f_k - F - gP peak) - [k = k*] gP peak,   F = sum p_k f_k
// because sum p (k - mu) = 0, sum p (k - mu)^2 = var and -sum p ln p = H.  So var and H are never formed: ONE extra sum, F, centred on
// mu itself (known after the softmax walk), where the raw second moment would subtract two numbers of ~maxdisp^2.
// The kernel keeps the shape of disp_softargmin_bwd_kernel (train.hip): a workgroup per 16 x 16 fine tile, the LDS tap table, the
// barrier-separated tile reduction and one global add per coarse cell and plane; the statistics take a second walk over the fine
// samples between the plain kernel's two passes.  Geometry, tap table and plane sampler are the shared parts of disp_common.h; the
// walk loops, the softmax step and the tile reduction are written out as in train.hip, because their shared forms measured slower
// here (profiles/disp_refactor_ab.json).
#include "disp_common.h"
#include "reduce.h"

namespace ragmi {

struct DispStatsBwdArgs {
  const float* cost;
  const float* dout;     // [B, Ho, Wo] or null
  const float* dstats;   // [B, 3, Ho, Wo] (variance, peak, entropy) or null
  float* dcost;
  DispGeom g;
};

__global__ __launch_bounds__(256) void disp_softargmin_stats_bwd_kernel(DispStatsBwdArgs a) {
  const DispGeom& g = a.g;
  extern __shared__ float4 ztab[];         // [maxdisp]: the fine-disparity taps, as in the forward kernel
  __shared__ float pix[DISP_BWD_T * DISP_BWD_T], colsum[DISP_BWD_T][DISP_BWD_WIN];
  __shared__ float wxw[DISP_BWD_T][DISP_BWD_WIN], wyw[DISP_BWD_T][DISP_BWD_WIN];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int tx = tid & (DISP_BWD_T - 1), ty = tid >> 4;
  const int ox = blockIdx.x * DISP_BWD_T + tx, oy = blockIdx.y * DISP_BWD_T + ty;
  const bool live = ox < g.Wo && oy < g.Ho;
  // window origin: the first coarse cell touched by the tile's first pixel (uniform over the workgroup)
  const int wy0 = lin_index(min(blockIdx.y * DISP_BWD_T, g.Ho - 1), g.h, g.Ho, g.sh, 0).i0;
  const int wx0 = lin_index(min(blockIdx.x * DISP_BWD_T, g.Wo - 1), g.w, g.Wo, g.sw, 0).i0;
  disp_fill_taps(ztab, g);
  if (tid < 2 * DISP_BWD_T) {                    // bilinear weights of the tile's columns (tid < 16) / rows onto the window
    const bool col = tid < DISP_BWD_T;
    const int k = tid & (DISP_BWD_T - 1);
    const int o = (col ? blockIdx.x : blockIdx.y) * DISP_BWD_T + k, n_out = col ? g.Wo : g.Ho;
    const LinIdx l = lin_index(min(o, n_out - 1), col ? g.w : g.h, n_out, col ? g.sw : g.sh, 0);
    const int j0 = l.i0 - (col ? wx0 : wy0), j1 = l.i1 - (col ? wx0 : wy0);
    for (int j = 0; j < DISP_BWD_WIN; ++j) {
      const float wv = o < n_out ? (j == j0 ? l.w0 : 0.f) + (j == j1 ? l.w1 : 0.f) : 0.f;
      if (col) wxw[k][j] = wv; else wyw[k][j] = wv;
    }
  }
  __syncthreads();
  const int hw = g.h * g.w;
  float* gbase = a.dcost + (int64_t)b * g.d * hw;
  const DispPlaneSampler<float> smp(a.cost + (int64_t)b * g.d * hw, g, min(oy, g.Ho - 1), min(ox, g.Wo - 1));
  // the pixel's four cotangents; a null plane is a zero plane, and pixels outside the image contribute nothing
  const int64_t npix = (int64_t)g.Ho * g.Wo, po = (int64_t)oy * g.Wo + ox;
  const float gmu = live && a.dout ? a.dout[b * npix + po] : 0.f;
  const float gV = live && a.dstats ? a.dstats[((int64_t)b * 3 + 0) * npix + po] : 0.f;
  const float gP = live && a.dstats ? a.dstats[((int64_t)b * 3 + 1) * npix + po] : 0.f;
  const float gH = live && a.dstats ? a.dstats[((int64_t)b * 3 + 2) * npix + po] : 0.f;
  constexpr float K = 1.4426950408889634f;
  // pass 1: softmax statistics (max, sum, expectation) exactly as the plain adjoint, and the first sample that holds the maximum
  float m = -INFINITY, s = 0.f, ws = 0.f;
  int kstar = 0;
  {
    int cz = 0;
    float b0 = smp.plane(0), b1 = smp.plane(g.d > 1 ? 1 : 0);
    for (int dd = 0; dd < g.maxdisp; ++dd) {
      const float4 tb = ztab[dd];
      const int i0 = (int)tb.x;
      while (i0 > cz) { ++cz; b0 = b1; b1 = smp.plane(cz + 1 < g.d ? cz + 1 : g.d - 1); }
      const float t = -fmaf(tb.y + tb.w, b0, tb.z * b1);
      const bool up = t > m;
      const float x = __builtin_amdgcn_exp2f((up ? m - t : t - m) * K);
      const float r = up ? x : 1.f, e = up ? 1.f : x;
      s = fmaf(s, r, e);
      ws = fmaf(ws, r, e * (float)dd);
      m = up ? t : m;
      kstar = up ? dd : kstar;
    }
  }
  const float mu = ws / s, ls = logf(s), rs = 1.f / s;
  // per-sample function of the statistics' cotangents, f_k = cV u^2 + cM u + cH (t - m) + cE with u = k - mu: ln p_k = (t - m) - ln s
  // costs no transcendental, and (t - m) is the exponent's own difference (formed before any scaling: no bits lost to |cost|)
  auto poly = [&](int dd, float tm, float cV, float cM, float cH, float cE) -> float {
    const float u = (float)dd - mu;
    return fmaf(cV * u, u, fmaf(cM, u, fmaf(cH, tm, cE)));
  };
  // pass 1b: F = sum p_k f_k.  Blocks of 8 samples folded into blocks of 64 folded into the total: a serial fp32 chain of 192 (639)
  // terms alone would spend the float64 gate's budget against ATen's pairwise sums, as the forward's moments did.
  float F;
  {
    float blk = 0.f, mid = 0.f, tot = 0.f;
    int cz = 0;
    float b0 = smp.plane(0), b1 = smp.plane(g.d > 1 ? 1 : 0);
    for (int dd = 0; dd < g.maxdisp; ++dd) {
      const float4 tb = ztab[dd];
      const int i0 = (int)tb.x;
      while (i0 > cz) { ++cz; b0 = b1; b1 = smp.plane(cz + 1 < g.d ? cz + 1 : g.d - 1); }
      const float t = -fmaf(tb.y + tb.w, b0, tb.z * b1);
      const float tm = t - m;
      blk = fmaf(__builtin_amdgcn_exp2f(tm * K), poly(dd, tm, gV, gmu, -gH, gH * ls), blk);
      if ((dd & 7) == 7) { mid += blk; blk = 0.f; }
      if ((dd & 63) == 63) { tot += mid; mid = 0.f; }
    }
    F = ((tot + mid) + blk) * rs;
  }
  const float gpk = gP * rs;               // gP * peak: the maximum's weight is 2^0 = 1
  // pass 2 evaluates -p_k (f_k - F - gP peak) = e_k q_k with the four coefficients of q scaled by -1/s once, here
  const float qV = -gV * rs, qM = -gmu * rs, qH = gH * rs, qE = (F + gpk - gH * ls) * rs;
  // one coarse plane's gradient: tile-wide reduction of the per-pixel values onto the window cells, then one global add per cell
  auto flush = [&](int z, float gv) {      // called by EVERY thread at the same point
    pix[tid] = gv;
    __syncthreads();
    if (tid < DISP_BWD_T * DISP_BWD_WIN) {             // (row r, window column j): sum over the row's 16 columns
      const int r = tid >> 3, j = tid & (DISP_BWD_WIN - 1);
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < DISP_BWD_T; ++c) acc = fmaf(wxw[c][j], pix[r * DISP_BWD_T + c], acc);
      colsum[r][j] = acc;
    }
    __syncthreads();
    if (tid < DISP_BWD_WIN * DISP_BWD_WIN) {           // (window row jy, window column jx): sum over the 16 rows
      const int jy = tid >> 3, jx = tid & (DISP_BWD_WIN - 1);
      float acc = 0.f;
#pragma unroll
      for (int r = 0; r < DISP_BWD_T; ++r) acc = fmaf(wyw[r][jy], colsum[r][jx], acc);
      const int cx = wx0 + jx, cy = wy0 + jy;
      if (acc != 0.f && cx < g.w && cy < g.h) atomicAdd(gbase + (int64_t)z * hw + cy * g.w + cx, acc);
    }
    // (the next flush writes pix only after its own barrier-separated readers are done, as in the plain adjoint)
  };
  // pass 2: walk the fine samples again; a0 / a1 collect the gradient of coarse planes cz / cz+1
  int cz = 0;
  float b0 = smp.plane(0), b1 = smp.plane(g.d > 1 ? 1 : 0);
  float a0 = 0.f, a1 = 0.f;
  for (int dd = 0; dd < g.maxdisp; ++dd) {
    const float4 tb = ztab[dd];
    const int i0 = (int)tb.x;
    while (i0 > cz) {                      // wave- and workgroup-uniform: the table is the same for every pixel
      flush(cz, a0); a0 = a1; a1 = 0.f;
      ++cz; b0 = b1; b1 = smp.plane(cz + 1 < g.d ? cz + 1 : g.d - 1);
    }
    const float t = -fmaf(tb.y + tb.w, b0, tb.z * b1);
    const float tm = t - m;
    const float gv = fmaf(__builtin_amdgcn_exp2f(tm * K), poly(dd, tm, qV, qM, qH, qE), dd == kstar ? -gpk : 0.f);   // dL / d v_fine, v = +cost (softMIN)
    a0 = fmaf(gv, tb.y + tb.w, a0);
    a1 = fmaf(gv, tb.z, a1);
  }
  flush(cz, a0);
  if (cz + 1 < g.d) flush(cz + 1, a1);
}

// ---------------------------------------------------------------------------------------------------------------
// Laplace-style NLL over the head's own variance (Kendall & Gal): per masked pixel (0 < gt < maxdisp), with s = variance + var_floor,
//   l = smooth_l1(est - gt) * rsqrt(s) + 0.5 ln s.
// Two-level reduction in the fixed order of reduce.h: workgroup (x, b) writes its four partial sums to slot (b * gridDim.x + x), the
// finalize workgroup adds the slots in double.
constexpr int UNC_N = 4;         // per slot: n_mask, sum l, sum smooth-L1, sum sqrt(s)
constexpr int UNC_GX = 64;       // at most this many workgroups per image

__global__ __launch_bounds__(256) void uncertainty_loss_kernel(const float* __restrict__ est, const float* __restrict__ stats,
                                                               const float* __restrict__ gt, int64_t hw, float maxdisp, float var_floor,
                                                               float* __restrict__ acc) {
  const int b = blockIdx.y;
  const float* pe = est + (int64_t)b * hw;
  const float* pv = stats + (int64_t)b * 3 * hw;      // plane 0: the variance
  const float* pg = gt + (int64_t)b * hw;
  float v[UNC_N] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const float g = pg[i];
    if (g > 0.f && g < maxdisp) {
      const float e = fabsf(pe[i] - g), sv = pv[i] + var_floor, sq = sqrtf(sv);
      const float sl1 = e < 1.f ? 0.5f * e * e : e - 0.5f;
      v[0] += 1.f;
      v[1] += fmaf(0.5f, logf(sv), sl1 / sq);
      v[2] += sl1;
      v[3] += sq;
    }
  }
  const auto sum = block_wave_sum(v);
  if (threadIdx.x < UNC_N) acc[((int64_t)b * gridDim.x + blockIdx.x) * UNC_N + threadIdx.x] = sum[threadIdx.x];
}

// out[0] = sum l / N, out[1] = masked smooth-L1 mean, out[2] = mean sqrt(s), out[3] = N; an empty mask gives 0 / 0 like stereo_metrics
__global__ __launch_bounds__(256) void uncertainty_loss_finalize_kernel(const float* __restrict__ acc, int nslots, float* __restrict__ out) {
  double v[UNC_N];
  gather_slots<256>(acc, nslots, v);
  const auto sum = block_tree_sum<256>(v);
  if (threadIdx.x == 0) {
    const double n = sum[0];
    out[0] = (float)(sum[1] / n);
    out[1] = (float)(sum[2] / n);
    out[2] = (float)(sum[3] / n);
    out[3] = (float)n;
  }
}

// d l / d est = clamp(est - gt, -1, 1) rsqrt(s) / N;  d l / d var = (0.5 / s - 0.5 smooth_l1 s^(-3/2)) / N;  zero off the mask and in
// the peak and entropy planes, which this launch writes too (no memset node in a captured step)
__global__ __launch_bounds__(256) void uncertainty_loss_bwd_kernel(const float* __restrict__ est, const float* __restrict__ stats,
                                                                   const float* __restrict__ gt, const float* __restrict__ out,
                                                                   const float* __restrict__ gout, float* __restrict__ ddisp,
                                                                   float* __restrict__ dstats, int64_t hw, float maxdisp, float var_floor) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int b = blockIdx.y;
  const float g = gt[(int64_t)b * hw + i], k = gout[0] / out[3];
  float dd = 0.f, dv = 0.f;
  if (g > 0.f && g < maxdisp) {
    const float df = est[(int64_t)b * hw + i] - g, e = fabsf(df), sv = stats[(int64_t)b * 3 * hw + i] + var_floor;
    const float sl1 = e < 1.f ? 0.5f * e * e : e - 0.5f, r = 1.f / sqrtf(sv);
    dd = k * (fminf(fmaxf(df, -1.f), 1.f) * r);
    dv = k * (0.5f * (1.f - sl1 * r) / sv);
  }
  ddisp[(int64_t)b * hw + i] = dd;
  float* const ps = dstats + (int64_t)b * 3 * hw + i;
  ps[0] = dv;
  ps[hw] = 0.f;
  ps[2 * hw] = 0.f;
}

}  // namespace ragmi

extern "C" int ragmi_disp_softargmin_stats_bwd(const void* cost, const void* dout, const void* dstats, void* dcost, int B, int d, int h,
                                               int w, int maxdisp, int Ho, int Wo, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(cost && dcost, RAGMI_EINVAL, "disp_softargmin_stats_bwd: null pointer");
  RAGMI_REQUIRE(dout || dstats, RAGMI_EINVAL, "disp_softargmin_stats_bwd: both cotangents are null");
  RAGMI_REQUIRE(B > 0 && d > 0 && h > 0 && w > 0 && maxdisp > 0 && Ho > 0 && Wo > 0 && B <= 65535, RAGMI_EINVAL,
                "disp_softargmin_stats_bwd: bad size");
  // the coarse window of a 16 x 16 fine tile must fit DISP_BWD_WIN cells per axis: holds for the x3 upsample of Disp (16/3 + 2 taps <= 8)
  RAGMI_REQUIRE(Ho == 3 * h && Wo == 3 * w, RAGMI_EUNSUPPORTED,
                "disp_softargmin_stats_bwd: built for the x3 upsample of Disp (Ho = 3h, Wo = 3w)");
  RAGMI_REQUIRE((int64_t)h * w < (1ll << 30), RAGMI_EUNSUPPORTED, "disp_softargmin_stats_bwd: size too large");
  const size_t lds = (size_t)maxdisp * sizeof(float4);
  RAGMI_REQUIRE(lds <= 48 * 1024, RAGMI_EUNSUPPORTED, "disp_softargmin_stats_bwd: maxdisp = %d exceeds the tap table (3072)", maxdisp);
  DispStatsBwdArgs a{(const float*)cost, (const float*)dout, (const float*)dstats, (float*)dcost, disp_geom(d, h, w, maxdisp, Ho, Wo)};
  hipLaunchKernelGGL(disp_softargmin_stats_bwd_kernel, dim3((unsigned)ceil_div(Wo, DISP_BWD_T), (unsigned)ceil_div(Ho, DISP_BWD_T), B), dim3(256), lds,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("disp_softargmin_stats_bwd");
}

extern "C" int64_t ragmi_uncertainty_loss_workspace_elems(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)ragmi::UNC_N * B * std::max<int64_t>(1, std::min<int64_t>(ragmi::ceil_div((int64_t)H * W, 1024), ragmi::UNC_GX));
}

extern "C" int ragmi_uncertainty_loss_fwd(const void* disp_est, const void* stats, const void* disp_gt, int B, int H, int W, float maxdisp,
                                          float var_floor, void* acc, void* out, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(disp_est && stats && disp_gt && acc && out, RAGMI_EINVAL, "uncertainty_loss: null pointer");
  RAGMI_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535, RAGMI_EINVAL, "uncertainty_loss: bad size");
  RAGMI_REQUIRE(var_floor > 0.f, RAGMI_EINVAL, "uncertainty_loss: var_floor must be positive (a variance of 0 has no logarithm)");
  const int64_t hw = (int64_t)H * W;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(hw, 1024), UNC_GX));
  hipLaunchKernelGGL(uncertainty_loss_kernel, dim3(gx, B), dim3(256), 0, st, (const float*)disp_est, (const float*)stats,
                     (const float*)disp_gt, hw, maxdisp, var_floor, (float*)acc);
  hipLaunchKernelGGL(uncertainty_loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)acc, (int)(gx * B), (float*)out);
  return check_launch("uncertainty_loss");
}

extern "C" int ragmi_uncertainty_loss_bwd(const void* disp_est, const void* stats, const void* disp_gt, const void* out, const void* gout,
                                          void* ddisp, void* dstats, int B, int H, int W, float maxdisp, float var_floor, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(disp_est && stats && disp_gt && out && gout && ddisp && dstats, RAGMI_EINVAL, "uncertainty_loss_bwd: null pointer");
  RAGMI_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535, RAGMI_EINVAL, "uncertainty_loss_bwd: bad size");
  RAGMI_REQUIRE(var_floor > 0.f, RAGMI_EINVAL, "uncertainty_loss_bwd: var_floor must be positive");
  const int64_t hw = (int64_t)H * W;
  hipLaunchKernelGGL(uncertainty_loss_bwd_kernel, dim3((unsigned)ceil_div(hw, 256), B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     (const float*)disp_est, (const float*)stats, (const float*)disp_gt, (const float*)out, (const float*)gout,
                     (float*)ddisp, (float*)dstats, hw, maxdisp, var_floor);
  return check_launch("uncertainty_loss_bwd");
}
