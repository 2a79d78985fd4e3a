// K2 — fused Disp.forward: trilinear x3 upsample (align_corners=False) -> Softmin over the
// disparity axis -> DisparityRegression.  Reference: src/models/rag_model.py:18-44.
//
// The reference materialises three [B,192,H,W] tensors (3.7 GB of traffic at the headline
// config); here each output pixel streams the d coarse planes once (4 bilinear taps per
// plane, L1/L2-served: neighbouring pixels share taps), lerps along the disparity axis in
// registers and keeps an online softmax (running max / sum / disparity-weighted sum).
// Algorithmic traffic: read d*h*w*4 B, write Ho*Wo*4 B per pair (15.5 MB at headline).
#include "common.h"

namespace ragmi {

struct DispArgs {
  const void* cost;   // [B, d, h, w], float or bf16_t
  float* out;         // [B, Ho, Wo]
  int d, h, w, maxdisp, Ho, Wo;
  float sd, sh, sw;
};

// Statistics of the softmin distribution p_k, formed in the pass that forms the disparity (the STATS = true instantiations; the
// STATS = false ones are the plain kernels: same arithmetic, registers and occupancy).  Per output pixel, with e_k = 2^(x_k) the unnormalised
// weights the kernels already hold (x_k <= 0 up to rounding) and s = sum e_k:
//   variance = sum p_k (k - disp)^2 = M2 / s - (M1 / s)^2,  M1 = sum e_k (k - pv), M2 = sum e_k (k - pv)^2 about a pivot pv NEAR THE
//              MODE.  The raw moment sum p k^2 - disp^2 subtracts two numbers of ~maxdisp^2 (6e-8 * 192^2 = 2e-3 px^2 of rounding, a
//              percent of a trained network's 1 - 10 px^2); about the pivot both are of the size of the variance itself.
//   peak     = max e_k / s
//   entropy  = -sum p_k ln p_k = ln s - ln 2 * (sum e_k x_k) / s      (both terms >= 0: no cancellation)
// stats: [B, 3, Ho, Wo] fp32, planes (variance, peak, entropy).
struct DispMoments {
  float pv = 0.f, m1 = 0.f, m2 = 0.f, xs = 0.f, pk = 0.f;
  // Sample fd with weight e = 2^x.  M1 and M2 run in three short chains (the tiled kernels: one per fine sample of a coarse plane)
  // that flush() folds into the totals every 8 coarse planes (the generic kernel: chain 0, every 16 samples).  On a BROAD distribution
  // the pivot can sit ~100 px from the mean, M2 / s is then 4 x the variance, and one serial fp32 chain of 192 terms loses 1e-6 of it -
  // the whole budget against ATen's pairwise sums; blocks of 8 terms and 8 block sums lose a third of that.  s and ws stay the serial
  // chains of the plain kernel (same bits).
  float b1[3] = {0.f, 0.f, 0.f}, b2[3] = {0.f, 0.f, 0.f};
  __device__ __forceinline__ void add_chain(int j, float e, float x, float fd) {
    const float t = fd - pv, et = e * t;
    b1[j] += et;
    b2[j] = fmaf(et, t, b2[j]);
    xs = fmaf(e, x, xs);
    pk = fmaxf(pk, e);
  }
  __device__ __forceinline__ void flush() {
    m1 += (b1[0] + b1[1]) + b1[2];
    m2 += (b2[0] + b2[1]) + b2[2];
    b1[0] = b1[1] = b1[2] = b2[0] = b2[1] = b2[2] = 0.f;
  }
  __device__ __forceinline__ void store(float* stats, int64_t b, int64_t npix, int64_t o, float s) const {
    const float c = m1 / s;                                              // disp - pv
    float* const p = stats + b * 3 * npix + o;
    p[0] = fmaxf(fmaf(-c, c, m2 / s), 0.f);
    p[npix] = pk / s;
    p[2 * npix] = fmaxf(fmaf(-0.6931471805599453f, xs / s, logf(s)), 0.f);
  }
};

// Mode-local regression (the MODE = true instantiations; they are STATS instantiations too).  k* is the fine index of the smallest
// upsampled cost (the lowest one on exact ties), W = {k : |k - k*| <= radius} clipped to [0, maxdisp) and not renormalised to a full
// width.  With the weights e_k the kernels already hold:
//   mode_mass = sum_W e_k / s,   mode_disp = k* + sum_W e_k (k - k*) / sum_W e_k       (about k*, as the moments run about their pivot)
// At a depth edge the softmin has two wells and out = sum p_k k lies between the two surfaces; mode_disp stays on the stronger one
// and mode_mass says how much of the distribution it speaks for.  mode: [B, 3, Ho, Wo] fp32, planes (index, disp, mass).
// Per fine sample: a subtract, a compare, a select and two accumulations.  The d = 64 register form then needs 103 VGPRs (the STATS one
// 95): no scratch, 4 waves per SIMD instead of 5; 42.7 -> 54.6 us at 384 x 1248.
struct DispWindow {
  float ks = 0.f, rf = 0.f, w0 = 0.f, w1 = 0.f;
  float c0[3] = {0.f, 0.f, 0.f}, c1[3] = {0.f, 0.f, 0.f};       // the chains and flush() cadence of DispMoments
  __device__ __forceinline__ void add_chain(int j, float e, float fd) {
    const float t = fd - ks, ew = fabsf(t) <= rf ? e : 0.f;
    c0[j] += ew;
    c1[j] = fmaf(ew, t, c1[j]);
  }
  __device__ __forceinline__ void flush() {
    w0 += (c0[0] + c0[1]) + c0[2];
    w1 += (c1[0] + c1[1]) + c1[2];
    c0[0] = c0[1] = c0[2] = c1[0] = c1[1] = c1[2] = 0.f;
  }
  __device__ __forceinline__ void store(float* mode, int64_t b, int64_t npix, int64_t o, float s) const {
    float* const p = mode + b * 3 * npix + o;
    p[0] = ks;
    p[npix] = w0 > 0.f ? ks + w1 / w0 : ks;
    p[2 * npix] = w0 / s;
  }
};

template <class T, bool STATS, bool MODE = false>
__device__ __forceinline__ void disp_softargmin_body(const DispArgs& a, float* stats, float* mode = nullptr, int radius = 0) {
  static_assert(STATS || !MODE, "the mode instantiations write the statistics too");
  extern __shared__ float4 ztab[];                 // [maxdisp]
  for (int dd = threadIdx.x; dd < a.maxdisp; dd += 256) {
    const LinIdx lz = lin_index(dd, a.d, a.maxdisp, a.sd, 0);
    const bool same = lz.i1 == lz.i0;
    ztab[dd] = make_float4((float)lz.i0, lz.w0, same ? 0.f : lz.w1, same ? lz.w1 : 0.f);
  }
  __syncthreads();
  const int64_t npix = (int64_t)a.Ho * a.Wo;
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= npix) return;
  const int b = blockIdx.y;
  const int ox = (int)(o % a.Wo), oy = (int)(o / a.Wo);
  const LinIdx ly = lin_index(oy, a.h, a.Ho, a.sh, 0);
  const LinIdx lx = lin_index(ox, a.w, a.Wo, a.sw, 0);
  const int hw = a.h * a.w;
  const T* base = static_cast<const T*>(a.cost) + (int64_t)b * a.d * hw;
  const int o00 = ly.i0 * a.w + lx.i0, o01 = ly.i0 * a.w + lx.i1;
  const int o10 = ly.i1 * a.w + lx.i0, o11 = ly.i1 * a.w + lx.i1;
  const float w00 = ly.w0 * lx.w0, w01 = ly.w0 * lx.w1, w10 = ly.w1 * lx.w0, w11 = ly.w1 * lx.w1;
  (void)w00; (void)w01; (void)w10; (void)w11;

  auto plane = [&](int z) -> float {  // bilinear sample of coarse plane z at (oy, ox); x innermost like ATen
    const T* p = base + (int64_t)z * hw;
    return lerp2(ly.w0, lerp2(lx.w0, ld(p + o00), lx.w1, ld(p + o01)), ly.w1, lerp2(lx.w0, ld(p + o10), lx.w1, ld(p + o11)));
  };

  // Walk the fine disparities in order; the coarse pair (cz, cz+1) only ever moves forward, so each
  // plane is sampled once.  Online softmax of -cost in base 2, branch-free:
  //   m' = max(m, t); s = s*2^((m-m')k) + 2^((t-m')k); differences are formed BEFORE scaling by k=log2(e)
  //   so large |cost| does not lose the bits that matter near the maximum.
  constexpr float K = 1.4426950408889634f;
  // The fine-disparity taps (i0, i1 == i0, w0, w1) are the same for every pixel: one table per workgroup in LDS instead
  // of ~12 VALU instructions of index arithmetic per fine sample per pixel (the kernel is VALU-bound).
  int cz = 0;
  float b0 = plane(0), b1 = plane(a.d > 1 ? 1 : 0);
  float m = -INFINITY, s = 0.f, ws = 0.f;
  DispMoments mo;
  for (int dd = 0; dd < a.maxdisp; ++dd) {
    const float4 tb = ztab[dd];                    // (i0, w0, w1 if i1 != i0 else 0, w1 if i1 == i0 else 0)
    const int i0 = (int)tb.x;
    while (i0 > cz) {   // rarely more than one step (only when down-sampling the disparity axis)
      ++cz;
      b0 = b1;
      b1 = plane(cz + 1 < a.d ? cz + 1 : a.d - 1);
    }
    const float t = -fmaf(tb.y + tb.w, b0, tb.z * b1);
    // one of (m - m'), (t - m') is exactly 0 and 2^0 is exactly 1: ONE transcendental per sample, the same bits as two
    const bool up = t > m;                                   // the running maximum moves
    const float xa = (up ? m - t : t - m) * K;
    const float x = __builtin_amdgcn_exp2f(xa);              // 2^(-inf) = 0 on the first sample
    const float r = up ? x : 1.f, e = up ? 1.f : x;
    if constexpr (STATS) {
      // There is no pass 1 here, so the pivot follows the running maximum.  When it moves to this sample (weight 1, exponent 0, offset
      // 0: it adds nothing to M1, M2, xs) the sums so far are re-centred about dd, re-based to the new maximum (every exponent drops
      // by xa = log2 r) and rescaled by r like s and ws:
      //   M2' = r (M2 - 2 dl M1 + dl^2 s),  M1' = r (M1 - dl s),  xs' = r (xs + xa s)      with dl = dd - pv and the OLD s.
      // The rounding of a re-centring is relative to the moments about the new pivot, and r <= 1 shrinks it with them.
      // Between moves the samples go into one block chain, folded into the totals every 16 samples and before a move (flush()):
      // d = 213 -> 639 fine samples in one serial chain lost more than the gate allows on a broad distribution.
      if (up) {
        mo.flush();
        const float dl = (float)dd - mo.pv;
        mo.m2 = x * fmaf(dl, fmaf(dl, s, -2.f * mo.m1), mo.m2);
        mo.m1 = x * fmaf(-dl, s, mo.m1);
        mo.xs = s > 0.f ? x * fmaf(xa, s, mo.xs) : 0.f;      // first sample: xa = -inf, s = 0
        mo.pv = (float)dd;
        mo.pk = 1.f;
      } else {
        mo.add_chain(0, x, xa, (float)dd);
      }
      if ((dd & 15) == 15) mo.flush();
    }
    s = fmaf(s, r, e);
    ws = fmaf(ws, r, e * (float)dd);
    m = up ? t : m;
  }
  a.out[(int64_t)b * npix + o] = ws / s;
  if constexpr (STATS) {
    mo.flush();
    mo.store(stats, b, npix, o, s);
  }
  if constexpr (MODE) {
    // k* is where the running maximum last moved (t > m is strict: the lowest index of equal costs), known only now: a second walk
    // over the at most 2 radius + 1 fine samples around it, with the taps, the plane clamping and the lerp of the walk above; the
    // weights are taken against the final maximum m.  One chain in blocks of 16 samples, as above.
    DispWindow wd;
    wd.ks = mo.pv;
    wd.rf = (float)radius;
    const int ks = (int)mo.pv, d_lo = max(ks - radius, 0), d_hi = min(ks + radius, a.maxdisp - 1);
    cz = (int)ztab[d_lo].x;
    b0 = plane(cz);
    b1 = plane(cz + 1 < a.d ? cz + 1 : a.d - 1);
    for (int dd = d_lo; dd <= d_hi; ++dd) {
      const float4 tb = ztab[dd];
      const int i0 = (int)tb.x;
      while (i0 > cz) {
        ++cz;
        b0 = b1;
        b1 = plane(cz + 1 < a.d ? cz + 1 : a.d - 1);
      }
      const float t = -fmaf(tb.y + tb.w, b0, tb.z * b1);
      wd.add_chain(0, __builtin_amdgcn_exp2f((t - m) * K), (float)dd);
      if (((dd - d_lo) & 15) == 15) wd.flush();
    }
    wd.flush();
    wd.store(mode, b, npix, o, s);
  }
}

template <class T>
__global__ __launch_bounds__(256) void disp_softargmin_kernel(DispArgs a) { disp_softargmin_body<T, false>(a, nullptr); }
template <class T>
__global__ __launch_bounds__(256) void disp_softargmin_stats_kernel(DispArgs a, float* stats) { disp_softargmin_body<T, true>(a, stats); }
template <class T>
__global__ __launch_bounds__(256) void disp_softargmin_mode_kernel(DispArgs a, float* stats, float* mode, int radius) {
  disp_softargmin_body<T, true, true>(a, stats, mode, radius);
}

// The reference's own shape — maxdisp = 3 d and a 3x spatial upsampling (rag_model.py:40, 272-273) — as a tiled, two-pass kernel.
//  * A workgroup owns 8 x 32 output pixels; the coarse cost block they interpolate from (d planes x 5 x 13 values) is staged through
//    LDS once: per pixel that replaces 4 d scattered global loads (every plane is a different cache line, the L1 misses them all)
//    by 4 d LDS reads.
//  * Pass 1 takes the minimum over the d bilinear plane samples: every fine sample is a convex combination of two neighbouring
//    planes, so -min is the softmin's largest exponent (up to rounding), which is all the max-subtraction needs.  Pass 2 walks the
//    planes again with a window (previous, current, next) and evaluates the three fine samples of coarse index k from it: lerp,
//    difference to the minimum, one exp2, two accumulations — 8 VALU instructions per sample instead of the ~14 of the online form
//    (compare / select / rescale), and no serial dependence on a running maximum.
//  * Tap table in LDS, built with the SAME lin_index arithmetic as the generic kernel: entry dd holds the weights of the three
//    window planes (one of them zero), so fp32 source indices that land a hair below an integer (i0 = k - 1, lambda ~ 1) are
//    reproduced exactly.  fmaf(wp, vp, fmaf(wc, vc, wn * vn)) with one zero weight is bit-identical to the generic kernel's
//    fmaf(w0, b0, w1 * b1).
constexpr int DX3_TY = 8, DX3_TX = 32, DX3_CR = 5, DX3_CC = 13, DX3_CP = DX3_CR * DX3_CC;

template <class T, bool STATS, bool MODE = false>
__device__ __forceinline__ void disp_softargmin_x3_body(const DispArgs& a, float* stats, float* mode = nullptr, int radius = 0) {
  static_assert(STATS || !MODE, "the mode instantiations write the statistics too");
  extern __shared__ __attribute__((aligned(16))) float dx3_lds[];
  float4* const ztab = reinterpret_cast<float4*>(dx3_lds);            // [maxdisp] (wp, wc, wn, dd)
  float* const tile = dx3_lds + 4 * a.maxdisp;                        // [d][5][13]
  const int tid = threadIdx.x, tx = tid % DX3_TX, ty = tid / DX3_TX;
  // XCD-aware tile order: workgroup j runs on XCD j % 8 (round-robin dispatch); every XCD walks one contiguous chunk of the
  // x-fastest tile list, so tiles that share coarse rows / columns of the cost meet in ONE L2.  With blockIdx.x = tile x the eight
  // neighbours of a tile sat on eight different XCDs and every L2 fetched its own copy of the shared halo: 77 MB from the memory
  // side for a 13.6 MB tensor (profiles/r04y_pmc_summary.txt).
  const int ntx = (a.Wo + DX3_TX - 1) / DX3_TX, nty = (a.Ho + DX3_TY - 1) / DX3_TY, ntile = ntx * nty;
  const int chunk = (ntile + 7) / 8, jb = blockIdx.x;
  const int tidx = (jb & 7) * chunk + (jb >> 3);
  if ((jb >> 3) >= chunk || tidx >= ntile) return;
  const int ox0 = (tidx % ntx) * DX3_TX, oy0 = (tidx / ntx) * DX3_TY, b = blockIdx.z;
  const int ox = min(ox0 + tx, a.Wo - 1), oy = min(oy0 + ty, a.Ho - 1);       // out-of-range threads shadow the last pixel, store nothing
  const int cy0 = lin_index(oy0, a.h, a.Ho, a.sh, 0).i0, cx0 = lin_index(ox0, a.w, a.Wo, a.sw, 0).i0;
  const int hw = a.h * a.w, D = a.d;
  const T* base = static_cast<const T*>(a.cost) + (int64_t)b * D * hw;
  for (int i = tid; i < D * DX3_CP; i += 256) {
    const int z = i / DX3_CP, r = i % DX3_CP;
    const int gy = min(cy0 + r / DX3_CC, a.h - 1), gx = min(cx0 + r % DX3_CC, a.w - 1);
    tile[i] = ld(base + (int64_t)z * hw + gy * a.w + gx);
  }
  for (int dd = tid; dd < a.maxdisp; dd += 256) {
    const LinIdx lz = lin_index(dd, D, a.maxdisp, a.sd, 0);
    const int k = dd / 3;
    float4 e = make_float4(0.f, 0.f, 0.f, (float)dd);
    if (lz.i0 < k) { e.x = lz.w0; e.y = lz.w1; }                      // planes (k-1, k)
    else if (lz.i1 != lz.i0) { e.y = lz.w0; e.z = lz.w1; }            // planes (k, k+1)
    else e.y = lz.w0 + lz.w1;                                         // clamped at the last plane
    ztab[dd] = e;
  }
  const LinIdx ly = lin_index(oy, a.h, a.Ho, a.sh, 0);
  const LinIdx lx = lin_index(ox, a.w, a.Wo, a.sw, 0);
  // the four corners' LDS addresses: a plane is then four reads at a common (compile-time, once unrolled) offset
  const float* const t00 = tile + (ly.i0 - cy0) * DX3_CC + (lx.i0 - cx0);
  const float* const t01 = t00 + (lx.i1 - lx.i0);
  const float* const t10 = t00 + (ly.i1 - ly.i0) * DX3_CC;
  const float* const t11 = t10 + (lx.i1 - lx.i0);
  __syncthreads();
  auto plane = [&](int z) {                  // bilinear sample of coarse plane z at (oy, ox); x innermost like ATen
    const int o = z * DX3_CP;
    return lerp2(ly.w0, lerp2(lx.w0, t00[o], lx.w1, t01[o]), ly.w1, lerp2(lx.w0, t10[o], lx.w1, t11[o]));
  };
  constexpr float K = 1.4426950408889634f;
  float s = 0.f, ws = 0.f;
  // STATS: the coarse arg-min of pass 1 gives the pivot of the moments, fine sample 3 argmin + 1 (the one whose source index IS that
  // plane); the softmin's mode is within a coarse step of it
  DispMoments mo;
  int am = 0;
  // MODE: fine sample 3 am + 1 sits exactly on plane am, the smallest of the planes every fine sample is a convex combination of, so
  // k* = 3 am + 1 - except am == 0: the source index is clamped at 0, fine samples 0 and 1 both evaluate to v[0], and k* = 0
  DispWindow wd;
  wd.rf = (float)radius;
  // d = 64 (maxdisp 192, the reference's only configuration, rag_model.py:274): the 64 plane samples of pass 1 stay in REGISTERS for
  // pass 2 — no second round of 4 d LDS reads and bilinear arithmetic (same operations on the same values: identical bits).  Chunks
  // of 8 planes fenced by sched_barrier: unfenced, the scheduler hoisted all 256 operand reads and the kernel spilled or ran at
  // 87 us (round 2).  Same box, both builds: 49.9 -> 40.3 us (90 VGPRs, 5 waves per SIMD).
  if (D == 64) {
    float v[64];
    float lo = INFINITY;
#pragma unroll
    for (int z = 0; z < 64; ++z) {
      v[z] = plane(z);
      lo = fminf(lo, v[z]);
      if ((z & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (STATS) {    // the arg-min from the FINAL minimum: tracked inside the loop above, every running minimum stayed live (142 VGPRs)
#pragma unroll
      for (int z = 63; z >= 0; --z) am = v[z] == lo ? z : am;
      mo.pv = (float)(3 * am + 1);
      if constexpr (MODE) wd.ks = am == 0 ? 0.f : mo.pv;
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const float vp_ = v[k > 0 ? k - 1 : 0], vc_ = v[k], vn_ = v[k < 63 ? k + 1 : 63];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float4 tb = ztab[3 * k + j];
        const float c = fmaf(tb.x, vp_, fmaf(tb.y, vc_, tb.z * vn_));
        const float x = (lo - c) * K;
        const float e = __builtin_amdgcn_exp2f(x);
        s += e;
        ws = fmaf(e, tb.w, ws);
        if constexpr (STATS) mo.add_chain(j, e, x, tb.w);
        if constexpr (MODE) wd.add_chain(j, e, tb.w);
      }
      if ((k & 7) == 7) {
        if constexpr (STATS) mo.flush();
        if constexpr (MODE) wd.flush();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
  float lo = INFINITY;
#pragma clang loop unroll_count(4) vectorize(disable)
  for (int z = 0; z < D; ++z) {
    const float vz = plane(z);
    if constexpr (STATS) am = vz < lo ? z : am;
    lo = fminf(lo, vz);
  }
  if constexpr (STATS) mo.pv = (float)(3 * am + 1);
  if constexpr (MODE) wd.ks = am == 0 ? 0.f : mo.pv;
  // exponent of a sample: (min - cost) * K: the difference is formed BEFORE the scaling by K, like the generic kernel, so large
  // |cost| does not lose the bits that matter near the minimum
  float vc = plane(0), vp = vc, vn = plane(min(1, D - 1));
  for (int k = 0; k < D; ++k) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float4 tb = ztab[3 * k + j];     // wave-uniform address: one broadcast read
      const float c = fmaf(tb.x, vp, fmaf(tb.y, vc, tb.z * vn));
      const float x = (lo - c) * K;
      const float e = __builtin_amdgcn_exp2f(x);
      s += e;
      ws = fmaf(e, tb.w, ws);
      if constexpr (STATS) mo.add_chain(j, e, x, tb.w);
      if constexpr (MODE) wd.add_chain(j, e, tb.w);
    }
    vp = vc; vc = vn; vn = plane(min(k + 2, D - 1));
    if constexpr (STATS) if ((k & 7) == 7) mo.flush();
    if constexpr (MODE) if ((k & 7) == 7) wd.flush();
  }
  if constexpr (STATS) mo.flush();
  if constexpr (MODE) wd.flush();
  }
  if (ox0 + tx < a.Wo && oy0 + ty < a.Ho) {
    a.out[(int64_t)b * a.Ho * a.Wo + (int64_t)oy * a.Wo + ox] = ws / s;
    if constexpr (STATS) mo.store(stats, b, (int64_t)a.Ho * a.Wo, (int64_t)oy * a.Wo + ox, s);
    if constexpr (MODE) wd.store(mode, b, (int64_t)a.Ho * a.Wo, (int64_t)oy * a.Wo + ox, s);
  }
}

template <class T>
__global__ __launch_bounds__(256) void disp_softargmin_x3_kernel(DispArgs a) { disp_softargmin_x3_body<T, false>(a, nullptr); }
template <class T>
__global__ __launch_bounds__(256) void disp_softargmin_x3_stats_kernel(DispArgs a, float* stats) { disp_softargmin_x3_body<T, true>(a, stats); }
template <class T>
__global__ __launch_bounds__(256) void disp_softargmin_x3_mode_kernel(DispArgs a, float* stats, float* mode, int radius) {
  disp_softargmin_x3_body<T, true, true>(a, stats, mode, radius);
}

// The wavefront-reduction form north_star names, for the same configuration (maxdisp = 3 d, 3x upsampling): 16 lanes share one
// output pixel, lane l owns the coarse planes 4l .. 4l+3 (d <= 64) and their 12 fine samples; a wave step is 4 pixels.
//  * per step a lane takes 4 bilinear plane samples (16 LDS reads — the thread-per-pixel form makes 2 x 4 d = 512 per pixel, plus a
//    broadcast tap-table read per fine sample) and gets the two neighbouring planes' samples from the lanes beside it (DPP row shifts);
//  * its 12 (wp, wc, wn, dd) tap entries are per-lane constants of the whole launch (registers), built with the same lin_index
//    arithmetic as the tap table of the tiled kernel;
//  * minimum, sum of exponentials and weighted sum are reduced over the 16 lanes of a DPP row (4 steps each, no LDS).
// Same reference exponent (the minimum over the coarse plane samples) and the same per-sample arithmetic as the tiled kernel; only
// the order of the two final sums differs (per lane, then across lanes).
__device__ __forceinline__ float dpp_row_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));     // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));     // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));    // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));    // row_mirror
  return v;
}
__device__ __forceinline__ float dpp_row_min(float v) {
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false)));
  return v;
}

template <class T>
__global__ __launch_bounds__(256) void disp_softargmin_wave_kernel(DispArgs a) {
  extern __shared__ __attribute__((aligned(16))) float dxw_lds[];
  float* const tile = dxw_lds;                                         // [d][5][13]: plane stride 65 = 1 mod 32
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 15, pq = lane >> 4;
  const int ox0 = blockIdx.x * DX3_TX, oy0 = blockIdx.y * DX3_TY, b = blockIdx.z;
  const int cy0 = lin_index(oy0, a.h, a.Ho, a.sh, 0).i0, cx0 = lin_index(ox0, a.w, a.Wo, a.sw, 0).i0;
  const int hw = a.h * a.w, D = a.d;
  const T* base = static_cast<const T*>(a.cost) + (int64_t)b * D * hw;
  for (int i = tid; i < D * DX3_CP; i += 256) {
    const int z = i / DX3_CP, r = i % DX3_CP;
    const int gy = min(cy0 + r / DX3_CC, a.h - 1), gx = min(cx0 + r % DX3_CC, a.w - 1);
    tile[i] = ld(base + (int64_t)z * hw + gy * a.w + gx);
  }
  // lane l owns the coarse planes k = l + 16 q (q = 0..3): the 16 lanes of a pixel read 16 CONSECUTIVE planes at a time, one bank
  // each.  Its 12 fine samples dd = 3 k + j: weights of the window (plane k-1, k, k+1) — per-lane constants of the launch
  float wp[12], wc[12], wn[12], fd[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const int k = l + 16 * (i / 3), dd = 3 * k + i % 3;
    const LinIdx lz = lin_index(min(dd, a.maxdisp - 1), D, a.maxdisp, a.sd, 0);
    wp[i] = wc[i] = wn[i] = 0.f;
    fd[i] = (float)dd;
    if (k < D && dd < a.maxdisp) {
      if (lz.i0 < k) { wp[i] = lz.w0; wc[i] = lz.w1; }
      else if (lz.i1 != lz.i0) { wc[i] = lz.w0; wn[i] = lz.w1; }
      else wc[i] = lz.w0 + lz.w1;
    }
  }
  __syncthreads();
  constexpr float K = 1.4426950408889634f;
  for (int step = 0; step < 16; ++step) {
    const int idx = step * 4 + pq, ty = wave * 2 + (idx >> 5), tx = idx & 31;
    const int ox = min(ox0 + tx, a.Wo - 1), oy = min(oy0 + ty, a.Ho - 1);
    const LinIdx ly = lin_index(oy, a.h, a.Ho, a.sh, 0);
    const LinIdx lx = lin_index(ox, a.w, a.Wo, a.sw, 0);
    const float* const t00 = tile + (ly.i0 - cy0) * DX3_CC + (lx.i0 - cx0);
    const int o01 = lx.i1 - lx.i0, o10 = (ly.i1 - ly.i0) * DX3_CC;
    float v[4], vm[4], vx[4];
    float lo = INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = l + 16 * q;
      const float* const t = t00 + min(k, D - 1) * DX3_CP;
      v[q] = lerp2(ly.w0, lerp2(lx.w0, t[0], lx.w1, t[o01]), ly.w1, lerp2(lx.w0, t[o10], lx.w1, t[o10 + o01]));
      lo = k < D ? fminf(lo, v[q]) : lo;
    }
    // plane k-1 / k+1: the lane before / after in the pixel's row, same q — across the row's ends it is q -/+ 1 of the lane at the other end
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      vm[q] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[q]), 0x121, 0xF, 0xF, false));   // row_ror:1: lane l <- lane l-1 (0 <- 15)
      vx[q] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[q]), 0x12F, 0xF, 0xF, false));   // row_ror:15: lane l <- lane l+1 (15 <- 0)
    }
    lo = dpp_row_min(lo);
    float s = 0.f, ws = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int q = i / 3;
      const float vp_ = l == 0 ? (q == 0 ? v[0] : vm[q - 1]) : vm[q];         // (plane -1 does not exist: its weight is 0)
      const float vn_ = l == 15 ? (q == 3 ? v[3] : vx[q + 1]) : vx[q];
      const float c = fmaf(wp[i], vp_, fmaf(wc[i], v[q], wn[i] * vn_));
      float e = __builtin_amdgcn_exp2f((lo - c) * K);
      e = (wp[i] + wc[i] + wn[i]) > 0.f ? e : 0.f;                     // samples past maxdisp / the volume (d < 64)
      s += e;
      ws = fmaf(e, fd[i], ws);
    }
    s = dpp_row_sum(s);
    ws = dpp_row_sum(ws);
    if (l == 0 && ox0 + tx < a.Wo && oy0 + ty < a.Ho) a.out[(int64_t)b * a.Ho * a.Wo + (int64_t)oy * a.Wo + ox] = ws / s;
  }
}

// standalone DisparityRegression: out = sum_d prob[:, d] * d
template <class T>
__global__ __launch_bounds__(256) void disparity_regression_kernel(const T* __restrict__ prob, float* __restrict__ out,
                                                                  int D, int64_t hw) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= hw) return;
  const int b = blockIdx.y;
  const T* p = prob + (int64_t)b * D * hw + o;
  float acc = 0.f;
#pragma unroll 8
  for (int dd = 0; dd < D; ++dd) acc = fmaf(ld(p + (int64_t)dd * hw), (float)dd, acc);
  out[(int64_t)b * hw + o] = acc;
}

// DisparityRegression with the statistics of `prob`, taken as given (not renormalised): out as above (the same fmaf chain, the same
// bits), variance = sum p (k - out)^2 by the definition in a second walk over the D planes (a one-hot prob gives exactly 0: out is
// exactly its index), peak = max p, entropy = -sum_{p > 0} p ln p.  The two stat sums run in 8 interleaved partial sums: there is no
// interpolation error to hide behind here, and a serial fp32 sum of 192 terms alone is ~5e-7 of the result.
// MODE: k* is the first arg-max of prob (found in the statistics walk: strictly greater moves it), and a third walk over the window
// |k - k*| <= radius alone sums prob and prob (k - k*), in 8 interleaved partial sums again: mode = (k*, k* + sum p (k - k*) / sum p,
// sum p), and a window without mass gives mode_disp = k*.  A one-hot prob gives (its index, its index, 1) exactly.
template <class T, bool MODE>
__device__ __forceinline__ void disparity_regression_stats_body(const T* __restrict__ prob, float* __restrict__ out, float* __restrict__ stats,
                                                                int D, int64_t hw, float* __restrict__ mode = nullptr, int radius = 0) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= hw) return;
  const int b = blockIdx.y;
  const T* p = prob + (int64_t)b * D * hw + o;
  float acc = 0.f;
#pragma unroll 8
  for (int dd = 0; dd < D; ++dd) acc = fmaf(ld(p + (int64_t)dd * hw), (float)dd, acc);
  float var[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ent[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, pk = 0.f;
  float best = -INFINITY;
  int ks = 0;
  for (int d0 = 0; d0 < D; d0 += 8) {
    static_for<8>([&](auto J) {
      constexpr int j = decltype(J)::value;
      if (d0 + j < D) {
        const float q = ld(p + (int64_t)(d0 + j) * hw), t = (float)(d0 + j) - acc;
        var[j] = fmaf(q * t, t, var[j]);
        ent[j] = q > 0.f ? fmaf(q, logf(q), ent[j]) : ent[j];
        pk = fmaxf(pk, q);
        if constexpr (MODE) {
          if (q > best) {
            best = q;
            ks = d0 + j;
          }
        }
      }
    });
  }
  out[(int64_t)b * hw + o] = acc;
  float* const st = stats + (int64_t)b * 3 * hw + o;
  st[0] = ((var[0] + var[1]) + (var[2] + var[3])) + ((var[4] + var[5]) + (var[6] + var[7]));
  st[hw] = pk;
  st[2 * hw] = 0.f - (((ent[0] + ent[1]) + (ent[2] + ent[3])) + ((ent[4] + ent[5]) + (ent[6] + ent[7])));
  if constexpr (MODE) {
    float w0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, w1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int d_lo = max(ks - radius, 0), d_hi = min(ks + radius, D - 1);
    for (int d0 = d_lo; d0 <= d_hi; d0 += 8) {
      static_for<8>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if (d0 + j <= d_hi) {
          const float q = ld(p + (int64_t)(d0 + j) * hw);
          w0[j] += q;
          w1[j] = fmaf(q, (float)(d0 + j - ks), w1[j]);
        }
      });
    }
    const float m0 = ((w0[0] + w0[1]) + (w0[2] + w0[3])) + ((w0[4] + w0[5]) + (w0[6] + w0[7]));
    const float m1 = ((w1[0] + w1[1]) + (w1[2] + w1[3])) + ((w1[4] + w1[5]) + (w1[6] + w1[7]));
    float* const mp = mode + (int64_t)b * 3 * hw + o;
    mp[0] = (float)ks;
    mp[hw] = m0 != 0.f ? (float)ks + m1 / m0 : (float)ks;
    mp[2 * hw] = m0;
  }
}

template <class T>
__global__ __launch_bounds__(256) void disparity_regression_stats_kernel(const T* __restrict__ prob, float* __restrict__ out,
                                                                        float* __restrict__ stats, int D, int64_t hw) {
  disparity_regression_stats_body<T, false>(prob, out, stats, D, hw);
}
template <class T>
__global__ __launch_bounds__(256) void disparity_regression_mode_kernel(const T* __restrict__ prob, float* __restrict__ out,
                                                                       float* __restrict__ stats, float* __restrict__ mode, int D, int64_t hw,
                                                                       int radius) {
  disparity_regression_stats_body<T, true>(prob, out, stats, D, hw, mode, radius);
}

}  // namespace ragmi

extern "C" int ragmi_disp_softargmin_fwd(const void* cost, void* out, int B, int d, int h, int w, int maxdisp, int Ho,
                                         int Wo, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(cost && out, RAGMI_EINVAL, "disp_softargmin: null pointer");
  RAGMI_REQUIRE(B > 0 && d > 0 && h > 0 && w > 0 && maxdisp > 0 && Ho > 0 && Wo > 0, RAGMI_EINVAL,
                "disp_softargmin: non-positive size");
  RAGMI_REQUIRE(dtype_ok(dtype), RAGMI_EUNSUPPORTED, "disp_softargmin: dtype %d not built", dtype);
  RAGMI_REQUIRE(B <= 65535 && (int64_t)h * w < (1ll << 30), RAGMI_EUNSUPPORTED, "disp_softargmin: size too large");
  DispArgs a{cost, (float*)out, d, h, w, maxdisp, Ho, Wo,
             lin_scale(d, maxdisp, 0), lin_scale(h, Ho, 0), lin_scale(w, Wo, 0)};
  dim3 grid((unsigned)ceil_div((int64_t)Ho * Wo, 256), B);
  const size_t lds = (size_t)maxdisp * sizeof(float4);
  RAGMI_REQUIRE(lds <= 64 * 1024, RAGMI_EUNSUPPORTED, "disp_softargmin: maxdisp %d exceeds the tap table (4096)", maxdisp);
  const size_t lds3 = lds + (size_t)d * DX3_CP * sizeof(float);
  if (maxdisp == 3 * d && Ho == 3 * h && Wo == 3 * w && lds3 <= 64 * 1024) {   // the reference's configuration (rag_model.py:40, 272-273): the tiled form
    const dim3 g3((unsigned)ceil_div(Wo, DX3_TX), (unsigned)ceil_div(Ho, DX3_TY), (unsigned)B);
    const dim3 g1((unsigned)(ceil_div((int64_t)g3.x * g3.y, 8) * 8), 1, (unsigned)B);      // the tiled kernel decodes its tile itself (XCD-aware)
#ifdef RAGMI_DISP_WAVE      // A/B build (tools/build_variant.sh): the wavefront-reduction form, d <= 64
    if (d <= 64) {
      const size_t ldsw = (size_t)d * DX3_CP * sizeof(float);
      if (dtype == RAGMI_BF16) hipLaunchKernelGGL(disp_softargmin_wave_kernel<bf16_t>, g3, dim3(256), ldsw, static_cast<hipStream_t>(stream), a);
      else hipLaunchKernelGGL(disp_softargmin_wave_kernel<float>, g3, dim3(256), ldsw, static_cast<hipStream_t>(stream), a);
      return check_launch("disp_softargmin");
    }
#endif
    if (dtype == RAGMI_BF16) hipLaunchKernelGGL(disp_softargmin_x3_kernel<bf16_t>, g1, dim3(256), lds3, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL(disp_softargmin_x3_kernel<float>, g1, dim3(256), lds3, static_cast<hipStream_t>(stream), a);
    return check_launch("disp_softargmin");
  }
  if (dtype == RAGMI_BF16) hipLaunchKernelGGL(disp_softargmin_kernel<bf16_t>, grid, dim3(256), lds, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(disp_softargmin_kernel<float>, grid, dim3(256), lds, static_cast<hipStream_t>(stream), a);
  return check_launch("disp_softargmin");
}

extern "C" int ragmi_disparity_regression_fwd(const void* prob, void* out, int B, int D, int H, int W, int dtype,
                                              void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(prob && out, RAGMI_EINVAL, "disparity_regression: null pointer");
  RAGMI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, RAGMI_EINVAL, "disparity_regression: non-positive size");
  RAGMI_REQUIRE(dtype_ok(dtype), RAGMI_EUNSUPPORTED, "disparity_regression: dtype %d not built", dtype);
  RAGMI_REQUIRE(B <= 65535, RAGMI_EUNSUPPORTED, "disparity_regression: B too large");
  const int64_t hw = (int64_t)H * W;
  dim3 grid((unsigned)ceil_div(hw, 256), B);
  if (dtype == RAGMI_BF16)
    hipLaunchKernelGGL(disparity_regression_kernel<bf16_t>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), (const bf16_t*)prob, (float*)out, D, hw);
  else
    hipLaunchKernelGGL(disparity_regression_kernel<float>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), (const float*)prob, (float*)out, D, hw);
  return check_launch("disparity_regression");
}

// The statistics launches: the argument checks, the dispatch rule and the launch geometry of the plain entry points above, one launch each.
extern "C" int ragmi_disp_softargmin_stats_fwd(const void* cost, void* out, void* stats, int B, int d, int h, int w, int maxdisp,
                                               int Ho, int Wo, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(cost && out && stats, RAGMI_EINVAL, "disp_softargmin_stats: null pointer");
  RAGMI_REQUIRE(B > 0 && d > 0 && h > 0 && w > 0 && maxdisp > 0 && Ho > 0 && Wo > 0, RAGMI_EINVAL,
                "disp_softargmin_stats: non-positive size");
  RAGMI_REQUIRE(dtype_ok(dtype), RAGMI_EUNSUPPORTED, "disp_softargmin_stats: dtype %d not built", dtype);
  RAGMI_REQUIRE(B <= 65535 && (int64_t)h * w < (1ll << 30), RAGMI_EUNSUPPORTED, "disp_softargmin_stats: size too large");
  DispArgs a{cost, (float*)out, d, h, w, maxdisp, Ho, Wo,
             lin_scale(d, maxdisp, 0), lin_scale(h, Ho, 0), lin_scale(w, Wo, 0)};
  float* const st = (float*)stats;
  const hipStream_t q = static_cast<hipStream_t>(stream);
  dim3 grid((unsigned)ceil_div((int64_t)Ho * Wo, 256), B);
  const size_t lds = (size_t)maxdisp * sizeof(float4);
  RAGMI_REQUIRE(lds <= 64 * 1024, RAGMI_EUNSUPPORTED, "disp_softargmin_stats: maxdisp %d exceeds the tap table (4096)", maxdisp);
  const size_t lds3 = lds + (size_t)d * DX3_CP * sizeof(float);
  if (maxdisp == 3 * d && Ho == 3 * h && Wo == 3 * w && lds3 <= 64 * 1024) {   // the tiled form (register form at d = 64, else the rolling window)
    const dim3 g3((unsigned)ceil_div(Wo, DX3_TX), (unsigned)ceil_div(Ho, DX3_TY), (unsigned)B);
    const dim3 g1((unsigned)(ceil_div((int64_t)g3.x * g3.y, 8) * 8), 1, (unsigned)B);
    if (dtype == RAGMI_BF16) hipLaunchKernelGGL(disp_softargmin_x3_stats_kernel<bf16_t>, g1, dim3(256), lds3, q, a, st);
    else hipLaunchKernelGGL(disp_softargmin_x3_stats_kernel<float>, g1, dim3(256), lds3, q, a, st);
    return check_launch("disp_softargmin_stats");
  }
  if (dtype == RAGMI_BF16) hipLaunchKernelGGL(disp_softargmin_stats_kernel<bf16_t>, grid, dim3(256), lds, q, a, st);
  else hipLaunchKernelGGL(disp_softargmin_stats_kernel<float>, grid, dim3(256), lds, q, a, st);
  return check_launch("disp_softargmin_stats");
}

extern "C" int ragmi_disparity_regression_stats_fwd(const void* prob, void* out, void* stats, int B, int D, int H, int W, int dtype,
                                                    void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(prob && out && stats, RAGMI_EINVAL, "disparity_regression_stats: null pointer");
  RAGMI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, RAGMI_EINVAL, "disparity_regression_stats: non-positive size");
  RAGMI_REQUIRE(dtype_ok(dtype), RAGMI_EUNSUPPORTED, "disparity_regression_stats: dtype %d not built", dtype);
  RAGMI_REQUIRE(B <= 65535, RAGMI_EUNSUPPORTED, "disparity_regression_stats: B too large");
  const int64_t hw = (int64_t)H * W;
  dim3 grid((unsigned)ceil_div(hw, 256), B);
  if (dtype == RAGMI_BF16)
    hipLaunchKernelGGL(disparity_regression_stats_kernel<bf16_t>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), (const bf16_t*)prob, (float*)out, (float*)stats, D, hw);
  else
    hipLaunchKernelGGL(disparity_regression_stats_kernel<float>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), (const float*)prob, (float*)out, (float*)stats, D, hw);
  return check_launch("disparity_regression_stats");
}

// The mode launches: the argument checks, the dispatch rule and the launch geometry of the statistics entry points above, one launch
// each; radius is a run-time argument of the kernels.
extern "C" int ragmi_disp_softargmin_mode_fwd(const void* cost, void* out, void* stats, void* mode, int B, int d, int h, int w,
                                              int maxdisp, int Ho, int Wo, int radius, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(cost && out && stats && mode, RAGMI_EINVAL, "disp_softargmin_mode: null pointer");
  RAGMI_REQUIRE(B > 0 && d > 0 && h > 0 && w > 0 && maxdisp > 0 && Ho > 0 && Wo > 0, RAGMI_EINVAL,
                "disp_softargmin_mode: non-positive size");
  RAGMI_REQUIRE(radius >= 0 && radius <= maxdisp, RAGMI_EINVAL, "disp_softargmin_mode: radius %d not in [0, maxdisp = %d]", radius, maxdisp);
  RAGMI_REQUIRE(dtype_ok(dtype), RAGMI_EUNSUPPORTED, "disp_softargmin_mode: dtype %d not built", dtype);
  RAGMI_REQUIRE(B <= 65535 && (int64_t)h * w < (1ll << 30), RAGMI_EUNSUPPORTED, "disp_softargmin_mode: size too large");
  DispArgs a{cost, (float*)out, d, h, w, maxdisp, Ho, Wo,
             lin_scale(d, maxdisp, 0), lin_scale(h, Ho, 0), lin_scale(w, Wo, 0)};
  float* const st = (float*)stats;
  float* const md = (float*)mode;
  const hipStream_t q = static_cast<hipStream_t>(stream);
  dim3 grid((unsigned)ceil_div((int64_t)Ho * Wo, 256), B);
  const size_t lds = (size_t)maxdisp * sizeof(float4);
  RAGMI_REQUIRE(lds <= 64 * 1024, RAGMI_EUNSUPPORTED, "disp_softargmin_mode: maxdisp %d exceeds the tap table (4096)", maxdisp);
  const size_t lds3 = lds + (size_t)d * DX3_CP * sizeof(float);
  if (maxdisp == 3 * d && Ho == 3 * h && Wo == 3 * w && lds3 <= 64 * 1024) {   // the tiled form (register form at d = 64, else the rolling window)
    const dim3 g3((unsigned)ceil_div(Wo, DX3_TX), (unsigned)ceil_div(Ho, DX3_TY), (unsigned)B);
    const dim3 g1((unsigned)(ceil_div((int64_t)g3.x * g3.y, 8) * 8), 1, (unsigned)B);
    if (dtype == RAGMI_BF16) hipLaunchKernelGGL(disp_softargmin_x3_mode_kernel<bf16_t>, g1, dim3(256), lds3, q, a, st, md, radius);
    else hipLaunchKernelGGL(disp_softargmin_x3_mode_kernel<float>, g1, dim3(256), lds3, q, a, st, md, radius);
    return check_launch("disp_softargmin_mode");
  }
  if (dtype == RAGMI_BF16) hipLaunchKernelGGL(disp_softargmin_mode_kernel<bf16_t>, grid, dim3(256), lds, q, a, st, md, radius);
  else hipLaunchKernelGGL(disp_softargmin_mode_kernel<float>, grid, dim3(256), lds, q, a, st, md, radius);
  return check_launch("disp_softargmin_mode");
}

extern "C" int ragmi_disparity_regression_mode_fwd(const void* prob, void* out, void* stats, void* mode, int B, int D, int H, int W,
                                                   int radius, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(prob && out && stats && mode, RAGMI_EINVAL, "disparity_regression_mode: null pointer");
  RAGMI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, RAGMI_EINVAL, "disparity_regression_mode: non-positive size");
  RAGMI_REQUIRE(radius >= 0 && radius <= D, RAGMI_EINVAL, "disparity_regression_mode: radius %d not in [0, D = %d]", radius, D);
  RAGMI_REQUIRE(dtype_ok(dtype), RAGMI_EUNSUPPORTED, "disparity_regression_mode: dtype %d not built", dtype);
  RAGMI_REQUIRE(B <= 65535, RAGMI_EUNSUPPORTED, "disparity_regression_mode: B too large");
  const int64_t hw = (int64_t)H * W;
  dim3 grid((unsigned)ceil_div(hw, 256), B);
  const hipStream_t q = static_cast<hipStream_t>(stream);
  if (dtype == RAGMI_BF16)
    hipLaunchKernelGGL(disparity_regression_mode_kernel<bf16_t>, grid, dim3(256), 0, q, (const bf16_t*)prob, (float*)out, (float*)stats, (float*)mode, D, hw, radius);
  else
    hipLaunchKernelGGL(disparity_regression_mode_kernel<float>, grid, dim3(256), 0, q, (const float*)prob, (float*)out, (float*)stats, (float*)mode, D, hw, radius);
  return check_launch("disparity_regression_mode");
}
