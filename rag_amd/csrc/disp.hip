// K2 — fused Disp.forward: trilinear x3 upsample (align_corners=False) -> Softmin over the
// disparity axis -> DisparityRegression.  Reference: src/models/rag_model.py:18-44.
//
// The reference materialises three [B,192,H,W] tensors (3.7 GB of traffic at the headline
// config); here each output pixel streams the d coarse planes once (4 bilinear taps per
// plane, L1/L2-served: neighbouring pixels share taps), lerps along the disparity axis in
// registers and keeps an online softmax (running max / sum / disparity-weighted sum).
// Algorithmic traffic: read d*h*w*4 B, write Ho*Wo*4 B per pair (15.5 MB at headline).
// The geometry, the tap table, the plane sampler, the walk and the online-softmax step are the parts of disp_common.h, shared with
// the two adjoints.
#include "disp_common.h"

namespace ragmi {

struct DispArgs {
  const void* cost;   // [B, d, h, w], float or bf16_t
  float* out;         // [B, Ho, Wo]
  DispGeom g;
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

// The generic form, any scales: one thread per output pixel walks the fine disparities once (DispWalk) with the online softmax.
template <class T, bool STATS, bool MODE>
__global__ __launch_bounds__(256) void disp_softargmin_kernel(DispArgs a, float* stats, float* mode, int radius) {
  static_assert(STATS || !MODE, "the mode instantiations write the statistics too");
  extern __shared__ float4 ztab[];                 // [maxdisp]
  const DispGeom& g = a.g;
  disp_fill_taps(ztab, g);
  __syncthreads();
  const int64_t npix = (int64_t)g.Ho * g.Wo;
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= npix) return;
  const int b = blockIdx.y;
  const DispPlaneSampler<T> smp(static_cast<const T*>(a.cost) + (int64_t)b * g.d * (g.h * g.w), g, (int)(o / g.Wo), (int)(o % g.Wo));
  DispSoftmax sm;
  DispMoments mo;
  DispWalk walk(ztab, smp, g.d);
  for (int dd = 0; dd < g.maxdisp; ++dd) {
    const float t = walk.sample(dd);
    const DispSoftmax::Step k = sm.weigh(t);
    if constexpr (STATS) {
      // There is no pass 1 here, so the pivot follows the running maximum.  When it moves to this sample (weight 1, exponent 0, offset
      // 0: it adds nothing to M1, M2, xs) the sums so far are re-centred about dd, re-based to the new maximum (every exponent drops
      // by xa = log2 r) and rescaled by r like s and ws:
      //   M2' = r (M2 - 2 dl M1 + dl^2 s),  M1' = r (M1 - dl s),  xs' = r (xs + xa s)      with dl = dd - pv and the OLD s.
      // The rounding of a re-centring is relative to the moments about the new pivot, and r <= 1 shrinks it with them.
      // Between moves the samples go into one block chain, folded into the totals every 16 samples and before a move (flush()):
      // d = 213 -> 639 fine samples in one serial chain lost more than the gate allows on a broad distribution.
      if (k.up) {
        mo.flush();
        const float dl = (float)dd - mo.pv;
        mo.m2 = k.x * fmaf(dl, fmaf(dl, sm.s, -2.f * mo.m1), mo.m2);
        mo.m1 = k.x * fmaf(-dl, sm.s, mo.m1);
        mo.xs = sm.s > 0.f ? k.x * fmaf(k.xa, sm.s, mo.xs) : 0.f;      // first sample: xa = -inf, s = 0
        mo.pv = (float)dd;
        mo.pk = 1.f;
      } else {
        mo.add_chain(0, k.x, k.xa, (float)dd);
      }
      if ((dd & 15) == 15) mo.flush();
    }
    sm.add(k, dd, t);
  }
  const float s = sm.s;
  a.out[(int64_t)b * npix + o] = sm.ws / s;
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
    const int ks = (int)mo.pv, d_lo = max(ks - radius, 0), d_hi = min(ks + radius, g.maxdisp - 1);
    DispWalk window(ztab, smp, g.d, (int)ztab[d_lo].x);
    for (int dd = d_lo; dd <= d_hi; ++dd) {
      wd.add_chain(0, __builtin_amdgcn_exp2f((window.sample(dd) - sm.m) * DISP_LOG2E), (float)dd);
      if (((dd - d_lo) & 15) == 15) wd.flush();
    }
    wd.flush();
    wd.store(mode, b, npix, o, s);
  }
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

template <class T, bool STATS, bool MODE>
__global__ __launch_bounds__(256) void disp_softargmin_x3_kernel(DispArgs a, float* stats, float* mode, int radius) {
  static_assert(STATS || !MODE, "the mode instantiations write the statistics too");
  extern __shared__ __attribute__((aligned(16))) float dx3_lds[];
  const DispGeom& g = a.g;
  float4* const ztab = reinterpret_cast<float4*>(dx3_lds);            // [maxdisp] (wp, wc, wn, dd)
  float* const tile = dx3_lds + 4 * g.maxdisp;                        // [d][5][13]
  const int tid = threadIdx.x, tx = tid % DX3_TX, ty = tid / DX3_TX;
  // XCD-aware tile order: workgroup j runs on XCD j % 8 (round-robin dispatch); every XCD walks one contiguous chunk of the
  // x-fastest tile list, so tiles that share coarse rows / columns of the cost meet in ONE L2.  With blockIdx.x = tile x the eight
  // neighbours of a tile sat on eight different XCDs and every L2 fetched its own copy of the shared halo: 77 MB from the memory
  // side for a 13.6 MB tensor (profiles/r04y_pmc_summary.txt).
  const int ntx = (g.Wo + DX3_TX - 1) / DX3_TX, nty = (g.Ho + DX3_TY - 1) / DX3_TY, ntile = ntx * nty;
  const int chunk = (ntile + 7) / 8, jb = blockIdx.x;
  const int tidx = (jb & 7) * chunk + (jb >> 3);
  if ((jb >> 3) >= chunk || tidx >= ntile) return;
  const int ox0 = (tidx % ntx) * DX3_TX, oy0 = (tidx / ntx) * DX3_TY, b = blockIdx.z;
  const int ox = min(ox0 + tx, g.Wo - 1), oy = min(oy0 + ty, g.Ho - 1);       // out-of-range threads shadow the last pixel, store nothing
  const int cy0 = lin_index(oy0, g.h, g.Ho, g.sh, 0).i0, cx0 = lin_index(ox0, g.w, g.Wo, g.sw, 0).i0;
  const int hw = g.h * g.w, D = g.d;
  const T* base = static_cast<const T*>(a.cost) + (int64_t)b * D * hw;
  for (int i = tid; i < D * DX3_CP; i += 256) {
    const int z = i / DX3_CP, r = i % DX3_CP;
    const int gy = min(cy0 + r / DX3_CC, g.h - 1), gx = min(cx0 + r % DX3_CC, g.w - 1);
    tile[i] = ld(base + (int64_t)z * hw + gy * g.w + gx);
  }
  for (int dd = tid; dd < g.maxdisp; dd += 256) {
    const LinIdx lz = lin_index(dd, D, g.maxdisp, g.sd, 0);
    const int k = dd / 3;
    float4 e = make_float4(0.f, 0.f, 0.f, (float)dd);
    if (lz.i0 < k) { e.x = lz.w0; e.y = lz.w1; }                      // planes (k-1, k)
    else if (lz.i1 != lz.i0) { e.y = lz.w0; e.z = lz.w1; }            // planes (k, k+1)
    else e.y = lz.w0 + lz.w1;                                         // clamped at the last plane
    ztab[dd] = e;
  }
  const LinIdx ly = lin_index(oy, g.h, g.Ho, g.sh, 0);
  const LinIdx lx = lin_index(ox, g.w, g.Wo, g.sw, 0);
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
  float s = 0.f, ws = 0.f;
  // STATS: the coarse arg-min of pass 1 gives the pivot of the moments, fine sample 3 argmin + 1 (the one whose source index IS that
  // plane); the softmin's mode is within a coarse step of it
  DispMoments mo;
  int am = 0;
  // MODE: fine sample 3 am + 1 sits exactly on plane am, the smallest of the planes every fine sample is a convex combination of, so
  // k* = 3 am + 1 - except am == 0: the source index is clamped at 0, fine samples 0 and 1 both evaluate to v[0], and k* = 0
  DispWindow wd;
  wd.rf = (float)radius;
  // Fine sample 3 k + j from the window (previous, current, next) of plane samples, against the minimum lo of pass 1.  Exponent of a
  // sample: (min - cost) * K: the difference is formed BEFORE the scaling by K, like the generic kernel, so large |cost| does not
  // lose the bits that matter near the minimum
  float lo = INFINITY;
  auto sample = [&](int j, const float4 tb, float vp, float vc, float vn) __attribute__((always_inline)) {
    const float c = fmaf(tb.x, vp, fmaf(tb.y, vc, tb.z * vn));
    const float x = (lo - c) * DISP_LOG2E;
    const float e = __builtin_amdgcn_exp2f(x);
    s += e;
    ws = fmaf(e, tb.w, ws);
    if constexpr (STATS) mo.add_chain(j, e, x, tb.w);
    if constexpr (MODE) wd.add_chain(j, e, tb.w);
  };
  auto fold = [&]() __attribute__((always_inline)) {      // every 8 coarse planes and at the end
    if constexpr (STATS) mo.flush();
    if constexpr (MODE) wd.flush();
  };
  // d = 64 (maxdisp 192, the reference's only configuration, rag_model.py:274): the 64 plane samples of pass 1 stay in REGISTERS for
  // pass 2 — no second round of 4 d LDS reads and bilinear arithmetic (same operations on the same values: identical bits).  Chunks
  // of 8 planes fenced by sched_barrier: unfenced, the scheduler hoisted all 256 operand reads and the kernel spilled or ran at
  // 87 us (round 2).  Same box, both builds: 49.9 -> 40.3 us (90 VGPRs, 5 waves per SIMD).
  if (D == 64) {
    float v[64];
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
      for (int j = 0; j < 3; ++j) sample(j, ztab[3 * k + j], vp_, vc_, vn_);
      if ((k & 7) == 7) {
        fold();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
#pragma clang loop unroll_count(4) vectorize(disable)
  for (int z = 0; z < D; ++z) {
    const float vz = plane(z);
    if constexpr (STATS) am = vz < lo ? z : am;
    lo = fminf(lo, vz);
  }
  if constexpr (STATS) mo.pv = (float)(3 * am + 1);
  if constexpr (MODE) wd.ks = am == 0 ? 0.f : mo.pv;
  float vc = plane(0), vp = vc, vn = plane(min(1, D - 1));
  for (int k = 0; k < D; ++k) {
#pragma unroll
    for (int j = 0; j < 3; ++j) sample(j, ztab[3 * k + j], vp, vc, vn);     // wave-uniform address: one broadcast read
    vp = vc; vc = vn; vn = plane(min(k + 2, D - 1));
    if ((k & 7) == 7) fold();
  }
  fold();
  }
  if (ox0 + tx < g.Wo && oy0 + ty < g.Ho) {
    a.out[(int64_t)b * g.Ho * g.Wo + (int64_t)oy * g.Wo + ox] = ws / s;
    if constexpr (STATS) mo.store(stats, b, (int64_t)g.Ho * g.Wo, (int64_t)oy * g.Wo + ox, s);
    if constexpr (MODE) wd.store(mode, b, (int64_t)g.Ho * g.Wo, (int64_t)oy * g.Wo + ox, s);
  }
}

// standalone DisparityRegression: out = sum_d prob[:, d] * d
// STATS: with the statistics of `prob`, taken as given (not renormalised): out as above (the same fmaf chain, the same
// bits), variance = sum p (k - out)^2 by the definition in a second walk over the D planes (a one-hot prob gives exactly 0: out is
// exactly its index), peak = max p, entropy = -sum_{p > 0} p ln p.  The two stat sums run in 8 interleaved partial sums: there is no
// interpolation error to hide behind here, and a serial fp32 sum of 192 terms alone is ~5e-7 of the result.
// MODE: k* is the first arg-max of prob (found in the statistics walk: strictly greater moves it), and a third walk over the window
// |k - k*| <= radius alone sums prob and prob (k - k*), in 8 interleaved partial sums again: mode = (k*, k* + sum p (k - k*) / sum p,
// sum p), and a window without mass gives mode_disp = k*.  A one-hot prob gives (its index, its index, 1) exactly.
template <class T, bool STATS, bool MODE>
__global__ __launch_bounds__(256) void disparity_regression_kernel(const T* __restrict__ prob, float* __restrict__ out, float* __restrict__ stats,
                                                                  float* __restrict__ mode, int D, int64_t hw, int radius) {
  static_assert(STATS || !MODE, "the mode instantiations write the statistics too");
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= hw) return;
  const int b = blockIdx.y;
  const T* p = prob + (int64_t)b * D * hw + o;
  float acc = 0.f;
#pragma unroll 8
  for (int dd = 0; dd < D; ++dd) acc = fmaf(ld(p + (int64_t)dd * hw), (float)dd, acc);
  out[(int64_t)b * hw + o] = acc;
  if constexpr (STATS) {
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
}

// One launch function per family: the argument checks, the dispatch rule and the launch geometry of the plain, statistics (STATS)
// and mode (MODE) entry points, which differ in the outputs they pass and in the name their messages carry.
template <bool STATS, bool MODE>
int launch_disp_softargmin(const char* name, const void* cost, void* out, void* stats, void* mode, int B, int d, int h, int w,
                           int maxdisp, int Ho, int Wo, int radius, int dtype, void* stream) {
  RAGMI_REQUIRE(B > 0 && d > 0 && h > 0 && w > 0 && maxdisp > 0 && Ho > 0 && Wo > 0, RAGMI_EINVAL, "%s: non-positive size", name);
  if constexpr (MODE)
    RAGMI_REQUIRE(radius >= 0 && radius <= maxdisp, RAGMI_EINVAL, "%s: radius %d not in [0, maxdisp = %d]", name, radius, maxdisp);
  RAGMI_REQUIRE(dtype_ok(dtype), RAGMI_EUNSUPPORTED, "%s: dtype %d not built", name, dtype);
  RAGMI_REQUIRE(B <= 65535 && (int64_t)h * w < (1ll << 30), RAGMI_EUNSUPPORTED, "%s: size too large", name);
  const DispArgs a{cost, (float*)out, disp_geom(d, h, w, maxdisp, Ho, Wo)};
  const size_t lds = (size_t)maxdisp * sizeof(float4);
  RAGMI_REQUIRE(lds <= 64 * 1024, RAGMI_EUNSUPPORTED, "%s: maxdisp %d exceeds the tap table (4096)", name, maxdisp);
  const size_t lds3 = lds + (size_t)d * DX3_CP * sizeof(float);
  // the reference's configuration (rag_model.py:40, 272-273): the tiled form (register form at d = 64, else the rolling window)
  const bool tiled = maxdisp == 3 * d && Ho == 3 * h && Wo == 3 * w && lds3 <= 64 * 1024, bf16 = dtype == RAGMI_BF16;
  const dim3 grid((unsigned)ceil_div((int64_t)Ho * Wo, 256), B);
  const dim3 g3((unsigned)ceil_div(Wo, DX3_TX), (unsigned)ceil_div(Ho, DX3_TY), (unsigned)B);
  const dim3 g1((unsigned)(ceil_div((int64_t)g3.x * g3.y, 8) * 8), 1, (unsigned)B);      // the tiled kernel decodes its tile itself (XCD-aware)
  void (*const kernel)(DispArgs, float*, float*, int) =
      tiled ? (bf16 ? disp_softargmin_x3_kernel<bf16_t, STATS, MODE> : disp_softargmin_x3_kernel<float, STATS, MODE>)
            : (bf16 ? disp_softargmin_kernel<bf16_t, STATS, MODE> : disp_softargmin_kernel<float, STATS, MODE>);
  hipLaunchKernelGGL(kernel, tiled ? g1 : grid, dim3(256), tiled ? lds3 : lds, static_cast<hipStream_t>(stream), a, (float*)stats,
                     (float*)mode, radius);
  return check_launch(name);
}

template <bool STATS, bool MODE>
int launch_disparity_regression(const char* name, const void* prob, void* out, void* stats, void* mode, int B, int D, int H, int W,
                                int radius, int dtype, void* stream) {
  RAGMI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, RAGMI_EINVAL, "%s: non-positive size", name);
  if constexpr (MODE) RAGMI_REQUIRE(radius >= 0 && radius <= D, RAGMI_EINVAL, "%s: radius %d not in [0, D = %d]", name, radius, D);
  RAGMI_REQUIRE(dtype_ok(dtype), RAGMI_EUNSUPPORTED, "%s: dtype %d not built", name, dtype);
  RAGMI_REQUIRE(B <= 65535, RAGMI_EUNSUPPORTED, "%s: B too large", name);
  const int64_t hw = (int64_t)H * W;
  const dim3 grid((unsigned)ceil_div(hw, 256), B);
  const hipStream_t q = static_cast<hipStream_t>(stream);
  if (dtype == RAGMI_BF16)
    hipLaunchKernelGGL((disparity_regression_kernel<bf16_t, STATS, MODE>), grid, dim3(256), 0, q, (const bf16_t*)prob, (float*)out,
                       (float*)stats, (float*)mode, D, hw, radius);
  else
    hipLaunchKernelGGL((disparity_regression_kernel<float, STATS, MODE>), grid, dim3(256), 0, q, (const float*)prob, (float*)out,
                       (float*)stats, (float*)mode, D, hw, radius);
  return check_launch(name);
}

}  // namespace ragmi

extern "C" int ragmi_disp_softargmin_fwd(const void* cost, void* out, int B, int d, int h, int w, int maxdisp, int Ho,
                                         int Wo, int dtype, void* stream) {
  RAGMI_REQUIRE(cost && out, RAGMI_EINVAL, "disp_softargmin: null pointer");
  return ragmi::launch_disp_softargmin<false, false>("disp_softargmin", cost, out, nullptr, nullptr, B, d, h, w, maxdisp, Ho, Wo, 0, dtype,
                                                     stream);
}
extern "C" int ragmi_disp_softargmin_stats_fwd(const void* cost, void* out, void* stats, int B, int d, int h, int w, int maxdisp,
                                               int Ho, int Wo, int dtype, void* stream) {
  RAGMI_REQUIRE(cost && out && stats, RAGMI_EINVAL, "disp_softargmin_stats: null pointer");
  return ragmi::launch_disp_softargmin<true, false>("disp_softargmin_stats", cost, out, stats, nullptr, B, d, h, w, maxdisp, Ho, Wo, 0,
                                                    dtype, stream);
}
// radius is a run-time argument of the kernels
extern "C" int ragmi_disp_softargmin_mode_fwd(const void* cost, void* out, void* stats, void* mode, int B, int d, int h, int w,
                                              int maxdisp, int Ho, int Wo, int radius, int dtype, void* stream) {
  RAGMI_REQUIRE(cost && out && stats && mode, RAGMI_EINVAL, "disp_softargmin_mode: null pointer");
  return ragmi::launch_disp_softargmin<true, true>("disp_softargmin_mode", cost, out, stats, mode, B, d, h, w, maxdisp, Ho, Wo, radius,
                                                   dtype, stream);
}

extern "C" int ragmi_disparity_regression_fwd(const void* prob, void* out, int B, int D, int H, int W, int dtype,
                                              void* stream) {
  RAGMI_REQUIRE(prob && out, RAGMI_EINVAL, "disparity_regression: null pointer");
  return ragmi::launch_disparity_regression<false, false>("disparity_regression", prob, out, nullptr, nullptr, B, D, H, W, 0, dtype, stream);
}
extern "C" int ragmi_disparity_regression_stats_fwd(const void* prob, void* out, void* stats, int B, int D, int H, int W, int dtype,
                                                    void* stream) {
  RAGMI_REQUIRE(prob && out && stats, RAGMI_EINVAL, "disparity_regression_stats: null pointer");
  return ragmi::launch_disparity_regression<true, false>("disparity_regression_stats", prob, out, stats, nullptr, B, D, H, W, 0, dtype,
                                                         stream);
}
extern "C" int ragmi_disparity_regression_mode_fwd(const void* prob, void* out, void* stats, void* mode, int B, int D, int H, int W,
                                                   int radius, int dtype, void* stream) {
  RAGMI_REQUIRE(prob && out && stats && mode, RAGMI_EINVAL, "disparity_regression_mode: null pointer");
  return ragmi::launch_disparity_regression<true, true>("disparity_regression_mode", prob, out, stats, mode, B, D, H, W, radius, dtype,
                                                        stream);
}
