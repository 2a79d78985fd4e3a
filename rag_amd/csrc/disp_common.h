// The parts the soft-argmin head is made of, shared by its forward (disp.hip), its adjoint (train.hip) and the adjoint of its statistics
// (disp_stats_train.hip): the geometry of the upsample, the fine-disparity tap table, the bilinear plane sampler (all three), the walk
// over the fine disparities (forward) and the one-exponential online-softmax step (forward and plain adjoint).
#pragma once
#include "common.h"

namespace ragmi {

// cost [B, d, h, w] -> [B, maxdisp, Ho, Wo] by trilinear interpolation (align_corners = False); sd / sh / sw are ATen's scales
struct DispGeom {
  int d, h, w, maxdisp, Ho, Wo;
  float sd, sh, sw;
};
inline DispGeom disp_geom(int d, int h, int w, int maxdisp, int Ho, int Wo) {
  return DispGeom{d, h, w, maxdisp, Ho, Wo, lin_scale(d, maxdisp, 0), lin_scale(h, Ho, 0), lin_scale(w, Wo, 0)};
}

constexpr float DISP_LOG2E = 1.4426950408889634f;

// The fine-disparity taps are the same for every pixel: one table per workgroup in LDS instead of ~12 VALU instructions of index
// arithmetic per fine sample per pixel (the kernels are VALU-bound).  Entry dd: (i0, w0, w1 if i1 != i0 else 0, w1 if i1 == i0 else 0).
// The caller's barrier publishes it.
__device__ __forceinline__ void disp_fill_taps(float4* ztab, const DispGeom& g) {
  for (int dd = threadIdx.x; dd < g.maxdisp; dd += 256) {
    const LinIdx lz = lin_index(dd, g.d, g.maxdisp, g.sd, 0);
    const bool same = lz.i1 == lz.i0;
    ztab[dd] = make_float4((float)lz.i0, lz.w0, same ? 0.f : lz.w1, same ? lz.w1 : 0.f);
  }
}

// Bilinear sample of a coarse plane at one output pixel (oy, ox), both inside the image; x innermost like ATen.
template <class T>
struct DispPlaneSampler {
  const T* base;       // the pair's cost [d, h, w]
  int hw, o00, o01, o10, o11;
  float wy0, wy1, wx0, wx1;
  __device__ __forceinline__ DispPlaneSampler(const T* cost, const DispGeom& g, int oy, int ox) : base(cost), hw(g.h * g.w) {
    const LinIdx ly = lin_index(oy, g.h, g.Ho, g.sh, 0);
    const LinIdx lx = lin_index(ox, g.w, g.Wo, g.sw, 0);
    o00 = ly.i0 * g.w + lx.i0, o01 = ly.i0 * g.w + lx.i1;
    o10 = ly.i1 * g.w + lx.i0, o11 = ly.i1 * g.w + lx.i1;
    wy0 = ly.w0, wy1 = ly.w1, wx0 = lx.w0, wx1 = lx.w1;
  }
  __device__ __forceinline__ float plane(int z) const {
    const T* p = base + (int64_t)z * hw;
    return lerp2(wy0, lerp2(wx0, ld(p + o00), wx1, ld(p + o01)), wy1, lerp2(wx0, ld(p + o10), wx1, ld(p + o11)));
  }
};

// The walk over the fine disparities, in ascending order from the coarse pair (cz, cz + 1): the pair only ever moves forward, so each
// plane is sampled once.  The caller's loop  for (dd = lo; dd <= hi; ++dd) { t = walk.sample(dd); ... }  gets the negated fine cost t.
// Used by the forward kernel (main walk and MODE window walk); the two adjoints keep their own text of this loop, with their flush
// at the advance, because every shared form of it measured slower there (profiles/disp_refactor_ab.json).
template <class Sampler>
struct DispWalk {
  const float4* ztab;  // [maxdisp] of disp_fill_taps
  const Sampler& smp;
  int d, cz;
  float b0, b1;        // the samples of planes cz and min(cz + 1, d - 1)
  __device__ __forceinline__ DispWalk(const float4* taps, const Sampler& sampler, int planes, int cz0 = 0)
      : ztab(taps), smp(sampler), d(planes), cz(cz0), b0(sampler.plane(cz0)), b1(sampler.plane(cz0 + 1 < planes ? cz0 + 1 : planes - 1)) {}
  __device__ __forceinline__ float sample(int dd) {
    const float4 tb = ztab[dd];
    const int i0 = (int)tb.x;
    while (i0 > cz) {   // rarely more than one step (only when down-sampling the disparity axis); wave- and workgroup-uniform
      ++cz;
      b0 = b1;
      b1 = smp.plane(cz + 1 < d ? cz + 1 : d - 1);
    }
    return -fmaf(tb.y + tb.w, b0, tb.z * b1);
  }
};

// Online softmax of t = -cost in base 2, branch-free:  m' = max(m, t); s = s 2^((m - m') k) + 2^((t - m') k).  The differences are
// formed BEFORE the scaling by k = log2(e), so large |cost| does not lose the bits that matter near the maximum.  One of (m - m'),
// (t - m') is exactly 0 and 2^0 is exactly 1: ONE transcendental per sample, the same bits as two.
struct DispSoftmax {
  float m = -INFINITY, s = 0.f, ws = 0.f;
  struct Step {
    bool up;       // the running maximum moves to this sample
    float x, xa;   // x = 2^xa: the rescale of the sums so far (up) or the sample's weight
  };
  __device__ __forceinline__ Step weigh(float t) const {
    const bool up = t > m;
    const float xa = (up ? m - t : t - m) * DISP_LOG2E;
    return Step{up, __builtin_amdgcn_exp2f(xa), xa};     // 2^(-inf) = 0 on the first sample
  }
  __device__ __forceinline__ void add(const Step& k, int dd, float t) {
    const float r = k.up ? k.x : 1.f, e = k.up ? 1.f : k.x;
    s = fmaf(s, r, e);
    ws = fmaf(ws, r, e * (float)dd);
    m = k.up ? t : m;
  }
};

// The adjoints' tile: a workgroup owns a 16 x 16 tile of fine pixels whose coarse cells form a window of at most 8 x 8.  These two
// constants are all that is shared of the tile reduction: its set-up and flush are written out in train.hip and in
// disp_stats_train.hip (a shared struct measured slower, profiles/disp_refactor_ab.json), so there is no struct to look for here.
constexpr int DISP_BWD_T = 16, DISP_BWD_WIN = 8;      // fine tile edge; coarse window edge (16/3 -> 6 cells + 1 each side for the taps)

}  // namespace ragmi
