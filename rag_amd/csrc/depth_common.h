// Shared by the depth head's forward (depth_head.hip) and backward (depth_train.hip): tile geometry and the source index / weights
// of ATen's two bilinear resamplings, so that the adjoint gathers exactly the weights the forward applied.
#pragma once
#include "common.h"

namespace ragmi {

constexpr int DH_TH = 8, DH_TW = 32, DH_THREADS = 256, DH_CMAX = 16;
constexpr int DH_UH = DH_TH + 6, DH_UW = DH_TW + 6;   // u: tile + 3 on every side
constexpr int DH_MH = DH_TH + 4, DH_MW = DH_TW + 4;   // m: tile + 2
constexpr int DH_SH = DH_TH + 2, DH_SW = DH_TW + 2;   // s: tile + 1

// ATen's linear source index, weights and neighbour for one axis (upsample_bilinear2d)
__device__ __forceinline__ void src_ac(int dst, float scale, int in, int& i0, int& i1, float& l1) {
  const float r = scale * (float)dst;                 // align_corners=True
  i0 = (int)r;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = r - (float)i0;
}
__device__ __forceinline__ void src_half(int dst, float inv_s, int in, int& i0, int& i1, float& l1) {
  float r = inv_s * ((float)dst + 0.5f) - 0.5f;       // align_corners=False, clamped at 0
  r = r < 0.f ? 0.f : r;
  i0 = (int)r;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = r - (float)i0;
}

}  // namespace ragmi
