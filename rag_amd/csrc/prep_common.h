// Device functions shared by the batch-preparation kernels (prep.hip, prep_resize.hip): one definition, so the fused launches
// cannot drift apart.
#pragma once
#include "common.h"

namespace ragmi {

// ToTensor + Normalize of a byte level in fp32, the reference's expression with two IEEE divisions (src/dataloaders/data_io.py:6-13)
__device__ __forceinline__ float normalize_level(int level, float mean, float std) {
#pragma clang fp contract(off)
  const float v = (float)level / 255.0f;
  return (v - mean) / std;
}

}  // namespace ragmi
