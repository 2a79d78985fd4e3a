// The fixed-order reductions of the loss, metric, optimiser and weight-gradient kernels: one definition of the contract
//   "no atomics, no memset, the same bits on every run, graph-capturable".
// Every such kernel ends the same way.  Each thread holds N partial sums; the workgroup adds them in a fixed order and one
// thread per sum writes it to the workgroup's slot; a finalize step (a small kernel, or the head of the consumer) gathers the
// slots per thread with a stride of the workgroup's width and adds them in the same fixed order.  The ORDER OF ADDITIONS IS THE
// CONTRACT: the tree strides, the butterfly offsets, (w0 + w1) + (w2 + w3), the strided gather and the element type of each
// level (float or double partials, double finalize, u64 in prep.hip) are what the results' bits rest on and what
// tests/test_reduce_order.py restates on the CPU.  Change them here, for every caller at once, or not at all.
//
// Two shapes:
//   block_tree_sum<WG>(v)   LDS halving tree, red[k][tid] += red[k][tid + s] for s = WG/2 ... 1, any power-of-two WG.
//   block_wave_sum(v)       256 threads: xor butterflies 32 ... 1 in each wave, then the four waves as (w0 + w1) + (w2 + w3).
// Both return an accessor, not values: sums[k] reads LDS, so only the threads that need a sum load it.  Every thread of the
// workgroup must make the call (it holds barriers; a branch around it must be uniform per workgroup).  The LDS array belongs to
// the instantiation (WG, type, N), so two calls of one instantiation in a kernel share it: READ YOUR SUMS BEFORE THE BARRIER THAT
// PRECEDES THE NEXT CALL, and put that barrier there (color_stats_finalize_kernel does both).
//
// What stays written out, on purpose:
//   - the tile reduction (`flush`) and the walk loops of disp_softargmin_bwd_kernel and disp_softargmin_stats_bwd_kernel: their
//     shared forms were measured 0.5-3 % slower (profiles/disp_refactor_ab.json);
//   - block_pair_store / block_pair_sum of train.hip (BN-train statistics and adjoint coefficients, six kernels on the training
//     step's critical path): on block_tree_sum the BN launches (per kernel, 1-2 %) and the training step (0.3 %) lay outside
//     the parent's min-max spread on the slow side (profiles/reduce_refactor_ab.json); same additions, two LDS arrays per tree;
//   - the partial butterflies (offsets 4, 8, 16, 32 only) of conv3d_k3_wgrad_kernel, x3_wave_max and the scans of sparsify.hip:
//     different operations;
//   - the float atomicAdd that combines the workgroups of stereo_metrics_kernel, conv3d_k1_wgrad_kernel and
//     conv2d_strided_wgrad_kernel: the only results here that are not run-to-run reproducible; a slot-and-finalize form of
//     them would change behaviour.
#pragma once
#include <algorithm>

#include "common.h"

namespace ragmi {

// sum over the 64 lanes of a wave, in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

template <int WG, class T, int N>
struct BlockTreeSums {
  const T (&red)[N][WG];
  __device__ __forceinline__ T operator[](int k) const { return red[k][0]; }
};
template <int WG, class T, int N>
__device__ __forceinline__ BlockTreeSums<WG, T, N> block_tree_sum(const T (&v)[N]) {
  static_assert(WG > 0 && (WG & (WG - 1)) == 0, "the halving tree needs a power-of-two workgroup");
  __shared__ T red[N][WG];
#pragma unroll
  for (int k = 0; k < N; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
#pragma unroll
  for (int s = WG / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int k = 0; k < N; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
    }
    __syncthreads();
  }
  return {red};
}

template <class T, int N>
struct BlockWaveSums {
  const T (&red)[4][N];
  __device__ __forceinline__ T operator[](int k) const { return (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]); }
};
template <class T, int N>
__device__ __forceinline__ BlockWaveSums<T, N> block_wave_sum(const T (&v)[N]) {
  __shared__ T red[4][N];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const T s = wave_sum(v[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  return {red};
}

// v[k] = sum of slots[s * N + k] over s = tid, tid + WG, ... < nslots, in that order, in T whatever the slots' type
template <int WG, class T, int N, class S, class I>
__device__ __forceinline__ void gather_slots(const S* __restrict__ slots, I nslots, T (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = T(0);
  for (I s = threadIdx.x; s < nslots; s += WG) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += (T)slots[(int64_t)s * N + k];
  }
}

// workgroups (= slots) of a grid-stride first level over n elements: four elements per thread, at least one, at most max_wg
inline int grid_stride_slots(int64_t n, int wg, int max_wg) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 4 * wg), max_wg));
}

}  // namespace ragmi
