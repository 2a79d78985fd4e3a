// Speckle filter: connected segments of similar disparity, their sizes, and a keep map without the small ones.  Definition:
// include/rag_amd.h, DESIGN.md section 4.5.3.
//
// A pixel is reliable iff it is kept and its disparity is finite; two 4-neighbours are joined iff both are reliable and
// fabsf(d_p - d_q) <= max_diff (one fp32 subtraction, one absolute value, one comparison); a segment is a connected component.  An
// unreliable value travels as a NaN pattern, so its comparison is false without a second test and it is never read as a value.
//
// ragmi_speckle_fwd, five launches in a fixed sequence (the seam launch is left out where the image is one tile; that depends on
// the shape alone):
//   tile      one workgroup labels a 16 x 64 tile in LDS, one wave per four rows.  A horizontal run needs no union: its head is the
//             nearest "not joined to the left" lane at or before a lane, found in the ballot of those bits with a count of leading
//             zeros.  Down edges unite the runs with the lock-free union on LDS (find both roots, atomicMin the larger root's slot
//             with the smaller, go on from the returned value if someone was first); an edge whose left neighbour joins the same two
//             runs is skipped.  parent[p] = the image index of the tile-local root (<= p; -1: unreliable), lcount[p] = the tile-local
//             segment's pixels at its root and 0 elsewhere (a run head adds its run's length: LDS atomicAdd per run, not per pixel),
//             total[p] = 0.
//   seam      one thread per pixel of a tile's last column / last row that has a neighbour across the seam: the same union on
//             `parent` in global memory.  Only slots of tile-local roots are ever written, every write lowers the slot, and no thread
//             waits for another; `parent` is read with relaxed agent-scope atomic loads, a stale value costs an iteration and the
//             atomicMin's return value decides.  No fence, flag or ticket.  An edge whose predecessor on the same tile edge unites
//             the same two segments is skipped, as in the tile launch.
//   flatten   every reliable pixel walks from its tile-local root to the segment's root (plain loads: the seam launch is complete)
//             and writes `label`; a tile-local root adds lcount to total[root]: integer atomicAdd, one per tile a segment touches.
//   apply     size = total[label], keep_out, and five integer counts per workgroup slot.
//   finalize  one workgroup per image folds the slots in the fixed order of reduce.h.
// Integer atomics only (min, add: the result does not depend on their order), no memset, no memcpy, no host synchronisation; every
// output element and every workspace element that is read is written by the call.
#include <cmath>

#include "reduce.h"

namespace ragmi {

constexpr int SP_WG = 256;                               // threads per workgroup of every kernel here
constexpr int SP_TR = RAGMI_SPECKLE_TILE_ROWS;           // the tile of the first launch
constexpr int SP_TC = RAGMI_SPECKLE_TILE_COLS;
constexpr int SP_RPW = SP_TR / (SP_WG / 64);             // rows per wave
constexpr int SP_PPT = 4;                                // pixels per thread of the apply launch
constexpr unsigned SP_NONE = 0xffffffffu;                // not reliable: a NaN pattern
constexpr unsigned SP_ONE = 0x3f800000u;                 // 1.0f: the only pattern that compares == 1.0f
static_assert(SP_TC == 64 && SP_TR % (SP_WG / 64) == 0 && SP_TR * SP_TC <= 65536, "a tile row is one wave");

__device__ __forceinline__ bool sp_finite(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }
// joined: false when either value is SP_NONE (NaN), or when the difference overflows to Inf
__device__ __forceinline__ bool sp_joined(unsigned a, unsigned b, float max_diff) {
  return fabsf(__uint_as_float(a) - __uint_as_float(b)) <= max_diff;
}

// The lock-free union on parent pointers that only ever decrease (slot[i] <= i; slot[i] == i: a root).  SCOPE: the workgroup for
// LDS, the agent for global memory.
template <int SCOPE>
__device__ __forceinline__ int sp_find(int* slot, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&slot[i], __ATOMIC_RELAXED, SCOPE);
    if (p == i) return i;
    i = p;                                               // p < i: the walk ends
  }
}
template <int SCOPE>
__device__ __forceinline__ void sp_union(int* slot, int a, int b) {
  for (;;) {
    a = sp_find<SCOPE>(slot, a);
    b = sp_find<SCOPE>(slot, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }        // a > b
    const int old = atomicMin(&slot[a], b);
    if (old == a) return;                                // a was still a root: linked
    a = old;                                             // someone linked a to old < a first: old and b are still to be united
  }
}

template <int KIND>
__global__ __launch_bounds__(SP_WG) void speckle_tile_kernel(const unsigned* __restrict__ disp, const void* __restrict__ keep, int H, int W,
                                                             unsigned tiles_x, unsigned tiles_y, float max_diff,
                                                             int* __restrict__ parent, int* __restrict__ lcount, int* __restrict__ total) {
  __shared__ unsigned val[SP_TR * SP_TC];                // the disparity's bits, SP_NONE where unreliable
  __shared__ int lab[SP_TR * SP_TC];                     // parent pointers inside the tile (local index row * 64 + column)
  __shared__ int cnt[SP_TR * SP_TC];
  __shared__ uint8_t jleft[SP_TR * SP_TC];               // joined to the left neighbour
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned tx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
  const unsigned ty = rest % tiles_y, b = rest / tiles_y;
  const int64_t x = (int64_t)tx * SP_TC + lane, y0 = (int64_t)ty * SP_TR;
  const int64_t img = (int64_t)b * H * W;
  unsigned v[SP_RPW];
  bool jl[SP_RPW];
  int head[SP_RPW], len[SP_RPW];
#pragma unroll
  for (int j = 0; j < SP_RPW; ++j) {
    const int r = wave * SP_RPW + j;
    const int64_t y = y0 + r;
    v[j] = SP_NONE;
    if (y < H && x < W) {
      const int64_t p = img + y * W + x;
      const unsigned d = disp[p];
      const bool k = KIND == 2 ? true
                   : KIND == 1 ? static_cast<const uint8_t*>(keep)[p] != 0 : static_cast<const unsigned*>(keep)[p] == SP_ONE;
      if (k && sp_finite(d)) v[j] = d;
    }
  }
#pragma unroll
  for (int j = 0; j < SP_RPW; ++j) {
    const int own = (wave * SP_RPW + j) * SP_TC + lane;
    const unsigned left = __shfl_up(v[j], 1);
    jl[j] = lane > 0 && sp_joined(v[j], left, max_diff);
    const unsigned long long starts = __ballot(!jl[j]);                     // bit 0 is always set
    head[j] = lane - __clzll((long long)(starts << (63 - lane)));          // the nearest start at or before this lane
    const unsigned long long after = lane == 63 ? 0ull : starts >> (lane + 1);
    len[j] = after ? __ffsll(after) : 64 - lane;                            // the run's length, read by its head only
    val[own] = v[j];
    lab[own] = own - lane + head[j];                                        // an unreliable pixel is its own head
    cnt[own] = 0;
    jleft[own] = jl[j];
  }
  __syncthreads();
  // down edges: unite the two runs; skipped where the edge one column to the left unites the same two
#pragma unroll
  for (int j = 0; j < SP_RPW; ++j) {
    const int r = wave * SP_RPW + j;
    if (r + 1 < SP_TR) {                                                    // uniform
      const int own = r * SP_TC + lane;
      const bool jd = sp_joined(v[j], val[own + SP_TC], max_diff);
      const bool jd_left = __shfl_up((int)jd, 1) != 0;
      const bool same_pair = lane > 0 && jl[j] && jleft[own + SP_TC] && jd_left;
      if (jd && !same_pair) sp_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, own, own + SP_TC);
    }
  }
  __syncthreads();
  int root[SP_RPW];
#pragma unroll
  for (int j = 0; j < SP_RPW; ++j) {
    const int own = (wave * SP_RPW + j) * SP_TC + lane;
    root[j] = sp_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, own);
    if (v[j] != SP_NONE && head[j] == lane) atomicAdd(&cnt[root[j]], len[j]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SP_RPW; ++j) {
    const int r = wave * SP_RPW + j;
    const int64_t y = y0 + r;
    if (y < H && x < W) {
      const int64_t p = img + y * W + x;
      const int own = r * SP_TC + lane;
      const bool reliable = v[j] != SP_NONE;
      const int64_t ry = y0 + (root[j] >> 6), rx = (int64_t)tx * SP_TC + (root[j] & 63);
      parent[p] = reliable ? (int)(ry * W + rx) : -1;
      lcount[p] = (reliable && root[j] == own) ? cnt[own] : 0;
      total[p] = 0;
    }
  }
}

// thread i of an image: the first (tiles_x - 1) * H are the pixels left of a vertical seam, the other (tiles_y - 1) * W the pixels
// above a horizontal one
__global__ __launch_bounds__(SP_WG) void speckle_seam_kernel(const unsigned* __restrict__ disp, int H, int W, unsigned tiles_x, int64_t per_image,
                                                             int64_t n, float max_diff, int* parent) {
  const int64_t i = (int64_t)blockIdx.x * SP_WG + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / per_image;
  int64_t s = i - b * per_image;
  const int64_t nv = (int64_t)(tiles_x - 1) * H;
  int64_t x, y, step;
  const bool vertical = s < nv;
  if (vertical) {
    y = s % H;
    x = (s / H + 1) * SP_TC - 1;
    step = 1;
  } else {
    s -= nv;
    x = s % W;
    y = (s / W + 1) * SP_TR - 1;
    step = W;
  }
  const int64_t img = (int64_t)b * H * W;
  int* par = parent + img;
  const int p = (int)(y * W + x), q = (int)(p + step);                      // x + 1 < W, y + 1 < H by the count of seams
  const int rp = __hip_atomic_load(&par[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // -1 never changes; else a pixel of
  const int rq = __hip_atomic_load(&par[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // p's (q's) segment, one hop nearer its root
  if (rp < 0 || rq < 0) return;
  const unsigned dp = disp[img + p], dq = disp[img + q];
  if (!sp_joined(dp, dq, max_diff)) return;
  // The previous pixel along the seam, if it lies on the same tile edge: where it is joined to p, its neighbour across the seam to q
  // and the two to each other, the tile launch has united p with it and q with its neighbour, and its own thread unites the two
  // segments (or leaves that to the one before it: the first pixel of a tile edge never does).  On a smooth surface that leaves
  // one union per tile edge and run, not one per pixel.
  const bool first = vertical ? y % SP_TR == 0 : x % SP_TC == 0;
  if (!first) {
    const int64_t back = vertical ? W : 1;
    const int p2 = (int)(p - back), q2 = (int)(q - back);
    if (__hip_atomic_load(&par[p2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0 &&
        __hip_atomic_load(&par[q2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) {
      const unsigned dp2 = disp[img + p2], dq2 = disp[img + q2];
      if (sp_joined(dp, dp2, max_diff) && sp_joined(dq, dq2, max_diff) && sp_joined(dp2, dq2, max_diff)) return;
    }
  }
  sp_union<__HIP_MEMORY_SCOPE_AGENT>(par, rp, rq);
}

__global__ __launch_bounds__(SP_WG) void speckle_flatten_kernel(const int* __restrict__ parent, const int* __restrict__ lcount, int64_t hw,
                                                                int64_t n, int* __restrict__ label, int* total) {
  const int64_t i = (int64_t)blockIdx.x * SP_WG + threadIdx.x;
  if (i >= n) return;
  const int64_t img = i / hw * hw;
  const int* par = parent + img;
  int r = parent[i];
  if (r >= 0) {
    for (int up = par[r]; up != r; up = par[r]) r = up;
    const int c = lcount[i];
    if (c > 0) atomicAdd(&total[img + r], c);                               // this pixel is a tile-local root
  }
  label[i] = r;
}

__device__ __forceinline__ int sp_block_max(int v) {
  __shared__ int red[SP_WG / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(red[0], red[1]), max(red[2], red[3]));
}

__global__ __launch_bounds__(SP_WG) void speckle_apply_kernel(const int* __restrict__ label, const int* __restrict__ total, int64_t hw,
                                                              unsigned groups, int max_size, int* __restrict__ size, uint8_t* __restrict__ keep_out,
                                                              int* __restrict__ sums, int* __restrict__ maxes) {
  const unsigned b = blockIdx.x / groups;
  const int64_t img = (int64_t)b * hw;
  const int64_t base = (int64_t)(blockIdx.x - b * groups) * (SP_WG * SP_PPT) + threadIdx.x;
  int n[4] = {0, 0, 0, 0};                                                  // reliable, segments, removed pixels, removed segments
  int largest = 0;
#pragma unroll
  for (int j = 0; j < SP_PPT; ++j) {
    const int64_t p = base + (int64_t)j * SP_WG;
    if (p < hw) {
      const int l = label[img + p];
      const int s = l >= 0 ? total[img + l] : 0;
      const bool kept = l >= 0 && s > max_size, own = l == (int)p;
      size[img + p] = s;
      keep_out[img + p] = kept;
      n[0] += l >= 0;
      n[1] += own;
      n[2] += l >= 0 && !kept;
      n[3] += own && !kept;
      largest = max(largest, s);
    }
  }
  const auto sum = block_wave_sum(n);
  const int mx = sp_block_max(largest);
  if (threadIdx.x < 4) sums[(int64_t)blockIdx.x * 4 + threadIdx.x] = sum[threadIdx.x];
  if (threadIdx.x == 0) maxes[blockIdx.x] = mx;
}

// counts[b] = (reliable, segments, removed pixels, removed segments, largest); density[b] = float(double(reliable - removed) / double(H W))
__global__ __launch_bounds__(SP_WG) void speckle_finalize_kernel(const int* __restrict__ sums, const int* __restrict__ maxes, unsigned groups,
                                                                 double hw, int* __restrict__ counts, float* __restrict__ density) {
  const int b = blockIdx.x;
  long long v[4];
  gather_slots<SP_WG>(sums + (int64_t)b * groups * 4, groups, v);
  int largest = 0;
  for (unsigned s = threadIdx.x; s < groups; s += SP_WG) largest = max(largest, maxes[(int64_t)b * groups + s]);
  const auto sum = block_tree_sum<SP_WG>(v);
  const int mx = sp_block_max(largest);
  if (threadIdx.x < 4) counts[b * 5 + threadIdx.x] = (int)sum[threadIdx.x];
  if (threadIdx.x == 0) {
    counts[b * 5 + 4] = mx;
    density[b] = (float)((double)(sum[0] - sum[2]) / hw);
  }
}

static int64_t speckle_groups(int H, int W) { return ceil_div((int64_t)H * W, SP_WG * SP_PPT); }
// sizes >= 1 whose per-image index, tile grid and pixel grid all fit an int (no product here can pass 2^62)
static bool speckle_fits(int B, int H, int W) {
  const int64_t hw = (int64_t)H * W;
  return hw <= 0x7fffffffLL && B * ceil_div(W, SP_TC) * ceil_div(H, SP_TR) <= 0x7fffffffLL && ceil_div(B * hw, SP_WG) <= 0x7fffffffLL;
}

}  // namespace ragmi

extern "C" int64_t ragmi_speckle_workspace_elems(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || !ragmi::speckle_fits(B, H, W)) return 0;      // sizes that ragmi_speckle_fwd refuses
  return 3 * (int64_t)B * H * W + 5 * (int64_t)B * ragmi::speckle_groups(H, W);   // parent, lcount, total; five counts per workgroup
}

extern "C" int ragmi_speckle_fwd(const void* disp, const void* keep, int keep_kind, int B, int H, int W, int max_size, float max_diff,
                                 void* workspace, void* label, void* size, void* keep_out, void* counts, void* density, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(keep_kind == 0 || keep_kind == 1 || keep_kind == 2, RAGMI_EINVAL, "speckle: keep_kind = %d, must be 0 (fp32), 1 (uint8) or 2 (none)",
                keep_kind);
  RAGMI_REQUIRE(disp && (keep || keep_kind == 2) && workspace && label && size && keep_out && counts && density, RAGMI_EINVAL,
                "speckle: null pointer");
  RAGMI_REQUIRE(B >= 1 && H >= 1 && W >= 1, RAGMI_EINVAL, "speckle: bad size B=%d H=%d W=%d", B, H, W);
  RAGMI_REQUIRE(max_size >= 0, RAGMI_EINVAL, "speckle: max_size = %d, must not be negative", max_size);
  RAGMI_REQUIRE(std::isfinite(max_diff) && max_diff >= 0.f, RAGMI_EINVAL, "speckle: max_diff must be finite and not negative");
  RAGMI_REQUIRE(aligned_to(workspace, 4), RAGMI_EINVAL, "speckle: workspace not 4-byte aligned");
  const int64_t hw = (int64_t)H * W, tiles_x = ceil_div(W, SP_TC), tiles_y = ceil_div(H, SP_TR), groups = speckle_groups(H, W);
  const int64_t seams = (tiles_x - 1) * H + (tiles_y - 1) * W;              // per image
  RAGMI_REQUIRE(speckle_fits(B, H, W), RAGMI_EINVAL,
                "speckle: too many pixels (H W, B tiles and B H W / 256 must stay below 2^31)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* parent = (int*)workspace;
  int* lcount = parent + B * hw;
  int* total = lcount + B * hw;
  int* sums = total + B * hw;
  int* maxes = sums + 4 * B * groups;
  const dim3 wg(SP_WG), tiles((unsigned)(B * tiles_x * tiles_y)), pixels((unsigned)ceil_div(B * hw, SP_WG));
  auto tile = keep_kind == 0 ? speckle_tile_kernel<0> : keep_kind == 1 ? speckle_tile_kernel<1> : speckle_tile_kernel<2>;
  hipLaunchKernelGGL(tile, tiles, wg, 0, st, (const unsigned*)disp, keep, H, W, (unsigned)tiles_x, (unsigned)tiles_y, max_diff, parent, lcount,
                     total);
  if (seams > 0)
    hipLaunchKernelGGL(speckle_seam_kernel, dim3((unsigned)ceil_div(B * seams, SP_WG)), wg, 0, st, (const unsigned*)disp, H, W, (unsigned)tiles_x,
                       seams, B * seams, max_diff, parent);
  hipLaunchKernelGGL(speckle_flatten_kernel, pixels, wg, 0, st, (const int*)parent, (const int*)lcount, hw, B * hw, (int*)label, total);
  hipLaunchKernelGGL(speckle_apply_kernel, dim3((unsigned)(B * groups)), wg, 0, st, (const int*)label, (const int*)total, hw, (unsigned)groups,
                     max_size, (int*)size, (uint8_t*)keep_out, sums, maxes);
  hipLaunchKernelGGL(speckle_finalize_kernel, dim3((unsigned)B), wg, 0, st, (const int*)sums, (const int*)maxes, (unsigned)groups, (double)hw,
                     (int*)counts, (float*)density);
  return check_launch("speckle_fwd");
}
