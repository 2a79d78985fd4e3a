// Dense disparity from a disparity map and a keep map (the left-right check's): background interpolation along rows, then along
// columns for the rows that have nothing to interpolate from, and an optional 3x3 / 5x5 median.  Definition: include/rag_amd.h,
// DESIGN.md section 4.5.2.
//
// A pixel is reliable iff it is kept and its disparity is finite.  Everything below moves BIT PATTERNS: a value is an unsigned, "no
// reliable pixel seen yet" is DF_NONE (a NaN pattern, which no reliable value has), and the one float operation is the `<` that
// picks the farther of two reliable values.  A non-finite or unkept value therefore never travels.
//
// ragmi_disp_fill_fwd, three launches:
//   row pass     one wave per row, four rows per workgroup, the row in 64-column tiles.  A sweep from the right carries the nearest
//                reliable value to the right of every pixel (per tile: a ballot of "reliable", the nearest set bit, ONE shuffle; the
//                carry into the next tile is the tile's first reliable lane) and parks it in `out`, with a provisional code in
//                `code`; the sweep from the left then has every lane read
//                back ONLY what it wrote itself, combine it with the value carried from the left and overwrite it.  The row's
//                "has a reliable pixel" flag goes to the workspace; a row without one skips the second sweep.
//   column pass  the same grid; a row whose flag is set only contributes zeros.  An empty row looks its nearest non-empty rows up
//                in the flags (64 per step, one ballot) and copies from them; it reads rows the row pass completed and writes its own.
//   finalize     one workgroup per image folds the per-workgroup integer counts (codes 0-2 from the row pass, 3-5 from the column
//                pass) in the fixed order of reduce.h.
// No atomics, no memset, no memcpy; every output element and every workspace element that is read is written by the call.
// ragmi_disp_median_fwd: one launch, a 32 x 8 tile with its halo in LDS, a compare-exchange selection in registers.
#include <cmath>

#include "reduce.h"

namespace ragmi {

constexpr int DF_WG = 256;                   // threads per workgroup of every kernel here
constexpr int DF_ROWS = DF_WG / 64;          // rows per workgroup: one wave each
constexpr int DF_BATCH = 8;                  // tiles whose loads are issued together, ahead of their scans
constexpr unsigned DF_NONE = 0xffffffffu;    // no reliable value: a NaN pattern
constexpr unsigned DF_ONE = 0x3f800000u;     // 1.0f: the only pattern that compares == 1.0f

__device__ __forceinline__ bool df_finite(unsigned u) { return (u & 0x7f800000u) != 0x7f800000u; }
// (later < first) ? later : first on two reliable values: a tie or a signed zero takes `first`
__device__ __forceinline__ unsigned df_farther(unsigned later, unsigned first) {
  return __uint_as_float(later) < __uint_as_float(first) ? later : first;
}
// the value of the nearest reliable lane at or before this one (FROM_LEFT) or at or after it, DF_NONE if the tile has none on that
// side: `mask` is the wave's ballot of "reliable", so the lane is found with a count of leading / trailing zeros and fetched with
// ONE shuffle, whatever the distance.  v is read from reliable lanes only.
template <bool FROM_LEFT>
__device__ __forceinline__ unsigned df_nearest(unsigned v, unsigned long long mask, int lane) {
  const unsigned long long m = FROM_LEFT ? mask << (63 - lane) : mask >> lane;      // this lane's own bit at bit 63 / bit 0
  const int src = FROM_LEFT ? lane - __clzll((long long)m) : lane + __ffsll(m) - 1;
  const unsigned t = __shfl(v, m ? src : lane);
  return m ? t : DF_NONE;
}
// what the tile hands to the next one: the value of its first (FROM_LEFT: last) reliable lane, or the carry it received
template <bool FROM_LEFT>
__device__ __forceinline__ unsigned df_carry(unsigned v, unsigned long long mask, unsigned carry) {
  if (mask == 0) return carry;                                                      // uniform
  return __shfl(v, FROM_LEFT ? 63 - __clzll((long long)mask) : __ffsll(mask) - 1);
}

template <bool U8>
__global__ __launch_bounds__(DF_WG) void disp_fill_row_kernel(const unsigned* __restrict__ disp, const void* __restrict__ keep, int H, int W,
                                                              unsigned groups, int* __restrict__ row_flag, int* __restrict__ slots,
                                                              unsigned* __restrict__ out, uint8_t* __restrict__ code) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned b = blockIdx.x / groups;
  const int64_t y = (int64_t)(blockIdx.x - b * groups) * DF_ROWS + wave;
  int n[3] = {0, 0, 0};                                     // this lane's pixels of codes 0, 1, 2
  if (y < H) {                                              // uniform per wave
    const int64_t row = ((int64_t)b * H + y) * W;
    const int tiles = (int)(((int64_t)W + 63) >> 6);
    // from the right: out = the pixel's own value if reliable, else the nearest reliable value to its right (DF_NONE: none);
    // code = 0 / 1 / 2 for the three
    unsigned carry = DF_NONE;
    for (int t0 = tiles - 1; t0 >= 0; t0 -= DF_BATCH) {
      unsigned d[DF_BATCH], k[DF_BATCH];
#pragma unroll
      for (int j = 0; j < DF_BATCH; ++j) {
        const int64_t x = (int64_t)(t0 - j) * 64 + lane;
        d[j] = DF_NONE;
        k[j] = 0;
        if (t0 - j >= 0 && x < W) {
          d[j] = disp[row + x];
          k[j] = U8 ? (unsigned)(static_cast<const uint8_t*>(keep)[row + x] != 0)
                    : (unsigned)(static_cast<const unsigned*>(keep)[row + x] == DF_ONE);
        }
      }
#pragma unroll
      for (int j = 0; j < DF_BATCH; ++j) {
        if (t0 - j < 0) break;                              // uniform
        const int64_t x = (int64_t)(t0 - j) * 64 + lane;
        const bool reliable = k[j] && df_finite(d[j]);
        const unsigned long long mask = __ballot(reliable);
        unsigned v = df_nearest<false>(d[j], mask, lane);
        if (v == DF_NONE) v = carry;
        carry = df_carry<false>(d[j], mask, carry);         // off the chain from tile to tile: only the two selects depend on it
        if (x < W) {
          out[row + x] = v;
          code[row + x] = reliable ? 0 : (v != DF_NONE ? 1 : 2);
          n[0] += reliable;
        }
      }
    }
    const bool any = carry != DF_NONE;                      // lane 0 of the leftmost tile has seen the whole row
    if (lane == 0) row_flag[(int64_t)b * H + y] = any;
    if (any) {
      // from the left: every lane re-reads its own (out, code), so the order inside the thread is all the ordering it needs
      carry = DF_NONE;
      for (int t0 = 0; t0 < tiles; t0 += DF_BATCH) {
        unsigned p[DF_BATCH];
        int c[DF_BATCH];
#pragma unroll
        for (int j = 0; j < DF_BATCH; ++j) {
          const int64_t x = (int64_t)(t0 + j) * 64 + lane;
          p[j] = DF_NONE;
          c[j] = 2;
          if (x < W) {                                      // x < W implies t0 + j < tiles
            p[j] = out[row + x];
            c[j] = code[row + x];
          }
        }
#pragma unroll
        for (int j = 0; j < DF_BATCH; ++j) {
          if (t0 + j >= tiles) break;                       // uniform
          const int64_t x = (int64_t)(t0 + j) * 64 + lane;
          const bool reliable = c[j] == 0;                  // a lane past the row's end holds (DF_NONE, 2): it passes values on
          const unsigned long long mask = __ballot(reliable);
          unsigned v = df_nearest<true>(p[j], mask, lane);
          if (v == DF_NONE) v = carry;
          carry = df_carry<true>(p[j], mask, carry);
          if (x < W && !reliable) {
            const bool both = c[j] == 1 && v != DF_NONE;    // the row has a reliable pixel, so at least one side exists
            out[row + x] = both ? df_farther(p[j], v) : (c[j] == 1 ? p[j] : v);
            code[row + x] = both ? 1 : 2;
            n[both ? 1 : 2] += 1;
          }
        }
      }
    }
  }
  const auto sum = block_wave_sum(n);
  if (threadIdx.x < 3) slots[(int64_t)blockIdx.x * 6 + threadIdx.x] = sum[threadIdx.x];
}

__global__ __launch_bounds__(DF_WG) void disp_fill_col_kernel(int H, int W, unsigned groups, unsigned fill_bits,
                                                              const int* __restrict__ row_flag, int* __restrict__ slots,
                                                              unsigned* __restrict__ out, uint8_t* __restrict__ code) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned b = blockIdx.x / groups;
  const int64_t y = (int64_t)(blockIdx.x - b * groups) * DF_ROWS + wave;
  const int* flag = row_flag + (int64_t)b * H;
  int n[3] = {0, 0, 0};                                     // this lane's pixels of codes 3, 4, 5
  if (y < H && flag[y] == 0) {                              // uniform per wave: an empty row
    int64_t up = -1, down = -1;                             // the nearest non-empty rows; 64 flags per step
    for (int64_t base = y - 1; base >= 0 && up < 0; base -= 64) {
      const int64_t r = base - lane;
      const unsigned long long m = __ballot(r >= 0 && flag[r >= 0 ? r : 0] != 0);
      if (m) up = base - (__ffsll(m) - 1);
    }
    for (int64_t base = y + 1; base < H && down < 0; base += 64) {
      const int64_t r = base + lane;
      const unsigned long long m = __ballot(r < H && flag[r < H ? r : H - 1] != 0);
      if (m) down = base + (__ffsll(m) - 1);
    }
    const int64_t img = (int64_t)b * H * W;
    const unsigned* pu = out + img + (up >= 0 ? up : 0) * W;                    // rows the row pass completed; never row y
    const unsigned* pd = out + img + (down >= 0 ? down : 0) * W;
    const int c = (up >= 0 && down >= 0) ? 3 : (up >= 0 || down >= 0) ? 4 : 5;
    for (int64_t x = lane; x < W; x += 64) {
      unsigned v = fill_bits;
      if (c == 3) v = df_farther(pd[x], pu[x]);
      else if (c == 4) v = up >= 0 ? pu[x] : pd[x];
      out[img + y * W + x] = v;
      code[img + y * W + x] = (uint8_t)c;
      n[c - 3] += 1;
    }
  }
  const auto sum = block_wave_sum(n);
  if (threadIdx.x < 3) slots[(int64_t)blockIdx.x * 6 + 3 + threadIdx.x] = sum[threadIdx.x];
}

// counts[b, k] = the pixels of code k in image b; density[b] = float(double(counts[b, 0]) / double(H W)); one workgroup per image
__global__ __launch_bounds__(DF_WG) void disp_fill_finalize_kernel(const int* __restrict__ slots, unsigned groups, double hw,
                                                                   int* __restrict__ counts, float* __restrict__ density) {
  const int b = blockIdx.x;
  long long v[6];
  gather_slots<DF_WG>(slots + (int64_t)b * groups * 6, groups, v);
  const auto sum = block_tree_sum<DF_WG>(v);
  if (threadIdx.x < 6) counts[b * 6 + threadIdx.x] = (int)sum[threadIdx.x];
  if (threadIdx.x == 0) density[b] = (float)((double)sum[0] / hw);
}

// ------------------------------------------------------------------------------------------------------------------ median
constexpr int MED_TW = 32, MED_TH = 8;       // output tile of one workgroup: one pixel per thread

// smaller to a, larger to b; both results are copies of an input
__device__ __forceinline__ void df_cex(float& a, float& b) {
  const bool swap = b < a;
  const float lo = swap ? b : a, hi = swap ? a : b;
  a = lo;
  b = hi;
}
// the minimum of a[0..K) to a[0], the maximum to a[K-1]
template <int K>
__device__ __forceinline__ void df_minmax(float* a) {
#pragma unroll
  for (int i = 0; i < K / 2; ++i) df_cex(a[i], a[K - 1 - i]);
#pragma unroll
  for (int i = 1; i < (K + 1) / 2; ++i) df_cex(a[0], a[i]);
#pragma unroll
  for (int i = K / 2; i < K - 1; ++i) df_cex(a[i], a[K - 1]);
}
// median of N (odd) values by forgetful selection: among N/2 + 2 values neither the minimum nor the maximum can be the median of
// all N, so both are dropped and the next value joins; the last three leave the median in the middle.  a is destroyed.
template <int N>
__device__ __forceinline__ float df_median(float (&a)[N]) {
  constexpr int K0 = N / 2 + 2;
  static_for<K0 - 2>([&](auto s) {
    constexpr int S = decltype(s)::value;
    df_minmax<K0 - S>(&a[S]);
    if constexpr (K0 + S < N) a[K0 - 1] = a[K0 + S];
  });
  return a[K0 - 2];
}

__device__ __forceinline__ int64_t df_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int M>
__global__ __launch_bounds__(DF_WG) void disp_median_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                            unsigned tiles_x, unsigned tiles_y) {
  constexpr int R = M / 2, LW = MED_TW + 2 * R, LH = MED_TH + 2 * R;
  __shared__ float tile[LH][LW];
  const unsigned tx = blockIdx.x % tiles_x, rest = blockIdx.x / tiles_x;
  const unsigned ty = rest % tiles_y, b = rest / tiles_y;
  const int64_t x0 = (int64_t)tx * MED_TW, y0 = (int64_t)ty * MED_TH;
  const float* img = in + (int64_t)b * H * W;
  for (int i = threadIdx.x; i < LH * LW; i += DF_WG) {      // the tile and its halo, coordinates clamped to the image
    const int ly = i / LW, lx = i - ly * LW;
    const int64_t gy = df_clamp(y0 + ly - R, H - 1), gx = df_clamp(x0 + lx - R, W - 1);
    tile[ly][lx] = img[gy * W + gx];
  }
  __syncthreads();
  const int lx = threadIdx.x % MED_TW, ly = threadIdx.x / MED_TW;
  const int64_t x = x0 + lx, y = y0 + ly;
  if (x >= W || y >= H) return;
  float a[M * M];
#pragma unroll
  for (int j = 0; j < M; ++j)
#pragma unroll
    for (int i = 0; i < M; ++i) a[j * M + i] = tile[ly + j][lx + i];
  out[(int64_t)b * H * W + y * W + x] = df_median(a);
}

static int64_t disp_fill_groups(int H) { return ceil_div(H, DF_ROWS); }

}  // namespace ragmi

extern "C" int64_t ragmi_disp_fill_workspace_elems(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return (int64_t)B * H + 6 * (int64_t)B * ragmi::disp_fill_groups(H);         // a flag per row, six counts per workgroup
}

extern "C" int ragmi_disp_fill_fwd(const void* disp, const void* keep, int keep_is_u8, int B, int H, int W, float fill_value,
                                   void* workspace, void* out, void* code, void* counts, void* density, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(disp && keep && workspace && out && code && counts && density, RAGMI_EINVAL, "disp_fill: null pointer");
  RAGMI_REQUIRE(B >= 1 && H >= 1 && W >= 1, RAGMI_EINVAL, "disp_fill: bad size B=%d H=%d W=%d", B, H, W);
  RAGMI_REQUIRE(std::isfinite(fill_value), RAGMI_EINVAL, "disp_fill: fill_value must be finite");
  RAGMI_REQUIRE(aligned_to(workspace, 4), RAGMI_EINVAL, "disp_fill: workspace not 4-byte aligned");
  const int64_t groups = disp_fill_groups(H);
  RAGMI_REQUIRE(B * groups <= 0x7fffffffLL && (int64_t)H * W <= 0x7fffffffLL, RAGMI_EINVAL,
                "disp_fill: too many pixels (B ceil(H/4) and H W must stay below 2^31)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* row_flag = (int*)workspace;
  int* slots = row_flag + (int64_t)B * H;
  unsigned fill_bits;
  static_assert(sizeof(fill_bits) == sizeof(fill_value));
  __builtin_memcpy(&fill_bits, &fill_value, sizeof(fill_bits));
  const dim3 grid((unsigned)(B * groups)), wg(DF_WG);
  if (keep_is_u8)
    hipLaunchKernelGGL((disp_fill_row_kernel<true>), grid, wg, 0, st, (const unsigned*)disp, keep, H, W, (unsigned)groups, row_flag,
                       slots, (unsigned*)out, (uint8_t*)code);
  else
    hipLaunchKernelGGL((disp_fill_row_kernel<false>), grid, wg, 0, st, (const unsigned*)disp, keep, H, W, (unsigned)groups, row_flag,
                       slots, (unsigned*)out, (uint8_t*)code);
  hipLaunchKernelGGL(disp_fill_col_kernel, grid, wg, 0, st, H, W, (unsigned)groups, fill_bits, (const int*)row_flag, slots,
                     (unsigned*)out, (uint8_t*)code);
  hipLaunchKernelGGL(disp_fill_finalize_kernel, dim3((unsigned)B), wg, 0, st, (const int*)slots, (unsigned)groups,
                     (double)((int64_t)H * W), (int*)counts, (float*)density);
  return check_launch("disp_fill_fwd");
}

extern "C" int ragmi_disp_median_fwd(const void* in, void* out, int B, int H, int W, int m, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(in && out, RAGMI_EINVAL, "disp_median: null pointer");
  RAGMI_REQUIRE(in != out, RAGMI_EINVAL, "disp_median: in and out must differ (every pixel reads its neighbours)");
  RAGMI_REQUIRE(B >= 1 && H >= 1 && W >= 1, RAGMI_EINVAL, "disp_median: bad size B=%d H=%d W=%d", B, H, W);
  RAGMI_REQUIRE(m == 3 || m == 5, RAGMI_EINVAL, "disp_median: m = %d, must be 3 or 5", m);
  const int64_t tiles_x = ceil_div(W, MED_TW), tiles_y = ceil_div(H, MED_TH);
  RAGMI_REQUIRE(tiles_x * tiles_y <= 0x7fffffffLL && B * tiles_x * tiles_y <= 0x7fffffffLL, RAGMI_EINVAL, "disp_median: too many pixels");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(B * tiles_x * tiles_y)), wg(DF_WG);
  if (m == 3)
    hipLaunchKernelGGL((disp_median_kernel<3>), grid, wg, 0, st, (const float*)in, (float*)out, H, W, (unsigned)tiles_x, (unsigned)tiles_y);
  else
    hipLaunchKernelGGL((disp_median_kernel<5>), grid, wg, 0, st, (const float*)in, (float*)out, H, W, (unsigned)tiles_x, (unsigned)tiles_y);
  return check_launch("disp_median_fwd");
}
