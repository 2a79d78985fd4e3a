// Batch preparation on the device: what the reference's loaders do per sample on the host, from the decoded bytes to the
// network's fp32 inputs (src/dataloaders/data_io.py:6-13, stereo_dataset.py:35-38, 57-121;
// src_self/dataloaders/sceneflow_driving_dataset.py:53-70).
//
//   prep_batch     [B,Hs,Ws,3] uint8 (left, right) + gt (uint16 or fp32) -> [B,3,H,W] fp32 + [B,H,W] fp32, ONE launch.  Output pixel
//                  (y, x) of sample b reads source pixel (y + origin[b,0], x + origin[b,1]) and is 0 outside the source: the
//                  training crop (origin = (y1, x1)) and the evaluation pad (origin = (-top_pad, 0), 0 AFTER normalisation) are
//                  the same rule.  The value is ToTensor + Normalize in fp32: ((float)u / 255 - mean_c) / std_c with two true
//                  divisions.  It is a function of (channel, byte) alone, so every workgroup builds the 3 x 256 table in LDS with
//                  exactly that expression and the pixels are lookups: bit-identical by construction.  With colour statistics
//                  the byte first goes through transfer_color's float64 sequence, truncated to a uint8 level as the reference
//                  stores it; the table is then per (sample, view) and the transferred image never exists in memory.
//   color_stats    mean and std-of-column-stds per channel, float64 [B,3,2].  The column sums of u and u^2 are integers, so
//                  they are accumulated EXACTLY in 64-bit integers (any order gives the same bits): a column's population
//                  variance is (Hs S2 - S1^2) / (255 Hs)^2 with an exact numerator, and the mean is an exact integer sum
//                  divided once.  The std over the column stds is the reference's two-pass form in double, reduced in the
//                  fixed order of reduce.h (strided, then an LDS tree) by one workgroup per sample.
//   color_transfer the stand-alone uint8 image of transfer_color (tests, callers that want the image).
#include "prep_common.h"
#include "reduce.h"

namespace ragmi {

constexpr int PREP_WG = 256;                 // threads per workgroup, every kernel of this file
constexpr int PREP_ROWS = 4;                 // output rows per workgroup of prep_batch (amortises the table)
constexpr int PREP_TW = 4 * PREP_WG;         // output columns per workgroup: 4 per thread
constexpr int PREP_SEG = 3 * PREP_TW + 8;    // staged source bytes of one row segment (+ up to 3 bytes of alignment shift)
constexpr int CS_ROWS = 32;                  // source rows per partial of color_stats

// transfer_color's per-pixel sequence for byte u of a channel with statistics (tm, ts) against (sm, ss), in float64 and in the
// reference's order: t = u/255; t -= tm; t /= ts/ss; t += sm; clip(t, 0, 1); (t*255) truncated.  ts == 0 (a constant channel)
// divides by zero in the reference and its cast of NaN is undefined: here such a level is some value in 0..255, never a fault.
__device__ __forceinline__ int transfer_level(int u, double tm, double ts, double sm, double ss) {
#pragma clang fp contract(off)
  double t = (double)u / 255.0;
  t = t - tm;
  t = t / (ts / ss);
  t = t + sm;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  t = t * 255.0;
  return (t >= 0.0 && t <= 255.0) ? (int)t : 0;        // NaN lands here
}

struct PrepArgs {
  const uint8_t* src[2];      // left, right: [B,Hs,Ws,3]
  float* dst[2];              // [B,3,H,W]
  const double* stats[2];     // (mean, std) of each view [B,3,2], or null
  const double* stats_src;    // of the real image [B,3,2], or null: no colour transfer
  const void* gt;             // [B,Hs,Ws] uint16 or fp32, or null
  float* gt_dst;              // [B,H,W]
  const int* origin;          // [B,2] (y, x), device
  float gt_scale;
  float mean[3], std[3];
  int nviews, B, Hs, Ws, H, W;
};

// grid: (column chunks of PREP_TW, row groups of PREP_ROWS, B * (nviews + has_gt)); VEC: W % 4 == 0 and 16-byte aligned outputs
template <bool VEC, bool GT16>
__global__ __launch_bounds__(PREP_WG) void prep_batch_kernel(const PrepArgs a) {
  __shared__ float table[3 * 256];
  __shared__ __attribute__((aligned(4))) uint8_t seg[PREP_ROWS][PREP_SEG];
  const int tid = threadIdx.x;
  const int planes = a.nviews + (a.gt ? 1 : 0);
  const int b = blockIdx.z / planes, v = blockIdx.z % planes;
  const int64_t oy = a.origin[2 * b], ox = a.origin[2 * b + 1];
  const int cx0 = blockIdx.x * PREP_TW, cx1 = min(cx0 + PREP_TW, a.W);
  const int y0 = blockIdx.y * PREP_ROWS;
  // output columns of this chunk that have a source pixel: [vlo, vhi)
  const int64_t vlo = max((int64_t)cx0, -ox), vhi = min((int64_t)cx1, (int64_t)a.Ws - ox);

  if (v == a.nviews) {                         // ground truth: convert, scale, place
    float* dst = a.gt_dst + (int64_t)b * a.H * a.W;
    for (int r = 0; r < PREP_ROWS; ++r) {
      const int y = y0 + r;
      if (y >= a.H) break;
      const int64_t sy = y + oy;
      const bool row_ok = sy >= 0 && sy < a.Hs;
      const int64_t srow = ((int64_t)b * a.Hs + (row_ok ? sy : 0)) * a.Ws;
      auto load = [&](int x) -> float {
        if (!row_ok || x < vlo || x >= vhi) return 0.f;
        const int64_t i = srow + x + ox;
        const float g = GT16 ? (float)((const uint16_t*)a.gt)[i] : ((const float*)a.gt)[i];
        return g * a.gt_scale;
      };
      if (VEC) {
        const int x = cx0 + 4 * tid;
        if (x < cx1) *reinterpret_cast<float4*>(dst + (int64_t)y * a.W + x) = make_float4(load(x), load(x + 1), load(x + 2), load(x + 3));
      } else {
        for (int x = cx0 + tid; x < cx1; x += PREP_WG) dst[(int64_t)y * a.W + x] = load(x);
      }
    }
    return;
  }

  // ---- the table of this (sample, view): 3 entries per thread
  {
    const bool color = a.stats_src != nullptr;
    for (int e = tid; e < 3 * 256; e += PREP_WG) {
      const int c = e >> 8, u = e & 255;
      int level = u;
      if (color) {
        const double* st = a.stats[v] + (int64_t)b * 6 + 2 * c;
        const double* ss = a.stats_src + (int64_t)b * 6 + 2 * c;
        level = transfer_level(u, st[0], st[1], ss[0], ss[1]);
      }
      table[e] = normalize_level(level, a.mean[c], a.std[c]);
    }
  }
  // ---- stage the source bytes of each row's valid segment: head bytes up to a 4-byte boundary, whole words, tail bytes.  The
  // segment sits in LDS at the same offset modulo 4 as in memory, so an aligned word in memory is an aligned word in LDS.
  const uint8_t* src = a.src[v];
  const int nbytes = vhi > vlo ? (int)(3 * (vhi - vlo)) : 0;
  int shift[PREP_ROWS];
#pragma unroll
  for (int r = 0; r < PREP_ROWS; ++r) {
    shift[r] = 0;
    const int64_t sy = (int64_t)y0 + r + oy;
    if (y0 + r >= a.H || sy < 0 || sy >= a.Hs || nbytes == 0) continue;
    const uint8_t* p = src + (((int64_t)b * a.Hs + sy) * a.Ws + (vlo + ox)) * 3;
    const int sh = (int)(reinterpret_cast<uintptr_t>(p) & 3);
    shift[r] = sh;
    const int head = min((4 - sh) & 3, nbytes);
    const int nwords = (nbytes - head) >> 2;
    const int tail0 = head + 4 * nwords;
    if (tid < head) seg[r][sh + tid] = p[tid];
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(p + head);
    uint32_t* sw = reinterpret_cast<uint32_t*>(&seg[r][sh + head]);
    for (int k = tid; k < nwords; k += PREP_WG) sw[k] = pw[k];
    if (tid < nbytes - tail0) seg[r][sh + tail0 + tid] = p[tail0 + tid];
  }
  __syncthreads();

  float* dst = a.dst[v] + (int64_t)b * 3 * a.H * a.W;
  const int64_t plane = (int64_t)a.H * a.W;
#pragma unroll
  for (int r = 0; r < PREP_ROWS; ++r) {
    const int y = y0 + r;
    if (y >= a.H) break;
    const int64_t sy = y + oy;
    const bool row_ok = sy >= 0 && sy < a.Hs;
    const uint8_t* s = &seg[r][shift[r]];
    float* drow = dst + (int64_t)y * a.W;
    if (VEC) {
      const int x = cx0 + 4 * tid;
      if (x < cx1) {
        float o[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool ok = row_ok && x + k >= vlo && x + k < vhi;
          const int i = ok ? 3 * (int)(x + k - vlo) : 0;
#pragma unroll
          for (int c = 0; c < 3; ++c) o[c][k] = ok ? table[c * 256 + s[i + c]] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(drow + c * plane + x) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
      }
    } else {
      for (int x = cx0 + tid; x < cx1; x += PREP_WG) {
        const bool ok = row_ok && x >= vlo && x < vhi;
        const int i = ok ? 3 * (int)(x - vlo) : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) drow[c * plane + x] = ok ? table[c * 256 + s[i + c]] : 0.f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ colour statistics
static int color_stats_chunks(int Hs) { return (int)ceil_div(Hs, CS_ROWS); }

// partial[b][chunk][col*3+c] = (sum u, sum u^2) over the chunk's rows, exact.  grid: (ceil(Ws*3 / WG), chunks, B)
__global__ __launch_bounds__(PREP_WG) void color_stats_partial_kernel(const uint8_t* __restrict__ img, int Hs, int Ws,
                                                                      unsigned long long* __restrict__ partial) {
  const int n = 3 * Ws;
  const int j = blockIdx.x * PREP_WG + threadIdx.x;
  if (j >= n) return;
  const int b = blockIdx.z, ch = blockIdx.y, nch = gridDim.y;
  const int r0 = ch * CS_ROWS, r1 = min(r0 + CS_ROWS, Hs);
  const uint8_t* p = img + ((int64_t)b * Hs + r0) * n + j;
  unsigned s1 = 0, s2 = 0;                       // CS_ROWS * 255^2 fits easily
  for (int r = r0; r < r1; ++r, p += n) {
    const unsigned u = *p;
    s1 += u;
    s2 += u * u;
  }
  unsigned long long* o = partial + (((int64_t)b * nch + ch) * n + j) * 2;
  o[0] = s1;
  o[1] = s2;
}

// one workgroup per sample: out[b][c] = (mean, std over columns of the column stds)
__global__ __launch_bounds__(PREP_WG) void color_stats_finalize_kernel(const unsigned long long* __restrict__ partial, int nch, int Hs,
                                                                       int Ws, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, tid = threadIdx.x, n = 3 * Ws;
  const unsigned long long* pb = partial + (int64_t)b * nch * n * 2;
  const double inv = 1.0 / ((double)Hs * 255.0);
  // the exact population std of column x, channel c (of u / 255)
  auto colstd = [&](int x, int c, unsigned long long* sum1) -> double {
    unsigned long long s1 = 0, s2 = 0;
    for (int k = 0; k < nch; ++k) {
      const unsigned long long* q = pb + ((int64_t)k * n + 3 * x + c) * 2;
      s1 += q[0];
      s2 += q[1];
    }
    if (sum1) *sum1 += s1;
    return sqrt((double)((unsigned long long)Hs * s2 - s1 * s1)) * inv;      // Hs * S2 >= S1^2 (Cauchy-Schwarz), exact in 64 bits
  };
  unsigned long long t1[3] = {0, 0, 0};
  double sd[3] = {0.0, 0.0, 0.0};
  for (int x = tid; x < Ws; x += PREP_WG)
    for (int c = 0; c < 3; ++c) sd[c] += colstd(x, c, &t1[c]);
  const auto sum_i = block_tree_sum<PREP_WG>(t1);                     // exact: u64 (reduce.h)
  const auto sum_s = block_tree_sum<PREP_WG>(sd);
  double m[3];
  for (int c = 0; c < 3; ++c) m[c] = sum_s[c] / (double)Ws;           // mean of the column stds
  __syncthreads();                                                    // every thread has read sum_s: the double tree's LDS is refilled below
  for (int c = 0; c < 3; ++c) sd[c] = 0.0;
  for (int x = tid; x < Ws; x += PREP_WG)
    for (int c = 0; c < 3; ++c) {
      const double d = colstd(x, c, nullptr) - m[c];
      sd[c] += d * d;
    }
  const auto sum_d = block_tree_sum<PREP_WG>(sd);
  if (tid < 3) {
    out[(int64_t)b * 6 + 2 * tid] = (double)sum_i[tid] / ((double)Hs * (double)Ws * 255.0);
    out[(int64_t)b * 6 + 2 * tid + 1] = sqrt(sum_d[tid] / (double)Ws);
  }
}

// ------------------------------------------------------------------------------------------------ stand-alone transfer
// out = transfer_color(target) as uint8, [B,H,W,3]; n = H*W*3 bytes per sample.  grid: (chunks, B); VEC: n % 4 == 0, aligned
template <bool VEC>
__global__ __launch_bounds__(PREP_WG) void color_transfer_kernel(const uint8_t* __restrict__ in, const double* __restrict__ st,
                                                                 const double* __restrict__ ss, uint8_t* __restrict__ out, int64_t n) {
  __shared__ uint8_t lut[3 * 256];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int e = tid; e < 3 * 256; e += PREP_WG) {
    const int c = e >> 8;
    const double* t = st + (int64_t)b * 6 + 2 * c;
    const double* s = ss + (int64_t)b * 6 + 2 * c;
    lut[e] = (uint8_t)transfer_level(e & 255, t[0], t[1], s[0], s[1]);
  }
  __syncthreads();
  const uint8_t* pi = in + (int64_t)b * n;
  uint8_t* po = out + (int64_t)b * n;
  if (VEC) {
    for (int64_t j = 4 * ((int64_t)blockIdx.x * PREP_WG + tid); j < n; j += 4 * (int64_t)gridDim.x * PREP_WG) {
      const uchar4 u = *reinterpret_cast<const uchar4*>(pi + j);
      const int c = (int)(j % 3);
      uchar4 o;
      o.x = lut[c * 256 + u.x];
      o.y = lut[((c + 1) % 3) * 256 + u.y];
      o.z = lut[((c + 2) % 3) * 256 + u.z];
      o.w = lut[c * 256 + u.w];
      *reinterpret_cast<uchar4*>(po + j) = o;
    }
  } else {
    for (int64_t j = (int64_t)blockIdx.x * PREP_WG + tid; j < n; j += (int64_t)gridDim.x * PREP_WG) po[j] = lut[(int)(j % 3) * 256 + pi[j]];
  }
}

}  // namespace ragmi

extern "C" int ragmi_prep_batch(const void* left_u8, const void* right_u8, const void* gt, int gt_dtype, float gt_scale, const void* origin,
                                void* left, void* right, void* gt_out, int B, int Hs, int Ws, int H, int W, float mean0, float mean1,
                                float mean2, float std0, float std1, float std2, const void* stats_left, const void* stats_right,
                                const void* stats_source, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(left_u8 && left && origin, RAGMI_EINVAL, "prep_batch: null pointer (left_u8, left, origin)");
  RAGMI_REQUIRE((right_u8 == nullptr) == (right == nullptr), RAGMI_EINVAL, "prep_batch: right_u8 and right go together (one is a null pointer)");
  RAGMI_REQUIRE((gt == nullptr) == (gt_out == nullptr), RAGMI_EINVAL, "prep_batch: gt and gt_out go together (one is a null pointer)");
  RAGMI_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, RAGMI_EINVAL, "prep_batch: bad size B=%d src %dx%d out %dx%d", B, Hs, Ws, H, W);
  RAGMI_REQUIRE(!gt || gt_dtype == RAGMI_GT_F32 || gt_dtype == RAGMI_GT_U16, RAGMI_EUNSUPPORTED,
                "prep_batch: gt dtype %d not built (RAGMI_GT_F32 or RAGMI_GT_U16)", gt_dtype);
  if (stats_source || stats_left || stats_right)
    RAGMI_REQUIRE(stats_source && stats_left && (stats_right != nullptr) == (right_u8 != nullptr), RAGMI_EINVAL,
                  "prep_batch: colour transfer needs the statistics of every view given and of the source image (null pointer)");
  RAGMI_REQUIRE(aligned_to(left, 4) && aligned_to(right, 4) && aligned_to(gt_out, 4) && aligned_to(origin, 4) &&
                    aligned_to(gt, gt_dtype == RAGMI_GT_U16 ? 2 : 4) && aligned_to(stats_left, 8) && aligned_to(stats_right, 8) &&
                    aligned_to(stats_source, 8),
                RAGMI_EINVAL, "prep_batch: misaligned pointer");
  const int planes = (right_u8 ? 2 : 1) + (gt ? 1 : 0);
  const int64_t gy = ceil_div(H, PREP_ROWS), gz = (int64_t)B * planes;
  RAGMI_REQUIRE(gy <= 65535 && gz <= 65535, RAGMI_EINVAL, "prep_batch: grid too large (H=%d, B=%d)", H, B);
  PrepArgs a;
  a.src[0] = (const uint8_t*)left_u8; a.src[1] = (const uint8_t*)right_u8;
  a.dst[0] = (float*)left; a.dst[1] = (float*)right;
  a.stats[0] = (const double*)stats_left; a.stats[1] = (const double*)stats_right;
  a.stats_src = (const double*)stats_source;
  a.gt = gt; a.gt_dst = (float*)gt_out; a.origin = (const int*)origin; a.gt_scale = gt_scale;
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
  a.std[0] = std0; a.std[1] = std1; a.std[2] = std2;
  a.nviews = right_u8 ? 2 : 1; a.B = B; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W;
  const bool vec = W % 4 == 0 && aligned_to(left, 16) && aligned_to(right, 16) && aligned_to(gt_out, 16);
  const bool gt16 = gt && gt_dtype == RAGMI_GT_U16;
  const dim3 grid((unsigned)ceil_div(W, PREP_TW), (unsigned)gy, (unsigned)gz);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec && gt16) hipLaunchKernelGGL((prep_batch_kernel<true, true>), grid, dim3(PREP_WG), 0, st, a);
  else if (vec) hipLaunchKernelGGL((prep_batch_kernel<true, false>), grid, dim3(PREP_WG), 0, st, a);
  else if (gt16) hipLaunchKernelGGL((prep_batch_kernel<false, true>), grid, dim3(PREP_WG), 0, st, a);
  else hipLaunchKernelGGL((prep_batch_kernel<false, false>), grid, dim3(PREP_WG), 0, st, a);
  return check_launch("prep_batch");
}

extern "C" int64_t ragmi_color_stats_workspace_elems(int B, int Hs, int Ws) {
  if (B <= 0 || Hs <= 0 || Ws <= 0) return 0;
  return (int64_t)B * ragmi::color_stats_chunks(Hs) * 3 * Ws * 2;      // 8-byte elements: (sum u, sum u^2) per (chunk, column, channel)
}

extern "C" int ragmi_color_stats(const void* img_u8, int B, int Hs, int Ws, void* workspace, void* stats, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(img_u8 && workspace && stats, RAGMI_EINVAL, "color_stats: null pointer");
  RAGMI_REQUIRE(B > 0 && Hs > 0 && Ws > 0, RAGMI_EINVAL, "color_stats: bad size B=%d %dx%d", B, Hs, Ws);
  RAGMI_REQUIRE(aligned_to(workspace, 8) && aligned_to(stats, 8), RAGMI_EINVAL, "color_stats: workspace / stats not 8-byte aligned");
  // Hs * S2 <= Hs^2 * 255^2 must fit 64 bits, and a chunk's sums 32 bits: true far beyond any image
  const int nch = color_stats_chunks(Hs);
  RAGMI_REQUIRE(Hs <= (1 << 23) && nch <= 65535 && B <= 65535, RAGMI_EINVAL, "color_stats: image too large (B=%d, Hs=%d)", B, Hs);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(color_stats_partial_kernel, dim3((unsigned)ceil_div(3 * (int64_t)Ws, PREP_WG), (unsigned)nch, (unsigned)B), dim3(PREP_WG), 0,
                     st, (const uint8_t*)img_u8, Hs, Ws, (unsigned long long*)workspace);
  hipLaunchKernelGGL(color_stats_finalize_kernel, dim3((unsigned)B), dim3(PREP_WG), 0, st, (const unsigned long long*)workspace, nch, Hs, Ws,
                     (double*)stats);
  return check_launch("color_stats");
}

extern "C" int ragmi_color_transfer(const void* target_u8, const void* stats_target, const void* stats_source, void* out_u8, int B, int H,
                                    int W, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(target_u8 && stats_target && stats_source && out_u8, RAGMI_EINVAL, "color_transfer: null pointer");
  RAGMI_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535, RAGMI_EINVAL, "color_transfer: bad size B=%d %dx%d", B, H, W);
  RAGMI_REQUIRE(aligned_to(stats_target, 8) && aligned_to(stats_source, 8), RAGMI_EINVAL, "color_transfer: statistics not 8-byte aligned");
  const int64_t n = (int64_t)H * W * 3;
  const bool vec = n % 4 == 0 && aligned_to(target_u8, 4) && aligned_to(out_u8, 4);
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, (vec ? 16 : 4) * PREP_WG), 4096));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(color_transfer_kernel<true>, dim3(gx, (unsigned)B), dim3(PREP_WG), 0, st, (const uint8_t*)target_u8,
                       (const double*)stats_target, (const double*)stats_source, (uint8_t*)out_u8, n);
  else
    hipLaunchKernelGGL(color_transfer_kernel<false>, dim3(gx, (unsigned)B), dim3(PREP_WG), 0, st, (const uint8_t*)target_u8,
                       (const double*)stats_target, (const double*)stats_source, (uint8_t*)out_u8, n);
  return check_launch("color_transfer");
}
