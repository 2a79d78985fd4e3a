// Lanczos resize on the device, alone and fused into batch preparation: the Cityscapes branch of the reference's loaders
// (src_self/dataloaders/stereo_dataset.py:56-69: left / right / disparity .resize((1024, 512), Image.ANTIALIAS) before the crop or
// pad, disparity / 256 / 2).  The arithmetic is Pillow's (src/libImaging/Resample.c), bit for bit:
//   8-bit (RGB)   int32 accumulator 2^21 + sum px * K, K = the float64 tap * 2^22 rounded half away from zero; clip8(acc >> 22)
//   16-bit (I;16) double accumulator from 0.0, acc += px * k with product and sum rounded separately (never fused), in ascending
//                 tap order; r = (int)(acc +- 0.5); the two bytes clip8(r % 256) and clip8(r >> 8) are clipped SEPARATELY
//   the horizontal pass first, STORED as uint8 / uint16, then the vertical pass on those values.
// The taps come from the host (rag_amd.data.lanczos_taps: Pillow's precompute_coeffs in float64): per axis bounds int32 [m,2] =
// (first source index, tap count), int32 [m,ksize] fixed-point taps, float64 [m,ksize] taps.
//
// ONE kernel serves the three entry points.  A workgroup owns a PR_TH x PR_TW tile of one output plane (a view or the ground truth
// of one sample).  It reads its origin from the device, looks up the source rows and columns its tile needs from the bounds
// tables, stages that window of source bytes in LDS, runs the horizontal pass into an LDS intermediate (uint8 / uint16, as Pillow
// stores it) and the vertical pass from there into the epilogue: prep.hip's normalisation table and fp32 CHW stores (fused), or
// the resized bytes themselves (stand-alone).  The resized image never reaches HBM in the fused form.
//
// Memory safety does not rest on the tables: every bound read from them is clamped to the source size and to the LDS window the
// host sized (from its OWN evaluation of the bounds formula), so wrong tables give wrong pixels, never an access out of bounds.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "prep_common.h"

namespace ragmi {

constexpr int PR_WG = 256;                   // threads per workgroup
constexpr int PR_TH = 16, PR_TW = 64;        // output tile: at x0.5 a 42 x 138-pixel source window (17.6 KB of RGB) + an 8 KB intermediate
constexpr int PR_RB = 4;                     // source rows per thread item of the horizontal pass (a tap is read once for 4 rows)
constexpr int64_t PR_LDS_MAX = 160 * 1024;   // one workgroup may hold the whole LDS of a CU

// the two pixel arithmetics
template <bool U16> struct Px;
template <> struct Px<false> {
  typedef uint8_t elem;
  typedef int32_t tap;
  typedef int32_t acc;
  static constexpr int C = 3;
  static __device__ __forceinline__ acc init() { return 1 << 21; }
  static __device__ __forceinline__ acc mac(acc a, int px, tap k) { return a + px * k; }
  static __device__ __forceinline__ int finish(acc a) {
    const int v = a >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
  }
};
template <> struct Px<true> {
  typedef uint16_t elem;
  typedef double tap;
  typedef double acc;
  static constexpr int C = 1;
  static __device__ __forceinline__ acc init() { return 0.0; }
  static __device__ __forceinline__ acc mac(acc a, int px, tap k) {
#pragma clang fp contract(off)
    const double p = (double)px * k;                  // the product is rounded, then the sum: never an fma (__dmul_rn / __dadd_rn are
    return a + p;                                     // plain operators here and contract under hipcc's default)
  }
  static __device__ __forceinline__ int finish(acc a) {
    const int r = (int)(a < 0.0 ? a - 0.5 : a + 0.5);
    int lo = r % 256, hi = r >> 8;                    // C remainder sign, arithmetic shift: a negative overshoot gives 0
    lo = lo < 0 ? 0 : (lo > 255 ? 255 : lo);
    hi = hi < 0 ? 0 : (hi > 255 ? 255 : hi);          // past 65535 only the high byte saturates
    return (hi << 8) | lo;
  }
};

struct ResizeArgs {
  const uint8_t* src[2];      // views: [B,Hs,Ws,3] uint8
  const uint16_t* gt;         // [B,Hs,Ws] uint16, or null
  void* dst[3];               // fused: fp32 [B,3,H,W] per view, [B,H,W] gt; stand-alone: the resized uint8 / uint16 image
  const int* origin;          // [B,2] (y, x) into the RESIZED image, device; null: (0, 0)
  const int* yb;              // bounds [Hr,2]
  const int* xb;              // bounds [Wr,2]
  const int32_t* yki;         // fixed-point taps [Hr,yks] (views)
  const int32_t* xki;
  const double* ykd;          // float64 taps (gt)
  const double* xkd;
  float gt_scale;
  float mean[3], std[3];
  int nviews, yks, xks, Hs, Ws, Hr, Wr, H, W;
  int cap_h, cap_w;           // LDS window: source rows / columns (pixels)
};

// dynamic LDS: [taps y | taps x] (8-byte slots) [table 3 x 256 fp32] [bounds] [source window] [intermediate]
struct LdsLayout {
  int64_t tapy, tapx, table, bnd, src, mid, total;
  int src_pitch;              // bytes per staged source row
};
__host__ __device__ inline LdsLayout lds_layout(int cap_h, int cap_w, int yks, int xks) {
  LdsLayout l;
  l.tapy = 0;
  l.tapx = l.tapy + (int64_t)PR_TH * yks * 8;
  l.table = l.tapx + (int64_t)PR_TW * xks * 8;
  l.bnd = l.table + 3 * 256 * 4;
  l.src = l.bnd + (PR_TH + PR_TW) * 2 * 4;
  l.src_pitch = (cap_w * 3 + 4 + 3) & ~3;                           // + up to 3 bytes of alignment shift, a multiple of 4
  l.mid = l.src + (int64_t)cap_h * l.src_pitch;
  l.total = l.mid + (((int64_t)cap_h * PR_TW * 3 + 7) & ~(int64_t)7);
  return l;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One tile of one plane.  RAW: write the resized image itself (origin (0,0), H x W = Hr x Wr); else the normalised fp32 planes.
template <bool U16, bool RAW, bool VEC>
__device__ __forceinline__ void resize_tile(const ResizeArgs& a, unsigned char* lds, const uint8_t* src_plane, void* dst_plane, int b, int v) {
  typedef Px<U16> P;
  typedef typename P::elem elem;
  typedef typename P::tap tap;
  typedef typename P::acc acc_t;
  constexpr int C = P::C, BPP = C * (int)sizeof(elem);
  const LdsLayout L = lds_layout(a.cap_h, a.cap_w, a.yks, a.xks);
  tap* tapy = reinterpret_cast<tap*>(lds + L.tapy);
  tap* tapx = reinterpret_cast<tap*>(lds + L.tapx);
  float* table = reinterpret_cast<float*>(lds + L.table);
  int* by = reinterpret_cast<int*>(lds + L.bnd);
  int* bx = by + 2 * PR_TH;
  unsigned char* srcl = lds + L.src;
  elem* mid = reinterpret_cast<elem*>(lds + L.mid);
  constexpr int MIDP = PR_TW * C;                                    // elements per intermediate row
  const int tid = threadIdx.x;

  int64_t oy = 0, ox = 0;
  if (a.origin) { oy = a.origin[2 * b]; ox = a.origin[2 * b + 1]; }
  const int ty0 = blockIdx.y * PR_TH, tx0 = blockIdx.x * PR_TW;
  const int th = min(PR_TH, a.H - ty0), tw = min(PR_TW, a.W - tx0);
  // rows / columns of the resized image under this tile: [ry0, ry1) x [rx0, rx1)
  // (clamped to [0, Hr] x [0, Wr] in 64 bits BEFORE the narrowing: an origin near +-2^31 must not wrap into a valid index)
  auto clip = [](int64_t v, int n) { return (int)max((int64_t)0, min((int64_t)n, v)); };
  const int ry0 = clip(ty0 + oy, a.Hr), ry1 = clip(ty0 + oy + th, a.Hr);
  const int rx0 = clip(tx0 + ox, a.Wr), rx1 = clip(tx0 + ox + tw, a.Wr);
  const bool empty = ry1 <= ry0 || rx1 <= rx0;
  const int ny = empty ? 0 : ry1 - ry0, nx = empty ? 0 : rx1 - rx0;

  if (!RAW && !U16)
    for (int e = tid; e < 3 * 256; e += PR_WG) table[e] = normalize_level(e & 255, a.mean[e >> 8], a.std[e >> 8]);

  if (!empty) {
    // ---- bounds of the tile's outputs relative to its window, clamped to the source and to the window; the tile's taps
    const int ys_lo = clampi(a.yb[2 * ry0], 0, a.Hs), xs_lo = clampi(a.xb[2 * rx0], 0, a.Ws);
    auto bounds = [&](const int* tb, int i, int n, int ks, int lo, int cap, int* out) {
      const int mn = clampi(tb[2 * i], 0, n);
      int len = clampi(tb[2 * i + 1], 0, min(n - mn, ks));
      const int rel = clampi(mn - lo, 0, cap);
      len = min(len, min(cap - rel, n - lo - rel));
      out[0] = rel;
      out[1] = max(len, 0);
    };
    if (tid < ny) bounds(a.yb, ry0 + tid, a.Hs, a.yks, ys_lo, a.cap_h, by + 2 * tid);
    else if (tid >= PR_WG - nx) { const int t = tid - (PR_WG - nx); bounds(a.xb, rx0 + t, a.Ws, a.xks, xs_lo, a.cap_w, bx + 2 * t); }
    {
      const tap* gy = (U16 ? (const tap*)a.ykd : (const tap*)a.yki) + (int64_t)ry0 * a.yks;
      const tap* gx = (U16 ? (const tap*)a.xkd : (const tap*)a.xki) + (int64_t)rx0 * a.xks;
      for (int i = tid; i < ny * a.yks; i += PR_WG) tapy[i] = gy[i];
      for (int i = tid; i < nx * a.xks; i += PR_WG) tapx[i] = gx[i];
    }
    __syncthreads();
    // the bounds are monotonic in the output index, so the last output's end is the window's
    const int nrows = by[2 * (ny - 1)] + by[2 * (ny - 1) + 1], ncols = bx[2 * (nx - 1)] + bx[2 * (nx - 1) + 1];

    // ---- stage the window: one source row per wave at a time; head bytes up to a 4-byte boundary, whole words, tail bytes.  A row
    // sits in LDS at the same offset modulo 4 as in memory, so an aligned word in memory is an aligned word in LDS.
    const uint8_t* p0 = src_plane + (((int64_t)b * a.Hs + ys_lo) * a.Ws + xs_lo) * BPP;
    const int sh0 = (int)(reinterpret_cast<uintptr_t>(p0) & 3), rowstep = (int)(((int64_t)a.Ws * BPP) & 3);
    {
      const int lane = tid & 63, nbytes = ncols * BPP;
      for (int r = tid >> 6; r < nrows; r += PR_WG / 64) {
        const uint8_t* p = p0 + (int64_t)r * a.Ws * BPP;
        const int sh = (sh0 + r * rowstep) & 3;
        unsigned char* d = srcl + (int64_t)r * L.src_pitch + sh;
        const int head = min((4 - sh) & 3, nbytes);
        const int nwords = (nbytes - head) >> 2;
        const int tail0 = head + 4 * nwords;
        if (lane < head) d[lane] = p[lane];
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(p + head);
        uint32_t* dw = reinterpret_cast<uint32_t*>(d + head);
        for (int k = lane; k < nwords; k += 64) dw[k] = pw[k];
        if (lane < nbytes - tail0) d[tail0 + lane] = p[tail0 + lane];
      }
    }
    __syncthreads();

    // ---- horizontal pass: mid[r][x * C + c] for every staged row, PR_RB rows per item
    {
      const int E = nx * C, nrg = (nrows + PR_RB - 1) / PR_RB;
      for (int it = tid; it < nrg * E; it += PR_WG) {
        const int rg = it / E, e = it - rg * E, x = e / C, c = e - x * C, r0 = rg * PR_RB;
        const int rel = bx[2 * x], len = bx[2 * x + 1];
        const tap* k = tapx + x * a.xks;
        const elem* row[PR_RB];
        acc_t acc[PR_RB];
#pragma unroll
        for (int q = 0; q < PR_RB; ++q) {
          const int r = min(r0 + q, nrows - 1);                                  // a repeated row is computed and not stored
          row[q] = reinterpret_cast<const elem*>(srcl + (int64_t)r * L.src_pitch + ((sh0 + r * rowstep) & 3)) + rel * C + c;
          acc[q] = P::init();
        }
        for (int j = 0; j < len; ++j) {
          const tap kk = k[j];
#pragma unroll
          for (int q = 0; q < PR_RB; ++q) acc[q] = P::mac(acc[q], row[q][j * C], kk);
        }
#pragma unroll
        for (int q = 0; q < PR_RB; ++q)
          if (r0 + q < nrows) mid[(r0 + q) * MIDP + e] = (elem)P::finish(acc[q]);
      }
    }
  }
  __syncthreads();

  // ---- vertical pass + epilogue
  if (RAW) {
    elem* dst = reinterpret_cast<elem*>(dst_plane) + ((int64_t)b * a.Hr * a.Wr) * C;
    const int E = nx * C;
    for (int it = tid; it < ny * E; it += PR_WG) {
      const int y = it / E, e = it - y * E;
      const int rel = by[2 * y], len = by[2 * y + 1];
      const tap* k = tapy + y * a.yks;
      acc_t acc = P::init();
      for (int j = 0; j < len; ++j) acc = P::mac(acc, mid[(rel + j) * MIDP + e], k[j]);
      dst[((int64_t)(ry0 + y) * a.Wr + rx0) * C + e] = (elem)P::finish(acc);
    }
  } else {
    float* dst = reinterpret_cast<float*>(dst_plane) + (int64_t)b * C * a.H * a.W;
    constexpr int X4 = PR_TW / 4;
    for (int it = tid; it < th * C * X4; it += PR_WG) {
      const int x4 = it % X4, c = (it / X4) % C, y = it / (X4 * C);
      if (4 * x4 >= tw) continue;
      const int64_t Y = ty0 + y + oy;
      const bool row_ok = !empty && Y >= ry0 && Y < ry1;
      const int yy = row_ok ? (int)(Y - ry0) : 0;
      const int rel = row_ok ? by[2 * yy] : 0, len = row_ok ? by[2 * yy + 1] : 0;
      const tap* k = tapy + yy * a.yks;
      bool ok[4];
      int col[4];
      acc_t acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t X = tx0 + 4 * x4 + q + ox;
        ok[q] = row_ok && X >= rx0 && X < rx1;
        col[q] = ok[q] ? ((int)(X - rx0)) * C + c : 0;
        acc[q] = P::init();
      }
      for (int j = 0; j < len; ++j) {
        const tap kk = k[j];
        const elem* m = mid + (rel + j) * MIDP;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = P::mac(acc[q], m[col[q]], kk);
      }
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int level = P::finish(acc[q]);
        o[q] = !ok[q] ? 0.f : (U16 ? (float)level * a.gt_scale : table[c * 256 + level]);
      }
      float* d = dst + ((int64_t)c * a.H + ty0 + y) * a.W + tx0 + 4 * x4;
      if (VEC) {
        *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * x4 + q < tw) d[q] = o[q];
      }
    }
  }
}

// grid: (ceil(W / PR_TW), ceil(H / PR_TH), B * planes), planes = nviews + (gt ? 1 : 0); dynamic LDS: lds_layout(...).total
template <bool RAW, bool VEC>
__global__ __launch_bounds__(PR_WG) void prep_resize_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pr_lds[];
  const int planes = a.nviews + (a.gt ? 1 : 0);
  const int b = blockIdx.z / planes, v = blockIdx.z % planes;
  if (v == a.nviews) resize_tile<true, RAW, VEC>(a, pr_lds, reinterpret_cast<const uint8_t*>(a.gt), a.dst[2], b, v);
  else resize_tile<false, RAW, VEC>(a, pr_lds, a.src[v], a.dst[v], b, v);
}

// ------------------------------------------------------------------------------------------------ host
// Pillow's bounds for resampling n -> m (precompute_coeffs), evaluated here so that the LDS window never rests on a device table:
// ksize, and the largest span of source samples that T consecutive outputs read.
struct AxisPlan {
  int ksize, window;
};
static AxisPlan axis_plan(int n, int m, int T) {
#pragma clang fp contract(off)
  AxisPlan p;
  if (n == m) {                                          // the axis is not filtered: the identity table, one tap
    p.ksize = 1;
    p.window = std::min(T, n);
    return p;
  }
  const double scale = (double)n / (double)m, fs = scale < 1.0 ? 1.0 : scale, support = 3.0 * fs;
  p.ksize = (int)std::ceil(support) * 2 + 1;
  auto xmin = [&](int i) { const double c = ((double)i + 0.5) * scale; return std::max(0, (int)(c - support + 0.5)); };
  auto xmax = [&](int i) { const double c = ((double)i + 0.5) * scale; return std::min(n, (int)(c + support + 0.5)); };
  int w = 0;
  for (int i = 0; i < m; ++i) w = std::max(w, xmax(std::min(i + T - 1, m - 1)) - xmin(i));
  p.window = std::max(w, 1);
  return p;
}

static LaunchState g_state[3];       // fused vector stores, fused scalar stores, stand-alone

// shared by the three entry points: validate the sizes against LDS, fill the window, launch
static int launch_resize(const char* what, ResizeArgs& a, int B, bool raw, bool vec, hipStream_t st) {
  RAGMI_REQUIRE(a.Hs <= (1 << 24) && a.Ws <= (1 << 24) && a.Hr <= (1 << 24) && a.Wr <= (1 << 24), RAGMI_EINVAL, "%s: image too large", what);
  const AxisPlan py = axis_plan(a.Hs, a.Hr, PR_TH), px = axis_plan(a.Ws, a.Wr, PR_TW);
  RAGMI_REQUIRE(a.yks == py.ksize && a.xks == px.ksize, RAGMI_EINVAL, "%s: tap tables of width %d (y), %d (x); %dx%d -> %dx%d needs %d, %d", what,
                a.yks, a.xks, a.Hs, a.Ws, a.Hr, a.Wr, py.ksize, px.ksize);
  a.cap_h = py.window;
  a.cap_w = px.window;
  const LdsLayout L = lds_layout(a.cap_h, a.cap_w, a.yks, a.xks);
  RAGMI_REQUIRE(L.total <= PR_LDS_MAX, RAGMI_EUNSUPPORTED,
                "%s: %dx%d -> %dx%d needs a %d x %d source window per %dx%d tile, %lld bytes of LDS (limit %lld): downscale too strong", what,
                a.Hs, a.Ws, a.Hr, a.Wr, a.cap_h, a.cap_w, PR_TH, PR_TW, (long long)L.total, (long long)PR_LDS_MAX);
  const int planes = a.nviews + (a.gt ? 1 : 0);
  const int64_t gx = ceil_div(a.W, PR_TW), gy = ceil_div(a.H, PR_TH), gz = (int64_t)B * planes;
  RAGMI_REQUIRE(gy <= 65535 && gz <= 65535, RAGMI_EINVAL, "%s: grid too large (H=%d, B=%d)", what, a.H, B);
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)gz);
  const void* fn = raw ? (const void*)prep_resize_kernel<true, false>
                       : (vec ? (const void*)prep_resize_kernel<false, true> : (const void*)prep_resize_kernel<false, false>);
  RAGMI_REQUIRE(g_state[raw ? 2 : (vec ? 0 : 1)].ensure_attr(fn, (size_t)PR_LDS_MAX), RAGMI_ELAUNCH, "%s: cannot raise the dynamic LDS limit", what);
  if (raw) hipLaunchKernelGGL((prep_resize_kernel<true, false>), grid, dim3(PR_WG), (size_t)L.total, st, a);
  else if (vec) hipLaunchKernelGGL((prep_resize_kernel<false, true>), grid, dim3(PR_WG), (size_t)L.total, st, a);
  else hipLaunchKernelGGL((prep_resize_kernel<false, false>), grid, dim3(PR_WG), (size_t)L.total, st, a);
  return check_launch(what);
}

}  // namespace ragmi

extern "C" int ragmi_prep_batch_resized(const void* left_u8, const void* right_u8, const void* gt, int gt_dtype, float gt_scale,
                                        const void* origin, void* left, void* right, void* gt_out, int B, int Hs, int Ws, int Hr, int Wr,
                                        int H, int W, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                        const void* ybounds, const void* ytaps_i32, const void* ytaps_f64, int yksize, const void* xbounds,
                                        const void* xtaps_i32, const void* xtaps_f64, int xksize, void* stream) {
  using namespace ragmi;
  const char* what = "prep_batch_resized";
  RAGMI_REQUIRE(left_u8 && left && origin, RAGMI_EINVAL, "%s: null pointer (left_u8, left, origin)", what);
  RAGMI_REQUIRE((right_u8 == nullptr) == (right == nullptr), RAGMI_EINVAL, "%s: right_u8 and right go together (one is a null pointer)", what);
  RAGMI_REQUIRE((gt == nullptr) == (gt_out == nullptr), RAGMI_EINVAL, "%s: gt and gt_out go together (one is a null pointer)", what);
  RAGMI_REQUIRE(ybounds && xbounds && ytaps_i32 && xtaps_i32 && (!gt || (ytaps_f64 && xtaps_f64)), RAGMI_EINVAL,
                "%s: null pointer (tap tables; the float64 taps are needed with a gt)", what);
  RAGMI_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hr > 0 && Wr > 0 && H > 0 && W > 0, RAGMI_EINVAL, "%s: bad size B=%d src %dx%d resized %dx%d out %dx%d",
                what, B, Hs, Ws, Hr, Wr, H, W);
  RAGMI_REQUIRE(!gt || gt_dtype == RAGMI_GT_U16, RAGMI_EUNSUPPORTED, "%s: gt dtype %d not built (RAGMI_GT_U16: the reference resizes 16-bit PNGs only)",
                what, gt_dtype);
  RAGMI_REQUIRE(aligned_to(left, 4) && aligned_to(right, 4) && aligned_to(gt_out, 4) && aligned_to(origin, 4) && aligned_to(gt, 2) &&
                    aligned_to(ybounds, 4) && aligned_to(xbounds, 4) && aligned_to(ytaps_i32, 4) && aligned_to(xtaps_i32, 4) &&
                    aligned_to(ytaps_f64, 8) && aligned_to(xtaps_f64, 8),
                RAGMI_EINVAL, "%s: misaligned pointer", what);
  ResizeArgs a;
  a.src[0] = (const uint8_t*)left_u8; a.src[1] = (const uint8_t*)right_u8; a.gt = (const uint16_t*)gt;
  a.dst[0] = left; a.dst[1] = right; a.dst[2] = gt_out;
  a.origin = (const int*)origin;
  a.yb = (const int*)ybounds; a.xb = (const int*)xbounds;
  a.yki = (const int32_t*)ytaps_i32; a.xki = (const int32_t*)xtaps_i32;
  a.ykd = (const double*)ytaps_f64; a.xkd = (const double*)xtaps_f64;
  a.gt_scale = gt_scale;
  a.mean[0] = mean0; a.mean[1] = mean1; a.mean[2] = mean2;
  a.std[0] = std0; a.std[1] = std1; a.std[2] = std2;
  a.nviews = right_u8 ? 2 : 1; a.yks = yksize; a.xks = xksize;
  a.Hs = Hs; a.Ws = Ws; a.Hr = Hr; a.Wr = Wr; a.H = H; a.W = W;
  const bool vec = W % 4 == 0 && aligned_to(left, 16) && aligned_to(right, 16) && aligned_to(gt_out, 16);
  return launch_resize(what, a, B, false, vec, static_cast<hipStream_t>(stream));
}

static int resize_standalone(const char* what, bool u16, const void* src, void* dst, int B, int Hs, int Ws, int Hr, int Wr, const void* ybounds,
                             const void* ytaps, int yksize, const void* xbounds, const void* xtaps, int xksize, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(src && dst && ybounds && ytaps && xbounds && xtaps, RAGMI_EINVAL, "%s: null pointer", what);
  RAGMI_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hr > 0 && Wr > 0, RAGMI_EINVAL, "%s: bad size B=%d src %dx%d resized %dx%d", what, B, Hs, Ws, Hr, Wr);
  const uintptr_t ta = u16 ? 8 : 4, ia = u16 ? 2 : 1;
  RAGMI_REQUIRE(aligned_to(src, ia) && aligned_to(dst, ia) && aligned_to(ybounds, 4) && aligned_to(xbounds, 4) && aligned_to(ytaps, ta) &&
                    aligned_to(xtaps, ta),
                RAGMI_EINVAL, "%s: misaligned pointer", what);
  ResizeArgs a = {};
  a.yb = (const int*)ybounds; a.xb = (const int*)xbounds;
  if (u16) {
    a.gt = (const uint16_t*)src; a.dst[2] = dst; a.nviews = 0;
    a.ykd = (const double*)ytaps; a.xkd = (const double*)xtaps;
  } else {
    a.src[0] = (const uint8_t*)src; a.dst[0] = dst; a.nviews = 1;
    a.yki = (const int32_t*)ytaps; a.xki = (const int32_t*)xtaps;
  }
  a.yks = yksize; a.xks = xksize;
  a.Hs = Hs; a.Ws = Ws; a.Hr = Hr; a.Wr = Wr; a.H = Hr; a.W = Wr;
  return launch_resize(what, a, B, true, false, static_cast<hipStream_t>(stream));
}

extern "C" int ragmi_resize_lanczos_u8(const void* src_u8, void* dst_u8, int B, int Hs, int Ws, int Hr, int Wr, const void* ybounds,
                                       const void* ytaps_i32, int yksize, const void* xbounds, const void* xtaps_i32, int xksize, void* stream) {
  return resize_standalone("resize_lanczos_u8", false, src_u8, dst_u8, B, Hs, Ws, Hr, Wr, ybounds, ytaps_i32, yksize, xbounds, xtaps_i32, xksize,
                           stream);
}

extern "C" int ragmi_resize_lanczos_u16(const void* src_u16, void* dst_u16, int B, int Hs, int Ws, int Hr, int Wr, const void* ybounds,
                                        const void* ytaps_f64, int yksize, const void* xbounds, const void* xtaps_f64, int xksize, void* stream) {
  return resize_standalone("resize_lanczos_u16", true, src_u16, dst_u16, B, Hs, Ws, Hr, Wr, ybounds, ytaps_f64, yksize, xbounds, xtaps_f64, xksize,
                           stream);
}
