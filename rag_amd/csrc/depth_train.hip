// Training kernels of the monocular-depth network (rag_depth/src/approaches/rag.py:182-246, Appr.train_epoch): the backward of
// the fused depth head (depth_head.hip) and the silog loss (utilstool/experiment.py:154-161) with its gradient.
//
// Head backward, d_out [B, S*H, S*W] -> dy [B, Cin, Hi, Wi], dw3 [Cin*9], dw1 [9], db1 [1], in two launches:
//   A  one workgroup per DH_TH x DH_TW tile of the (H, W) grid, as the forward: recompute u over tile+3, m over tile+2 and
//      z, s over tile+1 in LDS from y (nothing is saved by the forward); ds over tile+1 = max_depth * the adjoint of the x S
//      align_corners=False upsample in gather form (each s pixel collects its window of d_out, with the forward's own weights);
//      dz = ds s sigmoid(-z); dm over the tile = dz correlated with the flipped w1.  dm goes to the workspace ([B, H, W], one
//      channel); the tile's partial sums of dw3 = sum dm u, dw1 = sum dz m and db1 = sum dz go to per-workgroup slots (double).
//   B  one workgroup per DH_TH x DH_TW tile of the (Hi, Wi) grid owns its dy outright: each thread gathers the u pixels that
//      read its y pixel (the align_corners=True upsample's adjoint, again with the forward's weights) and the 3x3 dm window of
//      each, T_k = sum w dm(q + 1 - k), then dy_c = sum_k w3[c, k] T_k (du = w3^T dm is never formed).  Extra workgroups of
//      the same launch (one per weight-gradient entry) sum that entry's slots in a fixed order in double and write or add it.
// The 12-channel du never exists in memory; dm is 1/Cin of it.  Sums follow the fixed-order contract of reduce.h, without host
// synchronisation.  fp32 storage and arithmetic, double partial sums.  DESIGN.md 4.6.
//
// silog loss over the pixels with gt > 0 of the whole batch, d = log est - log gt:
//   fwd  grid-stride pass, per-thread double sums of n, sum d, sum d^2, LDS tree, slots; a one-workgroup finalize writes
//        loss = 10 sqrt(A), A = mean d^2 - lambda mean(d)^2, and saved = {n, mean d, sqrt A} (double) for the backward;
//   bwd  g_i = grad * 10 (d_i - lambda mean d) / (n sqrt(A) est_i) on masked pixels, 0 elsewhere (and everywhere when n = 0).
#include "depth_common.h"
#include "reduce.h"

namespace ragmi {

struct DepthHeadBwdArgs {
  const float* y;      // [B, Cin, Hi, Wi]
  const float* w3;     // [Cin, 3, 3]
  const float* w1;     // [3, 3]
  const float* b1;     // [1]
  const float* dout;   // [B, S*H, S*W]
  float* dy;           // [B, Cin, Hi, Wi]
  float* dw3;          // [Cin * 9]
  float* dw1;          // [9]
  float* db1;          // [1]
  double* part;        // [np][nslots]: per-tile partial sums of dw3 (Cin*9), dw1 (9), db1 (1)
  float* dm;           // [B, H, W]
  int Cin, Hi, Wi, H, W, S, np, nslots, ndy, accumulate;
  float sy, sx, inv_s, max_depth;
};

__global__ __launch_bounds__(DH_THREADS) void depth_head_bwd_tile_kernel(const DepthHeadBwdArgs a) {
  __shared__ float su[DH_CMAX][DH_UH * DH_UW];
  __shared__ float sm[DH_MH * DH_MW];
  __shared__ float sdz[DH_SH * DH_SW];
  __shared__ float sdm[DH_TH * DH_TW];
  const int tx0 = blockIdx.x * DH_TW, ty0 = blockIdx.y * DH_TH, b = blockIdx.z;
  const int H = a.H, W = a.W, Hi = a.Hi, Wi = a.Wi, Cin = a.Cin;
  const float* yb = a.y + (int64_t)b * Cin * Hi * Wi;

  // ---- u over tile + 3 and m over tile + 2, exactly as the forward computes them (zero outside the image)
  for (int i = threadIdx.x; i < DH_UH * DH_UW; i += DH_THREADS) {
    const int gy = ty0 - 3 + i / DH_UW, gx = tx0 - 3 + i % DH_UW;
    if (gy < 0 || gy >= H || gx < 0 || gx >= W) {
      for (int c = 0; c < Cin; ++c) su[c][i] = 0.f;
      continue;
    }
    int y0, y1, x0, x1;
    float ly1, lx1;
    src_ac(gy, a.sy, Hi, y0, y1, ly1);
    src_ac(gx, a.sx, Wi, x0, x1, lx1);
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const int64_t o00 = (int64_t)y0 * Wi + x0, o01 = (int64_t)y0 * Wi + x1, o10 = (int64_t)y1 * Wi + x0, o11 = (int64_t)y1 * Wi + x1;
    const int64_t hw = (int64_t)Hi * Wi;
    for (int c = 0; c < Cin; ++c) {
      const float* p = yb + c * hw;
      su[c][i] = ly0 * (lx0 * p[o00] + lx1 * p[o01]) + ly1 * (lx0 * p[o10] + lx1 * p[o11]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DH_MH * DH_MW; i += DH_THREADS) {
    const int my = i / DH_MW, mx = i % DH_MW;
    const int gy = ty0 - 2 + my, gx = tx0 - 2 + mx;
    float acc = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      for (int c = 0; c < Cin; ++c) {
        const float* wc = a.w3 + c * 9;
        const float* uc = &su[c][my * DH_UW + mx];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) acc = fmaf(wc[dy * 3 + dx], uc[dy * DH_UW + dx], acc);
      }
    }
    sm[i] = acc;
  }
  __syncthreads();

  // ---- dz over tile + 1: s recomputed, ds gathered from d_out with the forward's x S weights (zero outside the image)
  {
    const int S = a.S, OH = S * H, OW = S * W;
    const float* db = a.dout + (int64_t)b * OH * OW;
    const float bias = a.b1[0];
    for (int i = threadIdx.x; i < DH_SH * DH_SW; i += DH_THREADS) {
      const int ly = i / DH_SW, lx = i % DH_SW;
      const int gy = ty0 - 1 + ly, gx = tx0 - 1 + lx;
      float dz = 0.f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) acc = fmaf(a.w1[dy * 3 + dx], sm[(ly + dy) * DH_MW + lx + dx], acc);
        // sigmoid' = s (1 - s) with 1 - s taken as sigmoid(-z): it keeps its relative accuracy where s rounds to 1 in fp32
        const float z = acc + bias;
        const float s = 1.f / (1.f + expf(-z)), sn = 1.f / (1.f + expf(z));
        // output rows / cols whose source pair contains gy / gx lie in [S (g - 1), S (g + 2)); the weights are tested exactly
        const int oy0 = max(0, S * (gy - 1)), oy1 = min(OH, S * (gy + 2));
        const int ox0 = max(0, S * (gx - 1)), ox1 = min(OW, S * (gx + 2));
        float ds = 0.f;
        for (int oy = oy0; oy < oy1; ++oy) {
          int i0, i1;
          float l1;
          src_half(oy, a.inv_s, H, i0, i1, l1);
          if (i0 != gy && i1 != gy) continue;
          const float wy = (i0 == gy ? 1.f - l1 : 0.f) + (i1 == gy ? l1 : 0.f);
          const float* row = db + (int64_t)oy * OW;
          float racc = 0.f;
          for (int ox = ox0; ox < ox1; ++ox) {
            int j0, j1;
            float k1;
            src_half(ox, a.inv_s, W, j0, j1, k1);
            if (j0 != gx && j1 != gx) continue;
            const float wx = (j0 == gx ? 1.f - k1 : 0.f) + (j1 == gx ? k1 : 0.f);
            racc = fmaf(wx, row[ox], racc);
          }
          ds = fmaf(wy, racc, ds);
        }
        dz = a.max_depth * ds * s * sn;
      }
      sdz[i] = dz;
    }
  }
  __syncthreads();

  // ---- dm over the tile (one pixel per thread): dz correlated with the flipped w1; to the workspace
  {
    const int py = threadIdx.x / DH_TW, px = threadIdx.x % DH_TW;
    const int gy = ty0 + py, gx = tx0 + px;
    float dm = 0.f;
    if (gy < H && gx < W) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) dm = fmaf(a.w1[ky * 3 + kx], sdz[(py - ky + 2) * DH_SW + px - kx + 2], dm);
      a.dm[((int64_t)b * H + gy) * W + gx] = dm;
    }
    sdm[threadIdx.x] = dm;
  }
  __syncthreads();

  // ---- this tile's partial weight gradients, one entry per thread, summed over the tile in a fixed order in double
  const int j = threadIdx.x;
  if (j < a.np) {
    double acc = 0.0;
    if (j < 9 * Cin) {                                   // dw3[c, k] = sum_p dm(p) u_c(p + k - 1)
      const int c = j / 9, ky = (j % 9) / 3, kx = j % 3;
      for (int py = 0; py < DH_TH; ++py)
        for (int px = 0; px < DH_TW; ++px) acc += (double)sdm[py * DH_TW + px] * (double)su[c][(py + ky + 2) * DH_UW + px + kx + 2];
    } else if (j < 9 * Cin + 9) {                        // dw1[k] = sum_p dz(p) m(p + k - 1)
      const int k = j - 9 * Cin, ky = k / 3, kx = k % 3;
      for (int py = 0; py < DH_TH; ++py)
        for (int px = 0; px < DH_TW; ++px) acc += (double)sdz[(py + 1) * DH_SW + px + 1] * (double)sm[(py + ky + 1) * DH_MW + px + kx + 1];
    } else {                                             // db1 = sum_p dz(p)
      for (int py = 0; py < DH_TH; ++py)
        for (int px = 0; px < DH_TW; ++px) acc += (double)sdz[(py + 1) * DH_SW + px + 1];
    }
    const int slot = ((int)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.part[(int64_t)j * a.nslots + slot] = acc;
  }
}

// rows (or cols) g of the (H, W) grid whose align_corners=True source pair contains `yi`, with margin; the caller tests exactly
__device__ __forceinline__ void ac_window(int yi, float scale, int out, int& lo, int& hi) {
  if (!(scale > 0.f)) {
    lo = 0;
    hi = out - 1;
    return;
  }
  const float l = (float)(yi - 1) / scale - 1.f, h = (float)(yi + 1) / scale + 1.f;
  lo = l <= 0.f ? 0 : (int)l;
  hi = h >= (float)(out - 1) ? out - 1 : (int)ceilf(h);
}

__global__ __launch_bounds__(DH_THREADS) void depth_head_bwd_dy_kernel(const DepthHeadBwdArgs a) {
  if ((int)blockIdx.x >= a.ndy) {
    // ---- weight-gradient entry j: its slots in the fixed order of reduce.h, in double (the branch is uniform per workgroup)
    const int j = blockIdx.x - a.ndy;
    double acc[1];
    gather_slots<DH_THREADS>(a.part + (int64_t)j * a.nslots, a.nslots, acc);
    const auto sum = block_tree_sum<DH_THREADS>(acc);
    if (threadIdx.x == 0) {
      const int n3 = 9 * a.Cin;
      const int which = j < n3 ? 0 : (j < n3 + 9 ? 1 : 2);
      float* dst = which == 0 ? a.dw3 + j : (which == 1 ? a.dw1 + (j - n3) : a.db1);
      const float v = (float)sum[0];
      *dst = (a.accumulate >> which) & 1 ? *dst + v : v;
    }
    return;
  }
  // ---- dy of one y pixel per thread
  const int nbx = (a.Wi + DH_TW - 1) / DH_TW, nby = (a.Hi + DH_TH - 1) / DH_TH;
  const int blk = blockIdx.x, bx = blk % nbx, by = (blk / nbx) % nby, b = blk / (nbx * nby);
  const int yi = by * DH_TH + threadIdx.x / DH_TW, xi = bx * DH_TW + threadIdx.x % DH_TW;
  if (yi >= a.Hi || xi >= a.Wi) return;
  const int H = a.H, W = a.W;
  const float* dmb = a.dm + (int64_t)b * H * W;
  int gy0, gy1, gx0, gx1;
  ac_window(yi, a.sy, H, gy0, gy1);
  ac_window(xi, a.sx, W, gx0, gx1);
  float t[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = 0.f;
  for (int gy = gy0; gy <= gy1; ++gy) {
    int i0, i1;
    float l1;
    src_ac(gy, a.sy, a.Hi, i0, i1, l1);
    if (i0 != yi && i1 != yi) continue;
    const float wy = (i0 == yi ? 1.f - l1 : 0.f) + (i1 == yi ? l1 : 0.f);
    for (int gx = gx0; gx <= gx1; ++gx) {
      int j0, j1;
      float k1;
      src_ac(gx, a.sx, a.Wi, j0, j1, k1);
      if (j0 != xi && j1 != xi) continue;
      const float w = wy * ((j0 == xi ? 1.f - k1 : 0.f) + (j1 == xi ? k1 : 0.f));
      // du_c(q) = sum_k w3[c, k] dm(q + 1 - k): gather the 3x3 dm window of q once for all channels
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int r = gy + 1 - ky;
        if (r < 0 || r >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int cc = gx + 1 - kx;
          if (cc >= 0 && cc < W) t[ky * 3 + kx] = fmaf(w, dmb[(int64_t)r * W + cc], t[ky * 3 + kx]);
        }
      }
    }
  }
  const int64_t hw = (int64_t)a.Hi * a.Wi;
  float* o = a.dy + (int64_t)b * a.Cin * hw + (int64_t)yi * a.Wi + xi;
  for (int c = 0; c < a.Cin; ++c) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) v = fmaf(a.w3[c * 9 + k], t[k], v);
    o[c * hw] = v;
  }
}

static int64_t head_bwd_slots(int B, int H, int W) { return ceil_div(W, DH_TW) * ceil_div(H, DH_TH) * (int64_t)B; }

// ------------------------------------------------------------------------------------------------------------------ silog
constexpr int SL_WG = 256;       // threads per workgroup, every silog kernel
constexpr int SL_MAXWG = 1024;   // workgroups of the forward pass at most (grid-stride beyond)

__global__ __launch_bounds__(SL_WG) void silog_fwd_kernel(const float* __restrict__ est, const float* __restrict__ gt, int64_t n,
                                                          double* __restrict__ slots) {
  double v[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * SL_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_WG) {
    const float g = gt[i];
    if (!(g > 0.f)) continue;
    const float d = logf(est[i]) - logf(g);
    v[0] += 1.0;
    v[1] += d;
    v[2] += (double)(d * d);
  }
  const auto sum = block_tree_sum<SL_WG>(v);
  if (threadIdx.x < 3) slots[(int64_t)blockIdx.x * 3 + threadIdx.x] = sum[threadIdx.x];
}

__global__ __launch_bounds__(SL_WG) void silog_finalize_kernel(const double* __restrict__ slots, int nslots, double variance_focus,
                                                               float* __restrict__ out, double* __restrict__ saved) {
  double v[3];
  gather_slots<SL_WG>(slots, nslots, v);
  const auto sum = block_tree_sum<SL_WG>(v);
  if (threadIdx.x == 0) {
    const double n = sum[0];                           // n = 0: 0/0 = NaN, the reference's mean of an empty selection
    const double md = sum[1] / n, md2 = sum[2] / n;
    const double sa = sqrt(md2 - variance_focus * md * md);
    out[0] = (float)(sa * 10.0);
    saved[0] = n;
    saved[1] = md;
    saved[2] = sa;
  }
}

__global__ __launch_bounds__(SL_WG) void silog_bwd_kernel(const float* __restrict__ est, const float* __restrict__ gt, int64_t n,
                                                          float variance_focus, const double* __restrict__ saved,
                                                          const float* __restrict__ gout, float* __restrict__ grad) {
  const double cnt = saved[0];
  // no masked pixel: the loss is NaN but the gradient is 0 everywhere, so no NaN reaches a gradient bucket
  const float coef = cnt > 0.0 ? (float)(10.0 * (double)gout[0] / (cnt * saved[2])) : 0.f;
  const float mu = (float)((double)variance_focus * saved[1]);
  for (int64_t i = (int64_t)blockIdx.x * SL_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * SL_WG) {
    const float g = gt[i];
    float v = 0.f;
    if (g > 0.f && cnt > 0.0) {
      const float e = est[i];
      v = coef * (logf(e) - logf(g) - mu) / e;
    }
    grad[i] = v;
  }
}

}  // namespace ragmi

extern "C" int64_t ragmi_depth_head_bwd_workspace_elems(int B, int Cin, int H, int W) {
  using namespace ragmi;
  if (B < 1 || Cin < 1 || Cin > DH_CMAX || H < 1 || W < 1) return 0;
  return 2 * (int64_t)(9 * Cin + 10) * head_bwd_slots(B, H, W) + (int64_t)B * H * W;   // double partials, then dm
}

extern "C" int ragmi_depth_head_bwd(const void* y, const void* w3, const void* w1, const void* b1, const void* d_out, void* dy,
                                    void* dw3, void* dw1, void* db1, int accumulate, void* workspace, int B, int Cin, int Hi, int Wi,
                                    int H, int W, int scale, float max_depth, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(y && w3 && w1 && b1 && d_out && dy && dw3 && dw1 && db1 && workspace, RAGMI_EINVAL, "depth_head_bwd: null pointer");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "depth_head_bwd: dtype %d not built (float32 only)", dtype);
  RAGMI_REQUIRE(B > 0 && B <= 65535, RAGMI_EINVAL, "depth_head_bwd: bad batch %d", B);
  RAGMI_REQUIRE(ragmi_depth_head_supported(Cin, Hi, Wi, H, W, scale, dtype), RAGMI_EUNSUPPORTED,
                "depth_head_bwd: Cin=%d %dx%d -> %dx%d x%d not built (Cin 1..16, Hi <= H, Wi <= W, scale 1..8)", Cin, Hi, Wi, H, W,
                scale);
  RAGMI_REQUIRE(aligned_to(workspace, 8), RAGMI_EINVAL, "depth_head_bwd: workspace not 8-byte aligned");
  const int64_t nslots = head_bwd_slots(B, H, W);
  const int64_t ndy = ceil_div(Wi, DH_TW) * ceil_div(Hi, DH_TH) * (int64_t)B;
  const int np = 9 * Cin + 10;
  RAGMI_REQUIRE(nslots < (1 << 30) && ndy + np < (1 << 30), RAGMI_EUNSUPPORTED, "depth_head_bwd: %lld tiles not built",
                (long long)std::max(nslots, ndy));
  DepthHeadBwdArgs a;
  a.y = (const float*)y; a.w3 = (const float*)w3; a.w1 = (const float*)w1; a.b1 = (const float*)b1; a.dout = (const float*)d_out;
  a.dy = (float*)dy; a.dw3 = (float*)dw3; a.dw1 = (float*)dw1; a.db1 = (float*)db1;
  a.part = (double*)workspace;
  a.dm = (float*)workspace + 2 * (int64_t)np * nslots;
  a.Cin = Cin; a.Hi = Hi; a.Wi = Wi; a.H = H; a.W = W; a.S = scale;
  a.np = np; a.nslots = (int)nslots; a.ndy = (int)ndy; a.accumulate = accumulate & 7;
  a.sy = H > 1 ? (float)(Hi - 1) / (float)(H - 1) : 0.f;          // the forward's scales, bit for bit
  a.sx = W > 1 ? (float)(Wi - 1) / (float)(W - 1) : 0.f;
  a.inv_s = (float)(1.0 / scale);
  a.max_depth = max_depth;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(depth_head_bwd_tile_kernel, dim3((unsigned)ceil_div(W, DH_TW), (unsigned)ceil_div(H, DH_TH), (unsigned)B),
                     dim3(DH_THREADS), 0, st, a);
  hipLaunchKernelGGL(depth_head_bwd_dy_kernel, dim3((unsigned)(ndy + np)), dim3(DH_THREADS), 0, st, a);
  return check_launch("depth_head_bwd");
}

extern "C" int ragmi_silog_loss_workspace_elems(long long n) {
  if (n <= 0) return 0;
  return ragmi::grid_stride_slots(n, ragmi::SL_WG, ragmi::SL_MAXWG) * 3 * 2;      // three doubles per workgroup
}

extern "C" int ragmi_silog_loss_fwd(const void* est, const void* gt, long long n, float variance_focus, void* workspace, void* out,
                                    void* saved, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(est && gt && workspace && out && saved, RAGMI_EINVAL, "silog_loss: null pointer");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "silog_loss: dtype %d not built (float32 only)", dtype);
  RAGMI_REQUIRE(n > 0, RAGMI_EINVAL, "silog_loss: bad size %lld", n);
  RAGMI_REQUIRE(aligned_to(workspace, 8) && aligned_to(saved, 8), RAGMI_EINVAL,
                "silog_loss: workspace / saved not 8-byte aligned");
  const int nslots = grid_stride_slots(n, SL_WG, SL_MAXWG);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(silog_fwd_kernel, dim3((unsigned)nslots), dim3(SL_WG), 0, st, (const float*)est, (const float*)gt, (int64_t)n,
                     (double*)workspace);
  hipLaunchKernelGGL(silog_finalize_kernel, dim3(1), dim3(SL_WG), 0, st, (const double*)workspace, nslots, (double)variance_focus,
                     (float*)out, (double*)saved);
  return check_launch("silog_loss");
}

extern "C" int ragmi_silog_loss_bwd(const void* est, const void* gt, long long n, float variance_focus, const void* saved,
                                    const void* gout, void* grad, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(est && gt && saved && gout && grad, RAGMI_EINVAL, "silog_loss_bwd: null pointer");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "silog_loss_bwd: dtype %d not built (float32 only)", dtype);
  RAGMI_REQUIRE(n > 0, RAGMI_EINVAL, "silog_loss_bwd: bad size %lld", n);
  RAGMI_REQUIRE(aligned_to(saved, 8), RAGMI_EINVAL, "silog_loss_bwd: saved not 8-byte aligned");
  const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 4 * SL_WG), 2048));
  hipLaunchKernelGGL(silog_bwd_kernel, dim3((unsigned)nb), dim3(SL_WG), 0, static_cast<hipStream_t>(stream), (const float*)est,
                     (const float*)gt, (int64_t)n, variance_focus, (const double*)saved, (const float*)gout, (float*)grad);
  return check_launch("silog_loss_bwd");
}
