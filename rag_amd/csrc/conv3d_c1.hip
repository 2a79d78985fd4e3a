// 3x3x3 convolution with ONE output channel on the vector ALUs: the Matching-Net head's `last_3_3d`
// (ConvBR_3d(12, 1, 3, 1, 1, bn=False, relu=False), src/models/rag_model.py:269, used :361-365) at the cost volume's full
// resolution — 324 multiply-adds per output voxel and nothing for the matrix cores to hold on to (one output row).
//
// Input-stationary z-marching.  A workgroup (512 threads) owns a 64 x 32 (y, x) tile and a segment of ZSEG output planes; a thread owns
// 4 consecutive x of one row in every plane of the segment (ZSEG x 4 accumulators).  For one input channel at a time the 27
// weights sit in registers while the channel's input planes z-1 .. z+ZSEG of the tile (66 x 34 halo, fetched once per workgroup:
// global -> registers -> LDS, double-buffered in LDS, THREE stages deep in registers — a stage is ~0.3 us of arithmetic, an HBM
// round trip under load several times that) pass through: a plane feeds the three output planes around it — 108 FMAs per
// thread from 18 operand values (9 LDS reads).
// The generic small-Cout kernel (conv3d_k3_kernel<.., VALU>) re-reads every input voxel 1.65x from HBM (3-D box tiles with
// halos on all sides) and reloads weights per chunk: 78 us at the headline shape against the 27 us the input read costs.
#include "conv3d_k3.h"

namespace ragmi {

constexpr int C1_TY = 64, C1_TX = 32, C1_THREADS = 512;
// LDS tile: rows y0-1 .. y0+64 of columns x0 .. x0+31 — a row is exactly 32 banks, so the 16-byte operand reads of 8 lanes per
// row x 8 rows per wave are bank-conflict free (with the halo columns inside the rows, stride 40, they were 3-way conflicted and
// the kernel LDS-bound: 63 us of arithmetic + LDS against 17 us of arithmetic alone); the halo columns x0-1 / x0+32 live in `edge`
constexpr int C1_ROWS = C1_TY + 2, C1_COLS = C1_TX;
constexpr int C1_TILE = C1_ROWS * C1_COLS, C1_EDGE = C1_ROWS * 2;
// staging elements per stage: A = 4 consecutive x of an interior row (64 rows x 8: one per thread, 16 bytes);
// B = one voxel of the halo (rows y0-1 and y0+64: 2 x 32; columns x0-1 and x0+32 of all 66 rows: 132), 4 bytes, threads 0..195
constexpr int C1_NB = 2 * C1_TX + 2 * C1_ROWS;
static_assert(C1_TY * (C1_TX / 4) == C1_THREADS && C1_NB <= C1_THREADS, "staging map");
constexpr int C1_MAX_CIN = 64;
constexpr int64_t C1_MIN_VOXELS = 1 << 18;
#ifndef C1_ZSEG_OVERRIDE
constexpr int C1_ZSEG = 4;
#else
constexpr int C1_ZSEG = C1_ZSEG_OVERRIDE;
#endif

struct C1Args {
  const void* x;
  const float* w;          // [Cin][27], the reference layout of a [1, Cin, 3, 3, 3] weight
  const float* scale;      // optional folded BatchNorm of the single output channel
  const float* shift;
  void* y;
  int64_t x_bstride, y_bstride;
  int y_ch0, relu;
  int B, Cin, D, H, W;
  int tiles_x, tiles_y, nseg, nwork;
};

template <class T, class TO, int ZSEG>
__global__ __launch_bounds__(C1_THREADS, 2) void conv3d_c1_kernel(C1Args a) {
  constexpr int NP = ZSEG + 2;                            // input planes per channel
  // pipeline stages per channel: NP rounded up to a multiple of 6, so that the LDS double buffer (s % 2) and the three register
  // stages (s % 3) are indexed at compile time; the padding stages are dead (no loads, no arithmetic, one barrier)
  constexpr int NPS = (NP + 5) / 6 * 6;
  __shared__ __attribute__((aligned(16))) float tile[2][C1_TILE];
  __shared__ float edge[2][C1_EDGE];
  __shared__ __attribute__((aligned(16))) float wl[C1_MAX_CIN * 28];
  const int tid = threadIdx.x, tx = tid & 7, ty = tid >> 3;
  // XCD-aware order: workgroup j runs on XCD j % 8; every XCD walks one contiguous chunk of the x-fastest tile list, so tiles that
  // share halo rows / columns (and the depth segments that share two planes) meet in the same L2
  const int chunk = (a.nwork + 7) / 8, j = blockIdx.x;
  int t = (j & 7) * chunk + (j >> 3);
  if ((j >> 3) >= chunk || t >= a.nwork) return;
  const int x0 = (t % a.tiles_x) * C1_TX; t /= a.tiles_x;
  const int y0 = (t % a.tiles_y) * C1_TY; t /= a.tiles_y;
  const int seg = t % a.nseg, b = t / a.nseg;
  const int zs = seg * ZSEG, ze = min(a.D, zs + ZSEG);
  const int HW = a.H * a.W;
  const int64_t DHW = (int64_t)HW * a.D;
  for (int i = tid; i < a.Cin * 28; i += C1_THREADS) wl[i] = (i % 28) < 27 ? a.w[(i / 28) * 27 + i % 28] : 0.f;
  // this thread's two staging elements, located once (the same for every plane and channel).  The loads are UNCONDITIONAL
  // (addresses clamped into the tensor, zeros substituted at the commit): with a branch around them the compiler's wait counts
  // collapse to vmcnt(0) and every stage waits out a full memory round trip (measured: 0.6 us per stage, 90 us per launch with
  // the arithmetic removed)
  int offA, dstA, offB, dstB;
  bool okA, okB;
  {
    const int r = 1 + (tid >> 3), q = tid & 7, gy = y0 - 1 + r, gx = x0 + 4 * q;
    dstA = r * C1_COLS + 4 * q;
    okA = gy < a.H && gx + 3 < a.W;                        // W % 4 == 0: all four or none
    offA = okA ? gy * a.W + gx : 0;
  }
  {
    const int e = min(tid, C1_NB - 1);
    int r, gx;
    if (e < 2 * C1_TX) { r = e < C1_TX ? 0 : C1_ROWS - 1; gx = x0 + (e & (C1_TX - 1)); dstB = r * C1_COLS + (e & (C1_TX - 1)); }
    else { r = (e - 2 * C1_TX) >> 1; const int side = (e - 2 * C1_TX) & 1; gx = side ? x0 + C1_TX : x0 - 1; dstB = C1_TILE + r * 2 + side; }
    const int gy = y0 - 1 + r;
    okB = tid < C1_NB && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
    offB = okB ? gy * a.W + gx : 0;
  }
  const bool hasB = tid < C1_NB;
  float* const pB[2] = {dstB < C1_TILE ? tile[0] + dstB : edge[0] + (dstB - C1_TILE), dstB < C1_TILE ? tile[1] + dstB : edge[1] + (dstB - C1_TILE)};
  const T* const xb = static_cast<const T*>(a.x) + (int64_t)b * a.x_bstride;
  float pfA[3][4], pfB[3];
  // stage s = (channel c, input plane zi): plane z' = zs - 1 + zi.  Planes outside the volume (first / last segment) or past the
  // segment's last output plane + 1 contribute zeros: their (clamped) loads are discarded and their arithmetic skipped.
  auto plane_live = [&](int zi) { const int z = zs - 1 + zi; return zi < NP && z >= 0 && z <= min(ze, a.D - 1); };
  auto prefetch = [&](int c, int zi, int slot) {           // zi, slot: compile time after unrolling
#ifdef C1_DIAG_NOLOAD
    return;
#endif
    const T* const pc = xb + (int64_t)min(c, a.Cin - 1) * DHW + (int64_t)min(max(zs - 1 + zi, 0), a.D - 1) * HW;
    ld4(pc + offA, pfA[slot]);
    pfB[slot] = ld(pc + offB);
  };
  auto commit = [&](int buf, int slot) {
    *reinterpret_cast<float4*>(tile[buf] + dstA) = okA ? make_float4(pfA[slot][0], pfA[slot][1], pfA[slot][2], pfA[slot][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (hasB) *pB[buf] = okB ? pfB[slot] : 0.f;
  };
  float acc[ZSEG][4];
#pragma unroll
  for (int k = 0; k < ZSEG; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[k][i] = 0.f;
  // stages 0, 1, 2 are in flight before the first multiply; stage s + 3 is requested when stage s starts
  prefetch(0, 0, 0);
  prefetch(0, 1, 1);
  prefetch(0, 2, 2);
  commit(0, 0);
  __syncthreads();
  // operand window of this thread: rows ty .. ty+2, x0 + 4tx - 1 .. + 4: one aligned 16-byte read per row; the two outer
  // columns come from the neighbouring lanes' reads (DPP row shifts: lanes of one tile row are 8 consecutive lanes), except at
  // the row's ends, which read the halo column (one 4-byte read per row, bank-conflict free)
  const float4* const my4 = reinterpret_cast<const float4*>(&tile[0][0]) + ty * (C1_COLS / 4) + tx;
  const float* const myedge = &edge[0][0] + ty * 2 + (tx == 7 ? 1 : 0);
  const bool left_edge = tx == 0, right_edge = tx == 7;
  for (int c = 0; c < a.Cin; ++c) {
    float w[28];
#pragma unroll
    for (int i = 0; i < 28; i += 4) {
      const float4 q = *reinterpret_cast<const float4*>(wl + c * 28 + i);       // same address in every lane: a broadcast read
      w[i] = q.x; w[i + 1] = q.y; w[i + 2] = q.z; w[i + 3] = q.w;
    }
    static_for<NPS>([&](auto zi_) {
      constexpr int zi = decltype(zi_)::value;             // stage s = c * NPS + zi: s % 2 == zi % 2, s % 3 == zi % 3
      // stage s + 3 -> the register slot stage s has just left (its data went to LDS at the end of stage s - 1)
      if constexpr ((zi + 3) % NPS < NP) prefetch(zi + 3 < NPS ? c : c + 1, (zi + 3) % NPS, zi % 3);
#ifdef C1_DIAG_NOFMA
      if (false) {
#else
      if (plane_live(zi)) {
#endif
        float in[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#ifdef C1_DIAG_NOLDS
          const float4 m = make_float4(pfA[0][0] + r, pfA[1][1], pfA[2][2], pfA[0][3] + zi);
          const float e = pfB[0];
#else
          const float4 m = my4[(zi & 1) * (C1_TILE / 4) + r * (C1_COLS / 4)];
          const float e = myedge[(zi & 1) * C1_EDGE + r * 2];
#endif
          const float fl = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m.w), 0x111, 0xF, 0xF, false));   // row_shr:1
          const float fr = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m.x), 0x101, 0xF, 0xF, false));   // row_shl:1
          in[r][0] = left_edge ? e : fl; in[r][1] = m.x; in[r][2] = m.y; in[r][3] = m.z; in[r][4] = m.w; in[r][5] = right_edge ? e : fr;
        }
        static_for<3>([&](auto dz_) {
          constexpr int dz = decltype(dz_)::value, k = zi - dz;         // output plane zs + k = z' + 1 - dz
          if constexpr (zi < NP && k >= 0 && k < ZSEG) {
            if (zs + k < ze) {                                           // (wave-uniform: a partial last segment)
#pragma unroll
              for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                  for (int i = 0; i < 4; ++i) acc[k][i] = fmaf(w[dz * 9 + dy * 3 + dx], in[dy][i + dx], acc[k][i]);
            }
          }
        });
      }
      // stage s + 1 -> LDS (the buffer stage s - 1 read: every thread is past it since the last barrier)
      if constexpr ((zi + 1) % NPS < NP) commit((zi + 1) & 1, (zi + 1) % 3);
#ifndef C1_DIAG_NOBARRIER
      __syncthreads();
#endif
    });
  }
  const float sc = a.scale ? a.scale[0] : 1.f, sh = a.shift ? a.shift[0] : 0.f;
  TO* const yb = static_cast<TO*>(a.y) + (int64_t)b * a.y_bstride + (int64_t)a.y_ch0 * DHW;
  const int gx = x0 + 4 * tx, gy = y0 + ty;
  if (gy < a.H && gx < a.W) {
#pragma unroll
    for (int k = 0; k < ZSEG; ++k) {
      if (zs + k >= ze) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float u = fmaf(acc[k][i], sc, sh);
        v[i] = a.relu ? fmaxf(u, 0.f) : u;
      }
      st4(yb + (int64_t)(zs + k) * HW + gy * a.W + gx, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The head's last two steps as ONE kernel: mat = last_3_3d(Upsample(scale 2, trilinear, align_corners=True)(y6))
// (rag_model.py:357-365: `upsample_6` followed by the 12 -> 1 channel 3x3x3 convolution).  The upsampled tensor (164 MB at the
// headline shape: 43 us to write, then read back 1.4x by the convolution, which that read bounds at ~56 us) never exists: a
// thread interpolates ITS OWN operand window from the level-6 tensor (20 MB, L2 / memory-side-cache resident) in registers.
//
// For an exact factor 2 with align_corners=True the source index pattern is fixed — output 2k reads inputs (k-1, k), output 2k+1
// reads (k, k+1); only the weights vary (and, in fp32, the very last output of an axis may come out as (in-2, in-1) with a weight of
// ~1 on the second: lin_index is evaluated per thread and that one deviation is honoured) — so a thread's 4 x 6 operand window
// (2 output rows x 4 columns + halo) comes from 3 rows x 4 columns x 2 planes of the level-6 block: 12 8-byte LDS reads, 12 z-,
// 16 y-, 24 x-interpolations (two instructions each) next to the 216 multiply-adds.  Zero padding of the CONVOLUTION (positions
// outside the upsampled volume) is folded into the y / x interpolation weights (both zero).
// The level-6 block of a tile (4 planes x 34 rows x 18 columns per channel, 10 KB) is staged once per channel — one barrier per
// channel instead of one per plane — while the previous channel is multiplied.  Interpolation nesting is z, y, x (ATen: x, y, z):
// the same three linear interpolations in another order.
constexpr int CU_TY = 64, CU_TX = 32, CU_THREADS = 256, CU_ZSEG = 4;
constexpr int CU_PZ = CU_ZSEG / 2 + 2, CU_PY = CU_TY / 2 + 2, CU_PX = CU_TX / 2 + 2, CU_RS = CU_PX + 2;   // block 4 x 34 x 18, row stride 20
constexpr int CU_BLK = CU_PZ * CU_PY * CU_RS;
constexpr int CU_NPF = (CU_PZ * CU_PY * CU_PX + CU_THREADS - 1) / CU_THREADS;      // 10 loads per thread and channel

struct CUArgs {
  const void* x;           // [B, Cin, Di, Hi, Wi]
  const float* w;          // [Cin][27]
  const float* scale;
  const float* shift;
  void* y;                 // [B, *, 2 Di, 2 Hi, 2 Wi]
  int64_t x_bstride, y_bstride;
  int y_ch0, relu;
  int B, Cin, Di, Hi, Wi;
  float sd, sh, sw;        // (in - 1) / (out - 1) per axis, fp32 as lin_scale gives it
  int tiles_x, tiles_y, nseg, nwork;
};

template <class T, class TO>
__global__ __launch_bounds__(CU_THREADS, 2) void upconv3d_c1_kernel(CUArgs a) {
  constexpr int ZSEG = CU_ZSEG, NP = ZSEG + 2;
  __shared__ __attribute__((aligned(16))) float blk[2][CU_BLK];
  __shared__ __attribute__((aligned(16))) float wl[C1_MAX_CIN * 28];
  const int tid = threadIdx.x, tx = tid & 7, ty = tid >> 3;
  const int D = 2 * a.Di, H = 2 * a.Hi, W = 2 * a.Wi;
  const int chunk = (a.nwork + 7) / 8, j = blockIdx.x;      // XCD-aware order (as conv3d_c1_kernel)
  int t = (j & 7) * chunk + (j >> 3);
  if ((j >> 3) >= chunk || t >= a.nwork) return;
  const int x0 = (t % a.tiles_x) * CU_TX; t /= a.tiles_x;
  const int y0 = (t % a.tiles_y) * CU_TY; t /= a.tiles_y;
  const int seg = t % a.nseg, b = t / a.nseg;
  const int zs = seg * ZSEG, ze = min(D, zs + ZSEG);
  const int HWi = a.Hi * a.Wi;
  const int64_t DHWi = (int64_t)HWi * a.Di;
  for (int i = tid; i < a.Cin * 28; i += CU_THREADS) wl[i] = (i % 28) < 27 ? a.w[(i / 28) * 27 + i % 28] : 0.f;
  // level-6 block origin: plane zs/2 - 1, row y0/2 - 1, column x0/2 - 1 (coordinates clamped into the tensor at the load)
  const int pz0 = zs / 2 - 1, py0 = y0 / 2 - 1, px0 = x0 / 2 - 1;
  int soff[CU_NPF];
#pragma unroll
  for (int p = 0; p < CU_NPF; ++p) {
    const int e = min(tid + p * CU_THREADS, CU_PZ * CU_PY * CU_PX - 1);
    const int cx = e % CU_PX, cy = (e / CU_PX) % CU_PY, cz = e / (CU_PX * CU_PY);
    soff[p] = min(max(pz0 + cz, 0), a.Di - 1) * HWi + min(max(py0 + cy, 0), a.Hi - 1) * a.Wi + min(max(px0 + cx, 0), a.Wi - 1);
  }
  const T* const xb = static_cast<const T*>(a.x) + (int64_t)b * a.x_bstride;
  float pf[CU_NPF];
  auto prefetch = [&](int c) {
    const T* const pc = xb + (int64_t)min(c, a.Cin - 1) * DHWi;
#pragma unroll
    for (int p = 0; p < CU_NPF; ++p) pf[p] = ld(pc + soff[p]);
  };
  auto commit = [&](float* buf) {
#pragma unroll
    for (int p = 0; p < CU_NPF; ++p) {
      const int e = tid + p * CU_THREADS;
      if (e < CU_PZ * CU_PY * CU_PX) buf[(e / CU_PX) * CU_RS + e % CU_PX] = pf[p];
    }
  };
  // this thread's interpolation weights (fp32 lin_index, as the standalone upsample kernel evaluates them).  Window: block rows
  // ty .. ty+2 (level-6 rows j-1, j, j+1 with j = y0/2 + ty) and block columns 2tx .. 2tx+3 (k-1 .. k+2, k = x0/2 + 2tx).
  // Expected pairs (window indices): rows 2j-1, 2j -> (0, 1); 2j+1, 2j+2 -> (1, 2); columns 2k-1, 2k -> (0, 1); 2k+1, 2k+2 -> (1, 2);
  // 2k+3, 2k+4 -> (2, 3).  A pair that starts ONE lower than expected (the last output of an axis in fp32) is taken one lower.
  float wy0[4], wy1[4], wx0[6], wx1[6];
  bool ylow[4], xlow[6];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gy = y0 + 2 * ty - 1 + r;
    const LinIdx l = lin_index(min(max(gy, 0), H - 1), a.Hi, H, a.sh, 1);
    const int expect = py0 + ty + (r >= 2 ? 1 : 0);
    ylow[r] = l.i0 < expect;
    const bool in = (unsigned)gy < (unsigned)H;
    wy0[r] = in ? l.w0 : 0.f; wy1[r] = in ? l.w1 : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int gx = x0 + 4 * tx - 1 + i;
    const LinIdx l = lin_index(min(max(gx, 0), W - 1), a.Wi, W, a.sw, 1);
    const int expect = px0 + 2 * tx + (i >= 4 ? 2 : (i >= 2 ? 1 : 0));
    xlow[i] = l.i0 < expect;
    const bool in = (unsigned)gx < (unsigned)W;
    wx0[i] = in ? l.w0 : 0.f; wx1[i] = in ? l.w1 : 0.f;
  }
  float acc[ZSEG][2][4];
#pragma unroll
  for (int k = 0; k < ZSEG; ++k)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[k][r][i] = 0.f;
  prefetch(0);
  commit(blk[0]);
  __syncthreads();
  const int wbase = ty * CU_RS + 2 * tx;                    // this thread's window in a block plane (floats; even: 8-byte reads)
  for (int c = 0; c < a.Cin; ++c) {
    const float* const cur = blk[c & 1];
    prefetch(c + 1);                                       // the next channel's block travels under this channel's arithmetic
    float w[28];
#pragma unroll
    for (int i = 0; i < 28; i += 4) {
      const float4 q = *reinterpret_cast<const float4*>(wl + c * 28 + i);
      w[i] = q.x; w[i + 1] = q.y; w[i + 2] = q.z; w[i + 3] = q.w;
    }
    static_for<NP>([&](auto zi_) {
      constexpr int zi = decltype(zi_)::value;
      const int z = zs - 1 + zi;                           // upsampled plane (wave-uniform)
      if (z >= 0 && z <= min(ze, D - 1)) {
        const LinIdx lz = lin_index(z, a.Di, D, a.sd, 1);
        const int pa = lz.i0 - pz0, pb = lz.i1 - pz0;      // block planes (uniform): 0 .. 3
        float in[4][6];
        {
          float rz[3][4];
#pragma unroll
          for (int rr = 0; rr < 3; ++rr) {
            const float* const qa = cur + pa * (CU_PY * CU_RS) + wbase + rr * CU_RS;
            const float* const qb = cur + pb * (CU_PY * CU_RS) + wbase + rr * CU_RS;
            const float2 a0 = *reinterpret_cast<const float2*>(qa), a1 = *reinterpret_cast<const float2*>(qa + 2);
            const float2 b0 = *reinterpret_cast<const float2*>(qb), b1 = *reinterpret_cast<const float2*>(qb + 2);
            rz[rr][0] = lerp2(lz.w0, a0.x, lz.w1, b0.x); rz[rr][1] = lerp2(lz.w0, a0.y, lz.w1, b0.y);
            rz[rr][2] = lerp2(lz.w0, a1.x, lz.w1, b1.x); rz[rr][3] = lerp2(lz.w0, a1.y, lz.w1, b1.y);
          }
          float yv[4][4];
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float lo = r >= 2 ? (ylow[r] ? rz[0][q] : rz[1][q]) : rz[0][q];
              const float hi = r >= 2 ? (ylow[r] ? rz[1][q] : rz[2][q]) : rz[1][q];
              yv[r][q] = lerp2(wy0[r], lo, wy1[r], hi);
            }
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < 6; ++i) {
              const int e = i >= 4 ? 2 : (i >= 2 ? 1 : 0);           // compile time
              const float lo = e > 0 ? (xlow[i] ? yv[r][e - 1] : yv[r][e]) : yv[r][e];
              const float hi = e > 0 ? (xlow[i] ? yv[r][e] : yv[r][e + 1]) : yv[r][e + 1];
              in[r][i] = lerp2(wx0[i], lo, wx1[i], hi);
            }
        }
        static_for<3>([&](auto dz_) {
          constexpr int dz = decltype(dz_)::value, k = zi - dz;
          if constexpr (k >= 0 && k < ZSEG) {
            if (zs + k < ze) {
#pragma unroll
              for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                  for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[k][r][i] = fmaf(w[dz * 9 + dy * 3 + dx], in[r + dy][i + dx], acc[k][r][i]);
            }
          }
        });
      }
    });
    commit(blk[(c + 1) & 1]);      // (the buffer channel c - 1 read: every thread left it before the last barrier)
    __syncthreads();
  }
  const float sc = a.scale ? a.scale[0] : 1.f, sh = a.shift ? a.shift[0] : 0.f;
  const int64_t HW = (int64_t)H * W;
  TO* const yb = static_cast<TO*>(a.y) + (int64_t)b * a.y_bstride + (int64_t)a.y_ch0 * HW * D;
  const int gx = x0 + 4 * tx;
#pragma unroll
  for (int k = 0; k < ZSEG; ++k) {
    if (zs + k >= ze) continue;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int gy = y0 + 2 * ty + r;
      if (gy >= H || gx >= W) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float u = fmaf(acc[k][r][i], sc, sh);
        v[i] = a.relu ? fmaxf(u, 0.f) : u;
      }
      st4(yb + (int64_t)(zs + k) * HW + (int64_t)gy * W + gx, v);
    }
  }
}

template <class T, class TO>
static int upconv_launch_typed(CUArgs a, hipStream_t st) {
  const int D = 2 * a.Di, H = 2 * a.Hi, W = 2 * a.Wi;
  a.tiles_x = (int)ceil_div(W, CU_TX); a.tiles_y = (int)ceil_div(H, CU_TY); a.nseg = (int)ceil_div(D, CU_ZSEG);
  const int64_t nwork = (int64_t)a.tiles_x * a.tiles_y * a.nseg * a.B;
  RAGMI_REQUIRE(nwork < (1ll << 28), RAGMI_EUNSUPPORTED, "upconv3d_c1: too many tiles");
  a.nwork = (int)nwork;
  hipLaunchKernelGGL((upconv3d_c1_kernel<T, TO>), dim3((unsigned)(ceil_div(nwork, 8) * 8)), dim3(CU_THREADS), 0, st, a);
  return check_launch("upconv3d_c1");
}

// ---------------------------------------------------------------------------------------------------------------
// The same head with the channel sum taken BEFORE the x2 upsample (rag_model.py:269, 357-365).  The upsample U is linear and acts
// per channel and last_3_3d has one output channel, so
//   mat(v) = sum_tap sum_c w[c, tap] U(y6_c)(v + tap) = sum_tap U(P_tap)(v + tap),   P_tap = sum_c w[c, tap] y6_c,
// and the 27 single-channel level-6 volumes P_tap come out of the launch in front (trilinear_up_k1_kernel, resample.hip): 40 FMAs
// per output voxel instead of 324, and no channel loop here.  upconv3d_c1_kernel interpolates a 4 x 6 operand window per plane and
// CHANNEL (about 40 % of its instructions) before it multiplies; here the three blends are shared between the taps instead: for one
// (dz, dy) the three dx volumes are blended along x AT LEVEL 6 and summed (a row of 4 outputs from 3 x 4 level-6 values), the three
// dy of a dz are blended along y into the 2 x 4 outputs of a level-6 plane, and the three dz are blended along z into the ZSEG
// output planes.  Nesting is therefore x, y, z (ATen's).
// Every blend is written as weights over the thread's level-6 window (4 columns, 3 rows, UT_PZ planes) built from lin_index per
// thread — a source pair that starts one lower than the x2 pattern (the last output of an axis in fp32) just moves its two weights
// one slot down; positions outside the upsampled volume (the convolution's zero padding) get zero weights.  A slot outside a source
// pair, or a position outside the volume, is not multiplied where that can be helped without a cost (0 * Inf is NaN): the spare slot
// of the x2 pattern is skipped wave-uniformly and the padding's terms are taken back in the waves that have any.
// Frame as upconv3d_c1_kernel: 64 x 32 tile, 4 output planes, XCD-aware tile order; a stage is the THREE level-6 blocks of one
// (dz, dy) (30 KB), double-buffered in LDS: the next stage's loads travel under this stage's arithmetic.
constexpr int UT_TY = 64, UT_TX = 32, UT_THREADS = 256, UT_ZSEG = 4, UT_TAPS = 27;
constexpr int UT_PZ = UT_ZSEG / 2 + 2, UT_PY = UT_TY / 2 + 2, UT_PX = UT_TX / 2 + 2, UT_RS = UT_PX + 2;   // block 4 x 34 x 18, row stride 20
constexpr int UT_PLANE = UT_PY * UT_RS, UT_BLK = UT_PZ * UT_PLANE;
constexpr int UT_NPF = (UT_PZ * UT_PY * UT_PX + UT_THREADS - 1) / UT_THREADS;      // 10 loads per thread and tap volume
// XB (ragmi_uptaps3d_xblended_fwd): the x stage already ran in the launch in front (trilinear_up_k1_kernel<28, true>, resample.hip),
// which wrote Q [B, 9, Di, Hi, 2 Wi] — for every (dz, dy) the three dx volumes blended along x and summed, the `Q[i]` of the x stage
// below at full x resolution.  A stage is then ONE block of Q[g], UT_PZ planes x UT_PY rows x the tile's 32 columns: whole 128-byte
// rows and no x halo, 16-byte loads, and a thread's four values of a row are one 16-byte LDS read.  Everything behind the x stage
// (the skips, the y and z chains, the epilogue) is the same code.
constexpr int UQ_BLK = UT_PZ * UT_PY * UT_TX, UQ_NPF = (UQ_BLK / 4 + UT_THREADS - 1) / UT_THREADS;      // 17 KB; 5 loads per thread

struct UTArgs {
  const float* x;          // P [B, 27, Di, Hi, Wi]; XB: Q [B, 9, Di, Hi, 2 Wi]
  const float* scale;
  const float* shift;
  float* y;                // [B, *, 2 Di, 2 Hi, 2 Wi]
  int64_t x_bstride, y_bstride;
  int y_ch0, relu;
  int B, Di, Hi, Wi;
  float sd, sh, sw;
  int tiles_x, tiles_y, nseg, nwork;
};

template <bool XB>
__global__ __launch_bounds__(UT_THREADS, 2) void uptaps3d_kernel(UTArgs a) {
  constexpr int ZSEG = UT_ZSEG, NP = ZSEG + 2;
  __shared__ __attribute__((aligned(16))) float blk[2][XB ? UQ_BLK : 3 * UT_BLK];
  const int tid = threadIdx.x, tx = tid & 7, ty = tid >> 3;
  const int D = 2 * a.Di, H = 2 * a.Hi, W = 2 * a.Wi;
  const int chunk = (a.nwork + 7) / 8, j = blockIdx.x;      // XCD-aware order (as conv3d_c1_kernel)
  int t = (j & 7) * chunk + (j >> 3);
  if ((j >> 3) >= chunk || t >= a.nwork) return;
  const int x0 = (t % a.tiles_x) * UT_TX; t /= a.tiles_x;
  const int y0 = (t % a.tiles_y) * UT_TY; t /= a.tiles_y;
  const int seg = t % a.nseg, b = t / a.nseg;
  const int zs = seg * ZSEG, ze = min(D, zs + ZSEG);
  const int HWi = a.Hi * a.Wi;
  const int64_t DHWi = (int64_t)HWi * a.Di;
  const int pz0 = zs / 2 - 1, py0 = y0 / 2 - 1, px0 = x0 / 2 - 1;      // block origin (coordinates clamped into the tensor at the load)
  constexpr int NPF = XB ? UQ_NPF : UT_NPF;
  int soff[NPF], doff[NPF];
#pragma unroll
  for (int p = 0; p < NPF; ++p) {
    if constexpr (XB) {      // element = 4 columns of a Q row (W % 4 == 0: a group is inside the row or past it; past it loads the last one)
      const int e = min(tid + p * UT_THREADS, UQ_BLK / 4 - 1);
      const int cx = e % (UT_TX / 4), cy = (e / (UT_TX / 4)) % UT_PY, cz = e / (UT_TX / 4 * UT_PY);
      soff[p] = (min(max(pz0 + cz, 0), a.Di - 1) * a.Hi + min(max(py0 + cy, 0), a.Hi - 1)) * W + min(x0 + 4 * cx, W - 4);
      doff[p] = 4 * e;
    } else {
      const int e = min(tid + p * UT_THREADS, UT_PZ * UT_PY * UT_PX - 1);
      const int cx = e % UT_PX, cy = (e / UT_PX) % UT_PY, cz = e / (UT_PX * UT_PY);
      soff[p] = min(max(pz0 + cz, 0), a.Di - 1) * HWi + min(max(py0 + cy, 0), a.Hi - 1) * a.Wi + min(max(px0 + cx, 0), a.Wi - 1);
      doff[p] = (e / UT_PX) * UT_RS + cx;
    }
  }
  const float* const xb = a.x + (int64_t)b * a.x_bstride;
  float pf[XB ? UQ_NPF : 3][XB ? 4 : UT_NPF];                // XB: [load][column of the group]
  auto prefetch = [&](int g) {                               // stage g: tap volumes 3g .. 3g + 2; XB: Q[g]
    if constexpr (XB) {
      const float* const pc = xb + (int64_t)g * (2 * DHWi);
#pragma unroll
      for (int p = 0; p < UQ_NPF; ++p) {
        const float4 v = *reinterpret_cast<const float4*>(pc + soff[p]);
        pf[p][0] = v.x; pf[p][1] = v.y; pf[p][2] = v.z; pf[p][3] = v.w;
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float* const pc = xb + (int64_t)min(3 * g + ch, UT_TAPS - 1) * DHWi;
#pragma unroll
        for (int p = 0; p < UT_NPF; ++p) pf[ch][p] = pc[soff[p]];
      }
    }
  };
  auto commit = [&](float* buf) {
    if constexpr (XB) {
#pragma unroll
      for (int p = 0; p < UQ_NPF; ++p)
        if (tid + p * UT_THREADS < UQ_BLK / 4) *reinterpret_cast<float4*>(buf + doff[p]) = make_float4(pf[p][0], pf[p][1], pf[p][2], pf[p][3]);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int p = 0; p < UT_NPF; ++p)
          if (tid + p * UT_THREADS < UT_PZ * UT_PY * UT_PX) buf[ch * UT_BLK + doff[p]] = pf[ch][p];
    }
  };
  // y: upsampled rows gy = y0 + 2ty - 1 + r, r = 0 .. 3 (2 output rows + halo), over block rows ty .. ty+2 (slots 0 .. 2).  The x2
  // pattern puts r = 0, 1 on slots (0, 1) and r = 2, 3 on (1, 2), or one lower: (0, 1)
  // A term is multiplied only where the slot belongs to the row's source pair (i0, i1) — whatever its weight, as in ATen — and the row
  // is inside the volume: 0 * Inf is NaN, so a slot that merely carries a zero weight must not meet a non-finite value.  iny[r]: the
  // row is inside; ys0[r]: slot 0 belongs to its pair (r >= 2: only where the pair sits one lower)
  float wy[4][3];
  bool iny[4], ys0[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gy = y0 + 2 * ty - 1 + r, base = py0 + ty;
    const LinIdx l = lin_index(min(max(gy, 0), H - 1), a.Hi, H, a.sh, 1);
    const bool in = (unsigned)gy < (unsigned)H;
    iny[r] = in;
    ys0[r] = in && (l.i0 == base || l.i1 == base);
#pragma unroll
    for (int s = 0; s < 3; ++s) wy[r][s] = in ? (l.i0 - base == s ? l.w0 : 0.f) + (l.i1 - base == s ? l.w1 : 0.f) : 0.f;
  }
  // x: upsampled columns gx = x0 + 4tx - 1 + u, u = 0 .. 5 (4 outputs + halo), over block columns 2tx .. 2tx+3 (slots 0 .. 3):
  // u = 0, 1 on slots (0, 1); u = 2, 3 on (1, 2) or one lower; u = 4, 5 on (2, 3) or one lower.  wx[u][j]: slot xs(u) + j
  // inx0 / inx5: the halo columns u = 0 and u = 5 are inside the row (u = 1 .. 4 are the thread's own outputs); low_x: slot 0 of
  // some u >= 2 belongs to the pair of some lane of the wave (the pair sits one lower) — otherwise those terms are skipped
  // (wave-uniform)
  float wx[6][3];
  bool inx0 = true, inx5 = true, low_x = false;
#pragma unroll
  for (int u = 0; u < 6; ++u) {
    const int gx = x0 + 4 * tx - 1 + u, base = px0 + 2 * tx + (u >= 4 ? 1 : 0);
    const LinIdx l = lin_index(min(max(gx, 0), W - 1), a.Wi, W, a.sw, 1);
    const bool in = (unsigned)gx < (unsigned)W;
    if (u == 0) inx0 = in;
    if (u == 5) inx5 = in;
    if (u >= 2) low_x = low_x || __any(in && (l.i0 == base || l.i1 == base));
#pragma unroll
    for (int s = 0; s < 3; ++s) wx[u][s] = in ? (l.i0 - base == s ? l.w0 : 0.f) + (l.i1 - base == s ? l.w1 : 0.f) : 0.f;
  }
  // the block's first row enters the rows r = 2, 3 (the dy = 2 taps, and output row 1 of dy = 1) only where a row pair sits one lower
  // (wave-uniform skips otherwise)
  const bool row0_r2 = __any(ys0[2]), row0_dy2 = __any(ys0[2] || ys0[3]);
  // some lane's halo row r = 0 / r = 3 is outside the volume (the first / last rows of it only: wave-uniform)
  const bool edge_r0 = __any(!iny[0]), edge_r3 = __any(!iny[3]);
  // z (wave-uniform): upsampled plane z = zs - 1 + zi over block planes 0 .. UT_PZ-1; planes outside the volume or past the
  // segment's last output plane + 1 contribute nothing
  // lz(zi, p), one bit each of a wave-uniform mask: block plane p belongs to the plane's source pair (a weight of zero still
  // multiplies, as above)
  float wz[NP][UT_PZ];
  unsigned lzm = 0;
  auto lz = [&](int zi, int p) { return ((lzm >> (zi * UT_PZ + p)) & 1u) != 0; };
#pragma unroll
  for (int zi = 0; zi < NP; ++zi) {
    const int z = zs - 1 + zi;
    const bool live = z >= 0 && z <= min(ze, D - 1);
    const LinIdx l = lin_index(min(max(z, 0), D - 1), a.Di, D, a.sd, 1);
#pragma unroll
    for (int p = 0; p < UT_PZ; ++p) {
      if (live && (l.i0 - pz0 == p || l.i1 - pz0 == p)) lzm |= 1u << (zi * UT_PZ + p);
      wz[zi][p] = live ? (l.i0 - pz0 == p ? l.w0 : 0.f) + (l.i1 - pz0 == p ? l.w1 : 0.f) : 0.f;
    }
  }
  float acc[ZSEG][2][4];
#pragma unroll
  for (int k = 0; k < ZSEG; ++k)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[k][r][i] = 0.f;
  prefetch(0);
  commit(blk[0]);
  __syncthreads();
  const int wbase = ty * UT_RS + 2 * tx;                    // this thread's window in a block plane (floats; even: 8-byte reads)
  static_for<3>([&](auto dz_) {
    constexpr int dz = decltype(dz_)::value;
    // output plane zs + k reads upsampled plane index zi = k + dz through this dz
    bool need[UT_PZ];
#pragma unroll
    for (int p = 0; p < UT_PZ; ++p) {
      need[p] = false;
#pragma unroll
      for (int k = 0; k < ZSEG; ++k) need[p] = need[p] || (zs + k < ze && lz(k + dz, p));
    }
    float R[UT_PZ][2][4];                                   // sum over dy, dx of the taps of this dz, blended along x and y
#pragma unroll
    for (int p = 0; p < UT_PZ; ++p)
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) R[p][r][i] = 0.f;
    static_for<3>([&](auto dy_) {
      constexpr int dy = decltype(dy_)::value, g = dz * 3 + dy;
      const float* const cur = blk[g & 1];
      if constexpr (g + 1 < 9) prefetch(g + 1);
      // rows outside the volume (r = 0 above it: the dy = 0 terms of output row 0, which starts at zero; r = 3 below it: the dy = 2
      // terms of output row 1) are the convolution's zero padding: their terms are taken back where a wave has such a row
      float keep[UT_PZ][4];
      if (dy == 2 && edge_r3) {
#pragma unroll
        for (int p = 0; p < UT_PZ; ++p)
#pragma unroll
          for (int i = 0; i < 4; ++i) keep[p][i] = R[p][1][i];
      }
      static_for<UT_PZ>([&](auto p_) {
        constexpr int p = decltype(p_)::value;
        if (need[p]) {
          static_for<3>([&](auto s_) {
            constexpr int s = decltype(s_)::value;          // block row ty + s; output rows r = ro + dy
            if constexpr (!(dy == 0 && s == 2)) {
              if (dy < 2 || s > 0 || row0_dy2) {
                float Q[4];
                if constexpr (XB) {
                  const float4 v = *reinterpret_cast<const float4*>(cur + (p * UT_PY + ty + s) * UT_TX + 4 * tx);
                  Q[0] = v.x; Q[1] = v.y; Q[2] = v.z; Q[3] = v.w;
                } else {
                  auto xstage = [&](auto low_) {
                    constexpr bool LOW = decltype(low_)::value;      // slot 0 of the columns u >= 2 takes part
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                      const float* const q = cur + dx * UT_BLK + p * UT_PLANE + s * UT_RS + wbase;
                      const float2 v0 = *reinterpret_cast<const float2*>(q), v1 = *reinterpret_cast<const float2*>(q + 2);
                      const float v[4] = {v0.x, v0.y, v1.x, v1.y};
#pragma unroll
                      for (int i = 0; i < 4; ++i) {
                        const int u = i + dx, xs = u >= 4 ? 1 : 0;       // compile time
                        float qv;
                        if (u < 2 || LOW) {
                          qv = dx == 0 ? wx[u][0] * v[xs] : fmaf(wx[u][0], v[xs], Q[i]);
                          qv = fmaf(wx[u][1], v[xs + 1], qv);
                        } else {
                          qv = dx == 0 ? wx[u][1] * v[xs + 1] : fmaf(wx[u][1], v[xs + 1], Q[i]);
                        }
                        if (u >= 2) qv = fmaf(wx[u][2], v[xs + 2], qv);
                        // a halo column outside the row is the convolution's zero padding: its term is not taken
                        if (u == 0) qv = inx0 ? qv : 0.f;
                        if (u == 5) qv = inx5 ? qv : Q[i];
                        Q[i] = qv;
                      }
                    }
                  };
                  if (low_x) xstage(std::true_type{}); else xstage(std::false_type{});
                }
#pragma unroll
                for (int ro = 0; ro < 2; ++ro) {
                  const int r = ro + dy;
                  if (r < 2 && s == 2) continue;
                  if (r == 2 && s == 0 && !row0_r2) continue;
#pragma unroll
                  for (int i = 0; i < 4; ++i) R[p][ro][i] = fmaf(wy[r][s], Q[i], R[p][ro][i]);
                }
              }
            }
          });
        }
      });
      if (dy == 0 && edge_r0) {
#pragma unroll
        for (int p = 0; p < UT_PZ; ++p)
#pragma unroll
          for (int i = 0; i < 4; ++i) R[p][0][i] = iny[0] ? R[p][0][i] : 0.f;
      }
      if (dy == 2 && edge_r3) {
#pragma unroll
        for (int p = 0; p < UT_PZ; ++p)
#pragma unroll
          for (int i = 0; i < 4; ++i) R[p][1][i] = iny[3] ? R[p][1][i] : keep[p][i];
      }
      if constexpr (g + 1 < 9) commit(blk[(g + 1) & 1]);     // (the buffer stage g - 1 read: every thread left it before the last barrier)
      __syncthreads();
    });
#pragma unroll
    for (int p = 0; p < UT_PZ; ++p)
#pragma unroll
      for (int k = 0; k < ZSEG; ++k) {
        const float wk = wz[k + dz][p];
        if (zs + k < ze && lz(k + dz, p)) {
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[k][r][i] = fmaf(wk, R[p][r][i], acc[k][r][i]);
        }
      }
  });
  const float sc = a.scale ? a.scale[0] : 1.f, sh = a.shift ? a.shift[0] : 0.f;
  const int64_t HW = (int64_t)H * W;
  float* const yb = a.y + (int64_t)b * a.y_bstride + (int64_t)a.y_ch0 * HW * D;
  const int gx = x0 + 4 * tx;
#pragma unroll
  for (int k = 0; k < ZSEG; ++k) {
    if (zs + k >= ze) continue;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int gy = y0 + 2 * ty + r;
      if (gy >= H || gx >= W) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float u = fmaf(acc[k][r][i], sc, sh);
        v[i] = a.relu ? fmaxf(u, 0.f) : u;
      }
      st4(yb + (int64_t)(zs + k) * HW + (int64_t)gy * W + gx, v);
    }
  }
}

}  // namespace ragmi

extern "C" int ragmi_uptaps3d_supported(int Di, int Hi, int Wi) {
  using namespace ragmi;
  // as ragmi_upconv3d_c1_supported: whole 16-byte output rows, no axis of length 1, 32-bit offsets inside a sample
  return (Di >= 2 && Hi >= 2 && Wi >= 2 && (2 * Wi) % 4 == 0 && (int64_t)UT_TAPS * Di * Hi * Wi < (1ll << 31)) ? 1 : 0;
}

// xblended: p is Q [B, 9, Di, Hi, 2 Wi] (ragmi_uptaps3d_xblended_fwd), not P [B, 27, Di, Hi, Wi]
static int uptaps_launch(const void* p, int64_t p_bstride, const void* scale, const void* shift, int relu, void* y, int64_t y_bstride,
                         int y_ch0, int B, int Di, int Hi, int Wi, int dtype, void* stream, bool xblended) {
  using namespace ragmi;
  RAGMI_REQUIRE(p && y, RAGMI_EINVAL, "uptaps3d: null pointer");
  RAGMI_REQUIRE((scale == nullptr) == (shift == nullptr), RAGMI_EINVAL, "uptaps3d: scale/shift must both be given or both NULL");
  RAGMI_REQUIRE(B > 0 && B <= 65535 && y_ch0 >= 0, RAGMI_EINVAL, "uptaps3d: bad size");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "uptaps3d: dtype %d not built (fp32 only)", dtype);
  RAGMI_REQUIRE(ragmi_uptaps3d_supported(Di, Hi, Wi), RAGMI_EUNSUPPORTED, "uptaps3d: needs every input axis >= 2 and an even input width");
  RAGMI_REQUIRE(y_bstride % 4 == 0 && aligned4(y, RAGMI_F32), RAGMI_EUNSUPPORTED, "uptaps3d: output rows must be 16-byte aligned");
  RAGMI_REQUIRE(!xblended || (p_bstride % 4 == 0 && aligned4(p, RAGMI_F32)), RAGMI_EUNSUPPORTED,
                "uptaps3d: x-blended input rows must be 16-byte aligned");
  UTArgs a{};
  a.x = static_cast<const float*>(p); a.scale = static_cast<const float*>(scale); a.shift = static_cast<const float*>(shift);
  a.y = static_cast<float*>(y);
  a.x_bstride = p_bstride; a.y_bstride = y_bstride; a.y_ch0 = y_ch0; a.relu = relu ? 1 : 0;
  a.B = B; a.Di = Di; a.Hi = Hi; a.Wi = Wi;
  a.sd = lin_scale(Di, 2 * Di, 1); a.sh = lin_scale(Hi, 2 * Hi, 1); a.sw = lin_scale(Wi, 2 * Wi, 1);
  a.tiles_x = (int)ceil_div(2 * Wi, UT_TX); a.tiles_y = (int)ceil_div(2 * Hi, UT_TY); a.nseg = (int)ceil_div(2 * Di, UT_ZSEG);
  const int64_t nwork = (int64_t)a.tiles_x * a.tiles_y * a.nseg * B;
  RAGMI_REQUIRE(nwork < (1ll << 28), RAGMI_EUNSUPPORTED, "uptaps3d: too many tiles");
  a.nwork = (int)nwork;
  const dim3 grid((unsigned)(ceil_div(nwork, 8) * 8));
  if (xblended) hipLaunchKernelGGL(uptaps3d_kernel<true>, grid, dim3(UT_THREADS), 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(uptaps3d_kernel<false>, grid, dim3(UT_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return check_launch(xblended ? "uptaps3d_xblended" : "uptaps3d");
}

extern "C" int ragmi_uptaps3d_fwd(const void* p, int64_t p_bstride, const void* scale, const void* shift, int relu, void* y,
                                  int64_t y_bstride, int y_ch0, int B, int Di, int Hi, int Wi, int dtype, void* stream) {
  return uptaps_launch(p, p_bstride, scale, shift, relu, y, y_bstride, y_ch0, B, Di, Hi, Wi, dtype, stream, false);
}

// The same sum from the x-blended rows Q [B, 9, Di, Hi, 2 Wi] of ragmi_trilinear3d_act_k1_xblend_fwd: the y and z blends only.
extern "C" int ragmi_uptaps3d_xblended_supported(int Di, int Hi, int Wi) {
  return ragmi_uptaps3d_supported(Di, Hi, Wi);      // (2 Wi % 4 == 0: Q's rows are whole 16-byte groups)
}

extern "C" int ragmi_uptaps3d_xblended_fwd(const void* q, int64_t q_bstride, const void* scale, const void* shift, int relu, void* y,
                                           int64_t y_bstride, int y_ch0, int B, int Di, int Hi, int Wi, int dtype, void* stream) {
  return uptaps_launch(q, q_bstride, scale, shift, relu, y, y_bstride, y_ch0, B, Di, Hi, Wi, dtype, stream, true);
}

extern "C" int ragmi_upconv3d_c1_supported(int Cin, int Di, int Hi, int Wi) {
  using namespace ragmi;
  // whole 16-byte output rows; an axis of length 1 has no (in - 1) / (out - 1) scale; 32-bit offsets inside a sample
  return (Cin >= 1 && Cin <= C1_MAX_CIN && Di >= 2 && Hi >= 2 && Wi >= 2 && (2 * Wi) % 4 == 0 && (int64_t)Cin * Di * Hi * Wi < (1ll << 31)) ? 1 : 0;
}

extern "C" int ragmi_upconv3d_c1_fwd(const void* x, int64_t x_bstride, const void* weight, const void* scale, const void* shift, int relu,
                                     void* y, int64_t y_bstride, int y_ch0, int B, int Cin, int Di, int Hi, int Wi, int dtype, int y_dtype,
                                     void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(x && weight && y, RAGMI_EINVAL, "upconv3d_c1: null pointer");
  RAGMI_REQUIRE((scale == nullptr) == (shift == nullptr), RAGMI_EINVAL, "upconv3d_c1: scale/shift must both be given or both NULL");
  RAGMI_REQUIRE(B > 0 && B <= 65535 && y_ch0 >= 0, RAGMI_EINVAL, "upconv3d_c1: bad size");
  RAGMI_REQUIRE(dtype_ok(dtype) && (y_dtype == dtype || (dtype == RAGMI_BF16 && y_dtype == RAGMI_F32)), RAGMI_EUNSUPPORTED,
                "upconv3d_c1: dtype %d -> %d not built", dtype, y_dtype);
  RAGMI_REQUIRE(ragmi_upconv3d_c1_supported(Cin, Di, Hi, Wi), RAGMI_EUNSUPPORTED,
                "upconv3d_c1: needs 1..%d input channels, every input axis >= 2 and an even input width", C1_MAX_CIN);
  RAGMI_REQUIRE(y_bstride % 4 == 0 && aligned4(y, y_dtype), RAGMI_EUNSUPPORTED, "upconv3d_c1: output rows must be 16-byte aligned");
  CUArgs a{};
  a.x = x; a.w = (const float*)weight; a.scale = (const float*)scale; a.shift = (const float*)shift; a.y = y;
  a.x_bstride = x_bstride; a.y_bstride = y_bstride; a.y_ch0 = y_ch0; a.relu = relu ? 1 : 0;
  a.B = B; a.Cin = Cin; a.Di = Di; a.Hi = Hi; a.Wi = Wi;
  a.sd = lin_scale(Di, 2 * Di, 1); a.sh = lin_scale(Hi, 2 * Hi, 1); a.sw = lin_scale(Wi, 2 * Wi, 1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == RAGMI_BF16) return y_dtype == RAGMI_F32 ? upconv_launch_typed<bf16_t, float>(a, st) : upconv_launch_typed<bf16_t, bf16_t>(a, st);
  return upconv_launch_typed<float, float>(a, st);
}

namespace ragmi {

// Cout == 1, no residual input, rows of whole 16-byte elements (W % 4 == 0 and aligned bases), volumes big enough to fill the chip
// (x_aligned / y_aligned: the x and y pointers sit on four elements — the launch measures them, ragmi_conv3d_k3_small_route is told)
bool c1_eligible(const K3Args& a, bool x_aligned, bool y_aligned) {
#ifdef C1_DISABLE      // A/B build (tools/build_variant.sh): the generic small-Cout kernel everywhere
  return false;
#endif
  if (a.Cout != 1 || a.res != nullptr || a.Cin > C1_MAX_CIN || a.W % 4 != 0) return false;
  // per SAMPLE (which kernel a pair runs on must not depend on how a batch is split over ranks)
  if ((int64_t)a.D * a.H * a.W < C1_MIN_VOXELS || (int64_t)a.Cin * a.D * a.H * a.W >= (1ll << 31)) return false;
  // (a destination-channel offset moves the base by D*H*W elements, a multiple of 4 with W)
  return a.x_bstride % 4 == 0 && a.y_bstride % 4 == 0 && x_aligned && y_aligned;
}

template <class T, class TO>
static int c1_launch_typed(const C1Args& a, hipStream_t st) {
  constexpr int ZSEG = C1_ZSEG;
  C1Args b = a;
  b.tiles_x = (int)ceil_div(a.W, C1_TX); b.tiles_y = (int)ceil_div(a.H, C1_TY); b.nseg = (int)ceil_div(a.D, ZSEG);
  const int64_t nwork = (int64_t)b.tiles_x * b.tiles_y * b.nseg * a.B;
  RAGMI_REQUIRE(nwork < (1ll << 28), RAGMI_EUNSUPPORTED, "conv3d_c1: too many tiles");
  b.nwork = (int)nwork;
  const unsigned grid = (unsigned)(ceil_div(nwork, 8) * 8);
  hipLaunchKernelGGL((conv3d_c1_kernel<T, TO, ZSEG>), dim3(grid), dim3(C1_THREADS), 0, st, b);
  return check_launch("conv3d_c1");
}

// k: as filled for the generic small-Cout kernel (wp[0] = the raw [1][Cin][27] weight, y_ch[0] = destination channel)
int c1_launch(const K3Args& k, int dtype, int y_dtype, hipStream_t st) {
  C1Args a{};
  a.x = k.x; a.w = k.wp[0]; a.scale = k.scale[0]; a.shift = k.shift[0]; a.y = k.y;
  a.x_bstride = k.x_bstride; a.y_bstride = k.y_bstride; a.y_ch0 = k.y_ch[0]; a.relu = k.relu & 1;
  a.B = k.B; a.Cin = k.Cin; a.D = k.D; a.H = k.H; a.W = k.W;
  if (dtype == RAGMI_BF16) return y_dtype == RAGMI_F32 ? c1_launch_typed<bf16_t, float>(a, st) : c1_launch_typed<bf16_t, bf16_t>(a, st);
  return c1_launch_typed<float, float>(a, st);
}

}  // namespace ragmi
