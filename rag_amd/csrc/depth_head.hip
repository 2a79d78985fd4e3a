// Depth head of the monocular-depth network (rag_depth/src/models/rag_model.py:51-64, 357-416) as ONE launch, from last_6_3d's
// output y [B, Cin, Hi, Wi] to the depth map [B, S*H, S*W]:
//   u   = bilinear(y, (H, W), align_corners=True)                      upsample_6
//   m   = conv3x3(u, w3[1, Cin, 3, 3]), zero padding 1, no bias         last_3_3d (bn=False, relu=False)
//   s   = sigmoid(conv3x3(m, w1[1, 1, 3, 3]) + b1), zero padding 1      DispHead.conv1 + sigmoid
//   out = max_depth * bilinear(s, scale S, align_corners=False)         F.interpolate(scale_factor=S) (source index clamped at 0)
// One workgroup owns a DH_TH x DH_TW tile of s.  It stages u over tile+3 (all channels) in LDS, builds m over tile+2 and s over
// tile+1 in LDS, then writes its 3*DH_TH output rows with 16-byte stores along W.  The 12-channel full-resolution u and the
// one-channel m and s never reach HBM.  fp32 storage and arithmetic.  DESIGN.md section 4.6.
#include "depth_common.h"

namespace ragmi {

struct DepthHeadArgs {
  const float* y;     // [B, Cin, Hi, Wi]
  const float* w3;    // [Cin, 3, 3]
  const float* w1;    // [3, 3]
  const float* b1;    // [1]
  float* out;         // [B, S*H, S*W]
  int Cin, Hi, Wi, H, W, S;
  float sy, sx;       // align_corners=True source scales (Hi-1)/(H-1), (Wi-1)/(W-1); 0 for a size-1 output
  float inv_s;        // 1/S as ATen computes it (float(1.0 / S))
  float max_depth;
  int vec;            // the output rows can take 16-byte stores (S*W % 4 == 0 and `out` 16-byte aligned)
};

__global__ __launch_bounds__(DH_THREADS) void depth_head_kernel(const DepthHeadArgs a) {
  __shared__ float su[DH_CMAX][DH_UH * DH_UW];
  __shared__ float sm[DH_MH * DH_MW];
  __shared__ float ss[DH_SH * DH_SW];
  const int tx0 = blockIdx.x * DH_TW, ty0 = blockIdx.y * DH_TH, b = blockIdx.z;
  const int H = a.H, W = a.W, Hi = a.Hi, Wi = a.Wi, Cin = a.Cin;
  const float* yb = a.y + (int64_t)b * Cin * Hi * Wi;

  // ---- u over rows ty0-3 .. ty0+TH+2, cols tx0-3 .. tx0+TW+2 (zero outside the image: m's padding)
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

  // ---- m over tile + 2 (zero outside the image: s's padding)
  for (int i = threadIdx.x; i < DH_MH * DH_MW; i += DH_THREADS) {
    const int my = i / DH_MW, mx = i % DH_MW;
    const int gy = ty0 - 2 + my, gx = tx0 - 2 + mx;
    float acc = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      for (int c = 0; c < Cin; ++c) {
        const float* wc = a.w3 + c * 9;
        const float* uc = &su[c][my * DH_UW + mx];     // u(my - 1 + dy, mx - 1 + dx) in m coordinates = su[my + dy][mx + dx]
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) acc = fmaf(wc[dy * 3 + dx], uc[dy * DH_UW + dx], acc);
      }
    }
    sm[i] = acc;
  }
  __syncthreads();

  // ---- s over tile + 1 (positions outside the image are computed but never read: the x S upsample clamps into [0, H-1])
  {
    const float bias = a.b1[0];
    for (int i = threadIdx.x; i < DH_SH * DH_SW; i += DH_THREADS) {
      const int sy = i / DH_SW, sx = i % DH_SW;
      float acc = 0.f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) acc = fmaf(a.w1[dy * 3 + dx], sm[(sy + dy) * DH_MW + sx + dx], acc);
      const float z = acc + bias;
      ss[i] = 1.f / (1.f + expf(-z));
    }
  }
  __syncthreads();

  // ---- output rows S*ty0 .. S*(ty0+TH)-1, cols S*tx0 .. S*(tx0+TW)-1, clipped to the image
  const int S = a.S, OH = S * H, OW = S * W;
  const int oy0 = S * ty0, oy1 = min(S * (ty0 + DH_TH), OH);
  const int ox0 = S * tx0, ox1 = min(S * (tx0 + DH_TW), OW);
  float* ob = a.out + (int64_t)b * OH * OW;
  const int nx = ox1 - ox0;
  auto value = [&](int oy, int ox, int y0, int y1, float ly1) {
    int x0, x1;
    float lx1;
    src_half(ox, a.inv_s, W, x0, x1, lx1);
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const int r0 = (y0 - ty0 + 1) * DH_SW + 1 - tx0, r1 = (y1 - ty0 + 1) * DH_SW + 1 - tx0;   // s rows in tile coordinates
    return a.max_depth * (ly0 * (lx0 * ss[r0 + x0] + lx1 * ss[r0 + x1]) + ly1 * (lx0 * ss[r1 + x0] + lx1 * ss[r1 + x1]));
  };
  if (a.vec) {
    const int nv = nx >> 2;                             // nx is a multiple of 4 when vec is set
    for (int i = threadIdx.x; i < (oy1 - oy0) * nv; i += DH_THREADS) {
      const int oy = oy0 + i / nv, ox = ox0 + 4 * (i % nv);
      int y0, y1;
      float ly1;
      src_half(oy, a.inv_s, H, y0, y1, ly1);
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = value(oy, ox + k, y0, y1, ly1);
      st4<float>(ob + (int64_t)oy * OW + ox, v);
    }
  } else {
    for (int i = threadIdx.x; i < (oy1 - oy0) * nx; i += DH_THREADS) {
      const int oy = oy0 + i / nx, ox = ox0 + i % nx;
      int y0, y1;
      float ly1;
      src_half(oy, a.inv_s, H, y0, y1, ly1);
      ob[(int64_t)oy * OW + ox] = value(oy, ox, y0, y1, ly1);
    }
  }
}

}  // namespace ragmi

extern "C" int ragmi_depth_head_supported(int Cin, int Hi, int Wi, int H, int W, int scale, int dtype) {
  using namespace ragmi;
  if (dtype != RAGMI_F32) return 0;
  if (Cin < 1 || Cin > DH_CMAX || Hi < 1 || Wi < 1 || H < 1 || W < 1 || scale < 1 || scale > 8) return 0;
  if (Hi > H || Wi > W) return 0;                                   // upsampling (or same size) only
  if ((int64_t)scale * H > (1 << 20) || (int64_t)scale * W > (1 << 20)) return 0;
  if (ceil_div(H, DH_TH) > 65535) return 0;
  return 1;
}

extern "C" int ragmi_depth_head_fwd(const void* y, const void* w3, const void* w1, const void* b1, void* out, int B, int Cin, int Hi,
                                    int Wi, int H, int W, int scale, float max_depth, int dtype, void* stream) {
  using namespace ragmi;
  RAGMI_REQUIRE(y && w3 && w1 && b1 && out, RAGMI_EINVAL, "depth_head: null pointer");
  RAGMI_REQUIRE(dtype == RAGMI_F32, RAGMI_EUNSUPPORTED, "depth_head: dtype %d not built (float32 only)", dtype);
  RAGMI_REQUIRE(B > 0 && B <= 65535, RAGMI_EINVAL, "depth_head: bad batch %d", B);
  RAGMI_REQUIRE(ragmi_depth_head_supported(Cin, Hi, Wi, H, W, scale, dtype), RAGMI_EUNSUPPORTED,
                "depth_head: Cin=%d %dx%d -> %dx%d x%d not built (Cin 1..16, Hi <= H, Wi <= W, scale 1..8)", Cin, Hi, Wi, H, W, scale);
  DepthHeadArgs a;
  a.y = (const float*)y; a.w3 = (const float*)w3; a.w1 = (const float*)w1; a.b1 = (const float*)b1; a.out = (float*)out;
  a.Cin = Cin; a.Hi = Hi; a.Wi = Wi; a.H = H; a.W = W; a.S = scale;
  a.sy = H > 1 ? (float)(Hi - 1) / (float)(H - 1) : 0.f;
  a.sx = W > 1 ? (float)(Wi - 1) / (float)(W - 1) : 0.f;
  a.inv_s = (float)(1.0 / scale);
  a.max_depth = max_depth;
  a.vec = ((int64_t)scale * W) % 4 == 0 && aligned4(out, RAGMI_F32);
  hipLaunchKernelGGL(depth_head_kernel, dim3((unsigned)ceil_div(W, DH_TW), (unsigned)ceil_div(H, DH_TH), (unsigned)B), dim3(DH_THREADS), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("depth_head");
}
