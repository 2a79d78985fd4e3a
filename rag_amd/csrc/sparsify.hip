// Sparsification curves and AUSE / AURG of a per-pixel uncertainty, per image, without a sort.
//
// A curve needs, for K cut ranks n_j = N - (j N) / K, the sum of error and the count of D1-bad pixels over the n_j pixels of smallest
// key, where the key is the order-preserving 32-bit image of `unc` (the uncertainty curve S) or the quantised error e_q itself (the
// error-ranked curve O).  Both keys go through the same kernels (blockIdx.z picks the key).  The n_j-th smallest key is found exactly
// by four radix levels of 11 / 7 / 7 / 7 bits; every bin carries {count, bad count, sum of e_q}, so the totals BELOW the cut come out
// of the same histograms and the last level's bin is the group of pixels with exactly the cut's key: the tie group of the definition.
//
//   clear -> pass 1 (histogram of the top 11 bits) -> cut 1 (scan; per cut the bin that holds its rank and the totals below it)
//         -> pass 2..4 (pixels whose prefix equals one of the <= K distinct cut prefixes; the next 7 bits, one 128-bin histogram per
//            distinct prefix) each followed by its cut kernel (the last one also records the tie group) -> finalize (-> meter)
//
// Every pass keeps its whole histogram in LDS (2048 bins, then K x 128) and flushes the occupied bins once per workgroup, so the
// pixels of a tie group (a quantised or constant unc, equal errors) meet in LDS and never at one L2 address.  All accumulation across
// threads and workgroups is by 64-bit integer atomics ({count, bad} packed in one word, the sum of e_q in another), so the result does
// not depend on the order of arrival: bitwise reproducible.  No host synchronisation, no allocation, kernels only (no memset node).
#include "common.h"

namespace ragmi {

namespace sparsify {

constexpr int MAXK = 32;                      // cut records are laid out with this stride whatever K is
constexpr int L1_BITS = 11, LR_BITS = 7;      // 11 + 3 * 7 = 32
constexpr int L1_BINS = 1 << L1_BITS, LR_BINS = 1 << LR_BITS, LEVELS = 4;
constexpr int REC_ELEMS = 3;                  // one cut record = 48 bytes = three 16-byte elements
constexpr double EQ_SCALE = 1048576.0;        // 2^20: e_q = rint(|disp - gt| 2^20), saturated at 2^32 - 1 (4096 px - 2^-20)

struct alignas(16) Bin {                      // one 16-byte workspace element
  unsigned cnt, bad;
  unsigned long long sum;
};
struct alignas(16) Rec {                      // state of one cut after a level
  unsigned long long sum;                     // sum of e_q over the keys below `prefix`
  unsigned long long gsum;                    // last level only: e_q sum of the group with the cut's key
  unsigned prefix;                            // the top bits of the cut's key found so far
  unsigned cnt, bad;                          // pixels / bad pixels with keys below `prefix`
  unsigned gcnt, gbad;                        // last level only: size and bad count of that group
  unsigned pad[3];
};
static_assert(sizeof(Bin) == 16 && sizeof(Rec) == 16 * REC_ELEMS, "workspace elements are 16 bytes");

// the workspace, in 16-byte elements; the one place that knows the layout (the header states the formula)
struct Layout {
  int64_t hist1, histr, histr_stride, rec, rec_stride, info, total;
  Layout(int B, int K) {
    const int64_t bz = 2 * (int64_t)B;
    hist1 = 0;
    histr = hist1 + bz * L1_BINS;
    histr_stride = bz * K * LR_BINS;
    rec = histr + (LEVELS - 1) * histr_stride;
    rec_stride = bz * MAXK * REC_ELEMS;
    info = rec + LEVELS * rec_stride;
    total = info + bz;
  }
};

__global__ __launch_bounds__(256) void clear_kernel(uint4* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

struct Pixel {
  bool valid, bad;
  unsigned ukey, eq;    // the order-preserving image of unc; e_q (the key of the error-ranked curve O)
  __device__ __forceinline__ unsigned key(int z) const { return z ? eq : ukey; }
  // what one pixel adds to a bin: {count, bad} as one 64-bit word (count in the low half: it stays below 2^31, so it never carries)
  __device__ __forceinline__ unsigned long long cb() const { return 1ull | ((unsigned long long)bad << 32); }
};

// the definition's per-pixel part: mask, e_q, bad flag, the two keys
__device__ __forceinline__ Pixel load_pixel(const float* __restrict__ disp, const float* __restrict__ unc, const float* __restrict__ gt,
                                            int64_t i, float maxdisp) {
  Pixel p;
  const float g = gt[i], d = disp[i];
  const unsigned ub = __float_as_uint(unc[i]), db = __float_as_uint(d);
  p.valid = g > 0.f && g < maxdisp && (ub & 0x7f800000u) != 0x7f800000u && (db & 0x7f800000u) != 0x7f800000u;
  const double e = fmin(rint(fabs((double)d - (double)g) * EQ_SCALE), 4294967295.0);
  p.eq = p.valid ? (unsigned)e : 0u;
  const float E = fabsf(g - d);
  p.bad = E > 3.f && E / fabsf(g) > 0.05f;                       // D1's flag, as metrics.hip forms it
  const unsigned b = (ub & 0x7fffffffu) == 0u ? 0u : ub;          // -0 == +0
  p.ukey = (b & 0x80000000u) ? ~b : (b | 0x80000000u);            // negatives below positives, total order
  return p;
}

// a bin's {count, bad} pair as the 64-bit word Pixel::cb() adds to
__device__ __forceinline__ unsigned long long* cb_word(Bin* b) { return reinterpret_cast<unsigned long long*>(b); }

// the occupied bins of a workgroup's LDS histogram, added to the global one
__device__ __forceinline__ void flush_bins(const unsigned long long* s_cb, const unsigned long long* s_sum, int n, Bin* __restrict__ h) {
  for (int t = threadIdx.x; t < n; t += 256) {
    if (s_cb[t] == 0ull) continue;
    atomicAdd(cb_word(&h[t]), s_cb[t]);
    atomicAdd(&h[t].sum, s_sum[t]);
  }
}

// ---- pass 1: histogram of the key's top 11 bits -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pass1_kernel(const float* __restrict__ disp, const float* __restrict__ unc,
                                                    const float* __restrict__ gt, int64_t hw, float maxdisp, Bin* __restrict__ hist) {
  __shared__ unsigned long long s_cb[L1_BINS], s_sum[L1_BINS];
  const int b = blockIdx.y, z = blockIdx.z;
  for (int t = threadIdx.x; t < L1_BINS; t += 256) { s_cb[t] = 0ull; s_sum[t] = 0ull; }
  __syncthreads();
  const int64_t base = (int64_t)b * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const Pixel p = load_pixel(disp, unc, gt, base + i, maxdisp);
    if (!p.valid) continue;
    const unsigned bin = p.key(z) >> (32 - L1_BITS);
    atomicAdd(&s_cb[bin], p.cb());
    atomicAdd(&s_sum[bin], (unsigned long long)p.eq);
  }
  __syncthreads();
  flush_bins(s_cb, s_sum, L1_BINS, hist + ((int64_t)b * 2 + z) * L1_BINS);
}

// slot of each cut among the distinct prefixes of its (image, key): cuts are ordered by falling rank, so equal prefixes are adjacent
__device__ __forceinline__ int derive_slots(const Rec* __restrict__ rec, int K, unsigned* s_prefix, int* s_slot) {
  __shared__ int s_n;
  if (threadIdx.x < K) s_prefix[threadIdx.x] = rec[threadIdx.x].prefix;
  __syncthreads();
  if (threadIdx.x == 0) {
    int d = 0;
    s_slot[0] = 0;
    for (int j = 1; j < K; ++j) {
      if (s_prefix[j] != s_prefix[j - 1]) ++d;
      s_slot[j] = d;
    }
    s_n = d + 1;
  }
  __syncthreads();
  return s_n;
}

// ---- pass 2..4: the next 7 bits of the pixels whose prefix equals a cut's, one 128-bin histogram per distinct prefix -----------------
// PSHIFT: key >> PSHIFT is the prefix found so far; the bits binned now lie directly below it.  Dynamic LDS: K * 128 * 16 bytes.
template <int PSHIFT>
__global__ __launch_bounds__(256) void refine_kernel(const float* __restrict__ disp, const float* __restrict__ unc,
                                                     const float* __restrict__ gt, int64_t hw, float maxdisp, int K,
                                                     const Rec* __restrict__ rec_prev, Bin* __restrict__ hist) {
  extern __shared__ unsigned long long s_bins[];             // [K * 128] {count, bad} words, then [K * 128] sums
  __shared__ unsigned s_prefix[MAXK], s_dist[MAXK];
  __shared__ int s_slot[MAXK];
  const int b = blockIdx.y, z = blockIdx.z, nbins = K * LR_BINS;
  unsigned long long* s_cb = s_bins;
  unsigned long long* s_sum = s_bins + nbins;
  const int nslots = derive_slots(rec_prev + ((int64_t)b * 2 + z) * MAXK, K, s_prefix, s_slot);
  if (threadIdx.x < K) s_dist[s_slot[threadIdx.x]] = s_prefix[threadIdx.x];      // equal values where two cuts share a slot
  for (int t = threadIdx.x; t < nslots * LR_BINS; t += 256) { s_cb[t] = 0ull; s_sum[t] = 0ull; }   // only the histograms in use
  __syncthreads();
  const int64_t base = (int64_t)b * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const Pixel p = load_pixel(disp, unc, gt, base + i, maxdisp);
    if (!p.valid) continue;
    const unsigned key = p.key(z), pre = key >> PSHIFT;
    int target = -1;
    for (int d = 0; d < nslots; ++d)
      if (s_dist[d] == pre) target = d * LR_BINS + (int)((key >> (PSHIFT - LR_BITS)) & (LR_BINS - 1));
    if (target < 0) continue;
    atomicAdd(&s_cb[target], p.cb());
    atomicAdd(&s_sum[target], (unsigned long long)p.eq);
  }
  __syncthreads();
  flush_bins(s_cb, s_sum, nslots * LR_BINS, hist + ((int64_t)b * 2 + z) * nbins);
}

// exclusive prefix sums of one value per thread over the THREADS threads of the workgroup, and the total
template <int THREADS, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* s_wave, T& total) {
  constexpr int WAVES = THREADS / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) before += s_wave[w];
    all += s_wave[w];
  }
  total = all;
  return before + incl - v;
}

// ---- cut kernels: scan one histogram and, for each cut that lives in it, find the bin that holds the cut's rank ----------------------
// LEVEL 1: grid (1, B, 2), 256 threads, the image's 2048 bins, every cut.  LEVEL 2..4: grid (K, B, 2), 128 threads, blockIdx.x = the
// slot (distinct prefix) whose 128 bins are scanned; a workgroup past the number of slots returns.
template <int LEVEL, int BITS, int THREADS>
__global__ __launch_bounds__(THREADS) void cut_kernel(const Bin* __restrict__ hist, int K, const Rec* __restrict__ rec_prev,
                                                      Rec* __restrict__ rec_out, uint4* __restrict__ info) {
  constexpr int BINS = 1 << BITS, PER = BINS / THREADS, WAVES = THREADS / 64;
  __shared__ unsigned s_prefix[MAXK], s_pcnt[MAXK], s_pbad[MAXK];
  __shared__ unsigned long long s_psum[MAXK];
  __shared__ int s_slot[MAXK];
  __shared__ unsigned s_wc[WAVES], s_wb[WAVES];
  __shared__ unsigned long long s_ws[WAVES];
  const int b = blockIdx.y, z = blockIdx.z, tid = threadIdx.x;
  const int64_t bz = (int64_t)b * 2 + z;
  int slot = 0;
  if (LEVEL > 1) {
    if (tid < K) {                                                // the previous level's totals below each cut, read once
      const Rec* rp = rec_prev + bz * MAXK + tid;
      s_pcnt[tid] = rp->cnt; s_pbad[tid] = rp->bad; s_psum[tid] = rp->sum;
    }
    const int nslots = derive_slots(rec_prev + bz * MAXK, K, s_prefix, s_slot);
    slot = blockIdx.x;
    if (slot >= nslots) return;
  }
  const Bin* h = hist + (LEVEL == 1 ? bz * BINS : (bz * K + slot) * BINS) + (int64_t)tid * PER;
  Bin mine[PER];
  unsigned tc = 0u, tb = 0u;
  unsigned long long ts = 0ull;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    mine[k] = h[k];
    tc += mine[k].cnt; tb += mine[k].bad; ts += mine[k].sum;
  }
  unsigned nall, nbad;
  unsigned long long sall;
  const unsigned ec0 = block_excl_scan<THREADS>(tc, s_wc, nall), eb0 = block_excl_scan<THREADS>(tb, s_wb, nbad);
  const unsigned long long es0 = block_excl_scan<THREADS>(ts, s_ws, sall);
  unsigned N;
  if (LEVEL == 1) {
    N = nall;
    if (tid == 0) info[bz] = make_uint4(N, nbad, 0u, 0u);
  } else {
    N = info[bz].x;
  }
  if (tc == 0u) return;
  for (int j = 0; j < K; ++j) {
    if (LEVEL > 1 && s_slot[j] != slot) continue;
    const unsigned pcnt = LEVEL == 1 ? 0u : s_pcnt[j];
    const unsigned nj = N - (unsigned)(((unsigned long long)j * N) / (unsigned)K);
    const unsigned rank = nj - pcnt;                               // 1-based rank inside this histogram
    if (rank <= ec0 || rank > ec0 + tc) continue;                  // exactly one thread of one workgroup owns the cut
    unsigned ec = ec0, eb = eb0;
    unsigned long long es = es0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (rank > ec && rank <= ec + mine[k].cnt) {
        Rec r;
        r.prefix = (LEVEL == 1 ? 0u : s_prefix[j] << BITS) | (unsigned)(tid * PER + k);
        r.cnt = pcnt + ec;
        r.bad = (LEVEL == 1 ? 0u : s_pbad[j]) + eb;
        r.sum = (LEVEL == 1 ? 0ull : s_psum[j]) + es;
        r.gcnt = mine[k].cnt; r.gbad = mine[k].bad; r.gsum = mine[k].sum;
        r.pad[0] = r.pad[1] = r.pad[2] = 0u;
        rec_out[bz * MAXK + j] = r;
      }
      ec += mine[k].cnt; eb += mine[k].bad; es += mine[k].sum;
    }
  }
}

// ---- finalize: the curves and the scalars of image blockIdx.x ------------------------------------------------------------------------
// curves [B,4,K] = S_epe, O_epe, S_d1, O_d1;  scalars [B,6] = AUSE_epe, AURG_epe, AUSE_d1, AURG_d1, N, Nbad
__global__ __launch_bounds__(64) void finalize_kernel(const Rec* __restrict__ rec, const uint4* __restrict__ info, int K,
                                                      float* __restrict__ curves, float* __restrict__ scalars) {
#pragma clang fp contract(off)
  __shared__ float s_curve[4][MAXK];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float nan = __uint_as_float(0x7fc00000u);
  const unsigned N = info[(int64_t)b * 2].x, Nbad = info[(int64_t)b * 2].y;
  if (tid < 2 * K) {
    const int z = tid / K, j = tid % K;
    float epe = nan, d1 = nan;
    if (N > 0u) {
      const Rec r = rec[((int64_t)b * 2 + z) * MAXK + j];
      const unsigned rj = (unsigned)(((unsigned long long)j * N) / (unsigned)K);
      const double nj = (double)(N - rj), m = (double)(N - rj - r.cnt), c = (double)r.gcnt;
      epe = (float)(((double)r.sum + (double)r.gsum * m / c) * (1.0 / EQ_SCALE) / nj);
      if (z == 0) d1 = (float)(((double)r.bad + (double)r.gbad * m / c) / nj);
      else d1 = (float)((double)(Nbad > rj ? Nbad - rj : 0u) / nj);
    }
    s_curve[z][j] = epe;
    s_curve[2 + z][j] = d1;
    curves[((int64_t)b * 4 + z) * K + j] = epe;
    curves[((int64_t)b * 4 + 2 + z) * K + j] = d1;
  }
  __syncthreads();
  if (tid < 4) {                                                  // AUSE_epe, AURG_epe, AUSE_d1, AURG_d1: double means, j ascending
    const int s = (tid >> 1) * 2;                                 // S row: 0 (epe) or 2 (d1); the O row follows it
    double a = 0.0;
    for (int j = 0; j < K; ++j)
      a += (tid & 1) ? (double)s_curve[s][0] - (double)s_curve[s][j] : (double)s_curve[s][j] - (double)s_curve[s + 1][j];
    scalars[b * 6 + tid] = N > 0u ? (float)(a / (double)K) : nan;
  } else if (tid == 4) {
    scalars[b * 6 + 4] = (float)N;
  } else if (tid == 5) {
    scalars[b * 6 + 5] = (float)Nbad;
  }
}

// meter: double [4K + 7] = sums of the curves, of the six scalars, and the number of images counted.  One thread per column adds the
// rows of the images with N > 0 in image order: no atomics, the same sum whatever the launch.
__global__ __launch_bounds__(256) void meter_kernel(const float* __restrict__ curves, const float* __restrict__ scalars, int B, int K,
                                                    double* __restrict__ meter) {
  const int t = threadIdx.x, nc = 4 * K;
  if (t > nc + 6) return;
  double a = 0.0;
  for (int b = 0; b < B; ++b) {
    if (!(scalars[b * 6 + 4] > 0.f)) continue;
    a += t < nc ? (double)curves[(int64_t)b * nc + t] : (t < nc + 6 ? (double)scalars[b * 6 + (t - nc)] : 1.0);
  }
  meter[t] += a;
}

// workgroups per image and key of the four passes: each clears and flushes a histogram, so they are kept few and fat, about 1024 in all
static unsigned pass_blocks(int64_t hw, int B) {
  const int64_t per = std::max<int64_t>(16, std::min<int64_t>(128, 1024 / (2 * (int64_t)B)));
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(hw, 2048), per));
}

template <int PSHIFT>
static void launch_refine(dim3 grid, hipStream_t st, const float* d, const float* u, const float* g, int64_t hw, float maxdisp, int K,
                          const Rec* rec_prev, Bin* hist) {
  hipLaunchKernelGGL((refine_kernel<PSHIFT>), grid, dim3(256), (size_t)K * LR_BINS * 16, st, d, u, g, hw, maxdisp, K, rec_prev, hist);
}
constexpr int P2 = 32 - L1_BITS, P3 = P2 - LR_BITS, P4 = P3 - LR_BITS;      // the prefix shifts of passes 2, 3 and 4

}  // namespace sparsify
}  // namespace ragmi

extern "C" int64_t ragmi_sparsification_workspace_elems(int B, int H, int W, int K) {
  using namespace ragmi::sparsify;
  if (B <= 0 || H <= 0 || W <= 0 || K < 1 || K > MAXK) return 0;
  return Layout(B, K).total;
}

extern "C" int ragmi_sparsification_fwd(const void* disp, const void* unc, const void* gt, int B, int H, int W, float maxdisp, int K,
                                        void* workspace, void* curves, void* scalars, void* meter, void* stream) {
  using namespace ragmi;
  using namespace ragmi::sparsify;
  RAGMI_REQUIRE(disp && unc && gt && workspace && curves && scalars, RAGMI_EINVAL, "sparsification: null pointer");
  RAGMI_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535, RAGMI_EINVAL, "sparsification: bad size");
  RAGMI_REQUIRE(K >= 1 && K <= MAXK, RAGMI_EINVAL, "sparsification: fractions = %d is outside 1..%d", K, MAXK);
  RAGMI_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), RAGMI_EINVAL, "sparsification: H * W must stay below 2^31 (32-bit pixel counts)");
  RAGMI_REQUIRE(maxdisp > 0.f, RAGMI_EINVAL, "sparsification: maxdisp must be positive");
  RAGMI_REQUIRE(aligned_to(workspace, 16), RAGMI_EINVAL, "sparsification: workspace must be 16-byte aligned");
  RAGMI_REQUIRE(!meter || aligned_to(meter, 8), RAGMI_EINVAL, "sparsification: meter must be 8-byte aligned");
  const int64_t hw = (int64_t)H * W;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Layout L(B, K);
  Bin* ws = static_cast<Bin*>(workspace);
  Bin* histr[LEVELS - 1];
  Rec* rec[LEVELS];
  for (int l = 0; l < LEVELS - 1; ++l) histr[l] = ws + L.histr + l * L.histr_stride;
  for (int l = 0; l < LEVELS; ++l) rec[l] = reinterpret_cast<Rec*>(ws + L.rec + l * L.rec_stride);
  uint4* info = reinterpret_cast<uint4*>(ws + L.info);
  const float* d = (const float*)disp;
  const float* u = (const float*)unc;
  const float* g = (const float*)gt;
  const dim3 gp(pass_blocks(hw, B), B, 2), gc(K, B, 2);
  // K = 32 asks for 64 KiB of dynamic LDS next to the kernels' static arrays: raise the limit once per device (common.h)
  static LaunchState state[LEVELS - 1];
  constexpr size_t LDS_MAX = (size_t)MAXK * LR_BINS * 16;
  RAGMI_REQUIRE(state[0].ensure_attr((const void*)refine_kernel<P2>, LDS_MAX) && state[1].ensure_attr((const void*)refine_kernel<P3>, LDS_MAX) &&
                    state[2].ensure_attr((const void*)refine_kernel<P4>, LDS_MAX),
                RAGMI_ELAUNCH, "sparsification: cannot raise the dynamic LDS limit");
  // cleared by a kernel, not a memset node
  hipLaunchKernelGGL(clear_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(L.total, 256), 2048)), dim3(256), 0, st, (uint4*)workspace,
                     L.total);
  hipLaunchKernelGGL(pass1_kernel, gp, dim3(256), 0, st, d, u, g, hw, maxdisp, ws + L.hist1);
  hipLaunchKernelGGL((cut_kernel<1, L1_BITS, 256>), dim3(1, B, 2), dim3(256), 0, st, (const Bin*)(ws + L.hist1), K, (const Rec*)nullptr,
                     rec[0], info);
  launch_refine<P2>(gp, st, d, u, g, hw, maxdisp, K, rec[0], histr[0]);
  hipLaunchKernelGGL((cut_kernel<2, LR_BITS, 128>), gc, dim3(128), 0, st, (const Bin*)histr[0], K, (const Rec*)rec[0], rec[1], info);
  launch_refine<P3>(gp, st, d, u, g, hw, maxdisp, K, rec[1], histr[1]);
  hipLaunchKernelGGL((cut_kernel<3, LR_BITS, 128>), gc, dim3(128), 0, st, (const Bin*)histr[1], K, (const Rec*)rec[1], rec[2], info);
  launch_refine<P4>(gp, st, d, u, g, hw, maxdisp, K, rec[2], histr[2]);
  hipLaunchKernelGGL((cut_kernel<4, LR_BITS, 128>), gc, dim3(128), 0, st, (const Bin*)histr[2], K, (const Rec*)rec[2], rec[3], info);
  hipLaunchKernelGGL(finalize_kernel, dim3(B), dim3(64), 0, st, (const Rec*)rec[3], (const uint4*)info, K, (float*)curves,
                     (float*)scalars);
  if (meter)
    hipLaunchKernelGGL(meter_kernel, dim3(1), dim3(256), 0, st, (const float*)curves, (const float*)scalars, B, K, (double*)meter);
  return check_launch("sparsification");
}
