// Weight-streaming skinny GEMM for the decode hot loop (gfx950).
//   out[M, N] = x[M, K] @ W[N, K]^T,  M <= 16 (decode batch)
//
// At M = 16 the GEMM is bound by streaming W once (guide §5 "GEMV / M<=16
// decode weights"); hipBLASLt's tilings reach ~55% of that roofline on
// these shapes (measured: ~120us vs 67us weight-read per 7B layer).
// Design: grid = (N/64 tiles) x SPLITK K-slices — enough workgroups to
// fill 256 CUs at every decode shape; x tile staged once in LDS; W
// streamed straight into MFMA B-fragments (16 B/lane loads, one pass,
// nothing cached); fp32 split-K partials combined with global atomics;
// a trailing kernel converts to bf16.
// MFMA lane maps: mfma.h.
#include "mfma.h"
#include "slab_sum.h"

#define SG_TN 64  // n per workgroup (16 per wave)

// x_s[16][kslice] <- x[0..M)[k_lo..k_hi), zero-padded (m >= M, k >= k_hi);
// NT = threads per workgroup
template <int NT>
DEVINL void sg_stage_x(__bf16* x_s, const bf16* __restrict__ x, int M, int K,
                       int k_lo, int k_hi, int kslice) {
  const int kn = k_hi - k_lo;
  for (int idx = threadIdx.x * 8; idx < 16 * kslice; idx += NT * 8) {
    int m = idx / kslice;
    int kk = idx % kslice;
    bf16x8 v = {};
    if (kk < kn && m < M)
      v = *(const bf16x8*)(x + (long)m * K + k_lo + kk);
    *(bf16x8*)(&x_s[(long)m * kslice + kk]) = v;
  }
}

// out[off..off+4) = bf16(sum over the nks fp32 slabs at parts + s*slab + off
// (+ resid[off..off+4))), one 8-byte store
DEVINL void sg_reduce_store(const float* __restrict__ parts, long slab,
                            int nks, long off, const bf16* __restrict__ resid,
                            bf16* __restrict__ out) {
  // the residual goes out before the slabs and is used after them
  short4v rv = {};
  if (resid) rv = *(const short4v*)((const short*)resid + off);
  const float* const p[1] = {parts + off};
  f32x4 acc[1];
  slab_sum<1>(acc, p, slab, nks);
  const f32x4 v = acc[0];
  short o[4];
  if (resid) {
    #pragma unroll
    for (int j = 0; j < 4; j++)
      o[j] = f2bf(v[j] + __bfloat162float(((const bf16*)&rv)[j]));
  } else {
    #pragma unroll
    for (int j = 0; j < 4; j++) o[j] = f2bf(v[j]);
  }
  *(short4v*)((short*)out + off) = *(short4v*)o;
}

// ---------------------------------------------------------------------------
// One K-slice of one n-tile, shared by the bf16 and the FP8-weight kernel.
// A workgroup lives for a handful of memory round trips, so the loads are
// issued as early and as many together as the registers allow:
//   1. all of the thread's x loads (SG_XV 16-byte vectors: kslice <= 1024 at
//      256 threads; a loop takes the rest of a larger slice);
//   2. the first NB W loads;
//   3. x -> LDS and the barrier.  Loads retire in order, so the wait for x
//      leaves W in flight, and a barrier does not drain plain loads;
//   4. the k loop issues W batch i+1 before the MFMAs of batch i (two
//      register buffers, ping-pong: a copy would wait for the new batch);
//   5. the tail (< NB loads) is issued together, before the last batch's
//      MFMAs.
// Only the issue order changed: per accumulator the MFMA sequence is k
// ascending, batch element t on acc[t & 3] and the tail on acc[0] (FP8: two
// MFMAs per load, on acc[2t & 3], acc[(2t+1) & 3]; tail on acc[0], acc[1]).
typedef __attribute__((ext_vector_type(4))) int int4v;  // one 16-byte W load
typedef __attribute__((ext_vector_type(2))) float float2v;

DEVINL bf16x8 sg_e4m3x8_to_bf16(int lo, int hi);

#define SG_XV 8  // x vectors a thread stages through registers

// v[t] <- the thread's t-th 16-byte piece of the zero-padded x tile; piece t
// is x_s[idx, idx + 8) with idx = (threadIdx.x + t*NT) * 8, as in sg_stage_x.
// Pieces outside x load x[0..8) (a valid address) and are zeroed after.
template <int NT>
DEVINL void sg_x_load(bf16x8 (&v)[SG_XV], const bf16* __restrict__ x, int M,
                      int K, int k_lo, int k_hi, int kslice) {
  const int kn = k_hi - k_lo;
  // (m, kk) = divmod(idx, kslice), stepped instead of divided per piece
  const int dm = (NT * 8) / kslice, dk = (NT * 8) % kslice;
  int m = (threadIdx.x * 8) / kslice;
  int kk = (threadIdx.x * 8) % kslice;
  #pragma unroll
  for (int t = 0; t < SG_XV; t++) {
    const bool ok = kk < kn && m < M;  // m < M <= 16 implies idx < 16*kslice
    const bf16* p = ok ? x + (long)m * K + k_lo + kk : x;
    const bf16x8 r = *(const bf16x8*)p;
    v[t] = ok ? r : bf16x8{};
    m += dm;
    kk += dk;
    if (kk >= kslice) { kk -= kslice; m++; }
  }
}

template <int NT>
DEVINL void sg_x_store(__bf16* x_s, const bf16x8 (&v)[SG_XV],
                       const bf16* __restrict__ x, int M, int K, int k_lo,
                       int k_hi, int kslice) {
  #pragma unroll
  for (int t = 0; t < SG_XV; t++) {
    const int idx = (threadIdx.x + t * NT) * 8;
    if (idx < 16 * kslice) *(bf16x8*)(&x_s[idx]) = v[t];
  }
  // kslice > NT * SG_XV / 2: the remaining pieces, one at a time
  const int kn = k_hi - k_lo;
  for (int idx = (threadIdx.x + SG_XV * NT) * 8; idx < 16 * kslice;
       idx += NT * 8) {
    int m = idx / kslice;
    int kk = idx % kslice;
    bf16x8 r = {};
    if (kk < kn && m < M)
      r = *(const bf16x8*)(x + (long)m * K + k_lo + kk);
    *(bf16x8*)(&x_s[idx]) = r;
  }
}

// this lane's view of W and x_s.  KB = k elements per 16-byte W load.
template <bool FP8>
struct SgLane {
  static constexpr int KB = FP8 ? 64 : 32;
  const char* wl;     // the lane's W bytes for k = 0
  const __bf16* x_s;
  int xo;             // x_s index of the lane's first element of k is xo + k

  DEVINL int4v ldw(int k) const {
    return *(const int4v*)(wl + (long)k * (FP8 ? 1 : 2));
  }
  // the MFMA(s) of one W load at k; j = its place in the batch (tail: 0)
  DEVINL void mma(f32x4 (&acc)[4], const int4v& b, int k, int j) const {
    if constexpr (FP8) {
      const bf16x8 a0 = *(const bf16x8*)(&x_s[xo + k]);
      const bf16x8 a1 = *(const bf16x8*)(&x_s[xo + k + 8]);
      acc[(2 * j) & 3] = mfma16(a0, sg_e4m3x8_to_bf16(b[0], b[1]),
                                acc[(2 * j) & 3]);
      acc[(2 * j + 1) & 3] = mfma16(a1, sg_e4m3x8_to_bf16(b[2], b[3]),
                                    acc[(2 * j + 1) & 3]);
    } else {
      const bf16x8 a0 = *(const bf16x8*)(&x_s[xo + k]);
      acc[j & 3] = mfma16(a0, __builtin_bit_cast(bf16x8, b), acc[j & 3]);
    }
  }
  // issues the NB loads HERE: the scheduler otherwise sinks them below the
  // MFMAs (and their wait) that follow
  template <int NB>
  DEVINL void ldw_batch(int4v (&b)[NB], int k) const {
    #pragma unroll
    for (int t = 0; t < NB; t++) b[t] = ldw(k + t * KB);
    __builtin_amdgcn_sched_barrier(0);
  }
  template <int NB>
  DEVINL void mma_batch(f32x4 (&acc)[4], const int4v (&b)[NB], int k) const {
    #pragma unroll
    for (int t = 0; t < NB; t++) mma(acc, b[t], k + t * KB, t);
  }
};

// the end of a slice: the NTL tail loads go out together, then the MFMAs of
// the last full batch (in flight in `last`, at k; none if !has_last), then
// the tail's
template <bool FP8, int NB, int NTL>
DEVINL void sg_finish(const SgLane<FP8>& ln, f32x4 (&acc)[4],
                      const int4v (&last)[NB], bool has_last, int k) {
  constexpr int KB = SgLane<FP8>::KB;
  const int kt = has_last ? k + NB * KB : k;
  int4v tb[NTL > 0 ? NTL : 1];
  #pragma unroll
  for (int t = 0; t < NTL; t++) tb[t] = ln.ldw(kt + t * KB);
  __builtin_amdgcn_sched_barrier(0);
  if (has_last) ln.template mma_batch<NB>(acc, last, k);
  #pragma unroll
  for (int t = 0; t < NTL; t++) ln.mma(acc, tb[t], kt + t * KB, 0);
}

// ntail (0 .. NB-1, uniform) picks the compile-time tail length
template <bool FP8, int NB, int NTL = 0>
DEVINL void sg_finish_n(const SgLane<FP8>& ln, f32x4 (&acc)[4],
                        const int4v (&last)[NB], bool has_last, int k,
                        int ntail) {
  if (ntail == NTL) sg_finish<FP8, NB, NTL>(ln, acc, last, has_last, k);
  else if constexpr (NTL + 2 < NB)
    sg_finish_n<FP8, NB, NTL + 1>(ln, acc, last, has_last, k, ntail);
  else sg_finish<FP8, NB, NB - 1>(ln, acc, last, has_last, k);
}

// acc <- this lane's part of x[0..16)[k_lo..k_hi) @ W[n0 + i16][k_lo..k_hi)
// (unscaled in FP8 mode).  wrow: row n0 + i16 of W (bf16) or q (e4m3 bytes).
template <bool FP8, int NB, int NT>
DEVINL void sg_slice(f32x4 (&acc)[4], __bf16* x_s, const bf16* __restrict__ x,
                     const void* __restrict__ wrow, int g, int i16, int M,
                     int K, int k_lo, int k_hi, int kslice) {
  constexpr int KB = SgLane<FP8>::KB;
  constexpr int S = NB * KB;
  SgLane<FP8> ln;
  ln.wl = (const char*)wrow + g * 16;
  ln.x_s = x_s;
  ln.xo = i16 * kslice + g * (KB / 4) - k_lo;
  int nb = (k_hi - k_lo) / S;  // full batches
  const int ntail = ((k_hi - k_lo) - nb * S) / KB;

  bf16x8 xv[SG_XV];
  sg_x_load<NT>(xv, x, M, K, k_lo, k_hi, kslice);
  int4v b0[NB], b1[NB];
  int kk = k_lo;
  // unconditional (a branch here makes every later wait assume it was not
  // taken and drain W): without a full batch, NB loads of the first block
  #pragma unroll
  for (int t = 0; t < NB; t++) b0[t] = ln.ldw(nb > 0 ? kk + t * KB : kk);
  __builtin_amdgcn_sched_barrier(0);
  sg_x_store<NT>(x_s, xv, x, M, K, k_lo, k_hi, kslice);
  __syncthreads();

  if (nb == 0) {  // K 32 .. 96: no full batch, b0 is not used
    sg_finish_n<FP8, NB>(ln, acc, b0, false, kk, ntail);
    return;
  }
  // b0 holds (in flight) the batch at kk; nb batches remain, it included
  while (nb > 2) {
    ln.template ldw_batch<NB>(b1, kk + S);
    ln.template mma_batch<NB>(acc, b0, kk);
    ln.template ldw_batch<NB>(b0, kk + 2 * S);
    ln.template mma_batch<NB>(acc, b1, kk + S);
    kk += 2 * S;
    nb -= 2;
  }
  if (nb == 2) {
    ln.template ldw_batch<NB>(b1, kk + S);
    ln.template mma_batch<NB>(acc, b0, kk);
    sg_finish_n<FP8, NB>(ln, acc, b1, true, kk + S, ntail);
  } else {
    sg_finish_n<FP8, NB>(ln, acc, b0, true, kk, ntail);
  }
}

// NB x 32-deep k body, two batches of NB 16-byte W loads in flight/lane.
// WVS = waves per workgroup (n-tile = WVS*16): 4 (=SG_TN 64) default; 2
// halves the tile for TAIL-BOUND small-N shapes (o-proj N=4096: 64 tiles left
// 88% of wave cycles parked in PMC — 128 tiles x half work fills the tail).
// 4 rotating accumulators relax the MFMA RAW chain (PMC: 35%
// SQ_WAIT_INST_ANY with 2 accs at the qkv shape).  Plain loads: nt loads
// measured 15-40% SLOWER here.
template <int NB, int WVS = 4>
__global__ __launch_bounds__(64 * WVS, 4) void skinny_gemm_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    float* __restrict__ out32, int M, int N, int K, int kslice) {
  const int ntile = blockIdx.x;
  const int ks = blockIdx.y;
  const int k_lo = ks * kslice;
  const int k_hi = min(K, k_lo + kslice);
  const auto [lane, wv, i16, g] = mfma_lane();
  const int n0 = ntile * (WVS * 16) + wv * 16;

  extern __shared__ __bf16 x_s[];  // [16][kslice] rows (zero-padded m >= M)
  f32x4 acc[4] = {};
  sg_slice<false, NB, 64 * WVS>(acc, x_s, x, w + (long)(n0 + i16) * K, g, i16,
                                M, K, k_lo, k_hi, kslice);
  // non-atomic per-K-slice partial: out32[ks][m][n]
  #pragma unroll
  for (int r = 0; r < 4; r++) {
    int m = g * 4 + r;
    float vsum = acc[0][r] + acc[1][r] + acc[2][r] + acc[3][r];
    if (m < M)
      out32[((long)ks * M + m) * N + n0 + i16] = vsum;
  }
}

// pipeline depth: 4 (default) or 8 via REALHF_AMD_SKINNY_DEPTH=8
static int sg_depth() {
  static int d = [] {
    const char* e = getenv("REALHF_AMD_SKINNY_DEPTH");
    return (e && e[0] == '8') ? 8 : 4;
  }();
  return d;
}

// n-tile width threshold: shapes with N <= this use the 32-wide tile
// (2 waves).  Default 0 = DISABLED: the in-context A/B measured 3.55 vs
// 3.66 samples/s with it on at 4096 — doubling the workgroups also
// doubles the per-WG x-LDS stage and the tail moves, it does not
// shrink.  Kept env-gated (REALHF_AMD_SG_TN32_MAXN) for other shapes.
static int sg_tn32_maxn() {
  static int v = [] {
    const char* e = getenv("REALHF_AMD_SG_TN32_MAXN");
    return e ? atoi(e) : 0;
  }();
  return v;
}

// combine the nks fp32 partial slabs -> bf16 (+ optional residual add)
__global__ void sg_combine_kernel(const float* __restrict__ parts,
                                  const bf16* __restrict__ resid,
                                  bf16* __restrict__ out, long n, int nks) {
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n;
       i += (long)gridDim.x * blockDim.x * 4)
    sg_reduce_store(parts, n, nks, i, resid, out);
}

// ---------------------------------------------------------------------------
// no-combine variant: run ONLY the split-K GEMM and hand the fp32 partial
// slabs [nks, M, N] to the NEXT kernel's prologue (launch-boundary
// reduce, guide split-K recipe: "combine in the NEXT kernel's prologue
// ... costs nothing extra when that kernel exists anyway").  Consumers:
// rope_qkv_decode / add_rmsnorm_fwd / swiglu_fwd slab modes.
struct SgShape { int M, N, K, kslice, nks; size_t lds; };

// x [M, K] bf16; w [N, K] bf16 (row-major view, stride(1)==1);
// out32_ws: fp32 workspace >= nks * M * N (per-slice partials — no
// zeroing, no atomics)
static SgShape sg_shape(const torch::Tensor& x, const torch::Tensor& w,
                        const torch::Tensor& out32_ws, long splitk) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1);
  TORCH_CHECK(w.dim() == 2 && w.stride(1) == 1);
  SgShape s;
  s.M = x.size(0); s.K = x.size(1); s.N = w.size(0);
  TORCH_CHECK(s.M <= 16 && s.K % 32 == 0 && s.N % SG_TN == 0);
  TORCH_CHECK(x.stride(0) == s.K, "x must be contiguous");
  s.kslice = (s.K / (int)splitk + 63) / 64 * 64;
  s.nks = (s.K + s.kslice - 1) / s.kslice;
  TORCH_CHECK(out32_ws.numel() >= (long)s.nks * s.M * s.N, "workspace too small");
  s.lds = (size_t)16 * s.kslice * sizeof(short);
  TORCH_CHECK(s.lds <= 160 * 1024, "kslice too large for LDS");
  return s;
}

// the [nks, M, N] slab view of the workspace
static torch::Tensor sg_slabs(const torch::Tensor& out32_ws, const SgShape& s) {
  return out32_ws.narrow(0, 0, (long)s.nks * s.M * s.N)
      .view({(long)s.nks, (long)s.M, (long)s.N});
}

// launch the split-K partial kernel; returns the [nks, M, N] slab view
static torch::Tensor sg_partials(const torch::Tensor& x, const torch::Tensor& w,
                                 const torch::Tensor& out32_ws,
                                 const SgShape& s) {
  auto out32 = sg_slabs(out32_ws, s);
  auto launch = [&](auto nb, auto wvs) {
    dim3 grid(s.N / (16 * wvs.value), s.nks);
    hipLaunchKernelGGL((skinny_gemm_kernel<nb.value, wvs.value>), grid,
      dim3(64 * wvs.value), s.lds, cur_stream(),
      (const bf16*)x.data_ptr(), (const bf16*)w.data_ptr(),
      out32.data_ptr<float>(), s.M, s.N, s.K, s.kslice);
  };
  using c4 = std::integral_constant<int, 4>;
  using c8 = std::integral_constant<int, 8>;
  using c2 = std::integral_constant<int, 2>;
  const bool tn32 = s.N <= sg_tn32_maxn() && (s.N % 32) == 0;
  if (sg_depth() == 8) { if (tn32) launch(c8{}, c2{}); else launch(c8{}, c4{}); }
  else { if (tn32) launch(c4{}, c2{}); else launch(c4{}, c4{}); }
  return out32;
}

static const bf16* sg_resid_ptr(const c10::optional<torch::Tensor>& residual,
                                long n) {
  if (!residual.has_value()) return nullptr;
  TORCH_CHECK(residual->is_contiguous() && residual->numel() == n);
  return (const bf16*)residual->data_ptr();
}

// launch the combine kernel over the slabs (residual, optional [M, N] bf16,
// is folded into it); returns the bf16 [M, N] result, allocated like x
static torch::Tensor sg_combine(const torch::Tensor& out32,
                                const torch::Tensor& x, const SgShape& s,
                                const c10::optional<torch::Tensor>& residual) {
  auto out = torch::empty({s.M, (long)s.N}, x.options());
  long n = (long)s.M * s.N;
  int cgrid = (int)std::min<long>((n / 4 + 255) / 256, 2048);
  const bf16* rptr = sg_resid_ptr(residual, n);
  hipLaunchKernelGGL(sg_combine_kernel, dim3(cgrid), dim3(256), 0,
    cur_stream(), out32.data_ptr<float>(), rptr, (bf16*)out.data_ptr(), n,
    s.nks);
  CHECK_CUDA_OK();
  return out;
}

torch::Tensor skinny_gemm_nc(torch::Tensor x, torch::Tensor w,
                             torch::Tensor out32_ws, long splitk) {
  auto out32 = sg_partials(x, w, out32_ws, sg_shape(x, w, out32_ws, splitk));
  CHECK_CUDA_OK();
  return out32;
}

// ---------------------------------------------------------------------------
// v2: split-K combine fused into the GEMM kernel via self-resetting
// semaphores — the LAST workgroup to finish an n-tile sums the fp32
// partial slabs, folds the residual, converts to bf16 and resets the
// tile's counter (so the sem buffer only needs zeroing once, at
// allocation).  Removes the separate sg_combine launch (~5 us x 4 per
// decode layer) and its extra fp32 pass.  256-deep k body keeps 8
// 16-byte W loads in flight per lane (vs 4 in v1).
__global__ __launch_bounds__(256, 4) void skinny_gemm2_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    float* __restrict__ out32, int* __restrict__ sem,
    const bf16* __restrict__ resid, bf16* __restrict__ out,
    int M, int N, int K, int kslice, int nks) {
  // 1-D grid; when the tile count divides by 8, keep all K-slices of one
  // n-tile on ONE XCD (the dispatcher places block b on XCD b%8) so the
  // reducer reads same-XCD slabs — a pure speed choice, correctness comes
  // from the agent-scope fences below (guide §6 G16 / split-K recipe).
  const int nt_total = N / SG_TN;
  int ntile, ks;
  {
    const int id = blockIdx.x;
    if ((nt_total & 7) == 0) {
      const int ix = id >> 3;
      ntile = (id & 7) * (nt_total >> 3) + ix / nks;
      ks = ix % nks;
    } else {
      ntile = id / nks;
      ks = id % nks;
    }
  }
  const int k_lo = ks * kslice;
  const int k_hi = min(K, k_lo + kslice);
  const auto [lane, wv, i16, g] = mfma_lane();
  const int n0 = ntile * SG_TN + wv * 16;

  extern __shared__ __bf16 x_s[];  // [16][kslice] rows (zero-padded m >= M)
  sg_stage_x<256>(x_s, x, M, K, k_lo, k_hi, kslice);
  __syncthreads();

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const bf16* wrow = w + (long)(n0 + i16) * K;
  int kk = k_lo;
  for (; kk + 256 <= k_hi; kk += 256) {
    bf16x8 b0 = *(const bf16x8*)(wrow + kk + g * 8);
    bf16x8 b1 = *(const bf16x8*)(wrow + kk + 32 + g * 8);
    bf16x8 b2 = *(const bf16x8*)(wrow + kk + 64 + g * 8);
    bf16x8 b3 = *(const bf16x8*)(wrow + kk + 96 + g * 8);
    bf16x8 b4 = *(const bf16x8*)(wrow + kk + 128 + g * 8);
    bf16x8 b5 = *(const bf16x8*)(wrow + kk + 160 + g * 8);
    bf16x8 b6 = *(const bf16x8*)(wrow + kk + 192 + g * 8);
    bf16x8 b7 = *(const bf16x8*)(wrow + kk + 224 + g * 8);
    const long xb = (long)i16 * kslice + (kk - k_lo) + g * 8;
    bf16x8 a0 = *(const bf16x8*)(&x_s[xb]);
    bf16x8 a1 = *(const bf16x8*)(&x_s[xb + 32]);
    bf16x8 a2 = *(const bf16x8*)(&x_s[xb + 64]);
    bf16x8 a3 = *(const bf16x8*)(&x_s[xb + 96]);
    bf16x8 a4 = *(const bf16x8*)(&x_s[xb + 128]);
    bf16x8 a5 = *(const bf16x8*)(&x_s[xb + 160]);
    bf16x8 a6 = *(const bf16x8*)(&x_s[xb + 192]);
    bf16x8 a7 = *(const bf16x8*)(&x_s[xb + 224]);
    acc0 = mfma16(a0, b0, acc0);
    acc1 = mfma16(a1, b1, acc1);
    acc0 = mfma16(a2, b2, acc0);
    acc1 = mfma16(a3, b3, acc1);
    acc0 = mfma16(a4, b4, acc0);
    acc1 = mfma16(a5, b5, acc1);
    acc0 = mfma16(a6, b6, acc0);
    acc1 = mfma16(a7, b7, acc1);
  }
  for (; kk + 32 <= k_hi; kk += 32) {
    bf16x8 a0 = *(const bf16x8*)(&x_s[(long)i16 * kslice + (kk - k_lo) + g * 8]);
    bf16x8 b0 = *(const bf16x8*)(wrow + kk + g * 8);
    acc0 = mfma16(a0, b0, acc0);
  }
  // publish the fp32 slab with plain stores
  #pragma unroll
  for (int r = 0; r < 4; r++) {
    int m = g * 4 + r;
    if (m < M)
      out32[((long)ks * M + m) * N + n0 + i16] = acc0[r] + acc1[r];
  }

  // --- in-launch split-K hand-off (guide split-K recipe, counter form):
  // every wave drains its stores; lane 0 issues ONE agent-scope release
  // (buffer_wbl2) with the post-fence wait restated (ROCm 7.2 drops it
  // otherwise), THEN takes a relaxed ticket.  NEVER __threadfence() per
  // block — that is a per-WG L2 writeback+invalidate, measured 4x slower
  // end-to-end in the decode graph.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  volatile int* flag = (volatile int*)x_s;  // reuse the ONE shared array
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int tick = __hip_atomic_fetch_add(&sem[ntile], 1, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
    flag[0] = (tick == nks - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!flag[0]) return;

  // --- last arriver reduces: one agent-scope acquire (drops this CU's
  // L1), then plain 16-B slab loads.  Thread t owns row t/16, columns
  // 4*(t%16)..+3 of the 16 x 64 tile.
  if (threadIdx.x == 0)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  __syncthreads();
  const int base_n = ntile * SG_TN;
  const int m = threadIdx.x >> 4;
  const int c4 = (threadIdx.x & 15) * 4;
  if (m < M)
    sg_reduce_store(out32, (long)M * N, nks, (long)m * N + base_n + c4, resid,
                    out);
  // self-reset so the persistent sem buffer is zero for the next launch
  // (stream order makes this safe; the buffer is zeroed once at alloc)
  if (threadIdx.x == 0)
    __hip_atomic_store(&sem[ntile], 0, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

torch::Tensor skinny_gemm2(torch::Tensor x, torch::Tensor w,
                           torch::Tensor out32_ws, torch::Tensor sem,
                           long splitk, c10::optional<torch::Tensor> residual) {
  const SgShape s = sg_shape(x, w, out32_ws, splitk);
  TORCH_CHECK(sem.scalar_type() == torch::kInt32 && sem.numel() >= s.N / SG_TN,
              "semaphore buffer too small (must be zero-initialized once)");
  auto out = torch::empty({s.M, (long)s.N}, x.options());
  const bf16* rptr = sg_resid_ptr(residual, (long)s.M * s.N);
  dim3 grid((s.N / SG_TN) * s.nks);  // 1-D: kernel derives (tile, slice)
  hipLaunchKernelGGL(skinny_gemm2_kernel, grid, dim3(256), s.lds, cur_stream(),
    (const bf16*)x.data_ptr(), (const bf16*)w.data_ptr(),
    out32_ws.data_ptr<float>(), sem.data_ptr<int>(), rptr,
    (bf16*)out.data_ptr(), s.M, s.N, s.K, s.kslice, s.nks);
  CHECK_CUDA_OK();
  return out;
}

// partials, then the combine kernel
torch::Tensor skinny_gemm(torch::Tensor x, torch::Tensor w,
                          torch::Tensor out32_ws, long splitk,
                          c10::optional<torch::Tensor> residual) {
  const SgShape s = sg_shape(x, w, out32_ws, splitk);
  return sg_combine(sg_partials(x, w, out32_ws, s), x, s, residual);
}

// ---------------------------------------------------------------------------
// FP8 weight-only variant: W is stored as OCP e4m3fn codes q[N, K] (one
// byte per element) with one fp32 scale per row, W[n, k] = q[n, k] *
// scale[n] (quantize_fp8.hip).  x stays bf16; half the weight bytes are
// streamed.
//
// Fragment mapping.  The W stream keeps its 16 bytes per lane, which is now
// 16 k-elements, so one load feeds TWO mfma16 steps and the k body is 64
// deep per load.  Lane (i16, g) owns k in [g*16, g*16 + 16) of each
// 64-block: its low 8 bytes are the B fragment of the first MFMA, its high
// 8 bytes of the second.  An MFMA sums over k in whatever order the lanes
// present it, provided A and B agree: mfma.h puts logical k = g*8 + j in
// lane (i16, g) slot j of both operands, so the A fragments are read from
// x_s at the SAME physical offsets, x_s[i16][g*16 + 0..7] and
// x_s[i16][g*16 + 8..15].
//
// Conversion.  e4m3 -> f32 by v_cvt_pk_f32_fp8 (subnormals included), then
// the upper 16 bits are the bf16: exact, an e4m3 value has 3 mantissa bits
// and bf16 keeps 7.  The MFMA therefore sees q exactly, and the row scale is
// applied once per output in the epilogue, before the fp32 partial is
// stored: the slabs mean what the bf16 kernel's slabs mean and every slab
// consumer (sg_combine_kernel, rope_qkv_decode, add_rmsnorm, swiglu/geglu)
// is unchanged.
DEVINL unsigned sg_bf16_pair(float lo, float hi) {
  return (__builtin_bit_cast(unsigned, lo) >> 16) |
         (__builtin_bit_cast(unsigned, hi) & 0xffff0000u);
}

// 8 consecutive e4m3 bytes (lo = bytes 0..3, hi = 4..7) -> bf16x8, in order
DEVINL bf16x8 sg_e4m3x8_to_bf16(int lo, int hi) {
  const float2v p0 = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false);
  const float2v p1 = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
  const float2v p2 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false);
  const float2v p3 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
  int4v u;
  u[0] = (int)sg_bf16_pair(p0[0], p0[1]);
  u[1] = (int)sg_bf16_pair(p1[0], p1[1]);
  u[2] = (int)sg_bf16_pair(p2[0], p2[1]);
  u[3] = (int)sg_bf16_pair(p3[0], p3[1]);
  return __builtin_bit_cast(bf16x8, u);
}

// NB x 64-deep k body (sg_slice<true>): 2*NB MFMAs per batch of NB q loads
template <int NB>
__global__ __launch_bounds__(256, 4) void skinny_gemm_fp8_kernel(
    const bf16* __restrict__ x, const unsigned char* __restrict__ q,
    const float* __restrict__ scale, float* __restrict__ out32, int M, int N,
    int K, int kslice) {
  const int ntile = blockIdx.x;
  const int ks = blockIdx.y;
  const int k_lo = ks * kslice;
  const int k_hi = min(K, k_lo + kslice);  // K, kslice % 64 == 0
  const auto [lane, wv, i16, g] = mfma_lane();
  const int n0 = ntile * SG_TN + wv * 16;

  extern __shared__ __bf16 x_s[];  // [16][kslice] rows (zero-padded m >= M)
  const float sc = scale[n0 + i16];  // first out, so never waited for alone
  f32x4 acc[4] = {};
  sg_slice<true, NB, 256>(acc, x_s, x, q + (long)(n0 + i16) * K, g, i16, M, K,
                          k_lo, k_hi, kslice);
  // row scale once per output, then the per-K-slice partial out32[ks][m][n]
  #pragma unroll
  for (int r = 0; r < 4; r++) {
    int m = g * 4 + r;
    float vsum = acc[0][r] + acc[1][r] + acc[2][r] + acc[3][r];
    if (m < M)
      out32[((long)ks * M + m) * N + n0 + i16] = vsum * sc;
  }
}

// q [N, K] one byte per element (e4m3 codes), rows contiguous; scale fp32 [N]
static SgShape sg_shape_fp8(const torch::Tensor& x, const torch::Tensor& q,
                            const torch::Tensor& scale,
                            const torch::Tensor& out32_ws, long splitk) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 2 && q.element_size() == 1 &&
              q.is_contiguous() && (uintptr_t)q.data_ptr() % 16 == 0,
              "q must be contiguous, 16-byte aligned [N, K] e4m3 bytes");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == q.size(1), "x / q K mismatch");
  TORCH_CHECK(q.size(1) % 64 == 0, "fp8 skinny GEMM needs K % 64 == 0");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat32 &&
              scale.is_contiguous() && scale.numel() == q.size(0),
              "scale must be contiguous fp32 [N]");
  TORCH_CHECK(out32_ws.is_cuda() && out32_ws.scalar_type() == torch::kFloat32);
  return sg_shape(x, q, out32_ws, splitk);
}

static torch::Tensor sg_partials_fp8(const torch::Tensor& x,
                                     const torch::Tensor& q,
                                     const torch::Tensor& scale,
                                     const torch::Tensor& out32_ws,
                                     const SgShape& s) {
  auto out32 = sg_slabs(out32_ws, s);
  hipLaunchKernelGGL((skinny_gemm_fp8_kernel<4>), dim3(s.N / SG_TN, s.nks),
    dim3(256), s.lds, cur_stream(), (const bf16*)x.data_ptr(),
    (const unsigned char*)q.data_ptr(), scale.data_ptr<float>(),
    out32.data_ptr<float>(), s.M, s.N, s.K, s.kslice);
  return out32;
}

torch::Tensor skinny_gemm_fp8_nc(torch::Tensor x, torch::Tensor q,
                                 torch::Tensor scale, torch::Tensor out32_ws,
                                 long splitk) {
  auto out32 = sg_partials_fp8(x, q, scale, out32_ws,
                               sg_shape_fp8(x, q, scale, out32_ws, splitk));
  CHECK_CUDA_OK();
  return out32;
}

torch::Tensor skinny_gemm_fp8(torch::Tensor x, torch::Tensor q,
                              torch::Tensor scale, torch::Tensor out32_ws,
                              long splitk,
                              c10::optional<torch::Tensor> residual) {
  const SgShape s = sg_shape_fp8(x, q, scale, out32_ws, splitk);
  return sg_combine(sg_partials_fp8(x, q, scale, out32_ws, s), x, s, residual);
}
