// The skinny GEMM's device building blocks, shared by skinny_gemm.hip and
// moe_decode.hip: the x stage (sg_stage_x, sg_x_load / sg_x_store), the W
// load pipeline of one K-slice (SgLane, sg_finish, sg_slice) and the slab
// reduce of the combine (sg_reduce_store).  Host side: sg_combine_slabs
// launches the combine kernel over any [n, M, N] slab stack.
#pragma once
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

// e4m3 -> bf16 for the FP8 weight streams (skinny_gemm.hip "Conversion",
// moe_decode.hip): v_cvt_pk_f32_fp8, then the upper 16 bits of each f32
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

// bf16 [M, N] = sum of the n fp32 slabs [n, M, N] (+ residual [M, N] bf16),
// summed in slab order by sg_combine_kernel (skinny_gemm.hip); allocated
// like `like`
torch::Tensor sg_combine_slabs(const torch::Tensor& slabs,
                               const torch::Tensor& like,
                               const c10::optional<torch::Tensor>& residual);
