// MoE decode (gfx950): M <= 16 tokens, each routed to k distinct experts, so an
// expert sees at most one 16-row MFMA tile and the step is bound by streaming
// the weights of the experts that were chosen.  Three kernels, no host sync,
// no sort, no [tokens*k, hidden] copy, no atomics:
//
//   moe_route_decode    idx [M, k] int32, wts [M, k] fp32: router logits,
//                       fp32 softmax and top-k, one workgroup per token
//   moe_gate_up_swiglu  act [k, M, I] bf16, row (j, t) = silu(h_t Wg[e]^T) *
//                       (h_t Wu[e]^T) for e = idx[t, j]; grid (I/64, E)
//   moe_down            fp32 slabs [nks*k, M, H], slab (s, j) row t =
//                       wts[t, j] * act[j, t, k_s-slice] Wd[idx[t, j]]^T;
//                       grid (H/64, E, nks)
//
// and sg_combine_slabs (skinny_gemm.h) sums the nks*k slabs in order, folds the
// residual and rounds to bf16 once: the layer output.  moe_gate_up_swiglu_fp8
// and moe_down_fp8 (section 4) are the two expert kernels over e4m3 codes with
// per-row scales.
//
// Routing inside the expert kernels.  A workgroup belongs to one expert e.
// Lanes 0..15 of every wave scan idx (<= 128 ints): lane t finds the slot j
// with idx[t, j] == e, or -1.  If no token chose e the workgroup returns before
// its first weight load, so the bytes streamed follow the experts in use.
// Otherwise all 16 rows of the MFMA tile are staged and only routed rows are
// stored, to row (slot, t): each row of act and of every slab has exactly
// one writer because a token's k experts are distinct.  idx is compared, never
// used as an address.
//
// The W pipeline is sg_slice's (skinny_gemm.h): two register batches of NB
// 16-byte loads per lane and stream in flight across the MFMAs, the tail
// issued with the last batch.  NS streams share one x stage and one A
// fragment read per MFMA pair: gate and up rows of the same expert (NS = 2)
// halve the x restaging per weight byte.
#include "skinny_gemm.h"

// fp32 math in this file stays on the scalar-per-lane VALU forms
// (v_fma_f32, ...): no packed-fp32 instruction selection for its kernels
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define MOE_KSLICE 1024  // x stage: 16 x 1024 bf16 = 32 KiB = NT*SG_XV pieces
#define MOE_NT 256
#define MOE_MAX_K 8
#define MOE_MAX_E 256

// slot of expert e in token `lane`'s choices (lanes >= M and tokens that did
// not choose e: -1).  All MOE_MAX_K loads go out before the compares; slots
// past k read idx[0] and are dropped.
DEVINL int moe_slot(const int* __restrict__ idx, int M, int k, int e, int lane) {
  const bool row = lane < M;
  int v[MOE_MAX_K];
  #pragma unroll
  for (int j = 0; j < MOE_MAX_K; j++)
    v[j] = idx[row && j < k ? lane * k + j : 0];
  int slot = -1;
  #pragma unroll
  for (int j = MOE_MAX_K - 1; j >= 0; j--)
    if (row && j < k && v[j] == e) slot = j;
  return slot;
}

// this lane's view of NS weight rows and of x_s.  KB = k elements per 16-byte
// W load: 32 (bf16) or 64 (FP8: e4m3 codes, SgLane<true>'s fragment mapping:
// the lane owns k in [16g, 16g + 16) of each 64-block, its low 8 bytes feed
// the first MFMA of the load and its high 8 bytes the second)
template <int NS, bool FP8 = false>
struct MoeLane {
  static constexpr int KB = FP8 ? 64 : 32;
  static constexpr int WB = FP8 ? 1 : 2;  // bytes per W element
  const char* wl[NS];  // the lane's W bytes for k = 0, per stream
  const __bf16* x_s;
  int xo;              // x_s index of the lane's first element of k is xo + k
};

// full = false: NB loads of the block at k (a slice shorter than a batch must
// not be read past its end)
template <int NS, int NB, bool FP8>
DEVINL void moe_ldw(int4v (&b)[NS][NB], const MoeLane<NS, FP8>& ln, int k,
                    bool full = true) {
  constexpr int KB = MoeLane<NS, FP8>::KB, WB = MoeLane<NS, FP8>::WB;
  #pragma unroll
  for (int s = 0; s < NS; s++) {
    #pragma unroll
    for (int t = 0; t < NB; t++)
      b[s][t] = *(const int4v*)(ln.wl[s] + (long)(full ? k + t * KB : k) * WB);
  }
  __builtin_amdgcn_sched_barrier(0);  // issued HERE, as SgLane::ldw_batch
}

// one A fragment per k block, shared by the streams; element t on acc[.][j & 3]
// (FP8: two A fragments and two MFMAs per load, on acc[.][2j & 3] and
// acc[.][(2j + 1) & 3]; the codes reach the MFMA exactly, the row scale waits
// for the epilogue)
template <int NS, bool FP8>
DEVINL void moe_mma1(f32x4 (&acc)[NS][4], const MoeLane<NS, FP8>& ln,
                     const int4v (&b)[NS], int k, int j) {
  const bf16x8 a = *(const bf16x8*)(&ln.x_s[ln.xo + k]);
  if constexpr (FP8) {
    const bf16x8 a1 = *(const bf16x8*)(&ln.x_s[ln.xo + k + 8]);
    #pragma unroll
    for (int s = 0; s < NS; s++) {
      acc[s][(2 * j) & 3] = mfma16(a, sg_e4m3x8_to_bf16(b[s][0], b[s][1]),
                                   acc[s][(2 * j) & 3]);
      acc[s][(2 * j + 1) & 3] = mfma16(a1, sg_e4m3x8_to_bf16(b[s][2], b[s][3]),
                                       acc[s][(2 * j + 1) & 3]);
    }
  } else {
    #pragma unroll
    for (int s = 0; s < NS; s++)
      acc[s][j & 3] = mfma16(a, __builtin_bit_cast(bf16x8, b[s]), acc[s][j & 3]);
  }
}

template <int NS, int NB, bool FP8>
DEVINL void moe_mma(f32x4 (&acc)[NS][4], const MoeLane<NS, FP8>& ln,
                    const int4v (&b)[NS][NB], int k) {
  #pragma unroll
  for (int t = 0; t < NB; t++) {
    int4v bt[NS];
    #pragma unroll
    for (int s = 0; s < NS; s++) bt[s] = b[s][t];
    moe_mma1<NS, FP8>(acc, ln, bt, k + t * MoeLane<NS, FP8>::KB, t);
  }
}

// the end of a slice (sg_finish for NS streams): the NTL tail loads of every
// stream go out together, then the MFMAs of the last full batch, then the
// tail's (on acc[.][0]; FP8: acc[.][0] and acc[.][1])
template <int NS, int NB, int NTL, bool FP8>
DEVINL void moe_finish(f32x4 (&acc)[NS][4], const MoeLane<NS, FP8>& ln,
                       const int4v (&last)[NS][NB], bool has_last, int k) {
  constexpr int KB = MoeLane<NS, FP8>::KB, WB = MoeLane<NS, FP8>::WB;
  const int kt = has_last ? k + NB * KB : k;
  int4v tb[NTL > 0 ? NTL : 1][NS];
  #pragma unroll
  for (int t = 0; t < NTL; t++) {
    #pragma unroll
    for (int s = 0; s < NS; s++)
      tb[t][s] = *(const int4v*)(ln.wl[s] + (long)(kt + t * KB) * WB);
  }
  __builtin_amdgcn_sched_barrier(0);
  if (has_last) moe_mma<NS, NB, FP8>(acc, ln, last, k);
  #pragma unroll
  for (int t = 0; t < NTL; t++)
    moe_mma1<NS, FP8>(acc, ln, tb[t], kt + t * KB, 0);
}

template <int NS, int NB, bool FP8, int NTL = 0>
DEVINL void moe_finish_n(f32x4 (&acc)[NS][4], const MoeLane<NS, FP8>& ln,
                         const int4v (&last)[NS][NB], bool has_last, int k,
                         int ntail) {
  if (ntail == NTL) moe_finish<NS, NB, NTL, FP8>(acc, ln, last, has_last, k);
  else if constexpr (NTL + 2 < NB)
    moe_finish_n<NS, NB, FP8, NTL + 1>(acc, ln, last, has_last, k, ntail);
  else moe_finish<NS, NB, NB - 1, FP8>(acc, ln, last, has_last, k);
}

// the W stream of one slice [k_lo, k_hi) once x_s holds it: b0 carries (in
// flight) the first batch, issued by the caller before it stored x.  Same
// issue order and MFMA order as sg_slice.
template <int NS, int NB, bool FP8>
DEVINL void moe_stream(f32x4 (&acc)[NS][4], const MoeLane<NS, FP8>& ln,
                       int4v (&b0)[NS][NB], int k_lo, int k_hi) {
  constexpr int KB = MoeLane<NS, FP8>::KB;
  constexpr int S = NB * KB;
  int nb = (k_hi - k_lo) / S;
  const int ntail = ((k_hi - k_lo) - nb * S) / KB;
  int kk = k_lo;
  if (nb == 0) {
    moe_finish_n<NS, NB, FP8>(acc, ln, b0, false, kk, ntail);
    return;
  }
  int4v b1[NS][NB];
  while (nb > 2) {
    moe_ldw<NS, NB, FP8>(b1, ln, kk + S);
    moe_mma<NS, NB, FP8>(acc, ln, b0, kk);
    moe_ldw<NS, NB, FP8>(b0, ln, kk + 2 * S);
    moe_mma<NS, NB, FP8>(acc, ln, b1, kk + S);
    kk += 2 * S;
    nb -= 2;
  }
  if (nb == 2) {
    moe_ldw<NS, NB, FP8>(b1, ln, kk + S);
    moe_mma<NS, NB, FP8>(acc, ln, b0, kk);
    moe_finish_n<NS, NB, FP8>(acc, ln, b1, true, kk + S, ntail);
  } else {
    moe_finish_n<NS, NB, FP8>(acc, ln, b0, true, kk, ntail);
  }
}

// ---------------------------------------------------------------------------
// 1. router: one workgroup per token.  The token's row sits in LDS as fp32;
// waves take experts round-robin, two per trip (two independent load chains),
// 16-byte router loads, fp32 FMA in a fixed order, wave_sum.  Wave 0 then does
// the fp32 softmax over the E logits and k rounds of arg-max (lowest index
// wins a tie), and lane 0 writes the token's k (index, weight) pairs.
// ---------------------------------------------------------------------------
#define MOE_ROUTE_NT 1024

DEVINL float moe_dot8(const bf16x8& w, const float* __restrict__ h, float acc) {
  #pragma unroll
  for (int j = 0; j < 8; j++) acc = fmaf((float)w[j], h[j], acc);
  return acc;
}

__global__ __launch_bounds__(MOE_ROUTE_NT) void moe_route_kernel(
    const bf16* __restrict__ h, const bf16* __restrict__ rw,
    int* __restrict__ idx, float* __restrict__ wts, int H, int E, int k,
    int norm_topk) {
  extern __shared__ float route_s[];  // [H] token row, then [MOE_MAX_E] logits
  float* const h_s = route_s;
  float* const lg_s = route_s + H;
  const int t = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  constexpr int NW = MOE_ROUTE_NT / 64;

  for (int c = threadIdx.x * 8; c < H; c += MOE_ROUTE_NT * 8) {
    const bf16x8 v = *(const bf16x8*)((const __bf16*)h + (long)t * H + c);
    #pragma unroll
    for (int j = 0; j < 8; j++) h_s[c + j] = (float)v[j];
  }
  __syncthreads();

  for (int e0 = wv; e0 < E; e0 += 2 * NW) {
    const int e1 = e0 + NW;
    const bool two = e1 < E;
    const __bf16* r0 = (const __bf16*)rw + (long)e0 * H;
    const __bf16* r1 = (const __bf16*)rw + (long)(two ? e1 : e0) * H;
    float a0 = 0.f, a1 = 0.f;
    for (int c = lane * 8; c < H; c += 64 * 8) {
      const bf16x8 w0 = *(const bf16x8*)(r0 + c);
      const bf16x8 w1 = *(const bf16x8*)(r1 + c);
      a0 = moe_dot8(w0, h_s + c, a0);
      a1 = moe_dot8(w1, h_s + c, a1);
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if (lane == 0) {
      lg_s[e0] = a0;
      if (two) lg_s[e1] = a1;
    }
  }
  __syncthreads();
  if (wv != 0) return;

  // lane l owns experts l, l + 64, l + 128, l + 192
  constexpr int PL = MOE_MAX_E / 64;
  float p[PL];
  float mx = -INFINITY;
  #pragma unroll
  for (int i = 0; i < PL; i++) {
    const int e = lane + 64 * i;
    p[i] = e < E ? lg_s[e] : -INFINITY;
    mx = fmaxf(mx, p[i]);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  #pragma unroll
  for (int i = 0; i < PL; i++) {
    p[i] = lane + 64 * i < E ? expf(p[i] - mx) : -1.f;  // -1: never picked
    sum += fmaxf(p[i], 0.f);
  }
  sum = wave_sum(sum);
  #pragma unroll
  for (int i = 0; i < PL; i++) p[i] = p[i] >= 0.f ? p[i] / sum : -1.f;

  int sel_i[MOE_MAX_K];
  float sel_w[MOE_MAX_K];
  float tot = 0.f;
  #pragma unroll
  for (int r = 0; r < MOE_MAX_K; r++) {
    // the lane's best (strict >: the lowest of its indices wins), then the
    // wave's (ties to the lower expert index)
    float bv = -2.f;
    int bi = MOE_MAX_E;
    #pragma unroll
    for (int i = 0; i < PL; i++)
      if (p[i] > bv) { bv = p[i]; bi = lane + 64 * i; }
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    sel_i[r] = bi;
    sel_w[r] = bv;
    if (r < k) tot += bv;
    #pragma unroll
    for (int i = 0; i < PL; i++)
      if (bi == lane + 64 * i) p[i] = -1.f;
  }
  if (lane == 0) {
    #pragma unroll
    for (int r = 0; r < MOE_MAX_K; r++) {
      if (r < k) {
        idx[t * k + r] = sel_i[r];
        wts[t * k + r] = norm_topk ? sel_w[r] / tot : sel_w[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 2. gate/up + SwiGLU.  Workgroup (tile, e): 64 columns of expert e, 16 per
// wave, gate and up rows streamed as two streams over one x stage.  The whole
// K = H is reduced here, the x stage looping over K in MOE_KSLICE slices, so
// the activation runs on the fp32 sums and act is rounded to bf16 once.
// ---------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(MOE_NT, 2) void moe_gate_up_kernel(
    const bf16* __restrict__ h, const int* __restrict__ idx,
    const bf16* __restrict__ wg, const bf16* __restrict__ wu,
    bf16* __restrict__ act, int M, int H, int I, int k, long estride_g,
    long estride_u, int kslice) {
  const int e = blockIdx.y;
  const auto [lane, wv, i16, g] = mfma_lane();
  const int slot = moe_slot(idx, M, k, e, lane);
  if (__ballot(slot >= 0) == 0) return;  // idle expert: no weight load issued

  extern __shared__ __bf16 x_s[];  // [16][kslice] rows (zero-padded m >= M)
  const int n0 = blockIdx.x * SG_TN + wv * 16;
  MoeLane<2> ln;
  ln.wl[0] = (const char*)(wg + e * estride_g + (long)(n0 + i16) * H) + g * 16;
  ln.wl[1] = (const char*)(wu + e * estride_u + (long)(n0 + i16) * H) + g * 16;
  ln.x_s = x_s;

  f32x4 acc[2][4] = {};
  for (int k_lo = 0; k_lo < H; k_lo += kslice) {
    const int k_hi = min(H, k_lo + kslice);
    ln.xo = i16 * kslice + g * 8 - k_lo;
    bf16x8 xv[SG_XV];
    sg_x_load<MOE_NT>(xv, h, M, H, k_lo, k_hi, kslice);
    int4v b0[2][NB];
    // unconditional, as in sg_slice: the first block again when the slice
    // has no full batch (those registers are then not used)
    moe_ldw<2, NB, false>(b0, ln, k_lo, k_hi - k_lo >= NB * 32);
    if (k_lo > 0) __syncthreads();  // every wave is done with the last stage
    sg_x_store<MOE_NT>(x_s, xv, h, M, H, k_lo, k_hi, kslice);
    __syncthreads();
    moe_stream<2, NB, false>(acc, ln, b0, k_lo, k_hi);
  }

  #pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = g * 4 + r;
    const int j = __shfl(slot, m, 64);
    const float gs = acc[0][0][r] + acc[0][1][r] + acc[0][2][r] + acc[0][3][r];
    const float us = acc[1][0][r] + acc[1][1][r] + acc[1][2][r] + acc[1][3][r];
    const float a = gs / (1.f + __expf(-gs)) * us;
    if (j >= 0)  // j >= 0 implies m < M
      ((short*)act)[((long)j * M + m) * I + n0 + i16] = f2bf(a);
  }
}

// ---------------------------------------------------------------------------
// 3. down.  Workgroup (tile, e, s): 64 columns of expert e over K-slice s of
// I.  The x stage is gathered: row t is act[slot_t, t, slice] when token t
// chose e and zero otherwise (sg_x_load with a row pointer: a piece outside
// loads a valid address and is zeroed after, no branch around a load).  The
// routing weight multiplies the fp32 sum before the slab store, as the FP8
// row scale does.
// ---------------------------------------------------------------------------
template <int NT>
DEVINL void moe_x_gather(bf16x8 (&v)[SG_XV], const bf16* __restrict__ act,
                         int slot, int M, int I, int k_lo, int k_hi,
                         int kslice) {
  const int kn = k_hi - k_lo;
  const int dm = (NT * 8) / kslice, dk = (NT * 8) % kslice;
  int m = (threadIdx.x * 8) / kslice;
  int kk = (threadIdx.x * 8) % kslice;
  #pragma unroll
  for (int t = 0; t < SG_XV; t++) {
    const int j = __shfl(slot, m & 15, 64);  // wave-wide, before the select
    const bool ok = kk < kn && m < M && j >= 0;
    const bf16* p = ok ? act + ((long)j * M + m) * I + k_lo + kk : act;
    const bf16x8 r = *(const bf16x8*)p;
    v[t] = ok ? r : bf16x8{};
    m += dm;
    kk += dk;
    if (kk >= kslice) { kk -= kslice; m++; }
  }
}

template <int NB>
__global__ __launch_bounds__(MOE_NT, 4) void moe_down_kernel(
    const bf16* __restrict__ act, const int* __restrict__ idx,
    const float* __restrict__ wts, const bf16* __restrict__ wd,
    float* __restrict__ out32, int M, int H, int I, int k, long estride,
    int kslice) {
  const int e = blockIdx.y;
  const int ks = blockIdx.z;
  const auto [lane, wv, i16, g] = mfma_lane();
  const int slot = moe_slot(idx, M, k, e, lane);
  if (__ballot(slot >= 0) == 0) return;  // idle expert: no weight load issued

  extern __shared__ __bf16 x_s[];  // [16][kslice], kslice <= MOE_KSLICE
  const int k_lo = ks * kslice;
  const int k_hi = min(I, k_lo + kslice);
  const int n0 = blockIdx.x * SG_TN + wv * 16;
  MoeLane<1> ln;
  ln.wl[0] = (const char*)(wd + e * estride + (long)(n0 + i16) * I) + g * 16;
  ln.x_s = x_s;
  ln.xo = i16 * kslice + g * 8 - k_lo;

  // the lane's four output rows: slot and routing weight (first out)
  int js[4];
  float rw[4];
  #pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = g * 4 + r;
    js[r] = __shfl(slot, m, 64);
    rw[r] = wts[js[r] >= 0 ? m * k + js[r] : 0];
  }

  bf16x8 xv[SG_XV];
  moe_x_gather<MOE_NT>(xv, act, slot, M, I, k_lo, k_hi, kslice);
  int4v b0[1][NB];
  moe_ldw<1, NB, false>(b0, ln, k_lo, k_hi - k_lo >= NB * 32);
  #pragma unroll
  for (int t = 0; t < SG_XV; t++) {  // kslice <= NT * SG_XV / 2: no remainder
    const int i = (threadIdx.x + t * MOE_NT) * 8;
    if (i < 16 * kslice) *(bf16x8*)(&x_s[i]) = xv[t];
  }
  __syncthreads();
  f32x4 acc[1][4] = {};
  moe_stream<1, NB, false>(acc, ln, b0, k_lo, k_hi);

  #pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = g * 4 + r;
    const float vsum = acc[0][0][r] + acc[0][1][r] + acc[0][2][r] + acc[0][3][r];
    if (js[r] >= 0)  // slab (ks, slot) row m
      out32[(((long)ks * k + js[r]) * M + m) * H + n0 + i16] = vsum * rw[r];
  }
}

// ---------------------------------------------------------------------------
// 4. FP8 (e4m3) expert weights.  The stacks are codes q [E, N, K], one byte
// per element, with one fp32 scale per row, scale [E, N] (quantize_fp8.hip).
// Routing, x stage, slabs and the one-writer rule are the bf16 kernels'; the
// lanes stream 16 codes per load (MoeLane<NS, true>) and the row scale
// multiplies the fp32 sum once, in the epilogue: gate and up before SwiGLU,
// down together with the routing weight.  The scale loads go out before the
// stream, after the idle-expert return: an idle expert's codes and scales are
// never read.
//
// Load plan of gate/up.  A 1024-element x stage now holds 16 loads per lane
// and stream instead of 32, so the slice boundary of the bf16 kernel
// (barrier, x load, x store, barrier, with the W pipeline drained) weighs
// twice as much per byte.  This kernel double-buffers two 1024 stages (64
// KiB, two workgroups per CU still fit): a full slice is MOE_KSLICE /
// (NB * 64) batches, and before the MFMAs of its last batch the next slice's
// x loads and first W batch are issued; x is stored to the other stage behind
// those MFMAs and ONE barrier follows (the other stage was last read in the
// previous slice, which every wave left through that slice's barrier).  The
// W stream never drains between slices.  The last slice (any length) is
// moe_stream.  Measured against the bf16 kernel's loop over codes and against
// one 2048 stage: docs/kernels.md "MoE decode, FP8 experts".
// ---------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(MOE_NT, 2) void moe_gate_up_fp8_kernel(
    const bf16* __restrict__ h, const int* __restrict__ idx,
    const unsigned char* __restrict__ qg, const float* __restrict__ sg,
    const unsigned char* __restrict__ qu, const float* __restrict__ su,
    bf16* __restrict__ act, int M, int H, int I, int k, long estride_g,
    long estride_u, int kslice) {
  const int e = blockIdx.y;
  const auto [lane, wv, i16, g] = mfma_lane();
  const int slot = moe_slot(idx, M, k, e, lane);
  if (__ballot(slot >= 0) == 0) return;  // idle expert: no weight load issued

  extern __shared__ __bf16 x_s[];  // [16][kslice], twice when H > kslice
  const int n0 = blockIdx.x * SG_TN + wv * 16;
  const float scg = sg[(long)e * I + n0 + i16];  // first out
  const float scu = su[(long)e * I + n0 + i16];
  MoeLane<2, true> ln;
  ln.wl[0] = (const char*)(qg + e * estride_g + (long)(n0 + i16) * H) + g * 16;
  ln.wl[1] = (const char*)(qu + e * estride_u + (long)(n0 + i16) * H) + g * 16;
  ln.x_s = x_s;

  constexpr int S = NB * 64;
  f32x4 acc[2][4] = {};
  // kslice == MOE_KSLICE whenever a second slice exists (host side)
  static_assert(MOE_KSLICE % (2 * S) == 0, "a full slice is batch pairs");
  bf16x8 xv[SG_XV];
  int4v b0[2][NB], b1[2][NB];
  sg_x_load<MOE_NT>(xv, h, M, H, 0, min(H, kslice), kslice);
  moe_ldw<2, NB, true>(b0, ln, 0, min(H, kslice) >= S);
  sg_x_store<MOE_NT>(x_s, xv, h, M, H, 0, min(H, kslice), kslice);
  __syncthreads();
  int st = 0;
  int k_lo = 0;
  for (; k_lo + kslice < H; k_lo += kslice, st ^= 1) {  // full, not the last
    ln.x_s = x_s + st * 16 * kslice;
    ln.xo = i16 * kslice + g * 16 - k_lo;
    const int n_lo = k_lo + kslice, n_hi = min(H, n_lo + kslice);
    #pragma unroll
    for (int kk = 0; kk < MOE_KSLICE; kk += 2 * S) {
      moe_ldw<2, NB, true>(b1, ln, k_lo + kk + S);
      moe_mma<2, NB, true>(acc, ln, b0, k_lo + kk);
      if (kk + 2 * S < MOE_KSLICE) {
        moe_ldw<2, NB, true>(b0, ln, k_lo + kk + 2 * S);
      } else {  // the next slice's x and first batch, behind b1's loads
        sg_x_load<MOE_NT>(xv, h, M, H, n_lo, n_hi, kslice);
        moe_ldw<2, NB, true>(b0, ln, n_lo, n_hi - n_lo >= S);
      }
      moe_mma<2, NB, true>(acc, ln, b1, k_lo + kk + S);
    }
    sg_x_store<MOE_NT>(x_s + (st ^ 1) * 16 * kslice, xv, h, M, H, n_lo, n_hi,
                       kslice);
    __syncthreads();
  }
  ln.x_s = x_s + st * 16 * kslice;
  ln.xo = i16 * kslice + g * 16 - k_lo;
  moe_stream<2, NB, true>(acc, ln, b0, k_lo, H);

  #pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = g * 4 + r;
    const int j = __shfl(slot, m, 64);
    const float gs =
        (acc[0][0][r] + acc[0][1][r] + acc[0][2][r] + acc[0][3][r]) * scg;
    const float us =
        (acc[1][0][r] + acc[1][1][r] + acc[1][2][r] + acc[1][3][r]) * scu;
    const float a = gs / (1.f + __expf(-gs)) * us;
    if (j >= 0)  // j >= 0 implies m < M
      ((short*)act)[((long)j * M + m) * I + n0 + i16] = f2bf(a);
  }
}

// the bf16 down kernel over codes: gathered x stage, one K-slice per workgroup
template <int NB>
__global__ __launch_bounds__(MOE_NT, 4) void moe_down_fp8_kernel(
    const bf16* __restrict__ act, const int* __restrict__ idx,
    const float* __restrict__ wts, const unsigned char* __restrict__ qd,
    const float* __restrict__ sd, float* __restrict__ out32, int M, int H,
    int I, int k, long estride, int kslice) {
  const int e = blockIdx.y;
  const int ks = blockIdx.z;
  const auto [lane, wv, i16, g] = mfma_lane();
  const int slot = moe_slot(idx, M, k, e, lane);
  if (__ballot(slot >= 0) == 0) return;  // idle expert: no weight load issued

  extern __shared__ __bf16 x_s[];  // [16][kslice], kslice <= MOE_KSLICE
  const int k_lo = ks * kslice;
  const int k_hi = min(I, k_lo + kslice);
  const int n0 = blockIdx.x * SG_TN + wv * 16;
  const float sc = sd[(long)e * H + n0 + i16];  // first out
  MoeLane<1, true> ln;
  ln.wl[0] = (const char*)(qd + e * estride + (long)(n0 + i16) * I) + g * 16;
  ln.x_s = x_s;
  ln.xo = i16 * kslice + g * 16 - k_lo;

  // the lane's four output rows: slot and routing weight
  int js[4];
  float rw[4];
  #pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = g * 4 + r;
    js[r] = __shfl(slot, m, 64);
    rw[r] = wts[js[r] >= 0 ? m * k + js[r] : 0];
  }

  bf16x8 xv[SG_XV];
  moe_x_gather<MOE_NT>(xv, act, slot, M, I, k_lo, k_hi, kslice);
  int4v b0[1][NB];
  moe_ldw<1, NB, true>(b0, ln, k_lo, k_hi - k_lo >= NB * 64);
  #pragma unroll
  for (int t = 0; t < SG_XV; t++) {  // kslice <= NT * SG_XV / 2: no remainder
    const int i = (threadIdx.x + t * MOE_NT) * 8;
    if (i < 16 * kslice) *(bf16x8*)(&x_s[i]) = xv[t];
  }
  __syncthreads();
  f32x4 acc[1][4] = {};
  moe_stream<1, NB, true>(acc, ln, b0, k_lo, k_hi);

  #pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = g * 4 + r;
    const float vsum = acc[0][0][r] + acc[0][1][r] + acc[0][2][r] + acc[0][3][r];
    if (js[r] >= 0)  // slab (ks, slot) row m
      out32[(((long)ks * k + js[r]) * M + m) * H + n0 + i16] =
          vsum * sc * rw[r];
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static void moe_check_idx(const torch::Tensor& idx, long M) {
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt32 &&
              idx.dim() == 2 && idx.is_contiguous() && idx.size(0) == M &&
              idx.size(1) >= 1 && idx.size(1) <= MOE_MAX_K,
              "idx must be contiguous int32 [M, k], k <= 8");
}

// x [M, K] contiguous bf16, M <= 16, K % 64 == 0
static void moe_check_rows(const torch::Tensor& x, const char* what) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16 &&
              x.dim() == 2 && x.is_contiguous() && x.size(0) >= 1 &&
              x.size(0) <= 16 && x.size(1) % 64 == 0 &&
              (uintptr_t)x.data_ptr() % 16 == 0,
              what, " must be contiguous, 16-byte aligned bf16 [M <= 16, K % 64 == 0]");
}

// w [E, N, K] bf16 expert stack: rows contiguous, any expert stride that keeps
// 16-byte alignment; returns the expert stride in elements
static long moe_check_stack(const torch::Tensor& w, long E, long N, long K,
                            const char* what) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 &&
              w.dim() == 3 && w.size(0) == E && w.size(1) == N &&
              w.size(2) == K && w.stride(2) == 1 && w.stride(1) == K &&
              w.stride(0) % 8 == 0 && (uintptr_t)w.data_ptr() % 16 == 0 &&
              N % SG_TN == 0 && K % 64 == 0,
              what, " must be a 16-byte aligned bf16 [E, N % 64 == 0, K % 64 == 0] "
              "stack of contiguous rows");
  return w.stride(0);
}

std::vector<torch::Tensor> moe_route_decode(torch::Tensor h,
                                            torch::Tensor router_w, long top_k,
                                            bool norm_topk) {
  moe_check_rows(h, "h");
  const long M = h.size(0), H = h.size(1), E = router_w.size(0);
  TORCH_CHECK(router_w.is_cuda() && router_w.scalar_type() == torch::kBFloat16 &&
              router_w.dim() == 2 && router_w.is_contiguous() &&
              router_w.size(1) == H && (uintptr_t)router_w.data_ptr() % 16 == 0,
              "router_w must be contiguous, 16-byte aligned bf16 [E, H]");
  TORCH_CHECK(E <= MOE_MAX_E && top_k >= 1 && top_k <= MOE_MAX_K && top_k <= E,
              "moe_route_decode takes E <= 256 and top_k <= min(8, E)");
  auto idx = torch::empty({M, top_k}, h.options().dtype(torch::kInt32));
  auto wts = torch::empty({M, top_k}, h.options().dtype(torch::kFloat32));
  const size_t lds = (size_t)(H + MOE_MAX_E) * sizeof(float);
  TORCH_CHECK(lds <= 64 * 1024, "hidden size too large for the router stage");
  hipLaunchKernelGGL(moe_route_kernel, dim3(M), dim3(MOE_ROUTE_NT), lds,
    cur_stream(), (const bf16*)h.data_ptr(), (const bf16*)router_w.data_ptr(),
    idx.data_ptr<int>(), wts.data_ptr<float>(), (int)H, (int)E, (int)top_k,
    (int)norm_topk);
  CHECK_CUDA_OK();
  return {idx, wts};
}

// out: caller-owned [k, M, I] bf16 to write into (rows are written once each,
// nothing is cleared)
torch::Tensor moe_gate_up_swiglu(torch::Tensor h, torch::Tensor idx,
                                 torch::Tensor wg, torch::Tensor wu,
                                 c10::optional<torch::Tensor> out) {
  moe_check_rows(h, "h");
  const long M = h.size(0), H = h.size(1);
  moe_check_idx(idx, M);
  const long k = idx.size(1), E = wg.size(0), I = wg.size(1);
  const long sg = moe_check_stack(wg, E, I, H, "wg");
  const long su = moe_check_stack(wu, E, I, H, "wu");
  TORCH_CHECK(E <= MOE_MAX_E, "at most 256 experts");
  auto act = out.has_value() ? *out : torch::empty({k, M, I}, h.options());
  TORCH_CHECK(act.is_cuda() && act.scalar_type() == torch::kBFloat16 &&
              act.is_contiguous() && act.numel() == k * M * I,
              "out must be contiguous bf16 [k, M, I]");
  const int kslice = (int)std::min<long>(H, MOE_KSLICE);
  hipLaunchKernelGGL((moe_gate_up_kernel<4>), dim3(I / SG_TN, E), dim3(MOE_NT),
    (size_t)16 * kslice * sizeof(short), cur_stream(),
    (const bf16*)h.data_ptr(), idx.data_ptr<int>(), (const bf16*)wg.data_ptr(),
    (const bf16*)wu.data_ptr(), (bf16*)act.data_ptr(), (int)M, (int)H, (int)I,
    (int)k, sg, su, kslice);
  CHECK_CUDA_OK();
  return act.view({k, M, I});
}

// act [k, M, I] bf16; wts [M, k] fp32; out32_ws fp32 >= nks * k * M * H.
// Returns the [nks * k, M, H] slab view of the workspace.
torch::Tensor moe_down(torch::Tensor act, torch::Tensor idx, torch::Tensor wts,
                       torch::Tensor wd, torch::Tensor out32_ws, long splitk) {
  TORCH_CHECK(act.is_cuda() && act.scalar_type() == torch::kBFloat16 &&
              act.dim() == 3 && act.is_contiguous() &&
              (uintptr_t)act.data_ptr() % 16 == 0 && act.size(1) >= 1 &&
              act.size(1) <= 16,
              "act must be contiguous, 16-byte aligned bf16 [k, M <= 16, I]");
  const long k = act.size(0), M = act.size(1), I = act.size(2);
  moe_check_idx(idx, M);
  TORCH_CHECK(idx.size(1) == k, "act / idx top-k mismatch");
  TORCH_CHECK(wts.is_cuda() && wts.scalar_type() == torch::kFloat32 &&
              wts.is_contiguous() && wts.dim() == 2 && wts.size(0) == M &&
              wts.size(1) == k, "wts must be contiguous fp32 [M, k]");
  const long E = wd.size(0), H = wd.size(1);
  const long sd = moe_check_stack(wd, E, H, I, "wd");
  TORCH_CHECK(E <= MOE_MAX_E, "at most 256 experts");
  TORCH_CHECK(splitk >= 1);
  const int kslice = (int)((I / splitk + 63) / 64 * 64);
  const int nks = (int)((I + kslice - 1) / kslice);
  TORCH_CHECK(kslice <= MOE_KSLICE, "splitk too small: a K slice of ", kslice,
              " exceeds the ", MOE_KSLICE, "-element x stage");
  TORCH_CHECK(out32_ws.is_cuda() && out32_ws.scalar_type() == torch::kFloat32 &&
              out32_ws.is_contiguous() &&
              out32_ws.numel() >= (long)nks * k * M * H, "workspace too small");
  hipLaunchKernelGGL((moe_down_kernel<4>), dim3(H / SG_TN, E, nks),
    dim3(MOE_NT), (size_t)16 * kslice * sizeof(short), cur_stream(),
    (const bf16*)act.data_ptr(), idx.data_ptr<int>(), wts.data_ptr<float>(),
    (const bf16*)wd.data_ptr(), out32_ws.data_ptr<float>(), (int)M, (int)H,
    (int)I, (int)k, sd, kslice);
  CHECK_CUDA_OK();
  return out32_ws.flatten().narrow(0, 0, (long)nks * k * M * H)
      .view({(long)nks * k, M, H});
}

// q [E, N, K] e4m3 codes (one byte per element), rows contiguous, any expert
// stride that is a multiple of 16; scale fp32 [E, N] contiguous.  Returns the
// expert stride in bytes.
static long moe_check_stack_fp8(const torch::Tensor& q,
                                const torch::Tensor& scale, long E, long N,
                                long K, const char* what) {
  TORCH_CHECK(q.is_cuda() && q.element_size() == 1 && q.dim() == 3 &&
              q.size(0) == E && q.size(1) == N && q.size(2) == K &&
              q.stride(2) == 1 && q.stride(1) == K && q.stride(0) % 16 == 0 &&
              q.stride(0) >= N * K && (uintptr_t)q.data_ptr() % 16 == 0 &&
              N % SG_TN == 0 && K % 64 == 0,
              what, " codes must be a 16-byte aligned one-byte [E, N % 64 == 0, "
              "K % 64 == 0] stack of contiguous rows, expert stride % 16 == 0");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat32 &&
              scale.dim() == 2 && scale.is_contiguous() &&
              scale.size(0) == E && scale.size(1) == N,
              what, " scale must be contiguous fp32 [E, N]");
  return q.stride(0);
}

torch::Tensor moe_gate_up_swiglu_fp8(torch::Tensor h, torch::Tensor idx,
                                     torch::Tensor qg, torch::Tensor sg,
                                     torch::Tensor qu, torch::Tensor su,
                                     c10::optional<torch::Tensor> out) {
  moe_check_rows(h, "h");
  const long M = h.size(0), H = h.size(1);
  moe_check_idx(idx, M);
  TORCH_CHECK(qg.dim() == 3, "qg must be [E, I, H]");
  const long k = idx.size(1), E = qg.size(0), I = qg.size(1);
  const long eg = moe_check_stack_fp8(qg, sg, E, I, H, "gate");
  const long eu = moe_check_stack_fp8(qu, su, E, I, H, "up");
  TORCH_CHECK(E <= MOE_MAX_E, "at most 256 experts");
  auto act = out.has_value() ? *out : torch::empty({k, M, I}, h.options());
  TORCH_CHECK(act.is_cuda() && act.scalar_type() == torch::kBFloat16 &&
              act.is_contiguous() && act.numel() == k * M * I,
              "out must be contiguous bf16 [k, M, I]");
  const int kslice = (int)std::min<long>(H, MOE_KSLICE);
  const int stages = H > kslice ? 2 : 1;  // double-buffered past one slice
  hipLaunchKernelGGL((moe_gate_up_fp8_kernel<4>), dim3(I / SG_TN, E),
    dim3(MOE_NT), (size_t)stages * 16 * kslice * sizeof(short), cur_stream(),
    (const bf16*)h.data_ptr(), idx.data_ptr<int>(),
    (const unsigned char*)qg.data_ptr(), sg.data_ptr<float>(),
    (const unsigned char*)qu.data_ptr(), su.data_ptr<float>(),
    (bf16*)act.data_ptr(), (int)M, (int)H, (int)I, (int)k, eg, eu, kslice);
  CHECK_CUDA_OK();
  return act.view({k, M, I});
}

torch::Tensor moe_down_fp8(torch::Tensor act, torch::Tensor idx,
                           torch::Tensor wts, torch::Tensor qd,
                           torch::Tensor sd, torch::Tensor out32_ws,
                           long splitk) {
  TORCH_CHECK(act.is_cuda() && act.scalar_type() == torch::kBFloat16 &&
              act.dim() == 3 && act.is_contiguous() &&
              (uintptr_t)act.data_ptr() % 16 == 0 && act.size(1) >= 1 &&
              act.size(1) <= 16,
              "act must be contiguous, 16-byte aligned bf16 [k, M <= 16, I]");
  const long k = act.size(0), M = act.size(1), I = act.size(2);
  moe_check_idx(idx, M);
  TORCH_CHECK(idx.size(1) == k, "act / idx top-k mismatch");
  TORCH_CHECK(wts.is_cuda() && wts.scalar_type() == torch::kFloat32 &&
              wts.is_contiguous() && wts.dim() == 2 && wts.size(0) == M &&
              wts.size(1) == k, "wts must be contiguous fp32 [M, k]");
  TORCH_CHECK(qd.dim() == 3, "qd must be [E, H, I]");
  const long E = qd.size(0), H = qd.size(1);
  const long ed = moe_check_stack_fp8(qd, sd, E, H, I, "down");
  TORCH_CHECK(E <= MOE_MAX_E, "at most 256 experts");
  TORCH_CHECK(splitk >= 1);
  const int kslice = (int)((I / splitk + 63) / 64 * 64);
  const int nks = (int)((I + kslice - 1) / kslice);
  TORCH_CHECK(kslice <= MOE_KSLICE, "splitk too small: a K slice of ", kslice,
              " exceeds the ", MOE_KSLICE, "-element x stage");
  TORCH_CHECK(out32_ws.is_cuda() && out32_ws.scalar_type() == torch::kFloat32 &&
              out32_ws.is_contiguous() &&
              out32_ws.numel() >= (long)nks * k * M * H, "workspace too small");
  hipLaunchKernelGGL((moe_down_fp8_kernel<4>), dim3(H / SG_TN, E, nks),
    dim3(MOE_NT), (size_t)16 * kslice * sizeof(short), cur_stream(),
    (const bf16*)act.data_ptr(), idx.data_ptr<int>(), wts.data_ptr<float>(),
    (const unsigned char*)qd.data_ptr(), sd.data_ptr<float>(),
    out32_ws.data_ptr<float>(), (int)M, (int)H, (int)I, (int)k, ed, kslice);
  CHECK_CUDA_OK();
  return out32_ws.flatten().narrow(0, 0, (long)nks * k * M * H)
      .view({(long)nks * k, M, H});
}

// bf16 [M, H] = sum of the slabs in order (+ residual), one rounding
torch::Tensor moe_combine(torch::Tensor slabs, torch::Tensor like,
                          c10::optional<torch::Tensor> residual) {
  return sg_combine_slabs(slabs, like, residual);
}
