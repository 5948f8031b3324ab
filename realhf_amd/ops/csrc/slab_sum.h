// Sum of the skinny GEMM's fp32 split-K partial slabs, shared by every slab
// consumer (sg_combine_kernel, the slab add+rmsnorm, swiglu/geglu_slab,
// rope_qkv_decode<SLAB>).
//
// A thread owns NV float4 vectors; vector v of slab s is at p[v] + s*sstride.
// The loads of up to SLAB_BATCH slabs (all NV vectors of each) are issued
// before the first add, so a batch costs one memory round trip where a
// load-add loop over a run-time nks costs one per slab.  The adds stay in
// slab order (0, +1, +2, ...): the result is bit for bit what the sequential
// loop gives.  A batch is never padded with zero slabs (-0 + 0 is +0): the
// nks % SLAB_BATCH remainder runs its own exact-size batch.
//
// A caller that wants other loads (residual, bias, weight) in flight with the
// first batch issues them before the call and uses them after it.
#pragma once
#include "common.h"

#define SLAB_BATCH 8

// NB slabs from s0 on: NB*NV loads, then NB*NV adds; FIRST: acc starts as
// slab s0 instead of being added to
template <int NB, int NV, bool FIRST>
DEVINL void slab_batch(float4v (&acc)[NV], const float* const (&p)[NV],
                       long sstride, int s0) {
  float4v b[NB][NV];
  #pragma unroll
  for (int t = 0; t < NB; t++) {
    #pragma unroll
    for (int v = 0; v < NV; v++)
      b[t][v] = *(const float4v*)(p[v] + (long)(s0 + t) * sstride);
  }
  #pragma unroll
  for (int t = 0; t < NB; t++) {
    #pragma unroll
    for (int v = 0; v < NV; v++) {
      if (FIRST && t == 0) acc[v] = b[0][v];
      else acc[v] += b[t][v];
    }
  }
}

// a batch of n slabs, 1 <= n < MAXB (n is uniform: one scalar branch)
template <int MAXB, int NV, bool FIRST>
DEVINL void slab_rem(float4v (&acc)[NV], const float* const (&p)[NV],
                     long sstride, int s0, int n) {
  static_assert(MAXB <= 8, "slab_rem lists batches of up to 7");
  switch (n) {
    case 1: slab_batch<1, NV, FIRST>(acc, p, sstride, s0); break;
    case 2: slab_batch<2, NV, FIRST>(acc, p, sstride, s0); break;
    case 3: slab_batch<3, NV, FIRST>(acc, p, sstride, s0); break;
    case 4: if constexpr (MAXB > 4) slab_batch<4, NV, FIRST>(acc, p, sstride, s0); break;
    case 5: if constexpr (MAXB > 4) slab_batch<5, NV, FIRST>(acc, p, sstride, s0); break;
    case 6: if constexpr (MAXB > 4) slab_batch<6, NV, FIRST>(acc, p, sstride, s0); break;
    case 7: if constexpr (MAXB > 4) slab_batch<7, NV, FIRST>(acc, p, sstride, s0); break;
  }
}

// acc[v] = slab 0 + slab 1 + ... + slab nks-1 of vector v, nks >= 1.
// MAXB (4 or 8) is the batch depth: MAXB*NV float4 are live at once.
template <int NV, int MAXB = SLAB_BATCH>
DEVINL void slab_sum(float4v (&acc)[NV], const float* const (&p)[NV],
                     long sstride, int nks) {
  static_assert(MAXB == 4 || MAXB == 8, "batch depth 4 or 8");
  if (nks < MAXB) {
    slab_rem<MAXB, NV, true>(acc, p, sstride, 0, nks);
    return;
  }
  slab_batch<MAXB, NV, true>(acc, p, sstride, 0);
  int s = MAXB;
  for (; s + MAXB <= nks; s += MAXB)
    slab_batch<MAXB, NV, false>(acc, p, sstride, s);
  if (s < nks) slab_rem<MAXB, NV, false>(acc, p, sstride, s, nks - s);
}
