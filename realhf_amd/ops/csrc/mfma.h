// Building blocks shared by every v_mfma_f32_16x16x32_bf16 kernel:
// vector types, the lane map, fragment reads and the packed-varlen block
// mapping.  mfma_probe / tr16_probe (attn_varlen.hip) are written on top
// of these helpers, so the on-device probes check the code the kernels use.
//
// Lane map of D(16x16) += A(16x32) B(32x16), lane = threadIdx.x & 63,
// i16 = lane & 15, g = lane >> 4 (the ONE place it is written down):
//   A[i][k]:   i = i16, k = g*8 + j   (j = 0..7, one bf16x8)
//   B[k][n]:   n = i16, k = g*8 + j
//   C/D[i][n]: n = i16, i = g*4 + r   (r = 0..3, one f32x4)
// A and B share their lane geometry, so a row-major LDS tile whose rows are
// the i (or n) index and whose columns are k gives either fragment as one
// 16-byte read at tile[i16][g*8].
//
// tr16 hardware-transpose read (ds_read_b64_tr_b16), for tiles whose ROWS
// are k: within each 16-lane group, result lane c elem j is source lane
// (4j + c/4)'s element (c%4).  So lane i16 reading the 8-byte chunk at
// tile[kbase + g*8 + (i16>>2) (+4)][nbase + (i16&3)*4] leaves the group
// holding the fragment with k = LDS row, n (or i) = LDS column; tr16_bfrag
// takes krow0 = kbase + g*8 + (i16>>2) and col4 = nbase + (i16&3)*4.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"

using f32x4 = float4v;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((address_space(3))) bf16x4 lds_b64_t;

// use as: const auto [lane, wave, i16, g] = mfma_lane();
struct MfmaLane { int lane, wave, i16, g; };
DEVINL MfmaLane mfma_lane() {
  const int lane = threadIdx.x & 63;
  return {lane, (int)(threadIdx.x >> 6), lane & 15, lane >> 4};
}

DEVINL f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

DEVINL bf16x4 tr16_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64_t*)p);
}

DEVINL bf16x8 tr16_bfrag(const __bf16* base, int pitch, int krow0, int col4) {
  // two transpose reads -> one 8-deep fragment (k = rows, n = cols)
  bf16x4 r0 = tr16_read(base + (long)krow0 * pitch + col4);
  bf16x4 r1 = tr16_read(base + (long)(krow0 + 4) * pitch + col4);
  bf16x8 vb;
  #pragma unroll
  for (int j = 0; j < 4; j++) { vb[j] = r0[j]; vb[4 + j] = r1[j]; }
  return vb;
}

// reductions over the 16 lanes that share lane>>4 (one C/D row)
DEVINL float group16_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 1, 64));
  x = fmaxf(x, __shfl_xor(x, 2, 64));
  x = fmaxf(x, __shfl_xor(x, 4, 64));
  x = fmaxf(x, __shfl_xor(x, 8, 64));
  return x;
}
DEVINL float group16_sum(float x) {
  x += __shfl_xor(x, 1, 64);
  x += __shfl_xor(x, 2, 64);
  x += __shfl_xor(x, 4, 64);
  x += __shfl_xor(x, 8, 64);
  return x;
}

// ---------------------------------------------------------------------------
// Packed-varlen block mapping: blk_offsets[i] = sum_{j<i} ceil(L_j / BLK).
// Built by a tiny kernel each call so the host NEVER reads cu_seqlens (a
// host-built block list cost one DtoH sync per layer call in training).
// Workgroups past the real block count blk_offsets[bs] exit immediately;
// the grid is the cheap upper bound total/BLK + bs.
// ---------------------------------------------------------------------------
template <int BLK>  // a template so only the files that launch it emit it
static __global__ void build_blk_offsets_kernel(const int* __restrict__ cu,
                                                int bs, int* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < bs; i++) {
      out[i] = acc;
      int L = cu[i + 1] - cu[i];
      acc += (L + BLK - 1) / BLK;
    }
    out[bs] = acc;
  }
}

DEVINL int blk_lookup(const int* __restrict__ off, int bs, int blk_id) {
  int lo = 0, hi = bs;  // largest i with off[i] <= blk_id
  while (lo + 1 < hi) {
    int mid = (lo + hi) >> 1;
    if (off[mid] <= blk_id) lo = mid; else hi = mid;
  }
  return lo;
}

// cu_dev: int32 cu_seqlens on the device; returns the [bs + 1] offsets
template <int BLK>
static torch::Tensor build_blk_offsets(const torch::Tensor& cu_dev) {
  const int bs = cu_dev.numel() - 1;
  auto blk_off = torch::empty({(long)bs + 1}, cu_dev.options());
  hipLaunchKernelGGL(build_blk_offsets_kernel<BLK>, dim3(1), dim3(64), 0,
    cur_stream(), cu_dev.data_ptr<int>(), bs, blk_off.data_ptr<int>());
  return blk_off;
}
