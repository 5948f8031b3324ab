// OCP e4m3fn row quantization and decode, shared by the weight quantizer
// (quantize_fp8.hip), the FP8 KV cache writers (rope_decode.hip,
// kv_store_fp8.hip) and its reader (attn_decode.hip).
//
// One definition for every writer: scale = amax / 448 in fp32 (1 for an
// all-zero row), code = rne_e4m3(x / scale) clamped to +-448.  The division
// is a true fp32 division (hipcc's default is the correctly rounded one) and
// v_cvt_pk_fp8_f32 rounds to nearest even, so every writer is bit for bit
// quantize_rows_e4m3_ref.  The clamp keeps finite inputs off the NaN codes
// 0x7f / 0xff.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(2))) float float2v;

DEVINL float e4m3_row_scale(float amax) {
  return amax == 0.f ? 1.f : amax / 448.f;
}

DEVINL float e4m3_scaled(float x, float s) {
  return fminf(fmaxf(x / s, -448.f), 448.f);
}

// four already scaled and clamped floats -> four codes, f0 in the low byte
DEVINL int e4m3_pack4(float f0, float f1, float f2, float f3) {
  int u = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, u, true);
}

// amax over the G consecutive lanes of an aligned group (G a power of two,
// at most 64): every lane of the group must be active
template <int G>
DEVINL float group_max(float x) {
  #pragma unroll
  for (int off = 1; off < G; off <<= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}

// sum over the same group, same condition (the per-head QK RMSNorm's sum of
// squares); every lane of the group gets the same bits: the butterfly adds
// the same pairs in every lane
template <int G>
DEVINL float group_sum(float x) {
  #pragma unroll
  for (int off = 1; off < G; off <<= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// Decode.  e4m3 -> f32 by v_cvt_pk_f32_fp8 is exact (subnormals included);
// the upper 16 bits of that f32 are the same value as a bf16, exactly: an
// e4m3 value has 3 mantissa bits and bf16 keeps 7.
DEVINL unsigned bf16_pair_of(float lo, float hi) {
  return (__builtin_bit_cast(unsigned, lo) >> 16) |
         (__builtin_bit_cast(unsigned, hi) & 0xffff0000u);
}
