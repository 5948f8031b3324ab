// Per-row e4m3 weight quantizer for FP8 weight-only decode (gfx950, OCP
// e4m3fn).  For each row n of w [N, K] (bf16, row stride arbitrary):
//   amax     = max_k |float(w[n, k])|
//   scale[n] = amax / 448 in fp32, or 1 when amax == 0
//   q[n, k]  = rne_e4m3(float(w[n, k]) / scale[n]), clamped to +-448
// The scale, the correctly rounded division, the clamp and the conversion
// are fp8_e4m3.h's, shared with the FP8 KV cache writers: the result is bit
// for bit what quantize_rows_e4m3_ref computes on the CPU.  Rows with
// non-finite weights get no special handling.
//
// Shape follows rmsnorm.hip: one 256-thread workgroup per row, 16-byte
// loads, the row read twice (amax pass, quantize pass; the second read hits
// L2), wave reductions through LDS in a fixed order, no atomics.
#include "common.h"
#include "fp8_e4m3.h"

#define QF8_THREADS 256

// VEC = 8: 16-byte loads, 8-byte stores; VEC = 1: rows that are not
// 16-byte aligned or K % 8 != 0
template <int VEC>
__global__ __launch_bounds__(QF8_THREADS) void quantize_rows_e4m3_kernel(
    const bf16* __restrict__ w, long wstride, unsigned char* __restrict__ q,
    float* __restrict__ scale, int K) {
  __shared__ float red[QF8_THREADS / WAVE];
  const long row = blockIdx.x;
  const short* wr = (const short*)w + row * wstride;
  unsigned char* qr = q + row * K;

  float amax = 0.f;
  for (int i = threadIdx.x * VEC; i < K; i += QF8_THREADS * VEC) {
    short v[VEC];
    if constexpr (VEC == 8) *(short8*)v = *(const short8*)(wr + i);
    else v[0] = wr[i];
    #pragma unroll
    for (int j = 0; j < VEC; j++) amax = fmaxf(amax, fabsf(bf2f(v[j])));
  }
  amax = wave_max(amax);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float s = e4m3_row_scale(amax);
  if (threadIdx.x == 0) scale[row] = s;

  for (int i = threadIdx.x * VEC; i < K; i += QF8_THREADS * VEC) {
    short v[VEC];
    if constexpr (VEC == 8) *(short8*)v = *(const short8*)(wr + i);
    else v[0] = wr[i];
    float f[VEC];
    #pragma unroll
    for (int j = 0; j < VEC; j++)
      f[j] = e4m3_scaled(bf2f(v[j]), s);
    if constexpr (VEC == 8) {
      int2 o = {e4m3_pack4(f[0], f[1], f[2], f[3]),
                e4m3_pack4(f[4], f[5], f[6], f[7])};
      *(int2*)(qr + i) = o;
    } else {
      qr[i] = (unsigned char)(
          __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[0], 0, false) & 0xff);
    }
  }
}

// in-place form: q [N, K] (one byte per element, contiguous) and scale
// fp32 [N] are caller-owned, so their addresses survive a captured graph
void quantize_rows_e4m3_(torch::Tensor w, torch::Tensor q, torch::Tensor scale) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 &&
              w.dim() == 2 && w.stride(1) == 1,
              "w must be bf16 [N, K] with stride(1) == 1");
  const long N = w.size(0), K = w.size(1);
  TORCH_CHECK(q.is_cuda() && q.element_size() == 1 && q.dim() == 2 &&
              q.size(0) == N && q.size(1) == K && q.is_contiguous(),
              "q must be contiguous [N, K] with one byte per element");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat32 &&
              scale.is_contiguous() && scale.numel() == N,
              "scale must be contiguous fp32 [N]");
  TORCH_CHECK(K < (1L << 31) && N < (1L << 31));
  if (N == 0 || K == 0) return;
  const long wstride = N > 1 ? w.stride(0) : K;
  const bool vec = K % 8 == 0 && wstride % 8 == 0 &&
                   (uintptr_t)w.data_ptr() % 16 == 0 &&
                   (uintptr_t)q.data_ptr() % 8 == 0;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)N), dim3(QF8_THREADS), 0,
      cur_stream(), (const bf16*)w.data_ptr(), wstride,
      (unsigned char*)q.data_ptr(), scale.data_ptr<float>(), (int)K);
  };
  if (vec) launch(quantize_rows_e4m3_kernel<8>);
  else launch(quantize_rows_e4m3_kernel<1>);
  CHECK_CUDA_OK();
}

std::vector<torch::Tensor> quantize_rows_e4m3(torch::Tensor w) {
  TORCH_CHECK(w.dim() == 2);
  auto q = torch::empty({w.size(0), w.size(1)},
                        w.options().dtype(at::kFloat8_e4m3fn));
  auto scale = torch::empty({w.size(0)}, w.options().dtype(torch::kFloat32));
  quantize_rows_e4m3_(w, q, scale);
  return {q, scale};
}
