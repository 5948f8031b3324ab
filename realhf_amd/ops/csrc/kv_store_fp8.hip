// Quantizing prefill store for the FP8 KV cache (gfx950, OCP e4m3fn).
// Takes the packed prefill K and V [total, nkv, hd] (bf16, views into the
// QKV projection: any token stride) and writes each head row into the
// session cache at (sequence, position): codes [bs, maxlen, nkv, hd] and
// one fp32 scale per row in [bs, nkv, maxlen].  One kernel instead of
// bucketize + two index_put; the quantization is fp8_e4m3.h's, so a row is
// bit for bit quantize_rows_e4m3_ref of the bf16 row.
//
// Work item = 8 elements of one (token, k|v, head) row: a 16-byte load, an
// 8-byte store.  The hd/8 consecutive items of a row (8, 16 or 32 lanes,
// always inside one wave and in or out of the grid-stride loop together:
// 256-thread blocks, nwork a multiple of hd/8) take the row amax by
// shfl_xor.  The sequence of token t is the number of cu_seqlens[1:] entries
// <= t (what torch.bucketize(right=True) gives), found by bisection; the
// position is positions[t].  Rows that fall outside the cache are skipped.
#include "common.h"
#include "fp8_e4m3.h"

template <int HD>
__global__ __launch_bounds__(256) void kv_store_fp8_kernel(
    const bf16* __restrict__ k, const bf16* __restrict__ v, long kstride,
    long vstride, unsigned char* __restrict__ kcodes,
    float* __restrict__ kscale, unsigned char* __restrict__ vcodes,
    float* __restrict__ vscale, const int* __restrict__ cu_seqlens,
    const long* __restrict__ positions, long total, int bs, int nkv,
    long maxlen) {
  constexpr int G = HD / 8;
  const long nwork = total * 2 * nkv * G;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nwork;
       i += (long)gridDim.x * blockDim.x) {
    const int oct = i % G;
    const int hh = (i / G) % (2 * nkv);
    const long t = i / ((long)G * 2 * nkv);
    const bool is_k = hh < nkv;
    const int kvh = is_k ? hh : hh - nkv;
    const short* src = (const short*)(is_k ? k : v) +
                       t * (is_k ? kstride : vstride) + (long)kvh * HD + oct * 8;
    short x[8];
    *(short8*)x = *(const short8*)src;
    float amax = 0.f;
    #pragma unroll
    for (int j = 0; j < 8; j++) amax = fmaxf(amax, fabsf(bf2f(x[j])));
    amax = group_max<G>(amax);
    const float sc = e4m3_row_scale(amax);

    int lo = 0, hi = bs;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((long)cu_seqlens[mid + 1] <= t) lo = mid + 1;
      else hi = mid;
    }
    const long pos = positions[t];
    if (lo >= bs || pos < 0 || pos >= maxlen) continue;
    float f[8];
    #pragma unroll
    for (int j = 0; j < 8; j++) f[j] = e4m3_scaled(bf2f(x[j]), sc);
    int2 o = {e4m3_pack4(f[0], f[1], f[2], f[3]),
              e4m3_pack4(f[4], f[5], f[6], f[7])};
    unsigned char* dst = (is_k ? kcodes : vcodes) +
                         (((long)lo * maxlen + pos) * nkv + kvh) * HD + oct * 8;
    *(int2*)dst = o;
    if (oct == 0)
      (is_k ? kscale : vscale)[((long)lo * nkv + kvh) * maxlen + pos] = sc;
  }
}

void check_fp8_kv_cache(const torch::Tensor& codes, const torch::Tensor& scale,
                        const char* what);  // rope_decode.hip

void kv_store_fp8(torch::Tensor k, torch::Tensor v, torch::Tensor kcodes,
                  torch::Tensor kscale, torch::Tensor vcodes,
                  torch::Tensor vscale, torch::Tensor cu_seqlens,
                  torch::Tensor positions) {
  check_fp8_kv_cache(kcodes, kscale, "k");
  check_fp8_kv_cache(vcodes, vscale, "v");
  TORCH_CHECK(kcodes.sizes() == vcodes.sizes());
  const int bs = kcodes.size(0), nkv = kcodes.size(2), hd = kcodes.size(3);
  const long maxlen = kcodes.size(1);
  auto check_in = [&](const torch::Tensor& x, const char* what) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16 &&
                x.dim() == 3 && x.size(1) == nkv && x.size(2) == hd &&
                x.stride(2) == 1 && (nkv == 1 || x.stride(1) == hd) &&
                (x.size(0) <= 1 || x.stride(0) % 8 == 0) &&
                (uintptr_t)x.data_ptr() % 16 == 0,
                what, " must be bf16 [total, nkv, hd] with contiguous, 16-byte "
                "aligned token rows");
  };
  check_in(k, "k");
  check_in(v, "v");
  const long total = k.size(0);
  TORCH_CHECK(v.size(0) == total);
  TORCH_CHECK(cu_seqlens.is_cuda() && cu_seqlens.scalar_type() == torch::kInt &&
              cu_seqlens.is_contiguous() && cu_seqlens.numel() == bs + 1,
              "cu_seqlens must be int32 [bs + 1]");
  TORCH_CHECK(positions.is_cuda() && positions.scalar_type() == torch::kLong &&
              positions.is_contiguous() && positions.numel() == total,
              "positions must be int64 [total]");
  if (total == 0) return;
  const long nwork = total * 2 * nkv * (hd / 8);
  const int grid = (int)std::min<long>((nwork + 255) / 256, 8192);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, cur_stream(),
      (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(), (long)k.stride(0),
      (long)v.stride(0), (unsigned char*)kcodes.data_ptr(),
      kscale.data_ptr<float>(), (unsigned char*)vcodes.data_ptr(),
      vscale.data_ptr<float>(), (const int*)cu_seqlens.data_ptr<int>(),
      (const long*)positions.data_ptr<int64_t>(), total, bs, nkv, maxlen);
  };
  if (hd == 64) launch(kv_store_fp8_kernel<64>);
  else if (hd == 128) launch(kv_store_fp8_kernel<128>);
  else if (hd == 256) launch(kv_store_fp8_kernel<256>);
  else TORCH_CHECK(false, "fp8 KV cache: unsupported head_dim ", hd);
  CHECK_CUDA_OK();
}
