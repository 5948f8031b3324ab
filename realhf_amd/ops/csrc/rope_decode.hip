// Fused decode-path epilogue: QKV split + optional bias + RoPE(q,k) +
// KV-cache append, one kernel.
// Replaces ~8 small per-layer kernels in the captured decode graph
// (2x contiguous-copy, 2x rope, 2x index_put, arange, clamp) — each tiny
// kernel costs ~1.5-5us of dispatch floor (guide: boundary row), which at
// 32 layers x 512 tokens dominated the glue time.
//
// SLAB mode: qkv comes in as the skinny GEMM's fp32 split-K partial
// slabs [nks, bs, qkvd]; the per-element sum over nks happens in this
// kernel's prologue (launch-boundary reduce) instead of a separate
// sg_combine launch.
//
// FP8 mode (FP8 KV cache): the K and V head rows are not stored as bf16 but
// quantized from the bf16-rounded values, per head row of hd elements, by
// fp8_e4m3.h's definition: codes [bs, maxlen, nkv, hd] (one byte each) and
// one fp32 scale per row in [bs, nkv, maxlen].  The hd/8 consecutive work
// items of a head take its amax by shfl_xor.  That group is always inside
// one wave and leaves the grid-stride loop together: the block is 256
// threads, hd/8 is 8, 16 or 32, and nwork is a multiple of it.
//
// NORM mode (qwen3's per-head QK RMSNorm): after the slab sum and the bias
// add and before RoPE, a q or k head row is scaled by rstd * w[d], rstd over
// the head's hd elements in fp32 — the sum of squares goes over the same
// hd/8-lane group as the FP8 amax (group_sum).  V heads run the shuffles and
// drop the result.  The head dim to normalise over is a template argument
// (0 = no norm), like FP8_HD: the un-normed forms keep their code.
#include "common.h"
#include "fp8_e4m3.h"
#include "slab_sum.h"

template <bool SLAB, int FP8_HD = 0, int NORM_HD = 0>
__global__ __launch_bounds__(256) void rope_qkv_decode_kernel(
    const void* __restrict__ qkv_in,  // bf16 [bs, qkvd] | fp32 [nks, bs, qkvd]
    const bf16* __restrict__ bias,  // [(nq+2nkv)*hd] or null
    bf16* __restrict__ q_out,  // [bs, nq, hd]
    void* __restrict__ kcache,  // [bs, maxlen, nkv, hd] bf16 | e4m3 codes
    void* __restrict__ vcache,
    float* __restrict__ kscale,  // FP8: [bs, nkv, maxlen], else unused
    float* __restrict__ vscale,
    const int* __restrict__ cache_seqlens,  // [bs]
    const float* __restrict__ cosb, const float* __restrict__ sinb,  // [*, hd/2]
    int bs, int nq, int nkv, int hd, long maxlen, long qkv_stride,
    bool apply_rope, int nks,
    const bf16* __restrict__ q_w = nullptr,  // NORM: [hd] each, else unused
    const bf16* __restrict__ k_w = nullptr, float eps = 0.f) {
  const int nh = nq + 2 * nkv;
  const int hd2 = hd / 2;
  const long nwork = (long)bs * nh * (hd2 / 4);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nwork;
       i += (long)gridDim.x * blockDim.x) {
    const int quad = i % (hd2 / 4);
    const int h = (i / (hd2 / 4)) % nh;
    const int b = i / ((long)nh * (hd2 / 4));
    const int d0 = quad * 4;
    const int pos = max(cache_seqlens[b] - 1, 0);

    // everything that does not depend on the slab sum goes out before it:
    // bias and cos / sin (V heads load theirs too and ignore them) are in
    // flight with the first slab batch
    short4v b1 = {}, b2 = {};
    float4v c = {}, s = {};
    if (bias) {
      b1 = *(const short4v*)((const short*)bias + (long)h * hd + d0);
      b2 = *(const short4v*)((const short*)bias + (long)h * hd + hd2 + d0);
    }
    if (apply_rope) {
      c = *(const float4v*)(cosb + (long)pos * hd2 + d0);
      s = *(const float4v*)(sinb + (long)pos * hd2 + d0);
    }
    short4v w1 = {}, w2 = {};
    if constexpr (NORM_HD != 0) {
      // V heads load k_w and ignore it
      const short* w = (const short*)(h < nq ? q_w : k_w);
      w1 = *(const short4v*)(w + d0);
      w2 = *(const short4v*)(w + hd2 + d0);
    }
    float4v f1, f2;
    if constexpr (SLAB) {
      const float* src =
          (const float*)qkv_in + (long)b * qkv_stride + (long)h * hd;
      const float* const p[2] = {src + d0, src + hd2 + d0};
      float4v acc[2];
      slab_sum<2>(acc, p, (long)bs * qkv_stride, nks);
      f1 = acc[0];
      f2 = acc[1];
    } else {
      const bf16* src =
          (const bf16*)qkv_in + (long)b * qkv_stride + (long)h * hd;
      short4v x1 = *(const short4v*)((const short*)src + d0);
      short4v x2 = *(const short4v*)((const short*)src + hd2 + d0);
      #pragma unroll
      for (int j = 0; j < 4; j++) {
        f1[j] = __bfloat162float(((const bf16*)&x1)[j]);
        f2[j] = __bfloat162float(((const bf16*)&x2)[j]);
      }
    }
    if (bias) {
      #pragma unroll
      for (int j = 0; j < 4; j++) {
        f1[j] += __bfloat162float(((const bf16*)&b1)[j]);
        f2[j] += __bfloat162float(((const bf16*)&b2)[j]);
      }
    }
    if constexpr (NORM_HD != 0) {
      float ss = 0.f;
      #pragma unroll
      for (int j = 0; j < 4; j++) {
        // explicit fmas: every form (slab or not, FP8 cache or not) rounds
        // the sum alike, whatever the compiler would contract
        ss = fmaf(f1[j], f1[j], ss);
        ss = fmaf(f2[j], f2[j], ss);
      }
      ss = group_sum<NORM_HD / 8>(ss);
      const float rs = rsqrtf(fmaf(ss, 1.f / NORM_HD, eps));
      if (h < nq + nkv) {
        #pragma unroll
        for (int j = 0; j < 4; j++) {
          f1[j] *= rs * bf2f(w1[j]);
          f2[j] *= rs * bf2f(w2[j]);
        }
      }
    }
    bf16* dst;
    bool rope = apply_rope;
    if (h < nq) {
      dst = q_out + ((long)b * nq + h) * hd;
    } else if (h < nq + nkv) {
      dst = (bf16*)kcache + (((long)b * maxlen + pos) * nkv + (h - nq)) * hd;
    } else {
      dst = (bf16*)vcache +
            (((long)b * maxlen + pos) * nkv + (h - nq - nkv)) * hd;
      rope = false;
    }
    short o1[4], o2[4];
    if (rope) {
      #pragma unroll
      for (int j = 0; j < 4; j++) {
        ((bf16*)o1)[j] = __float2bfloat16(f1[j] * c[j] - f2[j] * s[j]);
        ((bf16*)o2)[j] = __float2bfloat16(f2[j] * c[j] + f1[j] * s[j]);
      }
    } else {
      #pragma unroll
      for (int j = 0; j < 4; j++) {
        ((bf16*)o1)[j] = __float2bfloat16(f1[j]);
        ((bf16*)o2)[j] = __float2bfloat16(f2[j]);
      }
    }
    if constexpr (FP8_HD != 0) {
      if (h >= nq) {
        // quantize the bf16-rounded head row: o1 / o2 hold what the bf16
        // cache would have stored (dst is not used for these heads)
        float amax = 0.f;
        #pragma unroll
        for (int j = 0; j < 4; j++)
          amax = fmaxf(amax, fmaxf(fabsf(bf2f(o1[j])), fabsf(bf2f(o2[j]))));
        amax = group_max<FP8_HD / 8>(amax);
        const float sc = e4m3_row_scale(amax);
        const bool is_k = h < nq + nkv;
        const int kvh = is_k ? h - nq : h - nq - nkv;
        unsigned char* cdst =
            (unsigned char*)(is_k ? kcache : vcache) +
            (((long)b * maxlen + pos) * nkv + kvh) * hd;
        *(int*)(cdst + d0) = e4m3_pack4(
            e4m3_scaled(bf2f(o1[0]), sc), e4m3_scaled(bf2f(o1[1]), sc),
            e4m3_scaled(bf2f(o1[2]), sc), e4m3_scaled(bf2f(o1[3]), sc));
        *(int*)(cdst + hd2 + d0) = e4m3_pack4(
            e4m3_scaled(bf2f(o2[0]), sc), e4m3_scaled(bf2f(o2[1]), sc),
            e4m3_scaled(bf2f(o2[2]), sc), e4m3_scaled(bf2f(o2[3]), sc));
        if (quad == 0)
          (is_k ? kscale : vscale)[((long)b * nkv + kvh) * maxlen + pos] = sc;
        continue;
      }
    }
    *(short4v*)((short*)dst + d0) = *(short4v*)o1;
    *(short4v*)((short*)dst + hd2 + d0) = *(short4v*)o2;
  }
}

// kscale / vscale null: bf16 caches; else e4m3 codes + fp32 row scales
static torch::Tensor rope_qkv_decode_impl(
    torch::Tensor qkv, c10::optional<torch::Tensor> bias, torch::Tensor kcache,
    torch::Tensor vcache, float* kscale, float* vscale,
    torch::Tensor cache_seqlens, torch::Tensor cosb, torch::Tensor sinb,
    long nq, bool apply_rope, const torch::Tensor* q_w = nullptr,
    const torch::Tensor* k_w = nullptr, double eps = 0.0) {
  TORCH_CHECK(qkv.is_cuda());
  const bool fp8 = kscale != nullptr;
  const bool norm = q_w != nullptr;
  const bool slab = qkv.dim() == 3;  // fp32 split-K partials [nks, bs, qkvd]
  if (slab) {
    TORCH_CHECK(qkv.scalar_type() == torch::kFloat && qkv.is_contiguous());
  } else {
    TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 && qkv.dim() == 2 &&
                qkv.stride(1) == 1);
  }
  int nks = slab ? qkv.size(0) : 1;
  int bs = slab ? qkv.size(1) : qkv.size(0);
  int nkv = kcache.size(2);
  int hd = kcache.size(3);
  long maxlen = kcache.size(1);
  TORCH_CHECK(qkv.size(-1) == (nq + 2 * nkv) * hd);
  TORCH_CHECK(hd % 8 == 0);
  auto q_out = torch::empty({bs, (long)nq, (long)hd},
                            kcache.options().dtype(torch::kBFloat16));
  long nwork = (long)bs * (nq + 2 * nkv) * (hd / 8);
  int grid = (int)std::min<long>((nwork + 255) / 256, 4096);
  const bf16* bptr = nullptr;
  if (bias.has_value()) bptr = (const bf16*)bias->data_ptr();
  long qkv_stride = slab ? qkv.stride(1) : qkv.stride(0);
  const bf16* qw = nullptr;
  const bf16* kw = nullptr;
  if (norm) {
    for (const torch::Tensor* w : {q_w, k_w})
      TORCH_CHECK(w->is_cuda() && w->scalar_type() == torch::kBFloat16 &&
                  w->dim() == 1 && w->size(0) == hd && w->is_contiguous(),
                  "qk norm weights must be contiguous bf16 [head_dim]");
    qw = (const bf16*)q_w->data_ptr();
    kw = (const bf16*)k_w->data_ptr();
  }
  auto launch = [&](auto kern, int nks_arg) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, cur_stream(),
      (const void*)qkv.data_ptr(), bptr, (bf16*)q_out.data_ptr(),
      kcache.data_ptr(), vcache.data_ptr(), kscale, vscale,
      (const int*)cache_seqlens.data_ptr<int>(),
      (const float*)cosb.data_ptr<float>(), (const float*)sinb.data_ptr<float>(),
      bs, (int)nq, nkv, hd, maxlen, qkv_stride, apply_rope, nks_arg,
      qw, kw, (float)eps);
  };
  if (norm) {
    // NORM forms: hd is compile-time for the group reduction, FP8 or not
    auto pick = [&](auto hdc) {
      constexpr int HD = decltype(hdc)::value;
      if (fp8) {
        if (slab) launch(rope_qkv_decode_kernel<true, HD, HD>, nks);
        else launch(rope_qkv_decode_kernel<false, HD, HD>, 1);
      } else {
        if (slab) launch(rope_qkv_decode_kernel<true, 0, HD>, nks);
        else launch(rope_qkv_decode_kernel<false, 0, HD>, 1);
      }
    };
    if (hd == 64) pick(std::integral_constant<int, 64>{});
    else if (hd == 128) pick(std::integral_constant<int, 128>{});
    else if (hd == 256) pick(std::integral_constant<int, 256>{});
    else TORCH_CHECK(false, "qk norm decode: unsupported head_dim ", hd);
  } else if (!fp8) {
    if (slab) launch(rope_qkv_decode_kernel<true>, nks);
    else launch(rope_qkv_decode_kernel<false>, 1);
  } else if (hd == 64) {
    if (slab) launch(rope_qkv_decode_kernel<true, 64>, nks);
    else launch(rope_qkv_decode_kernel<false, 64>, 1);
  } else if (hd == 128) {
    if (slab) launch(rope_qkv_decode_kernel<true, 128>, nks);
    else launch(rope_qkv_decode_kernel<false, 128>, 1);
  } else if (hd == 256) {
    if (slab) launch(rope_qkv_decode_kernel<true, 256>, nks);
    else launch(rope_qkv_decode_kernel<false, 256>, 1);
  } else {
    TORCH_CHECK(false, "fp8 KV cache: unsupported head_dim ", hd);
  }
  CHECK_CUDA_OK();
  return q_out;
}

torch::Tensor rope_qkv_decode(
    torch::Tensor qkv, c10::optional<torch::Tensor> bias, torch::Tensor kcache,
    torch::Tensor vcache, torch::Tensor cache_seqlens, torch::Tensor cosb,
    torch::Tensor sinb, long nq, bool apply_rope) {
  return rope_qkv_decode_impl(qkv, bias, kcache, vcache, nullptr, nullptr,
                              cache_seqlens, cosb, sinb, nq, apply_rope);
}

// rope_qkv_decode with the per-head QK RMSNorm (q_w, k_w bf16 [hd], eps)
// between the bias add and RoPE
torch::Tensor rope_qkv_decode_norm(
    torch::Tensor qkv, c10::optional<torch::Tensor> bias, torch::Tensor kcache,
    torch::Tensor vcache, torch::Tensor cache_seqlens, torch::Tensor cosb,
    torch::Tensor sinb, long nq, bool apply_rope, torch::Tensor q_w,
    torch::Tensor k_w, double eps) {
  return rope_qkv_decode_impl(qkv, bias, kcache, vcache, nullptr, nullptr,
                              cache_seqlens, cosb, sinb, nq, apply_rope, &q_w,
                              &k_w, eps);
}

// codes [bs, maxlen, nkv, hd] (one byte per element), scale fp32
// [bs, nkv, maxlen]; everything else as rope_qkv_decode
void check_fp8_kv_cache(const torch::Tensor& codes, const torch::Tensor& scale,
                        const char* what) {
  TORCH_CHECK(codes.is_cuda() && codes.element_size() == 1 &&
              codes.dim() == 4 && codes.is_contiguous(),
              what, " codes must be contiguous [bs, maxlen, nkv, hd] with one "
              "byte per element");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == torch::kFloat32 &&
              scale.dim() == 3 && scale.is_contiguous() &&
              scale.size(0) == codes.size(0) && scale.size(1) == codes.size(2) &&
              scale.size(2) == codes.size(1),
              what, " scale must be contiguous fp32 [bs, nkv, maxlen]");
}

static torch::Tensor rope_qkv_decode_fp8_impl(
    torch::Tensor qkv, c10::optional<torch::Tensor> bias, torch::Tensor kcodes,
    torch::Tensor kscale, torch::Tensor vcodes, torch::Tensor vscale,
    torch::Tensor cache_seqlens, torch::Tensor cosb, torch::Tensor sinb,
    long nq, bool apply_rope, const torch::Tensor* q_w = nullptr,
    const torch::Tensor* k_w = nullptr, double eps = 0.0) {
  check_fp8_kv_cache(kcodes, kscale, "k");
  check_fp8_kv_cache(vcodes, vscale, "v");
  TORCH_CHECK(kcodes.sizes() == vcodes.sizes());
  const long bs = qkv.dim() == 3 ? qkv.size(1) : qkv.size(0);
  TORCH_CHECK(bs == kcodes.size(0) && cache_seqlens.numel() == bs,
              "batch size of qkv, caches and cache_seqlens must agree");
  return rope_qkv_decode_impl(qkv, bias, kcodes, vcodes,
                              kscale.data_ptr<float>(),
                              vscale.data_ptr<float>(), cache_seqlens, cosb,
                              sinb, nq, apply_rope, q_w, k_w, eps);
}

torch::Tensor rope_qkv_decode_fp8(
    torch::Tensor qkv, c10::optional<torch::Tensor> bias, torch::Tensor kcodes,
    torch::Tensor kscale, torch::Tensor vcodes, torch::Tensor vscale,
    torch::Tensor cache_seqlens, torch::Tensor cosb, torch::Tensor sinb,
    long nq, bool apply_rope) {
  return rope_qkv_decode_fp8_impl(qkv, bias, kcodes, kscale, vcodes, vscale,
                                  cache_seqlens, cosb, sinb, nq, apply_rope);
}

torch::Tensor rope_qkv_decode_fp8_norm(
    torch::Tensor qkv, c10::optional<torch::Tensor> bias, torch::Tensor kcodes,
    torch::Tensor kscale, torch::Tensor vcodes, torch::Tensor vscale,
    torch::Tensor cache_seqlens, torch::Tensor cosb, torch::Tensor sinb,
    long nq, bool apply_rope, torch::Tensor q_w, torch::Tensor k_w,
    double eps) {
  return rope_qkv_decode_fp8_impl(qkv, bias, kcodes, kscale, vcodes, vscale,
                                  cache_seqlens, cosb, sinb, nq, apply_rope,
                                  &q_w, &k_w, eps);
}
