// Per-head QK RMSNorm + RoPE in one kernel, forward and backward (qwen3:
// an RMSNorm over head_dim on every q and every k head, between the QKV
// projection and RoPE; one weight [hd] for q, one for k).
//
// Work item = rope_kernel's: a lane holds 4 elements of the first half of a
// head row and their 4 RoPE partners of the second half.  The hd/8
// consecutive work items of a head (8, 16 or 32) are consecutive lanes of one
// wave and leave the grid-stride loop together — the block is 256 threads and
// the number of work items a multiple of hd/8 — so the row reductions are
// shfl_xor butterflies (group_sum), no LDS and no barrier.  One launch covers
// q and k: heads 0..nq-1 of a token are q's, the next nkv are k's.
//
// q and k come with their own token stride: they are normally views into the
// merged QKV GEMM output [total, (nq + 2 nkv) * hd].  Outputs are contiguous.
// All math is fp32 with one rounding at the store:
//   fwd:  y = rope(x * rstd * w),  rstd = rsqrt(mean(x^2) + eps)
//   bwd:  dn = rope^T(dy)  (the conjugate rotation)
//         dx = rstd * w * dn - rstd^3 / hd * x * sum_j(dn_j w_j x_j)
//         dw_j = sum_rows dn_j * x_j * rstd
// dw without atomics, as rmsnorm_bwd: 256 % (hd/8) == 0 makes a thread's
// columns the same in every iteration, so it accumulates 8 q and 8 k columns
// in registers; the block folds its 256 / (hd/8) threads per column through
// LDS in a fixed order into ONE partial row per block and weight, and the
// host sums the rows.  Two runs give the same bits.
#include "common.h"
#include "fp8_e4m3.h"  // group_sum

#define QKN_THREADS 256

template <typename T>
DEVINL void qkn_load4(const T* p, float (&f)[4]) {
  short4v v = *(const short4v*)p;
  #pragma unroll
  for (int j = 0; j < 4; j++) f[j] = to_f32<T>(((const T*)&v)[j]);
}

template <typename T>
DEVINL void qkn_store4(T* p, const float (&f)[4]) {
  short o[4];
  #pragma unroll
  for (int j = 0; j < 4; j++) ((T*)o)[j] = from_f32<T>(f[j]);
  *(short4v*)p = *(short4v*)o;
}

template <typename T, int HD>
__global__ __launch_bounds__(QKN_THREADS) void qk_norm_rope_fwd_kernel(
    const T* __restrict__ q, long q_stride,  // [total, nq, HD], token stride
    const T* __restrict__ k, long k_stride,  // [total, nkv, HD]
    const T* __restrict__ q_w, const T* __restrict__ k_w,  // [HD]
    T* __restrict__ q_out, T* __restrict__ k_out,  // contiguous
    float* __restrict__ rstd,  // [total, nq + nkv]
    const float* __restrict__ cosb, const float* __restrict__ sinb,
    const long* __restrict__ pos, long total, int nq, int nkv, float eps,
    bool apply_rope) {
  constexpr int G = HD / 8, HD2 = HD / 2;
  const int nh = nq + nkv;
  const long nwork = total * nh * G;
  for (long i = (long)blockIdx.x * QKN_THREADS + threadIdx.x; i < nwork;
       i += (long)gridDim.x * QKN_THREADS) {
    const int d0 = (int)(i % G) * 4;
    const long th = i / G;
    const int h = th % nh;
    const long t = th / nh;
    const bool is_q = h < nq;
    const T* src = is_q ? q + t * q_stride + (long)h * HD
                        : k + t * k_stride + (long)(h - nq) * HD;
    T* dst = is_q ? q_out + (t * nq + h) * HD
                  : k_out + (t * nkv + (h - nq)) * HD;
    const T* w = is_q ? q_w : k_w;
    float4v c = {1.f, 1.f, 1.f, 1.f}, s = {};
    if (apply_rope) {
      const long p = pos[t];
      c = *(const float4v*)(cosb + p * HD2 + d0);
      s = *(const float4v*)(sinb + p * HD2 + d0);
    }
    float x1[4], x2[4], w1[4], w2[4];
    qkn_load4(src + d0, x1);
    qkn_load4(src + HD2 + d0, x2);
    qkn_load4(w + d0, w1);
    qkn_load4(w + HD2 + d0, w2);
    float ss = 0.f;
    #pragma unroll
    for (int j = 0; j < 4; j++) {
      ss = fmaf(x1[j], x1[j], ss);
      ss = fmaf(x2[j], x2[j], ss);
    }
    ss = group_sum<G>(ss);
    const float rs = rsqrtf(fmaf(ss, 1.f / HD, eps));
    if (d0 == 0) rstd[th] = rs;
    float o1[4], o2[4];
    #pragma unroll
    for (int j = 0; j < 4; j++) {
      const float a = x1[j] * rs * w1[j];
      const float b = x2[j] * rs * w2[j];
      o1[j] = a * c[j] - b * s[j];
      o2[j] = b * c[j] + a * s[j];
    }
    qkn_store4(dst + d0, o1);
    qkn_store4(dst + HD2 + d0, o2);
  }
}

template <typename T, int HD>
__global__ __launch_bounds__(QKN_THREADS) void qk_norm_rope_bwd_kernel(
    const T* __restrict__ dqo, const T* __restrict__ dko,  // contiguous
    const T* __restrict__ q, long q_stride,  // the forward's inputs
    const T* __restrict__ k, long k_stride,
    const T* __restrict__ q_w, const T* __restrict__ k_w,
    const float* __restrict__ rstd,  // [total, nq + nkv]
    T* __restrict__ dq, T* __restrict__ dk,  // contiguous
    float* __restrict__ dw_part,  // [2, gridDim.x, HD]: q rows, then k rows
    const float* __restrict__ cosb, const float* __restrict__ sinb,
    const long* __restrict__ pos, long total, int nq, int nkv,
    bool apply_rope) {
  constexpr int G = HD / 8, HD2 = HD / 2;
  static_assert(QKN_THREADS % G == 0 && HD <= QKN_THREADS, "fixed columns");
  __shared__ float red[QKN_THREADS][8];
  const int nh = nq + nkv;
  const long nwork = total * nh * G;
  // this thread's columns never change: the loop stride is a multiple of G
  const int d0 = (int)(threadIdx.x % G) * 4;
  float dwq[8] = {}, dwk[8] = {};
  for (long i = (long)blockIdx.x * QKN_THREADS + threadIdx.x; i < nwork;
       i += (long)gridDim.x * QKN_THREADS) {
    const long th = i / G;
    const int h = th % nh;
    const long t = th / nh;
    const bool is_q = h < nq;
    const long orow = is_q ? (t * nq + h) * HD : (t * nkv + (h - nq)) * HD;
    const T* gsrc = (is_q ? dqo : dko) + orow;
    const T* src = is_q ? q + t * q_stride + (long)h * HD
                        : k + t * k_stride + (long)(h - nq) * HD;
    T* dst = (is_q ? dq : dk) + orow;
    const T* w = is_q ? q_w : k_w;
    float4v c = {1.f, 1.f, 1.f, 1.f}, s = {};
    if (apply_rope) {
      const long p = pos[t];
      c = *(const float4v*)(cosb + p * HD2 + d0);
      s = *(const float4v*)(sinb + p * HD2 + d0);
    }
    const float rs = rstd[th];
    float g1[4], g2[4], x1[4], x2[4], w1[4], w2[4];
    qkn_load4(gsrc + d0, g1);
    qkn_load4(gsrc + HD2 + d0, g2);
    qkn_load4(src + d0, x1);
    qkn_load4(src + HD2 + d0, x2);
    qkn_load4(w + d0, w1);
    qkn_load4(w + HD2 + d0, w2);
    float n1[4], n2[4];
    float dot = 0.f;
    #pragma unroll
    for (int j = 0; j < 4; j++) {
      n1[j] = g1[j] * c[j] + g2[j] * s[j];
      n2[j] = g2[j] * c[j] - g1[j] * s[j];
      dot += n1[j] * w1[j] * x1[j] + n2[j] * w2[j] * x2[j];
    }
    dot = group_sum<G>(dot);
    const float kx = dot * rs * rs * rs / HD;
    float o1[4], o2[4];
    #pragma unroll
    for (int j = 0; j < 4; j++) {
      o1[j] = rs * w1[j] * n1[j] - kx * x1[j];
      o2[j] = rs * w2[j] * n2[j] - kx * x2[j];
      const float a = n1[j] * x1[j] * rs, b = n2[j] * x2[j] * rs;
      // selects, not indexing by is_q: both arrays stay in registers
      dwq[j] += is_q ? a : 0.f;
      dwq[4 + j] += is_q ? b : 0.f;
      dwk[j] += is_q ? 0.f : a;
      dwk[4 + j] += is_q ? 0.f : b;
    }
    qkn_store4(dst + d0, o1);
    qkn_store4(dst + HD2 + d0, o2);
  }
  // fold the QKN_THREADS / G threads of every column, in thread order
  #pragma unroll
  for (int which = 0; which < 2; which++) {
    if (which) __syncthreads();
    #pragma unroll
    for (int j = 0; j < 8; j++)
      red[threadIdx.x][j] = which ? dwk[j] : dwq[j];
    __syncthreads();
    if (threadIdx.x < HD) {
      const int col = threadIdx.x;
      const int d = col % HD2;
      const int lane = d / 4, j = (col / HD2) * 4 + d % 4;
      float acc = 0.f;
      for (int r = 0; r < QKN_THREADS / G; r++) acc += red[r * G + lane][j];
      dw_part[((long)which * gridDim.x + blockIdx.x) * HD + col] = acc;
    }
  }
}

static void qkn_check(const torch::Tensor& x, const char* what, int hd) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.size(2) == hd &&
              x.stride(2) == 1 && (x.size(1) == 1 || x.stride(1) == hd) &&
              x.stride(0) % 4 == 0 &&
              reinterpret_cast<uintptr_t>(x.data_ptr()) % 8 == 0,
              "qk_norm_rope: ", what, " must be [total, heads, hd] with "
              "contiguous 8-byte aligned head rows");
}

static void qkn_check_w(const torch::Tensor& w, const torch::Tensor& x) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 1 && w.size(0) == x.size(2) &&
              w.is_contiguous() && w.scalar_type() == x.scalar_type(),
              "qk_norm_rope: weights must be contiguous [hd] of q's dtype");
}

// dispatch over the two-byte dtype and the head dim
template <typename F>
static void qkn_dispatch(const torch::Tensor& x, F&& f) {
  const int hd = x.size(2);
  auto by_hd = [&](auto tag) {
    if (hd == 64) f(tag, std::integral_constant<int, 64>{});
    else if (hd == 128) f(tag, std::integral_constant<int, 128>{});
    else if (hd == 256) f(tag, std::integral_constant<int, 256>{});
    else TORCH_CHECK(false, "qk_norm_rope: unsupported head_dim ", hd);
  };
  if (x.scalar_type() == at::ScalarType::BFloat16) by_hd(__hip_bfloat16{});
  else if (x.scalar_type() == at::ScalarType::Half) by_hd(__half{});
  else TORCH_CHECK(false, "qk_norm_rope: bf16/fp16 only");
}

// returns {q', k', rstd}
std::vector<torch::Tensor> qk_norm_rope_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor q_w, torch::Tensor k_w,
    double eps, torch::Tensor cosb, torch::Tensor sinb,
    torch::Tensor positions, bool apply_rope) {
  const int hd = q.size(-1);
  qkn_check(q, "q", hd);
  qkn_check(k, "k", hd);
  TORCH_CHECK(k.size(0) == q.size(0) && k.scalar_type() == q.scalar_type());
  qkn_check_w(q_w, q);
  qkn_check_w(k_w, q);
  const long total = q.size(0);
  const int nq = q.size(1), nkv = k.size(1);
  auto q_out = torch::empty({total, (long)nq, (long)hd}, q.options());
  auto k_out = torch::empty({total, (long)nkv, (long)hd}, q.options());
  auto rstd = torch::empty({total, (long)(nq + nkv)},
                           q.options().dtype(torch::kFloat));
  if (total == 0) return {q_out, k_out, rstd};
  torch::Tensor pos;
  const float* cp = nullptr;
  const float* sp = nullptr;
  if (apply_rope) {
    TORCH_CHECK(cosb.scalar_type() == torch::kFloat && cosb.is_contiguous() &&
                sinb.scalar_type() == torch::kFloat && sinb.is_contiguous() &&
                cosb.size(-1) == hd / 2 && positions.numel() == total);
    pos = positions.to(torch::kLong).contiguous();
    cp = cosb.data_ptr<float>();
    sp = sinb.data_ptr<float>();
  }
  const long n = total * (nq + nkv) * (hd / 8);
  const int grid = (int)std::min<long>((n + QKN_THREADS - 1) / QKN_THREADS, 8192);
  qkn_dispatch(q, [&](auto tag, auto hdc) {
    using T = decltype(tag);
    hipLaunchKernelGGL((qk_norm_rope_fwd_kernel<T, decltype(hdc)::value>), dim3(grid),
      dim3(QKN_THREADS), 0, cur_stream(), (const T*)q.data_ptr(),
      (long)q.stride(0), (const T*)k.data_ptr(), (long)k.stride(0),
      (const T*)q_w.data_ptr(), (const T*)k_w.data_ptr(),
      (T*)q_out.data_ptr(), (T*)k_out.data_ptr(), rstd.data_ptr<float>(), cp,
      sp, apply_rope ? pos.data_ptr<long>() : nullptr, total, nq, nkv,
      (float)eps, apply_rope);
  });
  CHECK_CUDA_OK();
  return {q_out, k_out, rstd};
}

// returns {dq, dk, dq_w, dk_w}
std::vector<torch::Tensor> qk_norm_rope_bwd(
    torch::Tensor dq_out, torch::Tensor dk_out, torch::Tensor q,
    torch::Tensor k, torch::Tensor q_w, torch::Tensor k_w, torch::Tensor rstd,
    torch::Tensor cosb, torch::Tensor sinb, torch::Tensor positions,
    bool apply_rope) {
  const int hd = q.size(-1);
  qkn_check(q, "q", hd);
  qkn_check(k, "k", hd);
  qkn_check_w(q_w, q);
  qkn_check_w(k_w, q);
  const long total = q.size(0);
  const int nq = q.size(1), nkv = k.size(1);
  TORCH_CHECK(dq_out.is_contiguous() && dk_out.is_contiguous() &&
              dq_out.sizes() == q.sizes() && dk_out.sizes() == k.sizes() &&
              dq_out.scalar_type() == q.scalar_type() &&
              dk_out.scalar_type() == q.scalar_type() &&
              k.scalar_type() == q.scalar_type());
  TORCH_CHECK(rstd.scalar_type() == torch::kFloat && rstd.is_contiguous() &&
              rstd.numel() == total * (nq + nkv));
  auto dq = torch::empty({total, (long)nq, (long)hd}, q.options());
  auto dk = torch::empty({total, (long)nkv, (long)hd}, q.options());
  if (total == 0)
    return {dq, dk, torch::zeros_like(q_w), torch::zeros_like(k_w)};
  torch::Tensor pos;
  const float* cp = nullptr;
  const float* sp = nullptr;
  if (apply_rope) {
    TORCH_CHECK(cosb.scalar_type() == torch::kFloat && cosb.is_contiguous() &&
                sinb.scalar_type() == torch::kFloat && sinb.is_contiguous() &&
                cosb.size(-1) == hd / 2 && positions.numel() == total);
    pos = positions.to(torch::kLong).contiguous();
    cp = cosb.data_ptr<float>();
    sp = sinb.data_ptr<float>();
  }
  const long n = total * (nq + nkv) * (hd / 8);
  const int grid = (int)std::min<long>((n + QKN_THREADS - 1) / QKN_THREADS, 2048);
  // every block writes its two rows in full: no zero fill
  auto part = torch::empty({2, (long)grid, (long)hd},
                           q.options().dtype(torch::kFloat));
  qkn_dispatch(q, [&](auto tag, auto hdc) {
    using T = decltype(tag);
    hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<T, decltype(hdc)::value>), dim3(grid),
      dim3(QKN_THREADS), 0, cur_stream(), (const T*)dq_out.data_ptr(),
      (const T*)dk_out.data_ptr(), (const T*)q.data_ptr(), (long)q.stride(0),
      (const T*)k.data_ptr(), (long)k.stride(0), (const T*)q_w.data_ptr(),
      (const T*)k_w.data_ptr(), rstd.data_ptr<float>(), (T*)dq.data_ptr(),
      (T*)dk.data_ptr(), part.data_ptr<float>(), cp, sp,
      apply_rope ? pos.data_ptr<long>() : nullptr, total, nq, nkv,
      apply_rope);
  });
  CHECK_CUDA_OK();
  auto dw = part.sum(1).to(q.scalar_type());  // [2, hd]
  return {dq, dk, dw[0], dw[1]};
}
