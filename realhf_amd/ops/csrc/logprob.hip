// Fused vocab log-prob statistics (forward) and dlogits (backward) for gfx950.
// HBM-bound: one 256-thread workgroup per row, lanes stride over the row
// with 16-byte loads (guide G13), every logit read once.  The forward keeps
// a per-lane running (max, sum) and merges lanes with the wave shuffles of
// common.h plus one LDS step across the four waves; nothing fp32 of size
// [n, V] is ever materialised.  No atomics: lane/wave merge order is fixed,
// so results are bitwise reproducible.
//
// Row bases are 16-byte aligned only when V is a multiple of the vector
// width (GPT-2: V = 50257), so each row is split into a scalar head up to
// the first 16-byte boundary, an aligned vector body and a scalar tail.
#include "common.h"

#include <cstdint>

#define LP_THREADS 256
#define LP_NWAVES (LP_THREADS / WAVE)

template <typename T> struct LpVec;
template <> struct LpVec<bf16> {
  static constexpr int N = 8;
  static DEVINL void load(const bf16* p, float* f) {
    short8 v = *(const short8*)p;
    #pragma unroll
    for (int j = 0; j < 8; j++) f[j] = bf2f(v[j]);
  }
  static DEVINL void store(bf16* p, const float* f) {
    short8 v;
    #pragma unroll
    for (int j = 0; j < 8; j++) v[j] = f2bf(f[j]);
    *(short8*)p = v;
  }
  static DEVINL float load1(const bf16* p) { return bf2f(*(const short*)p); }
  static DEVINL void store1(bf16* p, float f) { *(short*)p = f2bf(f); }
};
template <> struct LpVec<float> {
  static constexpr int N = 4;
  static DEVINL void load(const float* p, float* f) {
    float4v v = *(const float4v*)p;
    #pragma unroll
    for (int j = 0; j < 4; j++) f[j] = v[j];
  }
  static DEVINL void store(float* p, const float* f) {
    float4v v;
    #pragma unroll
    for (int j = 0; j < 4; j++) v[j] = f[j];
    *(float4v*)p = v;
  }
  static DEVINL float load1(const float* p) { return *p; }
  static DEVINL void store1(float* p, float f) { *p = f; }
};

// number of leading elements before the first 16-byte boundary of p
template <typename T> DEVINL int lp_head(const T* p, int V) {
  int h = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(T));
  return h < V ? h : V;
}

// online softmax-denominator update of (m, s) with one value.  m stays -inf
// (and s stays 0) while only -inf has been seen: the rescale is skipped so
// that (-inf) - (-inf) is never evaluated.
DEVINL void lp_acc(float& m, float& s, float f) {
  float mn = fmaxf(m, f);
  if (mn > -INFINITY) {
    s = s * __expf(m - mn) + __expf(f - mn);
    m = mn;
  }
}

template <typename T>
__global__ __launch_bounds__(LP_THREADS) void vocab_logprob_fwd_kernel(
    const T* __restrict__ x, const long* __restrict__ labels,
    float* __restrict__ target, float* __restrict__ rowmax,
    float* __restrict__ sumexp, int V, long vocab_start, long ignore_index) {
  using VT = LpVec<T>;
  constexpr int VEC = VT::N;
  __shared__ float red_m[LP_NWAVES], red_s[LP_NWAVES];
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  const long label = labels[row];
  if (label == ignore_index) {  // uniform over the workgroup
    if (tid == 0) { target[row] = 0.f; rowmax[row] = 0.f; sumexp[row] = 1.f; }
    return;
  }
  // range check BEFORE the label is used as an index
  const long ll = label - vocab_start;
  const int lbl = (ll >= 0 && ll < (long)V) ? (int)ll : -1;
  const T* xr = x + row * (long)V;
  const int head = lp_head(xr, V);
  const int nvec = (V - head) / VEC;
  const int tail0 = head + nvec * VEC;

  float m = -INFINITY, s = 0.f;
  for (int i = tid; i < head; i += LP_THREADS) {
    float f = VT::load1(xr + i);
    if (i == lbl) target[row] = f;
    lp_acc(m, s, f);
  }
  for (int i = tail0 + tid; i < V; i += LP_THREADS) {
    float f = VT::load1(xr + i);
    if (i == lbl) target[row] = f;
    lp_acc(m, s, f);
  }
  auto acc_vec = [&](const float* f, int i) {
    float vm = f[0];
    #pragma unroll
    for (int j = 1; j < VEC; j++) vm = fmaxf(vm, f[j]);
    if ((unsigned)(lbl - i) < (unsigned)VEC) {
      float t = 0.f;
      #pragma unroll
      for (int j = 0; j < VEC; j++) t = (i + j == lbl) ? f[j] : t;
      target[row] = t;
    }
    float mn = fmaxf(m, vm);
    if (mn > -INFINITY) {
      float acc = s * __expf(m - mn);
      #pragma unroll
      for (int j = 0; j < VEC; j++) acc += __expf(f[j] - mn);
      s = acc;
      m = mn;
    }
  };
  // two independent 16-byte loads in flight per lane
  int v = tid;
  for (; v + LP_THREADS < nvec; v += 2 * LP_THREADS) {
    const int i0 = head + v * VEC, i1 = i0 + LP_THREADS * VEC;
    float f0[VEC], f1[VEC];
    VT::load(xr + i0, f0);
    VT::load(xr + i1, f1);
    acc_vec(f0, i0);
    acc_vec(f1, i1);
  }
  if (v < nvec) {
    const int i = head + v * VEC;
    float f[VEC];
    VT::load(xr + i, f);
    acc_vec(f, i);
  }
  if (lbl < 0 && tid == 0) target[row] = 0.f;

  // lanes -> wave -> workgroup, fixed order
  const float wm = wave_max(m);
  const float ws = wave_sum(m > -INFINITY ? s * __expf(m - wm) : 0.f);
  if ((tid & (WAVE - 1)) == 0) { red_m[tid / WAVE] = wm; red_s[tid / WAVE] = ws; }
  __syncthreads();
  if (tid == 0) {
    float gm = red_m[0];
    #pragma unroll
    for (int w = 1; w < LP_NWAVES; w++) gm = fmaxf(gm, red_m[w]);
    float gs = 0.f;
    #pragma unroll
    for (int w = 0; w < LP_NWAVES; w++)
      gs += red_m[w] > -INFINITY ? red_s[w] * __expf(red_m[w] - gm) : 0.f;
    rowmax[row] = gm;
    sumexp[row] = gs;
  }
}

// dlogits[r, j] = grad_out[r] * ([j == label_r - vocab_start] - exp(x - lse))
template <typename T>
__global__ __launch_bounds__(LP_THREADS) void vocab_logprob_bwd_kernel(
    const T* __restrict__ x, const long* __restrict__ labels,
    const float* __restrict__ lse, const float* __restrict__ grad_out,
    T* __restrict__ dx, int V, long vocab_start, long ignore_index) {
  using VT = LpVec<T>;
  constexpr int VEC = VT::N;
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  const long label = labels[row];
  const T* xr = x + row * (long)V;
  T* dr = dx + row * (long)V;

  if (label == ignore_index) {  // exact zeros, logits not read
    const int head = lp_head(dr, V);
    const int nvec = (V - head) / VEC;
    const int tail0 = head + nvec * VEC;
    float z[VEC];
    #pragma unroll
    for (int j = 0; j < VEC; j++) z[j] = 0.f;
    for (int i = tid; i < head; i += LP_THREADS) VT::store1(dr + i, 0.f);
    for (int i = tail0 + tid; i < V; i += LP_THREADS) VT::store1(dr + i, 0.f);
    for (int v = tid; v < nvec; v += LP_THREADS) VT::store(dr + head + v * VEC, z);
    return;
  }
  const long ll = label - vocab_start;
  const int lbl = (ll >= 0 && ll < (long)V) ? (int)ll : -1;
  const float l = lse[row];
  const float go = grad_out[row];
  // input and output rows share one head/body/tail split only if they are
  // misaligned by the same amount; otherwise the whole row goes scalar
  int head = lp_head(xr, V);
  if ((((uintptr_t)xr ^ (uintptr_t)dr) & 15u) != 0) head = V;
  const int nvec = (V - head) / VEC;
  const int tail0 = head + nvec * VEC;

  for (int i = tid; i < head; i += LP_THREADS) {
    float p = __expf(VT::load1(xr + i) - l);
    VT::store1(dr + i, go * ((i == lbl ? 1.f : 0.f) - p));
  }
  for (int i = tail0 + tid; i < V; i += LP_THREADS) {
    float p = __expf(VT::load1(xr + i) - l);
    VT::store1(dr + i, go * ((i == lbl ? 1.f : 0.f) - p));
  }
  auto grad_vec = [&](float* f, int i) {
    #pragma unroll
    for (int j = 0; j < VEC; j++)
      f[j] = go * ((i + j == lbl ? 1.f : 0.f) - __expf(f[j] - l));
    VT::store(dr + i, f);
  };
  int v = tid;
  for (; v + LP_THREADS < nvec; v += 2 * LP_THREADS) {
    const int i0 = head + v * VEC, i1 = i0 + LP_THREADS * VEC;
    float f0[VEC], f1[VEC];
    VT::load(xr + i0, f0);
    VT::load(xr + i1, f1);
    grad_vec(f0, i0);
    grad_vec(f1, i1);
  }
  if (v < nvec) {
    const int i = head + v * VEC;
    float f[VEC];
    VT::load(xr + i, f);
    grad_vec(f, i);
  }
}

static void lp_check(const torch::Tensor& logits, const torch::Tensor& labels) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous(),
              "vocab_logprob: logits must be a contiguous [n, v_local] GPU tensor");
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 ||
              logits.scalar_type() == torch::kFloat,
              "vocab_logprob: logits must be bf16 or fp32");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == torch::kLong &&
              labels.is_contiguous() && labels.dim() == 1 &&
              labels.size(0) == logits.size(0),
              "vocab_logprob: labels must be a contiguous int64 [n] GPU tensor");
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) < (1L << 31) - 16 &&
              logits.size(0) < (1L << 31),
              "vocab_logprob: unsupported shape");
}

#define LP_DISPATCH(TYPE, ...) \
  [&] { \
    if (TYPE == at::ScalarType::BFloat16) { using scalar_t = bf16; return __VA_ARGS__(); } \
    else { using scalar_t = float; return __VA_ARGS__(); } \
  }()

std::vector<torch::Tensor> vocab_logprob_fwd(torch::Tensor logits,
                                             torch::Tensor labels,
                                             long vocab_start,
                                             long ignore_index) {
  lp_check(logits, labels);
  const long n = logits.size(0);
  const int V = (int)logits.size(1);
  auto opt = logits.options().dtype(torch::kFloat);
  auto target = torch::empty({n}, opt);
  auto rowmax = torch::empty({n}, opt);
  auto sumexp = torch::empty({n}, opt);
  if (n == 0) return {target, rowmax, sumexp};
  LP_DISPATCH(logits.scalar_type(), [&] {
    hipLaunchKernelGGL((vocab_logprob_fwd_kernel<scalar_t>), dim3((unsigned)n),
      dim3(LP_THREADS), 0, cur_stream(), (const scalar_t*)logits.data_ptr(),
      (const long*)labels.data_ptr<int64_t>(), target.data_ptr<float>(),
      rowmax.data_ptr<float>(), sumexp.data_ptr<float>(), V, vocab_start,
      ignore_index);
  });
  CHECK_CUDA_OK();
  return {target, rowmax, sumexp};
}

torch::Tensor vocab_logprob_bwd(torch::Tensor logits, torch::Tensor labels,
                                torch::Tensor lse, torch::Tensor grad_out,
                                long vocab_start, long ignore_index) {
  lp_check(logits, labels);
  const long n = logits.size(0);
  const int V = (int)logits.size(1);
  for (const auto& t : {lse, grad_out})
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat &&
                t.is_contiguous() && t.dim() == 1 && t.size(0) == n,
                "vocab_logprob_bwd: lse/grad_out must be contiguous fp32 [n]");
  auto dx = torch::empty_like(logits);
  if (n == 0) return dx;
  LP_DISPATCH(logits.scalar_type(), [&] {
    hipLaunchKernelGGL((vocab_logprob_bwd_kernel<scalar_t>), dim3((unsigned)n),
      dim3(LP_THREADS), 0, cur_stream(), (const scalar_t*)logits.data_ptr(),
      (const long*)labels.data_ptr<int64_t>(), lse.data_ptr<float>(),
      grad_out.data_ptr<float>(), (scalar_t*)dx.data_ptr(), V, vocab_start,
      ignore_index);
  });
  CHECK_CUDA_OK();
  return dx;
}
