// Fused RMSNorm forward/backward for gfx950.
// HBM-bound: vectorized 16-byte loads (guide G13: scalar bf16 is 2x slower).
// One 256-thread workgroup per row (hidden <= 16384), grid-stride over rows.
// Replaces the reference's TransformerEngine RMSNorm (SURVEY.md §2.2 ext deps).
//
// Weight mode (compile-time, GEMMA): plain RMSNorm scales by w, Gemma by
// 1 + w.  The sum is formed in fp32 from the stored weight, as HF Gemma and
// gemma_rms_norm_ref do; in bf16 it would keep 8 mantissa bits of 1 + w.
#include "common.h"
#include "slab_sum.h"

template <typename T, bool GEMMA>
DEVINL float norm_weight(T w) {
  if constexpr (GEMMA) return 1.0f + to_f32<T>(w);
  else return to_f32<T>(w);
}

// sum of v over the workgroup (<= 8 waves), returned to every thread; red is
// free again after the caller's next barrier
DEVINL float rms_block_sum(float v, float* red) {
  v = wave_sum(v);
  int wid = threadIdx.x / WAVE;
  int nw = blockDim.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) red[wid] = v;
  __syncthreads();
  if (threadIdx.x < 8) {
    float v2 = (threadIdx.x < nw) ? red[threadIdx.x] : 0.f;
    for (int off = 4; off > 0; off >>= 1) v2 += __shfl_down(v2, off, 64);
    if (threadIdx.x == 0) red[0] = v2;
  }
  __syncthreads();
  return red[0];
}

template <typename T, int VEC, bool RESID = false, bool GEMMA = false>
__global__ void rmsnorm_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ out,
    float* __restrict__ rstd, int rows, int H, float eps,
    const T* __restrict__ resid = nullptr, T* __restrict__ sum_out = nullptr) {
  __shared__ float red[8];
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* xr = x + (long)row * H;
    T* yr = out + (long)row * H;
    float ss = 0.f;
    for (int i = threadIdx.x * VEC; i < H; i += blockDim.x * VEC) {
      T v[VEC];
      *(float4v*)v = *(const float4v*)(xr + i);  // 16B when VEC matches
      if constexpr (RESID) {
        T r[VEC];
        *(float4v*)r = *(const float4v*)(resid + (long)row * H + i);
        #pragma unroll
        for (int j = 0; j < VEC; j++)
          v[j] = from_f32<T>(to_f32<T>(v[j]) + to_f32<T>(r[j]));
        *(float4v*)(sum_out + (long)row * H + i) = *(float4v*)v;
      }
      #pragma unroll
      for (int j = 0; j < VEC; j++) { float f = to_f32<T>(v[j]); ss += f * f; }
    }
    float rs = rsqrtf(rms_block_sum(ss, red) / H + eps);
    if (threadIdx.x == 0 && rstd) rstd[row] = rs;
    const T* src2 = RESID ? (sum_out + (long)row * H) : xr;
    for (int i = threadIdx.x * VEC; i < H; i += blockDim.x * VEC) {
      T v[VEC], wv[VEC], o[VEC];
      *(float4v*)v = *(const float4v*)(src2 + i);
      *(float4v*)wv = *(const float4v*)(w + i);
      #pragma unroll
      for (int j = 0; j < VEC; j++)
        o[j] = from_f32<T>(to_f32<T>(v[j]) * rs * norm_weight<T, GEMMA>(wv[j]));
      *(float4v*)(yr + i) = *(float4v*)o;
    }
    __syncthreads();
  }
}

// slab variant of the fused add+rmsnorm: x comes in as fp32 split-K
// partial slabs [nks, rows, H] from skinny_gemm_nc (launch-boundary
// reduce); sum_out = sum_s(parts) + resid, out = rmsnorm(sum_out).
template <typename T, int VEC, bool GEMMA = false>
__global__ void add_rmsnorm_slab_kernel(
    const float* __restrict__ parts, int nks, const T* __restrict__ resid,
    const T* __restrict__ w, T* __restrict__ out, T* __restrict__ sum_out,
    int rows, int H, float eps) {
  __shared__ float red[8];
  const long sstride = (long)rows * H;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    T* yr = out + (long)row * H;
    float ss = 0.f;
    for (int i = threadIdx.x * VEC; i < H; i += blockDim.x * VEC) {
      float f[VEC];
      const float* pr = parts + (long)row * H + i;
      #pragma unroll
      for (int j = 0; j < VEC; j += 4)
        *(float4v*)(f + j) = *(const float4v*)(pr + j);
      for (int s = 1; s < nks; s++) {
        #pragma unroll
        for (int j = 0; j < VEC; j += 4) {
          float4v p = *(const float4v*)(pr + (long)s * sstride + j);
          #pragma unroll
          for (int q = 0; q < 4; q++) f[j + q] += p[q];
        }
      }
      T r[VEC], v[VEC];
      *(float4v*)r = *(const float4v*)(resid + (long)row * H + i);
      #pragma unroll
      for (int j = 0; j < VEC; j++) {
        float fv = f[j] + to_f32<T>(r[j]);
        v[j] = from_f32<T>(fv);
        float fq = to_f32<T>(v[j]);
        ss += fq * fq;
      }
      *(float4v*)(sum_out + (long)row * H + i) = *(float4v*)v;
    }
    float rs = rsqrtf(rms_block_sum(ss, red) / H + eps);
    const T* src2 = sum_out + (long)row * H;
    for (int i = threadIdx.x * VEC; i < H; i += blockDim.x * VEC) {
      T v[VEC], wv[VEC], o[VEC];
      *(float4v*)v = *(const float4v*)(src2 + i);
      *(float4v*)wv = *(const float4v*)(w + i);
      #pragma unroll
      for (int j = 0; j < VEC; j++)
        o[j] = from_f32<T>(to_f32<T>(v[j]) * rs * norm_weight<T, GEMMA>(wv[j]));
      *(float4v*)(yr + i) = *(float4v*)o;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Few-row forward (decode: rows <= RMS_ROW_MAX_ROWS, H <= RMS_THREADS * 8 *
// RMS_ROW_MAX_NP = 8192).  With one workgroup per row and 16 rows on 256 CUs
// the kernels above are chains of dependent memory round trips: one per column
// pass and slab, a second pass that re-reads x (or the sum_out it has just
// stored) and only then asks for w.  Here a thread issues every load of all
// its NP column passes up front — w, the residual, x or the slab batches
// (slab_sum.h) — and keeps the bf16-rounded row in registers across the
// reduction; sum_out is written once and never read back.  Same 256 threads,
// same column of every thread (pass c: (c*256 + tid) * VEC), same ss order
// and reduction as the kernels above: out, sum_out and rstd are bit for bit
// theirs.  A thread whose pass-c column is past H loads column 0 instead and
// neither accumulates nor stores it.
// Two-byte types only: the square of a bf16 or fp16 value is exact in fp32,
// so ss comes out the same whether the compiler fuses ss += f * f or not (it
// fuses some elements and not others, differently per kernel).  For fp32
// input that choice shows in the last bit, so fp32 stays on the loops above.
// ---------------------------------------------------------------------------
#define RMS_THREADS 256
#define RMS_ROW_MAX_ROWS 16
#define RMS_ROW_MAX_NP 4
enum { RMS_SRC_PLAIN, RMS_SRC_RESID, RMS_SRC_SLAB };

template <typename T, int VEC, int NP, int SRC, bool GEMMA>
__global__ __launch_bounds__(RMS_THREADS) void rmsnorm_row_kernel(
    const void* __restrict__ xin,  // T [rows, H] | SLAB: fp32 [nks, rows, H]
    int nks, const T* __restrict__ resid, const T* __restrict__ w,
    T* __restrict__ out, T* __restrict__ sum_out, float* __restrict__ rstd,
    int rows, int H, float eps) {
  __shared__ float red[8];
  const long ro = (long)blockIdx.x * H;
  bool on[NP];
  int col[NP];
  #pragma unroll
  for (int c = 0; c < NP; c++) {
    const int i = (c * RMS_THREADS + (int)threadIdx.x) * VEC;
    on[c] = i < H;
    col[c] = on[c] ? i : 0;
  }
  T wv[NP][VEC], r[NP][VEC], v[NP][VEC];
  #pragma unroll
  for (int c = 0; c < NP; c++)
    *(float4v*)wv[c] = *(const float4v*)(w + col[c]);
  if constexpr (SRC != RMS_SRC_PLAIN) {
    #pragma unroll
    for (int c = 0; c < NP; c++)
      *(float4v*)r[c] = *(const float4v*)(resid + ro + col[c]);
  }
  if constexpr (SRC == RMS_SRC_SLAB) {
    static_assert(VEC == 8, "two float4 per thread and pass");
    const float* p[2 * NP];
    #pragma unroll
    for (int c = 0; c < NP; c++) {
      p[2 * c] = (const float*)xin + ro + col[c];
      p[2 * c + 1] = p[2 * c] + 4;
    }
    float4v acc[2 * NP];
    // 8 float4 per slab at NP 4: batches of 4 slabs keep it in registers
    slab_sum<2 * NP, (NP > 2 ? 4 : SLAB_BATCH)>(
        acc, (const float* const (&)[2 * NP])p, (long)rows * H, nks);
    #pragma unroll
    for (int c = 0; c < NP; c++) {
      #pragma unroll
      for (int j = 0; j < VEC; j++)
        v[c][j] = from_f32<T>(acc[2 * c + j / 4][j % 4] + to_f32<T>(r[c][j]));
    }
  } else {
    #pragma unroll
    for (int c = 0; c < NP; c++)
      *(float4v*)v[c] = *(const float4v*)((const T*)xin + ro + col[c]);
    if constexpr (SRC == RMS_SRC_RESID) {
      #pragma unroll
      for (int c = 0; c < NP; c++) {
        #pragma unroll
        for (int j = 0; j < VEC; j++)
          v[c][j] = from_f32<T>(to_f32<T>(v[c][j]) + to_f32<T>(r[c][j]));
      }
    }
  }
  float ss = 0.f;
  #pragma unroll
  for (int c = 0; c < NP; c++) {
    if (!on[c]) continue;
    if constexpr (SRC != RMS_SRC_PLAIN)
      *(float4v*)(sum_out + ro + col[c]) = *(float4v*)v[c];
    #pragma unroll
    for (int j = 0; j < VEC; j++) { float f = to_f32<T>(v[c][j]); ss += f * f; }
  }
  float rs = rsqrtf(rms_block_sum(ss, red) / H + eps);
  if (threadIdx.x == 0 && rstd) rstd[blockIdx.x] = rs;
  #pragma unroll
  for (int c = 0; c < NP; c++) {
    if (!on[c]) continue;
    T o[VEC];
    #pragma unroll
    for (int j = 0; j < VEC; j++)
      o[j] = from_f32<T>(to_f32<T>(v[c][j]) * rs * norm_weight<T, GEMMA>(wv[c][j]));
    *(float4v*)(out + ro + col[c]) = *(float4v*)o;
  }
}

static bool rms_row_gate(long rows, int H, int vec) {
  return rows <= RMS_ROW_MAX_ROWS && H <= RMS_THREADS * vec * RMS_ROW_MAX_NP;
}

// one workgroup per row; NP = the column passes H needs, rounded up to 1/2/4
template <typename T, int VEC, int SRC, bool GEMMA>
static void rms_row_launch(const void* xin, int nks, const T* resid, const T* w,
                           T* out, T* sum_out, float* rstd, int rows, int H,
                           float eps) {
  auto go = [&](auto np) {
    hipLaunchKernelGGL((rmsnorm_row_kernel<T, VEC, np.value, SRC, GEMMA>),
      dim3(rows), dim3(RMS_THREADS), 0, cur_stream(), xin, nks, resid, w, out,
      sum_out, rstd, rows, H, eps);
  };
  const int per = RMS_THREADS * VEC;
  if (H <= per) go(std::integral_constant<int, 1>{});
  else if (H <= 2 * per) go(std::integral_constant<int, 2>{});
  else go(std::integral_constant<int, 4>{});
}

// backward: dx = rs * w * dy - rs^3/H * x * sum(dy * w * x), with w the
// effective weight (1 + w in Gemma mode); dw = sum_rows dy * x * rs in both.
// dw: per-thread partials over this block's rows (each thread owns fixed
// columns), written as ONE partial row per block at the end.
#define RMS_MAX_COLS 64  // supports H <= 256 threads * VEC * (64/VEC)

template <typename T, int VEC, bool GEMMA = false>
__global__ void __launch_bounds__(GEMMA ? RMS_THREADS : 1024) rmsnorm_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ w,
    const float* __restrict__ rstd, T* __restrict__ dx,
    float* __restrict__ dw, int rows, int H) {
  __shared__ float red[8];
  float dwacc[RMS_MAX_COLS];
  #pragma unroll
  for (int j = 0; j < RMS_MAX_COLS; j++) dwacc[j] = 0.f;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* dyr = dy + (long)row * H;
    const T* xr = x + (long)row * H;
    T* dxr = dx + (long)row * H;
    float rs = rstd[row];
    float dot = 0.f;
    for (int i = threadIdx.x * VEC; i < H; i += blockDim.x * VEC) {
      T a[VEC], b[VEC], c[VEC];
      *(float4v*)a = *(const float4v*)(dyr + i);
      *(float4v*)b = *(const float4v*)(w + i);
      *(float4v*)c = *(const float4v*)(xr + i);
      #pragma unroll
      for (int j = 0; j < VEC; j++)
        dot += to_f32<T>(a[j]) * norm_weight<T, GEMMA>(b[j]) * to_f32<T>(c[j]);
    }
    float k = rms_block_sum(dot, red) * rs * rs * rs / H;
    if constexpr (GEMMA) {
      // the loop below with compile-time trips and slots (launched with
      // RMS_THREADS threads): dwacc is indexed by constants only and stays
      // in registers, where the runtime slot puts it in scratch
      #pragma unroll
      for (int c = 0; c < RMS_MAX_COLS / VEC; c++) {
        int i = (c * RMS_THREADS + (int)threadIdx.x) * VEC;
        if (i >= H) continue;
        T a[VEC], b[VEC], cx[VEC], o[VEC];
        *(float4v*)a = *(const float4v*)(dyr + i);
        *(float4v*)b = *(const float4v*)(w + i);
        *(float4v*)cx = *(const float4v*)(xr + i);
        #pragma unroll
        for (int j = 0; j < VEC; j++) {
          float g = to_f32<T>(a[j]);
          float xv = to_f32<T>(cx[j]);
          o[j] = from_f32<T>(rs * norm_weight<T, true>(b[j]) * g - k * xv);
          dwacc[c * VEC + j] += g * xv * rs;
        }
        *(float4v*)(dxr + i) = *(float4v*)o;
      }
    } else {
      int slot = 0;
      for (int i = threadIdx.x * VEC; i < H; i += blockDim.x * VEC, slot += VEC) {
        T a[VEC], b[VEC], c[VEC], o[VEC];
        *(float4v*)a = *(const float4v*)(dyr + i);
        *(float4v*)b = *(const float4v*)(w + i);
        *(float4v*)c = *(const float4v*)(xr + i);
        #pragma unroll
        for (int j = 0; j < VEC; j++) {
          float g = to_f32<T>(a[j]);
          float xv = to_f32<T>(c[j]);
          o[j] = from_f32<T>(rs * to_f32<T>(b[j]) * g - k * xv);
          if (slot + j < RMS_MAX_COLS) dwacc[slot + j] += g * xv * rs;
        }
        *(float4v*)(dxr + i) = *(float4v*)o;
      }
    }
    __syncthreads();
  }
  // one partial row per block — no atomics (2048 blocks contending on
  // 4096 floats serialized ~500x; partials + torch sum is ~30x faster)
  float* dwrow = dw + (long)blockIdx.x * H;
  if constexpr (GEMMA) {
    #pragma unroll
    for (int c = 0; c < RMS_MAX_COLS / VEC; c++) {
      int i = (c * RMS_THREADS + (int)threadIdx.x) * VEC;
      if (i >= H) continue;
      #pragma unroll
      for (int j = 0; j < VEC; j++) dwrow[i + j] = dwacc[c * VEC + j];
    }
  } else {
    int slot = 0;
    for (int i = threadIdx.x * VEC; i < H; i += blockDim.x * VEC, slot += VEC) {
      #pragma unroll
      for (int j = 0; j < VEC; j++)
        if (slot + j < RMS_MAX_COLS) dwrow[i + j] = dwacc[slot + j];
    }
  }
}

// Host side: one launcher per op, templated on the weight mode; the exported
// rmsnorm_* functions are plain RMSNorm, the gemma_* ones the 1 + w mode.
template <bool GEMMA>
static std::vector<torch::Tensor> rmsnorm_fwd_impl(torch::Tensor x, torch::Tensor w,
                                                   double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  int H = x.size(-1);
  long rows = x.numel() / H;
  auto out = torch::empty_like(x);
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat));
  int vec = 16 / x.element_size();
  TORCH_CHECK(H % vec == 0, "hidden dim must be divisible by ", vec);
  int grid = (int)std::min<long>(rows, 2048);
  const bool few = x.element_size() == 2 && rms_row_gate(rows, H, vec);
  DISPATCH_BF16_FP16_FP32(x.scalar_type(), "rmsnorm_fwd", [&] {
    if (few) {
      if constexpr (sizeof(scalar_t) == 2)
        rms_row_launch<scalar_t, 8, RMS_SRC_PLAIN, GEMMA>(
          x.data_ptr(), 1, nullptr, (const scalar_t*)w.data_ptr(),
          (scalar_t*)out.data_ptr(), nullptr, rstd.data_ptr<float>(),
          (int)rows, H, (float)eps);
    } else if (x.element_size() == 2) {
      hipLaunchKernelGGL((rmsnorm_fwd_kernel<scalar_t, 8, false, GEMMA>), dim3(grid), dim3(256), 0,
        cur_stream(), (const scalar_t*)x.data_ptr(), (const scalar_t*)w.data_ptr(),
        (scalar_t*)out.data_ptr(), rstd.data_ptr<float>(), (int)rows, H, (float)eps);
    } else {
      hipLaunchKernelGGL((rmsnorm_fwd_kernel<scalar_t, 4, false, GEMMA>), dim3(grid), dim3(256), 0,
        cur_stream(), (const scalar_t*)x.data_ptr(), (const scalar_t*)w.data_ptr(),
        (scalar_t*)out.data_ptr(), rstd.data_ptr<float>(), (int)rows, H, (float)eps);
    }
  });
  CHECK_CUDA_OK();
  return {out, rstd};
}

template <bool GEMMA>
static std::vector<torch::Tensor> add_rmsnorm_fwd_impl(torch::Tensor x,
                                                       torch::Tensor resid,
                                                       torch::Tensor w, double eps) {
  // out_norm = rmsnorm(x + resid); sum_out = x + resid (the new residual).
  // x may also be fp32 split-K partial slabs [nks, rows, H] from
  // skinny_gemm_nc — then x := sum over slabs (launch-boundary reduce).
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && resid.is_contiguous());
  int H = x.size(-1);
  long rows = resid.numel() / H;
  TORCH_CHECK(H % 8 == 0);
  auto out = torch::empty_like(resid);
  auto sum_out = torch::empty_like(resid);
  int grid = (int)std::min<long>(rows, 2048);
  if (x.dim() == 3 && x.scalar_type() == torch::kFloat) {
    TORCH_CHECK(resid.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(x.size(1) * x.size(2) == rows * H);
    if (rms_row_gate(rows, H, 8))
      rms_row_launch<bf16, 8, RMS_SRC_SLAB, GEMMA>(
        x.data_ptr(), (int)x.size(0), (const bf16*)resid.data_ptr(),
        (const bf16*)w.data_ptr(), (bf16*)out.data_ptr(),
        (bf16*)sum_out.data_ptr(), nullptr, (int)rows, H, (float)eps);
    else
      hipLaunchKernelGGL((add_rmsnorm_slab_kernel<bf16, 8, GEMMA>), dim3(grid),
        dim3(256), 0, cur_stream(), x.data_ptr<float>(), (int)x.size(0),
        (const bf16*)resid.data_ptr(), (const bf16*)w.data_ptr(),
        (bf16*)out.data_ptr(), (bf16*)sum_out.data_ptr(), (int)rows, H,
        (float)eps);
    CHECK_CUDA_OK();
    return {out, sum_out};
  }
  TORCH_CHECK(x.element_size() == 2);
  DISPATCH_BF16_FP16_FP32(x.scalar_type(), "add_rmsnorm", [&] {
    if constexpr (sizeof(scalar_t) == 2) {
      if (rms_row_gate(rows, H, 8))
        rms_row_launch<scalar_t, 8, RMS_SRC_RESID, GEMMA>(
          x.data_ptr(), 1, (const scalar_t*)resid.data_ptr(),
          (const scalar_t*)w.data_ptr(), (scalar_t*)out.data_ptr(),
          (scalar_t*)sum_out.data_ptr(), nullptr, (int)rows, H, (float)eps);
      else
        hipLaunchKernelGGL((rmsnorm_fwd_kernel<scalar_t, 8, true, GEMMA>), dim3(grid),
          dim3(256), 0, cur_stream(), (const scalar_t*)x.data_ptr(),
          (const scalar_t*)w.data_ptr(), (scalar_t*)out.data_ptr(),
          nullptr, (int)rows, H, (float)eps,
          (const scalar_t*)resid.data_ptr(), (scalar_t*)sum_out.data_ptr());
    }
  });
  CHECK_CUDA_OK();
  return {out, sum_out};
}

template <bool GEMMA>
static std::vector<torch::Tensor> rmsnorm_bwd_impl(torch::Tensor dy, torch::Tensor x,
                                                   torch::Tensor w,
                                                   torch::Tensor rstd) {
  int H = x.size(-1);
  TORCH_CHECK(H <= 256 * RMS_MAX_COLS, "rmsnorm_bwd supports hidden <= 16384");
  long rows = x.numel() / H;
  auto dx = torch::empty_like(x);
  int grid = (int)std::min<long>(rows, 512);
  auto dw32 = torch::zeros({grid, H}, x.options().dtype(torch::kFloat));
  DISPATCH_BF16_FP16_FP32(x.scalar_type(), "rmsnorm_bwd", [&] {
    if (x.element_size() == 2) {
      hipLaunchKernelGGL((rmsnorm_bwd_kernel<scalar_t, 8, GEMMA>), dim3(grid), dim3(RMS_THREADS), 0,
        cur_stream(), (const scalar_t*)dy.data_ptr(), (const scalar_t*)x.data_ptr(),
        (const scalar_t*)w.data_ptr(), rstd.data_ptr<float>(),
        (scalar_t*)dx.data_ptr(), dw32.data_ptr<float>(), (int)rows, H);
    } else {
      hipLaunchKernelGGL((rmsnorm_bwd_kernel<scalar_t, 4, GEMMA>), dim3(grid), dim3(RMS_THREADS), 0,
        cur_stream(), (const scalar_t*)dy.data_ptr(), (const scalar_t*)x.data_ptr(),
        (const scalar_t*)w.data_ptr(), rstd.data_ptr<float>(),
        (scalar_t*)dx.data_ptr(), dw32.data_ptr<float>(), (int)rows, H);
    }
  });
  CHECK_CUDA_OK();
  return {dx, dw32.sum(0).to(x.scalar_type())};
}

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w, double eps) {
  return rmsnorm_fwd_impl<false>(x, w, eps);
}
std::vector<torch::Tensor> gemma_rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                                             double eps) {
  return rmsnorm_fwd_impl<true>(x, w, eps);
}
std::vector<torch::Tensor> add_rmsnorm_fwd(torch::Tensor x, torch::Tensor resid,
                                           torch::Tensor w, double eps) {
  return add_rmsnorm_fwd_impl<false>(x, resid, w, eps);
}
std::vector<torch::Tensor> gemma_add_rmsnorm_fwd(torch::Tensor x, torch::Tensor resid,
                                                 torch::Tensor w, double eps) {
  return add_rmsnorm_fwd_impl<true>(x, resid, w, eps);
}
std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor w, torch::Tensor rstd) {
  return rmsnorm_bwd_impl<false>(dy, x, w, rstd);
}
std::vector<torch::Tensor> gemma_rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                             torch::Tensor w, torch::Tensor rstd) {
  return rmsnorm_bwd_impl<true>(dy, x, w, rstd);
}
