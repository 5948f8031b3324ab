// Grouped GEMM for MoE experts, forward and backward (gfx950, MFMA).
// Replaces the reference's external grouped_gemm CUDA dep (SURVEY.md §2.2
// ext deps (c): grouped_gemm.ops.gmm, experts.py:194-207), which the
// reference also trains through — with these three kernels MoE training
// stays on the hand-written MFMA path instead of falling back to a
// per-expert GEMM loop.
//
// For each expert e, with seg_e = rows [offs[e], offs[e+1]):
//   out[seg_e] = x[seg_e] @ W[e]^T                          -> [total, N]
//   dX[seg_e]  = dOut[seg_e] @ W[e]        (reduce over n)  -> [total, K]
//   dW[e]      = dOut[seg_e]^T @ x[seg_e]  (reduce over m)  -> [E, N, K]
//   x: [total, K] bf16 (tokens sorted by expert)
//   W: [E, N, K] bf16 (row-major, K contiguous — the canonical layout)
//
// One workgroup per 64 x 64 output tile; 4 waves, wave w owns 16 rows; the
// reduction dimension is staged in 32-deep LDS tiles.  The backward
// reductions run over a dimension that is NOT contiguous in one of the
// operands, so the LDS staging TRANSPOSES that operand tile at store time
// (8 scalar ds_writes per loaded 16-byte vector); MFMA fragments then read
// 8 contiguous reduction elements per lane in all three kernels (lane
// maps: mfma.h).
#include "mfma.h"

#define GG_TM 64   // output-row tile
#define GG_TN 64   // output-col tile
#define GG_TK 32   // reduction tile (MFMA k=32)
#define GG_PAD 8

// LDS operand tile: 64 output rows (or cols) x 32 reduction elems, padded
typedef __bf16 gg_tile_t[GG_TM][GG_TK + GG_PAD];

// acc[t] += A(rows wv*16.., k) x B(cols t*16.., k), t = 0..3: wave wv's 16
// rows of a_s against the four 16-column subtiles of b_s
DEVINL void gg_mma_step(const gg_tile_t& a_s, const gg_tile_t& b_s, int wv,
                        int i16, int g, f32x4 (&acc)[4]) {
  bf16x8 afrag = *(const bf16x8*)(&a_s[wv * 16 + i16][g * 8]);
  #pragma unroll
  for (int t = 0; t < 4; t++) {
    bf16x8 bfrag = *(const bf16x8*)(&b_s[t * 16 + i16][g * 8]);
    acc[t] = mfma16(afrag, bfrag, acc[t]);
  }
}

// bf16 store of the wave's 16 x 64 C fragments: local row r0 + g*4 + r goes
// to dst[(row_base + row) * ld + col0 + t*16 + i16] when row < nrows
DEVINL void gg_store_c(bf16* __restrict__ dst, long row_base, int ld,
                       int r0, int nrows, int col0, int i16, int g,
                       const f32x4 (&acc)[4]) {
  #pragma unroll
  for (int t = 0; t < 4; t++) {
    #pragma unroll
    for (int r = 0; r < 4; r++) {
      int row = r0 + g * 4 + r;
      if (row < nrows)
        dst[(row_base + row) * (long)ld + col0 + t * 16 + i16] =
            __float2bfloat16(acc[t][r]);
    }
  }
}

// ------------------------------------------------------------- forward
// tiles[0..3)[blockIdx.x] = (expert, m0, n0), host-built from the (already
// host-known) expert token counts
__global__ __launch_bounds__(256, 2) void grouped_gemm_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    bf16* __restrict__ out,
    const int* __restrict__ tile_expert, const int* __restrict__ tile_m0,
    const int* __restrict__ tile_n0, const long* __restrict__ seg_start,
    const int* __restrict__ seg_len, int K, int N, long w_estride) {
  const int e = tile_expert[blockIdx.x];
  const int m0 = tile_m0[blockIdx.x];
  const int n0 = tile_n0[blockIdx.x];
  const long s0 = seg_start[e];
  const int M = seg_len[e];
  const auto [lane, wv, i16, g] = mfma_lane();

  __shared__ gg_tile_t a_s, b_s;

  f32x4 acc[4];
  #pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = {0.f, 0.f, 0.f, 0.f};

  const long wbase = (long)e * w_estride;
  for (int k0 = 0; k0 < K; k0 += GG_TK) {
    __syncthreads();
    // stage A: 64 rows x 32 k (256 threads x 8 elems = 2048 = 64*32)
    {
      int idx = threadIdx.x;  // 256 threads, each 8 elems: 2048/8=256 slots
      int row = idx / 4;
      int col8 = (idx % 4) * 8;
      bf16x8 va = {};
      if (m0 + row < M)
        va = *(const bf16x8*)(x + (s0 + m0 + row) * (long)K + k0 + col8);
      *(bf16x8*)(&a_s[row][col8]) = va;
      // stage B: W[e][n0+row][k0+col8]
      bf16x8 vb = *(const bf16x8*)(w + wbase + (long)(n0 + row) * K + k0 + col8);
      *(bf16x8*)(&b_s[row][col8]) = vb;
    }
    __syncthreads();
    gg_mma_step(a_s, b_s, wv, i16, g, acc);
  }
  gg_store_c(out, s0, N, m0 + wv * 16, M, n0, i16, g, acc);
}

// ---------------------------------------------------------------- dX
// dX[m, k] = sum_n dOut[m, n] * W[e][n, k]
// a_s: dOut tile [64 m][32 n] staged directly (n contiguous in memory).
// wt_s: W^T tile [64 k][32 n] staged transposed from W rows (k contig).
__global__ __launch_bounds__(256, 2) void grouped_gemm_dx_kernel(
    const bf16* __restrict__ dout, const bf16* __restrict__ w,
    bf16* __restrict__ dx,
    const int* __restrict__ tile_expert, const int* __restrict__ tile_m0,
    const int* __restrict__ tile_k0, const long* __restrict__ seg_start,
    const int* __restrict__ seg_len, int K, int N, long w_estride) {
  const int e = tile_expert[blockIdx.x];
  const int m0 = tile_m0[blockIdx.x];
  const int k0 = tile_k0[blockIdx.x];
  const long s0 = seg_start[e];
  const int M = seg_len[e];
  const auto [lane, wv, i16, g] = mfma_lane();

  __shared__ gg_tile_t a_s, wt_s;

  f32x4 acc[4];
  #pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = {0.f, 0.f, 0.f, 0.f};

  const long wbase = (long)e * w_estride;
  for (int n0 = 0; n0 < N; n0 += GG_TK) {
    __syncthreads();
    {
      // A: 64 rows x 32 n, 8 elems/thread (n contiguous)
      int row = threadIdx.x >> 2;           // 0..63
      int c0 = (threadIdx.x & 3) * 8;       // 0,8,16,24
      bf16x8 va = {};
      if (m0 + row < M)
        va = *(const bf16x8*)(dout + (s0 + m0 + row) * (long)N + n0 + c0);
      *(bf16x8*)(&a_s[row][c0]) = va;
      // W^T: read 32 n-rows x 64 k (k contiguous), store transposed
      int nl = threadIdx.x >> 3;            // 0..31
      int kc0 = (threadIdx.x & 7) * 8;      // 0..56
      bf16x8 vw = *(const bf16x8*)(w + wbase + (long)(n0 + nl) * K + k0 + kc0);
      #pragma unroll
      for (int j = 0; j < 8; j++) wt_s[kc0 + j][nl] = vw[j];
    }
    __syncthreads();
    gg_mma_step(a_s, wt_s, wv, i16, g, acc);
  }
  gg_store_c(dx, s0, K, m0 + wv * 16, M, k0, i16, g, acc);
}

// ---------------------------------------------------------------- dW
// dW[e][n, k] = sum_{m in seg_e} dOut[s0+m, n] * x[s0+m, k]
// Both operands are m-strided: stage both tiles transposed.
// Grid is REGULAR: blockIdx -> (e, n-tile, k-tile); the m loop walks the
// whole segment so each workgroup owns its output tile exclusively.
__global__ __launch_bounds__(256, 2) void grouped_gemm_dw_kernel(
    const bf16* __restrict__ dout, const bf16* __restrict__ x,
    bf16* __restrict__ dw, const long* __restrict__ seg_start,
    const int* __restrict__ seg_len, int K, int N, int nt_n, int nt_k) {
  const int e = blockIdx.x / (nt_n * nt_k);
  const int rem = blockIdx.x % (nt_n * nt_k);
  const int n0 = (rem / nt_k) * GG_TM;
  const int k0 = (rem % nt_k) * GG_TN;
  const long s0 = seg_start[e];
  const int M = seg_len[e];
  const auto [lane, wv, i16, g] = mfma_lane();

  __shared__ gg_tile_t dot_s, xt_s;

  f32x4 acc[4];
  #pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = {0.f, 0.f, 0.f, 0.f};

  for (int m0 = 0; m0 < M; m0 += GG_TK) {
    __syncthreads();
    {
      // stage dOut^T tile [64 n][32 m] and x^T tile [64 k][32 m]:
      // read 32 m-rows (contiguous n / k), scatter-store transposed
      int ml = threadIdx.x >> 3;            // 0..31
      int c0 = (threadIdx.x & 7) * 8;       // 0..56
      bf16x8 vd = {}, vx = {};
      if (m0 + ml < M) {
        vd = *(const bf16x8*)(dout + (s0 + m0 + ml) * (long)N + n0 + c0);
        vx = *(const bf16x8*)(x + (s0 + m0 + ml) * (long)K + k0 + c0);
      }
      #pragma unroll
      for (int j = 0; j < 8; j++) {
        dot_s[c0 + j][ml] = vd[j];
        xt_s[c0 + j][ml] = vx[j];
      }
    }
    __syncthreads();
    gg_mma_step(dot_s, xt_s, wv, i16, g, acc);
  }
  // rows are n of dW[e]; N is a multiple of the tile, so none is cut
  gg_store_c(dw, (long)e * N, K, n0 + wv * 16, N, k0, i16, g, acc);
}

// ---------------------------------------------------------------- hosts
struct GgSegs {
  torch::Tensor lens;              // [E] int32, host
  torch::Tensor start_d, len_d;    // [E] int64 / int32, device
};

// seg_lens_cpu -> checked segment starts (E entries summing to total)
static GgSegs gg_segments(const torch::Tensor& seg_lens_cpu, long E,
                          long total, torch::Device dev) {
  GgSegs s;
  s.lens = seg_lens_cpu.to(torch::kInt).cpu().contiguous();
  TORCH_CHECK(s.lens.numel() == E, "seg_lens: ", s.lens.numel(), " vs ", E,
              " experts");
  const int* lp = s.lens.data_ptr<int>();
  std::vector<long> starts(E);
  long off = 0;
  for (long e = 0; e < E; e++) { starts[e] = off; off += lp[e]; }
  TORCH_CHECK(off == total, off, " vs ", total);
  s.start_d = torch::from_blob(starts.data(), {E}, torch::kLong).to(dev);
  s.len_d = s.lens.to(dev);
  return s;
}

// [3, ntiles] int32 on dev: (expert, row0, col0) of every 64 x 64 output
// tile of every segment, ncols wide; ntiles may be 0 (nothing uploaded)
static torch::Tensor gg_tile_list(const torch::Tensor& lens, int ncols,
                                  torch::Device dev) {
  const int* lp = lens.data_ptr<int>();
  std::vector<int> te, tr, tc;
  for (int e = 0; e < (int)lens.numel(); e++)
    for (int r0 = 0; r0 < lp[e]; r0 += GG_TM)
      for (int c0 = 0; c0 < ncols; c0 += GG_TN) {
        te.push_back(e);
        tr.push_back(r0);
        tc.push_back(c0);
      }
  const long nt = te.size();
  te.insert(te.end(), tr.begin(), tr.end());
  te.insert(te.end(), tc.begin(), tc.end());
  if (nt == 0) return torch::empty({3, 0}, torch::kInt);
  return torch::from_blob(te.data(), {3, nt}, torch::kInt).to(dev);
}

torch::Tensor grouped_gemm(torch::Tensor x, torch::Tensor w,
                           torch::Tensor seg_lens_cpu) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16);
  // w may be an expert-strided view of the flat buffer: stride(1) == K,
  // stride(2) == 1, stride(0) arbitrary
  TORCH_CHECK(w.dim() == 3 && x.is_contiguous());
  TORCH_CHECK(w.stride(2) == 1 && w.stride(1) == w.size(2));
  long total = x.size(0);
  int K = x.size(1);
  int E = w.size(0), N = w.size(1);
  TORCH_CHECK(w.size(2) == K);
  TORCH_CHECK(K % GG_TK == 0 && N % GG_TN == 0,
              "grouped_gemm needs K%32==0 and N%64==0, got ", K, " ", N);
  auto segs = gg_segments(seg_lens_cpu, E, total, x.device());
  auto tiles = gg_tile_list(segs.lens, N, x.device());
  auto out = torch::empty({total, (long)N}, x.options());
  const long nt = tiles.size(1);
  if (nt == 0) return out;
  const int* tp = tiles.data_ptr<int>();
  hipLaunchKernelGGL(grouped_gemm_kernel, dim3((unsigned)nt), dim3(256),
    0, cur_stream(), (const bf16*)x.data_ptr(), (const bf16*)w.data_ptr(),
    (bf16*)out.data_ptr(), tp, tp + nt, tp + 2 * nt,
    segs.start_d.data_ptr<long>(), segs.len_d.data_ptr<int>(), K, N,
    (long)w.stride(0));
  CHECK_CUDA_OK();
  return out;
}

torch::Tensor grouped_gemm_dx(torch::Tensor dout, torch::Tensor w,
                              torch::Tensor seg_lens_cpu) {
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(w.dim() == 3 && dout.is_contiguous());
  TORCH_CHECK(w.stride(2) == 1 && w.stride(1) == w.size(2));
  long total = dout.size(0);
  int N = dout.size(1);
  int E = w.size(0), K = w.size(2);
  TORCH_CHECK(w.size(1) == N);
  TORCH_CHECK(N % GG_TK == 0 && K % GG_TN == 0,
              "grouped_gemm_dx needs N%32==0 and K%64==0, got ", N, " ", K);
  auto segs = gg_segments(seg_lens_cpu, E, total, dout.device());
  auto tiles = gg_tile_list(segs.lens, K, dout.device());
  auto dx = torch::empty({total, (long)K}, dout.options());
  const long nt = tiles.size(1);
  if (nt == 0) return dx;
  const int* tp = tiles.data_ptr<int>();
  hipLaunchKernelGGL(grouped_gemm_dx_kernel, dim3((unsigned)nt),
    dim3(256), 0, cur_stream(), (const bf16*)dout.data_ptr(),
    (const bf16*)w.data_ptr(), (bf16*)dx.data_ptr(), tp, tp + nt,
    tp + 2 * nt, segs.start_d.data_ptr<long>(), segs.len_d.data_ptr<int>(),
    K, N, (long)w.stride(0));
  CHECK_CUDA_OK();
  return dx;
}

torch::Tensor grouped_gemm_dw(torch::Tensor dout, torch::Tensor x,
                              torch::Tensor seg_lens_cpu, long E) {
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(dout.is_contiguous() && x.is_contiguous());
  long total = dout.size(0);
  int N = dout.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == total);
  TORCH_CHECK(N % GG_TM == 0 && K % GG_TN == 0,
              "grouped_gemm_dw needs N%64==0 and K%64==0, got ", N, " ", K);
  auto segs = gg_segments(seg_lens_cpu, E, total, dout.device());
  auto dw = torch::empty({E, (long)N, (long)K}, dout.options());
  int nt_n = N / GG_TM, nt_k = K / GG_TN;
  hipLaunchKernelGGL(grouped_gemm_dw_kernel,
    dim3((unsigned)(E * nt_n * nt_k)), dim3(256), 0, cur_stream(),
    (const bf16*)dout.data_ptr(), (const bf16*)x.data_ptr(),
    (bf16*)dw.data_ptr(), segs.start_d.data_ptr<long>(),
    segs.len_d.data_ptr<int>(), K, N, nt_n, nt_k);
  CHECK_CUDA_OK();
  return dw;
}
