// LM-head log-prob statistics without logits (gfx950): a dense bf16 MFMA
// GEMM h [n, H] x W^T [H, v_local] whose epilogue is the online
// log-sum-exp of logprob.hip.  The only thing it writes is (target, rowmax,
// sumexp), fp32 [n] each, with the meaning of vocab_logprob_fwd taken over
// the warped logit x = warp(h . w^T): fp32 accumulation, the optional
// gemma-2 cap (softcap_tanh of common.h), then * inv_temperature.  No logit
// is rounded to bf16 and none reaches memory.
//
// Work split.  A workgroup (256 threads, waves 2 x 2) owns HL_BM = 128 rows
// and one vocab split; it walks the 128-column vocab tiles of its split,
// runs the K loop over H in steps of 64 for each, and folds the finished
// tile into per-row (m, s, target) state that stays in registers across
// tiles.  A wave holds 64 x 64 of C as 16 f32x4 fragments; the lane map is
// mfma.h's, W [V, H] is already its "rows = n, cols = k" form, so both
// operands are plain row-major LDS tiles (pad 8) read 16 bytes per
// fragment, no transpose anywhere.
//
// Grid.  blockIdx.x = row block (fastest), blockIdx.y = vocab split: the
// workgroups that stream the same W tiles are co-resident and W comes from
// L2/MALL after its first read.  Split heuristic (hl_plan): the device
// holds slots = 2 * CUs workgroups; nsplit = floor(slots / row_blocks),
// at least 1, at most min(64, vocab tiles), then shrunk so that no split
// is empty.  One wave of workgroups, no tail; the cap of 64 bounds the
// workspace to 64 * 3 * n floats.
//
// Pipeline.  Global -> register -> LDS, 16 B per lane, two LDS stages and
// two register sets.  Step i (stage i & 1) issues the loads of step i + 2
// into the register set that step i - 1 emptied, pinned in front of the
// MFMAs with sched_barrier as in sg_slice, runs the 32 MFMAs of step i,
// then moves the set loaded during step i - 1 to the other LDS stage: that
// wait is vmcnt(8), the newest loads stay in flight, and the steady state
// has no vmcnt(0).  The load stream runs over (tile, k) pairs, so it
// crosses tile boundaries and the epilogue of a tile hides under it.  One
// barrier per step.  LDS: 2 stages x 2 operands x 128 x 72 bf16 = 72 KB
// plus 2 KB of labels and merge space: two workgroups per CU.
//
// Edges.  Rows >= n and W rows >= v_local are loaded from a clamped index
// (no branch around a load) and never contribute: such columns are -inf in
// the epilogue, such rows are not written.  A K tail (H % 64 != 0) is
// loaded from a clamped k and zero-filled on its way into LDS.  H % 8 == 0
// and bf16 are required; the host routes the rest elsewhere.
//
// Epilogue.  A lane keeps (m, s, target) for each of its 16 C rows over
// the columns it holds and rescales once per row and tile, with
// logprob.hip's -inf rule: a state whose max is still -inf contributes 0
// and (-inf) - (-inf) is never evaluated.  The target is picked from the
// register of the lane that holds column label - vocab_start; the label
// never becomes an address and one outside [0, v_local) leaves target 0.
// Only at the end of the split are the 16 lanes of a row merged by
// shuffle, then the two column waves through LDS in a fixed order.  The
// per-split results go to a workspace [nsplit, 3, n]; head_logprob_merge
// folds them in split order and writes (0, 0, 1) for ignored rows.  No
// atomics anywhere: two runs give the same bits.
#include "mfma.h"

#include <cstdint>

#define HL_THREADS 256
#define HL_BM 128
#define HL_BN 128
#define HL_BK 64
#define HL_PITCH (HL_BK + 8)
#define HL_NLD 4          // 16-byte chunks per thread, operand and step
#define HL_MAX_SPLIT 64

typedef __bf16 hl_tile_t[HL_BM][HL_PITCH];

struct HlArgs {
  const bf16* h;
  const bf16* w;
  const long* labels;
  float* ws;              // [nsplit, 3, n]
  long w_stride;          // elements between W rows
  long vocab_start;
  int n, H, v_local;
  int tiles_per_split, ntiles;
  float inv_temp, cap_scale, ncap;  // cap_scale = softcap * inv_temp
};

// one (vocab tile, k step) position of a stream; wraps inside the split and
// stops at its last position, so a prefetch past the end re-reads that one
struct HlPos {
  int tile, ks;
  DEVINL void advance(int nk, int tile_end) {
    const bool last = tile == tile_end - 1 && ks == nk - 1;
    const bool wrap = ks == nk - 1;
    if (!last) { tile = wrap ? tile + 1 : tile; ks = wrap ? 0 : ks + 1; }
  }
};

__global__ __launch_bounds__(HL_THREADS, 2) void head_logprob_kernel(HlArgs p) {
  __shared__ hl_tile_t a_s[2], b_s[2];
  __shared__ int lbl_s[HL_BM];
  __shared__ float red_s[2][64][3];

  const MfmaLane ml = mfma_lane();  // plain ints: the lambdas capture them
  const int wave = ml.wave, i16 = ml.i16, g = ml.g;
  const int tid = threadIdx.x;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = blockIdx.x * HL_BM;
  const int tile0 = blockIdx.y * p.tiles_per_split;
  const int tile_end = min(tile0 + p.tiles_per_split, p.ntiles);
  const int nk = (p.H + HL_BK - 1) / HL_BK;
  const int total = (tile_end - tile0) * nk;
  const bool capped = p.ncap != 0.f;

  // the lane's local label index per row of the block, -1 = not in the slice
  if (tid < HL_BM) {
    const long ll = p.labels[min(m0 + tid, p.n - 1)] - p.vocab_start;
    lbl_s[tid] = (ll >= 0 && ll < (long)p.v_local) ? (int)ll : -1;
  }

  // load geometry: chunk c of a 128 x 64 tile is row (tid >> 3) + 32 c,
  // elements (tid & 7) * 8 .. + 8
  const int lrow = tid >> 3, lcol = (tid & 7) * 8;

  bf16x8 ra[2][HL_NLD], rb[2][HL_NLD];
  bool kval[2];
  HlPos lp = {tile0, 0};
  auto issue = [&](auto P) __attribute__((always_inline)) {
    constexpr int S = decltype(P)::value;
    const int k = lp.ks * HL_BK + lcol;
    kval[S] = k < p.H;
    const int kc = min(k, p.H - 8);
    // uniform 64-bit tile bases, 32-bit lane offsets inside the tile (the
    // host bounds H and the W row stride so that 128 rows fit)
    const int v0 = lp.tile * HL_BN;
    const char* ab = (const char*)(p.h + (long)m0 * p.H);
    const char* wb = (const char*)(p.w + (long)v0 * p.w_stride);
    #pragma unroll
    for (int c = 0; c < HL_NLD; c++) {
      const int r = min(lrow + 32 * c, p.n - 1 - m0);
      ra[S][c] = *(const bf16x8*)(ab + (unsigned)(r * p.H + kc) * 2u);
    }
    #pragma unroll
    for (int c = 0; c < HL_NLD; c++) {
      const int r = min(lrow + 32 * c, p.v_local - 1 - v0);
      rb[S][c] = *(const bf16x8*)(wb + (unsigned)(r * (int)p.w_stride + kc) * 2u);
    }
    lp.advance(nk, tile_end);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto stage = [&](auto P) __attribute__((always_inline)) {  // register set S -> LDS stage S
    constexpr int S = decltype(P)::value;
    const bf16x8 zero = {};
    #pragma unroll
    for (int c = 0; c < HL_NLD; c++) {
      *(bf16x8*)(&a_s[S][lrow + 32 * c][lcol]) = kval[S] ? ra[S][c] : zero;
      *(bf16x8*)(&b_s[S][lrow + 32 * c][lcol]) = kval[S] ? rb[S][c] : zero;
    }
  };

  f32x4 acc[4][4];
  float m[4][4], s[4][4], tg[4][4];  // [row tile][r]
  #pragma unroll
  for (int i = 0; i < 4; i++) {
    #pragma unroll
    for (int r = 0; r < 4; r++) { m[i][r] = -INFINITY; s[i][r] = 0.f; tg[i][r] = 0.f; }
    #pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  }

  // fold the finished tile `tile` into the running state
  auto fold = [&](int tile) __attribute__((always_inline)) {
    const int c0 = tile * HL_BN + wc * 64 + i16;
    #pragma unroll
    for (int i = 0; i < 4; i++) {
      #pragma unroll
      for (int r = 0; r < 4; r++) {
        const int lbl = lbl_s[wr * 64 + i * 16 + g * 4 + r];
        float x[4];
        #pragma unroll
        for (int j = 0; j < 4; j++) {
          float v = acc[i][j][r];
          const float vc = softcap_tanh(v, p.ncap) * p.cap_scale;
          v = capped ? vc : v * p.inv_temp;  // a select: no branch per logit
          const int col = c0 + j * 16;
          tg[i][r] += col == lbl ? v : 0.f;
          x[j] = col < p.v_local ? v : -INFINITY;
          acc[i][j][r] = 0.f;  // the next tile starts from zero
        }
        const float vm = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        const float mn = fmaxf(m[i][r], vm);
        // while the max is still -inf every term is exp(-inf - 0) = 0:
        // (-inf) - (-inf) is never evaluated and s stays 0
        const float ref = mn > -INFINITY ? mn : 0.f;
        float a = s[i][r] * __expf(m[i][r] - ref);
        #pragma unroll
        for (int j = 0; j < 4; j++) a += __expf(x[j] - ref);
        s[i][r] = a;
        m[i][r] = mn;
      }
    }
  };

  HlPos cp = {tile0, 0};
  // step of parity S: prefetch two ahead, MFMAs of LDS stage S, then the
  // other register set (loaded during the previous step) to the other stage
  auto step = [&](auto P) __attribute__((always_inline)) {
    constexpr int S = decltype(P)::value;
    issue(P);
    #pragma unroll
    for (int kk = 0; kk < HL_BK; kk += 32) {
      bf16x8 af[4], bfr[4];
      #pragma unroll
      for (int i = 0; i < 4; i++)
        af[i] = *(const bf16x8*)(&a_s[S][wr * 64 + i * 16 + i16][kk + g * 8]);
      #pragma unroll
      for (int j = 0; j < 4; j++)
        bfr[j] = *(const bf16x8*)(&b_s[S][wc * 64 + j * 16 + i16][kk + g * 8]);
      #pragma unroll
      for (int i = 0; i < 4; i++) {
        #pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = mfma16(af[i], bfr[j], acc[i][j]);
      }
    }
    if (cp.ks == nk - 1) fold(cp.tile);
    cp.advance(nk, tile_end);
    __builtin_amdgcn_sched_barrier(0);  // the wait for the set stays down here
    stage(std::integral_constant<int, S ^ 1>{});
    __syncthreads();
  };

  const std::integral_constant<int, 0> P0;
  const std::integral_constant<int, 1> P1;
  issue(P0);
  issue(P1);
  stage(P0);
  __syncthreads();
  int it = 0;
  for (; it + 1 < total; it += 2) { step(P0); step(P1); }
  if (it < total) step(P0);

  // lanes of a row -> column waves -> workspace, fixed order
  #pragma unroll
  for (int i = 0; i < 4; i++) {
    #pragma unroll
    for (int r = 0; r < 4; r++) {
      const float gm = group16_max(m[i][r]);
      const float gs = group16_sum(
          m[i][r] > -INFINITY ? s[i][r] * __expf(m[i][r] - gm) : 0.f);
      const float gt = group16_sum(tg[i][r]);
      m[i][r] = gm; s[i][r] = gs; tg[i][r] = gt;
      if (wc == 1 && i16 == 0) {
        float* d = red_s[wr][i * 16 + g * 4 + r];
        d[0] = gm; d[1] = gs; d[2] = gt;
      }
    }
  }
  __syncthreads();
  if (wc == 0 && i16 == 0) {
    float* out = p.ws + (long)blockIdx.y * 3 * p.n;
    #pragma unroll
    for (int i = 0; i < 4; i++) {
      #pragma unroll
      for (int r = 0; r < 4; r++) {
        const int lr = i * 16 + g * 4 + r;
        const int row = m0 + wr * 64 + lr;
        const float* o = red_s[wr][lr];
        const float gm = fmaxf(m[i][r], o[0]);
        float gs = m[i][r] > -INFINITY ? s[i][r] * __expf(m[i][r] - gm) : 0.f;
        gs += o[0] > -INFINITY ? o[1] * __expf(o[0] - gm) : 0.f;
        if (row < p.n) {
          out[row] = tg[i][r] + o[2];
          out[(long)p.n + row] = gm;
          out[2L * p.n + row] = gs;
        }
      }
    }
  }
}

// splits -> (target, rowmax, sumexp), in split order; ignored rows (0, 0, 1)
__global__ __launch_bounds__(256) void head_logprob_merge_kernel(
    const float* __restrict__ ws, const long* __restrict__ labels,
    float* __restrict__ target, float* __restrict__ rowmax,
    float* __restrict__ sumexp, int n, int nsplit, long ignore_index) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  if (labels[row] == ignore_index) {
    target[row] = 0.f; rowmax[row] = 0.f; sumexp[row] = 1.f;
    return;
  }
  float gm = -INFINITY, t = 0.f;
  for (int k = 0; k < nsplit; k++) {
    const float* w = ws + (long)k * 3 * n;
    t += w[row];
    gm = fmaxf(gm, w[(long)n + row]);
  }
  float gs = 0.f;
  for (int k = 0; k < nsplit; k++) {
    const float* w = ws + (long)k * 3 * n;
    const float mk = w[(long)n + row];
    gs += mk > -INFINITY ? w[2L * n + row] * __expf(mk - gm) : 0.f;
  }
  target[row] = t; rowmax[row] = gm; sumexp[row] = gs;
}

// (tiles per split, nsplit) for n rows and v_local columns; want = 0 asks
// for the heuristic of the file header
static std::pair<int, int> hl_plan(long n, long v_local, long want) {
  const long nrb = (n + HL_BM - 1) / HL_BM;
  const long ntiles = (v_local + HL_BN - 1) / HL_BN;
  if (want <= 0) {
    const long slots = 2L * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    want = std::max(1L, slots / nrb);
  }
  want = std::min({want, (long)HL_MAX_SPLIT, ntiles});
  const long tps = (ntiles + want - 1) / want;
  return {(int)tps, (int)((ntiles + tps - 1) / tps)};
}

std::vector<torch::Tensor> head_logprob_fwd(
    torch::Tensor h, torch::Tensor w, torch::Tensor labels, long vocab_start,
    long ignore_index, double inv_temperature, double softcap, long nsplit) {
  TORCH_CHECK(h.is_cuda() && w.is_cuda() && labels.is_cuda(),
              "head_logprob: GPU tensors only");
  TORCH_CHECK(h.scalar_type() == torch::kBFloat16 &&
              w.scalar_type() == torch::kBFloat16,
              "head_logprob: h and w must be bf16");
  TORCH_CHECK(h.dim() == 2 && h.is_contiguous() && w.dim() == 2 &&
              w.size(1) == h.size(1),
              "head_logprob: h [n, H] contiguous, w [v_local, H]");
  const long n = h.size(0), H = h.size(1), V = w.size(0);
  TORCH_CHECK(H >= 8 && H % 8 == 0, "head_logprob: H must be a multiple of 8");
  TORCH_CHECK(w.stride(1) == 1 && w.stride(0) >= H && w.stride(0) % 8 == 0 &&
              (uintptr_t)w.data_ptr() % 16 == 0 &&
              (uintptr_t)h.data_ptr() % 16 == 0,
              "head_logprob: rows of h and w must be 16-byte aligned");
  TORCH_CHECK(labels.scalar_type() == torch::kLong && labels.is_contiguous() &&
              labels.dim() == 1 && labels.size(0) == n,
              "head_logprob: labels must be a contiguous int64 [n] tensor");
  // 128 rows of h or W span fewer than 2^31 bytes: 32-bit in-tile offsets
  TORCH_CHECK(V >= 1 && V < (1L << 31) - HL_BN && n < (1L << 31) - HL_BM &&
              H <= (1L << 22) && w.stride(0) <= (1L << 22),
              "head_logprob: unsupported shape");
  TORCH_CHECK(softcap >= 0.0 && inv_temperature > 0.0,
              "head_logprob: softcap >= 0 and inv_temperature > 0");
  auto opt = h.options().dtype(torch::kFloat);
  auto target = torch::empty({n}, opt);
  auto rowmax = torch::empty({n}, opt);
  auto sumexp = torch::empty({n}, opt);
  if (n == 0) return {target, rowmax, sumexp};

  const auto [tps, ns] = hl_plan(n, V, nsplit);
  auto ws = torch::empty({(long)ns, 3, n}, opt);
  HlArgs a;
  a.h = (const bf16*)h.data_ptr();
  a.w = (const bf16*)w.data_ptr();
  a.labels = (const long*)labels.data_ptr<int64_t>();
  a.ws = ws.data_ptr<float>();
  a.w_stride = w.stride(0);
  a.vocab_start = vocab_start;
  a.n = (int)n; a.H = (int)H; a.v_local = (int)V;
  a.tiles_per_split = tps;
  a.ntiles = (int)((V + HL_BN - 1) / HL_BN);
  a.inv_temp = (float)inv_temperature;
  a.cap_scale = (float)(softcap * inv_temperature);
  a.ncap = softcap_ncap(softcap);
  const dim3 grid((unsigned)((n + HL_BM - 1) / HL_BM), (unsigned)ns);
  hipLaunchKernelGGL(head_logprob_kernel, grid, dim3(HL_THREADS), 0,
                     cur_stream(), a);
  CHECK_CUDA_OK();
  hipLaunchKernelGGL(head_logprob_merge_kernel,
    dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cur_stream(),
    (const float*)ws.data_ptr<float>(), a.labels, target.data_ptr<float>(),
    rowmax.data_ptr<float>(), sumexp.data_ptr<float>(), (int)n, ns,
    ignore_index);
  CHECK_CUDA_OK();
  return {target, rowmax, sumexp};
}
