// Flash-attention packed-varlen causal forward for gfx950 (MFMA).
// Replaces flash_attn_varlen_func in the reference training/prefill path
// (reference: realhf/impl/model/modules/attn.py:255).
//
// Structure (correctness-first instance of the guide's §B prefill recipe):
//   grid = (q_block, q_head); workgroup = 512 threads = 8 waves.
//   Each workgroup owns 128 query rows of one sequence+head (wave w: 16
//   rows) so the cooperative K/V staging amortizes over 2x the MFMA work.
//   KV tiles of 64 keys are staged cooperatively in LDS — K row-major
//   [64][136] (8-elem pad), V row-major [64][144], read by the PV stage
//   through the tr16 hardware transpose.  Online softmax state (m, l) is
//   held per C-row in registers, reduced with shfl_xor over the 16-lane
//   column groups.
//
// MFMA: v_mfma_f32_16x16x32_bf16; lane maps, fragment reads and the
// block mapping are in mfma.h (`mfma_probe` / `tr16_probe` below verify
// them numerically on device).
#include "mfma.h"

#define QBLK 128     // queries per workgroup (8 waves x 16 rows)
#define AV_WAVES 8
#define QW 16        // queries per wave
#define KVBLK 64     // keys per LDS tile
#define KPAD 8       // K tile row pad (bf16 elems)
#define VPAD 8       // P tile row pad
// V stays ROW-major: the PV B-fragment is gathered by the hardware
// transpose read (tr16_bfrag, mfma.h).  16 elems of row pad keep the four
// row-steps on distinct bank sets.
#define VROWPAD 16

// One kernel, two staging schemes (DB).  Everything but the staging and
// its barriers — block mapping, Q fragments, the per-tile S/softmax/PV body,
// the epilogue — is written once.  It is one kernel body and not a set of
// inlined helper functions on purpose: behind a function boundary the tile
// body compiles to different code for the default scheme (hd=64: 95 -> 98
// VGPRs, 5 -> 4 waves/SIMD); `if constexpr` leaves it untouched.
//
// DB = false (default): each 64-key tile is staged into one LDS buffer
// between two barriers, and a third barrier separates the P store from PV.
//
// DB = true: double-buffered long-context variant.  KV tiles ping-pong
// through two LDS buffers; tile i+1's global loads issue BEFORE tile i's
// compute and the LDS writes land after it, so the HBM/L2 stream overlaps
// the MFMA+softmax phases and the per-tile barriers collapse to one.
// ~90 KB LDS (2x KV tiles + P), still one workgroup per CU.  MEASURED
// SLOWER at every shape (317 vs 387 TF/s at 32k): the staging registers +
// larger LDS hurt more than the saved barrier+overlap help.  Kept behind
// REALHF_AMD_ATTN_DB=1 as the baseline for future pipelining work;
// default always uses the single-buffer scheme.
//
// HD = 256 (gemma) is instantiated for DB = false only: 85 KB of LDS
// (K 33 KB + V 34 KB + P 18 KB), 64 accumulator VGPRs per lane.  Two KV
// buffers plus P would be ~156 KB of the 160 KB LDS, so REALHF_AMD_ATTN_DB
// is ignored at 256.
//
// CAP = true is the soft-capped form (gemma-2): the scaled score becomes
// softcap * tanh(score / softcap) before the masks.  It is a template
// parameter and not a branch on the argument because the branch alone moved
// the register allocation of the uncapped hd=64 kernel (95 -> 96 VGPRs);
// CAP = false compiles to the code it was.  Instantiated for DB = false only.
template <int HD, bool DB, bool CAP = false>
__global__ __launch_bounds__(64 * AV_WAVES, 1) void attn_varlen_fwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const int* __restrict__ cu_seqlens,
    const int* __restrict__ blk_offsets, int n_seqs,
    bf16* __restrict__ out, float* __restrict__ lse,
    int nq, int nkv, float scale, bool causal, int window,
    float softcap, float ncap) {
  constexpr int HDCH = HD / 32;  // mfma K-chunks over head_dim
  constexpr int NBUF = DB ? 2 : 1;
  const int blk = blockIdx.x;
  if (blk >= blk_offsets[n_seqs]) return;  // over-provisioned grid tail
  const int qh = blockIdx.y;
  const int kvh = qh / (nq / nkv);
  const int seq = blk_lookup(blk_offsets, n_seqs, blk);
  const int q0_local = (blk - blk_offsets[seq]) * QBLK;  // local query start
  const int s0 = cu_seqlens[seq], s1 = cu_seqlens[seq + 1];
  const int L = s1 - s0;
  const auto [lane, w, i16, g] = mfma_lane();

  __shared__ __bf16 k_s[NBUF][KVBLK][HD + KPAD];
  __shared__ __bf16 v_s[NBUF][KVBLK][HD + VROWPAD];
  __shared__ __bf16 p_s[AV_WAVES][QW][KVBLK + VPAD];

  // ---- load Q fragments (registers, whole kernel) --------------------
  // wave w owns query rows qrow_local = q0_local + w*QW + i16 (A layout)
  bf16x8 qfrag[HDCH];
  const int my_qrow_a = q0_local + w * QW + i16;  // A-layout row
  {
    const bf16* qrow = q + ((long)(s0 + min(my_qrow_a, L - 1)) * nq + qh) * HD;
    #pragma unroll
    for (int c = 0; c < HDCH; c++)
      qfrag[c] = *(const bf16x8*)(qrow + c * 32 + g * 8);
  }

  // online state for the 4 C-rows this lane touches
  float m_r[4], l_r[4];
  f32x4 o_acc[HD / 16];
  #pragma unroll
  for (int r = 0; r < 4; r++) { m_r[r] = -1e30f; l_r[r] = 0.f; }
  #pragma unroll
  for (int t = 0; t < HD / 16; t++) o_acc[t] = {0.f, 0.f, 0.f, 0.f};

  // causal: keys needed up to q0_local + QBLK - 1 (inclusive); else all L
  const int kv_end = causal ? min(L, q0_local + QBLK) : L;
  // sliding window (mistral): query qrow sees keys (qrow-window, qrow];
  // the workgroup's earliest needed key is q0_local - window + 1
  int kv_begin = 0;
  if (window > 0) {
    kv_begin = q0_local - window + 1;
    kv_begin = (kv_begin > 0) ? (kv_begin / KVBLK) * KVBLK : 0;
  }

  // DB only: each thread holds SLOTS 8-elem groups of the next 64 x HD
  // tile per tensor in registers while the current tile computes
  constexpr int SLOTS = DB ? (KVBLK * (HD / 8) + 64 * AV_WAVES - 1) /
                                 (64 * AV_WAVES)
                           : 1;
  bf16x8 kreg[SLOTS], vreg[SLOTS];
  auto load_tile = [&](int kv0) {
    #pragma unroll
    for (int s = 0; s < SLOTS; s++) {
      int idx = threadIdx.x + s * 64 * AV_WAVES;
      if (idx >= KVBLK * (HD / 8)) break;
      int row = idx / (HD / 8);
      int col8 = (idx % (HD / 8)) * 8;
      bf16x8 kv8 = {}, vv8 = {};
      if (row < kv_end - kv0) {
        kv8 = *(const bf16x8*)(k + ((long)(s0 + kv0 + row) * nkv + kvh) * HD + col8);
        vv8 = *(const bf16x8*)(v + ((long)(s0 + kv0 + row) * nkv + kvh) * HD + col8);
      }
      kreg[s] = kv8;
      vreg[s] = vv8;
    }
  };
  auto store_tile = [&](int buf) {
    #pragma unroll
    for (int s = 0; s < SLOTS; s++) {
      int idx = threadIdx.x + s * 64 * AV_WAVES;
      if (idx >= KVBLK * (HD / 8)) break;
      int row = idx / (HD / 8);
      int col8 = (idx % (HD / 8)) * 8;
      *(bf16x8*)(&k_s[buf][row][col8]) = kreg[s];
      *(bf16x8*)(&v_s[buf][row][col8]) = vreg[s];
    }
  };
  if constexpr (DB) {
    load_tile(kv_begin);
    store_tile(0);
    __syncthreads();
  }

  int cur = 0;  // LDS buffer holding this tile (always 0 without DB)
  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += KVBLK) {
    if constexpr (DB) {
      if (kv0 + KVBLK < kv_end)
        load_tile(kv0 + KVBLK);  // global loads in flight during compute
    } else {
      const int kchunk = min(KVBLK, kv_end - kv0);
      // ---- stage K and V tiles -------------------------------------
      __syncthreads();
      // 64 rows x HD; all waves stage cooperatively, 16B per thread
      for (int idx = threadIdx.x; idx < KVBLK * (HD / 8); idx += 64 * AV_WAVES) {
        int row = idx / (HD / 8);
        int col8 = (idx % (HD / 8)) * 8;
        bf16x8 val = {};
        bf16x8 vv = {};
        if (row < kchunk) {
          val = *(const bf16x8*)(k + ((long)(s0 + kv0 + row) * nkv + kvh) * HD + col8);
          vv = *(const bf16x8*)(v + ((long)(s0 + kv0 + row) * nkv + kvh) * HD + col8);
        }
        *(bf16x8*)(&k_s[0][row][col8]) = val;
        *(bf16x8*)(&v_s[0][row][col8]) = vv;
      }
      __syncthreads();
    }

    // ---- S = Q K^T over 4 key subtiles ------------------------------
    f32x4 s_sub[4];
    #pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int c = 0; c < HDCH; c++) {
        // B fragment: K[key = ks*16 + i16][c*32 + g*8 + j]
        bf16x8 bfrag = *(const bf16x8*)(&k_s[cur][ks * 16 + i16][c * 32 + g * 8]);
        acc = mfma16(qfrag[c], bfrag, acc);
      }
      s_sub[ks] = acc;
    }

    // ---- softmax over the 64-key tile -------------------------------
    float tile_max[4];
    #pragma unroll
    for (int r = 0; r < 4; r++) {
      float mx = -1e30f;
      const int qrow = q0_local + w * QW + g * 4 + r;  // C-layout row
      #pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        int kidx = kv0 + ks * 16 + i16;
        bool ok = (kidx < kv_end) && (!causal || kidx <= qrow) && (qrow < L)
                  && (window <= 0 || kidx > qrow - window);
        float sv = ok ? s_sub[ks][r] * scale : -1e30f;
        // soft-cap on live scores only: a capped -1e30f sentinel would be
        // -softcap and pass for a live key in `s_sub > -1e29f` below
        if constexpr (CAP) {
          if (ok) sv = softcap * softcap_tanh(sv, ncap);
        }
        s_sub[ks][r] = sv;
        mx = fmaxf(mx, sv);
      }
      tile_max[r] = group16_max(mx);
    }
    #pragma unroll
    for (int r = 0; r < 4; r++) {
      float nm = fmaxf(m_r[r], tile_max[r]);
      if (nm < -1e29f) nm = 0.f;  // fully-masked row guard
      float f = __expf(m_r[r] - nm);
      if (m_r[r] < -1e29f) f = 0.f;
      m_r[r] = nm;
      l_r[r] *= f;
      #pragma unroll
      for (int t = 0; t < HD / 16; t++) o_acc[t][r] *= f;
      float rowsum = 0.f;
      #pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        float p = (s_sub[ks][r] > -1e29f) ? __expf(s_sub[ks][r] - nm) : 0.f;
        s_sub[ks][r] = p;
        rowsum += p;
      }
      l_r[r] += group16_sum(rowsum);
    }
    // ---- P -> LDS (bf16, C layout -> A-readable) --------------------
    #pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      #pragma unroll
      for (int r = 0; r < 4; r++)
        p_s[w][g * 4 + r][ks * 16 + i16] = (__bf16)s_sub[ks][r];
    }
    // p_s is per-wave (written and read by the same wave); the DB scheme
    // relies on same-wave LDS ordering and has no barrier here
    if constexpr (!DB) __syncthreads();

    // ---- O += P V ----------------------------------------------------
    #pragma unroll
    for (int kk = 0; kk < 2; kk++) {  // two K=32 chunks over 64 keys
      // A fragment: P[qrow = i16][kk*32 + g*8 + j]
      bf16x8 pa = *(const bf16x8*)(&p_s[w][i16][kk * 32 + g * 8]);
      const int krow0 = kk * 32 + g * 8 + (i16 >> 2);
      const int vcol4 = (i16 & 3) * 4;
      #pragma unroll
      for (int t = 0; t < HD / 16; t++) {
        // B fragment as in tr16_bfrag (mfma.h), on the typed tile: through
        // the helper's flat pointer the LDS offsets fold differently and
        // the register allocation of this kernel changes
        bf16x4 r0 = tr16_read(&v_s[cur][krow0][t * 16 + vcol4]);
        bf16x4 r1 = tr16_read(&v_s[cur][krow0 + 4][t * 16 + vcol4]);
        bf16x8 vb;
        #pragma unroll
        for (int j = 0; j < 4; j++) { vb[j] = r0[j]; vb[4 + j] = r1[j]; }
        o_acc[t] = mfma16(pa, vb, o_acc[t]);
      }
    }

    if constexpr (DB) {
      if (kv0 + KVBLK < kv_end) {
        store_tile(cur ^ 1);  // other buffer: no hazard with this tile
        __syncthreads();      // publish before every wave's next S phase
      }
      cur ^= 1;
    }
  }

  // ---- epilogue ------------------------------------------------------
  #pragma unroll
  for (int r = 0; r < 4; r++) {
    const int qrow = q0_local + w * QW + g * 4 + r;
    if (qrow >= L) continue;
    float inv = (l_r[r] > 0.f) ? 1.f / l_r[r] : 0.f;
    bf16* orow = out + ((long)(s0 + qrow) * nq + qh) * HD;
    #pragma unroll
    for (int t = 0; t < HD / 16; t++)
      orow[t * 16 + i16] = __float2bfloat16(o_acc[t][r] * inv);
    if (lse && i16 == 0)
      lse[(long)(s0 + qrow) * nq + qh] = m_r[r] + __logf(fmaxf(l_r[r], 1e-30f));
  }
}

static int attn_db_mode() {
  static int v = [] {
    const char* e = getenv("REALHF_AMD_ATTN_DB");
    return e ? atoi(e) : 0;  // default: single-buffer (db measured slower)
  }();
  return v;
}

std::vector<torch::Tensor> attn_varlen_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor cu_seqlens, long max_seqlen, bool causal, double scale,
    long window, double softcap) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16,
              "attn_varlen_fwd: bf16 only");
  TORCH_CHECK(softcap >= 0.0, "attn_varlen_fwd: softcap must be >= 0");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  int total = q.size(0), nq = q.size(1), hd = q.size(2);
  int nkv = k.size(1);
  TORCH_CHECK(nq % nkv == 0);
  auto cu_dev = cu_seqlens.to(torch::kInt).to(q.device());
  int bs = cu_dev.numel() - 1;
  auto blk_off = build_blk_offsets<QBLK>(cu_dev);
  auto out = torch::empty_like(q);
  auto lse = torch::empty({total, nq}, q.options().dtype(torch::kFloat));
  // upper bound on sum(ceil(L/QBLK)) — real tail blocks exit on the
  // device-side count, no host sync anywhere
  dim3 grid((unsigned)(total / QBLK + bs), nq);
  int dbm = attn_db_mode();
  bool use_db = (dbm == 1) || (dbm == -1 && max_seqlen >= 4096);
  TORCH_CHECK(hd == 256 || hd == 128 || hd == 64, "unsupported head_dim ", hd);
#define FW_LAUNCH(HD_, DB_, CAP_)                                         \
  hipLaunchKernelGGL((attn_varlen_fwd_kernel<HD_, DB_, CAP_>), grid,      \
    dim3(64 * AV_WAVES), 0, cur_stream(), (const bf16*)q.data_ptr(),      \
    (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),                 \
    cu_dev.data_ptr<int>(), blk_off.data_ptr<int>(), bs,                  \
    (bf16*)out.data_ptr(), lse.data_ptr<float>(), nq, nkv, (float)scale,  \
    causal, (int)window, (float)softcap,                                  \
    softcap_ncap(softcap))
  if (softcap > 0.0) {  // capped form: single-buffer, whatever ATTN_DB says
    if (hd == 256) FW_LAUNCH(256, false, true);
    else if (hd == 128) FW_LAUNCH(128, false, true);
    else FW_LAUNCH(64, false, true);
  } else if (hd == 256) {
    FW_LAUNCH(256, false, false);  // single-buffer only (LDS), whatever ATTN_DB says
  } else if (hd == 128) {
    if (use_db) FW_LAUNCH(128, true, false); else FW_LAUNCH(128, false, false);
  } else {
    if (use_db) FW_LAUNCH(64, true, false); else FW_LAUNCH(64, false, false);
  }
#undef FW_LAUNCH
  CHECK_CUDA_OK();
  return {out, lse};
}

// ---------------------------------------------------------------------------
// mfma_probe: D = A(16x32) @ B(32x16) with the assumed lane mapping —
// numerics check for the fragment layout (guide §3 "A=I-check with
// ASYMMETRIC B").
// ---------------------------------------------------------------------------
__global__ void mfma_probe_kernel(const bf16* A, const bf16* B, float* D) {
  const auto [lane, w, i16, g] = mfma_lane();
  bf16x8 a, b;
  #pragma unroll
  for (int j = 0; j < 8; j++) {
    a[j] = (__bf16)A[i16 * 32 + g * 8 + j];      // A[i][k] row-major
    b[j] = (__bf16)B[(g * 8 + j) * 16 + i16];    // B[k][n] row-major
  }
  f32x4 c = mfma16(a, b, f32x4{0.f, 0.f, 0.f, 0.f});
  #pragma unroll
  for (int r = 0; r < 4; r++) D[(g * 4 + r) * 16 + i16] = c[r];
}

torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}));
  TORCH_CHECK(B.sizes() == torch::IntArrayRef({32, 16}));
  auto Ac = A.to(torch::kBFloat16).contiguous();
  auto Bc = B.to(torch::kBFloat16).contiguous();
  auto D = torch::zeros({16, 16}, A.options().dtype(torch::kFloat).device(A.device()));
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, cur_stream(),
    (const bf16*)Ac.data_ptr(), (const bf16*)Bc.data_ptr(), D.data_ptr<float>());
  CHECK_CUDA_OK();
  return D;
}

// ---------------------------------------------------------------------------
// tr16_probe: empirical map of tr16_read (mfma.h) — each lane passes
// addr = lds_base + 2*addr_elem[lane] (bf16 elems); the kernel stages
// lds[i] = i and dumps what (lane, j) receives, so the host can derive
// the lane->element mapping for MFMA B-fragment use (guide §2 T10).
// ---------------------------------------------------------------------------
__global__ void tr16_probe_kernel(const int* __restrict__ addr_elem,
                                  float* __restrict__ out) {
  __shared__ __bf16 lds[1024];
  const int lane = mfma_lane().lane;
  for (int i = threadIdx.x; i < 1024; i += 64)
    lds[i] = (__bf16)(float)i;
  __syncthreads();
  bf16x4 r = tr16_read(&lds[addr_elem[lane]]);
  #pragma unroll
  for (int j = 0; j < 4; j++) out[lane * 4 + j] = (float)r[j];
}

torch::Tensor tr16_probe(torch::Tensor addr_elem) {
  auto a = addr_elem.to(torch::kInt).cuda().contiguous();
  TORCH_CHECK(a.numel() == 64);
  auto out = torch::zeros({64, 4}, torch::TensorOptions()
                          .dtype(torch::kFloat).device(a.device()));
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0, cur_stream(),
    a.data_ptr<int>(), out.data_ptr<float>());
  CHECK_CUDA_OK();
  return out;
}
