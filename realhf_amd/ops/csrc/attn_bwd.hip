// Flash-attention packed-varlen causal BACKWARD for gfx950 (MFMA).
// Replaces the batched-GEMM recompute path of _AttnVarlenFn.backward
// (reference counterpart: flash-attn 2's varlen bwd, an external CUDA
// dep of the reference — SURVEY.md §2.2).
//
// kv-stationary: grid = (kv_block, q_head); workgroup = 4 waves; wave w
// owns keys [k0 + 16w, k0 + 16w + 16) of a 64-key block and accumulates
// that slice's dK/dV in MFMA C fragments (16x128 fp32 = 64 VGPR/lane for
// both).  The workgroup loops over 32-query tiles >= the diagonal:
//   S^T = K Q^T               (A = K row frag, B = Q row frag)
//   P^T = exp(S^T*scale - lse[q])      (soft-cap: exp(cap*t - lse[q]),
//                                       t = tanh(S^T*scale / cap))
//   dV += P^T dO              (A = P^T via LDS, B = dO via tr16)
//   dP^T = V dO^T             (A = V row frag, B = dO row frag)
//   dS^T = P^T o (dP^T - D[q]) * scale (soft-cap: * (1 - t^2) too)
//   dK += dS^T Q              (A = dS^T via LDS, B = Q via tr16)
//   dQ += dS K  -> fp32 atomics, or (opt-in: max_seqlen given and the
//                 partials fit) per-kv-block fp32 partials summed in
//                 block order by bw_reduce_dq, bit-reproducible (A = dS
//                 via tr16 of the shared dS^T tile, B = K via tr16; hd
//                 chunks split across waves)
// dK/dV are written per Q-HEAD to fp32 buffers (no atomics); the host
// sums GQA groups.  D = rowsum(dO*O) and the final casts happen in
// torch (fp32).
//
// MFMA lane maps, the tr16 hardware-transpose fragment read and the block
// mapping are in mfma.h (verified by mfma_probe / tr16_probe).
#include "mfma.h"

#define BW_WAVES 4
#define BW_KV 64      // keys per workgroup (16 per wave)
#define BW_QT 32      // queries per tile
#define BW_PAD 8
#define BW_TPAD 16    // pad for tr16-read tiles (bank spread, fwd-proven)
#define BW_DET_MAX_BYTES (2L << 30)  // cap on the deterministic-dQ partials

// Query rows [*qb, *up) of a sequence of length L receive a dQ
// contribution from the kv block starting at key k0 (the q-tile loop of
// attn_varlen_bwd_kernel); false when the block visits no q tile.
DEVINL bool bw_q_range(int k0, int L, bool causal, int window,
                       int* qb, int* up) {
  const int q_begin = causal ? (k0 / BW_QT) * BW_QT : 0;
  const int q_end = (window > 0) ? min(L, k0 + BW_KV + window - 1) : L;
  if (q_end <= q_begin) return false;
  *qb = q_begin;
  *up = q_begin + ((q_end - q_begin + BW_QT - 1) / BW_QT) * BW_QT;
  return true;
}

// Deterministic dQ: dq[row] = sum over the kv blocks that visited the row,
// in ascending block order, of the per-block partials dq_part[slot][...].
// One thread per 4 floats of [total, nq, HD]; only visited (slot, row)
// cells are read, so dq_part needs no zero fill.  nslot comes from the
// caller's max_seqlen; it decides only which blocks are summed in order,
// never whether a contribution is counted.
template <int HD>
__global__ void bw_reduce_dq(const float* __restrict__ part,
                             float* dq,
                             const int* __restrict__ cu, int bs, int total,
                             int nq, int nslot, bool causal, int window) {
  const long n4 = (long)total * nq * (HD / 4);
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n4) return;
  const int row = (int)(idx / ((long)nq * (HD / 4)));
  int lo = 0, hi = bs;  // largest i with cu[i] <= row
  while (lo + 1 < hi) {
    int mid = (lo + hi) >> 1;
    if (cu[mid] <= row) lo = mid; else hi = mid;
  }
  const int s0 = cu[lo], L = cu[lo + 1] - s0, lr = row - s0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (lr >= 0 && lr < L) {
    const int nblk = min((L + BW_KV - 1) / BW_KV, nslot);
    for (int b = 0; b < nblk; b++) {
      int qb, up;
      if (!bw_q_range(b * BW_KV, L, causal, window, &qb, &up)) continue;
      if (lr < qb || lr >= up) continue;
      acc += ((const f32x4*)part)[(long)b * n4 + idx];
    }
  }
  // dq arrives zero-filled except for blocks beyond the last slot (a
  // sequence longer than max_seqlen), which added into it atomically
  ((f32x4*)dq)[idx] = acc + ((const f32x4*)dq)[idx];
}

// HD = 256 (gemma): the dK/dV accumulators alone are 128 registers per lane
// and the tiles take 112 KB of LDS, so that instantiation asks for one
// workgroup per CU; 64/128 keep two.
// CAP = true is the soft-capped form (gemma-2, see attn_varlen.hip); a
// template parameter because a branch on the argument moved the VGPR count of
// every uncapped instantiation.
template <int HD, bool DET, bool CAP = false>
__global__ __launch_bounds__(64 * BW_WAVES, HD > 128 ? 1 : 2)
void attn_varlen_bwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ Dsum,
    const int* __restrict__ cu_seqlens, const int* __restrict__ blk_offsets,
    int n_seqs, float* __restrict__ dq32,
    float* __restrict__ dk32, float* __restrict__ dv32,
    int nq, int nkv, float scale, bool causal, int window,
    float* __restrict__ dq_part, int nslot, long part_stride,
    float softcap, float ncap) {
  constexpr int HDCH = HD / 32;
  const int blk = blockIdx.x;
  if (blk >= blk_offsets[n_seqs]) return;  // over-provisioned grid tail
  const int qh = blockIdx.y;
  const int kvh = qh / (nq / nkv);
  const int seq = blk_lookup(blk_offsets, n_seqs, blk);
  const int k0 = (blk - blk_offsets[seq]) * BW_KV;
  const int s0 = cu_seqlens[seq], s1 = cu_seqlens[seq + 1];
  const int L = s1 - s0;
  const auto [lane, w, i16, g] = mfma_lane();

  __shared__ __bf16 k_s[BW_KV][HD + BW_TPAD];   // row-major; tr16-read too
  __shared__ __bf16 v_s[BW_KV][HD + BW_PAD];
  __shared__ __bf16 q_s[BW_QT][HD + BW_TPAD];   // row-major; tr16-read too
  __shared__ __bf16 do_s[BW_QT][HD + BW_TPAD];
  __shared__ __bf16 pt_s[BW_WAVES][16][BW_QT + BW_PAD];  // P^T per wave
  __shared__ __bf16 ds_all[BW_KV][BW_QT + BW_TPAD];      // dS^T, all waves
  __shared__ float lse_s[BW_QT], d_s[BW_QT];

  // ---- stage the K/V block (whole kernel) ---------------------------
  for (int idx = threadIdx.x; idx < BW_KV * (HD / 8); idx += 64 * BW_WAVES) {
    int row = idx / (HD / 8);
    int col8 = (idx % (HD / 8)) * 8;
    bf16x8 kv = {}, vv = {};
    if (k0 + row < L) {
      kv = *(const bf16x8*)(k + ((long)(s0 + k0 + row) * nkv + kvh) * HD + col8);
      vv = *(const bf16x8*)(v + ((long)(s0 + k0 + row) * nkv + kvh) * HD + col8);
    }
    *(bf16x8*)(&k_s[row][col8]) = kv;
    *(bf16x8*)(&v_s[row][col8]) = vv;
  }
  __syncthreads();

  // wave-resident A fragments of K and V (rows = this wave's 16 keys)
  bf16x8 kfrag[HDCH], vfrag[HDCH];
  #pragma unroll
  for (int c = 0; c < HDCH; c++) {
    kfrag[c] = *(const bf16x8*)(&k_s[w * 16 + i16][c * 32 + g * 8]);
    vfrag[c] = *(const bf16x8*)(&v_s[w * 16 + i16][c * 32 + g * 8]);
  }

  // dK/dV accumulators: C fragments [key16][hd16 chunks]
  f32x4 dk_acc[HD / 16], dv_acc[HD / 16];
  #pragma unroll
  for (int t = 0; t < HD / 16; t++) {
    dk_acc[t] = {0.f, 0.f, 0.f, 0.f};
    dv_acc[t] = {0.f, 0.f, 0.f, 0.f};
  }

  const int q_begin = causal ? (k0 / BW_QT) * BW_QT : 0;
  // sliding window (mistral, fwd-matching semantics: query q sees keys
  // (q-window, q]): key kidx is consumed only by queries < kidx + window,
  // so this kv block's last relevant query is k0 + BW_KV - 1 + window - 1
  const int q_end = (window > 0) ? min(L, k0 + BW_KV + window - 1) : L;
  for (int q0 = q_begin; q0 < q_end; q0 += BW_QT) {
    const int qn = min(BW_QT, L - q0);
    // ---- stage Q/dO tile + lse + D --------------------------------
    __syncthreads();
    for (int idx = threadIdx.x; idx < BW_QT * (HD / 8); idx += 64 * BW_WAVES) {
      int row = idx / (HD / 8);
      int col8 = (idx % (HD / 8)) * 8;
      bf16x8 qv = {}, dv = {};
      if (row < qn) {
        qv = *(const bf16x8*)(q + ((long)(s0 + q0 + row) * nq + qh) * HD + col8);
        dv = *(const bf16x8*)(dout + ((long)(s0 + q0 + row) * nq + qh) * HD + col8);
      }
      *(bf16x8*)(&q_s[row][col8]) = qv;
      *(bf16x8*)(&do_s[row][col8]) = dv;
    }
    if (threadIdx.x < BW_QT) {
      int row = threadIdx.x;
      bool ok = row < qn;
      lse_s[row] = ok ? lse[(long)(s0 + q0 + row) * nq + qh] : 0.f;
      d_s[row] = ok ? Dsum[(long)(s0 + q0 + row) * nq + qh] : 0.f;
    }
    __syncthreads();

    // ---- S^T and dP^T over the two 16-q subtiles -------------------
    f32x4 st[2], dpt[2];
    #pragma unroll
    for (int qs = 0; qs < 2; qs++) {
      f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int c = 0; c < HDCH; c++) {
        bf16x8 qb = *(const bf16x8*)(&q_s[qs * 16 + i16][c * 32 + g * 8]);
        bf16x8 db = *(const bf16x8*)(&do_s[qs * 16 + i16][c * 32 + g * 8]);
        a1 = mfma16(kfrag[c], qb, a1);
        a2 = mfma16(vfrag[c], db, a2);
      }
      st[qs] = a1;
      dpt[qs] = a2;
    }

    // ---- P^T, dS^T (C layout: row = key w*16 + g*4 + r, col = q i16)
    #pragma unroll
    for (int qs = 0; qs < 2; qs++) {
      const int qidx = q0 + qs * 16 + i16;
      #pragma unroll
      for (int r = 0; r < 4; r++) {
        const int kidx = k0 + w * 16 + g * 4 + r;
        bool ok = (kidx < L) && (qidx < L) && (!causal || kidx <= qidx)
                  && (window <= 0 || kidx > qidx - window);
        // soft-cap: the score is c = softcap * t with t = tanh(s * scale /
        // softcap), and dc/ds = (1 - t^2) * scale (exactly 0 at saturation)
        float sv = st[qs][r] * scale, dsc = scale;
        if constexpr (CAP) {
          const float t = softcap_tanh(sv, ncap);
          sv = softcap * t;
          dsc = scale * (1.f - t * t);
        }
        float p = ok ? __expf(sv - lse_s[qs * 16 + i16]) : 0.f;
        float ds = ok ? p * (dpt[qs][r] - d_s[qs * 16 + i16]) * dsc : 0.f;
        pt_s[w][g * 4 + r][qs * 16 + i16] = (__bf16)p;
        ds_all[w * 16 + g * 4 + r][qs * 16 + i16] = (__bf16)ds;
      }
    }
    __syncthreads();

    // ---- dV += P^T dO ; dK += dS^T Q (B fragments via tr16) --------
    {
      // A fragments: k = q dim is 32; the chunks g*8+j span [0,32) ✓
      bf16x8 pa = *(const bf16x8*)(&pt_s[w][i16][g * 8]);
      bf16x8 da = *(const bf16x8*)(&ds_all[w * 16 + i16][g * 8]);
      const int krow0 = g * 8 + (i16 >> 2);
      const int col4 = (i16 & 3) * 4;
      #pragma unroll
      for (int t = 0; t < HD / 16; t++) {
        bf16x8 dob = tr16_bfrag(&do_s[0][0], HD + BW_TPAD, krow0, t * 16 + col4);
        bf16x8 qb = tr16_bfrag(&q_s[0][0], HD + BW_TPAD, krow0, t * 16 + col4);
        dv_acc[t] = mfma16(pa, dob, dv_acc[t]);
        dk_acc[t] = mfma16(da, qb, dk_acc[t]);
      }
    }

    // ---- dQ += dS K (cooperative over hd chunks; DET: plain stores
    // into this kv block's slot, else fp32 atomics) -------------------
    // A = dS[q][key] via tr16 of ds_all (k = LDS row = key, i = col = q,
    // one 16-q column window per qs2); B = K[key][hd] via tr16 of k_s.
    {
      const int col4 = (i16 & 3) * 4;
      #pragma unroll
      for (int qs2 = 0; qs2 < 2; qs2++) {
        #pragma unroll
        for (int t = 0; t < HD / 16; t += 1) {
          if ((t & (BW_WAVES - 1)) != w) continue;  // split chunks by wave
          f32x4 dq_acc = {0.f, 0.f, 0.f, 0.f};
          #pragma unroll
          for (int kc = 0; kc < 2; kc++) {  // two key chunks of 32
            const int krow0 = kc * 32 + g * 8 + (i16 >> 2);
            bf16x8 dsa = tr16_bfrag(&ds_all[0][0], BW_QT + BW_TPAD, krow0,
                                    qs2 * 16 + col4);
            bf16x8 kb = tr16_bfrag(&k_s[0][0], HD + BW_TPAD, krow0,
                                   t * 16 + col4);
            dq_acc = mfma16(dsa, kb, dq_acc);
          }
          #pragma unroll
          for (int r = 0; r < 4; r++) {
            const int qrow = q0 + qs2 * 16 + g * 4 + r;
            if (qrow >= L) continue;
            const long o = ((long)(s0 + qrow) * nq + qh) * HD + t * 16 + i16;
            if (DET) {
              // plain store into this kv block's slot (slot = block index
              // within the sequence); bw_reduce_dq sums slots in order
              const int slot = k0 / BW_KV;
              if (slot < nslot)
                dq_part[(long)slot * part_stride + o] = dq_acc[r];
              else  // sequence longer than max_seqlen promised: stay
                    // correct (no slot to write), only the order is lost
                atomicAdd(&dq32[o], dq_acc[r]);
            } else {
              atomicAdd(&dq32[o], dq_acc[r]);
            }
          }
        }
      }
    }
  }

  // ---- write dK/dV per q-head (fp32, no atomics) --------------------
  __syncthreads();
  #pragma unroll
  for (int r = 0; r < 4; r++) {
    const int kidx = k0 + w * 16 + g * 4 + r;
    if (kidx >= L) continue;
    float* dkrow = dk32 + ((long)(s0 + kidx) * nq + qh) * HD;
    float* dvrow = dv32 + ((long)(s0 + kidx) * nq + qh) * HD;
    #pragma unroll
    for (int t = 0; t < HD / 16; t++) {
      dkrow[t * 16 + i16] = dk_acc[t][r];
      dvrow[t * 16 + i16] = dv_acc[t][r];
    }
  }
}

std::vector<torch::Tensor> attn_varlen_bwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor dout,
    torch::Tensor lse, torch::Tensor Dsum, torch::Tensor cu_seqlens,
    bool causal, double scale, long window, long max_seqlen, double softcap) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(softcap >= 0.0, "attn_varlen_bwd: softcap must be >= 0");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous() &&
              dout.is_contiguous());
  int total = q.size(0), nq = q.size(1), hd = q.size(2);
  int nkv = k.size(1);
  auto cu_dev = cu_seqlens.to(torch::kInt).to(q.device());
  int bs = cu_dev.numel() - 1;
  auto blk_off = build_blk_offsets<BW_KV>(cu_dev);
  auto f32 = q.options().dtype(torch::kFloat);
  // Deterministic dQ needs one [total, nq, hd] fp32 slot per kv block of
  // the longest sequence.  It is opt-in: max_seqlen = 0 (the default)
  // keeps the atomic path and allocates nothing extra.  When the slots
  // would exceed BW_DET_MAX_BYTES (long-context batches) the call also
  // uses atomics, whose summation order varies from run to run.
  const long part_stride = (long)total * nq * hd;
  const long nslot = max_seqlen > 0 ? (max_seqlen + BW_KV - 1) / BW_KV : 0;
  const bool det = nslot > 0 && total > 0 &&
                   nslot * part_stride * 4 <= BW_DET_MAX_BYTES;
  auto dq32 = torch::zeros({(long)total, (long)nq, (long)hd}, f32);
  torch::Tensor dq_part;
  if (det) dq_part = torch::empty({nslot, (long)total, (long)nq, (long)hd}, f32);
  float* part_ptr = det ? dq_part.data_ptr<float>() : nullptr;
  auto dk32 = torch::empty({(long)total, (long)nq, (long)hd}, f32);
  auto dv32 = torch::empty({(long)total, (long)nq, (long)hd}, f32);
  dim3 grid((unsigned)(total / BW_KV + bs), nq);
  TORCH_CHECK(hd == 256 || hd == 128 || hd == 64,
              "attn_varlen_bwd: unsupported head_dim ", hd);
#define BW_LAUNCH_(HD_, DET_, CAP_)                                       \
  hipLaunchKernelGGL((attn_varlen_bwd_kernel<HD_, DET_, CAP_>), grid,     \
    dim3(64 * BW_WAVES), 0, cur_stream(), (const bf16*)q.data_ptr(),      \
    (const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(),                 \
    (const bf16*)dout.data_ptr(), lse.data_ptr<float>(),                  \
    Dsum.data_ptr<float>(), cu_dev.data_ptr<int>(),                       \
    blk_off.data_ptr<int>(), bs,                                          \
    dq32.data_ptr<float>(), dk32.data_ptr<float>(), dv32.data_ptr<float>(), \
    nq, nkv, (float)scale, causal, (int)window,                           \
    part_ptr, (int)nslot, part_stride, (float)softcap,                    \
    softcap_ncap(softcap))
#define BW_LAUNCH(HD_, DET_)                                              \
  do {                                                                    \
    if (softcap > 0.0) BW_LAUNCH_(HD_, DET_, true);                       \
    else BW_LAUNCH_(HD_, DET_, false);                                    \
  } while (0)
  if (hd == 256) {
    if (det) BW_LAUNCH(256, true); else BW_LAUNCH(256, false);
  } else if (hd == 128) {
    if (det) BW_LAUNCH(128, true); else BW_LAUNCH(128, false);
  } else {
    if (det) BW_LAUNCH(64, true); else BW_LAUNCH(64, false);
  }
#undef BW_LAUNCH
#undef BW_LAUNCH_
  if (det) {
    const long n4 = part_stride / 4;
    dim3 rgrid((unsigned)((n4 + 255) / 256));
    if (hd == 256) {
      hipLaunchKernelGGL((bw_reduce_dq<256>), rgrid, dim3(256), 0,
        cur_stream(), part_ptr, dq32.data_ptr<float>(),
        cu_dev.data_ptr<int>(), bs, total, nq, (int)nslot, causal,
        (int)window);
    } else if (hd == 128) {
      hipLaunchKernelGGL((bw_reduce_dq<128>), rgrid, dim3(256), 0,
        cur_stream(), part_ptr, dq32.data_ptr<float>(),
        cu_dev.data_ptr<int>(), bs, total, nq, (int)nslot, causal,
        (int)window);
    } else {
      hipLaunchKernelGGL((bw_reduce_dq<64>), rgrid, dim3(256), 0,
        cur_stream(), part_ptr, dq32.data_ptr<float>(),
        cu_dev.data_ptr<int>(), bs, total, nq, (int)nslot, causal,
        (int)window);
    }
  }
  CHECK_CUDA_OK();
  return {dq32, dk32, dv32};
}
