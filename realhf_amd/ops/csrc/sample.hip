// Decode sampler for gfx950: temperature, top-k, top-p, the draw and the
// sampled token's log-prob in one launch, one 1024-thread workgroup per row.
//
// Every row element has a 56-bit composite  comp = key << 24 | (2^24-1 - idx)
// where key is the order-preserving 32-bit image of x = logit * inv_t.  A
// larger comp is an earlier candidate: value descending, index ascending, a
// total order, so nothing below depends on which lane meets an element first.
//
// Select form (k <= 1024):
//   1. the row is read once with 16-byte loads into 32 registers per lane
//      (8 vectors: V <= 65536 in bf16, 32768 in fp32; longer rows are
//      re-read from L2 by every pass), with an online (max, sum-exp) per
//      lane for the full-row lse.  Keys are re-derived from them per pass;
//   2. an 8-bit radix select over comp from the top digit finds the k-th
//      largest: integer LDS histograms (8 copies, spread by lane), stopping
//      at the first digit whose bucket is taken whole.  Running on into the
//      index digits is what makes "lower index wins" exact among equals;
//   3. the k candidates are compacted into LDS and sorted descending by a
//      bitonic network over 1024 slots, one slot per lane: strides below 64
//      are wave shuffles, the rest go through LDS;
//   4. a fixed-order workgroup scan of e = exp(x - x_0) gives the prefix
//      sums for the top-p cut and the inverse CDF;
//   5. optionally one more pass writes the mask row: removed iff comp is
//      below the last kept candidate's.
// Search form (k > 1024, which top_p without top_k is): no sort.  The cut
// and the draw are each "the candidate whose interval of the running mass
// holds a target", found by the same radix descent over comp with mass
// summed per bin next to the counts.  Mass is a 64-bit integer, exp(x - max)
// in units of 2^-39, so the LDS atomics that sum it give one result in any
// order and every comparison is exact.
// Full form (nothing filtered, or greedy): each lane owns a contiguous chunk
// of the row, so a scan of the chunk sums and a walk inside one chunk give
// the inverse CDF in index order; greedy is a (max, lowest index) reduction.
//
// No scratch, no float atomics, every float reduction in a fixed order:
// results are bitwise reproducible.
#include "common.h"

#include <cstdint>

#define SMP_THREADS 1024
#define SMP_NWAVES (SMP_THREADS / WAVE)
#define SMP_SWEEPS 8   // 16-byte vectors of the row a lane can hold
#define SMP_CHUNK 64   // values of a full-form chunk a lane can hold
#define SMP_MAX_K 1024
#define SMP_IDX_BITS 24
#define SMP_IDX_MASK ((1u << SMP_IDX_BITS) - 1u)
#define SMP_HIST_COPIES 8

typedef unsigned long long u64;

typedef __attribute__((ext_vector_type(4))) unsigned uint4v;

// one 16-byte vector of a row as loaded, and its values
template <typename T> struct SmpVec;
template <> struct SmpVec<bf16> {
  static constexpr int N = 8;
  static DEVINL void decode(uint4v v, float* f) {
    #pragma unroll
    for (int j = 0; j < 4; j++) {
      f[2 * j] = __uint_as_float(v[j] << 16);
      f[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u);
    }
  }
  static DEVINL float load1(const bf16* p) { return bf2f(*(const short*)p); }
};
template <> struct SmpVec<float> {
  static constexpr int N = 4;
  static DEVINL void decode(uint4v v, float* f) {
    #pragma unroll
    for (int j = 0; j < 4; j++) f[j] = __uint_as_float(v[j]);
  }
  static DEVINL float load1(const float* p) { return *p; }
};

// float <-> key with  a < b  <=>  key(a) < key(b); -0 is folded into +0
// first so that equal floats have equal keys.  -inf maps to 0x007fffff.
DEVINL unsigned smp_key(float x) {
  unsigned b = __float_as_uint(x + 0.f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
DEVINL float smp_unkey(unsigned k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
DEVINL u64 smp_comp(unsigned key, int idx) {
  return ((u64)key << SMP_IDX_BITS) | (u64)(SMP_IDX_MASK - (unsigned)idx);
}

// online softmax-denominator update; (m, s) stays (-inf, 0) while only -inf
// has been seen, so (-inf) - (-inf) is never evaluated
DEVINL void smp_acc(float& m, float& s, float f) {
  float mn = fmaxf(m, f);
  if (mn > -INFINITY) {
    s = s * __expf(m - mn) + __expf(f - mn);
    m = mn;
  }
}

template <typename V> DEVINL V smp_wave_incl_scan(V x) {
  const int lane = threadIdx.x & (WAVE - 1);
  #pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    V y = __shfl_up(x, off, WAVE);
    if (lane >= off) x += y;
  }
  return x;
}

DEVINL u64 smp_shfl_xor(u64 v, int mask) {
  unsigned lo = __shfl_xor((unsigned)v, mask, WAVE);
  unsigned hi = __shfl_xor((unsigned)(v >> 32), mask, WAVE);
  return ((u64)hi << 32) | lo;
}

// Workgroup helpers.  `red` is SMP_NWAVES words of LDS; each helper
// synchronises before it reuses them, merges the waves in index order and
// returns the result to every lane.
DEVINL int smp_block_min(int v, int* red) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, WAVE));
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  int r = red[0];
  #pragma unroll
  for (int w = 1; w < SMP_NWAVES; w++) r = min(r, red[w]);
  return r;
}
DEVINL float smp_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  float r = red[0];
  #pragma unroll
  for (int w = 1; w < SMP_NWAVES; w++) r = fmaxf(r, red[w]);
  return r;
}
// exclusive prefix sum of v over the workgroup in lane order; total to all
DEVINL float smp_block_excl_scan(float v, float* red, float& total) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const float incl = smp_wave_incl_scan(v);
  float prev = __shfl_up(incl, 1, WAVE);
  if (lane == 0) prev = 0.f;
  __syncthreads();
  if (lane == WAVE - 1) red[wave] = incl;
  __syncthreads();
  float off = 0.f, tot = 0.f;
  #pragma unroll
  for (int w = 0; w < SMP_NWAVES; w++) {
    if (w == wave) off = tot;
    tot += red[w];
  }
  total = tot;
  return off + prev;
}

// ---------------------------------------------------------------------------
// Select form
// ---------------------------------------------------------------------------
// The row as this lane sees it.  Rows start 16-byte aligned only when V is a
// multiple of the vector width, so a row is a scalar head up to the first
// 16-byte boundary, an aligned vector body and a scalar tail; the fewer
// than 2 * VEC head and tail elements are one extra value in the first lanes.
// With REG the lane keeps its SMP_SWEEPS vectors as loaded (32 registers:
// 64 bf16 or 32 fp32 values) and every pass re-derives the keys from them,
// a handful of VALU operations per value; without, every pass re-reads them.
template <typename T, bool REG> struct SmpRow {
  using VT = SmpVec<T>;
  static constexpr int VEC = VT::N;
  const T* xr;
  int head, nvec, tid;
  float inv_t;
  unsigned xkey;  // the head/tail element of this lane, if xidx >= 0
  int xidx;
  uint4v raw[REG ? SMP_SWEEPS : 1];

  DEVINL void keys(uint4v v, unsigned* k) const {
    float f[VEC];
    VT::decode(v, f);
    #pragma unroll
    for (int j = 0; j < VEC; j++) k[j] = smp_key(f[j] * inv_t);
  }

  // reads the row once; returns this lane's online (m, s)
  DEVINL void load(const T* row, int V, float inv_temperature, float& m, float& s) {
    xr = row;
    tid = threadIdx.x;
    inv_t = inv_temperature;
    int h = (int)(((16u - (unsigned)((uintptr_t)xr & 15u)) & 15u) / sizeof(T));
    head = h < V ? h : V;
    nvec = (V - head) / VEC;
    const int tail0 = head + nvec * VEC;
    m = -INFINITY; s = 0.f;
    xidx = tid < head ? tid : tail0 + (tid - head);
    if (xidx >= V) xidx = -1;
    xkey = 0;
    if (xidx >= 0) {
      float f = VT::load1(xr + xidx) * inv_t;
      xkey = smp_key(f);
      smp_acc(m, s, f);
    }
    auto acc_vec = [&](uint4v v) {
      float f[VEC];
      VT::decode(v, f);
      #pragma unroll
      for (int j = 0; j < VEC; j++) f[j] *= inv_t;
      float vm = f[0];
      #pragma unroll
      for (int j = 1; j < VEC; j++) vm = fmaxf(vm, f[j]);
      float mn = fmaxf(m, vm);
      if (mn > -INFINITY) {
        float acc = s * __expf(m - mn);
        #pragma unroll
        for (int j = 0; j < VEC; j++) acc += __expf(f[j] - mn);
        s = acc;
        m = mn;
      }
    };
    if constexpr (REG) {
      #pragma unroll
      for (int sw = 0; sw < SMP_SWEEPS; sw++) {
        const int v = sw * SMP_THREADS + tid;
        raw[sw] = uint4v{0u, 0u, 0u, 0u};  // never visited
        if (v < nvec) raw[sw] = *(const uint4v*)(xr + head + v * VEC);
      }
      // all loads are in flight; then one vector at a time: tying each
      // vector to the running max keeps 64 decoded values from being live
      #pragma unroll
      for (int sw = 0; sw < SMP_SWEEPS; sw++) {
        uint4v v = raw[sw];
        asm volatile("" : "+v"(v), "+v"(m));
        if (sw * SMP_THREADS + tid < nvec) acc_vec(v);
      }
    } else {
      for (int v = tid; v < nvec; v += SMP_THREADS)
        acc_vec(*(const uint4v*)(xr + head + v * VEC));
    }
  }

  // fs(key, idx) for the extra element, fv(keys[VEC], idx0) for every
  // vector this lane owns
  template <class FS, class FV> DEVINL void each_vec(FS&& fs, FV&& fv) {
    if (xidx >= 0) fs(xkey, xidx);
    unsigned k[VEC];
    if constexpr (REG) {
      // The keys and indices are loop invariants of the caller's loop over
      // passes; hoisted out of it they would take 128 registers.  The lane
      // id is made opaque per call and each vector per sweep, so that every
      // pass re-derives them, one sweep at a time.
      int t = tid;
      asm volatile("" : "+v"(t));
      #pragma unroll
      for (int sw = 0; sw < SMP_SWEEPS; sw++) {
        const int v = sw * SMP_THREADS + t;
        uint4v x = raw[sw];
        asm volatile("" : "+v"(x) : : "memory");
        if (v < nvec) { keys(x, k); fv(k, head + v * VEC); }
      }
    } else {
      for (int v = tid; v < nvec; v += SMP_THREADS) {
        keys(*(const uint4v*)(xr + head + v * VEC), k);
        fv(k, head + v * VEC);
      }
    }
  }
  template <class F> DEVINL void each(F&& f) {
    each_vec(f, [&](const unsigned* k, int i0) {
      #pragma unroll
      for (int j = 0; j < VEC; j++) f(k[j], i0 + j);
    });
  }
};

// The mask row: True = removed, that is after the last kept candidate in
// (value descending, index ascending).
template <typename T, bool REG>
DEVINL void smp_store_mask(SmpRow<T, REG>& r, bool* mr, u64 last) {
  constexpr int VEC = SmpVec<T>::N;
  const unsigned lkey = (unsigned)(last >> SMP_IDX_BITS);
  const int lidx = (int)(SMP_IDX_MASK - (unsigned)(last & SMP_IDX_MASK));
  auto removed = [&](unsigned key, int i) {
    return key < lkey || (key == lkey && i > lidx);
  };
  // the vectors of the logits row are VEC-byte aligned in the mask row
  // when both rows start equally far from such a boundary
  const bool vec_ok = ((uintptr_t)(mr + r.head) & (VEC - 1)) == 0;
  r.each_vec(
      [&](unsigned key, int i) { mr[i] = removed(key, i); },
      [&](const unsigned* kk, int i0) {
        unsigned char b[VEC];
        #pragma unroll
        for (int j = 0; j < VEC; j++) b[j] = removed(kk[j], i0 + j);
        if (vec_ok) {
          if constexpr (VEC == 8) {
            u64 w = 0;
            #pragma unroll
            for (int j = 0; j < 8; j++) w |= (u64)b[j] << (8 * j);
            *(u64*)(mr + i0) = w;
          } else {
            unsigned w = 0;
            #pragma unroll
            for (int j = 0; j < 4; j++) w |= (unsigned)b[j] << (8 * j);
            *(unsigned*)(mr + i0) = w;
          }
        } else {
          #pragma unroll
          for (int j = 0; j < VEC; j++) mr[i0 + j] = b[j];
        }
      });
}

template <typename T, bool REG>
__global__ __launch_bounds__(SMP_THREADS) void sample_select_kernel(
    const T* __restrict__ logits, const float* __restrict__ u,
    long* __restrict__ tokens, float* __restrict__ logp,
    bool* __restrict__ mask, int V, int k, float inv_t, float top_p) {
  constexpr int VEC = SmpVec<T>::N;
  __shared__ unsigned hist[SMP_HIST_COPIES * 256];
  __shared__ u64 slots[SMP_MAX_K];
  __shared__ float redf[SMP_NWAVES];
  __shared__ int redi[SMP_NWAVES];
  __shared__ int sh_digit, sh_need, sh_done, sh_ncand;
  __shared__ float sh_z2;
  __shared__ u64 sh_last;
  const long row = blockIdx.x;
  const int tid = threadIdx.x;

  SmpRow<T, REG> r;
  float lm, ls;
  r.load(logits + row * (long)V, V, inv_t, lm, ls);
  // full-row lse: lanes -> workgroup, fixed order
  const float M = smp_block_max(lm, redf);
  float zrow;
  smp_block_excl_scan(lm > -INFINITY ? ls * __expf(lm - M) : 0.f, redf, zrow);
  float lse = M + logf(zrow);
  // formed here, not where it is used at the end: sinking it would keep the
  // SMP_NWAVES partial sums in registers across the whole kernel
  asm volatile("" : "+v"(lse));

  // ---- radix select of the k-th largest comp ----
  // comp is never formed per element here: digits 6..3 are the key's bytes,
  // digits 2..0 those of the inverted index among elements with the key found
  unsigned pkey = 0, pinv = 0;
  int need = k, shift = 56;
  if (tid == 0) sh_ncand = 0;
  do {
    shift -= 8;
    __syncthreads();
    for (int i = tid; i < SMP_HIST_COPIES * 256; i += SMP_THREADS) hist[i] = 0;
    __syncthreads();
    unsigned* myhist = hist + (tid & (SMP_HIST_COPIES - 1)) * 256;
    if (shift >= SMP_IDX_BITS) {
      const int ks = shift - SMP_IDX_BITS, hs = ks + 8;
      const bool all = hs >= 32;  // top digit: every element takes part
      const unsigned want = all ? 0u : pkey >> (hs & 31);
      r.each([&](unsigned key, int idx) {
        if (all || (key >> (hs & 31)) == want)
          atomicAdd(&myhist[(key >> ks) & 255u], 1u);
      });
    } else {
      const unsigned want = pinv >> (shift + 8);
      r.each([&](unsigned key, int idx) {
        const unsigned inv = SMP_IDX_MASK - (unsigned)idx;
        if (key == pkey && (inv >> (shift + 8)) == want)
          atomicAdd(&myhist[(inv >> shift) & 255u], 1u);
      });
    }
    __syncthreads();
    if (tid < WAVE) {  // lane l owns bins 255 - 4l .. 252 - 4l, largest first
      const int b0 = 255 - 4 * tid;
      int c[4], tot = 0;
      #pragma unroll
      for (int q = 0; q < 4; q++) {
        c[q] = 0;
        #pragma unroll
        for (int cp = 0; cp < SMP_HIST_COPIES; cp++) c[q] += (int)hist[cp * 256 + b0 - q];
        tot += c[q];
      }
      const int incl = smp_wave_incl_scan(tot);
      int above = incl - tot;
      if (above < need && need <= incl) {  // exactly one lane
        #pragma unroll
        for (int q = 0; q < 4; q++) {
          if (above < need && need <= above + c[q]) {
            sh_digit = b0 - q;
            sh_need = need - above;
            sh_done = (c[q] == need - above);
          }
          above += c[q];
        }
      }
    }
    __syncthreads();
    if (shift >= SMP_IDX_BITS) pkey |= (unsigned)sh_digit << (shift - SMP_IDX_BITS);
    else pinv |= (unsigned)sh_digit << shift;
    need = sh_need;
  } while (!sh_done && shift > 0);  // shift 0: comps are distinct, one per bucket

  // ---- compact: every element at or above the threshold, exactly k ----
  auto put = [&](unsigned key, int idx) {
    const int slot = atomicAdd(&sh_ncand, 1);
    if (slot < SMP_MAX_K) slots[slot] = smp_comp(key, idx);
  };
  if (shift >= SMP_IDX_BITS) {
    const int ks = shift - SMP_IDX_BITS;
    r.each([&](unsigned key, int idx) {
      if ((key >> ks) >= (pkey >> ks)) put(key, idx);
    });
  } else {
    r.each([&](unsigned key, int idx) {
      const unsigned inv = SMP_IDX_MASK - (unsigned)idx;
      if (key > pkey || (key == pkey && (inv >> shift) >= (pinv >> shift)))
        put(key, idx);
    });
  }
  __syncthreads();
  u64 c = tid < k ? slots[tid] : 0ull;  // pads sort last

  // ---- bitonic sort, descending, one slot per lane ----
  for (int size = 2; size <= SMP_MAX_K; size <<= 1) {
    const bool desc = (tid & size) == 0;
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      u64 o;
      if (stride >= WAVE) {
        __syncthreads();
        slots[tid] = c;
        __syncthreads();
        o = slots[tid ^ stride];
      } else {
        o = smp_shfl_xor(c, stride);
      }
      const bool take_max = ((tid & stride) == 0) == desc;
      c = take_max ? (c > o ? c : o) : (c < o ? c : o);
    }
  }

  // ---- nucleus cut and draw over the sorted candidates ----
  const bool valid = tid < k;
  const float x = smp_unkey((unsigned)(c >> SMP_IDX_BITS));
  const int idx = (int)(SMP_IDX_MASK - (unsigned)(c & SMP_IDX_MASK));
  const float e = (valid && x > -INFINITY) ? __expf(x - M) : 0.f;
  float z1;
  const float excl = smp_block_excl_scan(e, redf, z1);
  const float incl = excl + e;
  const bool kept = valid && (tid == 0 || (x > -INFINITY &&
                                           (top_p >= 1.f || excl <= top_p * z1)));
  const int m = smp_block_min(kept ? SMP_MAX_K : tid, redi);  // prefix length
  if (tid == m - 1) { sh_z2 = incl; sh_last = c; }
  __syncthreads();
  const float z2 = sh_z2;
  const float target = u[row] * z2;
  const int sel = smp_block_min((tid < m && incl > target) ? tid : m - 1, redi);
  if (tid == sel) {
    tokens[row] = idx;
    logp[row] = mask != nullptr ? (x - M) - logf(z2) : x - lse;
  }

  // ---- mask row: True = removed ----
  if (mask != nullptr) smp_store_mask(r, mask + row * (long)V, sh_last);
}

// ---------------------------------------------------------------------------
// Search form: top_p without top_k, and k > SMP_MAX_K
// ---------------------------------------------------------------------------
// An element's mass, exp(x - M) in units of 2^-39, M the row max: at most
// 2^39 each, so fewer than 2^24 of them sum below 2^63.  Integer sums do not
// depend on their order, which is what lets mass go through LDS atomics.
#define SMP_MASS_ONE 549755813888.f  // 2^39

DEVINL u64 smp_mass(unsigned key, float M) {
  const float x = smp_unkey(key);
  return x > -INFINITY ? (u64)(__expf(x - M) * SMP_MASS_ONE) : 0ull;
}

DEVINL u64 smp_block_sum(u64 v, u64* red) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += smp_shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  u64 r = red[0];
  #pragma unroll
  for (int w = 1; w < SMP_NWAVES; w++) r += red[w];
  return r;
}
DEVINL u64 smp_block_min(u64 v, u64* red) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = smp_shfl_xor(v, off);
    v = o < v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  u64 r = red[0];
  #pragma unroll
  for (int w = 1; w < SMP_NWAVES; w++) r = red[w] < r ? red[w] : r;
  return r;
}

struct SmpSearchLds {
  unsigned cnt[SMP_HIST_COPIES * 256];
  u64 mass[SMP_HIST_COPIES * 256];
  u64 above, comp, q;
  unsigned digit, found;
};
struct SmpFound {
  u64 comp;   // the element found
  u64 above;  // weight of the candidates strictly before it
  u64 q;      // its own mass (MASS only)
};

// Radix search, 8 bits per pass from the top digit of comp, among the
// candidates with comp >= lo, each weighing its mass (MASS) or 1: finds the
// candidate whose interval [above, above + weight) of the running weight in
// candidate order holds `target`; the caller keeps target below the total.
// With unit weights that is the candidate of rank target, counted from 0.
// Per pass the candidates that share the digits found so far add to the
// bins of their next digit (8 copies, spread by lane); 256 lanes fold the
// copies, wave 0 scans the bins from 255 down and publishes the bin that
// holds the target, the weight before it and the number of candidates in
// it.  The descent ends at a bin of one candidate, after digit 0 at the
// latest (comps are distinct): at most 7 passes, and one more that reads the
// found candidate back.  A candidate of no mass is never found by mass.
template <bool MASS, typename T, bool REG>
DEVINL SmpFound smp_search(SmpRow<T, REG>& r, SmpSearchLds& s, u64 lo,
                           u64 target, float M) {
  const int tid = threadIdx.x;
  unsigned* mycnt = s.cnt + (tid & (SMP_HIST_COPIES - 1)) * 256;
  u64* mymass = s.mass + (tid & (SMP_HIST_COPIES - 1)) * 256;
  u64 pre = 0, above = 0;
  int shift = 56;
  unsigned found;
  do {
    shift -= 8;
    __syncthreads();
    for (int i = tid; i < SMP_HIST_COPIES * 256; i += SMP_THREADS) {
      s.cnt[i] = 0;
      if constexpr (MASS) s.mass[i] = 0;
    }
    if (tid == 0) { s.digit = 0; s.found = 0; s.above = above; }
    __syncthreads();
    const u64 want = pre >> (shift + 8);
    r.each([&](unsigned key, int idx) {
      const u64 c = smp_comp(key, idx);
      if (c >= lo && (c >> (shift + 8)) == want) {
        const unsigned d = (unsigned)(c >> shift) & 255u;
        atomicAdd(&mycnt[d], 1u);
        if constexpr (MASS) atomicAdd(&mymass[d], smp_mass(key, M));
      }
    });
    __syncthreads();
    if (tid < 256) {  // fold the copies into the first
      unsigned c = 0;
      u64 m = 0;
      #pragma unroll
      for (int cp = 0; cp < SMP_HIST_COPIES; cp++) {
        c += s.cnt[cp * 256 + tid];
        if constexpr (MASS) m += s.mass[cp * 256 + tid];
      }
      s.cnt[tid] = c;
      if constexpr (MASS) s.mass[tid] = m;
    }
    __syncthreads();
    if (tid < WAVE) {  // lane l owns bins 255 - 4l .. 252 - 4l, largest first
      const int b0 = 255 - 4 * tid;
      unsigned c[4];
      u64 w[4], tot = 0;
      #pragma unroll
      for (int j = 0; j < 4; j++) {
        c[j] = s.cnt[b0 - j];
        w[j] = MASS ? s.mass[b0 - j] : (u64)c[j];
        tot += w[j];
      }
      const u64 incl = smp_wave_incl_scan(tot);
      u64 ab = above + (incl - tot);
      if (ab <= target && target < ab + tot) {  // at most one lane
        #pragma unroll
        for (int j = 0; j < 4; j++) {
          if (ab <= target && target < ab + w[j]) {
            s.digit = (unsigned)(b0 - j);
            s.found = c[j];
            s.above = ab;
          }
          ab += w[j];
        }
      }
    }
    __syncthreads();
    pre |= (u64)s.digit << shift;
    above = s.above;
    found = s.found;
  } while (found > 1 && shift > 0);

  if (tid == 0) { s.comp = 0; s.q = 0; }
  __syncthreads();
  const u64 want = pre >> shift;
  r.each([&](unsigned key, int idx) {
    const u64 c = smp_comp(key, idx);
    if (c >= lo && (c >> shift) == want) {  // one element
      s.comp = c;
      if constexpr (MASS) s.q = smp_mass(key, M);
    }
  });
  __syncthreads();
  return SmpFound{s.comp, above, s.q};
}

// Steps: load as the select form does; with k < V a rank search for the k-th
// comp, below which nothing is a candidate; one pass for Z1, the candidates'
// mass, and for the smallest finite candidate, which is the last kept one
// when top_p keeps everything; with top_p < 1 a mass search for the
// candidate whose interval holds top_p * Z1, the last kept one, Z2 the mass
// down to it; a mass search among the kept for u * Z2, the token; the mask.
template <typename T, bool REG>
__global__ __launch_bounds__(SMP_THREADS) void sample_search_kernel(
    const T* __restrict__ logits, const float* __restrict__ u,
    long* __restrict__ tokens, float* __restrict__ logp,
    bool* __restrict__ mask, int V, int k, float inv_t, float top_p) {
  __shared__ SmpSearchLds s;
  __shared__ float redf[SMP_NWAVES];
  __shared__ u64 red64[SMP_NWAVES];
  const long row = blockIdx.x;

  SmpRow<T, REG> r;
  float lm, ls;
  r.load(logits + row * (long)V, V, inv_t, lm, ls);
  const float M = smp_block_max(lm, redf);
  float zrow;
  smp_block_excl_scan(lm > -INFINITY ? ls * __expf(lm - M) : 0.f, redf, zrow);
  float lse = M + logf(zrow);
  asm volatile("" : "+v"(lse));  // as in the select form

  u64 lo = 0;
  if (k < V) lo = smp_search<false>(r, s, 0ull, (u64)(k - 1), M).comp;

  const unsigned neginf = smp_key(-INFINITY);
  u64 zl = 0, fl = ~0ull;
  r.each([&](unsigned key, int idx) {
    const u64 c = smp_comp(key, idx);
    if (c >= lo && key > neginf) {
      zl += smp_mass(key, M);
      fl = c < fl ? c : fl;
    }
  });
  const u64 z1 = smp_block_sum(zl, red64);
  u64 last = smp_block_min(fl, red64);

  u64 z2 = z1, tok;
  if (last == ~0ull) {  // no finite entry: candidate 0 alone, as the reference
    last = tok = smp_comp(neginf, 0);
  } else {
    // the maximum weighs 2^39, so z1 > 0 and the threshold is below z1
    if (top_p < 1.f) {
      const u64 thr = (u64)((double)top_p * (double)z1);
      const SmpFound f = smp_search<true>(r, s, lo, thr < z1 ? thr : z1 - 1, M);
      last = f.comp;
      z2 = f.above + f.q;
    }
    const u64 t = (u64)((double)u[row] * (double)z2);
    tok = smp_search<true>(r, s, last, t < z2 ? t : z2 - 1, M).comp;
  }
  if (threadIdx.x == 0) {
    int idx = (int)(SMP_IDX_MASK - (unsigned)(tok & SMP_IDX_MASK));
    if (idx >= V) idx = 0;
    const float x = smp_unkey((unsigned)(tok >> SMP_IDX_BITS));
    tokens[row] = idx;
    logp[row] = mask != nullptr
        ? (x - M) - logf((float)z2 * (1.f / SMP_MASS_ONE)) : x - lse;
  }
  if (mask != nullptr) smp_store_mask(r, mask + row * (long)V, last);
}

// ---------------------------------------------------------------------------
// Full form: pure sampling in index order, or greedy
// ---------------------------------------------------------------------------
template <typename T, bool REG>
__global__ __launch_bounds__(SMP_THREADS) void sample_full_kernel(
    const T* __restrict__ logits, const float* __restrict__ u,
    long* __restrict__ tokens, float* __restrict__ logp,
    bool* __restrict__ mask, int V, float inv_t, int greedy) {
  using VT = SmpVec<T>;
  __shared__ float redf[SMP_NWAVES];
  __shared__ int redi[SMP_NWAVES];
  __shared__ int sh_tok;
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  const T* xr = logits + row * (long)V;
  const int chunk = (V + SMP_THREADS - 1) / SMP_THREADS;  // <= SMP_CHUNK if REG
  const int i0 = tid * chunk;
  const int cnt = max(0, min(chunk, V - i0));

  float xreg[REG ? SMP_CHUNK : 1];
  if constexpr (REG) {
    #pragma unroll
    for (int j = 0; j < SMP_CHUNK; j++)
      xreg[j] = j < cnt ? VT::load1(xr + i0 + j) * inv_t : -INFINITY;
  }
  // f(x, j) over this lane's chunk in index order
  auto each = [&](auto&& f) {
    if constexpr (REG) {
      #pragma unroll
      for (int j = 0; j < SMP_CHUNK; j++)
        if (j < cnt) f(xreg[j], j);
    } else {
      for (int j = 0; j < cnt; j++) f(VT::load1(xr + i0 + j) * inv_t, j);
    }
  };

  float lm = -INFINITY;
  int larg = 0x7fffffff, lastfin = -1;
  each([&](float x, int j) {
    if (x > lm) { lm = x; larg = i0 + j; }  // strict: lowest index of equals
    if (x > -INFINITY) lastfin = i0 + j;
  });
  const float M = smp_block_max(lm, redf);
  float s = 0.f;
  each([&](float x, int j) { s += __expf(x - M); });
  float z;
  const float excl = smp_block_excl_scan(s, redf, z);

  int tok;
  if (greedy) {
    tok = smp_block_min(lm == M ? larg : 0x7fffffff, redi);
  } else {
    const float target = u[row] * z;
    // first lane whose inclusive prefix exceeds the target; excl + s is the
    // last partial sum of the walk below, so the walk always lands
    const int lane = smp_block_min(excl + s > target ? tid : SMP_THREADS, redi);
    const int last = -smp_block_min(-lastfin, redi);
    if (tid == 0) sh_tok = last;  // rounding left no lane: the last finite entry
    __syncthreads();
    if (tid == lane) {
      float part = 0.f;
      int hit = -1;
      each([&](float x, int j) {
        part += __expf(x - M);
        if (hit < 0 && excl + part > target) hit = i0 + j;
      });
      if (hit >= 0) sh_tok = hit;
    }
    __syncthreads();
    tok = sh_tok;
  }
  if (tok < 0 || tok >= V) tok = 0;  // a row with no finite entry
  if (tid == 0) {
    tokens[row] = tok;
    logp[row] = (VT::load1(xr + tok) * inv_t - M) - logf(z);
  }
  if (mask != nullptr) {  // nothing is removed but -inf entries
    bool* mr = mask + row * (long)V;
    for (int i = tid; i < V; i += SMP_THREADS)
      mr[i] = !(VT::load1(xr + i) * inv_t > -INFINITY);
  }
}

std::vector<torch::Tensor> sample_logits(torch::Tensor logits, torch::Tensor u,
                                         double inv_temperature, long top_k,
                                         double top_p, bool greedy,
                                         bool want_mask) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous(),
              "sample_logits: logits must be a contiguous [bs, V] GPU tensor");
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 ||
              logits.scalar_type() == torch::kFloat,
              "sample_logits: logits must be bf16 or fp32");
  const long bs = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V <= (long)SMP_IDX_MASK && bs < (1L << 31),
              "sample_logits: unsupported shape");
  TORCH_CHECK(u.is_cuda() && u.scalar_type() == torch::kFloat &&
              u.is_contiguous() && u.dim() == 1 && u.size(0) == bs,
              "sample_logits: u must be a contiguous fp32 [bs] GPU tensor");
  const long k = (top_k <= 0 || top_k > V) ? V : top_k;
  const bool full = greedy || (k >= V && top_p >= 1.0);
  // more candidates than the select form sorts: the search form
  const bool search = !full && k > SMP_MAX_K;
  auto tokens = torch::empty({bs}, logits.options().dtype(torch::kLong));
  auto logp = torch::empty({bs}, logits.options().dtype(torch::kFloat));
  auto mask = want_mask ? torch::empty({bs, V}, logits.options().dtype(torch::kBool))
                        : torch::empty({0}, logits.options().dtype(torch::kBool));
  if (bs == 0) return {tokens, logp, mask};
  bool* mp = want_mask ? mask.data_ptr<bool>() : nullptr;
  // does the row fit the registers of one workgroup?
  const long vec = 16 / logits.element_size();
  const bool reg = full ? V <= (long)SMP_THREADS * SMP_CHUNK
                        : V <= (long)SMP_THREADS * SMP_SWEEPS * vec;
  auto launch = [&](auto tag, auto regtag) {
    using scalar_t = decltype(tag);
    constexpr bool REG = decltype(regtag)::value;
    const scalar_t* x = (const scalar_t*)logits.data_ptr();
    if (full)
      hipLaunchKernelGGL((sample_full_kernel<scalar_t, REG>), dim3((unsigned)bs),
        dim3(SMP_THREADS), 0, cur_stream(), x, u.data_ptr<float>(),
        (long*)tokens.data_ptr<int64_t>(), logp.data_ptr<float>(), mp, (int)V,
        (float)inv_temperature, (int)greedy);
    else if (search)
      hipLaunchKernelGGL((sample_search_kernel<scalar_t, REG>), dim3((unsigned)bs),
        dim3(SMP_THREADS), 0, cur_stream(), x, u.data_ptr<float>(),
        (long*)tokens.data_ptr<int64_t>(), logp.data_ptr<float>(), mp, (int)V,
        (int)k, (float)inv_temperature, (float)top_p);
    else
      hipLaunchKernelGGL((sample_select_kernel<scalar_t, REG>), dim3((unsigned)bs),
        dim3(SMP_THREADS), 0, cur_stream(), x, u.data_ptr<float>(),
        (long*)tokens.data_ptr<int64_t>(), logp.data_ptr<float>(), mp, (int)V,
        (int)k, (float)inv_temperature, (float)top_p);
  };
  if (logits.scalar_type() == torch::kBFloat16) {
    if (reg) launch(bf16{}, std::true_type{}); else launch(bf16{}, std::false_type{});
  } else {
    if (reg) launch(float{}, std::true_type{}); else launch(float{}, std::false_type{});
  }
  CHECK_CUDA_OK();
  return {tokens, logp, mask};
}
