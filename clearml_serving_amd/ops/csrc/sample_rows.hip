// Fused per-row sampler and logit penalties.
//
//   sample_rows      one launch sequence for a heterogeneous batch: per-row
//                    temperature, top-k, top-p, min-p and seed. No sort, no
//                    library op, no device-to-host sync, no memset, no float
//                    atomics.
//   apply_penalties  out-of-place copy of the logits plus a thread-per-entry
//                    scatter of repetition / frequency / presence penalties
//                    and min_tokens bans from a CSR list of (token, count,
//                    flags) entries.
//
// sample_rows: every filter is a value threshold, so a row's keep-set is
// {t : key(x_t) >= tkey} with key() the order-preserving uint32 image of the
// fp32 logit. Two kernels:
//
//   select  one 1024-thread workgroup per row, launched only when a filter
//           tensor is given. Rows whose filters are all off (and greedy rows)
//           leave at once. The others take a max pass and then radix-descend
//           the key space MSB first: each round streams the row once with
//           16-byte loads into an LDS histogram of (count u32, mass u64) per
//           digit, a block suffix scan finds the digit where the count
//           reaches k (top-k) or the mass passes p * M (top-p), and the next
//           round looks only at keys under that prefix. bf16 keys carry 16
//           significant bits (rounds of 11 + 5), fp16 19 (11 + 8), fp32 32
//           (11 + 11 + 10). Mass is exp((x - x_max) / T) in 2^32 fixed point,
//           summed with integer LDS atomics: the sums do not depend on the
//           order of arrival, so a borderline top-p cut cannot flip between
//           runs. The k-descent carries the mass above its cut, so M(tau_k)
//           falls out at its end and the p-descent runs against
//           p * M(tau_k) over keys >= key(tau_k). top_k == 1 and min-p alone
//           need only the max pass.
//   draw    token_mask.hip's gumbel-max draw with `key(x) >= tkey[row]` in
//           place of the mask bit: vocabulary split over gridDim.y, per-split
//           partial keys, finalize kernel. With no filter tensor this is the
//           only kernel, i.e. the cost of sample_token_bitmask at slot -1.
//
// Work split of the select stage: one workgroup per row keeps the histogram
// in LDS (24 KB) and needs no scratch tensor and no launch between rounds;
// the row (251 KB of bf16 at V = 128256) is re-read from L2 on each pass.
// The alternative -- the vocabulary split over gridDim.y with per-split
// histograms in global memory and a reduce-and-pick kernel between rounds --
// was not measured. Measured (MI355X, bf16, V = 128256, top-k 50 + top-p
// 0.9 on every row, profiles/sampler_bench.txt): 102 / 104 / 107 us at B =
// 1 / 8 / 64 against 178 / 655 / 980 us for sampling.hip's library
// composition; without filter tensors 11.2 / 11.3 / 18.6 us against 11.6 /
// 11.8 / 18.1 us for sample_token_bitmask at slot -1. The draw stage is
// split, and because the threshold is an integer key the split cannot
// change a token.
//
// Kernels carry target("no-packed-fp32-ops"), the choice moe_fp8.hip makes
// for its epilogue: the histogram and draw loops run the same fp32 multiply
// and subtract on the 4 or 8 logits of one 16-byte load, which the compiler
// would otherwise pair into packed VALU ops (v_pk_mul_f32 / v_pk_add_f32).
// With the attribute the vector body and the scalar head / tail go through
// the very same v_mul / v_sub / v_fma sequence, which is what the split
// independence of the top-p cut and of the draw rests on. It is set per
// function so that no other file's code generation changes. Functions that
// restrict their features cannot inline the runtime header's __syncthreads
// / __shfl / atomicAdd wrappers (they become out-of-line calls), hence the
// builtins in block_sync / lane_read / lds_add below.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
// zero scratch in every kernel; select 94-96 VGPRs and 24800 B of LDS per
// 1024-thread workgroup, draw 20-22 VGPRs, scatter 13.
#include "common.h"

namespace {

#ifdef __HIP_DEVICE_COMPILE__
#define SR_PLAIN_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SR_PLAIN_FP32  // the host pass has no such feature
#endif

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / WAVE_SIZE;
constexpr int HIST_BINS = 2048;  // 11-bit digits
// orderable(-FLT_MAX): the lowest threshold still drops -inf (0x007FFFFF)
constexpr unsigned int KEY_MIN_FINITE = 0x00800000u;
constexpr unsigned int KEY_NONE = 0xFFFFFFFFu;  // keeps nothing

template <typename T> struct KeyBits;  // significant (top) bits of a key
template <> struct KeyBits<__hip_bfloat16> { static constexpr int N = 16; };
template <> struct KeyBits<__half> { static constexpr int N = 19; };
template <> struct KeyBits<float> { static constexpr int N = 32; };

// Barrier, cross-lane moves, bit casts and LDS atomics as compiler builtins:
// the runtime header's wrappers are built with the default target features
// and would not inline into functions that restrict theirs.
__device__ __forceinline__ SR_PLAIN_FP32 void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ SR_PLAIN_FP32 unsigned int lane_read(
    unsigned int v, int src_lane) {
  return (unsigned int)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}

__device__ __forceinline__ SR_PLAIN_FP32 unsigned long long lane_read(
    unsigned long long v, int src_lane) {
  const unsigned int lo = lane_read((unsigned int)v, src_lane);
  const unsigned int hi = lane_read((unsigned int)(v >> 32), src_lane);
  return ((unsigned long long)hi << 32) | lo;
}

template <typename U>
__device__ __forceinline__ SR_PLAIN_FP32 void lds_add(U* p, U v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ SR_PLAIN_FP32 unsigned int pcg_hash(
    unsigned int x) {
  x = x * 747796405u + 2891336453u;
  unsigned int w = ((x >> ((x >> 28u) + 4u)) ^ x) * 277803737u;
  return (w >> 22u) ^ w;
}

// order-preserving float -> uint32 (works for +/-, inf)
__device__ __forceinline__ SR_PLAIN_FP32 unsigned int float_orderable(
    float f) {
  unsigned int u = __builtin_bit_cast(unsigned int, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ SR_PLAIN_FP32 float orderable_float(
    unsigned int k) {
  return __builtin_bit_cast(
      float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// Key of a logit: 0 for NaN (no other float maps to 0, and 0 is below every
// threshold); -0.0 shares the key of +0.0.
__device__ __forceinline__ SR_PLAIN_FP32 unsigned int logit_key(float x) {
  if (x != x) return 0u;
  if (x == 0.0f) x = 0.0f;
  return float_orderable(x);
}

// Elements of the scalar head before (p + i) reaches 16-byte alignment.
template <typename T>
__device__ __forceinline__ SR_PLAIN_FP32 int head_elems(const T* p, int n) {
  const int mis = (int)((size_t)p & 15);
  const int head = mis ? (16 - mis) / (int)sizeof(T) : 0;
  return min(head, n);
}

// f(token, logit) for tokens [lo, hi) of one row, thread `tid` of
// `nthreads`: 16-byte loads between a scalar head and tail.
template <typename T, typename F>
__device__ __forceinline__ SR_PLAIN_FP32 void for_each_logit(
    const T* __restrict__ src, int lo, int hi, int tid, int nthreads, F& f) {
  constexpr int VEC = 16 / sizeof(T);
  const int n = max(hi - lo, 0);
  const int head = head_elems(src + lo, n);
  const int nvec = (n - head) / VEC;
  const int tail0 = lo + head + nvec * VEC;
  for (int v = tid; v < nvec; v += nthreads) {
    const int t0 = lo + head + v * VEC;
    union {
      uint32x4 u;
      T e[VEC];
    } x;
    x.u = *reinterpret_cast<const uint32x4*>(src + t0);
#pragma unroll
    for (int j = 0; j < VEC; ++j) f(t0 + j, to_f32(x.e[j]));
  }
  const int nscalar = head + (hi - tail0);
  for (int i = tid; i < nscalar; i += nthreads) {
    const int t = i < head ? lo + i : tail0 + (i - head);
    f(t, to_f32(src[t]));
  }
}

// ------------------------------------------------------------------ //
// select
// ------------------------------------------------------------------ //
struct SelectShared {
  unsigned int cnt[HIST_BINS];
  unsigned long long mass[HIST_BINS];
  unsigned int wave_cnt[SEL_WAVES];
  unsigned long long wave_mass[SEL_WAVES];
  unsigned int max_key;
  // result of one round's scan
  int digit;  // -1: no digit crosses the target
  unsigned int above_cnt;
  unsigned long long above_mass;
  unsigned long long total_mass;
};

struct MaxKey {
  unsigned int key;
  __device__ __forceinline__ SR_PLAIN_FP32 void operator()(int, float x) {
    const unsigned int k = logit_key(x);
    if (k > key) key = k;
  }
};

// Histogram of one digit over the keys >= floor_key whose bits above the
// digit equal `prefix`. hs = 32 (first round) matches every key.
struct HistAdd {
  SelectShared* sh;
  unsigned int prefix, floor_key, digit_mask;
  int hs, shift;
  float x_max, inv_temp;
  __device__ __forceinline__ SR_PLAIN_FP32 void operator()(int, float x) {
    const unsigned int k = logit_key(x);
    if (k == 0u || k < floor_key) return;
    if ((unsigned int)((unsigned long long)k >> hs) != prefix) return;
    const unsigned int d = (k >> shift) & digit_mask;
    lds_add(&sh->cnt[d], 1u);
    // 2^32 fixed point, <= 2^32 per token; -inf and far tails weigh 0. A
    // token at the maximum weighs 2^32 also when the maximum is +inf
    // (inf - inf is NaN), next to which every finite token weighs 0.
    const float w = x == x_max
                        ? 4294967296.0f
                        : __expf((x - x_max) * inv_temp) * 4294967296.0f;
    const unsigned long long m = (unsigned long long)w;
    if (m) lds_add(&sh->mass[d], m);
  }
};

template <typename T>
__device__ __forceinline__ SR_PLAIN_FP32 void hist_round(
    const T* __restrict__ src, int vocab, SelectShared& sh, HistAdd& add,
    int bits) {
  for (int b = threadIdx.x; b < (1 << bits); b += SEL_THREADS) {
    sh.cnt[b] = 0u;
    sh.mass[b] = 0ull;
  }
  block_sync();
  for_each_logit(src, 0, vocab, (int)threadIdx.x, SEL_THREADS, add);
  block_sync();
}

// Suffix scan of the histogram from the top digit down, then the crossing:
//   BY_MASS = false: the digit d with count above d <  k <= count above d +
//                    cnt[d]            (target = k)
//   BY_MASS = true:  the digit d with mass above d  <= target < mass above d
//                    + mass[d]; with frac >= 0 the target is frac * total
//                    mass of this histogram.
// Leaves digit (-1 if none), the count and mass above it and the total mass
// in sh. Each thread owns digits 2t and 2t + 1.
template <bool BY_MASS>
__device__ __forceinline__ SR_PLAIN_FP32 void find_crossing(
    SelectShared& sh, int bits, unsigned long long target, double frac) {
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int nbins = 1 << bits;
  const int b0 = 2 * tid, b1 = 2 * tid + 1;
  const unsigned int c0 = b0 < nbins ? sh.cnt[b0] : 0u;
  const unsigned int c1 = b1 < nbins ? sh.cnt[b1] : 0u;
  const unsigned long long m0 = b0 < nbins ? sh.mass[b0] : 0ull;
  const unsigned long long m1 = b1 < nbins ? sh.mass[b1] : 0ull;
  unsigned int c = c0 + c1;
  unsigned long long m = m0 + m1;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const unsigned int oc = lane_read(c, lane + off);
    const unsigned long long om = lane_read(m, lane + off);
    if (lane + off < WAVE_SIZE) {
      c += oc;
      m += om;
    }
  }
  if (lane == 0) {
    sh.wave_cnt[wave] = c;
    sh.wave_mass[wave] = m;
  }
  if (tid == 0) sh.digit = -1;
  block_sync();
  unsigned int total_c = 0u;
  unsigned long long total_m = 0ull;
  unsigned int above_c = c - (c0 + c1);  // own wave, threads above
  unsigned long long above_m = m - (m0 + m1);
  for (int w = 0; w < SEL_WAVES; ++w) {
    total_c += sh.wave_cnt[w];
    total_m += sh.wave_mass[w];
    if (w > wave) {
      above_c += sh.wave_cnt[w];
      above_m += sh.wave_mass[w];
    }
  }
  if (frac >= 0.0) target = (unsigned long long)(frac * (double)total_m);
  if (tid == 0) sh.total_mass = total_m;
  // digit 2t + 1 lies above digit 2t
  const unsigned int ac[2] = {above_c + c1, above_c};
  const unsigned long long am[2] = {above_m + m1, above_m};
  const unsigned int oc[2] = {c0, c1};
  const unsigned long long om[2] = {m0, m1};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const bool hit =
        BY_MASS ? (am[j] <= target && target < am[j] + om[j])
                : ((unsigned long long)ac[j] < target &&
                   target <= (unsigned long long)ac[j] + oc[j]);
    if (hit) {  // at most one digit of the histogram
      sh.digit = 2 * tid + j;
      sh.above_cnt = ac[j];
      sh.above_mass = am[j];
    }
  }
  block_sync();
}

// One workgroup per row -> tkey[row].
template <typename T>
__global__ __launch_bounds__(SEL_THREADS) SR_PLAIN_FP32
void sample_rows_select_kernel(
    const T* __restrict__ logits, long row_stride,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ min_p,
    unsigned int* __restrict__ tkey, int vocab) {
  constexpr int KB = KeyBits<T>::N;
  __shared__ SelectShared sh;
  const int row = blockIdx.x;
  const T* src = logits + (long)row * row_stride;
  const float temp = temperature[row];
  const int k = top_k ? top_k[row] : 0;
  const float p = top_p ? top_p[row] : 1.0f;
  const float mp = min_p ? min_p[row] : 0.0f;
  const bool need_k = k > 0 && k < vocab;
  const bool need_p = p < 1.0f;
  const bool need_m = mp > 0.0f;
  // everything below branches on row-uniform values only
  if (!(temp > 0.0f) || !(need_k || need_p || need_m)) {
    if (threadIdx.x == 0) tkey[row] = KEY_MIN_FINITE;
    return;
  }

  if (threadIdx.x == 0) sh.max_key = 0u;
  block_sync();
  MaxKey mk{0u};
  for_each_logit(src, 0, vocab, (int)threadIdx.x, SEL_THREADS, mk);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    mk.key = max(mk.key, lane_read(mk.key, (int)(threadIdx.x & 63) ^ off));
  if ((threadIdx.x & (WAVE_SIZE - 1)) == 0)
    __hip_atomic_fetch_max(&sh.max_key, mk.key, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  block_sync();
  const unsigned int max_key = sh.max_key;
  if (max_key < KEY_MIN_FINITE) {  // nothing finite in this row
    if (threadIdx.x == 0) tkey[row] = KEY_NONE;
    return;
  }
  const float x_max = orderable_float(max_key);
  unsigned int tk = KEY_MIN_FINITE;
  if (need_m) tk = max(tk, logit_key(x_max + temp * __logf(mp)));
  if (need_k && k == 1) {
    // tau_k is the maximum, and top-p inside {x == max} keeps the maximum
    if (threadIdx.x == 0) tkey[row] = max(tk, max_key);
    return;
  }

  HistAdd add;
  add.sh = &sh;
  add.x_max = x_max;
  add.inv_temp = 1.0f / temp;

  // top-k: the k-th largest key, and M(tau_k)
  unsigned int key_k = 0u;        // 0: top-k off, every non-NaN key counts
  unsigned long long mass_k = 0;  // M(tau_k), valid once have_mass
  bool have_mass = false;
  if (need_k) {
    unsigned int prefix = 0u;
    unsigned long long k_rem = (unsigned long long)k, above = 0ull;
    bool found = true;
    for (int done = 0; done < KB && found;) {
      const int bits = min(11, KB - done);
      add.prefix = prefix;
      add.floor_key = 0u;
      add.hs = 32 - done;
      add.shift = 32 - done - bits;
      add.digit_mask = (1u << bits) - 1u;
      hist_round(src, vocab, sh, add, bits);
      find_crossing<false>(sh, bits, k_rem, -1.0);
      if (sh.digit < 0) {  // fewer than k non-NaN logits: top-k keeps all
        found = false;
        break;
      }
      prefix = (prefix << bits) | (unsigned int)sh.digit;
      k_rem -= sh.above_cnt;
      above += sh.above_mass;
      done += bits;
      if (done == KB) mass_k = above + sh.mass[sh.digit];
      block_sync();  // sh is rewritten by the next round
    }
    if (found) {
      key_k = KB == 32 ? prefix : prefix << (32 - KB);
      have_mass = true;
      tk = max(tk, key_k);
    } else {
      mass_k = sh.total_mass;  // first-round histogram holds the whole row
      have_mass = true;
      block_sync();
    }
  }

  // top-p: v' = the largest value with M(v') > p * M(tau_k); keep x > v',
  // or the maximum's tie group when v' is the maximum
  if (need_p) {
    const double frac = p > 0.0f ? (double)p : 0.0;
    unsigned long long target =
        have_mass ? (unsigned long long)(frac * (double)mass_k) : 0ull;
    unsigned int prefix = 0u;
    for (int done = 0; done < KB;) {
      const int bits = min(11, KB - done);
      add.prefix = prefix;
      add.floor_key = key_k;
      add.hs = 32 - done;
      add.shift = 32 - done - bits;
      add.digit_mask = (1u << bits) - 1u;
      hist_round(src, vocab, sh, add, bits);
      find_crossing<true>(sh, bits, target,
                          (done == 0 && !have_mass) ? frac : -1.0);
      if (done == 0 && !have_mass)
        target = (unsigned long long)(frac * (double)sh.total_mass);
      // the scope's mass exceeds the target (p < 1), so a digit crosses
      const unsigned int d = sh.digit < 0 ? 0u : (unsigned int)sh.digit;
      prefix = (prefix << bits) | d;
      target -= sh.above_mass;
      done += bits;
      block_sync();
    }
    const unsigned int max_prefix = KB == 32 ? max_key : max_key >> (32 - KB);
    const unsigned int cut = prefix == max_prefix ? prefix : prefix + 1u;
    tk = max(tk, KB == 32 ? cut : cut << (32 - KB));
  }
  if (threadIdx.x == 0) tkey[row] = tk;
}

// ------------------------------------------------------------------ //
// draw
// ------------------------------------------------------------------ //
// Running best of one thread as a packed key: (orderable score << 32) |
// (0xFFFFFFFF - token). Larger key wins, so equal scores resolve to the
// lowest token; key 0 = nothing kept seen.
struct Draw {
  unsigned long long key;
  float inv_temp;  // 0 = greedy
  unsigned int row_seed, tkey;
  __device__ __forceinline__ SR_PLAIN_FP32 void operator()(int tok,
                                                           float lg) {
    if (logit_key(lg) < tkey) return;  // NaN (key 0), -inf and filtered
    float s = lg;
    if (inv_temp != 0.0f) {
      const unsigned int h = pcg_hash(row_seed + (unsigned int)tok);
      // exact in fp32, u in [2^-24, 1 - 2^-24]: the noise is always finite
      // (same arithmetic as token_mask.hip)
      const float u = ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
      s = lg * inv_temp - __logf(-__logf(u));
    }
    if (s == 0.0f) s = 0.0f;  // -0.0 ties with +0.0, as in argmax
    const unsigned long long k =
        ((unsigned long long)float_orderable(s) << 32) |
        (0xFFFFFFFFu - (unsigned int)tok);
    if (k > key) key = k;
  }
};

template <typename T>
__global__ __launch_bounds__(256) SR_PLAIN_FP32
void sample_rows_draw_kernel(
    const T* __restrict__ logits, long row_stride,
    const float* __restrict__ temperature, const int* __restrict__ seed,
    const unsigned int* __restrict__ tkey,
    unsigned long long* __restrict__ partial, long* __restrict__ out,
    int vocab, int chunk) {
  const int row = blockIdx.x;
  const T* src = logits + (long)row * row_stride;
  const int lo = blockIdx.y * chunk;  // chunk is a multiple of 32
  const int hi = min(vocab, lo + chunk);
  const float temp = temperature[row];

  Draw best;
  best.key = 0ull;
  best.inv_temp = temp > 0.0f ? 1.0f / temp : 0.0f;
  best.row_seed = pcg_hash((unsigned int)seed[row]);
  best.tkey = tkey ? max(tkey[row], KEY_MIN_FINITE) : KEY_MIN_FINITE;
  for_each_logit(src, lo, hi, (int)threadIdx.x, (int)blockDim.x, best);

  unsigned long long key = best.key;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = lane_read(key, lane ^ off);
    if (other > key) key = other;
  }
  __shared__ unsigned long long skeys[16];
  const int wave = threadIdx.x / WAVE_SIZE;
  if (lane == 0) skeys[wave] = key;
  block_sync();
  if (threadIdx.x == 0) {
    const int nwaves = blockDim.x / WAVE_SIZE;
    for (int w = 1; w < nwaves; ++w)
      if (skeys[w] > key) key = skeys[w];
    if (out != nullptr) {  // single split: final answer, no second launch
      out[row] = key ? (long)(0xFFFFFFFFu - (unsigned int)key) : -1L;
    } else {
      partial[(long)row * gridDim.y + blockIdx.y] = key;
    }
  }
}

__global__ void sample_rows_finalize_kernel(
    const unsigned long long* __restrict__ partial, long* __restrict__ out,
    int rows, int splits) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  unsigned long long key = 0ull;
  for (int s = 0; s < splits; ++s) {
    const unsigned long long k = partial[(long)row * splits + s];
    if (k > key) key = k;
  }
  out[row] = key ? (long)(0xFFFFFFFFu - (unsigned int)key) : -1L;
}

// ------------------------------------------------------------------ //
// penalties
// ------------------------------------------------------------------ //
// Bit-exact row copy (U = 16- or 32-bit element) into a dense [B, V] tensor.
template <typename U>
__global__ void copy_rows_kernel(const U* __restrict__ logits,
                                 long row_stride, U* __restrict__ out,
                                 int vocab) {
  constexpr int VEC = 16 / sizeof(U);
  const int row = blockIdx.x;
  const U* src = logits + (long)row * row_stride;
  U* dst = out + (long)row * vocab;
  const int tid = blockIdx.y * blockDim.x + threadIdx.x;
  const int nthreads = gridDim.y * blockDim.x;
  // 16-byte path needs source and destination equally (mis)aligned
  const bool vec_ok = ((size_t)src & 15) == ((size_t)dst & 15);
  const int head = vec_ok ? head_elems(src, vocab) : vocab;
  const int nvec = vec_ok ? (vocab - head) / VEC : 0;
  const int tail0 = head + nvec * VEC;
  for (int v = tid; v < nvec; v += nthreads) {
    const int t0 = head + v * VEC;
    *reinterpret_cast<uint32x4*>(dst + t0) =
        *reinterpret_cast<const uint32x4*>(src + t0);
  }
  const int nscalar = head + (vocab - tail0);
  for (int i = tid; i < nscalar; i += nthreads) {
    const int t = i < head ? i : tail0 + (i - head);
    dst[t] = src[t];
  }
}

// One thread per entry; entries offsets[r]..offsets[r+1] belong to row r.
// Tokens are unique within a row (precondition), so no two threads touch
// the same element. Every step rounds to fp32 on its own (no fma), the
// result rounds once to T.
template <typename T>
__global__ SR_PLAIN_FP32 void penalty_scatter_kernel(
    T* __restrict__ out, const int* __restrict__ tok,
    const int* __restrict__ cnt, const int* __restrict__ flags,
    const int* __restrict__ offsets, const float* __restrict__ presence,
    const float* __restrict__ frequency, const float* __restrict__ repetition,
    int rows, int vocab, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || i < offsets[0]) return;
  int lo = 0, hi = rows;  // the last row with offsets[row] <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  if (i >= offsets[lo + 1]) return;
  const int t = tok[i];
  if (t < 0 || t >= vocab) return;  // never indexed
  T* dst = out + (long)lo * vocab + t;
  float x = to_f32(*dst);
  const float rep = repetition[lo];
  x = x > 0.0f ? __fdiv_rn(x, rep) : __fmul_rn(x, rep);
  const int c = cnt[i];
  x = __fsub_rn(x, __fmul_rn(frequency[lo], (float)c));
  if (c > 0) x = __fsub_rn(x, presence[lo]);
  if (flags[i] & 1) x = -INFINITY;
  *dst = from_f32<T>(x);
}

void check_logits(const torch::Tensor& logits) {
  TORCH_CHECK(logits.is_cuda(), "logits must be a GPU tensor");
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, V]");
  CHECK_LASTDIM_CONTIG(logits);
  const auto st = logits.scalar_type();
  TORCH_CHECK(st == at::kBFloat16 || st == at::kHalf || st == at::kFloat,
              "logits must be bf16, fp16 or fp32");
  TORCH_CHECK(logits.size(0) == 0 || logits.size(1) > 0, "empty vocabulary");
  TORCH_CHECK(logits.size(1) < (1L << 31) - 64, "vocabulary too large");
}

void check_vec(const torch::Tensor& t, const torch::Tensor& logits,
               at::ScalarType st, long n, const char* what) {
  TORCH_CHECK(t.device() == logits.device() && t.scalar_type() == st &&
                  t.dim() == 1 && t.is_contiguous() && t.size(0) == n,
              what, " must be a contiguous tensor of ", n, " ",
              c10::toString(st), " elements on the device of logits");
}

}  // namespace

torch::Tensor sample_rows(torch::Tensor logits, torch::Tensor temperature,
                          c10::optional<torch::Tensor> top_k,
                          c10::optional<torch::Tensor> top_p,
                          c10::optional<torch::Tensor> min_p,
                          torch::Tensor seed) {
  check_logits(logits);
  const int rows = logits.size(0);
  const int vocab = logits.size(1);
  check_vec(temperature, logits, at::kFloat, rows, "temperature");
  check_vec(seed, logits, at::kInt, rows, "seed");
  if (top_k) check_vec(*top_k, logits, at::kInt, rows, "top_k");
  if (top_p) check_vec(*top_p, logits, at::kFloat, rows, "top_p");
  if (min_p) check_vec(*min_p, logits, at::kFloat, rows, "min_p");
  auto out = torch::empty({rows}, logits.options().dtype(at::kLong));
  if (rows == 0) return out;
  hipStream_t stream_ = cmls::current_stream();
  const long stride = logits.stride(0);
  const auto st = logits.scalar_type();
  const float* tptr = temperature.data_ptr<float>();

  torch::Tensor tkey;
  unsigned int* kptr = nullptr;
  if (top_k || top_p || min_p) {
    tkey = torch::empty({rows}, logits.options().dtype(at::kInt));
    kptr = reinterpret_cast<unsigned int*>(tkey.data_ptr<int>());
    const int* kp = top_k ? top_k->data_ptr<int>() : nullptr;
    const float* pp = top_p ? top_p->data_ptr<float>() : nullptr;
    const float* mp = min_p ? min_p->data_ptr<float>() : nullptr;
    if (st == at::kBFloat16) {
      hipLaunchKernelGGL(sample_rows_select_kernel<__hip_bfloat16>,
                         dim3(rows), dim3(SEL_THREADS), 0, stream_,
                         (const __hip_bfloat16*)logits.data_ptr(), stride,
                         tptr, kp, pp, mp, kptr, vocab);
    } else if (st == at::kHalf) {
      hipLaunchKernelGGL(sample_rows_select_kernel<__half>, dim3(rows),
                         dim3(SEL_THREADS), 0, stream_,
                         (const __half*)logits.data_ptr(), stride, tptr, kp,
                         pp, mp, kptr, vocab);
    } else {
      hipLaunchKernelGGL(sample_rows_select_kernel<float>, dim3(rows),
                         dim3(SEL_THREADS), 0, stream_,
                         (const float*)logits.data_ptr(), stride, tptr, kp,
                         pp, mp, kptr, vocab);
    }
  }

  // vocabulary split as in token_mask.hip: never below 2048 tokens per
  // workgroup, chunk a multiple of 32
  int splits = std::max(1, std::min(16, 1024 / rows));
  splits = std::max(1, std::min(splits, (vocab + 2047) / 2048));
  const int chunk = (((vocab + splits - 1) / splits) + 31) / 32 * 32;
  splits = (vocab + chunk - 1) / chunk;
  torch::Tensor partial;
  unsigned long long* pptr = nullptr;
  long* optr = out.data_ptr<long>();
  if (splits > 1) {
    partial = torch::empty({rows, splits},
                           logits.options().dtype(at::kLong));
    pptr = reinterpret_cast<unsigned long long*>(partial.data_ptr<long>());
  }
  long* direct = splits > 1 ? nullptr : optr;
  const int* seedptr = seed.data_ptr<int>();
  dim3 grid(rows, splits);
  if (st == at::kBFloat16) {
    hipLaunchKernelGGL(sample_rows_draw_kernel<__hip_bfloat16>, grid,
                       dim3(256), 0, stream_,
                       (const __hip_bfloat16*)logits.data_ptr(), stride,
                       tptr, seedptr, kptr, pptr, direct, vocab, chunk);
  } else if (st == at::kHalf) {
    hipLaunchKernelGGL(sample_rows_draw_kernel<__half>, grid, dim3(256), 0,
                       stream_, (const __half*)logits.data_ptr(), stride,
                       tptr, seedptr, kptr, pptr, direct, vocab, chunk);
  } else {
    hipLaunchKernelGGL(sample_rows_draw_kernel<float>, grid, dim3(256), 0,
                       stream_, (const float*)logits.data_ptr(), stride,
                       tptr, seedptr, kptr, pptr, direct, vocab, chunk);
  }
  if (splits > 1) {
    hipLaunchKernelGGL(sample_rows_finalize_kernel, dim3((rows + 63) / 64),
                       dim3(64), 0, stream_, pptr, optr, rows, splits);
  }
  return out;
}

torch::Tensor apply_penalties(torch::Tensor logits, torch::Tensor tok,
                              torch::Tensor cnt, torch::Tensor flags,
                              torch::Tensor offsets, torch::Tensor presence,
                              torch::Tensor frequency,
                              torch::Tensor repetition) {
  check_logits(logits);
  const int rows = logits.size(0);
  const int vocab = logits.size(1);
  TORCH_CHECK(tok.dim() == 1 && tok.size(0) < (1L << 31), "tok must be [N]");
  const int n = tok.size(0);
  check_vec(tok, logits, at::kInt, n, "tok");
  check_vec(cnt, logits, at::kInt, n, "cnt");
  check_vec(flags, logits, at::kInt, n, "flags");
  check_vec(offsets, logits, at::kInt, rows + 1, "offsets");
  check_vec(presence, logits, at::kFloat, rows, "presence");
  check_vec(frequency, logits, at::kFloat, rows, "frequency");
  check_vec(repetition, logits, at::kFloat, rows, "repetition");
  auto out = torch::empty({rows, vocab}, logits.options());
  if (rows == 0) return out;
  hipStream_t stream_ = cmls::current_stream();
  const int block = 256;
  const int vec = 16 / (int)logits.element_size();
  const int chunks = std::max(
      1, std::min(1024, (vocab + block * vec - 1) / (block * vec)));
  const long stride = logits.stride(0);
  if (logits.element_size() == 2) {
    hipLaunchKernelGGL(copy_rows_kernel<unsigned short>, dim3(rows, chunks),
                       dim3(block), 0, stream_,
                       (const unsigned short*)logits.data_ptr(), stride,
                       (unsigned short*)out.data_ptr(), vocab);
  } else {
    hipLaunchKernelGGL(copy_rows_kernel<unsigned int>, dim3(rows, chunks),
                       dim3(block), 0, stream_,
                       (const unsigned int*)logits.data_ptr(), stride,
                       (unsigned int*)out.data_ptr(), vocab);
  }
  if (n == 0) return out;
  const dim3 grid((n + block - 1) / block);
  const auto st = logits.scalar_type();
#define LAUNCH_SCATTER(T)                                                   \
  hipLaunchKernelGGL(penalty_scatter_kernel<T>, grid, dim3(block), 0,       \
                     stream_, (T*)out.data_ptr(), tok.data_ptr<int>(),      \
                     cnt.data_ptr<int>(), flags.data_ptr<int>(),            \
                     offsets.data_ptr<int>(), presence.data_ptr<float>(),   \
                     frequency.data_ptr<float>(),                           \
                     repetition.data_ptr<float>(), rows, vocab, n)
  if (st == at::kBFloat16) {
    LAUNCH_SCATTER(__hip_bfloat16);
  } else if (st == at::kHalf) {
    LAUNCH_SCATTER(__half);
  } else {
    LAUNCH_SCATTER(float);
  }
#undef LAUNCH_SCATTER
  return out;
}
