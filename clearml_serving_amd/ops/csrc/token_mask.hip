// Guided decoding: token-bitmask kernels.
//
// A grammar state's allowed-token set is one row of a bitmask bank
// bank[S, W] (int32, W = ceil(V/32); token t is bit t&31 of word t>>5).
// slot[B] picks a bank row per logits row; slot -1 is an unconstrained row
// (a slot outside [0, S) reads no bank row and is treated the same way, so a
// bad slot can never index past the bank).
//
//   apply_token_bitmask   out-of-place copy with disallowed tokens at -inf;
//                         feeds the top-k/top-p, penalty and logprob paths.
//   sample_token_bitmask  fused mask + per-row greedy/gumbel-max draw for a
//                         heterogeneous batch (per-row temperature + seed).
//
// Both stream the logits once with 16-byte loads where the row base allows
// (scalar head/tail otherwise) and fetch the mask word once per vector: the
// lanes that share a word read the same address, which the memory pipeline
// serves as one request -- one word of traffic per 32 tokens.
//
// The draw reuses sampling.hip's scheme (pcg hash -> gumbel noise, orderable
// (value, index) pack, vocabulary split over gridDim.y) with two changes:
// the noise is hash(seed[row], token) -- no row index -- and the per-split
// winners land in their own partial slot instead of an atomicMax, so a row's
// token depends only on its logits, mask, temperature and seed, never on
// its position, the batch size or the split (and no memset launch is
// needed).
#include "common.h"

namespace {

// `n` (<= 32) mask bits for tokens t0..t0+n-1; bit i <-> token t0+i.
// t0 + n <= V is the caller's bound, so word t0>>5 exists; the second word
// is touched only when the run straddles a word boundary (never on the
// aligned vector path).
__device__ __forceinline__ unsigned int mask_bits(
    const unsigned int* __restrict__ mrow, int t0, int n) {
  if (mrow == nullptr) return 0xFFFFFFFFu;
  const int w = t0 >> 5;
  const int sh = t0 & 31;
  unsigned int bits = mrow[w] >> sh;
  if (sh + n > 32) bits |= mrow[w + 1] << (32 - sh);
  return bits;
}

// Elements of the scalar head before (p + i) reaches 16-byte alignment.
template <typename U>
__device__ __forceinline__ int head_elems(const U* p, int n) {
  const int mis = (int)((size_t)p & 15);
  const int head = mis ? (16 - mis) / (int)sizeof(U) : 0;
  return min(head, n);
}

// ------------------------------------------------------------------ //
// apply: works on the raw bit patterns (U = 16- or 32-bit element), so
// allowed values -- NaN payloads included -- are copied bit-identically.
// ------------------------------------------------------------------ //
template <typename U, unsigned int NEG_INF>
__global__ void apply_token_bitmask_kernel(
    const U* __restrict__ logits, long row_stride,
    const unsigned int* __restrict__ bank, const int* __restrict__ slot,
    U* __restrict__ out, int vocab, int n_slots, int words) {
  constexpr int VEC = 16 / sizeof(U);
  const int row = blockIdx.x;
  const U* src = logits + (long)row * row_stride;
  U* dst = out + (long)row * vocab;
  const int sl = slot[row];
  const unsigned int* mrow =
      (sl >= 0 && sl < n_slots) ? bank + (long)sl * words : nullptr;
  const int tid = blockIdx.y * blockDim.x + threadIdx.x;
  const int nthreads = gridDim.y * blockDim.x;

  // 16-byte path needs source and destination equally (mis)aligned
  const bool vec_ok = ((size_t)src & 15) == ((size_t)dst & 15);
  const int head = vec_ok ? head_elems(src, vocab) : vocab;
  const int nvec = vec_ok ? (vocab - head) / VEC : 0;
  const int tail0 = head + nvec * VEC;

  for (int v = tid; v < nvec; v += nthreads) {
    const int t0 = head + v * VEC;
    const unsigned int bits = mask_bits(mrow, t0, VEC);
    uint32x4 x = *reinterpret_cast<const uint32x4*>(src + t0);
    if (sizeof(U) == 2) {
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        unsigned int lo = x[d] & 0xFFFFu, hi = x[d] >> 16;
        if (!((bits >> (2 * d)) & 1u)) lo = NEG_INF;
        if (!((bits >> (2 * d + 1)) & 1u)) hi = NEG_INF;
        x[d] = lo | (hi << 16);
      }
    } else {
#pragma unroll
      for (int d = 0; d < 4; ++d)
        if (!((bits >> d) & 1u)) x[d] = NEG_INF;
    }
    *reinterpret_cast<uint32x4*>(dst + t0) = x;
  }
  // scalar head [0, head) and tail [tail0, vocab)
  const int nscalar = head + (vocab - tail0);
  for (int i = tid; i < nscalar; i += nthreads) {
    const int t = i < head ? i : tail0 + (i - head);
    const bool ok = mask_bits(mrow, t, 1) & 1u;
    dst[t] = ok ? src[t] : (U)NEG_INF;
  }
}

// ------------------------------------------------------------------ //
// sample
// ------------------------------------------------------------------ //
__device__ __forceinline__ unsigned int tm_pcg_hash(unsigned int x) {
  x = x * 747796405u + 2891336453u;
  unsigned int w = ((x >> ((x >> 28u) + 4u)) ^ x) * 277803737u;
  return (w >> 22u) ^ w;
}

// order-preserving float -> uint32 (works for +/-, inf)
__device__ __forceinline__ unsigned int tm_float_orderable(float f) {
  unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Running best of one thread as a packed key: (orderable score << 32) |
// (0xFFFFFFFF - token). Larger key wins, so equal scores resolve to the
// lowest token; key 0 = nothing allowed seen (orderable() of any non-NaN
// float is > 0).
struct Best {
  unsigned long long key;
  float inv_temp;       // 0 = greedy
  unsigned int row_seed;
  __device__ __forceinline__ void offer(int tok, float lg) {
    if (lg != lg) return;  // NaN never wins
    float s = lg;
    if (inv_temp != 0.0f) {
      const unsigned int h = tm_pcg_hash(row_seed + (unsigned int)tok);
      // exact in fp32, u in [2^-24, 1 - 2^-24]: the noise is always finite
      // (same arithmetic as sampling.hip)
      const float u = ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
      s = lg * inv_temp - __logf(-__logf(u));
    }
    if (s == 0.0f) s = 0.0f;  // -0.0 ties with +0.0, as in argmax
    const unsigned long long k =
        ((unsigned long long)tm_float_orderable(s) << 32) |
        (0xFFFFFFFFu - (unsigned int)tok);
    if (k > key) key = k;
  }
};

template <typename T>
__global__ void sample_token_bitmask_kernel(
    const T* __restrict__ logits, long row_stride,
    const unsigned int* __restrict__ bank, const int* __restrict__ slot,
    const float* __restrict__ temperature, const int* __restrict__ seed,
    unsigned long long* __restrict__ partial, long* __restrict__ out,
    int vocab, int n_slots, int words, int chunk) {
  constexpr int VEC = 16 / sizeof(T);
  const int row = blockIdx.x;
  const T* src = logits + (long)row * row_stride;
  const int sl = slot[row];
  const unsigned int* mrow =
      (sl >= 0 && sl < n_slots) ? bank + (long)sl * words : nullptr;
  const int lo = blockIdx.y * chunk;  // chunk is a multiple of 32
  const int hi = min(vocab, lo + chunk);
  const int n = max(hi - lo, 0);
  const float temp = temperature[row];

  Best best;
  best.key = 0ull;
  best.inv_temp = temp > 0.0f ? 1.0f / temp : 0.0f;
  best.row_seed = tm_pcg_hash((unsigned int)seed[row]);

  const int head = head_elems(src + lo, n);
  const int nvec = (n - head) / VEC;
  const int tail0 = lo + head + nvec * VEC;
  for (int v = threadIdx.x; v < nvec; v += blockDim.x) {
    const int t0 = lo + head + v * VEC;
    const unsigned int bits = mask_bits(mrow, t0, VEC);
    if (bits & ((1u << VEC) - 1u)) {
      union {
        uint32x4 u;
        T e[VEC];
      } x;
      x.u = *reinterpret_cast<const uint32x4*>(src + t0);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if ((bits >> j) & 1u) best.offer(t0 + j, to_f32(x.e[j]));
    }
  }
  const int nscalar = head + (hi - tail0);
  for (int i = threadIdx.x; i < nscalar; i += blockDim.x) {
    const int t = i < head ? lo + i : tail0 + (i - head);
    if (mask_bits(mrow, t, 1) & 1u) best.offer(t, to_f32(src[t]));
  }

  unsigned long long key = best.key;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(key, off, WAVE_SIZE);
    if (other > key) key = other;
  }
  __shared__ unsigned long long skeys[16];
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  if (lane == 0) skeys[wave] = key;
  __syncthreads();
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

__global__ void sample_finalize_kernel(
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

void check_mask_args(const torch::Tensor& logits, const torch::Tensor& bank,
                     const torch::Tensor& slot) {
  TORCH_CHECK(logits.is_cuda() && bank.is_cuda() && slot.is_cuda(),
              "logits, bank and slot must be GPU tensors");
  TORCH_CHECK(logits.dim() == 2, "logits must be [B, V]");
  CHECK_LASTDIM_CONTIG(logits);
  const auto st = logits.scalar_type();
  TORCH_CHECK(st == at::kBFloat16 || st == at::kHalf || st == at::kFloat,
              "logits must be bf16, fp16 or fp32");
  TORCH_CHECK(logits.size(0) == 0 || logits.size(1) > 0, "empty vocabulary");
  TORCH_CHECK(logits.size(1) < (1L << 31) - 64, "vocabulary too large");
  TORCH_CHECK(bank.scalar_type() == at::kInt, "bank must be int32");
  TORCH_CHECK(bank.dim() == 2 && bank.is_contiguous(),
              "bank must be contiguous [S, W]");
  TORCH_CHECK(bank.size(1) == (logits.size(1) + 31) / 32,
              "bank must have W = ceil(V/32) words per row, got ",
              bank.size(1), " for V = ", logits.size(1));
  TORCH_CHECK(slot.scalar_type() == at::kInt, "slot must be int32");
  TORCH_CHECK(slot.dim() == 1 && slot.is_contiguous() &&
                  slot.size(0) == logits.size(0),
              "slot must be contiguous [B]");
}

}  // namespace

torch::Tensor apply_token_bitmask(torch::Tensor logits, torch::Tensor bank,
                                  torch::Tensor slot) {
  check_mask_args(logits, bank, slot);
  const int rows = logits.size(0);
  const int vocab = logits.size(1);
  auto out = torch::empty({rows, vocab}, logits.options());
  if (rows == 0) return out;
  const int block = 256;
  const int vec = 16 / (int)logits.element_size();
  const int chunks = std::max(
      1, std::min(1024, (vocab + block * vec - 1) / (block * vec)));
  dim3 grid(rows, chunks);
  hipStream_t stream_ = cmls::current_stream();
  const auto* bptr = reinterpret_cast<const unsigned int*>(
      bank.data_ptr<int>());
  const int* sptr = slot.data_ptr<int>();
  const int n_slots = bank.size(0);
  const int words = bank.size(1);
  const long stride = logits.stride(0);
  const auto st = logits.scalar_type();
  if (st == at::kBFloat16) {
    hipLaunchKernelGGL(
        (apply_token_bitmask_kernel<unsigned short, 0xFF80u>), grid,
        dim3(block), 0, stream_, (const unsigned short*)logits.data_ptr(),
        stride, bptr, sptr, (unsigned short*)out.data_ptr(), vocab, n_slots,
        words);
  } else if (st == at::kHalf) {
    hipLaunchKernelGGL(
        (apply_token_bitmask_kernel<unsigned short, 0xFC00u>), grid,
        dim3(block), 0, stream_, (const unsigned short*)logits.data_ptr(),
        stride, bptr, sptr, (unsigned short*)out.data_ptr(), vocab, n_slots,
        words);
  } else {
    hipLaunchKernelGGL(
        (apply_token_bitmask_kernel<unsigned int, 0xFF800000u>), grid,
        dim3(block), 0, stream_, (const unsigned int*)logits.data_ptr(),
        stride, bptr, sptr, (unsigned int*)out.data_ptr(), vocab, n_slots,
        words);
  }
  return out;
}

torch::Tensor sample_token_bitmask(torch::Tensor logits, torch::Tensor bank,
                                   torch::Tensor slot,
                                   torch::Tensor temperature,
                                   torch::Tensor seed) {
  check_mask_args(logits, bank, slot);
  const int rows = logits.size(0);
  const int vocab = logits.size(1);
  TORCH_CHECK(temperature.is_cuda() && temperature.scalar_type() == at::kFloat
                  && temperature.dim() == 1 && temperature.is_contiguous()
                  && temperature.size(0) == rows,
              "temperature must be a contiguous float32 GPU tensor [B]");
  TORCH_CHECK(seed.is_cuda() && seed.scalar_type() == at::kInt
                  && seed.dim() == 1 && seed.is_contiguous()
                  && seed.size(0) == rows,
              "seed must be a contiguous int32 GPU tensor [B]");
  auto out = torch::empty({rows}, logits.options().dtype(at::kLong));
  if (rows == 0) return out;
  // vocabulary split as in sampling.hip (small decode batches would leave
  // most CUs idle), but never below 2048 tokens per workgroup
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
  dim3 grid(rows, splits);
  const int block = 256;
  hipStream_t stream_ = cmls::current_stream();
  const auto* bptr = reinterpret_cast<const unsigned int*>(
      bank.data_ptr<int>());
  const int* sptr = slot.data_ptr<int>();
  const float* tptr = temperature.data_ptr<float>();
  const int* seedptr = seed.data_ptr<int>();
  const int n_slots = bank.size(0);
  const int words = bank.size(1);
  const long stride = logits.stride(0);
  long* direct = splits > 1 ? nullptr : optr;
  const auto st = logits.scalar_type();
  if (st == at::kBFloat16) {
    hipLaunchKernelGGL(sample_token_bitmask_kernel<__hip_bfloat16>, grid,
                       dim3(block), 0, stream_,
                       (const __hip_bfloat16*)logits.data_ptr(), stride,
                       bptr, sptr, tptr, seedptr, pptr, direct, vocab,
                       n_slots, words, chunk);
  } else if (st == at::kHalf) {
    hipLaunchKernelGGL(sample_token_bitmask_kernel<__half>, grid,
                       dim3(block), 0, stream_,
                       (const __half*)logits.data_ptr(), stride, bptr, sptr,
                       tptr, seedptr, pptr, direct, vocab, n_slots, words,
                       chunk);
  } else {
    hipLaunchKernelGGL(sample_token_bitmask_kernel<float>, grid, dim3(block),
                       0, stream_, (const float*)logits.data_ptr(), stride,
                       bptr, sptr, tptr, seedptr, pptr, direct, vocab,
                       n_slots, words, chunk);
  }
  if (splits > 1) {
    hipLaunchKernelGGL(sample_finalize_kernel, dim3((rows + 63) / 64),
                       dim3(64), 0, stream_, pptr, optr, rows, splits);
  }
  return out;
}
