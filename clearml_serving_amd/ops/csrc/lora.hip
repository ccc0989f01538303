// Batched multi-LoRA (BGMV-style) adapter kernels: every row of one batch
// may use a different adapter, or none. The reference gets this from vLLM's
// lora_modules (preprocess_service.py:715-720).
//
//   lora_shrink:      y[t]   = A[idx[t]] @ x[t]              fp32 [T, R]
//   lora_expand_add:  out[t] = bf16(float(out[t]) + B[idx[t]] @ y[t])
//
// x: bf16 [T, K]; A: bf16 [L, R, K]; B: bf16 [L, N, R] (alpha/r folded in at
// load time); idx: int32 [T] in [-1, L). Rows with idx == -1 are not touched
// by either kernel (one workgroup serves one token, so the exit is
// workgroup-uniform): shrink leaves y[t] unwritten and expand never reads it.
// PRECONDITION: idx[t] < L. Checking it here would need a device sync (and
// break graph capture); the engine builds idx from its own name->index map.
//
// Both are memory-bound GEMVs, not MFMA work: 16 B/lane loads, fp32
// accumulation. No allocation besides y, no host sync -- capturable.
#include "common.h"

namespace {

constexpr int SHRINK_THREADS = 256;                       // 4 waves
constexpr int SHRINK_ROWS_PER_WAVE = 4;                   // x chunk reused 4x
constexpr int SHRINK_ROWS_PER_BLOCK =
    (SHRINK_THREADS / WAVE_SIZE) * SHRINK_ROWS_PER_WAVE;  // 16 | R
constexpr int EXPAND_THREADS = 256;  // one output column per thread
constexpr int LORA_MAX_RANK = 256;

__device__ __forceinline__ float dot8(const bf16x8& a, const bf16x8& b,
                                      float acc) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc += to_f32(a.h[j]) * to_f32(b.h[j]);
  return acc;
}

// grid (T, R/16): a wave owns 4 consecutive rank rows of its token's adapter
// and walks K in 64-lane x 8-element chunks, so each x chunk is loaded once
// per 4 A rows; lanes past K/8 in the last chunk (K/8 % 64 != 0) idle.
__global__ __launch_bounds__(SHRINK_THREADS) void lora_shrink_kernel(
    const __hip_bfloat16* __restrict__ x, const __hip_bfloat16* __restrict__ a,
    const int* __restrict__ idx, float* __restrict__ y, int k, int r) {
  const int t = blockIdx.x;
  const int slot = idx[t];
  if (slot < 0) return;  // workgroup-uniform
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int r0 = blockIdx.y * SHRINK_ROWS_PER_BLOCK +
                 wave * SHRINK_ROWS_PER_WAVE;
  const uint32x4* xrow =
      reinterpret_cast<const uint32x4*>(x + (long)t * k);
  const __hip_bfloat16* abase = a + ((long)slot * r + r0) * k;
  const int chunks = k / 8;
  float acc[SHRINK_ROWS_PER_WAVE] = {0.f, 0.f, 0.f, 0.f};
  for (int c = lane; c < chunks; c += WAVE_SIZE) {
    bf16x8 xv;
    xv.u = xrow[c];
#pragma unroll
    for (int j = 0; j < SHRINK_ROWS_PER_WAVE; ++j) {
      bf16x8 av;
      av.u = reinterpret_cast<const uint32x4*>(abase + (long)j * k)[c];
      acc[j] = dot8(xv, av, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < SHRINK_ROWS_PER_WAVE; ++j) {
    const float s = wave_reduce_sum(acc[j]);
    if (lane == 0) y[(long)t * r + r0 + j] = s;
  }
}

// grid (T, ceil(N/256)): y[t] is staged once per workgroup in LDS (broadcast
// reads), each thread streams its own B row (R bf16, 16 B at a time) and
// updates one out element with a single rounding.
__global__ __launch_bounds__(EXPAND_THREADS) void lora_expand_add_kernel(
    const float* __restrict__ y, const __hip_bfloat16* __restrict__ b,
    const int* __restrict__ idx, __hip_bfloat16* __restrict__ out, int n,
    int r) {
  __shared__ float ys[LORA_MAX_RANK];
  const int t = blockIdx.x;
  const int slot = idx[t];
  if (slot < 0) return;  // workgroup-uniform, before any read of y
  for (int i = threadIdx.x; i < r; i += EXPAND_THREADS)
    ys[i] = y[(long)t * r + i];
  __syncthreads();
  const int col = blockIdx.y * EXPAND_THREADS + threadIdx.x;
  if (col >= n) return;  // tail block when N % 256 != 0
  const uint32x4* brow =
      reinterpret_cast<const uint32x4*>(b + ((long)slot * n + col) * r);
  float acc = 0.f;
  for (int c = 0; c < r / 8; ++c) {
    bf16x8 bv;
    bv.u = brow[c];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += to_f32(bv.h[j]) * ys[c * 8 + j];
  }
  __hip_bfloat16* o = out + (long)t * n + col;
  *o = __float2bfloat16(to_f32(*o) + acc);
}

void check_idx(const torch::Tensor& idx, const torch::Tensor& like, long t) {
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.dim() == 1 &&
                  idx.size(0) == t && idx.is_contiguous(),
              "lora: idx must be contiguous int32 [T]");
  TORCH_CHECK(idx.device() == like.device(), "lora: idx on another device");
}

void check_aligned(const torch::Tensor& v, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0, "lora: ",
              name, " must be 16-byte aligned");
}

void check_rank(long r) {
  TORCH_CHECK(r % 16 == 0 && r >= 16 && r <= LORA_MAX_RANK,
              "lora: R must be a multiple of 16 and <= 256, got ", r);
}

}  // namespace

torch::Tensor lora_shrink(torch::Tensor x, torch::Tensor a,
                          torch::Tensor idx) {
  TORCH_CHECK(x.is_cuda() && a.device() == x.device(),
              "lora_shrink: x and A must be on one GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                  a.scalar_type() == at::kBFloat16,
              "lora_shrink: x and A must be bf16");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(),
              "lora_shrink: x must be contiguous [T, K]");
  TORCH_CHECK(a.dim() == 3 && a.is_contiguous(),
              "lora_shrink: A must be contiguous [L, R, K]");
  const long t = x.size(0), k = x.size(1), r = a.size(1);
  TORCH_CHECK(t >= 1 && t <= INT_MAX, "lora_shrink: bad T ", t);
  TORCH_CHECK(a.size(0) >= 1 && a.size(2) == k,
              "lora_shrink: A must be [L>=1, R, K=", k, "]");
  TORCH_CHECK(k % 8 == 0 && k >= 8 && k <= INT_MAX,
              "lora_shrink: K must be a multiple of 8, got ", k);
  check_rank(r);
  check_idx(idx, x, t);
  check_aligned(x, "x");
  check_aligned(a, "A");
  auto y = torch::empty({t, r}, x.options().dtype(at::kFloat));
  dim3 grid((unsigned)t, (unsigned)(r / SHRINK_ROWS_PER_BLOCK));
  hipLaunchKernelGGL(lora_shrink_kernel, grid, dim3(SHRINK_THREADS), 0,
                     cmls::current_stream(),
                     (const __hip_bfloat16*)x.data_ptr(),
                     (const __hip_bfloat16*)a.data_ptr(), idx.data_ptr<int>(),
                     y.data_ptr<float>(), (int)k, (int)r);
  return y;
}

void lora_expand_add(torch::Tensor y, torch::Tensor b, torch::Tensor idx,
                     torch::Tensor out) {
  TORCH_CHECK(out.is_cuda() && b.device() == out.device() &&
                  y.device() == out.device(),
              "lora_expand_add: y, B and out must be on one GPU");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16,
              "lora_expand_add: B and out must be bf16");
  TORCH_CHECK(y.scalar_type() == at::kFloat && y.dim() == 2 &&
                  y.is_contiguous(),
              "lora_expand_add: y must be contiguous fp32 [T, R]");
  TORCH_CHECK(out.dim() == 2 && out.is_contiguous(),
              "lora_expand_add: out must be contiguous [T, N]");
  TORCH_CHECK(b.dim() == 3 && b.is_contiguous(),
              "lora_expand_add: B must be contiguous [L, N, R]");
  const long t = out.size(0), n = out.size(1), r = y.size(1);
  TORCH_CHECK(t >= 1 && t <= INT_MAX && y.size(0) == t,
              "lora_expand_add: y and out disagree on T");
  TORCH_CHECK(b.size(0) >= 1 && b.size(1) == n && b.size(2) == r,
              "lora_expand_add: B must be [L>=1, N=", n, ", R=", r, "]");
  TORCH_CHECK(n % 8 == 0 && n >= 8 && n <= INT_MAX,
              "lora_expand_add: N must be a multiple of 8, got ", n);
  check_rank(r);
  check_idx(idx, out, t);
  check_aligned(b, "B");
  const long nblk = (n + EXPAND_THREADS - 1) / EXPAND_THREADS;
  TORCH_CHECK(nblk <= 65535, "lora_expand_add: N too large");
  dim3 grid((unsigned)t, (unsigned)nblk);
  hipLaunchKernelGGL(lora_expand_add_kernel, grid, dim3(EXPAND_THREADS), 0,
                     cmls::current_stream(), y.data_ptr<float>(),
                     (const __hip_bfloat16*)b.data_ptr(), idx.data_ptr<int>(),
                     (__hip_bfloat16*)out.data_ptr(), (int)n, (int)r);
}
