// Mixture-of-experts FFN for gfx950 (Mixtral-style top-k routed SwiGLU
// experts). The reference delegates MoE models to vLLM; here the block is
// five sync-free launches, so a decode step through it captures into the
// engine's hipGraphs:
//
//   moe_route    softmax over E router logits -> top-k ids + weights
//   moe_align    group the S = T*k (token, choice) slots by expert and pad
//                every expert's run to whole row blocks
//   gate/up      grouped skinny GEMM over w13[e] with a SwiGLU epilogue
//   down         grouped skinny GEMM over w2[e]
//   combine      out[t] = sum_j weights[t, j] * y[t*k + j]
//
// No device-to-host read anywhere and every output shape follows from the
// input shapes alone. Every reduction runs in a fixed order and nothing uses
// float atomics, so results are bit-reproducible and a token's output does
// not depend on which other tokens share its batch: one output element is
// one dot product whose k split over waves depends on K only.
//
// The grouped GEMMs reuse skinny_gemm.hip's design: one workgroup per
// (row block, 16 weight columns), 8 waves split K, mfma_f32_16x16x32_bf16
// with 16-byte lane loads straight from global and a deterministic LDS
// reduce. Expert weights stream once per row block; the gathered A rows are
// re-read by every column workgroup and ride in L2.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

#define MFMA16(A, B, C) \
  __builtin_amdgcn_mfma_f32_16x16x32_bf16((A), (B), (C), 0, 0, 0)

constexpr int MOE_MAX_E = 64;    // one lane per expert in moe_route
constexpr int MOE_MAX_K = 8;
constexpr int NT = 16;           // weight columns per workgroup
constexpr int NW = 8;            // waves (split K)
constexpr int KSTEP = 32;
constexpr int ROUTE_WAVES = 4;   // tokens per moe_route workgroup
constexpr int ALIGN_THREADS = 1024;

// ------------------------------------------------------------------- //
// route: one wave per token, lane e holds expert e
// ------------------------------------------------------------------- //
template <typename T>
__global__ __launch_bounds__(ROUTE_WAVES * 64) void moe_route_kernel(
    const T* __restrict__ logits,  // [T, E]
    int* __restrict__ ids,         // [T, k]
    float* __restrict__ weights,   // [T, k]
    int n_tok, int n_exp, int top_k, int renormalize) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * ROUTE_WAVES + (threadIdx.x >> 6);
  if (t >= n_tok) return;  // wave-uniform
  const bool live = lane < n_exp;
  const float v = live ? to_f32(logits[(long)t * n_exp + lane]) : -INFINITY;
  const float m = wave_reduce_max(v);
  const float p = live ? expf(v - m) : 0.f;
  // xor butterfly: every lane ends with the same bits (a + b == b + a)
  const float denom = wave_reduce_sum(p);
  const float prob = p / denom;

  // k rounds of wave arg-max on (logit, lowest index); lanes past E and
  // lanes already taken never win (k <= E keeps one candidate alive)
  bool taken = !live;
  float sel_w = 0.f;   // lane j < k keeps choice j
  int sel_id = 0;
  float wsum = 0.f;
  for (int j = 0; j < top_k; ++j) {
    float bv = v;
    int bi = lane;
    int bt = taken ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, WAVE_SIZE);
      const int oi = __shfl_xor(bi, off, WAVE_SIZE);
      const int ot = __shfl_xor(bt, off, WAVE_SIZE);
      const bool other = (ot < bt) ||
                         (ot == bt && (ov > bv || (ov == bv && oi < bi)));
      if (other) { bv = ov; bi = oi; bt = ot; }
    }
    const float w = __shfl(prob, bi, WAVE_SIZE);
    wsum += w;  // ascending j on every lane
    if (lane == j) { sel_w = w; sel_id = bi; }
    if (lane == bi) taken = true;
  }
  if (lane < top_k) {
    ids[(long)t * top_k + lane] = sel_id;
    weights[(long)t * top_k + lane] = renormalize ? sel_w / wsum : sel_w;
  }
}

// ------------------------------------------------------------------- //
// align: ONE workgroup, a stable counting sort of the S slots by expert.
// Wave w owns experts w, w+16, ...; it walks the slots 64 at a time and a
// ballot + popcount gives each matching slot its rank, so slots ascend
// within an expert with no atomics. Ids outside [0, E) match no expert and
// are dropped (never an out-of-range write).
// ------------------------------------------------------------------- //
__global__ __launch_bounds__(ALIGN_THREADS) void moe_align_kernel(
    const int* __restrict__ ids,      // [S]
    int* __restrict__ sorted_slots,   // [nb_max * block_m]
    int* __restrict__ block_expert,   // [nb_max]
    int n_slots, int n_exp, int block_m, int nb_max) {
  __shared__ int count[MOE_MAX_E];
  __shared__ int first_block[MOE_MAX_E + 1];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int n_waves = ALIGN_THREADS / 64;

  for (int i = threadIdx.x; i < nb_max * block_m; i += ALIGN_THREADS)
    sorted_slots[i] = n_slots;  // sentinel
  for (int i = threadIdx.x; i < nb_max; i += ALIGN_THREADS)
    block_expert[i] = -1;

  for (int e = wave; e < n_exp; e += n_waves) {
    int c = 0;
    for (int s0 = 0; s0 < n_slots; s0 += 64) {
      const int s = s0 + lane;
      const bool hit = s < n_slots && ids[s] == e;
      c += __popcll(__ballot(hit));
    }
    if (lane == 0) count[e] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int b = 0;
    for (int e = 0; e < n_exp; ++e) {
      first_block[e] = b;
      b += (count[e] + block_m - 1) / block_m;
    }
    first_block[n_exp] = b;  // <= nb_max by construction
  }
  __syncthreads();  // also orders the sentinel fill before the writes below

  for (int e = wave; e < n_exp; e += n_waves) {
    const int b0 = first_block[e];
    const int nb = first_block[e + 1] - b0;
    for (int i = lane; i < nb; i += 64) block_expert[b0 + i] = e;
    int run = 0;
    for (int s0 = 0; s0 < n_slots; s0 += 64) {
      const int s = s0 + lane;
      const bool hit = s < n_slots && ids[s] == e;
      const unsigned long long mask = __ballot(hit);
      if (hit) {
        const int rank = run + __popcll(mask & ((1ull << lane) - 1ull));
        sorted_slots[(long)b0 * block_m + rank] = s;
      }
      run += __popcll(mask);
    }
  }
}

// ------------------------------------------------------------------- //
// grouped skinny GEMM. grid (N/16, nb_max), block 8 waves, MT 16-row tiles
// per row block (block_m = 16 * MT).
//   GATED:  A row = x[slot / k], W = w13[e] ([2N, K], gate rows then up
//           rows), out = bf16 act[slot, n] = silu(g) * u
//   !GATED: A row = act[slot],   W = w2[e] ([N, K]), out = fp32 y[slot, n]
// Sentinel rows (slot == n_slots) replay row 0 and never store; a block
// whose expert is -1 exits at once (workgroup-uniform).
// ------------------------------------------------------------------- //
template <int MT, bool GATED>
__global__ __launch_bounds__(NW * 64, 2) void moe_gemm_kernel(
    const __hip_bfloat16* __restrict__ a,   // [T, K] or [S, K]
    const __hip_bfloat16* __restrict__ w,   // [E, (2)N, K]
    const int* __restrict__ sorted_slots,
    const int* __restrict__ block_expert,
    void* __restrict__ out,                 // bf16 [S, N] or fp32 [S, N]
    int n_slots, int top_k, int N, int K) {
  const int e = block_expert[blockIdx.y];
  if (e < 0) return;
  const int n0 = blockIdx.x * NT;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = lane & 15;         // fragment row (m or n within tile)
  const int koff = (lane >> 4) * 8;  // fragment k offset within KSTEP
  const int* slots = sorted_slots + (long)blockIdx.y * (MT * 16);

  // wave's K range (K % (NW*KSTEP) handled by the last wave's bound)
  const int kchunk = ((K / KSTEP + NW - 1) / NW) * KSTEP;
  const int k_lo = wave * kchunk;
  const int k_hi = min(K, k_lo + kchunk);

  const long w_rows = GATED ? 2L * N : (long)N;
  const __hip_bfloat16* wbase = w + (long)e * w_rows * K;
  const __hip_bfloat16* wrow0 = wbase + (long)(n0 + row) * K + koff;
  const __hip_bfloat16* wrow1 = wrow0 + (long)N * K;  // up rows (GATED)

  const __hip_bfloat16* arow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    int s = slots[t * 16 + row];
    if (s >= n_slots) s = 0;  // sentinel: replay a valid row
    const long r = GATED ? s / top_k : s;
    arow[t] = a + r * K + koff;
  }

  f32x4_t acc0[MT], acc1[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc0[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    acc1[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  int k = k_lo;
  for (; k + 2 * KSTEP <= k_hi; k += 2 * KSTEP) {
    const bf16x8_t g0 = *reinterpret_cast<const bf16x8_t*>(wrow0 + k);
    const bf16x8_t g1 = *reinterpret_cast<const bf16x8_t*>(wrow0 + k + KSTEP);
    bf16x8_t u0, u1;
    if (GATED) {
      u0 = *reinterpret_cast<const bf16x8_t*>(wrow1 + k);
      u1 = *reinterpret_cast<const bf16x8_t*>(wrow1 + k + KSTEP);
    }
    bf16x8_t a0[MT], a1[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      a0[t] = *reinterpret_cast<const bf16x8_t*>(arow[t] + k);
      a1[t] = *reinterpret_cast<const bf16x8_t*>(arow[t] + k + KSTEP);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc0[t] = MFMA16(a0[t], g0, acc0[t]);
      if (GATED) acc1[t] = MFMA16(a0[t], u0, acc1[t]);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc0[t] = MFMA16(a1[t], g1, acc0[t]);
      if (GATED) acc1[t] = MFMA16(a1[t], u1, acc1[t]);
    }
  }
  for (; k < k_hi; k += KSTEP) {
    const bf16x8_t g = *reinterpret_cast<const bf16x8_t*>(wrow0 + k);
    bf16x8_t u;
    if (GATED) u = *reinterpret_cast<const bf16x8_t*>(wrow1 + k);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const bf16x8_t av = *reinterpret_cast<const bf16x8_t*>(arow[t] + k);
      acc0[t] = MFMA16(av, g, acc0[t]);
      if (GATED) acc1[t] = MFMA16(av, u, acc1[t]);
    }
  }

  // deterministic cross-wave K reduction through LDS, as skinny_gemm:
  // lds[half][wave][m][n]; wave 0 sums the waves in a fixed order
  // GATED with MT = 4 is 2*8*64*16*4 B = 64 KB, exactly the static LDS limit:
  // a larger row block (MT up to 8 as in skinny_gemm) does not build until
  // this reduce is restructured (gate and up through one buffer in turn, or
  // fewer waves' partials staged at a time).
  constexpr int HALVES = GATED ? 2 : 1;
  __shared__ float lds[HALVES][NW][MT * 16][NT];
  const int crow = (lane >> 4) * 4;  // C fragment rows
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lds[0][wave][t * 16 + crow + r][lane & 15] = acc0[t][r];
      if (GATED) lds[HALVES - 1][wave][t * 16 + crow + r][lane & 15] =
          acc1[t][r];
    }
  }
  __syncthreads();
  if (wave == 0) {
    const int n = lane & 15;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mrow = t * 16 + crow + r;
        const int s = slots[mrow];
        float g = 0.f, u = 0.f;
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) {
          g += lds[0][wv][mrow][n];
          if (GATED) u += lds[HALVES - 1][wv][mrow][n];
        }
        if (s < n_slots) {
          if (GATED) {
            const float act = g / (1.f + expf(-g)) * u;
            reinterpret_cast<__hip_bfloat16*>(out)[(long)s * N + n0 + n] =
                __float2bfloat16(act);
          } else {
            reinterpret_cast<float*>(out)[(long)s * N + n0 + n] = g;
          }
        }
      }
    }
  }
}

// combine: one thread per 4 consecutive columns of one token
__global__ __launch_bounds__(256) void moe_combine_kernel(
    const float* __restrict__ y,        // [T*k, H]
    const float* __restrict__ weights,  // [T, k]
    __hip_bfloat16* __restrict__ out,   // [T, H]
    int top_k, int H) {
  const int t = blockIdx.x;
  const int c = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (c >= H) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < top_k; ++j) {  // ascending j, fp32
    const float wj = weights[(long)t * top_k + j];
    const floatx4 v = *reinterpret_cast<const floatx4*>(
        y + ((long)t * top_k + j) * H + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += wj * v[i];
  }
  union { uint32x2 u; __hip_bfloat16 h[4]; } o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o.h[i] = __float2bfloat16(acc[i]);
  *reinterpret_cast<uint32x2*>(out + (long)t * H + c) = o.u;
}

long moe_nb_max(long s, long e, long block_m) {
  return (s + std::min(e, s) * (block_m - 1)) / block_m;
}

void check_ids(const torch::Tensor& ids, const char* op) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kInt &&
                  ids.dim() == 2 && ids.is_contiguous(),
              op, ": ids must be contiguous int32 [T, k] on the GPU");
  TORCH_CHECK(ids.size(0) >= 1 && ids.size(1) >= 1 &&
                  ids.size(1) <= MOE_MAX_K,
              op, ": need T >= 1 and 1 <= k <= ", MOE_MAX_K);
  TORCH_CHECK(ids.numel() <= INT_MAX / 2, op, ": T * k too large");
}

void check_aligned16(const torch::Tensor& v, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0, "moe: ",
              name, " must be 16-byte aligned");
}

void launch_align(const torch::Tensor& ids, long n_exp, long block_m,
                  torch::Tensor& sorted_slots, torch::Tensor& block_expert) {
  const long s = ids.numel();
  const long nb_max = moe_nb_max(s, n_exp, block_m);
  auto opt = ids.options();
  sorted_slots = torch::empty({nb_max * block_m}, opt);
  block_expert = torch::empty({nb_max}, opt);
  hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(ALIGN_THREADS), 0,
                     cmls::current_stream(), ids.data_ptr<int>(),
                     sorted_slots.data_ptr<int>(),
                     block_expert.data_ptr<int>(), (int)s, (int)n_exp,
                     (int)block_m, (int)nb_max);
}

}  // namespace

std::vector<torch::Tensor> moe_route(torch::Tensor logits, int64_t top_k,
                                     bool renormalize) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous(),
              "moe_route: logits must be contiguous [T, E] on the GPU");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 ||
                  logits.scalar_type() == at::kFloat,
              "moe_route: logits must be bf16 or fp32");
  const long t = logits.size(0), e = logits.size(1);
  TORCH_CHECK(t >= 1 && t <= INT_MAX / MOE_MAX_K, "moe_route: bad T ", t);
  TORCH_CHECK(top_k >= 1 && top_k <= MOE_MAX_K && top_k <= e &&
                  e <= MOE_MAX_E,
              "moe_route: need 1 <= k <= ", MOE_MAX_K, " and k <= E <= ",
              MOE_MAX_E, ", got k=", top_k, " E=", e);
  auto ids = torch::empty({t, top_k}, logits.options().dtype(at::kInt));
  auto weights = torch::empty({t, top_k}, logits.options().dtype(at::kFloat));
  dim3 grid((unsigned)((t + ROUTE_WAVES - 1) / ROUTE_WAVES));
  if (logits.scalar_type() == at::kFloat) {
    hipLaunchKernelGGL(moe_route_kernel<float>, grid, dim3(ROUTE_WAVES * 64),
                       0, cmls::current_stream(), logits.data_ptr<float>(),
                       ids.data_ptr<int>(), weights.data_ptr<float>(), (int)t,
                       (int)e, (int)top_k, (int)renormalize);
  } else {
    hipLaunchKernelGGL(moe_route_kernel<__hip_bfloat16>, grid,
                       dim3(ROUTE_WAVES * 64), 0, cmls::current_stream(),
                       (const __hip_bfloat16*)logits.data_ptr(),
                       ids.data_ptr<int>(), weights.data_ptr<float>(), (int)t,
                       (int)e, (int)top_k, (int)renormalize);
  }
  return {ids, weights};
}

std::vector<torch::Tensor> moe_align(torch::Tensor ids, int64_t num_experts,
                                     int64_t block_m) {
  check_ids(ids, "moe_align");
  TORCH_CHECK(num_experts >= 1 && num_experts <= MOE_MAX_E,
              "moe_align: need 1 <= E <= ", MOE_MAX_E, ", got ", num_experts);
  TORCH_CHECK(block_m >= 1 && block_m <= 1024, "moe_align: bad block_m ",
              block_m);
  torch::Tensor sorted_slots, block_expert;
  launch_align(ids, num_experts, block_m, sorted_slots, block_expert);
  return {sorted_slots, block_expert};
}

torch::Tensor moe_experts(torch::Tensor x, torch::Tensor w13, torch::Tensor w2,
                          torch::Tensor ids, torch::Tensor weights,
                          int64_t block_m) {
  TORCH_CHECK(x.is_cuda() && w13.device() == x.device() &&
                  w2.device() == x.device() && ids.device() == x.device() &&
                  weights.device() == x.device(),
              "moe_experts: all operands must be on one GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
                  w13.scalar_type() == at::kBFloat16 &&
                  w2.scalar_type() == at::kBFloat16,
              "moe_experts: x, w13 and w2 must be bf16");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(),
              "moe_experts: x must be contiguous [T, H]");
  TORCH_CHECK(w13.dim() == 3 && w13.is_contiguous() && w2.dim() == 3 &&
                  w2.is_contiguous(),
              "moe_experts: w13 [E, 2I, H] and w2 [E, H, I] must be "
              "contiguous");
  const long t = x.size(0), h = x.size(1);
  const long e = w13.size(0), inter = w2.size(2);
  TORCH_CHECK(w13.size(1) == 2 * inter && w13.size(2) == h &&
                  w2.size(0) == e && w2.size(1) == h,
              "moe_experts: w13 must be [E, 2I, H] and w2 [E, H, I]");
  check_ids(ids, "moe_experts");
  const long k = ids.size(1), s = t * k;
  TORCH_CHECK(ids.size(0) == t, "moe_experts: ids and x disagree on T");
  TORCH_CHECK(e >= 1 && e <= MOE_MAX_E && k <= e,
              "moe_experts: need k <= E <= ", MOE_MAX_E, ", got k=", k,
              " E=", e);
  TORCH_CHECK(weights.scalar_type() == at::kFloat && weights.dim() == 2 &&
                  weights.size(0) == t && weights.size(1) == k &&
                  weights.is_contiguous(),
              "moe_experts: weights must be contiguous fp32 [T, k]");
  TORCH_CHECK(h % KSTEP == 0 && h >= KSTEP && h <= INT_MAX,
              "moe_experts: H must be a multiple of 32, got ", h);
  TORCH_CHECK(inter % KSTEP == 0 && inter >= KSTEP && inter <= INT_MAX,
              "moe_experts: I must be a multiple of 32, got ", inter);
  TORCH_CHECK(block_m == 16 || block_m == 64,
              "moe_experts: block_m must be 16 or 64, got ", block_m);
  check_aligned16(x, "x");
  check_aligned16(w13, "w13");
  check_aligned16(w2, "w2");

  torch::Tensor sorted_slots, block_expert;
  launch_align(ids, e, block_m, sorted_slots, block_expert);
  const long nb_max = block_expert.size(0);
  TORCH_CHECK(nb_max <= 65535, "moe_experts: too many row blocks (", nb_max,
              "); raise block_m or split the batch");

  auto act = torch::empty({s, inter}, x.options());
  auto y = torch::empty({s, h}, x.options().dtype(at::kFloat));
  auto out = torch::empty({t, h}, x.options());
  hipStream_t stream_ = cmls::current_stream();
  const int* ss = sorted_slots.data_ptr<int>();
  const int* be = block_expert.data_ptr<int>();
#define LAUNCH_MOE(MT, GATED, A, W, OUT, N, K)                              \
  hipLaunchKernelGGL((moe_gemm_kernel<MT, GATED>),                          \
                     dim3((unsigned)((N) / NT), (unsigned)nb_max),          \
                     dim3(NW * 64), 0, stream_,                             \
                     (const __hip_bfloat16*)(A).data_ptr(),                 \
                     (const __hip_bfloat16*)(W).data_ptr(), ss, be,         \
                     (OUT).data_ptr(), (int)s, (int)k, (int)(N), (int)(K))
  if (block_m == 16) {
    LAUNCH_MOE(1, true, x, w13, act, inter, h);
    LAUNCH_MOE(1, false, act, w2, y, h, inter);
  } else {
    LAUNCH_MOE(4, true, x, w13, act, inter, h);
    LAUNCH_MOE(4, false, act, w2, y, h, inter);
  }
#undef LAUNCH_MOE
  const long cblk = (h / 4 + 255) / 256;
  TORCH_CHECK(t <= INT_MAX && cblk <= 65535, "moe_experts: shape too large");
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)t, (unsigned)cblk),
                     dim3(256), 0, stream_, y.data_ptr<float>(),
                     weights.data_ptr<float>(),
                     (__hip_bfloat16*)out.data_ptr(), (int)k, (int)h);
  return out;
}
