// Mixture-of-experts FFN with fp8 (OCP e4m3) expert weights for gfx950.
//
// An MoE decode step is expert-weight streaming and little else: fp8 experts
// halve those bytes. The block keeps moe.hip's sync-free, capturable shape
// and reuses its align and combine stages (moe.h):
//
//   moe_align    group the S = T*k slots by expert            (moe.hip)
//   gate/up      grouped fp8 GEMM over w13[e], SwiGLU epilogue -> bf16 act
//   quant_fp8    act rows -> e4m3 bytes + per-row scale       (fp8_path.hip)
//   down         grouped fp8 GEMM over w2[e]                   -> fp32 y
//   combine      out[t] = sum_j weights[t, j] * y[t*k + j]    (moe.hip)
//
// moe_gemm_fp8_kernel: one workgroup per (row block, 16 weight columns), 8
// waves split K in whole 64-wide window pairs, mfma_f32_16x16x32_fp8_fp8.
//   weights      e4m3 bytes in the swizzle_fp8_weight layout: one 16-byte
//                lane load is both MFMA B operands of a window pair, so a
//                weight row costs HALF the load requests of the bf16 kernel
//                per k (the request rate, not only the bytes, bounds decode)
//   activations  gathered through sorted_slots from a row-major e4m3
//                matrix, two 8-byte loads per pair (+8g, +32+8g); they are
//                re-read by every column workgroup and ride in L2
//   reduction    every wave parks its partial tile in LDS; then ALL 512
//                threads (not wave 0 alone) each own output elements and sum
//                the 8 partials in wave order 0..7. One output element is one
//                dot product whose k split depends on K only, so results are
//                bit-reproducible, batch-invariant and the same for either
//                row block; no float atomics anywhere.
//   scaling      sum * a_scale[row] * w_scale[e, n], fp32 per activation row
//                and per (expert, output row)
#include "moe.h"

// fp8_path.hip: per-row absmax quantisation to e4m3, {bytes [R, C], scale [R]}
std::vector<torch::Tensor> quant_fp8(torch::Tensor x);

namespace {

typedef __attribute__((ext_vector_type(2))) long longx2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

#define MFMA16F8(A, B, C) \
  __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((A), (B), (C), 0, 0, 0)

constexpr int NT = 16;     // weight columns per workgroup
constexpr int NW = 8;      // waves (split K)
constexpr int KPAIR = 64;  // k per 16-byte weight load (two MFMA windows)

// grid (N/16, nb_max), block 8 waves, MT 16-row tiles per row block.
//   GATED:  A row = a[slot / k], W = w13[e] ([2N, K], gate rows then up
//           rows), out = bf16 act[slot, n] = silu(g) * u
//   !GATED: A row = a[slot],     W = w2[e] ([N, K]), out = fp32 y[slot, n]
// a_scale is indexed like a's rows, w_scale like w's rows. Sentinel rows
// (slot == n_slots) replay row 0 and never store; a block whose expert is -1
// exits at once (workgroup-uniform, before any barrier).
//
// The target attribute keeps the compiler from pairing the gate and up sums
// of the epilogue into packed fp32 VALU ops (v_pk_add_f32 / v_pk_mul_f32):
// plain v_add / v_mul only. It is set here rather than as a build flag so
// that no other file's code generation changes.
template <int MT, bool GATED>
__global__ __launch_bounds__(NW * 64, 2)
__attribute__((target("no-packed-fp32-ops"))) void moe_gemm_fp8_kernel(
    const unsigned char* __restrict__ a,   // [T, K] or [S, K] e4m3
    const float* __restrict__ a_scale,     // [T] or [S]
    const unsigned char* __restrict__ w,   // [E, (2)N, K] e4m3, swizzled
    const float* __restrict__ w_scale,     // [E, (2)N]
    const int* __restrict__ sorted_slots,
    const int* __restrict__ block_expert,
    void* __restrict__ out,                // bf16 [S, N] or fp32 [S, N]
    int n_slots, int top_k, int N, int K) {
  const int e = block_expert[blockIdx.y];
  if (e < 0) return;
  const int n0 = blockIdx.x * NT;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = lane & 15;  // fragment row (m or n within the tile)
  const int g = lane >> 4;    // lane group: k bytes 8g.. of each window
  const int* slots = sorted_slots + (long)blockIdx.y * (MT * 16);

  // whole window pairs per wave; the last wave that has work takes the
  // bound and the waves past it get k_lo >= k_hi, an empty range
  const int kchunk = ((K / KPAIR + NW - 1) / NW) * KPAIR;
  const int k_lo = wave * kchunk;
  const int k_hi = min(K, k_lo + kchunk);

  const long w_rows = GATED ? 2L * N : (long)N;
  const unsigned char* wrow0 =
      w + ((long)e * w_rows + n0 + row) * K + 16 * g;
  const unsigned char* wrow1 = wrow0 + (long)N * K;  // up rows (GATED)

  const unsigned char* arow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    int s = slots[t * 16 + row];
    if (s >= n_slots) s = 0;  // sentinel: replay a valid row
    const long r = GATED ? s / top_k : s;
    arow[t] = a + r * K + 8 * g;
  }

  f32x4_t acc0[MT], acc1[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc0[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    acc1[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  int k = k_lo;
  for (; k + 2 * KPAIR <= k_hi; k += 2 * KPAIR) {
    const longx2_t g0 = *reinterpret_cast<const longx2_t*>(wrow0 + k);
    const longx2_t g1 = *reinterpret_cast<const longx2_t*>(wrow0 + k + KPAIR);
    longx2_t u0, u1;
    if (GATED) {
      u0 = *reinterpret_cast<const longx2_t*>(wrow1 + k);
      u1 = *reinterpret_cast<const longx2_t*>(wrow1 + k + KPAIR);
    }
    long a0[MT], a1[MT], a2[MT], a3[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      a0[t] = *reinterpret_cast<const long*>(arow[t] + k);
      a1[t] = *reinterpret_cast<const long*>(arow[t] + k + 32);
      a2[t] = *reinterpret_cast<const long*>(arow[t] + k + KPAIR);
      a3[t] = *reinterpret_cast<const long*>(arow[t] + k + KPAIR + 32);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc0[t] = MFMA16F8(a0[t], g0[0], acc0[t]);
      acc0[t] = MFMA16F8(a1[t], g0[1], acc0[t]);
      if (GATED) {
        acc1[t] = MFMA16F8(a0[t], u0[0], acc1[t]);
        acc1[t] = MFMA16F8(a1[t], u0[1], acc1[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc0[t] = MFMA16F8(a2[t], g1[0], acc0[t]);
      acc0[t] = MFMA16F8(a3[t], g1[1], acc0[t]);
      if (GATED) {
        acc1[t] = MFMA16F8(a2[t], u1[0], acc1[t]);
        acc1[t] = MFMA16F8(a3[t], u1[1], acc1[t]);
      }
    }
  }
  for (; k < k_hi; k += KPAIR) {
    const longx2_t gw = *reinterpret_cast<const longx2_t*>(wrow0 + k);
    longx2_t uw;
    if (GATED) uw = *reinterpret_cast<const longx2_t*>(wrow1 + k);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const long aa = *reinterpret_cast<const long*>(arow[t] + k);
      const long ab = *reinterpret_cast<const long*>(arow[t] + k + 32);
      acc0[t] = MFMA16F8(aa, gw[0], acc0[t]);
      acc0[t] = MFMA16F8(ab, gw[1], acc0[t]);
      if (GATED) {
        acc1[t] = MFMA16F8(aa, uw[0], acc1[t]);
        acc1[t] = MFMA16F8(ab, uw[1], acc1[t]);
      }
    }
  }

  // lds[half][wave][m][n]: GATED with MT = 4 is 2*8*64*16*4 B = 64 KB, the
  // static LDS limit (as the bf16 kernel). Waves with an empty k range park
  // zeros, so the sum below always runs over all NW partials.
  constexpr int HALVES = GATED ? 2 : 1;
  __shared__ float lds[HALVES][NW][MT * 16][NT];
  const int crow = g * 4;  // C fragment rows
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      lds[0][wave][t * 16 + crow + r][row] = acc0[t][r];
      if (GATED) lds[HALVES - 1][wave][t * 16 + crow + r][row] = acc1[t][r];
    }
  }
  __syncthreads();

  // every thread owns output elements o = m * 16 + n: consecutive lanes read
  // consecutive LDS words (no bank conflict) and store consecutive columns
  const float* wsc = w_scale + (long)e * w_rows + n0;
  constexpr int OUTS = MT * 16 * NT;
  for (int o = threadIdx.x; o < OUTS; o += NW * 64) {
    const int mrow = o >> 4;
    const int n = o & 15;
    const int s = slots[mrow];
    if (s >= n_slots) continue;
    float gs = 0.f, us = 0.f;
#pragma unroll
    for (int wv = 0; wv < NW; ++wv) {  // fixed wave order
      gs += lds[0][wv][mrow][n];
      if (GATED) us += lds[HALVES - 1][wv][mrow][n];
    }
    const float as = a_scale[GATED ? s / top_k : s];
    const float gv = gs * as * wsc[n];
    if (GATED) {
      const float uv = us * as * wsc[N + n];
      const float act = gv / (1.f + expf(-gv)) * uv;
      reinterpret_cast<__hip_bfloat16*>(out)[(long)s * N + n0 + n] =
          __float2bfloat16(act);
    } else {
      reinterpret_cast<float*>(out)[(long)s * N + n0 + n] = gv;
    }
  }
}

bool is_fp8_bytes(const torch::Tensor& v) {
  return v.scalar_type() == at::kByte ||
         v.scalar_type() == at::kFloat8_e4m3fn;
}

void check_aligned16(const torch::Tensor& v, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0,
              "moe_experts_fp8: ", name, " must be 16-byte aligned");
}

void check_scale(const torch::Tensor& v, const torch::Tensor& like,
                 long numel, const char* name) {
  TORCH_CHECK(v.device() == like.device() &&
                  v.scalar_type() == at::kFloat && v.is_contiguous() &&
                  v.numel() == numel,
              "moe_experts_fp8: ", name, " must be contiguous fp32 with ",
              numel, " elements on the operands' GPU");
}

}  // namespace

torch::Tensor moe_experts_fp8(torch::Tensor x8, torch::Tensor x_scale,
                              torch::Tensor w13_8, torch::Tensor w13_scale,
                              torch::Tensor w2_8, torch::Tensor w2_scale,
                              torch::Tensor ids, torch::Tensor weights,
                              int64_t block_m) {
  TORCH_CHECK(x8.is_cuda() && w13_8.device() == x8.device() &&
                  w2_8.device() == x8.device() &&
                  ids.device() == x8.device() &&
                  weights.device() == x8.device(),
              "moe_experts_fp8: all operands must be on one GPU");
  TORCH_CHECK(is_fp8_bytes(x8) && is_fp8_bytes(w13_8) && is_fp8_bytes(w2_8),
              "moe_experts_fp8: x8, w13_8 and w2_8 must be uint8 / e4m3");
  TORCH_CHECK(x8.dim() == 2 && x8.is_contiguous(),
              "moe_experts_fp8: x8 must be contiguous [T, H]");
  TORCH_CHECK(w13_8.dim() == 3 && w13_8.is_contiguous() &&
                  w2_8.dim() == 3 && w2_8.is_contiguous(),
              "moe_experts_fp8: w13_8 [E, 2I, H] and w2_8 [E, H, I] must be "
              "contiguous");
  const long t = x8.size(0), h = x8.size(1);
  const long e = w13_8.size(0), inter = w2_8.size(2);
  TORCH_CHECK(w13_8.size(1) == 2 * inter && w13_8.size(2) == h &&
                  w2_8.size(0) == e && w2_8.size(1) == h,
              "moe_experts_fp8: w13_8 must be [E, 2I, H] and w2_8 [E, H, I]");
  cmls_moe::check_ids(ids, "moe_experts_fp8");
  const long k = ids.size(1), s = t * k;
  TORCH_CHECK(ids.size(0) == t, "moe_experts_fp8: ids and x8 disagree on T");
  TORCH_CHECK(e >= 1 && e <= cmls_moe::MAX_E && k <= e,
              "moe_experts_fp8: need k <= E <= ", cmls_moe::MAX_E,
              ", got k=", k, " E=", e);
  TORCH_CHECK(weights.scalar_type() == at::kFloat && weights.dim() == 2 &&
                  weights.size(0) == t && weights.size(1) == k &&
                  weights.is_contiguous(),
              "moe_experts_fp8: weights must be contiguous fp32 [T, k]");
  TORCH_CHECK(h % KPAIR == 0 && h >= KPAIR && h <= INT_MAX,
              "moe_experts_fp8: H must be a multiple of 64, got ", h);
  TORCH_CHECK(inter % KPAIR == 0 && inter >= KPAIR && inter <= INT_MAX,
              "moe_experts_fp8: I must be a multiple of 64, got ", inter);
  TORCH_CHECK(block_m == 16 || block_m == 64,
              "moe_experts_fp8: block_m must be 16 or 64, got ", block_m);
  check_scale(x_scale, x8, t, "x_scale");
  check_scale(w13_scale, x8, e * 2 * inter, "w13_scale");
  check_scale(w2_scale, x8, e * h, "w2_scale");
  check_aligned16(x8, "x8");
  check_aligned16(w13_8, "w13_8");
  check_aligned16(w2_8, "w2_8");

  torch::Tensor sorted_slots, block_expert;
  cmls_moe::launch_align(ids, e, block_m, sorted_slots, block_expert);
  const long nb_max = block_expert.size(0);
  TORCH_CHECK(nb_max <= 65535, "moe_experts_fp8: too many row blocks (",
              nb_max, "); raise block_m or split the batch");

  auto act = torch::empty({s, inter}, x8.options().dtype(at::kBFloat16));
  auto y = torch::empty({s, h}, x8.options().dtype(at::kFloat));
  auto out = torch::empty({t, h}, x8.options().dtype(at::kBFloat16));
  hipStream_t stream_ = cmls::current_stream();
  const int* ss = sorted_slots.data_ptr<int>();
  const int* be = block_expert.data_ptr<int>();
#define LAUNCH_MOE8(MT, GATED, A, AS, W, WS, OUT, N, K)                     \
  hipLaunchKernelGGL((moe_gemm_fp8_kernel<MT, GATED>),                      \
                     dim3((unsigned)((N) / NT), (unsigned)nb_max),          \
                     dim3(NW * 64), 0, stream_,                             \
                     (const unsigned char*)(A).data_ptr(),                  \
                     (const float*)(AS).data_ptr(),                         \
                     (const unsigned char*)(W).data_ptr(),                  \
                     (const float*)(WS).data_ptr(), ss, be,                 \
                     (OUT).data_ptr(), (int)s, (int)k, (int)(N), (int)(K))
  if (block_m == 16) {
    LAUNCH_MOE8(1, true, x8, x_scale, w13_8, w13_scale, act, inter, h);
  } else {
    LAUNCH_MOE8(4, true, x8, x_scale, w13_8, w13_scale, act, inter, h);
  }
  // every act row is a slot, and align places every slot exactly once
  auto q = quant_fp8(act);  // {e4m3 [S, I], fp32 scale [S]}
  if (block_m == 16) {
    LAUNCH_MOE8(1, false, q[0], q[1], w2_8, w2_scale, y, h, inter);
  } else {
    LAUNCH_MOE8(4, false, q[0], q[1], w2_8, w2_scale, y, h, inter);
  }
#undef LAUNCH_MOE8
  cmls_moe::launch_combine(y, weights, out, "moe_experts_fp8");
  return out;
}
