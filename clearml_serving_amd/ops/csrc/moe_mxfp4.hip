// Mixture-of-experts FFN with MXFP4 expert weights (OCP MX: e2m1 elements +
// one e8m0 scale per 32 k) for gfx950.
//
// An MoE decode step is expert-weight streaming and little else; at 4.25
// bits per weight the experts are 0.53x the bytes of e4m3. The block keeps
// the sync-free, capturable shape of moe.hip / moe_fp8.hip and reuses their
// align and combine stages (moe.h):
//
//   moe_align    group the S = T*k slots by expert               (moe.hip)
//   gate/up      grouped mxfp4 GEMM over w13[e], SwiGLU epilogue -> bf16 act
//   quant_fp8    act rows -> e4m3 bytes + per-row scale        (fp8_path.hip)
//   down         grouped mxfp4 GEMM over w2[e]                   -> fp32 y
//   combine      out[t] = sum_j weights[t, j] * y[t*k + j]       (moe.hip)
//
// moe_gemm_mxfp4_kernel: one workgroup per (row block, 16 weight columns) on
// mfma_scale_f32_16x16x128_f8f6f4 (A = e4m3, B = e2m1, the e8m0 block scale
// applied by the instruction; operand maps in mxfp4_path.hip).
//   weights      only the ops.tile_mxfp4_weight layout, per expert
//                  w4t [E][NB][K/128][64][16 B]
//                  e8t [E][NB][ceil(K/512)][64][4 B]
//                NB = N/16 (down) or 2N/16 (gate/up: tile rows nb and
//                N/16 + nb are the gate and up columns of one index, so a
//                workgroup holds both and SwiGLU happens in its epilogue).
//                One wave-wide 16-byte load is a contiguous 1 KiB line and is
//                the B operand; one dword per lane scales four k-steps.
//   activations  gathered through sorted_slots from a row-major e4m3 matrix,
//                two 16-byte loads per lane per k-step (+16g, +64+16g); they
//                are re-read by every column workgroup and ride in L2
//   K split      the 8 waves take whole scale quads (512 k) round-robin:
//                wave w owns quads w, w + 8, ...; the next quad's weight
//                lines and scale dwords are in flight while the current quad
//                is multiplied. The ragged last quad (K % 512 != 0, 1..3
//                steps) goes to the wave whose turn it is; a wave with no
//                quad parks zeros.
//   reduction    every wave parks its partial tile in LDS; then all 512
//                threads each own output elements and sum the 8 partials in
//                wave order 0..7. One output element is one dot product
//                whose k split depends on K only, so results are
//                bit-reproducible, batch-invariant and the same for either
//                row block; no float atomics anywhere.
//   scaling      sum * a_scale[row] * w_scale[e, n] in fp32 (A's MX scale is
//                held at 2^0; w_scale is the fp32 row scale of
//                quantize_mxfp4, all ones for weights quantised here)
#include "moe.h"

// fp8_path.hip: per-row absmax quantisation to e4m3, {bytes [R, C], scale [R]}
std::vector<torch::Tensor> quant_fp8(torch::Tensor x);

// moe_mxfp4_gemm.hip: the same five stages with 128-row blocks and the tiled
// GEMM kernel; operands already checked by moe_experts_mxfp4 below
torch::Tensor moe_experts_mxfp4_tiled(torch::Tensor x8, torch::Tensor x_scale,
                                      torch::Tensor w13_t,
                                      torch::Tensor w13_e8t,
                                      torch::Tensor w13_scale,
                                      torch::Tensor w2_t, torch::Tensor w2_e8t,
                                      torch::Tensor w2_scale,
                                      torch::Tensor ids,
                                      torch::Tensor weights);

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int NT = 16;      // weight columns per workgroup
constexpr int NW = 8;       // waves (split K)
constexpr int KSTEP = 128;  // k per MFMA
constexpr int QUAD = 4;     // k-steps per packed scale dword
constexpr int SCALE_ONE = 0x7f7f7f7f;  // e8m0 2^0 in every byte

// B operand (and its scale dword) of one weight tile row for one quad
template <int HALVES>
struct QuadW {
  uint32x4 w[HALVES][QUAD];
  int sc[HALVES];
};

// one k-step: the A fragments come straight from global memory (2 x 16 B per
// lane per 16-row tile) and feed the gate and, if HALVES == 2, the up MFMA.
// SEL (the scale byte of this step) must be a compile-time constant.
template <int SEL, int MT, int HALVES>
__device__ __forceinline__ void mx_step(const QuadW<HALVES>& q,
                                        const unsigned char* const* arow,
                                        const long koff,
                                        f32x4_t (*acc)[MT]) {
  i32x8_t b[HALVES];
#pragma unroll
  for (int hf = 0; hf < HALVES; ++hf) {
    const uint32x4 wv = q.w[hf][SEL];
    b[hf] = i32x8_t{(int)wv.x, (int)wv.y, (int)wv.z, (int)wv.w, 0, 0, 0, 0};
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const uint32x4 lo = *reinterpret_cast<const uint32x4*>(arow[t] + koff);
    const uint32x4 hi =
        *reinterpret_cast<const uint32x4*>(arow[t] + koff + 64);
    const i32x8_t a = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                       (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
    for (int hf = 0; hf < HALVES; ++hf) {
      acc[hf][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          a, b[hf], acc[hf][t], /*cbsz=e4m3*/ 0, /*blgp=e2m1*/ 4, 0,
          SCALE_ONE, SEL, q.sc[hf]);
    }
  }
}

// grid (N/16, nb_max), block 8 waves, MT 16-row tiles per row block.
//   GATED:  A row = a[slot / k], W = w13[e] (2N/16 tile rows, gate then up),
//           out = bf16 act[slot, n] = silu(g) * u
//   !GATED: A row = a[slot],     W = w2[e] (N/16 tile rows),
//           out = fp32 y[slot, n]
// a_scale is indexed like a's rows, w_scale like w's rows. Sentinel rows
// (slot == n_slots) replay row 0 and never store; a block whose expert is -1
// exits at once (workgroup-uniform, before any barrier).
//
// The target attribute keeps the compiler from pairing the gate and up sums
// of the epilogue into packed fp32 VALU ops: plain v_add / v_mul only. It is
// set here rather than as a build flag so that no other file's code
// generation changes (the choice moe_fp8.hip makes).
template <int MT, bool GATED>
__global__ __launch_bounds__(NW * 64)
__attribute__((target("no-packed-fp32-ops"))) void moe_gemm_mxfp4_kernel(
    const unsigned char* __restrict__ a,  // [T, K] or [S, K] e4m3
    const float* __restrict__ a_scale,    // [T] or [S]
    const uint32x4* __restrict__ w4t,     // [E][NB][K/128][64] 16-B lines
    const int* __restrict__ e8t,          // [E][NB][ceil(K/512)][64] dwords
    const float* __restrict__ w_scale,    // [E, (2)N]
    const int* __restrict__ sorted_slots,
    const int* __restrict__ block_expert,
    void* __restrict__ out,               // bf16 [S, N] or fp32 [S, N]
    int n_slots, int top_k, int N, int K) {
  constexpr int HALVES = GATED ? 2 : 1;
  const int e = block_expert[blockIdx.y];
  if (e < 0) return;
  const int nb = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = lane & 15;  // fragment row (m or n within the tile)
  const int g = lane >> 4;    // lane group
  const int* slots = sorted_slots + (long)blockIdx.y * (MT * 16);

  const int nsteps = K / KSTEP;
  const int nfull = nsteps / QUAD;  // whole scale dwords
  const int nquads = (nsteps + QUAD - 1) / QUAD;
  const long tile_rows = (long)HALVES * (N / NT);  // NB of expert e
  const uint32x4* wt[HALVES];
  const int* st[HALVES];
#pragma unroll
  for (int hf = 0; hf < HALVES; ++hf) {
    const long tr = (long)e * tile_rows + (long)hf * (N / NT) + nb;
    wt[hf] = w4t + tr * nsteps * 64 + lane;
    st[hf] = e8t + tr * nquads * 64 + lane;
  }

  const unsigned char* arow[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    int s = slots[t * 16 + row];
    if (s >= n_slots) s = 0;  // sentinel: replay a valid row
    const long r = GATED ? s / top_k : s;
    arow[t] = a + r * K + 16 * g;
  }

  f32x4_t acc[HALVES][MT];
#pragma unroll
  for (int hf = 0; hf < HALVES; ++hf) {
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[hf][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // full quads, round-robin over the waves, one quad of lookahead
  QuadW<HALVES> cur;
  int q = wave;
  if (q < nfull) {
#pragma unroll
    for (int hf = 0; hf < HALVES; ++hf) {
#pragma unroll
      for (int j = 0; j < QUAD; ++j)
        cur.w[hf][j] = wt[hf][(long)(q * QUAD + j) * 64];
      cur.sc[hf] = st[hf][(long)q * 64];
    }
  }
  while (q < nfull) {
    const int qn = q + NW;
    QuadW<HALVES> nxt;
#pragma unroll
    for (int hf = 0; hf < HALVES; ++hf) {
#pragma unroll
      for (int j = 0; j < QUAD; ++j) nxt.w[hf][j] = uint32x4{0u, 0u, 0u, 0u};
      nxt.sc[hf] = SCALE_ONE;
    }
    if (qn < nfull) {
#pragma unroll
      for (int hf = 0; hf < HALVES; ++hf) {
#pragma unroll
        for (int j = 0; j < QUAD; ++j)
          nxt.w[hf][j] = wt[hf][(long)(qn * QUAD + j) * 64];
        nxt.sc[hf] = st[hf][(long)qn * 64];
      }
    }
    const long k0 = (long)q * QUAD * KSTEP;
    mx_step<0, MT, HALVES>(cur, arow, k0, acc);
    mx_step<1, MT, HALVES>(cur, arow, k0 + KSTEP, acc);
    mx_step<2, MT, HALVES>(cur, arow, k0 + 2 * KSTEP, acc);
    mx_step<3, MT, HALVES>(cur, arow, k0 + 3 * KSTEP, acc);
    cur = nxt;
    q = qn;
  }
  // ragged last quad (K % 512 != 0): 1..3 steps, on the wave whose turn it
  // is; only the lines that exist are read
  const int rem = nsteps - nfull * QUAD;
  if (rem > 0 && (nfull % NW) == wave) {
    const int s0 = nfull * QUAD;
    QuadW<HALVES> last;
#pragma unroll
    for (int hf = 0; hf < HALVES; ++hf) {
#pragma unroll
      for (int j = 0; j < QUAD - 1; ++j) {
        last.w[hf][j] = uint32x4{0u, 0u, 0u, 0u};
        if (j < rem) last.w[hf][j] = wt[hf][(long)(s0 + j) * 64];
      }
      last.w[hf][QUAD - 1] = uint32x4{0u, 0u, 0u, 0u};
      last.sc[hf] = st[hf][(long)nfull * 64];
    }
    const long k0 = (long)s0 * KSTEP;
    mx_step<0, MT, HALVES>(last, arow, k0, acc);
    if (rem > 1) mx_step<1, MT, HALVES>(last, arow, k0 + KSTEP, acc);
    if (rem > 2) mx_step<2, MT, HALVES>(last, arow, k0 + 2 * KSTEP, acc);
  }

  // lds[half][wave][m][n]: GATED with MT = 4 is 2*8*64*16*4 B = 64 KB, the
  // static LDS limit (as the bf16 and fp8 kernels). Waves without a quad
  // park zeros, so the sum below always runs over all NW partials.
  __shared__ float lds[HALVES][NW][MT * 16][NT];
  const int crow = g * 4;  // C fragment rows
#pragma unroll
  for (int hf = 0; hf < HALVES; ++hf) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds[hf][wave][t * 16 + crow + r][row] = acc[hf][t][r];
    }
  }
  __syncthreads();

  // every thread owns output elements o = m * 16 + n: consecutive lanes read
  // consecutive LDS words (no bank conflict) and store consecutive columns
  const int n0 = nb * NT;
  const float* wsc = w_scale + (long)e * HALVES * N + n0;
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

void check_aligned16(const torch::Tensor& v, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0,
              "moe_experts_mxfp4: ", name, " must be 16-byte aligned");
}

void check_scale(const torch::Tensor& v, const torch::Tensor& like,
                 long numel, const char* name) {
  TORCH_CHECK(v.device() == like.device() &&
                  v.scalar_type() == at::kFloat && v.is_contiguous() &&
                  v.numel() == numel,
              "moe_experts_mxfp4: ", name, " must be contiguous fp32 with ",
              numel, " elements on the operands' GPU");
}

// w4t / e8t must be the per-expert tile_mxfp4_weight tiling of [E, n, k]
void check_tiles(const torch::Tensor& w4t, const torch::Tensor& e8t,
                 const torch::Tensor& like, long e, long n, long k,
                 const char* name) {
  TORCH_CHECK(w4t.device() == like.device() && e8t.device() == like.device(),
              "moe_experts_mxfp4: all operands must be on one GPU");
  TORCH_CHECK(w4t.scalar_type() == at::kByte &&
                  e8t.scalar_type() == at::kByte && w4t.is_contiguous() &&
                  e8t.is_contiguous(),
              "moe_experts_mxfp4: ", name,
              " tiles and scales must be contiguous uint8");
  const long steps = k / KSTEP, quads = (steps + QUAD - 1) / QUAD;
  TORCH_CHECK(w4t.numel() == e * (n / NT) * steps * 64 * 16 &&
                  e8t.numel() == e * (n / NT) * quads * 64 * 4,
              "moe_experts_mxfp4: ", name, " is not the tiling of [", e, ", ",
              n, ", ", k, "]");
  check_aligned16(w4t, name);
  check_aligned16(e8t, name);
}

}  // namespace

// E and I come from the row scales (w13_scale [E, 2I], w2_scale [E, H]): the
// tiled buffers carry padded sizes only.
torch::Tensor moe_experts_mxfp4(torch::Tensor x8, torch::Tensor x_scale,
                                torch::Tensor w13_t, torch::Tensor w13_e8t,
                                torch::Tensor w13_scale, torch::Tensor w2_t,
                                torch::Tensor w2_e8t, torch::Tensor w2_scale,
                                torch::Tensor ids, torch::Tensor weights,
                                int64_t block_m) {
  TORCH_CHECK(x8.is_cuda() && ids.device() == x8.device() &&
                  weights.device() == x8.device(),
              "moe_experts_mxfp4: all operands must be on one GPU");
  TORCH_CHECK(x8.scalar_type() == at::kByte ||
                  x8.scalar_type() == at::kFloat8_e4m3fn,
              "moe_experts_mxfp4: x8 must be uint8 / e4m3");
  TORCH_CHECK(x8.dim() == 2 && x8.is_contiguous(),
              "moe_experts_mxfp4: x8 must be contiguous [T, H]");
  TORCH_CHECK(w13_scale.dim() == 2 && w2_scale.dim() == 2 &&
                  w13_scale.size(1) % 2 == 0,
              "moe_experts_mxfp4: w13_scale must be [E, 2I] and w2_scale "
              "[E, H]");
  const long t = x8.size(0), h = x8.size(1);
  const long e = w13_scale.size(0), inter = w13_scale.size(1) / 2;
  cmls_moe::check_ids(ids, "moe_experts_mxfp4");
  const long k = ids.size(1), s = t * k;
  TORCH_CHECK(ids.size(0) == t, "moe_experts_mxfp4: ids and x8 disagree on T");
  TORCH_CHECK(e >= 1 && e <= cmls_moe::MAX_E && k <= e,
              "moe_experts_mxfp4: need k <= E <= ", cmls_moe::MAX_E,
              ", got k=", k, " E=", e);
  TORCH_CHECK(weights.scalar_type() == at::kFloat && weights.dim() == 2 &&
                  weights.size(0) == t && weights.size(1) == k &&
                  weights.is_contiguous(),
              "moe_experts_mxfp4: weights must be contiguous fp32 [T, k]");
  TORCH_CHECK(h % KSTEP == 0 && h >= KSTEP && h <= INT_MAX,
              "moe_experts_mxfp4: H must be a multiple of 128, got ", h);
  TORCH_CHECK(inter % KSTEP == 0 && inter >= KSTEP && inter <= INT_MAX,
              "moe_experts_mxfp4: I must be a multiple of 128, got ", inter);
  TORCH_CHECK(block_m == 16 || block_m == 64 || block_m == 128,
              "moe_experts_mxfp4: block_m must be 16, 64 or 128, got ",
              block_m);
  check_scale(x_scale, x8, t, "x_scale");
  check_scale(w13_scale, x8, e * 2 * inter, "w13_scale");
  check_scale(w2_scale, x8, e * h, "w2_scale");
  check_aligned16(x8, "x8");
  check_tiles(w13_t, w13_e8t, x8, e, 2 * inter, h, "w13");
  check_tiles(w2_t, w2_e8t, x8, e, h, inter, "w2");
  if (block_m == 128)  // prefill-shaped: 128 x 128 tiles through LDS
    return moe_experts_mxfp4_tiled(x8, x_scale, w13_t, w13_e8t, w13_scale,
                                   w2_t, w2_e8t, w2_scale, ids, weights);

  torch::Tensor sorted_slots, block_expert;
  cmls_moe::launch_align(ids, e, block_m, sorted_slots, block_expert);
  const long nb_max = block_expert.size(0);
  TORCH_CHECK(nb_max <= 65535, "moe_experts_mxfp4: too many row blocks (",
              nb_max, "); raise block_m or split the batch");

  auto act = torch::empty({s, inter}, x8.options().dtype(at::kBFloat16));
  auto y = torch::empty({s, h}, x8.options().dtype(at::kFloat));
  auto out = torch::empty({t, h}, x8.options().dtype(at::kBFloat16));
  hipStream_t stream_ = cmls::current_stream();
  const int* ss = sorted_slots.data_ptr<int>();
  const int* be = block_expert.data_ptr<int>();
#define LAUNCH_MOE4(MT, GATED, A, AS, W, WE, WS, OUT, N, K)                 \
  hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<MT, GATED>),                    \
                     dim3((unsigned)((N) / NT), (unsigned)nb_max),          \
                     dim3(NW * 64), 0, stream_,                             \
                     (const unsigned char*)(A).data_ptr(),                  \
                     (const float*)(AS).data_ptr(),                         \
                     (const uint32x4*)(W).data_ptr(),                       \
                     (const int*)(WE).data_ptr(),                           \
                     (const float*)(WS).data_ptr(), ss, be,                 \
                     (OUT).data_ptr(), (int)s, (int)k, (int)(N), (int)(K))
  if (block_m == 16) {
    LAUNCH_MOE4(1, true, x8, x_scale, w13_t, w13_e8t, w13_scale, act, inter,
                h);
  } else {
    LAUNCH_MOE4(4, true, x8, x_scale, w13_t, w13_e8t, w13_scale, act, inter,
                h);
  }
  // every act row is a slot, and align places every slot exactly once
  auto q = quant_fp8(act);  // {e4m3 [S, I], fp32 scale [S]}
  if (block_m == 16) {
    LAUNCH_MOE4(1, false, q[0], q[1], w2_t, w2_e8t, w2_scale, y, h, inter);
  } else {
    LAUNCH_MOE4(4, false, q[0], q[1], w2_t, w2_e8t, w2_scale, y, h, inter);
  }
#undef LAUNCH_MOE4
  cmls_moe::launch_combine(y, weights, out, "moe_experts_mxfp4");
  return out;
}
