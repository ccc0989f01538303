// MXFP4 (OCP MX: e2m1 elements + one e8m0 scale per 32 k) weight path:
// decode GEMM on the gfx950 block-scaled matrix instruction, plus the small
// dequantiser the prefill route uses.
//
// Decode streams weights (fp8_path.hip); e2m1 halves the bytes again, and
// v_mfma_scale_f32_16x16x128_f8f6f4 takes e2m1 x e4m3 directly, applying the
// e8m0 block scale in hardware -- no dequantisation in registers. The
// activations are the e4m3 rows + fp32 row scales the fused producers of
// fp8_path.hip already emit.
//
//   skinny_gemm_mxfp4 : C[M,N] = (A8 * s_a[m]) @ (deq(W4,E8) * s_w[n])^T
//                       -> bf16, M <= 64, K % 128 == 0, N % 16 == 0
//   dequant_mxfp4_bf16: tiled W4/E8 (* s_w) -> bf16 [N, K], any N, K % 32 == 0
//
// Operand maps of mfma_scale_f32_16x16x128_f8f6f4 (D[16x16] += A[16x128] *
// B[128x16]; lane l: r = l % 16, g = l / 16), pinned by
// tests/test_mxfp4_gpu.py:
//   A e4m3, cbsz=0: lane l holds row r in 8 VGPRs as two 16-byte halves, one
//                   per 64-wide half of K: VGPR v byte b is
//                   k = 64(v / 4) + 16g + 4(v % 4) + b (NOT 32 consecutive k)
//   B e2m1, blgp=4: lane l holds column r, k = 32g + e, e = 0..31: 16 bytes
//                   in VGPRs 0..3 (4..7 ignored), VGPR v nibble i (bits
//                   4i..4i+3) is k = 32g + 8v + i -- the low nibble of a byte
//                   is the even k
//   scales:         one VGPR per operand, op_sel (0..3) picks the byte; lane
//                   l's B byte scales exactly the 32 k-values lane l
//                   supplies, so one MX block == one lane's B operand. A's
//                   is held at 2^0 (127 in every byte), so how its blocks
//                   fall on lanes does not matter; B's is the stored e8m0.
//   D f32x4:        lane l register i is row 4g + i, column r (as the
//                   non-scaled 16x16 MFMAs)
//
// HBM layout (ops.tile_mxfp4_weight; only this copy is kept):
//   w4t [ceil(N/16)][ceil(K/128)][64 lanes][16 B]: lane l = (r, g) of tile
//       (nb, ks) holds row 16nb + r, k = 128ks + 32g .. +31 -- one wave-wide
//       16-byte load is a contiguous 1 KiB line and IS the B operand
//   e8t [ceil(N/16)][ceil(K/512)][64 lanes][4 B]: lane l, byte j is the
//       scale of row 16nb + r, k-step 4q + j, block g -- one dword per lane
//       per four k-steps, op_sel = j. Padding scales are 127, padding
//       elements 0.
#include "common.h"
#include "mxfp4_tiles.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) float mx_f32x4_t;

// one k-step: B operand from the 16-byte weight line, A fragments straight
// from global memory (2 x 16 B per lane per 16-row tile; rows >= M are
// exec-masked off and contribute zeros). SEL must be a compile-time constant.
template <int SEL, int MT>
__device__ __forceinline__ void mx_step(const uint32x4 wv, const int sc,
                                        const unsigned char* const* arow,
                                        const bool* avalid, const long koff,
                                        mx_f32x4_t* acc) {
  const i32x8_t b = {(int)wv.x, (int)wv.y, (int)wv.z, (int)wv.w, 0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    uint32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
    if (avalid[t]) {
      lo = *reinterpret_cast<const uint32x4*>(arow[t] + koff);
      hi = *reinterpret_cast<const uint32x4*>(arow[t] + koff + 64);
    }
    const i32x8_t a = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                       (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    acc[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
        a, b, acc[t], /*cbsz=e4m3*/ 0, /*blgp=e2m1*/ 4, 0, MX_SCALE_ONE, SEL,
        sc);
  }
}

// One workgroup per 16 output columns, NW waves split K by scale quads
// (wave w owns quads w, w + NW, ...; the next quad's weight lines are in
// flight while the current one is multiplied). Partials meet in LDS and are
// summed in wave order: no atomics, bit-reproducible.
// plain v_add / v_mul in the epilogue, set here so that no other file's
// code generation changes (the choice moe_fp8.hip makes)
template <int MT, int NW>  // 16-row m tiles (M <= 16*MT), waves
__global__ __launch_bounds__(NW * 64)
__attribute__((target("no-packed-fp32-ops"))) void skinny_gemm_mxfp4_kernel(
    const unsigned char* __restrict__ a,  // [M, K] e4m3 row-major
    const float* __restrict__ a_scale,    // [M]
    const uint32x4* __restrict__ w4t,     // [N/16][K/128][64] 16-B lines
    const int* __restrict__ e8t,          // [N/16][ceil(K/512)][64] dwords
    const float* __restrict__ w_scale,    // [N]
    __hip_bfloat16* __restrict__ c,       // [M, N]
    int M, int N, int K) {
  const int nb = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = lane & 15;
  const int g = lane >> 4;

  const int nsteps = K / MX_KSTEP;
  const int nfull = nsteps / MX_QUAD;               // whole scale dwords
  const int nquads = (nsteps + MX_QUAD - 1) / MX_QUAD;
  const uint32x4* wt = w4t + (long)nb * nsteps * 64 + lane;
  const int* st = e8t + (long)nb * nquads * 64 + lane;

  const unsigned char* arow[MT];
  bool avalid[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + row;
    avalid[t] = m < M;
    arow[t] = a + (long)(avalid[t] ? m : 0) * K + 16 * g;
  }

  mx_f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = mx_f32x4_t{0.f, 0.f, 0.f, 0.f};

  uint32x4 wv[MX_QUAD];
  int sc = MX_SCALE_ONE;
  int q = wave;
  if (q < nfull) {
#pragma unroll
    for (int j = 0; j < MX_QUAD; ++j) wv[j] = wt[(long)(q * MX_QUAD + j) * 64];
    sc = st[(long)q * 64];
  }
  while (q < nfull) {
    const int qn = q + NW;
    uint32x4 wn[MX_QUAD];
    int sn = MX_SCALE_ONE;
#pragma unroll
    for (int j = 0; j < MX_QUAD; ++j) wn[j] = uint32x4{0u, 0u, 0u, 0u};
    if (qn < nfull) {
#pragma unroll
      for (int j = 0; j < MX_QUAD; ++j)
        wn[j] = wt[(long)(qn * MX_QUAD + j) * 64];
      sn = st[(long)qn * 64];
    }
    const long k0 = (long)q * MX_QUAD * MX_KSTEP;
    mx_step<0, MT>(wv[0], sc, arow, avalid, k0, acc);
    mx_step<1, MT>(wv[1], sc, arow, avalid, k0 + MX_KSTEP, acc);
    mx_step<2, MT>(wv[2], sc, arow, avalid, k0 + 2 * MX_KSTEP, acc);
    mx_step<3, MT>(wv[3], sc, arow, avalid, k0 + 3 * MX_KSTEP, acc);
#pragma unroll
    for (int j = 0; j < MX_QUAD; ++j) wv[j] = wn[j];
    sc = sn;
    q = qn;
  }
  // ragged last dword (K % 512 != 0): 1..3 steps, on the wave whose turn it is
  const int rem = nsteps - nfull * MX_QUAD;
  if (rem > 0 && (nfull % NW) == wave) {
    const int s0 = nfull * MX_QUAD;
    const int sct = st[(long)nfull * 64];
    const long k0 = (long)s0 * MX_KSTEP;
    mx_step<0, MT>(wt[(long)s0 * 64], sct, arow, avalid, k0, acc);
    if (rem > 1)
      mx_step<1, MT>(wt[(long)(s0 + 1) * 64], sct, arow, avalid,
                     k0 + MX_KSTEP, acc);
    if (rem > 2)
      mx_step<2, MT>(wt[(long)(s0 + 2) * 64], sct, arow, avalid,
                     k0 + 2 * MX_KSTEP, acc);
  }

  __shared__ float lds[NW][MT * 16][MX_NT];
  const int crow = g * 4;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) lds[wave][t * 16 + crow + r][row] = acc[t][r];
  }
  __syncthreads();
  // every wave reduces its share of the m tiles, in wave order
  const int n = nb * MX_NT + row;
  const float ws = w_scale[n];
  for (int t = wave; t < MT; t += NW) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t * 16 + crow + r;
      float s = 0.f;
#pragma unroll
      for (int wvi = 0; wvi < NW; ++wvi) s += lds[wvi][m][row];
      if (m < M) c[(long)m * N + n] = __float2bfloat16(s * a_scale[m] * ws);
    }
  }
}

// e2m1 code (3 bits, sign handled by the caller) -> fp32
__device__ __forceinline__ float e2m1_to_f32(unsigned code) {
  const unsigned e = (code >> 1) & 3u, m = code & 1u;
  const unsigned bits = e ? ((e + 126u) << 23) | (m << 22)  // (1 + m/2) 2^(e-1)
                          : (m ? 0x3f000000u : 0u);         // 0 or 0.5
  return __uint_as_float(bits);
}

// dequant_mxfp4_bf16: one thread per 16-byte weight line entry (32 values of
// one row); a 256-thread block covers the four k-steps of one scale dword.
// grid (ceil(K/512), ceil(N/16)). Rows >= N and k >= K are padding: skipped.
__global__ __launch_bounds__(256)
__attribute__((target("no-packed-fp32-ops"))) void dequant_mxfp4_bf16_kernel(
    const uint32x4* __restrict__ w4t, const unsigned int* __restrict__ e8t,
    const float* __restrict__ w_scale, __hip_bfloat16* __restrict__ out,
    int N, int K) {
  const int nsteps = (K + MX_KSTEP - 1) / MX_KSTEP;
  const int nquads = gridDim.x;
  const int q = blockIdx.x, nb = blockIdx.y;
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int step = q * MX_QUAD + j;
  const int n = nb * MX_NT + (lane & 15);
  const int k0 = step * MX_KSTEP + (lane >> 4) * 32;
  if (step >= nsteps || n >= N || k0 >= K) return;
  const uint32x4 wv = w4t[((long)nb * nsteps + step) * 64 + lane];
  const unsigned sdw = e8t[((long)nb * nquads + q) * 64 + lane];
  const int e8 = (int)((sdw >> (8 * j)) & 0xffu);
  const float rs = w_scale[n];
  const unsigned words[4] = {wv.x, wv.y, wv.z, wv.w};
  __hip_bfloat16* orow = out + (long)n * K + k0;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned nib = (words[v] >> (4 * i)) & 0xfu;
      float f = ldexpf(e2m1_to_f32(nib & 7u), e8 - 127);
      if (nib & 8u) f = -f;
      o.h[i] = __float2bfloat16(f * rs);
    }
    *reinterpret_cast<uint32x4*>(orow + 8 * v) = o.u;
  }
}

}  // namespace

#ifndef CMLS_KERNEL_ONLY
namespace {

template <int NW>
void launch_skinny_mxfp4(const torch::Tensor& a8, const torch::Tensor& a_scale,
                         const torch::Tensor& w4t, const torch::Tensor& e8t,
                         const torch::Tensor& w_scale, torch::Tensor& c, int M,
                         int N, int K) {
  hipStream_t stream_ = cmls::current_stream();
  dim3 grid(N / MX_NT);
#define LAUNCH_MX(T)                                                         \
  hipLaunchKernelGGL((skinny_gemm_mxfp4_kernel<T, NW>), grid, dim3(NW * 64), \
                     0, stream_, (const unsigned char*)a8.data_ptr(),        \
                     (const float*)a_scale.data_ptr(),                       \
                     (const uint32x4*)w4t.data_ptr(),                        \
                     (const int*)e8t.data_ptr(),                             \
                     (const float*)w_scale.data_ptr(),                       \
                     (__hip_bfloat16*)c.data_ptr(), M, N, K)
  switch ((M + 15) / 16) {
    case 1: LAUNCH_MX(1); break;
    case 2: LAUNCH_MX(2); break;
    case 3: LAUNCH_MX(3); break;
    default: LAUNCH_MX(4); break;
  }
#undef LAUNCH_MX
}

}  // namespace

// waves: 4 or 8 k-split waves per workgroup (the Python layer picks the
// measured default; the benchmark times both)
torch::Tensor skinny_gemm_mxfp4(torch::Tensor a8, torch::Tensor a_scale,
                                torch::Tensor w4t, torch::Tensor e8t,
                                torch::Tensor w_scale, int64_t waves) {
  TORCH_CHECK(a8.dim() == 2, "skinny_gemm_mxfp4: a8 is [M, K]");
  TORCH_CHECK(a8.scalar_type() == at::kByte ||
              a8.scalar_type() == at::kFloat8_e4m3fn);
  TORCH_CHECK(a8.is_contiguous() && a_scale.is_contiguous());
  TORCH_CHECK(a_scale.scalar_type() == at::kFloat);
  const int M = a8.size(0), K = a8.size(1), N = w_scale.numel();
  TORCH_CHECK(M >= 1 && M <= 64, "skinny_gemm_mxfp4: M must be 1..64");
  TORCH_CHECK(K >= MX_KSTEP && K % MX_KSTEP == 0,
              "skinny_gemm_mxfp4: K % 128 != 0");
  TORCH_CHECK(N >= MX_NT && N % MX_NT == 0, "skinny_gemm_mxfp4: N % 16 != 0");
  TORCH_CHECK(a_scale.numel() == M);
  TORCH_CHECK((uintptr_t)a8.data_ptr() % 16 == 0,
              "skinny_gemm_mxfp4: misaligned activations");
  check_mx_tiles(w4t, e8t, w_scale, N, K, "skinny_gemm_mxfp4");
  auto c = torch::empty({M, N}, a8.options().dtype(torch::kBFloat16));
  if (waves == 4)
    launch_skinny_mxfp4<4>(a8, a_scale, w4t, e8t, w_scale, c, M, N, K);
  else if (waves == 8)
    launch_skinny_mxfp4<8>(a8, a_scale, w4t, e8t, w_scale, c, M, N, K);
  else
    TORCH_CHECK(false, "skinny_gemm_mxfp4: waves must be 4 or 8");
  return c;
}

torch::Tensor dequant_mxfp4_bf16(torch::Tensor w4t, torch::Tensor e8t,
                                 torch::Tensor w_scale, int64_t n, int64_t k) {
  TORCH_CHECK(n >= 1 && k >= 32 && k % 32 == 0,
              "dequant_mxfp4_bf16: K % 32 != 0");
  check_mx_tiles(w4t, e8t, w_scale, (int)n, (int)k, "dequant_mxfp4_bf16");
  auto out = torch::empty({n, k}, w4t.options().dtype(torch::kBFloat16));
  const int nsteps = (k + MX_KSTEP - 1) / MX_KSTEP;
  dim3 grid((nsteps + MX_QUAD - 1) / MX_QUAD, (n + MX_NT - 1) / MX_NT);
  hipLaunchKernelGGL(dequant_mxfp4_bf16_kernel, grid, dim3(256), 0,
                     cmls::current_stream(), (const uint32x4*)w4t.data_ptr(),
                     (const unsigned int*)e8t.data_ptr(),
                     (const float*)w_scale.data_ptr(),
                     (__hip_bfloat16*)out.data_ptr(), (int)n, (int)k);
  return out;
}
#endif  // CMLS_KERNEL_ONLY
