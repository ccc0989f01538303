// MXFP4 prefill GEMM: the compute-shaped companion of skinny_gemm_mxfp4
// (mxfp4_path.hip) on the same block-scaled matrix instruction and the same
// weight buffers.
//
//   gemm_mxfp4: C[M,N] = (A8 * s_a[m]) @ (deq(W4,E8) * s_w[n])^T -> bf16
//               any M >= 1, K % 128 == 0, N % 128 == 0; A contiguous e4m3
//               [M, K]; W4 / E8 in the ops.tile_mxfp4_weight layout
//
// Operand maps of v_mfma_scale_f32_16x16x128_f8f6f4 and the HBM layout are
// written out in mxfp4_path.hip; lane l = (r, g), r = l % 16, g = l / 16.
//
// Work split. One workgroup of 256 threads (4 waves) per BM x 128 output
// tile; grid (ceil(M/BM), N/128) with the M tiles on the fast axis, so that
// workgroups launched together read the same weight lines and share them in
// L2. Two instantiations:
//   BM = 128: waves 2 x 2, each 64 x 64 = 4 m-tiles x 4 n-blocks, 16 f32x4
//             accumulators
//   BM = 64 : waves 1 x 4, each 64 x 32 = 4 m-tiles x 2 n-blocks, 8
//             accumulators; no wave loads a weight line another one loads
// The host takes BM = 64 while the 128-row grid has fewer workgroups than
// the chip has CUs (rule and measurement: profiles/mxfp4_gemm.txt).
//
// K. No split-K, no atomics: every output element is accumulated by one wave
// over the k-steps in ascending order, in both instantiations, so a row's
// result does not depend on M, on the rows it is batched with or on the
// tile chosen, and the launch is capture-safe.
//
// A through LDS. Per k-step the A tile is BM rows x 128 bytes. Thread t
// loads 16 bytes of row t / 8 (+ 32 per pass), chunk t % 8: eight lanes read
// one whole 128-byte line, as a raw buffer load over the tile's valid rows:
// rows >= M are never read, the load returns zeros for them. Two LDS buffers (2 x 16 KiB at BM = 128); the global loads of step
// s + 1 are issued before the MFMAs of step s and written to the other
// buffer after them, one barrier per step.
//   Fragment read of a 16-row tile, cbsz = 0 map: lane (r, g) reads the
//   16-byte chunks g and 4 + g of row r (two ds_read_b128).
//   Banks: 64 banks x 4 bytes, so a 128-byte row covers half of them and an
//   unswizzled tile puts chunk c of rows r, r + 2, r + 4, ... on the same
//   four banks: the 16 lanes of one g that a b128 read serves together would
//   hit 8 rows per bank group, an 8-way conflict. Chunk c of row r is stored
//   at chunk c ^ ((r >> 1) & 7). For a fixed logical chunk the pair
//   (r & 1, (r >> 1) & 7) takes all 16 values over r = 0..15, and the bank
//   group of the access is 32 (r & 1) + 4 (c ^ ((r >> 1) & 7)): a bijection
//   onto the 16 four-bank groups. Conflict degree 1 for the reads. A write
//   pass has 16 consecutive lanes cover rows 2i and 2i + 1 with all eight
//   chunks each; the swizzle permutes chunks within a row, so the 16 lanes
//   again cover all 64 banks once: degree 1 for the writes.
//
// B from global memory. A wave's operand for one n-block and k-step is one
// contiguous 1 KiB line (16 B per lane), loaded one k-step ahead into
// registers. One step ahead, not the whole scale quad the skinny kernel
// keeps in flight: a quad of 4 n-blocks is 64 VGPRs per buffer, and with the
// 64 accumulators, 32 A-fragment and 16 A-staging registers that would take
// the kernel past 256 VGPRs and to one wave per SIMD; one step ahead is 16
// per buffer and leaves room for three. At BM = 128 the two waves of an N
// half load the same lines; the second load is an L2 / TCP hit.
//
// Scales. One dword per lane per n-block per four k-steps, op_sel picks the
// byte and must be a compile-time constant: the k loop is unrolled by the
// quad, the next quad's dwords are loaded a quad ahead, and a ragged tail
// runs the 1..3 steps of K % 512 != 0. A's scale is 2^0 in every byte.
//
// Epilogue. acc * a_scale[m] * w_scale[n], one rounding to bf16, then each
// wave transposes its tile through its own quarter of the (now idle) A
// buffers so that the global stores are 16 bytes per lane, eight lanes per
// 128-byte (64-byte at BM = 64) row piece, masked at rows >= M. The
// transpose is swizzled too: 16-byte chunk c of tile row R sits at
// c ^ (((R >> 2) & 3) * CH / 4), CH chunks per row, so the four g of a
// 2-byte write (rows 4g + i) land on different banks.
//
// Resources (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage):
//   BM = 128: 151 VGPRs, 0 AGPRs, 32 KiB LDS, 3 waves/SIMD (3 workgroups
//             per CU), scratch 0
//   BM = 64 : 103 VGPRs, 0 AGPRs, 16 KiB LDS, 4 waves/SIMD, scratch 0
#include "common.h"
#include "mxfp4_tiles.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int gx_i32x8_t;
typedef __attribute__((ext_vector_type(4))) float gx_f32x4_t;

constexpr int GX_BN = 128;      // output columns per workgroup
constexpr int GX_THREADS = 256;
constexpr int GX_CHUNKS = MX_KSTEP / 16;  // 16-byte chunks per A row and step

template <int BM, int WM>
struct GxTile {
  static constexpr int WN = 4 / WM;                // waves along N
  static constexpr int WROWS = BM / WM;            // rows per wave
  static constexpr int MT = WROWS / 16;            // m tiles per wave
  static constexpr int NT = GX_BN / WN / MX_NT;    // n blocks per wave
  static constexpr int LD = BM * GX_CHUNKS / GX_THREADS;  // A loads / thread
  static constexpr int CH = NT * MX_NT / 8;        // bf16x8 chunks per C row
};

// issue the global loads of one A tile: LD x 16 bytes per thread, as raw
// buffer loads over the tile's valid rows only. An offset past the
// descriptor's size (a row >= M) returns zeros without touching memory, and
// the loads need no branch, so all of a step's loads are in flight together.
template <int LD>
__device__ __forceinline__ void gx_load_a(__amdgpu_buffer_rsrc_t rsrc, int off,
                                          int pass_stride, uint32x4* regs) {
#pragma unroll
  for (int i = 0; i < LD; ++i)
    regs[i] = __builtin_bit_cast(
        uint32x4, __builtin_amdgcn_raw_buffer_load_b128(
                      rsrc, off + i * pass_stride, 0, 0));
}

// one k-step of a wave: MT A fragments out of LDS against NT weight lines
template <int SEL, int MT, int NT>
__device__ __forceinline__ void gx_mfma(const uint32x4* abuf, int lo, int hi,
                                        const uint32x4* bv, const int* sc,
                                        gx_f32x4_t (*acc)[NT]) {
  gx_i32x8_t af[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const uint32x4 l = abuf[lo + t * 16 * GX_CHUNKS];
    const uint32x4 h = abuf[hi + t * 16 * GX_CHUNKS];
    af[t] = gx_i32x8_t{(int)l.x, (int)l.y, (int)l.z, (int)l.w,
                       (int)h.x, (int)h.y, (int)h.z, (int)h.w};
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const gx_i32x8_t b = {(int)bv[j].x, (int)bv[j].y, (int)bv[j].z,
                          (int)bv[j].w, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < MT; ++t)
      acc[t][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          af[t], b, acc[t][j], /*cbsz=e4m3*/ 0, /*blgp=e2m1*/ 4, 0,
          MX_SCALE_ONE, SEL, sc[j]);
  }
}

// waves_per_eu: without it the accumulators are placed in AGPRs and the
// BM = 128 body takes 102 VGPRs + 84 AGPRs, two waves per SIMD instead of
// three
template <int BM, int WM>
__global__ __launch_bounds__(GX_THREADS)
__attribute__((amdgpu_waves_per_eu(2))) void gemm_mxfp4_kernel(
    const unsigned char* __restrict__ a,  // [M, K] e4m3 row-major
    const float* __restrict__ a_scale,    // [M]
    const uint32x4* __restrict__ w4t,     // [N/16][K/128][64] 16-B lines
    const int* __restrict__ e8t,          // [N/16][ceil(K/512)][64] dwords
    const float* __restrict__ w_scale,    // [N]
    __hip_bfloat16* __restrict__ c,       // [M, N]
    int M, int N, int K) {
  typedef GxTile<BM, WM> T;
  constexpr int MT = T::MT, NT = T::NT, LD = T::LD, CH = T::CH;
  __shared__ uint32x4 lds[2][BM * GX_CHUNKS];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int row = lane & 15, g = lane >> 4;
  const int wm = wave % WM, wn = wave / WM;
  const int m0 = blockIdx.x * BM;
  const int nb0 = blockIdx.y * (GX_BN / MX_NT) + wn * NT;

  const int nsteps = K / MX_KSTEP;
  const int nfull = nsteps / MX_QUAD;
  const int nquads = (nsteps + MX_QUAD - 1) / MX_QUAD;

  // A staging: thread -> (row tid / 8 + 32 i, chunk tid % 8); 32 i leaves
  // the swizzle key (r >> 1) & 7 alone, so one LDS offset serves every pass
  const int srow = tid >> 3, schunk = tid & 7;
  // descriptor: this tile's rows < M, byte-addressed (stride 0), 32-bit data
  const int rows = min(BM, M - m0);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(a) + (long)m0 * K, 0, rows * K, 0x00020000);
  const int aoff = srow * K + schunk * 16;
  const int pass_stride = 32 * K;
  const int soff = srow * GX_CHUNKS + (schunk ^ ((srow >> 1) & 7));

  // fragment reads: tile rows start at multiples of 16, so the key is row's
  const int frow = wm * T::WROWS + row;
  const int key = (row >> 1) & 7;
  const int flo = frow * GX_CHUNKS + (g ^ key);
  const int fhi = frow * GX_CHUNKS + ((4 + g) ^ key);

  const uint32x4* wt = w4t + (long)nb0 * nsteps * 64 + lane;
  const int* st = e8t + (long)nb0 * nquads * 64 + lane;
  const long wstride = (long)nsteps * 64;  // to the next n-block's lines
  const long sstride = (long)nquads * 64;

  gx_f32x4_t acc[MT][NT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[t][j] = gx_f32x4_t{0.f, 0.f, 0.f, 0.f};

  // b0 / b1: the weight lines of even / odd k-steps (quads and the tail
  // start on even steps, so which is which is static)
  uint32x4 areg[LD], b0[NT], b1[NT];
  int sc[NT], scn[NT];
  gx_load_a<LD>(rsrc, aoff, pass_stride, areg);
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    b0[j] = wt[j * wstride];
    sc[j] = st[j * sstride];
  }
#pragma unroll
  for (int i = 0; i < LD; ++i) lds[0][soff + i * 32 * GX_CHUNKS] = areg[i];
  __syncthreads();

  // step s: fetch step s + 1 (A to registers, B lines into BN), multiply
  // step s out of lds[s & 1] against BC, park A in lds[(s + 1) & 1]. The
  // barrier orders that write before the next step's reads, and this step's
  // reads before the write after next; the last one frees both buffers for
  // the epilogue. The last step fetches itself again instead of branching:
  // in bounds, and written to the buffer nobody reads any more.
#define GX_STEP(SEL, s, BC, BN)                                             \
  do {                                                                      \
    const int sn_ = min((s) + 1, nsteps - 1);                               \
    gx_load_a<LD>(rsrc, aoff + sn_ * MX_KSTEP, pass_stride, areg);          \
    _Pragma("unroll") for (int j = 0; j < NT; ++j)                          \
        BN[j] = wt[j * wstride + (long)sn_ * 64];                           \
    gx_mfma<SEL, MT, NT>(lds[SEL & 1], flo, fhi, BC, sc, acc);              \
    _Pragma("unroll") for (int i = 0; i < LD; ++i)                          \
        lds[(SEL + 1) & 1][soff + i * 32 * GX_CHUNKS] = areg[i];            \
    __syncthreads();                                                        \
  } while (0)

  for (int q = 0; q < nfull; ++q) {
    const long qn = min(q + 1, nquads - 1);
#pragma unroll
    for (int j = 0; j < NT; ++j) scn[j] = st[j * sstride + qn * 64];
    GX_STEP(0, q * MX_QUAD, b0, b1);
    GX_STEP(1, q * MX_QUAD + 1, b1, b0);
    GX_STEP(2, q * MX_QUAD + 2, b0, b1);
    GX_STEP(3, q * MX_QUAD + 3, b1, b0);
#pragma unroll
    for (int j = 0; j < NT; ++j) sc[j] = scn[j];
  }
  // ragged last dword (K % 512 != 0): 1..3 steps
  const int rem = nsteps - nfull * MX_QUAD;
  if (rem > 0) {
    GX_STEP(0, nfull * MX_QUAD, b0, b1);
    if (rem > 1) GX_STEP(1, nfull * MX_QUAD + 1, b1, b0);
    if (rem > 2) GX_STEP(2, nfull * MX_QUAD + 2, b0, b1);
  }
#undef GX_STEP

  // epilogue: scale, round once, transpose through this wave's share of LDS
  unsigned short* ct = reinterpret_cast<unsigned short*>(&lds[0][0]) +
                       wave * (T::WROWS * CH * 8);
  constexpr int KEYMUL = CH / 4;
  float ws[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) ws[j] = w_scale[(nb0 + j) * MX_NT + row];
  const int mw = m0 + wm * T::WROWS;  // first row of this wave
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int R = t * 16 + g * 4 + i;
      const float as = mw + R < M ? a_scale[mw + R] : 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const __hip_bfloat16 v = __float2bfloat16(acc[t][j][i] * as * ws[j]);
        const int col = j * MX_NT + row;
        const int chunk = (col >> 3) ^ (g * KEYMUL);  // (R >> 2) & 3 == g
        ct[(R * CH + chunk) * 8 + (col & 7)] =
            *reinterpret_cast<const unsigned short*>(&v);
      }
    }
  }
  __syncthreads();
  const uint32x4* cv = reinterpret_cast<const uint32x4*>(ct);
  __hip_bfloat16* cw = c + (long)nb0 * MX_NT;
#pragma unroll
  for (int it = 0; it < T::WROWS * CH / 64; ++it) {
    const int idx = it * 64 + lane;
    const int R = idx / CH, cc = idx % CH;
    const int m = mw + R;
    if (m < M)
      *reinterpret_cast<uint32x4*>(cw + (long)m * N + cc * 8) =
          cv[R * CH + (cc ^ (((R >> 2) & 3) * KEYMUL))];
  }
}

}  // namespace

#ifndef CMLS_KERNEL_ONLY
// tile: rows per workgroup, 64 or 128 (the Python layer picks the measured
// default; the benchmark times both)
torch::Tensor gemm_mxfp4(torch::Tensor a8, torch::Tensor a_scale,
                         torch::Tensor w4t, torch::Tensor e8t,
                         torch::Tensor w_scale, int64_t tile) {
  TORCH_CHECK(a8.dim() == 2, "gemm_mxfp4: a8 is [M, K]");
  TORCH_CHECK(a8.scalar_type() == at::kByte ||
              a8.scalar_type() == at::kFloat8_e4m3fn);
  TORCH_CHECK(a8.is_contiguous() && a_scale.is_contiguous());
  TORCH_CHECK(a_scale.scalar_type() == at::kFloat);
  const long M = a8.size(0), K = a8.size(1), N = w_scale.numel();
  TORCH_CHECK(M >= 1, "gemm_mxfp4: M must be >= 1");
  TORCH_CHECK(K >= MX_KSTEP && K % MX_KSTEP == 0, "gemm_mxfp4: K % 128 != 0");
  TORCH_CHECK(N >= GX_BN && N % GX_BN == 0, "gemm_mxfp4: N % 128 != 0");
  TORCH_CHECK(M <= (1 << 24) && K <= (1 << 23) && N / GX_BN <= 65535,
              "gemm_mxfp4: shape out of range");
  TORCH_CHECK(a_scale.numel() == M);
  TORCH_CHECK(a_scale.device() == a8.device() && w4t.device() == a8.device() &&
              e8t.device() == a8.device() && w_scale.device() == a8.device(),
              "gemm_mxfp4: all operands must be on one GPU");
  TORCH_CHECK((uintptr_t)a8.data_ptr() % 16 == 0,
              "gemm_mxfp4: misaligned activations");
  check_mx_tiles(w4t, e8t, w_scale, (int)N, (int)K, "gemm_mxfp4");
  auto c = torch::empty({M, N}, a8.options().dtype(torch::kBFloat16));
  TORCH_CHECK(tile == 64 || tile == 128, "gemm_mxfp4: tile must be 64 or 128");
#define LAUNCH_GX(BM, WM)                                                    \
  hipLaunchKernelGGL((gemm_mxfp4_kernel<BM, WM>),                            \
                     dim3((M + BM - 1) / BM, N / GX_BN), dim3(GX_THREADS),   \
                     0, cmls::current_stream(),                              \
                     (const unsigned char*)a8.data_ptr(),                    \
                     (const float*)a_scale.data_ptr(),                       \
                     (const uint32x4*)w4t.data_ptr(),                        \
                     (const int*)e8t.data_ptr(),                             \
                     (const float*)w_scale.data_ptr(),                       \
                     (__hip_bfloat16*)c.data_ptr(), (int)M, (int)N, (int)K)
  if (tile == 128)
    LAUNCH_GX(128, 2);
  else
    LAUNCH_GX(64, 1);
#undef LAUNCH_GX
  return c;
}
#endif  // CMLS_KERNEL_ONLY
