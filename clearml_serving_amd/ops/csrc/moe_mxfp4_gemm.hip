// MoE prefill with MXFP4 expert weights: the grouped variant of the
// mxfp4_gemm.hip tile, for calls whose experts see many rows each. The fused
// kernels of moe_mxfp4.hip are decode-shaped (one row block x 16 columns per
// workgroup, every row block re-streams the whole expert); here one
// workgroup owns 128 sorted slots of one expert x 128 weight columns and a
// weight line is read once per 128 rows.
//
//   moe_align(128)  group the S = T*k slots by expert, 128-row blocks (moe.hip)
//   gate/up         moe_gemm_mxfp4_tiled_kernel<true>   -> bf16 act [S, I]
//   quant_fp8       act rows -> e4m3 bytes + per-row scale      (fp8_path.hip)
//   down            moe_gemm_mxfp4_tiled_kernel<false>  -> fp32 y [S, H]
//   combine         out[t] = sum_j weights[t, j] * y[t*k + j]        (moe.hip)
//
// Same data flow and roundings as the fused path; sync-free and capturable.
// Weights are the per-expert ops.tile_mxfp4_weight buffers, unchanged:
//   w4t [E][NB][K/128][64][16 B], e8t [E][NB][ceil(K/512)][64][4 B]
// on v_mfma_scale_f32_16x16x128_f8f6f4 (A = e4m3 with scale 2^0, B = e2m1
// with the e8m0 block scales; operand maps in mxfp4_path.hip; lane l =
// (r, g), r = l % 16, g = l / 16).
//
// Work split. 256 threads = 4 waves as 2 (rows) x 2 (columns); a wave holds
// 4 m-tiles x 4 n-blocks = 16 f32x4 accumulators. Grid (nb_max, column
// tiles): the row blocks are on the fast axis and align places an expert's
// blocks next to each other, so workgroups that run together read the same
// weight lines and share them in L2. A block whose expert is -1 returns
// before any barrier.
//   !GATED  W = w2[e]: the workgroup's 8 n-blocks are tile rows 8 by .. 8 by
//           + 7, wave column wn takes 4 wn .. 4 wn + 3
//   GATED   W = w13[e]: the workgroup owns 64 activation columns; wave column
//           wn takes gate tile rows 4 by + 2 wn + {0, 1} (accumulators j = 0,
//           1) and the matching up rows I/16 + 4 by + 2 wn + {0, 1} (j = 2,
//           3). acc[t][jj] and acc[t][2 + jj] share one lane map, so
//           silu(g) * u is formed in registers.
//
// K. No split-K, no atomics: one wave accumulates an output element over the
// k-steps in ascending order, and MFMA rows are independent, so a slot's
// result does not depend on T, on the slots it is batched with or on its
// place in the block.
//
// A: gathered, through LDS. Per k-step the tile is 128 rows x 128 bytes.
// Thread t loads 16 bytes of tile row t / 8 + 32 i, chunk t % 8, i = 0..3:
// eight lanes read one 128-byte line of one source row. The source row is
// slot / top_k (GATED) or slot (!GATED), looked up once per pass before the
// k loop. The loads are raw buffer loads over the whole A matrix; a sentinel
// row (slot >= n_slots) gets the offset one past the matrix, which stays out
// of range at every k-step and returns zeros without a branch and without
// touching memory. The host keeps (rows + 1) * K below 2^32 so that offset
// never wraps. Two LDS buffers (2 x 16 KiB); step s + 1's global loads are
// issued before step s's MFMAs and written to the other buffer after them,
// one barrier per step.
//   Swizzle and fragment reads are those of mxfp4_gemm.hip: chunk c of tile
//   row r is stored at c ^ ((r >> 1) & 7); lane (r, g) reads chunks g and
//   4 + g of row r (two ds_read_b128). For a fixed logical chunk the bank
//   group of a read is 32 (r & 1) + 4 (c ^ ((r >> 1) & 7)), a bijection of
//   r = 0..15 onto the 16 four-bank groups: degree 1.
//   Gathered writes: the gather changes which global line a lane reads, not
//   where it parks it. A write pass still has 16 consecutive lanes cover
//   tile rows 2 i and 2 i + 1 with all eight chunks each (2 x 128 bytes = 64
//   banks), the swizzle permutes chunks within a row, so the 16 lanes cover
//   every bank once: degree 1, whatever rows the slots name. The + 32 i of
//   the passes leaves the key (r >> 1) & 7 alone, so one LDS offset serves
//   all four.
//
// B and scales. One contiguous 1 KiB line per n-block and k-step (16 B per
// lane) straight from global memory, one step ahead in registers; the two
// waves of a column half load the same lines, the second is an L2 / TCP hit.
// One scale dword per lane per n-block per four k-steps, loaded a quad
// ahead; op_sel picks the byte and must be a compile-time constant, so the k
// loop is unrolled by the quad and a ragged tail runs the 1..3 steps of
// K % 512 != 0.
//
// Epilogue. acc * a_scale[row] * w_scale[e, n] in fp32; GATED then forms
// g / (1 + expf(-g)) * u (the fused kernel's expression) and rounds once to
// bf16. Each wave transposes through its own 8 KiB of the idle A buffers so
// that a row piece leaves in 16-byte lane stores, scattered by slot;
// sentinel rows store nothing.
//   GATED   64 rows x 32 bf16 = 4 KiB, one pass; four lanes write a row's 64
//           bytes. 16-byte chunk c of tile row R sits at c ^ ((R >> 2) & 3):
//           the four g of a 2-byte write (rows 4 g + i) land on different
//           four-bank groups; the two column octets of a 16-column block
//           meet pairwise, a 2-way conflict on 32 writes per wave.
//   !GATED  the wave's 64 x 64 fp32 is 16 KiB against 8 KiB: staged in
//           halves of 32 rows (two m-tiles), 16 lanes write a row's 256
//           bytes. Chunk c of row R sits at c ^ (4 ((R >> 2) & 3)): a write
//           has bank 16 (j ^ g) + r, all 64 lanes distinct.
// The target attribute keeps the SwiGLU epilogue free of packed fp32 ops,
// as in moe_mxfp4.hip: set on the function, not as a build flag.
//
// Resources (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage):
//   GATED : 160 VGPRs, 0 AGPRs, 32 KiB LDS, 3 waves/SIMD (3 workgroups per
//           CU), scratch 0
//   !GATED: 164 VGPRs, 0 AGPRs, 32 KiB LDS, 3 waves/SIMD, scratch 0
#include "common.h"
#include "mxfp4_tiles.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int mt_i32x8_t;
typedef __attribute__((ext_vector_type(4))) float mt_f32x4_t;

constexpr int MT_BM = 128;      // sorted slots per workgroup
constexpr int MT_BN = 128;      // weight columns per workgroup
constexpr int MT_THREADS = 256;
constexpr int MT_CHUNKS = MX_KSTEP / 16;  // 16-byte chunks per A row and step
constexpr int MT_WROWS = 64;    // rows per wave
constexpr int MT_M = 4;         // m tiles per wave
constexpr int MT_N = 4;         // n blocks per wave
constexpr int MT_LD = MT_BM * MT_CHUNKS / MT_THREADS;  // A loads per thread

// The kernel's target attribute (below) keeps header functions that are not
// always_inline from being inlined into it: they would stay calls, and a
// call in the k loop spills the accumulators. So the barrier and the bf16
// rounding are spelled here. mt_barrier is __syncthreads; mt_bf16_bits is
// the round-to-nearest-even conversion of __float2bfloat16.
__device__ __forceinline__ void mt_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ unsigned short mt_bf16_bits(float v) {
  return __builtin_bit_cast(unsigned short, static_cast<__bf16>(v));
}

// issue the global loads of one gathered A tile: MT_LD x 16 bytes per
// thread, byte offsets off[i] + koff into the whole matrix. An offset past
// the descriptor's size (a sentinel row) returns zeros without touching
// memory; no branch, so all of a step's loads are in flight together.
__device__ __forceinline__ void mt_load_a(__amdgpu_buffer_rsrc_t rsrc,
                                          const unsigned* off, unsigned koff,
                                          uint32x4* regs) {
#pragma unroll
  for (int i = 0; i < MT_LD; ++i)
    regs[i] = __builtin_bit_cast(
        uint32x4, __builtin_amdgcn_raw_buffer_load_b128(
                      rsrc, (int)(off[i] + koff), 0, 0));
}

// one k-step of a wave: 4 A fragments out of LDS against 4 weight lines
template <int SEL>
__device__ __forceinline__ void mt_mfma(const uint32x4* abuf, int lo, int hi,
                                        const uint32x4* bv, const int* sc,
                                        mt_f32x4_t (*acc)[MT_N]) {
  mt_i32x8_t af[MT_M];
#pragma unroll
  for (int t = 0; t < MT_M; ++t) {
    const uint32x4 l = abuf[lo + t * 16 * MT_CHUNKS];
    const uint32x4 h = abuf[hi + t * 16 * MT_CHUNKS];
    af[t] = mt_i32x8_t{(int)l.x, (int)l.y, (int)l.z, (int)l.w,
                       (int)h.x, (int)h.y, (int)h.z, (int)h.w};
  }
#pragma unroll
  for (int j = 0; j < MT_N; ++j) {
    const mt_i32x8_t b = {(int)bv[j].x, (int)bv[j].y, (int)bv[j].z,
                          (int)bv[j].w, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < MT_M; ++t)
      acc[t][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          af[t], b, acc[t][j], /*cbsz=e4m3*/ 0, /*blgp=e2m1*/ 4, 0,
          MX_SCALE_ONE, SEL, sc[j]);
  }
}

// grid (nb_max, N/64 GATED or N/128), block 4 waves.
//   GATED:  A row = a[slot / k], W = w13[e] (2N/16 tile rows, gate then up),
//           out = bf16 act[slot, n] = silu(g) * u, N = I
//   !GATED: A row = a[slot],     W = w2[e] (N/16 tile rows),
//           out = fp32 y[slot, n], N = H
// a_scale is indexed like a's rows, w_scale like w's rows; a_bytes is the
// size of a (rows * K).
// waves_per_eu: as in mxfp4_gemm.hip, without it the accumulators go to
// AGPRs and the kernel drops a wave per SIMD.
template <bool GATED>
__global__ __launch_bounds__(MT_THREADS)
__attribute__((amdgpu_waves_per_eu(2), target("no-packed-fp32-ops")))
void moe_gemm_mxfp4_tiled_kernel(
    const unsigned char* __restrict__ a,  // [T, K] or [S, K] e4m3
    const float* __restrict__ a_scale,    // [T] or [S]
    const uint32x4* __restrict__ w4t,     // [E][NB][K/128][64] 16-B lines
    const int* __restrict__ e8t,          // [E][NB][ceil(K/512)][64] dwords
    const float* __restrict__ w_scale,    // [E, (2)N]
    const int* __restrict__ sorted_slots,
    const int* __restrict__ block_expert,
    void* __restrict__ out,               // bf16 [S, N] or fp32 [S, N]
    int n_slots, int top_k, int N, int K, unsigned a_bytes) {
  const int e = block_expert[blockIdx.x];
  if (e < 0) return;
  __shared__ uint32x4 lds[2][MT_BM * MT_CHUNKS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  const int by = blockIdx.y;
  const int* slots = sorted_slots + (long)blockIdx.x * MT_BM;

  const int nsteps = K / MX_KSTEP;
  const int nfull = nsteps / MX_QUAD;
  const int nquads = (nsteps + MX_QUAD - 1) / MX_QUAD;

  // weight lines and scale dwords of this wave's four n-blocks
  const long half_rows = N / MX_NT;  // tile rows of w2[e], or of a w13 half
  const long tile_rows = GATED ? 2 * half_rows : half_rows;
  const uint32x4* wt[MT_N];
  const int* st[MT_N];
#pragma unroll
  for (int j = 0; j < MT_N; ++j) {
    const long tr = GATED ? 4 * by + 2 * wn + (j & 1) + (j >> 1) * half_rows
                          : 8 * by + 4 * wn + j;
    wt[j] = w4t + ((long)e * tile_rows + tr) * nsteps * 64;
    st[j] = e8t + ((long)e * tile_rows + tr) * nquads * 64;
  }

  // A staging: thread -> (tile row tid / 8 + 32 i, chunk tid % 8)
  const int srow = tid >> 3, schunk = tid & 7;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(a), 0, a_bytes, 0x00020000);
  unsigned aoff[MT_LD];
#pragma unroll
  for (int i = 0; i < MT_LD; ++i) {
    const int s = slots[srow + 32 * i];
    const unsigned r = GATED ? s / top_k : s;
    aoff[i] = s < n_slots ? r * (unsigned)K + schunk * 16 : a_bytes;
  }
  const int soff = srow * MT_CHUNKS + (schunk ^ ((srow >> 1) & 7));

  // fragment reads: tile rows start at multiples of 16, so the key is row's
  const int frow = wm * MT_WROWS + row;
  const int key = (row >> 1) & 7;
  const int flo = frow * MT_CHUNKS + (g ^ key);
  const int fhi = frow * MT_CHUNKS + ((4 + g) ^ key);

  mt_f32x4_t acc[MT_M][MT_N];
#pragma unroll
  for (int t = 0; t < MT_M; ++t)
#pragma unroll
    for (int j = 0; j < MT_N; ++j) acc[t][j] = mt_f32x4_t{0.f, 0.f, 0.f, 0.f};

  // b0 / b1: the weight lines of even / odd k-steps (quads and the tail
  // start on even steps, so which is which is static)
  uint32x4 areg[MT_LD], b0[MT_N], b1[MT_N];
  int sc[MT_N], scn[MT_N];
  mt_load_a(rsrc, aoff, 0, areg);
#pragma unroll
  for (int j = 0; j < MT_N; ++j) {
    b0[j] = wt[j][lane];
    sc[j] = st[j][lane];
  }
#pragma unroll
  for (int i = 0; i < MT_LD; ++i) lds[0][soff + i * 32 * MT_CHUNKS] = areg[i];
  mt_barrier();

  // step s: fetch step s + 1 (A to registers, B lines into BN), multiply
  // step s out of lds[s & 1] against BC, park A in lds[(s + 1) & 1]. The
  // barrier orders that write before the next step's reads, and this step's
  // reads before the write after next; the last one frees both buffers for
  // the epilogue. The last step fetches itself again instead of branching:
  // in bounds, and written to the buffer nobody reads any more.
#define MT_STEP(SEL, s, BC, BN)                                             \
  do {                                                                      \
    const int sn_ = min((s) + 1, nsteps - 1);                               \
    mt_load_a(rsrc, aoff, (unsigned)sn_ * MX_KSTEP, areg);                  \
    _Pragma("unroll") for (int j = 0; j < MT_N; ++j)                        \
        BN[j] = (wt[j] + (long)sn_ * 64)[lane];                             \
    mt_mfma<SEL>(lds[SEL & 1], flo, fhi, BC, sc, acc);                      \
    _Pragma("unroll") for (int i = 0; i < MT_LD; ++i)                       \
        lds[(SEL + 1) & 1][soff + i * 32 * MT_CHUNKS] = areg[i];            \
    mt_barrier();                                                        \
  } while (0)

  for (int q = 0; q < nfull; ++q) {
    const long qn = min(q + 1, nquads - 1);
#pragma unroll
    for (int j = 0; j < MT_N; ++j) scn[j] = (st[j] + qn * 64)[lane];
    MT_STEP(0, q * MX_QUAD, b0, b1);
    MT_STEP(1, q * MX_QUAD + 1, b1, b0);
    MT_STEP(2, q * MX_QUAD + 2, b0, b1);
    MT_STEP(3, q * MX_QUAD + 3, b1, b0);
#pragma unroll
    for (int j = 0; j < MT_N; ++j) sc[j] = scn[j];
  }
  // ragged last dword (K % 512 != 0): 1..3 steps
  const int rem = nsteps - nfull * MX_QUAD;
  if (rem > 0) {
    MT_STEP(0, nfull * MX_QUAD, b0, b1);
    if (rem > 1) MT_STEP(1, nfull * MX_QUAD + 1, b1, b0);
    if (rem > 2) MT_STEP(2, nfull * MX_QUAD + 2, b0, b1);
  }
#undef MT_STEP

  // epilogue: scale, (SwiGLU, round once,) transpose through this wave's
  // 8 KiB of LDS, scatter by slot
  const int* wslots = slots + wm * MT_WROWS;
  uint32x4* cv = &lds[0][0] + wave * (MT_BM * MT_CHUNKS * 2 / 4);
  if (GATED) {
    constexpr int CH = 4;  // bf16x8 chunks per row: 32 activation columns
    const int c0 = (4 * by + 2 * wn) * MX_NT;  // the wave's first column
    const float* wsc = w_scale + (long)e * 2 * N + c0 + row;
    float wsg[2], wsu[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      wsg[jj] = wsc[jj * MX_NT];
      wsu[jj] = wsc[N + jj * MX_NT];
    }
    unsigned short* ct = reinterpret_cast<unsigned short*>(cv);
#pragma unroll
    for (int t = 0; t < MT_M; ++t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int R = t * 16 + g * 4 + i;
        const int s = wslots[R];
        const float as = s < n_slots ? a_scale[s / top_k] : 0.f;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const float gv = acc[t][jj][i] * as * wsg[jj];
          const float uv = acc[t][2 + jj][i] * as * wsu[jj];
          const float v = gv / (1.f + expf(-gv)) * uv;
          const int col = jj * MX_NT + row;
          const int chunk = (col >> 3) ^ g;  // (R >> 2) & 3 == g
          ct[(R * CH + chunk) * 8 + (col & 7)] = mt_bf16_bits(v);
        }
      }
    }
    mt_barrier();
    __hip_bfloat16* cw = reinterpret_cast<__hip_bfloat16*>(out) + c0;
#pragma unroll
    for (int it = 0; it < MT_WROWS * CH / 64; ++it) {
      const int idx = it * 64 + lane;
      const int R = idx / CH, cc = idx % CH;
      const int s = wslots[R];
      if (s < n_slots)
        *reinterpret_cast<uint32x4*>(cw + (long)s * N + cc * 8) =
            cv[R * CH + (cc ^ ((R >> 2) & 3))];
    }
  } else {
    constexpr int CH = 16;  // f32x4 chunks per row: 64 columns
    const int c0 = (8 * by + 4 * wn) * MX_NT;
    const float* wsc = w_scale + (long)e * N + c0 + row;
    float ws[MT_N];
#pragma unroll
    for (int j = 0; j < MT_N; ++j) ws[j] = wsc[j * MX_NT];
    float* ft = reinterpret_cast<float*>(cv);
    float* cw = reinterpret_cast<float*>(out) + c0;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {  // 32 rows = two m-tiles at a time
      const int* hslots = wslots + hf * 32;
#pragma unroll
      for (int tl = 0; tl < 2; ++tl) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int R = tl * 16 + g * 4 + i;
          const int s = hslots[R];
          const float as = s < n_slots ? a_scale[s] : 0.f;
#pragma unroll
          for (int j = 0; j < MT_N; ++j) {
            const int col = j * MX_NT + row;
            const int chunk = (col >> 2) ^ (g * 4);  // (R >> 2) & 3 == g
            ft[(R * CH + chunk) * 4 + (col & 3)] =
                acc[hf * 2 + tl][j][i] * as * ws[j];
          }
        }
      }
      mt_barrier();
#pragma unroll
      for (int it = 0; it < 32 * CH / 64; ++it) {
        const int idx = it * 64 + lane;
        const int R = idx / CH, cc = idx % CH;
        const int s = hslots[R];
        if (s < n_slots)
          *reinterpret_cast<uint32x4*>(cw + (long)s * N + cc * 4) =
              cv[R * CH + (cc ^ (((R >> 2) & 3) * 4))];
      }
      mt_barrier();  // the next half overwrites the staging rows
    }
  }
}

}  // namespace

#ifndef CMLS_KERNEL_ONLY
#include "moe.h"

// fp8_path.hip: per-row absmax quantisation to e4m3, {bytes [R, C], scale [R]}
std::vector<torch::Tensor> quant_fp8(torch::Tensor x);

// The block_m == 128 path of moe_experts_mxfp4 (moe_mxfp4.hip), which has
// checked dtypes, shapes, devices, alignment and the tilings; only what this
// kernel adds is checked here.
torch::Tensor moe_experts_mxfp4_tiled(torch::Tensor x8, torch::Tensor x_scale,
                                      torch::Tensor w13_t,
                                      torch::Tensor w13_e8t,
                                      torch::Tensor w13_scale,
                                      torch::Tensor w2_t, torch::Tensor w2_e8t,
                                      torch::Tensor w2_scale,
                                      torch::Tensor ids,
                                      torch::Tensor weights) {
  const long t = x8.size(0), h = x8.size(1);
  const long e = w13_scale.size(0), inter = w13_scale.size(1) / 2;
  const long k = ids.size(1), s = t * k;
  TORCH_CHECK(inter / (MT_BN / 2) <= 65535 && h / MT_BN <= 65535,
              "moe_experts_mxfp4: too many column tiles for block_m=128");
  // sentinel rows read at byte offset rows * K + k-step: must not wrap
  TORCH_CHECK((t + 1) * h < (1L << 32) && (s + 1) * inter < (1L << 32),
              "moe_experts_mxfp4: block_m=128 needs activation matrices "
              "under 4 GiB, got [", t, ", ", h, "] and [", s, ", ", inter,
              "]");

  torch::Tensor sorted_slots, block_expert;
  cmls_moe::launch_align(ids, e, MT_BM, sorted_slots, block_expert);
  const long nb_max = block_expert.size(0);  // grid x: up to 2^31 - 1

  auto act = torch::empty({s, inter}, x8.options().dtype(at::kBFloat16));
  auto y = torch::empty({s, h}, x8.options().dtype(at::kFloat));
  auto out = torch::empty({t, h}, x8.options().dtype(at::kBFloat16));
  hipStream_t stream_ = cmls::current_stream();
  const int* ss = sorted_slots.data_ptr<int>();
  const int* be = block_expert.data_ptr<int>();
#define LAUNCH_MT(GATED, TILES, A, AS, W, WE, WS, OUT, N, K)                \
  hipLaunchKernelGGL((moe_gemm_mxfp4_tiled_kernel<GATED>),                  \
                     dim3((unsigned)nb_max, (unsigned)(TILES)),             \
                     dim3(MT_THREADS), 0, stream_,                          \
                     (const unsigned char*)(A).data_ptr(),                  \
                     (const float*)(AS).data_ptr(),                         \
                     (const uint32x4*)(W).data_ptr(),                       \
                     (const int*)(WE).data_ptr(),                           \
                     (const float*)(WS).data_ptr(), ss, be,                 \
                     (OUT).data_ptr(), (int)s, (int)k, (int)(N), (int)(K),  \
                     (unsigned)((A).size(0) * (K)))
  LAUNCH_MT(true, inter / (MT_BN / 2), x8, x_scale, w13_t, w13_e8t,
            w13_scale, act, inter, h);
  // every act row is a slot, and align places every slot exactly once
  auto q = quant_fp8(act);  // {e4m3 [S, I], fp32 scale [S]}
  LAUNCH_MT(false, h / MT_BN, q[0], q[1], w2_t, w2_e8t, w2_scale, y, h, inter);
#undef LAUNCH_MT
  cmls_moe::launch_combine(y, weights, out, "moe_experts_mxfp4");
  return out;
}
#endif  // CMLS_KERNEL_ONLY
