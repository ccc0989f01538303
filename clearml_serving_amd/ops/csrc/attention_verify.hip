// Multi-query split-KV paged attention for gfx950: the verification forward
// of speculative decoding (1..8 in-flight query tokens per sequence against
// a paged KV cache). Key/position contract of attention_prefill_paged: the
// query tokens' K/V are already in the cache, kv_lens[b] counts them, row j
// sits at position kv_lens[b] - q_lens[b] + j and sees key n iff n <= pos
// (and n > pos - window with a sliding window).
//
// Grid and work split
//   grid = (B, Hkv, splits); block = 4 waves. One workgroup owns one
//   (sequence, kv head, key range), so K/V leave HBM once per kv head for
//   all R = GQ * Sq query rows. The key range [lo, kv_len) -- lo is the
//   window start of the first row, 0 without a window -- is cut into
//   `splits` chunks rounded up to the 32-key wave tile (no overlap); a split
//   past the end publishes a neutral partial (m = -inf, l = 0).
//   Inside a workgroup the four waves take the chunk's 32-key tiles
//   round-robin and never talk to each other until the end: every wave
//   stages ITS tile through ITS slice of LDS and carries its own
//   online-softmax state, so the key loop has no workgroup barrier. The
//   four states merge through LDS once (flash-decoding inside the block),
//   wave 0 then stores the output (splits == 1) or the fp32 partial
//   (o, m, l); attn_verify_combine_kernel folds the partials per row.
//
// Row tile
//   Row index ridx = j * GQ + gq (token-major), so the rows a sequence
//   really has (j < q_len) are the first GQ * q_len ones. The rows are the
//   N side of S^T = mfma(K, Q) and of O^T = mfma(V^T, P^T)
//   (v_mfma_f32_16x16x32_bf16, fp32 accumulate), padded to NT = 1, 2 or 4
//   tiles of 16: the instantiation is picked by R (<= 16, <= 32, <= 64),
//   not by the (GQ, Sq) pair. A K or V fragment read from LDS feeds all NT
//   row tiles. Q fragments stay in registers for the whole kernel.
//
// Swapped Q K^T without lane moves
//   As in attention.hip the C layout of S^T gives each lane one query
//   column (softmax max/sum = 2 shfl_xor, (m, l) lane-local). There the
//   lane's S values (keys 16t + 4g + r) need 8 shuffles per tile to become
//   the P^T B-fragment (keys 8g + e). Here the K rows are PERMUTED when
//   they are written to LDS instead: tile key kk = 8a + 4t + c sits in LDS
//   row 16t + 4a + c, so lane group g's accumulator element (t, r) IS key
//   8g + 4t + r = PV slot 8g + e with e = 4t + r. P packs straight into the
//   B-fragment, no shuffle and no LDS trip.
//
// K/V staging (per wave, 32 keys)
//   Global loads are whole rows: D/8 adjacent lanes read one key's 16-B
//   pieces (bf16; 8-B pieces of e4m3 bytes with fp8 KV), a wave instruction
//   covers 4 (D=128) or 8 (D=64) complete rows, and a lane's D/16 loads hold
//   the SAME d-piece of D/16 consecutive keys. The next tile's loads are
//   issued before the current tile's MFMAs and land in LDS afterwards.
//   K: row-major [32][D + 8] bf16 (padded row = conflict-free b128 fragment
//      reads), rows permuted as above.
//   V: the lane's 8 x (D/16) register block is transposed IN REGISTERS and
//      written as V^T rows d with D/16 keys contiguous (one ds_write_b128 or
//      _b64 per d) -- no 2-byte scatter. V^T lives in 16-B units
//      u(d, s) = 4d + (d >> 3) + (s ^ ((d >> 1) & 3)): the pad unit every 8
//      rows spreads the writes (rows 8c + e over lanes c), the xor spreads
//      the fragment reads (rows 16dt + i over lanes i) over all 8 bank
//      groups.
//   fp8 KV dequantises at that point with v_cvt_scalef32_pk_bf16_fp8, the
//   per-token scale folded into the conversion.
//   LDS per wave: K 32*(D+8)*2 + V^T (4D + D/8)*16 bytes = 17152 (D=128) or
//   8832 (D=64); per workgroup 68608 / 35328. The wave merge reuses the
//   space lane-indexed (2 waves x registers x 64 lanes); only NT=4, D=128
//   needs more for it (69632). Two workgroups fit a CU's 160 KB.
//
// Masking
//   A tile wholly below the first row's position, inside the split and
//   above the last row's window start runs unmasked; only the tiles at the
//   two ends of the key range pay the per-element compares. Keys past the
//   split end load a clamped (valid) address and are masked; nothing at or
//   past kv_len or below lo is ever read, block-table entries included.
//
// Instantiations: D in {64, 128} x NT in {1, 2, 4} x {bf16, fp8} KV x
// {full, window}. Registers and occupancy of the D=128 ones are recorded
// in profiles/verify_attn_bench.txt.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

#define MFMA_16x16x32(A, B, C) \
  __builtin_amdgcn_mfma_f32_16x16x32_bf16((A), (B), (C), 0, 0, 0)

constexpr int VW = 4;    // waves per workgroup
constexpr int VTK = 32;  // keys per wave tile (the K extent of the PV MFMA)

__device__ __forceinline__ unsigned int pack_bf16x2(float lo, float hi) {
  __hip_bfloat16 a = __float2bfloat16(lo), b = __float2bfloat16(hi);
  return (unsigned int)*reinterpret_cast<unsigned short*>(&a) |
         ((unsigned int)*reinterpret_cast<unsigned short*>(&b) << 16);
}

// 8 e4m3 bytes -> 8 bf16, scale folded into the packed conversion
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16(uint32x2 w, float sc) {
  union { bf16x2_t p[4]; bf16x8_t v; } o;
  o.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w[0], sc, false);
  o.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w[0], sc, true);
  o.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w[1], sc, false);
  o.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)w[1], sc, true);
  return o.v;
}

// LDS traffic between the lanes of ONE wave: DS instructions of a wave
// execute in issue order, so draining the wave's own LDS counter and
// pinning the compiler's order is all the synchronisation needed
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

template <int D, int NT>
struct VerifyLds {
  static constexpr int KSTRIDE = D + 8;                 // bf16 per K row
  static constexpr int K_BYTES = VTK * KSTRIDE * 2;
  static constexpr int VT_UNITS = 4 * D + D / 8;        // 16-B units
  static constexpr int WAVE_BYTES = K_BYTES + VT_UNITS * 16;
  static constexpr int NREG = NT * (D / 16) * 4 + 2 * NT;  // merged f32/lane
  static constexpr int MERGE_BYTES = 2 * NREG * 64 * 4;
  static constexpr int BYTES =
      VW * WAVE_BYTES > MERGE_BYTES ? VW * WAVE_BYTES : MERGE_BYTES;
};

template <int D, int NT, bool FP8KV, bool WINDOW>
__global__ __launch_bounds__(VW * 64, NT <= 2 ? 2 : 1) void
attn_verify_kernel(
    const __hip_bfloat16* __restrict__ q,   // [B, Sq, H, D], heads dense
    const void* __restrict__ k_cache,       // [NB, Hkv, BS, D] bf16 | e4m3
    const void* __restrict__ v_cache,
    const float* __restrict__ k_scale,      // [NB, Hkv, BS] (FP8KV)
    const float* __restrict__ v_scale,
    const int* __restrict__ block_table,    // [B, max_blocks]
    const int* __restrict__ kv_lens,        // [B]
    const int* __restrict__ q_lens,         // [B]
    __hip_bfloat16* __restrict__ out,       // [B, Sq, H, D]
    float* __restrict__ partial_o,          // [B, Sq, H, splits, D]
    float* __restrict__ partial_ml,         // [B, Sq, H, splits, 2]
    int splits, long q_bstride, long q_sstride, int Sq, int H, int Hkv,
    int GQ, int block_size, int max_blocks, float scale, int window) {
  using L = VerifyLds<D, NT>;
  constexpr int CPR = D / 8;    // lanes per key row (16-B bf16 pieces)
  constexpr int KPL = D / 16;   // keys (= loads) per lane per tile
  constexpr int KSTRIDE = L::KSTRIDE;
  __shared__ __attribute__((aligned(16))) unsigned char smem[L::BYTES];

  const float scale2 = scale * 1.4426950408889634f;  // exp2 domain
  const int b = blockIdx.x;
  const int hkv = blockIdx.y;
  const int split = blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 15;   // query row within a row tile
  const int g = lane >> 4;     // lane group

  const int kv_len = min(kv_lens[b], max_blocks * block_size);
  const int q_len = min(min(q_lens[b], Sq), kv_len);
  if (q_len <= 0) return;      // nothing to read, nothing to write
  const int rows = GQ * q_len;               // real rows of this sequence
  const int pos0 = kv_len - q_len;           // position of row 0
  const int lo = WINDOW ? max(0, pos0 - window + 1) : 0;
  const int chunk =
      ((kv_len - lo + splits - 1) / splits + VTK - 1) & ~(VTK - 1);
  const int key_lo = lo + split * chunk;
  const int n_end = min(kv_len, key_lo + chunk);

  // per row tile: token j, query head, validity
  int rj[NT], rh[NT];
  bool rvalid[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int ridx = n * 16 + col;
    rvalid[n] = ridx < rows;
    rj[n] = ridx / GQ;
    rh[n] = hkv * GQ + ridx % GQ;
  }

  if (key_lo >= kv_len) {
    // empty split (never split 0): neutral partial, combine skips it
    if (tid < rows) {
      const int j = tid / GQ, h = hkv * GQ + tid % GQ;
      float* ml = partial_ml +
                  ((((long)b * Sq + j) * H + h) * splits + split) * 2;
      ml[0] = -INFINITY;
      ml[1] = 0.f;
    }
    return;
  }

  // Q fragments: B[k = d][j = row], 8 d-contiguous bf16 of one query row
  bf16x8_t q_frag[NT][D / 32];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
#pragma unroll
    for (int kc = 0; kc < D / 32; ++kc) {
      if (rvalid[n]) {
        q_frag[n][kc] = *reinterpret_cast<const bf16x8_t*>(
            q + (long)b * q_bstride + (long)rj[n] * q_sstride +
            (long)rh[n] * D + kc * 32 + g * 8);
      } else {
        q_frag[n][kc] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  }

  float m_run[NT], l_run[NT];
  f32x4_t acc_o[NT][D / 16];  // O^T: d = 16dt + 4g + r, row = col
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    m_run[n] = -INFINITY;
    l_run[n] = 0.f;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
      acc_o[n][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // ---- staging geometry: lane = (key group sg, d-piece sc) ---- //
  const int sc = lane % CPR;
  const int sg = lane / CPR;
  short* lds_k = reinterpret_cast<short*>(smem + wave * L::WAVE_BYTES);
  unsigned char* lds_vt = smem + wave * L::WAVE_BYTES + L::K_BYTES;
  const int* btab = block_table + (long)b * max_blocks;
  const long hk_off = (long)hkv * block_size * D;

  uint32x4 kraw[FP8KV ? 1 : KPL], vraw[FP8KV ? 1 : KPL];
  uint32x2 kraw8[FP8KV ? KPL : 1], vraw8[FP8KV ? KPL : 1];
  float ksc[FP8KV ? KPL : 1], vsc[FP8KV ? KPL : 1];

  auto stage_load = [&](int n0) {
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      // keys past the split end read the split's last key (masked later)
      const int key = min(n0 + KPL * sg + i, n_end - 1);
      const long blk = btab[key / block_size];
      const int in_blk = key % block_size;
      const long base = blk * Hkv * block_size * D + hk_off +
                        (long)in_blk * D + sc * 8;
      if constexpr (FP8KV) {
        kraw8[i] = *reinterpret_cast<const uint32x2*>(
            (const unsigned char*)k_cache + base);
        vraw8[i] = *reinterpret_cast<const uint32x2*>(
            (const unsigned char*)v_cache + base);
        const long sidx = (blk * Hkv + hkv) * block_size + in_blk;
        ksc[i] = k_scale[sidx];
        vsc[i] = v_scale[sidx];
      } else {
        kraw[i] = *reinterpret_cast<const uint32x4*>(
            (const __hip_bfloat16*)k_cache + base);
        vraw[i] = *reinterpret_cast<const uint32x4*>(
            (const __hip_bfloat16*)v_cache + base);
      }
    }
  };

  auto stage_write = [&]() {
    bf16x8_t vreg[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      bf16x8_t kreg;
      if constexpr (FP8KV) {
        kreg = fp8x8_to_bf16(kraw8[i], ksc[i]);
        vreg[i] = fp8x8_to_bf16(vraw8[i], vsc[i]);
      } else {
        kreg = *reinterpret_cast<const bf16x8_t*>(&kraw[i]);
        vreg[i] = *reinterpret_cast<const bf16x8_t*>(&vraw[i]);
      }
      // tile key kk = 8a + 4t + c -> LDS row 16t + 4a + c
      const int kk = KPL * sg + i;
      const int row = 16 * ((kk >> 2) & 1) + 4 * (kk >> 3) + (kk & 3);
      *reinterpret_cast<bf16x8_t*>(&lds_k[row * KSTRIDE + sc * 8]) = kreg;
    }
    // V^T: row d = 8 sc + e holds this lane's KPL keys contiguously
    const int byte_in_row = KPL * sg * 2;          // key offset in bytes
    const int s = byte_in_row >> 4, half = byte_in_row & 15;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = sc * 8 + e;
      const int u = 4 * d + (d >> 3) + (s ^ ((d >> 1) & 3));
      unsigned char* dst = lds_vt + u * 16 + half;
      if constexpr (KPL == 8) {
        bf16x8_t t;
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = vreg[i][e];
        *reinterpret_cast<bf16x8_t*>(dst) = t;
      } else {
        bf16x4_t t;
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = vreg[i][e];
        *reinterpret_cast<bf16x4_t*>(dst) = t;
      }
    }
  };

  auto compute = [&](int n0) {
    // S^T[key][row] for 2 key tiles x NT row tiles
    f32x4_t acc_s[2][NT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc_s[t][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < D / 32; ++kc) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(
            &lds_k[(t * 16 + col) * KSTRIDE + kc * 32 + g * 8]);
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc_s[t][n] = MFMA_16x16x32(kf, q_frag[n][kc], acc_s[t][n]);
      }
    }

    // interior tile: inside the split, at or below the FIRST row's position
    // and above the LAST row's window start -> no per-element masking
    const bool tile_full =
        (n0 + VTK <= n_end) && (n0 + VTK - 1 <= pos0) &&
        (!WINDOW || (n0 > pos0 + q_len - 1 - window));
    bf16x8_t pf[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      float pv[2][4];
      float rmax = -INFINITY;
      if (tile_full) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pv[t][r] = acc_s[t][n][r] * scale2;
            rmax = fmaxf(rmax, pv[t][r]);
          }
      } else {
        const int pos = pos0 + rj[n];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = n0 + 8 * g + 4 * t + r;
            bool valid = key < n_end && key <= pos;
            if (WINDOW) valid = valid && (key > pos - window);
            pv[t][r] = valid ? acc_s[t][n][r] * scale2 : -INFINITY;
            rmax = fmaxf(rmax, pv[t][r]);
          }
      }
      rmax = fmaxf(rmax, __shfl_xor(rmax, 16, 64));
      rmax = fmaxf(rmax, __shfl_xor(rmax, 32, 64));
      const float m_new = fmaxf(m_run[n], rmax);
      // a row with nothing visible yet keeps m = -inf; both guards keep
      // exp2(-inf - -inf) out of the state
      const float alpha = (m_run[n] == -INFINITY)
                              ? 0.f
                              : __builtin_amdgcn_exp2f(m_run[n] - m_new);
      float rsum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = (pv[t][r] == -INFINITY || m_new == -INFINITY)
                              ? 0.f
                              : __builtin_amdgcn_exp2f(pv[t][r] - m_new);
          pv[t][r] = p;
          rsum += p;
        }
      rsum += __shfl_xor(rsum, 16, 64);
      rsum += __shfl_xor(rsum, 32, 64);
      l_run[n] = l_run[n] * alpha + rsum;
      m_run[n] = m_new;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc_o[n][dt][r] *= alpha;
      // P^T B-fragment: slot 8g + e, e = 4t + r -- already in this lane
      union { unsigned int u[4]; bf16x8_t v; } pk;
      pk.u[0] = pack_bf16x2(pv[0][0], pv[0][1]);
      pk.u[1] = pack_bf16x2(pv[0][2], pv[0][3]);
      pk.u[2] = pack_bf16x2(pv[1][0], pv[1][1]);
      pk.u[3] = pack_bf16x2(pv[1][2], pv[1][3]);
      pf[n] = pk.v;
    }

    // O^T += V^T P^T: A[i = d][k = slot], 8 key-contiguous bf16 per lane
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      const int d = dt * 16 + col;
      const int u = 4 * d + (d >> 3) + (g ^ ((d >> 1) & 3));
      const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(lds_vt + u * 16);
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc_o[n][dt] = MFMA_16x16x32(vf, pf[n], acc_o[n][dt]);
    }
  };

  // ---- key loop: this wave's tiles, round-robin over the 4 waves ---- //
  int n0 = key_lo + wave * VTK;
  if (n0 < n_end) stage_load(n0);
  for (; n0 < n_end; n0 += VW * VTK) {
    stage_write();
    wave_lds_sync();
    // next tile's global loads fly under this tile's MFMA + softmax
    if (n0 + VW * VTK < n_end) stage_load(n0 + VW * VTK);
    compute(n0);
    wave_lds_sync();
  }

  // ---- merge the 4 waves: (2,3) -> (0,1), then 1 -> 0 ---- //
  // lane-indexed exchange: every wave holds the same (row, d) per lane
  float* xch = reinterpret_cast<float*>(smem);
  auto publish = [&](int slot) {
    float* dst = xch + (long)slot * L::NREG * 64 + lane;
    int k = 0;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      dst[64 * k++] = m_run[n];
      dst[64 * k++] = l_run[n];
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[64 * k++] = acc_o[n][dt][r];
    }
  };
  auto absorb = [&](int slot) {
    const float* src = xch + (long)slot * L::NREG * 64 + lane;
    int k = 0;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const float m2 = src[64 * k++];
      const float l2 = src[64 * k++];
      const float m = fmaxf(m_run[n], m2);
      const float f1 = (m_run[n] == -INFINITY)
                           ? 0.f
                           : __builtin_amdgcn_exp2f(m_run[n] - m);
      const float f2 =
          (m2 == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m2 - m);
      l_run[n] = l_run[n] * f1 + l2 * f2;
      m_run[n] = m;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc_o[n][dt][r] = acc_o[n][dt][r] * f1 + src[64 * k++] * f2;
    }
  };
  __syncthreads();  // every wave is done with its staging slice
  if (wave >= 2) publish(wave - 2);
  __syncthreads();
  if (wave < 2) absorb(wave);
  __syncthreads();
  if (wave == 1) publish(0);
  __syncthreads();
  if (wave != 0) return;
  absorb(0);

  // ---- epilogue (wave 0): 4 d-contiguous values per (row tile, dt) ---- //
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    if (!rvalid[n]) continue;
    const long row = ((long)b * Sq + rj[n]) * H + rh[n];
    if (splits == 1) {
      const float inv_l = l_run[n] > 0.f ? 1.0f / l_run[n] : 0.f;
      __hip_bfloat16* dst = out + row * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        uint32x2 pk;
        pk[0] = pack_bf16x2(acc_o[n][dt][0] * inv_l, acc_o[n][dt][1] * inv_l);
        pk[1] = pack_bf16x2(acc_o[n][dt][2] * inv_l, acc_o[n][dt][3] * inv_l);
        *reinterpret_cast<uint32x2*>(dst + dt * 16) = pk;
      }
    } else {
      float* po = partial_o + (row * splits + split) * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
        *reinterpret_cast<f32x4_t*>(po + dt * 16) = acc_o[n][dt];
      if (g == 0) {
        float* ml = partial_ml + (row * splits + split) * 2;
        ml[0] = m_run[n];
        ml[1] = l_run[n];
      }
    }
  }
}

// fold the per-split partials of one (sequence, token, head) row: grid
// (B * Sq, H), one wave per block; rows at or past q_lens[b] are skipped
template <int D>
__global__ void attn_verify_combine_kernel(
    const float* __restrict__ partial_o,   // [B, Sq, H, splits, D]
    const float* __restrict__ partial_ml,  // [B, Sq, H, splits, 2]
    const int* __restrict__ kv_lens, const int* __restrict__ q_lens,
    __hip_bfloat16* __restrict__ out,      // [B, Sq, H, D]
    int splits, int Sq, int H) {
  const int bj = blockIdx.x;
  const int h = blockIdx.y;
  const int b = bj / Sq, j = bj % Sq;
  if (j >= min(q_lens[b], kv_lens[b])) return;
  const long base = ((long)bj * H + h) * splits;
  float m_tot = -INFINITY;
  for (int s = 0; s < splits; ++s)
    m_tot = fmaxf(m_tot, partial_ml[(base + s) * 2]);
  float l_tot = 0.f;
  float acc[D / 64];
#pragma unroll
  for (int i = 0; i < D / 64; ++i) acc[i] = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float m = partial_ml[(base + s) * 2];
    if (m == -INFINITY) continue;
    const float f = __builtin_amdgcn_exp2f(m - m_tot);  // exp2 domain
    l_tot += partial_ml[(base + s) * 2 + 1] * f;
    const float* po = partial_o + (base + s) * D;
#pragma unroll
    for (int i = 0; i < D / 64; ++i) acc[i] += po[i * 64 + threadIdx.x] * f;
  }
  const float inv_l = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  __hip_bfloat16* dst = out + ((long)bj * H + h) * D;
#pragma unroll
  for (int i = 0; i < D / 64; ++i)
    dst[i * 64 + threadIdx.x] = __float2bfloat16(acc[i] * inv_l);
}

}  // namespace

#ifndef CMLS_KERNEL_ONLY
torch::Tensor attention_decode_multi(
    torch::Tensor q,            // [B, Sq, H, D] bf16, 1 <= Sq <= 8
    torch::Tensor k_cache,      // [NB, Hkv, BS, D] bf16, or e4m3 bytes
    torch::Tensor v_cache,
    torch::Tensor block_table,  // int32 [B, max_blocks]
    torch::Tensor kv_lens,      // int32 [B] total keys, query tokens included
    torch::Tensor q_lens,       // int32 [B] valid query rows per sequence
    double scale, c10::optional<torch::Tensor> k_scale,
    c10::optional<torch::Tensor> v_scale, int64_t window) {
  TORCH_CHECK(q.dim() == 4 && q.scalar_type() == at::kBFloat16,
              "q must be [B, Sq, H, D] bf16");
  TORCH_CHECK(q.stride(3) == 1 && q.stride(2) == q.size(3),
              "q heads must be dense");
  TORCH_CHECK(q.stride(0) % 8 == 0 && q.stride(1) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "q rows must be 16-byte aligned");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.is_contiguous() &&
              v_cache.is_contiguous());
  TORCH_CHECK(window >= 0, "window must be >= 0");
  const bool fp8kv = k_cache.scalar_type() == at::kByte ||
                     k_cache.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(fp8kv || k_cache.scalar_type() == at::kBFloat16,
              "kv cache must be bf16 or e4m3 bytes");
  const float* ksp = nullptr;
  const float* vsp = nullptr;
  if (fp8kv) {
    TORCH_CHECK(k_scale.has_value() && v_scale.has_value(),
                "fp8 KV cache needs k_scale/v_scale");
    TORCH_CHECK(k_scale->scalar_type() == at::kFloat &&
                k_scale->is_contiguous() && v_scale->is_contiguous());
    ksp = k_scale->data_ptr<float>();
    vsp = v_scale->data_ptr<float>();
  }
  const int B = q.size(0), Sq = q.size(1), H = q.size(2), D = q.size(3);
  const int Hkv = k_cache.size(1), BS = k_cache.size(2);
  const int max_blocks = block_table.size(1);
  TORCH_CHECK(D == 64 || D == 128, "head_dim must be 64 or 128");
  TORCH_CHECK(k_cache.size(3) == D && Hkv >= 1 && H % Hkv == 0);
  const int GQ = H / Hkv;
  TORCH_CHECK(Sq >= 1 && Sq <= 8, "1..8 query tokens per sequence, got ", Sq);
  TORCH_CHECK(GQ >= 1 && GQ <= 8, "GQA group must be 1..8, got ", GQ);
  TORCH_CHECK(BS % 16 == 0, "page size must be a multiple of 16");
  TORCH_CHECK(block_table.dim() == 2 && block_table.size(0) == B &&
              kv_lens.numel() == B && q_lens.numel() == B);
  auto bt = block_table.to(q.device(), at::kInt).contiguous();
  auto kl = kv_lens.to(q.device(), at::kInt).contiguous();
  auto ql = q_lens.to(q.device(), at::kInt).contiguous();
  auto out = torch::empty({B, Sq, H, D}, q.options());
  if (B == 0) return out;
  // a window no sequence of this table can outgrow is the windowless kernel
  const bool win = window > 0 && window < (int64_t)max_blocks * BS;
  const int W = win ? (int)window : 0;
  hipStream_t stream_ = cmls::current_stream();

  // split count: the decode kernel's fill heuristic (~4 workgroups per CU)
  int splits = 1;
  const long base_wg = (long)B * Hkv;
  if (base_wg < 1024)
    splits = (int)std::min<long>((1024 + base_wg - 1) / base_wg, 16);
  torch::Tensor partial_o, partial_ml;
  float* po = nullptr;
  float* pml = nullptr;
  if (splits > 1) {
    auto opts = q.options().dtype(at::kFloat);
    partial_o = torch::empty({B, Sq, H, splits, D}, opts);
    partial_ml = torch::empty({B, Sq, H, splits, 2}, opts);
    po = partial_o.data_ptr<float>();
    pml = partial_ml.data_ptr<float>();
  }
  dim3 grid(B, Hkv, splits);

#define LAUNCH_VER(DD, NN, F8, WW)                                           \
  hipLaunchKernelGGL((attn_verify_kernel<DD, NN, F8, WW>), grid,             \
                     dim3(VW * 64), 0, stream_,                              \
                     (const __hip_bfloat16*)q.data_ptr(),                    \
                     (const void*)k_cache.data_ptr(),                        \
                     (const void*)v_cache.data_ptr(), ksp, vsp,              \
                     bt.data_ptr<int>(), kl.data_ptr<int>(),                 \
                     ql.data_ptr<int>(), (__hip_bfloat16*)out.data_ptr(),    \
                     po, pml, splits, (long)q.stride(0), (long)q.stride(1),  \
                     Sq, H, Hkv, GQ, BS, max_blocks, (float)scale, W)
#define LAUNCH_VER_F(DD, NN)                                                 \
  do { if (win) { if (fp8kv) LAUNCH_VER(DD, NN, true, true);                 \
                  else LAUNCH_VER(DD, NN, false, true); }                    \
       else { if (fp8kv) LAUNCH_VER(DD, NN, true, false);                    \
              else LAUNCH_VER(DD, NN, false, false); } } while (0)
  // row tiles by R = GQ * Sq: 16, 32 or 64 padded rows
  const int R = GQ * Sq;
  if (D == 128) {
    if (R <= 16) LAUNCH_VER_F(128, 1);
    else if (R <= 32) LAUNCH_VER_F(128, 2);
    else LAUNCH_VER_F(128, 4);
  } else {
    if (R <= 16) LAUNCH_VER_F(64, 1);
    else if (R <= 32) LAUNCH_VER_F(64, 2);
    else LAUNCH_VER_F(64, 4);
  }
#undef LAUNCH_VER_F
#undef LAUNCH_VER
  if (splits > 1) {
    dim3 cgrid(B * Sq, H);
    if (D == 128) {
      hipLaunchKernelGGL(attn_verify_combine_kernel<128>, cgrid, dim3(64), 0,
                         stream_, po, pml, kl.data_ptr<int>(),
                         ql.data_ptr<int>(), (__hip_bfloat16*)out.data_ptr(),
                         splits, Sq, H);
    } else {
      hipLaunchKernelGGL(attn_verify_combine_kernel<64>, cgrid, dim3(64), 0,
                         stream_, po, pml, kl.data_ptr<int>(),
                         ql.data_ptr<int>(), (__hip_bfloat16*)out.data_ptr(),
                         splits, Sq, H);
    }
  }
  return out;
}
#endif  // CMLS_KERNEL_ONLY
