// Fused per-head RMSNorm (optional) + scaled RoPE + paged KV-cache write.
// One launch covers the stretch between the QKV projection and attention
// for the models that need a frequency table (Llama-3.1/3.2 rope_scaling,
// YaRN, linear) or a q/k norm (Qwen3):
//
//   q [T, Hq, D], k [T, Hkv, D], v [T, Hkv, D]  token-strided views of the
//   merged QKV output; positions i32 [T]; inv_freq f32 [D/2].
//
//   per (token, q head):  x = row (fp32) -> x * rsqrt(mean(x^2)+eps) * w
//                         -> rotate NeoX pairs (i, i + D/2) by
//                            float(pos) * inv_freq[i], cos/sin * attn_factor
//                         -> one rounding to the model dtype, in place
//   per (token, kv head): the same for k; the rounded row also goes to its
//                         slot of the paged cache [NB, Hkv, BS, D], the v row
//                         is copied bit for bit. fp8 caches quantise the
//                         ROUNDED rows by kv_cache_write_fp8_kernel's rule
//                         (attention_decode.hip), so the cache holds what
//                         rope + kv_cache_write would have stored.
//
// Work split: D/8 lanes own one head row (16 lanes at D=128, 8 at D=64).
// A lane holds 4 low elements and the 4 high elements they pair with, so a
// rotation never leaves the lane, every access is 8 bytes, and the row stays
// in registers from its load to its last store. Sum-of-squares and absmax
// reduce over the D/8-lane group by shfl_xor. Rows are numbered
// token-major over the Hq + Hkv heads and dealt to groups across the whole
// grid: T = 1 still spreads over several workgroups and large T leaves no
// lane idle. Control flow around the shuffles is uniform: lanes without a row
// (the tail of the last block) carry zeros and skip only the memory accesses.
#include "common.h"

namespace {

// The kernel carries target("no-packed-fp32-ops"), the choice moe_fp8.hip
// and sample_rows.hip make: the 4-wide rotation would otherwise pair into
// packed fp32 VALU ops; plain v_mul / v_fma only. The helpers are
// force-inlined, so the kernel's attribute covers them.
#ifdef __HIP_DEVICE_COMPILE__
#define QRK_PLAIN_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define QRK_PLAIN_FP32
#endif

constexpr int kThreads = 128;

struct QkRopeKvParams {
  void* q;
  void* k;
  const void* v;
  const int* positions;
  const float* inv_freq;
  const void* q_norm_w;
  const void* k_norm_w;
  void* k_cache;
  void* v_cache;
  float* k_scale;
  float* v_scale;
  const int* slots;
  long q_tstride, k_tstride, v_tstride;  // elements
  long rows;                             // tokens * (hq + hkv)
  int hq, hkv, block_size;
  float attn_factor, eps;
};

template <typename T>
__device__ __forceinline__ float elem_f32(unsigned int bits16) {
  return to_f32(__builtin_bit_cast(T, (unsigned short)bits16));
}

template <typename T>
__device__ __forceinline__ unsigned int f32_elem(float v) {
  return __builtin_bit_cast(unsigned short, from_f32<T>(v));
}

// 4 elements (8 bytes) <-> 4 floats
template <typename T>
__device__ __forceinline__ void unpack4(uint32x2 u, float* x) {
  x[0] = elem_f32<T>(u.x & 0xffffu);
  x[1] = elem_f32<T>(u.x >> 16);
  x[2] = elem_f32<T>(u.y & 0xffffu);
  x[3] = elem_f32<T>(u.y >> 16);
}

template <typename T>
__device__ __forceinline__ uint32x2 pack4(const float* x) {
  uint32x2 u;
  u.x = f32_elem<T>(x[0]) | (f32_elem<T>(x[1]) << 16);
  u.y = f32_elem<T>(x[2]) | (f32_elem<T>(x[3]) << 16);
  return u;
}

template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1)
    v += __shfl_xor(v, off, WAVE_SIZE);
  return v;
}

template <int LANES>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, WAVE_SIZE));
  return v;
}

__device__ __forceinline__ float absmax8(const float* x) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(x[j]));
  return m;
}

// 4 floats * inv -> 4 e4m3 bytes in one dword
__device__ __forceinline__ unsigned int quant4_e4m3(const float* x,
                                                    float inv) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, w, true);
  return (unsigned int)w;
}

// KV: 0 = no cache, 1 = cache in the model dtype, 2 = e4m3 cache + scales
template <typename T, int D, bool NORM, int KV>
__global__ __launch_bounds__(kThreads) QRK_PLAIN_FP32 void qk_rope_kv_kernel(
    const QkRopeKvParams p) {
  constexpr int LANES = D / 8;  // lanes per head row
  constexpr int HALF = D / 2;
  const int sub = threadIdx.x % LANES;
  const int i0 = 4 * sub;  // this lane's low elements; high ones at + HALF
  const long row =
      (long)blockIdx.x * (kThreads / LANES) + threadIdx.x / LANES;
  const bool valid = row < p.rows;
  const int htot = p.hq + p.hkv;
  const long t = valid ? row / htot : 0;
  const int h = valid ? (int)(row % htot) : 0;
  const bool is_k = h >= p.hq;
  const int hk = h - p.hq;  // kv head, meaningful when is_k
  T* base = is_k ? (T*)p.k + t * p.k_tstride + (long)hk * D
                 : (T*)p.q + t * p.q_tstride + (long)h * D;

  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (valid) {
    unpack4<T>(*(const uint32x2*)(base + i0), x);
    unpack4<T>(*(const uint32x2*)(base + HALF + i0), x + 4);
  }

  if constexpr (NORM) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
    ss = group_sum<LANES>(ss);
    const float r = rsqrtf(ss * (1.0f / D) + p.eps);
    const T* wrow = (const T*)(is_k ? p.k_norm_w : p.q_norm_w);
    float w[8];
    unpack4<T>(*(const uint32x2*)(wrow + i0), w);
    unpack4<T>(*(const uint32x2*)(wrow + HALF + i0), w + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = x[j] * r * w[j];
  }

  // rotation: the angle is ONE fp32 product; sincosf stays the precise form
  // (the fast one loses range reduction at large positions, see rope.hip)
  const float pos = (float)p.positions[t];
  const floatx4 f = *(const floatx4*)(p.inv_freq + i0);
  float y[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float s, c;
    sincosf(pos * f[j], &s, &c);
    s *= p.attn_factor;
    c *= p.attn_factor;
    y[j] = x[j] * c - x[j + 4] * s;
    y[j + 4] = x[j + 4] * c + x[j] * s;
  }
  const uint32x2 lo = pack4<T>(y), hi = pack4<T>(y + 4);
  if (valid) {
    *(uint32x2*)(base + i0) = lo;
    *(uint32x2*)(base + HALF + i0) = hi;
  }

  if constexpr (KV != 0) {
    int slot = -1;
    if (valid && is_k) slot = p.slots[t];
    const bool wr = slot >= 0;
    uint32x2 vlo = {0u, 0u}, vhi = {0u, 0u};
    long dst = 0;  // element offset of the row in [NB, Hkv, BS, D]
    long sidx = 0;
    if (wr) {
      const T* vrow = (const T*)p.v + t * p.v_tstride + (long)hk * D;
      vlo = *(const uint32x2*)(vrow + i0);
      vhi = *(const uint32x2*)(vrow + HALF + i0);
      const long blk = slot / p.block_size;
      const int off = slot % p.block_size;
      sidx = (blk * p.hkv + hk) * p.block_size + off;
      dst = sidx * D;
    }
    if constexpr (KV == 1) {
      if (wr) {
        T* kc = (T*)p.k_cache + dst;
        T* vc = (T*)p.v_cache + dst;
        *(uint32x2*)(kc + i0) = lo;
        *(uint32x2*)(kc + HALF + i0) = hi;
        *(uint32x2*)(vc + i0) = vlo;
        *(uint32x2*)(vc + HALF + i0) = vhi;
      }
    } else {
      // quantise what was stored: the rounded k row and the v row as is
      float kr[8], vr[8];
      unpack4<T>(lo, kr);
      unpack4<T>(hi, kr + 4);
      unpack4<T>(vlo, vr);
      unpack4<T>(vhi, vr + 4);
      const float kamax = group_max<LANES>(absmax8(kr));
      const float vamax = group_max<LANES>(absmax8(vr));
      // power-of-two scales, as in kv_cache_write_fp8_kernel
      const float kscale = exp2f(ceilf(log2f(fmaxf(kamax, 1e-8f) / 448.0f)));
      const float vscale = exp2f(ceilf(log2f(fmaxf(vamax, 1e-8f) / 448.0f)));
      const float kinv = 1.0f / kscale, vinv = 1.0f / vscale;
      if (wr) {
        unsigned char* kc = (unsigned char*)p.k_cache + dst;
        unsigned char* vc = (unsigned char*)p.v_cache + dst;
        *(unsigned int*)(kc + i0) = quant4_e4m3(kr, kinv);
        *(unsigned int*)(kc + HALF + i0) = quant4_e4m3(kr + 4, kinv);
        *(unsigned int*)(vc + i0) = quant4_e4m3(vr, vinv);
        *(unsigned int*)(vc + HALF + i0) = quant4_e4m3(vr + 4, vinv);
        if (sub == 0) {
          p.k_scale[sidx] = kscale;
          p.v_scale[sidx] = vscale;
        }
      }
    }
  }
}

template <typename T, int D, bool NORM>
void launch_kv(const QkRopeKvParams& p, int kv, hipStream_t stream) {
  const long rows_per_block = kThreads / (D / 8);
  const dim3 grid((unsigned)((p.rows + rows_per_block - 1) / rows_per_block));
  if (kv == 0) {
    hipLaunchKernelGGL((qk_rope_kv_kernel<T, D, NORM, 0>), grid,
                       dim3(kThreads), 0, stream, p);
  } else if (kv == 1) {
    hipLaunchKernelGGL((qk_rope_kv_kernel<T, D, NORM, 1>), grid,
                       dim3(kThreads), 0, stream, p);
  } else {
    hipLaunchKernelGGL((qk_rope_kv_kernel<T, D, NORM, 2>), grid,
                       dim3(kThreads), 0, stream, p);
  }
}

template <typename T>
void launch(const QkRopeKvParams& p, int d, bool norm, int kv,
            hipStream_t stream) {
  if (d == 128) {
    if (norm) launch_kv<T, 128, true>(p, kv, stream);
    else launch_kv<T, 128, false>(p, kv, stream);
  } else {
    if (norm) launch_kv<T, 64, true>(p, kv, stream);
    else launch_kv<T, 64, false>(p, kv, stream);
  }
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

void check_rows(const torch::Tensor& x, const char* name, int64_t tokens,
                int64_t d, at::ScalarType st) {
  TORCH_CHECK(x.dim() == 3, name, " must be [T, H, D]");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == st, name,
              ": device tensor of the model dtype expected");
  TORCH_CHECK(x.size(0) == tokens && x.size(2) == d, name, ": shape mismatch");
  TORCH_CHECK(x.stride(2) == 1 && x.stride(1) == d, name,
              " heads must be dense");
  // the kernel moves 8 bytes per access and has no 2-byte variant: the
  // merged-QKV layout satisfies this, other layouts are rejected
  TORCH_CHECK(aligned16(x) && x.stride(0) % 4 == 0, name,
              " needs a 16-byte-aligned base and an 8-byte-aligned token "
              "stride");
}

}  // namespace

void qk_rope_kv(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                torch::Tensor positions, torch::Tensor inv_freq,
                double attn_factor, c10::optional<torch::Tensor> q_norm_w,
                c10::optional<torch::Tensor> k_norm_w, double eps,
                c10::optional<torch::Tensor> k_cache,
                c10::optional<torch::Tensor> v_cache,
                c10::optional<torch::Tensor> slot_mapping,
                c10::optional<torch::Tensor> k_scale,
                c10::optional<torch::Tensor> v_scale) {
  TORCH_CHECK(q.dim() == 3, "q must be [T, Hq, D]");
  const int64_t tokens = q.size(0), hq = q.size(1), d = q.size(2);
  const auto st = q.scalar_type();
  TORCH_CHECK(st == at::kBFloat16 || st == at::kHalf,
              "qk_rope_kv: bf16 or fp16 only, got ", st);
  TORCH_CHECK(d == 64 || d == 128, "qk_rope_kv: head_dim must be 64 or 128");
  check_rows(q, "q", tokens, d, st);
  check_rows(k, "k", tokens, d, st);
  check_rows(v, "v", tokens, d, st);
  const int64_t hkv = k.size(1);
  TORCH_CHECK(v.size(1) == hkv, "k and v head counts differ");
  TORCH_CHECK(positions.is_cuda() && positions.scalar_type() == at::kInt &&
                  positions.is_contiguous() && positions.numel() == tokens,
              "positions must be a contiguous int32 [T] device tensor");
  TORCH_CHECK(inv_freq.is_cuda() && inv_freq.scalar_type() == at::kFloat &&
                  inv_freq.is_contiguous() && inv_freq.dim() == 1 &&
                  inv_freq.size(0) == d / 2 && aligned16(inv_freq),
              "inv_freq must be a float32 [D/2] device tensor");

  QkRopeKvParams p = {};
  TORCH_CHECK(q_norm_w.has_value() == k_norm_w.has_value(),
              "q_norm_w and k_norm_w come together");
  const bool norm = q_norm_w.has_value();
  if (norm) {
    for (const torch::Tensor* w : {&*q_norm_w, &*k_norm_w}) {
      TORCH_CHECK(w->is_cuda() && w->scalar_type() == st && w->dim() == 1 &&
                      w->size(0) == d && w->is_contiguous() && aligned16(*w),
                  "norm weights must be [D] device tensors of the model "
                  "dtype");
    }
    p.q_norm_w = q_norm_w->data_ptr();
    p.k_norm_w = k_norm_w->data_ptr();
  }

  const bool cached = k_cache.has_value();
  TORCH_CHECK(v_cache.has_value() == cached &&
                  slot_mapping.has_value() == cached,
              "k_cache, v_cache and slot_mapping are all given or all absent");
  TORCH_CHECK(k_scale.has_value() == v_scale.has_value() &&
                  (cached || !k_scale.has_value()),
              "k_scale and v_scale come together, with the caches");
  int kv = 0;
  if (cached) {
    const auto ct = k_cache->scalar_type();
    const bool fp8 = ct == at::kByte || ct == at::kFloat8_e4m3fn;
    kv = fp8 ? 2 : 1;
    TORCH_CHECK(fp8 || ct == st, "cache dtype must be the model dtype or fp8");
    TORCH_CHECK(v_cache->scalar_type() == ct, "k/v cache dtypes differ");
    TORCH_CHECK(fp8 == k_scale.has_value(),
                "scales are given exactly for fp8 caches");
    TORCH_CHECK(k_cache->is_cuda() && k_cache->dim() == 4 &&
                    k_cache->size(1) == hkv && k_cache->size(3) == d &&
                    k_cache->is_contiguous() && v_cache->is_contiguous() &&
                    v_cache->sizes() == k_cache->sizes() &&
                    aligned16(*k_cache) && aligned16(*v_cache),
                "caches must be contiguous [NB, Hkv, BS, D]");
    TORCH_CHECK(slot_mapping->is_cuda() &&
                    slot_mapping->scalar_type() == at::kInt &&
                    slot_mapping->is_contiguous() &&
                    slot_mapping->numel() == tokens,
                "slot_mapping must be a contiguous int32 [T] device tensor");
    if (fp8) {
      for (const torch::Tensor* s : {&*k_scale, &*v_scale}) {
        TORCH_CHECK(s->is_cuda() && s->scalar_type() == at::kFloat &&
                        s->is_contiguous() &&
                        s->numel() == k_cache->numel() / d,
                    "scales must be contiguous float32 [NB, Hkv, BS]");
      }
      p.k_scale = k_scale->data_ptr<float>();
      p.v_scale = v_scale->data_ptr<float>();
    }
    p.k_cache = k_cache->data_ptr();
    p.v_cache = v_cache->data_ptr();
    p.slots = slot_mapping->data_ptr<int>();
    p.block_size = (int)k_cache->size(2);
  }
  if (tokens == 0) return;

  p.q = q.data_ptr();
  p.k = k.data_ptr();
  p.v = v.data_ptr();
  p.positions = positions.data_ptr<int>();
  p.inv_freq = inv_freq.data_ptr<float>();
  p.q_tstride = q.stride(0);
  p.k_tstride = k.stride(0);
  p.v_tstride = v.stride(0);
  p.rows = tokens * (hq + hkv);
  p.hq = (int)hq;
  p.hkv = (int)hkv;
  p.attn_factor = (float)attn_factor;
  p.eps = (float)eps;

  hipStream_t stream = cmls::current_stream();
  if (st == at::kBFloat16) {
    launch<__hip_bfloat16>(p, (int)d, norm, kv, stream);
  } else {
    launch<__half>(p, (int)d, norm, kv, stream);
  }
}
