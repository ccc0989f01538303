// Shared by the MXFP4 GEMM kernels (mxfp4_path.hip, mxfp4_gemm.hip): the
// constants of the ops.tile_mxfp4_weight layout (layout comment in
// mxfp4_path.hip) and the host-side check that a pair of buffers is that
// tiling of an [N, K] weight.
#pragma once

#include "common.h"

constexpr int MX_NT = 16;      // N columns per weight tile (one MFMA)
constexpr int MX_KSTEP = 128;  // k per MFMA
constexpr int MX_QUAD = 4;     // k-steps per packed scale dword
constexpr int MX_SCALE_ONE = 0x7f7f7f7f;  // e8m0 2^0 in every byte

#ifndef CMLS_KERNEL_ONLY
inline void check_mx_tiles(const torch::Tensor& w4t, const torch::Tensor& e8t,
                           const torch::Tensor& w_scale, int N, int K,
                           const char* op) {
  TORCH_CHECK(w4t.scalar_type() == at::kByte && e8t.scalar_type() == at::kByte,
              op, ": tiled weights and scales are uint8");
  TORCH_CHECK(w4t.is_contiguous() && e8t.is_contiguous() &&
              w_scale.is_contiguous());
  TORCH_CHECK(w_scale.scalar_type() == at::kFloat && w_scale.numel() == N,
              op, ": w_scale is fp32 [N]");
  const long nbs = (N + MX_NT - 1) / MX_NT;
  const long nsteps = (K + MX_KSTEP - 1) / MX_KSTEP;
  const long nquads = (nsteps + MX_QUAD - 1) / MX_QUAD;
  TORCH_CHECK(w4t.numel() == nbs * nsteps * 64 * 16, op,
              ": w4t is not the tiling of [", N, ", ", K, "]");
  TORCH_CHECK(e8t.numel() == nbs * nquads * 64 * 4, op,
              ": e8t is not the tiling of [", N, ", ", K, "]");
  TORCH_CHECK((uintptr_t)w4t.data_ptr() % 16 == 0 &&
              (uintptr_t)e8t.data_ptr() % 4 == 0, op, ": misaligned tiles");
}
#endif  // CMLS_KERNEL_ONLY
