// Stages of the mixture-of-experts path that do not depend on the expert
// weight format: moe.hip (bf16 experts) defines them, moe_fp8.hip (e4m3
// experts) launches the same align and combine around its own GEMMs.
#pragma once

#include "common.h"

namespace cmls_moe {

constexpr int MAX_E = 64;  // one lane per expert in moe_route
constexpr int MAX_K = 8;

// ids: contiguous int32 [T, k] on the GPU, 1 <= k <= MAX_K
void check_ids(const torch::Tensor& ids, const char* op);

// allocates and fills sorted_slots [nb_max * block_m] and block_expert
// [nb_max] for the S = ids.numel() slots (one launch, no host read)
void launch_align(const torch::Tensor& ids, long n_exp, long block_m,
                  torch::Tensor& sorted_slots, torch::Tensor& block_expert);

// out[t] = sum_j weights[t, j] * y[t*k + j] (fp32, ascending j, one rounding)
// y fp32 [T*k, H], weights fp32 [T, k], out bf16 [T, H], H % 4 == 0
void launch_combine(const torch::Tensor& y, const torch::Tensor& weights,
                    torch::Tensor& out, const char* op);

}  // namespace cmls_moe
