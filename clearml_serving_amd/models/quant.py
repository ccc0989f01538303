"""fp8 (OCP e4m3) weight quantization for LLM serving.

Decode is weight-streaming bound: fp8 weights halve the HBM bytes per step.
Round 1 ran fp8 through hipBLASLt with FOUR un-fused elementwise passes of
dynamic activation quantization per projection and measured SLOWER than
bf16 end to end (3.7k vs 6.0k out-tok/s). Round 2 fuses the quantization
into the producing kernels -- ops.rmsnorm_fp8 / ops.silu_mul_fp8 emit fp8
bytes + per-row scales directly (one HBM pass), and decode-shaped GEMMs run
on the in-tree fp8 MFMA skinny kernel (ops.skinny_gemm_fp8) that fills the
256-CU chip where hipBLASLt's tiles cannot. Prefill-shaped GEMMs stay on
hipBLASLt scaled_mm (measured 1.69x vs bf16 at M=2048).

Scheme: per-output-row weight scales (absmax/448), dynamic per-row (token)
activation scales. Enable per endpoint via model card / aux
``{"quantization": "fp8"}``. The reference delegates all quantization to
vLLM (preprocess_service.py:619-1095).

``{"quantization": "mxfp4"}`` (llama-family models) halves the weight bytes
again: OCP MX e2m1 weights with an e8m0 scale per 32 k-values, taken
directly by the gfx950 block-scaled MFMA against the same fused fp8
activations, for decode-shaped rows (ops/csrc/mxfp4_path.hip) and for
prefill-shaped ones (ops/csrc/mxfp4_gemm.hip: workgroup tiles, A through
LDS) on the one tiled copy of the weight (Mxfp4Linear). Expert stacks of a
mixture-of-experts model are quantised the same way, one expert at a time,
and kept only in the kernel-tiled layout (quantize_experts_mxfp4,
ops.moe_experts_mxfp4, ops/csrc/moe_mxfp4.hip).
"""

import os

import torch
import torch.nn as nn

from .. import ops

F8 = torch.float8_e4m3fn
F8_MAX = 448.0


class Fp8Linear(nn.Module):
    """nn.Linear replacement: fp8 weights with per-row scales (an optional
    bias -- Qwen2 QKV -- stays in the compute dtype, added after the GEMM).

    Two entry points:
      forward(x)           -- bf16 in: quantize (one fused kernel) then GEMM
      forward_q(x8, xs)    -- pre-quantized activations from a fused
                              producer (rmsnorm_fp8 / silu_mul_fp8)
    """

    # decode-shaped rows route to the in-tree fp8 MFMA kernel; above this
    # hipBLASLt scaled_mm wins (measured crossover, profiles/fp8_kernels)
    SKINNY_MAX_M = int(__import__("os").environ.get("CMLS_FP8_SKINNY_MAX", 16))

    def __init__(self, linear: nn.Linear):
        super().__init__()
        w = linear.weight.data.float()
        row_max = w.abs().amax(dim=1, keepdim=True).clamp(min=1e-8)
        scale = row_max / F8_MAX
        w8 = (w / scale).to(F8).contiguous()
        self.register_buffer("weight_fp8", w8)
        # decode kernel reads a byte-swizzled copy (one 16-B lane load =
        # both MFMA operands of a 64-wide k pair); prefill scaled_mm needs
        # the plain layout, so both live in HBM (fp8: still half of bf16).
        # in_features % 64 != 0 never routes to that kernel (_route -> "lt")
        # and has no swizzled form
        self.register_buffer(
            "weight_fp8_sw",
            ops.swizzle_fp8_weight(w8) if w8.shape[1] % 64 == 0 else None)
        self.register_buffer("weight_scale",
                             scale.to(torch.float32).reshape(-1)
                             .contiguous())  # [N]
        self.out_features = linear.out_features
        self.in_features = linear.in_features
        self.out_dtype = linear.weight.dtype  # model compute dtype
        # Qwen2 QKV bias: added in the compute dtype after the fp8 GEMM
        if linear.bias is not None:
            self.register_buffer("bias", linear.bias.data.clone())
        else:
            self.bias = None

    # LDS-staged v2 (skinny_gemm_fp8_v2) beats STANDALONE hipBLASLt
    # scaled_mm at M 17..64 on qkv/o_proj shapes, but INSIDE the decode
    # hipGraphs scaled_mm has no launch floor and wins end to end
    # (12,170 vs 12,076 out-tok/s at 64 seqs, 6,928 vs 6,230 at 32) --
    # so v2 is OFF by default and kept as the measured exhibit
    # (CMLS_FP8_V2_MAX raises the cap for standalone/no-graph serving).
    V2_MAX_M = int(__import__("os").environ.get("CMLS_FP8_V2_MAX", 0))

    def _route(self, m: int) -> str:
        """Measured per-shape routing (profiles/fp8_kernels.txt):
        - v1 (8-wave k-split, swizzled weights) owns M<=16 -- except the
          huge-N gate_up shape above M=1, where hipBLASLt's ~22 us floor
          wins
        - v2 (LDS-staged, 4 waves) owns M 17..64 on the qkv/o_proj-class
          shapes (N < 16k, K < 8k)
        - hipBLASLt scaled_mm keeps huge-N / huge-K shapes at M >= 17 and
          everything above 64."""
        n, k = self.out_features, self.in_features
        if not (k % 64 == 0 and n % 16 == 0):
            return "lt"
        if m <= self.SKINNY_MAX_M:
            if n >= 16384 and m > 1:
                return "lt"
            return "v1"
        if m <= self.V2_MAX_M and k % 128 == 0 and n < 16384 and k < 8192:
            return "v2"
        return "lt"

    def forward_q(self, x8: torch.Tensor, x_scale: torch.Tensor,
                  out_dtype=None) -> torch.Tensor:
        out_dtype = out_dtype or self.out_dtype
        out = self._gemm_q(x8, x_scale, out_dtype)
        if self.bias is not None:
            out = out + self.bias.to(out_dtype)
        return out

    def _gemm_q(self, x8: torch.Tensor, x_scale: torch.Tensor,
                out_dtype) -> torch.Tensor:
        m = x8.shape[0]
        route = self._route(m) if x8.is_cuda else "lt"
        if route == "v1":
            out = ops.skinny_gemm_fp8(x8, x_scale, self.weight_fp8_sw,
                                      self.weight_scale, swizzled=True)
            return out if out.dtype == out_dtype else out.to(out_dtype)
        if route == "v2":
            out = ops.skinny_gemm_fp8_v2(x8, x_scale, self.weight_fp8,
                                         self.weight_scale)
            return out if out.dtype == out_dtype else out.to(out_dtype)
        if not x8.is_cuda:
            return ops.skinny_gemm_fp8(x8, x_scale, self.weight_fp8,
                                       self.weight_scale).to(out_dtype)
        # prefill-shaped: hipBLASLt scaled_mm (rowwise scales); M % 16 pad
        pad = (-m) % 16
        xq = x8.view(F8)
        xs = x_scale.reshape(-1, 1)
        if pad:
            xq = torch.nn.functional.pad(xq.view(torch.uint8),
                                         (0, 0, 0, pad)).view(F8)
            xs = torch.nn.functional.pad(xs, (0, 0, 0, pad), value=1.0)
        out = torch._scaled_mm(
            xq, self.weight_fp8.t(), scale_a=xs.contiguous(),
            scale_b=self.weight_scale.reshape(1, -1), out_dtype=out_dtype)
        return out[:m] if pad else out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        orig_shape = x.shape
        x2 = x.reshape(-1, orig_shape[-1])
        x8, xs = ops.quant_fp8(x2)
        out = self.forward_q(x8, xs, out_dtype=x.dtype)
        return out.reshape(*orig_shape[:-1], self.out_features)


class Mxfp4Linear(nn.Module):
    """nn.Linear replacement: MXFP4 weights (OCP MX e2m1 + e8m0 scale per 32
    k-values, ops.quantize_mxfp4; row scale all ones) against the same e4m3
    activations Fp8Linear takes, with the same forward / forward_q surface
    and the same bias handling. Only the kernel-tiled copy of the weight
    (ops.tile_mxfp4_weight) lives in HBM: 4.25 bits per weight.

    Routing, all on the block-scaled MFMA and the same buffers:
    - "skinny": M <= SKINNY_MAX_M on K % 128 == 0, N % 16 == 0 runs
      ops.skinny_gemm_mxfp4 (decode).
    - "tiled": larger M, up to TILED_MAX_M, on K % 128 == 0, N % 128 == 0
      runs ops.gemm_mxfp4 (prefill, chunked prefill, speculation
      verification, large decode batches). CMLS_MXFP4_TILED=0 turns this
      route off. A CPU tensor on this route takes the op's CPU path, one
      fp32 product: the oracle of the kernel.
    - "dequant": everything else -- other shapes (e.g. TP shards), M above
      TILED_MAX_M, every other CPU tensor -- dequantises the whole weight
      to a transient bf16 [N, K] buffer (ops.dequant_mxfp4_bf16: 2 bytes
      per weight written and read back, and N*K*2 bytes of peak memory per
      call) and runs a bf16 matmul on the dequantised activations."""

    # largest M at which skinny_gemm_mxfp4 beats the dequant + matmul route
    # on every Llama-3-8B projection shape (profiles/mxfp4_kernels.txt: at
    # M=64 12-60 us against 46-195 us); 64 is also the kernel's own limit
    SKINNY_MAX_M = 64
    # largest M at which gemm_mxfp4 beat the dequant + matmul route on every
    # Llama-3-8B projection shape (profiles/mxfp4_gemm.txt); None = no limit
    TILED_MAX_M = None

    def __init__(self, linear: nn.Linear):
        super().__init__()
        w4, e8, row_scale = ops.quantize_mxfp4(linear.weight.data)
        w4t, e8t = ops.tile_mxfp4_weight(w4, e8)
        self.register_buffer("weight_mx", w4t)
        self.register_buffer("scale_mx", e8t)
        self.register_buffer("weight_scale", row_scale)  # [N] fp32
        self.out_features = linear.out_features
        self.in_features = linear.in_features
        self.out_dtype = linear.weight.dtype
        if linear.bias is not None:
            self.register_buffer("bias", linear.bias.data.clone())
        else:
            self.bias = None

    def _route(self, m: int) -> str:
        n, k = self.out_features, self.in_features
        if m <= self.SKINNY_MAX_M and k % 128 == 0 and n % 16 == 0:
            return "skinny"
        if (m > self.SKINNY_MAX_M and k % 128 == 0 and n % 128 == 0
                and (self.TILED_MAX_M is None or m <= self.TILED_MAX_M)
                and os.environ.get("CMLS_MXFP4_TILED", "1") != "0"):
            return "tiled"
        return "dequant"

    def forward_q(self, x8: torch.Tensor, x_scale: torch.Tensor,
                  out_dtype=None) -> torch.Tensor:
        out_dtype = out_dtype or self.out_dtype
        route = self._route(x8.shape[0])
        # a CPU tensor on the "tiled" route takes gemm_mxfp4's CPU path, one
        # fp32 product: the CPU's bf16 matmul below does not keep an fp32 sum
        # over a long K and is no oracle for the kernel at K = 1024. Decode
        # shapes on the CPU stay where they were
        if route == "skinny" and not x8.is_cuda:
            route = "dequant"
        if route == "skinny":
            out = ops.skinny_gemm_mxfp4(x8, x_scale, self.weight_mx,
                                        self.scale_mx, self.weight_scale)
        elif route == "tiled":
            out = ops.gemm_mxfp4(x8, x_scale, self.weight_mx, self.scale_mx,
                                 self.weight_scale)
        else:
            w = ops.dequant_mxfp4_bf16(self.weight_mx, self.scale_mx,
                                       self.weight_scale, self.out_features,
                                       self.in_features)
            # e4m3 is exact in bf16; the row scale goes on in fp32 after
            out = (x8.view(F8).to(torch.bfloat16) @ w.t()).float() \
                * x_scale[:, None]
        out = out if out.dtype == out_dtype else out.to(out_dtype)
        if self.bias is not None:
            out = out + self.bias.to(out_dtype)
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        orig_shape = x.shape
        x8, xs = ops.quant_fp8(x.reshape(-1, orig_shape[-1]))
        out = self.forward_q(x8, xs, out_dtype=x.dtype)
        return out.reshape(*orig_shape[:-1], self.out_features)


def quantize_experts_mxfp4(w: torch.Tensor):
    """Expert stack [E, N, K] (N % 16 == 0, K % 128 == 0) -> (e2m1 bytes
    uint8 [E, N/16, K/128, 64, 16], e8m0 scales uint8 [E, N/16, ceil(K/512),
    64, 4], fp32 row scales [E, N], all ones): every expert quantised by
    ops.quantize_mxfp4 and kept in the ops.tile_mxfp4_weight layout, the
    operands of ops.moe_experts_mxfp4. One expert at a time, so the fp32
    temporaries stay at one expert's size."""
    e, n, k = w.shape
    if n % 16 or k % 128:
        raise ValueError("quantize_experts_mxfp4: need N % 16 == 0 and "
                         "K % 128 == 0, got N={} K={}".format(n, k))
    steps = k // 128
    w4t = torch.empty(e, n // 16, steps, 64, 16, dtype=torch.uint8,
                      device=w.device)
    e8t = torch.empty(e, n // 16, (steps + 3) // 4, 64, 4, dtype=torch.uint8,
                      device=w.device)
    scale = torch.empty(e, n, dtype=torch.float32, device=w.device)
    for i in range(e):
        w4, e8, scale[i] = ops.quantize_mxfp4(w[i])
        w4t[i], e8t[i] = ops.tile_mxfp4_weight(w4, e8)
    return w4t, e8t, scale


def quantize_llama_mxfp4(model: nn.Module) -> int:
    """Swap the projection Linears (qkv, o_proj, gate_up, down) of a
    LlamaForCausalLM to Mxfp4Linear; lm_head stays bf16. A layer with experts
    also gets its ``w13`` / ``w2`` stacks replaced by tiled e2m1 buffers of
    the same names plus ``w13_e8`` / ``w2_e8`` (tiled e8m0 scales) and
    ``w13_scale`` / ``w2_scale`` (quantize_experts_mxfp4); the bf16
    parameters are dropped and the router stays in the model dtype. Returns
    the number of projections and expert stacks converted."""
    n = 0
    for layer in getattr(model, "layers", []):
        for name in ("w13", "w2"):
            w = getattr(layer, name, None)
            if isinstance(w, nn.Parameter):
                w4t, e8t, scale = quantize_experts_mxfp4(w.data)
                delattr(layer, name)
                layer.register_buffer(name, w4t)
                layer.register_buffer(name + "_e8", e8t)
                layer.register_buffer(name + "_scale", scale)
                n += 1
        for name in ("qkv", "o_proj", "gate_up", "down"):
            lin = getattr(layer, name, None)
            if isinstance(lin, nn.Linear):
                setattr(layer, name, Mxfp4Linear(lin))
                n += 1
    return n


def quantize_experts_fp8(w: torch.Tensor):
    """Expert stack [E, N, K] -> (e4m3 bytes uint8 [E, N, K], every row in
    the ops.swizzle_fp8_weight layout, fp32 scales [E, N] = row absmax/448):
    the operands of ops.moe_experts_fp8. One expert at a time, so the fp32
    temporaries stay at one expert's size."""
    e, n, k = w.shape
    w8 = torch.empty(e, n, k, dtype=torch.uint8, device=w.device)
    scale = torch.empty(e, n, dtype=torch.float32, device=w.device)
    for i in range(e):
        wf = w[i].float()
        s = wf.abs().amax(dim=1, keepdim=True).clamp(min=1e-8) / F8_MAX
        w8[i] = ops.swizzle_fp8_weight((wf / s).to(F8))
        scale[i] = s.reshape(-1)
    return w8, scale


def quantize_llama_fp8(model: nn.Module) -> int:
    """Swap the projection Linears of a LlamaForCausalLM to Fp8Linear
    (lm_head stays bf16 for logit fidelity). A layer with experts also gets
    its ``w13`` / ``w2`` stacks replaced by e4m3 buffers of the same names
    plus ``w13_scale`` / ``w2_scale`` (quantize_experts_fp8); the bf16
    parameters are dropped and the router stays in the model dtype. Returns
    the number of projections and expert stacks converted."""
    n = 0
    for layer in getattr(model, "layers", []):
        for name in ("w13", "w2"):
            w = getattr(layer, name, None)
            if isinstance(w, nn.Parameter):
                w8, scale = quantize_experts_fp8(w.data)
                delattr(layer, name)
                layer.register_buffer(name, w8)
                layer.register_buffer(name + "_scale", scale)
                n += 1
        for name in ("qkv", "o_proj", "gate_up", "down"):
            lin = getattr(layer, name, None)
            if isinstance(lin, nn.Linear):
                setattr(layer, name, Fp8Linear(lin))
                n += 1
    return n
