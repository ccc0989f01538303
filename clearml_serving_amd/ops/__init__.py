"""HIP/CDNA4 kernel library: python dispatch layer.

The compute tier the reference outsources to Triton/vLLM
lives here as hand-written gfx950 kernels (``csrc/*.hip``), compiled in-tree
to ``_hip_ops.so`` by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950
via torch.utils.cpp_extension).

Dispatch policy:
- tensor on GPU  -> the HIP extension is REQUIRED; a missing .so raises
  instead of silently falling back to eager PyTorch (so a GPU run can never
  "pass" on the fallback path).
- tensor on CPU  -> plain PyTorch reference implementations (used by the CPU
  test suite and as the fp32 numerics reference for the GPU kernels).

Set CLEARML_SERVING_AMD_FORCE_EAGER=1 to bypass the extension on GPU
(debug/ablation only).
"""

import importlib.machinery
import importlib.util
import math
import os
from typing import Optional, Tuple

import torch

_ext = None
_ext_error: Optional[str] = None
_FORCE_EAGER = os.environ.get("CLEARML_SERVING_AMD_FORCE_EAGER") == "1"


def _try_load_ext() -> None:
    global _ext, _ext_error
    if _ext is not None or _ext_error is not None:
        return
    so_path = os.path.join(os.path.dirname(__file__), "_hip_ops.so")
    if not os.path.exists(so_path):
        _ext_error = "extension not built ({} missing)".format(so_path)
        return
    try:
        loader = importlib.machinery.ExtensionFileLoader("_hip_ops", so_path)
        spec = importlib.util.spec_from_loader("_hip_ops", loader)
        mod = importlib.util.module_from_spec(spec)
        loader.exec_module(mod)
        _ext = mod
    except Exception as ex:  # loud, but deferred to first GPU use
        _ext_error = "failed loading {}: {}".format(so_path, ex)


_try_load_ext()


def has_extension() -> bool:
    return _ext is not None


def _require_ext(opname: str):
    if _FORCE_EAGER:
        return None
    if _ext is None:
        raise RuntimeError(
            "clearml_serving_amd HIP extension required for GPU op '{}' but "
            "not loaded: {}. Build it with __graft_entry__.build() "
            "(hipcc --offload-arch=gfx950).".format(opname, _ext_error)
        )
    return _ext


def extension_or_none():
    return _ext


# --------------------------------------------------------------------- #
# LayerNorm (+ fused residual add)
# --------------------------------------------------------------------- #
def layernorm(
    x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
    eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """out = LN(x + residual) over the last dim. bf16/fp32 in, same dtype out."""
    if x.is_cuda:
        ext = _require_ext("layernorm")
        if ext is not None:
            return ext.layernorm(x, weight, bias, eps, residual)
    if residual is not None:
        x = x + residual
    return torch.nn.functional.layer_norm(
        x.float(), (x.shape[-1],), weight.float(), bias.float(), eps
    ).to(x.dtype)


def rmsnorm(
    x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6,
    residual: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """out = x / rms(x) * weight (llama-style), optional fused residual add.

    When ``residual`` is given the op ALSO writes x+residual back into
    ``residual`` in-place on the GPU path (the running residual stream),
    matching the CPU reference below.
    """
    if x.is_cuda:
        ext = _require_ext("rmsnorm")
        if ext is not None:
            return ext.rmsnorm(x, weight, eps, residual)
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
        residual.copy_(xf.to(residual.dtype))
    out = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (out * weight.float()).to(x.dtype)


# --------------------------------------------------------------------- #
# Activations / epilogues
# --------------------------------------------------------------------- #
def bias_gelu(x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = gelu(x + bias), erf formulation (BERT)."""
    if x.is_cuda:
        ext = _require_ext("bias_gelu")
        if ext is not None:
            return ext.bias_gelu(x, bias)
    if bias is not None:
        x = x + bias
    return torch.nn.functional.gelu(x.float()).to(x.dtype)


def bias_relu_add(
    x: torch.Tensor, bias: Optional[torch.Tensor] = None,
    residual: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """out = relu(x + bias + residual) -- ResNet bottleneck epilogue."""
    if x.is_cuda:
        ext = _require_ext("bias_relu_add")
        if ext is not None:
            return ext.bias_relu_add(x, bias, residual)
    if bias is not None:
        x = x + bias
    if residual is not None:
        x = x + residual
    return torch.relu(x)


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """out = silu(gate) * up -- llama MLP."""
    if gate.is_cuda:
        ext = _require_ext("silu_mul")
        if ext is not None:
            return ext.silu_mul(gate, up)
    return (torch.nn.functional.silu(gate.float()) * up.float()).to(gate.dtype)


# --------------------------------------------------------------------- #
# fp8 (OCP e4m3) decode path: fused activation quant + skinny fp8 GEMM
# (kernels: csrc/fp8_path.hip; replaces the round-1 un-fused quantization
# that made fp8 slower than bf16 end to end)
# --------------------------------------------------------------------- #
F8_MAX = 448.0


def _quant_fp8_ref(y: torch.Tensor):
    """Reference per-row quantization (CPU path / numerics oracle)."""
    y2 = y.float().reshape(-1, y.shape[-1])
    amax = y2.abs().amax(dim=1).clamp(min=1e-8)
    scale = (amax / F8_MAX).to(torch.float32)
    q = (y2 / scale[:, None]).clamp(-F8_MAX, F8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def rmsnorm_fp8(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6,
                residual: Optional[torch.Tensor] = None):
    """rmsnorm (+fused residual update, same contract as rmsnorm()) emitting
    fp8-e4m3 bytes + per-row scales in ONE pass over HBM."""
    if x.is_cuda:
        ext = _require_ext("rmsnorm_fp8")
        if ext is not None:
            out8, scales = ext.rmsnorm_fp8(x, weight, eps, residual)
            return out8, scales
    return _quant_fp8_ref(rmsnorm(x, weight, eps, residual=residual))


def silu_mul_fp8(gate: torch.Tensor, up: torch.Tensor):
    """silu(gate) * up -> fp8-e4m3 bytes + per-row scales, one fused pass."""
    if gate.is_cuda:
        ext = _require_ext("silu_mul_fp8")
        if ext is not None:
            out8, scales = ext.silu_mul_fp8(gate, up)
            return out8, scales
    return _quant_fp8_ref(silu_mul(gate, up))


def quant_fp8(x: torch.Tensor):
    """Per-row dynamic fp8 quantization (for activations whose producer
    isn't one of the fused kernels, e.g. attention context)."""
    if x.is_cuda:
        ext = _require_ext("quant_fp8")
        if ext is not None:
            out8, scales = ext.quant_fp8(x)
            return out8, scales
    return _quant_fp8_ref(x)


def swizzle_fp8_weight(w8: torch.Tensor) -> torch.Tensor:
    """Reorder an fp8 [N, K] weight for skinny_gemm_fp8: within each
    64-byte k window-pair, bytes become [lane-group][window][8] so one
    16-byte lane load yields both MFMA operands of the pair (un-swizzled
    weights need two 8-byte loads -- measured request-rate bound)."""
    n, k = w8.shape
    assert k % 64 == 0
    v = w8.view(torch.uint8).reshape(n, k // 64, 2, 4, 8)
    return v.permute(0, 1, 3, 2, 4).contiguous().reshape(n, k)


def unswizzle_fp8_weight(w8s: torch.Tensor) -> torch.Tensor:
    n, k = w8s.shape
    v = w8s.view(torch.uint8).reshape(n, k // 64, 4, 2, 8)
    return v.permute(0, 1, 3, 2, 4).contiguous().reshape(n, k)


def skinny_gemm_fp8(a8: torch.Tensor, a_scale: torch.Tensor,
                    w8: torch.Tensor, w_scale: torch.Tensor,
                    swizzled: bool = False) -> torch.Tensor:
    """C[M,N] = (Aq*s_a) @ (Wq*s_w)^T -> bf16, decode-shaped M <= 64.

    One workgroup per 16 W columns (fills the 256-CU chip at llama
    projection N), fp8 operands halve the weight-streaming bytes vs bf16.
    ``swizzled``: w8 is already in swizzle_fp8_weight layout (Fp8Linear
    prepares it once at quantization time).
    """
    if a8.is_cuda:
        ext = _require_ext("skinny_gemm_fp8")
        if ext is not None:
            ws = w8 if swizzled else swizzle_fp8_weight(w8)
            return ext.skinny_gemm_fp8(
                a8.view(torch.uint8), a_scale, ws.view(torch.uint8), w_scale)
    if swizzled:
        w8 = unswizzle_fp8_weight(w8)
    a = a8.view(torch.float8_e4m3fn).float() * a_scale[:, None]
    w = w8.view(torch.float8_e4m3fn).float() * w_scale[:, None]
    return (a @ w.t()).to(torch.bfloat16)


def skinny_gemm_fp8_v2(a8: torch.Tensor, a_scale: torch.Tensor,
                       w8: torch.Tensor, w_scale: torch.Tensor
                       ) -> torch.Tensor:
    """LDS-staged skinny fp8 GEMM for M 17..64 (plain fp8 weight layout):
    4 waves share one k progression over register-pipelined 128-byte
    windows -- covers the mid-batch decode regime where v1's direct
    fragment loads collapse and hipBLASLt underfills the chip."""
    if a8.is_cuda:
        ext = _require_ext("skinny_gemm_fp8_v2")
        if ext is not None:
            return ext.skinny_gemm_fp8_v2(
                a8.view(torch.uint8), a_scale, w8.view(torch.uint8), w_scale)
    a = a8.view(torch.float8_e4m3fn).float() * a_scale[:, None]
    w = w8.view(torch.float8_e4m3fn).float() * w_scale[:, None]
    return (a @ w.t()).to(torch.bfloat16)


def conv3x3_supported(x: torch.Tensor, w: torch.Tensor) -> bool:
    """True when the in-tree conv kernel serves this shape (3x3 s1 p1,
    ResNet-50 bottleneck widths, bf16 GPU)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
            and x.shape[2] == x.shape[3] and x.shape[2] in (56, 28, 14)
            and x.shape[1] % 32 == 0 and w.shape[0] % 64 == 0
            and w.shape[2] == 3 and w.shape[3] == 3
            and os.environ.get("CMLS_CONV3", "1") != "0"
            and _ext is not None)


def conv3x3_nhwc(x: torch.Tensor, w: torch.Tensor,
                 bias: Optional[torch.Tensor] = None, relu: bool = False,
                 residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 stride-1 pad-1 NHWC bf16 conv (implicit GEMM, MFMA) for the
    ResNet-50 bottleneck widths 56/28/14; optional fused bias+residual+relu
    epilogue. Kernel: csrc/conv3x3.hip. CPU/odd shapes: torch reference."""
    if (x.is_cuda and x.dtype == torch.bfloat16
            and x.shape[2] == x.shape[3] and x.shape[2] in (56, 28, 14)
            and x.shape[1] % 32 == 0 and w.shape[0] % 64 == 0):
        ext = _require_ext("conv3x3_nhwc")
        if ext is not None:
            xc = x.contiguous(memory_format=torch.channels_last)
            wc = w.contiguous(memory_format=torch.channels_last)
            return ext.conv3x3_nhwc(xc, wc, bias, relu, residual)
    y = torch.nn.functional.conv2d(x.float(), w.float(),
                                   bias.float() if bias is not None else None,
                                   stride=1, padding=1)
    if residual is not None:
        y = y + residual.float()
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype)


def softmax(x: torch.Tensor, dim: int = -1) -> torch.Tensor:
    """Numerically-stable softmax over the last dim."""
    if x.is_cuda and dim in (-1, x.dim() - 1):
        ext = _require_ext("softmax")
        if ext is not None:
            return ext.softmax_lastdim(x)
    return torch.softmax(x.float(), dim=dim).to(x.dtype)


# --------------------------------------------------------------------- #
# Attention
# --------------------------------------------------------------------- #
def _check_window(window: Optional[int]) -> int:
    """Sliding-window argument -> kernel convention (0 = full context)."""
    if window is None:
        return 0
    window = int(window)
    if window < 0:
        raise ValueError("window must be >= 0, got {}".format(window))
    return window


def attention(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
    causal: bool = False, scale: Optional[float] = None,
    seq_lens: Optional[torch.Tensor] = None,
    layout: str = "bhsd",
    window: Optional[int] = None,
) -> torch.Tensor:
    """Fused scaled-dot-product attention (prefill / encoder).

    layout "bhsd": q,k,v = [B, H, S, D]; layout "bshd": [B, S, H, D]
    (strided views into a merged QKV projection are accepted -- no
    transpose copies). GQA via H_kv dividing H; ``seq_lens`` (int32 [B])
    masks keys >= len. Output has the input layout.

    ``window`` (sliding-window attention, causal only): query position i
    sees key j iff ``i - window < j <= i``; None or 0 = full context.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    window = _check_window(window)
    if window and not causal:
        raise ValueError("attention: a sliding window needs causal=True")
    bshd = layout == "bshd"
    if q.is_cuda:
        ext = _require_ext("attention")
        if ext is not None:
            return ext.attention_prefill(q, k, v, bool(causal), float(scale),
                                         seq_lens, bshd, window)
    if bshd:
        out = attention(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                        v.permute(0, 2, 1, 3), causal=causal, scale=scale,
                        seq_lens=seq_lens, window=window)
        return out.permute(0, 2, 1, 3).contiguous()
    # reference path (fp32 math)
    qf, kf, vf = q.float(), k.float(), v.float()
    hq, hkv = q.shape[1], k.shape[1]
    if hkv != hq:
        rep = hq // hkv
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    scores = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    sq, sk = q.shape[2], k.shape[2]
    if causal:
        mask = torch.ones(sq, sk, dtype=torch.bool, device=q.device).tril(
            diagonal=sk - sq)
        if window:
            # query row r sits at position r + (sk - sq); it keeps the
            # `window` most recent keys, its own included
            mask &= ~torch.ones(sq, sk, dtype=torch.bool,
                                device=q.device).tril(
                diagonal=sk - sq - window)
        scores = scores.masked_fill(~mask, float("-inf"))
    if seq_lens is not None:
        key_idx = torch.arange(sk, device=q.device)
        pad = key_idx[None, None, None, :] >= seq_lens[:, None, None, None]
        scores = scores.masked_fill(pad, float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    return torch.matmul(probs, vf).to(q.dtype)


def _dequant_kv_cpu(cache: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3 paged cache [NB, Hkv, BS, D] + scales [NB, Hkv, BS] ->
    float cache (CPU reference path for the fp8 KV cache)."""
    f = cache.view(torch.float8_e4m3fn).float()
    return f * scale[..., None]


def attention_prefill_paged(
    q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    block_table: torch.Tensor, kv_lens: torch.Tensor, q_lens: torch.Tensor,
    scale: Optional[float] = None,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
    window: Optional[int] = None,
) -> torch.Tensor:
    """Chunked-prefill attention: chunk queries [B, Sq, H, D] (bshd) attend
    causally to the full PAGED history (kv_lens keys per seq, already in the
    cache); q_lens masks per-seq chunk padding. Output [B, Sq, H, D].

    ``window``: sliding window as in :func:`attention`. Pages that lie
    wholly below the window start of a sequence's first query are never
    read, so their block-table entries may point at any valid page.

    fp8 KV: uint8 e4m3 caches + per-token-per-head ``k_scale``/``v_scale``
    float32 [NB, Hkv, BS]; the gfx950 kernel dequantizes while staging tiles
    to LDS (attention.hip FP8KV)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    window = _check_window(window)
    if q.is_cuda:
        ext = _require_ext("attention_prefill_paged")
        if ext is not None:
            return ext.attention_prefill_paged(
                q, k_cache, v_cache, block_table, kv_lens, q_lens,
                float(scale), k_scale, v_scale, window)
    if k_scale is not None:
        return attention_prefill_paged(
            q, _dequant_kv_cpu(k_cache, k_scale),
            _dequant_kv_cpu(v_cache, v_scale), block_table, kv_lens, q_lens,
            scale, window=window)
    # reference path: gather pages -> dense causal attention with history
    b, sq, h, d = q.shape
    hkv = k_cache.shape[1]
    bs = k_cache.shape[2]
    out = torch.zeros_like(q)
    for i in range(b):
        n = int(kv_lens[i])
        ql = int(q_lens[i])
        nb = (n + bs - 1) // bs
        blocks = block_table[i, :nb].long()
        k = k_cache[blocks].float().permute(1, 0, 2, 3).reshape(
            hkv, nb * bs, d)[:, :n]
        v = v_cache[blocks].float().permute(1, 0, 2, 3).reshape(
            hkv, nb * bs, d)[:, :n]
        if window:
            # keys below the first query's window are masked for every
            # row; their pages may be recycled, so drop them unread
            lo = max(0, n - ql - window + 1)
            k, v = k[:, lo:], v[:, lo:]
        o = attention(
            q[i, :ql].permute(1, 0, 2)[None].float(),
            k[None], v[None], causal=True, scale=scale, window=window)
        out[i, :ql] = o[0].permute(1, 0, 2).to(q.dtype)
    return out


def attention_decode(
    q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    block_table: torch.Tensor, seq_lens: torch.Tensor,
    scale: Optional[float] = None,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
    window: Optional[int] = None,
) -> torch.Tensor:
    """Paged-KV decode attention: one new token per sequence.

    q:        [B, H, D]         (current-step queries)
    k_cache:  [num_blocks, H_kv, block_size, D]
    v_cache:  [num_blocks, H_kv, block_size, D]
    block_table: int32 [B, max_blocks] physical block ids per sequence
    seq_lens: int32 [B] total keys per sequence (including current token)

    fp8 KV: uint8 e4m3 caches + float32 [NB, Hkv, BS] per-token scales;
    halves the decode KV-read bytes (the long-context bandwidth bound).

    ``window``: the query sees only the last ``window`` keys (None or 0 =
    all of them); keys and block-table entries below that are never read.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    window = _check_window(window)
    if q.is_cuda:
        ext = _require_ext("attention_decode")
        if ext is not None:
            return ext.attention_decode(q, k_cache, v_cache, block_table,
                                        seq_lens, float(scale),
                                        k_scale, v_scale, window)
    if k_scale is not None:
        return attention_decode(
            q, _dequant_kv_cpu(k_cache, k_scale),
            _dequant_kv_cpu(v_cache, v_scale), block_table, seq_lens, scale,
            window=window)
    # reference path: gather pages then dense attention per sequence
    bsz, hq, d = q.shape
    hkv = k_cache.shape[1]
    block_size = k_cache.shape[2]
    rep = hq // hkv
    out = torch.empty_like(q, dtype=q.dtype)
    qf = q.float()
    for b in range(bsz):
        n = int(seq_lens[b])
        nblocks = (n + block_size - 1) // block_size
        blocks = block_table[b, :nblocks].long()
        k = k_cache[blocks].float()  # [nb, hkv, bs, d]
        v = v_cache[blocks].float()
        k = k.permute(1, 0, 2, 3).reshape(hkv, nblocks * block_size, d)[:, :n]
        v = v.permute(1, 0, 2, 3).reshape(hkv, nblocks * block_size, d)[:, :n]
        if window:
            k, v = k[:, max(0, n - window):], v[:, max(0, n - window):]
        if rep > 1:
            k = k.repeat_interleave(rep, dim=0)
            v = v.repeat_interleave(rep, dim=0)
        scores = torch.einsum("hd,hnd->hn", qf[b], k) * scale
        probs = torch.softmax(scores, dim=-1)
        out[b] = torch.einsum("hn,hnd->hd", probs, v).to(q.dtype)
    return out


def kv_cache_write(
    k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor,
    v_cache: torch.Tensor, slot_mapping: torch.Tensor,
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
) -> None:
    """Scatter [T, H_kv, D] new keys/values into the paged caches at flat
    slots (block_id * block_size + offset); slot -1 skips the token.

    fp8 KV: pass uint8 caches + float32 [NB, Hkv, BS] scale tensors; each
    (token, head) row is absmax-quantized to e4m3 and its scale recorded."""
    if k_new.is_cuda:
        ext = _require_ext("kv_cache_write")
        if ext is not None:
            ext.kv_cache_write(k_new, v_new, k_cache, v_cache, slot_mapping,
                               k_scale, v_scale)
            return
    block_size = k_cache.shape[2]
    fp8 = k_scale is not None
    for t in range(k_new.shape[0]):
        slot = int(slot_mapping[t])
        if slot < 0:
            continue
        blk, off = slot // block_size, slot % block_size
        if fp8:
            for cache, scales, new in ((k_cache, k_scale, k_new),
                                       (v_cache, v_scale, v_new)):
                row = new[t].float()  # [H_kv, D]
                amax = row.abs().amax(dim=-1).clamp_min(1e-8)
                # pow2 scales match the GPU quantizer (scalef32 dequant
                # applies only the scale exponent -- MX semantics)
                sc = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
                q8 = (row / sc[:, None]).to(torch.float8_e4m3fn)
                cache[blk, :, off] = q8.view(torch.uint8)
                scales[blk, :, off] = sc
        else:
            k_cache[blk, :, off] = k_new[t]
            v_cache[blk, :, off] = v_new[t]


# --------------------------------------------------------------------- #
# Rotary embedding
# --------------------------------------------------------------------- #
def rope_inplace(
    q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor,
    theta: float = 10000.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Apply rotary position embedding in place (NeoX interleaving: rotate
    pairs (i, i+D/2)). q: [T, H, D], k: [T, H_kv, D], positions: int32 [T]."""
    if q.is_cuda:
        ext = _require_ext("rope")
        if ext is not None:
            ext.rope_inplace(q, k, positions, float(theta))
            return q, k
    d = q.shape[-1]
    half = d // 2
    inv_freq = 1.0 / (theta ** (torch.arange(half, dtype=torch.float32,
                                             device=q.device) / half))
    angles = positions.float()[:, None] * inv_freq[None, :]  # [T, half]
    cos = angles.cos()[:, None, :]
    sin = angles.sin()[:, None, :]
    for t in (q, k):
        # clone: .float() on an fp32 tensor returns SELF, and lo/hi must not
        # alias the destination (in-place write of :half corrupted hi's input)
        tf = t.float().clone()
        lo, hi = tf[..., :half], tf[..., half:]
        t[..., :half] = (lo * cos - hi * sin).to(t.dtype)
        t[..., half:] = (hi * cos + lo * sin).to(t.dtype)
    return q, k


# --------------------------------------------------------------------- #
# Sampling
# --------------------------------------------------------------------- #
def sample_top_k_top_p(
    logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0,
    top_p: float = 1.0, generator: Optional[torch.Generator] = None,
) -> torch.Tensor:
    """Sample token ids from [B, V] logits with temperature/top-k/top-p.

    Greedy when temperature == 0. Returns int64 [B].
    """
    if temperature == 0.0:
        return logits.argmax(dim=-1)
    if logits.is_cuda:
        ext = _require_ext("sample")
        if ext is not None:
            seed = int(torch.randint(0, 2**31 - 1, (1,),
                                     generator=generator).item())
            return ext.sample_top_k_top_p(
                logits, float(temperature), int(top_k), float(top_p), seed)
    lf = logits.float() / temperature
    if top_k and top_k < lf.shape[-1]:
        kth = torch.topk(lf, top_k, dim=-1).values[..., -1:]
        lf = lf.masked_fill(lf < kth, float("-inf"))
    if top_p < 1.0:
        sorted_logits, idx = torch.sort(lf, descending=True, dim=-1)
        probs = torch.softmax(sorted_logits, dim=-1)
        # drop tokens whose inclusive cumulative prob exceeds p; always keep
        # the top token
        cutoff = probs.cumsum(dim=-1) > top_p
        cutoff[..., 0] = False
        sorted_logits = sorted_logits.masked_fill(cutoff, float("-inf"))
        lf = torch.full_like(lf, float("-inf")).scatter(-1, idx, sorted_logits)
    probs = torch.softmax(lf, dim=-1)
    return torch.multinomial(probs, 1, generator=generator).squeeze(-1)


# --------------------------------------------------------------------- #
# GEMM (bf16 MFMA)
# --------------------------------------------------------------------- #
def gemm_bf16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """C[M,N] = A[M,K] @ B[N,K]^T in bf16 with fp32 accumulation on MFMA
    (nn.Linear orientation: b is a [out, in] weight matrix).

    STATUS: test fixture / benchmark exhibit, NOT routed in any serving
    model. Measured 867 TF vs hipBLASLt's 1362 TF on large dense shapes
    (profiles/README.md §4), so production GEMMs go through torch.matmul
    (hipBLASLt); the decode-shaped regime where hand-written kernels DO win
    is covered by skinny_gemm / skinny_gemm_fp8 / conv3x3_nhwc, all routed.
    Kept (with tests + kernel_bench entry) as the dense-tile reference the
    conv kernel's tiling derives from. Shapes off the 128/128/32 tile grid
    are zero-padded here.
    """
    if a.is_cuda:
        ext = _require_ext("gemm_bf16")
        if ext is not None:
            m, k = a.shape
            n = b.shape[0]
            pm, pn, pk = (-m) % 128, (-n) % 128, (-k) % 32
            if pm or pn or pk:
                a2 = torch.nn.functional.pad(a, (0, pk, 0, pm))
                b2 = torch.nn.functional.pad(b, (0, pk, 0, pn))
                return ext.gemm_bf16(a2.contiguous(),
                                     b2.contiguous())[:m, :n].contiguous()
            return ext.gemm_bf16(a.contiguous(), b.contiguous())
    return (a.float() @ b.float().T).to(a.dtype)


def skinny_linear(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """y = x @ weight.T for decode-shaped activations (rows <= 128).

    Routes to the in-tree skinny MFMA kernel on GPU exactly where it
    MEASURES faster than hipBLASLt (profiles/skinny_bench.txt): the
    small-N llama projections at M <= 16 (qkv 1.2x, o_proj 2.0-2.8x --
    hipBLASLt's tiles under-fill the 256-CU chip there) and the large-K
    down projection at M <= 2. Everything else falls back to
    torch.nn.functional.linear (hipBLASLt) -- as does an empty batch, and
    a non-contiguous weight (the kernel streams W rows as stored; copying
    a weight per call would cost more than the kernel saves).
    """
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2
            and x.shape[1] % 32 == 0 and weight.shape[0] % 16 == 0
            and weight.is_contiguous()
            and os.environ.get("CMLS_SKINNY", "1") != "0"):
        m, k = x.shape
        n = weight.shape[0]
        if ((1 <= m <= 16 and n <= 8192 and k <= 8192)
                or (1 <= m <= 2 and n <= 8192)):
            ext = _require_ext("skinny_gemm")
            # the kernel's fragment loads are 16-byte vectors: a single row
            # sliced at an odd column offset is "contiguous" yet misaligned
            xc = x.contiguous()
            if (ext is not None and xc.data_ptr() % 16 == 0
                    and weight.data_ptr() % 16 == 0):
                return ext.skinny_gemm(xc, weight, 1)
    return torch.nn.functional.linear(x, weight)


# --------------------------------------------------------------------- #
# Multi-LoRA (BGMV-style): per-token adapter deltas in one launch each
# (kernels: csrc/lora.hip)
# --------------------------------------------------------------------- #
def lora_shrink(x: torch.Tensor, a: torch.Tensor,
                idx: torch.Tensor) -> torch.Tensor:
    """y[t] = A[idx[t]] @ x[t] -> fp32 [T, R].

    x: [T, K]; a: [L, R, K] stacked adapter A matrices; idx: int32 [T] in
    [-1, L) (PRECONDITION: idx < L is not checked on the GPU path -- that
    would cost a device sync). Rows with idx == -1 (base model, decode-graph
    padding) are skipped: the GPU kernel leaves them unwritten, the
    reference zeroes them. GPU: bf16, K % 8 == 0, R % 16 == 0, R <= 256."""
    if x.is_cuda:
        ext = _require_ext("lora_shrink")
        if ext is not None:
            return ext.lora_shrink(x.contiguous(), a, idx)
    sel = a.float().index_select(0, idx.clamp(min=0).long())  # [T, R, K]
    y = torch.bmm(sel, x.float().unsqueeze(-1)).squeeze(-1)
    return torch.where((idx >= 0).unsqueeze(-1), y, torch.zeros_like(y))


def lora_expand_add(y: torch.Tensor, b: torch.Tensor, idx: torch.Tensor,
                    out: torch.Tensor) -> torch.Tensor:
    """out[t] += B[idx[t]] @ y[t], in place (fp32 accumulation, one
    rounding to out's dtype); returns ``out``.

    y: fp32 [T, R] from lora_shrink; b: [L, N, R] with alpha/r folded in;
    out: contiguous [T, N]. Rows with idx == -1 keep ``out`` bit-identical
    and their ``y`` row is never read."""
    if out.is_cuda:
        ext = _require_ext("lora_expand_add")
        if ext is not None:
            ext.lora_expand_add(y, b, idx, out)
            return out
    live = (idx >= 0).unsqueeze(-1)
    sel = b.float().index_select(0, idx.clamp(min=0).long())  # [T, N, R]
    yf = torch.where(live, y.float(), torch.zeros_like(y, dtype=torch.float32))
    delta = torch.bmm(sel, yf.unsqueeze(-1)).squeeze(-1)
    out.copy_(torch.where(live, (out.float() + delta).to(out.dtype), out))
    return out


# --------------------------------------------------------------------- #
# Guided decoding: token bitmasks (kernels: csrc/token_mask.hip)
# --------------------------------------------------------------------- #
def _check_mask_args(logits: torch.Tensor, bank: torch.Tensor,
                     slot: torch.Tensor) -> None:
    if logits.dim() != 2:
        raise ValueError("logits must be [B, V]")
    if bank.dtype != torch.int32 or bank.dim() != 2 \
            or bank.shape[1] != (logits.shape[1] + 31) // 32:
        raise ValueError("bank must be int32 [S, ceil(V/32)]")
    if slot.dtype != torch.int32 or slot.dim() != 1 \
            or slot.shape[0] != logits.shape[0]:
        raise ValueError("slot must be int32 [B]")


def _unpack_token_bitmask(bank: torch.Tensor, slot: torch.Tensor,
                          vocab: int) -> torch.Tensor:
    """bool [B, V] allowed-token matrix; slot -1 rows are all True."""
    rows = bank.index_select(0, slot.clamp(min=0).long())  # [B, W]
    shifts = torch.arange(32, dtype=torch.int32, device=bank.device)
    bits = (rows.unsqueeze(-1) >> shifts) & 1                # [B, W, 32]
    allowed = bits.reshape(rows.shape[0], -1)[:, :vocab].bool()
    return allowed | (slot < 0).unsqueeze(-1)


def apply_token_bitmask(logits: torch.Tensor, bank: torch.Tensor,
                        slot: torch.Tensor) -> torch.Tensor:
    """Copy of ``logits`` [B, V] with the tokens its row's mask disallows
    set to -inf; the source is never written (decode-graph logits are static
    replay buffers).

    bank: int32 [S, W], W = ceil(V/32), token t = bit t&31 of word t>>5;
    slot: int32 [B] bank row per logits row, -1 = unconstrained (copied
    bit-identically). PRECONDITION: slot < S (not checked on the GPU path --
    that would cost a device sync; the kernel treats an out-of-range slot
    as -1 rather than read past the bank)."""
    if logits.is_cuda:
        ext = _require_ext("apply_token_bitmask")
        if ext is not None:
            return ext.apply_token_bitmask(logits, bank, slot)
    _check_mask_args(logits, bank, slot)
    allowed = _unpack_token_bitmask(bank, slot, logits.shape[1])
    return logits.masked_fill(~allowed, float("-inf"))


def sample_token_bitmask(logits: torch.Tensor, bank: torch.Tensor,
                         slot: torch.Tensor, temperature: torch.Tensor,
                         seed: torch.Tensor) -> torch.Tensor:
    """Fused mask + draw for a heterogeneous batch -> int64 [B].

    temperature: float32 [B], 0 = greedy (argmax of the masked row, lowest
    index on ties); otherwise one categorical draw from softmax(masked /
    temperature), reproducible from that row's (logits, mask, temperature,
    seed) alone -- independent of the row's position and of the batch.
    seed: int32 [B]. A row whose mask allows nothing returns -1.

    The CPU reference draws with torch.multinomial under a per-row
    generator: same allowed set and greedy results as the GPU kernel, not
    the same sampled tokens."""
    if logits.is_cuda:
        ext = _require_ext("sample_token_bitmask")
        if ext is not None:
            return ext.sample_token_bitmask(logits, bank, slot, temperature,
                                            seed)
    _check_mask_args(logits, bank, slot)
    allowed = _unpack_token_bitmask(bank, slot, logits.shape[1])
    masked = logits.float().masked_fill(~allowed, float("-inf"))
    out = masked.argmax(dim=-1)
    for i in range(logits.shape[0]):
        t = float(temperature[i])
        if t > 0.0 and bool(allowed[i].any()):
            gen = torch.Generator(device=logits.device)
            gen.manual_seed(int(seed[i]) & 0x7FFFFFFF)
            probs = torch.softmax(masked[i] / t, dim=-1)
            out[i] = torch.multinomial(probs, 1, generator=gen)[0]
    return torch.where(allowed.any(dim=-1), out, torch.full_like(out, -1))


# --------------------------------------------------------------------- #
# Mixture of experts (kernels: csrc/moe.hip). The plain-PyTorch references
# below DEFINE the semantics the kernels are tested against.
# --------------------------------------------------------------------- #
MOE_MAX_EXPERTS = 64
MOE_MAX_TOP_K = 8


def _check_moe_route(num_experts: int, top_k: int) -> None:
    if not (1 <= top_k <= MOE_MAX_TOP_K
            and top_k <= num_experts <= MOE_MAX_EXPERTS):
        raise RuntimeError(
            "moe: need 1 <= k <= {} and k <= E <= {}, got k={} E={}".format(
                MOE_MAX_TOP_K, MOE_MAX_EXPERTS, top_k, num_experts))


def moe_nb_max(num_slots: int, num_experts: int, block_m: int) -> int:
    """Row blocks moe_align reserves: the worst case over all routings of
    sum_e ceil(count_e / block_m) -- a function of shapes only."""
    return ((num_slots + min(num_experts, num_slots) * (block_m - 1))
            // block_m)


def moe_route(logits: torch.Tensor, top_k: int,
              renormalize: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Router: logits [T, E] (bf16 or fp32) -> (ids int32 [T, k], weights
    fp32 [T, k]).

    Reference semantics (this function's CPU path): softmax over all E
    experts in fp32; the top-k experts are selected by LOGIT order (monotonic
    with the probabilities), a tie going to the lowest expert index, and
    emitted in descending probability; ``renormalize`` divides the k weights
    by their sum (Mixtral). 1 <= k <= 8 and k <= E <= 64, else RuntimeError.
    """
    _check_moe_route(logits.shape[-1], top_k)
    if logits.is_cuda:
        ext = _require_ext("moe_route")
        if ext is not None:
            ids, weights = ext.moe_route(logits.contiguous(), int(top_k),
                                         bool(renormalize))
            return ids, weights
    lf = logits.float()
    probs = torch.softmax(lf, dim=-1)
    # a stable descending sort keeps the lowest index first among equals
    ids = torch.sort(lf, dim=-1, descending=True,
                     stable=True).indices[:, :top_k]
    weights = probs.gather(-1, ids)
    if renormalize:
        weights = weights / weights.sum(dim=-1, keepdim=True)
    return ids.to(torch.int32), weights


def moe_align(ids: torch.Tensor, num_experts: int,
              block_m: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """Group the S = T*k flat slots (slot = t*k + j) of ``ids`` int32 [T, k]
    by expert for the grouped GEMMs -> (sorted_slots int32 [NB_max*block_m],
    block_expert int32 [NB_max]), NB_max = moe_nb_max(S, E, block_m).

    Reference semantics (this function's CPU path): experts in ascending
    order, each expert's slots ascending and padded to a multiple of
    ``block_m`` rows with the sentinel S; ``block_expert[b]`` is the expert
    of rows [b*block_m, (b+1)*block_m); unused trailing blocks hold -1 (and
    sentinel rows). Every slot appears exactly once. PRECONDITION: ids in
    [0, E) -- not checked on the GPU path (a device sync); the kernel drops
    a slot whose id is out of range."""
    if not 1 <= num_experts <= MOE_MAX_EXPERTS:
        raise RuntimeError("moe_align: need 1 <= E <= {}, got {}".format(
            MOE_MAX_EXPERTS, num_experts))
    if ids.is_cuda:
        ext = _require_ext("moe_align")
        if ext is not None:
            sorted_slots, block_expert = ext.moe_align(
                ids.contiguous(), int(num_experts), int(block_m))
            return sorted_slots, block_expert
    flat = ids.reshape(-1)
    s = flat.numel()
    nb_max = moe_nb_max(s, num_experts, block_m)
    sorted_slots = torch.full((nb_max * block_m,), s, dtype=torch.int32,
                              device=ids.device)
    block_expert = torch.full((nb_max,), -1, dtype=torch.int32,
                              device=ids.device)
    blk = 0
    for e in range(num_experts):
        slots = (flat == e).nonzero().flatten()
        c = slots.numel()
        if c == 0:
            continue
        nb = (c + block_m - 1) // block_m
        sorted_slots[blk * block_m: blk * block_m + c] = slots.to(torch.int32)
        block_expert[blk: blk + nb] = e
        blk += nb
    return sorted_slots, block_expert


def _moe_experts_ref(x, w13, w2, ids, weights, act_dtype=None):
    """fp32 per-expert loop. ``act_dtype`` rounds silu(g)*u to that dtype
    first, the one place the fused path stores an intermediate in bf16."""
    t, h = x.shape
    inter = w2.shape[2]
    k = ids.shape[1]
    xf = x.float()
    y = torch.zeros(t, k, h, dtype=torch.float32, device=x.device)
    for e in range(w13.shape[0]):
        tok, choice = (ids == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        gu = xf[tok] @ w13[e].float().t()
        act = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
        if act_dtype is not None:
            act = act.to(act_dtype).float()
        y[tok, choice] = act @ w2[e].float().t()
    out = torch.zeros(t, h, dtype=torch.float32, device=x.device)
    for j in range(k):  # ascending j, fp32, one rounding at the end
        out += weights[:, j, None].float() * y[:, j]
    return out.to(x.dtype)


# Rows (tokens) up to which the fused grouped-GEMM path serves a GPU call
# outside graph capture; above it the call runs the per-expert hipBLASLt
# loop. From the Mixtral-8x7B layer table in profiles/moe_bench.txt: fused
# (64-row block) 1008 us vs loop 1419 us at T=128, 1654 vs 1510 us at T=256.
MOE_FUSED_MAX = int(os.environ.get("CMLS_MOE_FUSED_MAX", "128"))
# Row block of the fused path: 16 rows up to this many tokens, 64 above
# (same table: 720 vs 856 us at T=64, 1252 vs 1008 us at T=128).
MOE_BLOCK16_MAX = int(os.environ.get("CMLS_MOE_BLOCK16_MAX", "64"))


def _moe_experts_loop(x, w13, w2, ids, weights):
    """Prefill-sized GPU path: per-expert hipBLASLt GEMMs in the model
    dtype. Reads the per-expert row sets back to the host, so it is not
    capturable; moe_experts never routes here under graph capture.

    Same combine as the fused path (fp32 sum in ascending j, one rounding),
    but the GEMMs are hipBLASLt's: the down projection is rounded to bf16
    before the combine and its accumulation order follows the row count, so
    results agree with the fused path to bf16 tolerance, not bit for bit."""
    t, h = x.shape
    inter = w2.shape[2]
    k = ids.shape[1]
    y = torch.zeros(t, k, h, dtype=torch.float32, device=x.device)
    for e in range(w13.shape[0]):
        tok, choice = (ids == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        gu = torch.nn.functional.linear(x[tok], w13[e])
        act = silu_mul(gu[:, :inter].contiguous(), gu[:, inter:].contiguous())
        y[tok, choice] = torch.nn.functional.linear(act, w2[e]).float()
    out = torch.zeros(t, h, dtype=torch.float32, device=x.device)
    for j in range(k):
        out += weights[:, j, None] * y[:, j]
    return out.to(x.dtype)


def moe_experts(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor,
                ids: torch.Tensor, weights: torch.Tensor,
                block_m: Optional[int] = None) -> torch.Tensor:
    """Routed SwiGLU expert FFN: out[t] = sum_j weights[t, j] *
    (silu(x[t] @ Wg^T) * (x[t] @ Wu^T)) @ W2^T with the matrices of expert
    ids[t, j] -> [T, H] in x's dtype.

    x: [T, H]; w13: [E, 2I, H] (gate rows then up rows); w2: [E, H, I];
    ids int32 [T, k] and weights fp32 [T, k] from moe_route. The sum over j
    runs in fp32 in ascending j with one final rounding.

    Reference semantics (CPU path): an fp32 per-expert loop. GPU: bf16,
    H % 32 == 0, I % 32 == 0, k <= E <= 64, contiguous 16-byte-aligned
    operands, else RuntimeError. The fused path (csrc/moe.hip) is sync-free
    and is the only path under graph capture; it stores silu(g)*u once in
    bf16. ``block_m`` (16 or 64) forces its row block; None picks the path
    and block from the measured thresholds above.

    Bit-reproducibility and batch invariance (a token's output does not
    depend on the other rows) hold WITHIN the fused path, for either row
    block. Outside capture a call with T > MOE_FUSED_MAX runs the
    per-expert hipBLASLt loop instead, whose results agree to bf16
    tolerance only: a token's bits can change when its batch crosses that
    threshold (prefill vs decode), as they do for every dense projection
    that switches between skinny_linear and hipBLASLt.

    PRECONDITION: ids in [0, E). Not checked on the GPU (a device sync).
    No access goes out of bounds for a bad id, but moe_align drops that
    slot, its expert output is never written, and the token's result is
    then undefined (the fused path reads an uninitialised row).
    """
    if x.is_cuda:
        ext = _require_ext("moe_experts")
        if ext is not None:
            t = x.shape[0]
            if block_m is None:
                if (t > MOE_FUSED_MAX
                        and not torch.cuda.is_current_stream_capturing()):
                    _check_moe_shapes(x, w13, w2, ids)
                    return _moe_experts_loop(x, w13, w2, ids, weights)
                block_m = 16 if t <= MOE_BLOCK16_MAX else 64
            return ext.moe_experts(x, w13, w2, ids, weights, int(block_m))
    return _moe_experts_ref(x, w13, w2, ids, weights)


def _check_moe_shapes(x, w13, w2, ids) -> None:
    """The fused kernel's shape contract, held on the loop path too so that
    what a shape does never depends on T."""
    h, inter, e, k = x.shape[1], w2.shape[2], w13.shape[0], ids.shape[1]
    if h % 32 or inter % 32 or not (k <= e <= MOE_MAX_EXPERTS):
        raise RuntimeError(
            "moe_experts: need H % 32 == 0, I % 32 == 0 and k <= E <= {}, "
            "got H={} I={} E={} k={}".format(MOE_MAX_EXPERTS, h, inter, e, k))


def moe_ffn(x: torch.Tensor, router_weight: torch.Tensor, w13: torch.Tensor,
            w2: torch.Tensor, top_k: int,
            renormalize: bool = True) -> torch.Tensor:
    """Whole MoE block: router logits = x @ router_weight^T ([E, H]), then
    moe_route and moe_experts."""
    logits = torch.nn.functional.linear(x, router_weight)
    ids, weights = moe_route(logits, top_k, renormalize)
    return moe_experts(x, w13, w2, ids, weights)
