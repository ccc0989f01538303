"""Rotary frequency tables for the scaled-RoPE model families.

``rope_inv_freq`` turns a HuggingFace ``rope_scaling`` / ``rope_parameters``
dict into the float32 ``inv_freq`` table ([head_dim / 2]) and the attention
factor that ``ops.qk_rope_kv`` consumes. The formulas follow
``transformers.modeling_rope_utils`` (pinned against it in
tests/test_rope_scaling_cpu.py); the arithmetic runs in float64 on the host
and is rounded to float32 once.

Supported: no scaling, ``linear``, ``llama3`` (Llama-3.1/3.2) and ``yarn``.
``dynamic`` and ``longrope`` change the table with the running sequence
length, which a table fixed at load time cannot express: they raise.
"""

import math
from typing import Optional, Tuple

import torch


def _scaling_type(scaling: Optional[dict]) -> str:
    if not scaling:
        return "default"
    return str(scaling.get("rope_type", scaling.get("type", "default")))


def _llama3(inv_freq: torch.Tensor, s: dict) -> torch.Tensor:
    factor = float(s["factor"])
    low, high = float(s["low_freq_factor"]), float(s["high_freq_factor"])
    old_len = float(s["original_max_position_embeddings"])
    wavelen = 2 * math.pi / inv_freq
    # three bands: short wavelengths stay, long ones divide by factor, the
    # band between blends the two
    scaled = torch.where(wavelen > old_len / low, inv_freq / factor, inv_freq)
    smooth = (old_len / wavelen - low) / (high - low)
    blended = (1 - smooth) * scaled / factor + smooth * scaled
    medium = ~(wavelen < old_len / high) & ~(wavelen > old_len / low)
    return torch.where(medium, blended, scaled)


def _yarn_mscale(scale: float, mscale: float = 1.0) -> float:
    return 1.0 if scale <= 1 else 0.1 * mscale * math.log(scale) + 1.0


def _yarn(inv_freq: torch.Tensor, s: dict, dim: int,
          theta: float) -> Tuple[torch.Tensor, float]:
    factor = float(s["factor"])
    attn = s.get("attention_factor")
    if attn is None:
        if s.get("mscale") and s.get("mscale_all_dim"):
            attn = (_yarn_mscale(factor, s["mscale"])
                    / _yarn_mscale(factor, s["mscale_all_dim"]))
        else:
            attn = _yarn_mscale(factor)
    beta_fast = s.get("beta_fast") or 32
    beta_slow = s.get("beta_slow") or 1
    old_len = s["original_max_position_embeddings"]

    def correction_dim(rotations):
        return (dim * math.log(old_len / (rotations * 2 * math.pi))
                / (2 * math.log(theta)))

    lo, hi = correction_dim(beta_fast), correction_dim(beta_slow)
    if s.get("truncate", True):
        lo, hi = math.floor(lo), math.ceil(hi)
    lo, hi = max(lo, 0), min(hi, dim - 1)
    if lo == hi:
        hi += 0.001  # no singular ramp
    ramp = ((torch.arange(dim // 2, dtype=torch.float64) - lo)
            / (hi - lo)).clamp(0, 1)
    extrapolation = 1 - ramp  # 1 where the original frequency is kept
    out = inv_freq / factor * (1 - extrapolation) + inv_freq * extrapolation
    return out, float(attn)


def rope_inv_freq(head_dim: int, theta: float, scaling: Optional[dict],
                  max_position: int) -> Tuple[torch.Tensor, float]:
    """(inv_freq float32 [head_dim / 2], attn_factor) for a rope_scaling
    dict (None = plain RoPE). ``max_position`` stands in for a missing
    ``original_max_position_embeddings``."""
    kind = _scaling_type(scaling)
    inv_freq = 1.0 / (float(theta) ** (
        torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    attn = 1.0
    if kind == "default":
        pass
    elif kind == "linear":
        inv_freq = inv_freq / float(scaling["factor"])
    elif kind in ("llama3", "yarn"):
        s = dict(scaling)
        s.setdefault("original_max_position_embeddings", max_position)
        if kind == "llama3":
            inv_freq = _llama3(inv_freq, s)
        else:
            inv_freq, attn = _yarn(inv_freq, s, head_dim, float(theta))
    else:
        raise ValueError(
            "rope scaling type '{}' is not supported (the table is fixed at "
            "load time; supported: linear, llama3, yarn)".format(kind))
    return inv_freq.to(torch.float32), attn
