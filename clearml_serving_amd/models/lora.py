"""LoRA adapters for the llama family: PEFT loading, the per-engine adapter
bank the batched kernels read (ops.lora_shrink / ops.lora_expand_add), and an
offline merge.

The reference serves adapters through vLLM's ``lora_modules``
(preprocess_service.py:715-720). Here an adapter is mapped onto the MERGED
projections of models/llama.py (layout of models/convert.py: ``qkv`` is
[q;k;v], ``gate_up`` is [gate;up]) so the kernels see one plain
``A [L, R, K]`` / ``B [L, N, R]`` pair per projection:

- the A matrices of the merged parts stack along rank (R = 3*Rp for qkv,
  2*Rp for gate_up, Rp = max_lora_rank rounded up to 16);
- B is block-diagonal: part p's rows carry its B in columns [p*Rp, p*Rp+r),
  zeros elsewhere; ``alpha/r`` is folded into B;
- ranks below Rp pad with zeros; a module the adapter does not target is an
  all-zero slot.

Not supported (ValueError at load): bias terms, DoRA, ``modules_to_save``,
embedding / lm_head targets, per-module rank or alpha patterns, ranks above
``max_lora_rank``. ``peft`` itself is not needed.
"""

import json
import math
import os
import re
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch

from .llama import LlamaConfig

PROJECTIONS = ("qkv", "o_proj", "gate_up", "down")

# PEFT target module -> (merged projection, part index inside it)
_TARGETS = {
    "q_proj": ("qkv", 0), "k_proj": ("qkv", 1), "v_proj": ("qkv", 2),
    "o_proj": ("o_proj", 0),
    "gate_proj": ("gate_up", 0), "up_proj": ("gate_up", 1),
    "down_proj": ("down", 0),
}
_KEY_RE = re.compile(
    r"^base_model\.model\.model\.layers\.(\d+)\.(?:self_attn|mlp)\."
    r"(\w+)\.lora_([AB])\.weight$")
_KERNEL_MAX_RANK = 256  # ops/csrc/lora.hip


@dataclass
class LoraAdapter:
    name: str
    path: str
    r: int
    scale: float  # alpha / r
    # (layer, target module) -> (A [r, K], B [N_part, r]) fp32, unscaled
    tensors: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]] = \
        field(default_factory=dict)


def projection_shapes(mcfg: LlamaConfig) -> Dict[str, Tuple[int, List[int]]]:
    """Merged projection -> (K, output sizes of its parts)."""
    q_out = mcfg.heads * mcfg.head_dim
    kv_out = mcfg.kv_heads * mcfg.head_dim
    return {
        "qkv": (mcfg.hidden, [q_out, kv_out, kv_out]),
        "o_proj": (q_out, [mcfg.hidden]),
        "gate_up": (mcfg.hidden, [mcfg.intermediate, mcfg.intermediate]),
        "down": (mcfg.intermediate, [mcfg.hidden]),
    }


def load_adapter(path: str, max_lora_rank: int = 16,
                 name: str = None) -> LoraAdapter:
    """Read a PEFT adapter directory (adapter_config.json +
    adapter_model.safetensors)."""
    from safetensors.torch import load_file

    name = name or os.path.basename(os.path.normpath(path))
    with open(os.path.join(path, "adapter_config.json")) as f:
        cfg = json.load(f)

    def bad(msg):
        return ValueError("LoRA adapter '{}' ({}): {}".format(name, path, msg))

    if str(cfg.get("peft_type", "LORA")).upper() != "LORA":
        raise bad("peft_type '{}' is not LORA".format(cfg.get("peft_type")))
    if cfg.get("bias", "none") not in (None, "none"):
        raise bad("bias='{}' is not supported (bias terms)".format(
            cfg["bias"]))
    if cfg.get("use_dora"):
        raise bad("DoRA is not supported")
    if cfg.get("modules_to_save"):
        raise bad("modules_to_save {} is not supported".format(
            cfg["modules_to_save"]))
    if cfg.get("rank_pattern") or cfg.get("alpha_pattern"):
        raise bad("rank_pattern / alpha_pattern are not supported")
    targets = cfg.get("target_modules")
    if not isinstance(targets, (list, tuple)) or not targets:
        raise bad("target_modules must be a list of module names")
    for t in targets:
        if t not in _TARGETS:
            raise bad("target module '{}' is not supported (embedding and "
                      "lm_head adapters are out of scope; have: {})".format(
                          t, sorted(_TARGETS)))
    r = int(cfg["r"])
    if r < 1:
        raise bad("rank must be >= 1, got {}".format(r))
    if r > max_lora_rank:
        raise bad("rank {} exceeds max_lora_rank {}".format(r, max_lora_rank))
    alpha = float(cfg.get("lora_alpha", r))
    scale = alpha / math.sqrt(r) if cfg.get("use_rslora") else alpha / r

    halves: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
    for key, t in load_file(
            os.path.join(path, "adapter_model.safetensors")).items():
        m = _KEY_RE.match(key)
        if m is None or m.group(2) not in targets:
            raise bad("unsupported tensor '{}' (only lora_A / lora_B weights "
                      "of the target projections are)".format(key))
        halves.setdefault((int(m.group(1)), m.group(2)), {})[m.group(3)] = \
            t.float()
    adapter = LoraAdapter(name=name, path=path, r=r, scale=scale)
    for (layer, mod), ab in halves.items():
        if set(ab) != {"A", "B"}:
            raise bad("layer {} {} lacks lora_A or lora_B".format(layer, mod))
        a, b = ab["A"], ab["B"]
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != r or b.shape[1] != r:
            raise bad("layer {} {}: lora_A {} / lora_B {} do not match "
                      "r={}".format(layer, mod, tuple(a.shape),
                                    tuple(b.shape), r))
        adapter.tensors[(layer, mod)] = (a, b)
    return adapter


def _check_shapes(adapter: LoraAdapter, mcfg: LlamaConfig) -> None:
    shapes = projection_shapes(mcfg)
    for (layer, mod), (a, b) in adapter.tensors.items():
        proj, part = _TARGETS[mod]
        k, parts = shapes[proj]
        if layer >= mcfg.layers or a.shape[1] != k \
                or b.shape[0] != parts[part]:
            raise ValueError(
                "LoRA adapter '{}': layer {} {} (A {}, B {}) does not fit "
                "the base model ({} layers, expects A [r, {}], B [{}, r])"
                .format(adapter.name, layer, mod, tuple(a.shape),
                        tuple(b.shape), mcfg.layers, k, parts[part]))


class LoraBank:
    """All adapters of one engine, stacked per layer and merged projection
    on the engine device: ``layer(i, proj) -> (A [L, R, K], B [L, N, R])``.
    ``index`` maps adapter name -> slot (the per-token idx the kernels
    take; -1 is the base model)."""

    def __init__(self, adapters: List[LoraAdapter], mcfg: LlamaConfig,
                 max_lora_rank: int, device, dtype):
        if not adapters:
            raise ValueError("LoraBank needs at least one adapter")
        self.rank_pad = -(-int(max_lora_rank) // 16) * 16
        if 3 * self.rank_pad > _KERNEL_MAX_RANK:
            raise ValueError(
                "max_lora_rank {} is too large: the stacked qkv rank "
                "3*{} exceeds the kernel limit {}".format(
                    max_lora_rank, self.rank_pad, _KERNEL_MAX_RANK))
        self.names = [a.name for a in adapters]
        if len(set(self.names)) != len(self.names):
            raise ValueError("duplicate LoRA adapter names: {}".format(
                self.names))
        self.index = {n: i for i, n in enumerate(self.names)}
        self.paths = [a.path for a in adapters]
        # prefix-cache salt per slot: KV content depends on the adapter
        # (0 is reserved for the base model)
        self.salts = [hash(("lora", n)) or 1 for n in self.names]
        shapes = projection_shapes(mcfg)
        rp = self.rank_pad
        self._layers: List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = []
        for a in adapters:
            if a.r > max_lora_rank:
                raise ValueError(
                    "LoRA adapter '{}': rank {} exceeds max_lora_rank {}"
                    .format(a.name, a.r, max_lora_rank))
            _check_shapes(a, mcfg)
        for layer in range(mcfg.layers):
            entry = {}
            for proj in PROJECTIONS:
                k, parts = shapes[proj]
                A = torch.zeros(len(adapters), len(parts) * rp, k)
                B = torch.zeros(len(adapters), sum(parts), len(parts) * rp)
                for slot, ad in enumerate(adapters):
                    for mod, (p, part) in _TARGETS.items():
                        if p != proj or (layer, mod) not in ad.tensors:
                            continue
                        a, b = ad.tensors[(layer, mod)]
                        row = sum(parts[:part])
                        A[slot, part * rp:part * rp + ad.r] = a
                        B[slot, row:row + parts[part],
                          part * rp:part * rp + ad.r] = b * ad.scale
                entry[proj] = (A.to(device=device, dtype=dtype).contiguous(),
                               B.to(device=device, dtype=dtype).contiguous())
            self._layers.append(entry)

    def __len__(self) -> int:
        return len(self.names)

    def layer(self, i: int, proj: str) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._layers[i][proj]


def merge_adapter(state_dict: Dict[str, torch.Tensor], adapter: LoraAdapter,
                  mcfg: LlamaConfig) -> Dict[str, torch.Tensor]:
    """Base weights (native or HuggingFace llama layout) with
    ``W + (alpha/r) * B @ A`` folded into every targeted projection; the
    result loads into LlamaForCausalLM as a stand-alone fine-tune."""
    from .convert import convert_hf_auto

    _check_shapes(adapter, mcfg)
    out = dict(convert_hf_auto(state_dict))
    shapes = projection_shapes(mcfg)
    for (layer, mod), (a, b) in adapter.tensors.items():
        proj, part = _TARGETS[mod]
        parts = shapes[proj][1]
        key = "layers.{}.{}.weight".format(layer, proj)
        w = out[key].float().clone()
        row = sum(parts[:part])
        w[row:row + parts[part]] += adapter.scale * (b @ a)
        out[key] = w.to(out[key].dtype)
    return out
