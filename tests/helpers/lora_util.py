"""Shared fixtures for the multi-LoRA tests: write PEFT-layout adapters for
a llama preset and drive an engine with a mixed-adapter batch."""

import asyncio
import json
import os

import torch
from safetensors.torch import save_file

from clearml_serving_amd.engines.llm.engine import SamplingParams
from clearml_serving_amd.models.lora import projection_shapes

_PEFT_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn",
                "v_proj": "self_attn", "o_proj": "self_attn",
                "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}
_PART = {"q_proj": ("qkv", 0), "k_proj": ("qkv", 1), "v_proj": ("qkv", 2),
         "o_proj": ("o_proj", 0), "gate_proj": ("gate_up", 0),
         "up_proj": ("gate_up", 1), "down_proj": ("down", 0)}

ATTN_ONLY = ["q_proj", "k_proj", "v_proj", "o_proj"]
ALL_LINEAR = ATTN_ONLY + ["gate_proj", "up_proj", "down_proj"]


def write_adapter(path, mcfg, targets, r=8, alpha=16, seed=0, std=0.05,
                  config_extra=None, tensors_extra=None):
    """PEFT adapter directory (adapter_config.json +
    adapter_model.safetensors) with random NON-zero A and B, so the
    adapter visibly changes the model."""
    os.makedirs(path, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    shapes = projection_shapes(mcfg)
    tensors = {}
    for layer in range(mcfg.layers):
        for mod in targets:
            proj, part = _PART[mod]
            k, parts = shapes[proj]
            base = "base_model.model.model.layers.{}.{}.{}.".format(
                layer, _PEFT_PARENT[mod], mod)
            tensors[base + "lora_A.weight"] = \
                torch.randn(r, k, generator=g) * std
            tensors[base + "lora_B.weight"] = \
                torch.randn(parts[part], r, generator=g) * std
    tensors.update(tensors_extra or {})
    save_file(tensors, os.path.join(path, "adapter_model.safetensors"))
    cfg = {"peft_type": "LORA", "r": r, "lora_alpha": alpha,
           "target_modules": list(targets), "bias": "none",
           "use_dora": False, "modules_to_save": None}
    cfg.update(config_extra or {})
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(cfg, f)
    return path


def run(coro):
    loop = asyncio.new_event_loop()
    try:
        return loop.run_until_complete(coro)
    finally:
        loop.close()


def generate_batch(eng, prompts, loras, max_tokens=8, logprobs=None):
    """Submit all prompts at once (one batch); returns per request
    (token ids, per-token stream items)."""
    async def go():
        outs = [[] for _ in prompts]
        items = [[] for _ in prompts]

        async def one(i):
            kw = {}
            if loras[i] is not None:
                kw["lora_idx"] = loras[i]
            seq = await eng.add_request(list(prompts[i]), SamplingParams(
                temperature=0.0, max_tokens=max_tokens, ignore_eos=True,
                logprobs=logprobs), **kw)
            while True:
                item = await seq.stream.get()
                assert not item.get("error"), item
                outs[i].extend(item["token_ids"])
                items[i].append(item)
                if item["finished"]:
                    return

        await asyncio.gather(*[one(i) for i in range(len(prompts))])
        return outs, items

    return run(go())
