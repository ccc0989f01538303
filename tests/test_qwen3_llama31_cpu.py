"""Qwen3 (q/k norm, head_dim of its own) and Llama-3.1 (rope_scaling llama3)
against random-init transformers models: config.json -> LlamaConfig, convert,
full logits in fp32, at the tolerance tests/test_hf_convert.py applies to
Qwen2."""

import pytest
import torch
import transformers

from clearml_serving_amd.models.convert import (convert_hf_auto,
                                                llama_config_from_hf)
from clearml_serving_amd.models.llama import LlamaForCausalLM

COMMON = dict(vocab_size=160, hidden_size=64, intermediate_size=96,
              num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=2, max_position_embeddings=256,
              attention_dropout=0.0, tie_word_embeddings=False,
              use_cache=False, attn_implementation="eager")
# Qwen3: head_dim 32 with hidden 64 / 4 heads = 16, so the override is needed.
# Llama-3.1: original max 32, sequence 96, so all three bands are reached.
CASES = {
    "Qwen3": (dict(head_dim=32, rms_norm_eps=1e-6, rope_parameters={
        "rope_type": "default", "rope_theta": 1e6}), 12, 32),
    "Llama": (dict(rms_norm_eps=1e-5, rope_parameters={
        "rope_type": "llama3", "rope_theta": 10000.0, "factor": 8.0,
        "low_freq_factor": 1.0, "high_freq_factor": 4.0,
        "original_max_position_embeddings": 32}), 96, 16),
}


@pytest.mark.parametrize("family", sorted(CASES))
def test_logits_match_transformers(family):
    extra, t, head_dim = CASES[family]
    torch.manual_seed(6)
    hf = getattr(transformers, family + "ForCausalLM")(
        getattr(transformers, family + "Config")(**COMMON, **extra)).eval()
    state = dict(hf.state_dict())
    for key in state:  # norm weights init to ones: make them matter
        if "q_norm" in key or "k_norm" in key:
            state[key].uniform_(0.5, 1.5)
    cfg = llama_config_from_hf(hf.config.to_dict())
    assert cfg.head_dim == head_dim and cfg.qk_norm == (family == "Qwen3")
    ours = LlamaForCausalLM(cfg).eval()
    ours.load_state_dict(convert_hf_auto(state))

    ids = torch.randint(0, 160, (t,))
    attn_ctx = {"mode": "prefill", "batch": 1, "seq": t,
                "seq_lens": torch.tensor([t], dtype=torch.int32),
                "slot_mapping": torch.full((t,), -1, dtype=torch.int32)}
    with torch.inference_mode():
        ref = hf(input_ids=ids[None]).logits[0]
        got = ours(ids, torch.arange(t, dtype=torch.int32), kv_caches=None,
                   attn_ctx=attn_ctx)
    torch.testing.assert_close(got, ref, atol=3e-4, rtol=3e-4)
