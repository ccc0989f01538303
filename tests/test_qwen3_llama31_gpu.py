"""qwen3-tiny and llama-3.1-tiny through the engine on gfx950: prefill,
chunked prefill and decode graphs all run ops.qk_rope_kv (q/k norm, the
llama3 frequency table, bf16 and fp8 KV caches). Greedy generation must match
the fp32 CPU forward of the same weights token for token. The prompts are
seeded so that the CPU reference's top-2 logit gap stays above 0.08 at every
step (found on the CPU, asserted below): far above the bf16 noise of logits
that are ~0.3 in magnitude."""

import asyncio

import pytest
import torch

from clearml_serving_amd.engines.llm.engine import (
    LlmEngine, LlmEngineConfig, SamplingParams)
from clearml_serving_amd.models.llama import LlamaForCausalLM

pytestmark = pytest.mark.gpu

PROMPT_LEN, STEPS = 40, 44  # positions pass llama-3.1-tiny's original max 32
PROMPT_SEED = {"qwen3-tiny": 74, "llama-3.1-tiny": 27}


@pytest.mark.parametrize("kv_dtype", ["bfloat16", "fp8"])
@pytest.mark.parametrize("preset", sorted(PROMPT_SEED))
def test_engine_matches_cpu_forward(preset, kv_dtype):
    g = torch.Generator().manual_seed(PROMPT_SEED[preset])
    prompt = torch.randint(0, 512, (PROMPT_LEN,), generator=g).tolist()
    eng = LlmEngine(LlmEngineConfig(
        preset=preset, num_kv_blocks=16, block_size=16, max_model_len=128,
        device="cuda:0", max_num_seqs=4, prefill_chunk=16, kv_dtype=kv_dtype))
    eng.start()
    assert eng.model_config.fused_qk_rope

    async def go():
        seq = await eng.add_request(list(prompt), SamplingParams(
            temperature=0.0, max_tokens=STEPS, ignore_eos=True))
        toks = []
        while True:
            item = await seq.stream.get()
            assert "error" not in item, item
            toks.extend(item["token_ids"])
            if item["finished"]:
                return toks

    toks = asyncio.new_event_loop().run_until_complete(go())
    assert len(toks) == STEPS and eng.stats["graph_replays"] > 0

    # teacher-forced fp32 CPU forward over prompt + generated tokens: its
    # argmax at every step is the CPU's own greedy continuation
    ref = LlamaForCausalLM(eng.model_config).eval()
    ref.load_state_dict({k: v.float().cpu()
                         for k, v in eng.model.state_dict().items()})
    t = PROMPT_LEN + STEPS - 1
    ctx = {"mode": "prefill", "batch": 1, "seq": t,
           "seq_lens": torch.tensor([t], dtype=torch.int32),
           "slot_mapping": torch.full((t,), -1, dtype=torch.int32)}
    with torch.inference_mode():
        logits = ref(torch.tensor(prompt + toks[:-1]),
                     torch.arange(t, dtype=torch.int32), kv_caches=None,
                     attn_ctx=ctx)[PROMPT_LEN - 1:]
    top = logits.topk(2)
    assert top.indices[:, 0].tolist() == toks
    assert (top.values[:, 0] - top.values[:, 1]).min() > 0.08
