"""Mixture-of-experts serving, CPU side: the plain-PyTorch references in
ops (which define the kernels' semantics), the Mixtral converter against
transformers, and the engine running an MoE model."""

import asyncio

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine,
    LlmEngineConfig,
    SamplingParams,
)
from clearml_serving_amd.models.convert import convert_hf_auto
from clearml_serving_amd.models.llama import (
    PRESETS,
    LlamaConfig,
    LlamaForCausalLM,
)


def run(coro):
    loop = asyncio.new_event_loop()
    try:
        return loop.run_until_complete(coro)
    finally:
        pending = asyncio.all_tasks(loop)
        for t in pending:
            t.cancel()
        if pending:
            loop.run_until_complete(
                asyncio.gather(*pending, return_exceptions=True))
        loop.close()


def tie_free_logits(t, e, seed):
    """Per-row random permutation of arange(E) * 0.37: distinct values, so
    the selected experts are decided exactly."""
    g = torch.Generator().manual_seed(seed)
    base = torch.arange(e, dtype=torch.float32) * 0.37
    return torch.stack([base[torch.randperm(e, generator=g)]
                        for _ in range(t)])


def check_align(ids, num_experts, block_m, sorted_slots, block_expert):
    """The moe_align contract (shared with tests/test_moe_gpu.py)."""
    flat = ids.reshape(-1).tolist()
    s = len(flat)
    nb_max = (s + min(num_experts, s) * (block_m - 1)) // block_m
    assert sorted_slots.dtype == torch.int32
    assert block_expert.dtype == torch.int32
    assert sorted_slots.shape == (nb_max * block_m,)
    assert block_expert.shape == (nb_max,)
    slots = sorted_slots.tolist()
    experts = block_expert.tolist()
    real = [v for v in slots if v != s]
    assert sorted(real) == list(range(s)), "every slot exactly once"
    per_expert = {}
    seen_tail = False
    for b, e in enumerate(experts):
        rows = [v for v in slots[b * block_m:(b + 1) * block_m] if v != s]
        if e == -1:
            seen_tail = True
            assert rows == [], "unused block holds only sentinels"
            continue
        assert not seen_tail, "-1 blocks only trail"
        assert 0 <= e < num_experts and rows
        assert all(flat[v] == e for v in rows)
        per_expert.setdefault(e, []).extend(rows)
    for e, rows in per_expert.items():
        assert rows == sorted(rows), "slots ascend within expert %d" % e


# --------------------------------------------------------------------- #
# transformers parity
# --------------------------------------------------------------------- #
def _to_hub_layout(state, num_experts):
    """Rewrite transformers' in-memory Mixtral keys into the hub checkpoint
    layout (block_sparse_moe.gate / experts.{j}.w1|w3|w2)."""
    out = {}
    for key, v in state.items():
        if key.endswith("mlp.gate.weight"):
            out[key.replace("mlp.gate.", "block_sparse_moe.gate.")] = v
        elif key.endswith("mlp.experts.gate_up_proj"):
            p = key.replace("mlp.experts.gate_up_proj",
                            "block_sparse_moe.experts.")
            inter = v.shape[1] // 2
            for j in range(num_experts):
                out["{}{}.w1.weight".format(p, j)] = v[j, :inter].clone()
                out["{}{}.w3.weight".format(p, j)] = v[j, inter:].clone()
        elif key.endswith("mlp.experts.down_proj"):
            p = key.replace("mlp.experts.down_proj",
                            "block_sparse_moe.experts.")
            for j in range(num_experts):
                out["{}{}.w2.weight".format(p, j)] = v[j].clone()
        else:
            out[key] = v
    return out


def test_mixtral_matches_transformers():
    pytest.importorskip("transformers")
    from transformers import MixtralConfig, MixtralForCausalLM

    torch.manual_seed(3)
    hf = MixtralForCausalLM(MixtralConfig(
        vocab_size=128, hidden_size=64, intermediate_size=96,
        num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
        num_local_experts=4, num_experts_per_tok=2,
        max_position_embeddings=64, rope_theta=10000.0, rms_norm_eps=1e-5,
        sliding_window=None, tie_word_embeddings=False)).eval().float()
    cfg = LlamaConfig(vocab_size=128, hidden=64, layers=2, heads=4,
                      kv_heads=2, intermediate=96, rope_theta=10000.0,
                      rms_eps=1e-5, max_position=64, num_experts=4,
                      experts_per_tok=2)
    ids = torch.tensor([3, 17, 99, 4, 56, 23, 8, 120, 64, 1, 77, 5])
    t = ids.shape[0]
    positions = torch.arange(t, dtype=torch.int32)
    attn_ctx = {"mode": "prefill", "batch": 1, "seq": t,
                "seq_lens": torch.tensor([t], dtype=torch.int32),
                "slot_mapping": torch.full((t,), -1, dtype=torch.int32)}
    with torch.inference_mode():
        ref = hf(input_ids=ids[None]).logits[0]
    state = dict(hf.state_dict())
    assert any(k.endswith("mlp.experts.gate_up_proj") for k in state), \
        "expected transformers' stacked in-memory expert layout"
    hub = _to_hub_layout(state, 4)
    assert any(".block_sparse_moe.experts.3.w3.weight" in k for k in hub)
    for layout in (state, hub):
        ours = LlamaForCausalLM(cfg).eval()
        ours.load_state_dict(convert_hf_auto(layout))
        with torch.inference_mode():
            got = ours(ids, positions, kv_caches=None, attn_ctx=attn_ctx)
        torch.testing.assert_close(got, ref, atol=3e-4, rtol=3e-4)


# --------------------------------------------------------------------- #
# route reference
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("t,e,k", [(1, 4, 2), (5, 8, 2), (67, 60, 4),
                                   (5, 64, 8)])
def test_route_reference_is_softmax_topk(t, e, k):
    logits = tie_free_logits(t, e, seed=t * 100 + e)
    ids, w = ops.moe_route(logits, k, renormalize=True)
    assert ids.dtype == torch.int32 and ids.shape == (t, k)
    assert w.dtype == torch.float32 and w.shape == (t, k)
    top = torch.topk(torch.softmax(logits, dim=-1), k, dim=-1)
    assert torch.equal(ids.long(), top.indices)
    torch.testing.assert_close(
        w, top.values / top.values.sum(-1, keepdim=True))
    torch.testing.assert_close(w.sum(-1), torch.ones(t))
    assert (w[:, :-1] >= w[:, 1:]).all(), "descending probability"
    ids_raw, w_raw = ops.moe_route(logits, k, renormalize=False)
    assert torch.equal(ids_raw, ids)
    torch.testing.assert_close(w_raw, top.values)


def test_route_reference_ties_take_lowest_index():
    logits = torch.tensor([[1.0, 2.0, 2.0, 0.5, 2.0, -1.0],
                           [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    ids, w = ops.moe_route(logits, 2, renormalize=True)
    assert ids.tolist() == [[1, 2], [0, 1]]
    torch.testing.assert_close(w, torch.full((2, 2), 0.5))
    ids3, _ = ops.moe_route(logits.to(torch.bfloat16), 3)
    assert ids3.tolist() == [[1, 2, 4], [0, 1, 2]]


@pytest.mark.parametrize("e,k", [(4, 0), (4, 5), (65, 2), (64, 9)])
def test_route_reference_refuses_unsupported(e, k):
    with pytest.raises(RuntimeError):
        ops.moe_route(torch.zeros(3, e), k)


# --------------------------------------------------------------------- #
# align reference
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("block_m", [16, 64])
@pytest.mark.parametrize("e,k", [(4, 2), (8, 2), (60, 4)])
@pytest.mark.parametrize("t", [1, 5, 67])
def test_align_reference_invariants(t, e, k, block_m):
    ids, _ = ops.moe_route(tie_free_logits(t, e, seed=7 * t + e), k)
    sorted_slots, block_expert = ops.moe_align(ids, e, block_m)
    check_align(ids, e, block_m, sorted_slots, block_expert)


def test_align_reference_skewed_and_exact_layout():
    # 5 slots: expert 2 gets slots 0, 2, 3; expert 0 gets 1, 4; 1 is empty
    ids = torch.tensor([[2], [0], [2], [2], [0]], dtype=torch.int32)
    sorted_slots, block_expert = ops.moe_align(ids, 3, 2)
    # NB_max = (5 + 3*1) // 2 = 4 blocks: e0 [1,4] | e2 [0,2] [3,S] | unused
    assert sorted_slots.tolist() == [1, 4, 0, 2, 3, 5, 5, 5]
    assert block_expert.tolist() == [0, 2, 2, -1]


# --------------------------------------------------------------------- #
# experts reference
# --------------------------------------------------------------------- #
def test_experts_reference_matches_dense_formula():
    torch.manual_seed(0)
    t, h, inter, e, k = 9, 32, 64, 4, 2
    x = torch.randn(t, h)
    w13 = torch.randn(e, 2 * inter, h) * h ** -0.5
    w2 = torch.randn(e, h, inter) * inter ** -0.5
    router = torch.randn(e, h)
    ids, w = ops.moe_route(x @ router.t(), k)
    got = ops.moe_experts(x, w13, w2, ids, w)
    want = torch.zeros(t, h)
    for i in range(t):
        for j in range(k):
            ex = int(ids[i, j])
            gu = w13[ex] @ x[i]
            act = torch.nn.functional.silu(gu[:inter]) * gu[inter:]
            want[i] += w[i, j] * (w2[ex] @ act)
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(ops.moe_ffn(x, router, w13, w2, k), got)


# --------------------------------------------------------------------- #
# model + engine
# --------------------------------------------------------------------- #
def test_dense_models_are_untouched():
    cfg = LlamaConfig(vocab_size=64, hidden=32, layers=2, heads=4,
                      kv_heads=2, intermediate=64, max_position=32)
    assert cfg.num_experts == 0
    keys = set(LlamaForCausalLM(cfg).state_dict().keys())
    want = {"embed.weight", "final_norm", "lm_head.weight"}
    for i in range(2):
        want |= {"layers.{}.{}".format(i, n) for n in (
            "attn_norm", "qkv.weight", "o_proj.weight", "mlp_norm",
            "gate_up.weight", "down.weight")}
    assert keys == want
    assert LlamaConfig().num_experts == 0  # the default preset stays dense


def test_moe_model_layout_and_init():
    cfg = PRESETS["mixtral-tiny"]
    assert (cfg.num_experts, cfg.experts_per_tok) == (4, 2)
    big = PRESETS["mixtral-8x7b"]
    assert (big.vocab_size, big.hidden, big.layers, big.heads, big.kv_heads,
            big.intermediate, big.num_experts, big.experts_per_tok,
            big.max_position) == (32000, 4096, 32, 32, 8, 14336, 8, 2, 32768)
    model = LlamaForCausalLM(cfg)
    state = model.state_dict()
    assert state["layers.0.router.weight"].shape == (4, 256)
    assert state["layers.1.w13"].shape == (4, 1024, 256)
    assert state["layers.1.w2"].shape == (4, 256, 512)
    assert "layers.0.gate_up.weight" not in state
    for name in ("layers.0.w13", "layers.1.w2"):
        std = float(state[name].std())
        assert 0.015 < std < 0.025, (name, std)  # normal(0, 0.02), not empty


def _moe_engine(**kw):
    return LlmEngine(LlmEngineConfig(
        preset="mixtral-tiny", num_kv_blocks=64, block_size=16,
        max_model_len=128, device="cpu", dtype="float32", **kw))


def test_moe_engine_cpu_decode_matches_prefill():
    eng = _moe_engine()
    eng.start()
    assert eng.model_config.num_experts == 4
    prompt = [3, 7, 11, 19, 23, 29, 31, 37]

    async def gen():
        seq = await eng.add_request(
            list(prompt), SamplingParams(temperature=0.0, max_tokens=8,
                                         ignore_eos=True))
        toks = []
        while True:
            item = await seq.stream.get()
            toks.extend(item["token_ids"])
            if item["finished"]:
                return toks

    generated = run(gen())
    assert len(generated) == 8
    full = prompt + generated
    t = len(full)
    attn_ctx = {"mode": "prefill", "batch": 1, "seq": t,
                "seq_lens": torch.tensor([t], dtype=torch.int32),
                "slot_mapping": torch.full((t,), -1, dtype=torch.int32)}
    with torch.inference_mode():
        logits = eng.model(torch.tensor(full),
                           torch.arange(t, dtype=torch.int32),
                           kv_caches=None, attn_ctx=attn_ctx)
    # fp32 on both sides: each decode step picked the teacher-forced argmax
    # (a margin below fp32 noise counts as a tie)
    for step in range(8):
        top2 = logits[len(prompt) + step - 1].topk(2)
        assert generated[step] == int(top2.indices[0]) or \
            float(top2.values[0] - top2.values[1]) < 1e-4
    assert eng.allocator.available == eng.allocator.num_blocks


def test_moe_engine_overrides_declare_any_size():
    eng = _moe_engine(overrides={"num_experts": 6, "experts_per_tok": 3,
                                 "norm_topk_prob": False,
                                 "sliding_window": None})
    eng.start()
    assert eng.model_config.num_experts == 6
    assert eng.model.layers[0].w13.shape[0] == 6
    dense = LlmEngine(LlmEngineConfig(
        preset="llama-tiny", num_kv_blocks=16, device="cpu",
        dtype="float32", overrides={"num_experts": 4}))
    dense.start()
    assert hasattr(dense.model.layers[0], "router")


def test_moe_engine_refuses_unimplemented_combinations(monkeypatch):
    with pytest.raises(ValueError, match="fp8"):
        _moe_engine(quantization="fp8").start()
    with pytest.raises(ValueError, match="lora_modules"):
        _moe_engine(lora_modules=[{"name": "a", "path": "/nonexistent"}]
                    ).start()
    with pytest.raises(ValueError, match="sliding_window"):
        _moe_engine(overrides={"sliding_window": 4096}).start()
    from clearml_serving_amd.parallel import tp as tp_mod

    monkeypatch.setattr(tp_mod, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="tensor parallelism"):
        _moe_engine().start()
