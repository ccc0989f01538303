"""Multi-LoRA serving on the CPU path: op references, PEFT loading, the model
hook against offline-merged weights, engine routing / scheduling paths,
prefix-cache isolation, the OpenAI surface and config errors."""

import os
import sys

import pytest
import torch
from safetensors.torch import save_file

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine, LlmEngineConfig, PrefixCacheAllocator, Sequence)
from clearml_serving_amd.models.llama import PRESETS, LlamaForCausalLM
from clearml_serving_amd.models.lora import (
    LoraBank, load_adapter, merge_adapter)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))
import lora_util  # noqa: E402
from lora_util import run  # noqa: E402

MCFG = PRESETS["llama-tiny"]
# fixed seeds (adapters + prompts), chosen so that every greedy step of the
# merged-weight oracle has a top-2 logprob gap > 1e-3: an argmax near-tie
# could legitimately flip between W x + B(A x) and (W + BA) x
AD1_SEED, AD2_SEED = 1, 2
PROMPTS = [[(5 + 3 * j) % 500 for j in range(19)],
           [(11 + 7 * j) % 500 for j in range(23)],
           [(2 + 13 * j * j) % 500 for j in range(21)]]
LORAS = [-1, 0, 1]  # base, adapter 1, adapter 2
MAX_TOKENS = 12


# --------------------------------------------------------------------- #
# ops: CPU reference == explicit per-token loop
# --------------------------------------------------------------------- #
def test_ops_reference_matches_explicit_loop():
    g = torch.Generator().manual_seed(0)
    t, k, n, r, nl = 7, 24, 40, 16, 3
    x = torch.randn(t, k, generator=g)
    a = torch.randn(nl, r, k, generator=g)
    b = torch.randn(nl, n, r, generator=g)
    out0 = torch.randn(t, n, generator=g)
    idx = torch.tensor([0, -1, 2, 2, 1, -1, 0], dtype=torch.int32)

    y = ops.lora_shrink(x, a, idx)
    assert y.dtype == torch.float32 and tuple(y.shape) == (t, r)
    y_in = y.clone()
    y_in[idx < 0] = float("nan")  # skipped rows of y are never read
    out = out0.clone()
    ret = ops.lora_expand_add(y_in, b, idx, out)
    assert ret is out
    for i in range(t):
        if idx[i] < 0:
            assert torch.equal(out[i], out0[i])
            continue
        yi = a[idx[i]] @ x[i]
        torch.testing.assert_close(y[i], yi, atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(out[i], out0[i] + b[idx[i]] @ yi,
                                   atol=1e-4, rtol=1e-5)


def test_ops_reference_rounds_once_in_bf16():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 16, generator=g).to(torch.bfloat16)
    a = torch.randn(2, 16, 16, generator=g).to(torch.bfloat16)
    b = torch.randn(2, 8, 16, generator=g).to(torch.bfloat16)
    out0 = torch.randn(3, 8, generator=g).to(torch.bfloat16)
    idx = torch.tensor([1, -1, 0], dtype=torch.int32)
    out = out0.clone()
    ops.lora_expand_add(ops.lora_shrink(x, a, idx), b, idx, out)
    assert out.dtype == torch.bfloat16
    for i in (0, 2):
        want = (out0[i].float()
                + b[idx[i]].float() @ (a[idx[i]].float() @ x[i].float()))
        assert torch.equal(out[i], want.to(torch.bfloat16))
    assert torch.equal(out[1], out0[1])


# --------------------------------------------------------------------- #
# fixtures: two adapters with different targets, merged-weight oracles
# --------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    root = tmp_path_factory.mktemp("lora")
    lora_util.write_adapter(str(root / "ad1"), MCFG, lora_util.ALL_LINEAR,
                            r=8, alpha=16, seed=AD1_SEED)
    lora_util.write_adapter(str(root / "ad2"), MCFG, lora_util.ATTN_ONLY,
                            r=8, alpha=4, seed=AD2_SEED)
    return [{"name": "ad1", "path": str(root / "ad1")},
            {"name": "ad2", "path": str(root / "ad2")}]


def lora_engine(adapters, **kw) -> LlmEngine:
    defaults = dict(preset="llama-tiny", num_kv_blocks=128, block_size=16,
                    max_model_len=256, device="cpu", lora_modules=adapters)
    eng = LlmEngine(LlmEngineConfig(**{**defaults, **kw}))
    eng.start()
    return eng


@pytest.fixture(scope="module")
def oracle(adapters, tmp_path_factory):
    """Greedy tokens of three single-model engines (base, base merged with
    adapter 1, base merged with adapter 2) for PROMPTS[i], plus the proof
    that no step was an argmax near-tie."""
    root = tmp_path_factory.mktemp("merged")
    base = LlmEngine(LlmEngineConfig(
        preset="llama-tiny", num_kv_blocks=128, block_size=16,
        max_model_len=256, device="cpu"))
    base.start()
    state = {k: v.clone() for k, v in base.model.state_dict().items()}
    engines = [base]
    for m in adapters:
        merged = merge_adapter(state, load_adapter(m["path"], 16), MCFG)
        path = str(root / (m["name"] + ".safetensors"))
        save_file({k: v.contiguous() for k, v in merged.items()}, path)
        eng = LlmEngine(LlmEngineConfig(
            preset="llama-tiny", num_kv_blocks=128, block_size=16,
            max_model_len=256, device="cpu", weights=path))
        eng.start()
        engines.append(eng)
    want = []
    for eng, prompt in zip(engines, PROMPTS):
        toks, items = lora_util.generate_batch(
            eng, [prompt], [None], max_tokens=MAX_TOKENS, logprobs=2)
        for item in items[0]:
            top = sorted(item["top_logprobs"].values(), reverse=True)
            gap = top[0] - top[1]
            print("oracle top-2 gap", gap)
            assert gap > 1e-3, "argmax near-tie: pick another seed"
        want.append(toks[0])
    return want


# --------------------------------------------------------------------- #
# loader + model hook vs merged weights
# --------------------------------------------------------------------- #
def test_loader_maps_onto_merged_projections(adapters):
    ad1 = load_adapter(adapters[0]["path"], 16, name="ad1")
    ad2 = load_adapter(adapters[1]["path"], 16, name="ad2")
    assert ad1.r == 8 and ad1.scale == 2.0 and ad2.scale == 0.5
    bank = LoraBank([ad1, ad2], MCFG, 16, "cpu", torch.float32)
    assert bank.index == {"ad1": 0, "ad2": 1}
    h, inter = MCFG.hidden, MCFG.intermediate
    q_out = MCFG.heads * MCFG.head_dim
    kv_out = MCFG.kv_heads * MCFG.head_dim
    a, b = bank.layer(1, "qkv")
    assert tuple(a.shape) == (2, 48, h)          # 3 parts x rank 8 -> 16
    assert tuple(b.shape) == (2, q_out + 2 * kv_out, 48)
    a_k, b_k = ad1.tensors[(1, "k_proj")]
    assert torch.equal(a[0, 16:24], a_k) and not a[0, 24:32].any()
    assert torch.equal(b[0, q_out:q_out + kv_out, 16:24], b_k * 2.0)
    # block-diagonal: k's rows carry nothing in q's or v's rank columns
    assert not b[0, q_out:q_out + kv_out, :16].any()
    assert not b[0, q_out:q_out + kv_out, 32:].any()
    a, b = bank.layer(0, "gate_up")
    assert tuple(a.shape) == (2, 32, h) and tuple(b.shape) == (2, 2 * inter,
                                                               32)
    assert a[0].any() and not a[1].any() and not b[1].any()  # ad2: attn only
    a, b = bank.layer(0, "down")
    assert tuple(a.shape) == (2, 16, inter) and tuple(b.shape) == (2, h, 16)


def test_model_forward_matches_merged_weights(adapters):
    torch.manual_seed(0)
    model = LlamaForCausalLM(MCFG).eval()
    ads = [load_adapter(m["path"], 16, name=m["name"]) for m in adapters]
    bank = LoraBank(ads, MCFG, 16, "cpu", torch.float32)
    b, s = 3, 13
    tokens = torch.randint(0, MCFG.vocab_size, (b * s,))
    positions = torch.arange(s, dtype=torch.int32).repeat(b)

    def ctx():
        return {"mode": "prefill", "batch": b, "seq": s,
                "seq_lens": torch.full((b,), s, dtype=torch.int32)}

    idx = torch.tensor([-1] * s + [0] * s + [1] * s, dtype=torch.int32)
    with torch.inference_mode():
        base = model(tokens, positions, attn_ctx=ctx())
        got = model(tokens, positions,
                    attn_ctx={**ctx(), "lora": (bank, idx)})
        # rows routed with -1 are the unmodified base model, exactly
        assert torch.equal(got[:s], base[:s])
        state = model.state_dict()
        for slot, ad in enumerate(ads):
            merged = LlamaForCausalLM(MCFG).eval()
            merged.load_state_dict(merge_adapter(state, ad, MCFG))
            want = merged(tokens, positions, attn_ctx=ctx())
            rows = slice((slot + 1) * s, (slot + 2) * s)
            torch.testing.assert_close(got[rows], want[rows],
                                       atol=1e-4, rtol=1e-4)
            assert (got[rows] - base[rows]).abs().max() > 1e-2


# --------------------------------------------------------------------- #
# engine: one mixed batch == three single-model engines
# --------------------------------------------------------------------- #
def test_engine_mixed_batch_matches_merged_engines(adapters, oracle):
    eng = lora_engine(adapters)
    got, _ = lora_util.generate_batch(eng, PROMPTS, LORAS,
                                      max_tokens=MAX_TOKENS)
    assert eng.stats["prefill_batches"] == 1  # one batch, three adapters
    assert got == oracle
    assert eng.stats["lora_requests"] == 2
    # the adapters change the output: same prompt, base vs each adapter
    same, _ = lora_util.generate_batch(eng, [PROMPTS[0]] * 3, LORAS,
                                       max_tokens=MAX_TOKENS)
    assert same[0] == oracle[0]
    assert same[1] != same[0] and same[2] != same[0]


def test_engine_mixed_batch_chunked_prefill(adapters, oracle):
    eng = lora_engine(adapters, prefill_chunk=8)
    chunks = []
    orig = eng._exec_chunk
    eng._exec_chunk = lambda plan: (chunks.append(plan["lora"]),
                                    orig(plan))[1]
    got, _ = lora_util.generate_batch(eng, PROMPTS, LORAS,
                                      max_tokens=MAX_TOKENS)
    assert len(chunks) > 3  # prompts really advanced in chunks
    assert got == oracle


def test_engine_mixed_batch_speculative(adapters, oracle):
    eng = lora_engine(adapters, speculative={
        "method": "ngram", "num_spec_tokens": 4, "ngram": 1})
    got, _ = lora_util.generate_batch(eng, PROMPTS, LORAS,
                                      max_tokens=MAX_TOKENS)
    assert eng.stats["spec_proposed"] > 0  # the verify forward really ran
    assert got == oracle


def test_preempted_sequence_keeps_adapter(adapters, oracle):
    eng = lora_engine(adapters)
    params = lora_util.SamplingParams(temperature=0.0, max_tokens=MAX_TOKENS,
                                      ignore_eos=True)
    other = Sequence("base", list(PROMPTS[0]), params)
    seq = Sequence("ad1", list(PROMPTS[1]), params, lora_idx=0,
                   cache_salt=eng.lora_bank.salts[0])
    other.created, seq.created = 1.0, 2.0  # the adapter row is the victim
    eng.waiting.extend([other, seq])
    for _ in range(4):
        eng.step()
    assert 0 < seq.generated < MAX_TOKENS
    assert eng._preempt_one() and seq in eng.waiting and not seq.blocks
    while not (seq.finished and other.finished):
        eng.step()
    assert eng.stats["preemptions"] == 1

    def drain(s):
        toks = []
        while not s.stream.empty():
            toks.extend(s.stream.get_nowait()["token_ids"])
        return toks

    assert drain(seq) == oracle[1]
    assert drain(other) == oracle[0]


# --------------------------------------------------------------------- #
# prefix caching: blocks are never shared across adapters
# --------------------------------------------------------------------- #
def test_prefix_cache_is_salted_per_adapter(adapters):
    eng = lora_engine(adapters, enable_prefix_caching=True)
    prompt = [(9 + 5 * j) % 500 for j in range(40)]  # two full blocks

    def hits():
        return eng.stats.get("prefix_cache_hit_tokens", 0)

    first, _ = lora_util.generate_batch(eng, [prompt], [0], max_tokens=4)
    assert hits() == 0
    lora_util.generate_batch(eng, [prompt], [1], max_tokens=4)
    assert hits() == 0  # same prompt, other adapter: nothing shared
    lora_util.generate_batch(eng, [prompt], [-1], max_tokens=4)
    assert hits() == 0  # nor with the base model
    again, _ = lora_util.generate_batch(eng, [prompt], [0], max_tokens=4)
    assert hits() == 32  # same adapter: served from its cached blocks
    assert again == first


def test_prefix_chain_hash_unchanged_for_base_model():
    alloc = PrefixCacheAllocator(8, 4)
    toks = list(range(9))
    assert alloc._chain_hashes(toks) == alloc._chain_hashes(toks, 0)
    h = 0
    for i in range(2):
        h = hash((h, tuple(toks[i * 4:(i + 1) * 4])))
    assert alloc._chain_hashes(toks)[-1] == h
    assert alloc._chain_hashes(toks, 77) != alloc._chain_hashes(toks)


# --------------------------------------------------------------------- #
# OpenAI surface
# --------------------------------------------------------------------- #
def test_openai_model_routing(adapters):
    eng = lora_engine(adapters)
    models = eng.openai_models("base-llm")["data"]
    assert [m["id"] for m in models] == ["base-llm", "ad1", "ad2"]
    assert "parent" not in models[0]
    for m, cfg in zip(models[1:], adapters):
        assert m["parent"] == "base-llm" and m["root"] == cfg["path"]

    def chat(model=None):
        body = {"messages": [{"role": "user", "content": "hi there"}],
                "max_tokens": 6, "temperature": 0.0, "ignore_eos": True}
        if model is not None:
            body["model"] = model
        return run(eng.openai_chat_completions(body, "base-llm"))

    base, ad1, unknown = chat(), chat("ad1"), chat("no-such-model")
    assert base["model"] == "base-llm" and ad1["model"] == "ad1"
    assert unknown["model"] == "base-llm"  # served by the base model
    text = lambda r: r["choices"][0]["message"]["content"]  # noqa: E731
    assert text(unknown) == text(base)
    assert text(ad1) != text(base)
    assert eng.stats["lora_requests"] == 1

    comp = run(eng.openai_completions(
        {"prompt": "hi there", "model": "ad2", "max_tokens": 6,
         "temperature": 0.0, "ignore_eos": True, "echo": True,
         "logprobs": 1}, "base-llm"))
    assert comp["model"] == "ad2"
    simple = run(eng.generate_simple(
        {"prompt": "hi there", "lora": "ad2", "max_tokens": 6,
         "temperature": 0.0, "ignore_eos": True}))
    assert comp["choices"][0]["text"] == "hi there" + simple["text"]
    assert eng.stats["lora_requests"] == 3


def test_config_from_aux_resolves_relative_adapter_paths(adapters, tmp_path):
    cfg = LlmEngineConfig.from_aux(str(tmp_path), {
        "preset": "llama-tiny", "max_lora_rank": 32,
        "lora_modules": [{"name": "a", "path": "adapters/a"},
                         {"name": "b", "path": adapters[0]["path"]}]})
    assert cfg.max_lora_rank == 32
    assert cfg.lora_modules[0]["path"] == str(tmp_path / "adapters" / "a")
    assert cfg.lora_modules[1]["path"] == adapters[0]["path"]
    assert LlmEngineConfig().lora_modules is None


# --------------------------------------------------------------------- #
# unsupported combinations fail loudly
# --------------------------------------------------------------------- #
def test_config_errors(adapters, tmp_path):
    with pytest.raises(ValueError, match="fp8"):
        lora_engine(adapters, quantization="fp8")
    with pytest.raises(ValueError, match="gpt2"):
        lora_engine(adapters, preset="gpt2-tiny")
    with pytest.raises(ValueError, match="max_lora_rank"):
        lora_engine(adapters, max_lora_rank=4)
    lora_util.write_adapter(str(tmp_path / "bias"), MCFG, lora_util.ATTN_ONLY,
                            config_extra={"bias": "all"})
    with pytest.raises(ValueError, match="bias"):
        lora_engine([{"name": "bias", "path": str(tmp_path / "bias")}])
    lora_util.write_adapter(
        str(tmp_path / "head"), MCFG, lora_util.ATTN_ONLY,
        config_extra={"target_modules": lora_util.ATTN_ONLY + ["lm_head"]})
    with pytest.raises(ValueError, match="lm_head"):
        lora_engine([{"name": "head", "path": str(tmp_path / "head")}])
    lora_util.write_adapter(str(tmp_path / "dora"), MCFG, lora_util.ATTN_ONLY,
                            config_extra={"use_dora": True})
    with pytest.raises(ValueError, match="DoRA"):
        load_adapter(str(tmp_path / "dora"), 16)
    lora_util.write_adapter(str(tmp_path / "save"), MCFG, lora_util.ATTN_ONLY,
                            config_extra={"modules_to_save": ["lm_head"]})
    with pytest.raises(ValueError, match="modules_to_save"):
        load_adapter(str(tmp_path / "save"), 16)
    lora_util.write_adapter(
        str(tmp_path / "emb"), MCFG, lora_util.ATTN_ONLY, tensors_extra={
            "base_model.model.model.embed_tokens.lora_embedding_A":
                torch.zeros(8, MCFG.vocab_size)})
    with pytest.raises(ValueError, match="embed_tokens"):
        load_adapter(str(tmp_path / "emb"), 16)
