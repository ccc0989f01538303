"""Sliding-window attention (Mistral) on the CPU reference paths: the op
oracles against a brute-force masked softmax, numerics against
transformers' MistralForCausalLM, engine generation with KV page
reclamation, preemption, and option validation.

Semantics under test: with window W, query position i sees key j iff
i - W < j <= i; W = None / 0 is full context.
"""

import asyncio
import math

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    FREED_BLOCK, LlmEngine, LlmEngineConfig, SamplingParams)
from clearml_serving_amd.models.convert import convert_hf_auto
from clearml_serving_amd.models.llama import (
    PRESETS, LlamaConfig, LlamaForCausalLM)


def run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


# --------------------------------------------------------------------- #
# op references vs brute force
# --------------------------------------------------------------------- #
def brute_attention(q, k, v, window, scale):
    """q [H, Sq, D], k/v [Hkv, Sk, D] fp32; the last query sits on the last
    key. One (query, key) pair at a time: no shared masking code."""
    h, sq, d = q.shape
    hkv, sk, _ = k.shape
    rep = h // hkv
    out = torch.zeros(h, sq, d)
    for hh in range(h):
        kk, vv = k[hh // rep], v[hh // rep]
        for r in range(sq):
            p = r + sk - sq
            keys = [j for j in range(sk)
                    if j <= p and (not window or j > p - window)]
            s = (kk[keys] @ q[hh, r]) * scale
            out[hh, r] = torch.softmax(s, dim=0) @ vv[keys]
    return out


@pytest.mark.parametrize("window", [1, 5, 16, 40, 41, 100])
def test_attention_window_matches_brute_force(window):
    torch.manual_seed(0)
    b, h, hkv, sq, sk, d = 2, 4, 2, 23, 40, 16
    q = torch.randn(b, h, sq, d)
    k = torch.randn(b, hkv, sk, d)
    v = torch.randn(b, hkv, sk, d)
    scale = 1.0 / math.sqrt(d)
    got = ops.attention(q, k, v, causal=True, window=window)
    for i in range(b):
        ref = brute_attention(q[i], k[i], v[i], window, scale)
        torch.testing.assert_close(got[i], ref, atol=1e-5, rtol=1e-5)
    # bshd layout takes the same mask
    got_bshd = ops.attention(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3),
                             v.permute(0, 2, 1, 3), causal=True,
                             layout="bshd", window=window)
    torch.testing.assert_close(got_bshd.permute(0, 2, 1, 3), got)
    if window >= sk:
        assert torch.equal(got, ops.attention(q, k, v, causal=True))


def test_attention_window_off_values_and_errors():
    torch.manual_seed(1)
    q = torch.randn(1, 2, 9, 8)
    k = torch.randn(1, 2, 9, 8)
    v = torch.randn(1, 2, 9, 8)
    base = ops.attention(q, k, v, causal=True)
    assert torch.equal(ops.attention(q, k, v, causal=True, window=None), base)
    assert torch.equal(ops.attention(q, k, v, causal=True, window=0), base)
    assert torch.equal(ops.attention(q, k, v, causal=True, window=9), base)
    assert not torch.equal(ops.attention(q, k, v, causal=True, window=8),
                           base)
    with pytest.raises(ValueError):
        ops.attention(q, k, v, causal=False, window=4)
    with pytest.raises(ValueError):
        ops.attention(q, k, v, causal=True, window=-1)
    # positional calls are unchanged: window is a trailing keyword
    assert torch.equal(ops.attention(q, k, v, True, None, None, "bhsd"), base)


def paged_case(kv_lens, hkv, d, bs, seed):
    """Shuffled pages holding random K/V for each sequence; 3 pages stay
    unmapped (the last of the permutation serves as a spare)."""
    g = torch.Generator().manual_seed(seed)
    nblk = [(n + bs - 1) // bs for n in kv_lens]
    total = sum(nblk) + 3
    perm = torch.randperm(total, generator=g).tolist()
    k_cache = torch.randn(total, hkv, bs, d, generator=g)
    v_cache = torch.randn(total, hkv, bs, d, generator=g)
    btab = torch.zeros(len(kv_lens), max(nblk), dtype=torch.int32)
    at = 0
    for i, n in enumerate(nblk):
        btab[i, :n] = torch.tensor(perm[at:at + n], dtype=torch.int32)
        at += n
    return k_cache, v_cache, btab


def gather(cache, row, n, bs):
    nb = (n + bs - 1) // bs
    x = cache[row[:nb].long()]            # [nb, hkv, bs, d]
    return x.permute(1, 0, 2, 3).reshape(x.shape[1], nb * bs, -1)[:, :n]


@pytest.mark.parametrize("window", [1, 7, 16, 50, 64, 333, 1000])
def test_prefill_paged_window_matches_brute_force(window):
    kv_lens, q_lens = [40, 77], [8, 30]
    h, hkv, d, bs = 4, 2, 16, 16
    k_cache, v_cache, btab = paged_case(kv_lens, hkv, d, bs, seed=2)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(2, max(q_lens), h, d, generator=g)
    kl = torch.tensor(kv_lens, dtype=torch.int32)
    ql = torch.tensor(q_lens, dtype=torch.int32)
    got = ops.attention_prefill_paged(q, k_cache, v_cache, btab, kl, ql,
                                      window=window)
    for i in range(2):
        ref = brute_attention(
            q[i, :q_lens[i]].permute(1, 0, 2),
            gather(k_cache, btab[i], kv_lens[i], bs),
            gather(v_cache, btab[i], kv_lens[i], bs), window,
            1.0 / math.sqrt(d))
        torch.testing.assert_close(got[i, :q_lens[i]].permute(1, 0, 2), ref,
                                   atol=1e-5, rtol=1e-5)
    if window >= max(kv_lens):
        assert torch.equal(got, ops.attention_prefill_paged(
            q, k_cache, v_cache, btab, kl, ql))


@pytest.mark.parametrize("window", [1, 5, 16, 100, 4096])
def test_decode_window_matches_brute_force(window):
    seqs = [1, 17, 200]
    h, hkv, d, bs = 4, 2, 16, 16
    k_cache, v_cache, btab = paged_case(seqs, hkv, d, bs, seed=4)
    g = torch.Generator().manual_seed(5)
    q = torch.randn(len(seqs), h, d, generator=g)
    sl = torch.tensor(seqs, dtype=torch.int32)
    got = ops.attention_decode(q, k_cache, v_cache, btab, sl, window=window)
    for i, n in enumerate(seqs):
        ref = brute_attention(q[i][:, None], gather(k_cache, btab[i], n, bs),
                              gather(v_cache, btab[i], n, bs), window,
                              1.0 / math.sqrt(d))
        torch.testing.assert_close(got[i], ref[:, 0], atol=1e-5, rtol=1e-5)
    if window >= max(seqs):
        assert torch.equal(
            got, ops.attention_decode(q, k_cache, v_cache, btab, sl))


def test_paged_references_never_use_pages_below_the_window():
    """Block-table entries wholly below a sequence's window start point at a
    NaN page: the oracles the GPU tests rely on must not let it through."""
    h, hkv, d, bs, window = 4, 2, 16, 16, 20
    kv_lens, q_lens = [100, 61], [9, 1]
    k_cache, v_cache, btab = paged_case(kv_lens, hkv, d, bs, seed=6)
    nb = [(n + bs - 1) // bs for n in kv_lens]
    used = {int(x) for i in range(2) for x in btab[i, :nb[i]]}
    spare = next(p for p in range(k_cache.shape[0]) if p not in used)
    g = torch.Generator().manual_seed(7)
    q = torch.randn(2, max(q_lens), h, d, generator=g)
    kl = torch.tensor(kv_lens, dtype=torch.int32)
    ql = torch.tensor(q_lens, dtype=torch.int32)
    want_p = ops.attention_prefill_paged(q, k_cache, v_cache, btab, kl, ql,
                                         window=window)
    want_d = ops.attention_decode(q[:, 0], k_cache, v_cache, btab, kl,
                                  window=window)
    k_cache[spare] = float("nan")
    v_cache[spare] = float("nan")
    stale_p, stale_d = btab.clone(), btab.clone()
    for i in range(2):
        first_p = max(0, kv_lens[i] - q_lens[i] - window + 1)
        stale_p[i, :first_p // bs] = spare
        stale_d[i, :max(0, kv_lens[i] - window) // bs] = spare
    assert (stale_p == spare).any() and (stale_d == spare).any()
    got_p = ops.attention_prefill_paged(q, k_cache, v_cache, stale_p, kl, ql,
                                        window=window)
    got_d = ops.attention_decode(q[:, 0], k_cache, v_cache, stale_d, kl,
                                 window=window)
    for i in range(2):
        assert torch.equal(got_p[i, :q_lens[i]], want_p[i, :q_lens[i]])
    assert torch.equal(got_d, want_d)


# --------------------------------------------------------------------- #
# numerics vs transformers
# --------------------------------------------------------------------- #
def dense_forward(model, ids):
    t = len(ids)
    attn_ctx = {"mode": "prefill", "batch": 1, "seq": t,
                "seq_lens": torch.tensor([t], dtype=torch.int32),
                "slot_mapping": torch.full((t,), -1, dtype=torch.int32)}
    with torch.inference_mode():
        return model(torch.as_tensor(ids), torch.arange(t, dtype=torch.int32),
                     kv_caches=None, attn_ctx=attn_ctx)


def test_mistral_matches_transformers():
    pytest.importorskip("transformers")
    from transformers import MistralConfig, MistralForCausalLM

    tiny = PRESETS["mistral-tiny"]
    assert tiny.sliding_window == 24
    torch.manual_seed(11)
    hf = MistralForCausalLM(MistralConfig(
        vocab_size=tiny.vocab_size, hidden_size=tiny.hidden,
        intermediate_size=tiny.intermediate, num_hidden_layers=tiny.layers,
        num_attention_heads=tiny.heads, num_key_value_heads=tiny.kv_heads,
        head_dim=tiny.head_dim, max_position_embeddings=tiny.max_position,
        rope_theta=tiny.rope_theta, rms_norm_eps=tiny.rms_eps,
        sliding_window=8, tie_word_embeddings=False,
        attn_implementation="eager")).eval().float()
    ids = torch.randint(0, tiny.vocab_size, (40,),
                        generator=torch.Generator().manual_seed(12))
    with torch.inference_mode():
        ref = hf(input_ids=ids[None]).logits[0]
    # Mistral checkpoints use the llama tensor names: no converter of their
    # own, convert_hf_auto routes them through convert_hf_llama
    state = convert_hf_auto(dict(hf.state_dict()))

    cfg = LlamaConfig(**{**tiny.__dict__, "sliding_window": 8})
    ours = LlamaForCausalLM(cfg).eval()
    ours.load_state_dict(state)
    torch.testing.assert_close(dense_forward(ours, ids), ref,
                               atol=3e-4, rtol=3e-4)

    # the same weights with the window off agree only while the window
    # still covers the whole history (positions 0..7)
    full = LlamaForCausalLM(
        LlamaConfig(**{**tiny.__dict__, "sliding_window": 0})).eval()
    full.load_state_dict(state)
    got_full = dense_forward(full, ids)
    torch.testing.assert_close(got_full[:8], ref[:8], atol=3e-4, rtol=3e-4)
    for pos in range(8, 40):
        assert float((got_full[pos] - ref[pos]).abs().max()) > 3e-3, pos


def test_mistral_7b_preset_is_the_v01_card():
    c = PRESETS["mistral-7b"]
    assert (c.vocab_size, c.hidden, c.layers, c.heads, c.kv_heads,
            c.intermediate) == (32000, 4096, 32, 32, 8, 14336)
    assert (c.rope_theta, c.rms_eps, c.max_position, c.sliding_window) == (
        10000.0, 1e-5, 32768, 4096)
    assert c.num_experts == 0 and c.head_dim == 128


# --------------------------------------------------------------------- #
# engine: generation, page reclamation, preemption
# --------------------------------------------------------------------- #
def swa_engine(num_kv_blocks=12, max_model_len=160, **kw):
    kw.setdefault("preset", "mistral-tiny")
    return LlmEngine(LlmEngineConfig(
        num_kv_blocks=num_kv_blocks, block_size=16,
        max_model_len=max_model_len, device="cpu", dtype="float32", **kw))


def watch_pages(eng):
    """Record, after every scheduler step, the pages each running sequence
    holds; also check the books: held + free == all, no page twice."""
    held = []
    inner = eng.step

    def step():
        inner()
        alloc = eng.allocator
        mine = []
        for s in eng.running + eng.waiting:
            live = [b for b in s.blocks if b != FREED_BLOCK]
            assert all(b == FREED_BLOCK for b in s.blocks[:s.swa_freed])
            held.append(len(live))
            mine.extend(live)
        if not hasattr(alloc, "_lru"):  # plain allocator: exact partition
            assert sorted(mine + alloc._free) == list(range(alloc.num_blocks))

    eng.step = step
    return held


async def generate(eng, prompt, max_tokens):
    seq = await eng.add_request(
        list(prompt), SamplingParams(temperature=0.0, max_tokens=max_tokens,
                                     ignore_eos=True))
    toks = []
    while True:
        item = await seq.stream.get()
        assert "error" not in item, item
        toks.extend(item["token_ids"])
        if item["finished"]:
            return toks


def assert_teacher_forced(eng, prompt, generated):
    """fp32 on both sides: every step picked the argmax of ONE windowed
    forward over the whole sequence (a margin below fp32 noise is a tie)."""
    assert eng.model_config.sliding_window > 0
    logits = dense_forward(eng.model, list(prompt) + list(generated))
    for step, tok in enumerate(generated):
        top2 = logits[len(prompt) + step - 1].topk(2)
        assert tok == int(top2.indices[0]) or \
            float(top2.values[0] - top2.values[1]) < 1e-4, step


# 40 tokens with a repeated motif, so prompt-lookup speculation has
# something to propose
PROMPT = [3, 7, 11, 19, 23, 29, 31, 37, 41, 43] * 4


@pytest.mark.parametrize("variant", ["plain", "chunked", "prefix", "spec"])
def test_engine_generates_past_four_windows(variant):
    kw = {"plain": {},
          "chunked": {"prefill_chunk": 16},
          "prefix": {"enable_prefix_caching": True},
          "spec": {"speculative": {"method": "ngram", "num_spec_tokens": 4,
                                   "ngram": 2}}}[variant]
    eng = swa_engine(**kw)
    eng.start()
    window, bs = eng.model_config.sliding_window, eng.cfg.block_size
    assert window == 24 and window % bs != 0
    held = watch_pages(eng)
    generated = run(generate(eng, PROMPT, 80))
    assert len(generated) == 80
    assert len(PROMPT) + len(generated) >= 4 * window
    assert_teacher_forced(eng, PROMPT, generated)
    assert eng.stats["swa_blocks_freed"] > 0
    assert max(held) <= math.ceil(window / bs) + 2, max(held)
    assert eng.allocator.available == eng.allocator.num_blocks
    if variant == "chunked":
        assert eng.stats["prefill_batches"] >= 3
    if variant == "spec":
        assert eng.stats["spec_proposed"] > 0
    if variant == "prefix":
        # pages went back through allocator.free AFTER being published: a
        # second request still hits the prefix, and generates the same text
        again = run(generate(eng, PROMPT, 80))
        assert eng.stats.get("prefix_cache_hit_tokens", 0) >= 32
        assert again == generated
        assert eng.allocator.available == eng.allocator.num_blocks


def test_engine_window_off_frees_nothing():
    eng = swa_engine(preset="llama-tiny")
    eng.start()
    assert eng.model_config.sliding_window == 0
    run(generate(eng, PROMPT, 40))
    assert eng.stats["swa_blocks_freed"] == 0
    assert eng.allocator.available == eng.allocator.num_blocks


def test_engine_preemption_with_window():
    """Two sequences that each want ceil(64/16)+1 = 5 pages of a 9-page
    cache: the newer one is preempted, re-prefills, and both finish."""
    eng = swa_engine(num_kv_blocks=9, overrides={"sliding_window": 64})
    eng.start()
    assert eng.model_config.sliding_window == 64
    watch_pages(eng)
    prompts = [PROMPT[:20], PROMPT[5:25]]

    async def both():
        return await asyncio.gather(generate(eng, prompts[0], 110),
                                    generate(eng, prompts[1], 110))

    outs = run(both())
    assert eng.stats["preemptions"] >= 1
    assert eng.stats["swa_blocks_freed"] > 0
    for prompt, out in zip(prompts, outs):
        assert len(out) == 110
        assert_teacher_forced(eng, prompt, out)
    free = eng.allocator._free
    assert len(free) == len(set(free)) == eng.allocator.num_blocks
    assert eng.allocator.available == eng.allocator.num_blocks


# --------------------------------------------------------------------- #
# option validation
# --------------------------------------------------------------------- #
def test_sliding_window_override_validation():
    with pytest.raises(ValueError, match="sliding_window"):
        swa_engine(preset="llama-tiny",
                   overrides={"sliding_window": -1}).start()
    with pytest.raises(ValueError, match="sliding_window"):
        swa_engine(arch="gpt2", preset="gpt2-tiny",
                   overrides={"sliding_window": 8}).start()
    with pytest.raises(ValueError, match="sliding_window"):
        swa_engine(preset="mixtral-tiny",
                   overrides={"sliding_window": 8}).start()
    # null (what released Mixtral cards carry) is dropped: the preset stands
    for preset, want in (("llama-tiny", 0), ("mistral-tiny", 24),
                         ("mixtral-tiny", 0)):
        eng = swa_engine(preset=preset, overrides={"sliding_window": None})
        eng.start()
        assert eng.model_config.sliding_window == want
    # a dense card's window reaches the model
    eng = swa_engine(preset="llama-tiny", overrides={"sliding_window": 8})
    eng.start()
    assert eng.model_config.sliding_window == 8
    assert eng.model.layers[0].cfg.sliding_window == 8
