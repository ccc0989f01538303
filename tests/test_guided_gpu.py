"""Guided decoding on the GPU: the token_mask kernels against the CPU
references in ops/__init__.py, and the engine end to end with decode graphs."""

import asyncio
import json
import re

import pytest
import torch

from clearml_serving_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 97), (5, 257), (64, 4099), (3, 128256)]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def make_bank(vocab, n_random=5, seed=0):
    """Random density-0.5 rows, then an all-ones row and a single-bit row
    (the last slot); bits at positions >= vocab are zero."""
    g = torch.Generator().manual_seed(seed)
    allowed = torch.rand(n_random + 2, vocab, generator=g) < 0.5
    allowed[n_random] = True
    allowed[n_random + 1] = False
    allowed[n_random + 1, vocab - 1] = True
    words = (vocab + 31) // 32
    padded = torch.zeros(allowed.shape[0], words * 32, dtype=torch.int64)
    padded[:, :vocab] = allowed
    weights = torch.tensor([1 << i for i in range(32)], dtype=torch.int64)
    packed = (padded.view(-1, words, 32) * weights).sum(-1)
    packed = torch.where(packed >= 2**31, packed - 2**32, packed)
    return packed.to(torch.int32), allowed


def make_slots(rows, n_slots, seed=0):
    """-1, repeated slots and the last slot all occur (rows permitting)."""
    g = torch.Generator().manual_seed(seed)
    slot = torch.randint(-1, n_slots, (rows,), generator=g,
                         dtype=torch.int32)
    slot[0] = n_slots - 1
    if rows >= 5:
        slot[1] = -1
        slot[2] = slot[3] = 2
        slot[4] = n_slots - 2
    return slot


_CASES = {}


def case(rows, vocab, dtype):
    """Inputs + CPU references, computed once and shared."""
    key = (rows, vocab, dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(rows * 131 + vocab)
        logits = (torch.randn(rows, vocab, generator=g) * 4).to(dtype)
        bank, _ = make_bank(vocab)
        slot = make_slots(rows, bank.shape[0])
        ref = ops.apply_token_bitmask(logits, bank, slot)
        _CASES[key] = (logits, bank, slot, ref)
    return _CASES[key]


def same_bits(a, b):
    ia = a.view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.view(torch.int16 if b.element_size() == 2 else torch.int32)
    return torch.equal(ia, ib)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,vocab", SHAPES)
def test_apply_matches_cpu_reference(rows, vocab, dtype):
    logits, bank, slot, ref = case(rows, vocab, dtype)
    src = logits.to(DEV)
    keep = src.clone()
    out = ops.apply_token_bitmask(src, bank.to(DEV), slot.to(DEV))
    assert out.dtype == dtype and out.shape == (rows, vocab)
    assert same_bits(out.cpu(), ref)
    assert same_bits(src, keep), "the source tensor was written"
    assert out.data_ptr() != src.data_ptr()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,vocab", SHAPES)
def test_apply_row_strided_views(rows, vocab, dtype):
    logits, bank, slot, ref = case(rows, vocab, dtype)
    wide = torch.zeros(rows, vocab + 13, dtype=dtype, device=DEV)
    wide[:, :vocab] = logits.to(DEV)
    out = ops.apply_token_bitmask(wide[:, :vocab], bank.to(DEV),
                                  slot.to(DEV))
    assert same_bits(out.cpu(), ref)
    tall = torch.zeros(rows + 3, vocab, dtype=dtype, device=DEV)
    tall[:rows] = logits.to(DEV)
    out = ops.apply_token_bitmask(tall[:rows], bank.to(DEV), slot.to(DEV))
    assert same_bits(out.cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,vocab", SHAPES)
def test_sample_greedy_is_argmax_of_masked_row(rows, vocab, dtype):
    logits, bank, slot, _ = case(rows, vocab, dtype)
    logits = logits.clone()
    _, allowed = make_bank(vocab)
    # a maximum on a disallowed token, and tied maxima on allowed ones
    for r in range(rows):
        if slot[r] < 0:
            continue
        ok = allowed[slot[r]].nonzero().flatten()
        bad = (~allowed[slot[r]]).nonzero().flatten()
        if len(bad):
            logits[r, bad[len(bad) // 2]] = 100.0
        if len(ok) >= 3:
            logits[r, ok[len(ok) // 3]] = 50.0
            logits[r, ok[-1]] = 50.0
    ref = ops.apply_token_bitmask(logits, bank, slot).float().argmax(-1)
    got = ops.sample_token_bitmask(
        logits.to(DEV), bank.to(DEV), slot.to(DEV),
        torch.zeros(rows, device=DEV), torch.zeros(rows, dtype=torch.int32,
                                                   device=DEV))
    assert got.dtype == torch.int64
    assert torch.equal(got.cpu(), ref)
    # strided input takes the same answer
    wide = torch.zeros(rows, vocab + 13, dtype=dtype, device=DEV)
    wide[:, :vocab] = logits.to(DEV)
    got = ops.sample_token_bitmask(
        wide[:, :vocab], bank.to(DEV), slot.to(DEV),
        torch.zeros(rows, device=DEV), torch.zeros(rows, dtype=torch.int32,
                                                   device=DEV))
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("rows,vocab", SHAPES)
def test_sampled_draws_stay_inside_the_mask(rows, vocab):
    logits, bank, slot, _ = case(rows, vocab, torch.bfloat16)
    _, allowed = make_bank(vocab)
    reps = -(-200 // rows)  # >= 200 draws per shape, batched in one launch
    big = logits.repeat(reps, 1).to(DEV)
    slots = slot.repeat(reps)
    n = big.shape[0]
    got = ops.sample_token_bitmask(
        big, bank.to(DEV), slots.to(DEV),
        torch.full((n,), 1.5, device=DEV),
        torch.arange(n, dtype=torch.int32, device=DEV)).cpu()
    assert ((got >= 0) & (got < vocab)).all()
    guided = slots >= 0
    assert allowed[slots[guided].long(), got[guided]].all()
    if rows >= 5:  # row 1 is unconstrained: its seeds spread over tokens
        assert len(set(got[1::rows].tolist())) > 1


def test_sampled_token_is_invariant_to_row_and_batch():
    vocab = 128256  # splits the vocabulary at B=1, not at B=64
    g = torch.Generator().manual_seed(5)
    bank, _ = make_bank(vocab)
    rows = (torch.randn(64, vocab, generator=g) * 3).to(torch.bfloat16)
    slot = torch.full((64,), 1, dtype=torch.int32)
    temp = torch.full((64,), 0.8)
    seed = torch.arange(64, dtype=torch.int32) + 1000
    rows[37] = rows[0]
    seed[37] = 77
    big = ops.sample_token_bitmask(rows.to(DEV), bank.to(DEV), slot.to(DEV),
                                   temp.to(DEV), seed.to(DEV)).cpu()
    one = ops.sample_token_bitmask(
        rows[:1].to(DEV), bank.to(DEV), slot[:1].to(DEV), temp[:1].to(DEV),
        torch.tensor([77], dtype=torch.int32, device=DEV)).cpu()
    assert int(big[37]) == int(one[0])
    assert len(set(big.tolist())) > 8  # other seeds draw other tokens


def test_sampled_distribution_matches_softmax_of_allowed_tokens():
    vocab, n = 64, 4096
    probs = {5: 0.6, 20: 0.3, 41: 0.1}
    row = torch.full((vocab,), -8.0)
    for t, p in probs.items():
        row[t] = torch.log(torch.tensor(p))
    row[7] = 3.0   # higher logits, masked out
    row[33] = 2.0
    allowed = torch.zeros(2, 64, dtype=torch.int64)
    allowed[0, list(probs)] = 1
    weights = torch.tensor([1 << i for i in range(32)], dtype=torch.int64)
    packed = (allowed.view(2, 2, 32) * weights).sum(-1)
    bank = torch.where(packed >= 2**31, packed - 2**32,
                       packed).to(torch.int32)
    got = ops.sample_token_bitmask(
        row.repeat(n, 1).to(DEV), bank.to(DEV),
        torch.zeros(n, dtype=torch.int32, device=DEV),
        torch.ones(n, device=DEV),
        torch.arange(n, dtype=torch.int32, device=DEV)).cpu()
    counts = torch.bincount(got, minlength=vocab).float() / n
    freqs = {t: float(counts[t]) for t in probs}
    print("frequencies", freqs)
    assert abs(sum(freqs.values()) - 1.0) < 1e-6
    for t, p in probs.items():
        # >= 5 sigma of the binomial at n = 4096 (sigma <= 0.0077)
        assert abs(freqs[t] - p) < 0.04, freqs


def test_empty_mask_row_returns_minus_one():
    vocab = 4099
    logits, bank, _, _ = case(64, vocab, torch.bfloat16)
    bank = torch.cat([bank, torch.zeros(1, bank.shape[1],
                                        dtype=torch.int32)])
    empty = bank.shape[0] - 1
    slot = torch.full((64,), 0, dtype=torch.int32)
    base = {}
    for temp in (0.0, 1.0):
        t = torch.full((64,), temp, device=DEV)
        seed = torch.arange(64, dtype=torch.int32, device=DEV)
        base[temp] = ops.sample_token_bitmask(
            logits.to(DEV), bank.to(DEV), slot.to(DEV), t, seed).cpu()
        slot2 = slot.clone()
        slot2[9] = empty
        got = ops.sample_token_bitmask(
            logits.to(DEV), bank.to(DEV), slot2.to(DEV), t, seed).cpu()
        assert int(got[9]) == -1
        keep = torch.arange(64) != 9
        assert torch.equal(got[keep], base[temp][keep])


def test_wrong_bank_or_slot_raises():
    logits, bank, slot, _ = case(5, 257, torch.bfloat16)
    lg, bk, sl = logits.to(DEV), bank.to(DEV), slot.to(DEV)
    t = torch.zeros(5, device=DEV)
    seed = torch.zeros(5, dtype=torch.int32, device=DEV)
    bad = [
        (lg, bk.long(), sl),           # bank dtype
        (lg, bk[:, :-1].contiguous(), sl),  # bank width != ceil(V/32)
        (lg, bk.view(-1), sl),         # bank rank
        (lg, bk, sl.long()),           # slot dtype
        (lg, bk, sl[:-1]),             # slot length
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            ops.apply_token_bitmask(*args)
        with pytest.raises(RuntimeError):
            ops.sample_token_bitmask(*args, t, seed)
    with pytest.raises(RuntimeError):
        ops.sample_token_bitmask(lg, bk, sl, t.double(), seed)
    with pytest.raises(RuntimeError):
        ops.sample_token_bitmask(lg, bk, sl, t, seed.long())


# --------------------------------------------------------------------- #
# engine
# --------------------------------------------------------------------- #
SCHEMA = {"type": "object",
          "properties": {"kind": {"enum": ["cat", "dog"]},
                         "ok": {"type": "boolean"},
                         "tags": {"type": "array", "maxItems": 2,
                                  "items": {"type": "string",
                                            "maxLength": 3}}},
          "required": ["kind", "ok"]}
REGEX = "[0-9]{3}-[a-f]{2}"
BODIES = [
    {"guided_regex": REGEX, "temperature": 0.0},
    {"guided_json": SCHEMA, "temperature": 0.0},
    {"temperature": 0.0, "ignore_eos": True, "max_tokens": 12},
    {"guided_regex": REGEX, "temperature": 1.0, "seed": 11},
    {"guided_json": SCHEMA, "temperature": 0.7, "seed": 5},
    {"guided_regex": "(yes|no)!{1,3}", "temperature": 0.0, "logprobs": 2},
]


def run_engine(decode_graphs, bodies, prompts):
    from clearml_serving_amd.engines.llm.engine import (
        LlmEngine, LlmEngineConfig, SamplingParams)

    eng = LlmEngine(LlmEngineConfig(
        preset="llama-tiny", num_kv_blocks=64, block_size=16,
        max_model_len=128, device=DEV, decode_graphs=decode_graphs,
        guided_decoding=True))
    eng.start()

    async def one(prompt, body):
        params = SamplingParams.from_request(
            {"max_tokens": 80, **body}, guided=True)
        toks, reason = [], None
        async for item in eng.generate(prompt, params):
            assert not item.get("error"), item
            toks.extend(item["token_ids"])
            reason = item.get("finish_reason") or reason
        return toks, reason, eng.tokenizer.decode(toks)

    async def main():
        return await asyncio.gather(
            *[one(p, b) for p, b in zip(prompts, bodies)])

    out = asyncio.new_event_loop().run_until_complete(main())
    stats = dict(eng.stats)
    eng.stop()
    return out, stats


def test_engine_mixed_batch_with_decode_graphs():
    prompts = ["prompt number {}".format(i) for i in range(len(BODIES))]
    graphs, stats = run_engine(True, BODIES, prompts)
    assert stats["graph_replays"] > 0 and stats["guided_requests"] == 5
    for i in (0, 3):
        assert re.fullmatch(REGEX, graphs[i][2]), graphs[i]
        assert graphs[i][1] == "stop"
    for i in (1, 4):
        doc = json.loads(graphs[i][2])
        assert graphs[i][1] == "stop"
        assert doc["kind"] in ("cat", "dog") and isinstance(doc["ok"], bool)
        assert set(doc) <= {"kind", "ok", "tags"}
        assert all(isinstance(t, str) and len(t) <= 3
                   for t in doc.get("tags", []))
        assert len(doc.get("tags", [])) <= 2
    assert re.fullmatch("(yes|no)!{1,3}", graphs[5][2])
    eager, _ = run_engine(False, BODIES, prompts)
    assert [g[0] for g in graphs] == [e[0] for e in eager]
    solo, _ = run_engine(True, [BODIES[2]], [prompts[2]])
    assert solo[0][0] == graphs[2][0] and len(solo[0][0]) == 12
