"""CPU paths of ops.sample_rows / ops.apply_penalties against the float64
rules at [5, 257]; min_p parsing; the engine's incremental counters."""

import asyncio
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine, LlmEngineConfig, SamplingParams)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import gumbel_ref as gr  # noqa: E402
import penalty_cases as pen  # noqa: E402

ROWS, VOCAB = 5, 257
# per row: (temperature, top_k, top_p, min_p)
PARAMS = [(0.0, 3, 0.5, 0.5), (0.7, 0, 1.0, 0.0), (1.3, 10, 1.0, 0.0),
          (0.7, 0, 0.9, 0.0), (1.3, 10, 0.9, 0.05)]


def test_sample_rows_cpu_path():
    g = torch.Generator().manual_seed(99)
    logits = torch.randn(ROWS, VOCAB, generator=g)
    logits[1, 7] = float("nan")
    logits[2, 9] = float("-inf")
    lg64 = logits.double().numpy()
    live = np.nan_to_num(lg64, nan=-np.inf)
    temp, k, p, mp = (np.array(c) for c in zip(*PARAMS))
    seed = np.arange(ROWS) * 977 - 5
    got = ops.sample_rows(logits, *[torch.tensor(v, dtype=d) for v, d in (
        (temp, torch.float32), (k, torch.int32), (p, torch.float32),
        (mp, torch.float32), (seed, torch.int32))])
    keep = np.ones((ROWS, VOCAB), dtype=bool)
    for r in range(1, ROWS):   # row 0 is greedy: its filters are ignored
        row = live[r:r + 1]
        keep[r] = gr.keep_set(row, temp[r], k[r], p[r])[0]
        if mp[r] > 0:
            keep[r] &= (row[0] - row.max()) / temp[r] >= np.log(mp[r])
    want = gr.argmax_lowest(gr.scores(
        lg64, temp.astype(np.float32), gr.masked_row_seeds(seed), keep))
    assert got.tolist() == want.tolist()


@pytest.mark.parametrize("dtype", pen.DTYPES, ids=pen.DTYPE_IDS)
def test_apply_penalties_cpu_path(dtype):
    pen.run_case(ROWS, VOCAB, dtype, "cpu")


def test_min_p_parsing_and_validation():
    assert SamplingParams.from_request({}).min_p == 0.0
    assert SamplingParams.from_request({"min_p": 0.25}).min_p == 0.25
    for bad in (-0.1, 1.5, "x", float("nan")):
        with pytest.raises(ValueError):
            SamplingParams.from_request({"min_p": bad})


def _serve(requests, **cfg):
    """llama-tiny on the CPU, seeded weights, the (prompt, params) requests
    in flight together -> (engine, finished Sequences)."""
    torch.manual_seed(0)
    eng = LlmEngine(LlmEngineConfig(
        preset="llama-tiny", num_kv_blocks=128, block_size=16,
        max_model_len=256, device="cpu", **cfg))
    eng.start()

    async def one(prompt, params):
        seq = await eng.add_request(eng.tokenizer.encode(prompt), params)
        while not (await seq.stream.get())["finished"]:
            pass
        return seq

    async def main():
        return await asyncio.gather(*[one(*r) for r in requests])

    return eng, asyncio.run(main())


def test_incremental_counters_equal_a_recount_after_speculation():
    greedy = SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True)
    eng, seqs = _serve(
        [(p, greedy) for p in ("abcabcabcabcabc", "the quick brown fox",
                               "zq!7#")],
        speculative={"method": "ngram", "num_spec_tokens": 4, "ngram": 2})
    # some proposals were rejected, i.e. rolled back
    assert eng.stats["spec_proposed"] > eng.stats["spec_accepted"] > 0
    for seq in seqs:
        assert len(seq.output_ids) == 24
        assert seq.output_counts == Counter(seq.output_ids)
        assert seq.prompt_set == set(seq.prompt_ids)


def test_min_p_applies_next_to_a_guided_row():
    """min_p = 1 keeps the maximum alone, so the row equals the greedy one
    also in steps that a guided row sends through the masked sampler."""
    kw = dict(max_tokens=8, ignore_eos=True)
    guided = SamplingParams.from_request(
        {"guided_regex": "[ab]{4,8}", "max_tokens": 8}, guided=True)
    _, (a, b, _g) = _serve(
        [("hello", SamplingParams(temperature=0.0, **kw)),
         ("hello", SamplingParams(temperature=1.0, min_p=1.0, seed=3, **kw)),
         ("x", guided)], guided_decoding=True)
    assert len(a.output_ids) == 8 and a.output_ids == b.output_ids
