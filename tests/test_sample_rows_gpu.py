"""GPU: ops.sample_rows against the numpy replica of the draw and float64
keep-sets; acceptance rule (gumbel_ref.MARGIN) as test_sampling_exact_gpu."""

import asyncio
import os
import sys

import numpy as np
import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine, LlmEngineConfig, SamplingParams)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, HERE)
import gumbel_ref as gr  # noqa: E402
import test_sampling_exact_gpu as exact  # noqa: E402  (inputs, _judge)

pytestmark = pytest.mark.gpu

DEV, TEMPS3 = exact.DEV, exact.MASKED_TEMPS   # 0, 0.7, 1.3
# (top_k, top_p, min_p): the eleven FILTERS pairs, min-p alone, all three
GRID = [(k, p, 0.0) for k, p in exact.FILTERS] + [
    (0, 1.0, 0.05), (0, 1.0, 0.5), (10, 0.9, 0.05)]


def _run(logits, temp, top_k, top_p, min_p, seed):
    def dev(x, dtype):
        return None if x is None else torch.as_tensor(
            np.ascontiguousarray(x), dtype=dtype).to(DEV)
    return ops.sample_rows(
        logits.to(DEV), dev(temp, torch.float32), dev(top_k, torch.int32),
        dev(top_p, torch.float32), dev(min_p, torch.float32),
        dev(seed, torch.int32)).cpu().numpy()


@pytest.mark.parametrize("dtype", exact.DTYPES, ids=exact.DTYPE_IDS)
@pytest.mark.parametrize("rows,vocab", [(1, 5), (5, 257), (3, 4099),
                                        (65, 1000), (2, 128256)])
def test_unfiltered_batch_is_the_masked_replica(rows, vocab, dtype):
    logits = exact._logits(rows, vocab, dtype)
    temp = np.array([TEMPS3[r % 3] for r in range(rows)], dtype=np.float32)
    seed = (np.arange(rows) * 2654435761 + 17) % 2**32 - 2**31
    off = (np.zeros(rows), np.ones(rows), np.zeros(rows))
    got = _run(logits, temp, *off, seed)
    assert got.dtype == np.int64 and got.shape == (rows,)
    score = gr.scores(logits.double().numpy(), temp,
                      gr.masked_row_seeds(seed))
    _, _, bad = exact._judge(got, score, "plain")
    assert not bad, "\n".join(bad[:10])
    # no filter tensors (no select launch) and a misaligned row-strided view
    assert (_run(logits, temp, None, None, None, seed) == got).all()
    wide = torch.zeros(rows, vocab + 13, dtype=dtype, device=DEV)
    view = wide[:, 3:3 + vocab]
    view.copy_(logits)
    assert (_run(view, temp, *off, seed) == got).all()


def _keep(lg64, temp, k, p, mp, sign):   # sign +1: loose, -1: strict
    slack = sign * exact.P_SLACK if p < 1.0 else 0.0
    keep = gr.keep_set(lg64, temp, k, p + slack)
    if mp > 0.0:
        ratio = (lg64 - lg64.max(-1, keepdims=True)) / temp
        keep &= ratio >= np.log(mp) - sign * exact.P_SLACK
    return keep


def _grid_batch(shift, temp):
    rows = exact.FILTER_ROWS
    entry = [(r + shift) % len(GRID) for r in range(rows)]
    k, p, mp = (np.array([GRID[e][i] for e in entry]) for i in range(3))
    seed = (np.arange(rows) * 2654435761 + 17 + shift) % 2**32 - 2**31
    return entry, np.full(rows, temp, dtype=np.float32), k, p, mp, seed


def test_heterogeneous_filters():
    logits = exact._filter_logits()
    lg64 = logits.double().numpy()
    rows = np.arange(exact.FILTER_ROWS)
    total = undecided = 0
    bad = []
    for temp in exact.TEMPS:
        sets = [(_keep(lg64, temp, *g, -1), _keep(lg64, temp, *g, +1))
                for g in GRID]
        for shift in range(len(GRID)):
            entry, t, k, p, mp, seed = _grid_batch(shift, temp)
            got = _run(logits, t, k, p, mp, seed)
            strict = np.stack([sets[e][0][r] for r, e in enumerate(entry)])
            loose = np.stack([sets[e][1][r] for r, e in enumerate(entry)])
            what = "T={} shift={}".format(temp, shift)
            assert ((got >= 0) & (got < lg64.shape[1])).all(), what
            bad += ["{} row {}: token {} is outside the keep-set".format(
                what, r, got[r]) for r in rows[~loose[rows, got]]]
            rs = gr.masked_row_seeds(seed)
            s_loose = gr.scores(lg64, t, rs, loose)
            s_strict = gr.scores(lg64, t, rs, strict)
            same = gr.argmax_lowest(s_loose) == gr.argmax_lowest(s_strict)
            undecided += int((~same).sum())
            total += len(rows)
            bad += exact._judge(got[same], s_loose[same], what)[2]
    assert not bad, "\n".join(bad[:10])
    assert total == 672 and undecided * 20 <= total


def test_row_independence():
    logits = exact._filter_logits()
    _, t, k, p, mp, seed = _grid_batch(0, 0.7)
    t[::5] = 0.0
    got = _run(logits, t, k, p, mp, seed)
    rev = slice(None, None, -1)
    again = _run(logits.flip(0), t[rev], k[rev], p[rev], mp[rev], seed[rev])
    assert (again[rev] == got).all()
    alone = [int(_run(logits[r:r + 1], t[r:r + 1], k[r:r + 1], p[r:r + 1],
                      mp[r:r + 1], seed[r:r + 1])[0])
             for r in range(len(got))]
    assert alone == got.tolist()


def test_tied_maximum_with_top_k_1_returns_the_whole_group():
    vocab, tied = 1000, [3, 500, 999]
    row = exact._logits(1, vocab, torch.bfloat16)
    row[0, tied] = row.max() + 1
    n = 64
    got = _run(row.expand(n, vocab).contiguous(), np.ones(n), np.ones(n),
               np.ones(n), np.zeros(n), np.arange(n) - 32)
    assert sorted(set(got.tolist())) == tied


def test_tie_group_across_the_top_p_cut_goes_one_way():
    vocab, p, group = 257, 0.7, [5, 64, 130, 256]
    row = torch.full((1, vocab), -10.0)
    row[0, 17] = 2.0
    row[0, group] = 1.0
    # float64 group rule: tau = lowest v with M(v) <= p * M(all)
    x = row[0].double().numpy()
    vals = np.unique(x)[::-1]
    mass = np.array([np.exp(x[x >= v] - x.max()).sum() for v in vals])
    tau = vals[mass <= p * mass[-1]].min()
    assert tau == 2.0   # one member would fit under p, the group does not
    n = 64
    got = _run(row.expand(n, vocab).contiguous(), np.ones(n), np.zeros(n),
               np.full(n, p), np.zeros(n), np.arange(n) * 7919 - 2**20)
    assert (got == 17).all(), got.tolist()


@pytest.mark.parametrize("dtype", exact.DTYPES, ids=exact.DTYPE_IDS)
def test_invalid_and_masked_rows(dtype):
    rows, vocab = 8, 4099
    logits = exact._logits(rows, vocab, dtype)
    g = torch.Generator().manual_seed(5)
    logits[:4][torch.rand(4, vocab, generator=g) < 0.5] = float("-inf")
    logits[2:6][torch.rand(4, vocab, generator=g) < 0.3] = float("nan")
    logits[4, logits[4].nan_to_num(-1e9).argmax()] = float("nan")
    logits[6] = float("-inf")
    logits[7] = float("nan")
    temp = np.array([TEMPS3[r % 3] for r in range(rows)], dtype=np.float32)
    seed = np.arange(rows) * -7919
    lg64 = logits.double().numpy()
    score = gr.scores(lg64, temp, gr.masked_row_seeds(seed))
    got = _run(logits, temp, np.zeros(rows), np.ones(rows), np.zeros(rows),
               seed)
    _, _, bad = exact._judge(got, score, "unfiltered")   # rows 6, 7: -1
    assert not bad, "\n".join(bad)
    # filtered rows too find nothing in the dead rows, something elsewhere
    got = _run(logits, temp, np.full(rows, 10), np.full(rows, 0.9),
               np.full(rows, 0.01), seed)
    assert (got[6:] == -1).all() and np.isfinite(lg64[range(6), got[:6]]).all()


def test_top_k_1_is_argmax_for_every_seed():
    logits = exact._filter_logits()
    rows = exact.FILTER_ROWS
    want = logits.argmax(-1).numpy()
    for top_p, seed in [(p, s) for p in (1.0, 0.9, 0.1)
                        for s in exact.PLANT_SEEDS]:
        got = _run(logits, np.full(rows, 1.3), np.ones(rows),
                   np.full(rows, top_p), np.zeros(rows),
                   np.full(rows, seed - 2**31))
        assert (got == want).all(), (top_p, seed)


def test_engine_rows_do_not_depend_on_their_batch():
    eng = LlmEngine(LlmEngineConfig(preset="llama-tiny", num_kv_blocks=128,
                                    block_size=16, max_model_len=128,
                                    device=DEV))
    eng.start()

    async def one(prompt, **kw):
        return [t async for item in eng.generate(prompt, SamplingParams(
            max_tokens=6, ignore_eos=True, **kw)) for t in item["token_ids"]]

    async def batch(*requests):
        return await asyncio.gather(*[one(p, **kw) for p, kw in requests])

    greedy = ("abc", dict(temperature=0.0))
    seeded = ("hello world", dict(temperature=1.0, top_p=0.9, seed=1234))

    async def main():
        return (await batch(greedy), await batch(seeded), await batch(
            greedy, ("abc", dict(temperature=1.0, top_k=1)), seeded,
            ("zq!7#", dict(temperature=1.0, min_p=0.1)),
            ("the fox", dict(temperature=0.8, presence_penalty=0.5,
                             repetition_penalty=1.2, min_tokens=3))))

    (g,), (alone,), mixed = asyncio.run(main())
    assert len(g) == 6 and all(len(t) == 6 for t in mixed)
    assert mixed[:3] == [g, g, alone]
