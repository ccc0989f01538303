"""GPU: which token the sampling kernels must return.

gumbel_argmax_kernel (sampling.hip, behind ops._ext.sample_top_k_top_p) and
sample_token_bitmask_kernel (token_mask.hip) draw with noise that is a pure
function of (seed, row, token), so helpers/gumbel_ref.py can state the
winning token of every row from numpy alone; test_sampling_exact_cpu.py
shows that this replica samples softmax(logits / T).

Acceptance rule of every "exact" check: the returned token's replica score
is >= the replica's best - gumbel_ref.MARGIN (1e-3, derived there from the
fp32 ulp of the scores and the native log's error -- not from measurements),
and over the whole module at most 1% of the rows may return a token other
than the replica argmax (near-ties closer than the kernels' fp32 error; with
randn*3 logits a top-2 gap under 1e-3 occurs in about 0.03% of rows).

Shapes of the plain sampler (its wrapper splits the vocabulary over
min(16, 1024 / rows) workgroups of ceil(V / splits) tokens): 16 splits
(rows 1..5), 15 (rows 65), 1 (rows 1100); V=5 < 16 leaves eleven splits
empty, V=97 two; 4099 = 15 * 257 + 244 and 1000 = 14 * 67 + 62 end in a short
split; 128256 is the llama-3 vocabulary.
"""

import os
import sys

import numpy as np
import pytest
import torch

import clearml_serving_amd.ops as ops

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, HERE)
import gumbel_ref as gr  # noqa: E402
import test_guided_gpu as guided  # noqa: E402  (bank/slot builders, shapes)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]
PLAIN_SHAPES = [(1, 5), (1, 97), (5, 257), (3, 4099), (65, 1000), (1100, 33),
                (2, 128256)]
TEMPS = [0.7, 1.3]
# as the wrapper's (unsigned int) cast sees them: 7, 2^31 + 12345, 2^32 - 3
SEEDS = [7, 2**31 + 12345, -3]
PLANT_SEEDS = [(i * 2654435761 + 17) % 2**32 for i in range(32)]

FILTER_ROWS, FILTER_VOCAB = 24, 1000
FILTERS = ([(k, 1.0) for k in (1, 10, FILTER_VOCAB)]
           + [(0, p) for p in (0.1, 0.9)]
           + [(k, p) for k in (1, 10, FILTER_VOCAB) for p in (0.1, 0.9)])
P_SLACK = 1e-4

MASKED_SHAPES = guided.SHAPES
MASKED_TEMPS = [0.0, 0.7, 1.3]

_DONE = {}   # case key -> (rows judged, rows != replica argmax, violations)


def _ext():
    ext = ops.extension_or_none()
    assert ext is not None, "HIP extension missing on GPU box"
    return ext


def _once(key, fn):
    if key not in _DONE:
        _DONE[key] = fn()
    return _DONE[key]


def _judge(got, score, what):
    """(rows, rows whose token is not the replica argmax, violations of the
    acceptance rule as readable strings)."""
    got = np.asarray(got)
    rows, vocab = score.shape
    want = gr.argmax_lowest(score)
    best = score.max(axis=-1)
    inside = (got >= 0) & (got < vocab)
    got_score = np.where(
        inside, score[np.arange(rows), np.clip(got, 0, vocab - 1)], -np.inf)
    ok = np.where(want < 0, got == -1,
                  inside & (got_score > -np.inf)
                  & (got_score >= best - gr.MARGIN))
    bad = ["{} row {}: got {} (score {}), replica {} (score {})".format(
        what, r, got[r], got_score[r], want[r], best[r])
        for r in np.nonzero(~ok)[0]]
    return rows, int((got != want).sum()), bad


def _logits(rows, vocab, dtype, scale=3.0):
    g = torch.Generator().manual_seed(rows * 131 + vocab)
    return (torch.randn(rows, vocab, generator=g) * scale).to(dtype)


def _pack(allowed):
    """bool [S, V] -> int32 bank [S, ceil(V/32)], token t = bit t&31 of word
    t>>5."""
    n, vocab = allowed.shape
    words = (vocab + 31) // 32
    padded = torch.zeros(n, words * 32, dtype=torch.int64)
    padded[:, :vocab] = allowed
    weights = torch.tensor([1 << i for i in range(32)], dtype=torch.int64)
    packed = (padded.view(n, words, 32) * weights).sum(-1)
    return torch.where(packed >= 2**31, packed - 2**32,
                       packed).to(torch.int32)


# --------------------------------------------------------------------- #
# plain sampler
# --------------------------------------------------------------------- #
def _plain_case(rows, vocab, dtype):
    logits = _logits(rows, vocab, dtype)
    dev = logits.to(DEV)
    lg64 = logits.double().numpy()
    total = mismatch = 0
    bad = []
    for temp in TEMPS:
        for seed in SEEDS:
            got = _ext().sample_top_k_top_p(dev, temp, 0, 1.0, seed)
            assert got.dtype == torch.int64 and got.shape == (rows,)
            score = gr.scores(lg64, temp, gr.plain_row_seeds(seed, rows))
            n, m, b = _judge(got.cpu().numpy(), score,
                             "T={} seed={}".format(temp, seed))
            total, mismatch, bad = total + n, mismatch + m, bad + b
    return total, mismatch, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("rows,vocab", PLAIN_SHAPES)
def test_plain_draw_is_the_replica_argmax(rows, vocab, dtype):
    total, mismatch, bad = _once(("plain", rows, vocab, dtype),
                                 lambda: _plain_case(rows, vocab, dtype))
    print("rows", total, "not the replica argmax", mismatch)
    assert not bad, "\n".join(bad[:10])


def _split_edges(rows, vocab):
    """Tokens at the edges of the wrapper's vocabulary split."""
    splits = max(1, min(16, 1024 // rows))
    chunk = -(-vocab // splits)
    last = (vocab - 1) // chunk          # last non-empty split
    edges = {0, min(chunk, vocab) - 1, last * chunk, vocab - 1}
    if chunk < vocab:
        edges.add(chunk)                 # first token of split 1
    return sorted(edges)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("rows,vocab", PLAIN_SHAPES)
def test_plain_planted_winner_at_split_edges(rows, vocab, dtype):
    """+40 over a zero row: at T <= 1.3 the planted score is >= 40 / 1.3 +
    G_MIN > 27.9, every other one <= G_MAX < 16.7, so the planted token wins
    for every seed."""
    assert 40 / max(TEMPS) + gr.G_MIN > gr.G_MAX + 1
    for pos in _split_edges(rows, vocab):
        logits = torch.zeros(rows, vocab, dtype=dtype, device=DEV)
        logits[:, pos] = 40.0
        got = torch.stack([
            _ext().sample_top_k_top_p(logits, temp, 0, 1.0, seed)
            for temp in TEMPS for seed in PLANT_SEEDS]).cpu()
        assert (got == pos).all(), (pos, got[got != pos][:8].tolist())


def test_plain_nan_logits_never_win():
    rows, vocab = 3, 4099   # 16 splits of 257
    logits = _logits(rows, vocab, torch.float32)
    logits[0, :257] = float("nan")          # a whole split
    logits[1, ::2] = float("nan")
    logits[2, logits[2].argmax()] = float("nan")
    logits[2, vocab - 1] = float("nan")
    lg64 = logits.double().numpy()
    for seed in SEEDS:
        got = _ext().sample_top_k_top_p(logits.to(DEV), 0.7, 0, 1.0,
                                        seed).cpu()
        assert not torch.isnan(logits[torch.arange(rows), got]).any()
        score = gr.scores(lg64, 0.7, gr.plain_row_seeds(seed, rows))
        _, _, bad = _judge(got.numpy(), score, "seed={}".format(seed))
        assert not bad, "\n".join(bad)


# --------------------------------------------------------------------- #
# u == 1.0 regression: a token whose hash is one of the top 128 values had
# g == +inf and won its row whatever its logit was
# --------------------------------------------------------------------- #
_TAILS = {}


def _tail_pairs(vocab, negative):
    """[(seed, token)] with pcg(pcg(seed) + token) >= 2^32 - 128: row 0 of
    the plain sampler and any row of the masked one."""
    key = (vocab, negative)
    if key not in _TAILS:
        seeds = range(-1, -60000, -1) if negative else range(60000)
        count = 2 if (vocab == 4096 and not negative) else 1
        _TAILS[key] = [(s, t) for s, t, _ in gr.find_hash_hits(
            vocab, gr.TAIL_LO, gr.TAIL_HI, seeds, count=count)]
    return _TAILS[key]


def _peak_for(tok, vocab):
    return (tok + vocab // 2) % vocab


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("vocab", [4096, 128256])
def test_plain_top_hash_token_does_not_beat_the_peak(vocab, dtype):
    pairs = _tail_pairs(vocab, False)
    if vocab == 4096:
        assert pairs == [(2697, 2891), (18583, 488)]
    for seed, tok in pairs:
        assert gr.plain_row_seeds(seed, 1).tolist() == \
            gr.masked_row_seeds([seed]).tolist()
        peak = _peak_for(tok, vocab)
        logits = torch.zeros(1, vocab, dtype=dtype, device=DEV)
        logits[0, peak] = 40.0
        for temp in (1.0, 1.3):
            got = int(_ext().sample_top_k_top_p(logits, temp, 0, 1.0, seed))
            assert got == peak, (
                "seed {} T {}: token {} returned, peak is {}, token {} has "
                "the top hash".format(seed, temp, got, peak, tok))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("vocab", [4096, 128256])
def test_masked_top_hash_token_does_not_beat_the_peak(vocab, dtype):
    pairs = _tail_pairs(vocab, False) + _tail_pairs(vocab, True)
    assert any(s < 0 for s, _ in pairs)
    n = len(pairs)
    logits = torch.zeros(2 * n, vocab, dtype=dtype)
    peaks = []
    for i, (_, tok) in enumerate(pairs):
        peaks.append(_peak_for(tok, vocab))
        logits[i, peaks[i]] = logits[n + i, peaks[i]] = 40.0
    bank = _pack(torch.ones(1, vocab, dtype=torch.bool))
    # first half unconstrained (slot -1), second half through an all-ones row
    slot = torch.tensor([-1] * n + [0] * n, dtype=torch.int32)
    seed = torch.tensor([s for s, _ in pairs] * 2, dtype=torch.int32)
    for temp in (1.0, 1.3):
        got = ops.sample_token_bitmask(
            logits.to(DEV), bank.to(DEV), slot.to(DEV),
            torch.full((2 * n,), temp, device=DEV), seed.to(DEV)).cpu()
        assert got.tolist() == peaks * 2, (temp, pairs, got.tolist())


# --------------------------------------------------------------------- #
# top-k / top-p
# --------------------------------------------------------------------- #
def _filter_logits():
    g = torch.Generator().manual_seed(99)
    logits = torch.randn(FILTER_ROWS, FILTER_VOCAB, generator=g)
    for row in logits:
        assert row.unique().numel() == FILTER_VOCAB  # no ties at the k-th
    return logits


def _filter_case(top_k, top_p):
    logits = _filter_logits()
    dev = logits.to(DEV)
    lg64 = logits.double().numpy()
    rows = np.arange(FILTER_ROWS)
    total = mismatch = undecided = 0
    bad = []
    for temp in TEMPS:
        slack = P_SLACK if top_p < 1.0 else 0.0
        strict = gr.keep_set(lg64, temp, top_k, top_p - slack)
        loose = gr.keep_set(lg64, temp, top_k, top_p + slack)
        assert (loose | ~strict).all()       # strict is a subset of loose
        for seed in SEEDS:
            what = "k={} p={} T={} seed={}".format(top_k, top_p, temp, seed)
            got = _ext().sample_top_k_top_p(dev, temp, top_k, top_p,
                                            seed).cpu().numpy()
            assert ((got >= 0) & (got < FILTER_VOCAB)).all(), what
            outside = rows[~loose[rows, got]]
            bad += ["{} row {}: token {} is outside the keep-set".format(
                what, r, got[r]) for r in outside]
            rs = gr.plain_row_seeds(seed, FILTER_ROWS)
            s_loose = gr.scores(lg64, temp, rs, loose)
            s_strict = gr.scores(lg64, temp, rs, strict)
            same = gr.argmax_lowest(s_loose) == gr.argmax_lowest(s_strict)
            undecided += int((~same).sum())
            n, m, b = _judge(got[same], s_loose[same], what)
            total, mismatch, bad = total + n, mismatch + m, bad + b
    return total, mismatch, bad, undecided


@pytest.mark.parametrize("top_k,top_p", FILTERS)
def test_filtered_draw_is_the_replica_argmax_inside_the_keep_set(top_k,
                                                                 top_p):
    total, mismatch, bad, undecided = _once(
        ("filter", top_k, top_p), lambda: _filter_case(top_k, top_p))
    print("rows", total, "not the replica argmax", mismatch,
          "rows where p -/+ 1e-4 changes the winner", undecided)
    assert not bad, "\n".join(bad[:10])
    # the cut moves by at most the tokens whose cumulative probability lies
    # within 1e-4 of p, and such a token wins with about its own probability
    assert undecided * 2 <= total


def test_top_k_1_is_argmax_for_every_seed():
    logits = _filter_logits()
    want = logits.argmax(-1)
    dev = logits.to(DEV)
    for top_p in (1.0, 0.9, 0.1):
        got = torch.stack([
            _ext().sample_top_k_top_p(dev, temp, 1, top_p, seed)
            for temp in TEMPS for seed in PLANT_SEEDS]).cpu()
        assert (got == want).all(), top_p


# --------------------------------------------------------------------- #
# masked sampler
# --------------------------------------------------------------------- #
def _masked_inputs(rows, vocab, dtype, variant):
    """Logits, bank, slots, temperatures and seeds of one batch; every row
    meets every temperature over the three variants, seeds of both signs."""
    logits = _logits(rows, vocab, dtype)
    bank, allowed = guided.make_bank(vocab)
    slot = guided.make_slots(rows, bank.shape[0], seed=variant)
    if variant == 1:
        slot[rows - 1] = -1
    temp = torch.tensor([MASKED_TEMPS[(r + variant) % 3]
                         for r in range(rows)])
    g = torch.Generator().manual_seed(1000 * variant + rows)
    seed = torch.randint(-2**31, 2**31, (rows,), generator=g,
                         dtype=torch.int64).to(torch.int32)
    seed[0] = [-1, 2**31 - 1, -2**31][variant]
    ok = allowed[slot.clamp(min=0).long()] | (slot < 0).unsqueeze(-1)
    return logits, bank, slot, temp, seed, ok


def _run_masked(logits, bank, slot, temp, seed):
    return ops.sample_token_bitmask(
        logits if logits.is_cuda else logits.to(DEV), bank.to(DEV),
        slot.to(DEV), temp.to(DEV), seed.to(DEV)).cpu()


def _masked_score(logits, temp, seed, ok):
    return gr.scores(logits.double().numpy(), temp.numpy(),
                     gr.masked_row_seeds(seed.numpy()), ok.numpy())


def _masked_case(rows, vocab, dtype):
    total = mismatch = 0
    bad = []
    for variant in range(3):
        logits, bank, slot, temp, seed, ok = _masked_inputs(
            rows, vocab, dtype, variant)
        got = _run_masked(logits, bank, slot, temp, seed)
        assert got.dtype == torch.int64 and got.shape == (rows,)
        score = _masked_score(logits, temp, seed, ok)
        n, m, b = _judge(got.numpy(), score, "variant {}".format(variant))
        total, mismatch, bad = total + n, mismatch + m, bad + b
        # a row-strided view that starts 3 elements into its allocation:
        # every row base is misaligned, the scalar head path runs
        wide = torch.zeros(rows, vocab + 13, dtype=dtype, device=DEV)
        view = wide[:, 3:3 + vocab]
        view.copy_(logits)
        assert view.data_ptr() % 16 != 0 and view.stride(0) == vocab + 13
        again = _run_masked(view, bank, slot, temp, seed)
        if not torch.equal(again, got):
            bad.append("variant {}: strided view draws {} != {}".format(
                variant, again.tolist()[:8], got.tolist()[:8]))
    return total, mismatch, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("rows,vocab", MASKED_SHAPES)
def test_masked_draw_is_the_replica_argmax(rows, vocab, dtype):
    total, mismatch, bad = _once(("masked", rows, vocab, dtype),
                                 lambda: _masked_case(rows, vocab, dtype))
    print("rows", total, "not the replica argmax", mismatch)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("rows,vocab", MASKED_SHAPES)
def test_masked_nan_logits_never_win(rows, vocab, dtype):
    logits, bank, slot, temp, seed, ok = _masked_inputs(rows, vocab, dtype, 0)
    # NaN on every row's winner, on token 0 and vocab-1, and on 1% at random
    first = _masked_score(logits, temp, seed, ok)
    win = torch.from_numpy(gr.argmax_lowest(first))
    logits[torch.arange(rows), win] = float("nan")
    logits[:, 0] = float("nan")
    logits[:, vocab - 1] = float("nan")
    g = torch.Generator().manual_seed(3)
    logits[torch.rand(rows, vocab, generator=g) < 0.01] = float("nan")
    got = _run_masked(logits, bank, slot, temp, seed)
    picked = logits[torch.arange(rows), got.clamp(min=0)]
    assert not torch.isnan(picked[got >= 0]).any()
    score = _masked_score(logits, temp, seed, ok)
    # slot[0] is the single-bit row on vocab-1, now NaN: nothing can win
    assert gr.argmax_lowest(score)[0] == -1 and int(got[0]) == -1
    _, _, bad = _judge(got.numpy(), score, "nan")
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("rows,vocab", MASKED_SHAPES)
def test_masked_single_bit_rows(rows, vocab, dtype):
    """A mask with one bit returns that token at any temperature: token 0,
    the last token and the one before it (V=4099 ends in a scalar tail of
    three tokens on an aligned row; the odd row strides of 97, 257 and 4099
    move the other rows' head/tail boundaries around)."""
    only = [0, vocab - 2, vocab - 1]
    allowed = torch.zeros(3, vocab, dtype=torch.bool)
    for i, t in enumerate(only):
        allowed[i, t] = True
    bank = _pack(allowed)
    n = max(rows, 9)   # every (bit, temperature) pair at least once
    logits = _logits(n, vocab, dtype)
    slot = torch.tensor([r % 3 for r in range(n)], dtype=torch.int32)
    temp = torch.tensor([MASKED_TEMPS[(r // 3) % 3] for r in range(n)])
    seed = torch.arange(n, dtype=torch.int32) - n // 2
    got = _run_masked(logits, bank, slot, temp, seed)
    assert got.tolist() == [only[r % 3] for r in range(n)]


@pytest.mark.parametrize("rows,vocab", MASKED_SHAPES)
def test_masked_empty_row_returns_minus_one(rows, vocab):
    n = max(rows, 6)
    logits = _logits(n, vocab, torch.bfloat16)
    bank, _ = guided.make_bank(vocab)
    bank = torch.cat([bank, torch.zeros(1, bank.shape[1],
                                        dtype=torch.int32)])
    empty = bank.shape[0] - 1
    slot = guided.make_slots(n, empty)
    temp = torch.tensor([MASKED_TEMPS[r % 3] for r in range(n)])
    seed = torch.arange(n, dtype=torch.int32) * -7919
    base = _run_masked(logits, bank, slot, temp, seed)
    assert (base >= 0).all()
    hit = torch.zeros(n, dtype=torch.bool)
    hit[[0, 1, 2, n - 1]] = True   # a greedy, a 0.7, a 1.3 row and the last
    got = _run_masked(logits, bank, torch.where(
        hit, torch.tensor(empty, dtype=torch.int32), slot), temp, seed)
    assert (got[hit] == -1).all()
    assert torch.equal(got[~hit], base[~hit])


# --------------------------------------------------------------------- #
# last: the module-wide cap on rows that differ from the replica argmax
# --------------------------------------------------------------------- #
def test_zz_at_most_one_percent_of_rows_differ_from_the_replica():
    results = []
    for rows, vocab in PLAIN_SHAPES:
        for dtype in DTYPES:
            results.append(_once(("plain", rows, vocab, dtype),
                                 lambda: _plain_case(rows, vocab, dtype)))
    for top_k, top_p in FILTERS:
        results.append(_once(("filter", top_k, top_p),
                             lambda: _filter_case(top_k, top_p)))
    for rows, vocab in MASKED_SHAPES:
        for dtype in DTYPES:
            results.append(_once(("masked", rows, vocab, dtype),
                                 lambda: _masked_case(rows, vocab, dtype)))
    total = sum(r[0] for r in results)
    mismatch = sum(r[1] for r in results)
    print("sampling exact: {} of {} rows returned a token other than the "
          "replica argmax".format(mismatch, total))
    assert total > 20000
    assert mismatch * 100 <= total
