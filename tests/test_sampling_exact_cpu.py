"""CPU: the replica of the sampling kernels' gumbel-max draw
(helpers/gumbel_ref.py) checked against hand-computed values, the uniform
mapping checked over its whole range, and the replica shown to be a correct
categorical sampler -- which is what lets test_sampling_exact_gpu.py conclude
"kernel == replica" => "kernel samples softmax(logits / T)".
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))
import gumbel_ref as gr  # noqa: E402

# pcg_hash worked out with Python integers, step by step:
#   x = (x * 747796405 + 2891336453) mod 2^32
#   w = ((x >> ((x >> 28) + 4)) ^ x) * 277803737 mod 2^32
#   return (w >> 22) ^ w
HASHES = {0: 129708002, 1: 2831084092, 2: 2055130248, 9781: 3949268940,
          0x80000000: 566699590, 0xFFFFFFFF: 3861530882,
          123456789: 4272394698}

# vocabulary 4096, row 0: (seed, token) whose hash lies in the top 128 values
TAIL_PAIRS_4096 = [(2697, 2891), (18583, 488), (27529, 1282)]


def _py_pcg(x):
    x = (x * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((x >> ((x >> 28) + 4)) ^ x) * 277803737) & 0xFFFFFFFF
    return (w >> 22) ^ w


def test_pcg_hash_matches_hand_computed_values():
    for x, want in HASHES.items():
        assert _py_pcg(x) == want
        assert int(gr.pcg_hash(x)[0]) == want
    xs = np.random.default_rng(0).integers(0, 2**32, 4096, dtype=np.uint64)
    got = gr.pcg_hash(xs.astype(np.uint32))
    assert got.dtype == np.uint32
    assert got.tolist() == [_py_pcg(int(x)) for x in xs]


def test_row_seeds():
    # plain sampler: seed cast long -> uint32, row r mixes in r * 9781
    assert gr.plain_row_seeds(5, 3).tolist() == [
        _py_pcg(5), _py_pcg(5 ^ 9781), _py_pcg(5 ^ 19562)]
    assert gr.plain_row_seeds(-3, 1).tolist() == [_py_pcg(0xFFFFFFFD)]
    assert gr.plain_row_seeds(2**33 + 7, 1).tolist() == [_py_pcg(7)]
    # the row term wraps modulo 2^32 as well
    big = gr.plain_row_seeds(1, 500000)
    assert int(big[-1]) == _py_pcg(1 ^ ((499999 * 9781) & 0xFFFFFFFF))
    # masked sampler: int32 seed reinterpreted as uint32, no row term
    assert gr.masked_row_seeds([0, 7, -1, -2**31, 2**31 - 1]).tolist() == [
        _py_pcg(0), _py_pcg(7), _py_pcg(0xFFFFFFFF), _py_pcg(0x80000000),
        _py_pcg(0x7FFFFFFF)]
    # row 0 of the plain sampler and the masked sampler share a stream
    assert gr.plain_row_seeds(2697, 1).tolist() == \
        gr.masked_row_seeds([2697]).tolist()


def test_searcher_finds_the_known_tail_pairs():
    for row in (0, None):
        hits = gr.find_hash_hits(4096, gr.TAIL_LO, gr.TAIL_HI, range(30000),
                                 row=row, count=3)
        assert [(s, t) for s, t, _ in hits] == TAIL_PAIRS_4096
        for seed, tok, h in hits:
            assert _py_pcg((_py_pcg(seed) + tok) & 0xFFFFFFFF) == h
            assert h >= 2**32 - 128
    # negative int32 seeds and a non-zero row, checked with Python integers
    (seed, tok, h), = gr.find_hash_hits(4096, gr.TAIL_LO, gr.TAIL_HI,
                                        range(-1, -60000, -1), count=1)
    assert seed < 0
    assert _py_pcg((_py_pcg(seed & 0xFFFFFFFF) + tok) & 0xFFFFFFFF) == h
    (seed, tok, h), = gr.find_hash_hits(128256, gr.TAIL_LO, gr.TAIL_HI,
                                        range(3000), row=1, count=1)
    assert _py_pcg((_py_pcg(seed ^ 9781) + tok) & 0xFFFFFFFF) == h
    assert h >= 2**32 - 128


def test_uniform_is_strictly_inside_the_unit_interval():
    """u == 0 or u == 1 makes the gumbel term infinite, and a token with
    g == +inf wins its row whatever its logit is. (float)h + 1.0f did that
    for the top 128 hashes."""
    rng = np.random.default_rng(1)
    h = np.concatenate([
        np.array([0, 2**32 - 1], dtype=np.uint64),
        np.arange(2**16, dtype=np.uint64),
        np.arange(2**32 - 2**16, 2**32, dtype=np.uint64),
        rng.integers(0, 2**32, 1_000_000, dtype=np.uint64),
    ]).astype(np.uint32)
    u = gr.uniform_from_hash(h)
    assert u.dtype == np.float32
    assert (u > 0).all() and (u < 1).all()
    assert u.min() == np.float32(2.0**-24)
    assert u.max() == np.float32(1.0) - np.float32(2.0**-24)
    # exact: u * 2^23 - 0.5 recovers the 23 hash bits
    assert np.array_equal(u.astype(np.float64) * 2**23 - 0.5,
                          (h >> np.uint32(9)).astype(np.float64))
    g = gr.gumbel_from_uniform(u)
    assert np.isfinite(g).all()
    assert gr.G_MIN < g.min() and g.max() < gr.G_MAX
    # also in the kernels' own precision
    with np.errstate(divide="ignore"):
        g32 = -np.log(-np.log(u))
    assert g32.dtype == np.float32 and np.isfinite(g32).all()


def test_scores_and_tie_rule():
    logits = np.array([[1.0, np.nan, -np.inf, 3.0, 3.0, 0.5]])
    allowed = np.array([[True, True, True, True, True, False]])
    rs = gr.masked_row_seeds([11])
    s = gr.scores(logits, 0.7, rs, allowed)
    assert np.isneginf(s[0, [1, 2, 5]]).all()
    h = gr.token_hashes(rs, 6)[0]
    inv_t = float(np.float32(1.0) / np.float32(0.7))
    for t in (0, 3, 4):
        u = (float(int(h[t]) >> 9) + 0.5) / 2**23
        want = float(logits[0, t]) * inv_t - np.log(-np.log(u))
        assert abs(s[0, t] - want) < 1e-12
    # greedy row: the score is the logit; ties and -0.0 go to the lowest index
    s0 = gr.scores(logits, 0.0, rs, allowed)
    assert gr.argmax_lowest(s0).tolist() == [3]
    z = gr.scores(np.array([[-1.0, -0.0, 0.0]]), 0.0, rs)
    assert gr.argmax_lowest(z).tolist() == [1]
    dead = gr.scores(logits, 1.0, rs, np.zeros((1, 6), dtype=bool))
    assert gr.argmax_lowest(dead).tolist() == [-1]


def test_keep_set_definition():
    lg = np.log(np.array([[0.5, 0.2, 0.2, 0.06, 0.04]]))
    assert gr.keep_set(lg, 1.0, 0, 1.0).all()
    assert gr.keep_set(lg, 1.0, 5, 1.0).all()
    # top-k keeps everything >= the k-th value, ties included
    assert gr.keep_set(lg, 1.0, 1, 1.0).tolist() == [[1, 0, 0, 0, 0]]
    assert gr.keep_set(lg, 1.0, 2, 1.0).tolist() == [[1, 1, 1, 0, 0]]
    # top-p drops tokens whose inclusive cumulative probability exceeds p
    assert gr.keep_set(lg, 1.0, 0, 0.95).tolist() == [[1, 1, 1, 0, 0]]
    assert gr.keep_set(lg, 1.0, 0, 0.75).tolist() == [[1, 1, 0, 0, 0]]
    assert gr.keep_set(lg, 1.0, 0, 0.1).tolist() == [[1, 0, 0, 0, 0]]
    # the temperature sharpens the distribution top-p sees
    assert gr.keep_set(lg, 0.25, 0, 0.95).tolist() == [[1, 0, 0, 0, 0]]
    # top-p works on the softmax of what top-k left: 0.5 / 0.9 < 0.6
    assert gr.keep_set(lg, 1.0, 3, 0.6).tolist() == [[1, 0, 0, 0, 0]]
    assert gr.keep_set(lg, 1.0, 3, 0.8).tolist() == [[1, 1, 0, 0, 0]]


def test_replica_draws_follow_softmax():
    """200 000 (seed, row) draws on one V = 8 logit vector: chi-square of
    the replica's argmax counts against the float64 softmax, 7 degrees of
    freedom, below the 99.99th percentile (29.88). The seeds are fixed, so
    the statistic is one fixed number (printed)."""
    logits = np.array([2.0, 1.5, 1.0, 0.5, 0.0, -0.5, -1.0, -2.0])
    temperature, seeds, rows = 0.7, 200, 1000
    counts = np.zeros(8)
    batch = np.tile(logits, (rows, 1))
    for seed in range(seeds):
        s = gr.scores(batch, temperature, gr.plain_row_seeds(seed, rows))
        counts += np.bincount(gr.argmax_lowest(s), minlength=8)
    n = seeds * rows
    assert counts.sum() == n == 200_000
    z = logits * float(gr.inv_temperature(temperature))
    p = np.exp(z - z.max())
    p /= p.sum()
    chi2 = float(((counts - n * p) ** 2 / (n * p)).sum())
    print("chi-square", chi2, "counts", counts.tolist())
    assert chi2 < 29.88
