"""CPU replica of the gumbel-max draw of the two sampling kernels.

gumbel_argmax_kernel (ops/csrc/sampling.hip) and sample_token_bitmask_kernel
(ops/csrc/token_mask.hip) pick, per row,

    argmax_t  logit[t] * inv_temp + g(t),   g = -log(-log(u(t)))

with noise that is a pure function of (seed, row, token):

    row_seed = pcg(seed ^ (row * 9781))      plain sampler, seed cast to uint32
    row_seed = pcg((uint32) seed[row])       masked sampler, per-row int32 seed
    h        = pcg(row_seed + token)
    u        = ((float)(h >> 9) + 0.5f) * 2^-23      exact in fp32

so the token a kernel must return for given (logits, temperature, seed) can
be stated from numpy alone. The integer part is reproduced bit-exactly with
uint32 arithmetic and u is evaluated in float32 exactly as the kernels do;
g and the score are evaluated in float64. The kernels evaluate them in fp32
with the native log, so they may differ from the replica only where the two
best scores of a row are closer than that error (see MARGIN).

Nothing in this file calls the code under test.
"""

import numpy as np

U32 = np.uint32

# A kernel's token is accepted when its replica score is within MARGIN of the
# replica's best. Derivation: scores stay below 64 in magnitude, where the
# fp32 ulp is 3.8e-6; the native log is good to a few ulp and nesting it turns
# the inner log's relative error into an absolute error of g: about 1e-5 in
# total. MARGIN is 100 times that.
MARGIN = 1e-3

# (float)h rounds every h >= 2^32 - 128 up to 2^32: the hashes for which the
# kernels' earlier formula u = ((float)h + 1) * 2^-32 gave u == 1, g == +inf.
TAIL_LO = 2**32 - 128
TAIL_HI = 2**32 - 1

# every u lies in [2^-24, 1 - 2^-24], so g lies inside (G_MIN, G_MAX)
G_MIN = -2.82
G_MAX = 16.64


def pcg_hash(x):
    """The kernels' pcg_hash on a uint32 array (wraps modulo 2^32)."""
    x = np.atleast_1d(np.asarray(x)).astype(U32)
    x = x * U32(747796405) + U32(2891336453)
    w = ((x >> ((x >> U32(28)) + U32(4))) ^ x) * U32(277803737)
    return (w >> U32(22)) ^ w


def plain_row_seeds(seed, rows):
    """sampling.hip: the long seed is cast to unsigned int by the wrapper."""
    s = U32(int(seed) & 0xFFFFFFFF)
    return pcg_hash(s ^ (np.arange(rows, dtype=U32) * U32(9781)))


def masked_row_seeds(seeds):
    """token_mask.hip: (unsigned int)seed[row] of an int32 seed, so -1 is
    0xFFFFFFFF."""
    s = np.atleast_1d(np.asarray(seeds, dtype=np.int64))
    assert ((s >= -2**31) & (s < 2**31)).all(), "seeds are int32"
    return pcg_hash((s & 0xFFFFFFFF).astype(U32))


def token_hashes(row_seeds, vocab):
    """h[r, t] = pcg(row_seed[r] + t), uint32 [R, V]."""
    rs = np.atleast_1d(np.asarray(row_seeds)).astype(U32)
    return pcg_hash(rs[:, None] + np.arange(vocab, dtype=U32)[None, :])


def uniform_from_hash(h):
    """The kernels' u, evaluated in float32 operation by operation."""
    h = np.atleast_1d(np.asarray(h)).astype(U32)
    top = (h >> U32(9)).astype(np.float32)
    return (top + np.float32(0.5)) * np.float32(1.0 / 8388608.0)


def gumbel_from_uniform(u):
    """g = -log(-log(u)) in float64 (of the float32 u)."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.log(-np.log(u))


def inv_temperature(temperature):
    """Both wrappers/kernels form 1.0f / (float)T in fp32."""
    return np.float32(1.0) / np.float32(temperature)


def scores(logits, temperature, row_seeds, allowed=None):
    """Replica scores, float64 [R, V]; -inf means "never wins".

    logits: [R, V], any float dtype holding exactly the values the kernel
    reads (i.e. already rounded to bf16/fp16/fp32). temperature: a scalar or
    [R]; 0 marks a greedy row (masked sampler), whose score is the logit
    itself. allowed: optional bool [R, V] mask. Filtered (-inf), masked and
    NaN logits get -inf.
    """
    lg = np.asarray(logits, dtype=np.float64)
    rows, vocab = lg.shape
    temp = np.broadcast_to(
        np.asarray(temperature, dtype=np.float32), (rows,))
    g = gumbel_from_uniform(uniform_from_hash(token_hashes(row_seeds, vocab)))
    out = np.empty_like(lg)
    for r in range(rows):
        if temp[r] > 0:
            inv_t = np.float64(inv_temperature(temp[r]))
            out[r] = lg[r] * inv_t + g[r]
        else:
            out[r] = lg[r]
    dead = np.isnan(lg) | (lg == -np.inf)
    if allowed is not None:
        dead |= ~np.asarray(allowed, dtype=bool)
    out[dead] = -np.inf
    return out


def argmax_lowest(score):
    """Row-wise argmax, lowest index on ties; -1 where nothing can win."""
    best = score.argmax(axis=-1)  # numpy returns the first maximum
    live = (score > -np.inf).any(axis=-1)
    return np.where(live, best, -1)


def find_hash_hits(vocab, h_lo, h_hi, seeds, row=None, count=1,
                   seeds_per_step=2048):
    """First `count` (seed, token, h) with h_lo <= h <= h_hi, walking
    `seeds` in order and tokens [0, vocab) within a seed.

    row=None uses the masked sampler's seeding (seeds are int32 values);
    row=r uses the plain sampler's seeding for row r of the batch.
    """
    seeds = np.asarray(list(seeds), dtype=np.int64)
    step = max(1, min(seeds_per_step, (1 << 24) // vocab))
    hits = []
    for i in range(0, len(seeds), step):
        part = seeds[i:i + step]
        if row is None:
            rs = masked_row_seeds(part)
        else:
            rs = pcg_hash((part & 0xFFFFFFFF).astype(U32)
                          ^ U32((row * 9781) & 0xFFFFFFFF))
        h = token_hashes(rs, vocab)
        si, ti = np.nonzero((h >= U32(h_lo)) & (h <= U32(h_hi)))
        for s, t in zip(si, ti):
            hits.append((int(part[s]), int(t), int(h[s, t])))
            if len(hits) == count:
                return hits
    raise LookupError("only {} of {} hits in {} seeds".format(
        len(hits), count, len(seeds)))


def keep_set(logits, temperature, top_k, top_p):
    """bool [R, V]: the tokens top-k / top-p filtering keeps, in float64.

    top-k (0 < k < V) keeps everything >= the k-th largest logit. top-p
    (p < 1) then sorts the survivors by descending probability under
    softmax(logit / T) and drops those whose inclusive cumulative
    probability exceeds p; the top token is always kept.
    """
    lg = np.asarray(logits, dtype=np.float64)
    rows, vocab = lg.shape
    keep = np.ones((rows, vocab), dtype=bool)
    if 0 < top_k < vocab:
        kth = np.sort(lg, axis=-1)[:, vocab - top_k]
        keep = lg >= kth[:, None]
    if top_p < 1.0:
        z = np.where(keep, lg, -np.inf) / float(temperature)
        z = z - z.max(axis=-1, keepdims=True)
        prob = np.exp(z)
        prob /= prob.sum(axis=-1, keepdims=True)
        order = np.argsort(-prob, axis=-1, kind="stable")
        cum = np.cumsum(np.take_along_axis(prob, order, -1), axis=-1)
        cut = cum > top_p
        cut[:, 0] = False
        dropped = np.zeros_like(keep)
        np.put_along_axis(dropped, order, cut, -1)
        keep &= ~dropped
    return keep
