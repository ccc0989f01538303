"""Sliding-window attention kernels on gfx950 (attention.hip WINDOW,
attention_decode.hip WINDOW) against the fp32 CPU references of
clearml_serving_amd.ops, plus the engine with decode hipGraphs.

bf16 tolerance atol = rtol = 3e-2: the value tests/test_ops_gpu.py and
tests/test_llm_gpu.py use for the same kernels without a window.
"""

import asyncio

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    FREED_BLOCK, LlmEngine, LlmEngineConfig, SamplingParams)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(atol=3e-2, rtol=3e-2)
BS = 16  # KV page


def close(got, ref):
    got = got.detach().float().cpu()
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, ref.detach().float().cpu(), **TOL)


# --------------------------------------------------------------------- #
# dense prefill
# --------------------------------------------------------------------- #
def dense_qkv(b, h, hkv, s, d, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, h, s, d, generator=g).to(torch.bfloat16)
    k = torch.randn(b, hkv, s, d, generator=g).to(torch.bfloat16)
    v = torch.randn(b, hkv, s, d, generator=g).to(torch.bfloat16)
    return q, k, v


def dense_ref(q, k, v, window, seq_lens=None):
    return ops.attention(q.float(), k.float(), v.float(), causal=True,
                         seq_lens=seq_lens, window=window)


# (S, W): windows below / at / above the 64-key tile and the 128-row block;
# (300, 64) and (257, 128) leave the first tile fully masked for the high
# rows of a block while its low rows still need it
@pytest.mark.parametrize("s,w", [(200, 1), (200, 7), (300, 64), (300, 100),
                                 (257, 128), (300, 129), (96, 500)])
def test_dense_prefill_window(s, w):
    q, k, v = dense_qkv(1, 8, 2, s, 128, seed=s + w)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), causal=True,
                        window=w)
    close(got, dense_ref(q, k, v, w))


def test_dense_prefill_window_d64_bshd():
    q, k, v = dense_qkv(2, 8, 2, 300, 64, seed=1)
    qd, kd, vd = (t.permute(0, 2, 1, 3).contiguous().to(DEV)
                  for t in (q, k, v))
    got = ops.attention(qd, kd, vd, causal=True, layout="bshd", window=100)
    close(got.permute(0, 2, 1, 3), dense_ref(q, k, v, 100))


def test_dense_prefill_window_padded_batch():
    lens = [5, 130, 300]
    q, k, v = dense_qkv(3, 8, 2, 300, 128, seed=2)
    sl = torch.tensor(lens, dtype=torch.int32)
    got = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), causal=True,
                        seq_lens=sl.to(DEV), window=64)
    ref = dense_ref(q, k, v, 64, seq_lens=sl)
    for i, n in enumerate(lens):  # padded query rows are don't-care
        close(got[i, :, :n], ref[i, :, :n])


def test_dense_prefill_window_covering_all_keys_is_bit_equal():
    q, k, v = dense_qkv(3, 8, 2, 300, 128, seed=3)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    base = ops.attention(qd, kd, vd, causal=True)
    for w in (300, 301, 4096):
        assert torch.equal(ops.attention(qd, kd, vd, causal=True, window=w),
                           base)
    # windowed kernel, sequences the window covers: same tiles, same bits
    lens = [5, 130, 300]
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    base = ops.attention(qd, kd, vd, causal=True, seq_lens=sl)
    got = ops.attention(qd, kd, vd, causal=True, seq_lens=sl, window=200)
    for i in (0, 1):
        assert torch.equal(got[i, :, :lens[i]], base[i, :, :lens[i]])
    with pytest.raises(ValueError):
        ops.attention(qd, kd, vd, causal=False, window=64)


# --------------------------------------------------------------------- #
# paged caches
# --------------------------------------------------------------------- #
def paged_case(kv_lens, hkv, d, seed, fp8=False):
    """Shuffled pages for each sequence. Page 0 is the spare: never mapped,
    inside the cache tensor. Returns device caches + fp32 CPU copies."""
    g = torch.Generator().manual_seed(seed)
    nblk = [(n + BS - 1) // BS for n in kv_lens]
    total = sum(nblk) + 1
    kf = torch.randn(total, hkv, BS, d, generator=g).to(torch.bfloat16)
    vf = torch.randn(total, hkv, BS, d, generator=g).to(torch.bfloat16)
    perm = (torch.randperm(total - 1, generator=g) + 1).tolist()
    btab = torch.zeros(len(kv_lens), max(nblk), dtype=torch.int32)
    at = 0
    for i, n in enumerate(nblk):
        btab[i, :n] = torch.tensor(perm[at:at + n], dtype=torch.int32)
        btab[i, n:] = perm[at]  # padding entries stay in range
        at += n
    case = {"btab": btab, "scales": {}}
    if fp8:
        k8 = torch.zeros(total, hkv, BS, d, device=DEV, dtype=torch.uint8)
        v8 = torch.zeros_like(k8)
        ks = torch.ones(total, hkv, BS, device=DEV)
        vs = torch.ones_like(ks)
        slots = torch.arange(total * BS, dtype=torch.int32, device=DEV)
        ops.kv_cache_write(
            kf.permute(0, 2, 1, 3).reshape(-1, hkv, d).contiguous().to(DEV),
            vf.permute(0, 2, 1, 3).reshape(-1, hkv, d).contiguous().to(DEV),
            k8, v8, slots, ks, vs)
        case.update(k=k8, v=v8, scales={"k_scale": ks, "v_scale": vs},
                    k_ref=ops._dequant_kv_cpu(k8.cpu(), ks.cpu()),
                    v_ref=ops._dequant_kv_cpu(v8.cpu(), vs.cpu()))
    else:
        case.update(k=kf.to(DEV), v=vf.to(DEV), k_ref=kf.float(),
                    v_ref=vf.float())
    return case


def stale_table(btab, first_keys):
    """Entries wholly below each sequence's first visible key -> page 0."""
    out = btab.clone()
    for i, first in enumerate(first_keys):
        out[i, :max(0, first) // BS] = 0
    return out


def poison_spare(case):
    case["k"][0] = float("nan")
    case["v"][0] = float("nan")


KV_LENS, Q_LENS = [40, 333], [8, 77]


def paged_prefill(case, q, window, btab=None):
    btab = case["btab"] if btab is None else btab
    kl = torch.tensor(KV_LENS, dtype=torch.int32, device=DEV)
    ql = torch.tensor(Q_LENS, dtype=torch.int32, device=DEV)
    return ops.attention_prefill_paged(q.to(DEV), case["k"], case["v"],
                                       btab.to(DEV), kl, ql, window=window,
                                       **case["scales"])


def paged_prefill_ref(case, q, window):
    return ops.attention_prefill_paged(
        q.float(), case["k_ref"], case["v_ref"], case["btab"],
        torch.tensor(KV_LENS, dtype=torch.int32),
        torch.tensor(Q_LENS, dtype=torch.int32), window=window)


def check_paged_prefill(got, ref):
    for i, n in enumerate(Q_LENS):
        close(got[i, :n], ref[i, :n])


def prefill_q(d, seed=20):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, max(Q_LENS), 8, d, generator=g).to(torch.bfloat16)


@pytest.fixture(scope="module")
def prefill_case():
    return paged_case(KV_LENS, 2, 128, seed=21)


@pytest.mark.parametrize("w", [16, 50, 64])
def test_paged_prefill_window(prefill_case, w):
    q = prefill_q(128)
    check_paged_prefill(paged_prefill(prefill_case, q, w),
                        paged_prefill_ref(prefill_case, q, w))


def test_paged_prefill_window_d64():
    case = paged_case(KV_LENS, 2, 64, seed=22)
    q = prefill_q(64)
    check_paged_prefill(paged_prefill(case, q, 50),
                        paged_prefill_ref(case, q, 50))


def test_paged_prefill_window_fp8_kv():
    case = paged_case(KV_LENS, 2, 128, seed=23, fp8=True)
    q = prefill_q(128)
    check_paged_prefill(paged_prefill(case, q, 50),
                        paged_prefill_ref(case, q, 50))


def test_paged_prefill_window_covering_all_keys_is_bit_equal(prefill_case):
    q = prefill_q(128)
    base = paged_prefill(prefill_case, q, None)
    for w in (333, 4096):
        got = paged_prefill(prefill_case, q, w)
        for i, n in enumerate(Q_LENS):
            assert torch.equal(got[i, :n], base[i, :n])
    # windowed kernel (W < longest sequence): the sequence it covers
    got = paged_prefill(prefill_case, q, 100)
    assert torch.equal(got[0, :Q_LENS[0]], base[0, :Q_LENS[0]])


@pytest.mark.parametrize("w", [16, 50, 64])
def test_paged_prefill_never_reads_pages_below_the_window(w):
    case = paged_case(KV_LENS, 2, 128, seed=24)
    q = prefill_q(128)
    ref = paged_prefill_ref(case, q, w)
    stale = stale_table(case["btab"], [kv - ql - w + 1
                                       for kv, ql in zip(KV_LENS, Q_LENS)])
    assert (stale[1] == 0).sum() >= (333 - 77 - w + 1) // BS > 0
    poison_spare(case)
    check_paged_prefill(paged_prefill(case, q, w, btab=stale), ref)


# --------------------------------------------------------------------- #
# decode
# --------------------------------------------------------------------- #
SEQS = [1, 17, 200, 1000]


def decode_q(b, h, d, seed=30):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, h, d, generator=g).to(torch.bfloat16)


def decode(case, q, seqs, window, btab=None):
    btab = case["btab"] if btab is None else btab
    sl = torch.tensor(seqs, dtype=torch.int32, device=DEV)
    return ops.attention_decode(q.to(DEV), case["k"], case["v"],
                                btab.to(DEV), sl, window=window,
                                **case["scales"])


def decode_ref(case, q, seqs, window):
    return ops.attention_decode(q.float(), case["k_ref"], case["v_ref"],
                                case["btab"],
                                torch.tensor(seqs, dtype=torch.int32),
                                window=window)


@pytest.fixture(scope="module")
def decode_case():
    return paged_case(SEQS, 2, 128, seed=31)


@pytest.mark.parametrize("w", [1, 5, 16, 100, 4096])
def test_decode_window(decode_case, w):
    q = decode_q(len(SEQS), 8, 128)
    close(decode(decode_case, q, SEQS, w),
          decode_ref(decode_case, q, SEQS, w))


def test_decode_window_empty_splits():
    """B=1 runs 16 flash-decoding splits; a 37-key window gives each split
    a 16-key chunk, so 13 of them are empty and publish the neutral
    partial."""
    case = paged_case([1000], 2, 128, seed=32)
    q = decode_q(1, 8, 128)
    close(decode(case, q, [1000], 37), decode_ref(case, q, [1000], 37))


def test_decode_window_d64():
    case = paged_case(SEQS, 2, 64, seed=33)
    q = decode_q(len(SEQS), 8, 64)
    close(decode(case, q, SEQS, 100), decode_ref(case, q, SEQS, 100))


def test_decode_window_fp8_kv():
    case = paged_case(SEQS, 2, 128, seed=34, fp8=True)
    q = decode_q(len(SEQS), 8, 128)
    close(decode(case, q, SEQS, 100), decode_ref(case, q, SEQS, 100))


def test_decode_window_covering_all_keys_is_bit_equal(decode_case):
    q = decode_q(len(SEQS), 8, 128)
    base = decode(decode_case, q, SEQS, None)
    # 1000 and 1007 run the windowed kernel (the table spans 1008 keys),
    # 4096 can never bind and takes the windowless one
    for w in (1000, 1007, 4096):
        assert torch.equal(decode(decode_case, q, SEQS, w), base)
    # a binding window leaves the sequences it covers untouched
    got = decode(decode_case, q, SEQS, 200)
    assert torch.equal(got[:3], base[:3])
    assert not torch.equal(got[3], base[3])


@pytest.mark.parametrize("w", [1, 5, 16, 100])
def test_decode_never_reads_pages_below_the_window(w):
    case = paged_case(SEQS, 2, 128, seed=35)
    q = decode_q(len(SEQS), 8, 128)
    ref = decode_ref(case, q, SEQS, w)
    stale = stale_table(case["btab"], [n - w for n in SEQS])
    assert (stale[3] == 0).sum() == (1000 - w) // BS
    poison_spare(case)
    close(decode(case, q, SEQS, w, btab=stale), ref)


# --------------------------------------------------------------------- #
# engine
# --------------------------------------------------------------------- #
def run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


def test_engine_window_graphs_match_eager():
    prompt = [3, 7, 11, 19, 23, 29, 31, 37, 41, 43] * 4

    def gen(graphs):
        eng = LlmEngine(LlmEngineConfig(
            preset="mistral-tiny", num_kv_blocks=12, block_size=BS,
            max_model_len=160, device=DEV, max_num_seqs=4,
            decode_graphs=graphs))
        eng.start()
        window = eng.model_config.sliding_window
        assert window == 24
        held = []
        inner = eng.step

        def step():
            inner()
            held.extend(sum(b != FREED_BLOCK for b in s.blocks)
                        for s in eng.running)

        eng.step = step

        async def go():
            seq = await eng.add_request(list(prompt), SamplingParams(
                temperature=0.0, max_tokens=80, ignore_eos=True))
            toks = []
            while True:
                item = await seq.stream.get()
                assert "error" not in item, item
                toks.extend(item["token_ids"])
                if item["finished"]:
                    return toks

        toks = run(go())
        assert len(prompt) + len(toks) >= 4 * window
        assert eng.stats["swa_blocks_freed"] > 0
        assert max(held) <= -(-window // BS) + 2
        assert eng.allocator.available == eng.allocator.num_blocks
        assert (eng.stats["graph_replays"] > 0) == graphs
        return toks

    assert gen(True) == gen(False)
