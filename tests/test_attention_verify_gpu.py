"""Multi-query split-KV paged attention (ops.attention_decode_multi,
attention_verify.hip) against the fp32 CPU reference of
ops.attention_prefill_paged, against ops.attention_decode at one query
token, and through the engine's ngram verification forward."""

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine,
    LlmEngineConfig,
    SamplingParams,
)
from tests.test_llm_gpu import run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAGE = 16
TOL = 3e-2     # the sibling kernels' bound against the same references
POISON = 1e4   # a key or value that escapes the mask dominates its row


def build_cache(hkv, d, kv_lens, q_lens, fp8=False, window=0, seed=0):
    """Paged caches on the GPU for one batch: the block table is a random
    permutation of the pages, every slot at or past kv_len, every
    unreferenced page and (with a window) every page wholly below the first
    row's window start is poison."""
    gen = torch.Generator().manual_seed(seed)
    nbs = [max(1, -(-n // PAGE)) for n in kv_lens]
    pages = sum(nbs) + 2
    perm = torch.randperm(pages, generator=gen).tolist()
    poison_page = perm.pop()
    btab = torch.full((len(kv_lens), max(nbs)), poison_page,
                      dtype=torch.int32)
    slots = []
    for i, (n, nb) in enumerate(zip(kv_lens, nbs)):
        btab[i, :nb] = torch.tensor([perm.pop() for _ in range(nb)])
        slots += [int(btab[i, p // PAGE]) * PAGE + p % PAGE for p in range(n)]
        if window:
            btab[i, :max(0, n - q_lens[i] - window + 1) // PAGE] = poison_page
    t = len(slots)
    k_new = torch.randn(t, hkv, d, generator=gen).to(DEV, torch.bfloat16)
    v_new = torch.randn(t, hkv, d, generator=gen).to(DEV, torch.bfloat16)
    slots = torch.tensor(slots, dtype=torch.int32, device=DEV)
    shape = (pages, hkv, PAGE, d)
    if fp8:  # 0x7e = 448, the largest finite e4m3; 448 * 32 > POISON
        k = torch.full(shape, 0x7E, dtype=torch.uint8, device=DEV)
        v = k.clone()
        ks = torch.full(shape[:3], 32.0, device=DEV)
        vs = ks.clone()
    else:
        k = torch.full(shape, POISON, dtype=torch.bfloat16, device=DEV)
        v = k.clone()
        ks = vs = None
    ops.kv_cache_write(k_new, v_new, k, v, slots, ks, vs)
    return {"k": k, "v": v, "ks": ks, "vs": vs, "btab": btab.to(DEV),
            "kv": torch.tensor(kv_lens, dtype=torch.int32, device=DEV),
            "ql": torch.tensor(q_lens, dtype=torch.int32, device=DEV),
            "window": window}


def check_against_reference(case, q, q_lens):
    cpu = {n: (t.cpu() if torch.is_tensor(t) else t) for n, t in case.items()}
    got = ops.attention_decode_multi(
        q, case["k"], case["v"], case["btab"], case["kv"], case["ql"],
        k_scale=case["ks"], v_scale=case["vs"], window=case["window"])
    ref = ops.attention_prefill_paged(
        q.cpu(), cpu["k"], cpu["v"], cpu["btab"], cpu["kv"], cpu["ql"],
        k_scale=cpu["ks"], v_scale=cpu["vs"], window=cpu["window"])
    assert got.shape == q.shape
    for i, n in enumerate(q_lens):
        g, r = got[i, :n].float().cpu(), ref[i, :n].float()
        assert torch.isfinite(g).all()
        torch.testing.assert_close(g, r, atol=TOL, rtol=TOL)


EDGE_Q = [1, 3, 8, 0]
CASES = [
    # h, hkv, sq, d, kv_lens, q_lens, fp8, window
    # row tiles: R = 1, 16, 20, 56, 64
    pytest.param(4, 4, 1, 128, [45, 200], [1, 1], False, 0, id="R1"),
    pytest.param(8, 2, 4, 128, [45, 200], [4, 2], False, 0, id="R16"),
    pytest.param(8, 2, 5, 128, [45, 200], [5, 3], False, 0, id="R20"),
    pytest.param(28, 4, 8, 128, [45, 200], [8, 6], False, 0, id="R56"),
    pytest.param(8, 1, 8, 128, [45, 200], [8, 6], False, 0, id="R64"),
    pytest.param(8, 2, 5, 64, [45, 200], [5, 3], False, 0, id="R20-d64"),
    # key-range edges: no history, around one page / one tile, every split
    pytest.param(16, 8, 8, 128, EDGE_Q, EDGE_Q, False, 0, id="kv=qlen"),
    *[pytest.param(16, 8, 8, 128, [n] * 4, EDGE_Q, False, 0,
                   id="kv={}".format(n)) for n in (15, 16, 17, 33, 700)],
    # fp8 KV
    pytest.param(8, 2, 5, 128, [45, 200], [5, 3], True, 0, id="R20-fp8"),
    pytest.param(16, 8, 8, 128, [700] * 4, EDGE_Q, True, 0, id="kv=700-fp8"),
    # window: below Sq, below a key tile, crossing a tile, covering all
    *[pytest.param(8, 2, 5, 128, [300, 300], [5, 3], False, w,
                   id="window={}".format(w)) for w in (1, 7, 40, 4096)],
]


@pytest.mark.parametrize("h,hkv,sq,d,kv_lens,q_lens,fp8,window", CASES)
def test_decode_multi_matches_reference(h, hkv, sq, d, kv_lens, q_lens, fp8,
                                        window):
    case = build_cache(hkv, d, kv_lens, q_lens, fp8=fp8, window=window)
    torch.manual_seed(1)
    q = torch.randn(len(kv_lens), sq, h, d).to(DEV, torch.bfloat16)
    check_against_reference(case, q, q_lens)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_multi_one_token_matches_decode(fp8):
    kv_lens = [1, 33, 700]
    case = build_cache(2, 128, kv_lens, [1, 1, 1], fp8=fp8)
    torch.manual_seed(2)
    q = torch.randn(3, 1, 8, 128).to(DEV, torch.bfloat16)
    got = ops.attention_decode_multi(
        q, case["k"], case["v"], case["btab"], case["kv"], case["ql"],
        k_scale=case["ks"], v_scale=case["vs"])
    want = ops.attention_decode(
        q[:, 0], case["k"], case["v"], case["btab"], case["kv"],
        k_scale=case["ks"], v_scale=case["vs"])
    assert torch.isfinite(got.float()).all()
    torch.testing.assert_close(got[:, 0].float(), want.float(), atol=TOL,
                               rtol=TOL)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_verify_takes_multi_kernel(kv_dtype, monkeypatch):
    """Greedy ngram speculation is token-identical to plain decoding, its
    verify forwards run the multi-query kernel, and CMLS_VERIFY_ATTN=0
    sends them back through the chunked-prefill kernel."""
    def gen(speculative):
        torch.manual_seed(11)
        eng = LlmEngine(LlmEngineConfig(
            preset="llama-tiny", num_kv_blocks=128, block_size=16,
            max_model_len=256, device=DEV, max_num_seqs=8,
            kv_dtype=kv_dtype, speculative=speculative))
        eng.start()

        async def go():
            toks = []
            async for item in eng.generate("abcabcabcabcabc", SamplingParams(
                    temperature=0.0, max_tokens=12, ignore_eos=True)):
                toks.extend(item["token_ids"])
            return toks

        return run(go()), eng.stats

    spec_cfg = {"method": "ngram", "num_spec_tokens": 4, "ngram": 2}
    plain, _ = gen(None)
    spec, stats = gen(spec_cfg)
    assert spec == plain
    assert stats["spec_verify_multi"] > 0 and stats["spec_accepted"] > 0
    monkeypatch.setenv("CMLS_VERIFY_ATTN", "0")
    old, old_stats = gen(spec_cfg)
    assert old == plain
    assert old_stats["spec_verify_multi"] == 0
