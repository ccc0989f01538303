"""Tiled MXFP4 prefill GEMM on the GPU (csrc/mxfp4_gemm.hip): against a
float64 product of the same quantised operands, the operand maps through the
LDS path, row invariance, Mxfp4Linear's "tiled" route and the engine."""

import asyncio
import copy

import pytest
import torch

import clearml_serving_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gemm_and_ref(a8, xs, w4, e8, rs, tile=0):
    w4t, e8t = ops.tile_mxfp4_weight(w4, e8)
    got = ops.gemm_mxfp4(a8.to(DEV), xs.to(DEV), w4t.to(DEV), e8t.to(DEV),
                         rs.to(DEV), tile=tile)
    a = (a8.view(torch.float8_e4m3fn).float() * xs[:, None]).double()
    w = ops.dequant_mxfp4(w4, e8, rs).double()
    return got.double().cpu(), a @ w.T, a.abs() @ w.abs().T


def _operands(m, k, n):
    g = torch.Generator().manual_seed(m * 1000 + k + n)
    a8, xs = ops._quant_fp8_ref(torch.randn(m, k, generator=g))
    blocks = torch.randn(n, k // 32, 32, generator=g) * torch.exp2(
        torch.randint(-6, 6, (n, k // 32, 1), generator=g).float())
    w4, e8, _ = ops.quantize_mxfp4(blocks.reshape(n, k))
    return a8, xs, w4, e8, torch.rand(n, generator=g) + 0.5


@pytest.mark.parametrize("tile", [64, 128])  # both instantiations
@pytest.mark.parametrize("n", [128, 384])
@pytest.mark.parametrize("k", [128, 640, 1024])
@pytest.mark.parametrize("m", [1, 65, 127, 128, 129, 300])
def test_gemm_mxfp4_matches_float64(m, k, n, tile):
    got, ref, mag = _gemm_and_ref(*_operands(m, k, n), tile=tile)
    # products are exact in fp32: only fp32 accumulation + the bf16 store
    bound = 2.0 ** -8 * ref.abs() + k * 2.0 ** -23 * mag
    excess = ((got - ref).abs() - bound).max().item()
    print("max excess over bound: {:.3e}".format(excess))
    assert got.shape == (m, n) and excess <= 0


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("k", [128, 256])
@pytest.mark.parametrize("pattern", ["values", "scales", "even", "odd"])
def test_operand_maps_exact(pattern, k, tile):
    """One e4m3 1.0 per A row at column 7m % K picks single weights out, so
    every output is one dequantised element: exact in bf16. Pins the swizzled
    LDS staging of A and its fragment reads next to the B maps."""
    m, n, nblk = 192, 256, k // 32
    col = (7 * torch.arange(m)) % k
    a8 = torch.zeros(m, k, dtype=torch.uint8)
    a8[torch.arange(m), col] = 0x38  # e4m3 1.0
    nn_, kk = torch.meshgrid(torch.arange(n), torch.arange(k), indexing="ij")
    nb, bb = torch.meshgrid(torch.arange(n), torch.arange(nblk), indexing="ij")
    e8 = torch.full((n, nblk), 127, dtype=torch.uint8)
    if pattern == "values":  # a different element at every neighbour
        code, e8 = (3 * nn_ + 5 * kk) % 16, (125 + (nb + bb) % 5).byte()
    elif pattern == "scales":  # all 1.0, one scale per (n, block)
        code = torch.full((n, k), 2)
        e8 = ((nb * nblk + bb) % 131 + 60).byte()
    else:  # 1.0 at even (odd) k only: nibble order
        code = 2 * (kk % 2 == (pattern == "odd"))
    code = code.to(torch.uint8)
    w4 = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    got, ref, _ = _gemm_and_ref(a8, torch.ones(m), w4, e8, torch.ones(n),
                                tile=tile)
    assert torch.equal(got, ref)


def test_rows_do_not_depend_on_the_batch():
    """No split-K, one accumulation order: the first 65 rows of an M = 300
    call equal an M = 65 call bit for bit, whichever tile either takes."""
    a8, xs, w4, e8, rs = _operands(300, 640, 128)
    w4t, e8t = (t.to(DEV) for t in ops.tile_mxfp4_weight(w4, e8))
    a8, xs, rs = a8.to(DEV), xs.to(DEV), rs.to(DEV)
    small = ops.gemm_mxfp4(a8[:65].contiguous(), xs[:65].contiguous(), w4t,
                           e8t, rs)
    for tile in (0, 64, 128):
        big = ops.gemm_mxfp4(a8, xs, w4t, e8t, rs, tile=tile)
        assert torch.equal(big[:65], small)


def test_mxfp4_linear_takes_the_tiled_route(monkeypatch):
    """The CPU side is gemm_mxfp4's CPU path (an fp32 product), which
    forward_q gives a CPU tensor on the "tiled" route."""
    from clearml_serving_amd.models.quant import Mxfp4Linear

    torch.manual_seed(200)
    m, n, k = 200, 1024, 1024
    lin = torch.nn.Linear(k, n, bias=True).to(torch.bfloat16)
    q = Mxfp4Linear(lin)
    assert q._route(m) == "tiled"
    x8, xs = ops._quant_fp8_ref(torch.randn(m, k))
    cpu = q.forward_q(x8, xs).double()
    q, x8d, xsd = q.to(DEV), x8.to(DEV), xs.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = q.forward_q(x8d, xsd)
    torch.cuda.synchronize()
    # the transient bf16 weight of the dequant route alone is 2 * N * K
    assert torch.cuda.max_memory_allocated() - before < n * k
    a = (x8.view(torch.float8_e4m3fn).float() * xs[:, None]).double()
    w = ops.dequant_mxfp4(*ops.untile_mxfp4_weight(
        q.weight_mx.cpu(), q.scale_mx.cpu(), n, k),
        q.weight_scale.cpu()).double()
    # the bound of test_mxfp4_linear_gpu_matches_cpu_path: either side rounds
    # to bf16 at most three times and accumulates in fp32
    bound = (6 * 2.0 ** -9 * ((a @ w.T).abs() + lin.bias.double().abs())
             + 2 * k * 2.0 ** -23 * (a.abs() @ w.abs().T))
    ratio = (got.double().cpu() - cpu).abs() / bound
    print("max |gpu - cpu| / bound: {:.4f}".format(ratio.max().item()))
    assert (ratio <= 1).all()
    monkeypatch.setenv("CMLS_MXFP4_TILED", "0")
    assert q._route(m) == "dequant"


def test_mxfp4_engine_prefill_on_the_tiled_route():
    """A 204-token prompt: every projection of llama-tiny (N and K multiples
    of 128) prefills through gemm_mxfp4. The first greedy token equals the
    argmax of the same quantised model's prefill on the CPU (the engine does
    not start an mxfp4 model there, so its model is copied over), whose top-1
    logit leads the runner-up by 0.1445 at |logit| ~ 1: 18 bf16 ulps,
    measured on the CPU over 40 candidate prompts; decode then runs through
    the graphs."""
    from clearml_serving_amd.engines.llm.engine import (
        LlmEngine, LlmEngineConfig, SamplingParams)

    prompt = "mxfp4 prefill 35 " * 12
    eng = LlmEngine(LlmEngineConfig(
        preset="llama-tiny", num_kv_blocks=64, block_size=16,
        max_model_len=256, device=DEV, quantization="mxfp4",
        decode_graphs=True))
    eng.start()
    ids = eng.tokenizer.encode(prompt)
    t = len(ids)
    assert t > 128
    assert all(getattr(layer, name)._route(t) == "tiled"
               for layer in eng.model.layers
               for name in ("qkv", "o_proj", "gate_up", "down"))

    async def go():
        toks = []
        async for item in eng.generate(prompt, SamplingParams(
                temperature=0.0, max_tokens=8, ignore_eos=True)):
            toks.extend(item["token_ids"])
        return toks

    toks = asyncio.new_event_loop().run_until_complete(go())
    cpu_model = copy.deepcopy(eng.model).to("cpu")
    eng.stop()
    assert len(toks) == 8
    ctx = {"mode": "prefill", "batch": 1, "seq": t,
           "seq_lens": torch.tensor([t], dtype=torch.int32),
           "slot_mapping": torch.full((t,), -1, dtype=torch.int32)}
    with torch.inference_mode():
        logits = cpu_model(torch.tensor(ids), torch.arange(
            t, dtype=torch.int32), kv_caches=None, attn_ctx=ctx,
            last_token_idx=torch.tensor([t - 1]))[0].float()
    top = logits.topk(2)
    print("cpu top-1 over top-2 margin: {:.4f}".format(
        float(top.values[0] - top.values[1])))
    assert toks[0] == int(top.indices[0])
