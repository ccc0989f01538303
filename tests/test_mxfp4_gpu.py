"""MXFP4 decode path on the GPU (csrc/mxfp4_path.hip): the scaled-MFMA
skinny GEMM against a float64 product of the same quantised operands, the
operand-map pins, Mxfp4Linear's two routes and the engine."""

import asyncio

import pytest
import torch

import clearml_serving_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _pack(code):  # e2m1 codes [N, K] -> bytes, even k in the low nibble
    code = code.to(torch.uint8)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()


def _gemm_and_ref(a8, xs, w4, e8, rs, waves=0):
    w4t, e8t = ops.tile_mxfp4_weight(w4, e8)
    got = ops.skinny_gemm_mxfp4(a8.to(DEV), xs.to(DEV), w4t.to(DEV),
                                e8t.to(DEV), rs.to(DEV), waves=waves)
    a = (a8.view(torch.float8_e4m3fn).float() * xs[:, None]).double()
    w = ops.dequant_mxfp4(w4, e8, rs).double()
    return got.double().cpu(), a @ w.T, a.abs() @ w.abs().T


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("k,n", [(128, 16), (512, 48), (640, 32)])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 64])
def test_skinny_gemm_mxfp4_matches_float64(m, k, n, waves):
    g = torch.Generator().manual_seed(m * 1000 + k + n)
    a8, xs = ops._quant_fp8_ref(torch.randn(m, k, generator=g))
    blocks = torch.randn(n, k // 32, 32, generator=g) * torch.exp2(
        torch.randint(-6, 6, (n, k // 32, 1), generator=g).float())
    w4, e8, _ = ops.quantize_mxfp4(blocks.reshape(n, k))
    rs = torch.rand(n, generator=g) + 0.5  # the kernel's per-column input
    got, ref, mag = _gemm_and_ref(a8, xs, w4, e8, rs, waves)
    # products are exact in fp32: only fp32 accumulation + the bf16 store
    bound = 2.0 ** -8 * ref.abs() + k * 2.0 ** -23 * mag
    excess = ((got - ref).abs() - bound).max().item()
    print("max excess over bound: {:.3e}".format(excess))
    assert excess <= 0


@pytest.mark.parametrize("k", [128, 256])
@pytest.mark.parametrize("pattern", ["values", "scales", "even", "odd"])
def test_operand_maps_exact(pattern, k):
    """One e4m3 1.0 per A row at column 7m % K picks single weights out, so
    every output is one dequantised element: exact in bf16."""
    m, n, nblk = 64, 32, k // 32
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
    got, ref, _ = _gemm_and_ref(a8, torch.ones(m), _pack(code), e8,
                                torch.ones(n))
    assert torch.equal(got, ref)


@pytest.mark.parametrize("m", [3, 80])  # kernel route, dequant route
def test_mxfp4_linear_gpu_matches_cpu_path(m):
    from clearml_serving_amd.models.quant import Mxfp4Linear

    torch.manual_seed(m)
    lin = torch.nn.Linear(256, 48, bias=True).to(torch.bfloat16)
    q = Mxfp4Linear(lin)
    assert q._route(m) == ("skinny" if m <= q.SKINNY_MAX_M else "dequant")
    x8, xs = ops._quant_fp8_ref(torch.randn(m, 256))
    cpu = q.forward_q(x8, xs).double()
    got = q.to(DEV).forward_q(x8.to(DEV), xs.to(DEV)).double().cpu()
    a = (x8.view(torch.float8_e4m3fn).float() * xs[:, None]).double()
    w = ops.dequant_mxfp4(*ops.untile_mxfp4_weight(
        q.weight_mx.cpu(), q.scale_mx.cpu(), 48, 256),
        q.weight_scale.cpu()).double()
    # either side rounds to bf16 at most three times (GEMM store, row scale,
    # bias add), each within 2^-9 of |gemm| + |bias|, and accumulates in fp32
    bound = (6 * 2.0 ** -9 * ((a @ w.T).abs() + lin.bias.double().abs())
             + 2 * 256 * 2.0 ** -23 * (a.abs() @ w.abs().T))
    assert ((got - cpu).abs() <= bound).all()


def test_mxfp4_engine_graphs_and_dequantised_bf16():
    from clearml_serving_amd.engines.llm.engine import (
        LlmEngine, LlmEngineConfig, SamplingParams)

    def gen(quant, graphs):
        eng = LlmEngine(LlmEngineConfig(
            preset="llama-tiny", num_kv_blocks=64, block_size=16,
            max_model_len=128, device=DEV, quantization=quant,
            decode_graphs=graphs))
        eng.start()
        if quant is None:  # bf16 model holding the dequantised mxfp4 weights
            for layer in eng.model.layers:
                for name in ("qkv", "o_proj", "gate_up", "down"):
                    w = getattr(layer, name).weight.data
                    w.copy_(ops.dequant_mxfp4(*ops.quantize_mxfp4(w)))

        async def go():
            toks = []
            async for item in eng.generate(
                    "mxfp4 smoke", SamplingParams(
                        temperature=0.0, max_tokens=8, ignore_eos=True)):
                toks.extend(item["token_ids"])
            return toks

        out = asyncio.new_event_loop().run_until_complete(go())
        eng.stop()
        return out

    eager = gen("mxfp4", False)
    assert len(eager) == 8
    assert gen("mxfp4", True) == eager  # capture-safe and deterministic
    # what is left against bf16 is the activations' fp8 rounding: the same
    # first-greedy-token agreement test_fp8_llama_gpu_generation asks of fp8
    assert gen(None, False)[0] == eager[0]
