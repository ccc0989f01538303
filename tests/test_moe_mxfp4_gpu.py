"""GPU tests: ops.moe_experts_mxfp4 (ops/csrc/moe_mxfp4.hip) against its CPU
path on the same quantised operands, and an MXFP4 MoE model through the
engine."""

import asyncio
import functools

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine, LlmEngineConfig, SamplingParams)
from clearml_serving_amd.models.quant import quantize_experts_mxfp4
from tests.test_moe_cpu import run
from tests.test_moe_fp8_gpu import TOL
from tests.test_moe_gpu import DEV, bits, expert_weights, routing

pytestmark = pytest.mark.gpu


def block_scaled(w, seed):
    """Every 32-block of K times 2^randint(-3, 3): neighbouring MX blocks get
    different exponents, so a kernel reading the wrong block's scale fails."""
    g = torch.Generator().manual_seed(seed)
    e, n, k = w.shape
    exp = torch.randint(-3, 4, (e, n, k // 32, 1), generator=g)
    return torch.ldexp(w.float().reshape(e, n, k // 32, 32), exp).reshape(
        e, n, k)


def quantized(w, seed):
    """quantize_experts_mxfp4 of the block-scaled stack, with fp32 row scales
    of 2^-2 or 2^-3 per (expert, row) in place of the all-ones it returns.
    The block factors have an rms of 3.5 per GEMM, which would put the
    outputs near 100 where TOL (set for the O(1) outputs of expert_weights)
    is an absolute bound; these row scales bring the gain back to 0.7, and
    being unequal they show a kernel that indexes w_scale wrongly."""
    w4t, e8t, scale = quantize_experts_mxfp4(block_scaled(w, seed))
    g = torch.Generator().manual_seed(seed + 10)
    exp = torch.randint(-3, -1, scale.shape, generator=g)
    return w4t, e8t, torch.ldexp(scale, exp)


@functools.lru_cache(maxsize=None)
def operands(t, h, inter, e, seed):
    """(gpu operands, the CPU path's fp32 result on the same operands) of one
    case; built once, never modified."""
    w13, w2, _, _ = expert_weights(h, inter, e)
    x, ids, w = routing(t, e, h, seed=seed)
    cpu = (*ops.quant_fp8(x), *quantized(w13, 1), *quantized(w2, 2), ids, w)
    return (tuple(v.to(DEV) for v in cpu),
            ops.moe_experts_mxfp4(*cpu).float())


# gate/up K = H, down K = I; the 8 waves take 512-wide scale quads round-robin
@pytest.mark.parametrize("block_m", [None, 16, 64])
@pytest.mark.parametrize("e", [4, 8])
@pytest.mark.parametrize("h,inter", [
    (256, 512),    # a 2-step ragged quad with seven idle waves; one full quad
    (1536, 1408),  # three full quads; two full + a 3-step ragged quad
    (4608, 128),   # nine full quads: wave 0 owns quads 0 and 8, so its
                   # prefetch loop iterates; a 1-step ragged quad
])
@pytest.mark.parametrize("t", [1, 5, 67])
def test_fused_mxfp4_matches_cpu_reference(t, h, inter, e, block_m):
    gpu, ref = operands(t, h, inter, e, t + h + e)
    got = ops.moe_experts_mxfp4(*gpu, block_m=block_m)
    assert got.dtype == torch.bfloat16 and got.shape == (t, h)
    got = got.float().cpu()
    print("T={} H={} I={} E={} block_m={}: |ref|max {:.3f}  max diff {:.2e}"
          .format(t, h, inter, e, block_m, float(ref.abs().max()),
                  float((got - ref).abs().max())))
    torch.testing.assert_close(got, ref, **TOL)


@pytest.mark.parametrize("h,inter,e", [(256, 512, 4), (1536, 1408, 8)])
def test_fused_mxfp4_bitwise_properties(h, inter, e):
    gpu, _ = operands(67, h, inter, e, 23)
    x8, xs, *wts, ids, w = gpu
    full = ops.moe_experts_mxfp4(*gpu)
    assert torch.equal(bits(full), bits(ops.moe_experts_mxfp4(*gpu))), "rerun"
    assert torch.equal(bits(ops.moe_experts_mxfp4(*gpu, block_m=16)),
                       bits(ops.moe_experts_mxfp4(*gpu, block_m=64)))
    for r in (0, 13, 66):
        alone = ops.moe_experts_mxfp4(
            x8[r:r + 1].clone(), xs[r:r + 1].clone(), *wts,
            ids[r:r + 1].clone(), w[r:r + 1].clone())
        assert torch.equal(bits(alone), bits(full[r:r + 1])), "row %d" % r


def test_loop_path_matches_cpu_reference(monkeypatch):
    """T=200 with the path threshold lowered to 128: the measured default
    keeps every eager call up to T=2048 on the fused path."""
    monkeypatch.setattr(ops, "MOE_MXFP4_FUSED_MAX", 128)
    gpu, ref = operands(200, 1536, 1408, 8, 200)
    calls = []
    real_loop = ops._moe_experts_mxfp4_loop
    monkeypatch.setattr(ops, "_moe_experts_mxfp4_loop",
                        lambda *a: calls.append(1) or real_loop(*a))
    loop = ops.moe_experts_mxfp4(*gpu)
    assert calls == [1], "an eager T=200 call takes the loop path"
    assert loop.dtype == torch.bfloat16 and loop.shape == (200, 1536)
    for name, got in [("loop", loop)] + [
            (bm, ops.moe_experts_mxfp4(*gpu, block_m=bm)) for bm in (16, 64)]:
        got = got.float().cpu()
        print("T=200 {}: max diff {:.2e}".format(
            name, float((got - ref).abs().max())))
        torch.testing.assert_close(got, ref, **TOL)
    assert calls == [1]


@pytest.mark.parametrize("h,inter,e,k,off,cut", [
    (192, 512, 4, 2, 0, 0),    # H % 128
    (256, 448, 4, 2, 0, 0),    # I % 128
    (256, 128, 65, 2, 0, 0),   # E > 64
    (256, 128, 2, 3, 0, 0),    # k > E
    (256, 128, 4, 2, 8, 0),    # x8 off the 16-byte grid
    (256, 128, 4, 2, 0, 1),    # w2 tiles one expert short
])
def test_fused_mxfp4_refusals(h, inter, e, k, off, cut):
    def u8(*shape):
        return torch.zeros(*shape, device=DEV, dtype=torch.uint8)

    def tiles(ne, n, kk):
        steps = -(-kk // 128)
        return (u8(ne, n // 16, steps, 64, 16),
                u8(ne, n // 16, -(-steps // 4), 64, 4))

    x8 = u8(3 * h + off)[off:].view(3, h)
    args = (x8, torch.ones(3, device=DEV), *tiles(e, 2 * inter, h),
            torch.ones(e, 2 * inter, device=DEV), *tiles(e - cut, h, inter),
            torch.ones(e, h, device=DEV),
            torch.zeros(3, k, device=DEV, dtype=torch.int32),
            torch.full((3, k), 1.0 / k, device=DEV))
    with pytest.raises(RuntimeError):
        ops.moe_experts_mxfp4(*args)


def test_mxfp4_moe_engine_graphs_match_eager():
    """The engine starts, the expert stacks are tiled byte buffers, and
    greedy decode is token-identical with decode graphs on and off."""
    def gen(graphs):
        torch.manual_seed(5)
        eng = LlmEngine(LlmEngineConfig(
            preset="mixtral-tiny", num_kv_blocks=128, block_size=16,
            max_model_len=256, device=DEV, max_num_seqs=8,
            decode_graphs=graphs, quantization="mxfp4"))
        eng.start()
        for layer in eng.model.layers:
            bufs = dict(layer.named_buffers(recurse=False))
            assert bufs["w13"].dtype == bufs["w2"].dtype == torch.uint8
            assert bufs["w13"].shape == (4, 64, 2, 64, 16)  # [4, 1024, 256]
            assert bufs["w13_e8"].shape == (4, 64, 1, 64, 4)
            assert bufs["w2"].shape == (4, 16, 4, 64, 16)   # [4, 256, 512]
            assert bufs["w2_e8"].shape == (4, 16, 1, 64, 4)
            assert layer.router.weight.dtype == torch.bfloat16

        async def one(prompt):
            seq = await eng.add_request(prompt, SamplingParams(
                temperature=0.0, max_tokens=24, ignore_eos=True))
            toks = []
            while True:
                item = await seq.stream.get()
                toks.extend(item["token_ids"])
                if item["finished"]:
                    return toks

        async def go():
            return await asyncio.gather(*[
                one([(i * 7 + j) % 500 for j in range(9 + i)])
                for i in range(5)])

        return run(go())

    eager = gen(False)
    graphed = gen(True)
    assert all(len(o) == 24 for o in eager)
    assert eager == graphed
