"""GPU tests: ops.moe_experts_fp8 (ops/csrc/moe_fp8.hip) against its CPU path
on the same quantised operands, and an fp8 MoE model through the engine."""

import asyncio
import functools

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine, LlmEngineConfig, SamplingParams)
from clearml_serving_amd.models.quant import quantize_experts_fp8
from tests.test_moe_cpu import run
from tests.test_moe_gpu import DEV, bits, expert_weights, routing

pytestmark = pytest.mark.gpu

TOL = dict(atol=5e-2, rtol=5e-2)  # test_skinny_gemm_fp8_matches_dequant_matmul


@functools.lru_cache(maxsize=None)
def operands(t, h, inter, e, seed):
    """(cpu tuple, gpu tuple) of one case; built once, never modified."""
    w13, w2, _, _ = expert_weights(h, inter, e)
    x, ids, w = routing(t, e, h, seed=seed)
    cpu = (*ops.quant_fp8(x), *quantize_experts_fp8(w13),
           *quantize_experts_fp8(w2), ids, w)
    return cpu, tuple(v.to(DEV) for v in cpu)


@pytest.mark.parametrize("block_m", [None, 16, 64])
@pytest.mark.parametrize("e", [4, 8])
@pytest.mark.parametrize("h,inter", [(256, 512), (1536, 1408)])
@pytest.mark.parametrize("t", [1, 5, 67])
def test_fused_fp8_matches_cpu_reference(t, h, inter, e, block_m):
    cpu, gpu = operands(t, h, inter, e, t + h + e)
    ref = ops.moe_experts_fp8(*cpu).float()
    got = ops.moe_experts_fp8(*gpu, block_m=block_m)
    assert got.dtype == torch.bfloat16 and got.shape == (t, h)
    got = got.float().cpu()
    print("T={} H={} I={} E={} block_m={}: |ref|max {:.3f}  max diff {:.2e}"
          .format(t, h, inter, e, block_m, float(ref.abs().max()),
                  float((got - ref).abs().max())))
    torch.testing.assert_close(got, ref, **TOL)


@pytest.mark.parametrize("h,inter,e", [(256, 512, 4), (1536, 1408, 8)])
def test_fused_fp8_bitwise_properties(h, inter, e):
    _, gpu = operands(67, h, inter, e, 23)
    x8, xs, *wts, ids, w = gpu
    full = ops.moe_experts_fp8(*gpu)
    assert torch.equal(bits(full), bits(ops.moe_experts_fp8(*gpu))), "rerun"
    assert torch.equal(bits(ops.moe_experts_fp8(*gpu, block_m=16)),
                       bits(ops.moe_experts_fp8(*gpu, block_m=64)))
    for r in (0, 13, 66):
        alone = ops.moe_experts_fp8(
            x8[r:r + 1].clone(), xs[r:r + 1].clone(), *wts,
            ids[r:r + 1].clone(), w[r:r + 1].clone())
        assert torch.equal(bits(alone), bits(full[r:r + 1])), "row %d" % r


def test_loop_path_matches_cpu_reference(monkeypatch):
    """T=200 with the path threshold at the value the fp8 path started from
    (the bf16 MOE_FUSED_MAX, 128): the measured fp8 default, 256, would keep
    an eager T=200 call on the fused path."""
    monkeypatch.setattr(ops, "MOE_FP8_FUSED_MAX", 128)
    cpu, gpu = operands(200, 1536, 1408, 8, 200)
    ref = ops.moe_experts_fp8(*cpu).float()
    calls = []
    real_loop = ops._moe_experts_fp8_loop
    monkeypatch.setattr(ops, "_moe_experts_fp8_loop",
                        lambda *a: calls.append(1) or real_loop(*a))
    loop = ops.moe_experts_fp8(*gpu)
    assert calls == [1], "an eager T=200 call takes the loop path"
    assert loop.dtype == torch.bfloat16 and loop.shape == (200, 1536)
    for name, got in [("loop", loop)] + [
            (bm, ops.moe_experts_fp8(*gpu, block_m=bm)) for bm in (16, 64)]:
        got = got.float().cpu()
        print("T=200 {}: max diff {:.2e}".format(
            name, float((got - ref).abs().max())))
        torch.testing.assert_close(got, ref, **TOL)
    assert calls == [1]


@pytest.mark.parametrize("h,inter,e,k,off", [
    (224, 512, 4, 2, 0),    # H % 64
    (256, 480, 4, 2, 0),    # I % 64
    (256, 64, 65, 2, 0),    # E > 64
    (256, 64, 2, 3, 0),     # k > E
    (256, 64, 4, 2, 8),     # x8 off the 16-byte grid
])
def test_fused_fp8_refusals(h, inter, e, k, off):
    def u8(*shape):
        return torch.zeros(*shape, device=DEV, dtype=torch.uint8)

    x8 = u8(3 * h + off)[off:].view(3, h)
    args = (x8, torch.ones(3, device=DEV), u8(e, 2 * inter, h),
            torch.ones(e, 2 * inter, device=DEV), u8(e, h, inter),
            torch.ones(e, h, device=DEV),
            torch.zeros(3, k, device=DEV, dtype=torch.int32),
            torch.full((3, k), 1.0 / k, device=DEV))
    with pytest.raises(RuntimeError):
        ops.moe_experts_fp8(*args)


def test_fp8_moe_engine_graphs_match_eager():
    """test_moe_decode_graphs_match_eager with quantization="fp8": the engine
    starts, every layer's expert stacks are e4m3 byte buffers, and greedy
    decode is token-identical with decode graphs on and off."""
    def gen(graphs):
        torch.manual_seed(5)
        eng = LlmEngine(LlmEngineConfig(
            preset="mixtral-tiny", num_kv_blocks=128, block_size=16,
            max_model_len=256, device=DEV, max_num_seqs=8,
            decode_graphs=graphs, quantization="fp8"))
        eng.start()
        for layer in eng.model.layers:
            bufs = dict(layer.named_buffers(recurse=False))
            assert bufs["w13"].dtype == bufs["w2"].dtype == torch.uint8
            assert bufs["w13"].shape == (4, 1024, 256)
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
