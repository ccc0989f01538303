"""MXFP4 MoE on the CPU: quantize_experts_mxfp4, the reference path of
ops.moe_experts_mxfp4, and the engine's shape refusal."""

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import LlmEngine, LlmEngineConfig
from clearml_serving_amd.models.quant import quantize_experts_mxfp4


def dequant_experts(w4t, e8t, scale, n, k):
    return torch.stack([
        ops.dequant_mxfp4(*ops.untile_mxfp4_weight(w4t[i], e8t[i], n, k),
                          scale[i]) for i in range(w4t.shape[0])])


@pytest.mark.parametrize("e,n,k", [(3, 32, 128), (2, 48, 640)])
def test_quantize_experts_mxfp4_round_trips_mx_exact_weights(e, n, k):
    """e2m1 grid values times one power of two per 32-block; element 0 of a
    block is 4 or 6, so the quantiser picks that block's exponent again."""
    g = torch.Generator().manual_seed(n + k)
    grid = torch.tensor(ops.E2M1_GRID)
    v = grid[torch.randint(0, 8, (e, n, k // 32, 32), generator=g)]
    v[..., 0] = grid[torch.randint(6, 8, (e, n, k // 32), generator=g)]
    v = v * (torch.randint(0, 2, v.shape, generator=g) * 2 - 1)
    exp = torch.randint(-6, 4, (e, n, k // 32, 1), generator=g)
    w = torch.ldexp(v, exp).reshape(e, n, k)
    w4t, e8t, scale = quantize_experts_mxfp4(w)
    steps = k // 128
    assert w4t.dtype == e8t.dtype == torch.uint8
    assert w4t.shape == (e, n // 16, steps, 64, 16)
    assert e8t.shape == (e, n // 16, (steps + 3) // 4, 64, 4)
    assert torch.equal(scale, torch.ones(e, n))
    assert torch.equal(dequant_experts(w4t, e8t, scale, n, k), w)


def test_cpu_path_is_the_fp8_reference_maths_on_dequantised_weights():
    t, h, inter, e, k = 7, 256, 128, 4, 2
    g = torch.Generator().manual_seed(3)
    q13 = quantize_experts_mxfp4(
        torch.randn(e, 2 * inter, h, generator=g) * h ** -0.5)
    q2 = quantize_experts_mxfp4(
        torch.randn(e, h, inter, generator=g) * inter ** -0.5)
    x8, xs = ops.quant_fp8(torch.randn(t, h, generator=g))
    ids, wts = ops.moe_route(torch.randn(t, e, generator=g), k)
    got = ops.moe_experts_mxfp4(x8, xs, *q13, *q2, ids, wts)
    assert got.dtype == torch.bfloat16 and got.shape == (t, h)

    d13, d2 = dequant_experts(*q13, 2 * inter, h), dequant_experts(*q2, h, inter)
    xf = x8.view(torch.float8_e4m3fn).float() * xs[:, None]
    out = torch.zeros(t, h)
    for j in range(k):  # ascending j, as the op sums
        gu = torch.einsum("th,tnh->tn", xf, d13[ids[:, j].long()])
        act = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
        a8, a_s = ops._quant_fp8_ref(act.to(torch.bfloat16))
        a = a8.view(torch.float8_e4m3fn).float() * a_s[:, None]
        out += wts[:, j, None] * torch.einsum("ti,thi->th", a,
                                              d2[ids[:, j].long()])
    # same maths, other fp32 summation order: one bf16 ulp of the result
    torch.testing.assert_close(got.float(), out.to(torch.bfloat16).float(),
                               atol=2 ** -7, rtol=2 ** -7)


def test_engine_refuses_mxfp4_moe_with_hidden_off_the_128_grid():
    eng = LlmEngine(LlmEngineConfig(
        preset="mixtral-tiny", device="cpu", quantization="mxfp4",
        overrides={"hidden": 192}))
    with pytest.raises(ValueError, match="multiples of 128"):
        eng._check_moe_options()
    assert getattr(eng, "model", None) is None
