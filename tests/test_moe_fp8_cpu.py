"""fp8 MoE on the CPU: K-permutation invariance, quantize_llama_fp8."""

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.models.llama import PRESETS, LlamaForCausalLM
from clearml_serving_amd.models.quant import Fp8Linear, quantize_llama_fp8

F8 = torch.float8_e4m3fn


@pytest.mark.parametrize("rows,n,k", [(1, 16, 64), (5, 48, 192)])
def test_common_k_swizzle_leaves_the_product_unchanged(rows, n, k):
    """swizzle(a) @ swizzle(w)^T == a @ w^T. Products of two e4m3 values and
    their sums over these K are exact in float64, so equality is exact there;
    in fp32 the two differ by summation order only."""
    g = torch.Generator().manual_seed(rows + n + k)
    a = torch.randn(rows, k, generator=g).to(F8)
    w = torch.randn(n, k, generator=g).to(F8)
    a_sw = ops.swizzle_fp8_weight(a).view(F8)
    w_sw = ops.swizzle_fp8_weight(w).view(F8)
    assert not torch.equal(a_sw.view(torch.uint8), a.view(torch.uint8))
    assert torch.equal(a_sw.double() @ w_sw.double().t(),
                       a.double() @ w.double().t())
    torch.testing.assert_close(a_sw.float() @ w_sw.float().t(),
                               a.float() @ w.float().t(),
                               atol=k * 2.0 ** -20, rtol=0)


@pytest.fixture(scope="module")
def quantized_model():
    torch.manual_seed(5)
    model = LlamaForCausalLM(PRESETS["mixtral-tiny"]).to(torch.bfloat16)
    stacks = [(l.w13.data.clone(), l.w2.data.clone()) for l in model.layers]
    return model, stacks, quantize_llama_fp8(model)


def test_quantize_llama_fp8_converts_the_expert_stacks(quantized_model):
    model, stacks, count = quantized_model
    assert count == 2 * (2 + 2)  # per layer: qkv, o_proj, w13, w2
    for layer, (w13, w2) in zip(model.layers, stacks):
        assert isinstance(layer.qkv, Fp8Linear)
        assert type(layer.router) is torch.nn.Linear
        assert [n for n, _ in layer.named_parameters(recurse=False)] == [
            "attn_norm", "mlp_norm"]
        for name, ref in (("w13", w13), ("w2", w2)):
            w8, scale = getattr(layer, name), getattr(layer, name + "_scale")
            assert w8.dtype == torch.uint8 and w8.shape == ref.shape
            torch.testing.assert_close(
                scale, ref.float().abs().amax(dim=2) / 448.0)
            # round-to-nearest e4m3: half a step is 2**-4 relative for normal
            # values, 2**-10 row scales for subnormals (1e-5: fp32 div/mul)
            err = ops._dequant_fp8(w8[1], scale[1], True) - ref[1].float()
            assert bool((err.abs() <= (ref[1].float().abs() * 2.0 ** -4
                                       + scale[1][:, None] * 2.0 ** -10)
                         * (1 + 1e-5)).all())


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_fp8_experts_are_close_to_the_bf16_weight_reference(quantized_model,
                                                            seed):
    """CPU moe_experts_fp8 on the quantised stacks against the fp32
    moe_experts reference on the bf16 stacks and the unquantised x: the
    quantisation error itself. Observed max |diff| over the four seeds and
    both layers: 6.23e-3 (|ref|max 0.060 .. 0.090: the tiny model's expert
    outputs are small); the bound is twice that, 1.25e-2 absolute."""
    model, stacks, _ = quantized_model
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(19, 256, generator=g).to(torch.bfloat16)
    ids, w = ops.moe_route(torch.randn(19, 4, generator=g), 2)
    for layer, (w13, w2) in zip(model.layers, stacks):
        ref = ops.moe_experts(x.float(), w13.float(), w2.float(), ids, w)
        got = ops.moe_experts_fp8(*ops.quant_fp8(x), layer.w13,
                                  layer.w13_scale, layer.w2, layer.w2_scale,
                                  ids, w)
        assert got.dtype == torch.bfloat16 and got.shape == (19, 256)
        diff = float((got.float() - ref).abs().max())
        print("seed {}: |ref|max {:.4f}  max diff {:.3e}".format(
            seed, float(ref.abs().max()), diff))
        assert diff <= 1.25e-2
