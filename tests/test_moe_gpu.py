"""GPU tests: the fused MoE kernels (ops/csrc/moe.hip) against the CPU
references in ops, their bitwise reproducibility and batch invariance, graph
capture, and an MoE model through the engine."""

import asyncio
import functools

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine,
    LlmEngineConfig,
    SamplingParams,
)
from clearml_serving_amd.models.llama import PRESETS, LlamaForCausalLM
from tests.test_moe_cpu import check_align, run, tie_free_logits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


# --------------------------------------------------------------------- #
# route
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("e,k", [(4, 2), (8, 2), (60, 4), (64, 8)])
@pytest.mark.parametrize("t", [1, 5, 67])
@pytest.mark.parametrize("renorm", [True, False])
def test_route_matches_reference(t, e, k, renorm):
    logits = tie_free_logits(t, e, seed=1000 * t + e)
    ids, w = ops.moe_route(logits.to(DEV), k, renorm)
    ref_ids, ref_w = ops.moe_route(logits, k, renorm)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32
    assert torch.equal(ids.cpu(), ref_ids)
    torch.testing.assert_close(w.cpu(), ref_w, atol=1e-6, rtol=1e-5)
    if renorm:
        torch.testing.assert_close(w.sum(-1).cpu(), torch.ones(t),
                                   atol=1e-6, rtol=1e-5)


def test_route_ties_take_lowest_index():
    logits = torch.tensor([[1.0, 2.0, 2.0, 0.5, 2.0, -1.0],
                           [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    ids, w = ops.moe_route(logits.to(DEV), 3, True)
    assert ids.cpu().tolist() == [[1, 2, 4], [0, 1, 2]]
    torch.testing.assert_close(w.cpu(), torch.full((2, 3), 1.0 / 3),
                               atol=1e-6, rtol=1e-5)


def test_route_bf16_logits():
    logits = tie_free_logits(5, 8, seed=9).to(torch.bfloat16)
    # bf16 keeps arange(8) * 0.37 distinct, so ids are still decided exactly
    assert all(len(set(r)) == 8 for r in logits.float().tolist())
    ids, w = ops.moe_route(logits.to(DEV), 2, True)
    ref_ids, ref_w = ops.moe_route(logits, 2, True)
    assert torch.equal(ids.cpu(), ref_ids)
    torch.testing.assert_close(w.cpu(), ref_w, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("e,k", [(4, 0), (4, 5), (65, 2), (64, 9)])
def test_route_refuses_unsupported(e, k):
    with pytest.raises(RuntimeError):
        ops.moe_route(torch.zeros(3, e, device=DEV), k)
    ext = ops.extension_or_none()
    with pytest.raises(RuntimeError):  # the binding itself checks too
        ext.moe_route(torch.zeros(3, e, device=DEV), k, True)


# --------------------------------------------------------------------- #
# align
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("block_m", [16, 64])
@pytest.mark.parametrize("e,k", [(4, 2), (8, 2), (60, 4)])
@pytest.mark.parametrize("t", [1, 5, 67])
def test_align_invariants(t, e, k, block_m):
    ids, _ = ops.moe_route(tie_free_logits(t, e, seed=7 * t + e), k)
    sorted_slots, block_expert = ops.moe_align(ids.to(DEV), e, block_m)
    check_align(ids, e, block_m, sorted_slots.cpu(), block_expert.cpu())
    ref_slots, ref_blocks = ops.moe_align(ids, e, block_m)
    assert torch.equal(sorted_slots.cpu(), ref_slots)
    assert torch.equal(block_expert.cpu(), ref_blocks)


@pytest.mark.parametrize("block_m", [16, 64])
def test_align_all_rows_on_two_experts(block_m):
    ids = torch.tensor([[5, 2]] * 67, dtype=torch.int32)
    sorted_slots, block_expert = ops.moe_align(ids.to(DEV), 8, block_m)
    check_align(ids, 8, block_m, sorted_slots.cpu(), block_expert.cpu())
    nb = (67 + block_m - 1) // block_m
    assert block_expert.cpu().tolist()[:2 * nb] == [2] * nb + [5] * nb


# --------------------------------------------------------------------- #
# experts
# --------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def expert_weights(h, inter, e):
    """bf16 expert stacks scaled by K**-0.5 (outputs O(1)), built once per
    shape and shared (never modified) by the tests below."""
    g = torch.Generator().manual_seed(h + inter + e)
    w13 = (torch.randn(e, 2 * inter, h, generator=g) * h ** -0.5
           ).to(torch.bfloat16)
    w2 = (torch.randn(e, h, inter, generator=g) * inter ** -0.5
          ).to(torch.bfloat16)
    return w13, w2, w13.to(DEV), w2.to(DEV)


def routing(t, e, h, seed):
    """x bf16 [T, H], ids, weights. T=67 gets a skewed router: every token's
    first choice is expert 0 (67 rows = 4 full 16-row blocks + a ragged
    3-row tail, 5 blocks) and the last expert receives nothing."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(t, h, generator=g).to(torch.bfloat16)
    if t == 67:
        second = 1 + torch.arange(t) % (e - 2)
        ids = torch.stack([torch.zeros(t, dtype=torch.long), second],
                          dim=1).to(torch.int32)
        assert not (ids == e - 1).any()
        w = torch.rand(t, 2, generator=g) + 0.1
        w = w / w.sum(-1, keepdim=True)
    else:
        ids, w = ops.moe_route(torch.randn(t, e, generator=g), 2)
    return x, ids, w


@pytest.mark.parametrize("e", [4, 8])
@pytest.mark.parametrize("h,inter", [(256, 512), (1536, 1408)])
@pytest.mark.parametrize("t", [1, 5, 67])
def test_experts_match_fp32_reference(t, h, inter, e):
    """Against the plain fp32 reference, which does NOT round silu(g)*u to
    bf16 the way the kernel's [S, I] buffer does: the tolerance holds without
    that allowance at these shapes. The reference with the rounding emulated
    is computed too and its distance from the plain one printed, to show how
    much of the budget that rounding takes."""
    w13, w2, w13_d, w2_d = expert_weights(h, inter, e)
    x, ids, w = routing(t, e, h, seed=t + h + e)
    ref = ops.moe_experts(x, w13, w2, ids, w).float()
    ref_rounded = ops._moe_experts_ref(x, w13, w2, ids, w,
                                       act_dtype=torch.bfloat16).float()
    got = ops.moe_experts(x.to(DEV), w13_d, w2_d, ids.to(DEV), w.to(DEV))
    assert got.dtype == torch.bfloat16 and got.shape == (t, h)
    got = got.float().cpu()
    print("T={} H={} I={} E={}: |ref|max {:.3f}  act-rounding effect {:.2e}  "
          "gpu-vs-fp32 {:.2e}  gpu-vs-rounded {:.2e}".format(
              t, h, inter, e, float(ref.abs().max()),
              float((ref_rounded - ref).abs().max()),
              float((got - ref).abs().max()),
              float((got - ref_rounded).abs().max())))
    torch.testing.assert_close(got, ref, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("block_m", [16, 64])
def test_experts_row_blocks_agree_bitwise(block_m):
    """Both row-block sizes of the fused path compute every output element
    with the same k split, so they agree bit for bit."""
    w13, w2, w13_d, w2_d = expert_weights(256, 512, 4)
    x, ids, w = routing(67, 4, 256, seed=11)
    auto = ops.moe_experts(x.to(DEV), w13_d, w2_d, ids.to(DEV), w.to(DEV))
    forced = ops.moe_experts(x.to(DEV), w13_d, w2_d, ids.to(DEV), w.to(DEV),
                             block_m=block_m)
    assert torch.equal(bits(auto), bits(forced))


@pytest.mark.parametrize("h,inter,e", [(256, 512, 4), (1536, 1408, 8)])
def test_experts_batch_invariant_bitwise(h, inter, e):
    w13, w2, w13_d, w2_d = expert_weights(h, inter, e)
    x, ids, w = routing(67, e, h, seed=23)
    x, ids, w = x.to(DEV), ids.to(DEV), w.to(DEV)
    full = ops.moe_experts(x, w13_d, w2_d, ids, w)
    again = ops.moe_experts(x, w13_d, w2_d, ids, w)
    assert torch.equal(bits(full), bits(again)), "run-to-run"
    for r in (0, 13, 66):
        alone = ops.moe_experts(x[r:r + 1].clone(), w13_d, w2_d,
                                ids[r:r + 1].clone(), w[r:r + 1].clone())
        assert torch.equal(bits(alone), bits(full[r:r + 1])), "row %d" % r


@pytest.mark.parametrize("h,inter,e,k", [
    (240, 512, 4, 2),    # H % 32
    (256, 496, 4, 2),    # I % 32
    (256, 64, 65, 2),    # E > 64
    (256, 64, 2, 3),     # k > E
])
def test_experts_unsupported_shapes_raise(h, inter, e, k):
    x = torch.zeros(3, h, device=DEV, dtype=torch.bfloat16)
    w13 = torch.zeros(e, 2 * inter, h, device=DEV, dtype=torch.bfloat16)
    w2 = torch.zeros(e, h, inter, device=DEV, dtype=torch.bfloat16)
    ids = torch.zeros(3, k, device=DEV, dtype=torch.int32)
    w = torch.full((3, k), 1.0 / k, device=DEV)
    with pytest.raises(RuntimeError):
        ops.moe_experts(x, w13, w2, ids, w)


def test_experts_misaligned_operand_raises():
    w13, w2, w13_d, w2_d = expert_weights(256, 512, 4)
    x, ids, w = routing(1, 4, 256, seed=2)
    flat = torch.zeros(256 + 1, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.moe_experts(flat[1:].view(1, 256), w13_d, w2_d, ids.to(DEV),
                        w.to(DEV))


# --------------------------------------------------------------------- #
# graph capture
# --------------------------------------------------------------------- #
def test_moe_block_captures_into_a_graph():
    # under inference_mode like the engine's own captures: the default
    # generator's graph-state tensors become inference tensors the first time
    # any test captures that way, and capture_begin updates them in place
    with torch.inference_mode():
        _capture_and_replay()


def _capture_and_replay():
    e, k, h, inter, t = 8, 2, 256, 512, 5
    w13, w2, w13_d, w2_d = expert_weights(h, inter, e)
    g = torch.Generator().manual_seed(41)
    logits = torch.randn(t, e, generator=g).to(DEV)
    x = torch.randn(t, h, generator=g).to(torch.bfloat16).to(DEV)

    def block():
        ids, w = ops.moe_route(logits, k, True)
        slots, blocks = ops.moe_align(ids, e, 16)
        return ops.moe_experts(x, w13_d, w2_d, ids, w), slots, blocks

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        block()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, slots, blocks = block()

    # new contents in the static inputs, then replay
    logits.copy_(torch.randn(t, e, generator=g))
    x.copy_(torch.randn(t, h, generator=g).to(torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    eager_out, eager_slots, eager_blocks = block()
    assert torch.equal(bits(out), bits(eager_out))
    assert torch.equal(slots.cpu(), eager_slots.cpu())
    assert torch.equal(blocks.cpu(), eager_blocks.cpu())


# --------------------------------------------------------------------- #
# engine
# --------------------------------------------------------------------- #
def test_moe_decode_graphs_match_eager():
    """mixtral-tiny: greedy generation with per-bucket decode hipGraphs is
    token-identical to eager decode (GPU tokens are NOT compared with CPU
    tokens: near-tied router logits in a random tiny model make that
    meaningless)."""
    def gen(graphs):
        torch.manual_seed(5)
        cfg = LlmEngineConfig(preset="mixtral-tiny", num_kv_blocks=128,
                              block_size=16, max_model_len=256, device=DEV,
                              max_num_seqs=8, decode_graphs=graphs)
        eng = LlmEngine(cfg)
        eng.start()
        assert eng.model_config.num_experts == 4

        async def go():
            prompts = [[(i * 7 + j) % 500 for j in range(9 + i)]
                       for i in range(5)]
            outs = [[] for _ in prompts]

            async def one(i):
                seq = await eng.add_request(prompts[i], SamplingParams(
                    temperature=0.0, max_tokens=24, ignore_eos=True))
                while True:
                    item = await seq.stream.get()
                    outs[i].extend(item["token_ids"])
                    if item["finished"]:
                        return

            await asyncio.gather(*[one(i) for i in range(len(prompts))])
            return outs

        return run(go())

    eager = gen(False)
    graphed = gen(True)
    assert all(len(o) == 24 for o in eager)
    assert eager == graphed


def test_moe_prefill_logits_match_cpu_reference():
    """Prefill logits of the bf16 GPU model vs the same (bf16-valued)
    weights run in fp32 through the CPU reference ops."""
    torch.manual_seed(5)
    cfg = PRESETS["mixtral-tiny"]
    cpu_model = LlamaForCausalLM(cfg).eval()
    cpu_model.load_state_dict({k: v.to(torch.bfloat16).float()
                               for k, v in cpu_model.state_dict().items()})
    gpu_model = LlamaForCausalLM(cfg).eval()
    gpu_model.load_state_dict(cpu_model.state_dict())
    gpu_model = gpu_model.to(DEV).to(torch.bfloat16)
    tokens = torch.tensor([3, 7, 11, 19, 23, 29, 31, 37, 41, 43, 47, 53])
    t = tokens.shape[0]

    def prefill(model, dev):
        attn_ctx = {"mode": "prefill", "batch": 1, "seq": t,
                    "seq_lens": torch.tensor([t], dtype=torch.int32,
                                             device=dev),
                    "slot_mapping": torch.full((t,), -1, dtype=torch.int32,
                                               device=dev)}
        with torch.inference_mode():
            return model(tokens.to(dev),
                         torch.arange(t, dtype=torch.int32, device=dev),
                         kv_caches=None, attn_ctx=attn_ctx).float().cpu()

    got = prefill(gpu_model, DEV)
    ref = prefill(cpu_model, "cpu")
    print("prefill logits: |ref|max {:.3f}, max diff {:.2e}".format(
        float(ref.abs().max()), float((got - ref).abs().max())))
    torch.testing.assert_close(got, ref, atol=3e-2, rtol=3e-2)


# --------------------------------------------------------------------- #
# prefill-sized calls: the per-expert hipBLASLt loop above MOE_FUSED_MAX
# --------------------------------------------------------------------- #
def test_experts_loop_path_matches_fp32_reference(monkeypatch):
    """T=200 is above the default threshold, so an eager call runs the
    per-expert loop; same tolerance and reference as the fused path, and the
    two paths agree with each other to that tolerance (not bitwise)."""
    assert ops.MOE_FUSED_MAX < 200
    h, inter, e = 1536, 1408, 8
    w13, w2, w13_d, w2_d = expert_weights(h, inter, e)
    g = torch.Generator().manual_seed(200)
    x = torch.randn(200, h, generator=g).to(torch.bfloat16)
    ids, w = ops.moe_route(torch.randn(200, e, generator=g), 2)
    ref = ops.moe_experts(x, w13, w2, ids, w).float()
    args = (x.to(DEV), w13_d, w2_d, ids.to(DEV), w.to(DEV))
    calls = []
    real_loop = ops._moe_experts_loop
    monkeypatch.setattr(ops, "_moe_experts_loop",
                        lambda *a: calls.append(1) or real_loop(*a))
    loop = ops.moe_experts(*args)
    assert calls == [1], "an eager T=200 call takes the loop path"
    assert loop.dtype == torch.bfloat16 and loop.shape == (200, h)
    torch.testing.assert_close(loop.float().cpu(), ref, atol=3e-2, rtol=3e-2)
    for block_m in (16, 64):  # the fused path serves the same T when forced
        fused = ops.moe_experts(*args, block_m=block_m)
        torch.testing.assert_close(fused.float().cpu(), ref,
                                   atol=3e-2, rtol=3e-2)


def test_experts_threshold_selects_the_path(monkeypatch):
    """MOE_FUSED_MAX decides between the two paths for an eager call."""
    h, inter, e = 256, 512, 4
    w13, w2, w13_d, w2_d = expert_weights(h, inter, e)
    x, ids, w = routing(67, e, h, seed=31)
    ref = ops.moe_experts(x, w13, w2, ids, w).float()
    args = (x.to(DEV), w13_d, w2_d, ids.to(DEV), w.to(DEV))
    calls = []
    real_loop = ops._moe_experts_loop
    monkeypatch.setattr(ops, "_moe_experts_loop",
                        lambda *a: calls.append(1) or real_loop(*a))
    fused = ops.moe_experts(*args)
    assert calls == [], "T=67 is below the default threshold"
    monkeypatch.setattr(ops, "MOE_FUSED_MAX", 16)
    looped = ops.moe_experts(*args)
    assert calls == [1]
    for got in (fused, looped):
        torch.testing.assert_close(got.float().cpu(), ref,
                                   atol=3e-2, rtol=3e-2)
    # the shape contract holds on the loop path too
    bad = torch.zeros(67, 240, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.moe_experts(bad, w13_d[:, :, :240].contiguous(),
                        w2_d[:, :240].contiguous(), args[3], args[4])
