"""GPU tests: the 128-row tiled path of ops.moe_experts_mxfp4
(ops/csrc/moe_mxfp4_gemm.hip, block_m=128) against the op's CPU path on the
same quantised operands, its bitwise properties, graph capture and an MXFP4
MoE prefill through the engine."""

import asyncio
import copy

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import (
    LlmEngine, LlmEngineConfig, SamplingParams)
from tests.test_moe_fp8_gpu import TOL
from tests.test_moe_gpu import DEV, bits
from tests.test_moe_mxfp4_gpu import operands

pytestmark = pytest.mark.gpu


# top-2 routing: T=1 is one block of 2 live rows and 126 sentinels; T=300
# gives ~150 slots per expert at E=4 (a full and a partial block, trailing -1
# blocks) and single partial blocks at E=8. Gate/up K = H, down K = I.
@pytest.mark.parametrize("e", [4, 8])
@pytest.mark.parametrize("h,inter", [
    (256, 512),    # a 2-step ragged quad; one full quad
    (1536, 1408),  # three full quads; two quads + a 3-step tail
    (128, 640),    # a single k-step and one column tile; a quad + a 1-step
                   # tail, 10 gated column tiles
])
@pytest.mark.parametrize("t", [1, 67, 300])
def test_tiled_mxfp4_matches_cpu_reference(t, h, inter, e):
    gpu, ref = operands(t, h, inter, e, t + h + e)
    got = ops.moe_experts_mxfp4(*gpu, block_m=128)
    assert got.dtype == torch.bfloat16 and got.shape == (t, h)
    got = got.float().cpu()
    print("T={} H={} I={} E={}: |ref|max {:.3f}  max diff {:.2e}".format(
        t, h, inter, e, float(ref.abs().max()),
        float((got - ref).abs().max())))
    torch.testing.assert_close(got, ref, **TOL)


@pytest.mark.parametrize("h,inter,e", [(256, 512, 4), (1536, 1408, 8)])
def test_tiled_mxfp4_bitwise_properties(monkeypatch, h, inter, e):
    gpu, _ = operands(300, h, inter, e, 300 + h + e)
    x8, xs, *wts, ids, w = gpu
    full = ops.moe_experts_mxfp4(*gpu, block_m=128)
    assert torch.equal(bits(full), bits(
        ops.moe_experts_mxfp4(*gpu, block_m=128))), "rerun"
    for r in (0, 13, 299):
        alone = ops.moe_experts_mxfp4(
            x8[r:r + 1].clone(), xs[r:r + 1].clone(), *wts,
            ids[r:r + 1].clone(), w[r:r + 1].clone(), block_m=128)
        assert torch.equal(bits(alone), bits(full[r:r + 1])), "row %d" % r
    monkeypatch.setattr(ops, "MOE_MXFP4_TILED_MIN", 128)
    assert ops._moe_mxfp4_path(300, False) == "tiled"
    assert torch.equal(bits(ops.moe_experts_mxfp4(*gpu)), bits(full))


@torch.inference_mode()  # as test_moe_block_captures_into_a_graph explains
def test_tiled_mxfp4_graph_replays_match_eager():
    gpu, _ = operands(300, 256, 512, 4, 300 + 256 + 4)
    eager = ops.moe_experts_mxfp4(*gpu, block_m=128)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.moe_experts_mxfp4(*gpu, block_m=128)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.moe_experts_mxfp4(*gpu, block_m=128)
    for i in range(3):
        out.zero_()
        graph.replay()
        assert torch.equal(bits(out), bits(eager)), "replay %d" % i


def test_mxfp4_moe_engine_prefill_on_the_tiled_path(monkeypatch):
    """A 189-token prompt with the tiled threshold lowered to 128: both MoE
    layers of mixtral-tiny prefill through the tiled kernels. The first greedy
    token equals the argmax of the same quantised model's prefill on the CPU
    (its model is copied over: the engine starts no mxfp4 model there), whose
    top-1 logit leads the runner-up by 0.1367 at |logit| ~ 0.99: 35 bf16
    ulps, measured on the CPU over 40 candidate prompts; decode then runs
    through the graphs."""
    monkeypatch.setattr(ops, "MOE_MXFP4_TILED_MIN", 128)
    prompt = "mxfp4 moe prefill 22 " * 9
    eng = LlmEngine(LlmEngineConfig(
        preset="mixtral-tiny", num_kv_blocks=128, block_size=16,
        max_model_len=256, device=DEV, max_num_seqs=8, decode_graphs=True,
        quantization="mxfp4"))
    eng.start()
    ids = eng.tokenizer.encode(prompt)
    t = len(ids)
    assert t > 128 and ops._moe_mxfp4_path(t, False) == "tiled"

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
