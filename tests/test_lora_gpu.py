"""GPU: the batched multi-LoRA kernels (ops/csrc/lora.hip) against the CPU
fp32 reference, and an engine mixed-adapter batch through decode graphs."""

import os
import sys

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.engines.llm.engine import LlmEngine, LlmEngineConfig
from clearml_serving_amd.models.llama import PRESETS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))
import lora_util  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L = 3
TOL = dict(atol=3e-2, rtol=3e-2)  # bf16 kernel tolerance of test_ops_gpu


def _mixed_idx(t):
    # -1..2 in a fixed scramble: 1, 2, -1, 0, 1, ... (T=1 -> adapter 1)
    return ((torch.arange(t) * 5 + 2) % (L + 1) - 1).to(torch.int32)


def _inputs(t, k, n, r, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(t, k, generator=g).to(torch.bfloat16)
    a = (torch.randn(L, r, k, generator=g) * k ** -0.5).to(torch.bfloat16)
    b = torch.randn(L, n, r, generator=g).to(torch.bfloat16)
    out = torch.randn(t, n, generator=g).to(torch.bfloat16)
    return x, a, b, out


# K 8960: K/8 is no multiple of the 64 lanes; N 1528: no multiple of 256
@pytest.mark.parametrize("r", [16, 48])
@pytest.mark.parametrize("k,n", [(256, 256), (1536, 2048), (8960, 1528)])
@pytest.mark.parametrize("t", [1, 5, 67])
def test_lora_kernels_match_cpu_reference(t, k, n, r):
    x, a, b, out = _inputs(t, k, n, r, seed=t + k + r)
    idx = _mixed_idx(t)
    live = idx >= 0
    y_ref = ops.lora_shrink(x.float(), a.float(), idx)
    out_ref = ops.lora_expand_add(y_ref, b.float(), idx, out.float().clone())

    idx_d = idx.to(DEV)
    y = ops.lora_shrink(x.to(DEV), a.to(DEV), idx_d)
    assert y.dtype == torch.float32 and tuple(y.shape) == (t, r)
    torch.testing.assert_close(y.cpu()[live], y_ref[live], **TOL)

    # expand alone on the reference y (skipped rows poisoned: never read)
    y_in = y_ref.clone()
    y_in[~live] = float("nan")
    out_d = out.to(DEV)
    ops.lora_expand_add(y_in.to(DEV), b.to(DEV), idx_d, out_d)
    torch.testing.assert_close(out_d.float().cpu(), out_ref, **TOL)
    assert torch.equal(out_d.cpu()[~live].view(torch.int16),
                       out[~live].view(torch.int16))

    # the pair as the model chains it (y straight from the shrink kernel)
    out_d2 = out.to(DEV)
    ops.lora_expand_add(y, b.to(DEV), idx_d, out_d2)
    torch.testing.assert_close(out_d2.float().cpu(), out_ref, **TOL)
    assert torch.equal(out_d2.cpu()[~live].view(torch.int16),
                       out[~live].view(torch.int16))


@pytest.mark.parametrize("t", [5, 67])
def test_lora_all_rows_skipped_leave_out_untouched(t):
    k, n, r = 1536, 1528, 48
    x, a, b, out = _inputs(t, k, n, r, seed=3)
    idx = torch.full((t,), -1, dtype=torch.int32, device=DEV)
    y = ops.lora_shrink(x.to(DEV), a.to(DEV), idx)
    assert tuple(y.shape) == (t, r)
    y_nan = torch.full((t, r), float("nan"), device=DEV)
    out_d = out.to(DEV)
    ops.lora_expand_add(y_nan, b.to(DEV), idx, out_d)
    assert torch.equal(out_d.cpu().view(torch.int16), out.view(torch.int16))


def test_lora_kernels_reject_unsupported_shapes():
    x, a, b, out = (v.to(DEV) for v in _inputs(2, 64, 64, 16))
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    y = ops.lora_shrink(x, a, idx)
    with pytest.raises(RuntimeError):  # K % 8
        ops.lora_shrink(x[:, :60].contiguous(), a[:, :, :60].contiguous(),
                        idx)
    with pytest.raises(RuntimeError):  # R % 16
        ops.lora_shrink(x, a[:, :8].contiguous(), idx)
    with pytest.raises(RuntimeError):  # idx dtype
        ops.lora_shrink(x, a, idx.long())
    with pytest.raises(RuntimeError):  # N % 8
        ops.lora_expand_add(y, b[:, :60].contiguous(), idx,
                            out[:, :60].contiguous())
    with pytest.raises(RuntimeError):  # out not contiguous
        ops.lora_expand_add(y, b[:, :32].contiguous(), idx, out[:, ::2])


def test_engine_mixed_adapter_batch_graphs_match_eager(tmp_path):
    """llama-tiny bf16, one batch of base + adapter 1 + adapter 2 rows:
    decode graphs (lora_idx staged, padded rows -1; 3 rows in the 4-bucket)
    emit the tokens of eager decode, and a second run repeats them."""
    mcfg = PRESETS["llama-tiny"]
    lora_util.write_adapter(str(tmp_path / "ad1"), mcfg, lora_util.ALL_LINEAR,
                            seed=1)
    lora_util.write_adapter(str(tmp_path / "ad2"), mcfg, lora_util.ATTN_ONLY,
                            seed=2)
    prompts = [[(3 + 7 * j) % 500 for j in range(11)]] * 3
    loras = [-1, 0, 1]

    def engine(graphs):
        eng = LlmEngine(LlmEngineConfig(
            preset="llama-tiny", num_kv_blocks=128, block_size=16,
            max_model_len=256, device=DEV, max_num_seqs=8,
            decode_graphs=graphs,
            lora_modules=[{"name": "ad1", "path": str(tmp_path / "ad1")},
                          {"name": "ad2", "path": str(tmp_path / "ad2")}]))
        eng.start()
        return eng

    eager = engine(False)
    want, _ = lora_util.generate_batch(eager, prompts, loras, max_tokens=16)
    assert eager.stats["graph_replays"] == 0
    graphed = engine(True)
    got, _ = lora_util.generate_batch(graphed, prompts, loras, max_tokens=16)
    again, _ = lora_util.generate_batch(graphed, prompts, loras,
                                        max_tokens=16)
    assert graphed.stats["graph_replays"] > 0
    assert got == want
    assert again == got
    # the adapters are live: same prompt, three different continuations
    assert got[0] != got[1] and got[0] != got[2] and got[1] != got[2]
    assert graphed.stats["lora_requests"] == 4
