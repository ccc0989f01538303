"""ops.attention_decode_multi on the CPU: the contract it shares with
ops.attention_prefill_paged, and its shape limits."""

import pytest
import torch

import clearml_serving_amd.ops as ops


def _batch(sq):
    torch.manual_seed(0)
    pages, hkv, page, d = 12, 2, 16, 64
    k = torch.randn(pages, hkv, page, d)
    v = torch.randn(pages, hkv, page, d)
    btab = torch.randperm(pages, dtype=torch.int32).reshape(3, 4)
    q = torch.randn(3, sq, 8, d)
    kv = torch.tensor([5, 40, 64], dtype=torch.int32)
    ql = torch.tensor([min(3, sq), sq, 0], dtype=torch.int32)
    return q, k, v, btab, kv, ql


@pytest.mark.parametrize("window", [None, 7])
def test_decode_multi_is_paged_prefill_on_cpu(window):
    args = _batch(5)
    got = ops.attention_decode_multi(*args, window=window)
    want = ops.attention_prefill_paged(*args, window=window)
    assert torch.equal(got, want)


def test_decode_multi_rejects_nine_query_tokens():
    with pytest.raises(ValueError):
        ops.attention_decode_multi(*_batch(9))
