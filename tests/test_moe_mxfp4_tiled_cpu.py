"""Routing of ops.moe_experts_mxfp4 between the loop, the tiled kernels and
the two fused row blocks, with the thresholds patched so that the measured
defaults do not matter."""

import pytest

import clearml_serving_amd.ops as ops


@pytest.mark.parametrize("t,capturing,path", [
    (256, False, "fused16"), (256, True, "fused16"),
    (511, False, "fused64"), (511, True, "fused64"),
    (512, False, "tiled"), (512, True, "tiled"),
    (4096, False, "tiled"), (4096, True, "tiled"),
    (5000, False, "loop"),
    (5000, True, "tiled"),
])
def test_moe_mxfp4_path(monkeypatch, t, capturing, path):
    monkeypatch.setattr(ops, "MOE_MXFP4_BLOCK16_MAX", 256)
    monkeypatch.setattr(ops, "MOE_MXFP4_TILED_MIN", 512)
    monkeypatch.setattr(ops, "MOE_MXFP4_FUSED_MAX", 4096)
    assert ops._moe_mxfp4_path(t, capturing) == path
