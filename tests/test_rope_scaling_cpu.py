"""models/rope_scaling.py against transformers' ROPE_INIT_FUNCTIONS. The
oracle computes in float32, ours in float64 rounded once, so the oracle's own
error bounds the comparison: its exponent i/dim carries one fp32 rounding
(2^-24), which base**x amplifies by ln(base)*x <= ln(1e6) = 13.8 (8.2e-7),
plus a few 6e-8 ulps for pow, divide and the band blend: rtol 2e-6."""

import pytest
import torch
from transformers import LlamaConfig as HfLlamaConfig
from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS

from clearml_serving_amd.models.rope_scaling import rope_inv_freq

SCALINGS = [
    ({"rope_type": "linear", "factor": 4.0}, 10000.0),
    ({"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
      "high_freq_factor": 4.0, "original_max_position_embeddings": 8192},
     500000.0),
    ({"rope_type": "yarn", "factor": 4.0, "beta_fast": 32.0, "beta_slow": 1.0,
      "original_max_position_embeddings": 4096}, 1000000.0),
]


@pytest.mark.parametrize("head_dim", [64, 128])
@pytest.mark.parametrize("scaling,theta", SCALINGS)
def test_inv_freq_matches_transformers(scaling, theta, head_dim):
    hf_cfg = HfLlamaConfig(
        hidden_size=4 * head_dim, num_attention_heads=4, head_dim=head_dim,
        max_position_embeddings=32768,
        rope_parameters={**scaling, "rope_theta": theta})
    ref, ref_attn = ROPE_INIT_FUNCTIONS[scaling["rope_type"]](hf_cfg, "cpu")
    got, attn = rope_inv_freq(head_dim, theta, scaling, 32768)
    torch.testing.assert_close(got, ref, rtol=2e-6, atol=0.0)
    assert attn == pytest.approx(ref_attn, rel=1e-12)


def test_dynamic_scaling_raises():
    with pytest.raises(ValueError, match="dynamic"):
        rope_inv_freq(128, 1e4, {"rope_type": "dynamic", "factor": 2.0}, 4096)
