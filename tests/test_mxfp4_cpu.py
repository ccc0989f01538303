"""MXFP4 quantiser, oracle and kernel tiling (ops/__init__.py), CPU only."""

import pytest
import torch

import clearml_serving_amd.ops as ops

GRID = torch.tensor(ops.E2M1_GRID)


def test_roundtrip_exact_on_representable_values():
    g = torch.Generator().manual_seed(0)
    n, k = 24, 160
    vals = GRID[torch.randint(0, 8, (n, k), generator=g)]
    vals[:, ::32] = 6.0  # pin each block's exponent: amax = 6 * 2^e
    sign = torch.randint(0, 2, (n, k), generator=g) * 2.0 - 1.0
    exp = torch.randint(-20, 20, (n, k // 32), generator=g)
    exp[0, 0], exp[1, 1] = -127, 125  # both ends of the e8m0 range
    w = torch.ldexp(vals * sign, exp.repeat_interleave(32, dim=1))
    w[2, 32:64] = 0.0  # all-zero block: scale 2^0
    w4, e8, rs = ops.quantize_mxfp4(w)
    assert w4.shape == (n, k // 2) and e8.shape == (n, k // 32)
    assert e8[2, 1] == 127 and torch.equal(e8[:2, :2].diag(),
                                           torch.tensor([0, 252]).byte())
    assert torch.equal(ops.dequant_mxfp4(w4, e8, rs), w)
    # even k in the low nibble: k=0 holds +-6 (code 7), sign in bit 3
    assert (w4[:, 0] & 0x7 == 7).all()


def test_error_within_half_a_grid_step():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(32, 256, generator=g) * torch.logspace(
        -3, 3, 32)[:, None]
    w4, e8, rs = ops.quantize_mxfp4(w)
    scale = torch.ldexp(torch.ones(32, 8), e8.int() - 127) \
        .repeat_interleave(32, dim=1)
    s = (w / scale).abs()  # exact: power-of-two scale
    # e2m1 spacing is .5 below 2, 1 on [2, 4), 2 on [4, 6]; above 6 the value
    # saturates, so the error is exactly the overshoot
    half = torch.where(s < 2, 0.25, torch.where(s < 4, 0.5, 1.0))
    bound = torch.where(s > 6, s - 6, half) * scale
    err = (ops.dequant_mxfp4(w4, e8, rs) - w).abs()
    assert (err <= bound).all()
    assert s.amax() < 8 and (s.reshape(32, 8, 32).amax(dim=2) >= 4).all()


@pytest.mark.parametrize("n,k", [(16, 128), (48, 512), (32, 640), (24, 96)])
def test_tile_untile_roundtrip(n, k):
    g = torch.Generator().manual_seed(k)
    w4 = torch.randint(0, 256, (n, k // 2), generator=g, dtype=torch.uint8)
    e8 = torch.randint(0, 255, (n, k // 32), generator=g, dtype=torch.uint8)
    w4t, e8t = ops.tile_mxfp4_weight(w4, e8)
    steps = (k + 127) // 128
    assert w4t.shape == ((n + 15) // 16, steps, 64, 16)
    assert e8t.shape == ((n + 15) // 16, (steps + 3) // 4, 64, 4)
    # lane 16g + r of tile (nb, ks): row 16nb + r, k = 128ks + 32g ..
    assert torch.equal(w4t[0, steps - 1, 16 * 0 + 5],
                       w4[5, (steps - 1) * 64:(steps - 1) * 64 + 16])
    assert e8t[0, 0, 16 * 2 + 3, 0] == e8[3, 2]
    if k % 512:
        assert (e8t[:, -1, :, (k // 128) % 4 + (k % 128 > 0):] == 127).all()
    back = ops.untile_mxfp4_weight(w4t, e8t, n, k)
    assert torch.equal(back[0], w4) and torch.equal(back[1], e8)
