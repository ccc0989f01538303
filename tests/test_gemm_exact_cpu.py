"""CPU side of the bit-exact GEMM/conv tests.

Proves the instrument before the GPU file relies on it: assert_bit_equal
sees a one-ulp change, the integer inputs of every GPU case make a single
dropped 32-wide k-step visible after bf16 rounding, and the CPU fallbacks of
the ops agree bit for bit with the float64 references. Also the pure-Python
routing around the kernels (Fp8Linear._route, ops.skinny_linear).
"""

import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import clearml_serving_amd.ops as ops
from clearml_serving_amd.models.quant import Fp8Linear

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))
import exact_gemm as eg  # noqa: E402

N = eg.SKINNY_N


def _bf16_inputs(m, k, n=N):
    seed = eg.case_seed(m, k, n)
    return (eg.int_bf16((m, k), -3, 3, seed),
            eg.int_bf16((n, k), -3, 3, seed + 1))


def _fp8_inputs(m, k, n=N):
    seed = eg.case_seed(m, k, n, 8)
    return (eg.int_fp8((m, k), -4, 4, seed), eg.pow2_scales(m, "a"),
            eg.int_fp8((n, k), -4, 4, seed + 1), eg.pow2_scales(n, "w"))


def _conv_inputs(n, c, k, width):
    seed = eg.case_seed(n, c, k, width)
    x = eg.int_bf16((n, c, width, width), -2, 2, seed)
    w = eg.int_bf16((k, c, 3, 3), -2, 2, seed + 1)
    bias = eg.int_bf16((k,), -2, 2, seed + 2)
    res = eg.int_bf16((n, k, width, width), -2, 2, seed + 3)
    return x, w, bias, res


# ------------------------------------------------------------------ #
# the instrument
# ------------------------------------------------------------------ #
def test_assert_bit_equal_accepts_equal_and_rejects_one_ulp():
    a, w = _bf16_inputs(17, 96)
    ref = eg.ref_gemm_bf16_exact(a, w)
    eg.assert_bit_equal(ref.clone(), ref)
    got = ref.clone()
    got.view(torch.int16)[5, 33] += 1          # one ulp, one element
    with pytest.raises(AssertionError) as ei:
        eg.assert_bit_equal(got, ref)
    msg = str(ei.value)
    assert "1 of {} elements".format(ref.numel()) in msg
    assert "(row 5, col 33)" in msg
    assert "rows hit [5]" in msg and "cols hit [33]" in msg


def test_assert_bit_equal_rejects_nan_shape_and_dtype():
    ref = torch.zeros(4, 16, dtype=torch.bfloat16)
    got = ref.clone()
    got[2, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"\(row 2, col 3\)"):
        eg.assert_bit_equal(got, ref)
    with pytest.raises(AssertionError, match="shape"):
        eg.assert_bit_equal(ref[:3], ref)
    with pytest.raises(AssertionError, match="dtype"):
        eg.assert_bit_equal(ref.float(), ref)


def test_assert_bit_equal_reports_tile_pattern():
    # a whole 16-column tile of rows 16..31 wrong -> the report names it
    ref = eg.ref_gemm_bf16_exact(*_bf16_inputs(33, 64))
    got = ref.clone()
    got[16:32, 16:32] += 1
    with pytest.raises(AssertionError) as ei:
        eg.assert_bit_equal(got, ref)
    msg = str(ei.value)
    assert "rows hit {}".format(list(range(16, 32))) in msg
    assert "cols hit {}".format(list(range(16, 32))) in msg


def test_inputs_are_integers_without_constant_rows():
    a = eg.int_bf16((64, 32), -3, 3, 7).float()
    assert a.min() >= -3 and a.max() <= 3 and torch.equal(a, a.round())
    assert not (a == a[:, :1]).all(dim=1).any()
    assert not torch.equal(a[:32], a[:32].T)   # asymmetric
    b = eg.int_fp8((64, 64), -4, 4, 7).view(eg.F8).float()
    assert b.min() >= -4 and b.max() <= 4 and torch.equal(b, b.round())
    assert torch.equal(eg.int_bf16((5, 7), -3, 3, 11),
                       eg.int_bf16((5, 7), -3, 3, 11))
    for pat in ("a", "w"):
        s = eg.pow2_scales(48, pat)
        assert s.dtype == torch.float32
        assert torch.equal(torch.log2(s), torch.log2(s).round())
        assert s.unique().numel() > 1


# ------------------------------------------------------------------ #
# a dropped 32-wide k-step is visible at every GPU case
# ------------------------------------------------------------------ #
def _assert_every_dropped_step_visible(a, w, ref_fn):
    """Zero each 32-wide k-step of A in turn (= the kernel skipping that
    MFMA step); the bf16-rounded result must change every time."""
    ref = ref_fn(a, w)
    k = a.shape[1]
    for k0 in range(0, k, 32):
        a2 = a.clone()
        a2[:, k0:k0 + 32] = 0
        with pytest.raises(AssertionError, match="not bit-equal"):
            eg.assert_bit_equal(ref_fn(a2, w), ref)


@pytest.mark.parametrize(
    "m,k", sorted(set(eg.SKINNY_V1_CASES + eg.SKINNY_V2_CASES
                      + eg.SKINNY_AUTO_CASES)))
def test_dropped_kstep_visible_bf16_skinny(m, k):
    a, w = _bf16_inputs(m, k)
    _assert_every_dropped_step_visible(a, w, eg.ref_gemm_bf16_exact)


@pytest.mark.parametrize("m,k",
                         sorted(set(eg.FP8_V1_CASES + eg.FP8_V2_CASES)))
def test_dropped_kstep_visible_fp8_skinny(m, k):
    a8, as_, w8, ws = _fp8_inputs(m, k)

    def ref_fn(a, w):
        return eg.ref_gemm_fp8_exact(a, as_, w, ws)

    _assert_every_dropped_step_visible(a8, w8, ref_fn)


@pytest.mark.parametrize("m,n,k", eg.GEMM_GRID_CASES + eg.GEMM_PADDED_CASES)
def test_dropped_kstep_visible_gemm_bf16(m, n, k):
    a, w = _bf16_inputs(m, k, n)
    _assert_every_dropped_step_visible(a, w, eg.ref_gemm_bf16_exact)


@pytest.mark.parametrize("n,c,k,width", [(1, 32, 128, 14), (2, 64, 192, 14),
                                         (1, 96, 64, 14)])
def test_dropped_tap_chunk_visible_conv(n, c, k, width):
    # the conv's k-step is one (tap, 32-channel chunk)
    x, w, bias, res = _conv_inputs(n, c, k, width)
    ref = eg.ref_conv3x3_exact(x, w, bias, True, res)
    for c0 in range(0, c, 32):
        for dy, dx in ((0, 0), (1, 1), (2, 1)):
            w2 = w.clone()
            w2[:, c0:c0 + 32, dy, dx] = 0
            with pytest.raises(AssertionError, match="not bit-equal"):
                eg.assert_bit_equal(
                    eg.ref_conv3x3_exact(x, w2, bias, True, res), ref)


def test_exactness_headroom():
    # the worst partial sum of every case stays far below 2^24, and the
    # fp32 matmul equals the float64 one exactly at the largest K
    assert 3 * 3 * 800 < 2 ** 24 and 4 * 4 * 1600 < 2 ** 24
    assert 9 * 256 * 2 * 2 + 4 < 2 ** 24
    a, w = _bf16_inputs(17, 800)
    assert torch.equal((a.float() @ w.float().T).double(),
                       a.double() @ w.double().T)
    vals = torch.arange(-8, 9).float()
    assert torch.equal(vals.to(eg.F8).float(), vals)
    assert torch.equal(vals.to(torch.bfloat16).float(), vals)


# ------------------------------------------------------------------ #
# CPU fallbacks of the ops == exact references
# ------------------------------------------------------------------ #
@pytest.mark.parametrize("m,k", [(1, 64), (17, 192), (64, 1088)])
def test_cpu_skinny_gemm_fp8_plain_and_swizzled(m, k):
    a8, as_, w8, ws = _fp8_inputs(m, k)
    ref = eg.ref_gemm_fp8_exact(a8, as_, w8, ws)
    eg.assert_bit_equal(ops.skinny_gemm_fp8(a8, as_, w8, ws), ref)
    w8s = ops.swizzle_fp8_weight(w8)
    assert not torch.equal(w8s, w8)
    assert torch.equal(ops.unswizzle_fp8_weight(w8s), w8)
    eg.assert_bit_equal(
        ops.skinny_gemm_fp8(a8, as_, w8s, ws, swizzled=True), ref)


@pytest.mark.parametrize("m,k", [(1, 128), (33, 384), (64, 896)])
def test_cpu_skinny_gemm_fp8_v2(m, k):
    a8, as_, w8, ws = _fp8_inputs(m, k)
    eg.assert_bit_equal(ops.skinny_gemm_fp8_v2(a8, as_, w8, ws),
                        eg.ref_gemm_fp8_exact(a8, as_, w8, ws))


@pytest.mark.parametrize("m,n,k", [(128, 128, 32)] + eg.GEMM_PADDED_CASES)
def test_cpu_gemm_bf16(m, n, k):
    a, w = _bf16_inputs(m, k, n)
    eg.assert_bit_equal(ops.gemm_bf16(a, w), eg.ref_gemm_bf16_exact(a, w))


@pytest.mark.parametrize("bias,relu,res", eg.EPILOGUES)
def test_cpu_conv3x3_nhwc(bias, relu, res):
    x, w, b, r = _conv_inputs(1, 32, 64, 14)
    b = b if bias else None
    r = r if res else None
    eg.assert_bit_equal(ops.conv3x3_nhwc(x, w, b, relu, r).contiguous(),
                        eg.ref_conv3x3_exact(x, w, b, relu, r))


def test_cpu_conv3x3_supported_is_false():
    x, w, _, _ = _conv_inputs(1, 32, 64, 14)
    assert ops.conv3x3_supported(x, w) is False


# ------------------------------------------------------------------ #
# Fp8Linear._route as a pure table
# ------------------------------------------------------------------ #
def _fp8_linear(k, n, skinny_max=16, v2_max=0):
    lin = Fp8Linear(nn.Linear(k, n, bias=False))
    lin.SKINNY_MAX_M = skinny_max      # instance attributes: the class
    lin.V2_MAX_M = v2_max              # defaults (and the env) stay put
    return lin


def test_fp8_route_boundaries_default_v2_off():
    lin = _fp8_linear(128, 32)
    assert [lin._route(m) for m in (1, 16, 17, 64, 65)] == \
        ["v1", "v1", "lt", "lt", "lt"]


def test_fp8_route_boundaries_v2_enabled():
    lin = _fp8_linear(128, 32, v2_max=64)
    assert [lin._route(m) for m in (1, 16, 17, 64, 65)] == \
        ["v1", "v1", "v2", "v2", "lt"]


def test_fp8_route_k_alignment():
    # k % 64 != 0 -> never a skinny kernel
    lin = _fp8_linear(96, 32, v2_max=64)
    assert [lin._route(m) for m in (1, 16, 17, 64)] == ["lt"] * 4
    # k % 64 == 0 but k % 128 != 0: v1 still serves, v2 cannot
    lin = _fp8_linear(192, 32, v2_max=64)
    assert [lin._route(m) for m in (1, 16, 17, 64)] == \
        ["v1", "v1", "lt", "lt"]
    # n % 16 != 0 -> "lt"
    lin = _fp8_linear(128, 24, v2_max=64)
    assert [lin._route(m) for m in (1, 17)] == ["lt", "lt"]


def test_fp8_linear_unaligned_k_constructs_and_runs():
    # in_features % 64 != 0 has no swizzled weight (only v1 reads one) but
    # must still quantize and serve through the "lt" route
    torch.manual_seed(0)
    dense = nn.Linear(96, 32, bias=False)
    lin = Fp8Linear(dense)
    assert lin.weight_fp8_sw is None
    assert "weight_fp8_sw" not in lin.state_dict()
    x = torch.randn(3, 96)
    torch.testing.assert_close(lin(x), dense(x), atol=0.1, rtol=0.1)


def test_fp8_route_huge_n():
    lin = _fp8_linear(64, 16384, v2_max=64)
    assert lin._route(1) == "v1"
    assert lin._route(2) == "lt"
    assert lin._route(17) == "lt"      # v2 needs n < 16384


def test_fp8_linear_cpu_forward_q_is_exact():
    # the CPU route of Fp8Linear goes through the plain-layout fallback
    k, n, m = 128, 32, 5
    lin = _fp8_linear(k, n)
    a8, as_, w8, ws = _fp8_inputs(m, k, n)
    lin.weight_fp8.copy_(w8.view(eg.F8))
    lin.weight_fp8_sw.copy_(ops.swizzle_fp8_weight(w8))   # uint8 bytes
    lin.weight_scale.copy_(ws)
    eg.assert_bit_equal(lin.forward_q(a8, as_, out_dtype=torch.bfloat16),
                        eg.ref_gemm_fp8_exact(a8, as_, w8, ws))


# ------------------------------------------------------------------ #
# ops.skinny_linear on CPU == F.linear
# ------------------------------------------------------------------ #
def test_cpu_skinny_linear_empty_batch():
    _, w = _bf16_inputs(1, 64)
    x = torch.empty(0, 64, dtype=torch.bfloat16)
    y = ops.skinny_linear(x, w)
    assert y.shape == (0, N) and y.dtype == torch.bfloat16
    assert torch.equal(y, F.linear(x, w))


def test_cpu_skinny_linear_noncontiguous_weight():
    x, _ = _bf16_inputs(3, 64)
    big = eg.int_bf16((2 * N, 64), -3, 3, 5)
    w_rows = big[::2]                              # row slice, step 2
    w_t = eg.int_bf16((64, N), -3, 3, 6).t()       # .t() view
    for w in (w_rows, w_t):
        assert not w.is_contiguous()
        y = ops.skinny_linear(x, w)
        assert torch.equal(y, F.linear(x, w))
        eg.assert_bit_equal(y, eg.ref_gemm_bf16_exact(x, w))


def test_cpu_skinny_linear_3d_input():
    _, w = _bf16_inputs(1, 64)
    x = eg.int_bf16((2, 3, 64), -3, 3, 9)
    y = ops.skinny_linear(x, w)
    assert y.shape == (2, 3, N)
    assert torch.equal(y, F.linear(x, w))
    eg.assert_bit_equal(y.reshape(6, N),
                        eg.ref_gemm_bf16_exact(x.reshape(6, 64), w))
