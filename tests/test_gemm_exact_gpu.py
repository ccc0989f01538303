"""GPU: bit-exact tile-edge tests for the MFMA GEMM/conv kernel family.

Every case feeds small integers (helpers/exact_gemm.py), so fp32
accumulation is exact in any order and the kernel output must equal
round_to_bf16(float64 result) bit for bit -- no tolerance anywhere. The
shapes come from the kernels' loop structure:

- skinny_gemm v1 (8 waves split K in 32-wide steps, 2-deep unrolled loop +
  tail): K=32 leaves waves 1..7 idle, K=96 three waves one tail step each,
  K=352 five waves one unrolled pair / one wave tail only / two idle, K=544
  five waves pair+tail / one pair only / two idle, K=800 six waves two pairs
  / one tail only / one idle. skinny_gemm_fp8 v1 is the same with 64-wide
  steps: K = 64, 192, 704, 1088, 1600.
- skinny_gemm v2 / fp8 v2 (LDS windows of 64 / 128 k): n_win = 1 (no
  second load), 2 (no third load), 3 (odd, ends in buffer 0), 7.
- M on both sides of every 16-row edge, i.e. every MT instantiation.
- gemm_bf16: grids of 1, 2, 6 (< 8), 8, 16 (% 8 == 0), 9, 20 (% 8 != 0)
  workgroups for the XCD block remap; K=32 is the single-stage case.
- conv3x3_nhwc: C=32 (no prefetch), K=192 (NT=64, three z-blocks), all
  eight bias x relu x residual epilogues at the three widths.
"""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

import clearml_serving_amd.ops as ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))
import exact_gemm as eg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = eg.SKINNY_N
CL = torch.channels_last


def _ext():
    ext = ops.extension_or_none()
    assert ext is not None, "HIP extension missing on GPU box"
    return ext


def _bf16_inputs(m, k, n=N):
    seed = eg.case_seed(m, k, n)
    return (eg.int_bf16((m, k), -3, 3, seed),
            eg.int_bf16((n, k), -3, 3, seed + 1))


def _fp8_inputs(m, k, n=N):
    seed = eg.case_seed(m, k, n, 8)
    return (eg.int_fp8((m, k), -4, 4, seed), eg.pow2_scales(m, "a"),
            eg.int_fp8((n, k), -4, 4, seed + 1), eg.pow2_scales(n, "w"))


def _dev(*tensors):
    return [t.to(DEV) for t in tensors]


# ------------------------------------------------------------------ #
# skinny_gemm (bf16) v1 / v2 / auto
# ------------------------------------------------------------------ #
def _check_skinny(m, k, variant, n=N):
    a, w = _bf16_inputs(m, k, n)
    got = _ext().skinny_gemm(*_dev(a, w), variant)
    eg.assert_bit_equal(got, eg.ref_gemm_bf16_exact(a, w))


@pytest.mark.parametrize("m,k", eg.SKINNY_V1_CASES)
def test_skinny_gemm_v1_exact(m, k):
    _check_skinny(m, k, 1)


@pytest.mark.parametrize("m,k", eg.SKINNY_V2_CASES)
def test_skinny_gemm_v2_exact(m, k):
    _check_skinny(m, k, 2)


@pytest.mark.parametrize("m,k", eg.SKINNY_AUTO_CASES)
def test_skinny_gemm_auto_exact(m, k):
    # (16, 192) -> v1, (17, 192) -> v2, (17, 96) -> v1 (K % 64 != 0)
    _check_skinny(m, k, 0)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_skinny_gemm_single_workgroup_exact(variant):
    _check_skinny(33, 192, variant, n=16)


@pytest.mark.parametrize("variant", [1, 2])
def test_skinny_gemm_single_row_view_exact(variant):
    # decode M=1: a row cut out of a wider tensor is contiguous (torch
    # ignores the stride of a size-1 dim) though stride(0) != K
    big, w = _bf16_inputs(1, 256)
    w = w[:, 128:].contiguous()
    dbig, dw = _dev(big, w)
    dx = dbig[:, 128:]
    assert dx.is_contiguous() and dx.stride(0) == 256
    eg.assert_bit_equal(_ext().skinny_gemm(dx, dw, variant),
                        eg.ref_gemm_bf16_exact(big[:, 128:], w))


# ------------------------------------------------------------------ #
# skinny_gemm_fp8 v1 (plain + pre-swizzled weight) / v2
# ------------------------------------------------------------------ #
@pytest.mark.parametrize("m,k", eg.FP8_V1_CASES)
def test_skinny_gemm_fp8_v1_exact(m, k):
    a8, as_, w8, ws = _fp8_inputs(m, k)
    ref = eg.ref_gemm_fp8_exact(a8, as_, w8, ws)
    da8, das, dw8, dws = _dev(a8, as_, w8, ws)
    plain = ops.skinny_gemm_fp8(da8, das, dw8, dws)
    eg.assert_bit_equal(plain, ref)
    dw8s = ops.swizzle_fp8_weight(dw8)
    pre = ops.skinny_gemm_fp8(da8, das, dw8s, dws, swizzled=True)
    eg.assert_bit_equal(pre, ref)
    assert torch.equal(plain, pre)


@pytest.mark.parametrize("m,k", eg.FP8_V2_CASES)
def test_skinny_gemm_fp8_v2_exact(m, k):
    a8, as_, w8, ws = _fp8_inputs(m, k)
    got = ops.skinny_gemm_fp8_v2(*_dev(a8, as_, w8, ws))
    eg.assert_bit_equal(got, eg.ref_gemm_fp8_exact(a8, as_, w8, ws))


@pytest.mark.parametrize("version", [1, 2])
def test_skinny_gemm_fp8_single_workgroup_exact(version):
    a8, as_, w8, ws = _fp8_inputs(33, 384, n=16)
    fn = ops.skinny_gemm_fp8 if version == 1 else ops.skinny_gemm_fp8_v2
    eg.assert_bit_equal(fn(*_dev(a8, as_, w8, ws)),
                        eg.ref_gemm_fp8_exact(a8, as_, w8, ws))


# ------------------------------------------------------------------ #
# gemm_bf16
# ------------------------------------------------------------------ #
@pytest.mark.parametrize("m,n,k", eg.GEMM_GRID_CASES)
def test_gemm_bf16_on_grid_exact(m, n, k):
    a, w = _bf16_inputs(m, k, n)
    got = _ext().gemm_bf16(*_dev(a, w))
    eg.assert_bit_equal(got, eg.ref_gemm_bf16_exact(a, w))


@pytest.mark.parametrize("m,n,k", eg.GEMM_PADDED_CASES)
def test_gemm_bf16_padded_exact(m, n, k):
    a, w = _bf16_inputs(m, k, n)
    got = ops.gemm_bf16(*_dev(a, w))
    assert got.is_contiguous()
    eg.assert_bit_equal(got, eg.ref_gemm_bf16_exact(a, w))


# ------------------------------------------------------------------ #
# conv3x3_nhwc
# ------------------------------------------------------------------ #
_CONV_CACHE = {}


def _conv_case(n, c, k, width):
    """CPU inputs + the float64 convolution, computed once per shape and
    shared (unchanged) by every epilogue of that shape."""
    key = (n, c, k, width)
    if key not in _CONV_CACHE:
        seed = eg.case_seed(n, c, k, width)
        x = eg.int_bf16((n, c, width, width), -2, 2, seed)
        w = eg.int_bf16((k, c, 3, 3), -2, 2, seed + 1)
        bias = eg.int_bf16((k,), -2, 2, seed + 2)
        res = eg.int_bf16((n, k, width, width), -2, 2, seed + 3)
        _CONV_CACHE[key] = (x, w, bias, res, eg.conv3x3_f64(x, w))
    return _CONV_CACHE[key]


def _check_conv(n, c, k, width, has_bias, relu, has_res):
    x, w, bias, res, conv = _conv_case(n, c, k, width)
    b = bias if has_bias else None
    r = res if has_res else None
    got = _ext().conv3x3_nhwc(
        x.to(DEV).contiguous(memory_format=CL),
        w.to(DEV).contiguous(memory_format=CL),
        b.to(DEV) if has_bias else None, relu,
        r.to(DEV).contiguous(memory_format=CL) if has_res else None)
    assert got.shape == (n, k, width, width)
    assert got.is_contiguous(memory_format=CL)
    eg.assert_bit_equal(got, eg.ref_conv3x3_exact(x, w, b, relu, r,
                                                  conv=conv))


@pytest.mark.parametrize("has_bias,relu,has_res", eg.EPILOGUES)
@pytest.mark.parametrize("n,c,k", eg.CONV_EPILOGUE_SHAPES)
@pytest.mark.parametrize("width", eg.CONV_WIDTHS)
def test_conv3x3_epilogues_exact(width, n, c, k, has_bias, relu, has_res):
    _check_conv(n, c, k, width, has_bias, relu, has_res)


@pytest.mark.parametrize("n,c,k,width", eg.CONV_DEEP_CASES)
def test_conv3x3_deep_channels_exact(n, c, k, width):
    _check_conv(n, c, k, width, True, True, True)


@pytest.mark.parametrize("width", eg.CONV_WIDTHS)
def test_conv3x3_wrapper_converts_nchw(width):
    n, c, k = 1, 32, 128
    x, w, bias, res, conv = _conv_case(n, c, k, width)
    dx, dw, db, dr = _dev(x, w, bias, res)
    assert dx.is_contiguous() and dw.is_contiguous()   # NCHW as built
    assert ops.conv3x3_supported(dx, dw) is True
    dr = dr.contiguous(memory_format=CL)
    from_nchw = ops.conv3x3_nhwc(dx, dw, db, True, dr)
    from_nhwc = ops.conv3x3_nhwc(dx.contiguous(memory_format=CL),
                                 dw.contiguous(memory_format=CL),
                                 db, True, dr)
    assert from_nchw.is_contiguous(memory_format=CL)
    assert torch.equal(from_nchw, from_nhwc)
    eg.assert_bit_equal(from_nchw, eg.ref_conv3x3_exact(x, w, bias, True,
                                                        res, conv=conv))


def test_conv3x3_wrapper_unsupported_shape_falls_back():
    n, c, k, width = 1, 48, 64, 7
    x, w, bias, res, conv = _conv_case(n, c, k, width)
    dx, dw, db, dr = _dev(x, w, bias, res)
    assert ops.conv3x3_supported(dx, dw) is False
    got = ops.conv3x3_nhwc(dx, dw, db, True, dr)
    assert got.shape == (n, k, width, width)
    eg.assert_bit_equal(got.contiguous(),
                        eg.ref_conv3x3_exact(x, w, bias, True, res,
                                             conv=conv))


# ------------------------------------------------------------------ #
# determinism (greedy decoding depends on it)
# ------------------------------------------------------------------ #
def test_skinny_kernels_are_deterministic():
    # K=800 is in contract for bf16 v1 only; the other three run at the
    # next K their window size admits (832 = 13*64, 896 = 7*128)
    m, n = 17, 320
    g = torch.Generator().manual_seed(17800320)
    ext = _ext()

    def randn(k):
        a = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
        w = torch.randn(n, k, generator=g).to(torch.bfloat16).to(DEV)
        return a, w

    def twice(fn, *args):
        first = fn(*args)
        second = fn(*args)
        assert torch.isfinite(first.float()).all()
        assert torch.equal(first, second), fn

    a, w = randn(800)
    twice(ext.skinny_gemm, a, w, 1)
    a, w = randn(832)
    twice(ext.skinny_gemm, a, w, 2)
    a8, as_ = ops.quant_fp8(a)
    w8, ws = ops.quant_fp8(w)
    twice(ops.skinny_gemm_fp8, a8, as_, w8, ws)
    a, w = randn(896)
    a8, as_ = ops.quant_fp8(a)
    w8, ws = ops.quant_fp8(w)
    twice(ops.skinny_gemm_fp8_v2, a8, as_, w8, ws)


# ------------------------------------------------------------------ #
# host contract: rejected by TORCH_CHECK before any launch
# ------------------------------------------------------------------ #
@pytest.mark.parametrize("m,k,n,variant", [
    (129, 64, 48, 1), (129, 64, 48, 2), (0, 64, 48, 1),
    (4, 48, 48, 1), (4, 64, 40, 1), (33, 96, 48, 2)])
def test_skinny_gemm_rejects_out_of_contract(m, k, n, variant):
    a = torch.zeros(m, k, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(n, k, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="skinny_gemm"):
        _ext().skinny_gemm(a, w, variant)


def test_skinny_gemm_rejects_noncontiguous_weight():
    a = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(96, 64, dtype=torch.bfloat16, device=DEV)[::2]
    with pytest.raises(RuntimeError, match="W must be contiguous"):
        _ext().skinny_gemm(a, w, 1)


@pytest.mark.parametrize("version,m,k", [(1, 65, 64), (1, 4, 96),
                                         (2, 65, 128), (2, 33, 192)])
def test_skinny_gemm_fp8_rejects_out_of_contract(version, m, k):
    ext = _ext()
    fn = ext.skinny_gemm_fp8 if version == 1 else ext.skinny_gemm_fp8_v2
    a8 = torch.zeros(m, k, dtype=torch.uint8, device=DEV)
    w8 = torch.zeros(N, k, dtype=torch.uint8, device=DEV)
    as_ = torch.ones(m, dtype=torch.float32, device=DEV)
    ws = torch.ones(N, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="skinny_gemm_fp8"):
        fn(a8, as_, w8, ws)


def test_gemm_bf16_ext_rejects_off_grid():
    a = torch.zeros(100, 32, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(128, 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="gemm_bf16 needs"):
        _ext().gemm_bf16(a, b)


def test_conv3x3_ext_rejects_width_7():
    x = torch.zeros(1, 32, 7, 7, dtype=torch.bfloat16,
                    device=DEV).contiguous(memory_format=CL)
    w = torch.zeros(64, 32, 3, 3, dtype=torch.bfloat16,
                    device=DEV).contiguous(memory_format=CL)
    with pytest.raises(RuntimeError, match="supported widths"):
        _ext().conv3x3_nhwc(x, w, None, False, None)


# ------------------------------------------------------------------ #
# ops.skinny_linear: both sides of the routing boundary
# ------------------------------------------------------------------ #
@pytest.mark.parametrize("m", [0, 1, 2, 16, 17])
def test_skinny_linear_exact(m):
    k = 64
    a = eg.int_bf16((m, k), -3, 3, eg.case_seed(m, k, N, 1))
    _, w = _bf16_inputs(1, k)
    got = ops.skinny_linear(*_dev(a, w))
    assert got.shape == (m, N)
    eg.assert_bit_equal(got, eg.ref_gemm_bf16_exact(a, w))


@pytest.mark.parametrize("m", [1, 16, 17])
def test_skinny_linear_noncontiguous_weight_exact(m):
    a, _ = _bf16_inputs(m, 64)
    big = eg.int_bf16((2 * N, 64), -3, 3, eg.case_seed(m, 2 * N))
    da, dbig = _dev(a, big)
    dw = dbig[::2]                       # row slice, step 2
    assert not dw.is_contiguous()
    got = ops.skinny_linear(da, dw)
    assert torch.equal(got, F.linear(da, dw))
    eg.assert_bit_equal(got, eg.ref_gemm_bf16_exact(a, big[::2]))


@pytest.mark.parametrize("m,off", [(1, 0), (16, 0), (17, 0), (1, 4), (2, 4)])
def test_skinny_linear_noncontiguous_x_exact(m, off):
    # column slice; off=4 starts 8 bytes into a row, so the single-row
    # view (which .contiguous() does not copy) is not 16-byte aligned and
    # must not reach the kernel's vector loads
    big, w = _bf16_inputs(m, 128)
    w = w[:, :64].contiguous()
    dbig, dw = _dev(big, w)
    dx = dbig[:, off:off + 64]
    assert not (dx.is_contiguous() and m > 1)
    got = ops.skinny_linear(dx, dw)
    eg.assert_bit_equal(got,
                        eg.ref_gemm_bf16_exact(big[:, off:off + 64], w))
