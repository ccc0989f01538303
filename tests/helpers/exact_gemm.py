"""Bit-exact fixtures for the MFMA GEMM/conv kernels.

Small-integer operands make every product and every partial sum an integer
below 2^24, so fp32 accumulation is exact in ANY order: the K split across
waves, the LDS reduce and the MFMA-internal order all give the same fp32
value, and a kernel's bf16 output must equal round_to_bf16(exact sum) bit for
bit. Power-of-two scales keep the fp8 epilogue exact as well. No tolerance is
involved; the float64 references below are the whole specification.

The case lists are shared by the CPU file (which proves that the chosen
inputs make a dropped k-step visible) and the GPU file (which runs them).
"""

import itertools

import torch

F8 = torch.float8_e4m3fn

# ------------------------------------------------------------------ #
# case lists (the shapes are chosen from the kernels' loop structure)
# ------------------------------------------------------------------ #
SKINNY_N = 48                      # three 16-column workgroups
M_EDGES_128 = [1, 16, 17, 33, 49, 65, 81, 97, 113, 128]   # every MT 1..8
M_EDGES_64 = [1, 16, 17, 33, 49, 64]                      # every MT 1..4


def _cases(ks, ms, m_edges, k_edge):
    out = [(m, k) for k in ks for m in ms]
    out += [(m, k_edge) for m in m_edges if (m, k_edge) not in out]
    return out


# bf16 v1: 8 waves split K in 32-wide steps, 2-deep unrolled loop + tail
SKINNY_V1_CASES = _cases([32, 96, 352, 544, 800], [1, 17], M_EDGES_128, 544)
# bf16 v2: 64-wide LDS windows, n_win = 1, 2, 3, 7
SKINNY_V2_CASES = _cases([64, 128, 192, 448], [1, 33], M_EDGES_128, 192)
# fp8 v1: as bf16 v1 with 64-wide steps
FP8_V1_CASES = _cases([64, 192, 704, 1088, 1600], [1, 17], M_EDGES_64, 1088)
# fp8 v2: 128-wide LDS windows, n_win = 1, 2, 3, 7
FP8_V2_CASES = _cases([128, 256, 384, 896], [1, 33], M_EDGES_64, 384)
# variant=0 dispatch: (M, K) -> kernel the host picks
SKINNY_AUTO_CASES = [(16, 192), (17, 192), (17, 96)]

# gemm_bf16 on the 128/128/32 grid: 1, 2, 6, 8, 9, 16 and 20 workgroups
GEMM_GRID_CASES = [(128, 128, 32), (128, 256, 64), (384, 256, 96),
                   (256, 512, 64), (384, 384, 64), (512, 512, 32),
                   (512, 640, 160)]
GEMM_PADDED_CASES = [(1, 1, 1), (129, 127, 33), (100, 200, 300)]

# conv3x3: (n, C, K, width)
CONV_WIDTHS = [56, 28, 14]
CONV_EPILOGUE_SHAPES = [(2, 64, 192), (1, 32, 128)]        # per width
CONV_DEEP_CASES = [(1, 96, 64, 14), (2, 256, 256, 14)]
EPILOGUES = list(itertools.product([False, True], repeat=3))  # bias,relu,res


def case_seed(*dims):
    """Deterministic seed per case, distinct for distinct shapes."""
    s = 0
    for d in dims:
        s = s * 4099 + int(d)
    return s % (2 ** 31 - 1)


# ------------------------------------------------------------------ #
# inputs
# ------------------------------------------------------------------ #
def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    # no constant rows: a row of equal values hides swaps along k
    if t.dim() >= 1 and t.shape[-1] >= 2 and t.numel():
        flat = t.view(-1, t.shape[-1])
        const = (flat == flat[:, :1]).all(dim=1)
        flat[const, 0] = lo
        flat[const, 1] = hi
    return t


def int_bf16(shape, lo, hi, seed):
    """bf16 tensor of integers in [lo, hi] (all exact in bf16)."""
    assert -256 <= lo < hi <= 256
    return _ints(shape, lo, hi, seed).to(torch.bfloat16)


def int_fp8(shape, lo, hi, seed):
    """e4m3 bytes (uint8) of integers in [lo, hi]; -8..8 are exact in e4m3."""
    assert -8 <= lo < hi <= 8
    return _ints(shape, lo, hi, seed).to(F8).view(torch.uint8)


def pow2_scales(n, pattern):
    """float32 [n] power-of-two scales: 'a' = 2^-(i%3) (activation rows),
    'w' = 2^((i%4)-2) (weight rows), 'one' = 1."""
    i = torch.arange(n)
    if pattern == "a":
        e = -(i % 3)
    elif pattern == "w":
        e = (i % 4) - 2
    elif pattern == "one":
        e = torch.zeros_like(i)
    else:
        raise ValueError(pattern)
    return torch.exp2(e.double()).float()


# ------------------------------------------------------------------ #
# references (float64 on the CPU, one rounding to bf16)
# ------------------------------------------------------------------ #
def _f64(t):
    return t.detach().cpu().double()


def ref_gemm_bf16_exact(a, w):
    """round_to_bf16(A @ W^T), a [M, K], w [N, K]."""
    return (_f64(a) @ _f64(w).T).float().to(torch.bfloat16)


def ref_gemm_fp8_exact(a8, as_, w8, ws):
    """round_to_bf16((A @ W^T) * as[m] * ws[n]) from e4m3 bytes."""
    a = _f64(a8.detach().cpu().view(F8).float())
    w = _f64(w8.detach().cpu().view(F8).float())
    s = (a @ w.T) * _f64(as_)[:, None] * _f64(ws)[None, :]
    return s.float().to(torch.bfloat16)


def conv3x3_f64(x, w):
    """float64 3x3 stride-1 pad-1 convolution (no epilogue); pass it as
    ``conv=`` to share one convolution among several epilogues."""
    return torch.nn.functional.conv2d(_f64(x), _f64(w), None, stride=1,
                                      padding=1)


def ref_conv3x3_exact(x, w, bias=None, relu=False, residual=None, conv=None):
    """float64 conv2d + bias, + residual, relu, -> fp32 -> bf16 (NCHW
    logical shape, contiguous)."""
    y = conv3x3_f64(x, w) if conv is None else conv
    if bias is not None:
        y = y + _f64(bias)[None, :, None, None]
    if residual is not None:
        y = y + _f64(residual)
    if relu:
        y = torch.relu(y)
    return y.float().to(torch.bfloat16).contiguous()


# ------------------------------------------------------------------ #
# assertion
# ------------------------------------------------------------------ #
def _short(values, limit=24):
    values = [int(v) for v in values]
    if len(values) <= limit:
        return str(values)
    return "{} ... ({} in all)".format(values[:limit], len(values))


def assert_bit_equal(got, ref):
    """``got`` must equal ``ref`` element for element (torch.equal; a NaN
    never matches). On failure the message gives the number of differing
    elements, the first differing (row, col) and the distinct rows and
    columns hit -- the pattern that names the tile, wave or k-step at
    fault. 4-D tensors are read as NCHW: row = pixel (n*H + y)*W + x,
    col = channel."""
    assert isinstance(got, torch.Tensor) and isinstance(ref, torch.Tensor)
    assert got.dtype == ref.dtype, \
        "dtype {} != reference {}".format(got.dtype, ref.dtype)
    assert tuple(got.shape) == tuple(ref.shape), \
        "shape {} != reference {}".format(tuple(got.shape), tuple(ref.shape))
    g = got.detach().cpu()
    r = ref.detach().cpu()
    if torch.equal(g, r):
        return
    if g.dim() == 4:
        g = g.permute(0, 2, 3, 1)
        r = r.permute(0, 2, 3, 1)
    cols = g.shape[-1] if g.dim() else 1
    g2 = g.reshape(-1, cols)
    r2 = r.reshape(-1, cols)
    bad = g2 != r2                      # NaN != anything -> flagged
    idx = bad.nonzero()
    row0, col0 = int(idx[0, 0]), int(idx[0, 1])
    raise AssertionError(
        "not bit-equal: {} of {} elements differ; first at (row {}, col {}): "
        "got {!r}, reference {!r}; rows hit {}; cols hit {}".format(
            int(bad.sum()), bad.numel(), row0, col0,
            float(g2[row0, col0]), float(r2[row0, col0]),
            _short(idx[:, 0].unique()), _short(idx[:, 1].unique())))
