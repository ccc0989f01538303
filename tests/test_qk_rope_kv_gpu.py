"""ops.qk_rope_kv on gfx950 (qk_rope_kv.hip) against a float64 reference: the
angle is the fp32 product float(pos) * inv_freq[i] (part of the op's
contract) lifted to float64, everything else is float64, no rounding.

q, k and the K cache: |got - ref| <= 2^-8 |ref| + 2^-16 max|row|. One bf16
rounding is 2^-9 relative, the bound allows twice that; the floor covers fp32
arithmetic where lo*c - hi*s cancels. fp8 caches: the scale is
2^ceil(log2(amax / 448)) of the kernel's own rounded row and |dequant - row|
<= 2^-4 |row| + scale * 2^-10, e4m3's half-ulp for normals and subnormals.
"""

import pytest
import torch

import clearml_serving_amd.ops as ops
from clearml_serving_amd.models.rope_scaling import rope_inv_freq

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS, NB = 16, 3  # page size, pages
POSITIONS = {1: [100000], 5: [0, 1, 100000, 31, 4097]}
SLOTS = {1: [17], 5: [14, 15, 16, -1, 40]}  # crosses a page; one skipped
FILL = {"bf16": -7.0, "fp8": 0xAB}  # sentinels; fp8 scales hold -1


def reference(x, w, pos, inv_freq, attn, eps):
    x = x.double()
    if w is not None:
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    angle = (pos.float()[:, None] * inv_freq[None, :]).double()[:, None, :]
    c, s = angle.cos() * attn, angle.sin() * attn
    lo, hi = x.chunk(2, dim=-1)
    return torch.cat([lo * c - hi * s, hi * c + lo * s], dim=-1)


def check_rows(got, ref):
    got = got.double().cpu()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -16 * ref.abs().amax(-1, keepdim=True)
    assert torch.isfinite(got).all() and ((got - ref).abs() <= bound).all()


def check_fp8(cache, scale, row):  # one slot: u8 [H, D], [H], [H, D]
    row, scale = row.double(), scale.double()
    want = torch.exp2(torch.ceil(torch.log2(row.abs().amax(-1) / 448.0)))
    assert torch.equal(scale, want)
    deq = cache.view(torch.float8_e4m3fn).double() * scale[:, None]
    bound = 2.0 ** -4 * row.abs() + scale[:, None] * 2.0 ** -10
    assert ((deq - row).abs() <= bound).all()


def run_case(t, hq, hkv, d, norm, kv, dtype=torch.bfloat16, attn=1.0,
             scaling=None):
    g = torch.Generator().manual_seed(t * 1000 + hq * 100 + d + norm)
    inv_freq, _ = rope_inv_freq(d, 10000.0, scaling, 4096)
    sizes = [hq * d, hkv * d, hkv * d]
    merged = (torch.randn(t, sum(sizes), generator=g) * 2).to(dtype)
    qw = kw = None
    if norm:
        qw = (torch.rand(d, generator=g) + 0.5).to(dtype)
        kw = (torch.rand(d, generator=g) + 0.5).to(dtype)
    pos = torch.tensor(POSITIONS[t], dtype=torch.int32)
    q0, k0, v0 = (x.unflatten(-1, (-1, d)) for x in merged.split(sizes, -1))
    q_ref = reference(q0, qw, pos, inv_freq, attn, 1e-6)
    k_ref = reference(k0, kw, pos, inv_freq, attn, 1e-6)

    # q/k/v stay token-strided views of the merged buffer
    q, k, v = (x.unflatten(-1, (-1, d))
               for x in merged.to(DEV).split(sizes, -1))
    cache, fp8 = {}, kv == "fp8"
    if kv:
        for name in ("k_cache", "v_cache"):
            cache[name] = torch.full(
                (NB, hkv, BS, d), FILL[kv], device=DEV,
                dtype=torch.uint8 if fp8 else dtype)
        if fp8:
            cache["k_scale"] = torch.full((NB, hkv, BS), -1.0, device=DEV)
            cache["v_scale"] = cache["k_scale"].clone()
        cache["slot_mapping"] = torch.tensor(SLOTS[t], dtype=torch.int32,
                                             device=DEV)
    ops.qk_rope_kv(q, k, v, pos.to(DEV), inv_freq.to(DEV), attn,
                   None if qw is None else qw.to(DEV),
                   None if kw is None else kw.to(DEV), 1e-6, **cache)

    check_rows(q, q_ref)
    check_rows(k, k_ref)
    assert torch.equal(v.cpu(), v0)  # v is read only
    if not kv:
        return
    # [NB, BS, H, ...] host copies: one row per slot
    host = {n: c.cpu().transpose(1, 2) for n, c in cache.items()
            if n != "slot_mapping"}
    used = torch.zeros(NB, BS, dtype=torch.bool)
    for i, s in enumerate(SLOTS[t]):
        if s < 0:
            continue
        at = (s // BS, s % BS)
        used[at] = True
        for c, row in (("k", k.cpu()[i]), ("v", v0[i])):
            if fp8:
                check_fp8(host[c + "_cache"][at], host[c + "_scale"][at], row)
            else:  # bit for bit: the in-place k row, the v row
                assert torch.equal(host[c + "_cache"][at], row)
    # the -1 row and every other slot keep the sentinel
    for name, c in host.items():
        assert (c[~used] == (-1.0 if "scale" in name else FILL[kv])).all()


@pytest.mark.parametrize("kv", [None, "bf16", "fp8"])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("hq,hkv", [(4, 2), (5, 1)])
@pytest.mark.parametrize("t", [1, 5])
def test_qk_rope_kv(t, hq, hkv, d, norm, kv):
    run_case(t, hq, hkv, d, norm, kv)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_qk_rope_kv_fp16(kv):
    run_case(5, 5, 1, 128, True, kv, dtype=torch.float16)


def test_qk_rope_kv_attn_factor_and_scaled_table():
    yarn = {"rope_type": "yarn", "factor": 4.0,
            "original_max_position_embeddings": 1024}
    attn = rope_inv_freq(128, 10000.0, yarn, 4096)[1]  # 0.1 ln 4 + 1
    run_case(5, 4, 2, 128, True, "bf16", attn=attn, scaling=yarn)
