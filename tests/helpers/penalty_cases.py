"""One apply_penalties case, run on a device and checked against float64
numpy in the documented operation order."""

import numpy as np
import torch

import clearml_serving_amd.ops as ops

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]
MANT = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}


def run_case(rows, vocab, dtype, device):
    """Row 1 has no entry; the others hold tokens 0, V-1, two out of range
    and up to 40 random unique ones, a third prompt-only, some banned."""
    g = torch.Generator().manual_seed(rows * 131 + vocab)
    logits = (torch.randn(rows, vocab, generator=g) * 3).to(dtype)
    floats = [torch.linspace(-1.5, 2.0, rows), torch.linspace(0.3, -0.2, rows),
              torch.linspace(0.8, 1.7, rows)]
    pres, freq, rep = (f.double().numpy() for f in floats)
    want = logits.double().numpy().copy()
    touched = np.zeros((rows, vocab), dtype=bool)
    scale = np.abs(want)   # largest magnitude an element passes through
    tok, cnt, flags, offsets = [], [], [], [0]
    for r in range(rows):
        if r != 1:
            mid = torch.randperm(vocab - 2, generator=g)[:40] + 1
            t = np.array([0, vocab - 1, vocab + 5 * r, -1 - r] + mid.tolist())
            c = (np.arange(len(t)) * 7 + r) % 3
            f = (np.arange(len(t)) % 11 == 1).astype(int)
            tok, cnt, flags = tok + t.tolist(), cnt + c.tolist(), \
                flags + f.tolist()
            t, c, f = (v[(t >= 0) & (t < vocab)] for v in (t, c, f))
            x = want[r, t]
            x = np.where(x > 0, x / rep[r], x * rep[r])
            y = x - freq[r] * c
            z = y - pres[r] * (c > 0)
            scale[r, t] = np.maximum.reduce([abs(x), abs(y), abs(z)]) + 1e-30
            want[r, t] = np.where(f == 1, -np.inf, z)
            touched[r, t] = True
        offsets.append(len(tok))
    ints = [torch.tensor(v, dtype=torch.int32)
            for v in (tok, cnt, flags, offsets)]
    src = logits.to(device)
    out = ops.apply_penalties(
        src, *[v.to(device) for v in ints + floats]).cpu()
    raw = torch.int16 if dtype != torch.float32 else torch.int32
    assert torch.equal(src.cpu().view(raw), logits.view(raw))  # not written
    assert out.dtype == dtype and out.shape == logits.shape
    assert (out.view(raw) == logits.view(raw)).numpy()[~touched].all()
    got, exp = out.double().numpy()[touched], want[touched]
    banned = np.isinf(exp)
    assert banned.any() and (got[banned] == -np.inf).all()
    # one ulp of the output dtype at the expected value. fp32 alone takes
    # the ulp at the largest magnitude the element passes through: there the
    # fp32 rounding of the division is as large as the output ulp, and a
    # cancelling subtraction carries it into a smaller result.
    at = scale[touched] if dtype == torch.float32 else np.abs(exp)
    ulp = 2.0 ** (np.floor(np.log2(at[~banned])) - MANT[dtype] + 1)
    assert (np.abs(got[~banned] - exp[~banned]) <= ulp).all()
