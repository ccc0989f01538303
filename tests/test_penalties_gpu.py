"""GPU: ops.apply_penalties against float64 numpy in the documented order:
touched elements within one ulp, the rest bit-identical, bans at -inf."""

import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))
import penalty_cases as pen  # noqa: E402


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", pen.DTYPES, ids=pen.DTYPE_IDS)
@pytest.mark.parametrize("rows,vocab", [(5, 257), (3, 4099)])
def test_apply_penalties(rows, vocab, dtype):
    pen.run_case(rows, vocab, dtype, "cuda:0")
