"""Check functions for tests/test_gpu_narrow_spmm.py: spmm_sum on the
TRANSPOSED fixture CSR of kernel_path_checks.py (the path a backward
takes; its hub column is a split row), under the same float64 any-order
summation bound, and the BNSGCN_SPMM_NARROW_MAX=0 variant.

Run as a script (`python tests/narrow_spmm_checks.py narrow_off`) it
executes that variant in a fresh process — the extension reads the switch
once per process — and exits non-zero on a mismatch.
"""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kernel_path_checks as K  # noqa: E402
from kernel_path_checks import (N_COLS, N_ROWS, assert_sum_bound, cu, dbl,  # noqa: E402
                                degrees, gen)

from bnsgcn_amd.ops import reference as ref  # noqa: E402

COMBOS = ((True, False), (False, False), (False, True), (True, True))


def transposed_fixture_csr():
    from bnsgcn_amd.ops.csr_torch import transpose_csr
    indptr, indices = K.fixture_csr()
    tip, tix, _ = transpose_csr(indptr, indices, N_COLS)
    assert degrees(tip).max() > 512       # hub column -> split row
    return tip, tix


def check_spmm_sum_transposed(F, scales, acc):
    """kernel_path_checks.check_spmm_sum on the transposed fixture: 80
    rows gathering from 96 source rows."""
    from bnsgcn_amd.ops.functional import spmm_sum_raw
    tip, tix = transposed_fixture_csr()
    g = gen(150 + F)
    x = torch.randn(N_ROWS, F, generator=g)
    ss = torch.rand(N_ROWS, generator=g) + 0.5 if scales else None
    ds = torch.rand(N_COLS, generator=g) + 0.5 if scales else None
    base = torch.randn(N_COLS, F, generator=g) if acc else None
    want = ref.spmm_sum(tip, tix, dbl(x), dbl(ss), dbl(ds),
                        dbl(base).clone() if acc else None)
    want_abs = ref.spmm_sum(tip, tix, dbl(x).abs(), dbl(ss), dbl(ds),
                            dbl(base).abs() if acc else None)
    got = spmm_sum_raw(cu(tip), cu(tix), cu(x), cu(ss), cu(ds),
                       cu(base).clone() if acc else None)
    what = f"spmm_sum transposed F={F} scales={scales} acc={acc}"
    assert_sum_bound(got, want, want_abs, degrees(tip)[:, None], what)
    if not acc:
        empty = degrees(tip) == 0
        assert (got.cpu()[empty] == 0).all(), f"{what}: empty rows not zero"


def check_all(F):
    for scales, acc in COMBOS:
        K.check_spmm_sum(F, scales, acc, nan_prefill=not acc)
        check_spmm_sum_transposed(F, scales, acc)


def _case_narrow_off():
    assert os.environ.get("BNSGCN_SPMM_NARROW_MAX") == "0"
    for F in (44, 64):
        check_all(F)


CASES = {"narrow_off": ({"BNSGCN_SPMM_NARROW_MAX": "0"}, _case_narrow_off)}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print(f"usage: {argv[0]} {{{'|'.join(CASES)}}}", file=sys.stderr)
        return 2
    if not torch.cuda.is_available():
        print("no GPU", file=sys.stderr)
        return 3
    CASES[argv[1]][1]()
    torch.cuda.synchronize()
    print(f"{argv[1]}: ok")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
