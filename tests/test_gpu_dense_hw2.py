"""gmc_dense_hw2_f32 alone against float64 (tests/blocks_ref.py: dense_ref, bound (F + 3) u |dinv| sum |H||W2|): the
MFMA kernel of csrc/dense_mfma.hip - one wave per 16 rows, four waves per workgroup, 16 columns of H per round of four
MFMA steps, a k-tail loop of 4 columns per step - at every edge of that tiling.

  rows     1, 15, 16, 17 (a second wave of one row), 63, 64, 65 (a second workgroup of one live row), 130
  F        1, 3, 4, 5 (tail only), 15, 16, 17 (one round + a tail of 1), 19, 20, 31, 32, 33, 48, 500, 4096
  ldh      F rounded up to 4, + 0 or + 4; the padding is NaN, Z0 lies between NaN rows, dinv has both signs
  exact    one asymmetric small-integer problem per F % 16 class (F = 16 .. 31) must be reproduced exactly

CASES is the designed list (tests/test_blocks_host.py runs the float32 restatement over it on the CPU).

Measured on the MI355X, worst err / bound (-s prints every call; 53 calls, the module takes 2.1 s):
  rows 0.108    widths 0.359 (F = 1: the one product's rounding and the scale's)    integer_exact: exact
"""
import numpy as np
import pytest
import torch

from tests import blocks_ref as BR
from tests.blocks_ref import dense_case as case

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 63, 64, 65, 130)
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 19, 20, 31, 32, 33, 48, 500, 4096)
CASES = {
    "rows": [case(n, F, pad) for i, n in enumerate(ROWS) for F, pad in ((17, 4 * (i % 2)), (48, 4 * ((i + 1) % 2)))],
    "widths": [case(37, F, 4 * (i % 2)) for i, F in enumerate(WIDTHS)]
              + [case(65, F, 4) for F in (1, 5, 19, 33)] + [case(130, 4096, 0), case(130, 500, 4)],
    "integer_exact": [case(37, 16 + k, 4 * (k % 2), kind="int") for k in range(16)],
}
DETERMINISM = case(65, 500, 4)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def launch(pkg, pr):
    """One call; H with its NaN padding, Z0 NaN with a NaN row either side: the Z0 buffer [(n + 2), 3]."""
    hip = pkg.hip
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    H, W2, dinv = dev(pr["H"]), dev(pr["W2"]), dev(pr["dinv"])
    Zbuf = torch.full((pr["n"] + 2, 3), float("nan"), dtype=torch.float32, device="cuda")
    rc = hip.load().gmc_dense_hw2_f32(hip.ptr(H), pr["ldh"], hip.ptr(dinv), hip.ptr(W2), Zbuf.data_ptr() + 12, pr["n"],
                                      pr["F"], hip.stream())
    hip.check(rc, "gmc_dense_hw2_f32")
    torch.cuda.synchronize()
    return Zbuf.cpu().numpy()


@pytest.mark.parametrize("group", list(CASES))
def test_against_float64(pkg, group):
    worst = 0.0
    for c in CASES[group]:
        pr = BR.dense_problem(c)
        ratio = BR.judge_dense(pr, launch(pkg, pr))
        print(f"{c['name']}: max err / bound = {ratio:.3f}")
        worst = max(worst, ratio)
    print(f"hw2 group {group}: worst {worst:.3f}")


def test_two_runs_give_equal_bytes(pkg):
    pr = BR.dense_problem(DETERMINISM)
    a, b = launch(pkg, pr), launch(pkg, pr)
    assert a.tobytes() == b.tobytes()


def test_probe_names_the_launch(pkg):
    with pkg.hip.Probe(4) as p:
        launch(pkg, BR.dense_problem(case(8, 8)))
    assert [t for t, _ms in p.records] == ["dense_mfma"]
