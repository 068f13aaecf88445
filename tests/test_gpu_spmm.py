"""gmc_spmm_f32 alone against float64 (tests/blocks_ref.py: spmm_ref and its derived bounds): the three kernels of
csrc/spmm.hip (spmm_rows_v4 at 1, 2 and 4 passes, spmm_rows_wide, spmm_rows_scalar) at their edges - rows of 0 .. 200
entries around the 64-entry chunk, both rows of a wave long / a long row beside an empty one, odd row counts, F either
side of every launch class, every way into the scalar kernel, the W2 epilogue, each option off in turn, and the XCD
remap of the workgroup index (group_rows).

CSR built in numpy: rectangular, sorted rows, real signed weights with exact zeros.  Source row 0 is referenced by no
entry and holds NaN (the kernels' idle lanes point at it); X's leading-dimension padding is NaN; Y and Z0 are NaN with
a NaN row either side and NaN padding: a row never written stays NaN, a write past the edge shows in the band.

CASES is the designed list (tests/test_blocks_host.py runs the float32 restatement over the same list on the CPU).

Measured on the MI355X, worst err / bound per group (-s prints every call; 75 calls, the module takes 2.6 s):
  row_lengths Y 0.347    row_counts Y 0.337    f_classes Y 0.414    scalar Y 0.359
  epilogue    Y 0.356, Z0 0.106    options Y 0.459, Z0 0.001    group_rows Y 0.422, Z0 0.003
Y's ratios are those of the sequential float32 restatement (the kernels add in CSR order); Z0 sums in another order.
"""
import numpy as np
import pytest
import torch

from tests import blocks_ref as BR
from tests.blocks_ref import spmm_case as case

pytestmark = pytest.mark.gpu

UNSUPPORTED = -7
# 17 rows, 2 per wave and 8 per workgroup: both rows of a wave long (200, 129), a long row beside an empty one
# (128 | 0, 0 | 127), the 64-entry chunk edge either way round (65, 64 | 64, 65), short rows around the unroll of 8,
# and a last wave of one row with a second chunk of one entry
ROWLENS = [200, 129, 128, 0, 0, 127, 65, 64, 63, 9, 8, 7, 1, 0, 64, 65, 129]
SHORT = [9, 65, 0, 7, 130, 1, 8, 64, 3]              # 9 rows: two workgroups, the last wave has one row


def pattern(n):
    return [(3, 70, 0, 9, 64, 1, 129, 8)[i % 8] for i in range(n)]


def light(n):
    return [(i * 7 + 3) % 6 for i in range(n)]        # 0 .. 5 entries per row


def both(name, rows, F, **kw):
    return [case(f"{name} val", rows, F, vals=True, **kw), case(f"{name} unit", rows, F, vals=False, **kw)]


CASES = {
    "row_lengths": [c for F in (4, 260, 1028) for c in both(f"lengths F{F}", ROWLENS, F)],
    "row_counts": [c for n in (1, 7, 8, 9, 17) for c in both(f"count {n}", pattern(n), 260)],
    "f_classes": [c for F in (4, 252, 256, 260, 508, 512, 516, 1020, 1024, 1028, 2052, 4096)
                  for c in both(f"class F{F}", SHORT, F)],
    "scalar": [case(f"scalar F{F}", SHORT, F, ldx=F, ldy=F, vals=F % 2 == 0) for F in (1, 6, 63, 64, 65, 130)]
              + both("scalar X off 4 bytes", SHORT, 64, xoff=1)
              + both("scalar ldx 66", SHORT, 64, ldx=66)
              + both("scalar F4100", SHORT, 4100),
    "epilogue": [c for F in (4, 260, 1024, 1028, 4096) for c in both(f"epi F{F}", SHORT, F, epi=True)],
    "options": [case("no scale", SHORT, 260, scale=False), case("no bias", SHORT, 260, bias=False),
                case("no relu", SHORT, 260, relu=0), case("no relu unit", SHORT, 260, relu=0, vals=False),
                case("bare epi", SHORT, 260, scale=False, bias=False, relu=0, epi=True),
                case("no scale epi", SHORT, 516, scale=False, epi=True),
                case("wide no scale no bias", SHORT, 1028, scale=False, bias=False, epi=True),
                case("wide no relu", SHORT, 1028, relu=0, vals=False)],
    # 424 rows = 53 workgroups; group_rows 24 = 3 workgroups: one full remap round of 8 * 3 * 2 = 48, a remainder of 5
    "group_rows": [case("group 24 of 424", light(424), 260, group_rows=24, epi=True),
                   case("group 24 of 424 unit", light(424), 8, group_rows=24, vals=False),
                   case("group 24 of 424 wide", light(424), 1028, group_rows=24, vals=False),
                   case("group 1000 of 3000", light(3000), 12, group_rows=1000),
                   case("group past n_rows", pattern(17), 260, group_rows=5000)],
}
REFUSED = [case("scalar X off 4 bytes epi", SHORT, 64, xoff=1, epi=True),
           case("scalar ldx 66 epi", SHORT, 64, ldx=66, epi=True),
           case("scalar F4100 epi", SHORT, 4100, epi=True)]
DETERMINISM = case("129 entries F516 epi", [129, 3, 129], 516, epi=True)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def launch(pkg, pr):
    """One call on NaN-filled, NaN-banded buffers: (rc, Y buffer [(n + 2), ldy], Z0 buffer [(n + 2), 3] or None)."""
    hip = pkg.hip
    c, n, ldx, ldy = pr["case"], pr["n"], pr["ldx"], pr["ldy"]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = {k: dev(pr[k]) for k in ("rowptr", "col", "vals", "scale", "bias", "W2")}
    Xbuf = torch.full((pr["X"].size + 4,), float("nan"), dtype=torch.float32, device="cuda")
    Xbuf[c["xoff"]:c["xoff"] + pr["X"].size] = torch.from_numpy(pr["X"].ravel())
    Ybuf = torch.full((n + 2, ldy), float("nan"), dtype=torch.float32, device="cuda")
    Zbuf = torch.full((n + 2, 3), float("nan"), dtype=torch.float32, device="cuda") if c["epi"] else None
    p = hip.ptr
    rc = hip.load().gmc_spmm_f32(p(t["rowptr"]), p(t["col"]), p(t["vals"]), p(t["scale"]), Xbuf.data_ptr() + 4 * c["xoff"],
                                 ldx, p(t["bias"]), int(pr["relu"]), Ybuf.data_ptr() + 4 * ldy, ldy, n, pr["F"],
                                 c["group_rows"], p(t["W2"]), None if Zbuf is None else Zbuf.data_ptr() + 12,
                                 hip.stream())
    torch.cuda.synchronize()
    return rc, Ybuf.cpu().numpy(), None if Zbuf is None else Zbuf.cpu().numpy()


def check(pkg, c):
    pr = BR.spmm_problem(c)
    rc, Yw, Zw = launch(pkg, pr)
    pkg.hip.check(rc, "gmc_spmm_f32")
    worst = BR.judge_spmm(pr, Yw, Zw)
    print(f"spmm {c['name']}: max err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("group", list(CASES))
def test_against_float64(pkg, group):
    worst = {}
    for c in CASES[group]:
        for k, v in check(pkg, c).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"spmm group {group}: worst " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("c", REFUSED, ids=[c["name"] for c in REFUSED])
def test_scalar_shapes_with_w2_are_refused_and_write_nothing(pkg, c):
    rc, Yw, Zw = launch(pkg, BR.spmm_problem(c))
    assert rc == UNSUPPORTED
    assert np.isnan(Yw).all() and np.isnan(Zw).all()


def test_no_rows_writes_nothing(pkg):
    rc, Yw, Zw = launch(pkg, BR.spmm_problem(case("no rows", [], 260, epi=True)))
    assert rc == 0
    assert np.isnan(Yw).all() and np.isnan(Zw).all()


def test_two_runs_give_equal_bytes(pkg):
    pr = BR.spmm_problem(DETERMINISM)
    a, b = launch(pkg, pr), launch(pkg, pr)
    BR.judge_spmm(pr, a[1], a[2])
    assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_probe_names_the_launch(pkg):
    with pkg.hip.Probe(4) as p:
        launch(pkg, BR.spmm_problem(case("probe", SHORT, 8)))
    assert [t for t, _ms in p.records] == ["spmm_user"]
