"""The step checker judged on the CPU (tests/stepcheck.py): on a small batch the reference itself, rounded to float32,
is the step that "ran" - it must pass, and every wrong answer made from it (a probability, a gradient row or entry, a
NaN, the tail slot, a loss one ulp off, a partition flipped at a clear or at a near-tie row, gradient columns off the
bar with and without a relu kink to excuse them) must fail, for both reference builders."""
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import ref_dense as R
from tests import stepcheck as SC

N, F = 40, 16
F64_RULES = dict(p_tol=SC.P_TOL, grad_bar=SC.ORACLE_BAR, row_tol=SC.ROW_TOL, row_floor=SC.ROW_FLOOR)
KINDS = {   # reference builder, the bars its GPU tests pass, which restatement finds the kink columns
    "f64_dense": (SC.f64_step, F64_RULES, False),
    "f64_sparse": (lambda *a, **k: SC.f64_step(*a, sparse=True, **k), F64_RULES, True),
    "oracle": (SC.oracle_step, dict(p_tol=SC.PROB_TOL, grad_bar=SC.ORACLE_BAR), False),
}


@pytest.fixture(scope="module")
def problem():
    """Three graphs (the second with integer weights 1..3), hidden 16, and the float64 partition of each."""
    rng = np.random.RandomState(3)
    params = {"conv1.weight": rng.standard_normal((N, F)) * 0.5, "conv1.bias": rng.standard_normal(F) * 0.1,
              "conv2.weight": rng.standard_normal((F, 3)) * 0.5, "conv2.bias": rng.standard_normal(3) * 0.1}
    params = {k: v.astype(np.float32) for k, v in params.items()}
    graphs = [R.regular_graph(30, 5, 1), R.regular_graph(24, 4, 2), R.regular_graph(12, 3, 3)]
    for u, v in graphs[1].edges():
        graphs[1][u][v]["weight"] = int(rng.randint(1, 4))
    csrs = [CO.csr_of(g) for g in graphs]
    W = [params[k] for k in SC.KEYS]
    fwd = [SC.f64_forward(rp, cl, vl, *W) for rp, cl, vl in csrs]
    return csrs, params, np.concatenate([SC.f64_partition(f["P"]) for f in fwd]), fwd


def as_step(ref, S):
    """The reference as the device would hand it back: float32, the loss sum in the tail slot."""
    return SC.Step(ref.P.astype(np.float32), S.copy(), ref.loss.copy(), {k: g.astype(np.float32) for k, g in ref.grads.items()},
                   float(ref.loss.sum()), [], [])


def judge(kind, problem, got, tie=1e-6, **over):
    csrs, params, _S, _fwd = problem
    build, rules, sparse = KINDS[kind]
    ref = build(csrs, params, got.S, tie=tie)
    return SC.compare_step(got, ref, csrs=csrs, params=params, sparse=sparse, **{**rules, **over})


def reference(kind, problem, S=None, tie=1e-6):
    csrs, params, S0, _fwd = problem
    return KINDS[kind][0](csrs, params, S0 if S is None else S, tie=tie)


def fails(kind, problem, got, **kw):
    with pytest.raises(AssertionError):
        judge(kind, problem, got, **kw)


def moved(got, key, index, by):
    grads = {k: g.copy() for k, g in got.grads.items()}
    grads[key][index] += by
    return got._replace(grads=grads)


@pytest.mark.parametrize("kind", KINDS)
def test_the_reference_itself_passes(problem, kind):
    ref = reference(kind, problem)
    assert ref.near_ties == 0 and ref.loss.dtype == np.float32 and ref.P.shape == (66, 3)
    assert [ref.grads[k].shape for k in SC.KEYS] == [(N, F), (F,), (F, 3), (3,)]
    assert not ref.grads["conv1.weight"][30:].any() and np.abs(ref.grads["conv1.weight"]).max() > 0.1
    res = judge(kind, problem, as_step(ref, problem[2]))
    assert res["near_ties"] == 0 and res["bad_cols"] == [] and res["kink_cols"] is None
    assert res["p_err"] < 1e-7 and res["rows"] < 1e-6


def test_the_two_references_agree(problem):
    a, b = reference("f64_dense", problem), reference("oracle", problem)
    assert np.abs(a.P - b.P).max() < 1e-6 and np.array_equal(a.loss, b.loss)
    for k in SC.KEYS:
        assert np.abs(a.grads[k] - b.grads[k]).max() <= 1e-5 * np.abs(a.grads[k]).max(), k


@pytest.mark.parametrize("kind", KINDS)
def test_a_probability_off_by_more_than_p_tol_fails(problem, kind):
    got = as_step(reference(kind, problem), problem[2])
    p_tol = KINDS[kind][1]["p_tol"]
    for factor, ok in ((0.5, True), (2.0, False), (-2.0, False)):
        P = got.P.copy()
        P[17, 1] += np.float32(factor * p_tol)
        if ok:
            assert abs(judge(kind, problem, got._replace(P=P))["p_err"] - 0.5 * p_tol) < 0.2 * p_tol
        else:
            fails(kind, problem, got._replace(P=P))


@pytest.mark.parametrize("kind", KINDS)
def test_a_gradient_entry_past_the_bar_fails(problem, kind):
    ref = reference(kind, problem)
    got = as_step(ref, problem[2])
    for key, index in (("conv1.weight", (3, 5)), ("conv1.weight", (35, 0)), ("conv1.bias", 2), ("conv2.weight", (7, 1)),
                       ("conv2.bias", 0)):
        bar = SC.ORACLE_BAR * max(1.0, float(np.abs(ref.grads[key]).max()))
        judge(kind, problem, moved(got, key, index, 0.5 * bar), row_tol=None)
        fails(kind, problem, moved(got, key, index, 2.0 * bar), row_tol=None)
        fails(kind, problem, moved(got, key, index, -2.0 * bar), row_tol=None)


@pytest.mark.parametrize("kind", ["f64_dense", "f64_sparse"])
def test_a_gradient_row_past_row_tol_fails_inside_the_bar(problem, kind):
    ref = reference(kind, problem)
    got = as_step(ref, problem[2])
    for key in ("conv1.weight", "conv2.weight", "conv1.bias"):
        r = ref.grads[key]
        scale = SC.row_scale(r, SC.ROW_FLOOR)
        j = int(np.argmin(np.where(scale > SC.ROW_FLOOR * np.abs(r).max(), scale, np.inf)))     # the smallest live row
        index = (j, 0) if r.ndim == 2 else j
        step = 1.5 * SC.ROW_TOL * scale[j]
        assert step < 0.5 * SC.ORACLE_BAR * max(1.0, np.abs(r).max())             # the bar alone would let it through
        judge(kind, problem, moved(got, key, index, step), row_tol=None)
        fails(kind, problem, moved(got, key, index, step))
        res = judge(kind, problem, moved(got, key, index, 0.5 * SC.ROW_TOL * scale[j]))
        assert 0.4 * SC.ROW_TOL < res["rows"] < 0.6 * SC.ROW_TOL
    # a row that is zero in the reference (past every graph's n) is held to row_floor of the tensor
    top = np.abs(ref.grads["conv1.weight"]).max()
    fails(kind, problem, moved(got, "conv1.weight", (38, 4), 1.5 * SC.ROW_TOL * SC.ROW_FLOOR * top))
    judge(kind, problem, moved(got, "conv1.weight", (38, 4), 0.5 * SC.ROW_TOL * SC.ROW_FLOOR * top))


@pytest.mark.parametrize("kind", KINDS)
def test_nan_tail_and_loss_are_checked(problem, kind):
    got = as_step(reference(kind, problem), problem[2])
    for key, index in (("conv1.weight", (39, 15)), ("conv1.bias", 0), ("conv2.weight", (0, 2)), ("conv2.bias", 1)):
        fails(kind, problem, moved(got, key, index, float("nan")))
    fails(kind, problem, got._replace(tail=got.tail + 1.0))
    fails(kind, problem, got._replace(tail=float("nan")))
    judge(kind, problem, got._replace(tail=None))                 # an entry without a gradient buffer has no tail
    for g in range(3):
        for towards in (-np.inf, np.inf):
            loss = got.loss.copy()
            loss[g] = np.nextafter(loss[g], np.float32(towards))
            fails(kind, problem, got._replace(loss=loss, tail=float(loss.sum())))
    fails(kind, problem, got._replace(loss=got.loss.astype(np.float64)))


@pytest.mark.parametrize("kind", KINDS)
def test_a_partition_may_differ_only_at_a_near_tie(problem, kind):
    csrs, params, S0, fwd = problem
    srt = np.sort(fwd[0]["P"], axis=1)
    margin = srt[:, 2] - srt[:, 1]
    margin[:3] = np.inf                                           # terminals are overridden, not decoded
    row, clear = int(np.argmin(margin)), int(np.argmax(np.where(np.isfinite(margin), margin, 0.0)))
    tie = 0.5 * (margin[row] + np.sort(margin)[1])                # this row qualifies, no other does
    assert margin[row] > 1e-4 and np.sort(margin)[1] > 1.1 * margin[row] and margin[clear] > 0.1
    second = lambda r: int(np.argsort(fwd[0]["P"][r])[1])
    original = as_step(reference(kind, problem), S0)
    # a clear-margin row decoded differently: refused under every tie the tests use, and under this one
    S = S0.copy()
    S[clear] = second(clear)
    fails(kind, problem, original._replace(S=S))
    fails(kind, problem, as_step(reference(kind, problem, S0), S), tie=tie)
    # the near-tie row: refused at the default threshold; with `tie` above its margin accepted - but only with the loss
    # and the gradient of the partition that was chosen
    S = S0.copy()
    S[row] = second(row)
    with pytest.raises(AssertionError):
        reference(kind, problem, S)
    flipped = reference(kind, problem, S, tie=tie)
    assert flipped.near_ties == 1
    assert judge(kind, problem, as_step(flipped, S), tie=tie)["near_ties"] == 1
    fails(kind, problem, original._replace(S=S), tie=tie)                                  # the other partition's loss and gradient
    fails(kind, problem, as_step(flipped, S)._replace(grads=original.grads), tie=tie)      # ... its gradient alone
    assert not np.array_equal(flipped.loss, original.loss)
    fails(kind, problem, as_step(flipped, S)._replace(loss=original.loss, tail=original.tail), tie=tie)


@pytest.mark.parametrize("kind", KINDS)
def test_columns_off_the_bar_need_a_relu_kink(problem, kind):
    csrs, params, S0, fwd = problem
    ref = reference(kind, problem)
    got = as_step(ref, S0)
    nearest = np.min([np.abs(f["pre"]).min(0) for f in fwd], axis=0)          # per column: how close a pre-activation comes to 0
    f1, f2, *_rest, far = np.argsort(nearest)
    noise = 0.5 * (nearest[f2] + np.sort(nearest)[2])                         # f1 and f2 qualify, no other column does
    assert np.array_equal(np.nonzero(SC.kink_columns(csrs, params, noise))[0], sorted((f1, f2)))
    assert np.array_equal(SC.kink_columns(csrs, params, noise), SC.kink_columns(csrs, params, noise, sparse=True))
    off = 3.0 * SC.ORACLE_BAR * max(1.0, float(np.abs(ref.grads["conv1.weight"]).max()))
    one = moved(moved(got, "conv1.weight", (4, f1), off), "conv1.bias", f1, off)
    fails(kind, problem, one)
    fails(kind, problem, one, kinks=(0.5 * nearest[f1], 2))                  # (no column is a kink at that noise)
    res = judge(kind, problem, one, kinks=(noise, 1))
    assert res["bad_cols"] == [f1] and res["kink_cols"] == 2
    two = moved(one, "conv1.weight", (9, f2), -off)
    assert judge(kind, problem, two, kinks=(noise, 2))["bad_cols"] == sorted((f1, f2))
    fails(kind, problem, two, kinks=(noise, 1))                              # more columns off than max_cols
    fails(kind, problem, moved(one, "conv1.bias", f2, off), kinks=(noise, 1))   # a db1 entry counts as its column
    fails(kind, problem, moved(one, "conv1.weight", (4, far), off), kinks=(noise, 3))   # an off column that is no kink
    fails(kind, problem, moved(got, "conv1.bias", far, off), kinks=(noise, 3))
    off2 = 3.0 * SC.ORACLE_BAR * max(1.0, float(np.abs(ref.grads["conv2.weight"]).max()))
    fails(kind, problem, moved(one, "conv2.weight", (f1, 0), off2), kinks=(noise, 3))   # dW2 / db2 get no exception
    fails(kind, problem, moved(one, "conv1.weight", (4, f1), float("nan")), kinks=(noise, 3))
    fails(kind, problem, moved(one, "conv1.weight", (6, f1), float("nan")), kinks=(noise, 3))   # a NaN is no kink
    assert judge(kind, problem, got, kinks=(noise, 0))["kink_cols"] is None     # nothing off: the rule is not consulted
