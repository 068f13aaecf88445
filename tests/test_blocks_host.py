"""The building blocks' checker checked (CPU only): tests/blocks_ref.py holds the float64 references, the derived
bounds and a float32 restatement of each operation; the GPU modules test_gpu_spmm / test_gpu_dense_hw2 / test_gpu_adam
judge the kernels with it.  Here:

1. each float32 restatement stays within its bound over the GPU modules' own case lists (-s prints the worst ratios);
2. wrong answers - the faults such kernels have: a dropped or doubled chunk entry, swapped weights, the epilogue in
   another order, a shifted column, a write into padding, a dropped k-tail, a repeated row tile, permuted W2 columns,
   a step number one off, eps inside the root, float32 bias corrections, a tail element updated twice or never, a
   non-zero slab pad column - are every one rejected;
3. the documented refusals of every entry point, with fake pointers that are never dereferenced: expectations follow
   include/gcnmaxcut.h and the order of the checks in the sources.  No call here reaches a launch.
"""
import numpy as np
import pytest

from tests import blocks_ref as BR
from tests import test_gpu_adam as ga
from tests import test_gpu_dense_hw2 as gd
from tests import test_gpu_spmm as gs
from tests import util
from tests.blocks_ref import Rejected

H = BR.HYPER


# ---- 1. the restatements stay within the bounds ---------------------------------------------------------------------
@pytest.mark.parametrize("group", list(gs.CASES))
def test_spmm_restatement_within_bounds(group):
    worst = {}
    for c in gs.CASES[group] + ([gs.DETERMINISM] if group == "epilogue" else []):
        pr = BR.spmm_problem(c)
        for k, v in BR.judge_spmm(pr, *BR.spmm_wholes(pr, *BR.spmm_f32(pr))).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"spmm restatement, {group}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert worst["Y"] <= 1.0


def test_spmm_case_list_covers_what_it_claims():
    calls = [c for g in gs.CASES.values() for c in g]
    assert 55 <= len(calls) <= 90 and len({c["name"] for c in calls}) == len(calls)
    lens = set(gs.ROWLENS)
    assert lens >= {0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200} and len(gs.ROWLENS) % 2 == 1
    assert {c["F"] for c in calls} >= {1, 4, 6, 63, 64, 65, 130, 252, 256, 260, 508, 512, 516, 1020, 1024, 1028, 2052,
                                       4096, 4100}
    assert {c["group_rows"] for c in calls} >= {0, 24, 1000, 5000}
    for key in ("vals", "scale", "bias", "relu", "epi"):
        assert {bool(c[key]) for c in calls} == {False, True}, key
    for pr in (BR.spmm_problem(c) for c in gs.CASES["row_lengths"][:2] + gs.CASES["group_rows"][:1]):
        assert pr["n_src"] > pr["n"] and np.isnan(pr["X"][0]).all() and np.isnan(pr["X"][:, pr["F"]:]).all()
        assert pr["col"].min() >= 1 and pr["col"].max() < pr["n_src"]
        assert all(np.all(np.diff(pr["col"][a:b]) > 0) for a, b in zip(pr["rowptr"][:-1], pr["rowptr"][1:]))
        if pr["vals"] is not None:
            assert (pr["vals"] == 0).any() and (pr["vals"] < 0).any() and (pr["vals"] > 0).any()


@pytest.mark.parametrize("group", list(gd.CASES))
def test_dense_restatement_within_bounds(group):
    worst = 0.0
    for c in gd.CASES[group]:
        pr = BR.dense_problem(c)
        worst = max(worst, BR.judge_dense(pr, BR.embed(BR.dense_f32(pr), 3)[0]))
    print(f"H@W2 restatement, {group}: worst err / bound {worst:.3f}")


def test_dense_case_list_covers_what_it_claims():
    calls = [c for g in gd.CASES.values() for c in g]
    assert {c["n"] for c in calls} >= set(gd.ROWS) and {c["F"] for c in calls} >= set(gd.WIDTHS)
    assert {c["F"] % 16 for c in gd.CASES["integer_exact"]} == set(range(16))
    assert {c["pad"] for c in calls} == {0, 4}
    pr = BR.dense_problem(gd.CASES["widths"][1])
    assert np.isnan(pr["H"][:, pr["F"]:]).all() and (pr["dinv"] < 0).any() and (pr["dinv"] > 0).any()


@pytest.mark.parametrize("count,step", [(c, 2) for c in ga.COUNTS] + [(200003, t) for t in (1, 2, 3, 10, 1000, 100000)])
def test_adam_restatement_within_bounds(count, step):
    st = BR.adam_problem(count, None if step == 2 else f"sweep {step}")
    worst = BR.judge_adam(BR.adam_ref(st, step, **H), *BR.adam_wholes(BR.adam_f32(st, step, **H), st["g"]), (count, step))
    print(f"adam restatement count {count} step {step}: worst err / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    # with numpy's correctly rounded root and division the update's share is 10u of the 16u: p stays clear of 1
    assert worst["p"] < 1.0 and worst["m"] < 1.0 and worst["v"] < 1.0


def test_adam_problem_has_the_state_it_claims():
    st = BR.adam_problem(1027)
    p, g, m, v = (st[k] for k in "pgmv")
    assert (p == 0).sum() >= 1027 // 3 and ((np.abs(p) > 0) & (np.abs(p) < 1e-2)).sum() > 300 and (np.abs(p) > 0.1).any()
    assert (g == 0).sum() >= 250 and np.abs(g).max() > 100 and np.abs(g[g != 0]).min() < 1e-5
    assert ((m == 0) & (v == 0)).sum() >= 250 and (v >= 0).all() and (v > 0).sum() > 500
    for count in (1, 2, 3):
        assert BR.adam_problem(count)["p"].size == count


@pytest.mark.parametrize("N,F", sorted(set(ga.SLABS + ga.MODELS)))
def test_slab_restatement_is_the_documented_layout(N, F):
    W1 = np.random.RandomState(N * F).standard_normal((N, F)).astype(np.float32)
    flat = BR.slab_f32(W1)
    assert flat.size == BR.slab_floats(N, F)
    assert np.array_equal(flat.reshape(-1, N, 16), util._slab_of(W1))
    BR.judge_slab(W1, BR.banded(flat)[0])


# ---- 2. wrong answers are caught -------------------------------------------------------------------------------------
LONG = 6                                  # the row of gs.ROWLENS with 65 entries


@pytest.fixture(scope="module")
def spmm_problem():
    assert gs.ROWLENS[LONG] == 65
    pr = BR.spmm_problem(BR.spmm_case("wrong answers", gs.ROWLENS, 12, epi=True))
    b = pr["rowptr"][LONG]
    pr["vals"][b + 62:b + 65] = [1.5, -0.75, 1.25]             # the entries the faults below touch are not zeros
    return pr


def with_csr(pr, fn):
    """The problem with row LONG's entries rewritten by fn(cols, vals) -> (cols, vals)."""
    b, e = pr["rowptr"][LONG], pr["rowptr"][LONG + 1]
    col, val = fn(pr["col"][b:e].copy(), pr["vals"][b:e].copy())
    rp = pr["rowptr"].copy()
    rp[LONG + 1:] += col.size - (e - b)
    return {**pr, "rowptr": rp, "col": np.concatenate([pr["col"][:b], col, pr["col"][e:]]),
            "vals": np.concatenate([pr["vals"][:b], val, pr["vals"][e:]])}


def shifted(Y, Z):
    Y = Y.copy()
    Y[:, 3] = Y[:, 7]
    return Y, Z


SPMM_WRONG = {
    "last entry of the 65-entry row dropped": lambda pr: BR.spmm_f32(with_csr(pr, lambda c, v: (c[:-1], v[:-1]))),
    "entry 64 counted twice": lambda pr: BR.spmm_f32(with_csr(pr, lambda c, v: (np.append(c, c[64]), np.append(v, v[64])))),
    "weights of two neighbouring entries swapped":
        lambda pr: BR.spmm_f32(with_csr(pr, lambda c, v: (c, np.concatenate([v[:62], v[[63, 62]], v[64:]])))),
    "scale applied to the sum with the bias in it": lambda pr: BR.spmm_f32(pr, order="scale after bias"),
    "relu before the bias": lambda pr: BR.spmm_f32(pr, order="relu before bias"),
    "one column shifted by 4": lambda pr: shifted(*BR.spmm_f32(pr)),
}


def test_spmm_right_answer_passes(spmm_problem):
    pr = spmm_problem
    assert pr["bias"] is not None and pr["relu"]
    print("spmm wrong-answer problem, restatement:", BR.judge_spmm(pr, *BR.spmm_wholes(pr, *BR.spmm_f32(pr))))


@pytest.mark.parametrize("fault", list(SPMM_WRONG))
def test_spmm_wrong_answer_is_rejected(spmm_problem, fault):
    pr = spmm_problem
    Y, Z = SPMM_WRONG[fault](pr)
    with pytest.raises(Rejected) as e:
        BR.judge_spmm(pr, *BR.spmm_wholes(pr, Y, Z))
    print(fault, "->", e.value)
    if "dropped" in fault or "twice" in fault or "swapped" in fault:      # Z0 alone catches what Y carries into it
        with pytest.raises(Rejected):
            BR.judge_spmm(pr, BR.spmm_wholes(pr, BR.spmm_f32(pr)[0], None)[0], BR.embed(Z, 3)[0])


@pytest.mark.parametrize("where", ["Y padding", "Y band", "Z0 band", "a row never written", "source row 0 read"])
def test_spmm_stray_write_or_missing_row_is_rejected(spmm_problem, where):
    pr = spmm_problem
    Y, Z = BR.spmm_f32(pr)
    if where == "source row 0 read":
        Y[3] += pr["X"][0, :pr["F"]]
    if where == "a row never written":
        Y[13] = np.nan
    Yw, Zw = BR.spmm_wholes(pr, Y, Z)
    if where == "Y padding":
        Yw[2, pr["F"]] = 0.0
    if where == "Y band":
        Yw[-1, 0] = 1.0
    if where == "Z0 band":
        Zw[0, 2] = 0.0
    with pytest.raises(Rejected) as e:
        BR.judge_spmm(pr, Yw, Zw)
    print(where, "->", e.value)


DENSE_WRONG = {
    "the k-tail dropped for F = 17": lambda pr: BR.dense_f32(pr, F_used=16),
    "rows 16..31 given rows 0..15's result": lambda pr: np.concatenate([BR.dense_f32(pr)[:16]] * 2 + [BR.dense_f32(pr)[32:]]),
    "W2's columns permuted": lambda pr: BR.dense_f32(pr)[:, [1, 0, 2]],
}


@pytest.mark.parametrize("kind", ["real", "int"])
@pytest.mark.parametrize("fault", list(DENSE_WRONG))
def test_dense_wrong_answer_is_rejected(fault, kind):
    pr = BR.dense_problem(BR.dense_case(37, 17, 4, kind=kind))
    BR.judge_dense(pr, BR.embed(BR.dense_f32(pr), 3)[0])
    with pytest.raises(Rejected) as e:
        BR.judge_dense(pr, BR.embed(DENSE_WRONG[fault](pr), 3)[0])
    print(fault, "->", e.value)
    Zw = BR.embed(BR.dense_f32(pr), 3)[0]
    Zw[-1, 0] = 0.0
    with pytest.raises(Rejected):
        BR.judge_dense(pr, Zw)


def adam_judged(st, t, res, g=None):
    return BR.judge_adam(BR.adam_ref(st, t, **H), *BR.adam_wholes(res, st["g"] if g is None else g), "wrong answer")


@pytest.mark.parametrize("t", (1, 2, 1000))
@pytest.mark.parametrize("fault", ["step t - 1", "step t + 1", "eps inside the root", "float32 bias corrections"])
def test_adam_wrong_step_or_formula_is_rejected(fault, t):
    st = BR.adam_problem(1027, "wrong answers")
    adam_judged(st, t, BR.adam_f32(st, t, **H))
    if fault.startswith("step"):
        with np.errstate(divide="ignore"):
            res = BR.adam_f32(st, t + (1 if fault.endswith("+ 1") else -1), **H)
    else:
        res = BR.adam_f32(st, t, wrong=fault, **H)
    with pytest.raises(Rejected) as e:
        adam_judged(st, t, res)
    print(fault, "at step", t, "->", e.value)


@pytest.mark.parametrize("count", (1, 1026, 1027, ga.FULL // 256 + 1))
@pytest.mark.parametrize("fault", ["the tail element updated twice", "the tail element not updated", "g written",
                                   "a write past count"])
def test_adam_tail_faults_are_rejected(fault, count):
    st = BR.adam_problem(count, f"tail {count}")
    st["g"][-1], st["m"][-1], st["v"][-1] = 0.3, 0.01, 0.02          # (a tail element with a gradient and a history)
    res = BR.adam_f32(st, 3, **H)
    adam_judged(st, 3, res)
    g = st["g"]
    wholes = None
    if fault.endswith("twice"):
        again = BR.adam_f32({**res, "g": st["g"]}, 3, **H)
        for k in "pmv":
            res[k][-1] = again[k][-1]
    elif fault.endswith("not updated"):
        for k in "pmv":
            res[k][-1] = st[k][-1]
    elif fault == "g written":
        g = st["g"].copy()
        g[-1] = np.nextafter(g[-1], np.float32(1))
    else:
        wholes = list(BR.adam_wholes(res, g))
        wholes[1][BR.BAND + count] = 0.0
    with pytest.raises(Rejected) as e:
        if wholes is None:
            adam_judged(st, 3, res, g)
        else:
            BR.judge_adam(BR.adam_ref(st, 3, **H), *wholes, "wrong answer")
    print(fault, "->", e.value)


def test_slab_with_a_nonzero_pad_column_is_rejected():
    W1 = np.random.RandomState(5).standard_normal((3, 20)).astype(np.float32)
    flat = BR.slab_f32(W1)
    BR.judge_slab(W1, BR.banded(flat)[0])
    bad = flat.copy()
    bad[BR.slab_index(1, 27, 3)] = 1e-30                          # column 27 of a 20-column W1: padding of slab 1
    with pytest.raises(Rejected):
        BR.judge_slab(W1, BR.banded(bad)[0])
    swapped = flat.copy()
    swapped[[BR.slab_index(0, 16, 3), BR.slab_index(1, 16, 3)]] = swapped[[BR.slab_index(1, 16, 3), BR.slab_index(0, 16, 3)]]
    with pytest.raises(Rejected):
        BR.judge_slab(W1, BR.banded(swapped)[0])
    past = BR.banded(flat)[0]
    past[BR.BAND + flat.size] = 0.0
    with pytest.raises(Rejected):
        BR.judge_slab(W1, past)


# ---- 3. documented refusals --------------------------------------------------------------------------------------------
SOME, ODD = 4096, 4100          # fake device addresses: 16-byte aligned / not (never dereferenced)
OK, NULL, SHAPE, ALIGN = 0, -1, -2, -4
ADAM = (1e-3, 0.9, 0.999, 1e-8)


def refusals(lib):
    """[(name, thunk, expected status)]: every call has exactly one thing wrong, or has nothing to do."""
    out = []

    def entry(name, order, base):
        def add(what, want, **kw):
            a = {**base, **kw}
            out.append((f"{name}: {what}", lambda: getattr(lib, name)(*(a[k] for k in order), None), want))
        return add

    # gmc_spmm_f32: pointers, then sizes, then W2 / Z0 as a pair, then n_rows == 0 (csrc/spmm.hip, gmc_spmm_launch)
    add = entry("gmc_spmm_f32", ("rowptr", "col", "vals", "scale", "X", "ldx", "bias", "relu", "Y", "ldy", "n_rows", "F",
                                 "group_rows", "W2", "Z0"),
                dict(rowptr=SOME, col=SOME, vals=SOME, scale=SOME, X=SOME, ldx=64, bias=SOME, relu=1, Y=SOME, ldy=64,
                     n_rows=10, F=64, group_rows=0, W2=None, Z0=None))
    for p in ("rowptr", "col", "X", "Y"):
        add(f"{p} = NULL", NULL, **{p: None})
    add("W2 without Z0", NULL, W2=SOME)
    add("Z0 without W2", NULL, Z0=SOME)
    add("n_rows < 0", SHAPE, n_rows=-1)
    add("F = 0", SHAPE, F=0)
    add("F < 0", SHAPE, F=-4)
    add("ldx < F", SHAPE, ldx=60)
    add("ldy < F", SHAPE, ldy=60)
    add("n_rows = 0", OK, n_rows=0)
    add("n_rows = 0 with W2", OK, n_rows=0, W2=SOME, Z0=SOME)

    # gmc_dense_hw2_f32: pointers, sizes, alignment, n_rows == 0 (csrc/dense_mfma.hip)
    add = entry("gmc_dense_hw2_f32", ("H", "ldh", "dinv", "W2", "Z0", "n_rows", "F"),
                dict(H=SOME, ldh=32, dinv=SOME, W2=SOME, Z0=SOME, n_rows=10, F=32))
    for p in ("H", "dinv", "W2", "Z0"):
        add(f"{p} = NULL", NULL, **{p: None})
    add("ldh < F", SHAPE, ldh=28)
    add("n_rows < 0", SHAPE, n_rows=-1)
    add("F = 0", SHAPE, F=0)
    add("ldh % 4", ALIGN, ldh=34)
    add("H odd", ALIGN, H=ODD)
    add("n_rows = 0", OK, n_rows=0)

    # gmc_adam_f32: pointers, count / step, alignment, count == 0 (csrc/adam.hip)
    flat = dict(p=SOME, g=SOME, m=SOME, v=SOME, count=1000, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
    add = entry("gmc_adam_f32", ("p", "g", "m", "v", "count", "lr", "b1", "b2", "eps", "step"), dict(flat, step=1))
    for p in "pgmv":
        add(f"{p} = NULL", NULL, **{p: None})
        add(f"{p} odd", ALIGN, **{p: ODD})
    add("count < 0", SHAPE, count=-1)
    add("step = 0", SHAPE, step=0)
    add("step < 0", SHAPE, step=-3)
    add("count = 0", OK, count=0)

    # the devstep forms (adam_devstep): pointers with the counter, count, alignment; the model forms look at N, F and the
    # slab first, the publishing form at its two pointers before that.  (No count == 0 call: they tick even then.)
    add = entry("gmc_adam_devstep_f32", ("p", "g", "m", "v", "count", "lr", "b1", "b2", "eps", "counter"),
                dict(flat, counter=SOME))
    for p in ("p", "g", "m", "v", "counter"):
        add(f"{p} = NULL", NULL, **{p: None})
    for p in "pgmv":
        add(f"{p} odd", ALIGN, **{p: ODD})
    add("count < 0", SHAPE, count=-1)

    model = dict(p=SOME, g=SOME, m=SOME, v=SOME, N=100, F=32, slab=SOME, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, counter=SOME)
    forms = (("gmc_adam_devstep_model_f32", ("p", "g", "m", "v", "N", "F", "slab", "lr", "b1", "b2", "eps", "counter"),
              model),
             ("gmc_publish_adam_devstep_model_f32", ("src", "publish_n", "dst", "p", "g", "m", "v", "N", "F", "slab", "lr", "b1",
                                                     "b2", "eps", "counter"), dict(model, src=SOME, publish_n=1, dst=SOME)))
    for name, order, base in forms:
        add = entry(name, order, base)
        for p in ("p", "g", "m", "v", "counter"):
            add(f"{p} = NULL", NULL, **{p: None})
        for p in "pgmv":
            add(f"{p} odd", ALIGN, **{p: ODD})
        add("slab odd", ALIGN, slab=ODD)
        for what, kw in (("N = 0", dict(N=0)), ("N < 0", dict(N=-1)), ("F = 0", dict(F=0)), ("F < 0", dict(F=-4)),
                         ("F % 4", dict(F=30))):
            add(what, SHAPE, **kw)
        if "publish" in name:
            add("publish_src = NULL", NULL, src=None)
            add("pinned_dst = NULL", NULL, dst=None)
            add("publish_n = 0", SHAPE, publish_n=0)
            add("publish_n < 0", SHAPE, publish_n=-1)

    # gmc_w1_slab_f32 / gmc_publish_f32 (csrc/w1_slab.hip)
    add = entry("gmc_w1_slab_f32", ("W1", "N", "F", "slab"), dict(W1=SOME, N=100, F=32, slab=SOME))
    for p in ("W1", "slab"):
        add(f"{p} = NULL", NULL, **{p: None})
        add(f"{p} odd", ALIGN, **{p: ODD})
    for what, kw in (("N = 0", dict(N=0)), ("F = 0", dict(F=0)), ("F % 4", dict(F=30))):
        add(what, SHAPE, **kw)
    add = entry("gmc_publish_f32", ("src", "n", "dst"), dict(src=SOME, n=4, dst=SOME))
    add("src = NULL", NULL, src=None)
    add("pinned_dst = NULL", NULL, dst=None)
    add("n < 0", SHAPE, n=-1)
    add("n = 0", OK, n=0)
    return out


def test_documented_refusals(built):
    lib = built.hip.load()
    cases = refusals(lib)
    wrong = {}
    for name, thunk, want in cases:
        got = thunk()
        assert got <= 0, (name, got, "the call reached a launch")
        if got != want:
            wrong[name] = (got, want)
    assert not wrong, wrong
    assert {n.split(":")[0] for n, _t, _w in cases} == {
        "gmc_spmm_f32", "gmc_dense_hw2_f32", "gmc_adam_f32", "gmc_adam_devstep_f32", "gmc_adam_devstep_model_f32",
        "gmc_publish_adam_devstep_model_f32", "gmc_w1_slab_f32", "gmc_publish_f32"}
    assert {w for _n, _t, w in cases} == {OK, NULL, SHAPE, ALIGN}
    print(f"{len(cases)} refusals as documented")


def test_slab_floats_of_an_empty_model_is_zero(built):
    lib = built.hip.load()
    for N, F in ((0, 16), (-1, 16), (16, 0), (16, -4)):
        assert lib.gmc_w1_slab_floats(N, F) == 0
    assert lib.gmc_w1_slab_floats(1000, 72) == 5 * 1000 * 16 == BR.slab_floats(1000, 72)
    assert lib.gmc_w1_slab_floats(3, 4) == 48
