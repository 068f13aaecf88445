"""CPU checks of the functional form of the model (include/gcnmaxcut.h, gmc_fn_*; gcn_max_cut_amd.functional): the premise
of the GPU test on every case of tests/functional_ref.py, the restatement itself against torch autograd on the dense
formula and against enumeration, every argument error of the five entry points (fake pointers, one thing wrong per call:
no call reaches a launch), the workspace sizes, and the kernels in the code object."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest
import torch

from tests import functional_ref as FR
from tests import kway_ref as KR
from tests import large_ref as LR
from tests import stepcheck, util
from tests import test_api_status as A
from tests.stepcheck import KEYS

SOME, ODD, BIG = A.SOME, A.ODD, A.BIG
LARGE = 1 << 20


# ---- the premise of the GPU test
@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_cases_are_decided_and_within_float32_reach(case):
    gap, margin, unsaturated = FR.preconditions(case)
    assert gap >= KR.KINK and margin >= KR.MARGIN and unsaturated >= LR.UNSATURATED, (gap, margin, unsaturated)
    figures = FR.f32_figures(case)
    assert max(figures.values()) <= 0.5, figures                # a plain float32 evaluation keeps half of every bar
    for seed in range(case.seed):                                # the seed is the first for which all of that holds
        earlier = case._replace(seed=seed)
        assert not (FR.well_posed(earlier) and max(FR.f32_figures(earlier).values()) <= 0.5), seed


def test_case_list_covers_what_it_should():
    shapes = {c.shape for c in FR.CASES}
    assert shapes == set(FR.SHAPES)
    for shape in shapes:
        assert {c.weights for c in FR.CASES if c.shape == shape} == {"unit", "real"}, shape
        assert any(c.features != "adj" for c in FR.CASES if c.shape == shape), shape
    assert {c.K for c in FR.CASES} == {2, 3, 4, 8} and {c.hidden for c in FR.CASES} == {4, 12, 36}
    assert {c.features for c in FR.CASES} == {"adj", 64, 62}
    sizes = {len(rp) - 1 for c in FR.CASES for rp, _cl, _vl in FR.case_csrs(c)}
    assert {3, 4, 5, 8, 9, 65, 257, 300, 71, 4200} <= sizes
    star = FR.case_csrs(next(c for c in FR.CASES if c.shape == "star70"))[0]
    assert int(np.diff(star[0]).max()) == 70 > 64                # the wave-per-row path


# ---- the restatement against torch autograd on the dense formula
def dense_torch(csr, params, X, K):
    rp, cl, vl = csr
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    A_ = torch.zeros((n, n), dtype=torch.float64)
    A_[rows, cl] = 1.0
    Aval = torch.zeros((n, n), dtype=torch.float64)
    Aval[rows, cl] = torch.ones(len(cl), dtype=torch.float64) if vl is None else torch.from_numpy(vl.astype(np.float64))
    W = [torch.tensor(np.asarray(params[k], np.float64), requires_grad=True) for k in KEYS]
    Xt = None if X is None else torch.tensor(np.asarray(X, np.float64), requires_grad=True)
    dinv = torch.from_numpy(1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(np.float64)))[:, None]
    T0 = dinv * ((Aval @ W[0][:n]) if Xt is None else (Xt @ W[0]))
    H = torch.relu(dinv * (A_ @ T0) + W[1])
    P = torch.softmax(dinv * (A_ @ (dinv * H @ W[2])) + W[3], dim=1)
    return P, W, Xt, Aval


@pytest.mark.parametrize("K,n,features", [(2, 5, "adj"), (3, 12, "adj"), (5, 9, 6), (2, 12, 7), (8, 10, "adj")])
def test_restatement_against_torch_autograd(K, n, features):
    rng = np.random.RandomState(K * 100 + n)
    _n, rp, col = LR.circulant(n, 3, 1)
    csr = (rp.astype(np.int32), col.astype(np.int32), LR.edge_weights(n, rp, col, 3))
    params = KR.random_params(12 if features == "adj" else features, 5, K, 1)
    X = None if features == "adj" else rng.uniform(-1, 1, (n, features))
    f = FR.forward(csr, params, X)
    P, W, Xt, Aval = dense_torch(csr, params, X, K)
    assert np.abs(P.detach().numpy() - f["P"]).max() < 1e-12
    eye = torch.eye(K, dtype=torch.float64)

    def compare(GP, loss_t):
        grads, dX = FR.backward(f, GP, params)
        leaves = W + ([] if Xt is None else [Xt])
        got = torch.autograd.grad(loss_t, leaves, retain_graph=True)
        for k, g in zip(KEYS, got):
            assert np.abs(g.numpy() - grads[k]).max() < 1e-11 * max(1.0, np.abs(grads[k]).max()), k
        if Xt is not None:
            assert np.abs(got[4].numpy() - dX).max() < 1e-11

    GP = rng.standard_normal((n, K))
    compare(GP, (torch.from_numpy(GP) * P).sum())                # the backward as a linear map
    for relaxed, terminals in FR.LOSSES:
        value, GP = FR.loss_and_gp(csr, f["P"], FR.CC, relaxed, terminals)
        # override_fixed_nodes with its straight-through form, then (hard) apply_max_to_one_hot's
        Pt = P + (torch.cat([eye[:min(K, n)], P[K:]]) - P).detach() if terminals else P
        if not relaxed:
            S = (KR.partition(f["P"], K) if terminals else f["P"].argmax(1))
            Pt = Pt + (eye[torch.from_numpy(np.asarray(S))] - Pt).detach()
        # compute_loss: -C/2 * sum_uv w_uv (1 - Pt_u . Pt_v); its gradient in Pt is -C/2 * (-2 A_val Pt) = C * A_val @ Pt
        loss_t = -FR.CC * 0.5 * (Aval * (1.0 - Pt @ Pt.T)).sum()
        assert abs(float(loss_t.detach()) - value) < 1e-10, (relaxed, terminals)
        compare(GP, loss_t)


# ---- terminals = False against enumeration
@pytest.mark.parametrize("K,n", [(2, 8), (3, 6), (4, 5)])
def test_loss_without_terminals_against_brute_force(K, n):
    _n, rp, col = LR.circulant(n, 3, 2)
    csr = (rp.astype(np.int32), col.astype(np.int32), LR.edge_weights(n, rp, col, 5))
    rp_, cl_, w, rows = KR._edges(*csr)
    best, values = FR.brute_force_best_cut(csr, K), []
    P = np.random.RandomState(n).dirichlet(np.ones(K), n)
    expected = 0.0
    for S in itertools.product(range(K), repeat=n):
        S = np.array(S)
        cut = 0.5 * float((w * (S[rows] != S[cl_])).sum())
        onehot = np.eye(K)[S] * 0.9 + 0.1 / K                   # probabilities whose plain argmax is S
        hard, GP = FR.loss_and_gp(csr, onehot, 1.3, False, False)
        assert abs(hard + 1.3 * cut) < 1e-12                     # no node is forced: node 0 may sit in class 1
        assert np.allclose(GP, 1.3 * stepcheck.csr_mm(rp_, cl_, w, np.eye(K)[S]))
        soft, _gp = FR.loss_and_gp(csr, np.eye(K)[S], 1.3, True, False)
        assert abs(soft - hard) < 1e-12                          # the relaxed loss of a decided P is the hard one
        values.append(hard)
        expected += float(np.prod(P[np.arange(n), S])) * cut
    assert abs(min(values) + 1.3 * best) < 1e-12                # unconstrained max-K-cut is within the loss's reach
    soft, GP = FR.loss_and_gp(csr, P, 1.3, True, False)
    assert abs(soft + 1.3 * expected) < 1e-10                    # the expected cut of independent rounding, no row overridden
    with_terms, _gp = FR.loss_and_gp(csr, P, 1.3, True, True)
    assert abs(with_terms - soft) > 1e-3                         # (and the terminals do change it)


# ---- the C ABI: argument errors
def fn_model(**kw):
    return {**dict(N=1000, F=32, K=4, flags=0, W1=SOME, b1=SOME, W2=SOME, b2=SOME), **kw}


def fn_batch(**kw):
    return {**A.batch_fields(table=False), **kw}


def fn_call(hip, entry, batch="default", model="default", nbytes=BIG, **a):
    lib = hip.load()
    b = None if batch is None else C.byref(hip.GmcBatch(**(fn_batch() if batch == "default" else batch)))
    m = None if model is None else C.byref(hip.GmcModel(**(fn_model() if model == "default" else model)))
    g = {**dict(ws=SOME, P=SOME, GP=SOME, grad=SOME, X=None, ldx=0, dX=None, lddx=0, K=4, terminals=1, kind=0, loss=SOME), **a}
    if entry == "gmc_fn_forward":
        return lib.gmc_fn_forward(b, m, g["X"], g["ldx"], g["ws"], nbytes, g["P"], None)
    if entry == "gmc_fn_backward":
        return lib.gmc_fn_backward(b, m, g["X"], g["ldx"], g["ws"], nbytes, g["P"], g["GP"], g["grad"], g["dX"], g["lddx"],
                                   None)
    assert entry == "gmc_fn_cut_loss_f32"
    return lib.gmc_fn_cut_loss_f32(b, g["K"], g["terminals"], g["P"], 1.0, g["kind"], g["ws"], nbytes, g["loss"],
                                   g["GP"] if "GP" in a else None, None)


@pytest.mark.parametrize("entry", ("gmc_fn_forward", "gmc_fn_backward"))
def test_argument_errors_of_forward_and_backward(built, entry):
    hip = built.hip
    lib = hip.load()
    backward = entry == "gmc_fn_backward"
    call = lambda **kw: fn_call(hip, entry, **kw)   # noqa: E731
    bat, mod = lambda **kw: fn_batch(**kw), lambda **kw: fn_model(**kw)   # noqa: E731
    assert call(batch=None) == -1 and call(model=None) == -1
    assert call(batch=bat(abi=100)) == -8 and call(model=mod(abi=100)) == -8
    for f in A.BATCH_PTRS:
        assert call(batch=bat(**{f: None})) == -1, f
    for f in ("W1", "b1", "W2", "b2"):
        assert call(model=mod(**{f: None})) == -1, f
    for K in (1, 9, 0):
        assert call(model=mod(K=K)) == -3, K
    for K in (2, 3, 8):                                          # 3 included
        assert call(model=mod(K=K), nbytes=0) == -5, K
    for f in ("B", "R", "nnz"):
        assert call(batch=bat(**{f: -1})) == -2, f
    for n in (0, -1):
        assert call(model=mod(N=n)) == -2
    for f, rc in ((0, -2), (-4, -2), (30, -7), (4100, -7)):
        assert call(model=mod(F=f)) == rc, f
    for p, rc in ((-0.25, -2), (1.0, -2), (float("nan"), -2), (0.5, -7)):   # no dropout
        assert call(model=mod(dropout_p=p)) == rc, p
    assert call(model=mod(W1_slab=ODD)) == -4
    assert call(batch=bat(n_max=3)) == -6 and call(batch=bat(n_max=LARGE + 1)) == -6      # fewer than K nodes, beyond the bound
    assert call(batch=bat(n_max=LARGE), model=mod(N=LARGE), nbytes=0) == -5               # the bound itself is served
    assert call(batch=bat(n_max=4200), model=mod(N=4200), nbytes=0) == -5                 # beyond the one-workgroup heads
    assert call(model=mod(N=48)) == -2                                                    # more nodes than rows of W1 ...
    assert call(model=mod(N=48), X=SOME, ldx=48, nbytes=0) == -5                          # ... which features of their own allow
    # the features
    assert call(X=SOME, ldx=996) == -2 and call(X=ODD, ldx=1000) == -4 and call(X=SOME, ldx=1002) == -4
    assert call(X=SOME, ldx=1000, model=mod(W1=ODD)) == -4
    # workspace and outputs
    assert call(ws=None) == -1 and call(P=None) == -1
    assert call(P=ODD) == -4 and call(model=mod(W2=ODD)) == -4
    if backward:
        assert call(GP=None) == -1 and call(grad=None) == -1
        assert call(GP=ODD) == -4 and call(grad=ODD) == -4
        assert call(X=SOME, ldx=1000, dX=SOME, lddx=996) == -2
        assert call(X=SOME, ldx=1000, dX=ODD, lddx=1000) == -4 and call(X=SOME, ldx=1000, dX=SOME, lddx=1002) == -4
        assert call(ws=None, dX=ODD, lddx=1000, X=SOME, ldx=1000) == -1                   # step 4 before step 5
    # the order: the structs before the features before the outputs before the size
    assert call(batch=bat(abi=100), P=None, nbytes=0) == -8 and call(model=mod(K=9), X=ODD, ldx=1000) == -3
    assert call(X=ODD, ldx=1000, P=None) == -4 and call(P=None, nbytes=0) == -1
    for features, X in ((0, {}), (1, dict(X=SOME, ldx=1000))):
        need = lib.gmc_fn_workspace_bytes(C.byref(hip.GmcBatch(**fn_batch())), C.byref(hip.GmcModel(**fn_model())), features)
        assert need > 256 and call(nbytes=need - 1, **X) == -5
    if not backward:   # (the backward zeroes the gradient of an empty batch: a GPU test)
        assert call(batch=bat(B=0, R=0, nnz=0, n_max=0)) == 0


def test_argument_errors_of_the_loss(built):
    hip = built.hip
    lib = hip.load()
    call = lambda **kw: fn_call(hip, "gmc_fn_cut_loss_f32", **kw)   # noqa: E731
    bat = lambda **kw: fn_batch(**kw)   # noqa: E731
    assert call(batch=None) == -1 and call(batch=bat(abi=100)) == -8
    for f in ("goff", "rowptr", "gcol", "lcol"):
        assert call(batch=bat(**{f: None})) == -1, f
    assert call(batch=bat(dinv=None), nbytes=0) == -5            # (the loss does not read dinv)
    for K in (1, 9):
        assert call(K=K) == -3
    for f in ("B", "R", "nnz"):
        assert call(batch=bat(**{f: -1})) == -2, f
    for kind in (2, -1):
        assert call(kind=kind) == -9
    assert call(batch=bat(n_max=3)) == -6 and call(batch=bat(n_max=3), terminals=0, nbytes=0) == -5   # no terminals: any size
    assert call(batch=bat(n_max=LARGE + 1)) == -6 and call(batch=bat(n_max=LARGE), nbytes=0) == -5
    assert call(ws=None) == -1 and call(P=None) == -1 and call(loss=None) == -1
    assert call(P=ODD) == -4 and call(GP=ODD) == -4
    assert call(K=9, kind=5, P=None) == -3 and call(kind=5, P=None) == -9 and call(P=None, nbytes=0) == -1
    need = lib.gmc_fn_cut_loss_workspace_bytes(C.byref(hip.GmcBatch(**fn_batch())), 4)
    assert need >= 256 and call(nbytes=need - 1) == -5
    assert call(batch=bat(B=0, R=0, nnz=0, n_max=0)) == 0 and call(batch=bat(B=0, R=0, nnz=0, n_max=0), GP=SOME) == 0
    for name in ("gmc_fn_workspace_bytes", "gmc_fn_forward", "gmc_fn_backward", "gmc_fn_cut_loss_workspace_bytes",
                 "gmc_fn_cut_loss_f32"):
        assert name in hip.SYMBOLS


def test_workspace_sizes(built):
    hip = built.hip
    lib = hip.load()
    up = lambda x: (x + 255) // 256 * 256   # noqa: E731
    for n, B in ((100, 6), (5000, 1), (70000, 2)):
        b = hip.GmcBatch(**A.batch_fields(n=n, B=B, table=False))
        R_ = n * B
        slots = R_ // LR.T + B + 1
        for K in range(2, 9):
            m = hip.GmcModel(**fn_model(K=K, N=70000))
            kway = int(lib.gmc_kway_workspace_bytes(C.byref(b), C.byref(m), 1))
            with_adj = int(lib.gmc_fn_workspace_bytes(C.byref(b), C.byref(m), 0))
            with_x = int(lib.gmc_fn_workspace_bytes(C.byref(b), C.byref(m), 1))
            # gmc_kway_*'s training buffers, then dinv o GZ [R,K] and the tile partials of db2 [slots][K]
            extra = up(R_ * K * 4) + up(slots * K * 4)
            assert kway > 0 and with_adj == kway + extra, (n, B, K)
            assert 0 < with_x <= with_adj and (with_adj - with_x) % 256 == 0      # (features: no dW1 scratch)
            assert int(lib.gmc_fn_cut_loss_workspace_bytes(C.byref(b), K)) == up(slots * 4)
    b = hip.GmcBatch(**A.batch_fields())
    assert lib.gmc_fn_workspace_bytes(None, None, 0) == 0
    assert lib.gmc_fn_workspace_bytes(C.byref(b), C.byref(hip.GmcModel(**fn_model(K=9))), 0) == 0
    assert lib.gmc_fn_workspace_bytes(C.byref(b), C.byref(hip.GmcModel(**fn_model(abi=100))), 0) == 0
    assert lib.gmc_fn_workspace_bytes(C.byref(hip.GmcBatch(**A.batch_fields(), abi=100)), C.byref(hip.GmcModel(**fn_model())), 0) == 0
    assert lib.gmc_fn_cut_loss_workspace_bytes(None, 3) == 0 and lib.gmc_fn_cut_loss_workspace_bytes(C.byref(b), 9) == 0
    assert lib.gmc_fn_cut_loss_workspace_bytes(C.byref(hip.GmcBatch(**A.batch_fields(), abi=100)), 3) == 0


# ---- the kernels
FN_KERNELS = {"fn_prob_kernel": 7, "fn_softmax_bwd_kernel": 7, "fn_gy2_kernel": 7, "fn_loss_kernel": 14, "fn_fold_kernel": 1}


def test_no_instantiation_of_the_kernels_is_missing_and_none_uses_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = [s for s in util.kernel_symbols(lib_path) if "fn_" in s]
    for K in range(2, 9):
        for kernel in ("fn_prob_kernel", "fn_softmax_bwd_kernel", "fn_gy2_kernel"):
            assert any(f"{kernel}<{K}>" in s for s in names), (kernel, K)
        for soft in ("true", "false"):
            assert any(f"fn_loss_kernel<{K}, {soft}>" in s for s in names), (K, soft)
    seen = dict.fromkeys(FN_KERNELS, 0)
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
            for kernel in FN_KERNELS:
                if kernel in fields.get(".name", ""):
                    seen[kernel] += 1
                    assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
                    assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
    assert seen == FN_KERNELS


# ---- the Python surface, as far as it goes without a GPU
def test_functional_module_checks_its_arguments(built):
    Fn = built.functional
    W1, b1, W2, b2 = torch.zeros(8, 4), torch.zeros(4), torch.zeros(4, 2), torch.zeros(2)
    h = built.GraphHandle(*LR.circulant(5, 2))
    with pytest.raises(ValueError, match="parameters must be"):
        Fn.gcn_softmax(h, W1, torch.zeros(5), W2, b2)
    with pytest.raises(ValueError, match="number_classes must be in 2..8"):
        Fn.gcn_softmax(h, W1, b1, torch.zeros(4, 9), torch.zeros(9))
    with pytest.raises(ValueError, match="hidden_dim must be in 1..4096"):
        Fn.gcn_softmax(h, torch.zeros(8, 4097), torch.zeros(4097), torch.zeros(4097, 2), b2)
    with pytest.raises(ValueError, match="number_classes must be in 2..8"):
        Fn.cut_loss(h, torch.zeros(5, 1))
    with pytest.raises(ValueError, match="P must be"):
        Fn.cut_loss(h, torch.zeros(5))
    if not torch.cuda.is_available():   # there is no CPU fallback
        with pytest.raises(built.hip.HipExtensionError):
            Fn.gcn_softmax(h, W1, b1, W2, b2)
        with pytest.raises(built.hip.HipExtensionError):
            Fn.cut_loss(h, torch.full((5, 2), 0.5))
