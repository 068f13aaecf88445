"""GPU tests of the functional form of the model (gmc_fn_* of include/gcnmaxcut.h, csrc/functional.hip;
gcn_max_cut_amd.functional) against the float64 restatement of tests/functional_ref.py.

Every case of functional_ref.CASES - single graphs of K, K + 1, 65, 257 and 300 nodes, a star of 70 leaves (the wave-per-row
path), the mixed batch (5, 300, 65, 257), one graph of 4200 nodes; K in {2, 3, 4, 8}; hidden 4, 12, 36; unit and real-valued
weights; the adjacency or dense features of 64 / 62 columns - runs through the entry points themselves, workspace and
outputs filled with NaN first: P, the backward of a dLoss/dP drawn at random (the backward as a linear map), both losses
with terminals on and off (loss, GP, and the backward of that GP), twice for the same bytes.  Then: each graph of a batch
alone gives the bytes it gives inside the batch; K = 3 against the existing net(g, a_pad) / net(g, embed.weight) autograd
path and Training.cut_loss; the loss against the one gmc_kway_forward / gmc_large_forward reports for the same P; a 2-class
model trained with torch.optim.Adam through probabilities + cut_loss.

Bars: stepcheck's - P_TOL for P, ORACLE_BAR and ROW_TOL / ROW_FLOOR for the gradients and (per row) dX and GP; losses within
5e-5 * C * (total edge weight), the bar tests/test_gpu_expected_cut.py uses, and the hard loss of a unit-weight graph
exactly -C * cut.  tests/test_functional_host.py asserts the premise on the float64 reference: every case is decided (no
relu kink, no argmax tie, no saturated row) and a plain float32 numpy evaluation keeps half of every bar.

Measured on the MI355X (the tests print each figure with -s): see DESIGN.md section 26."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import functional_ref as FR
from tests import kway_ref as KR
from tests import util
from tests.stepcheck import KEYS, P_TOL

pytestmark = pytest.mark.gpu
LOSS_BAR = 5e-5
CC = FR.CC
SOME = 4096


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


class Library:
    """The gmc_fn_* entry points themselves on a batch and a set of parameters (float32 numpy by name); every buffer a
    call writes is NaN before it."""

    def __init__(self, pkg, batch, params, X=None):
        self.pkg, self.lib, self.batch = pkg, pkg.hip.load(), batch
        (self.N, self.F), self.K = params[KEYS[0]].shape, params[KEYS[2]].shape[1]
        self.Fp = (self.F + 3) // 4 * 4
        self.offs, self.count = pkg.engine.flat_layout(self.N, self.Fp, self.K)
        self.flat = torch.zeros(self.count, device="cuda")
        for k, v in self.views(self.flat).items():
            v.copy_(torch.from_numpy(params[k]))
        p, o = pkg.hip.ptr(self.flat), self.offs
        self.model = pkg.hip.GmcModel(N=self.N, F=self.Fp, K=self.K, W1=p, b1=p + 4 * o[1], W2=p + 4 * o[2], b2=p + 4 * o[3])
        self.X = None
        if X is not None:   # [R, N] padded to a multiple of 4 columns
            self.X = torch.zeros((batch.R, (self.N + 3) // 4 * 4), device="cuda")
            self.X[:, :self.N] = torch.from_numpy(X)
        self.need = int(self.lib.gmc_fn_workspace_bytes(batch.ref(), C.byref(self.model), int(X is not None)))
        assert self.need > 0
        self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")
        self.loss_need = int(self.lib.gmc_fn_cut_loss_workspace_bytes(batch.ref(), self.K))
        assert self.loss_need > 0

    def views(self, buf):
        o, N, F, Fp, K = self.offs, self.N, self.F, self.Fp, self.K
        return {KEYS[0]: buf[o[0]:o[1]].view(N, Fp)[:, :F], KEYS[1]: buf[o[1]:o[2]][:F], KEYS[2]: buf[o[2]:o[3]].view(Fp, K)[:F],
                KEYS[3]: buf[o[3]:o[4]]}

    def _x(self):
        return (self.pkg.hip.ptr(self.X), 0 if self.X is None else self.X.shape[1])

    def forward(self):
        p = self.pkg.hip.ptr
        self.ws.fill_(255)                 # all-ones bytes = NaN
        P = torch.full((self.batch.R, self.K), float("nan"), device="cuda")
        rc = self.lib.gmc_fn_forward(self.batch.ref(), C.byref(self.model), *self._x(), p(self.ws), self.need, p(P),
                                     self.pkg.hip.stream())
        self.pkg.hip.check(rc, "gmc_fn_forward")
        return P

    def backward(self, P, GP, want_dx=True):
        """(gradient by name, dX [R,N] or None) - numpy - from the workspace the last forward left."""
        p = self.pkg.hip.ptr
        grad = torch.full((self.count,), float("nan"), device="cuda")
        dX = torch.full_like(self.X, float("nan")) if self.X is not None and want_dx else None
        rc = self.lib.gmc_fn_backward(self.batch.ref(), C.byref(self.model), *self._x(), p(self.ws), self.need, p(P), p(GP),
                                      p(grad), p(dX), 0 if dX is None else dX.shape[1], self.pkg.hip.stream())
        self.pkg.hip.check(rc, "gmc_fn_backward")
        pad = grad.clone()
        for v in self.views(pad).values():
            v.zero_()
        assert not pad.any()               # the hidden width's pad columns: exact zeros
        return ({k: v.cpu().numpy() for k, v in self.views(grad).items()},
                None if dX is None else dX[:, :self.N].cpu().numpy())

    def loss(self, P, relaxed, terminals, want_gp=True, Cc=CC):
        p = self.pkg.hip.ptr
        ws = torch.full((self.loss_need,), 255, dtype=torch.uint8, device="cuda")
        losses = torch.full((self.batch.B,), float("nan"), device="cuda")
        GP = torch.full((self.batch.R, self.K), float("nan"), device="cuda") if want_gp else None
        rc = self.lib.gmc_fn_cut_loss_f32(self.batch.ref(), self.K, int(terminals), p(P), Cc, int(relaxed), p(ws),
                                          self.loss_need, p(losses), p(GP), self.pkg.hip.stream())
        self.pkg.hip.check(rc, "gmc_fn_cut_loss_f32")
        return losses, GP


def library_of(pkg, case):
    batch = pkg.GraphBatch(FR.case_handles(pkg, case), None, torch.device("cuda", 0))
    assert (batch.host.vals is not None) == (case.weights == "real")
    return Library(pkg, batch, FR.case_params(case), FR.case_features(case))


def within_bars(got, ref, what):
    """A dict of tensors against its float64 reference at the gradient bars; prints and returns the two fractions."""
    a, r = FR.grad_ratios(got, ref)
    print(f"{what}: {a:.3f} of ORACLE_BAR, {r:.3f} of ROW_TOL")
    assert a <= 1.0 and r <= 1.0, (what, a, r)
    return a, r


def check_losses(case, got, ref, relaxed, terminals, what):
    csrs = FR.case_csrs(case)
    for g, csr in enumerate(csrs):
        bar = LOSS_BAR * CC * KR.total_weight([csr])
        err = abs(float(got[g]) - ref[g])
        print(f"{what} graph {g}: loss {got[g]:.6f} float64 {ref[g]:.6f} err {err:.2e} bar {bar:.2e}")
        if not relaxed and case.weights == "unit":   # the cut is an integer, the loss its one float32 product with -C
            cut = round(-ref[g] / CC)
            assert abs(-ref[g] / CC - cut) < 1e-9 and got[g] == -(np.float32(CC) * np.float32(cut)), (what, g, got[g], ref[g])
        assert err <= bar, (what, g, got[g], ref[g])


# ---- every case through the entry points against float64
@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_case_against_float64(pkg, case):
    run, ref, what = library_of(pkg, case), FR.reference(case), FR.case_id(case)
    dense = case.features != "adj"
    P = run.forward()
    p_err = float(np.abs(P.cpu().numpy() - ref.P).max())
    print(f"{what}: P {p_err:.2e}")
    assert torch.isfinite(P).all() and p_err < P_TOL, (what, p_err)
    assert np.array_equal(P.cpu().numpy().argmax(1), ref.P.argmax(1))       # (no row of a case is near a tie)
    # the backward as a linear map: a dLoss/dP drawn at random
    GP = torch.from_numpy(FR.case_gp(case)).cuda()
    grads, dX = run.backward(P, GP)
    within_bars(grads, ref.grads, f"{what} random GP")
    if dense:
        within_bars({"dX": dX}, {"dX": ref.dX}, f"{what} random GP dX")
    else:
        assert dX is None and not grads[KEYS[0]][run.batch.n_max:].any()    # rows past every graph's n: exactly 0
    # a second run gives the same bytes
    P2 = run.forward()
    grads2, dX2 = run.backward(P2, GP)
    assert P2.cpu().numpy().tobytes() == P.cpu().numpy().tobytes()
    assert all(grads2[k].tobytes() == grads[k].tobytes() for k in KEYS) and (dX is None or dX2.tobytes() == dX.tobytes())
    # both losses, terminals on and off: the loss, its GP, and the backward of that GP
    for relaxed, terminals in FR.LOSSES:
        variant = (relaxed, terminals)
        tag = f"{what} relaxed={relaxed} terminals={terminals}"
        losses, GPl = run.loss(P, relaxed, terminals)
        check_losses(case, losses.cpu().numpy(), ref.losses[variant], relaxed, terminals, tag)
        within_bars({"GP": GPl.cpu().numpy()}, {"GP": ref.loss_gp[variant]}, f"{tag} GP")
        alone, none = run.loss(P, relaxed, terminals, want_gp=False)
        again, GPl2 = run.loss(P, relaxed, terminals)
        assert none is None and alone.cpu().numpy().tobytes() == losses.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
        assert GPl2.cpu().numpy().tobytes() == GPl.cpu().numpy().tobytes()
        run.forward()
        grads, dX = run.backward(P, GPl, want_dx=dense)
        within_bars(grads, ref.loss_grads[variant], f"{tag} gradient")
        if dense:
            within_bars({"dX": dX}, {"dX": ref.loss_dX[variant]}, f"{tag} dX")


def test_constant_features_skip_dx(pkg):
    case = next(c for c in FR.CASES if c.shape == "n65" and c.features == 62)
    run, ref = library_of(pkg, case), FR.reference(case)
    GP = torch.from_numpy(FR.case_gp(case)).cuda()
    P = run.forward()
    with pkg.hip.Probe(32) as probe:
        grads, dX = run.backward(P, GP, want_dx=False)
    assert dX is None and [t for t, _ms in probe.records].count("gemm") == 1            # dW1 = X^T @ U alone
    within_bars(grads, ref.grads, "constant X")
    P = run.forward()
    with pkg.hip.Probe(32) as probe:
        grads2, dX = run.backward(P, GP)
    assert [t for t, _ms in probe.records].count("gemm") == 2                           # ... and dX = U @ W1^T
    assert all(grads2[k].tobytes() == grads[k].tobytes() for k in KEYS)


# ---- a graph's results do not depend on the rest of the batch
@pytest.mark.parametrize("case", [c for c in FR.CASES if c.shape == "batch"], ids=FR.case_id)
def test_each_graph_alone_gives_the_bytes_it_gives_in_the_batch(pkg, case):
    whole = library_of(pkg, case)
    P = whole.forward()
    outs = {v: whole.loss(P, *v) for v in FR.LOSSES}
    handles, params = FR.case_handles(pkg, case), FR.case_params(case)
    for g, (h, X, Pg) in enumerate(zip(handles, FR.split(case, FR.case_features(case)), FR.split(case, P.cpu().numpy()))):
        if h.n < case.K:
            continue
        one = Library(pkg, pkg.GraphBatch([h], None, torch.device("cuda", 0)), params, X)
        P1 = one.forward()
        assert P1.cpu().numpy().tobytes() == Pg.tobytes(), g
        for v, (losses, GP) in outs.items():
            l1, GP1 = one.loss(P1, *v)
            assert l1.cpu().numpy().tobytes() == losses[g:g + 1].cpu().numpy().tobytes(), (g, v)
            assert GP1.cpu().numpy().tobytes() == FR.split(case, GP.cpu().numpy())[g].tobytes(), (g, v)


def test_empty_batch_zeroes_the_gradient(pkg):
    hip = pkg.hip
    lib = hip.load()
    N, F, K = 16, 4, 2
    _offs, count = pkg.engine.flat_layout(N, F, K)
    grad = torch.full((count + 4,), float("nan"), device="cuda")
    b = hip.GmcBatch(B=0, R=0, nnz=0, n_max=0, goff=SOME, rowptr=SOME, gcol=SOME, lcol=SOME, dinv=SOME)
    m = hip.GmcModel(N=N, F=F, K=K, W1=SOME, b1=SOME, W2=SOME, b2=SOME)
    rc = lib.gmc_fn_backward(C.byref(b), C.byref(m), None, 0, SOME, 1 << 20, SOME, SOME, hip.ptr(grad), None, 0, hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert not grad[:count].any() and torch.isnan(grad[count:]).all()                   # no tail slot is written
    Fn = pkg.functional
    W = [torch.randn(s, device="cuda", requires_grad=True) for s in ((N, F), (F,), (F, K), (K,))]
    P = Fn.gcn_softmax(pkg.GraphBatch([], None, torch.device("cuda", 0)), *W)
    assert tuple(P.shape) == (0, K)
    P.sum().backward()
    assert all(w.grad is not None and not w.grad.any() for w in W)


# ---- K = 3: the existing autograd path and Training.cut_loss
def test_three_classes_agree_with_the_existing_autograd_path(pkg):
    Fn = pkg.functional
    T, _cfg, net, _embed, _opt, params = util.model(32, n_nodes=1000, seed=3)
    ds = util.product_dataset([(60, 7, 1)])
    (g, a_pad, nx_g, _terms), = ds.values()
    csr = util.csrs_of(ds)[0]
    named = dict(net.named_parameters())
    net.eval()
    f = FR.forward(csr, params)
    for relaxed in (False, True):
        value, GP = FR.loss_and_gp(csr, f["P"], CC, relaxed, True)
        ref, _ = FR.backward(f, GP, params)
        got = {}
        for path in ("existing", "functional"):
            net.zero_grad()
            if path == "existing":
                loss = T.cut_loss(g, net(g, a_pad), C=CC, relaxed=relaxed)
            else:
                loss = Fn.cut_loss(g, Fn.probabilities(net, g), C=CC, relaxed=relaxed)
            loss.backward()
            got[path] = (float(loss.detach()), {k: named[k].grad.detach().cpu().numpy().copy() for k in KEYS})
            within_bars(got[path][1], ref, f"K=3 relaxed={relaxed} {path} against float64")
        within_bars(got["functional"][1], got["existing"][1], f"K=3 relaxed={relaxed} functional against existing")
        bar = LOSS_BAR * CC * KR.total_weight([csr])
        print(f"K=3 relaxed={relaxed}: loss existing {got['existing'][0]:.6f} functional {got['functional'][0]:.6f} "
              f"float64 {value:.6f} bar {bar:.2e}")
        if not relaxed:   # unit weights: exactly equal
            assert got["functional"][0] == got["existing"][0] == float(-(np.float32(CC) * np.float32(round(-value / CC))))
        assert abs(got["functional"][0] - got["existing"][0]) <= bar and abs(got["functional"][0] - value) <= bar
    # learned embeddings: net(g, embed.weight) against probabilities(net, g, X)
    X = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, (60, 1000)).astype(np.float32)).cuda().requires_grad_()
    fx = FR.forward(csr, params, X.detach().cpu().numpy())
    value, GP = FR.loss_and_gp(csr, fx["P"], CC, True, True)
    ref, ref_dX = FR.backward(fx, GP, params)
    got = {}
    for path in ("existing", "functional"):
        net.zero_grad()
        X.grad = None
        P = net(g, X) if path == "existing" else Fn.probabilities(net, g, X)
        (T.cut_loss if path == "existing" else Fn.cut_loss)(g, P, C=CC, relaxed=True).backward()
        got[path] = {**{k: named[k].grad.detach().cpu().numpy().copy() for k in KEYS}, "dX": X.grad.cpu().numpy().copy()}
        within_bars(got[path], {**ref, "dX": ref_dX}, f"K=3 embeddings {path} against float64")
    within_bars(got["functional"], got["existing"], "K=3 embeddings functional against existing")


# ---- the loss against the one the K-class forwards report for the same P
@pytest.mark.parametrize("case", [c for c in FR.CASES if c.features == "adj" and c.shape not in ("nK", "nK1", "batch")],
                         ids=FR.case_id)
def test_loss_equals_the_one_the_forward_reports(pkg, case):
    params = FR.case_params(case)
    eng = pkg.engine.FusedEngine(*params[KEYS[0]].shape, case.K, kway=True)   # gmc_kway_* / gmc_large_*, K = 3 too
    for k, v in eng.views().items():
        v.copy_(torch.from_numpy(params[k]))
    run = library_of(pkg, case)
    csr = FR.case_csrs(case)[0]
    for relaxed in (False, True):
        P, _S, reported = eng.forward(run.batch, CC, want_loss=True, loss="expected_cut" if relaxed else "cut")
        losses, _gp = run.loss(P, relaxed, True, want_gp=False)
        got, want = float(losses[0]), float(reported[0])
        bar = LOSS_BAR * CC * KR.total_weight([csr])
        print(f"{FR.case_id(case)} relaxed={relaxed}: gmc_fn_cut_loss_f32 {got:.6f} forward {want:.6f} bar {bar:.2e}")
        if not relaxed and case.weights == "unit":
            assert got == want
        assert abs(got - want) <= bar
        assert float(np.abs(run.forward().cpu().numpy() - P.cpu().numpy()).max()) < 2 * P_TOL   # (and the same probabilities)


# ---- the open loop: a 2-class model, torch's Adam
def test_two_class_model_trains_with_torch_adam(pkg):
    Fn = pkg.functional
    case = FR.Case("n65", 2, 12, "real", "adj", 0)
    csr, params = FR.case_csrs(case)[0], FR.case_params(case)
    g = FR.case_handles(pkg, case)[0]
    net = pkg.engine.module_of({k: torch.from_numpy(v) for k, v in params.items()})
    assert net.conv2.weight.shape[1] == 2
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.5)
    history = []
    for step in range(20):
        opt.zero_grad()
        loss = Fn.cut_loss(g, Fn.probabilities(net, g), C=CC, relaxed=True)
        loss.backward()
        if step == 0:
            f = FR.forward(csr, params)
            value, GP = FR.loss_and_gp(csr, f["P"], CC, True, True)
            ref, _ = FR.backward(f, GP, params)
            got = {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}
            within_bars(got, ref, "2-class first step")
            assert abs(float(loss.detach()) - value) <= LOSS_BAR * CC * KR.total_weight([csr])
        torch.nn.utils.clip_grad_norm_(net.parameters(), 10.0)
        opt.step()
        sched.step()
        history.append(float(loss.detach()))
    print(f"2-class relaxed loss: {history[0]:.4f} -> {history[-1]:.4f}")
    assert history[-1] < history[0], history
    # a hidden width that is no multiple of 4, constant features (parameter gradients only), a retained graph walked twice
    Xn = np.random.RandomState(1).uniform(-1, 1, (g.n, 62)).astype(np.float32)
    wide = KR.random_params(62, 6, 2, 2)
    X = torch.from_numpy(Xn).cuda()
    W = [torch.from_numpy(wide[k]).cuda().requires_grad_() for k in KEYS]
    out = Fn.cut_loss(g, Fn.gcn_softmax(g, *W, X=X), C=CC, relaxed=True, terminals=False)
    first = torch.autograd.grad(out, W, retain_graph=True)
    second = torch.autograd.grad(out, W)
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and X.grad is None
    f = FR.forward(csr, wide, Xn)
    value, GP = FR.loss_and_gp(csr, f["P"], CC, True, False)
    within_bars({k: t.cpu().numpy() for k, t in zip(KEYS, first)}, FR.backward(f, GP, wide)[0], "hidden 6, N = 62")
    assert abs(float(out.detach()) - value) <= LOSS_BAR * CC * KR.total_weight([csr])
