"""CPU-side checks of the relaxed loss (GMC_LOSS_EXPECTED_CUT): the float64 restatement the GPU tests compare with
(tests/expected_cut_ref.py) against autograd through the package's own compute_loss(override_fixed_nodes(P)), its
one-hot limit, the argument checks of the three new entry points, and the Python plumbing of the loss name."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import expected_cut_ref as ER
from tests import util

F32_BAR = 1e-5   # float32 rounding of the torch chain (extend_matrix_torch stores Pt Pt^T in float32): x max(1, max|value|)


def graph_case(weighted):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    specs = [(40, 7, 3)]
    if weighted:
        graphs, terms = util.weighted_copy(specs, seed=2)
        ds = util.dataset_of(graphs, terms)
    else:
        ds = util.product_dataset(specs)
    (g, a_pad, nx_g, _t), = ds.values()
    w = g.edge_values(a_pad)
    rng = np.random.RandomState(11)
    z = rng.standard_normal((40, 3)) * 1.5
    P = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    return T, g, a_pad, w, P


@pytest.mark.parametrize("weighted", (False, True), ids=("unit", "weights"))
def test_restatement_equals_autograd_through_compute_loss_on_the_override(weighted):
    """n = 40, d = 7, C = 1.7: loss and dLoss/dP of the definition against torch autograd through
    compute_loss(override_fixed_nodes(P), A_pad, C=C) - the reference's chain without apply_max_to_one_hot."""
    T, g, a_pad, w, P = graph_case(weighted)
    Cc = 1.7
    Pt = torch.tensor(P, dtype=torch.float32, requires_grad=True)
    loss = T.compute_loss(T.override_fixed_nodes(Pt), a_pad.to(torch.float32), C=Cc)
    loss.backward()
    ref_loss, ref_gp = ER.loss_and_gp(g.rowptr, g.col, w, Pt.detach().numpy().astype(np.float64), Cc)
    err_loss = abs(float(loss.detach()) - ref_loss)
    err_gp = float(np.abs(Pt.grad.numpy() - ref_gp).max())
    print(f"expected cut vs autograd: loss {err_loss / abs(ref_loss):.1e} relative, dP {err_gp:.1e} absolute")
    assert err_loss <= F32_BAR * max(1.0, abs(ref_loss))
    assert err_gp <= F32_BAR * max(1.0, float(np.abs(ref_gp).max()))
    assert (w is not None) == weighted


@pytest.mark.parametrize("weighted", (False, True), ids=("unit", "weights"))
def test_one_hot_probabilities_give_minus_c_times_the_cut_exactly(weighted):
    _T, g, _a, w, P = graph_case(weighted)
    S = P.argmax(1)
    S[:3] = [0, 1, 2]
    hot = np.eye(3)[S]
    hot[:3] = 1.0 / 3                                     # (the override replaces rows 0..2 whatever they hold)
    Cc = 1.7
    loss, gp = ER.loss_and_gp(g.rowptr, g.col, w, hot, Cc)
    hard, hard_gp = ER.hard_loss_and_gp(g.rowptr, g.col, w, S, Cc)
    assert loss == hard and np.array_equal(gp, hard_gp)
    rows = np.repeat(np.arange(40), np.diff(g.rowptr))
    ww = np.ones(len(g.col)) if w is None else w.astype(np.float64)
    assert hard == -Cc * 0.5 * float(ww[S[rows] != S[g.col]].sum())
    assert ER.total_weight([(g.rowptr, g.col, w)]) == 0.5 * ww.sum()


def test_new_entry_points_check_their_arguments_without_a_gpu(built):
    hip = built.hip
    lib = hip.load()
    null, some = C.c_void_p(None), C.c_void_p(4096)       # (never dereferenced: the calls fail first)
    mk = lambda **kw: hip.GmcBatch(**{**dict(B=2, R=100, nnz=700, n_max=60, goff=4096, rowptr=4096, gcol=4096, lcol=4096,
                                             dinv=4096), **kw})
    b = mk()
    assert (hip.LOSS_KINDS, hip.MODEL_LOSS_EXPECTED) == ({"cut": 0, "expected_cut": 1}, 2)
    assert b"loss kind" in lib.gmc_error_string(-9)        # GMC_ERR_LOSS has its own string

    def head(batch, kind=1, Z0=some, b2=some, P=some, zparts=1, GY2=null, db2=null):
        return lib.gmc_head_loss_f32(batch, Z0, zparts, b2, 1.0, kind, P, null, null, GY2, db2, None)

    def cut(batch, kind=1, P=some, loss=some, GP=null):
        return lib.gmc_cut_loss_f32(batch, P, 1.0, kind, loss, GP, None)

    def step(batch, kind=1, param=some, grad=some, m=some, v=some, counter=some, P=some, ws=some, N=1000, F=16):
        return lib.gmc_train_step_loss_f32(batch, N, F, param, 1.0, kind, ws, 1 << 30, P, null, null, grad, m, v, 1e-3,
                                           0.9, 0.999, 1e-8, counter, null, None)

    for f in (head, cut, step):
        for kind in (2, -1, 7):
            assert f(C.byref(b), kind=kind) == -9, (f.__name__, kind)        # GMC_ERR_LOSS ...
        assert f(None, kind=2) == -9 and f(C.byref(mk(abi=100)), kind=2) == -9   # ... before anything else is looked at
        assert f(None) == -1                                                  # GMC_ERR_NULL
        assert f(C.byref(mk(abi=100))) == -8                                  # GMC_ERR_ABI
        assert f(C.byref(mk(lcol=None))) == -1
        assert f(C.byref(mk(n_max=4097))) == -6                               # GMC_ERR_GRAPH_SIZE
        for kind in (0, 1):
            assert f(C.byref(b), kind=kind, P=null) == -1
    assert head(C.byref(b), Z0=null) == -1 and head(C.byref(b), b2=null) == -1
    assert head(C.byref(b), zparts=0) == -2                                   # GMC_ERR_SHAPE
    assert head(C.byref(b), GY2=some) == -1                                   # GY2 without db2part
    assert cut(C.byref(b), loss=null) == -1
    assert cut(C.byref(mk(R=-1))) == -2
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, gcol=4096, lcol=4096, dinv=4096)
    assert cut(C.byref(empty)) == 0 and head(C.byref(empty)) == 0             # nothing launched
    for name in ("param", "grad", "m", "v", "counter"):
        assert step(C.byref(b), **{name: null}) == -1, name
    assert step(C.byref(b), param=C.c_void_p(4100)) == -4                     # GMC_ERR_ALIGN
    assert step(C.byref(b), F=18) == -7                                       # GMC_ERR_UNSUPPORTED
    assert step(C.byref(b), N=50) == -2                                       # more nodes than rows of conv1.weight
    for name in ("gmc_head_loss_f32", "gmc_train_step_loss_f32", "gmc_cut_loss_f32"):
        assert name in hip.SYMBOLS


def test_loss_names_and_the_environment_default(built, monkeypatch):
    hip = built.hip
    monkeypatch.delenv(hip.LOSS_ENV, raising=False)
    assert hip.LOSS_ENV == "GCN_MAXCUT_LOSS"
    assert (hip.loss_kind(None), hip.loss_kind("cut"), hip.loss_kind("expected_cut")) == (0, 0, 1)
    assert hip.loss_name(None) == "cut"
    monkeypatch.setenv(hip.LOSS_ENV, "expected_cut")
    assert hip.loss_kind(None) == 1 and hip.loss_name(None) == "expected_cut" and hip.loss_kind("cut") == 0
    monkeypatch.setenv(hip.LOSS_ENV, "")
    assert hip.loss_name(None) == "cut"
    for bad in ("soft", "CUT", 1, ""):
        with pytest.raises(ValueError):
            hip.loss_kind(bad)
    monkeypatch.setenv(hip.LOSS_ENV, "relaxed")
    with pytest.raises(ValueError):
        hip.loss_kind(None)
    assert hip.loss_kind("cut") == 0


class RecordingEngine:
    """CPU stand-in with the engine surface the trainer's data-parallel sequence uses; records the keywords it gets."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.count = 8
        self.grad = torch.zeros(self.count + 4)
        self.calls = []

    def make_batch(self, handles, values=None):
        return types.SimpleNamespace(B=len(handles), R=sum(h.n for h in handles))

    def train_fwd_bwd(self, batch, C_=1.0, out=None, **kw):
        self.calls.append(kw)
        out[2][:batch.B] = -1.0
        self.grad[self.count] = -float(batch.B)

    def allreduce_grad(self):
        pass

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8):
        pass


def test_trainer_hands_the_loss_to_the_engine_only_when_it_is_not_the_default(built, monkeypatch):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.delenv(built.hip.LOSS_ENV, raising=False)
    ds = util.product_dataset([(30, 5, 1), (40, 7, 3)])
    assert len(ds) == 2
    cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=16)
    net = types.SimpleNamespace(dropout_frac=0.0, training=True)
    for loss, want in ((None, {}), ("cut", {}), ("expected_cut", {"loss": "expected_cut"})):
        eng = RecordingEngine()
        tr = T.FusedTrainer(net, None, cfg, graphs_per_step=1, engine=eng, loss=loss)
        assert tr.loss == (loss or "cut")
        assert tr.epoch(ds) == -2.0
        assert eng.calls == [want, want], (loss, eng.calls)
    monkeypatch.setenv(built.hip.LOSS_ENV, "expected_cut")
    assert T.FusedTrainer(net, None, cfg, engine=RecordingEngine()).loss == "expected_cut"
    with pytest.raises(ValueError):
        T.FusedTrainer(net, None, cfg, engine=RecordingEngine(), loss="hinge")


def test_trainer_for_rebuilds_when_the_loss_changes(built, monkeypatch):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.delenv(built.hip.LOSS_ENV, raising=False)
    eng = RecordingEngine()
    net = types.SimpleNamespace(engine=lambda: eng, train=lambda: None)
    opt, cfg = object(), T.TrainingConfig(n_nodes=1000, hidden_dim=16)
    a = T._trainer_for(net, opt, cfg)
    assert a.loss == "cut" and T._trainer_for(net, opt, cfg, loss="cut") is a and T._trainer_for(net, opt, cfg, 1) is a
    b = T._trainer_for(net, opt, cfg, loss="expected_cut")
    assert b is not a and b.loss == "expected_cut" and net._fused_trainer is b
    assert T._trainer_for(net, opt, cfg, loss="expected_cut") is b
    monkeypatch.setenv(built.hip.LOSS_ENV, "expected_cut")
    assert T._trainer_for(net, opt, cfg) is b                 # None reads the environment
    monkeypatch.delenv(built.hip.LOSS_ENV)
    assert T._trainer_for(net, opt, cfg).loss == "cut"
    with pytest.raises(ValueError):
        T._trainer_for(net, opt, cfg, loss="soft")
    with pytest.raises(ValueError):
        T.train_single_epoch({}, net, opt, None, cfg, loss="soft")
    with pytest.raises(ValueError):
        T.evaluate_model(net, {}, cfg, loss="soft")
    assert "loss" not in T.TrainingConfig.__dataclass_fields__
