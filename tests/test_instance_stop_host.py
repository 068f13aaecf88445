"""CPU checks of per-graph early stopping for one model per graph (gmc_inst_early_stop_f32, gmc_inst_adam_f32,
InstanceEngine.subset, solve_dataset(early_stopping=True)): the restatement of the rule (tests/instance_stop_ref.py)
against a literal transcription of the reference's loop on made-up loss sequences, the status codes of both entry
points in the documented order (fake pointers: no call reaches a launch), and solve_dataset's loop with a stub engine."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import instance_ref as IR
from tests import instance_stop_ref as SR
from tests import test_api_status as A
from tests import util

SOME, ODD = A.SOME, A.ODD
ALL = [(tol, pat, seq) for (tol, pat), seqs in SR.SEQUENCES.items() for seq in seqs]


# ---- the rule against the reference's loop
@pytest.mark.parametrize("tol,pat,seq", ALL, ids=[s.name for _t, _p, s in ALL])
def test_rule_against_the_literal_loop(tol, pat, seq):
    assert len(seq.losses) == SR.EPOCHS
    stopped, best_loss, best_epoch, counter, prev = SR.reference_loop(seq.losses, tol, pat)
    assert stopped == seq.stop and best_epoch == seq.best_epoch and best_loss == seq.best_loss     # what the table says
    n = 5
    rule = SR.StopRule([0, n], tol, pat)
    for e, L in enumerate(seq.losses):
        before = rule.state()
        was_stopped = rule.stop_epoch[0] >= 0
        rule.update(np.full(n, 10 + e, np.int32), [L], e)
        if was_stopped:
            assert rule.state() == before, e               # a stopped graph: nothing is written, whatever its loss
        # the loop over the first e + 1 losses
        want = SR.reference_loop(seq.losses[:e + 1], tol, pat)
        assert (int(rule.stop_epoch[0]) if rule.stop_epoch[0] >= 0 else None) == want[0], e
        assert float(rule.best_loss[0]) == want[1] and int(rule.best_epoch[0]) == want[2], e
        assert int(rule.stall[0]) == want[3], e
        assert float(rule.prev_loss[0]) == want[4] or (math.isnan(want[4]) and math.isnan(rule.prev_loss[0])), e
        assert rule.best_S.tolist() == [10 + want[2] if want[2] >= 0 else 0] * n, e
    assert SR.replay(seq.losses, tol, pat) == (seq.stop, seq.best_loss, seq.best_epoch)
    assert rule.prev_loss.dtype == np.float32 and rule.stall.dtype == np.int32 and rule.stop_epoch.dtype == np.int32


def test_the_sequences_cover_what_they_promise():
    names = [s.name for _t, _p, s in ALL]
    assert len(names) == len(set(names)) == 12
    stops = [s.stop for _t, _p, s in ALL]
    assert None in stops and len({s for s in stops if s is not None}) >= 4
    exact = next(s for _t, _p, s in ALL if "exactly" in s.name)
    a, b = np.float32(exact.losses[0]), np.float32(exact.losses[1])
    assert float(a) - float(b) == 0.25 and float(a) == exact.losses[0] and float(b) == exact.losses[1]
    low = next(s for _t, _p, s in ALL if "stop epoch" in s.name)
    assert np.float32(low.losses[low.stop]) < np.float32(low.best_loss)       # lower at the stop epoch, and not the best
    later = next(s for _t, _p, s in ALL if "later" in s.name)
    assert min(later.losses[later.stop:]) < later.best_loss


def test_a_batch_is_its_graphs_one_by_one():
    for (tol, pat), seqs in SR.SEQUENCES.items():
        sizes = [3 + 2 * i for i in range(len(seqs))]
        goff = np.concatenate([[0], np.cumsum(sizes)])
        rule = SR.StopRule(goff, tol, pat)
        for e in range(SR.EPOCHS):
            rule.update(np.full(goff[-1], e, np.int32), [s.losses[e] for s in seqs], e)
        for g, s in enumerate(seqs):
            assert (int(rule.stop_epoch[g]) if rule.stop_epoch[g] >= 0 else None) == s.stop, s.name
            assert float(rule.best_loss[g]) == s.best_loss and int(rule.best_epoch[g]) == s.best_epoch, s.name
            assert rule.best_S[goff[g]:goff[g + 1]].tolist() == [s.best_epoch] * sizes[g], s.name


def test_segments_tile_the_flat_buffer_and_masked_adam_passes_stopped_graphs_by():
    sizes, F, K = [5, 9, 4], 8, 3
    segs = SR.segments(sizes, F, K)
    count = IR.flat_offsets(sizes, F, K)[-1]
    assert sorted(np.concatenate(segs).tolist()) == list(range(count))
    assert [len(s) for s in segs] == [n * F + F + F * K + K for n in sizes]
    rng = np.random.RandomState(0)
    p, g, m, v = rng.randn(count), rng.randn(count), rng.randn(count) * 0.1, rng.rand(count) * 0.01
    g[segs[1]] = np.nan
    p1, m1, v1 = SR.adam_f64_masked(sizes, F, K, p, g, m, v, 3, 1e-2, [False, True, False])
    assert np.array_equal(p1[segs[1]], p[segs[1]]) and np.array_equal(m1[segs[1]], m[segs[1]])
    assert np.array_equal(v1[segs[1]], v[segs[1]]) and np.isfinite(p1).all()
    for s in (segs[0], segs[2]):
        mm, vv, upd = IR.adam_f64(m[s], v[s], g[s], 3, 1e-2)
        assert np.array_equal(m1[s], mm) and np.array_equal(v1[s], vv) and np.array_equal(p1[s], p[s] + upd)


# ---- status codes (fake pointers: no call reaches a launch)
def test_status_codes_of_the_early_stop_entry_point(built):
    hip = built.hip
    lib = hip.load()
    bf = A.batch_fields(n=100, B=6)

    def stop(batch=bf, tolerance=1e-4, patience=20, **a):
        g = {**dict(S=SOME, loss=SOME, prev_loss=SOME, stall=SOME, stop_epoch=SOME, best_S=SOME, best_loss=SOME,
                    best_epoch=SOME), **a}
        bb = None if batch is None else C.byref(hip.GmcBatch(**batch))
        return lib.gmc_inst_early_stop_f32(bb, g["S"], g["loss"], 3, tolerance, patience, g["prev_loss"], g["stall"],
                                           g["stop_epoch"], g["best_S"], g["best_loss"], g["best_epoch"], None)

    assert stop(batch=None) == -1 and stop(batch={**bf, "abi": 100}) == -8 and stop(batch={**bf, "goff": None}) == -1
    assert stop(batch={**bf, "abi": 100, "goff": None}) == -8                   # (abi before any other field)
    for f in ("S", "loss", "prev_loss", "stall", "stop_epoch", "best_S", "best_loss", "best_epoch"):
        assert stop(**{f: None}) == -1, f
        assert stop(**{f: None}, patience=0) == -1, f                           # (NULL before SHAPE)
    assert stop(batch={**bf, "B": -1}) == -2 and stop(batch={**bf, "R": -1}) == -2 and stop(batch={**bf, "n_max": 0}) == -2
    assert stop(patience=0) == -2 and stop(patience=-3) == -2
    assert stop(tolerance=-1e-9) == -2 and stop(tolerance=float("nan")) == -2
    empty = {**bf, "B": 0, "R": 0, "n_max": 0}
    assert stop(batch=empty) == 0 and stop(batch=empty, tolerance=0.0, patience=1) == 0
    assert stop(batch=empty, tolerance=float("inf")) == 0                       # (an infinite tolerance is one)
    assert stop(batch=empty, patience=0) == -2                                  # (checked before B == 0 returns)
    assert "gmc_inst_early_stop_f32" in hip.SYMBOLS


def test_status_codes_of_the_segmented_adam_entry_point(built):
    hip = built.hip
    lib = hip.load()
    bf = A.batch_fields(n=100, B=6)

    def adam(batch=bf, F=32, K=3, step=1, stop_epoch=SOME, **a):
        g = {**dict(param=SOME, grad=SOME, m=SOME, v=SOME), **a}
        bb = None if batch is None else C.byref(hip.GmcBatch(**batch))
        return lib.gmc_inst_adam_f32(bb, F, K, g["param"], g["grad"], g["m"], g["v"], 1e-3, 0.9, 0.999, 1e-8, step,
                                     stop_epoch, None)

    assert adam(batch=None) == -1 and adam(batch={**bf, "abi": 100}) == -8 and adam(batch={**bf, "goff": None}) == -1
    for f in ("param", "grad", "m", "v"):
        assert adam(**{f: None}) == -1, f
        assert adam(**{f: None}, step=0) == -1, f                               # (NULL before SHAPE)
        assert adam(**{f: ODD}) == -4, f
        assert adam(**{f: ODD}, step=0) == -2, f                                # (SHAPE before ALIGN)
    assert adam(batch={**bf, "B": -1}) == -2 and adam(batch={**bf, "R": -1}) == -2 and adam(batch={**bf, "n_max": 0}) == -2
    assert adam(step=0) == -2 and adam(F=0) == -2 and adam(F=-4) == -2 and adam(K=0) == -2
    assert adam(F=30) == -4 and adam(F=1) == -4
    empty = {**bf, "B": 0, "R": 0, "n_max": 0}
    assert adam(batch=empty) == 0 and adam(batch=empty, stop_epoch=None) == 0   # launches nothing; the mask is optional
    assert adam(batch=empty, F=30) == -4
    assert "gmc_inst_adam_f32" in hip.SYMBOLS
    assert hip.INST_ADAM_TILE_FLOATS == 4096
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define GMC_INST_ADAM_TILE_FLOATS 4096" in open(os.path.join(root, "include", "gcnmaxcut.h")).read()
    names = util.kernel_symbols(hip.LIB_PATH)
    for kernel in ("inst_adam_kernel", "stop_rows_kernel", "stop_state_kernel", "keep_rows_kernel", "keep_loss_kernel"):
        assert any(kernel in s for s in names), kernel


# ---- solve_dataset(early_stopping=True) with a stub engine
class StubStopEngine:
    """What solve_dataset asks of an InstanceEngine, on the CPU.  Graph g's loss in epoch e is -min(e, n_g % 7): it
    improves for n_g % 7 epochs and is flat from then on, whatever batch the graph stands in.  The partition of epoch e
    is e everywhere but on the terminals; a graph's "parameters" count the Adam steps it has taken."""
    made = []

    def __init__(self, handles, F, K, device=None, *, values=None):
        self.handles = list(handles)
        self.sizes = [h.n for h in self.handles]
        self.F, self.K, self.B, self.R = F, K, len(handles), sum(self.sizes)
        self.device = torch.device("cpu")
        self.values, self.steps, self.reset, self.forwards, self.subsets, self.reads = values, 0, 0, 0, 0, 0
        self.rule = None
        self.updates = np.zeros(self.B, np.int64)
        self.plain = IR.KeepBest(self._goff())
        StubStopEngine.made.append(self)

    def _goff(self):
        return np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)

    def reset_parameters(self):
        self.reset += 1

    def _S(self, e):
        S = torch.full((self.R,), e, dtype=torch.int32)
        for off in self._goff()[:-1]:
            S[off:off + self.K] = torch.arange(self.K, dtype=torch.int32)
        return S

    def train_fwd_bwd(self, C_, loss="cut"):
        e = self.steps
        losses = torch.tensor([-min(e, n % 7) * C_ for n in self.sizes], dtype=torch.float32)
        return torch.full((self.R, self.K), 1.0 / self.K), self._S(e), losses

    def forward(self, C_, loss="cut"):
        self.forwards += 1
        P = torch.cat([torch.full((n, self.K), float(u)) for n, u in zip(self.sizes, self.updates)])
        return P, self._S(self.steps), torch.zeros(self.B)

    def adam_step(self, lr, running_only=False):
        self.steps += 1
        self.lr = lr
        running = np.ones(self.B, bool) if not (running_only and self.rule) else self.rule.stop_epoch < 0
        self.updates += running
        self.running_only = running_only

    def keep_best(self, S, losses, epoch):
        self.plain.update(S.numpy(), losses.numpy(), epoch)

    def early_stop(self, S, losses, epoch, tolerance, patience):
        assert epoch == self.steps - 1
        if self.rule is None:
            self.rule = SR.StopRule(self._goff(), tolerance, patience)
        assert (self.rule.tolerance, self.rule.patience) == (tolerance, patience)
        self.rule.update(S.numpy(), losses.numpy(), epoch)

    def stopped(self):
        self.reads += 1
        return torch.from_numpy((self.rule.stop_epoch if self.rule else np.full(self.B, -1, np.int32)).copy())

    def subset(self, keep):
        made = StubStopEngine.made
        sub = StubStopEngine([self.handles[g] for g in keep], self.F, self.K,
                             values=None if self.values is None else [self.values[g] for g in keep])
        assert made[-1] is sub
        self.subsets += 1
        sub.steps, sub.updates, sub.reset = self.steps, self.updates[list(keep)].copy(), self.reset
        sub.rule = SR.StopRule(sub._goff(), self.rule.tolerance, self.rule.patience)
        go = self._goff()
        for j, g in enumerate(keep):
            for name in ("prev_loss", "stall", "stop_epoch", "best_loss", "best_epoch"):
                getattr(sub.rule, name)[j] = getattr(self.rule, name)[g]
            sub.rule.best_S[sub._goff()[j]:sub._goff()[j + 1]] = self.rule.best_S[go[g]:go[g + 1]]
        return sub

    def _kept(self):
        return self.rule if self.rule is not None else self.plain

    best_S = property(lambda self: torch.from_numpy(self._kept().best_S))
    best_loss = property(lambda self: torch.from_numpy(self._kept().best_loss))
    best_epoch = property(lambda self: torch.from_numpy(self._kept().best_epoch))

    def parameters(self):
        return [{"conv1.weight": torch.zeros(n, self.F), "conv1.bias": torch.full((self.F,), float(u)),
                 "conv2.weight": torch.zeros(self.F, self.K), "conv2.bias": torch.zeros(self.K)}
                for n, u in zip(self.sizes, self.updates)]


KEYS_DEFAULT = ["best_loss", "best_epoch", "partition", "cut", "probabilities", "loss_history", "model"]
SIZES = [40, 30, 10, 50, 6, 23]                      # n % 7 = 5, 2, 3, 1, 6, 2
PATIENCE, EPOCHS = 3, 12


def plain(res):
    """A result without its callable, with tensors as lists."""
    return {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in res.items() if k != "model"}


@pytest.fixture
def stubbed(built, monkeypatch):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.setattr(T, "InstanceEngine", StubStopEngine)
    monkeypatch.setattr(T, "module_of", lambda params: params)
    monkeypatch.delenv("GCN_MAXCUT_LOSS", raising=False)
    monkeypatch.delenv("GCN_MAXCUT_LAYER1", raising=False)
    StubStopEngine.made = []
    ds = {}
    for i, n in enumerate(SIZES):
        g = util.near_regular(n, 3, i)
        ds[i] = [built.from_networkx(g), None, g, [0, 1, 2]]
    cfg = T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=3, number_epochs=EPOCHS, learning_rate=0.01, C=2.0,
                           patience=PATIENCE, tolerance=1e-4)
    return T, ds, cfg


def test_solve_dataset_with_early_stopping_and_a_stub_engine(stubbed):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    T, ds, cfg = stubbed
    out = T.solve_dataset(ds, cfg, early_stopping=True, check_every=1, compact_fraction=0.25, max_rows_per_chunk=90)
    made = StubStopEngine.made
    assert all(e.values == [None] * e.B and e.lr == 0.01 and e.running_only for e in made if e.steps)
    # chunk 1: graph 1 (n % 7 = 2) stops at epoch 2 + 3 and holds 30 of 80 rows: one rebuild over [40, 10]; graph 2 stops
    # at 6 with 10 of 50 rows (below a quarter: it rides on), graph 0 at 8 - then all have stopped and the chunk ends
    assert [e.sizes for e in made] == [[40, 30, 10], [40, 10], [50, 6, 23], [6, 23], [6]]
    assert made[0].subsets == 1 and made[1].subsets == 0 and made[1].steps == 9       # the loop left at epoch 8's check
    assert made[4].steps == 10                                                        # graph 4: stopped at 9, seen at 10
    assert all(e.reset == 1 for e in made) and len(out) == len(SIZES)
    for n, res, item in zip(SIZES, out, ds.values()):
        stop = n % 7 + PATIENCE
        assert list(res) == KEYS_DEFAULT + ["stopped_epoch"]
        assert res["stopped_epoch"] == stop
        assert res["loss_history"] == [-min(e, n % 7) * 2.0 for e in range(stop + 1)]
        assert SR.replay(res["loss_history"], 1e-4, PATIENCE) == (stop, res["best_loss"], res["best_epoch"])
        assert res["best_epoch"] == n % 7 and res["best_loss"] == -(n % 7) * 2.0
        assert res["partition"] == [0, 1, 2] + [n % 7] * (n - 3)
        assert res["cut"] == TN.calculate_cut_value(res["partition"], item[2])
        # frozen at the stop: stop + 1 updates, and the probabilities are the forward of those parameters
        assert res["model"]()["conv1.bias"].tolist() == [float(stop + 1)] * 8
        assert tuple(res["probabilities"].shape) == (n, 3) and res["probabilities"].unique().tolist() == [float(stop + 1)]


def test_results_do_not_depend_on_checks_compaction_or_chunks(stubbed):
    T, ds, cfg = stubbed
    want = [plain(r) for r in T.solve_dataset(ds, cfg, early_stopping=True, check_every=1)]
    for kw in (dict(check_every=0), dict(check_every=3), dict(check_every=1, compact_fraction=0.0),
               dict(check_every=3, compact_fraction=1.0), dict(check_every=1, max_rows_per_chunk=50),
               dict(check_every=0, max_rows_per_chunk=1)):
        StubStopEngine.made = []
        got = T.solve_dataset(ds, cfg, early_stopping=True, **kw)
        assert [plain(r) for r in got] == want, kw
        if kw["check_every"] == 0:
            assert all(e.subsets == 0 and e.steps == EPOCHS and e.reads == 1 for e in StubStopEngine.made), kw
        assert [r["model"]()["conv1.bias"][0].item() for r in got] == [float(n % 7 + PATIENCE + 1) for n in SIZES]
    # a graph that runs to the end: stopped_epoch None, the whole history
    long_cfg = T.TrainingConfig(**{**cfg.__dict__, "number_epochs": 6})
    got = T.solve_dataset(ds, long_cfg, early_stopping=True, check_every=2)
    assert [r["stopped_epoch"] for r in got] == [None, 5, None, 4, None, 5]
    assert [len(r["loss_history"]) for r in got] == [6, 6, 6, 5, 6, 6]
    assert T.solve_dataset({}, cfg, early_stopping=True) == []
    with pytest.raises(ValueError, match="check_every"):
        T.solve_dataset(ds, cfg, early_stopping=True, check_every=-1)


def test_the_default_call_is_unchanged(stubbed):
    T, ds, cfg = stubbed
    defaults = {k: p.default for k, p in inspect.signature(T.solve_dataset).parameters.items() if k != "dataset"}
    assert defaults["early_stopping"] is False and (defaults["check_every"], defaults["compact_fraction"]) == (64, 0.25)
    out = T.solve_dataset(ds, cfg)
    assert all(list(r) == KEYS_DEFAULT for r in out)                                  # no stopped_epoch key
    assert all(len(r["loss_history"]) == EPOCHS for r in out)                         # patience ignored
    (eng,) = StubStopEngine.made
    assert eng.steps == EPOCHS and eng.rule is None and eng.running_only is False and eng.reads == eng.forwards == 0
