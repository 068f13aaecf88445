"""The library calls of the Python decoder layer (``Testing/TestingNeuralNetwork.py``), without a GPU or the library.

Every device wrapper is run on a stub batch with ``hip.load`` replaced by a recorder: each case leaves the sequence of
entry points it called with every argument (a tensor as dtype and shape), the ``refine_order`` / ``refine_classes`` it
asked the batch for, and what it returned or raised.  ``tests/golden/decoder_calls.json`` holds those records as the
tree BEFORE the wrappers were unified made them (:func:`record` run with a table naming that tree's functions, the
large route's wrappers among them); the wrappers of this tree have to make the same calls, symbol by symbol and
argument by argument.  :func:`table` is all that names a wrapper, so one recorder serves both trees.
"""
import json
import os
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_calls.json")
K, CANDS, SAMPLES, SWEEPS = 3, 3, 4, 2
BATCHES = {"two": (4, 5), "empty": ()}


def table(T):
    """operation -> callable; a case calls ``table[op](batch, *args, **keywords)``."""
    return {"round": T._round_on_gpu, "sample": T._kway_sample_on_gpu, "anneal": T._kway_anneal_on_gpu,
            "tabu": T._kway_tabu_on_gpu, "balance": T._kway_balance_on_gpu, "evolve": T._kway_evolve_on_gpu,
            "refine3": T._refine_on_gpu, "anneal3": T._anneal_on_gpu, "sample3": T._sample_on_gpu,
            "plain_argmax": T._plain_argmax}


def _plain(a):
    if a is None or isinstance(a, (str, list)):
        return a
    if isinstance(a, (bool, np.bool_)):
        return bool(a)
    if isinstance(a, (int, np.integer)):
        return int(a)
    raise TypeError(f"an argument the recorder does not know: {a!r}")


class Ptr(list):
    """What the stub of ``hip.ptr`` returns: ["ptr", dtype, shape], and the tensor it was asked for."""
    tensor = None


def _shape(t, passed):
    """A returned tensor as dtype, shape and where it was handed to the library ([call, argument], or None)."""
    if t is None:
        return None
    if isinstance(t, (tuple, list)):
        return [_shape(x, passed) for x in t]
    return [str(t.dtype), list(t.shape), passed.get(id(t))]


class Recorder:
    """Stands for the loaded library: every attribute is an entry point that records its call and succeeds."""

    def __init__(self):
        self.calls, self.passed, self.alive = [], {}, []

    def __getattr__(self, symbol):
        def entry(*args):
            for i, a in enumerate(args):
                if isinstance(a, Ptr):
                    self.passed[id(a.tensor)] = [len(self.calls), i]
                    self.alive.append(a.tensor)   # (an id is only unique among live objects)
            self.calls.append([symbol, [_plain(a) for a in args]])
            return 64 if symbol.endswith("_workspace_bytes") else 0
        return entry


def _ptr(t):
    if t is None:
        return None
    assert t.is_contiguous(), "hip.ptr refuses a tensor that is not contiguous"
    p = Ptr(["ptr", str(t.dtype), list(t.shape)])
    p.tensor = t
    return p


def stub_batch(pkg, sizes, rec):
    batch = pkg.GraphBatch.__new__(pkg.GraphBatch)
    batch.B, batch.R, batch.device = len(sizes), int(sum(sizes)), torch.device("cpu")
    batch.sizes = np.asarray(sizes, np.int64)
    batch.host = types.SimpleNamespace(vals=None)
    batch.ref = lambda: "batch"
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    order = (i32(max(batch.R, 1)), i32(batch.B + 1), i32(max(batch.B, 1)))

    def refine_order(K=3, terminals=True):
        rec.calls.append(["batch.refine_order", [int(K), bool(terminals)]])
        return order

    def refine_classes(K=3, terminals=True):
        rec.calls.append(["batch.refine_classes", [int(K), bool(terminals)]])
        return 2
    batch.refine_order, batch.refine_classes = refine_order, refine_classes
    return batch


def cases():
    """name -> (batch, operation, arguments after the batch as a function of (T, R, B), keywords)."""
    P = lambda T, R, B: torch.full((R, K), 1.0 / K)
    cands = lambda T, R, B: torch.zeros((CANDS, R), dtype=torch.int8)
    cost = lambda R: torch.zeros((R, K))
    bounds = lambda B: (np.zeros((B, K), np.int32), np.full((B, K), 9, np.int32))
    ops = {
        "round": lambda T, R, B: (P(T, R, B), 1),
        "sample": lambda T, R, B: (P(T, R, B), SAMPLES, 7, None, True),
        "anneal": lambda T, R, B: (K, cands(T, R, B), T.anneal_schedule(SWEEPS), -3, 5),
    }
    chains = {
        "tabu": lambda T, R, B: (K, cands(T, R, B), 6, T.TABU_TENURE, -3),
        "balance": lambda T, R, B: (K, cands(T, R, B), *bounds(B), 6, T.TABU_TENURE, -3),
    }
    out = {}
    for b in BATCHES:
        for op, args in ops.items():
            for terminals in (True, False):
                for with_cost in (False, True):
                    out[f"{b}-{op}-small-t{int(terminals)}-c{int(with_cost)}"] = (
                        b, op, args, lambda R, t=terminals, c=with_cost: {"terminals": t, "node_cost": cost(R) if c else None})
                out[f"{b}-{op}-large-t{int(terminals)}"] = (b, op, args, lambda R, t=terminals: {"terminals": t, "large": True})
                if op != "round":
                    out[f"{b}-{op}-large-t{int(terminals)}-workspace"] = (
                        b, op, args, lambda R, t=terminals: {"terminals": t, "large": True,
                                                             "workspace": torch.empty(128, dtype=torch.uint8)})
        out[f"{b}-sample-small-dropped"] = (b, "sample", lambda T, R, B: (P(T, R, B), SAMPLES, 7, list(range(B)), False),
                                            lambda R: {})
        for op, args in chains.items():
            for terminals in (True, False):
                for with_cost in (False, True):
                    out[f"{b}-{op}-t{int(terminals)}-c{int(with_cost)}"] = (
                        b, op, args, lambda R, t=terminals, c=with_cost: {"terminals": t, "node_cost": cost(R) if c else None})
        out[f"{b}-evolve"] = (b, "evolve", lambda T, R, B: (K, cands(T, R, B), 2, 1, T.anneal_schedule(SWEEPS), -3, 5),
                              lambda R: {})
        out[f"{b}-refine3"] = (b, "refine3", lambda T, R, B: (cands(T, R, B), 5), lambda R: {})
        out[f"{b}-anneal3"] = (b, "anneal3", lambda T, R, B: (cands(T, R, B), T.anneal_schedule(SWEEPS), -3, 5), lambda R: {})
        out[f"{b}-anneal3-no-sweeps"] = (b, "anneal3", lambda T, R, B: (cands(T, R, B), T.anneal_schedule(0), 1, 5),
                                         lambda R: {})
        out[f"{b}-sample3"] = (b, "sample3", lambda T, R, B: (P(T, R, B), SAMPLES), lambda R: {"seed": 7})
        for large in (False, True):
            out[f"{b}-plain_argmax-{'large' if large else 'small'}"] = (b, "plain_argmax", lambda T, R, B: (P(T, R, B), K),
                                                                        lambda R, l=large: {"large": l})
    return out


def record_case(pkg, monkeypatch, operations, case):
    """Runs one case against the recorder; returns {"calls", "returns", "raises"}."""
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    b, op, args, keywords = case
    rec = Recorder()
    monkeypatch.setattr(pkg.hip, "load", lambda: rec)
    monkeypatch.setattr(pkg.hip, "ptr", _ptr)
    monkeypatch.setattr(pkg.hip, "stream", lambda: "stream")

    def no_gpu(*_a, **_k):
        raise AssertionError("a device wrapper asked for the GPU")
    monkeypatch.setattr(pkg.hip, "require_gpu", no_gpu)
    batch = stub_batch(pkg, BATCHES[b], rec)
    returns, raises = None, None
    try:
        returns = _shape(operations[op](batch, *args(T, batch.R, batch.B), **keywords(batch.R)), rec.passed)
    except (ValueError, NotImplementedError, RuntimeError) as e:
        raises = [type(e).__name__, str(e)]
    return {"calls": rec.calls, "returns": returns, "raises": raises}


def record(operations):
    """Every case's record, as the fixture holds them."""
    import gcn_max_cut_amd as pkg
    with pytest.MonkeyPatch.context() as mp:
        return {name: record_case(pkg, mp, operations, case) for name, case in cases().items()}


with open(GOLDEN) as f:
    RECORDED = json.load(f)


def test_every_recorded_case_is_compared():
    assert sorted(RECORDED) == sorted(cases())
    symbols = {c[0] for r in RECORDED.values() for c in r["calls"]}
    for family in ("gmc_round_conditional", "gmc_kway_decode_sample_seeded", "gmc_kway_refine_anneal"):
        assert {family + "_f32", family + "_t_f32", family + "_c_f32"} <= symbols
    for family in ("gmc_large_round_conditional", "gmc_large_sample_seeded", "gmc_large_anneal"):
        assert {family + "_f32", family + "_t_f32"} <= symbols
    assert {"gmc_kway_tabu_f32", "gmc_kway_tabu_c_f32", "gmc_kway_balance_f32", "gmc_kway_balance_c_f32",
            "gmc_kway_evolve_f32", "gmc_refine_local_f32", "gmc_refine_anneal_f32", "gmc_decode_sample_seeded_f32",
            "gmc_large_round_workspace_bytes", "gmc_large_search_workspace_bytes"} <= symbols


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_the_calls_are_the_recorded_ones(name, monkeypatch):
    import gcn_max_cut_amd as pkg
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    got = json.loads(json.dumps(record_case(pkg, monkeypatch, table(T), cases()[name])))
    want = RECORDED[name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for have, expect in zip(got["calls"], want["calls"]):
        assert have == expect
    assert got["raises"] == want["raises"]
    assert got["returns"] == want["returns"]


@pytest.mark.parametrize("b", sorted(BATCHES))
@pytest.mark.parametrize("op", ["round", "sample", "anneal"])
def test_large_with_a_node_cost_is_refused(b, op, monkeypatch):
    import gcn_max_cut_amd as pkg
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    _, _, args, _ = cases()[f"{b}-{op}-large-t1"]
    case = (b, op, args, lambda R: {"large": True, "node_cost": torch.zeros((R, K))})
    got = record_case(pkg, monkeypatch, table(T), case)
    assert got["raises"] is not None and got["raises"][0] == "NotImplementedError"
    assert got["calls"] == [] and got["returns"] is None
