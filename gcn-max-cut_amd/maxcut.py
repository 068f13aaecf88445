"""Plain max-K-cut from the tensors a GNN user holds: ``solve(edge_index, ptr, ...)``.

The tensor-first front door of the instance-wise solver.  One call builds the batch on the GPU
(``GraphBatch.from_edge_index``), gives every graph its own model and trains them all at once
(``engine.InstanceEngine``: train / Adam / keep_best, ``epochs`` times), and decodes with one rounding, one sampler and
one annealing launch (the ``_t`` entry points of include/gcnmaxcut.h).  By default there are no terminals: this is the
max-cut of Gset and the max-cut papers, not the reference's variant with nodes 0..K-1 forced apart; ``terminals=True``
gives that one.  No ``networkx`` graph and no dataset item is involved.

``node_cost`` adds a linear term per node and class to the objective, and two more doors map the
QUBO family onto it exactly: :func:`solve_ising` and :func:`solve_qubo`.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from . import hip
from .engine import InstanceEngine, LargeInstanceEngine, instance_too_large
from .graph import GraphBatch, _check_pins, _host_array


_TOO_LARGE = ("a graph of {n} nodes is beyond the one-workgroup head of the per-graph models (number_classes = {K}): "
              "train a model through gcn_max_cut_amd.functional (terminal-free up to 2^20 nodes) and decode it with "
              "search_large_dataset(..., terminals=False), or call maxcut.solve_large, which trains one model per graph up "
              "to 2^20 nodes")
_NO_TABU = "the tabu stage keeps a graph's state in one workgroup: solve_large does not have it (tabu_iterations must be 0)"
_NO_BALANCE = ("the balanced stage keeps a graph's state in one workgroup, as the tabu stage does: solve_large does not "
               "have it (class_sizes must be None)")
_BATCH_DOOR = "this door does not take the two together; solve_batch(GraphBatch.from_edge_index(...), ...), which it wraps, does"
_NO_COST_TABU = "node_cost with tabu_iterations > 0: " + _BATCH_DOOR + " - its tabu stage follows the objective"
_NO_COST_SIZES = "node_cost with class_sizes: " + _BATCH_DOOR + " - its balanced stage follows the objective"
_NO_COST_FIXED = ("node_cost with fixed: " + _BATCH_DOOR + " - it carries the free nodes' costs to the contracted batch and "
                  "reports the pinned nodes' as fixed_cost")
_NO_COST_LARGE = ("node_cost on the large route: the multi-workgroup head and decoders of solve_large take no per-node "
                  "costs - maxcut.solve has them for graphs within its bound")
_NO_TEMPER = ("the tempering stage keeps a graph's state in one workgroup, as the tabu stage does: solve_large does not have "
              "it (tempering_rounds must be 0)")
_TEMPER_ALONE = ("tempering_rounds > 0 together with {other}: the tempering stage is not combined with the tabu or the "
                 "balanced stage - pass one of tempering_rounds and {other}")
_BEYOND_LARGE = "a graph of {n} nodes is beyond the {bound} nodes of the per-graph models' large sequence (solve_large)"


@dataclass
class MaxCutResult:
    """What :func:`solve` returns: device tensors, graph g owning rows ``ptr[g] .. ptr[g+1]-1`` of ``partition``."""
    partition: torch.Tensor     # [R] int32: the class of every node
    cut: torch.Tensor           # [B] float32: the cut of ``partition``
    trained_cut: torch.Tensor   # [B] float32: the cut of the best partition training saw (``best_S``)
    rounded_cut: torch.Tensor   # [B] float32: the cut of the conditional rounding of the last P
    ptr: torch.Tensor           # [B + 1] int32
    annealed_cut: Optional[torch.Tensor] = None   # [B] float32, with tabu_iterations > 0 or tempering_rounds > 0 only: the
    #                                               cut the annealing reached
    fixed_cut: Optional[torch.Tensor] = None      # [B] float32, with fixed only: the weight of the edges between pinned
    #                                               nodes of different classes (a constant of every partition)
    unconstrained_cut: Optional[torch.Tensor] = None   # [B] float32, with class_sizes only: what ``cut`` would have been
    node_cost_sum: Optional[torch.Tensor] = None   # [B] float32, with node_cost only: sum_v node_cost[v][partition_v]; every
    #                                                ``*_cut`` field then holds the objective cut - cost of its partition,
    #                                                and the plain cut of ``partition`` is ``cut + node_cost_sum``
    fixed_cost: Optional[torch.Tensor] = None      # [B] float32, with fixed and node_cost only: the cost of the pinned nodes,
    #                                                sum_v node_cost[v][class_v] (a constant of every partition)


def _classes(number_classes) -> int:
    K = int(number_classes)
    if not 2 <= K <= hip.KWAY_MAX_CLASSES:
        raise ValueError(f"number_classes must be in 2..{hip.KWAY_MAX_CLASSES}, got {K}")
    return K


def balanced_sizes(ptr, number_classes: int, imbalance: float = 0.0):
    """``class_sizes`` for :func:`solve` from the graphs' sizes: ``(lo, hi)``, int32 numpy arrays [B, K] with
    ``lo = floor((1 - imbalance) * n / K)`` and ``hi = ceil((1 + imbalance) * n / K)`` for every class of a graph of n
    nodes (``ptr`` [B + 1] as :func:`solve` takes it).  ``imbalance = 0``: ``"balanced"``.  The products are taken in
    float64 and a value within 1e-9 of an integer counts as that integer, so 1.03 * 1000 / 2 is 515 and not 516."""
    K = _classes(number_classes)
    if not 0.0 <= float(imbalance) <= 1.0:
        raise ValueError(f"imbalance must be in 0..1, got {imbalance}")
    p = _host_array(ptr)
    if p.ndim != 1 or p.size < 1:
        raise ValueError("ptr must be [B + 1]")
    n = np.diff(p.astype(np.int64)).astype(np.float64)
    lo = np.floor((1.0 - float(imbalance)) * n / K + 1e-9).astype(np.int32)
    hi = np.ceil((1.0 + float(imbalance)) * n / K - 1e-9).astype(np.int32)
    return np.repeat(lo[:, None], K, axis=1), np.repeat(hi[:, None], K, axis=1)


def solve(edge_index, ptr=None, num_nodes: Optional[int] = None, edge_weight=None, *, number_classes: int = 2,
          terminals: bool = False, pairs: str = "both", hidden_dim: int, epochs: int, learning_rate: float,
          loss: str = "expected_cut", samples: int = 32, anneal_sweeps: int = 100, max_descent_sweeps: int = 100,
          seed: int = 0, tabu_iterations: int = 0, fixed=None, class_sizes=None,
          balance_iterations: Optional[int] = None, node_cost=None, tempering_rounds: int = 0,
          tempering_sweeps: int = 4, tempering_rungs: int = 8) -> MaxCutResult:
    """Max-K-cut of every graph of a batch given as ``edge_index`` [2, E] (with ``ptr`` [B+1], or ``num_nodes`` for one
    graph, ``edge_weight`` and ``pairs`` as ``GraphBatch.from_edge_index`` takes them).

    1. the batch, built on the GPU;
    2. one ``GraphConv(n_g, hidden_dim) -> GraphConv(hidden_dim, number_classes)`` model per graph, initialised as the
       reference initialises one (from a generator seeded with ``seed``; torch's global generator is left alone), trained
       together for ``epochs`` steps of train / Adam(``learning_rate``) / keep_best on ``loss``;
    3. one forward for P;
    4. one conditional rounding of P, ``samples`` seeded samples of P and one annealing launch (``anneal_sweeps``
       Metropolis sweeps, then at most ``max_descent_sweeps`` sweeps of the local search) over the candidates: the best
       partition training saw, the rounded one and the samples.  ``cut`` is therefore never below ``trained_cut`` or
       ``rounded_cut``.
    5. with ``tabu_iterations > 0`` only: one call of the tabu stage (``gmc_kway_tabu_f32``,
       ``Testing.kway_tabu_search``; ``tabu_iterations`` iterations per candidate, seeded by ``seed``) on a copy of the
       annealed candidates.  Per graph ``partition`` / ``cut`` are then the better of the annealed and the tabu result
       by their recounted cuts, chosen on the device, and ``annealed_cut`` holds the annealed one: ``cut >=
       annealed_cut``.  The default 0 launches nothing more and leaves ``annealed_cut`` None.
       With ``tempering_rounds > 0`` only, in the tabu stage's place: one call of the tempering stage
       (``gmc_kway_temper_f32``, ``Testing.kway_tempering``: ``tempering_rounds`` rounds of ``tempering_sweeps`` Metropolis
       sweeps on ladders of ``tempering_rungs`` fixed temperatures with replica exchange between the rounds, seeded by
       ``seed``) on a copy of the first ``tempering_rungs * (candidates // tempering_rungs)`` annealed candidates, then
       the local search from every walker's best state.  ``partition`` / ``cut`` and ``annealed_cut`` are chosen and
       filled exactly as for the tabu stage: ``cut >= annealed_cut``.  Fewer candidates (``samples + 2``) than
       ``tempering_rungs`` raise ``ValueError``; together with ``tabu_iterations > 0`` or ``class_sizes`` it raises
       ``NotImplementedError``.  The default 0 launches nothing more and changes no byte of the result.
    6. with ``class_sizes`` only: one call of the balanced stage (``gmc_kway_balance_f32``,
       ``Testing.kway_balanced_search``; ``balance_iterations`` iterations per candidate, ``None``: 20 times the
       largest graph's nodes; seeded by ``seed``) on a copy of the annealed candidates, which it first repairs into the
       bounds.  ``class_sizes`` is ``"balanced"`` (every class ``n // K`` to ``ceil(n / K)`` nodes), or a pair
       ``(lo, hi)`` of [K] or [B, K] integers, e.g. from :func:`balanced_sizes`; a terminal counts for its class.
       ``partition`` / ``cut`` are then this stage's pick - every returned partition is within its bounds - and
       ``unconstrained_cut`` holds what ``cut`` would have been without the keyword, so ``cut`` may be below
       ``trained_cut`` and ``rounded_cut``.  On this path the annealing's temperature is in units of the mean ABSOLUTE
       edge weight (1 when that is 0), so negated weights - balanced minimum cut - go through.  Bounds that admit no
       partition raise ``ValueError`` naming the graph; ``class_sizes`` together with ``fixed`` raises ``ValueError``
       (a contracted super-node stands for many nodes, and node weights are not implemented).  The default ``None``
       launches nothing more and changes no byte of the result.

    ``terminals=False`` (default): no node is fixed.  ``terminals=True``: nodes 0..K-1 of every graph keep classes
    0..K-1, as everywhere else in this package.  The same arguments give the same bytes.

    ``fixed=(nodes, classes)``: any nodes pinned to classes - ``nodes`` [P] global ids as in ``edge_index``, ``classes``
    [P] in 0..K-1, as ``GraphBatch.contract`` takes them; every class needs a pin in every graph.  The pinned nodes are
    contracted on the GPU (``GraphBatch.contract``), the steps above run on the contracted batch with its K super-nodes
    as terminals, and the result is lifted: ``partition`` and ``ptr`` are the original graph's, ``cut``, ``trained_cut``,
    ``rounded_cut`` (and ``annealed_cut``) are recounts of the lifted partitions on the original batch, ``fixed_cut``
    holds the weight of the edges between pinned nodes of different classes, and the size refusal below is judged on
    the contracted sizes: a graph of up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes is taken when enough of it is pinned,
    and its cuts are then recounted by the large decoders' scoring call (the cut order of ``solve_large``; the same
    number for unit and integer weights).  ``fixed`` together with ``terminals=True`` raises ``ValueError``.

    ``node_cost`` [R, K] (numpy or torch, any float dtype; row = global node id, converted to float32 once): the
    objective becomes ``cut(S) - sum_v node_cost[v][S_v]`` - node preferences, external fields, the linear part of a QUBO.
    Training (both losses), the rounding, the sampler's scores and the annealing all follow it (the ``_c`` entry points
    of include/gcnmaxcut.h), every ``*_cut`` field of the result then holds the objective of its partition (what the
    stages compared), and ``node_cost_sum`` holds the cost of ``partition``, so its plain cut is ``cut +
    node_cost_sum``.  A wrong shape or a value that is not finite raises ``ValueError`` before anything is built.
    Through THIS door ``node_cost`` together with ``tabu_iterations > 0``, ``class_sizes`` or ``fixed`` raises
    ``NotImplementedError``; :func:`solve_batch` on ``GraphBatch.from_edge_index(...)``, which this function wraps,
    takes each of the three: the tabu and the balanced stage then follow the objective
    (``gmc_kway_tabu_c_f32``, ``gmc_kway_balance_c_f32``), and pins carry the free nodes' costs to the contracted batch.
    ``None`` changes no byte, and an all-zero array returns the bytes of ``None`` in ``partition`` and ``cut``.

    A graph beyond the one-workgroup head of the per-graph models raises ``ValueError``: for such a graph train a model
    through ``gcn_max_cut_amd.functional`` (terminal-free up to 2^20 nodes) and decode it with
    ``search_large_dataset(..., terminals=False)``."""
    K, terminals = _classes(number_classes), bool(terminals)
    loss = hip.loss_name(loss)
    _check_fixed(fixed, terminals, K)
    _check_sizes(class_sizes, balance_iterations, fixed)
    tempering = _check_tempering(tempering_rounds, tempering_sweeps, tempering_rungs, tabu_iterations, class_sizes, samples)
    if node_cost is not None:
        node_cost = _check_node_cost(node_cost, _rows_of(ptr, num_nodes), K, tabu_iterations, class_sizes, fixed)
    if ptr is not None:   # judged before anything is built: the sizes are all it takes
        p = _host_array(ptr)
        n_max = int(np.diff(p.astype(np.int64)).max()) if p.ndim == 1 and p.size > 1 else 0
        if class_sizes is not None and p.ndim == 1 and p.size > 1:
            _size_bounds(class_sizes, np.diff(p.astype(np.int64)), K, terminals)
    else:
        n_max = int(num_nodes) if num_nodes is not None else 0
        if class_sizes is not None and num_nodes is not None:
            _size_bounds(class_sizes, [n_max], K, terminals)
    if fixed is None and n_max > 0:   # (with pins: the contracted sizes decide)
        _refuse_small(n_max, K, loss)
    batch = GraphBatch.from_edge_index(edge_index, ptr, num_nodes, edge_weight, pairs=pairs)
    if node_cost is not None:   # (checked above, once: no tabu, sizes or pins come with it)
        return _solve_batch(_SMALL, batch, K, terminals, hidden_dim, epochs, learning_rate, loss, samples,
                            anneal_sweeps, max_descent_sweeps, seed, node_cost=node_cost, tempering=tempering)
    return solve_batch(batch, number_classes=K, terminals=terminals, hidden_dim=hidden_dim, epochs=epochs,
                       learning_rate=learning_rate, loss=loss, samples=samples, anneal_sweeps=anneal_sweeps,
                       max_descent_sweeps=max_descent_sweeps, seed=seed, tabu_iterations=tabu_iterations, fixed=fixed,
                       class_sizes=class_sizes, balance_iterations=balance_iterations, tempering_rounds=tempering_rounds,
                       tempering_sweeps=tempering_sweeps, tempering_rungs=tempering_rungs)


def solve_batch(batch: GraphBatch, *, number_classes: int = 2, terminals: bool = False, hidden_dim: int, epochs: int,
                learning_rate: float, loss: str = "expected_cut", samples: int = 32, anneal_sweeps: int = 100,
                max_descent_sweeps: int = 100, seed: int = 0, tabu_iterations: int = 0, fixed=None, class_sizes=None,
                balance_iterations: Optional[int] = None, node_cost=None, tempering_rounds: int = 0,
                tempering_sweeps: int = 4, tempering_rungs: int = 8) -> MaxCutResult:
    """Steps 2 to 6 of :func:`solve` on a ready batch - one built on the device or one built from handles: the batches
    hold the same bytes, so the results do too.  ``fixed``: as :func:`solve`, with row ids of ``batch``;
    ``class_sizes``, ``balance_iterations`` and ``node_cost`` (rows = batch rows): as :func:`solve`.

    ``node_cost`` goes together with each of ``tabu_iterations``, ``class_sizes`` and ``fixed`` here.  The tabu stage
    and the balanced stage then search the objective ``cut - cost`` (``gmc_kway_tabu_c_f32``,
    ``gmc_kway_balance_c_f32``): the better of the annealed and the tabu result is chosen by objective, and
    ``annealed_cut`` and ``unconstrained_cut`` are objectives like every other ``*_cut`` field; ``node_cost_sum`` is the
    cost of the returned ``partition``.  With ``fixed``, a free node's cost row goes to its contracted row, the K
    super-nodes get zero rows, ``fixed_cost`` [B] holds the cost of each graph's pinned nodes, and every reported value
    is a recount of the lifted partition on the original batch with the original cost.  ``tempering_rounds``,
    ``tempering_sweeps`` and ``tempering_rungs``: as :func:`solve`; the stage takes ``node_cost`` and ``fixed``."""
    _check_sizes(class_sizes, balance_iterations, fixed)
    tempering = _check_tempering(tempering_rounds, tempering_sweeps, tempering_rungs, tabu_iterations, class_sizes, samples)
    if node_cost is not None:
        node_cost = _check_node_cost(node_cost, batch.R, int(number_classes))
    return _solve_fixed(_SMALL, batch, fixed, number_classes, terminals, hidden_dim, epochs, learning_rate, loss,
                        samples, anneal_sweeps, max_descent_sweeps, seed, tabu_iterations, class_sizes,
                        balance_iterations, node_cost=node_cost, tempering=tempering)


def solve_large(edge_index, ptr=None, num_nodes: Optional[int] = None, edge_weight=None, *, number_classes: int = 2,
                terminals: bool = False, pairs: str = "both", hidden_dim: int, epochs: int, learning_rate: float,
                loss: str = "expected_cut", samples: int = 32, anneal_sweeps: int = 100, max_descent_sweeps: int = 100,
                seed: int = 0, tabu_iterations: int = 0, fixed=None, class_sizes=None,
                balance_iterations: Optional[int] = None, node_cost=None, tempering_rounds: int = 0,
                tempering_sweeps: int = 4, tempering_rungs: int = 8) -> MaxCutResult:
    """:func:`solve` for graphs of up to ``hip.LARGE_MAX_GRAPH_NODES`` (2^20) nodes: the same arguments, steps and
    result, with ``engine.LargeInstanceEngine`` (gmc_inst_large_*) as the trainer and the large decoders (one rounding,
    one sampler and one annealing call of gmc_large_*_t_f32; several workgroups share a graph).  It takes small graphs
    too - :func:`solve` is the faster route for those; nothing routes from one to the other.  The large decoders issue
    every launch of ``anneal_sweeps`` + ``max_descent_sweeps`` sweeps whether or not the descent has converged, and the
    samples live on the device while they are scored (``samples`` + 2 bytes per node).  Memory while training: about
    16 * hidden_dim bytes per node for parameters, gradient and Adam moments plus 8 * ld for the workspace (ld =
    hidden_dim rounded up to 32): 1.5 KB per node at hidden_dim = 64.  The tabu stage keeps a graph's state in one
    workgroup, so this route does not have it: ``tabu_iterations`` is taken for the sake of one signature and anything
    but 0 raises ``NotImplementedError``.  So are ``class_sizes`` and ``balance_iterations``: the balanced stage is the
    tabu kernel's sibling, and ``class_sizes`` other than ``None`` raises ``NotImplementedError``.  ``node_cost`` other
    than ``None`` raises it too: the large head and decoders take no per-node costs.  And so does
    ``tempering_rounds`` other than 0: the tempering stage is a one-workgroup kernel as well."""
    if node_cost is not None:
        raise NotImplementedError(_NO_COST_LARGE)
    if tempering_rounds:
        raise NotImplementedError(_NO_TEMPER)
    if tabu_iterations:
        raise NotImplementedError(_NO_TABU)
    if class_sizes is not None:
        raise NotImplementedError(_NO_BALANCE)
    K, terminals = _classes(number_classes), bool(terminals)
    loss = hip.loss_name(loss)
    _check_fixed(fixed, terminals, K)
    batch = GraphBatch.from_edge_index(edge_index, ptr, num_nodes, edge_weight, pairs=pairs)
    return solve_large_batch(batch, number_classes=K, terminals=terminals, hidden_dim=hidden_dim, epochs=epochs,
                             learning_rate=learning_rate, loss=loss, samples=samples, anneal_sweeps=anneal_sweeps,
                             max_descent_sweeps=max_descent_sweeps, seed=seed, tabu_iterations=tabu_iterations,
                             fixed=fixed)


def solve_large_batch(batch: GraphBatch, *, number_classes: int = 2, terminals: bool = False, hidden_dim: int,
                      epochs: int, learning_rate: float, loss: str = "expected_cut", samples: int = 32,
                      anneal_sweeps: int = 100, max_descent_sweeps: int = 100, seed: int = 0,
                      tabu_iterations: int = 0, fixed=None, class_sizes=None,
                      balance_iterations: Optional[int] = None, node_cost=None, tempering_rounds: int = 0,
                      tempering_sweeps: int = 4, tempering_rungs: int = 8) -> MaxCutResult:
    """:func:`solve_batch` through ``engine.LargeInstanceEngine`` and the large decoders: steps 2 to 4 of
    :func:`solve_large` on a ready batch (``tabu_iterations``, ``class_sizes``: as :func:`solve_large`; ``fixed``: as
    :func:`solve_batch`; ``node_cost`` and ``tempering_rounds``: as :func:`solve_large`)."""
    if node_cost is not None:
        raise NotImplementedError(_NO_COST_LARGE)
    if tempering_rounds:
        raise NotImplementedError(_NO_TEMPER)
    if class_sizes is not None:
        raise NotImplementedError(_NO_BALANCE)
    return _solve_fixed(_LARGE, batch, fixed, number_classes, terminals, hidden_dim, epochs, learning_rate, loss,
                        samples, anneal_sweeps, max_descent_sweeps, seed, tabu_iterations)


def _check_fixed(fixed, terminals: bool, number_classes: int) -> None:
    """The argument errors of ``fixed``, raised before anything is built."""
    if fixed is None:
        return
    if terminals:
        raise ValueError("fixed pins the nodes it names and terminals=True pins nodes 0..K-1 of every graph: pass one of "
                         "the two (add nodes 0..K-1 to fixed to have both)")
    if not isinstance(fixed, (tuple, list)) or len(fixed) != 2:
        raise ValueError("fixed must be a pair (nodes, classes)")
    _check_pins(fixed[0], fixed[1], number_classes)


def _rows_of(ptr, num_nodes) -> Optional[int]:
    """The batch's row count as ``ptr`` / ``num_nodes`` state it (None when they do not: from_edge_index then raises)."""
    if ptr is not None:
        p = _host_array(ptr)
        return int(p[-1]) if p.ndim == 1 and p.size >= 1 else None
    return None if num_nodes is None else int(num_nodes)


def _check_node_cost(node_cost, rows: Optional[int], K: int, tabu_iterations=0, class_sizes=None, fixed=None) -> torch.Tensor:
    """The argument errors of ``node_cost``, raised before anything is built; returns it as a float32 tensor [R, K]
    (on whatever device it came from: the one conversion)."""
    if isinstance(node_cost, torch.Tensor):
        t = node_cost.detach()
        if not t.is_floating_point():
            raise ValueError(f"node_cost must hold floats, got {t.dtype}")
    else:
        a = np.asarray(node_cost)
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f"node_cost must hold floats, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[1] != K or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"node_cost must be [R, number_classes] = [{'R' if rows is None else rows}, {K}], got "
                         f"{tuple(t.shape)}")
    t = t.to(torch.float32)
    if not bool(torch.isfinite(t).all()):
        raise ValueError("node_cost holds values that are not finite (in float32)")
    if tabu_iterations:
        raise NotImplementedError(_NO_COST_TABU)
    if class_sizes is not None:
        raise NotImplementedError(_NO_COST_SIZES)
    if fixed is not None:
        raise NotImplementedError(_NO_COST_FIXED)
    return t.contiguous()


def _check_sizes(class_sizes, balance_iterations, fixed) -> None:
    """The argument errors of ``class_sizes`` that need no graph, raised before anything is built."""
    if balance_iterations is not None and not 0 <= int(balance_iterations) < 1 << 31:
        raise ValueError(f"balance_iterations must be None or in 0..2^31-1, got {balance_iterations}")
    if class_sizes is not None and fixed is not None:
        raise ValueError("class_sizes with fixed: a contracted super-node stands for many nodes and the balanced stage "
                         "counts nodes, not node weights - pass one of the two")


def _check_tempering(rounds, sweeps, rungs, tabu_iterations=0, class_sizes=None, samples: Optional[int] = None):
    """The argument errors of the tempering keywords, raised before anything is built; returns (rounds, sweeps, rungs),
    or None when the stage is off (``rounds == 0``: the other two are then not looked at)."""
    if not 0 <= int(rounds) < 1 << 20:
        raise ValueError(f"tempering_rounds must be in 0..2^20-1, got {rounds}")
    if not int(rounds):
        return None
    if tabu_iterations:
        raise NotImplementedError(_TEMPER_ALONE.format(other="tabu_iterations > 0"))
    if class_sizes is not None:
        raise NotImplementedError(_TEMPER_ALONE.format(other="class_sizes"))
    if not 1 <= int(rungs) <= hip.TEMPER_MAX_RUNGS:
        raise ValueError(f"tempering_rungs must be in 1..{hip.TEMPER_MAX_RUNGS}, got {rungs}")
    if int(sweeps) < 1 or int(rounds) * int(sweeps) >= 1 << 20:
        raise ValueError(f"tempering_sweeps must be >= 1 and tempering_rounds * tempering_sweeps below 2^20, got {sweeps}")
    if samples is not None and int(samples) >= 0 and int(samples) + 2 < int(rungs):
        raise ValueError(f"the tempering stage needs at least tempering_rungs = {rungs} candidates, and samples + 2 = "
                         f"{int(samples) + 2} are annealed")
    return int(rounds), int(sweeps), int(rungs)


def _size_bounds(class_sizes, sizes, K: int, terminals: bool):
    from .Testing import TestingNeuralNetwork as T
    return T.class_size_bounds("solve", class_sizes, sizes, K, terminals)


def _mean_abs_edge_weight(batch: GraphBatch) -> float:
    """The annealing's temperature scale on the class_sizes path: the mean absolute edge weight, 1 when that is 0."""
    vals = batch.host.vals
    mean = 1.0 if vals is None or len(vals) == 0 else float(np.mean(np.abs(vals), dtype=np.float64))
    return mean if mean > 0 else 1.0


def _solve_fixed(route: "_Route", batch: GraphBatch, fixed, number_classes: int, terminals: bool, *args,
                 node_cost: Optional[torch.Tensor] = None, tempering: Optional[tuple] = None) -> MaxCutResult:
    """:func:`_solve_batch`, or with ``fixed``: contract, solve the contracted batch with its super-nodes as terminals, lift,
    and recount every reported cut on the original batch (the route's annealing call with zero sweeps and no terminals
    moves nothing and scores: the bits every other decoder reports for those bytes).  The route is chosen by the
    contracted sizes, the recount by the original ones: an original graph beyond ``hip.MAX_GRAPH_NODES`` nodes is
    scored by the large sequence's call, the only decoders that take it.  ``node_cost`` (checked, [R, K] float32): the
    free rows' costs go to the contracted batch (``Contraction.contract_cost``), the recount is the annealing's scoring
    call with the ORIGINAL cost on the original batch, and ``fixed_cost`` holds the pinned nodes' share."""
    if fixed is None:
        return _solve_batch(route, batch, number_classes, terminals, *args, node_cost=node_cost, tempering=tempering)
    K = int(number_classes)
    _check_fixed(fixed, bool(terminals), K)
    from .Testing import TestingNeuralNetwork as T
    large = route.large or (bool(batch.B) and batch.n_max > hip.MAX_GRAPH_NODES)   # the recount's route
    if node_cost is not None and large:
        raise NotImplementedError(_NO_COST_LARGE)
    ct = batch.contract(fixed[0], fixed[1], K)
    parts = {}
    cost, fixed_cost = None, None
    if node_cost is not None:
        node_cost = node_cost.to(batch.device)
        cost, fixed_cost = ct.contract_cost(node_cost, batch.goff)
    res = _solve_batch(route, ct.batch, K, True, *args, parts=parts, node_cost=cost, tempering=tempering)
    no_sweeps = np.zeros(0, np.float32)

    def recount(partition):
        return T._kway_anneal_on_gpu(batch, K, partition.to(torch.int8).reshape(1, -1).contiguous(), no_sweeps, 0, 0, False,
                                     node_cost, large=large)[1]

    partition = ct.lift(res.partition)
    cuts, cost_sum = (res.cut, res.trained_cut, res.rounded_cut, None), res.node_cost_sum
    if batch.B:
        # the cuts of the contracted run differ from the original graph's by fixed_cut; for weights that are not integers
        # the sum of the two need not carry the bits of a recount, so every cut is recounted from its lifted partition
        cuts = (recount(partition), recount(ct.lift(parts["trained"])), recount(ct.lift(parts["rounded"])),
                recount(ct.lift(parts["annealed"])) if "annealed" in parts else None)
        cost_sum = None if node_cost is None else _node_cost_sum(batch, node_cost, partition)
    cut, trained_cut, rounded_cut, annealed_cut = cuts
    return MaxCutResult(partition, cut, trained_cut, rounded_cut, batch.goff, annealed_cut, ct.fixed_cut,
                        node_cost_sum=cost_sum, fixed_cost=fixed_cost)


def _refuse_small(n_max: int, K: int, loss: str) -> None:
    if instance_too_large(n_max, K, loss):
        raise ValueError(_TOO_LARGE.format(n=n_max, K=K))


def _refuse_large(n_max: int, K: int, loss: str) -> None:
    if n_max > hip.LARGE_MAX_GRAPH_NODES:
        raise ValueError(_BEYOND_LARGE.format(n=n_max, bound=hip.LARGE_MAX_GRAPH_NODES))


@dataclass(frozen=True)
class _Route:
    """What tells :func:`solve_batch` from :func:`solve_large_batch`: the engine class, the refusal of a batch by its
    largest graph, ``large`` as the decoders of ``Testing.TestingNeuralNetwork`` take it, and whether the route has the
    tabu and the balanced stage - and with them per-node costs."""
    engine: type
    refuse: Callable
    large: bool
    stages: bool


_SMALL = _Route(InstanceEngine, _refuse_small, large=False, stages=True)
_LARGE = _Route(LargeInstanceEngine, _refuse_large, large=True, stages=False)


def _solve_batch(route: _Route, batch: GraphBatch, number_classes: int, terminals: bool, hidden_dim: int, epochs: int,
                 learning_rate: float, loss: str, samples: int, anneal_sweeps: int, max_descent_sweeps: int,
                 seed: int, tabu_iterations: int = 0, class_sizes=None, balance_iterations: Optional[int] = None,
                 parts: Optional[dict] = None, *, node_cost: Optional[torch.Tensor] = None,
                 abs_scale: bool = False, tempering: Optional[tuple] = None) -> MaxCutResult:
    """``parts``: a dict that receives the partitions behind ``trained_cut``, ``rounded_cut`` (and ``annealed_cut``).
    ``node_cost``: a float32 tensor [R, K] that :func:`_check_node_cost` has returned - the public doors check once and
    pass the checked tensor down (small route); the tabu and the balanced stage then take it too; ``abs_scale``: the
    annealing's temperature in units of the mean absolute edge weight (the doors with signed weights); ``tempering``:
    what :func:`_check_tempering` returned."""
    from .Testing import TestingNeuralNetwork as T
    K, terminals = _classes(number_classes), bool(terminals)
    if epochs < 0 or samples < 0 or anneal_sweeps < 0 or max_descent_sweeps < 0:
        raise ValueError(f"epochs, samples, anneal_sweeps and max_descent_sweeps must be >= 0, got {epochs}, {samples}, "
                         f"{anneal_sweeps}, {max_descent_sweeps}")
    if not 0 <= int(tabu_iterations) < 1 << 31:
        raise ValueError(f"tabu_iterations must be in 0..2^31-1, got {tabu_iterations}")
    if tabu_iterations and not route.stages:
        raise NotImplementedError(_NO_TABU)
    _check_sizes(class_sizes, balance_iterations, None)
    if tempering is not None:
        if not route.stages:
            raise NotImplementedError(_NO_TEMPER)
        tempering = _check_tempering(*tempering, tabu_iterations, class_sizes, samples)
    bounds = None
    if class_sizes is not None:
        if not route.stages:
            raise NotImplementedError(_NO_BALANCE)
        bounds = _size_bounds(class_sizes, batch.sizes, K, terminals)   # on the host, before anything is trained
    loss = hip.loss_name(loss)
    if batch.B:
        route.refuse(batch.n_max, K, loss)
    cost = {}
    if node_cost is not None:
        if not route.stages:
            raise NotImplementedError(_NO_COST_LARGE)
        node_cost = node_cost.to(batch.device)
        cost = {"node_cost": node_cost}
    eng = route.engine(batch, int(hidden_dim), K, batch.device, terminals=terminals, **cost)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        eng.reset_parameters()
    for epoch in range(int(epochs)):
        _, S, losses = eng.train_fwd_bwd(1.0, loss=loss)
        eng.adam_step(float(learning_rate))
        eng.keep_best(S, losses, epoch)
    P, S, _ = eng.forward(1.0, loss=loss)
    best_S = eng.best_S if epochs > 0 else S
    dev = batch.device
    if batch.B == 0:
        none = torch.empty(0, dtype=torch.float32, device=dev)
        return MaxCutResult(best_S, none, none.clone(), none.clone(), batch.goff,
                            node_cost_sum=None if node_cost is None else none.clone())
    large = route.large
    rounded, rounded_cut, _, _ = T._round_on_gpu(batch, P, 0, terminals, node_cost, large=large)
    trained = best_S.to(torch.int8).reshape(1, -1)
    no_sweeps = np.zeros(0, np.float32)
    _, trained_cut, _ = T._kway_anneal_on_gpu(batch, K, trained.clone(), no_sweeps, 0, 0, terminals, node_cost,
                                              large=large)   # scores, moves nothing
    rows = [trained, rounded.reshape(1, -1)]
    if samples > 0:
        rows.append(T._kway_sample_on_gpu(batch, P, int(samples), int(seed) & T._M64, range(batch.B), True, terminals,
                                          node_cost, large=large)[3])
    cands = torch.cat(rows).contiguous()
    scale = T._mean_edge_weight(batch) if bounds is None and not abs_scale else _mean_abs_edge_weight(batch)
    inv_temp = T.anneal_schedule(int(anneal_sweeps), scale=scale)
    partition, cut, _ = T._kway_anneal_on_gpu(batch, K, cands, inv_temp, seed, int(max_descent_sweeps), terminals,
                                              node_cost, large=large)
    cost_sum = (lambda part: None) if node_cost is None else (lambda part: _node_cost_sum(batch, node_cost, part))
    if parts is not None:
        parts.update(trained=best_S, rounded=rounded)
        if tabu_iterations or tempering is not None:
            parts.update(annealed=partition)
    annealed_cut = None
    if tempering is not None:
        # the annealing left its candidates in `cands`: whole ladders of them become the walkers (a copy), their best
        # states descend and are picked by the annealing call without sweeps; then the better of the two, as below
        rounds, sweeps, rungs = tempering
        walkers = cands[:rungs * (cands.shape[0] // rungs)].clone()
        best = T._kway_temper_on_gpu(batch, K, walkers, T.temper_ladder(rungs, scale=scale), rounds, sweeps, seed,
                                     terminals, node_cost)[0]
        temper_partition, temper_cut, _ = T._kway_anneal_on_gpu(batch, K, best, no_sweeps, 0, int(max_descent_sweeps),
                                                                terminals, node_cost)
        better = temper_cut > cut
        sizes = (batch.goff[1:] - batch.goff[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(better, sizes, output_size=batch.R)
        partition, cut, annealed_cut = (torch.where(rows, temper_partition, partition), torch.where(better, temper_cut, cut),
                                        cut)
    if tabu_iterations:
        # the annealing left its candidates in `cands`; the better of the two results per graph, chosen on the device
        tabu_partition, tabu_cut = T._kway_tabu_on_gpu(batch, K, cands.clone(), int(tabu_iterations), T.TABU_TENURE, seed,
                                                       terminals, node_cost)[:2]
        better = tabu_cut > cut
        sizes = (batch.goff[1:] - batch.goff[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(better, sizes, output_size=batch.R)
        partition, cut, annealed_cut = torch.where(rows, tabu_partition, partition), torch.where(better, tabu_cut, cut), cut
    if bounds is None:
        return MaxCutResult(partition, cut, trained_cut, rounded_cut, batch.goff, annealed_cut,
                            node_cost_sum=cost_sum(partition))
    # the balanced stage starts from the annealed candidates too (a copy: repaired into the bounds, then searched)
    iterations = 20 * int(batch.n_max) if balance_iterations is None else int(balance_iterations)
    within, within_cut = T._kway_balance_on_gpu(batch, K, cands.clone(), bounds[0], bounds[1], iterations, T.TABU_TENURE,
                                                seed, terminals, node_cost)[:2]
    return MaxCutResult(within, within_cut, trained_cut, rounded_cut, batch.goff, annealed_cut, unconstrained_cut=cut,
                        node_cost_sum=cost_sum(within))


def _node_cost_sum(batch: GraphBatch, node_cost: torch.Tensor, partition: torch.Tensor) -> torch.Tensor:
    """[B] float32: sum_v node_cost[v][partition_v] per graph, without atomics: a float64 running sum over the batch's
    rows (a scan: the same bits every time), differenced at the graphs' boundaries."""
    picked = node_cost.gather(1, partition.to(torch.int64).reshape(-1, 1)).reshape(-1).to(torch.float64)
    run = torch.cat([picked.new_zeros(1), torch.cumsum(picked, 0)])
    goff = batch.goff.to(torch.int64)
    return (run[goff[1:]] - run[goff[:-1]]).to(torch.float32)


@dataclass
class IsingResult:
    """What :func:`solve_ising` returns."""
    spins: torch.Tensor    # [R] int8: +1 / -1 (device)
    energy: torch.Tensor   # [B] float64: H(spins) per graph (host)
    ptr: torch.Tensor      # [B + 1] int32
    result: MaxCutResult   # the max-cut run behind it: class 0 is spin +1, result.cut the objective sum(J) - H


@dataclass
class QuboResult:
    """What :func:`solve_qubo` returns."""
    x: torch.Tensor        # [R] int8: 0 / 1 (device)
    energy: torch.Tensor   # [B] float32: E(x) per graph (device)
    ptr: torch.Tensor      # [B + 1] int32
    result: MaxCutResult   # the max-cut run behind it: class 1 is x = 1, result.cut the objective -E


def _values(what: str, values, shape_name: str, count: int, default: float) -> np.ndarray:
    """A door's per-edge or per-node values as float64 [count] (``None``: ``default`` everywhere): the shape, finite."""
    if values is None:
        return np.full(count, default, np.float64)
    v = _host_array(values)
    if v.ndim != 1 or v.shape[0] != count:
        raise ValueError(f"{what} must be [{shape_name}] = [{count}], got {tuple(v.shape)}")
    if not np.all(np.isfinite(v.astype(np.float64))):
        raise ValueError(f"{what} holds values that are not finite")
    return v.astype(np.float64)


def _door(edge_index, ptr, num_nodes):
    """(edge_index on the host, graph offsets [B + 1] int64) of a door's arguments."""
    ei = _host_array(edge_index)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(ei.shape)}")
    if (ptr is None) == (num_nodes is None):
        raise ValueError("pass exactly one of ptr (graph boundaries) and num_nodes (a single graph)")
    goff = np.asarray([0, int(num_nodes)], np.int64) if ptr is None else _host_array(ptr).astype(np.int64)
    if goff.ndim != 1 or goff.size < 1:
        raise ValueError("ptr must be [B + 1]")
    return ei, goff


def _solve_door(batch: GraphBatch, node_cost: np.ndarray, hidden_dim, epochs, learning_rate, loss, samples, anneal_sweeps,
                max_descent_sweeps, seed, tabu_iterations=0, class_sizes=None, balance_iterations=None,
                tempering=None) -> MaxCutResult:
    loss = hip.loss_name(loss)
    if batch.B:
        _refuse_small(batch.n_max, 2, loss)
    return _solve_batch(_SMALL, batch, 2, False, hidden_dim, epochs, learning_rate, loss, samples, anneal_sweeps,
                        max_descent_sweeps, seed, tabu_iterations, class_sizes, balance_iterations,
                        node_cost=_check_node_cost(node_cost, batch.R, 2), abs_scale=True, tempering=tempering)


def _door_stages(what: str, goff: np.ndarray, tabu_iterations, class_sizes, balance_iterations):
    """The argument errors of a door's stage keywords, raised on the host before anything is built; returns
    ``class_sizes`` as (lo, hi) int32 [B, 2], or None."""
    if not 0 <= int(tabu_iterations) < 1 << 31:
        raise ValueError(f"tabu_iterations must be in 0..2^31-1, got {tabu_iterations}")
    _check_sizes(class_sizes, balance_iterations, None)
    if class_sizes is None:
        return None
    from .Testing import TestingNeuralNetwork as T
    return T.class_size_bounds(what, class_sizes, np.diff(goff), 2, False)


def _cardinality_sizes(cardinality, goff: np.ndarray):
    """``cardinality`` of :func:`solve_qubo` - an integer k or a pair (lo, hi) on the number of ``x_i = 1`` of every
    graph - as ``class_sizes``: class 1 holds lo..hi nodes, class 0 the rest."""
    pair = (cardinality, cardinality) if isinstance(cardinality, (int, np.integer)) else cardinality
    if (not isinstance(pair, (tuple, list)) or len(pair) != 2
            or not all(isinstance(x, (int, np.integer)) for x in pair)):
        raise ValueError(f"cardinality must be an integer or a pair (lo, hi) of integers, got {cardinality!r}")
    lo, hi = int(pair[0]), int(pair[1])
    n = np.diff(goff).astype(np.int64)
    ones = np.ones_like(n)
    return (np.stack([np.maximum(n - hi, 0), lo * ones], axis=1), np.stack([np.maximum(n - lo, 0), hi * ones], axis=1))


def solve_ising(edge_index, ptr=None, num_nodes: Optional[int] = None, coupling=None, field=None, *, pairs: str = "both",
                hidden_dim: int, epochs: int, learning_rate: float, loss: str = "expected_cut", samples: int = 32,
                anneal_sweeps: int = 100, max_descent_sweeps: int = 100, seed: int = 0, tabu_iterations: int = 0,
                class_sizes=None, balance_iterations: Optional[int] = None, tempering_rounds: int = 0,
                tempering_sweeps: int = 4, tempering_rungs: int = 8) -> IsingResult:
    """Minimises ``H(s) = sum_{i<j} J_ij s_i s_j + sum_i h_i s_i`` over ``s`` in {+1, -1}^n for every graph of a batch:
    ``edge_index`` / ``ptr`` / ``num_nodes`` / ``pairs`` as :func:`solve` takes them, ``coupling`` [E] the J of every
    entry (``None``: 1; with ``pairs="both"`` both directions carry the same J), ``field`` [R] the h of every node
    (``None``: 0); the training and decoding keywords are :func:`solve`'s.

    The mapping onto :func:`solve` is exact: edge weight ``w = 2 J``, two classes without terminals, class 0 is ``s =
    +1`` (class 1 is ``s = -1``), ``node_cost[i] = (h_i, -h_i)``; then ``H(s) = sum_{i<j} J_ij - obj``, ``obj`` the objective ``cut - cost``
    the solver maximises.  The weights are signed, so the annealing's temperature is in units of the mean absolute edge
    weight.  Returns ``spins`` [R] int8, ``energy`` [B] float64 (``sum J`` taken in float64 on the host, ``obj`` the
    solver's float32), ``ptr`` and the :class:`MaxCutResult` as ``.result``.

    ``tabu_iterations``, ``class_sizes`` and ``balance_iterations`` have :func:`solve`'s meaning, on the objective (the
    tabu and the balanced stage with costs, ``gmc_kway_tabu_c_f32`` / ``gmc_kway_balance_c_f32``).  Class 0 is ``s = +1``
    and class 1 is ``s = -1``, so ``class_sizes=(lo, hi)`` bounds the number of up spins by ``lo[0]..hi[0]`` and of down
    spins by ``lo[1]..hi[1]`` - a bounded magnetisation; ``spins`` and ``energy`` are then those of the within-bounds
    partition.  Bounds that admit no partition raise ``ValueError`` before anything is built.  The defaults launch
    nothing more and change no byte.  ``tempering_rounds``, ``tempering_sweeps`` and ``tempering_rungs``: :func:`solve`'s
    tempering stage on the objective, its ladder in units of the mean absolute edge weight.

    A spin without any coupling is refused by the batch builder (``ValueError``: "nodes without neighbours"); its optimum
    is its own sign, ``s_i = -sign(h_i)`` - leave it out and add ``-|h_i|`` to the energy."""
    ei, goff = _door(edge_index, ptr, num_nodes)
    class_sizes = _door_stages("solve_ising", goff, tabu_iterations, class_sizes, balance_iterations)
    tempering = _check_tempering(tempering_rounds, tempering_sweeps, tempering_rungs, tabu_iterations, class_sizes, samples)
    E, R = ei.shape[1], int(goff[-1])
    J = _values("coupling", coupling, "E", E, 1.0)
    h = _values("field", field, "R", R, 0.0)
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    once = src < dst if pairs == "both" else src != dst   # every undirected edge once; a self-loop is no i < j
    B = goff.size - 1
    graph = np.clip(np.searchsorted(goff, src[once], side="right") - 1, 0, max(B - 1, 0))
    sum_j = np.zeros(B, np.float64)
    np.add.at(sum_j, graph, J[once])
    node_cost = np.stack([h, -h], axis=1).astype(np.float32)
    batch = GraphBatch.from_edge_index(edge_index, ptr, num_nodes, (2.0 * J).astype(np.float32), pairs=pairs)
    res = _solve_door(batch, node_cost, hidden_dim, epochs, learning_rate, loss, samples, anneal_sweeps,
                      max_descent_sweeps, seed, tabu_iterations, class_sizes, balance_iterations, tempering)
    spins = (1 - 2 * res.partition).to(torch.int8)
    energy = torch.from_numpy(sum_j) - res.cut.detach().cpu().to(torch.float64)
    return IsingResult(spins, energy, res.ptr, res)


def solve_qubo(edge_index, ptr=None, num_nodes: Optional[int] = None, quadratic=None, linear=None, *, pairs: str = "both",
               hidden_dim: int, epochs: int, learning_rate: float, loss: str = "expected_cut", samples: int = 32,
               anneal_sweeps: int = 100, max_descent_sweeps: int = 100, seed: int = 0, tabu_iterations: int = 0,
               class_sizes=None, balance_iterations: Optional[int] = None, cardinality=None, tempering_rounds: int = 0,
               tempering_sweeps: int = 4, tempering_rungs: int = 8) -> QuboResult:
    """Minimises ``E(x) = sum_i a_i x_i + sum_{i<j} q_ij x_i x_j`` over ``x`` in {0, 1}^n for every graph of a batch:
    ``edge_index`` / ``ptr`` / ``num_nodes`` / ``pairs`` as :func:`solve` takes them, ``quadratic`` [E] the q of every
    entry (``None``: 1; with ``pairs="both"`` both directions carry the same q), ``linear`` [R] the a of every variable
    (``None``: 0); the training and decoding keywords are :func:`solve`'s.

    The mapping onto :func:`solve` is exact and has no offset: edge weight ``w_ij = q_ij / 2``, two classes without
    terminals, class 1 is ``x = 1``, ``node_cost[i] = (0, a_i + 1/2 sum_j q_ij)``; then ``E(x) = -obj``.  The row sums
    ``1/2 sum_j q_ij = sum_j w_ij`` are taken on the device from the built batch's sorted CSR, one thread per row in CSR
    order (gmc_row_weight_sums_f32: no atomics, the same bits every time).  The weights are signed, so the annealing's
    temperature is in units of the mean absolute edge weight.  Returns ``x`` [R] int8, ``energy`` [B] float32, ``ptr``
    and the :class:`MaxCutResult` as ``.result``.

    ``tabu_iterations``, ``class_sizes`` and ``balance_iterations`` have :func:`solve`'s meaning, on the objective (the
    tabu and the balanced stage with costs, ``gmc_kway_tabu_c_f32`` / ``gmc_kway_balance_c_f32``).  Class 1 is ``x = 1``
    and class 0 is ``x = 0``.  ``cardinality``: an integer ``k`` (exactly ``k`` variables set per graph) or a pair
    ``(lo, hi)`` (between ``lo`` and ``hi``) - the cardinality-constrained QUBO; it is mapped onto ``class_sizes``
    (class 1 holds ``lo..hi`` nodes), and passing both raises ``ValueError``.  With bounds ``x`` and ``energy`` are those
    of the within-bounds partition.  Bounds that admit no partition raise ``ValueError`` before anything is built.  The
    defaults launch nothing more and change no byte.  ``tempering_rounds``, ``tempering_sweeps`` and ``tempering_rungs``:
    :func:`solve`'s tempering stage on the objective, its ladder in units of the mean absolute edge weight.

    A variable without any quadratic term is refused by the batch builder (``ValueError``: "nodes without
    neighbours"); its optimum is its own sign, ``x_i = 1`` iff ``a_i < 0`` - leave it out and add ``min(a_i, 0)``."""
    ei, goff = _door(edge_index, ptr, num_nodes)
    if cardinality is not None:
        if class_sizes is not None:
            raise ValueError("cardinality is mapped onto class_sizes: pass one of the two")
        class_sizes = _cardinality_sizes(cardinality, goff)
    class_sizes = _door_stages("solve_qubo", goff, tabu_iterations, class_sizes, balance_iterations)
    tempering = _check_tempering(tempering_rounds, tempering_sweeps, tempering_rungs, tabu_iterations, class_sizes, samples)
    E, R = ei.shape[1], int(goff[-1])
    q = _values("quadratic", quadratic, "E", E, 1.0)
    a = _values("linear", linear, "R", R, 0.0)
    batch = GraphBatch.from_edge_index(edge_index, ptr, num_nodes, (0.5 * q).astype(np.float32), pairs=pairs)
    half = torch.zeros(batch.R, dtype=torch.float32, device=batch.device)
    if batch.R:
        rc = hip.load().gmc_row_weight_sums_f32(batch.R, hip.ptr(batch.rowptr), hip.ptr(batch.gcol), hip.ptr(batch.vals),
                                                hip.ptr(half), hip.stream())
        hip.check(rc, "gmc_row_weight_sums_f32")
    node_cost = np.zeros((R, 2), np.float32)
    node_cost[:, 1] = a.astype(np.float32) + half.cpu().numpy()   # (one fp32 addition per variable)
    res = _solve_door(batch, node_cost, hidden_dim, epochs, learning_rate, loss, samples, anneal_sweeps,
                      max_descent_sweeps, seed, tabu_iterations, class_sizes, balance_iterations, tempering)
    return QuboResult(res.partition.to(torch.int8), -res.cut, res.ptr, res)


# ---- the semidefinite relaxation (Goemans-Williamson): no model, no training ---------------------
@dataclass
class SdpResult:
    """What :func:`solve_sdp` returns: device tensors, graph g owning rows ``ptr[g] .. ptr[g+1]-1`` of ``partition``."""
    partition: torch.Tensor       # [R] int32: the class of every node
    cut: torch.Tensor             # [B] float32: the cut of ``partition`` (with node_cost: the objective cut - cost)
    rounded_cut: torch.Tensor     # [B] float32: the best hyperplane's, before any search
    relaxed_value: torch.Tensor   # [B] float32: the relaxed objective after the last sweep - an upper bound on the optimum
    #                               only at the relaxation's optimum, not a certificate
    ptr: torch.Tensor             # [B + 1] int32
    node_cost_sum: Optional[torch.Tensor] = None   # [B] float32, with node_cost only: sum_v node_cost[v][partition_v]


def _sdp_rank(rank, n_max: int) -> int:
    if rank is None:
        need = np.sqrt(2.0 * max(int(n_max), 1)) + 1.0
        return next((r for r in hip.SDP_RANKS if r >= need), hip.SDP_RANKS[-1])
    if int(rank) not in hip.SDP_RANKS:
        raise ValueError(f"rank must be one of {hip.SDP_RANKS} (or None), got {rank}")
    return int(rank)


def _sdp_cost(batch: GraphBatch, node_cost) -> Optional[torch.Tensor]:
    if node_cost is None:
        return None
    return _check_node_cost(node_cost, batch.R, 2).to(batch.device).contiguous()


def _sdp_keys(batch: GraphBatch, seed: int) -> torch.Tensor:
    from .Testing import TestingNeuralNetwork as T
    keys = T.sample_keys(int(seed) & T._M64, range(batch.B))
    return torch.from_numpy(keys.view(np.int64)).to(batch.device)


def _sdp_relax_keys(batch: GraphBatch, gkey: Optional[torch.Tensor], rank: int, sweeps: int, terminals: bool,
                    node_cost: Optional[torch.Tensor], V: Optional[torch.Tensor]):
    """gmc_sdp_relax_f32 with the graphs' keys given ([B] int64 on the device: the uint64 words; None with ``V``)."""
    from .Testing import TestingNeuralNetwork as T
    if not 0 <= int(sweeps) < 1 << 31:
        raise ValueError(f"sweeps must be in 0..2^31-1, got {sweeps}")
    T._needs_terminals(batch, 2, terminals)
    dev = batch.device
    if V is None:
        V = torch.empty((batch.R, rank), dtype=torch.float32, device=dev)
        init = 1
    else:
        if not isinstance(V, torch.Tensor) or tuple(V.shape) != (batch.R, rank) or V.dtype != torch.float32:
            raise ValueError(f"V must be a float32 tensor [{batch.R}, {rank}] (what sdp_relax returned)")
        V = V.to(dev).contiguous().clone()
        init = 0
    value = torch.empty(batch.B, dtype=torch.float32, device=dev)
    if batch.B == 0:
        return V, value
    lib = hip.load()
    need = int(lib.gmc_sdp_workspace_bytes(batch.ref(), rank))
    if need <= 0:
        raise hip.HipExtensionError(f"gmc_sdp_workspace_bytes refused the batch (rank = {rank})")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    order, cgoff, cptr = batch.refine_order(2, terminals)
    p = hip.ptr
    rc = lib.gmc_sdp_relax_f32(batch.ref(), rank, int(terminals), p(node_cost), p(order), p(cgoff), p(cptr),
                               batch.refine_classes(2, terminals), p(gkey), init, int(sweeps), p(V), p(value), p(ws),
                               ws.numel(), hip.stream())
    hip.check(rc, "gmc_sdp_relax_f32")
    return V, value


def _sdp_round_keys(batch: GraphBatch, V: torch.Tensor, gkey: torch.Tensor, first_plane: int, planes: int,
                    terminals: bool) -> torch.Tensor:
    """gmc_sdp_round_f32: planes ``first_plane .. first_plane + planes - 1`` as [planes, R] int8."""
    if V.dim() != 2 or V.shape[0] != batch.R or int(V.shape[1]) not in hip.SDP_RANKS or V.dtype != torch.float32:
        raise ValueError(f"V must be a float32 tensor [{batch.R}, rank], rank one of {hip.SDP_RANKS}")
    if planes < 0 or first_plane < 0 or first_plane + planes >= 1 << 31:
        raise ValueError(f"planes and first_plane must be >= 0 and end below 2^31, got {planes}, {first_plane}")
    assign = torch.empty((int(planes), batch.R), dtype=torch.int8, device=batch.device)
    if batch.B == 0 or planes == 0:
        return assign
    V = V.to(batch.device).contiguous()
    p = hip.ptr
    rc = hip.load().gmc_sdp_round_f32(batch.ref(), int(V.shape[1]), int(terminals), p(V), p(gkey), int(first_plane),
                                      int(planes), p(assign), hip.stream())
    hip.check(rc, "gmc_sdp_round_f32")
    return assign


def sdp_relax(batch: GraphBatch, *, rank: Optional[int] = None, sweeps: int = 50, seed: int = 0, terminals: bool = False,
              node_cost=None, V: Optional[torch.Tensor] = None):
    """The low-rank semidefinite relaxation of max-cut (K = 2) of every graph of ``batch`` by the mixing method
    (include/gcnmaxcut_sdp.h, ``gmc_sdp_relax_f32``): one unit vector of ``rank`` floats per node, ``sweeps`` sweeps of
    ``v_i <- -normalize(sum_j w_ij v_j)`` over the colour classes.  Returns ``(V [R, rank], value [B])``, float32 on
    the device; ``value`` is the relaxed objective ``1/2 sum_uv w_uv (1 - v_u . v_v)`` after the last sweep, which no
    sweep lowers.  It is an upper bound on the optimum only at the relaxation's optimum, not a certificate.

    ``rank``: 16, 32 or 64; ``None`` takes the smallest of them that is at least ``sqrt(2 n_max) + 1`` - the bound above
    which the low-rank form has no spurious local optima - else 64: beyond 2,048 nodes rank 64 lies under that bound, and
    the sweeps may then stop at a local optimum of the low-rank problem.  ``seed`` seeds the start (graph ``g`` of the
    batch draws from ``sample_keys(seed, [g])``).  ``V``: a state to continue from instead (``sdp_relax(sweeps=a + b)``
    equals ``sdp_relax(sweeps=a)`` followed by ``sdp_relax(sweeps=b, V=...)`` byte for byte; it is not modified).
    ``terminals=True``: nodes 0 and 1 of every graph are fixed to classes 0 and 1.  ``node_cost`` [R, 2]: the objective
    ``cut(S) - sum_v node_cost[v][S_v]`` as :func:`solve` takes it, relaxed along the reference direction."""
    rank = _sdp_rank(rank, batch.n_max if batch.B else 1)
    cost = _sdp_cost(batch, node_cost)
    gkey = _sdp_keys(batch, seed) if V is None else None
    return _sdp_relax_keys(batch, gkey, rank, sweeps, bool(terminals), cost, V)


def sdp_round(batch: GraphBatch, V: torch.Tensor, planes: int = 200, seed: int = 0, terminals: bool = False) -> torch.Tensor:
    """``planes`` random hyperplanes through the vectors ``V`` of :func:`sdp_relax` (``gmc_sdp_round_f32``): [planes, R]
    int8 class bytes, class 0 on the side of the reference direction.  The normals are seeded by ``seed``; plane m's
    bytes do not depend on ``planes``."""
    return _sdp_round_keys(batch, V, _sdp_keys(batch, seed), 0, int(planes), bool(terminals))


def solve_sdp_batch(batch: GraphBatch, *, rank: Optional[int] = None, sweeps: int = 50, planes: int = 200,
                    anneal_sweeps: int = 100, max_descent_sweeps: int = 100, seed: int = 0, terminals: bool = False,
                    node_cost=None) -> SdpResult:
    """:func:`solve_sdp` on a ready batch (``node_cost`` rows = batch rows)."""
    from .Testing import TestingNeuralNetwork as T
    terminals = bool(terminals)
    if planes < 1 or anneal_sweeps < 0 or max_descent_sweeps < 0:
        raise ValueError(f"planes must be >= 1, anneal_sweeps and max_descent_sweeps >= 0, got {planes}, {anneal_sweeps}, "
                         f"{max_descent_sweeps}")
    large = bool(batch.B) and batch.n_max > hip.MAX_GRAPH_NODES
    if large and node_cost is not None:
        raise NotImplementedError("node_cost with a graph beyond hip.MAX_GRAPH_NODES nodes: the annealing for such graphs "
                                  "(gmc_large_anneal_f32) takes no per-node costs")
    cost = _sdp_cost(batch, node_cost)
    V, value = sdp_relax(batch, rank=rank, sweeps=sweeps, seed=seed, terminals=terminals, node_cost=cost)
    if batch.B == 0:
        none = torch.empty(0, dtype=torch.float32, device=batch.device)
        return SdpResult(torch.empty(0, dtype=torch.int32, device=batch.device), none, none.clone(), value, batch.goff,
                         None if cost is None else none.clone())
    cands = sdp_round(batch, V, int(planes), seed, terminals)
    _, rounded_cut, _ = T._kway_anneal_on_gpu(batch, 2, cands.clone(), np.zeros(0, np.float32), 0, 0, terminals, cost,
                                              large=large)   # scores and picks, moves nothing
    inv_temp = T.anneal_schedule(int(anneal_sweeps), scale=_mean_abs_edge_weight(batch))
    partition, cut, _ = T._kway_anneal_on_gpu(batch, 2, cands, inv_temp, seed, int(max_descent_sweeps), terminals, cost,
                                              large=large)
    return SdpResult(partition, cut, rounded_cut, value, batch.goff,
                     None if cost is None else _node_cost_sum(batch, cost, partition))


def solve_sdp(edge_index, ptr=None, num_nodes: Optional[int] = None, edge_weight=None, *, pairs: str = "both",
              rank: Optional[int] = None, sweeps: int = 50, planes: int = 200, anneal_sweeps: int = 100,
              max_descent_sweeps: int = 100, seed: int = 0, terminals: bool = False, node_cost=None) -> SdpResult:
    """Max-cut (two classes) of every graph of a batch given as :func:`solve` takes it, without a model and without
    training: the Goemans-Williamson route.

    1. the batch, built on the GPU;
    2. :func:`sdp_relax`: ``sweeps`` sweeps of the low-rank semidefinite relaxation at ``rank``;
    3. :func:`sdp_round`: ``planes`` random hyperplanes, each a candidate partition; ``rounded_cut`` is the best of them;
    4. the annealing launch of :func:`solve` over these candidates (``anneal_sweeps`` Metropolis sweeps, then at most
       ``max_descent_sweeps`` sweeps of the local search; for a graph beyond ``hip.MAX_GRAPH_NODES`` nodes through
       ``gmc_large_anneal_f32``), which scores and picks: ``cut >= rounded_cut``.

    ``relaxed_value`` is the relaxation's objective after the last sweep.  At the relaxation's optimum it bounds the
    optimum from above; after finitely many sweeps of a low-rank form it is below that optimum and is NOT a certificate.
    ``node_cost`` [R, 2] has :func:`solve`'s meaning (every ``*_cut`` field is then the objective, ``relaxed_value`` its
    relaxed form); with a graph beyond ``hip.MAX_GRAPH_NODES`` nodes it raises ``NotImplementedError``.  Signed weights
    are taken (the annealing's temperature is in units of the mean absolute weight), but the 0.878 guarantee of the
    hyperplane rounding holds for non-negative weights only."""
    if node_cost is not None:
        node_cost = _check_node_cost(node_cost, _rows_of(ptr, num_nodes), 2)
    batch = GraphBatch.from_edge_index(edge_index, ptr, num_nodes, edge_weight, pairs=pairs)
    return solve_sdp_batch(batch, rank=rank, sweeps=sweeps, planes=planes, anneal_sweeps=anneal_sweeps,
                           max_descent_sweeps=max_descent_sweeps, seed=seed, terminals=terminals, node_cost=node_cost)


# ---- dense instances: annealing on cached local fields, no model, no training ---------------------
@dataclass
class DenseResult:
    """What :func:`solve_dense` returns: device tensors, one row per instance."""
    partition: torch.Tensor                 # [B, n] int32: the class of every node
    cut: torch.Tensor                       # [B] float32: the cut of ``partition`` (with node_cost: the objective cut - cost)
    node_cost_sum: Optional[torch.Tensor]   # [B] float32, with node_cost only: sum_v node_cost[v][partition_v]
    moves: torch.Tensor                     # [B, candidates] int64: the annealing moves every chain accepted


@dataclass
class DenseIsingResult:
    """What :func:`solve_ising_dense` returns."""
    spins: torch.Tensor     # [B, n] int8: +1 / -1 (device)
    energy: torch.Tensor    # [B] float64: H(spins), recounted in float64 (device)
    result: DenseResult     # the max-cut run behind it: class 0 is spin +1, result.cut the objective sum(J) - H in float32


@dataclass
class DenseQuboResult:
    """What :func:`solve_qubo_dense` returns."""
    x: torch.Tensor         # [B, n] int8: 0 / 1 (device)
    energy: torch.Tensor    # [B] float64: E(x), recounted in float64 (device)
    result: DenseResult     # the max-cut run behind it: class 1 is x = 1, result.cut the objective -E in float32


def _dense_cost(what: str, node_cost, B: int, n: int, dev) -> Optional[torch.Tensor]:
    """``node_cost`` of a dense door -> [B * n, 2] float32 on the device, or None: [n, 2] / [B, n, 2] / [B * n, 2], finite."""
    if node_cost is None:
        return None
    t = node_cost if isinstance(node_cost, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(node_cost))
    if t.numel() != B * n * 2 or t.shape[-1] != 2:
        raise ValueError(f"{what} must be [{n}, 2] per instance ({B} instances), got {tuple(t.shape)}")
    t = t.to(dev, torch.float32).reshape(B * n, 2).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what} holds values that are not finite (in float32)")
    return t


def _dense_vector(what: str, values, B: int, n: int, dev) -> torch.Tensor:
    """A dense door's per-node values -> [B, n] float64 on the device (None: zeros): [n] / [B, n], finite."""
    if values is None:
        return torch.zeros((B, n), dtype=torch.float64, device=dev)
    t = values if isinstance(values, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(values))
    if t.numel() != B * n:
        raise ValueError(f"{what} must be [{n}] per instance ({B} instances), got {tuple(t.shape)}")
    t = t.to(dev, torch.float64).reshape(B, n)
    if not bool(torch.isfinite(t.to(torch.float32)).all()):
        raise ValueError(f"{what} holds values that are not finite")
    return t


def _dense_starts(B: int, n: int, candidates: int, seed: int, partitions, dev) -> torch.Tensor:
    """The chains' starts [candidates, B * n] int8: ``partitions`` when given ([candidates, B * n] or, for one instance,
    [candidates, n]; classes 0 / 1), else seeded random bytes drawn by torch on the device - plumbing: reproducible on one
    installation, NOT part of the kernel's byte-for-byte contract."""
    if partitions is not None:
        p = partitions if isinstance(partitions, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(partitions))
        if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] != B * n:
            raise ValueError(f"partitions must be [candidates, {B * n}], got {tuple(p.shape)}")
        if int(p.min()) < 0 or int(p.max()) > 1:
            raise ValueError("partitions holds a class outside 0..1")
        return p.to(dev, torch.int8).contiguous().clone()
    if int(candidates) < 1:
        raise ValueError(f"candidates must be >= 1, got {candidates}")
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed) & ((1 << 63) - 1))
    return torch.randint(0, 2, (int(candidates), B * n), generator=gen, device=dev, dtype=torch.int8)


def _check_bifurcation(partitions, bifurcation_steps) -> None:
    """The dense doors' refusals about ``bifurcation_steps``, made before the GPU is asked for."""
    if int(bifurcation_steps) < 0:
        raise ValueError(f"bifurcation_steps must be >= 0, got {bifurcation_steps}")
    if int(bifurcation_steps) > 0 and partitions is not None:
        raise ValueError("partitions= and bifurcation_steps > 0 both name the chains' starts: give one of them")


def _solve_dense(W: torch.Tensor, cost: Optional[torch.Tensor], candidates, anneal_sweeps, seed, max_descent_sweeps,
                 t_start, t_end, partitions, bifurcation_steps=0, bifurcation_dt=1.25,
                 bifurcation_c0=None) -> DenseResult:
    from .Testing import TestingNeuralNetwork as T
    if anneal_sweeps < 0 or max_descent_sweeps < 0:
        raise ValueError(f"anneal_sweeps and max_descent_sweeps must be >= 0, got {anneal_sweeps} and {max_descent_sweeps}")
    B, n = int(W.shape[0]), int(W.shape[1])
    _check_bifurcation(partitions, bifurcation_steps)
    if int(bifurcation_steps) > 0:
        starts, _, _ = T._dense_bifurcation_on_gpu(W, int(candidates), T.bifurcation_pump(int(bifurcation_steps)),
                                                   T.bifurcation_c0(W, bifurcation_c0), float(bifurcation_dt), cost,
                                                   seed=seed)
    else:
        starts = _dense_starts(B, n, candidates, seed, partitions, W.device)
    inv_temp = T.anneal_schedule(int(anneal_sweeps), t_start, t_end, T.dense_scale(W))
    out = T._dense_anneal_on_gpu(W, starts, inv_temp, seed, int(max_descent_sweeps), cost)
    partition = out["best_assign"].reshape(B, n)
    cost_sum = None
    if cost is not None:
        picked = cost.reshape(B, n, 2).gather(2, partition.to(torch.int64).unsqueeze(2)).squeeze(2)
        cost_sum = picked.to(torch.float64).sum(dim=1).to(torch.float32)
    return DenseResult(partition, out["best_score"], cost_sum, out["moves"])


def solve_dense(W, candidates: int = 200, anneal_sweeps: int = 100, seed: int = 0, node_cost=None, *,
                max_descent_sweeps: int = 100, t_start: float = 1.5, t_end: float = 0.15, partitions=None,
                bifurcation_steps: int = 0, bifurcation_dt: float = 1.25,
                bifurcation_c0: Optional[float] = None) -> DenseResult:
    """Max-cut (two classes, no terminals) of dense instances given as matrices: ``W`` is [n, n] or [B, n, n] (B instances
    of one size, 2 <= n <= ``hip.MAX_GRAPH_NODES``), a tensor on the host or the device or a numpy array, symmetric and
    finite (``ValueError`` otherwise; the diagonal is ignored).  No model and no training: ``candidates`` chains per
    instance start from seeded random partitions (drawn by torch on the device; or from ``partitions``), run
    ``anneal_sweeps`` Metropolis sweeps and at most ``max_descent_sweeps`` sweeps of single-move descent on the GPU
    (``gmc_dense_anneal_f32``, include/gcnmaxcut_dense.h), and the best chain of every instance is returned.
    ``node_cost`` [n, 2] / [B, n, 2]: the objective ``cut - sum_v node_cost[v][class_v]`` of :func:`solve`.

    A chain keeps one cached local field per node, decides a visit from it and reads a row of ``W`` only for an accepted
    move - the form for matrices where :func:`solve`'s sparse decoders walk n entries per visit.  The schedule cools from
    ``t_start`` to ``t_end`` in units of ``sqrt(mean_v sum_u w_vu^2)``, the spread of a local field, where the sparse doors
    use the mean absolute weight.  That unit and the defaults are PROVISIONAL: nobody has measured them (DESIGN.md section
    40).  For a given start the kernel's outputs are reproducible bit for bit; the random starts are torch's.

    ``bifurcation_steps`` > 0 (keyword only, default 0: nothing new is launched): the chains start from the partitions of
    that many steps of discrete simulated bifurcation (``gmc_dense_sb_f32``, include/gcnmaxcut_bifurcation.h: all nodes of
    all chains move at once, a step is an fp32 MFMA product) where they started from torch's random bytes; everything
    after it is unchanged.  ``bifurcation_dt`` is the time step, ``bifurcation_c0`` the coupling scale (None:
    ``0.5 / dense_scale(W)``); the start is seeded by ``seed`` on the device.  ``partitions=`` together with
    ``bifurcation_steps > 0`` raises ``ValueError``.  These defaults are the literature's as far as recalled and
    PROVISIONAL as well: nobody has measured them on this code."""
    _check_bifurcation(partitions, bifurcation_steps)
    dev = hip.require_gpu()
    from .Testing import TestingNeuralNetwork as T
    Wd = T.dense_matrices("W", W, dev)
    cost = _dense_cost("node_cost", node_cost, int(Wd.shape[0]), int(Wd.shape[1]), dev)
    return _solve_dense(Wd, cost, candidates, anneal_sweeps, seed, max_descent_sweeps, t_start, t_end, partitions,
                       bifurcation_steps, bifurcation_dt, bifurcation_c0)


def _pair_energy(M: torch.Tensor, lin: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """[B] float64: sum_{i<j} M_ij z_i z_j + sum_i lin_i z_i of z [B, n] (M symmetric, its diagonal ignored)."""
    off = ~torch.eye(M.shape[1], dtype=torch.bool, device=M.device)
    M64 = torch.where(off, M.to(torch.float64), torch.zeros((), dtype=torch.float64, device=M.device))
    z = z.to(torch.float64)
    return 0.5 * torch.einsum("bi,bij,bj->b", z, M64, z) + (lin * z).sum(dim=1)


def solve_ising_dense(J, field=None, candidates: int = 200, anneal_sweeps: int = 100, seed: int = 0, *,
                      max_descent_sweeps: int = 100, t_start: float = 1.5, t_end: float = 0.15,
                      partitions=None, bifurcation_steps: int = 0, bifurcation_dt: float = 1.25,
                      bifurcation_c0: Optional[float] = None) -> DenseIsingResult:
    """Minimises ``H(s) = sum_{i<j} J_ij s_i s_j + sum_i h_i s_i`` over ``s`` in {+1, -1}^n for dense couplings ``J``
    ([n, n] or [B, n, n], symmetric, as :func:`solve_dense` takes ``W``) and ``field`` h ([n] / [B, n]; None: 0) - a
    Sherrington-Kirkpatrick instance, for one.  The mapping is :func:`solve_ising`'s: ``w = 2 J`` (exact in float32),
    class 0 is ``s = +1``, ``node_cost[i] = (h_i, -h_i)``; then ``H(s) = sum_{i<j} J_ij - obj``.  Returns ``spins``
    [B, n] int8, ``energy`` [B] float64 - ``H(spins)`` recounted in float64 from ``J`` and ``h``, not derived from the
    kernel's float32 objective - and the :class:`DenseResult` as ``.result``.  The other keywords, and the provisional
    temperature unit, are :func:`solve_dense`'s."""
    _check_bifurcation(partitions, bifurcation_steps)
    dev = hip.require_gpu()
    from .Testing import TestingNeuralNetwork as T
    Jd = T.dense_matrices("J", J, dev)
    B, n = int(Jd.shape[0]), int(Jd.shape[1])
    h = _dense_vector("field", field, B, n, dev)
    h32 = h.to(torch.float32).reshape(B * n)
    cost = torch.stack([h32, -h32], dim=1).contiguous()
    res = _solve_dense(2.0 * Jd, cost, candidates, anneal_sweeps, seed, max_descent_sweeps, t_start, t_end, partitions,
                       bifurcation_steps, bifurcation_dt, bifurcation_c0)
    spins = (1 - 2 * res.partition).to(torch.int8)
    return DenseIsingResult(spins, _pair_energy(Jd, h, spins), res)


def dense_row_sums(w: torch.Tensor) -> torch.Tensor:
    """[B, n] float32: ``sum_{j != i} w_ij`` of w [B, n, n], every row summed in float32 from +0 over j ascending (one
    elementwise addition per column, so the order is the stated one whatever the device's reductions do)."""
    off = ~torch.eye(w.shape[1], dtype=torch.bool, device=w.device)
    wz = torch.where(off, w, torch.zeros((), dtype=w.dtype, device=w.device))
    acc = torch.zeros(w.shape[:2], dtype=torch.float32, device=w.device)
    for j in range(w.shape[2]):
        acc = acc + wz[:, :, j]
    return acc


def solve_qubo_dense(Q, linear=None, candidates: int = 200, anneal_sweeps: int = 100, seed: int = 0, *,
                     max_descent_sweeps: int = 100, t_start: float = 1.5, t_end: float = 0.15,
                     partitions=None, bifurcation_steps: int = 0, bifurcation_dt: float = 1.25,
                     bifurcation_c0: Optional[float] = None) -> DenseQuboResult:
    """Minimises ``E(x) = sum_i a_i x_i + sum_{i<j} q_ij x_i x_j`` over ``x`` in {0, 1}^n for a dense ``Q`` ([n, n] or
    [B, n, n], symmetric, as :func:`solve_dense` takes ``W``; Beasley / BiqMac style) and ``linear`` a ([n] / [B, n]; None:
    0).  The mapping is :func:`solve_qubo`'s and has no offset: ``w = q / 2``, class 1 is ``x = 1``, ``node_cost[i] =
    (0, a_i + sum_j w_ij)``, the row sums in float32 over j ascending (:func:`dense_row_sums`) and one float32 addition
    per variable; then ``E(x) = -obj``.  Returns ``x`` [B, n] int8, ``energy`` [B] float64 - ``E(x)`` recounted in float64
    from ``Q`` and ``a`` - and the :class:`DenseResult` as ``.result``.  The other keywords, and the provisional
    temperature unit, are :func:`solve_dense`'s."""
    _check_bifurcation(partitions, bifurcation_steps)
    dev = hip.require_gpu()
    from .Testing import TestingNeuralNetwork as T
    Qd = T.dense_matrices("Q", Q, dev)
    B, n = int(Qd.shape[0]), int(Qd.shape[1])
    a = _dense_vector("linear", linear, B, n, dev)
    w = 0.5 * Qd
    cost = torch.zeros((B * n, 2), dtype=torch.float32, device=dev)
    cost[:, 1] = a.to(torch.float32).reshape(B * n) + dense_row_sums(w).reshape(B * n)
    res = _solve_dense(w, cost, candidates, anneal_sweeps, seed, max_descent_sweeps, t_start, t_end, partitions,
                       bifurcation_steps, bifurcation_dt, bifurcation_c0)
    x = res.partition.to(torch.int8)
    return DenseQuboResult(x, _pair_energy(Qd, a, x), res)
