"""TestingNeuralNetwork - the inference harness functions of
``python/Testing/TestingNeuralNetwork.py`` that drive the hot path (BASELINE configs[4]).

Same names, arguments and result dictionaries as the reference for ``assign_partitions``
(:18-46), ``calculate_cut_value`` (:48-64), ``post_processing_optimization`` (:66-98),
``simple_partition_assignment`` (:100-122), ``test_single_graph`` (:124-186) and
``test_multiple_graphs`` (:188-295).  The forward runs through ``GCNSoftmax`` (HIP), the 200
sampling iterations and their cut counts run in one launch of ``gmc_decode_sample_f32``; the
uniform draws still come from numpy's global RNG in the reference's order, so with the same
``np.random.seed`` the sampled assignments and cut values are the reference's, exactly.
With a ``seed`` (argument, or the switch ``GCN_MAXCUT_SAMPLE_SEED``) the uniforms are instead drawn on the GPU by
``gmc_decode_sample_seeded_f32`` from a counter-based hash (extension): numpy's RNG is not touched, nothing is
generated on the host, and a graph's samples depend on the seed and its index in the dataset alone.
``conditional_rounding`` / ``round_dataset`` (extension) round the probabilities by conditional expectations
(``gmc_round_conditional_f32``): one deterministic partition per graph whose cut is not below the expected cut, for
any ``number_classes`` in 2..8.
``sampling_optimization``, ``kway_local_search``, ``kway_annealing`` and ``search_dataset`` (extension) are the seeded
sampler, the local search and the annealing for ``number_classes`` in 2..8 (``gmc_kway_decode_sample_seeded_f32``,
``gmc_kway_refine_anneal_f32``); at three classes they return what the 3-class functions return - the library's
3-class sampler and annealing are the K-class kernels at K = 3.  Those, and ``decode_dataset``, keep refusing any other
class count.
``kway_evolution`` and ``search_dataset(..., generations=G)`` (extension) recombine the annealed candidates of a graph
across generations (``gmc_kway_evolve_f32``): children of two class-aligned parents, annealed and kept when no worse.
``kway_tabu_search`` and ``search_dataset(..., tabu_iterations=I)`` (extension) run a one-flip tabu search over
partitions (``gmc_kway_tabu_f32``): the best single move every iteration, a recency ban with aspiration, the best state
kept.  Off by default.
``kway_tempering`` (extension) runs parallel tempering over partitions of a graph (``gmc_kway_temper_f32``,
include/gcnmaxcut_temper.h): the annealing's sweep on ladders of fixed temperatures with replica exchange between rounds.
``large_conditional_rounding``, ``large_local_search``, ``round_large_dataset``, ``large_sampling_optimization``,
``large_annealing`` and ``search_large_dataset`` (extension) are the same rounding, local search, sampler and annealing
for graphs of up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes (``gmc_large_round_conditional_f32``,
``gmc_large_local_search_f32``, ``gmc_large_sample_seeded_f32``, ``gmc_large_anneal_f32``): a graph shared by several
workgroups, its state in a workspace on the device.
Every K-class function above takes ``terminals`` (default ``True``: nodes 0..K-1 of a graph are fixed to classes
0..K-1, the reference's problem).  ``terminals=False`` is plain max-K-cut: no node is fixed, a graph needs one node, and
the calls go through the ``_t`` entry points of the library with ``terminals = 0``.  The 3-class functions and
``decode_dataset`` keep their terminals.
The reporting / plotting half of the reference module (``analyze_results`` .. ``generate_summary_report``,
:297-638) is presentation code outside the path and is not reproduced.
"""
from __future__ import annotations

import ctypes as C
import os
from time import time
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import hip
from ..graph import GraphBatch, GraphHandle, _host_array, from_networkx


def assign_partitions(node_probs: np.ndarray) -> List[int]:
    """One sample of the post-processing (host form, TestingNeuralNetwork.py:18-46)."""
    out = [0, 1, 2]
    for probs in node_probs[3:]:
        r = float(np.random.rand())
        running = 0.0
        for i, p in enumerate(probs):
            # double running sum, double compare: what `cumulative_prob = 0; += np.float32` does under
            # the reference's pinned NumPy 1.x (envList.txt:105) - and what decode.hip does; written with
            # Python floats so that the installed NumPy's promotion rules do not matter
            running += float(p)
            if r < running:
                out.append(i)
                break
        else:
            out.append(len(probs) - 1)
    return out


SAMPLE_SEED_ENV = "GCN_MAXCUT_SAMPLE_SEED"
_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


def _mix64(z: int) -> int:
    """splitmix64's finaliser on a Python integer (csrc/mix64.h)."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _sample_seed(seed: Optional[int]) -> Optional[int]:
    """The sampler's seed as a uint64, or None for the numpy stream: the argument, else the environment switch
    GCN_MAXCUT_SAMPLE_SEED (read here, at call time; the library itself reads no environment)."""
    if seed is None:
        text = os.environ.get(SAMPLE_SEED_ENV)
        if text is None or not text.strip():
            return None
        try:
            seed = int(text.strip(), 0)
        except ValueError:
            raise ValueError(f"{SAMPLE_SEED_ENV} must be an integer, got {text!r}") from None
    return int(seed) & _M64


def _graph_key(seed: int, index: int) -> int:
    if int(index) < 0:
        raise ValueError(f"a graph's index must be >= 0, got {index}")
    return _mix64((int(seed) + _GOLD * (int(index) + 1)) & _M64)


def sample_keys(seed: int, indices) -> np.ndarray:
    """The keys of the seeded sampler (include/gcnmaxcut.h, gmc_decode_sample_seeded_f32) for the graphs at positions
    ``indices`` of a dataset: ``mix64(seed + GOLD * (index + 1))`` in uint64 arithmetic."""
    return np.array([_graph_key(seed, i) for i in indices], dtype=np.uint64)


def assign_partitions_seeded(node_probs: np.ndarray, seed: int, graph_index: int = 0, iteration: int = 0) -> List[int]:
    """One sample of the seeded post-processing (host form of kway_search.hip's sampler at K = 3, the counterpart of
    :func:`assign_partitions`): iteration ``iteration`` of the graph at position ``graph_index``, the uniform of local
    node l hashed from the graph's key, the iteration and l.  Python integers masked to 64 bits and Python floats."""
    if int(iteration) < 0 or int(iteration) >= 1 << 31:
        raise ValueError(f"iteration must be in 0..2^31-1, got {iteration}")
    key = _graph_key(seed, graph_index)
    out = [0, 1, 2]
    for l, probs in enumerate(node_probs[3:], 3):
        h = _mix64((key + _GOLD * (((int(iteration) << 32) | l) + 1)) & _M64)
        r = float(h >> 11) * 2.0 ** -53          # < 2^53: exact
        c0 = float(probs[0])
        c1 = c0 + float(probs[1])
        out.append(0 if r < c0 else (1 if r < c1 else 2))
    return out


def calculate_cut_value(partition_assignment: List[int], graph) -> int:
    """Sum of the weights of edges whose endpoints differ (TestingNeuralNetwork.py:48-64)."""
    k = len(partition_assignment)
    total = 0
    for u, v, data in graph.edges(data=True):
        if u < k and v < k and partition_assignment[u] != partition_assignment[v]:
            total += data.get('weight', 1)
    return total


def simple_partition_assignment(node_probabilities: torch.Tensor) -> List[int]:
    """argmax decode with the terminals forced to 0,1,2 (TestingNeuralNetwork.py:100-122); for probabilities of K != 3
    columns the first min(K, n) nodes are the terminals of classes 0..K-1."""
    part = torch.argmax(node_probabilities, dim=1).cpu().numpy().tolist()
    K = int(node_probabilities.shape[1])
    if K == 3:   # the reference's lines: they differ from the loop below only for n < 3, where they fix nothing
        if len(part) >= 3:
            part[0], part[1], part[2] = 0, 1, 2
        return part
    for i in range(min(K, len(part))):
        part[i] = i
    return part


def _three_classes_only(what: str, classes: int) -> None:
    """The numpy-stream sampler and the local search (decode.hip, refine.hip) are 3-class, and so are the entry points
    these functions call (gmc_decode_sample_seeded_f32, gmc_refine_anneal_f32: kway_search.hip at K = 3)."""
    if int(classes) != 3:
        raise ValueError(f"{what} is implemented for number_classes = 3 only, got {int(classes)} classes: use the "
                         "argmax decode (simple_partition_assignment) for a model with another number_classes")


def _decoder_graph_size(what: str, nodes: int) -> None:
    """The sampler, the rounding and the searches keep a graph's state in one workgroup's LDS (include/gcnmaxcut.h:
    GMC_MAX_GRAPH_NODES)."""
    if int(nodes) > hip.MAX_GRAPH_NODES:
        raise ValueError(f"{what} is implemented for graphs of up to {hip.MAX_GRAPH_NODES} nodes, got one with {int(nodes)}: "
                         "a larger graph gets the argmax partition (evaluate_model for its loss, "
                         "simple_partition_assignment on net(g, None) under torch.no_grad() for the assignment), or "
                         "the rounding and the local search of large_conditional_rounding, large_local_search and "
                         "round_large_dataset, or the sampler and the annealing of large_sampling_optimization, "
                         "large_annealing and search_large_dataset")


def _best_outputs(batch: GraphBatch):
    """Where every search and sampler leaves its pick: best_assign [R], best_cut [B] and the index of the best
    candidate [B]."""
    dev = batch.device
    return (torch.empty(batch.R, dtype=torch.int32, device=dev), torch.empty(batch.B, dtype=torch.float32, device=dev),
            torch.empty(batch.B, dtype=torch.int32, device=dev))


def _search_outputs(batch: GraphBatch, cands: int):
    """What every search and sampler writes: cut_all [B, cands], then :func:`_best_outputs`."""
    return (torch.empty((batch.B, cands), dtype=torch.float32, device=batch.device),) + _best_outputs(batch)


def _sample_outputs(batch: GraphBatch, iterations: int, keep_samples: bool, seed: int, indices):
    """What a seeded sampler reads and writes: gkey [B] (the keys of the graphs at dataset positions ``indices``,
    default 0..B-1), assign_all [iterations, R] int8 (None unless ``keep_samples``), then :func:`_search_outputs`."""
    keys = sample_keys(seed, range(batch.B) if indices is None else indices)
    if keys.size != batch.B:
        raise ValueError(f"{keys.size} graph indices for a batch of {batch.B} graphs")
    dev = batch.device
    gkey = torch.from_numpy(keys.view(np.int64)).to(dev) if batch.B else torch.zeros(1, dtype=torch.int64, device=dev)
    assign_all = torch.empty((iterations, batch.R), dtype=torch.int8, device=dev) if keep_samples else None
    return (gkey, assign_all) + _search_outputs(batch, iterations)


def _schedule_tensors(inv_temp: np.ndarray, dev):
    """An annealing schedule on the device: inv_t [sweeps] and the level table (both None without sweeps), and sweeps."""
    sweeps = int(len(inv_temp))
    if not sweeps:
        return None, None, 0
    return (torch.from_numpy(np.ascontiguousarray(inv_temp, np.float32)).to(dev),
            torch.from_numpy(anneal_levels()).to(dev), sweeps)


def _sample_on_gpu(batch: GraphBatch, P: torch.Tensor, iterations: int, seed: Optional[int] = None, indices=None,
                   keep_samples: bool = True):
    """Draw the uniforms in the reference's order and run the fused sampler + cut count.  With ``seed`` (a uint64; the
    callers resolve argument and environment with ``_sample_seed``) the seeded sampler runs instead: the graphs'
    dataset positions ``indices`` (default 0..B-1) make their keys, no uniform exists on the host, and the
    [iterations, R] samples are allocated only if ``keep_samples`` (else ``assign_all`` is returned as None)."""
    _three_classes_only("the sampling post-processing", P.shape[1])
    p = hip.ptr
    if seed is not None:
        gkey, assign_all, cut_all, best_assign, best_cut, best_iter = _sample_outputs(batch, iterations, keep_samples,
                                                                                      seed, indices)
        rc = hip.load().gmc_decode_sample_seeded_f32(batch.ref(), p(P.contiguous()), p(gkey), iterations, p(assign_all),
                                                     p(cut_all), p(best_assign), p(best_cut), p(best_iter), hip.stream())
        hip.check(rc, "gmc_decode_sample_seeded_f32")
        return best_assign, best_cut, cut_all, assign_all
    sizes = [int(n) - 3 for n in batch.sizes]
    draws = [np.random.rand(iterations, m) for m in sizes]          # graph -> iteration -> node
    uoff = np.zeros(batch.B + 1, np.int64)
    np.cumsum([d.size for d in draws], out=uoff[1:])
    dev = batch.device
    u = torch.from_numpy(np.concatenate([d.ravel() for d in draws]) if uoff[-1] else np.zeros(1)).to(dev)
    uo = torch.from_numpy(uoff).to(dev)
    assign_all = torch.empty((iterations, batch.R), dtype=torch.int8, device=dev)
    cut_all, best_assign, best_cut, best_iter = _search_outputs(batch, iterations)
    rc = hip.load().gmc_decode_sample_f32(batch.ref(), p(P.contiguous()), p(u), p(uo), iterations, p(assign_all),
                                          p(cut_all), p(best_assign), p(best_cut), p(best_iter), hip.stream())
    hip.check(rc, "gmc_decode_sample_f32")
    return best_assign, best_cut, cut_all, assign_all


def _refine_on_gpu(batch: GraphBatch, assign: torch.Tensor, max_sweeps: int):
    """Local search (gmc_refine_local_f32) over the candidates assign [cands, R] int8, refined in place; returns the
    best refined assignment [R], its cut and candidate index per graph."""
    cands = int(assign.shape[0])
    order, cgoff, cptr = batch.refine_order()
    cut_all, best_assign, best_cut, best_idx = _search_outputs(batch, cands)
    p = hip.ptr
    rc = hip.load().gmc_refine_local_f32(batch.ref(), p(order), p(cgoff), p(cptr), cands, p(assign), int(max_sweeps),
                                         p(cut_all), p(best_assign), p(best_cut), p(best_idx), None, hip.stream())
    hip.check(rc, "gmc_refine_local_f32")
    return best_assign, best_cut, best_idx


def anneal_levels() -> np.ndarray:
    """The level table ``gmc_refine_anneal_f32`` compares ``delta / T`` against: ``-log((i + 0.5) / 1024)`` for
    i = 0..1023, quantiles of an exponential variate (float64, rounded to float32 once).  With it the kernel's move
    rule is a Metropolis test at 10-bit resolution, and the device evaluates neither exp nor log."""
    i = np.arange(hip.ANNEAL_LEVELS, dtype=np.float64)
    return (-np.log((i + 0.5) / hip.ANNEAL_LEVELS)).astype(np.float32)


def anneal_schedule(sweeps: int, t_start: float = 1.5, t_end: float = 0.15, scale: float = 1.0) -> np.ndarray:
    """float32 ``1 / T_s`` of a geometric cooling ``T_s = scale * t_start * (t_end / t_start) ** (s / max(sweeps-1, 1))``
    (float64, rounded once).  ``scale``: the mean edge weight of the batch (1 for unit weights)."""
    if sweeps < 0:
        raise ValueError(f"sweeps must be >= 0, got {sweeps}")
    if not (t_start > 0 and t_end > 0 and scale > 0):
        raise ValueError("t_start, t_end and scale must be > 0")
    s = np.arange(int(sweeps), dtype=np.float64)
    temps = float(scale) * float(t_start) * (float(t_end) / float(t_start)) ** (s / max(int(sweeps) - 1, 1))
    return (1.0 / temps).astype(np.float32)


def _anneal_on_gpu(batch: GraphBatch, assign: torch.Tensor, inv_temp: np.ndarray, seed: int, max_descent_sweeps: int):
    """Annealing + descent (gmc_refine_anneal_f32) over the candidates assign [cands, R] int8, in place; returns the
    best annealed assignment [R], its cut and candidate index per graph."""
    cands = int(assign.shape[0])
    order, cgoff, cptr = batch.refine_order()
    inv_t, levels, sweeps = _schedule_tensors(inv_temp, batch.device)
    cut_all, best_assign, best_cut, best_idx = _search_outputs(batch, cands)
    p = hip.ptr
    rc = hip.load().gmc_refine_anneal_f32(batch.ref(), p(order), p(cgoff), p(cptr), cands, p(assign), p(inv_t), sweeps,
                                          p(levels), int(seed) & (2 ** 64 - 1), int(max_descent_sweeps), p(cut_all),
                                          p(best_assign), p(best_cut), p(best_idx), None, None, hip.stream())
    hip.check(rc, "gmc_refine_anneal_f32")
    return best_assign, best_cut, best_idx


def _mean_edge_weight(batch: GraphBatch) -> float:
    vals = batch.host.vals
    return 1.0 if vals is None else float(np.mean(vals, dtype=np.float64))


def _as_number(x: float):
    return int(x) if float(x).is_integer() else float(x)


def _graph_batch(graph, dev, large: bool = False) -> GraphBatch:
    """The batch of a one-graph function: a networkx graph, or on the large route a ``GraphHandle`` as well."""
    handle = graph if large and isinstance(graph, GraphHandle) else from_networkx(graph)
    return GraphBatch([handle], None, dev)


def _one_candidate(part: np.ndarray, dev) -> torch.Tensor:
    """A checked partition [n] as the searches' candidates [1, n] int8 on the device."""
    return torch.from_numpy(part.astype(np.int8)).to(dev).reshape(1, -1)


def _graph_result(assign: torch.Tensor, cut: torch.Tensor) -> Tuple[List[int], Any]:
    """What a one-graph function returns: the assignment as a list and its cut as a number."""
    return assign.cpu().tolist(), _as_number(cut.item())


def _graph_probabilities(what: str, node_probabilities, graph, terminals: bool) -> Tuple[torch.Tensor, int]:
    """The checks the one-graph functions share for node probabilities [n, K], all on the host: two dimensions, the
    class count (refused in ``what``'s name), the terminals' room, one row per node.  Returns them as a tensor, and K."""
    probs = node_probabilities if isinstance(node_probabilities, torch.Tensor) else torch.from_numpy(np.asarray(node_probabilities))
    if probs.dim() != 2:
        raise ValueError(f"node_probabilities must be [n, number_classes], got {tuple(probs.shape)}")
    K = _search_classes(what, probs.shape[1])
    n = graph.number_of_nodes()
    _check_graph_size(n, K, terminals)
    if probs.shape[0] != n:
        raise ValueError(f"node_probabilities has {probs.shape[0]} rows, the graph {n} nodes")
    return probs, K


def post_processing_optimization(node_probabilities, graph, iterations: int = 200, *, seed: Optional[int] = None,
                                 graph_index: int = 0) -> Tuple[List[int], int]:
    """Best of ``iterations`` random samples (TestingNeuralNetwork.py:66-98), on the GPU.  ``seed`` (extension; None
    reads GCN_MAXCUT_SAMPLE_SEED, and without either the numpy stream of the reference is drawn): the samples of the
    seeded sampler for the graph at position ``graph_index`` of its dataset; numpy's RNG is then left alone."""
    dev = hip.require_gpu()
    seed = _sample_seed(seed)
    probs = node_probabilities if isinstance(node_probabilities, torch.Tensor) else torch.from_numpy(np.asarray(node_probabilities))
    probs = probs.detach().to(dev, torch.float32)
    if iterations <= 0:
        return None, -float('inf')
    best_assign, best_cut, _, _ = _sample_on_gpu(_graph_batch(graph, dev), probs, iterations, seed, [graph_index],
                                                 keep_samples=False)
    return _graph_result(best_assign, best_cut)


def local_search_optimization(partition_assignment, graph, max_sweeps: int = 100,
                              number_classes: int = 3) -> Tuple[List[int], Any]:
    """Refine one assignment of ``graph`` (e.g. ``simple_partition_assignment``'s) by single-node moves on the GPU
    (extension, include/gcnmaxcut.h ``gmc_refine_local_f32``): nodes 0, 1, 2 keep their classes, every other node
    moves to the class that cuts the most of its edge weight, sweep after sweep, until a sweep moves nothing or
    ``max_sweeps`` have run.  Returns the refined assignment and its cut value.  The kernel is 3-class - it would treat
    nodes 0, 1, 2 of a 2-class partition as terminals and move nodes into class 2 - so ``number_classes`` other than 3
    (say which model the partition comes from) raises ``ValueError``."""
    _three_classes_only("local_search_optimization", number_classes)
    dev = hip.require_gpu()
    part = np.asarray(list(partition_assignment), dtype=np.int64)
    n = graph.number_of_nodes()
    if part.shape != (n,):
        raise ValueError(f"partition_assignment has {part.size} entries, the graph {n} nodes")
    if part.size and (int(part.min()) < 0 or int(part.max()) > 2):
        raise ValueError("partition_assignment holds a class outside 0..2 (the refinement kernels are written for "
                         "number_classes = 3)")
    if max_sweeps < 0:
        raise ValueError(f"max_sweeps must be >= 0, got {max_sweeps}")
    best_assign, best_cut, _ = _refine_on_gpu(_graph_batch(graph, dev), _one_candidate(part, dev), max_sweeps)
    return _graph_result(best_assign, best_cut)


def annealing_optimization(partition_assignment, graph, sweeps: int = 100, t_start: float = 1.5, t_end: float = 0.15,
                           seed: int = 0, max_descent_sweeps: int = 100, number_classes: int = 3) -> Tuple[List[int], Any]:
    """Anneal one assignment of ``graph`` on the GPU past the single-move local optima ``local_search_optimization``
    stops at (extension, include/gcnmaxcut.h ``gmc_refine_anneal_f32``): ``sweeps`` Metropolis sweeps cooling from
    ``t_start`` to ``t_end`` (in units of the graph's mean edge weight), the best state passed through kept, then the
    local search from it.  Nodes 0, 1, 2 keep their classes; the result is never worse than the input and is
    reproducible from ``seed``.  Returns the assignment and its cut value.  3-class like
    :func:`local_search_optimization`: ``number_classes`` other than 3 raises ``ValueError``."""
    _three_classes_only("annealing_optimization", number_classes)
    dev = hip.require_gpu()
    part = np.asarray(list(partition_assignment), dtype=np.int64)
    n = graph.number_of_nodes()
    if part.shape != (n,):
        raise ValueError(f"partition_assignment has {part.size} entries, the graph {n} nodes")
    if part.size and (int(part.min()) < 0 or int(part.max()) > 2):
        raise ValueError("partition_assignment holds a class outside 0..2 (the refinement kernels are written for "
                         "number_classes = 3)")
    if sweeps < 0 or max_descent_sweeps < 0:
        raise ValueError(f"sweeps and max_descent_sweeps must be >= 0, got {sweeps} and {max_descent_sweeps}")
    batch = _graph_batch(graph, dev)
    inv_temp = anneal_schedule(sweeps, t_start, t_end, _mean_edge_weight(batch))
    best_assign, best_cut, _ = _anneal_on_gpu(batch, _one_candidate(part, dev), inv_temp, seed, max_descent_sweeps)
    return _graph_result(best_assign, best_cut)


def _search_classes(what: str, classes: int) -> int:
    """The class count of the K-class decoders (round.hip and kway_search.hip are written for 2..8 classes)."""
    K = int(classes)
    if not 2 <= K <= hip.KWAY_MAX_CLASSES:
        raise ValueError(f"{what} takes number_classes in 2..{hip.KWAY_MAX_CLASSES}, got {K} classes")
    return K


def _rounding_classes(classes: int) -> int:
    return _search_classes("conditional rounding", classes)


def _cost_tensor(batch: GraphBatch, K: int, node_cost) -> Optional[torch.Tensor]:
    """``node_cost`` as the ``_c`` entry points read it: a contiguous [R, K] float32 tensor on the batch's device."""
    if node_cost is None:
        return None
    if not isinstance(node_cost, torch.Tensor) or tuple(node_cost.shape) != (batch.R, K):
        raise ValueError(f"node_cost must be a [{batch.R}, {K}] tensor (one row per batch row, one column per class)")
    return node_cost.to(batch.device, torch.float32).contiguous()


def _graph_cost(what: str, node_cost, n: int, K: int) -> Optional[torch.Tensor]:
    """``node_cost`` of a one-graph search -> a [n, K] float32 tensor (host), or None: floats, the shape, finite."""
    if node_cost is None:
        return None
    a = _host_array(node_cost)
    if not np.issubdtype(a.dtype, np.floating) or a.shape != (n, K):
        raise ValueError(f"{what}: node_cost must hold floats of shape [{n}, {K}], got {a.dtype} {tuple(a.shape)}")
    a = np.ascontiguousarray(a, np.float32)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what}: node_cost holds values that are not finite (in float32)")
    return torch.from_numpy(a)


def _call(name: str, terminals: bool, head: tuple, tail: tuple, node_cost: Optional[torch.Tensor] = None, *,
          t_twin: bool = True) -> None:
    """Calls one entry point of the family ``name`` with ``head + middle + tail`` and raises on a status code.  With
    ``node_cost`` ([R, K] float32 on the device) it is the ``_c`` twin, whose middle is ``terminals`` and the cost array.
    Without one, a family with a ``_t`` twin (the rounding, the samplers, the annealings) calls ``name`` itself, which
    has no middle, with terminals and the ``_t`` twin with ``terminals = 0`` without them; a family without one
    (``t_twin=False``: the chain searches) calls ``name``, whose middle is ``terminals``."""
    flag = int(bool(terminals))
    if node_cost is not None:
        name, middle = name[:-len("_f32")] + "_c_f32", (flag, hip.ptr(node_cost))
    elif not t_twin:
        middle = (flag,)
    elif terminals:
        middle = ()
    else:
        name, middle = name[:-len("_f32")] + "_t_f32", (0,)
    hip.check(getattr(hip.load(), name)(*head, *middle, *tail), name)


def _no_large_cost(large: bool, node_cost) -> None:
    """The large entry points (gmc_large_*) have no ``_c`` twin."""
    if large and node_cost is not None:
        raise NotImplementedError("the decoders for graphs beyond hip.MAX_GRAPH_NODES nodes (gmc_large_*) take no "
                                  "per-node costs: node_cost must be None with large=True")


def _first_argmax(P: torch.Tensor) -> torch.Tensor:
    """The first maximum of every row of P [R, K] as int32 [R]: the argmax decode when no row is overridden."""
    K = P.shape[1]
    ids = torch.arange(K, device=P.device, dtype=torch.int32).expand_as(P)
    top = P.max(dim=1, keepdim=True).values
    return torch.where(P == top, ids, torch.full_like(ids, K)).min(dim=1).values.clamp_(max=K - 1)


def _round_on_gpu(batch: GraphBatch, P: torch.Tensor, descent_sweeps: int, terminals: bool = True, node_cost=None, *,
                  large: bool = False):
    """Rounding by conditional expectations + descent (gmc_round_conditional_f32) of P [R, K] for every graph of the
    batch, one launch; returns the assignment [R] int8, and per graph its cut, the expected cut and the descent sweeps
    run.  ``node_cost`` [R, K]: per-node class costs (gmc_round_conditional_c_f32) - cut and expected cut are then the
    objective, cut minus cost, and its expectation.  ``large``: through gmc_large_round_conditional_f32 - the same rule
    with a graph shared by several workgroups, for graphs of up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes."""
    _no_large_cost(large, node_cost)
    K = _rounding_classes(P.shape[1])
    node_cost = _cost_tensor(batch, K, node_cost)
    if descent_sweeps < 0:
        raise ValueError(f"descent_sweeps must be >= 0, got {descent_sweeps}")
    _needs_terminals(batch, K, terminals)
    dev = batch.device
    assign = torch.empty(batch.R, dtype=torch.int8, device=dev)
    cut = torch.empty(batch.B, dtype=torch.float32, device=dev)
    expected = torch.empty(batch.B, dtype=torch.float32, device=dev)
    sweeps = torch.empty(batch.B, dtype=torch.int32, device=dev)
    if batch.B == 0:   # nothing to launch (empty tensors have no device pointer to hand over)
        return assign, cut, expected, sweeps
    order, cgoff, cptr = batch.refine_order(K, terminals)
    p = hip.ptr
    name, classes, scratch = "gmc_round_conditional_f32", (), ()
    if large:
        ws = _large_workspace(batch, K)
        name, classes, scratch = "gmc_large_round_conditional_f32", (batch.refine_classes(K, terminals),), (p(ws), ws.numel())
    _call(name, terminals, (batch.ref(), p(P.contiguous()), K),
          (p(order), p(cgoff), p(cptr), *classes, int(descent_sweeps), *scratch, p(assign), p(cut), p(expected), p(sweeps),
           hip.stream()), node_cost)
    return assign, cut, expected, sweeps


def conditional_rounding(node_probabilities, graph, descent_sweeps: int = 0,
                         terminals: bool = True) -> Tuple[List[int], Any]:
    """Round the node probabilities of ``graph`` ([n, K], K = number_classes in 2..8, nodes 0..K-1 the terminals) into
    one partition by conditional expectations on the GPU (extension, include/gcnmaxcut.h
    ``gmc_round_conditional_f32``): every node in turn takes the class that keeps the expected cut of the still
    unrounded rest from falling, so the cut returned is at least the expected cut of rounding every node independently
    from its row - what ``loss="expected_cut"`` trains on - deterministic, one visit per node.  ``descent_sweeps > 0``
    then runs that many sweeps of the local search's rule at K classes (until one moves nothing).  Returns the
    assignment and its cut value.  ``terminals=False``: no node is fixed, every node is rounded (and may move)."""
    return _round_graph(node_probabilities, graph, descent_sweeps, terminals, large=False)


def _round_graph(node_probabilities, graph, descent_sweeps: int, terminals: bool, large: bool) -> Tuple[List[int], Any]:
    probs, _ = _graph_probabilities("conditional rounding", node_probabilities, graph, terminals)
    if descent_sweeps < 0:
        raise ValueError(f"descent_sweeps must be >= 0, got {descent_sweeps}")
    dev = hip.require_gpu()
    probs = probs.detach().to(dev, torch.float32)
    assign, cut, _, _ = _round_on_gpu(_graph_batch(graph, dev, large), probs, descent_sweeps, terminals, large=large)
    return _graph_result(assign, cut)


# ---- the rounding and the local search for graphs beyond hip.MAX_GRAPH_NODES nodes (extension) ----------------------
def _large_workspace(batch: GraphBatch, K: int) -> torch.Tensor:
    """The scratch of gmc_large_round_conditional_f32 / gmc_large_local_search_f32 (not zeroed: the calls write every
    word they read)."""
    need = int(hip.load().gmc_large_round_workspace_bytes(batch.ref(), K))
    if need <= 0:
        raise hip.HipExtensionError(f"gmc_large_round_workspace_bytes refused the batch (number_classes = {K})")
    return torch.empty(need, dtype=torch.uint8, device=batch.device)


def large_conditional_rounding(node_probabilities, graph, descent_sweeps: int = 0,
                               terminals: bool = True) -> Tuple[List[int], Any]:
    """:func:`conditional_rounding` for a graph of any size from number_classes to ``hip.LARGE_MAX_GRAPH_NODES`` nodes
    (extension, include/gcnmaxcut.h ``gmc_large_round_conditional_f32``): the same rule, arguments and results - on a
    graph :func:`conditional_rounding` takes, the same assignment - with the graph shared by several workgroups and
    one launch per colour class.  It issues every launch of ``descent_sweeps`` sweeps whenever the descent converges
    (a converged graph costs nothing but the launches), so give it the sweeps the descent may need, not a huge bound."""
    return _round_graph(node_probabilities, graph, descent_sweeps, terminals, large=True)


def large_local_search(partition_assignment, graph, number_classes: int, max_sweeps: int = 100,
                       terminals: bool = True) -> Tuple[List[int], Any]:
    """:func:`kway_local_search` for a graph of any size from number_classes to ``hip.LARGE_MAX_GRAPH_NODES`` nodes
    (extension, include/gcnmaxcut.h ``gmc_large_local_search_f32``): the same rule, arguments and results - on a graph
    :func:`kway_local_search` takes, the same assignment - with the graph shared by several workgroups.  Every launch
    of ``max_sweeps`` sweeps is issued whenever the search converges."""
    K, part = _kway_partition("large_local_search", partition_assignment, graph, number_classes, terminals)
    if max_sweeps < 0:
        raise ValueError(f"max_sweeps must be >= 0, got {max_sweeps}")
    dev = hip.require_gpu()
    batch = _graph_batch(graph, dev, large=True)
    assign = torch.from_numpy(part.astype(np.int8)).to(dev)
    cut = torch.empty(1, dtype=torch.float32, device=dev)
    order, cgoff, cptr = batch.refine_order(K, terminals)
    ws = _large_workspace(batch, K)
    p = hip.ptr
    _call("gmc_large_local_search_f32", terminals, (batch.ref(), K),
          (p(order), p(cgoff), p(cptr), batch.refine_classes(K, terminals), int(max_sweeps), p(ws), ws.numel(), p(assign),
           p(cut), None, hip.stream()))
    return _graph_result(assign, cut)


# ---- the seeded sampler and the annealing for graphs beyond hip.MAX_GRAPH_NODES nodes (extension) -------------------
def _large_search_workspace(batch: GraphBatch, K: int, cands: int) -> torch.Tensor:
    """The scratch of gmc_large_sample_seeded_f32 / gmc_large_anneal_f32 for ``cands`` candidates (not zeroed: the
    calls write every word they read)."""
    need = int(hip.load().gmc_large_search_workspace_bytes(batch.ref(), K, int(cands)))
    if need <= 0:
        raise hip.HipExtensionError(f"gmc_large_search_workspace_bytes refused the batch (number_classes = {K}, "
                                    f"{int(cands)} candidates)")
    return torch.empty(need, dtype=torch.uint8, device=batch.device)


def large_sampling_optimization(node_probabilities, graph, iterations: int = 200, *, seed: int = 0,
                                graph_index: int = 0, terminals: bool = True) -> Tuple[List[int], Any]:
    """:func:`sampling_optimization` for a graph of any size from number_classes to ``hip.LARGE_MAX_GRAPH_NODES`` nodes
    (extension, include/gcnmaxcut.h ``gmc_large_sample_seeded_f32``): the same draws, arguments and results - on a
    graph :func:`sampling_optimization` takes, the same assignment - with the graph shared by several workgroups.  The
    samples live on the device while they are scored: about ``iterations`` bytes per node."""
    return _sample_graph("large_sampling_optimization", node_probabilities, graph, iterations, seed, graph_index,
                         terminals, large=True)


def large_annealing(partition_assignment, graph, number_classes: int, sweeps: int = 100, t_start: float = 1.5,
                    t_end: float = 0.15, seed: int = 0, max_descent_sweeps: int = 100,
                    terminals: bool = True) -> Tuple[List[int], Any]:
    """:func:`kway_annealing` for a graph of any size from number_classes to ``hip.LARGE_MAX_GRAPH_NODES`` nodes
    (extension, include/gcnmaxcut.h ``gmc_large_anneal_f32``): the same rule, arguments and results - on a graph
    :func:`kway_annealing` takes with unit or integer weights, the same assignment - with the graph shared by several
    workgroups and one launch per colour class.  Every launch of ``sweeps`` annealing and ``max_descent_sweeps`` descent
    sweeps is issued whenever the descent converges, so give the descent the sweeps it may need, not a huge bound."""
    return _anneal_graph("large_annealing", partition_assignment, graph, number_classes, sweeps, t_start, t_end, seed,
                         max_descent_sweeps, terminals, large=True)


# ---- the seeded sampler, the local search and the annealing for number_classes K in 2..8 (extension) -----------------
def assign_partitions_seeded_kway(node_probs: np.ndarray, seed: int, graph_index: int = 0, iteration: int = 0,
                                  terminals: bool = True) -> List[int]:
    """:func:`assign_partitions_seeded` for probabilities of K = 2..8 columns (host form of kway_search.hip's sampler):
    nodes 0..K-1 are the terminals, node l >= K takes the first class j in 0..K-2 whose running double sum exceeds the
    hashed uniform, else class K-1 (no compare against the last sum).  At K = 3 it is :func:`assign_partitions_seeded`.
    ``terminals=False``: every node, 0..K-1 included, is drawn by that rule with its own local id in the counter."""
    probs_all = np.asarray(node_probs)
    if probs_all.ndim != 2:
        raise ValueError(f"node_probs must be [n, number_classes], got {tuple(probs_all.shape)}")
    K = _search_classes("assign_partitions_seeded_kway", probs_all.shape[1])
    if int(iteration) < 0 or int(iteration) >= 1 << 31:
        raise ValueError(f"iteration must be in 0..2^31-1, got {iteration}")
    key = _graph_key(int(seed) & _M64, graph_index)
    first = K if terminals else 0
    out = list(range(min(first, len(probs_all))))
    for l, probs in enumerate(probs_all[first:], first):
        h = _mix64((key + _GOLD * (((int(iteration) << 32) | l) + 1)) & _M64)
        r = float(h >> 11) * 2.0 ** -53          # < 2^53: exact
        running = float(probs[0])
        for j in range(K - 1):
            if j:
                running = running + float(probs[j])
            if r < running:
                out.append(j)
                break
        else:
            out.append(K - 1)
    return out


def _check_graph_size(n: int, K: int, terminals: bool = True) -> None:
    """One graph's room for its terminals: K nodes with them, one node without."""
    if terminals and n < K:
        raise ValueError(f"number_classes = {K}: the graph needs at least {K} nodes (nodes 0..{K - 1} are the "
                         f"terminals), got {n}")
    if n < 1:
        raise ValueError("the graph has no nodes")


def _needs_terminals(batch: GraphBatch, K: int, terminals: bool = True) -> None:
    """The batch form of :func:`_check_graph_size`: every graph has room for its terminals (K nodes), or, without
    terminals, at least one node."""
    if batch.B and not terminals:
        if int(batch.sizes.min()) < 1:
            raise ValueError("every graph needs at least one node, got an empty one")
        return
    if batch.B and int(batch.sizes.min()) < K:
        raise ValueError(f"number_classes = {K}: every graph needs at least {K} nodes (nodes 0..{K - 1} are the "
                         f"terminals), got one with {int(batch.sizes.min())}")


def _kway_sample_on_gpu(batch: GraphBatch, P: torch.Tensor, iterations: int, seed: int, indices, keep_samples: bool,
                        terminals: bool = True, node_cost=None, *, large: bool = False,
                        workspace: Optional[torch.Tensor] = None):
    """The seeded sampler at K = P.shape[1] classes (gmc_kway_decode_sample_seeded_f32), as the seeded
    ``_sample_on_gpu``.  ``node_cost`` [R, K]: the samples are scored by cut minus cost
    (gmc_kway_decode_sample_seeded_c_f32).  ``large``: through gmc_large_sample_seeded_f32 - the same draws with a graph
    shared by several workgroups, for graphs of up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes, in ``workspace``
    (:func:`_large_search_workspace`; None: its own)."""
    _no_large_cost(large, node_cost)
    K = _search_classes("the K-class sampler", P.shape[1])
    node_cost = _cost_tensor(batch, K, node_cost)
    _needs_terminals(batch, K, terminals)
    gkey, assign_all, cut_all, best_assign, best_cut, best_iter = _sample_outputs(batch, iterations, keep_samples, seed,
                                                                                  indices)
    p = hip.ptr
    name, scratch = "gmc_kway_decode_sample_seeded_f32", ()
    if large:
        if batch.B == 0:   # nothing to launch (the workspace query refuses an empty batch)
            return best_assign, best_cut, cut_all, assign_all
        ws = _large_search_workspace(batch, K, iterations) if workspace is None else workspace
        name, scratch = "gmc_large_sample_seeded_f32", (p(ws), ws.numel())
    _call(name, terminals, (batch.ref(), p(P.contiguous()), K),
          (p(gkey), iterations, p(assign_all), *scratch, p(cut_all), p(best_assign), p(best_cut), p(best_iter),
           hip.stream()), node_cost)
    return best_assign, best_cut, cut_all, assign_all


def sampling_optimization(node_probabilities, graph, iterations: int = 200, *, seed: int = 0,
                          graph_index: int = 0, terminals: bool = True) -> Tuple[List[int], Any]:
    """Best of ``iterations`` seeded samples of the node probabilities [n, K], K = number_classes in 2..8 (extension,
    include/gcnmaxcut.h ``gmc_kway_decode_sample_seeded_f32``): what ``post_processing_optimization(..., seed=seed)``
    does for a 3-class model - and, at K = 3, returns.  Nodes 0..K-1 are the terminals; ``graph_index`` is the graph's
    position in its dataset.  Returns the assignment and its cut value."""
    return _sample_graph("sampling_optimization", node_probabilities, graph, iterations, seed, graph_index, terminals,
                         large=False)


def _sample_graph(what: str, node_probabilities, graph, iterations: int, seed: int, graph_index: int, terminals: bool,
                  large: bool) -> Tuple[List[int], Any]:
    probs, _ = _graph_probabilities(what, node_probabilities, graph, terminals)
    dev = hip.require_gpu()
    probs = probs.detach().to(dev, torch.float32)
    if iterations <= 0:
        return None, -float('inf')
    best_assign, best_cut, _, _ = _kway_sample_on_gpu(_graph_batch(graph, dev, large), probs, iterations,
                                                      int(seed) & _M64, [graph_index], keep_samples=False,
                                                      terminals=terminals, large=large)
    return _graph_result(best_assign, best_cut)


def _kway_anneal_on_gpu(batch: GraphBatch, K: int, assign: torch.Tensor, inv_temp: np.ndarray, seed: int,
                        max_descent_sweeps: int, terminals: bool = True, node_cost=None, *, large: bool = False,
                        workspace: Optional[torch.Tensor] = None):
    """Annealing + descent at K classes (gmc_kway_refine_anneal_f32) over the candidates assign [cands, R] int8, in
    place; returns the best assignment [R], its cut and candidate index per graph.  No annealing sweeps: the K-class
    local search.  ``node_cost`` [R, K]: moves and scores follow cut minus cost (gmc_kway_refine_anneal_c_f32).
    ``large``: through gmc_large_anneal_f32, for graphs of up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes, in ``workspace``
    (:func:`_large_search_workspace`; None: its own)."""
    _no_large_cost(large, node_cost)
    _needs_terminals(batch, K, terminals)
    node_cost = _cost_tensor(batch, K, node_cost)
    cands = int(assign.shape[0])
    cut_all, best_assign, best_cut, best_idx = _search_outputs(batch, cands)
    if large and batch.B == 0:   # nothing to launch (the workspace query refuses an empty batch)
        return best_assign, best_cut, best_idx
    order, cgoff, cptr = batch.refine_order(K, terminals)
    inv_t, levels, sweeps = _schedule_tensors(inv_temp, batch.device)
    p = hip.ptr
    name, classes, scratch = "gmc_kway_refine_anneal_f32", (), ()
    if large:
        ws = _large_search_workspace(batch, K, cands) if workspace is None else workspace
        name, classes, scratch = "gmc_large_anneal_f32", (batch.refine_classes(K, terminals),), (p(ws), ws.numel())
    _call(name, terminals, (batch.ref(), K),
          (p(order), p(cgoff), p(cptr), *classes, cands, p(assign), p(inv_t), sweeps, p(levels), int(seed) & _M64,
           int(max_descent_sweeps), *scratch, p(cut_all), p(best_assign), p(best_cut), p(best_idx), None, None,
           hip.stream()), node_cost)
    return best_assign, best_cut, best_idx


def _kway_partition(what: str, partition_assignment, graph, number_classes: int,
                    terminals: bool = True) -> Tuple[int, np.ndarray]:
    """The checks the K-class searches share: the class count, the length, the class values, the terminals' room."""
    K = _search_classes(what, number_classes)
    part = np.asarray(list(partition_assignment), dtype=np.int64)
    n = graph.number_of_nodes()
    if part.shape != (n,):
        raise ValueError(f"partition_assignment has {part.size} entries, the graph {n} nodes")
    _check_graph_size(n, K, terminals)
    if int(part.min()) < 0 or int(part.max()) > K - 1:
        raise ValueError(f"partition_assignment holds a class outside 0..{K - 1} (number_classes = {K})")
    return K, part


def kway_local_search(partition_assignment, graph, number_classes: int, max_sweeps: int = 100,
                      terminals: bool = True) -> Tuple[List[int], Any]:
    """:func:`local_search_optimization` for a partition into ``number_classes`` = 2..8 classes (extension,
    include/gcnmaxcut.h ``gmc_kway_refine_anneal_f32`` without annealing sweeps): nodes 0..K-1 keep their classes,
    every other node moves to the class that cuts the most of its edge weight, sweep after sweep, until a sweep moves
    nothing or ``max_sweeps`` have run.  Returns the refined assignment and its cut value.  ``terminals=False``: every
    node may move, so the result is a local optimum of plain max-K-cut under single moves."""
    K, part = _kway_partition("kway_local_search", partition_assignment, graph, number_classes, terminals)
    if max_sweeps < 0:
        raise ValueError(f"max_sweeps must be >= 0, got {max_sweeps}")
    dev = hip.require_gpu()
    best_assign, best_cut, _ = _kway_anneal_on_gpu(_graph_batch(graph, dev), K, _one_candidate(part, dev),
                                                   np.zeros(0, np.float32), 0, max_sweeps, terminals)
    return _graph_result(best_assign, best_cut)


def kway_annealing(partition_assignment, graph, number_classes: int, sweeps: int = 100, t_start: float = 1.5,
                   t_end: float = 0.15, seed: int = 0, max_descent_sweeps: int = 100,
                   terminals: bool = True) -> Tuple[List[int], Any]:
    """:func:`annealing_optimization` for a partition into ``number_classes`` = 2..8 classes (extension,
    include/gcnmaxcut.h ``gmc_kway_refine_anneal_f32``): ``sweeps`` Metropolis sweeps cooling from ``t_start`` to
    ``t_end`` (in units of the graph's mean edge weight), each node proposing the best of the K-1 other classes, the
    best state passed through kept, then the K-class local search from it.  Nodes 0..K-1 keep their classes; the result
    is never worse than the input and is reproducible from ``seed``.  Returns the assignment and its cut value."""
    return _anneal_graph("kway_annealing", partition_assignment, graph, number_classes, sweeps, t_start, t_end, seed,
                         max_descent_sweeps, terminals, large=False)


def _anneal_graph(what: str, partition_assignment, graph, number_classes: int, sweeps: int, t_start: float, t_end: float,
                  seed: int, max_descent_sweeps: int, terminals: bool, large: bool) -> Tuple[List[int], Any]:
    K, part = _kway_partition(what, partition_assignment, graph, number_classes, terminals)
    if sweeps < 0 or max_descent_sweeps < 0:
        raise ValueError(f"sweeps and max_descent_sweeps must be >= 0, got {sweeps} and {max_descent_sweeps}")
    dev = hip.require_gpu()
    batch = _graph_batch(graph, dev, large)
    inv_temp = anneal_schedule(sweeps, t_start, t_end, _mean_edge_weight(batch))
    best_assign, best_cut, _ = _kway_anneal_on_gpu(batch, K, _one_candidate(part, dev), inv_temp, seed, max_descent_sweeps,
                                                   terminals, large=large)
    return _graph_result(best_assign, best_cut)


# The tabu stage's tenure defaults are PROVISIONAL: the literature's 3 + rand(n / 10), taken over
# as a starting point, not a measured choice.
TABU_TENURE = (3, 0, 10)   # tenure_base, tenure_span, tenure_div


def _tabu_arguments(what: str, iterations: int, tenure) -> Tuple[int, int, int]:
    """The checks the tabu stage's callers share; returns (tenure_base, tenure_span, tenure_div)."""
    base, span, div = (int(t) for t in tenure)
    if not 0 <= int(iterations) < 1 << 31:
        raise ValueError(f"{what}: iterations must be in 0..2^31-1, got {iterations}")
    if min(base, span, div) < 0 or max(base, span, div) >= 1 << 31:
        raise ValueError(f"{what}: tenure_base, tenure_span and tenure_div must be in 0..2^31-1, got {base}, {span}, {div}")
    return base, span, div


def _chain_outputs(batch: GraphBatch, cands: int):
    """What both chain searches write: :func:`_search_outputs`, then best_iter and moves [B, cands]."""
    per_chain = lambda: torch.empty((batch.B, cands), dtype=torch.int32, device=batch.device)
    return _search_outputs(batch, cands) + (per_chain(), per_chain())


def _kway_tabu_on_gpu(batch: GraphBatch, K: int, assign: torch.Tensor, iterations: int, tenure, seed: int,
                      terminals: bool = True, node_cost=None):
    """One-flip tabu search at K classes (gmc_kway_tabu_f32) over the candidates assign [cands, R] int8, in place:
    ``iterations`` iterations per candidate with ``tenure`` = (tenure_base, tenure_span, tenure_div).  Returns the best
    assignment [R], its cut and candidate index per graph, then best_iter and moves [B, cands] and cut_all [B, cands].
    ``node_cost`` [R, K]: moves and scores follow cut minus cost (gmc_kway_tabu_c_f32)."""
    _needs_terminals(batch, K, terminals)
    node_cost = _cost_tensor(batch, K, node_cost)
    base, span, div = _tabu_arguments("the tabu search", iterations, tenure)
    cands = int(assign.shape[0])
    cut_all, best_assign, best_cut, best_idx, best_iter, moves = _chain_outputs(batch, cands)
    p = hip.ptr
    _call("gmc_kway_tabu_f32", terminals, (batch.ref(), K),
          (cands, p(assign), int(iterations), base, span, div, int(seed) & _M64, p(cut_all), p(best_assign), p(best_cut),
           p(best_idx), p(best_iter), p(moves), hip.stream()), node_cost, t_twin=False)
    return best_assign, best_cut, best_idx, best_iter, moves, cut_all


def kway_tabu_search(partition_assignment, graph, number_classes: int, iterations: Optional[int] = None,
                     tenure_base: int = 3, tenure_span: int = 0, tenure_div: int = 10, seed: int = 0,
                     terminals: bool = True, node_cost=None) -> Tuple[List[int], Any]:
    """One-flip tabu search from a partition into ``number_classes`` = 2..8 classes (extension, include/gcnmaxcut.h
    ``gmc_kway_tabu_f32``), the sibling of :func:`kway_annealing`: every iteration makes the best single move, the
    moved node may not move again for ``tenure_base + rand(tenure_span + n_mov // tenure_div)`` iterations
    (``tenure_div = 0``: no size term) unless moving it would beat the best cut seen, and the best state passed through
    is returned.  ``iterations=None`` means ``20 * n``.  Nodes 0..K-1 keep their classes (``terminals=False``: every
    node may move); for unit and integer weights the result is never worse than the input; reproducible from ``seed``.
    The tenure defaults are the literature's ``3 + rand(n / 10)``, provisional: a starting point nobody has tuned, see
    DESIGN.md section 30.  Returns the assignment and its cut value.  ``node_cost`` [n, K] (numpy or torch floats, row =
    node): the search follows the objective ``cut - sum_v node_cost[v][class_v]`` (``gmc_kway_tabu_c_f32``) and the
    returned value is that objective."""
    K, part = _kway_partition("kway_tabu_search", partition_assignment, graph, number_classes, terminals)
    node_cost = _graph_cost("kway_tabu_search", node_cost, graph.number_of_nodes(), K)
    iterations = 20 * graph.number_of_nodes() if iterations is None else int(iterations)
    tenure = _tabu_arguments("kway_tabu_search", iterations, (tenure_base, tenure_span, tenure_div))
    dev = hip.require_gpu()
    best_assign, best_cut = _kway_tabu_on_gpu(_graph_batch(graph, dev), K, _one_candidate(part, dev), iterations, tenure,
                                              seed, terminals, node_cost)[:2]
    return _graph_result(best_assign, best_cut)


def class_size_bounds(what: str, class_sizes, sizes, K: int, terminals: bool) -> Tuple[np.ndarray, np.ndarray]:
    """``class_sizes`` as the balanced stage takes it -> (lo, hi), int32 [B, K], for graphs of ``sizes`` [B] nodes, all on
    the host: ``"balanced"`` is ``n // K`` and ``ceil(n / K)`` for every class; a pair ``(lo, hi)`` holds [K] (every
    graph) or [B, K] integers.  Bounds that admit no partition (include/gcnmaxcut.h, gmc_kway_balance_f32: ``lo <= hi``,
    ``hi >= 1`` for a terminal's class, ``sum(max(lo, t)) <= n <= sum(hi)``) raise ``ValueError`` naming the graph."""
    sizes = np.asarray(sizes, np.int64).reshape(-1)
    B = sizes.size
    if isinstance(class_sizes, str):
        if class_sizes != "balanced":
            raise ValueError(f"{what}: class_sizes must be 'balanced' or a pair (lo, hi), got {class_sizes!r}")
        lo = np.repeat((sizes // K)[:, None], K, axis=1)
        hi = np.repeat((-(-sizes // K))[:, None], K, axis=1)
    else:
        if not isinstance(class_sizes, (tuple, list)) or len(class_sizes) != 2:
            raise ValueError(f"{what}: class_sizes must be 'balanced' or a pair (lo, hi)")
        pair = []
        for name, x in zip(("lo", "hi"), class_sizes):
            x = _host_array(x)
            if x.dtype.kind not in "iu" or x.shape not in ((K,), (B, K)):
                raise ValueError(f"{what}: class_sizes {name} must hold integers of shape [{K}] or [{B}, {K}], got "
                                 f"{x.dtype} {tuple(x.shape)}")
            if x.size and (int(x.min()) < -(1 << 31) or int(x.max()) >= 1 << 31):
                raise ValueError(f"{what}: class_sizes {name} does not fit int32")
            pair.append(np.broadcast_to(x.astype(np.int64), (B, K)))
        lo, hi = pair
    t = 1 if terminals else 0
    for g in range(B):
        n = int(sizes[g])
        why = None
        if (lo[g] > hi[g]).any():
            why = f"lo > hi for class {int(np.argmax(lo[g] > hi[g]))}"
        elif (hi[g] < t).any():
            why = f"hi < 1 for class {int(np.argmax(hi[g] < t))}, which holds a terminal"
        elif int(np.maximum(lo[g], t).sum()) > n:
            why = f"the lower bounds ask for {int(np.maximum(lo[g], t).sum())} nodes"
        elif int(hi[g].sum()) < n:
            why = f"the upper bounds leave room for {int(hi[g].sum())} nodes"
        if why is not None:
            raise ValueError(f"{what}: the class sizes of graph {g} ({n} nodes, number_classes = {K}) admit no "
                             f"partition: {why}")
    return np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)


def _kway_balance_on_gpu(batch: GraphBatch, K: int, assign: torch.Tensor, lo: np.ndarray, hi: np.ndarray,
                         iterations: int, tenure, seed: int, terminals: bool = True, node_cost=None):
    """Tabu search under class-size bounds (gmc_kway_balance_f32) over the candidates assign [cands, R] int8, in place,
    with lo, hi int32 [B, K] as :func:`class_size_bounds` returns them.  Returns the best assignment [R], its cut and
    candidate index per graph, then best_iter, moves and repairs [B, cands] and cut_all [B, cands].  ``node_cost``
    [R, K]: moves, repairs and scores follow cut minus cost (gmc_kway_balance_c_f32)."""
    _needs_terminals(batch, K, terminals)
    node_cost = _cost_tensor(batch, K, node_cost)
    base, span, div = _tabu_arguments("the balanced search", iterations, tenure)
    if lo.shape != (batch.B, K) or hi.shape != (batch.B, K):
        raise ValueError(f"the balanced search: bounds of shape {lo.shape} and {hi.shape} for {batch.B} graphs and {K} classes")
    dev = batch.device
    cands = int(assign.shape[0])
    size_lo = torch.from_numpy(np.ascontiguousarray(lo, np.int32)).to(dev)
    size_hi = torch.from_numpy(np.ascontiguousarray(hi, np.int32)).to(dev)
    cut_all, best_assign, best_cut, best_idx, best_iter, moves = _chain_outputs(batch, cands)
    repairs = torch.empty_like(moves)
    p = hip.ptr
    _call("gmc_kway_balance_f32", terminals, (batch.ref(), K),
          (cands, p(assign), p(size_lo), p(size_hi), int(iterations), base, span, div, int(seed) & _M64, p(cut_all),
           p(best_assign), p(best_cut), p(best_idx), p(best_iter), p(moves), p(repairs), None, hip.stream()), node_cost,
          t_twin=False)
    return best_assign, best_cut, best_idx, best_iter, moves, repairs, cut_all


def kway_balanced_search(partition_assignment, graph, number_classes: int, class_sizes="balanced",
                         iterations: Optional[int] = None, tenure_base: int = 3, tenure_span: int = 0,
                         tenure_div: int = 10, seed: int = 0, terminals: bool = True,
                         node_cost=None) -> Tuple[List[int], Any]:
    """:func:`kway_tabu_search` with the size of every class kept within bounds (extension, include/gcnmaxcut.h
    ``gmc_kway_balance_f32``): max-bisection and balanced max-K-cut, and on negated weights balanced minimum cut.
    ``class_sizes`` is ``"balanced"`` (every class holds ``n // K`` to ``ceil(n / K)`` nodes, terminals included) or a
    pair ``(lo, hi)`` of ``number_classes`` integers each.  The input need not be within the bounds: it is first
    repaired by the moves that cost the least cut.  Then every iteration makes the best single move that keeps the
    bounds, or the best move that breaks one followed by the best move back out of the class it entered; the best
    state passed through is returned and is always within the bounds.  ``iterations=None`` means ``20 * n``; the tenure
    arguments are :func:`kway_tabu_search`'s.  Bounds that admit no partition raise ``ValueError``.  With
    ``class_sizes=([0] * K, [n] * K)`` it is :func:`kway_tabu_search`, byte for byte.  Returns the assignment and
    its cut value.  ``node_cost`` [n, K]: as :func:`kway_tabu_search` takes it (``gmc_kway_balance_c_f32``); the repair
    then gives up the least objective, and the returned value is the objective."""
    K, part = _kway_partition("kway_balanced_search", partition_assignment, graph, number_classes, terminals)
    n = graph.number_of_nodes()
    node_cost = _graph_cost("kway_balanced_search", node_cost, n, K)
    iterations = 20 * n if iterations is None else int(iterations)
    tenure = _tabu_arguments("kway_balanced_search", iterations, (tenure_base, tenure_span, tenure_div))
    lo, hi = class_size_bounds("kway_balanced_search", class_sizes, [n], K, terminals)
    dev = hip.require_gpu()
    best_assign, best_cut = _kway_balance_on_gpu(_graph_batch(graph, dev), K, _one_candidate(part, dev), lo, hi,
                                                 iterations, tenure, seed, terminals, node_cost)[:2]
    return _graph_result(best_assign, best_cut)


# The evolution stage's defaults are PROVISIONAL: 10 generations of 10 sweeps cooling from 0.6
# are a starting point nobody has measured yet, not the outcome of the sweep described there.
EVOLVE_GENERATIONS = 10
EVOLVE_GENERATION_SWEEPS = 10
EVOLVE_T_START = 0.6


def _evolve_arguments(what: str, cands: int, generations: int, generation_sweeps: int, elite: Optional[int],
                      max_descent_sweeps: int) -> int:
    """The checks the evolution's callers share; returns the elite count (``None``: ``max(2, cands // 4)``)."""
    if generations < 0 or generation_sweeps < 0 or max_descent_sweeps < 0:
        raise ValueError(f"{what}: generations, generation_sweeps and max_descent_sweeps must be >= 0, got "
                         f"{generations}, {generation_sweeps} and {max_descent_sweeps}")
    if generations >= 1 << 20 or generation_sweeps >= 1 << 20:
        raise ValueError(f"{what}: generations and generation_sweeps must be below 2^20")
    elite = max(2, cands // 4) if elite is None else int(elite)
    if elite < 1:
        raise ValueError(f"{what}: elite must be >= 1, got {elite}")
    return elite


def _kway_evolve_on_gpu(batch: GraphBatch, K: int, population: torch.Tensor, generations: int, elite: int,
                        inv_temp: np.ndarray, seed: int, max_descent_sweeps: int):
    """The evolution stage (gmc_kway_evolve_f32) over the population [cands, R] int8, which is left alone; returns the
    best assignment [R], its cut and slot per graph, the best cut per generation [generations + 1, B] and the two
    planes of the population and of its cuts."""
    _needs_terminals(batch, K)
    dev = batch.device
    cands = int(population.shape[0])
    order, cgoff, cptr = batch.refine_order(K)
    inv_t, levels, sweeps = _schedule_tensors(inv_temp, dev)
    pop = torch.empty((2, cands, batch.R), dtype=torch.int8, device=dev)
    pop[0].copy_(population)
    cut = torch.empty((2, batch.B, cands), dtype=torch.float32, device=dev)
    best_assign, best_cut, best_idx = _best_outputs(batch)
    history = torch.empty((generations + 1, batch.B), dtype=torch.float32, device=dev)
    p = hip.ptr
    rc = hip.load().gmc_kway_evolve_f32(batch.ref(), K, p(order), p(cgoff), p(cptr), cands, p(pop), p(cut),
                                        int(generations), int(elite), p(inv_t), sweeps, p(levels), int(seed) & _M64,
                                        int(max_descent_sweeps), p(best_assign), p(best_cut), p(best_idx), p(history),
                                        hip.stream())
    hip.check(rc, "gmc_kway_evolve_f32")
    return best_assign, best_cut, best_idx, history, pop, cut


def kway_evolution(partitions, graph, number_classes: int, generations: int = EVOLVE_GENERATIONS,
                   generation_sweeps: int = EVOLVE_GENERATION_SWEEPS, elite: Optional[int] = None,
                   t_start: float = EVOLVE_T_START, t_end: float = 0.15, seed: int = 0,
                   max_descent_sweeps: int = 100) -> Tuple[List[int], Any, List[Any]]:
    """Recombine ``partitions`` [cands, n] of one graph into ``number_classes`` = 2..8 classes across ``generations``
    generations (extension, include/gcnmaxcut.h ``gmc_kway_evolve_f32``): every generation gives each partition a
    child of itself and one of the ``elite`` best (``None``: ``max(2, cands // 4)``) - class names aligned, the nodes
    the two disagree on taken from either - anneals the child for ``generation_sweeps`` sweeps cooling from ``t_start``
    to ``t_end`` (:func:`anneal_schedule`, in units of the mean edge weight), descends from the best state and keeps
    the child when its cut is not below the partition's.  Nodes 0..K-1 are the terminals.  Reproducible from ``seed``.
    Returns the best assignment, its cut and the best cut after every generation (``generations + 1`` entries, the
    first that of the input; never decreasing).  The defaults of ``generations``, ``generation_sweeps`` and
    ``t_start`` are provisional, see DESIGN.md section 22."""
    K = _search_classes("kway_evolution", number_classes)
    parts = np.asarray(partitions, dtype=np.int64)
    n = graph.number_of_nodes()
    if parts.ndim != 2 or parts.shape[0] < 1 or parts.shape[1] != n:
        raise ValueError(f"partitions must be [cands, {n}] with cands >= 1, got {tuple(parts.shape)}")
    _check_graph_size(n, K)
    if int(parts.min()) < 0 or int(parts.max()) > K - 1:
        raise ValueError(f"partitions holds a class outside 0..{K - 1} (number_classes = {K})")
    elite = _evolve_arguments("kway_evolution", parts.shape[0], generations, generation_sweeps, elite,
                              max_descent_sweeps)
    dev = hip.require_gpu()
    batch = _graph_batch(graph, dev)
    population = torch.from_numpy(parts.astype(np.int8)).to(dev)
    inv_temp = anneal_schedule(generation_sweeps, t_start, t_end, _mean_edge_weight(batch))
    best_assign, best_cut, _, history, _, _ = _kway_evolve_on_gpu(batch, K, population, generations, elite, inv_temp,
                                                                  seed, max_descent_sweeps)
    return (best_assign.cpu().tolist(), _as_number(best_cut.item()),
            [_as_number(c) for c in history[:, 0].cpu().tolist()])


# The tempering stage's defaults are PROVISIONAL: the annealing's own temperature range as a
# ladder of 8 rungs, 50 rounds of 4 sweeps - a starting point, not the outcome of the grid described there.
TEMPER_ROUNDS = 50
TEMPER_ROUND_SWEEPS = 4
TEMPER_RUNGS = 8
TEMPER_T_HOT = 1.5
TEMPER_T_COLD = 0.15


def temper_ladder(rungs: int, t_hot: float = TEMPER_T_HOT, t_cold: float = TEMPER_T_COLD, scale: float = 1.0) -> np.ndarray:
    """float32 ``1 / T_r`` of a geometric ladder ``T_r = scale * t_hot * (t_cold / t_hot) ** (r / max(rungs-1, 1))``,
    rung 0 the hottest (float64, rounded once; one rung: ``t_hot``).  ``scale``: the mean edge weight of the batch, the
    mean absolute weight for signed weights (1 for unit weights)."""
    if not 1 <= int(rungs) <= hip.TEMPER_MAX_RUNGS:
        raise ValueError(f"rungs must be in 1..{hip.TEMPER_MAX_RUNGS}, got {rungs}")
    if not (t_hot > 0 and t_cold > 0 and scale > 0):
        raise ValueError("t_hot, t_cold and scale must be > 0")
    r = np.arange(int(rungs), dtype=np.float64)
    temps = float(scale) * float(t_hot) * (float(t_cold) / float(t_hot)) ** (r / max(int(rungs) - 1, 1))
    return (1.0 / temps).astype(np.float32)


def _temper_arguments(what: str, cands: int, rounds: int, round_sweeps: int, rungs: int, max_descent_sweeps: int = 0) -> None:
    """The checks the tempering's callers share."""
    if not 1 <= int(rungs) <= hip.TEMPER_MAX_RUNGS:
        raise ValueError(f"{what}: rungs must be in 1..{hip.TEMPER_MAX_RUNGS}, got {rungs}")
    if cands < 1 or cands % int(rungs):
        raise ValueError(f"{what}: {cands} candidates do not fill ladders of {rungs} rungs (rungs must divide the count)")
    if rounds < 0 or max_descent_sweeps < 0 or round_sweeps < (1 if rounds else 0):
        raise ValueError(f"{what}: rounds and max_descent_sweeps must be >= 0 and round_sweeps >= 1, got {rounds}, "
                         f"{max_descent_sweeps} and {round_sweeps}")
    if int(rounds) * int(round_sweeps) >= 1 << 20:
        raise ValueError(f"{what}: rounds * round_sweeps must be below 2^20")


def _kway_temper_on_gpu(batch: GraphBatch, K: int, state: torch.Tensor, ladder: np.ndarray, rounds: int,
                        round_sweeps: int, seed: int, terminals: bool = True, node_cost=None):
    """Parallel tempering (gmc_kway_temper_f32) over the walkers state [cands, R] int8, in place: ``rounds`` rounds of
    ``round_sweeps`` sweeps on ladders of ``len(ladder)`` inverse temperatures.  Returns the best states [cands, R] int8,
    their scores [B, cands] and best_round, rung and swaps [B, cands] int32.  ``node_cost`` [R, K]: moves and scores
    follow cut minus cost."""
    _needs_terminals(batch, K, terminals)
    node_cost = _cost_tensor(batch, K, node_cost)
    dev = batch.device
    cands, rungs = int(state.shape[0]), int(len(ladder))
    _temper_arguments("the tempering", cands, int(rounds), int(round_sweeps), rungs)
    order, cgoff, cptr = batch.refine_order(K, terminals)
    lad = torch.from_numpy(np.ascontiguousarray(ladder, np.float32)).to(dev)
    levels = torch.from_numpy(anneal_levels()).to(dev)
    best = torch.empty_like(state)
    best_score = torch.empty((batch.B, cands), dtype=torch.float32, device=dev)
    best_round, rung, swaps = (torch.empty((batch.B, cands), dtype=torch.int32, device=dev) for _ in range(3))
    lib, p = hip.load(), hip.ptr
    ws = torch.empty(max(int(lib.gmc_kway_temper_workspace_bytes(batch.ref(), cands)), 16), dtype=torch.uint8, device=dev)
    rc = lib.gmc_kway_temper_f32(batch.ref(), K, int(bool(terminals)), p(node_cost), p(order), p(cgoff), p(cptr), cands,
                                 rungs, p(lad), int(rounds), int(round_sweeps), p(levels), int(seed) & _M64, p(state),
                                 p(best), p(best_score), p(best_round), p(rung), p(swaps), p(ws), ws.numel(), hip.stream())
    hip.check(rc, "gmc_kway_temper_f32")
    return best, best_score, best_round, rung, swaps


def kway_tempering(partitions, graph, number_classes: int, rounds: int = TEMPER_ROUNDS,
                   round_sweeps: int = TEMPER_ROUND_SWEEPS, rungs: int = TEMPER_RUNGS, t_hot: float = TEMPER_T_HOT,
                   t_cold: float = TEMPER_T_COLD, seed: int = 0, max_descent_sweeps: int = 100, terminals: bool = True,
                   node_cost=None) -> Tuple[List[int], Any, Dict[str, Any]]:
    """Parallel tempering (replica exchange) from ``partitions`` [cands, n] of one graph into ``number_classes`` = 2..8
    classes (extension, include/gcnmaxcut_temper.h ``gmc_kway_temper_f32``): the partitions are walkers of the
    annealing's Metropolis sweep on ``cands / rungs`` ladders of ``rungs`` fixed temperatures from ``t_hot`` to ``t_cold``
    (:func:`temper_ladder`, in units of the graph's mean absolute edge weight); after every round of ``round_sweeps``
    sweeps neighbouring rungs exchange their temperatures by the Metropolis rule, so a walker frozen in a poor basin can
    climb to a hot rung and leave it.  The best state every walker passed through is kept, the K-class local search
    descends from each and the best is returned.  ``rungs`` must divide the number of partitions.  Nodes 0..K-1 keep
    their classes (``terminals=False``: every node may move); reproducible from ``seed``; ``node_cost`` [n, K]: the
    objective ``cut - sum_v node_cost[v][class_v]``.  Returns the assignment, its cut (objective) and a dict with
    ``best_round``, ``rung``, ``swaps`` and ``scores`` (per partition: the round that found its best state, its final
    rung, the exchanges it took part in, its best score before the descent).  The defaults are provisional, see
    DESIGN.md section 39."""
    K = _search_classes("kway_tempering", number_classes)
    parts = np.asarray(partitions, dtype=np.int64)
    n = graph.number_of_nodes()
    if parts.ndim != 2 or parts.shape[0] < 1 or parts.shape[1] != n:
        raise ValueError(f"partitions must be [cands, {n}] with cands >= 1, got {tuple(parts.shape)}")
    _check_graph_size(n, K, terminals)
    if int(parts.min()) < 0 or int(parts.max()) > K - 1:
        raise ValueError(f"partitions holds a class outside 0..{K - 1} (number_classes = {K})")
    _temper_arguments("kway_tempering", parts.shape[0], rounds, round_sweeps, rungs, max_descent_sweeps)
    cost = _graph_cost("kway_tempering", node_cost, n, K)
    dev = hip.require_gpu()
    batch = _graph_batch(graph, dev)
    from ..maxcut import _mean_abs_edge_weight
    ladder = temper_ladder(rungs, t_hot, t_cold, _mean_abs_edge_weight(batch))
    state = torch.from_numpy(parts.astype(np.int8)).to(dev)
    best, scores, best_round, rung, swaps = _kway_temper_on_gpu(batch, K, state, ladder, rounds, round_sweeps, seed,
                                                                terminals, cost)
    best_assign, best_cut, _ = _kway_anneal_on_gpu(batch, K, best, np.zeros(0, np.float32), 0, max_descent_sweeps,
                                                   terminals, cost)
    info = {"best_round": best_round[0].cpu().tolist(), "rung": rung[0].cpu().tolist(), "swaps": swaps[0].cpu().tolist(),
            "scores": [_as_number(c) for c in scores[0].cpu().tolist()]}
    return best_assign.cpu().tolist(), _as_number(best_cut.item()), info


def dense_matrices(what: str, W, dev) -> torch.Tensor:
    """A dense door's matrices -> a contiguous [B, n, n] float32 tensor on ``dev``: ``W`` is [n, n] or [B, n, n], a
    tensor (host or device) or a numpy array; 2 <= n <= ``hip.MAX_GRAPH_NODES``, every entry finite in float32, and
    symmetric bit for bit (the diagonal is never read and is not checked).  ``ValueError`` otherwise."""
    t = W if isinstance(W, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(W))
    if t.ndim == 2:
        t = t.reshape(1, *t.shape)
    if t.ndim != 3 or t.shape[1] != t.shape[2]:
        raise ValueError(f"{what} must be [n, n] or [B, n, n], got {tuple(t.shape)}")
    if not 2 <= t.shape[1] <= hip.MAX_GRAPH_NODES:
        raise ValueError(f"{what}: n must be in 2..{hip.MAX_GRAPH_NODES}, got {t.shape[1]}")
    t = t.to(dev, torch.float32).contiguous()
    off = ~torch.eye(t.shape[1], dtype=torch.bool, device=dev)
    if not bool(torch.isfinite(t[:, off]).all()):
        raise ValueError(f"{what} holds values that are not finite (in float32)")
    if not bool((t == t.transpose(1, 2))[:, off].all()):
        raise ValueError(f"{what} is not symmetric")
    return t


def dense_scale(W: torch.Tensor) -> float:
    """The temperature unit of the dense doors: ``sqrt(mean_v sum_{u != v} w_vu^2)`` over all rows of W [B, n, n], the
    spread of a local field under random classes, in float64 (1 for matrices of zeros).  PROVISIONAL: nobody has
    measured this choice against the sparse doors' mean absolute weight."""
    off = ~torch.eye(W.shape[1], dtype=torch.bool, device=W.device)
    sq = torch.where(off, W.to(torch.float64) ** 2, torch.zeros((), dtype=torch.float64, device=W.device))
    s = float(sq.sum(dim=2).mean().sqrt().item())
    return s if s > 0 else 1.0


def _dense_anneal_on_gpu(W: torch.Tensor, assign: torch.Tensor, inv_temp: np.ndarray, seed: int, max_descent_sweeps: int,
                         node_cost: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None) -> Dict[str, Any]:
    """gmc_dense_anneal_f32 over the candidates assign [cands, B * n] int8, in place, on W [B, n, n] (contiguous float32
    on the device, symmetric); ``node_cost`` [B * n, 2] float32 and ``order`` [B * n] int32 (local ids) on the device, or
    None.  Returns best_assign [B * n] int32, best_score / best_idx [B], score_all [B, cands], snap_sweep / sweeps
    [B, cands] int32 and moves [B, cands] int64."""
    B, n = int(W.shape[0]), int(W.shape[1])
    dev, cands = W.device, int(assign.shape[0])
    if tuple(assign.shape) != (cands, B * n) or assign.dtype != torch.int8 or cands < 1:
        raise ValueError(f"assign must be [cands, {B * n}] int8 with cands >= 1, got {assign.dtype} {tuple(assign.shape)}")
    inv_t, levels, sweeps = _schedule_tensors(inv_temp, dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out = dict(best_assign=i32(B * n), best_score=f32(B), best_idx=i32(B), score_all=f32(B, cands),
               snap_sweep=i32(B, cands), sweeps=i32(B, cands),
               moves=torch.empty((B, cands), dtype=torch.int64, device=dev))
    lib, p = hip.load(), hip.ptr
    ws = torch.empty(max(int(lib.gmc_dense_anneal_workspace_bytes(B, n, cands)), 16), dtype=torch.uint8, device=dev)
    rc = lib.gmc_dense_anneal_f32(B, n, p(W), n, p(node_cost), p(order), cands, p(assign), p(inv_t), sweeps, p(levels),
                                  int(seed) & _M64, int(max_descent_sweeps), p(ws), ws.numel(), p(out["score_all"]),
                                  p(out["best_assign"]), p(out["best_score"]), p(out["best_idx"]), p(out["snap_sweep"]),
                                  p(out["sweeps"]), p(out["moves"]), hip.stream())
    hip.check(rc, "gmc_dense_anneal_f32")
    return out


def dense_annealing(partitions, W, sweeps: int = 100, t_start: float = 1.5, t_end: float = 0.15, seed: int = 0,
                    max_descent_sweeps: int = 100, node_cost=None, order=None) -> Tuple[List[int], Any, Dict[str, Any]]:
    """Annealing + descent of two-class partitions of ONE dense instance (extension, include/gcnmaxcut_dense.h
    ``gmc_dense_anneal_f32``): ``W`` [n, n] symmetric (max-cut weights; the diagonal is ignored), ``partitions`` [cands, n]
    (or [n]) of 0 / 1, ``node_cost`` [n, 2] the objective ``cut - sum_v node_cost[v][class_v]``, ``order`` a permutation
    of 0..n-1 (the visit order; None: 0, 1, ...).  Every chain keeps one cached local field per node, so a rejected
    proposal costs no row of W.  ``sweeps`` Metropolis sweeps cool from ``t_start`` to ``t_end`` (:func:`anneal_schedule`,
    :func:`anneal_levels`) in units of :func:`dense_scale` - the spread of a local field, where the sparse searches use
    the mean absolute weight; that unit and these defaults are PROVISIONAL, nobody has measured them (DESIGN.md section
    40).  Reproducible from ``seed``.  Returns the best assignment, its objective and a dict with ``scores``,
    ``snap_sweep``, ``sweeps`` and ``moves`` per partition."""
    if sweeps < 0 or max_descent_sweeps < 0:
        raise ValueError(f"sweeps and max_descent_sweeps must be >= 0, got {sweeps} and {max_descent_sweeps}")
    dev = hip.require_gpu()
    Wd = dense_matrices("W", W, dev)
    if Wd.shape[0] != 1:
        raise ValueError("dense_annealing takes one instance: W must be [n, n]")
    n = int(Wd.shape[1])
    parts = np.asarray(partitions, dtype=np.int64)
    parts = parts.reshape(1, -1) if parts.ndim == 1 else parts
    if parts.ndim != 2 or parts.shape[0] < 1 or parts.shape[1] != n:
        raise ValueError(f"partitions must be [cands, {n}] with cands >= 1, got {tuple(parts.shape)}")
    if int(parts.min()) < 0 or int(parts.max()) > 1:
        raise ValueError("partitions holds a class outside 0..1")
    cost = _graph_cost("dense_annealing", node_cost, n, 2)
    ord_t = None
    if order is not None:
        o = np.asarray(order, dtype=np.int64)
        if o.shape != (n,) or not np.array_equal(np.sort(o), np.arange(n)):
            raise ValueError(f"order must be a permutation of 0..{n - 1}")
        ord_t = torch.from_numpy(o.astype(np.int32)).to(dev)
    inv_temp = anneal_schedule(sweeps, t_start, t_end, dense_scale(Wd))
    out = _dense_anneal_on_gpu(Wd, torch.from_numpy(parts.astype(np.int8)).to(dev), inv_temp, seed, max_descent_sweeps,
                               None if cost is None else cost.to(dev), ord_t)
    info = {"scores": [_as_number(c) for c in out["score_all"][0].cpu().tolist()],
            "snap_sweep": out["snap_sweep"][0].cpu().tolist(), "sweeps": out["sweeps"][0].cpu().tolist(),
            "moves": out["moves"][0].cpu().tolist()}
    return out["best_assign"].cpu().tolist(), _as_number(out["best_score"].item()), info


def bifurcation_pump(steps: int) -> np.ndarray:
    """The pump table of the bifurcation, ``a0 - a(t)`` with a0 = 1 as float32 [steps]: the linear ramp from 1 at the
    first step to 0 at the last (one step: 1).  PROVISIONAL, like every default of the stage."""
    steps = int(steps)
    if steps < 0:
        raise ValueError(f"steps must be >= 0, got {steps}")
    return np.linspace(1.0, 0.0, steps).astype(np.float32) if steps > 1 else np.ones(steps, np.float32)


def _dense_bifurcation_on_gpu(W: torch.Tensor, cands: int, pump: np.ndarray, c0: float, dt: float,
                              node_cost: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None,
                              y: Optional[torch.Tensor] = None, seed: int = 0,
                              amplitude: float = 0.1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """gmc_dense_sb_f32 over ``cands`` chains per problem of W [B, n, n] (contiguous float32 on the device, symmetric):
    ``len(pump)`` steps from the state ``x``, ``y`` ([B * n, cands] float32 on the device, updated in place) or, without
    one, from gmc_dense_sb_init_f32's seeded start.  Returns (assign [cands, B * n] int8, x, y)."""
    B, n = int(W.shape[0]), int(W.shape[1])
    dev, cands = W.device, int(cands)
    if cands < 1:
        raise ValueError(f"candidates must be >= 1, got {cands}")
    lib, p = hip.load(), hip.ptr
    if (x is None) != (y is None):
        raise ValueError("a state is both x and y")
    if x is None:
        x = torch.empty((B * n, cands), dtype=torch.float32, device=dev)
        y = torch.empty((B * n, cands), dtype=torch.float32, device=dev)
        hip.check(lib.gmc_dense_sb_init_f32(B, n, cands, int(seed) & _M64, float(amplitude), p(x), p(y), hip.stream()),
                  "gmc_dense_sb_init_f32")
    for name, t in (("x", x), ("y", y)):
        if tuple(t.shape) != (B * n, cands) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous [{B * n}, {cands}] float32 tensor on {dev}")
    pump_t = torch.from_numpy(np.ascontiguousarray(pump, dtype=np.float32)).to(dev)
    steps = int(pump_t.numel())
    assign = torch.empty((cands, B * n), dtype=torch.int8, device=dev)
    ws = torch.empty(max(int(lib.gmc_dense_sb_workspace_bytes(B, n, cands)), 16), dtype=torch.uint8, device=dev)
    rc = lib.gmc_dense_sb_f32(B, n, p(W), n, p(node_cost), cands, p(x), p(y), p(pump_t) if steps else None, steps,
                              float(c0), float(dt), p(ws), ws.numel(), p(assign), hip.stream())
    hip.check(rc, "gmc_dense_sb_f32")
    return assign, x, y


def bifurcation_c0(W: torch.Tensor, c0: Optional[float]) -> float:
    """The coupling scale of the bifurcation: ``c0``, or for None ``0.5 / dense_scale(W)`` - the literature's
    ``0.5 / (sigma_J sqrt(N))`` up to N - 1 against N.  PROVISIONAL."""
    value = 0.5 / dense_scale(W) if c0 is None else float(c0)
    if not (np.isfinite(value) and value > 0):
        raise ValueError(f"bifurcation c0 must be finite and > 0, got {value}")
    return value


def dense_bifurcation(W, candidates: int = 200, steps: int = 1000, dt: float = 1.25, c0: Optional[float] = None,
                      amplitude: float = 0.1, seed: int = 0, node_cost=None,
                      state: Optional[Dict[str, Any]] = None) -> Tuple[np.ndarray, List[Any], Dict[str, Any]]:
    """Discrete simulated bifurcation of ONE dense instance (extension, include/gcnmaxcut_bifurcation.h
    ``gmc_dense_sb_f32``): ``W`` [n, n] symmetric (max-cut weights; the diagonal is ignored), ``node_cost`` [n, 2] the
    objective ``cut - sum_v node_cost[v][class_v]``.  ``candidates`` chains move all their nodes at once for ``steps``
    time steps of length ``dt`` under the linear pump (:func:`bifurcation_pump`); a step is one fp32 MFMA product
    ``W . sign(X)`` and an elementwise update.  ``c0=None`` means ``0.5 / dense_scale(W)``.  The chains start from the
    seeded state of ``gmc_dense_sb_init_f32`` (positions 0, momenta uniform in ``amplitude * [-1, 1)``) or continue from
    ``state``, the dict a previous call returned: ``x`` and ``y`` as numpy float32 [n, candidates] - the device's own
    layout, a node's candidates side by side.  To continue a ramp, pass the tail of the table yourself through
    ``gmc_dense_sb_f32``; this function always runs a whole ramp.

    Every default here (dt, c0's unit, amplitude, steps, the linear pump) is the literature's as far as recalled and
    PROVISIONAL: nobody has measured any of them on this code.

    Returns the partitions [candidates, n] (numpy int8, class 0 is spin +1), their scores - from ``gmc_dense_anneal_f32``
    with zero sweeps and zero descent, so they carry the bits every other dense output reports - and the dict
    ``{"x", "y"}``."""
    if steps < 0:
        raise ValueError(f"steps must be >= 0, got {steps}")
    dev = hip.require_gpu()
    Wd = dense_matrices("W", W, dev)
    if Wd.shape[0] != 1:
        raise ValueError("dense_bifurcation takes one instance: W must be [n, n]")
    n = int(Wd.shape[1])
    cost = _graph_cost("dense_bifurcation", node_cost, n, 2)
    cost = None if cost is None else cost.to(dev)
    x = y = None
    if state is not None:
        x, y = (torch.from_numpy(np.ascontiguousarray(state[k], dtype=np.float32)).to(dev) for k in ("x", "y"))
        if tuple(x.shape) != (n, int(candidates)) or tuple(y.shape) != (n, int(candidates)):
            raise ValueError(f"state must hold x and y of shape [{n}, {int(candidates)}]")
    assign, x, y = _dense_bifurcation_on_gpu(Wd, candidates, bifurcation_pump(steps), bifurcation_c0(Wd, c0), dt, cost, x,
                                             y, seed, amplitude)
    out = _dense_anneal_on_gpu(Wd, assign, np.zeros(0, np.float32), seed, 0, cost)
    scores = [_as_number(c) for c in out["score_all"][0].cpu().tolist()]
    return assign.cpu().numpy(), scores, {"x": x.cpu().numpy(), "y": y.cpu().numpy()}


def test_single_graph(model, dgl_graph, adjacency_matrix, nx_graph, terminals: List[int],
                      post_processing_iterations: int = 200, *, seed: Optional[int] = None,
                      graph_index: int = 0) -> Dict[str, Any]:
    """Argmax decode and post-processed decode of one graph (TestingNeuralNetwork.py:124-186).  ``seed`` /
    ``graph_index``: as for :func:`post_processing_optimization`."""
    _decoder_graph_size("test_single_graph", len(nx_graph.nodes()) if nx_graph is not None else 0)
    try:
        with torch.no_grad():
            node_probabilities = model(dgl_graph, adjacency_matrix)
        t0 = time()
        simple_assignment = simple_partition_assignment(node_probabilities)
        simple_cut = calculate_cut_value(simple_assignment, nx_graph)
        simple_time = time() - t0
        t0 = time()
        if post_processing_iterations <= 0 and node_probabilities.shape[1] != 3:
            # argmax-only evaluation of a model with number_classes != 3 (the sampler is 3-class): no post-processing
            post_assignment, post_cut = list(simple_assignment), simple_cut
        else:
            post_assignment, post_cut = post_processing_optimization(node_probabilities, nx_graph,
                                                                     post_processing_iterations, seed=seed,
                                                                     graph_index=graph_index)
        post_time = time() - t0
        improvement = post_cut - simple_cut
        return {
            'success': True, 'nodes': len(nx_graph.nodes()), 'edges': len(nx_graph.edges()),
            'simple_cut': simple_cut, 'simple_time': simple_time, 'simple_assignment': simple_assignment,
            'post_cut': post_cut, 'post_time': post_time, 'post_assignment': post_assignment,
            'improvement': improvement,
            'improvement_percent': (improvement / simple_cut * 100) if simple_cut > 0 else 0,
            'terminals': terminals, 'node_probabilities': node_probabilities.detach().cpu().numpy(),
        }
    except Exception as e:  # the reference reports and continues (:180-186)
        return {'success': False, 'error': str(e), 'nodes': len(nx_graph.nodes()) if nx_graph else 0,
                'edges': len(nx_graph.edges()) if nx_graph else 0}


test_single_graph.__test__ = False  # harness function, not a pytest test


def test_multiple_graphs(model, processed_graphs: Dict, graph_sizes: List[int],
                         post_processing_iterations: int = 200, verbose: bool = True, *,
                         seed: Optional[int] = None) -> Tuple[List[Dict], Dict]:
    """Evaluate a dataset and bucket the results by graph size (TestingNeuralNetwork.py:188-295).  ``seed``
    (extension): the seeded sampler, a graph's index being its position in ``processed_graphs`` (skipped graphs
    still count), so the per-graph results equal ``decode_dataset(..., sample_seed=seed)``'s."""
    if verbose:
        print("Testing neural network performance...")
        print("=" * 60)
    test_results: List[Dict] = []
    results_by_size = {size: {'simple': {'cut_values': [], 'times': []},
                              'post_processed': {'cut_values': [], 'times': []}} for size in graph_sizes}
    total = len(processed_graphs)
    if verbose:
        print(f"Sample keys from processed_graphs: {list(processed_graphs.keys())[:3]}")
    for count, (key, (g, adjacency_matrix, nx_graph, terminals)) in enumerate(processed_graphs.items(), 1):
        if isinstance(key, str):
            name = key
            try:
                size = int(name.split('_')[1][1:])
            except (IndexError, ValueError):
                size = len(nx_graph.nodes())
        else:
            name = f"graph_{key}"
            size = len(nx_graph.nodes())
            closest = min(graph_sizes, key=lambda x: abs(x - size))
            if abs(closest - size) <= 5:
                size = closest
        if verbose:
            print(f"\\nProcessing graph {count}/{total}: {name}")
            print(f"  Nodes: {len(nx_graph.nodes())}, Edges: {len(nx_graph.edges())}, Size category: {size}")
        if size not in graph_sizes:
            if verbose:
                print(f"  Skipping: graph size {size} not in test configuration")
            continue
        result = test_single_graph(model, g, adjacency_matrix, nx_graph, terminals, post_processing_iterations,
                                   seed=seed, graph_index=count - 1)
        if result['success']:
            result.update({'graph_name': name, 'graph_size': size})
            test_results.append(result)
            bucket = results_by_size[size]
            bucket['simple']['cut_values'].append(result['simple_cut'])
            bucket['simple']['times'].append(result['simple_time'])
            bucket['post_processed']['cut_values'].append(result['post_cut'])
            bucket['post_processed']['times'].append(result['post_time'])
            if verbose:
                print(f"  Simple GCN:      Cut = {result['simple_cut']}, Time = {result['simple_time']:.4f}s")
                print(f"  Post-processed:  Cut = {result['post_cut']}, Time = {result['post_time']:.4f}s")
                print(f"  Improvement:     {result['improvement']:+d} ({result['improvement_percent']:+.1f}%)")
        elif verbose:
            print(f"  ✗ Error processing graph: {result['error']}")
        if verbose and count % 10 == 0:
            print(f"\\n--- Progress: {count}/{total} ({count / total * 100:.1f}%) ---")
    if verbose:
        print(f"\\n{'=' * 60}")
        print("Neural network testing completed!")
        print(f"Successfully processed: {len(test_results)}/{total} graphs")
    return test_results, results_by_size


test_multiple_graphs.__test__ = False


def _dataset_batch(what: str, model, processed_graphs: Dict, large: bool, classes):
    """What opens every dataset function: the model's engine, the batch of the dataset's graphs with their edge values
    on the engine's device, and ``classes(eng.K)`` - the function's check of the class count, made before anything is
    built.  Unless ``large``, a graph beyond ``hip.MAX_GRAPH_NODES`` nodes is refused in ``what``'s name."""
    items = list(processed_graphs.values())
    eng = model.engine()
    K = classes(eng.K)
    model.eval()
    handles = [it[0] for it in items]
    if not large:
        _decoder_graph_size(what, max((h.n for h in handles), default=0))
    vals = [h.edge_values(it[1]) for h, it in zip(handles, items)]
    return eng, GraphBatch(handles, vals, eng.device), K


def _graph_rows(batch: GraphBatch):
    """(g, lo, hi) for every graph of the batch: graph g owns rows lo..hi-1."""
    for g in range(batch.B):
        yield g, int(batch.goff_host[g]), int(batch.goff_host[g + 1])


def decode_dataset(model, processed_graphs: Dict, post_processing_iterations: int = 200,
                   local_search_sweeps: int = 0, anneal_sweeps: int = 0, anneal_candidates: Optional[int] = None,
                   anneal_seed: int = 0, *, sample_seed: Optional[int] = None,
                   rounding_descent_sweeps: Optional[int] = None) -> List[Dict[str, Any]]:
    """Throughput form of the same evaluation (extension): ONE batched forward and ONE sampler
    launch for the whole dataset.  Results equal ``test_multiple_graphs``'s per-graph numbers when
    the RNG state is the same (uniforms are drawn graph by graph in dataset order).
    ``local_search_sweeps > 0`` also refines the argmax decode (candidate 0) and every sample (candidates
    1..iterations, in draw order) by local search (``local_search_optimization``) in one more launch; each result
    then carries ``refined_cut``, ``refined_assignment`` and ``refined_from`` (the winning candidate).
    ``anneal_sweeps > 0`` anneals a copy of the first ``anneal_candidates`` of the same 1 + iterations candidates
    (``None``: all of them) with ``annealing_optimization``'s defaults in one more launch; each result then carries
    ``annealed_cut``, ``annealed_assignment`` and ``annealed_from``.  Neither option changes the other keys or the
    uniforms drawn.
    ``sample_seed`` (None reads GCN_MAXCUT_SAMPLE_SEED; without either, the numpy stream above): the samples come
    from the seeded sampler, a graph's index being its position in ``processed_graphs.values()`` - the per-graph
    numbers of ``test_multiple_graphs(..., seed=sample_seed)``.  No uniform is drawn or copied by the host, numpy's
    RNG is left alone, and the [iterations, R] samples exist only when one of the two searches wants them.
    ``rounding_descent_sweeps`` (not None): one more launch rounds the same probabilities by conditional expectations
    (``conditional_rounding``) and descends that many sweeps from the result; each result then carries
    ``expected_cut``, ``rounded_cut`` and ``rounded_assignment``.  The other keys and the uniforms drawn stay what they
    are without it, and the rounded assignment is not among the candidates of the two searches."""
    if rounding_descent_sweeps is not None and rounding_descent_sweeps < 0:
        raise ValueError(f"rounding_descent_sweeps must be >= 0, got {rounding_descent_sweeps}")
    eng, batch, _ = _dataset_batch("decode_dataset", model, processed_graphs, False,
                                   lambda K: _three_classes_only("decode_dataset", K))
    P, S, loss = eng.forward(batch, 1.0, want_loss=True)
    best_assign, best_cut, _, assign_all = _sample_on_gpu(batch, P, post_processing_iterations,
                                                          _sample_seed(sample_seed), range(batch.B),
                                                          keep_samples=local_search_sweeps > 0 or anneal_sweeps > 0)
    refined = None
    if local_search_sweeps > 0:
        cands = torch.cat([S.to(torch.int8).reshape(1, -1), assign_all])
        refined = [t.cpu().numpy() for t in _refine_on_gpu(batch, cands, local_search_sweeps)]
    annealed = None
    if anneal_sweeps > 0:
        take = 1 + post_processing_iterations if anneal_candidates is None else int(anneal_candidates)
        if not 1 <= take <= 1 + post_processing_iterations:
            raise ValueError(f"anneal_candidates must be in 1..{1 + post_processing_iterations}, got {anneal_candidates}")
        cands = torch.cat([S.to(torch.int8).reshape(1, -1), assign_all[:take - 1]]).contiguous()
        inv_temp = anneal_schedule(anneal_sweeps, scale=_mean_edge_weight(batch))
        annealed = [t.cpu().numpy() for t in _anneal_on_gpu(batch, cands, inv_temp, anneal_seed, 100)]
    rounded = None
    if rounding_descent_sweeps is not None:
        rounded = [t.cpu().numpy() for t in _round_on_gpu(batch, P, rounding_descent_sweeps)]
    S_host, best_host = S.cpu().numpy(), best_assign.cpu().numpy()
    simple, post = (-loss).cpu().tolist(), best_cut.cpu().tolist()
    out = []
    for g, lo, hi in _graph_rows(batch):
        out.append({'nodes': hi - lo, 'simple_cut': _as_number(simple[g]), 'simple_assignment': S_host[lo:hi].tolist(),
                    'post_cut': _as_number(post[g]), 'post_assignment': best_host[lo:hi].tolist(),
                    'improvement': _as_number(post[g] - simple[g])})
        if refined is not None:
            ref_assign, ref_cut, ref_idx = refined
            out[-1].update({'refined_cut': _as_number(ref_cut[g]), 'refined_assignment': ref_assign[lo:hi].tolist(),
                            'refined_from': int(ref_idx[g])})
        if annealed is not None:
            ann_assign, ann_cut, ann_idx = annealed
            out[-1].update({'annealed_cut': _as_number(ann_cut[g]), 'annealed_assignment': ann_assign[lo:hi].tolist(),
                            'annealed_from': int(ann_idx[g])})
        if rounded is not None:
            rnd_assign, rnd_cut, rnd_expected, _ = rounded
            out[-1].update({'expected_cut': float(rnd_expected[g]), 'rounded_cut': _as_number(rnd_cut[g]),
                            'rounded_assignment': rnd_assign[lo:hi].tolist()})
    return out


def _plain_forward(terminals: bool) -> dict:
    """What a dataset decode adds to ``eng.forward``: without terminals the per-graph minimum of number_classes nodes is
    waived (``FusedEngine.forward(..., terminals=False)``: P is the plain softmax either way)."""
    return {} if terminals else {"terminals": False}


def _plain_argmax(batch: GraphBatch, P: torch.Tensor, K: int, large: bool = False):
    """The argmax decode without terminals: the first maximum of every row of P (no row overridden) as int32 [R], and
    its cut per graph, scored by a search launch that runs no sweep."""
    S = _first_argmax(P)
    if batch.B == 0:
        return S, torch.empty(0, dtype=torch.float32, device=P.device)
    _, cut, _ = _kway_anneal_on_gpu(batch, K, S.to(torch.int8).reshape(1, -1).contiguous(), np.zeros(0, np.float32), 0, 0,
                                    terminals=False, large=large)
    return S, cut


def round_dataset(model, processed_graphs: Dict, descent_sweeps: int = 0, terminals: bool = True) -> List[Dict[str, Any]]:
    """Argmax decode and conditional rounding of a whole dataset (extension): ONE batched forward and ONE rounding
    launch (``gmc_round_conditional_f32``), for a model of any ``number_classes`` in 2..8 - the decoder, and with
    ``descent_sweeps > 0`` the local search, of the models the 3-class sampler and searches refuse.  Per graph:
    ``nodes``, ``simple_cut`` / ``simple_assignment`` (the argmax decode, as ``decode_dataset`` reports it),
    ``expected_cut`` (of rounding every node independently from its row, terminals fixed), ``rounded_cut`` /
    ``rounded_assignment`` (never below ``expected_cut`` but for fp32 rounding) and ``descent_sweeps`` (the sweeps
    run, the last of them the one that moved nothing when the descent converged).
    ``terminals=False``: plain max-K-cut - ``simple_assignment`` is the row argmax of P (first maximum, no row
    overridden), the expected cut fixes no node, and the rounding and the descent visit every node.  A graph may then
    have fewer than number_classes nodes, as long as the dataset's largest graph has that many (the shared model's
    forward, ``gmc_kway_forward``, refuses a batch below that: ``ValueError``)."""
    return _round_dataset("round_dataset", model, processed_graphs, descent_sweeps, terminals, large=False)


def _round_dataset(what: str, model, processed_graphs: Dict, descent_sweeps: int, terminals: bool,
                   large: bool) -> List[Dict[str, Any]]:
    if descent_sweeps < 0:
        raise ValueError(f"descent_sweeps must be >= 0, got {descent_sweeps}")
    eng, batch, K = _dataset_batch(what, model, processed_graphs, large, _rounding_classes)
    P, S, loss = eng.forward(batch, 1.0, want_loss=True, **_plain_forward(terminals))
    assign, cut, expected, sweeps = [t.cpu().numpy() for t in
                                     _round_on_gpu(batch, P, descent_sweeps, terminals, large=large)]
    if not terminals:
        S, plain = _plain_argmax(batch, P, K, large)
        loss = -plain
    S_host, simple = S.cpu().numpy(), (-loss).cpu().tolist()
    return [{'nodes': hi - lo, 'simple_cut': _as_number(simple[g]), 'simple_assignment': S_host[lo:hi].tolist(),
             'expected_cut': float(expected[g]), 'rounded_cut': _as_number(cut[g]),
             'rounded_assignment': assign[lo:hi].tolist(), 'descent_sweeps': int(sweeps[g])}
            for g, lo, hi in _graph_rows(batch)]


def round_large_dataset(model, processed_graphs: Dict, descent_sweeps: int = 0,
                        terminals: bool = True) -> List[Dict[str, Any]]:
    """:func:`round_dataset` for datasets with graphs of any size up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes (extension):
    ONE batched forward (the engine takes a batch with a graph beyond ``hip.MAX_GRAPH_NODES`` nodes through
    ``gmc_large_forward``; an ``adjacency="none"`` dataset has no padded adjacency and its edge weights come from the
    graph) and ONE call of ``gmc_large_round_conditional_f32``.  The keys and, on a dataset :func:`round_dataset`
    takes, the assignments and sweep counts are :func:`round_dataset`'s, with and without ``terminals``."""
    return _round_dataset("round_large_dataset", model, processed_graphs, descent_sweeps, terminals, large=True)


def search_dataset(model, processed_graphs: Dict, samples: int = 200, *, sample_seed: int = 0, anneal_sweeps: int = 100,
                   anneal_seed: int = 0, max_descent_sweeps: int = 100,
                   candidates: Optional[int] = None, generations: int = 0,
                   generation_sweeps: int = EVOLVE_GENERATION_SWEEPS,
                   elite: Optional[int] = None, terminals: bool = True, tabu_iterations: int = 0,
                   tabu_seed: int = 0) -> List[Dict[str, Any]]:
    """Decode a whole dataset of a model of any ``number_classes`` in 2..8 with everything the 3-class path has
    (extension): ONE batched forward, ONE rounding launch (``round_dataset(..., 0)``), ONE launch of the seeded sampler
    (``gmc_kway_decode_sample_seeded_f32``, a graph's index its position in ``processed_graphs.values()``) and ONE
    search launch (``gmc_kway_refine_anneal_f32``) over the candidates of every graph: candidate 0 the argmax decode,
    candidate 1 the rounded partition, candidates 2.. the ``samples`` samples in iteration order.  ``candidates`` in
    1..2 + samples takes a prefix of them (``None``: all); ``anneal_sweeps = 0`` is the local search alone.
    ``samples = 0`` is allowed: the candidates are then the argmax and the rounded one.  Per graph: ``nodes``,
    ``simple_cut`` / ``simple_assignment``, ``expected_cut``, ``rounded_cut`` / ``rounded_assignment`` (as
    ``round_dataset(..., 0)`` reports them), ``post_cut`` / ``post_assignment`` (the best sample, with ``samples > 0``)
    and ``searched_cut``, ``searched_assignment``, ``searched_from`` (the winning candidate).
    ``generations > 0``: ONE call of the evolution stage (``gmc_kway_evolve_f32``, :func:`kway_evolution`) follows over
    the searched candidates of every graph as its population - ``generations`` generations of ``generation_sweeps``
    annealing sweeps cooling from ``EVOLVE_T_START``, ``elite`` as there, seeded by ``anneal_seed`` - and each result
    gains ``evolved_cut`` (never below ``searched_cut``), ``evolved_assignment`` and ``evolved_history`` (the best cut
    after every generation, ``generations + 1`` entries).  No other key changes; ``generations = 0`` launches nothing
    more and adds no key.
    ``terminals=False``: plain max-K-cut - candidate 0 is the row argmax of P (first maximum, no row overridden), and
    the rounding, the sampler and the search fix no node.  The evolution stage keeps its terminals:
    ``generations > 0`` then raises ``NotImplementedError``.
    ``tabu_iterations > 0``: ONE call of the tabu stage (``gmc_kway_tabu_f32``, :func:`kway_tabu_search`, the tenure
    ``TABU_TENURE``, seeded by ``tabu_seed``) follows on a copy of the candidates the annealing (and the evolution, if
    any) left, ``tabu_iterations`` iterations each, and each result gains ``tabu_cut``, ``tabu_assignment`` and
    ``tabu_iteration`` (the iteration at which the winning chain found it; 0: its input).  No other key changes;
    ``tabu_iterations = 0`` launches nothing more and adds no key."""
    return _search_dataset("search_dataset", model, processed_graphs, samples, sample_seed, anneal_sweeps, anneal_seed,
                           max_descent_sweeps, candidates, generations, generation_sweeps, elite, terminals,
                           tabu_iterations, tabu_seed, large=False)


def _search_dataset(what: str, model, processed_graphs: Dict, samples: int, sample_seed: int, anneal_sweeps: int,
                    anneal_seed: int, max_descent_sweeps: int, candidates: Optional[int], generations: int,
                    generation_sweeps: int, elite: Optional[int], terminals: bool, tabu_iterations: int, tabu_seed: int,
                    large: bool) -> List[Dict[str, Any]]:
    """:func:`search_dataset`, or with ``large`` :func:`search_large_dataset`: the large decoders, which have neither the
    evolution nor the tabu stage (its caller passes ``generations = tabu_iterations = 0``), in one workspace."""
    _tabu_arguments(what, tabu_iterations, TABU_TENURE)
    if not terminals and generations > 0:
        raise NotImplementedError(f"{what}(generations > 0, terminals=False): the evolution stage "
                                  "(gmc_kway_evolve_f32) keeps its terminals")
    if samples < 0:
        raise ValueError(f"samples must be >= 0, got {samples}")
    if anneal_sweeps < 0 or max_descent_sweeps < 0:
        raise ValueError(f"anneal_sweeps and max_descent_sweeps must be >= 0, got {anneal_sweeps} and {max_descent_sweeps}")
    take = 2 + samples if candidates is None else int(candidates)
    if not 1 <= take <= 2 + samples:
        raise ValueError(f"candidates must be in 1..{2 + samples}, got {candidates}")
    elite = _evolve_arguments(what, take, generations, generation_sweeps, elite, max_descent_sweeps)
    eng, batch, K = _dataset_batch(what, model, processed_graphs, large, lambda classes: _search_classes(what, classes))
    _needs_terminals(batch, K, terminals)
    P, S, loss = eng.forward(batch, 1.0, want_loss=True, **_plain_forward(terminals))
    if not terminals:
        S, plain = _plain_argmax(batch, P, K, large)
        loss = -plain
    rnd_assign, rnd_cut, rnd_expected, _ = _round_on_gpu(batch, P, 0, terminals, large=large)
    rows = [S.to(torch.int8).reshape(1, -1), rnd_assign.reshape(1, -1)]
    # the large route's sampler and annealing share one scratch
    ws = _large_search_workspace(batch, K, max(take, samples)) if large and batch.B else None
    sampled = None
    if samples > 0:
        best_assign, best_cut, _, assign_all = _kway_sample_on_gpu(batch, P, samples, int(sample_seed) & _M64,
                                                                   range(batch.B), keep_samples=take > 2,
                                                                   terminals=terminals, large=large, workspace=ws)
        sampled = (best_assign.cpu().numpy(), best_cut.cpu().tolist())
        if assign_all is not None:
            rows.append(assign_all)
    cands = torch.cat(rows)[:take].contiguous()
    inv_temp = anneal_schedule(anneal_sweeps, scale=_mean_edge_weight(batch))
    found_assign, found_cut, found_idx = [t.cpu().numpy() for t in
                                          _kway_anneal_on_gpu(batch, K, cands, inv_temp, anneal_seed, max_descent_sweeps,
                                                              terminals, large=large, workspace=ws)]
    evolved = None
    start = cands             # what the tabu stage starts from: the searched candidates, or the last population
    if generations > 0:   # the search left its candidates in `cands`: the population
        inv_temp = anneal_schedule(generation_sweeps, t_start=EVOLVE_T_START, scale=_mean_edge_weight(batch))
        ev = _kway_evolve_on_gpu(batch, K, cands, generations, elite, inv_temp, anneal_seed, max_descent_sweeps)
        evolved = [t.cpu().numpy() for t in ev[:4]]
        start = ev[4][generations & 1]
    tabu = None
    if tabu_iterations > 0:
        tb_assign, tb_cut, tb_idx, tb_iter = _kway_tabu_on_gpu(batch, K, start.clone(), int(tabu_iterations), TABU_TENURE,
                                                               tabu_seed, terminals)[:4]
        tb_iter = tb_iter.gather(1, tb_idx.to(torch.int64).reshape(-1, 1)).reshape(-1)
        tabu = [t.cpu().numpy() for t in (tb_assign, tb_cut, tb_iter)]
    S_host, simple = S.cpu().numpy(), (-loss).cpu().tolist()
    rnd_assign, rnd_cut, rnd_expected = rnd_assign.cpu().numpy(), rnd_cut.cpu().numpy(), rnd_expected.cpu().numpy()
    out = []
    for g, lo, hi in _graph_rows(batch):
        out.append({'nodes': hi - lo, 'simple_cut': _as_number(simple[g]), 'simple_assignment': S_host[lo:hi].tolist(),
                    'expected_cut': float(rnd_expected[g]), 'rounded_cut': _as_number(rnd_cut[g]),
                    'rounded_assignment': rnd_assign[lo:hi].tolist()})
        if sampled is not None:
            out[-1].update({'post_cut': _as_number(sampled[1][g]), 'post_assignment': sampled[0][lo:hi].tolist()})
        out[-1].update({'searched_cut': _as_number(found_cut[g]), 'searched_assignment': found_assign[lo:hi].tolist(),
                        'searched_from': int(found_idx[g])})
        if evolved is not None:
            ev_assign, ev_cut, _, ev_history = evolved[:4]
            out[-1].update({'evolved_cut': _as_number(ev_cut[g]), 'evolved_assignment': ev_assign[lo:hi].tolist(),
                            'evolved_history': [_as_number(c) for c in ev_history[:, g].tolist()]})
        if tabu is not None:
            out[-1].update({'tabu_cut': _as_number(tabu[1][g]), 'tabu_assignment': tabu[0][lo:hi].tolist(),
                            'tabu_iteration': int(tabu[2][g])})
    return out


def search_large_dataset(model, processed_graphs: Dict, samples: int = 200, *, sample_seed: int = 0,
                         anneal_sweeps: int = 100, anneal_seed: int = 0, max_descent_sweeps: int = 100,
                         candidates: Optional[int] = None, terminals: bool = True) -> List[Dict[str, Any]]:
    """:func:`search_dataset` for datasets with graphs of any size up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes
    (extension): ONE batched forward (the engine takes a batch with a graph beyond ``hip.MAX_GRAPH_NODES`` nodes
    through ``gmc_large_forward``; an ``adjacency="none"`` dataset has no padded adjacency and its edge weights come
    from the graph), ONE ``gmc_large_round_conditional_f32`` at descent 0, ONE ``gmc_large_sample_seeded_f32`` and ONE
    ``gmc_large_anneal_f32``.  Arguments, candidates (0 the argmax, 1 the rounded partition, 2.. the samples) and keys
    are :func:`search_dataset`'s; on a dataset that function takes, with unit or integer weights, so is every value.
    ``searched_cut`` is never below ``rounded_cut`` when the rounded partition is among the candidates.
    ``terminals=False`` is :func:`search_dataset`'s: plain max-K-cut, for graphs of any size.

    Memory on the device, R the nodes of the dataset: the candidates and the samples, ``candidates + samples`` bytes
    per node, and the workspace of the search, about ``2.02 * cpad`` bytes per node, ``cpad`` the larger of
    ``candidates`` and ``samples`` rounded up to a multiple of ``cp = min(64, its next power of two)`` - about
    ``(candidates + samples + 2 * cpad) * R`` bytes in all (200 samples, all of them candidates: 0.9 GiB per million
    nodes; 8 samples: 50 MiB).  The calls issue ``anneal_sweeps * (classes + 3) +
    max_descent_sweeps * (classes + 1)`` launches and more (``classes`` the colour classes of the batch, see the
    header), whenever the descent converges: give ``max_descent_sweeps`` the sweeps the descent may need."""
    return _search_dataset("search_large_dataset", model, processed_graphs, samples, sample_seed, anneal_sweeps,
                           anneal_seed, max_descent_sweeps, candidates, 0, EVOLVE_GENERATION_SWEEPS, None, terminals, 0, 0,
                           large=True)
