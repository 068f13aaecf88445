"""Graph handle and HBM-resident batches (host side of ``gmc_batch``).

``GraphHandle`` stands where the reference stores a ``DGLGraph``
(``python/DataGenerator/graphExtender.py:102-103,114``): entry 0 of every dataset
item.  It answers what the reference and its notebooks ask of that object
(``number_of_nodes``, ``number_of_edges`` == 2|E|, ``.to(device)``, picklable) and owns
the CSR the HIP kernels aggregate over.

``GraphBatch`` is a block-diagonal batch of graphs laid out for the kernels: one
``rowptr``/``gcol``/``lcol``/``vals``/``dinv`` set in HBM plus per-graph row offsets.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import hip


class DGLError(Exception):
    """Name-compatible stand-in for the error DGL raises (zero in-degree nodes)."""


class GraphHandle:
    """CSR of an undirected graph as ``dgl.from_networkx`` would hold it: node ids are
    the sorted networkx labels, every undirected edge appears in both directions."""

    def __init__(self, n: int, rowptr: np.ndarray, col: np.ndarray, weight: Optional[np.ndarray] = None):
        self.n = int(n)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        # edge 'weight' attribute in CSR order (what the padded adjacency holds), or None = all 1
        self.weight = None if weight is None else np.ascontiguousarray(weight, dtype=np.float32)
        self.device = torch.device("cpu")
        self._cache = {}

    # ---- the DGLGraph surface the reference touches
    def number_of_nodes(self) -> int:
        return self.n

    def number_of_edges(self) -> int:
        return int(self.col.size)

    num_nodes = number_of_nodes
    num_edges = number_of_edges

    def in_degrees(self) -> torch.Tensor:
        return torch.from_numpy(np.diff(self.rowptr).astype(np.int64))

    out_degrees = in_degrees

    def to(self, device) -> "GraphHandle":
        self.device = torch.device(device)
        return self

    def edges(self):
        rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.rowptr))
        return torch.from_numpy(self.col.astype(np.int64)), torch.from_numpy(rows)  # (src, dst)

    def __repr__(self) -> str:
        return f"GraphHandle(num_nodes={self.n}, num_edges={self.col.size})"

    def __getstate__(self):
        return {"n": self.n, "rowptr": self.rowptr, "col": self.col, "weight": self.weight}

    def __setstate__(self, st):
        self.__init__(st["n"], st["rowptr"], st["col"], st.get("weight"))

    # ---- kernels' view
    def row_index(self) -> np.ndarray:
        r = self._cache.get("rows")
        if r is None:
            r = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.rowptr))
            self._cache["rows"] = r
        return r

    def check_degrees(self) -> None:
        if self.n and int(np.diff(self.rowptr).min()) == 0:
            raise DGLError(
                "There are 0-in-degree nodes in the graph, output for those nodes will be invalid "
                "(GraphConv, allow_zero_in_degree=False)")

    def edge_values(self, inputs: Optional[torch.Tensor]) -> Optional[np.ndarray]:
        """Values the feature matrix ``inputs`` ([n, N], the padded adjacency) holds on the
        graph's edges, in CSR order; ``None`` when they are all exactly 1.  ``inputs`` must be
        zero off the edges (true for every call site of the reference:
        TrainingNeural.py:373,555; TestingNeuralNetwork.py:143)."""
        if inputs is None:
            w = self.weight
        else:
            key = ("vals", inputs.data_ptr(), inputs._version, tuple(inputs.shape), str(inputs.device))
            if key in self._cache:
                return self._cache[key]
            if inputs.dim() != 2 or inputs.shape[0] != self.n:
                raise ValueError(f"features must be [n={self.n}, N], got {tuple(inputs.shape)}")
            if inputs.shape[1] < self.n:
                raise ValueError("N should be greater than or equal to the original matrix size.")
            rows = torch.from_numpy(self.row_index()).to(inputs.device)
            cols = torch.from_numpy(self.col.astype(np.int64)).to(inputs.device)
            vals = inputs[rows, cols]
            if int(torch.count_nonzero(inputs)) != int(torch.count_nonzero(vals)):
                raise NotImplementedError(
                    "features with non-zeros off the graph's edges: this path implements the "
                    "reference's usage net(g, padded_adjacency) (TrainingNeural.py:373)")
            w = vals.detach().to("cpu", torch.float32).numpy()
            self._cache.clear()
            self._cache[key] = None if bool(np.all(w == 1.0)) else w
            return self._cache[key]
        if w is None or bool(np.all(w == 1.0)):
            return None
        return w


def from_networkx(nx_graph) -> GraphHandle:
    """``dgl.from_networkx`` for undirected graphs (graphExtender.py:102): labels sorted
    to 0..n-1, both directions of each edge, plus the ``weight`` attribute per edge."""
    if nx_graph.is_directed():
        raise NotImplementedError("directed graphs are outside the reference's data path")
    nodes = sorted(nx_graph.nodes())
    n = len(nodes)
    identity = nodes == list(range(n))
    index = None if identity else {u: i for i, u in enumerate(nodes)}
    m = nx_graph.number_of_edges()
    src = np.empty(m, np.int64); dst = np.empty(m, np.int64); w = np.empty(m, np.float32)
    for i, (u, v, wt) in enumerate(nx_graph.edges(data="weight", default=1)):
        src[i] = u if identity else index[u]
        dst[i] = v if identity else index[v]
        w[i] = wt
    loops = src == dst
    rows = np.concatenate([src, dst[~loops]])
    cols = np.concatenate([dst, src[~loops]])
    ww = np.concatenate([w, w[~loops]])
    order = np.lexsort((cols, rows))
    rows, cols, ww = rows[order], cols[order], ww[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    rowptr = np.cumsum(rowptr)
    return GraphHandle(n, rowptr.astype(np.int32), cols.astype(np.int32),
                       None if bool(np.all(ww == 1.0)) else ww)


PAIRS = ("both", "once")


def _check_pairs(pairs: str) -> None:
    if pairs not in PAIRS:
        raise ValueError(f"pairs must be one of {PAIRS}, got {pairs!r}")


def _host_array(x) -> np.ndarray:
    """``x`` (numpy, torch on any device, or anything ``np.asarray`` takes) as a numpy array on the host."""
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _integer_dtype(dtype) -> bool:
    if isinstance(dtype, torch.dtype):
        return dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
    return np.issubdtype(dtype, np.integer)


def _check_edge_arrays(edge_index, edge_weight) -> int:
    """Shapes and dtypes of an ``edge_index`` [2, E] / ``edge_weight`` [E] pair (numpy or torch); returns E."""
    shape = tuple(getattr(edge_index, "shape", ()))
    if len(shape) != 2 or shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got shape {shape}")
    if not _integer_dtype(edge_index.dtype):
        raise ValueError(f"edge_index must hold integers, got {edge_index.dtype}")
    E = int(shape[1])
    if edge_weight is not None:
        wshape = tuple(getattr(edge_weight, "shape", ()))
        if wshape != (E,):
            raise ValueError(f"edge_weight must be [E = {E}], got shape {wshape}")
        floating = edge_weight.dtype.is_floating_point if isinstance(edge_weight.dtype, torch.dtype) \
            else np.issubdtype(edge_weight.dtype, np.floating)
        if not (floating or _integer_dtype(edge_weight.dtype)):
            raise ValueError(f"edge_weight must hold real numbers, got {edge_weight.dtype}")
    return E


def from_edge_index(edge_index, num_nodes: int, edge_weight=None, pairs: str = "both") -> GraphHandle:
    """The ``GraphHandle`` of one undirected graph given as an ``edge_index`` [2, E] array of node ids 0..num_nodes-1
    (numpy or CPU torch, any integer dtype) and an optional ``edge_weight`` [E]: what ``from_networkx`` returns for the
    same graph, byte for byte (``rowptr``, ``col``, ``weight`` or ``None`` when every weight is exactly 1), in vectorised
    numpy.  ``pairs="both"``: every edge is listed in both directions and a self-loop once (the convention of the GNN
    libraries); ``pairs="once"``: every edge is listed once, in either orientation.  Raises ``ValueError`` for ids out of
    range, repeated entries, and - ``pairs="both"`` - an entry whose reverse is missing or carries another weight."""
    _check_pairs(pairs)
    E = _check_edge_arrays(edge_index, edge_weight)
    n = int(num_nodes)
    if n < 0 or n >= 2 ** 31:
        raise ValueError(f"num_nodes = {n}: need 0 <= num_nodes < 2^31")
    ei = _host_array(edge_index)
    rows, cols = ei[0].astype(np.int64), ei[1].astype(np.int64)
    if edge_weight is None:
        ww = np.ones(E, np.float32)
    else:
        ww = _host_array(edge_weight).astype(np.float32)
    bad = int(((rows < 0) | (rows >= n) | (cols < 0) | (cols >= n)).sum())
    if bad:
        raise ValueError(f"edge_index: {bad} entries with an id outside 0..{n - 1}")
    if pairs == "once":
        keep = rows != cols
        rows, cols, ww = (np.concatenate([rows, cols[keep]]), np.concatenate([cols, rows[keep]]),
                          np.concatenate([ww, ww[keep]]))
    if rows.size >= 2 ** 31:
        raise ValueError("graph too large for int32 indices")
    order = np.lexsort((cols, rows))
    rows, cols, ww = rows[order], cols[order], ww[order]
    dup = int(((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])).sum())
    if dup:
        raise ValueError(f"edge_index: {dup} repeated entries")
    keys = rows * max(n, 1) + cols   # ascending (the sort above) and distinct: every entry's reverse is looked up in it
    at = np.minimum(np.searchsorted(keys, cols * max(n, 1) + rows), max(keys.size - 1, 0))
    asym = int(((keys[at] != cols * max(n, 1) + rows) | (ww[at] != ww)).sum())
    if asym:
        raise ValueError(f"edge_index: {asym} entries whose reverse is missing or carries another weight")
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return GraphHandle(n, rowptr.astype(np.int32), cols.astype(np.int32),
                       None if bool(np.all(ww == 1.0)) else ww)


def _check_pins(nodes, classes, number_classes) -> int:
    """Shapes and dtypes of a pin list (``nodes`` [P], ``classes`` [P]; numpy or torch) and the class count; returns P.
    Touches neither the library nor a device."""
    K = int(number_classes)
    if not 2 <= K <= hip.KWAY_MAX_CLASSES:
        raise ValueError(f"number_classes must be in 2..{hip.KWAY_MAX_CLASSES}, got {K}")
    for name, a in (("nodes", nodes), ("classes", classes)):
        shape = getattr(a, "shape", None)
        if shape is None or len(tuple(shape)) != 1:
            raise ValueError(f"{name} must be a one-dimensional array, got {type(a).__name__}"
                             + ("" if shape is None else f" of shape {tuple(shape)}"))
        if not _integer_dtype(a.dtype):
            raise ValueError(f"{name} must hold integers, got {a.dtype}")
    if tuple(nodes.shape) != tuple(classes.shape):
        raise ValueError(f"nodes and classes must have one length, got {tuple(nodes.shape)} and {tuple(classes.shape)}")
    return int(nodes.shape[0])


def _pin_ids(a, top: int, device) -> torch.Tensor:
    """A pin list's ids or classes as contiguous int32 on ``device``.  Values beyond int32 must not wrap into range, so
    anything but int32 is clamped to -1..``top`` first - both are refused on the device - and clamped as int64: neither
    bound need fit a narrow dtype, and a uint64 beyond int64 turns negative."""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if a.dtype != np.int32:
            a = np.clip(a.astype(np.int64), -1, top).astype(np.int32)
        a = torch.from_numpy(np.ascontiguousarray(a))
    a = a.to(device)
    return (a if a.dtype == torch.int32 else a.to(torch.int64).clamp(-1, top).to(torch.int32)).contiguous()


def _pin_faults(rep: dict, K: int) -> None:
    """Raise ``ValueError`` for a contraction report (``hip.CT_REPORT`` names -> counts) with bad input in it."""
    kinds = [("pin_out_of_range", "{} pins with a node id out of range"),
             ("pin_class", "{} pins with a class outside 0.." + str(K - 1)),
             ("pin_conflict", "{} nodes pinned to two different classes"),
             ("graphs_missing_class", "{} graphs in which some class has no pinned node (pin every class in every graph: "
                                      "a class without a pin has no terminal to stand for it)"),
             ("graphs_no_free", "{} graphs without a free node (nothing is left to solve)"),
             ("bare_terminals", "{} (graph, class) pairs whose pinned nodes have no free neighbour (pin a node with a free "
                                "neighbour in that class: the class's terminal would be a node without neighbours)")]
    found = [text.format(rep[k]) for k, text in kinds if rep[k]]
    if found:
        raise ValueError("pins: " + "; ".join(found))


def _sequential_sums(keys: np.ndarray, w: np.ndarray):
    """``(distinct keys, float32 sums)`` of ``w`` grouped by the ascending ``keys``: every sum starts at +0 and adds its
    group's weights one after the other in array order (the k-th step of every group in one vector operation)."""
    if keys.size == 0:
        return keys[:0], np.zeros(0, np.float32)
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    length = np.diff(np.concatenate([first, [keys.size]]))
    sums = np.zeros(first.size, np.float32)
    for k in range(int(length.max())):
        m = length > k
        sums[m] = sums[m] + w[first[m] + k]
    return keys[first], sums


def _fold_fixed_cut(t: np.ndarray) -> np.float32:
    """The fixed-shape fold of include/gcnmaxcut.h over one graph's per-row sums ``t`` [n] (float32): tiles of 256 rows,
    a butterfly over each quarter of 64, the quarters in order, the tiles in order."""
    tiles = (t.size + 255) // 256
    v = np.zeros(tiles * 256, np.float32)
    v[:t.size] = t
    v = v.reshape(tiles, 4, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ d]
    q = v[:, :, 0]
    part = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    return np.cumsum(np.concatenate([np.zeros(1, np.float32), part]), dtype=np.float32)[-1]


class HostContraction:
    """What :func:`contract` returns: ``handle`` (the contracted graph), ``node_map`` [n] int32, ``fixed_cut`` (float32),
    ``pinned`` [n] bool, and ``lift``."""

    def __init__(self, handle: GraphHandle, node_map: np.ndarray, fixed_cut: np.float32, pinned: np.ndarray):
        self.handle, self.node_map, self.fixed_cut, self.pinned = handle, node_map, fixed_cut, pinned

    def lift(self, partition) -> np.ndarray:
        """The partition of the original nodes a partition of the contracted graph stands for."""
        return np.asarray(partition)[self.node_map].astype(np.int32)

    def contract_cost(self, node_cost):
        """Per-node class costs [n, K] of the original graph -> (the costs of the contracted graph [n_out, K] float32,
        ``fixed_cost`` float32): a free node's row goes to its contracted row, the K super-nodes get zero rows, and
        ``fixed_cost`` is the sum of ``node_cost[v][class_v]`` over the pinned nodes (a float64 running sum in node
        order, rounded once).  The host twin of ``Contraction.contract_cost``."""
        cost = np.asarray(node_cost, np.float32)
        K = cost.shape[1]
        free = ~self.pinned
        out = np.zeros((self.handle.n, K), np.float32)
        out[self.node_map[free]] = cost[free]
        picked = cost[np.flatnonzero(self.pinned), self.node_map[self.pinned]].astype(np.float64)
        return out, np.float32(np.cumsum(picked)[-1] if picked.size else 0.0)


def contract(handle: GraphHandle, nodes, classes, number_classes: int) -> HostContraction:
    """Contract the pinned nodes of one graph on the host, in vectorised numpy: the host twin of
    ``GraphBatch.contract`` and the rule of include/gcnmaxcut.h ("pinning any nodes to classes") array for array.
    ``nodes`` [P] are node ids of ``handle``, ``classes`` [P] their classes in 0..number_classes-1 (numpy or CPU torch, any
    integer dtype, any order; a repeated identical pin is harmless).  Every node pinned to class c becomes node c of the
    result, the free nodes follow in ascending order from ``number_classes``, parallel edges are merged by adding their
    weights, edges between pinned nodes of different classes add up to ``fixed_cut``.  Bad pins raise ``ValueError``
    naming the kind and the count, as ``GraphBatch.contract`` does."""
    _check_pins(nodes, classes, number_classes)
    K, n = int(number_classes), handle.n
    nd, cl = _host_array(nodes), _host_array(classes)
    # (compared as Python-sized integers: no id wraps into range)
    node_ok = (nd >= 0) & (nd < n)
    class_ok = (cl >= 0) & (cl < K)
    rep = dict.fromkeys(hip.CT_REPORT, 0)
    rep["pin_out_of_range"] = int((~node_ok).sum())
    rep["pin_class"] = int((node_ok & ~class_ok).sum())
    ok = node_ok & class_ok
    pairs = np.unique(nd[ok].astype(np.int64) * K + cl[ok].astype(np.int64))
    pin_node, pin_class = pairs // K, pairs % K
    rep["pin_conflict"] = int((np.unique(pin_node, return_counts=True)[1] > 1).sum())
    cls = np.full(n, -1, np.int64)
    cls[pin_node[::-1]] = pin_class[::-1]   # (with a conflict: the smallest class; the call raises below anyway)
    free = cls < 0
    rows, cols = handle.row_index(), handle.col.astype(np.int64)
    w = np.ones(cols.size, np.float32) if handle.weight is None else handle.weight
    row_free, col_free = free[rows], free[cols]
    present = np.zeros(K, bool)
    present[cls[~free]] = True
    touched = np.zeros(K, bool)
    touched[cls[cols[row_free & ~col_free]]] = True
    rep["graphs_missing_class"] = int(not present.all())
    rep["graphs_no_free"] = int(not free.any())
    rep["bare_terminals"] = int((present & ~touched).sum())
    _pin_faults(rep, K)
    new_id = np.where(free, K + np.cumsum(free) - 1, cls)
    ff = row_free & col_free
    fp = np.flatnonzero(row_free & ~col_free)
    key = rows[fp] * K + cls[cols[fp]]
    order = np.argsort(key, kind="stable")   # a (row, class) group keeps its ascending columns
    groups, sums = _sequential_sums(key[order], w[fp][order])
    v, c = new_id[groups // K], groups % K
    out_rows = np.concatenate([new_id[rows[ff]], v, c])
    out_cols = np.concatenate([new_id[cols[ff]], c, v])
    out_w = np.concatenate([w[ff], sums, sums])
    order = np.lexsort((out_cols, out_rows))
    out_rows, out_cols, out_w = out_rows[order], out_cols[order], out_w[order]
    n_out = K + int(free.sum())
    rowptr = np.zeros(n_out + 1, np.int64)
    np.cumsum(np.bincount(out_rows, minlength=n_out), out=rowptr[1:])
    pp = np.flatnonzero(~row_free & ~col_free & (cols > rows) & (cls[rows] != cls[cols]))
    t = np.zeros(n, np.float32)
    at, per_row = _sequential_sums(rows[pp], w[pp])
    t[at] = per_row
    out = GraphHandle(n_out, rowptr.astype(np.int32), out_cols.astype(np.int32),
                      None if bool(np.all(out_w == 1.0)) else out_w.astype(np.float32))
    return HostContraction(out, new_id.astype(np.int32), _fold_fixed_cut(t), ~free)


class BatchArrays:
    """Host-side (numpy) form of a block-diagonal batch: everything ``struct gmc_batch``
    points to, built without touching a GPU (so the layout is testable on CPU)."""

    def __init__(self, handles: Sequence[GraphHandle], values: Optional[Sequence[Optional[np.ndarray]]] = None,
                 allow_zero_degree: bool = False):
        """``allow_zero_degree``: nodes without neighbours are no error.  GraphConv refuses them as DGL does, and so does
        every function of the Python API that builds its batches itself (the trainer, ``net(g, X)``, ``evaluate_model``, the
        decoders), whatever the model's first layer; the attention layer gives every row a self term, so a caller of the
        engine (``FusedEngine(..., attention=True)``: forward, train_fwd_bwd) may hand it a batch built with this flag."""
        B = len(handles)
        ns = np.asarray([h.n for h in handles], np.int64)
        for h in handles:
            if h.n < 3 or h.n > hip.LARGE_MAX_GRAPH_NODES:
                raise ValueError(f"graph with {h.n} nodes: need 3 <= n <= {hip.LARGE_MAX_GRAPH_NODES}")
            if not allow_zero_degree:
                h.check_degrees()
        goff = np.zeros(B + 1, np.int64)
        np.cumsum(ns, out=goff[1:])
        nnzs = np.asarray([h.col.size for h in handles], np.int64)
        eoff = np.zeros(B + 1, np.int64)
        np.cumsum(nnzs, out=eoff[1:])
        if goff[-1] >= 2 ** 31 or eoff[-1] >= 2 ** 31:
            raise ValueError("batch too large for int32 indices")
        rowptr = np.zeros(int(goff[-1]) + 1, np.int32)
        lcol = np.empty(int(eoff[-1]), np.int32)
        gcol = np.empty(int(eoff[-1]), np.int32)
        if values is None:
            values = [h.edge_values(None) for h in handles]
        unit = all(v is None for v in values)
        vals = None if unit else np.ones(int(eoff[-1]), np.float32)
        for g, h in enumerate(handles):
            rowptr[goff[g] + 1: goff[g + 1] + 1] = h.rowptr[1:] + eoff[g]
            lcol[eoff[g]:eoff[g + 1]] = h.col
            gcol[eoff[g]:eoff[g + 1]] = h.col + goff[g]
            if vals is not None and values[g] is not None:
                vals[eoff[g]:eoff[g + 1]] = values[g]
        degi = np.diff(rowptr)
        dinv = (1.0 / np.sqrt(np.maximum(degi.astype(np.float32), 1.0))).astype(np.float32)
        # ELL copy for the LDS-tiled kernels: W slots per row (8 or 16) holding the row's first W neighbours
        # (CSR order, then re-arranged over the slots by the library), padded with the graph's node count (the id
        # of an all-zero tile row) / weight 0.  Neighbours beyond the W-th of a row go to the overflow lists
        # (blocks of eight ids per row): a hub node costs its own extra blocks, the batch stays on the LDS path.
        ell = ell_vals = None
        ovf_ptr = ovf_ids = ovf_vals = None
        ovf_max_blocks = 0
        ell_slots = 0
        max_deg = int(degi.max()) if degi.size else 0
        R = int(goff[-1])
        W = self.choose_width(degi)
        if B and int(ns.max()) > hip.MAX_GRAPH_NODES:   # no LDS-tiled kernel serves such a batch: no table for it
            W = 0
        if W and int(ns.max()) < 65535:
            deg64 = degi.astype(np.int64)
            slot = np.arange(int(eoff[-1]), dtype=np.int64) - np.repeat(rowptr[:-1].astype(np.int64), deg64)
            rows = np.repeat(np.arange(R, dtype=np.int64), deg64)
            n_of_row = np.repeat(ns, ns)
            inside = slot < W
            ell = n_of_row.astype(np.uint16)[:, None].repeat(W, axis=1)
            ell[rows[inside], slot[inside]] = lcol[inside].astype(np.uint16)
            if vals is not None:
                ell_vals = np.zeros((R, W), np.float32)
                ell_vals[rows[inside], slot[inside]] = vals[inside]
            if max_deg > W:
                blocks = (np.maximum(deg64 - W, 0) + 7) // 8
                ovf_ptr = np.zeros(R + 1, np.int64)
                np.cumsum(blocks, out=ovf_ptr[1:])
                # what the kernels' 16-bit row descriptors can say: <= 15 blocks per row (degree <= W + 120), <= 4095
                # blocks per graph; beyond that the batch takes the row kernels
                ovf_max_blocks = int(np.diff(ovf_ptr[goff]).max())
                if int(blocks.max()) > 15 or ovf_max_blocks > 4095:
                    W = 0
            if W and max_deg > W:
                nblk = int(ovf_ptr[-1])
                ovf_ids = np.repeat(n_of_row.astype(np.uint16), blocks * 8)       # padding: the zero row of the graph
                where = ovf_ptr[:-1][rows[~inside]] * 8 + (slot[~inside] - W)
                ovf_ids[where] = lcol[~inside].astype(np.uint16)
                if vals is not None:
                    ovf_vals = np.zeros(nblk * 8, np.float32)
                    ovf_vals[where] = vals[~inside]
                ovf_ptr = ovf_ptr.astype(np.int32)
            if not W:
                ell = ell_vals = ovf_ptr = None
                ovf_max_blocks = 0
        if W and int(ns.max()) < 65535:
            # LDS-bank-aware slot order (host routine of the library; plain CSR order otherwise)
            try:
                lib = hip.load()
            except hip.HipExtensionError:
                lib = None
            if lib is not None:
                ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
                go32 = goff.astype(np.int32)
                rc = lib.gmc_ell_arrange_host(B, ptr(go32), ptr(rowptr), ptr(lcol), ptr(vals), W, ptr(ell), ptr(ell_vals))
                hip.check(rc, "gmc_ell_arrange_host")
                # s < W when no row of the batch has more than s neighbours: slots s.. of every row are then padding
                ell_slots = int(lib.gmc_ell_slots_for(R, ptr(rowptr), W))
        self.B, self.R, self.nnz = B, int(goff[-1]), int(eoff[-1])
        self.n_max = int(ns.max()) if B else 0
        self.nnz_max = int(nnzs.max()) if B else 0
        self.uniform_n = int(ns[0]) if B and bool(np.all(ns == ns[0])) else 0
        self.sizes, self.goff = ns, goff
        self.rowptr, self.gcol, self.lcol, self.vals, self.dinv = rowptr, gcol, lcol, vals, dinv
        self.ell, self.ell_vals, self.ell_width = ell, ell_vals, (W if ell is not None else 0)
        self.ell_slots = ell_slots if ell is not None else 0   # (without the library: CSR slot order, every slot live)
        self.ovf_ptr, self.ovf_ids, self.ovf_vals = ovf_ptr, ovf_ids, ovf_vals
        self.ovf_max_blocks = ovf_max_blocks if ovf_ptr is not None else 0
        self.max_degree = max_deg

    @staticmethod
    def choose_width(degi: np.ndarray) -> int:
        """Slots per row of the ELL table for rows of these degrees; 0 = no table (row kernels).  8 when (almost)
        every row has at most 8 neighbours - up to one row in 200 may be longer, its extra neighbours become
        overflow blocks - else 16 with the same allowance; no table once the overflow lists would hold more than
        an eighth of the edges (dense graphs: the row kernels read those from HBM / L2 anyway)."""
        if degi.size == 0 or int(degi.max()) <= 0:
            return 0
        R, nnz = degi.size, int(degi.sum())
        for W in (8, 16):
            over = degi > W
            if int(over.sum()) * 200 <= R or (W == 16 and int((degi[over] - W).sum()) * 8 <= nnz):
                return W
        return 0


class GraphBatch:
    """Block-diagonal batch resident on one GPU; mirrors ``struct gmc_batch``."""

    def __init__(self, handles: Sequence[GraphHandle], values: Optional[Sequence[Optional[np.ndarray]]] = None,
                 device: Optional[torch.device] = None, allow_zero_degree: bool = False):
        device = device or hip.require_gpu()
        self.device = device
        h = BatchArrays(handles, values, allow_zero_degree)
        self.host = h
        self.B, self.R, self.nnz, self.n_max, self.uniform_n = h.B, h.R, h.nnz, h.n_max, h.uniform_n
        self.sizes, self.goff_host = h.sizes, h.goff
        dev = lambda a: None if a is None else torch.from_numpy(a).to(device)
        self.goff = dev(h.goff.astype(np.int32))
        self.rowptr, self.gcol, self.lcol = dev(h.rowptr), dev(h.gcol), dev(h.lcol)
        self.vals, self.dinv = dev(h.vals), dev(h.dinv)
        self.ell = None if h.ell is None else torch.from_numpy(h.ell.view(np.int16)).to(device)
        self.ell_vals = dev(h.ell_vals)
        self.ovf_ptr = dev(h.ovf_ptr)
        self.ovf_ids = None if h.ovf_ids is None else torch.from_numpy(h.ovf_ids.view(np.int16)).to(device)
        self.ovf_vals = dev(h.ovf_vals)
        self.c = hip.GmcBatch(
            B=h.B, R=h.R, nnz=h.nnz, n_max=h.n_max, uniform_n=h.uniform_n, nnz_max=h.nnz_max,
            goff=hip.ptr(self.goff), rowptr=hip.ptr(self.rowptr), gcol=hip.ptr(self.gcol),
            lcol=hip.ptr(self.lcol), vals=hip.ptr(self.vals), dinv=hip.ptr(self.dinv),
            ell=hip.ptr(self.ell), ell_vals=hip.ptr(self.ell_vals), ell_width=h.ell_width, ell_slots=h.ell_slots,
            ovf_ptr=hip.ptr(self.ovf_ptr), ovf_ids=hip.ptr(self.ovf_ids), ovf_vals=hip.ptr(self.ovf_vals),
            ovf_max_blocks=h.ovf_max_blocks)

    @classmethod
    def from_edge_index(cls, edge_index, ptr=None, num_nodes: Optional[int] = None, edge_weight=None, *,
                        pairs: str = "both", device: Optional[torch.device] = None,
                        allow_zero_degree: bool = False) -> "GraphBatch":
        """The batch of the graphs an ``edge_index`` [2, E] tensor describes, built on the GPU: every array and scalar
        equals, byte for byte, what ``GraphBatch([from_networkx(g) for g in graphs])`` holds for the same graphs.

        ``edge_index``: global node ids in block-diagonal numbering (graph ``g`` owns ``ptr[g] .. ptr[g+1]-1``), any
        integer dtype, numpy or torch, on the CPU or already on the device.  ``ptr`` [B+1] is PyG's ``Batch.ptr``; for
        one graph pass ``num_nodes`` instead.  ``edge_weight`` [E] is optional; weights that are all exactly 1.0 give
        ``vals is None``.  ``pairs="both"``: every undirected edge is present in both directions and a self-loop once
        (PyG's convention); ``pairs="once"``: every edge is listed once in either orientation and the flipped entries
        are appended here.

        Shapes, dtypes, a ``ptr`` that does not ascend from 0, graph sizes outside 3..``hip.LARGE_MAX_GRAPH_NODES`` and
        the int32 limits raise ``ValueError`` before the library is loaded.  What only the data can tell - ids out of
        range, endpoints in two graphs, repeated entries, an entry whose reverse is missing or weighted differently,
        nodes without neighbours (unless ``allow_zero_degree``) - is counted on the device (such entries are never used
        as an index) and raises ``ValueError`` naming the kind and the count, before the table stage is launched.

        Synchronisation: the call reads the device's report (80 bytes) once, between gmc_batch_build_csr and
        gmc_batch_build_table; that read is the only point at which it waits for the GPU when ``ptr`` is host data and
        ``pairs="both"``.  (``ptr`` is needed on the host and is copied there when it is a device tensor; ``"once"``
        selects the non-loop entries with a boolean mask, whose length torch reads back.)

        The result is an ordinary ``GraphBatch``; ``.host`` (what ``refine_order`` and the colour orders read) is copied
        back from the device on first access."""
        _check_pairs(pairs)
        E = _check_edge_arrays(edge_index, edge_weight)
        if (ptr is None) == (num_nodes is None):
            raise ValueError("pass exactly one of ptr (graph boundaries) and num_nodes (a single graph)")
        if ptr is None:
            goff = np.asarray([0, int(num_nodes)], np.int64)
        else:
            p = _host_array(ptr)
            if p.ndim != 1 or p.size < 1:
                raise ValueError(f"ptr must be [B + 1], got shape {tuple(p.shape)}")
            if not np.issubdtype(p.dtype, np.integer):
                raise ValueError(f"ptr must hold integers, got {p.dtype}")
            goff = p.astype(np.int64)
            if int(goff[0]) != 0 or bool(np.any(np.diff(goff) < 0)):
                raise ValueError("ptr must ascend from 0")
        ns = np.diff(goff)
        B = int(ns.size)
        for n in ns:
            if n < 3 or n > hip.LARGE_MAX_GRAPH_NODES:
                raise ValueError(f"graph with {int(n)} nodes: need 3 <= n <= {hip.LARGE_MAX_GRAPH_NODES}")
        R = int(goff[-1])
        if R >= 2 ** 31 or E * (2 if pairs == "once" else 1) >= 2 ** 31:
            raise ValueError("batch too large for int32 indices")
        if B == 0 and E:
            raise ValueError(f"edge_index holds {E} entries but ptr describes no graph")
        device = device or hip.require_gpu()
        lib = hip.load()
        ei = edge_index if isinstance(edge_index, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(edge_index))
        ei = ei.to(device)
        if ei.dtype != torch.int32:   # ids beyond int32 must not wrap into range: -1 and R are both refused on the device
            ei = ei.clamp(-1, R).to(torch.int32)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        w = None
        if edge_weight is not None:
            w = edge_weight if isinstance(edge_weight, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(edge_weight))
            w = w.to(device=device, dtype=torch.float32).contiguous()
        if pairs == "once":
            keep = src != dst
            src, dst = torch.cat([src, dst[keep]]), torch.cat([dst, src[keep]])
            if w is not None:
                w = torch.cat([w, w[keep]])
            E = int(src.numel())
            if E >= 2 ** 31:
                raise ValueError("batch too large for int32 indices")
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
        self = cls.__new__(cls)
        self.device = device
        self.B, self.R, self.sizes, self.goff_host = B, R, ns, goff
        self.n_max = int(ns.max()) if B else 0
        self.uniform_n = int(ns[0]) if B and bool(np.all(ns == ns[0])) else 0
        self.goff = torch.from_numpy(goff.astype(np.int32)).to(device)
        self.rowptr = torch.zeros(R + 1, dtype=torch.int32, device=device) if B == 0 else new(R + 1, torch.int32)
        self.gcol, self.lcol, self.dinv = new(E, torch.int32), new(E, torch.int32), new(R, torch.float32)
        self.vals = None if w is None else new(E, torch.float32)
        self.ell = self.ell_vals = self.ovf_ptr = self.ovf_ids = self.ovf_vals = None
        W = ell_slots = ovf_max_blocks = max_degree = nnz_max = 0
        if B:
            report = new(hip.BB_REPORT_WORDS, torch.int32)
            ws = new(int(lib.gmc_batch_build_workspace_bytes(B, R, E)), torch.uint8)
            rc = lib.gmc_batch_build_csr(B, R, E, hip.ptr(self.goff), hip.ptr(src), hip.ptr(dst), hip.ptr(w),
                                         hip.ptr(self.rowptr), hip.ptr(self.lcol), hip.ptr(self.gcol), hip.ptr(self.vals),
                                         hip.ptr(self.dinv), hip.ptr(report), hip.ptr(ws), ws.numel(), hip.stream())
            hip.check(rc, "gmc_batch_build_csr")
            rep = dict(zip(hip.BB_REPORT, report.cpu().tolist()))   # the call's one wait for the device
            faults = [("out_of_range", "with an id outside 0..R-1"), ("cross_graph", "whose endpoints lie in two graphs"),
                      ("duplicate", "that repeat another entry"),
                      ("asymmetric", "whose reverse entry is missing or carries another weight")]
            found = [f"{rep[k]} entries {what}" for k, what in faults if rep[k]]
            if rep["zero_degree"] and not allow_zero_degree:
                found.append(f"{rep['zero_degree']} nodes without neighbours (allow_zero_degree=False)")
            if found:
                raise ValueError("edge_index: " + "; ".join(found))
            max_degree, nnz_max = rep["max_degree"], rep["nnz_max"]
            if w is not None and rep["non_unit"] == 0:
                self.vals = None
            W = 0
            if max_degree > 0:   # BatchArrays.choose_width on the report's statistics
                for cand in (8, 16):
                    if rep[f"rows_over_{cand}"] * 200 <= R or (cand == 16 and rep["excess_16"] * 8 <= E):
                        W = cand
                        break
            if self.n_max > hip.MAX_GRAPH_NODES or self.n_max >= 65535:
                W = 0
            blocks = 0
            if W and max_degree > W:
                ovf_max_blocks, blocks = rep[f"graph_blocks_{W}"], rep[f"blocks_{W}"]
                if rep[f"row_blocks_{W}"] > 15 or ovf_max_blocks > 4095:
                    W = ovf_max_blocks = blocks = 0
            if W:
                ell_slots = max(min(max_degree, W), 7 if W == 8 else 9)   # gmc_ell_slots_for
                self.ell = new((R, W), torch.int16)
                if self.vals is not None:
                    self.ell_vals = new((R, W), torch.float32)
                if max_degree > W:
                    self.ovf_ptr, self.ovf_ids = new(R + 1, torch.int32), new(blocks * 8, torch.int16)
                    if self.vals is not None:
                        self.ovf_vals = new(blocks * 8, torch.float32)
                rc = lib.gmc_batch_build_table(B, R, self.n_max, hip.ptr(self.goff), hip.ptr(self.rowptr),
                                               hip.ptr(self.lcol), hip.ptr(self.vals), W, ell_slots, hip.ptr(self.ell),
                                               hip.ptr(self.ell_vals), hip.ptr(self.ovf_ptr), hip.ptr(self.ovf_ids),
                                               hip.ptr(self.ovf_vals), blocks, hip.ptr(ws), ws.numel(), hip.stream())
                hip.check(rc, "gmc_batch_build_table")
        self.nnz = E
        self._scalars = dict(nnz_max=nnz_max, max_degree=max_degree, ell_width=W, ell_slots=ell_slots,
                             ovf_max_blocks=ovf_max_blocks)
        self.c = hip.GmcBatch(
            B=B, R=R, nnz=E, n_max=self.n_max, uniform_n=self.uniform_n, nnz_max=nnz_max,
            goff=hip.ptr(self.goff), rowptr=hip.ptr(self.rowptr), gcol=hip.ptr(self.gcol),
            lcol=hip.ptr(self.lcol), vals=hip.ptr(self.vals), dinv=hip.ptr(self.dinv),
            ell=hip.ptr(self.ell), ell_vals=hip.ptr(self.ell_vals), ell_width=W, ell_slots=ell_slots,
            ovf_ptr=hip.ptr(self.ovf_ptr), ovf_ids=hip.ptr(self.ovf_ids), ovf_vals=hip.ptr(self.ovf_vals),
            ovf_max_blocks=ovf_max_blocks)
        return self

    def contract(self, nodes, classes, number_classes: int) -> "Contraction":
        """Pin ``nodes`` [P] (global row ids of this batch) to ``classes`` [P] (0..number_classes-1) and contract them on
        the GPU: every node pinned to class c of a graph becomes local node c of the contracted graph, the free nodes
        follow in ascending order, parallel edges are merged by adding their weights (the rule and its sum orders:
        include/gcnmaxcut.h, "pinning any nodes to classes").  The result's ``batch`` is the problem ``terminals=True``
        solves; ``lift`` carries a partition of it back to this batch's rows, and the cut of the lifted partition is the
        contracted one plus ``fixed_cut``.

        ``nodes`` / ``classes``: any integer dtype, numpy or torch, on the CPU or the device, in any order; a repeated
        identical pin is harmless.  Shapes, dtypes and ``number_classes`` outside 2..8 raise ``ValueError`` before the
        library is loaded.  What only the data can tell is counted on the device and raises ``ValueError`` naming the kind
        and the count before the entries are emitted: ids or classes out of range (such a pin is never used as an index),
        a node pinned to two classes, a graph in which some class has no pin (a graph without pins included), a graph
        without a free node, and a class of a graph whose pinned nodes have no free neighbour.

        Synchronisation: the call waits for the device once, to read the report and the contracted graphs' offsets (one
        copy); ``GraphBatch.from_edge_index``, which builds ``batch`` from the emitted entries, then reads its own
        report."""
        P = _check_pins(nodes, classes, number_classes)
        K, B, R, device = int(number_classes), self.B, self.R, self.device
        lib = hip.load()

        pin_node, pin_class = _pin_ids(nodes, R, device), _pin_ids(classes, K, device)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
        words = new(hip.CT_REPORT_WORDS + B + 1, torch.int32)   # the report and goff_out: read back in one copy
        report, goff_out = words[:hip.CT_REPORT_WORDS], words[hip.CT_REPORT_WORDS:]
        node_map, fixed_cut = new(R, torch.int32), new(B, torch.float32)
        if B == 0:
            empty = GraphBatch.from_edge_index(new((2, 0), torch.int32), np.zeros(1, np.int64), device=device)
            return Contraction(empty, node_map, fixed_cut, new(R, torch.bool))
        ws = new(int(lib.gmc_contract_workspace_bytes(B, R, self.nnz, K)), torch.uint8)
        rc = lib.gmc_contract_map(self.ref(), K, P, hip.ptr(pin_node), hip.ptr(pin_class), hip.ptr(node_map),
                                  hip.ptr(goff_out), hip.ptr(report), hip.ptr(ws), ws.numel(), hip.stream())
        hip.check(rc, "gmc_contract_map")
        host = words.cpu().numpy()   # the call's one wait for the device
        rep = dict(zip(hip.CT_REPORT, host[:hip.CT_REPORT_WORDS].tolist()))
        _pin_faults(rep, K)
        E = rep["nnz"]
        entries, w = new((2, E), torch.int32), new(E, torch.float32)
        rc = lib.gmc_contract_entries(self.ref(), K, hip.ptr(node_map), hip.ptr(goff_out), E, hip.ptr(entries[0]),
                                      hip.ptr(entries[1]), hip.ptr(w), hip.ptr(fixed_cut), hip.ptr(ws), ws.numel(),
                                      hip.stream())
        hip.check(rc, "gmc_contract_entries")
        batch = GraphBatch.from_edge_index(entries, host[hip.CT_REPORT_WORDS:].astype(np.int64), edge_weight=w,
                                           device=device)
        # pinned rows sit in the first K rows of their contracted graph (a binary search per row over goff_out)
        first = goff_out[torch.bucketize(node_map, goff_out[1:], right=True).clamp_(max=B - 1)]
        return Contraction(batch, node_map, fixed_cut, node_map < first + K)

    def __getattr__(self, name):
        # only reached for attributes the instance lacks: a batch built on the device has no ``host`` until it is asked for
        if name == "host" and "_scalars" in self.__dict__:
            h = BatchArrays.__new__(BatchArrays)
            back = lambda t, dtype=None: None if t is None else (t.cpu().numpy() if dtype is None else t.cpu().numpy().view(dtype))
            h.B, h.R, h.nnz, h.n_max, h.uniform_n = self.B, self.R, self.nnz, self.n_max, self.uniform_n
            h.sizes, h.goff = self.sizes, self.goff_host
            h.rowptr, h.gcol, h.lcol = back(self.rowptr), back(self.gcol), back(self.lcol)
            h.vals, h.dinv = back(self.vals), back(self.dinv)
            h.ell, h.ell_vals = back(self.ell, np.uint16), back(self.ell_vals)
            h.ovf_ptr, h.ovf_ids, h.ovf_vals = back(self.ovf_ptr), back(self.ovf_ids, np.uint16), back(self.ovf_vals)
            for k, v in self._scalars.items():
                setattr(h, k, v)
            self.__dict__["host"] = h
            return h
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def handles(self) -> List[GraphHandle]:
        """One ``GraphHandle`` per graph of the batch, from the batch's own arrays (read through ``.host``): what
        ``from_networkx`` gives for each graph, for the entry points that take dataset items."""
        h = self.host
        out = []
        for g in range(h.B):
            r0, r1 = int(h.goff[g]), int(h.goff[g + 1])
            e0, e1 = int(h.rowptr[r0]), int(h.rowptr[r1])
            wt = None if h.vals is None else h.vals[e0:e1]
            out.append(GraphHandle(r1 - r0, h.rowptr[r0:r1 + 1] - e0, h.lcol[e0:e1],
                                   None if wt is None or bool(np.all(wt == 1.0)) else wt.copy()))
        return out

    def ref(self):
        return C.byref(self.c)

    def refine_order(self, K: int = 3, terminals: bool = True):
        """(order, cgoff, cptr) on the device: the colour classes gmc_refine_local_f32 walks (gmc_refine_order_host),
        or, for ``K`` other than 3, the ones gmc_round_conditional_f32 walks when nodes 0..K-1 are the terminals
        (gmc_round_order_host).  A batch with a graph beyond ``hip.MAX_GRAPH_NODES`` nodes gets the same arrays from
        gmc_large_round_order_host (the order gmc_large_round_conditional_f32 walks).  Computed on first use and kept
        with the batch, per ``(K, terminals)``; batches that are never refined never pay for it.

        ``terminals=False``: no node is fixed, every node is coloured and ``order`` holds all ``R`` rows
        (gmc_order_host_t): the order the ``_t`` entry points walk with ``terminals = 0``."""
        K, terminals = int(K), bool(terminals)
        key = (K, terminals)
        cache = self.__dict__.setdefault("_refine", {})
        if key not in cache:
            classes = C.c_int32(-1)   # the largest class count of any graph: known without a look at cgoff
            h = self.host
            order = np.zeros(max(h.R, 1), np.int32)
            cgoff = np.zeros(h.B + 1, np.int32)
            cptr = np.zeros(h.R + h.B, np.int32)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            go32 = h.goff.astype(np.int32)
            if not terminals:
                rc = hip.load().gmc_order_host_t(h.B, ptr(go32), ptr(h.rowptr), ptr(h.lcol), K, 0, ptr(order), ptr(cgoff),
                                                 ptr(cptr), cptr.size, C.byref(classes))
                hip.check(rc, "gmc_order_host_t")
            elif h.B and h.n_max > hip.MAX_GRAPH_NODES:
                rc = hip.load().gmc_large_round_order_host(h.B, ptr(go32), ptr(h.rowptr), ptr(h.lcol), K, ptr(order),
                                                           ptr(cgoff), ptr(cptr), cptr.size, C.byref(classes))
                hip.check(rc, "gmc_large_round_order_host")
            elif K == 3:
                rc = hip.load().gmc_refine_order_host(h.B, ptr(go32), ptr(h.rowptr), ptr(h.lcol), ptr(order),
                                                      ptr(cgoff), ptr(cptr), cptr.size)
                hip.check(rc, "gmc_refine_order_host")
            else:
                rc = hip.load().gmc_round_order_host(h.B, ptr(go32), ptr(h.rowptr), ptr(h.lcol), K, ptr(order),
                                                     ptr(cgoff), ptr(cptr), cptr.size)
                hip.check(rc, "gmc_round_order_host")
            dev = lambda a: torch.from_numpy(a).to(self.device)
            cache[key] = (dev(order), dev(cgoff), dev(cptr[:max(int(cgoff[-1]), 1)].copy()))
            if classes.value < 0:
                classes.value = int(np.diff(cgoff).max()) - 1 if h.B else 0
            self.__dict__.setdefault("_refine_classes", {})[key] = int(classes.value)
        return cache[key]

    def refine_classes(self, K: int = 3, terminals: bool = True) -> int:
        """The largest number of colour classes any graph of the batch has in ``refine_order(K, terminals)``: the colour launches
        gmc_large_round_conditional_f32 / gmc_large_local_search_f32 issue per sweep (0 for an empty batch)."""
        self.refine_order(K, terminals)
        return self.__dict__["_refine_classes"][(int(K), bool(terminals))]

    def split(self, t: torch.Tensor) -> List[torch.Tensor]:
        """Per-graph views of a [R, ...] tensor."""
        return [t[int(self.goff_host[g]):int(self.goff_host[g + 1])] for g in range(self.B)]

    def spmm_bytes(self, F: int) -> int:
        """Algorithmic HBM bytes of one F-wide SpMM over this batch."""
        return 2 * self.R * F * 4 + self.nnz * 4 + (self.R + 1) * 4 + 2 * self.R * 4 + F * 4


class Contraction:
    """What ``GraphBatch.contract`` returns, all on the device: ``batch`` (the contracted graphs as an ordinary
    ``GraphBatch``: local nodes 0..K-1 of every graph are the classes' super-nodes), ``node_map`` [R] int32 (the row of
    ``batch`` every original row went to), ``fixed_cut`` [B] float32 (the weight of the edges between pinned nodes of
    different classes), ``pinned`` [R] bool, and ``lift``."""

    def __init__(self, batch: GraphBatch, node_map: torch.Tensor, fixed_cut: torch.Tensor, pinned: torch.Tensor):
        self.batch, self.node_map, self.fixed_cut, self.pinned = batch, node_map, fixed_cut, pinned

    def lift(self, partition: torch.Tensor) -> torch.Tensor:
        """The [R] int32 partition of the original rows a partition of ``batch``'s rows stands for."""
        return partition.to(torch.int32)[self.node_map.to(torch.int64)]

    def contract_cost(self, node_cost: torch.Tensor, goff: torch.Tensor):
        """Per-node class costs [R, K] (float32, on the device) of the original batch, whose graph offsets are ``goff``
        [B + 1] -> (the costs of ``batch`` [R_out, K], ``fixed_cost`` [B] float32): a free row's costs go to its
        contracted row, the K super-nodes of every graph get zero rows, and ``fixed_cost`` is the sum of
        ``node_cost[v][class_v]`` over each graph's pinned rows - a float64 running sum over the rows differenced at the
        graphs' boundaries, without atomics: the same bits every time."""
        K = node_cost.shape[1]
        node_map = self.node_map.to(torch.int64)
        out = torch.zeros((self.batch.R, K), dtype=torch.float32, device=node_cost.device)
        free = ~self.pinned
        out[node_map[free]] = node_cost[free]   # (a free row has a contracted row of its own: no two writes meet)
        B = goff.numel() - 1
        goff = goff.to(torch.int64)
        sizes = goff[1:] - goff[:-1]
        first = torch.repeat_interleave(self.batch.goff.to(torch.int64)[:-1], sizes, output_size=node_map.numel())
        cls = (node_map - first).clamp_(0, K - 1)   # a pinned row's class is its super-node's local id
        picked = node_cost.gather(1, cls.reshape(-1, 1)).reshape(-1).to(torch.float64)
        picked = torch.where(self.pinned, picked, torch.zeros_like(picked))
        run = torch.cat([picked.new_zeros(1), torch.cumsum(picked, 0)])
        return out, (run[goff[1:]] - run[goff[:-1]]).to(torch.float32) if B else picked.new_zeros(0).to(torch.float32)
