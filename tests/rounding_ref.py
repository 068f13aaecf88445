"""CPU restatement of the rounding by conditional expectations of include/gcnmaxcut.h (gmc_round_order_host /
gmc_round_conditional_f32), written from the header's description: nodes 0..K-1 are terminals, the movable nodes K..n-1
are coloured first-fit, every node is visited once in (colour, id) order and takes the class k of the smallest
M_k = sum_e w_e * q_u[k] (product and sum separate float32 operations, CSR order, self-loops skipped, lowest index on
ties), then the local search's sweeps at K classes.

``round_sequential`` is the one-node-at-a-time definition, ``round_by_classes`` the class-parallel form the kernel
runs (all nodes of a class from the state at the start of the colour step); ``expected_cut`` is float64.  ``cases()``
is the list of (K, graph, weights, P) the CPU and GPU tests share."""
import functools

import networkx as nx
import numpy as np

F32 = np.float32


def colouring(n, rowptr, col, K):
    """colour[v] for v >= K (-1 for the terminals) and the classes as sorted node arrays."""
    colour = np.full(n, -1, np.int64)
    for v in range(K, n):
        taken = {int(colour[u]) for u in col[rowptr[v]:rowptr[v + 1]] if K <= u < v}
        c = 0
        while c in taken:
            c += 1
        colour[v] = c
    ncol = int(colour.max()) + 1 if n > K else 0
    return colour, [np.flatnonzero(colour == c) for c in range(ncol)]


def order_of_batch(handles, K):
    """What gmc_round_order_host writes for a batch of GraphHandles: order, cgoff, cptr (trimmed)."""
    order, cgoff, cptr, r0 = [], [], [], 0
    for h in handles:
        _colour, classes = colouring(h.n, h.rowptr, h.col, K)
        cgoff.append(len(cptr))
        cptr.append(len(order))
        for cls in classes:
            order.extend((cls + r0).tolist())
            cptr.append(len(order))
        r0 += h.n
    cgoff.append(len(cptr))
    return np.asarray(order, np.int32), np.asarray(cgoff, np.int32), np.asarray(cptr, np.int32)


def initial_state(P, K):
    """q [n, K] float32: terminals e_u (their rows of P are not read), every other node its row of P."""
    q = np.array(P, dtype=F32, copy=True)
    q[:K] = np.eye(K, dtype=F32)
    return q


def state_sums(rowptr, col, w, q, v):
    """M [K] of node v over the state q: per edge one float32 product and one float32 sum, from +0."""
    M = np.zeros(q.shape[1], F32)
    for e in range(rowptr[v], rowptr[v + 1]):
        u = int(col[e])
        if u == v:
            continue
        t = (F32(1.0) if w is None else F32(w[e])) * q[u]      # float32 product, rounded
        M = M + t                                              # float32 sum, rounded
    return M


def round_sequential(n, rowptr, col, w, P, K):
    """The definition: one node at a time in (colour, id) order.  Returns the class bytes (int8)."""
    q = initial_state(P, K)
    a = np.zeros(n, np.int8)
    a[:K] = np.arange(K)
    for cls in colouring(n, rowptr, col, K)[1]:
        for v in cls:
            kk = int(np.argmin(state_sums(rowptr, col, w, q, v)))   # first of the smallest
            q[v] = np.eye(K, dtype=F32)[kk]
            a[v] = kk
    return a


def round_by_classes(n, rowptr, col, w, P, K):
    """The class-parallel form: every node of a colour class decides from the state at the start of its colour step."""
    q = initial_state(P, K)
    a = np.zeros(n, np.int8)
    a[:K] = np.arange(K)
    for cls in colouring(n, rowptr, col, K)[1]:
        frozen = q.copy()
        picks = [int(np.argmin(state_sums(rowptr, col, w, frozen, v))) for v in cls]
        for v, kk in zip(cls, picks):
            q[v] = np.eye(K, dtype=F32)[kk]
            a[v] = kk
    return a


def descent(n, rowptr, col, w, assign, K, max_sweeps):
    """The local search's sweeps at K classes from `assign`: (class bytes, sweeps run), one node at a time in
    (colour, id) order; a sweep that moves nothing is the last and is counted."""
    a = np.array(assign, np.int8, copy=True)
    classes = colouring(n, rowptr, col, K)[1]
    sweeps = 0
    while sweeps < max_sweeps:
        sweeps += 1
        moved = False
        for cls in classes:
            for v in cls:
                M = np.zeros(K, F32)
                for e in range(rowptr[v], rowptr[v + 1]):
                    u = int(col[e])
                    if u != v:
                        M[a[u]] = M[a[u]] + (F32(1.0) if w is None else F32(w[e]))
                kk = int(np.argmin(M))
                if M[kk] < M[a[v]]:
                    a[v] = kk
                    moved = True
        if not moved:
            break
    return a, sweeps


def round_and_descend(n, rowptr, col, w, P, K, max_sweeps):
    return descent(n, rowptr, col, w, round_sequential(n, rowptr, col, w, P, K), K, max_sweeps)


def expected_cut(n, rowptr, col, w, P, K):
    """float64: 1/2 * sum_v sum_{e in row v, u != v} w_e * (1 - q_u . q_v) over the initial state."""
    q = initial_state(P, K).astype(np.float64)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rowptr, np.int64)))
    cols = np.asarray(col, np.int64)
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    keep = rows != cols
    dots = np.einsum("ek,ek->e", q[rows[keep]], q[cols[keep]])
    return float((ww[keep] * (1.0 - dots)).sum()) / 2


def cut(rowptr, col, w, assign):
    """float64 cut of one assignment (each undirected edge seen twice in the CSR)."""
    rowptr = np.asarray(rowptr, np.int64)
    a = np.asarray(assign)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    diff = a[rows] != a[np.asarray(col)]
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    return float(ww[diff].sum()) / 2


def abs_weight(rowptr, col, w):
    """W_abs: the absolute edge weight of the graph, every undirected edge once (self-loops not counted)."""
    rowptr = np.asarray(rowptr, np.int64)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    keep = rows != np.asarray(col)
    ww = np.ones(rows.size) if w is None else np.abs(np.asarray(w, np.float64))
    return float(ww[keep].sum()) / 2


def argmax_assignment(P, K):
    a = np.argmax(np.asarray(P)[:, :K], axis=1).astype(np.int8)
    a[:K] = np.arange(K)
    return a


def softmax_rows(n, K, seed, scale=2.0):
    """softmax of normal logits scaled by `scale` (at most 2), as float32"""
    rng = np.random.RandomState(seed)
    logits = rng.standard_normal((n, K)) * scale
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(F32)


def signed_weights(g, seed):
    """real-valued weights of both signs on the edges of g: magnitudes in [0.1, 2), about a third negative"""
    rng = np.random.RandomState(seed)
    for u, v in g.edges():
        mag = float(F32(rng.uniform(0.1, 2.0)))
        g[u][v]["weight"] = -mag if rng.rand() < 0.35 else mag
    return g


def connected_gnp(n, p, seed):
    g = nx.gnp_random_graph(n, p, seed=seed)
    for v in range(n):                       # no isolated node
        if g.degree(v) == 0:
            g.add_edge(v, (v + 1) % n)
    return g


CASE_KS = (2, 3, 4, 8)


@functools.lru_cache(maxsize=None)
def cases():
    """48 cases (K, n, rowptr, col, w, P): K in 2, 3, 4, 8; six graphs of 60..100 nodes each (regular of degree 3..8 and
    G(n, p)); unit weights and signed real-valued weights.  P: softmax rows, every row (terminals too: the rounding
    must not read them)."""
    from gcn_max_cut_amd.graph import from_networkx
    out = []
    for K in CASE_KS:
        for i in range(6):
            n = 60 + 8 * i
            seed = 1000 * K + i
            for signed in (False, True):
                g = connected_gnp(n, 0.08, seed) if i % 3 == 2 else nx.random_regular_graph(3 + i, n, seed=seed)
                if signed:
                    signed_weights(g, seed + 500)
                h = from_networkx(g)
                P = softmax_rows(n, K, seed + 7, scale=(0.5, 1.0, 2.0)[i % 3])
                out.append((K, h.n, h.rowptr, h.col, h.weight, P))
    return tuple(out)


def check_case_inputs(K, n, rowptr, col, w, P):
    """What the restatement relies on: no entry of P and no product w * P is small enough for a tie to hinge on how
    denormals are flushed."""
    assert P.dtype == F32 and P.shape == (n, K)
    assert float(P.min()) >= 1e-10
    wmin = 1.0 if w is None else float(np.abs(w).min())
    assert wmin * float(P.min()) >= 1e-30
