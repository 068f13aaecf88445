"""CPU restatement of the rounding and the K-class local search for graphs of up to 2^20 nodes (include/gcnmaxcut.h:
gmc_large_round_order_host, gmc_large_round_conditional_f32, gmc_large_local_search_f32), and the cases of their tests.

The rule is that of tests/rounding_ref.py (``round_sequential``, ``descent``) and tests/kway_search_ref.py (``refine``);
those walk one node at a time in Python, which a million nodes do not allow.  Here all nodes of a colour class are taken
at once from the state at the start of the colour step - the class-parallel form, equal to the sequential one because
no two nodes of a class are adjacent - through padded neighbour tables and a loop over the edge POSITION, the form of
``kway_search_ref._sums``: position j of every row is added before position j + 1 of any, so each row's float32 sum is
taken in CSR order, product and sum separate float32 operations.  A class is split by degree (rows of more than 64
entries get a table of their own) so that one hub does not pad a whole class to its length; that changes no result.

The state is what the device keeps: a class value per node, UNROUNDED for a movable node not visited yet (its state row
is its row of P), NONE for the padding column.  A rounded neighbour adds w * 1 = w to its class and w * 0 = +-0 to the
others, which leaves a sum as it is, exactly as the header's q does.

Graphs are numpy CSR (tests/large_ref.py's builders: circulants, a star, a ring with a hub); inputs keep every
P >= 1e-10 and every |w * P| >= 1e-30 (``check_inputs``), so no tie hinges on how denormals are flushed and no row is
ever excused from a comparison."""
import functools

import numpy as np

from tests import large_ref as LR
from tests import rounding_ref as CR

F32 = np.float32
UNROUNDED = -1
NONE = -2
LONG_ROW = 64


# ---- colouring ----------------------------------------------------------------------------------------------------------
def colouring(n, rowptr, col, K):
    """First-fit colours of the movable nodes K..n-1 against their movable neighbours of smaller id (rounding_ref's
    ``colouring`` on plain lists: a million nodes in seconds).  Returns the classes as sorted int64 arrays."""
    rp = np.asarray(rowptr).tolist()
    cl = np.asarray(col).tolist()
    colour = [-1] * n
    for v in range(K, n):
        taken = {colour[u] for u in cl[rp[v]:rp[v + 1]] if K <= u < v}
        c = 0
        while c in taken:
            c += 1
        colour[v] = c
    colour = np.asarray(colour, np.int64)
    ncol = int(colour.max()) + 1 if n > K else 0
    order = np.argsort(colour, kind="stable")
    counts = np.bincount(colour[colour >= 0], minlength=ncol)
    starts = np.concatenate([[0], np.cumsum(counts)]) + int((colour < 0).sum())
    return [order[starts[c]:starts[c + 1]] for c in range(ncol)]


def order_arrays(graphs, K):
    """What gmc_large_round_order_host writes for a batch of (n, rowptr, col) graphs: order, cgoff, cptr (trimmed) and
    max_classes."""
    order, cgoff, cptr, r0, most = [], [], [], 0, 0
    for n, rowptr, col in graphs:
        classes = colouring(n, rowptr, col, K)
        most = max(most, len(classes))
        cgoff.append(len(cptr))
        cptr.append(len(order))
        for cls in classes:
            order.extend((cls + r0).tolist())
            cptr.append(len(order))
        r0 += n
    cgoff.append(len(cptr))
    return np.asarray(order, np.int32), np.asarray(cgoff, np.int32), np.asarray(cptr, np.int32), most


def classes_from_order(order, cgoff, cptr, g=0, r0=0):
    """The classes of graph g out of the arrays the host routine wrote (local ids)."""
    k0, k1 = int(cgoff[g]), int(cgoff[g + 1]) - 1
    return [np.asarray(order[cptr[k]:cptr[k + 1]], np.int64) - r0 for k in range(k0, k1)]


# ---- tables -------------------------------------------------------------------------------------------------------------
def _table(n, rowptr, col, w, nodes):
    """[m, D] neighbour ids (n: padding) and float32 weights of the rows of `nodes`; a self-loop keeps its place with
    the id n, so it adds to no sum."""
    deg = rowptr[nodes + 1] - rowptr[nodes]
    D = int(deg.max()) if nodes.size else 0
    pos = np.arange(D, dtype=np.int64)[None, :]
    live = pos < deg[:, None]
    idx = np.where(live, rowptr[nodes][:, None] + pos, 0)
    ids = col[idx]
    nb = np.where(live & (ids != nodes[:, None]), ids, n)
    wt = live.astype(F32) if w is None else np.where(live, w[idx], F32(0)).astype(F32)
    return nb, wt


def class_tables(n, rowptr, col, w, classes):
    """Per class a list of (nodes, nb, wt): the short rows together, every row of more than LONG_ROW entries alone."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    w = None if w is None else np.asarray(w, F32)
    out = []
    for cls in classes:
        deg = rowptr[cls + 1] - rowptr[cls]
        groups = [cls[deg <= LONG_ROW]] + [cls[i:i + 1] for i in np.flatnonzero(deg > LONG_ROW)]
        out.append([(nodes, *_table(n, rowptr, col, w, nodes)) for nodes in groups if nodes.size])
    return out


# ---- the rule -----------------------------------------------------------------------------------------------------------
def _state_sums(state, Pext, nb, wt, K):
    """M [m, K]: per edge position one float32 product and one float32 sum over the state rows of the neighbours."""
    M = np.zeros((nb.shape[0], K), F32)
    ks = np.arange(K)[None, :]
    for j in range(nb.shape[1]):
        u = nb[:, j]
        c = state[u][:, None]
        q = np.where(c == UNROUNDED, Pext[u], (c == ks).astype(F32))
        t = wt[:, j:j + 1] * q                                         # float32 product, rounded
        M = M + t                                                      # float32 sum, rounded
    return M


def _class_sums(state, nb, wt, K):
    """W [m, K]: per edge position one float32 add of the weight to the sum of the neighbour's class."""
    W = np.zeros((nb.shape[0], K), F32)
    ks = np.arange(K)[None, :]
    for j in range(nb.shape[1]):
        c = state[nb[:, j]][:, None]
        W = W + np.where(c == ks, wt[:, j:j + 1], F32(0))
    return W


def round_by_classes(n, P, K, tables):
    """The rounding: class values (int8) of one visit of every movable node, colour class by colour class."""
    state = np.full(n + 1, UNROUNDED, np.int64)
    state[:K] = np.arange(K)
    state[n] = NONE
    Pext = np.zeros((n + 1, K), F32)
    Pext[K:n] = np.asarray(P, F32)[K:]                                 # the terminals' rows are never read
    for groups in tables:
        picks = [_state_sums(state, Pext, nb, wt, K).argmin(axis=1) for _nodes, nb, wt in groups]
        for (nodes, _nb, _wt), kk in zip(groups, picks):               # all of a class decide from the state before it
            state[nodes] = kk
    return state[:n].astype(np.int8)


def descent(n, assign, K, tables, max_sweeps):
    """The local search's sweeps at K classes: (class values int8, sweeps run); a value outside 0..K-1 on a movable
    node counts for no class and always moves; a sweep that moves nothing is the last and is counted."""
    state = np.full(n + 1, NONE, np.int64)
    state[:n] = np.asarray(assign, np.int8)
    sweeps = 0
    while sweeps < max_sweeps:
        sweeps += 1
        moved = False
        for groups in tables:
            new = []
            for nodes, nb, wt in groups:
                W = _class_sums(state, nb, wt, K)
                c = state[nodes]
                own = (c >= 0) & (c < K)
                wc = np.where(own, W[np.arange(nodes.size), np.clip(c, 0, K - 1)], F32(np.inf))
                kk = W.argmin(axis=1)                                  # the first smallest: lowest index on ties
                move = W[np.arange(nodes.size), kk] < wc
                new.append(np.where(move, kk, c))
                moved |= bool(move.any())
            for (nodes, _nb, _wt), vals in zip(groups, new):
                state[nodes] = vals
        if not moved:
            break
    return state[:n].astype(np.int8), sweeps


def best_single_move_gain(n, rowptr, col, w, assign, K):
    """kway_search_ref.best_single_move_gain in numpy (float64): the largest cut gain of moving one node >= K."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    a = np.asarray(assign, np.int64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    keep = (rows != col) & (a[col] >= 0) & (a[col] < K)
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    W = np.zeros((n, K))
    np.add.at(W, (rows[keep], a[col[keep]]), ww[keep])
    gain = W[np.arange(n), a] - W.min(axis=1)
    return float(gain[K:].max()) if n > K else 0.0


# ---- cases --------------------------------------------------------------------------------------------------------------
def signed_edge_weights(n, rowptr, col, seed):
    """float32 weights of both signs, one per undirected edge in CSR order (both directions the same value): magnitudes
    in [0.1, 2), about a third negative - rounding_ref.signed_weights for a numpy CSR."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    key = np.minimum(rows, col) * n + np.maximum(rows, col)
    uniq, inv = np.unique(key, return_inverse=True)
    rng = np.random.RandomState(300 + seed)
    mag = rng.uniform(0.1, 2.0, uniq.size).astype(F32)
    return np.where(rng.rand(uniq.size) < 0.35, -mag, mag).astype(F32)[inv]


def hubring(n, hub):
    """A ring of n nodes plus an edge from `hub` to every other node."""
    return LR.with_hub(*LR.circulant(n, 2), hub)


def softmax_rows(n, K, seed, scale=1.0):
    """rounding_ref.softmax_rows with the draws made in float32 blocks (2^20 rows in a fraction of a second)."""
    rng = np.random.RandomState(seed)
    logits = rng.standard_normal((n, K)).astype(F32) * F32(scale)
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(F32)


# name -> (K, graph spec, weights, max sweeps of the run "with a descent")
BIG_CASES = {
    "n4097_K2": (2, ("circ", 4097, 7, 6), "signed", 100),
    "n4097_K8": (8, ("circ", 4097, 7, 6), "unit", 100),
    "n5000_K3": (3, ("circ", 5000, 7, 7), "signed", 100),
    "star4200": (3, ("star", 4200, 5), "unit", 100),
    "hubring4200": (4, ("hubring", 4201, 9), "signed", 100),
    "n70000": (4, ("circ", 70000, 7, None), "unit", 100),
    "n2^20": (3, ("circ", 1 << 20, 4, None), "unit", 3),
}


def build_graph(spec):
    """(n, rowptr int64, col int64) of a graph spec: ("circ", n, d, chord seed or None), ("star", leaves, hub),
    ("hubring", n, hub)."""
    if spec[0] == "circ":
        return LR.circulant(spec[1], spec[2], spec[3])
    if spec[0] == "star":
        return LR.star(spec[1], spec[2])
    return hubring(spec[1], spec[2])


def check_inputs(K, n, rowptr, col, w, P):
    CR.check_case_inputs(K, n, rowptr, col, w, P)


@functools.lru_cache(maxsize=None)
def big_case(name):
    """(K, n, rowptr, col, w, P, max_sweeps) of a case beyond 4096 nodes; P has every row drawn, terminals included."""
    K, spec, weights, max_sweeps = BIG_CASES[name]
    n, rowptr, col = build_graph(spec)
    seed = sum(map(ord, name))
    w = signed_edge_weights(n, rowptr, col, seed) if weights == "signed" else None
    P = softmax_rows(n, K, seed + 1)
    check_inputs(K, n, rowptr, col, w, P)
    return K, n, rowptr, col, w, P, max_sweeps


def restate(n, rowptr, col, w, P, K, max_sweeps, classes=None):
    """The rounding and the descent from it: dict of a0 (rounded), a1 / sweeps (after up to max_sweeps sweeps)."""
    if classes is None:
        classes = colouring(n, rowptr, col, K)
    tables = class_tables(n, rowptr, col, w, classes)
    a0 = round_by_classes(n, P, K, tables)
    a1, sweeps = descent(n, a0, K, tables, max_sweeps)
    return dict(a0=a0, a1=a1, sweeps=sweeps)
