"""CPU restatement of the local search of include/gcnmaxcut.h (gmc_refine_order_host / gmc_refine_local_f32),
written from the header's description: first-fit colouring of the movable nodes 3..n-1, sweeps over the colour
classes in increasing colour, per node fp32 class sums in the CSR order of its row, a move to the class of the
smallest sum (lowest index on ties) iff it is strictly smaller than the sum of the node's own class.

``refine`` runs every candidate of a graph at once (numpy over candidates and over the nodes of a class); the
per-position sum ``W += (class == k ? w : 0)`` is the kernel's own fp32 arithmetic, so results are bit for bit.
``sequential_sweep`` is the plain one-node-at-a-time form the parallel one must equal."""
import numpy as np


def colouring(n, rowptr, col):
    """colour[v] for v >= 3 (-1 for 0..2) and the classes as sorted node lists."""
    colour = np.full(n, -1, np.int64)
    for v in range(3, n):
        taken = {int(colour[u]) for u in col[rowptr[v]:rowptr[v + 1]] if 3 <= u < v}
        c = 0
        while c in taken:
            c += 1
        colour[v] = c
    ncol = int(colour.max()) + 1 if n > 3 else 0
    return colour, [np.flatnonzero(colour == c) for c in range(ncol)]


def order_of_batch(handles):
    """What gmc_refine_order_host writes for a batch of GraphHandles: order, cgoff, cptr (trimmed)."""
    order, cgoff, cptr, r0 = [], [], [], 0
    for h in handles:
        _colour, classes = colouring(h.n, h.rowptr, h.col)
        cgoff.append(len(cptr))
        cptr.append(len(order))
        for cls in classes:
            order.extend((cls + r0).tolist())
            cptr.append(len(order))
        r0 += h.n
    cgoff.append(len(cptr))
    return np.asarray(order, np.int32), np.asarray(cgoff, np.int32), np.asarray(cptr, np.int32)


def _class_tables(n, rowptr, col, w, nodes):
    """[m, D] neighbour ids (n = none: self-loops and padding) and fp32 weights of the rows of `nodes`."""
    deg = rowptr[nodes + 1] - rowptr[nodes]
    D = int(deg.max()) if nodes.size else 0
    nb = np.full((nodes.size, D), n, np.int64)
    wt = np.zeros((nodes.size, D), np.float32)
    for i, v in enumerate(nodes):
        a, b = rowptr[v], rowptr[v + 1]
        ids = col[a:b].astype(np.int64)
        nb[i, :b - a] = np.where(ids == v, n, ids)
        wt[i, :b - a] = 1.0 if w is None else w[a:b]
    return nb, wt


def refine(n, rowptr, col, w, assign, max_sweeps, classes=None):
    """assign [cands, n] (int8) -> (refined [cands, n] int8, sweeps [cands]): sweeps run per candidate, the last
    one the sweep that moved nothing when it converged within max_sweeps."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    if classes is None:
        classes = colouring(n, rowptr, col)[1]
    tables = [(cls, *_class_tables(n, rowptr, col, w, cls)) for cls in classes]
    cands = assign.shape[0]
    A = np.full((cands, n + 1), -1, np.int8)       # column n: "no neighbour", a class byte of no class
    A[:, :n] = assign
    sweeps = np.zeros(cands, np.int64)
    active = np.ones(cands, bool)
    inf = np.float32(np.inf)
    for _ in range(max_sweeps):
        if not active.any():
            break
        sweeps[active] += 1
        moved = np.zeros(cands, bool)
        for nodes, nb, wt in tables:
            W = [np.zeros((cands, nodes.size), np.float32) for _k in range(3)]
            for j in range(nb.shape[1]):
                cls = A[:, nb[:, j]]
                for k in range(3):
                    W[k] += np.where(cls == k, wt[:, j], np.float32(0))
            c = A[:, nodes]
            wc = np.where(c == 0, W[0], np.where(c == 1, W[1], np.where(c == 2, W[2], inf)))
            kk = np.zeros(c.shape, np.int8)
            wk = W[0].copy()
            for k in (1, 2):
                better = W[k] < wk
                kk[better] = k
                wk[better] = W[k][better]
            move = wk < wc
            A[:, nodes] = np.where(move, kk, c)
            moved |= move.any(axis=1)
        active &= moved
    return A[:, :n].copy(), sweeps


def sequential_sweep(n, rowptr, col, w, assign):
    """ONE sweep, one node at a time in (colour, id) order, for a single assignment (list) - the definition."""
    a = list(assign)
    _colour, classes = colouring(n, rowptr, col)
    for cls in classes:
        for v in cls:
            W = [np.float32(0)] * 3
            for e in range(rowptr[v], rowptr[v + 1]):
                u = int(col[e])
                if u == v:
                    continue
                if 0 <= a[u] <= 2:
                    W[a[u]] = np.float32(W[a[u]] + np.float32(1.0 if w is None else w[e]))
            c = a[v]
            wc = W[c] if 0 <= c <= 2 else np.float32(np.inf)
            k = min(range(3), key=lambda i: (W[i], i))
            if W[k] < wc:
                a[v] = k
    return a


def cut(rowptr, col, w, assign):
    """float64 cut of one assignment (each undirected edge seen twice in the CSR)."""
    rowptr = np.asarray(rowptr, np.int64)
    a = np.asarray(assign)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    diff = a[rows] != a[np.asarray(col)]
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    return float(ww[diff].sum()) / 2


def best_single_move_gain(n, rowptr, col, w, assign):
    """Largest cut gain of moving one node >= 3 to another class (float64)."""
    best = 0.0
    a = list(assign)
    for v in range(3, n):
        W = [0.0, 0.0, 0.0]
        for e in range(rowptr[v], rowptr[v + 1]):
            u = int(col[e])
            if u != v and 0 <= a[u] <= 2:
                W[a[u]] += 1.0 if w is None else float(w[e])
        best = max(best, W[a[v]] - min(W))
    return best
