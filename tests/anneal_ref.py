"""CPU restatement of the annealing of include/gcnmaxcut.h (gmc_refine_anneal_f32), written from the header's text on
top of tests/refine_ref.py (colouring, class tables, the descent's sweeps).

``anneal`` runs every candidate of a graph at once (numpy over candidates and over the nodes of a class) with the
kernel's own fp32 arithmetic per node; ``sequential`` is the plain one-node-at-a-time form that serves as the
definition.  Cuts are counted in float64 and rounded to fp32 once: for unit, integer and dyadic weights that is the
value any fp32 summation order gives, so snapshot decisions are bit for bit the device's there (and only there)."""
import numpy as np

from tests import refine_ref as RR

LEVELS = 1024
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def levels():
    """The recommended table: quantiles of an exponential variate, float64 rounded once."""
    return (-np.log((np.arange(LEVELS, dtype=np.float64) + 0.5) / LEVELS)).astype(np.float32)


def schedule(sweeps, t_start=1.5, t_end=0.15, scale=1.0):
    """1 / T_s, T_s = scale * t_start * (t_end / t_start) ** (s / max(sweeps - 1, 1)), float64 rounded once."""
    s = np.arange(sweeps, dtype=np.float64)
    return (1.0 / (scale * t_start * (t_end / t_start) ** (s / max(sweeps - 1, 1)))).astype(np.float32)


def mix64_int(z):
    """splitmix64 finaliser on a Python integer."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def level_index(seed, cand, s, v):
    """Index into the level table for node v of candidate cand in sweep s (Python integers)."""
    ctr = (cand << 32) | (s << 12) | v
    return mix64_int(seed + GOLD * (ctr + 1)) >> 54


def _mix64(z):
    u = np.uint64
    with np.errstate(over="ignore"):
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    return z ^ (z >> u(31))


def level_indices(seed, cand_ids, s, nodes):
    """level_index for every (candidate, node): [cands, m] int64."""
    u = np.uint64
    ctr = (np.asarray(cand_ids, np.uint64)[:, None] << u(32)) | u(s << 12) | np.asarray(nodes, np.uint64)[None, :]
    with np.errstate(over="ignore"):
        h = _mix64(u(seed & M64) + u(GOLD) * (ctr + u(1)))
    return (h >> u(54)).astype(np.int64)


def cuts_f32(rowptr, col, w, A):
    """fp32 cut of every row of A [cands, n] (float64 count, rounded once)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    return (((A[:, rows] != A[:, col]) * ww).sum(axis=1) / 2).astype(np.float32)


def anneal(n, rowptr, col, w, assign, inv_temp, table, seed, max_descent_sweeps, cand_ids=None, classes=None):
    """assign [cands, n] int8 -> (annealed [cands, n] int8, snap_sweep [cands], descent sweeps [cands]).
    cand_ids: the candidates' indices in the call (default 0 .. cands-1)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    if classes is None:
        classes = RR.colouring(n, rowptr, col)[1]
    cands = assign.shape[0]
    cand_ids = np.arange(cands) if cand_ids is None else np.asarray(cand_ids)
    tables = [(cls, *RR._class_tables(n, rowptr, col, w, cls)) for cls in classes]
    A = np.full((cands, n + 1), -1, np.int8)       # column n: "no neighbour", a class byte of no class
    A[:, :n] = assign
    best = A.copy()
    snap = np.zeros(cands, np.int64)
    inf = np.float32(np.inf)
    if len(inv_temp):
        best_cut = cuts_f32(rowptr, col, w, A[:, :n])
    for s, inv_t in enumerate(np.asarray(inv_temp, np.float32)):
        for nodes, nb, wt in tables:
            W = np.zeros((3, cands, nodes.size), np.float32)
            for j in range(nb.shape[1]):
                cls = A[:, nb[:, j]]
                for k in range(3):
                    W[k] += np.where(cls == k, wt[:, j], np.float32(0))
            c = A[:, nodes]
            own = np.arange(3)[:, None, None] == c[None]
            others = np.where(own, inf, W)                  # a byte of no class masks nothing: the local search's k
            kk = others.argmin(axis=0)                      # the first smallest: lowest index on ties
            wk = np.take_along_axis(others, kk[None], 0)[0]
            wc = np.where(own, W, np.float32(0)).sum(axis=0, dtype=np.float32)
            wc = np.where(own.any(axis=0), wc, inf)
            delta = wk - wc
            lvl = table[level_indices(seed, cand_ids, s, nodes)]
            move = (delta < 0) | (delta * inv_t <= lvl)
            A[:, nodes] = np.where(move, kk.astype(np.int8), c)
        cs = cuts_f32(rowptr, col, w, A[:, :n])
        better = cs > best_cut
        best[better] = A[better]
        best_cut[better] = cs[better]
        snap[better] = s + 1
    out, sweeps = RR.refine(n, rowptr, col, w, best[:, :n], max_descent_sweeps, classes=classes)
    return out, snap, sweeps


def sequential(n, rowptr, col, w, assign, inv_temp, table, seed, max_descent_sweeps, cand=0):
    """The definition, for a single assignment (list): one node at a time in (colour, id) order.
    Returns (assignment list, snap_sweep, descent sweeps)."""
    f32 = np.float32
    a = list(assign)
    _colour, classes = RR.colouring(n, rowptr, col)
    best, snap = list(a), 0
    if len(inv_temp):
        best_cut = f32(RR.cut(rowptr, col, w, a))
    for s, inv_t in enumerate(inv_temp):
        for cls in classes:
            for v in cls:
                v = int(v)
                W = [f32(0)] * 3
                for e in range(rowptr[v], rowptr[v + 1]):
                    u = int(col[e])
                    if u != v and 0 <= a[u] <= 2:
                        W[a[u]] = f32(W[a[u]] + f32(1.0 if w is None else w[e]))
                c = a[v]
                if 0 <= c <= 2:
                    k = min((i for i in range(3) if i != c), key=lambda i: (W[i], i))
                    delta = f32(W[k] - W[c])
                    if delta < 0 or f32(delta * f32(inv_t)) <= table[level_index(seed, cand, s, v)]:
                        a[v] = k
                else:
                    a[v] = min(range(3), key=lambda i: (W[i], i))
        cs = f32(RR.cut(rowptr, col, w, a))
        if cs > best_cut:
            best, best_cut, snap = list(a), cs, s + 1
    a, sweeps = best, 0
    while sweeps < max_descent_sweeps:
        sweeps += 1
        nxt = RR.sequential_sweep(n, rowptr, col, w, a)
        if nxt == a:
            break
        a = nxt
    return a, snap, sweeps
