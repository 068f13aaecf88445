"""CPU restatement of the K-class decoders of include/gcnmaxcut.h (gmc_kway_decode_sample_seeded_f32 and
gmc_kway_refine_anneal_f32), written from the header's text on top of tests/seeded_ref.py (keys, hashes, uniforms),
tests/anneal_ref.py (level indices, the fp32 cut, levels and schedule), tests/refine_ref.py (class tables, the float64
cut) and tests/rounding_ref.py (the colouring with terminals 0..K-1).

Sampler: ``assignments`` / ``sample``, K taken from the columns of P.  Search: ``refine`` (the local search's sweeps at
K classes) and ``anneal`` run every candidate of a graph at once (numpy over candidates and over the nodes of a class)
with the kernel's own fp32 arithmetic per node; ``sequential`` is the plain one-node-at-a-time form that serves as the
definition.  Cuts are counted in float64 and rounded to fp32 once: for unit, integer and dyadic weights that is the
value any fp32 summation order gives, so snapshot decisions are bit for bit the device's there (and only there)."""
import numpy as np

from tests import anneal_ref as AR
from tests import refine_ref as RR
from tests import rounding_ref as RO
from tests import seeded_ref as SR

F32 = np.float32
INF = F32(np.inf)


# ---- the sampler ------------------------------------------------------------------------------------------------------
def assignments(P, key, iters, first_iter=0):
    """P [n, K] float32 -> [iters, n] int8: nodes 0..K-1 fixed; node l >= K takes the first class j in 0..K-2 with
    u < c_j (c_j the running double sum of its row), else K-1 - no compare against c_{K-1}."""
    P = np.asarray(P)
    assert P.dtype == np.float32 and P.ndim == 2
    n, K = P.shape
    u = SR.uniforms(key, iters, n, first_iter)
    a = np.full((iters, n), K - 1, np.int8)
    open_ = np.ones((iters, n), bool)
    c = None
    with np.errstate(invalid="ignore"):
        for j in range(K - 1):
            pj = P[:, j].astype(np.float64)
            c = pj if c is None else c + pj
            take = open_ & (u < c[None, :])
            a[take] = j
            open_ &= ~take
    m = min(n, K)
    a[:, :m] = np.arange(m, dtype=np.int8)
    return a


def sample(handle, P, key, iters):
    """What the entry point reports for one graph: assign_all [iters, n] int8, cut_all [iters] float32, best_assign
    [n] int32, best_cut (float32), best_iter."""
    a = assignments(P, key, iters)
    cuts = np.array([RR.cut(handle.rowptr, handle.col, handle.weight, row) for row in a])
    cut_all = cuts.astype(np.float32)
    assert (cut_all.astype(np.float64) == cuts).all()       # the cases the tests use have exactly representable cuts
    bi = int(np.argmax(cut_all))                            # the first of the largest
    return dict(assign_all=a, cut_all=cut_all, best_assign=a[bi].astype(np.int32), best_cut=cut_all[bi], best_iter=bi)


# ---- the search -------------------------------------------------------------------------------------------------------
def classes_of(n, rowptr, col, K):
    """The colour classes of the movable nodes K..n-1 as sorted node arrays (gmc_round_order_host)."""
    return RO.colouring(n, np.asarray(rowptr, np.int64), np.asarray(col, np.int64), K)[1]


def _sums(A, nb, wt, K):
    """W [K, cands, m]: per position of the row one fp32 add of the weight to the sum of the neighbour's class."""
    W = np.zeros((K, A.shape[0], nb.shape[0]), F32)
    for j in range(nb.shape[1]):
        cls = A[:, nb[:, j]]
        for k in range(K):
            W[k] += np.where(cls == k, wt[:, j], F32(0))
    return W


def _own(W, c, K):
    """(own [K, cands, m] bool, wc [cands, m]): the sum of the node's own class, +inf for a byte of no class."""
    own = np.arange(K)[:, None, None] == c[None]
    wc = np.where(own, W, F32(0)).sum(axis=0, dtype=F32)
    return own, np.where(own.any(axis=0), wc, INF)


def _padded(assign, n):
    A = np.full((assign.shape[0], n + 1), -1, np.int8)      # column n: "no neighbour", a class byte of no class
    A[:, :n] = assign
    return A


def refine(n, rowptr, col, w, assign, K, max_sweeps, classes=None):
    """The local search at K classes: assign [cands, n] int8 -> (refined [cands, n] int8, sweeps [cands])."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    if classes is None:
        classes = classes_of(n, rowptr, col, K)
    tables = [(cls, *RR._class_tables(n, rowptr, col, w, cls)) for cls in classes]
    cands = assign.shape[0]
    A = _padded(assign, n)
    sweeps = np.zeros(cands, np.int64)
    active = np.ones(cands, bool)
    for _ in range(max_sweeps):
        if not active.any():
            break
        sweeps[active] += 1
        moved = np.zeros(cands, bool)
        for nodes, nb, wt in tables:
            W = _sums(A, nb, wt, K)
            c = A[:, nodes]
            _own_mask, wc = _own(W, c, K)
            kk = W.argmin(axis=0)                            # the first smallest: lowest index on ties
            wk = np.take_along_axis(W, kk[None], 0)[0]
            move = wk < wc
            A[:, nodes] = np.where(move, kk.astype(np.int8), c)
            moved |= move.any(axis=1)
        active &= moved
    return A[:, :n].copy(), sweeps


def anneal(n, rowptr, col, w, assign, K, inv_temp, table, seed, max_descent_sweeps, cand_ids=None):
    """assign [cands, n] int8 -> (annealed [cands, n] int8, snap_sweep [cands], descent sweeps [cands])."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    classes = classes_of(n, rowptr, col, K)
    cands = assign.shape[0]
    cand_ids = np.arange(cands) if cand_ids is None else np.asarray(cand_ids)
    tables = [(cls, *RR._class_tables(n, rowptr, col, w, cls)) for cls in classes]
    A = _padded(assign, n)
    best = A.copy()
    snap = np.zeros(cands, np.int64)
    if len(inv_temp):
        best_cut = AR.cuts_f32(rowptr, col, w, A[:, :n])
    for s, inv_t in enumerate(np.asarray(inv_temp, F32)):
        for nodes, nb, wt in tables:
            W = _sums(A, nb, wt, K)
            c = A[:, nodes]
            own, wc = _own(W, c, K)
            others = np.where(own, INF, W)                   # a byte of no class masks nothing: the smallest of all
            kk = others.argmin(axis=0)
            wk = np.take_along_axis(others, kk[None], 0)[0]
            delta = wk - wc
            lvl = table[AR.level_indices(seed, cand_ids, s, nodes)]
            move = (delta < 0) | (delta * inv_t <= lvl)
            A[:, nodes] = np.where(move, kk.astype(np.int8), c)
        cs = AR.cuts_f32(rowptr, col, w, A[:, :n])
        better = cs > best_cut
        best[better] = A[better]
        best_cut[better] = cs[better]
        snap[better] = s + 1
    out, sweeps = refine(n, rowptr, col, w, best[:, :n], K, max_descent_sweeps, classes=classes)
    return out, snap, sweeps


def _node_sums(rowptr, col, w, a, v, K):
    W = [F32(0)] * K
    for e in range(rowptr[v], rowptr[v + 1]):
        u = int(col[e])
        if u != v and 0 <= a[u] < K:
            W[a[u]] = F32(W[a[u]] + F32(1.0 if w is None else w[e]))
    return W


def sequential_sweep(n, rowptr, col, w, assign, K, classes=None):
    """ONE sweep of the local search at K classes, one node at a time in (colour, id) order (a list in, a list out)."""
    a = list(assign)
    for cls in classes_of(n, rowptr, col, K) if classes is None else classes:
        for v in cls:
            v = int(v)
            W = _node_sums(rowptr, col, w, a, v, K)
            wc = W[a[v]] if 0 <= a[v] < K else INF
            k = min(range(K), key=lambda i: (W[i], i))
            if W[k] < wc:
                a[v] = k
    return a


def sequential(n, rowptr, col, w, assign, K, inv_temp, table, seed, max_descent_sweeps, cand=0):
    """The definition, for a single assignment (list): one node at a time in (colour, id) order.
    Returns (assignment list, snap_sweep, descent sweeps)."""
    a = [int(x) for x in assign]
    classes = classes_of(n, rowptr, col, K)
    best, snap = list(a), 0
    if len(inv_temp):
        best_cut = F32(RR.cut(rowptr, col, w, a))
    for s, inv_t in enumerate(inv_temp):
        for cls in classes:
            for v in cls:
                v = int(v)
                W = _node_sums(rowptr, col, w, a, v, K)
                c = a[v]
                if 0 <= c < K:
                    k = min((i for i in range(K) if i != c), key=lambda i: (W[i], i))
                    delta = F32(W[k] - W[c])
                    if delta < 0 or F32(delta * F32(inv_t)) <= table[AR.level_index(seed, cand, s, v)]:
                        a[v] = k
                else:
                    a[v] = min(range(K), key=lambda i: (W[i], i))
        cs = F32(RR.cut(rowptr, col, w, a))
        if cs > best_cut:
            best, best_cut, snap = list(a), cs, s + 1
    a, sweeps = best, 0
    while sweeps < max_descent_sweeps:
        sweeps += 1
        nxt = sequential_sweep(n, rowptr, col, w, a, K, classes)
        if nxt == a:
            break
        a = nxt
    return a, snap, sweeps


def best_single_move_gain(n, rowptr, col, w, assign, K):
    """Largest cut gain of moving one node >= K to another class (float64)."""
    best = 0.0
    a = list(assign)
    for v in range(K, n):
        W = [0.0] * K
        for e in range(rowptr[v], rowptr[v + 1]):
            u = int(col[e])
            if u != v and 0 <= a[u] < K:
                W[a[u]] += 1.0 if w is None else float(w[e])
        best = max(best, W[a[v]] - min(W))
    return best
