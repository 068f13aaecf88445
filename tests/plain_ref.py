"""CPU restatement of the decoders with the terminals optional (include/gcnmaxcut.h, "plain max-K-cut": gmc_order_host_t
and the ``_t`` entry points), written from the header's text with the first movable local id as an argument:
``first = K`` is the problem with terminals 0..K-1, ``first = 0`` the one without.

Everything that depends on ``first`` is stated here - the colouring and the (colour, id) order, the rounding's initial
state and its visit of every movable node, the descent, the draw rule, the annealing with its counters (the wide one of
graphs beyond 4096 nodes included), the expected cut and the best single move.  What does not know about terminals is
taken from the existing restatements: the padded neighbour tables (large_round_ref.class_tables), the per-position fp32
class sums (kway_search_ref._sums / _own), the hashes (seeded_ref.uniforms, large_search_ref.level_indices) and the fp32
cut (anneal_ref.cuts_f32).  With ``first = K`` every function equals rounding_ref / kway_search_ref / large_round_ref /
large_search_ref output for output (tests/test_plain_maxcut_host.py)."""
import collections

import numpy as np

from tests import anneal_ref as AR
from tests import functional_ref as FR
from tests import kway_ref as KR
from tests import kway_search_ref as KS
from tests import large_round_ref as LRR
from tests import large_search_ref as LS
from tests import seeded_ref as SR

F32 = np.float32
INF = F32(np.inf)
UNROUNDED = -1
NONE = -2


def first_of(K, terminals):
    return K if terminals else 0


# ---- colouring and order ------------------------------------------------------------------------------------------------
def colouring(n, rowptr, col, first):
    """First-fit colours of the movable nodes first..n-1 against their movable neighbours of smaller id; the classes
    as sorted int64 arrays."""
    rp = np.asarray(rowptr).tolist()
    cl = np.asarray(col).tolist()
    colour = [-1] * n
    for v in range(first, n):
        taken = {colour[u] for u in cl[rp[v]:rp[v + 1]] if first <= u < v}
        c = 0
        while c in taken:
            c += 1
        colour[v] = c
    colour = np.asarray(colour, np.int64)
    ncol = int(colour.max()) + 1 if n > first else 0
    return [np.flatnonzero(colour == c).astype(np.int64) for c in range(ncol)]


def order_arrays(graphs, first):
    """What gmc_order_host_t writes for a batch of (n, rowptr, col) graphs: order (R - first * B entries), cgoff, cptr
    (trimmed) and max_classes."""
    order, cgoff, cptr, r0, most = [], [], [], 0, 0
    for n, rowptr, col in graphs:
        classes = colouring(n, rowptr, col, first)
        most = max(most, len(classes))
        cgoff.append(len(cptr))
        cptr.append(len(order))
        for cls in classes:
            order.extend((cls + r0).tolist())
            cptr.append(len(order))
        r0 += n
    cgoff.append(len(cptr))
    return np.asarray(order, np.int32), np.asarray(cgoff, np.int32), np.asarray(cptr, np.int32), most


def tables_of(n, rowptr, col, w, first):
    return LRR.class_tables(n, rowptr, col, w, colouring(n, rowptr, col, first))


# ---- rounding and descent -----------------------------------------------------------------------------------------------
def _state_sums(state, Pext, nb, wt, K):
    """M [m, K]: per edge position one float32 product and one float32 sum over the state rows of the neighbours."""
    M = np.zeros((nb.shape[0], K), F32)
    ks = np.arange(K)[None, :]
    for j in range(nb.shape[1]):
        u = nb[:, j]
        c = state[u][:, None]
        q = np.where(c == UNROUNDED, Pext[u], (c == ks).astype(F32))
        M = M + wt[:, j:j + 1] * q
    return M


def round_conditional(n, P, K, first, tables):
    """Step 1 and the one visit of every movable node: nodes below `first` start as e_l (their rows of P are not read),
    every other node as its row of P; class by class every node takes the class of its smallest M (lowest index)."""
    state = np.full(n + 1, UNROUNDED, np.int64)
    state[:min(first, n)] = np.arange(min(first, n))
    state[n] = NONE
    Pext = np.zeros((n + 1, K), F32)
    Pext[first:n] = np.asarray(P, F32)[first:n]
    for groups in tables:
        picks = [_state_sums(state, Pext, nb, wt, K).argmin(axis=1) for _nodes, nb, wt in groups]
        for (nodes, _nb, _wt), kk in zip(groups, picks):
            state[nodes] = kk
    out = state[:n].copy()
    out[out == UNROUNDED] = 0           # (none: every node is a terminal or is visited)
    return out.astype(np.int8)


def descent(n, assign, K, tables, max_sweeps):
    """The local search's sweeps over the classes of `tables` (the movable nodes): assign [cands, n] int8 ->
    (refined [cands, n] int8, sweeps [cands]); a byte outside 0..K-1 on a movable node always moves."""
    A = KS._padded(np.asarray(assign, np.int8), n)
    groups = [grp for cls in tables for grp in cls]
    sweeps = LS.descent(A, groups, K, max_sweeps)
    return A[:, :n].copy(), sweeps


def restate_round(n, rowptr, col, w, P, K, first, max_sweeps):
    """dict of a0 (rounded), a1 / sweeps (after up to max_sweeps sweeps of the descent)."""
    tables = tables_of(n, rowptr, col, w, first)
    a0 = round_conditional(n, P, K, first, tables)
    a1, sweeps = descent(n, a0[None], K, tables, max_sweeps)
    return dict(a0=a0, a1=a1[0], sweeps=int(sweeps[0]))


def expected_cut(n, rowptr, col, w, P, K, first):
    """float64: 1/2 * sum_v sum_{e in row v, u != v} w_e * (1 - q_u . q_v) over the initial state."""
    q = np.array(P, np.float64, copy=True)
    m = min(first, n)
    q[:m] = np.eye(K)[:m]
    rowptr = np.asarray(rowptr, np.int64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    cols = np.asarray(col, np.int64)
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    keep = rows != cols
    dots = np.einsum("ek,ek->e", q[rows[keep]], q[cols[keep]])
    return float((ww[keep] * (1.0 - dots)).sum()) / 2


# ---- the sampler --------------------------------------------------------------------------------------------------------
def assignments(P, key, iters, first):
    """P [n, K] float32 -> [iters, n] int8: local ids below `first` keep their own id; node l >= first takes the first
    class j in 0..K-2 with u < c_j (c_j the running double sum of its row, u hashed from (iteration, l)), else K-1."""
    P = np.asarray(P)
    assert P.dtype == np.float32 and P.ndim == 2
    n, K = P.shape
    u = SR.uniforms(key, iters, n)
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
    m = min(n, first)
    a[:, :m] = np.arange(m, dtype=np.int8)
    return a


def sample(n, rowptr, col, w, P, key, iters, first):
    """What the sampler reports for one graph (cuts must be exactly representable: unit / integer weights)."""
    a = assignments(np.asarray(P, F32)[:n], key, iters, first)
    cut_all = AR.cuts_f32(np.asarray(rowptr, np.int64), np.asarray(col, np.int64), w, a)
    bi = int(np.argmax(cut_all))
    return dict(assign_all=a, cut_all=cut_all, best_assign=a[bi].astype(np.int32), best_cut=cut_all[bi], best_iter=bi)


# ---- annealing ----------------------------------------------------------------------------------------------------------
def anneal(n, rowptr, col, w, assign, K, first, inv_temp, table, seed, max_descent_sweeps, wide_layout=False,
           tables=None):
    """assign [cands, n] int8 -> dict as `search` of large_search_ref: every node >= first is movable; the counter is
    cand << 32 | s << 12 | v, or, with wide_layout (a graph beyond 4096 nodes in the large entry points),
    cand << 40 | s << 20 | v."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    if tables is None:
        tables = tables_of(n, rowptr, col, w, first)
    groups = [grp for cls in tables for grp in cls]
    cands = assign.shape[0]
    cand_ids = np.arange(cands)
    A = KS._padded(np.asarray(assign, np.int8), n)
    best = A.copy()
    snap = np.zeros(cands, np.int64)
    if len(inv_temp):
        best_cut = AR.cuts_f32(rowptr, col, w, A[:, :n])
    for s, inv_t in enumerate(np.asarray(inv_temp, F32)):
        for nodes, nb, wt in groups:
            W = KS._sums(A, nb, wt, K)
            c = A[:, nodes]
            own, wc = KS._own(W, c, K)
            others = np.where(own, INF, W)
            kk = others.argmin(axis=0)
            wk = np.take_along_axis(others, kk[None], 0)[0]
            delta = wk - wc
            lvl = table[LS.level_indices(seed, cand_ids, s, nodes, wide_layout)]
            move = (delta < 0) | (delta * inv_t <= lvl)
            A[:, nodes] = np.where(move, kk.astype(np.int8), c)
        cs = AR.cuts_f32(rowptr, col, w, A[:, :n])
        better = cs > best_cut
        best[better] = A[better]
        best_cut[better] = cs[better]
        snap[better] = s + 1
    sweeps = LS.descent(best, groups, K, max_descent_sweeps)
    out = best[:, :n].copy()
    cut_all = AR.cuts_f32(rowptr, col, w, out)
    bi = int(np.argmax(cut_all))
    return dict(assign=out, cut_all=cut_all, snap=snap.astype(np.int32), sweeps=sweeps.astype(np.int32),
                best_assign=out[bi].astype(np.int32), best_cut=cut_all[bi], best_idx=bi)


def best_single_move_gain(n, rowptr, col, w, assign, K, first):
    """The largest cut gain of moving one node >= first to another class (float64)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    a = np.asarray(assign, np.int64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    keep = (rows != col) & (a[col] >= 0) & (a[col] < K)
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    W = np.zeros((n, K))
    np.add.at(W, (rows[keep], a[col[keep]]), ww[keep])
    gain = W[np.arange(n), a] - W.min(axis=1)
    return float(gain[first:].max()) if n > first else 0.0


def cut(rowptr, col, w, assign):
    return float(AR.cuts_f32(np.asarray(rowptr, np.int64), np.asarray(col, np.int64), w, np.asarray(assign)[None])[0])


# ---- the graphs the GPU tests share -------------------------------------------------------------------------------------
def path_021():
    """The path 0 - 2 - 1 as (n, rowptr, col)."""
    return 3, np.array([0, 1, 2, 4], np.int64), np.array([2, 2, 0, 1], np.int64)


def star_centre2(leaves=70):
    """A star of `leaves` leaves whose centre is node 2 (its row has more than 64 entries)."""
    n = leaves + 1
    others = [v for v in range(n) if v != 2]
    rowptr, col = [0], []
    for v in range(n):
        col.extend(others if v == 2 else [2])
        rowptr.append(len(col))
    return n, np.asarray(rowptr, np.int64), np.asarray(col, np.int64)


def ring_with_chords(n, seed):
    """A connected graph of n >= 3 nodes: the ring plus about n / 2 random chords (no duplicates, no loops)."""
    rng = np.random.RandomState(seed)
    edges = {(v, (v + 1) % n) if v < (v + 1) % n else ((v + 1) % n, v) for v in range(n)}
    for _ in range(n // 2):
        a, b = int(rng.randint(n)), int(rng.randint(n))
        if a != b:
            edges.add((min(a, b), max(a, b)))
    nb = [[] for _ in range(n)]
    for a, b in sorted(edges):
        nb[a].append(b)
        nb[b].append(a)
    rowptr, col = [0], []
    for v in range(n):
        col.extend(sorted(nb[v]))
        rowptr.append(len(col))
    return n, np.asarray(rowptr, np.int64), np.asarray(col, np.int64)


def integer_weights(n, rowptr, col, seed):
    return LS.integer_edge_weights(n, rowptr, col, seed)


def softmax_rows(n, K, seed, scale=1.0):
    return LRR.softmax_rows(n, K, seed, scale)


# ---- one model per graph without terminals (gmc_inst_forward_t / gmc_inst_train_fwd_bwd_t, terminals = 0) ---------------
# The float64 step is composed from what exists: functional_ref.forward / backward (stepcheck's f64_forward_sparse /
# f64_backward_sparse) around functional_ref.loss_and_gp(..., terminals=False).
MARGIN = 1e-5      # no row within this of an argmax tie (every row: none is overridden)
KINK = 1e-6        # no layer-1 unit within this of the relu kink
INST_C = 1.3
# a graph below the class count, the terminals' boundary sizes, a row past a wave; the mixed batch; the centre-2 star
INST_BATCHES = {"edge": (3, "K", "K+1", 65), "mixed": (5, 300, 65, 257), "star": ("star70",)}
INST_HIDDEN = {2: 4, 3: 12, 4: 20, 8: 36}
InstCase = collections.namedtuple("InstCase", "batch K weights loss seed")
# seed: the first (from 0) for which, under both losses, the three rules of `inst_rules` hold
# (tests/test_plain_maxcut_host.py asserts them)
INST_SEEDS = {('edge', 2, 'unit'): 2, ('edge', 3, 'integer'): 1, ('mixed', 2, 'unit'): 1, ('mixed', 2, 'integer'): 1,
              ('mixed', 3, 'integer'): 1, ('star', 2, 'integer'): 1, ('star', 4, 'integer'): 2}   # others: 0
INST_CASES = [InstCase(b, K, w, l, INST_SEEDS.get((b, K, w), 0)) for b in INST_BATCHES for K in INST_HIDDEN
              for w in ("unit", "integer") for l in ("cut", "expected_cut")]


def inst_case_id(c):
    return f"{c.batch}-K{c.K}-{c.weights}-{c.loss}"


def inst_case_csrs(c):
    """The graphs of a case as (rowptr int32, col int32, weights float32 or None)."""
    out = []
    for i, spec in enumerate(INST_BATCHES[c.batch]):
        if spec == "star70":
            n, rp, cl = star_centre2(70)
        else:
            n = max({"K": c.K, "K+1": c.K + 1}.get(spec, spec), 3)      # (a GraphBatch takes graphs of at least 3 nodes)
            n, rp, cl = ring_with_chords(n, 40 + i)
        w = integer_weights(n, rp, cl, 7 + i) if c.weights == "integer" else None
        out.append((rp.astype(np.int32), cl.astype(np.int32), w))
    return out


def inst_case_params(c, csrs=None):
    csrs = inst_case_csrs(c) if csrs is None else csrs
    return [KR.random_params(len(rp) - 1, INST_HIDDEN[c.K], c.K, 10 * c.seed + g) for g, (rp, _cl, _w) in enumerate(csrs)]


def inst_step(csr, p, C, loss):
    """(forward dict, loss, gradient by parameter name) of one graph under its own model, float64, no terminals."""
    f = FR.forward(csr, p)
    value, GP = FR.loss_and_gp(csr, f["P"], C, relaxed=loss == "expected_cut", terminals=False)
    grads, _ = FR.backward(f, GP, p)
    return f, value, grads


def inst_rules(csrs, params, C, loss):
    """(smallest top-2 margin of any row, smallest |layer-1 pre-activation|, worst row ratio of a float32 numpy
    evaluation against the float64 step in units of ROW_TOL)."""
    margin, gap, ratio = float("inf"), float("inf"), 0.0
    relaxed = loss == "expected_cut"
    for csr, p in zip(csrs, params):
        f, _value, grads = inst_step(csr, p, C, loss)
        srt = np.sort(f["P"], axis=1)
        margin = min(margin, float((srt[:, -1] - srt[:, -2]).min()))
        gap = min(gap, float(np.abs(f["pre"]).min()))
        gp32 = lambda P32: FR.loss_and_gp(csr, P32, C, relaxed=relaxed, terminals=False)[1]
        _P32, g32, _ = FR.f32_eval(csr, p, None, gp32)
        ratio = max(ratio, FR.grad_ratios(g32, grads)[1])
    return margin, gap, ratio
