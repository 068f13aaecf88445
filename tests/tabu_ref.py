"""CPU restatement of the one-flip tabu search of include/gcnmaxcut.h (gmc_kway_tabu_f32), written from the header's
text in numpy float32 scalars and arrays and independent of the library: one chain - one (candidate, graph) pair - at a
time.  Every fp32 step of the header is one numpy float32 operation here; the class sums are accumulated in the CSR
order of a row and the updates of a move are applied in the CSR order of the moved node's row."""
import collections

import numpy as np

GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
F = np.float32


def mix64(z):
    """splitmix64 finaliser on a Python integer."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draws(seed, cand, it, n_mov, tenure_base, tenure_span, tenure_div):
    """(r, tenure) of step 1."""
    h = mix64(seed + GOLD * (((cand << 32) | it) + 1))
    r = (h & 0xFFFFFFFF) % n_mov
    span = tenure_span + (n_mov // tenure_div if tenure_div > 0 else 0)
    return r, tenure_base + (h >> 32) % (span + 1)


def class_sums(n, rowptr, col, w, state, K):
    """W [n, K] float32: per node the sums of its edge weights by the neighbour's class, in the CSR order of the row,
    from +0.0; self-loops skipped; a byte outside 0..K-1 adds to no sum."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    ww = np.ones(col.size, F) if w is None else np.asarray(w, F)
    W = np.zeros((n, K), F)
    deg = np.diff(rowptr)
    for j in range(int(deg.max()) if n else 0):
        v = np.nonzero(deg > j)[0]
        e = rowptr[v] + j
        u = col[e]
        cu = state[u].astype(np.int64)
        ok = (u != v) & (cu >= 0) & (cu < K)
        W[v[ok], cu[ok]] = W[v[ok], cu[ok]] + ww[e[ok]]    # one node once per j: a plain fp32 add each
    return W


Result = collections.namedtuple("Result", "assign best_it moves best trace")


def tabu(n, rowptr, col, w, state0, K, terminals, cand, iterations, tenure_base=3, tenure_span=0, tenure_div=10,
         seed=0, trace=False):
    """One chain from state0 [n] int8 -> Result: the snapshot [n] int8, best_it, the iterations that moved a node,
    `best` (float32) and, with trace=True, the moves as (it, v, k, gain, was_tabu)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    ww = np.ones(col.size, F) if w is None else np.asarray(w, F)
    state = np.array(state0, np.int8).copy()
    snap = state.copy()
    first = K if terminals else 0
    n_mov = n - first
    best_it = moves = 0
    rel = best = F(0.0)
    log = []
    if iterations > 0 and n_mov > 0:
        W = class_sums(n, rowptr, col, w, state, K)
        until = np.zeros(n, np.int64)                     # it + 1 + tenure < 2^34: never saturates
        mov = np.arange(first, n)
        ks = np.arange(K)
        for it in range(iterations):
            r, tenure = draws(seed & M64, cand, it, n_mov, tenure_base, tenure_span, tenure_div)
            c = state[mov].astype(np.int64)
            in_class = (c >= 0) & (c < K)
            cc = np.where(in_class, c, 0)
            gain = W[mov, cc][:, None] - W[mov]           # [n_mov, K] float32, one subtraction each
            assert gain.dtype == F
            free = until[mov] <= it
            adm = in_class[:, None] & (ks[None, :] != cc[:, None]) & (free[:, None] | ((rel + gain) > best))
            if not adm.any():
                continue
            top = gain[adm].max()
            rank = (mov - first - r) % n_mov
            order = np.where(adm & (gain == top), rank[:, None] * K + ks[None, :], n_mov * K)
            i, k = divmod(int(order.argmin()), K)
            v, c_v, g = int(mov[i]), int(cc[i]), gain[i, k]
            log.append((it, v, k, g, not free[i]))
            state[v] = k
            for e in range(rowptr[v], rowptr[v + 1]):     # CSR order
                u = col[e]
                if u != v:
                    W[u, c_v] = W[u, c_v] - ww[e]
                    W[u, k] = W[u, k] + ww[e]
            rel = F(rel + g)
            until[v] = it + 1 + tenure
            moves += 1
            if rel > best:
                best, best_it = rel, it + 1
                snap = state.copy()
    return Result(snap, best_it, moves, best, log if trace else None)


def tabu_all(n, rowptr, col, w, A, K, terminals, iterations, tenure_base=3, tenure_span=0, tenure_div=10, seed=0):
    """Every candidate of A [cands, n] int8: (assign [cands, n] int8, best_it [cands] int32, moves [cands] int32)."""
    A = np.asarray(A, np.int8)
    res = [tabu(n, rowptr, col, w, A[i], K, terminals, i, iterations, tenure_base, tenure_span, tenure_div, seed)
           for i in range(A.shape[0])]
    return (np.stack([x.assign for x in res]), np.asarray([x.best_it for x in res], np.int32),
            np.asarray([x.moves for x in res], np.int32))


def cut_f64(rowptr, col, w, a):
    """The cut of one assignment, counted in float64."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    ww = np.ones(col.size) if w is None else np.asarray(w, np.float64)
    a = np.asarray(a)
    return float(((a[rows] != a[col]) * ww).sum() / 2)
