"""CPU restatement of the tabu search under class-size bounds of include/gcnmaxcut.h (gmc_kway_balance_f32), written
from the header's text in numpy float32 and independent of the library, as tests/tabu_ref.py restates
gmc_kway_tabu_f32: one chain - one (candidate, graph) pair - at a time, every fp32 step one numpy float32 operation, the
updates of a move applied in the CSR order of the moved node's row."""
import collections

import numpy as np

from tests.tabu_ref import M64, class_sums, draws

F = np.float32


def admits(lo, hi, n, terminals):
    """The header's "bounds admit a partition" for one graph of n nodes."""
    lo, hi = [int(x) for x in lo], [int(x) for x in hi]
    t = 1 if terminals else 0
    return (all(l <= h and h >= t for l, h in zip(lo, hi)) and sum(max(l, t) for l in lo) <= n <= sum(hi))


def sizes(state, K, first):
    """(s, m): the nodes of every class, over the graph and over its movable nodes."""
    state = np.asarray(state).astype(np.int64)
    s = np.array([(state == c).sum() for c in range(K)], np.int64)
    m = np.array([(state[first:] == c).sum() for c in range(K)], np.int64)
    return s, m


def violation(s, lo, hi):
    return int(np.maximum(0, lo - s).sum() + np.maximum(0, s - hi).sum())


def balanced_bounds(n, K):
    """The exact bounds: floor and ceil of n / K for every class."""
    return np.full(K, n // K, np.int64), np.full(K, -(-n // K), np.int64)


Result = collections.namedtuple("Result", "assign best_it moves repairs best trace")


def _apply(W, state, rowptr, col, ww, v, a, b):
    state[v] = b
    for e in range(rowptr[v], rowptr[v + 1]):                 # CSR order
        u = col[e]
        if u != v:
            W[u, a] = W[u, a] - ww[e]
            W[u, b] = W[u, b] + ww[e]


def _best(gain, ok, rank, K):
    """The largest gain among ok [n_mov, K], ties to the smallest rank, then the smallest class: (row, class) or None."""
    if not ok.any():
        return None
    top = gain[ok].max()
    order = np.where(ok & (gain == top), rank[:, None] * K + np.arange(K)[None, :], rank.size * K)
    return divmod(int(order.argmin()), K)


def balanced(n, rowptr, col, w, state0, K, terminals, cand, lo, hi, iterations, tenure_base=3, tenure_span=0,
             tenure_div=10, seed=0, trace=False):
    """One chain from state0 [n] int8 under lo, hi [K] -> Result: the snapshot [n] int8, best_it, the iterations that
    moved a node, the repair moves, `best` (float32) and, with trace=True, the moves as (it, v, b, gain, kind) with
    kind in "repair", "free", "paired", "counter" (it = -1 for repairs).  The caller checks admits() first."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    ww = np.ones(col.size, F) if w is None else np.asarray(w, F)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    state = np.array(state0, np.int8).copy()
    first = K if terminals else 0
    n_mov = n - first
    best_it = moves = repairs = 0
    rel = best = F(0.0)
    log = []
    s, m = sizes(state, K, first)
    snap = state.copy()
    if n_mov > 0 and (iterations > 0 or violation(s, lo, hi) > 0):
        W = class_sums(n, rowptr, col, w, state, K)
        mov = np.arange(first, n)
        ks = np.arange(K)

        def view():
            c = state[mov].astype(np.int64)
            in_class = (c >= 0) & (c < K)
            cc = np.where(in_class, c, 0)
            gain = W[mov, cc][:, None] - W[mov]               # [n_mov, K] float32, one subtraction each
            assert gain.dtype == F
            return in_class, cc, gain

        # ---- repair
        while violation(s, lo, hi) > 0:
            da = np.where(s > hi, -1, np.where(s <= lo, 1, 0))
            db = np.where(s < lo, -1, np.where(s >= hi, 1, 0))
            lowers = (da[:, None] + db[None, :] < 0) & (ks[:, None] != ks[None, :])
            in_class, cc, gain = view()
            pick = _best(gain, in_class[:, None] & lowers[cc], mov - first, K)
            if pick is None:
                break
            i, b = pick
            v, a = int(mov[i]), int(cc[i])
            log.append((-1, v, b, gain[i, b], "repair"))
            _apply(W, state, rowptr, col, ww, v, a, b)
            s[a] -= 1; m[a] -= 1; s[b] += 1; m[b] += 1
            repairs += 1
        snap = state.copy()
        until = np.zeros(n, np.int64)                         # it + 1 + tenure < 2^34: never saturates
        # ---- the iterations
        for it in range(iterations):
            r, tenure = draws(seed & M64, cand, it, n_mov, tenure_base, tenure_span, tenure_div)
            free_ab = (s > lo)[:, None] & (s < hi)[None, :] & (ks[:, None] != ks[None, :])
            paired_ab = ~free_ab & (m >= 1)[None, :] & (ks[:, None] != ks[None, :])
            in_class, cc, gain = view()
            unbanned = until[mov] <= it
            free_mv = in_class[:, None] & free_ab[cc]
            adm = (free_mv & (unbanned[:, None] | ((rel + gain) > best))) | \
                  (in_class[:, None] & paired_ab[cc] & unbanned[:, None])
            rank = (mov - first - r) % n_mov
            pick = _best(gain, adm, rank, K)
            if pick is None:
                continue
            i, b = pick
            v, a, g = int(mov[i]), int(cc[i]), gain[i, b]
            is_free = bool(free_ab[a, b])
            log.append((it, v, b, g, "free" if is_free else "paired"))
            _apply(W, state, rowptr, col, ww, v, a, b)
            rel = F(rel + g)
            until[v] = it + 1 + tenure
            moves += 1
            if is_free:
                s[a] -= 1; m[a] -= 1; s[b] += 1; m[b] += 1
            else:
                in_class, cc, gain = view()                   # from the updated table
                ok = np.zeros((n_mov, K), bool)
                ok[:, a] = in_class & (cc == b) & (mov != v)
                i2, a2 = _best(gain, ok, rank, K)             # m[b] >= 1: it exists
                u, g2 = int(mov[i2]), gain[i2, a]
                assert a2 == a
                log.append((it, u, a, g2, "counter"))
                _apply(W, state, rowptr, col, ww, u, b, a)
                rel = F(rel + g2)
                until[u] = it + 1 + tenure
            if rel > best:
                best, best_it = rel, it + 1
                snap = state.copy()
    return Result(snap, best_it, moves, repairs, best, log if trace else None)


def balanced_all(n, rowptr, col, w, A, K, terminals, lo, hi, iterations, tenure_base=3, tenure_span=0, tenure_div=10,
                 seed=0):
    """Every candidate of A [cands, n] int8: (assign [cands, n] int8, best_it, moves, repairs [cands] int32)."""
    A = np.asarray(A, np.int8)
    res = [balanced(n, rowptr, col, w, A[i], K, terminals, i, lo, hi, iterations, tenure_base, tenure_span, tenure_div,
                    seed) for i in range(A.shape[0])]
    return (np.stack([x.assign for x in res]), np.asarray([x.best_it for x in res], np.int32),
            np.asarray([x.moves for x in res], np.int32), np.asarray([x.repairs for x in res], np.int32))
