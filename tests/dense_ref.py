"""CPU restatement of the annealing of dense two-class instances on cached local fields (include/gcnmaxcut_dense.h,
gmc_dense_anneal_f32), written from the header's text in numpy float32: the fields, the score in the device's own
summation order (rows per lane of 64, the butterfly), the sweeps that decide a visit from F[v] alone and update the
fields on a move, the snapshot by the running objective, the descent from freshly summed fields, the recounted final
score and the pick.  Every candidate of a problem runs at once (numpy over candidates); the visits are sequential, as the
rule is.

Also here: the instances, costs and orders the CPU and GPU tests of the call share, the dense <-> CSR conversion used to
hold the call against the sparse annealing, and the two changes of variables of the energy doors."""
import numpy as np

from tests import anneal_ref as AR
from tests import plain_ref as PR

F32 = np.float32
ZERO = F32(0)
LANES = 64


def _square(W):
    """[n, n] float32 of a problem's matrix [n, ld]: the columns n.. dropped, the diagonal (never read) as zero."""
    W = np.asarray(W, F32)
    Wz = np.array(W[:, :W.shape[0]], F32, copy=True)
    np.fill_diagonal(Wz, ZERO)
    return Wz


def _wave_sum(acc):
    """[cands, 64] -> [cands]: x[i] += x[i ^ d], d = 32 .. 1."""
    v = np.asarray(acc, F32).copy()
    lanes = np.arange(LANES)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ d]
    return v[:, 0]


def _lane_sums(t):
    """[cands, n] per-row values -> [cands, 64]: lane j adds rows j, j + 64, ... ascending, from +0."""
    cands, n = t.shape
    acc = np.zeros((cands, LANES), F32)
    for lo in range(0, n, LANES):
        m = min(LANES, n - lo)
        acc[:, :m] = acc[:, :m] + t[:, lo:lo + m]
    return acc


def fields(Wz, cost, S):
    """Step 1: F [cands, n] float32 of the states S [cands, n] (0 / 1)."""
    cands, n = S.shape
    off = ~np.eye(n, dtype=bool)
    W0 = np.zeros((cands, n), F32)
    W1 = np.zeros((cands, n), F32)
    if cost is not None:
        W0 += np.asarray(cost, F32)[None, :, 0]
        W1 += np.asarray(cost, F32)[None, :, 1]
    for u in range(n):
        w = Wz[:, u][None, :]                      # W[v][u] for every v
        su = S[:, u][:, None]
        on = off[u][None, :]
        W0 = np.where(on, W0 + np.where(su == 0, w, ZERO), W0)
        W1 = np.where(on, W1 + np.where(su == 1, w, ZERO), W1)
    return (W1 - W0).astype(F32)


def scores(Wz, cost, S):
    """Step 2: float32 [cands]."""
    cands, n = S.shape
    off = ~np.eye(n, dtype=bool)
    t = np.zeros((cands, n), F32)
    for u in range(n):
        w = Wz[:, u][None, :]
        su = S[:, u][:, None]
        t = np.where(off[u][None, :], t + np.where(su != S, w, ZERO), t)
    cut = (_wave_sum(_lane_sums(t)) * F32(0.5)).astype(F32)
    if cost is None:
        return cut
    picked = np.asarray(cost, F32)[np.arange(n)[None, :], S]
    return (cut - _wave_sum(_lane_sums(picked))).astype(F32)


def _sweep(Wz, order, F, S, obj, move_rule):
    """One sweep in place; move_rule(v, delta) -> bool [cands].  Returns (moved [cands] bool, moves [cands] int64)."""
    cands, n = S.shape
    moved = np.zeros(cands, bool)
    count = np.zeros(cands, np.int64)
    for v in order:
        v = int(v)
        if not 0 <= v < n:
            continue
        c = S[:, v].copy()
        f = F[:, v]
        delta = np.where(c == 0, f, -f).astype(F32)
        move = move_rule(v, delta)
        idx = np.flatnonzero(move)
        if not idx.size:
            continue
        obj[idx] = obj[idx] - delta[idx]
        two = (F32(2.0) * Wz[v]).astype(F32)[None, :]
        rows = F[idx]
        keep = rows[:, v].copy()
        rows = rows + np.where(c[idx, None] == 0, two, -two)
        rows[:, v] = keep                            # u != v
        F[idx] = rows
        S[idx, v] = 1 - c[idx]
        moved[idx] = True
        count[idx] += 1
    return moved, count


def anneal(W, cost, order, assign, inv_temp, table, seed, max_descent_sweeps, cand_ids=None):
    """One problem: W [n, ld], cost [n, 2] or None, order [n] or None, assign [cands, n] int8 -> dict of what
    gmc_dense_anneal_f32 leaves for it: assign [cands, n] int8, score_all float32 [cands], snap, sweeps int32 [cands],
    moves int64 [cands], best_assign int32 [n], best_score, best_idx; and `refused`, the uphill proposals turned down."""
    Wz = _square(W)
    n = Wz.shape[0]
    cost = None if cost is None else np.asarray(cost, F32)
    S = (np.asarray(assign, np.int8) & 1).astype(np.int64)
    cands = S.shape[0]
    ids = np.arange(cands) if cand_ids is None else np.asarray(cand_ids)
    order = np.arange(n) if order is None else np.asarray(order, np.int64)
    inv_temp = np.asarray(inv_temp, F32)
    snap = np.zeros(cands, np.int32)
    moves = np.zeros(cands, np.int64)
    refused = uphill = 0
    if len(inv_temp):
        F = fields(Wz, cost, S)
        obj = scores(Wz, cost, S)
        best, best_obj = S.copy(), obj.copy()
        for s, inv_t in enumerate(inv_temp):
            tally = [0, 0]
            lvl = np.asarray(table, F32)[AR.level_indices(seed, ids, s, np.arange(n))]     # [cands, n]

            def rule(v, delta, lvl=lvl, inv_t=inv_t):
                with np.errstate(invalid="ignore", over="ignore"):
                    move = (delta < 0) | ((delta * inv_t).astype(F32) <= lvl[:, v])
                tally[0] += int((~move).sum())
                tally[1] += int((move & (delta > 0)).sum())
                return move
            _moved, count = _sweep(Wz, order, F, S, obj, rule)
            moves += count
            refused += tally[0]
            uphill += tally[1]
            better = obj > best_obj
            best[better] = S[better]
            best_obj[better] = obj[better]
            snap[better] = s + 1
        S = best.copy()
    F = fields(Wz, cost, S)
    sweeps = np.zeros(cands, np.int32)
    live = np.ones(cands, bool)
    obj = np.zeros(cands, F32)
    while True:                                       # a candidate stops after a sweep of its own that moved nothing
        run = live & (sweeps < max_descent_sweeps)
        if not run.any():
            break
        sweeps[run] += 1
        moved, _ = _sweep(Wz, order, F, S, obj, lambda v, delta, run=run: (delta < 0) & run)
        live = run & moved
    score_all = scores(Wz, cost, S)
    bi = int(np.argmax(score_all))
    return dict(assign=S.astype(np.int8), score_all=score_all, snap=snap, sweeps=sweeps, moves=moves,
                best_assign=S[bi].astype(np.int32), best_score=score_all[bi], best_idx=bi, refused=refused, uphill=uphill)


def anneal_batch(W, cost, order, assign, inv_temp, table, seed, max_descent_sweeps):
    """The whole call: W [B, n, ld], cost [B * n, 2] or None, order [B * n] or None, assign [cands, B * n] -> the
    outputs in the call's layouts (assign [cands, R], score_all / snap / sweeps / moves [B, cands], best_assign [R],
    best_score / best_idx [B])."""
    B, n = W.shape[0], W.shape[1]
    runs = [anneal(W[b], None if cost is None else cost[b * n:(b + 1) * n],
                   None if order is None else order[b * n:(b + 1) * n], assign[:, b * n:(b + 1) * n], inv_temp, table,
                   seed, max_descent_sweeps) for b in range(B)]
    return dict(assign=np.concatenate([r["assign"] for r in runs], axis=1),
                score_all=np.stack([r["score_all"] for r in runs]).astype(F32),
                snap=np.stack([r["snap"] for r in runs]).astype(np.int32),
                sweeps=np.stack([r["sweeps"] for r in runs]).astype(np.int32),
                moves=np.stack([r["moves"] for r in runs]).astype(np.int64),
                best_assign=np.concatenate([r["best_assign"] for r in runs]).astype(np.int32),
                best_score=np.asarray([r["best_score"] for r in runs], F32),
                best_idx=np.asarray([r["best_idx"] for r in runs], np.int32),
                refused=sum(r["refused"] for r in runs), uphill=sum(r["uphill"] for r in runs))


# ---- dense <-> CSR -------------------------------------------------------------------------------------------------------
def csr_of_dense(W):
    """(rowptr, col, w float32) of the non-zero off-diagonal entries of W [n, >= n]."""
    Wz = _square(W)
    n = Wz.shape[0]
    rowptr, col, w = [0], [], []
    for v in range(n):
        nz = np.flatnonzero(Wz[v] != 0)
        col.extend(nz.tolist())
        w.extend(Wz[v, nz].tolist())
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, F32)


def colour_order(n, rowptr, col):
    """The (colour, id) order of tests/plain_ref.py without terminals, as local ids [n]."""
    classes = PR.colouring(n, rowptr, col, 0)
    return np.concatenate(classes).astype(np.int32) if classes else np.zeros(0, np.int32)


# ---- instances -------------------------------------------------------------------------------------------------------------
def symmetric(n, draw, density=1.0, seed=0):
    """[n, n] float32, symmetric bit for bit, zero diagonal: draw(rng, count) on the kept pairs u < v."""
    rng = np.random.RandomState(seed)
    iu = np.triu_indices(n, 1)
    vals = np.asarray(draw(rng, iu[0].size), F32)
    if density < 1.0:
        vals = np.where(rng.rand(iu[0].size) < density, vals, ZERO)
    W = np.zeros((n, n), F32)
    W[iu] = vals
    return (W + W.T).astype(F32)


def weights_of(kind, n, seed, density=1.0):
    if kind == "unit":
        return symmetric(n, lambda r, m: np.ones(m), density, seed)
    if kind == "pm1":
        return symmetric(n, lambda r, m: r.choice([-1.0, 1.0], size=m), density, seed)
    if kind == "int":
        return symmetric(n, lambda r, m: r.choice([-3, -2, -1, 1, 2, 3, 4], size=m).astype(np.float64), density, seed)
    assert kind == "real"
    return symmetric(n, lambda r, m: r.uniform(-1.5, 2.0, m) * (1.0 + 2.0 ** -20), density, seed)


def regular_dense(n, degree, seed):
    """[n, n] unit weights of a `degree`-regular graph on a ring (v +- 1 .. +- degree // 2, plus the antipode for an odd
    degree and even n), relabelled by a seeded permutation."""
    W = np.zeros((n, n), F32)
    for v in range(n):
        for d in range(1, degree // 2 + 1):
            W[v, (v + d) % n] = W[(v + d) % n, v] = 1.0
        if degree % 2 and n % 2 == 0:
            W[v, (v + n // 2) % n] = W[(v + n // 2) % n, v] = 1.0
    p = np.random.RandomState(seed).permutation(n)
    return W[np.ix_(p, p)].copy()


def cost_of(kind, rows, seed):
    rng = np.random.RandomState(seed)
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros((rows, 2), F32)
    if kind == "negzero":
        return np.full((rows, 2), -0.0, F32)
    if kind == "int":
        return rng.randint(-3, 4, (rows, 2)).astype(F32)
    if kind == "barrier":                             # a few nodes pinned to a class by a cost of 1e6 on the other
        c = rng.randint(-2, 3, (rows, 2)).astype(F32)
        pick = rng.choice(rows, max(rows // 8, 1), replace=False)
        c[pick, rng.randint(0, 2, pick.size)] = 1e6
        return c
    assert kind == "real"
    return (rng.uniform(-2.0, 2.0, (rows, 2)) * (1.0 + 2.0 ** -20)).astype(F32)


def padded(W, ld):
    """[B, n, ld] with NaN in the columns n.. and on the diagonal: neither may be read."""
    B, n = W.shape[0], W.shape[1]
    out = np.full((B, n, ld), np.nan, F32)
    out[:, :, :n] = W
    out[:, np.arange(n), np.arange(n)] = np.nan
    return out


def rms_field(W):
    """The temperature unit of the dense doors: sqrt(mean_v sum_u w_vu^2), float64 (1 for an all-zero matrix)."""
    Wz = np.stack([_square(w) for w in np.asarray(W, F32).reshape(-1, W.shape[-2], W.shape[-1])]).astype(np.float64)
    s = float(np.sqrt((Wz ** 2).sum(axis=2).mean()))
    return s if s > 0 else 1.0


# ---- the energy doors --------------------------------------------------------------------------------------------------------
def ising_energy(J, h, s):
    """H(s) = sum_{i<j} J_ij s_i s_j + sum_i h_i s_i, float64."""
    J = np.asarray(J, np.float64)
    s = np.asarray(s, np.float64)
    return float(np.triu(J, 1).dot(s).dot(s)) + float(np.dot(np.asarray(h, np.float64), s))


def qubo_energy(Q, a, x):
    """E(x) = sum_i a_i x_i + sum_{i<j} q_ij x_i x_j, float64."""
    Q = np.asarray(Q, np.float64)
    x = np.asarray(x, np.float64)
    return float(np.triu(Q, 1).dot(x).dot(x)) + float(np.dot(np.asarray(a, np.float64), x))


def _row_sums(w):
    """sum_j w_ij over j ascending, j != i, in float32 from +0: the doors' stated order."""
    n = w.shape[0]
    acc = np.zeros(n, F32)
    for j in range(n):
        acc = np.where(np.arange(n) != j, acc + w[:, j], acc)
    return acc


def ising_to_dense(J, h):
    """w = 2 J, node_cost[i] = (h_i, -h_i), class 0 is s = +1: H(s) = sum_{i<j} J_ij - obj."""
    w = (F32(2.0) * _square(J)).astype(F32)
    h = np.zeros(w.shape[0]) if h is None else np.asarray(h, np.float64)
    return w, np.stack([h, -h], axis=1).astype(F32)


def qubo_to_dense(Q, a):
    """w = q / 2, node_cost[i] = (0, a_i + sum_j w_ij), class 1 is x = 1: E(x) = -obj."""
    w = (F32(0.5) * _square(Q)).astype(F32)
    a = np.zeros(w.shape[0], F32) if a is None else np.asarray(a, F32)
    cost = np.zeros((w.shape[0], 2), F32)
    cost[:, 1] = a + _row_sums(w)
    return w, cost


# ---- the cases of tests/test_gpu_dense.py (tests/test_dense_host.py counts the uphill moves they take and refuse) ------------
SEED = 0x2468ACE
#        n   B cands pad order     weights density cost       sweeps descent
CASES = [(2, 1, 1, 0, None, "unit", 1.0, None, 4, 3),
         (3, 3, 3, 2, "colour", "pm1", 1.0, "zero", 4, 3),
         (63, 1, 4, 1, "colour", "int", 0.5, "int", 5, 4),
         (64, 3, 5, 0, "perm", "real", 1.0, "real", 5, 4),
         (65, 1, 9, 3, "colour", "int", 1.0, "barrier", 5, 4),
         (130, 3, 3, 5, "colour", "pm1", 0.1, "negzero", 4, 4),
         (257, 1, 5, 7, None, "real", 1.0, "real", 3, 3),
         (65, 1, 4, 0, "perm", "real", 0.5, None, 0, 5),
         (130, 1, 3, 0, None, "unit", 1.0, "int", 4, 0),
         (257, 1, 3, 2, "colour", "unit", 0.03, None, 4, 4)]
INTEGER = ("unit", "pm1", "int")
INTEGER_COSTS = (None, "zero", "negzero", "int", "barrier")


def is_integer_case(case):
    return case[5] in INTEGER and case[7] in INTEGER_COSTS


def case_inputs(case):
    """dict of W [B, n, ld] (NaN in the padding and on the diagonal), square [B, n, n], cost, order, assign, inv_temp."""
    n, B, cands, pad, order_kind, weights, density, cost_kind, sweeps, _descent = case
    square = np.stack([weights_of(weights, n, 100 * n + b, density) for b in range(B)])
    if order_kind is None:
        order = None
    elif order_kind == "perm":
        order = np.concatenate([np.random.RandomState(7 + b).permutation(n) for b in range(B)]).astype(np.int32)
    else:
        order = np.concatenate([colour_order(n, *csr_of_dense(square[b])[:2]) for b in range(B)]).astype(np.int32)
    assign = np.random.RandomState(n + cands).randint(0, 2, (cands, B * n)).astype(np.int8)
    assign[0, 0] = 6                                   # a class byte is byte & 1
    assign[cands - 1, B * n - 1] = -1
    return dict(W=padded(square, n + pad), square=square, cost=cost_of(cost_kind, B * n, 3 * n + 1), order=order,
                assign=assign, inv_temp=AR.schedule(sweeps, scale=rms_field(square)))
