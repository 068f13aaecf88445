"""CPU restatement of the per-node class costs of include/gcnmaxcut.h (the ``_c`` entry points), written from the header's
text: the objective ``obj(S) = cut(S) - sum_v node_cost[v][S_v]``, the class sums and the rounding's M_k that start from
the node's cost row, the scores ``block_cut - block_cost`` in the kernel's own fp32 summation order (rows per thread,
the wave's butterfly, the four wave sums), the expected objective, and the head's loss and GP in float64.

Everything takes ``first`` (the first movable local id: K with terminals, 0 without, as tests/plain_ref.py) and ``cost``
([n, K] float32 by local id, or None).  With ``cost=None`` - and with an all-zero array - the decoders here equal
tests/plain_ref.py, tests/kway_search_ref.py and tests/rounding_ref.py output for output (tests/test_node_cost_host.py).
The forms are the one-node-at-a-time definitions: nodes of a colour class share no edge, so the class-parallel kernel
decides the same.  Unlike the older restatements the scores are not a float64 count rounded once but the device's sum
order, so they hold bit for bit for real-valued weights and costs as well."""
import itertools

import numpy as np

from tests import anneal_ref as AR
from tests import functional_ref as FR
from tests import kway_ref as KR
from tests import plain_ref as PR
from tests import seeded_ref as SR

F32 = np.float32
INF = F32(np.inf)
THREADS = 256


# ---- the objective in float64 -------------------------------------------------------------------------------------------
def cut64(rowptr, col, w, a):
    rowptr = np.asarray(rowptr, np.int64)
    a = np.asarray(a)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    return float(ww[a[rows] != a[np.asarray(col, np.int64)]].sum()) / 2


def cost64(cost, a, K):
    a = np.asarray(a, np.int64)
    ok = (a >= 0) & (a < K)
    return float(np.asarray(cost, np.float64)[np.flatnonzero(ok), a[ok]].sum())


def objective64(rowptr, col, w, cost, a, K):
    return cut64(rowptr, col, w, a) - (0.0 if cost is None else cost64(cost, a, K))


# ---- the scores in the kernel's fp32 order ------------------------------------------------------------------------------
def _wave_sum(v):
    """The butterfly over 64 lanes: v[i] += v[i ^ d] for d = 32, 16, 8, 4, 2, 1 (every lane ends with the total)."""
    v = np.asarray(v, F32).copy()
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ d]
    return v[0]


def _block_reduce(per_thread):
    q = [_wave_sum(per_thread[64 * i:64 * i + 64]) for i in range(4)]
    return F32(F32(F32(q[0] + q[1]) + q[2]) + q[3])


def block_cut(n, rowptr, col, w, a):
    """fp32: thread t adds, from +0, w_e (or 0 where the classes agree) for every edge of the rows t, t + 256, ... in
    CSR order; butterfly; ((q0 + q1) + q2) + q3; halved."""
    a = np.asarray(a, np.int8)
    acc = np.zeros(THREADS, F32)
    for l in range(n):
        t = l % THREADS
        for e in range(int(rowptr[l]), int(rowptr[l + 1])):
            if a[int(col[e])] != a[l]:
                acc[t] = acc[t] + (F32(1.0) if w is None else F32(w[e]))
    return F32(_block_reduce(acc) * F32(0.5))


def block_cost(n, cost, a, K):
    a = np.asarray(a, np.int8)
    acc = np.zeros(THREADS, F32)
    for l in range(n):
        if 0 <= a[l] < K:
            acc[l % THREADS] = acc[l % THREADS] + F32(cost[l, a[l]])
    return _block_reduce(acc)


def score(n, rowptr, col, w, cost, a, K):
    """block_cut, and with costs one fp32 subtraction of block_cost."""
    c = block_cut(n, rowptr, col, w, a)
    return c if cost is None else F32(c - block_cost(n, np.asarray(cost, F32), a, K))


# ---- class sums, descent, annealing -------------------------------------------------------------------------------------
def class_sums(rowptr, col, w, cost, a, v, K):
    """W [K] fp32 of node v: from the node's cost row (or +0), then the row's edges in CSR order, self-loops skipped, a
    neighbour's byte outside 0..K-1 adding to none."""
    W = np.zeros(K, F32) if cost is None else np.array(cost[v], F32, copy=True)
    for e in range(int(rowptr[v]), int(rowptr[v + 1])):
        u = int(col[e])
        if u != v and 0 <= a[u] < K:
            W[a[u]] = W[a[u]] + (F32(1.0) if w is None else F32(w[e]))
    return W


def descent(n, rowptr, col, w, cost, assign, K, first, max_sweeps, classes=None):
    """The local search's sweeps: a node moves to the class of its smallest sum (lowest index) iff that sum is below its
    own; a byte of no class always moves.  (class bytes int8, sweeps run)."""
    a = np.array(assign, np.int8, copy=True)
    classes = PR.colouring(n, rowptr, col, first) if classes is None else classes
    sweeps = 0
    while sweeps < max_sweeps:
        sweeps += 1
        moved = False
        for cls in classes:
            for v in cls:
                v = int(v)
                W = class_sums(rowptr, col, w, cost, a, v, K)
                kk = int(np.argmin(W))
                if not 0 <= a[v] < K or W[kk] < W[a[v]]:
                    a[v] = kk
                    moved = True
        if not moved:
            break
    return a, sweeps


def anneal_one(n, rowptr, col, w, cost, assign, K, first, inv_temp, table, seed, max_descent_sweeps, cand):
    """Steps 1-3 of the annealing for candidate `cand`: (class bytes, snap sweep, descent sweeps, final score)."""
    a = np.array(assign, np.int8, copy=True)
    classes = PR.colouring(n, rowptr, col, first)
    best, snap = a.copy(), 0
    if len(inv_temp):
        best_score = score(n, rowptr, col, w, cost, a, K)
    for s, inv_t in enumerate(np.asarray(inv_temp, F32)):
        for cls in classes:
            for v in cls:
                v = int(v)
                W = class_sums(rowptr, col, w, cost, a, v, K)
                c = int(a[v])
                lvl = table[AR.level_index(seed, cand, s, v)]
                if 0 <= c < K:
                    others = W.copy()
                    others[c] = INF
                    kk = int(np.argmin(others))
                    delta = F32(W[kk] - W[c])
                    if delta < 0 or F32(delta * inv_t) <= lvl:
                        a[v] = kk
                else:
                    a[v] = int(np.argmin(W))
        sc = score(n, rowptr, col, w, cost, a, K)
        if sc > best_score:
            best, best_score, snap = a.copy(), sc, s + 1
    out, sweeps = descent(n, rowptr, col, w, cost, best, K, first, max_descent_sweeps, classes)
    return out, snap, sweeps, score(n, rowptr, col, w, cost, out, K)


def anneal(n, rowptr, col, w, cost, assign, K, first, inv_temp, table, seed, max_descent_sweeps):
    """assign [cands, n] -> what the entry point reports for one graph (plain_ref.anneal's dict)."""
    runs = [anneal_one(n, rowptr, col, w, cost, row, K, first, inv_temp, table, seed, max_descent_sweeps, c)
            for c, row in enumerate(np.asarray(assign, np.int8))]
    out = np.stack([r[0] for r in runs])
    cut_all = np.asarray([r[3] for r in runs], F32)
    bi = int(np.argmax(cut_all))
    return dict(assign=out, cut_all=cut_all, snap=np.asarray([r[1] for r in runs], np.int32),
                sweeps=np.asarray([r[2] for r in runs], np.int32), best_assign=out[bi].astype(np.int32),
                best_cut=cut_all[bi], best_idx=bi)


# ---- the sampler --------------------------------------------------------------------------------------------------------
def sample(n, rowptr, col, w, cost, P, key, iters, first):
    a = PR.assignments(np.asarray(P, F32)[:n], key, iters, first)
    K = np.asarray(P).shape[1]
    cut_all = np.asarray([score(n, rowptr, col, w, cost, row, K) for row in a], F32)
    bi = int(np.argmax(cut_all))
    return dict(assign_all=a, cut_all=cut_all, best_assign=a[bi].astype(np.int32), best_cut=cut_all[bi], best_iter=bi)


# ---- the rounding -------------------------------------------------------------------------------------------------------
def initial_state(n, P, K, first):
    q = np.array(P, dtype=F32, copy=True)[:n]
    m = min(first, n)
    q[:m] = np.eye(K, dtype=F32)[:m]
    return q


def state_sums(rowptr, col, w, cost, q, v):
    """M [K] fp32: from the node's cost row (or +0), per edge one fp32 product and one fp32 sum."""
    M = np.zeros(q.shape[1], F32) if cost is None else np.array(cost[v], F32, copy=True)
    for e in range(int(rowptr[v]), int(rowptr[v + 1])):
        u = int(col[e])
        if u == v:
            continue
        t = (F32(1.0) if w is None else F32(w[e])) * q[u]
        M = M + t
    return M


def round_conditional(n, rowptr, col, w, cost, P, K, first):
    q = initial_state(n, P, K, first)
    a = np.zeros(n, np.int8)
    a[:min(first, n)] = np.arange(min(first, n))
    for cls in PR.colouring(n, rowptr, col, first):
        for v in cls:
            v = int(v)
            kk = int(np.argmin(state_sums(rowptr, col, w, cost, q, v)))
            q[v] = np.eye(K, dtype=F32)[kk]
            a[v] = kk
    return a


def restate_round(n, rowptr, col, w, cost, P, K, first, max_sweeps):
    """dict of a0 (rounded), a1 / sweeps (after the descent) and the score of a1."""
    a0 = round_conditional(n, rowptr, col, w, cost, P, K, first)
    a1, sweeps = descent(n, rowptr, col, w, cost, a0, K, first, max_sweeps)
    return dict(a0=a0, a1=a1, sweeps=sweeps, cut=score(n, rowptr, col, w, cost, a1, K))


def expected_objective(n, rowptr, col, w, cost, P, K, first):
    """float64: the expected cut of the initial state minus sum_v cost[v] . q_v."""
    value = PR.expected_cut(n, rowptr, col, w, np.asarray(P)[:n], K, first)
    if cost is None:
        return value
    q = initial_state(n, P, K, first).astype(np.float64)
    return value - float((np.asarray(cost, np.float64) * q).sum())


def best_single_move_gain(n, rowptr, col, w, cost, a, K, first):
    """The largest gain in obj of moving one node >= first to another class (float64)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    a = np.asarray(a, np.int64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    keep = rows != col
    ww = np.ones(rows.size) if w is None else np.asarray(w, np.float64)
    W = np.zeros((n, K)) if cost is None else np.array(cost, np.float64, copy=True)
    np.add.at(W, (rows[keep], a[col[keep]]), ww[keep])
    gain = W[np.arange(n), a] - W.min(axis=1)      # obj(moved) - obj = W[own] - W[target]
    return float(gain[first:].max()) if n > first else 0.0


# ---- the doors: QUBO and Ising ------------------------------------------------------------------------------------------
def qubo_energy(edges, q, a_lin, x):
    """E(x) = sum_i a_i x_i + sum_{i<j} q_ij x_i x_j; edges [(i, j)] every pair once."""
    x = np.asarray(x, np.float64)
    return float(np.dot(a_lin, x)) + float(sum(qq * x[i] * x[j] for (i, j), qq in zip(edges, q)))


def ising_energy(edges, J, h, s):
    s = np.asarray(s, np.float64)
    return float(np.dot(h, s)) + float(sum(jj * s[i] * s[j] for (i, j), jj in zip(edges, J)))


def csr_of_edges(n, edges, weights):
    """(rowptr, col, w float32) of an undirected weighted graph given as pairs listed once."""
    nb = [[] for _ in range(n)]
    for (i, j), ww in zip(edges, weights):
        nb[i].append((j, ww))
        nb[j].append((i, ww))
    rowptr, col, w = [0], [], []
    for v in range(n):
        for u, ww in sorted(nb[v]):
            col.append(u)
            w.append(ww)
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, F32)


def qubo_to_maxcut(n, edges, q, a_lin):
    """w = q / 2, node_cost[i] = (0, a_i + 1/2 sum_j q_ij): E(x) = -obj(x)."""
    rowptr, col, w = csr_of_edges(n, edges, [0.5 * qq for qq in q])
    half = np.zeros(n)
    for (i, j), qq in zip(edges, q):
        half[i] += 0.5 * qq
        half[j] += 0.5 * qq
    cost = np.zeros((n, 2), F32)
    cost[:, 1] = np.asarray(a_lin, np.float64) + half
    return rowptr, col, w, cost


def ising_to_maxcut(n, edges, J, h):
    """w = 2 J, class 0 is s = +1, node_cost[i] = (h_i, -h_i): H(s) = sum J - obj."""
    rowptr, col, w = csr_of_edges(n, edges, [2.0 * jj for jj in J])
    cost = np.stack([np.asarray(h, np.float64), -np.asarray(h, np.float64)], axis=1).astype(F32)
    return rowptr, col, w, cost


def brute_force_min(n, energy):
    """(minimum, minimiser bits) of energy(bits) over {0, 1}^n."""
    best, arg = float("inf"), None
    for bits in itertools.product((0, 1), repeat=n):
        e = energy(bits)
        if e < best:
            best, arg = e, bits
    return best, arg


def drawn_instance(seed, n):
    """A connected small instance with integer data: the ring plus chords (plain_ref.ring_with_chords), couplings in
    -2..2 without 0, fields / linear terms in -3..3: (n, edges, quadratic, linear)."""
    _n, rp, cl = PR.ring_with_chords(n, seed)
    edges = [(v, int(u)) for v in range(n) for u in cl[rp[v]:rp[v + 1]] if v < u]
    rng = np.random.RandomState(1000 + seed)
    quad = rng.choice([-2, -1, 1, 2], size=len(edges)).astype(np.float64)
    lin = rng.randint(-3, 4, size=n).astype(np.float64)
    return n, edges, quad, lin


def search(n, rowptr, col, w, cost, K, starts, sweeps, seed, scale):
    """The numpy restatement of "random starts + annealing + descent": the best objective (float64) and its state."""
    rng = np.random.RandomState(seed)
    A = rng.randint(0, K, (starts, n)).astype(np.int8)
    res = anneal(n, rowptr, col, w, cost, A, K, 0, AR.schedule(sweeps, scale=scale), AR.levels(), seed, 100)
    a = res["best_assign"]
    return objective64(rowptr, col, w, cost, a, K), a


# instances (seed, n) of drawn_instance for which `search` (8 starts, 30 sweeps) reaches the brute-force optimum of both
# the QUBO and the Ising reading on the machine that drew the list; tests/test_node_cost_host.py requires it for all
DOOR_INSTANCES = ((0, 6), (1, 7), (2, 8), (3, 9), (4, 10), (5, 11), (6, 12), (13, 12))


# ---- the head in float64 ------------------------------------------------------------------------------------------------
def head_loss_and_gp(csr, P, cost, C, relaxed, terminals, S=None):
    """(loss, GP) of functional_ref.loss_and_gp with the cost in the loss: -C (cut - costsum), GP += C cost.  S: the
    partition the hard loss is taken of (the device's, as stepcheck takes it); None: the reference's own."""
    P = np.asarray(P, np.float64)
    n, K = P.shape
    m = min(K, n) if terminals else 0
    if S is None:
        S = P.argmax(1)
        S[:m] = np.arange(m)
    S = np.asarray(S, np.int64)
    if relaxed:
        value, GP = FR.loss_and_gp(csr, P, C, relaxed=True, terminals=terminals)
    else:
        value, GP = KR.hard_loss_and_gp(*csr, S, K, C)
    if cost is None:
        return value, GP
    cost = np.asarray(cost, np.float64)
    Pt = P.copy()
    Pt[:m] = np.eye(K)[:m]
    costsum = float((cost * Pt).sum()) if relaxed else float(cost[np.arange(n), S].sum())
    return value + C * costsum, GP + C * cost


def inst_step(csr, p, cost, C, loss, terminals, S=None):
    """(forward dict, loss, gradient by parameter name) of one graph under its own model, float64."""
    f = FR.forward(csr, p)
    value, GP = head_loss_and_gp(csr, f["P"], cost, C, loss == "expected_cut", terminals, S)
    grads, _ = FR.backward(f, GP, p)
    return f, value, grads


def head_rules(csr, p, cost, C, terminals):
    """(smallest top-2 margin of any row, smallest |layer-1 pre-activation|, worst gradient-row ratio of a float32 numpy
    evaluation against the float64 step in units of ROW_TOL, over both losses, largest |P32 - P64| of that evaluation):
    plain_ref.inst_rules with the cost, and the probabilities' own float32 error."""
    f = FR.forward(csr, p)
    srt = np.sort(f["P"], axis=1)
    margin = float((srt[:, -1] - srt[:, -2]).min()) if f["P"].shape[1] > 1 else 1.0
    gap = float(np.abs(f["pre"]).min())
    ratio, p_err = 0.0, 0.0
    for loss in ("cut", "expected_cut"):
        _f, _value, grads = inst_step(csr, p, cost, C, loss, terminals)
        gp32 = lambda P32: head_loss_and_gp(csr, P32, cost, C, loss == "expected_cut", terminals)[1]
        P32, g32, _ = FR.f32_eval(csr, p, None, gp32)
        ratio = max(ratio, FR.grad_ratios(g32, grads)[1])
        p_err = max(p_err, float(np.abs(P32.astype(np.float64) - f["P"]).max()))
    return margin, gap, ratio, p_err
