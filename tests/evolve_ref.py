"""CPU restatement of the evolution stage of include/gcnmaxcut.h (gmc_kway_evolve_f32), written from the header's text:
the ranking, the parents, the alignment and the crossover in plain Python, one slot at a time; step 5 is
tests/kway_search_ref.py's ``anneal`` (which is ``refine`` without annealing sweeps) on the children of a generation at
once, slot i in the place of the candidate index.  Cuts are counted in float64 and rounded to fp32 once
(tests/anneal_ref.py): for unit and small-integer weights that is the value any fp32 summation order gives, so every
comparison of cuts is the device's there (and only there).  The module also holds the case list of the GPU tests."""
import collections

import numpy as np

from tests import anneal_ref as AR
from tests import kway_search_ref as KS

GOLD, M64 = AR.GOLD, AR.M64
SELECT = 0x53454C4543543031
CROSS = 0x43524F5353303031
mix64 = AR.mix64_int


def seeds(seed, g):
    """(S_g, select_g, cross_g) of generation g >= 1."""
    s = mix64(seed + GOLD * g)
    return s, mix64(s ^ SELECT), mix64(s ^ CROSS)


def ranking(cuts):
    """The slots ordered by (cut descending, slot ascending)."""
    return sorted(range(len(cuts)), key=lambda j: (-float(cuts[j]), j))


def parent_b(cuts, elite, select_seed, slot):
    """The slot of parent b, or None when a is the only elite member."""
    E = min(max(int(elite), 1), len(cuts))
    order = ranking(cuts)
    r = mix64(select_seed + GOLD * (slot + 1)) % E
    if order[r] != slot:
        return order[r]
    return order[(r + 1) % E] if E > 1 else None


def align(a, b, K):
    """pi: class of b -> class of a, by K rounds of greedy matching on the overlap counts of the movable nodes."""
    O = [[0] * K for _ in range(K)]
    for ca, cb in zip(a[K:], b[K:]):
        if 0 <= ca < K and 0 <= cb < K:
            O[ca][cb] += 1
    free_a, free_b, pi = set(range(K)), set(range(K)), {}
    for _ in range(K):
        ca, cb = min(((x, y) for x in free_a for y in free_b), key=lambda p: (-O[p[0]][p[1]], p[0], p[1]))
        pi[cb] = ca
        free_a.remove(ca)
        free_b.remove(cb)
    return pi


def child_of(a, b, K, cross_seed, slot):
    """The child of steps 3-4 (b None: a with the terminals set), a list of ints."""
    a = [int(x) for x in a]
    child = list(range(K)) + a[K:]
    if b is None:
        return child
    b = [int(x) for x in b]
    pi = align(a, b, K)
    for v in range(K, len(a)):
        if not 0 <= b[v] < K:
            continue                                     # a byte of no class loses: a[v]
        t = pi[b[v]]
        if t == a[v]:
            continue
        if not 0 <= a[v] < K or mix64(cross_seed + GOLD * (((slot << 32) | v) + 1)) >> 63:
            child[v] = t
    return child


Result = collections.namedtuple("Result", "pop cut best_assign best_cut best_idx history written")


def evolve(n, rowptr, col, w, pop0, K, generations, elite, inv_temp, table, seed, max_descent_sweeps):
    """pop0 [cands, n] int8 -> Result: pop [2, cands, n] int8 and cut [2, cands] float32 (plane 1 meaningful only when
    written: ``written`` = generations > 0), best_assign [n] int32, best_cut, best_idx, history [generations + 1]."""
    pop0 = np.asarray(pop0, np.int8)
    cands = pop0.shape[0]
    pop = np.zeros((2, cands, n), np.int8)
    cut = np.zeros((2, cands), np.float32)
    pop[0] = pop0
    cut[0] = AR.cuts_f32(rowptr, col, w, pop0)
    history = [cut[0].max()]
    for g in range(1, generations + 1):
        prev, nxt = (g - 1) & 1, g & 1
        s_g, select, cross = seeds(seed, g)
        children = np.empty((cands, n), np.int8)
        for i in range(cands):
            pb = parent_b(cut[prev], elite, select, i)
            children[i] = child_of(pop[prev, i], None if pb is None else pop[prev, pb], K, cross, i)
        improved, _snap, _sweeps = KS.anneal(n, rowptr, col, w, children, K, inv_temp, table, s_g, max_descent_sweeps)
        c = AR.cuts_f32(rowptr, col, w, improved)
        keep = c >= cut[prev]
        pop[nxt] = np.where(keep[:, None], improved, pop[prev])
        cut[nxt] = np.where(keep, c, cut[prev])
        history.append(cut[nxt].max())
    last = generations & 1
    bi = int(np.argmax(cut[last]))                           # the first of the largest
    return Result(pop, cut, pop[last, bi].astype(np.int32), cut[last, bi], bi, np.asarray(history, np.float32),
                  generations > 0)


# ---- the cases of tests/test_gpu_evolve.py ---------------------------------------------------------------------------
# graphs: a name of GRAPH_SETS there; sweeps / descent: anneal_sweeps and max_descent_sweeps of the children
Case = collections.namedtuple("Case", "K graphs cands elite generations sweeps descent")

CASES = [
    # n = K (nothing movable), n = K + 1, past a wave, past the workgroup; every K; both plane parities
    *[Case(K, "edges", 7, 2, G, 6, 100) for K in (2, 3, 8) for G in (0, 1, 3)],
    # the population sizes and the elite at its bounds (1, 2 and beyond cands)
    *[Case(4, "edges", cands, elite, 3, 4, 100) for cands, elite in ((1, 1), (1, 2), (2, 1), (2, 2), (2, 5))],
    *[Case(K, "small", 70, elite, 2, 3, 100) for K, elite in ((2, 1), (3, 2), (8, 71))],
    # a batch of three graphs of different sizes, one skipped for n < K
    Case(5, "batch", 7, 3, 3, 5, 100),
    # crossover alone
    *[Case(K, "edges", 7, 3, G, 0, 0) for K in (2, 3, 8) for G in (1, 2)],
    # descent alone and annealing alone
    Case(3, "small", 7, 2, 2, 0, 100), Case(3, "small", 7, 2, 2, 5, 0),
    # the copy of the graph in LDS beside the batch's arrays in global memory; small-integer weights on both
    *[Case(K, name, 7, 2, 2, 5, 100) for K in (2, 8) for name in ("staged", "global", "weights_staged", "weights_global")],
]
