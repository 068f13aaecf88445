"""Float64 restatement of one model per graph (include/gcnmaxcut.h, gmc_inst_*), built from what exists: per graph,
`kway_ref.f64_step` on the one-graph batch with that graph's own parameters (`conv1.weight [n_g, F]`); the float64 Adam
step the K-class trainer test replays; keep-best.  Nothing couples two graphs, so there is nothing else to restate.

The cases of tests/test_gpu_instance.py (`CASES`) live here so that tests/test_instance_host.py can assert on this float64
reference what lets the GPU test demand identical partitions: no non-terminal row within `kway_ref.MARGIN` of an argmax
tie, no layer-1 unit within `kway_ref.KINK` of the relu kink - and that the row bars are within float32's reach at all
(`f32_row_ratio`)."""
import collections

import numpy as np

from tests import kway_ref as KR
from tests import stepcheck, util
from tests.stepcheck import KEYS

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


# ---- one step
def graph_step(csr, params_g, C=1.0, loss="cut", S_got=None):
    """stepcheck.Ref of ONE graph under its own model (params_g["conv1.weight"] is [n_g, F])."""
    assert params_g["conv1.weight"].shape[0] == len(csr[0]) - 1
    return KR.f64_step([csr], params_g, C, loss, S_got=S_got)


def batch_step(csrs, params, C=1.0, loss="cut", S_got=None):
    """One Ref per graph; S_got (optional): the device's partition over the batch's rows."""
    refs, off = [], 0
    for csr, p in zip(csrs, params):
        n = len(csr[0]) - 1
        refs.append(graph_step(csr, p, C, loss, None if S_got is None else S_got[off:off + n]))
        off += n
    return refs


def adam_f64(m0, v0, g, t, lr):
    """(m1, v1, update) of one float64 Adam step number t (the replay of test_gpu_kway.py)."""
    m1 = BETA1 * m0 + (1 - BETA1) * g
    v1 = BETA2 * v0 + (1 - BETA2) * g * g
    return m1, v1, -lr / (1 - BETA1 ** t) * m1 / (np.sqrt(v1) / np.sqrt(1 - BETA2 ** t) + EPS)


# ---- keep-best
class KeepBest:
    """best_S / best_loss / best_epoch of a batch: a graph's rows, loss and epoch are taken when its loss is strictly
    below its best so far (the first minimum wins; NaN compares false and never wins); +inf to start with."""

    def __init__(self, goff):
        self.goff = [int(x) for x in goff]
        B = len(self.goff) - 1
        self.best_S = np.zeros(self.goff[-1], np.int32)
        self.best_loss = np.full(B, np.inf, np.float32)
        self.best_epoch = np.full(B, -1, np.int32)

    def update(self, S, loss, epoch):
        S, loss = np.asarray(S, np.int32), np.asarray(loss, np.float32)
        for g in range(len(self.best_loss)):
            if loss[g] < self.best_loss[g]:
                self.best_S[self.goff[g]:self.goff[g + 1]] = S[self.goff[g]:self.goff[g + 1]]
                self.best_loss[g] = loss[g]
                self.best_epoch[g] = epoch


# ---- the cases of tests/test_gpu_instance.py
# batches whose graph boundaries fall off every power of two: a terminals-only graph, one free node, a row past a wave;
# and a graph past one 256-row tile with the next graph starting mid-tile.  "K" / "K+1": the run's class count.  The
# first graph of "mixed" is the 5-node graph where number_classes allows one (K <= 5) and the terminals-only graph of K
# nodes at K = 8, where a 5-node graph is refused (fewer nodes than classes).
BATCHES = {"edge": (("K", 3, 1), ("K+1", 3, 2), (65, 7, 3)),
           "mixed": ((5, 3, 4), (300, 7, 5), (65, 6, 6), (257, 7, 7))}
HIDDEN = {2: 4, 3: 12, 5: 260, 8: 516}     # the h* widths of kway_ref.SHAPES, one per class count
Case = collections.namedtuple("Case", "batch K weights loss seed")
# seed: the first (from 0) for which, under both losses, the precondition above holds and `f32_row_ratio` (below) stays
# within half of ROW_TOL (tests/test_instance_host.py asserts all three)
SEEDS = {("edge", 2, "unit"): 2, ("edge", 8, "unit"): 3, ("edge", 8, "real"): 3, ("mixed", 8, "real"): 3}   # others: 0
CASES = [Case(b, K, w, l, SEEDS.get((b, K, w), 0)) for b in BATCHES for K in HIDDEN for w in ("unit", "real")
         for l in ("cut", "expected_cut")]


def case_id(c):
    return f"{c.batch}-K{c.K}-{c.weights}-{c.loss}"


def case_sizes(c):
    sizes = [{"K": c.K, "K+1": c.K + 1}.get(n, n) for n, _d, _s in BATCHES[c.batch]]
    return [max(n, 3, c.K) for n in sizes]             # (a GraphBatch takes graphs of at least 3 nodes)


def case_graphs(c):
    """The networkx graphs of a case: near-regular, unit weights or real-valued float32 weights in [0.3, 3)."""
    graphs = []
    for n, (_n, d, seed) in zip(case_sizes(c), BATCHES[c.batch]):
        g = util.near_regular(n, d, seed)
        if c.weights == "real":
            rng = np.random.RandomState(100 + seed)
            for u, v in g.edges():
                g[u][v]["weight"] = float(np.float32(rng.uniform(0.3, 3.0)))
        graphs.append(g)
    return graphs


def case_params(c, sizes=None):
    """One parameter dict per graph (kway_ref.random_params of a model with n_g rows)."""
    sizes = case_sizes(c) if sizes is None else sizes
    return [KR.random_params(n, HIDDEN[c.K], c.K, 10 * c.seed + g) for g, n in enumerate(sizes)]


def decided(csrs, params, C, loss):
    """(smallest top-2 margin of a non-terminal row, smallest |layer-1 pre-activation|) over the batch, in float64."""
    margin, gap = float("inf"), float("inf")
    for csr, p in zip(csrs, params):
        ref = graph_step(csr, p, C, loss)
        margin = min(margin, KR.min_margin(ref.P, p["conv2.weight"].shape[1]))
        gap = min(gap, KR.preactivation_gap([csr], p))
    return margin, gap


# ---- what float32 itself can promise
# The per-row bar of a gradient entry that cancels to below ROW_FLOOR of its tensor's largest is ROW_TOL * ROW_FLOOR *
# largest = 2e-7 * largest: three float32 ulps of the largest entry.  P is asked to P_TOL = 5e-7 only, and an error d in P
# moves an entry of db1 by about n * d * |GP| * |W2| * dinv^2 - on graphs of a handful of nodes with hundreds of hidden
# units (the terminals-only graph at K = 8 has 8 rows and 516 b1 entries) some entry is below the floor and beyond that
# bar in ANY float32 evaluation.  `f32_gradient` is such an evaluation, in numpy, with its own summation order and
# nothing of the library in it; a case is seeded so that it stays within HALF the row bar (`f32_row_ratio`).
def _mm32(rp, cl, w, M):
    f32 = np.float32
    out = np.zeros((len(rp) - 1, M.shape[1]), f32)
    for r in range(len(rp) - 1):
        acc = np.zeros(M.shape[1], f32)
        for e in range(rp[r], rp[r + 1]):
            acc = (acc + (M[cl[e]] if w is None else f32(w[e]) * M[cl[e]])).astype(f32)
        out[r] = acc
    return out


def f32_gradient(csr, p, C, loss):
    """One graph's gradient by parameter name with every intermediate rounded to float32 (numpy; rows summed in CSR order,
    matrix products as numpy orders them)."""
    f32 = np.float32
    rp, cl, vl = csr
    W1, b1, W2, b2 = (np.asarray(p[k], f32) for k in KEYS)
    K = W2.shape[1]
    dinv = (1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(f32))).astype(f32)
    T0 = (_mm32(rp, cl, vl, W1) * dinv[:, None]).astype(f32)
    H = np.maximum(((_mm32(rp, cl, None, T0) * dinv[:, None]).astype(f32) + b1).astype(f32), 0).astype(f32)
    Z0 = ((H @ W2).astype(f32) * dinv[:, None]).astype(f32)
    Z = (_mm32(rp, cl, None, Z0) * dinv[:, None] + b2).astype(f32)
    E = np.exp((Z - Z.max(1, keepdims=True)).astype(f32)).astype(f32)
    P = (E / E.sum(1, keepdims=True, dtype=f32)).astype(f32)
    onehot = np.eye(K, dtype=f32)[KR.partition(P.copy(), K)] if loss == "cut" else KR.override(P).astype(f32)
    GP = (f32(C) * _mm32(rp, cl, vl, onehot)).astype(f32)
    gz = (P * (GP - (GP * P).sum(1, keepdims=True, dtype=f32))).astype(f32)
    gy2 = _mm32(rp, cl, None, (gz * dinv[:, None]).astype(f32))
    gpre = np.where(H > 0, (gy2 @ W2.T).astype(f32) * dinv[:, None], 0).astype(f32)
    U = (_mm32(rp, cl, None, (gpre * dinv[:, None]).astype(f32)) * dinv[:, None]).astype(f32)
    return {"conv1.weight": _mm32(rp, cl, vl, U), "conv1.bias": gpre.sum(0, dtype=f32),
            "conv2.weight": ((H * dinv[:, None]).astype(f32).T @ gy2).astype(f32), "conv2.bias": gz.sum(0, dtype=f32)}


def f32_row_ratio(csrs, params, C, loss):
    """Worst stepcheck.row_error_ratio of `f32_gradient` against the float64 reference over the batch's graphs."""
    worst = 0.0
    for csr, p in zip(csrs, params):
        ref, got = graph_step(csr, p, C, loss), f32_gradient(csr, p, C, loss)
        worst = max(worst, max(stepcheck.row_error_ratio(got[k], np.asarray(ref.grads[k], np.float64), stepcheck.ROW_FLOOR)
                               for k in KEYS))
    return worst


# ---- the flat layout, restated
def flat_offsets(sizes, F, K):
    R, B = sum(sizes), len(sizes)
    return [0, R * F, R * F + B * F, R * F + B * F + B * F * K, R * F + B * (F + F * K + K)]


def pack(params):
    """The flat float32 buffer [W1 | b1 | W2 | b2] of per-graph parameter dicts."""
    return np.concatenate([np.concatenate([np.asarray(p[k], np.float32).ravel() for p in params]) for k in KEYS])
