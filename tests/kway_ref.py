"""Float64 restatement of one training step of the K-class model (number_classes K in 2..8; include/gcnmaxcut.h,
gmc_kway_*), in numpy, and the cases the GPU tests run.

    Pt   = P with rows 0..K-1 replaced by e_0..e_{K-1}             (override_fixed_nodes, straight-through)
    S    = row-argmax of P, first maximum wins, rows 0..K-1 forced to their own class
    hard:    loss = -C * cut(S),                                   GP = C * A_val @ onehot_K(S)
    relaxed: loss = -C/2 * sum_u sum_{v in N(u)} w_uv (1 - Pt_u . Pt_v),   GP_u = C * sum_{v in N(u)} w_uv Pt_v

The forward and the backward around it are tests/stepcheck.py's (width-agnostic).  At K = 3 every function here is the
3-wide one of stepcheck / tests/expected_cut_ref.py, value for value (tests/test_kway_host.py).

The cases (`CASES`) live here so that the CPU test can assert, on this float64 reference, what lets the GPU test demand
identical partitions everywhere: no top-2 margin of a non-terminal row below `MARGIN`, no layer-1 pre-activation within
`KINK` of the relu kink."""
import collections

import numpy as np

from tests import stepcheck, util
from tests.stepcheck import KEYS

MARGIN = 1e-5
KINK = 1e-6


def partition(P, K=None):
    """The decode: argmax per row (first maximum), the first min(K, n) rows forced to their own class."""
    P = np.asarray(P)
    K = P.shape[1] if K is None else K
    S = P.argmax(1)
    k = min(K, len(S))
    S[:k] = np.arange(k)
    return S


def override(P):
    Pt = np.array(P, np.float64)
    k = min(Pt.shape[1], Pt.shape[0])
    Pt[:k] = np.eye(Pt.shape[1])[:k]
    return Pt


def _edges(rp, cl, vl):
    rp, cl = np.asarray(rp), np.asarray(cl)
    w = np.ones(len(cl)) if vl is None else np.asarray(vl, np.float64)
    return rp, cl, w, np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def hard_loss_and_gp(rp, cl, vl, S, K, C=1.0):
    """(-C * cut(S), GP [n,K] = C * A_val @ onehot_K(S)); vl None = unit weights."""
    rp, cl, w, rows = _edges(rp, cl, vl)
    S = np.asarray(S).astype(np.int64)
    return -C * 0.5 * float((w * (S[rows] != S[cl])).sum()), C * stepcheck.csr_mm(rp, cl, w, np.eye(K)[S])


def relaxed_loss_and_gp(rp, cl, vl, P, C=1.0):
    """(loss, GP [n,K]) of the relaxed loss at probabilities P [n,K]."""
    rp, cl, w, rows = _edges(rp, cl, vl)
    Pt = override(P)
    dots = (Pt[rows] * Pt[cl]).sum(1)
    return -C * 0.5 * float((w * (1.0 - dots)).sum()), C * stepcheck.csr_mm(rp, cl, w, Pt)


def min_margin(P, K=None):
    """Smallest top-2 margin of P over the non-terminal rows (inf when every row is a terminal)."""
    P = np.asarray(P, np.float64)
    K = P.shape[1] if K is None else K
    free = np.sort(P[K:], axis=1)
    return float((free[:, -1] - free[:, -2]).min()) if len(free) else float("inf")


def near_tie_rows(P_ref, s_got, tie, where=None):
    """stepcheck.near_tie_rows for K columns: rows whose decode differs from the reference's, each of which must have a
    top-2 margin below `tie` in the reference."""
    diff = np.nonzero(np.asarray(s_got) != partition(P_ref))[0]
    if diff.size:
        srt = np.sort(np.asarray(P_ref, np.float64)[diff], axis=1)
        assert (srt[:, -1] - srt[:, -2]).max() < tie, (where, diff, srt)
    return diff.size


def total_weight(csrs):
    return sum(0.5 * float(len(cl) if vl is None else np.abs(np.asarray(vl, np.float64)).sum()) for _rp, cl, vl in csrs)


def f64_step(csrs, params, C=1.0, loss="cut", S_got=None, tie=1e-6):
    """Float64 reference of one step of the batch: stepcheck.Ref(P, per-graph loss in float64, summed gradient by
    parameter name, near ties).  Hard loss: of the reference's own partition, or (S_got given) of the device's, which
    may differ from it on rows within `tie` of a tie only."""
    W = [np.asarray(params[k], np.float64) for k in KEYS]
    K = W[2].shape[1]
    grad, Ps, losses, near, off = None, [], [], 0, 0
    for i, (rp, cl, vl) in enumerate(csrs):
        n = len(rp) - 1
        f = stepcheck.f64_forward_sparse(rp, cl, vl, *W)
        if loss == "cut":
            S = partition(f["P"], K)
            if S_got is not None:
                S = np.asarray(S_got[off:off + n]).astype(np.int64)
                near += near_tie_rows(f["P"], S, tie, i)
            value, GP = hard_loss_and_gp(rp, cl, vl, S, K, C)
        else:
            assert loss == "expected_cut", loss
            value, GP = relaxed_loss_and_gp(rp, cl, vl, f["P"], C)
        g = stepcheck.f64_backward_sparse(f, GP, W[2], W[0].shape[0])
        grad = g if grad is None else {k: grad[k] + g[k] for k in grad}
        Ps.append(f["P"])
        losses.append(value)
        off += n
    return stepcheck.Ref(np.concatenate(Ps), np.asarray(losses), stepcheck.named(grad), near)


def preactivation_gap(csrs, params):
    """Smallest |layer-1 pre-activation| of the batch in float64: the distance of the nearest unit to the relu kink."""
    W = [np.asarray(params[k], np.float64) for k in KEYS]
    return min(float(np.abs(stepcheck.f64_forward_sparse(rp, cl, vl, *W)["pre"]).min()) for rp, cl, vl in csrs)


# ---- the cases of tests/test_gpu_kway.py
# shape -> (graph specs (n, d, seed), hidden width, rows of conv1.weight); "K" in n: the class count of the run
SHAPES = {
    "nK": ([("K", 3, 1)], 16, 64),                                   # every node is a terminal
    "nK1": ([("K+1", 3, 2)], 16, 64),                                # one free node
    "n65": ([(65, 7, 3)], 16, 128),                                  # crosses one wave / one 64-row tile
    "n1030": ([(1030, 7, 4)], 16, 1040),                             # second trip of the head's row loop
    "batch3": ([(60, 7, 5), (97, 6, 6), (5, 3, 7)], 16, 128),        # non-zero goff, mixed sizes
    "h4": ([(70, 7, 8)], 4, 128),                                    # column tail of a wave
    "h12": ([(70, 7, 9)], 12, 128),
    "h260": ([(70, 7, 10)], 260, 128),                               # more than one wave of float4 columns
    "h516": ([(70, 7, 11)], 516, 128),                               # second column slice of the hidden backward
}
Case = collections.namedtuple("Case", "shape K weights loss seed")
# every shape, every K of {2, 4, 5, 8} and both losses at least twice; unit and real-valued weights.  The seeds are the
# first (from 0) for which the precondition above holds (tests/test_kway_host.py asserts it).
CASES = [
    Case("nK", 4, "unit", "cut", 0), Case("nK", 8, "real", "expected_cut", 0), Case("nK", 5, "unit", "expected_cut", 0),
    Case("nK1", 2, "unit", "cut", 0), Case("nK1", 5, "real", "cut", 0), Case("nK1", 8, "unit", "expected_cut", 0),
    Case("n65", 2, "real", "expected_cut", 1), Case("n65", 5, "unit", "cut", 0), Case("n65", 8, "real", "cut", 1),
    Case("n1030", 4, "unit", "cut", 0), Case("n1030", 8, "real", "expected_cut", 0),
    Case("batch3", 2, "unit", "expected_cut", 0), Case("batch3", 4, "real", "cut", 0), Case("batch3", 5, "unit", "cut", 0),
    Case("h4", 2, "real", "cut", 0), Case("h4", 5, "unit", "expected_cut", 0),
    Case("h12", 4, "unit", "expected_cut", 0), Case("h12", 8, "real", "cut", 0),
    Case("h260", 2, "unit", "cut", 0), Case("h260", 8, "real", "expected_cut", 0),
    Case("h516", 4, "real", "expected_cut", 0), Case("h516", 5, "unit", "cut", 0),
]


def case_id(c):
    return f"{c.shape}-K{c.K}-{c.weights}-{c.loss}"


def case_graphs(c):
    """The networkx graphs of a case: near-regular, unit weights or real-valued float32 weights in [0.3, 3)."""
    graphs = []
    for n, d, seed in SHAPES[c.shape][0]:
        n = {"K": c.K, "K+1": c.K + 1}.get(n, n)
        g = util.near_regular(max(n, 3), d, seed)          # (a GraphBatch takes graphs of at least 3 nodes)
        if c.weights == "real":
            rng = np.random.RandomState(100 + seed)
            for u, v in g.edges():
                g[u][v]["weight"] = float(np.float32(rng.uniform(0.3, 3.0)))
        graphs.append(g)
    return graphs


def random_params(N, F, K, seed):
    """float32 parameters by name: uniform weights wide enough for decided rows, small normal biases (numpy: the same
    values with and without a GPU)."""
    rng = np.random.RandomState(1000 + seed)
    return {"conv1.weight": rng.uniform(-0.3, 0.3, (N, F)).astype(np.float32),
            "conv1.bias": (0.05 * rng.standard_normal(F)).astype(np.float32),
            "conv2.weight": rng.uniform(-1.0, 1.0, (F, K)).astype(np.float32),
            "conv2.bias": (0.1 * rng.standard_normal(K)).astype(np.float32)}


def case_params(c):
    _specs, hidden, N = SHAPES[c.shape]
    return random_params(N, hidden, c.K, c.seed)


def csr_of_handle(h):
    return h.rowptr, h.col, h.weight


# the batch on which K = 3 runs through gmc_kway_train_fwd_bwd and through the fused 3-way step (decided rows as well)
def three_way_graphs():
    return [util.near_regular(60, 7, 21), util.near_regular(97, 6, 22), util.near_regular(130, 12, 23)]


def three_way_params():
    return random_params(160, 32, 3, 7)
