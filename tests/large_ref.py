"""The cases of the large-graph tests (gmc_large_*: csrc/large.hip, graphs of up to 2^20 nodes) and their graph builders.

The float64 reference is tests/kway_ref.py's (`f64_step`, on stepcheck.csr_mm): nothing here restates the model.  The
graphs are built in numpy - a circulant (node i next to i +- o for every offset o), optionally with a seeded matching on top
("ring plus chords") or a hub - as GraphHandles with sorted rows; no networkx at these sizes.

The tile of csrc/large.hip is `T` = 256 rows: the shapes sit on its edges (T - 1, T, T + 1, 2T + 3, a batch whose graph
boundaries are off the tile grid and whose smaller graphs leave empty tiles), past the limits of the one-workgroup heads
(4097 and 5000 nodes at K = 3, 2500 at K = 8), on the wave-per-row path (a hub of 4200 neighbours) and past 16-bit ids
(70,000 nodes) up to the bound itself (2^20).

Preconditions, asserted on the float64 reference by tests/test_large_graphs_host.py: a case of at most 10,000 rows has no
top-2 margin below kway_ref.MARGIN, no layer-1 pre-activation within kway_ref.KINK of the relu kink, and no row whose
largest probability is within UNSATURATED = 6e-4 of 1 (the seeds are the first from 0 for which all of that holds), so the
GPU test demands the reference's partition everywhere.  The last condition is about the number format, not about a kernel:
the softmax backward of a row is p_k (gp_k - sum_j gp_j p_j), which for a saturated row is gp_c p_c (1 - p_c) + ..., and a
float32 P carries 1 - p_c to eps32 / (1 - p_c) only - 6e-8 / 6e-4 = 1e-4, half the gradient's row bar.  A hub of 4200
neighbours gets there easily (its logits are 65 times a leaf's: the star at seed 0 has 1 - p_c = 1.1e-7, one ulp, and its
hub's dLoss/dZ is then good to a factor of two in any float32 head); every other case stays above 7e-4 by itself.  The two cases above
65,535 nodes draw b1 from [0.5, 1] and W1 small enough that every pre-activation is at least 0.1 (the kink is covered by the
small cases); their partition may differ from the reference's on rows whose float64 margin is below TIE = 1e-6, at most
MAX_TIES = 8 of them, and the reference itself has at most that many such rows."""
import collections
import functools

import numpy as np

from tests import kway_ref as KR

T = 256                 # kLargeTile of csrc/large.hip
TIE = 1e-6
MAX_TIES = 8
BIG_GAP = 1e-3          # the big cases: every layer-1 pre-activation at least this far from 0
SMALL_ROWS = 10000
UNSATURATED = 6e-4      # eps32 / UNSATURATED = 1e-4: what a float32 P leaves of 1 - p_max, against ROW_TOL = 2e-4


# ---- graphs
def _csr(n, nb):
    """CSR (sorted rows, no self-loops, no repeats) from an [n, m] table of neighbour ids."""
    nb = np.sort(np.asarray(nb, np.int64), axis=1)
    keep = nb != np.arange(n)[:, None]
    keep[:, 1:] &= nb[:, 1:] != nb[:, :-1]
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(keep.sum(1), out=rowptr[1:])
    return rowptr, nb[keep]


def circulant(n, d, seed=None):
    """Node i next to i +- 1 .. i +- d // 2 (mod n); odd d: also next to i +- n // 2 (seed None: one neighbour for even n,
    two for odd n), else to the partner of a seeded matching of the nodes (the chords; with n odd one node stays without).
    Degrees are lower where offsets coincide (tiny n).  Returns (n, rowptr, col)."""
    i = np.arange(n, dtype=np.int64)
    cols = [(i + s * o) % n for o in range(1, d // 2 + 1) for s in (1, -1)]
    if d % 2:
        if seed is None:
            cols += [(i + n // 2) % n, (i - n // 2) % n]
        else:
            perm = np.random.RandomState(seed).permutation(n)
            mate = i.copy()
            half = n // 2
            mate[perm[:half]], mate[perm[half:2 * half]] = perm[half:2 * half], perm[:half]
            cols.append(mate)
    rowptr, col = _csr(n, np.stack(cols, 1))
    return n, rowptr, col


def with_hub(n, rowptr, col, hub):
    """The graph plus an edge from `hub` to every other node."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    others = np.delete(np.arange(n, dtype=np.int64), hub)
    rows = np.concatenate([rows, others, np.full(n - 1, hub, np.int64)])
    cols = np.concatenate([col, np.full(n - 1, hub, np.int64), others])
    key = np.unique(rows * n + cols)
    rows, cols = key // n, key % n
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp, cols


def star(leaves, hub):
    """`leaves` + 1 nodes, every node but `hub` next to `hub` alone."""
    n = leaves + 1
    return with_hub(n, np.zeros(n + 1, np.int64), np.zeros(0, np.int64), hub)


def edge_weights(n, rowptr, col, seed):
    """float32 weights in [0.3, 3), one per undirected edge, in CSR order (both directions carry the same value)."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    key = np.minimum(rows, col) * n + np.maximum(rows, col)
    uniq, inv = np.unique(key, return_inverse=True)
    return np.random.RandomState(100 + seed).uniform(0.3, 3.0, uniq.size).astype(np.float32)[inv]


# ---- the cases
# shape -> (graph specs, rows of conv1.weight).  A spec: ("circ", n, d, chord seed or None), ("star", leaves, hub),
# ("hubring", n, hub): a ring plus a hub; "K" / "K+1" in n: of the run's class count
SHAPES = {
    "nK": ([("circ", "K", 3, None)], 16),
    "nK1": ([("circ", "K+1", 3, None)], 16),
    "nT-1": ([("circ", T - 1, 7, 1)], 256),
    "nT": ([("circ", T, 7, 2)], 256),
    "nT+1": ([("circ", T + 1, 7, 3)], 260),
    "n2T+3": ([("circ", 2 * T + 3, 7, 4)], 516),
    "batch": ([("circ", 5, 3, None), ("circ", 700, 7, 5), ("circ", T + 1, 6, None)], 700),
    "n4097": ([("circ", 4097, 7, 6)], 4100),
    "n5000": ([("circ", 5000, 7, 7)], 5000),
    "k8n2500": ([("circ", 2500, 7, 8)], 2500),
    "star4200": ([("star", 4200, 5)], 4204),
    "hubring4200": ([("hubring", 4201, 9)], 4204),
    "d12": ([("circ", 2 * T + 3, 12, None)], 516),
    "n70000": ([("circ", 70000, 7, None)], 70000),
    "n2^20": ([("circ", 1 << 20, 4, None)], 1 << 20),
}
SHAPES["n1030"] = ([("circ", 1030, 7, 9)], 1032)   # (the comparison with gmc_kway_*: second trip of head_k's row loop)
BIG = ("n70000", "n2^20")
Case = collections.namedtuple("Case", "shape hidden K weights loss seed")
CASES = [
    Case("nK", 12, 3, "unit", "cut", 0), Case("nK", 4, 4, "real", "expected_cut", 0), Case("nK", 12, 8, "unit", "expected_cut", 0),
    Case("nK1", 12, 2, "unit", "cut", 0), Case("nK1", 4, 4, "real", "cut", 0), Case("nK1", 12, 8, "real", "expected_cut", 0),
    Case("nT-1", 12, 3, "unit", "cut", 0), Case("nT-1", 260, 4, "real", "expected_cut", 0),
    Case("nT", 12, 2, "real", "cut", 0), Case("nT", 4, 8, "unit", "expected_cut", 0),
    Case("nT+1", 12, 3, "real", "expected_cut", 0), Case("nT+1", 12, 4, "unit", "cut", 0),
    Case("n2T+3", 260, 2, "unit", "expected_cut", 0), Case("n2T+3", 12, 8, "real", "cut", 0),
    Case("batch", 12, 3, "unit", "cut", 0), Case("batch", 12, 4, "real", "expected_cut", 0), Case("batch", 4, 2, "real", "cut", 0),
    Case("n4097", 12, 3, "unit", "cut", 0), Case("n4097", 12, 3, "real", "expected_cut", 0),
    Case("n5000", 12, 3, "unit", "expected_cut", 0), Case("n5000", 4, 3, "real", "cut", 3),
    Case("k8n2500", 12, 8, "unit", "cut", 0), Case("k8n2500", 12, 8, "real", "expected_cut", 0),
    Case("star4200", 12, 3, "unit", "cut", 6), Case("hubring4200", 12, 4, "real", "expected_cut", 1),
    Case("d12", 12, 4, "unit", "cut", 0), Case("d12", 12, 3, "real", "expected_cut", 0),
    Case("n70000", 12, 4, "unit", "expected_cut", 0), Case("n2^20", 4, 3, "unit", "cut", 0),
]
# the shapes both heads run: gmc_large_* against gmc_kway_* on the same inputs (same preconditions, so S is identical)
COMPARE = [Case(shape, 12, K, weights, loss, 0)
           for shape in ("nT+1", "n1030") for K, weights in ((3, "unit"), (4, "real")) for loss in ("cut", "expected_cut")]
CC = 1.3


def case_id(c):
    return f"{c.shape}-h{c.hidden}-K{c.K}-{c.weights}-{c.loss}"


def is_big(c):
    return c.shape in BIG


def _graph(spec, K):
    if spec[0] == "star":
        return star(spec[1], spec[2])
    if spec[0] == "hubring":
        return with_hub(*circulant(spec[1], 2), spec[2])
    _kind, n, d, seed = spec
    return circulant({"K": K, "K+1": K + 1}.get(n, n), d, seed)


@functools.lru_cache(maxsize=4)
def case_csrs(c):
    """[(rowptr int32, col int32, weights float32 or None)] of a case."""
    out = []
    for i, spec in enumerate(SHAPES[c.shape][0]):
        n, rp, col = _graph(spec, c.K)
        w = edge_weights(n, rp, col, 10 * c.seed + i) if c.weights == "real" else None
        out.append((rp.astype(np.int32), col.astype(np.int32), w))
    return out


def case_handles(pkg, c):
    return [pkg.GraphHandle(len(rp) - 1, rp, col, w) for rp, col, w in case_csrs(c)]


def case_params(c):
    """Small cases: kway_ref.random_params.  Big cases: b1 in [0.5, 1] and |W1| <= 0.35 / d, which bounds every layer-1
    pre-activation below by 0.5 - 0.35 (unit weights: |dinv sum dinv sum W1| <= d * max|W1|); conv2.weight uniform in
    [-4, 4] with its columns made orthogonal to b1, so that the classes are decided by what differs between the rows and
    not by the bias all rows share (about a third of the nodes per class, margins spread over [0, 0.5])."""
    N = SHAPES[c.shape][1]
    if not is_big(c):
        return KR.random_params(N, c.hidden, c.K, c.seed)
    d = SHAPES[c.shape][0][0][2]
    rng = np.random.RandomState(2000 + c.seed)
    W1 = rng.uniform(-0.35 / d, 0.35 / d, (N, c.hidden)).astype(np.float32)
    b1 = rng.uniform(0.5, 1.0, c.hidden).astype(np.float32)
    W2 = rng.uniform(-4.0, 4.0, (c.hidden, c.K))
    W2 -= np.outer(b1, b1 @ W2) / float(b1 @ b1)
    return {"conv1.weight": W1, "conv1.bias": b1, "conv2.weight": W2.astype(np.float32),
            "conv2.bias": (0.1 * rng.standard_normal(c.K)).astype(np.float32)}


def reference(c, S_got=None):
    """kway_ref.f64_step of the case at C = CC (hard loss of a big case: of the partition the device chose)."""
    return KR.f64_step(case_csrs(c), case_params(c), CC, c.loss, S_got=S_got, tie=TIE)


def rows_under(P, K, width):
    """Non-terminal rows (of one graph's P) whose top-2 margin is below `width`."""
    srt = np.sort(np.asarray(P, np.float64)[K:], axis=1)
    return int(((srt[:, -1] - srt[:, -2]) < width).sum())
