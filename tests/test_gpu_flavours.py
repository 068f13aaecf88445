"""GPU flavour matrix: every reachable instantiation of the LDS-tiled kernels (tests/test_lds_flavours.py: MATRIX, the
census that pins it) at both ends of its n_max window, against a float64 restatement of the training step.

Each case builds the batch of its kind (the n_max graph beside a smaller one, so that clamped passes and rows past a
graph's n run; a one-graph gmc_train_step_f32 for the head kinds), checks that the batch has the table width / live
slots / overflow lists of its kind, that the query gives the kind's words, and that the probe saw exactly those words
launched - the fused sequence, then (no overflow lists) the gmc_set_fuse(0) sequence.  Workspace and gradient are
poisoned first.  P, the partition, the per-graph loss and the full gradient are compared with the float64 step; the
gradient per parameter row (util.row_error_ratio), never looser than the 1e-4 x max bar of the oracle tests.

Measured on the MI355X over the whole matrix (194 steps, worst case): P 6.8e-8 absolute (w16_val, n = 13); gradient
row ratio 2.2e-5 (w8_val, n = 256, both sequences).  The bars below are at most 10x those.
"""
import networkx as nx
import numpy as np
import pytest
import torch

from tests import util
from tests.test_lds_flavours import BOUNDARIES, KINDS, MATRIX, PER_CASES, expected_words, name

pytestmark = pytest.mark.gpu

P_TOL = 5e-7            # absolute, probabilities
ROW_TOL = 2e-4          # per parameter row, relative to the row's own magnitude
ROW_FLOOR = 1e-3        # ... or this fraction of the tensor's largest entry, for rows that are (near) zero
ORACLE_BAR = 1e-4       # the oracle tests' bar (x max(1, max|grad|)): the per-row bar is never looser
BETA1 = 0.9
KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")
FLAV = {"fwd1_fused", "bwd1_fused", "gather_w1", "agg_fwd", "agg_bwd", "dw1"}


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def near_regular(n, d, seed):
    """d-regular on n nodes; when n * d is odd, a d-regular graph on n + 1 nodes without its last node."""
    d = min(d, n - 1)
    m = n if n * d % 2 == 0 else n + 1
    g = nx.random_regular_graph(d, m, seed=seed)
    if m > n:
        g.remove_node(n)
    out = nx.Graph()
    out.add_nodes_from(range(n))
    out.add_edges_from(g.edges)
    nx.set_edge_attributes(out, 1, "weight")
    nx.set_edge_attributes(out, 1, "capacity")
    return out


def add_hub(g, hub_degree, seed, hub=5):
    rng = np.random.RandomState(seed)
    for v in rng.permutation(g.number_of_nodes()):
        if g.degree(hub) >= hub_degree:
            break
        if int(v) != hub and not g.has_edge(hub, int(v)):
            g.add_edge(hub, int(v), weight=1, capacity=1)
    assert g.degree(hub) == hub_degree


def graphs_of(kind, n, count, seed):
    W, slots, val, ovf, one, d, _n = KINDS[kind]
    big = near_regular(n, d, seed)
    graphs = {0: big}
    if ovf:
        add_hub(big, W + 4, seed)     # one overflow block
    if count == 2:
        n2 = max(3, min(n - 1, 2 * n // 3))
        if kind == "w8_ovf":
            n2 = max(n2, 200 - n)     # one long row per 200 rows keeps the 8-slot table
        graphs[1] = near_regular(n2, d, seed + 1)
    for i in range(2, count):         # (slice-group cases) many small graphs
        graphs[i] = near_regular(12, 3, seed + i)
    if val:
        rng = np.random.RandomState(seed)
        for g in graphs.values():
            for u, v in g.edges():
                g[u][v]["weight"] = int(rng.randint(1, 4))
    return graphs


def window(kind, n):
    return next((fs, acc) for fs, acc, lo, hi in BOUNDARIES[kind] if lo <= n <= hi)


def run_case(pkg, kind, n, hidden, count, per=1, stats=None):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    W, slots, val, ovf, one, _d, _n = KINDS[kind]
    N = 1000 if n <= 1000 else 1024
    seed = 1000 * hidden + n
    graphs = graphs_of(kind, n, count, seed)
    terms = {i: [g.number_of_nodes() - k for k in (1, 2, 3)] for i, g in graphs.items()}   # (never two of 0, 1, 2)
    ds = util.dataset_of(graphs, terms, N)
    torch.manual_seed(seed)
    net, _embed, _opt = T.setup_model_and_optimizer(T.TrainingConfig(n_nodes=N, hidden_dim=hidden))
    params = util.np_params(net.state_dict())
    eng = net.engine()
    items = list(ds.values())
    batch = pkg.GraphBatch([it[0] for it in items], [it[0].edge_values(it[1]) for it in items], eng.device)
    h = batch.host
    assert (h.n_max, h.ell_width, h.ell_slots, h.ovf_ptr is not None, h.vals is not None) == (n, W, slots, ovf, val)
    if ovf:
        assert h.ovf_max_blocks == 1
    want = expected_words(kind, *window(kind, n), per=per)
    query = pkg.hip.lds_flavours(batch.c, eng.Fp, one)
    assert query == want, ([name(w) for w in query], [name(w) for w in want])
    csrs = util.csrs_of(ds)
    lib = pkg.hip.load()
    seqs = [(1, want[:2])] + ([] if ovf or one else [(0, want[2:])])
    for fuse, words in seqs:
        prev = lib.gmc_set_fuse(fuse)
        try:
            eng._workspace(batch, True)              # sized, then poisoned (all-ones bytes = NaN)
            eng._ws.fill_(255)
            eng.grad.fill_(float("nan"))
            if one:
                eng.m.zero_(); eng.v.zero_()         # zero Adam moments: m = (1 - beta1) g after the step
                with pkg.hip.Probe(64) as probe:
                    P, S, loss = eng.train_step(batch, 1e-3)
                grads = {k: v.cpu().numpy() / (1.0 - BETA1) for k, v in eng.views(eng.m).items()}
            else:
                with pkg.hip.Probe(64) as probe:
                    P, S, loss = eng.train_fwd_bwd(batch)
                grads = {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()}
        finally:
            lib.gmc_set_fuse(prev)
        got = [w for w in probe.flavours if w]
        assert got == words, ([name(w) for w in got], [name(w) for w in words])
        assert all((w != 0) == (t in FLAV) for (t, _ms), w in zip(probe.records, probe.flavours)), probe.records
        P, S, loss = P.cpu().numpy(), S.cpu().numpy(), loss.cpu().numpy()
        P64, loss64, g64 = util.f64_step(csrs, params, S)
        p_err = float(np.abs(P - P64).max())
        assert p_err <= P_TOL, (kind, n, hidden, fuse, p_err)
        assert np.array_equal(loss, loss64.astype(np.float32)), (loss, loss64)
        worst = 0.0
        for k, key in zip(("W1", "b1", "W2", "b2"), KEYS):
            g, r = grads[key], g64[k]
            assert np.isfinite(g).all(), key
            ratio = util.row_error_ratio(g, r, ROW_FLOOR)
            bar = ORACLE_BAR * max(1.0, float(np.abs(r).max()))
            assert np.abs(g - r).max() <= bar, (kind, n, hidden, fuse, key)
            assert ratio <= ROW_TOL, (kind, n, hidden, fuse, key, ratio)
            worst = max(worst, ratio)
        if stats is not None:
            stats.append((kind, n, hidden, fuse, p_err, worst))
            print(f"flavour case {kind} n={n} hidden={hidden} fuse={fuse}: P {p_err:.2e} rows {worst:.2e}")


@pytest.mark.parametrize("kind,n,hidden,count", MATRIX, ids=[f"{k}-n{n}-h{h}" for k, n, h, c in MATRIX])
def test_flavour_matrix(pkg, kind, n, hidden, count):
    run_case(pkg, kind, n, hidden, count, stats=[])


@pytest.mark.parametrize("kind,n,hidden,count,per", PER_CASES, ids=[f"per{p}" for *_x, p in PER_CASES])
def test_slice_group_classes(pkg, kind, n, hidden, count, per):
    run_case(pkg, kind, n, hidden, count, per=per, stats=[])
