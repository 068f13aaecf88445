"""GPU flavour matrix: every reachable instantiation of the LDS-tiled kernels (tests/test_lds_flavours.py: MATRIX, the
census that pins it) at both ends of its n_max window, against a float64 restatement of the training step.

Each case builds the batch of its kind (the n_max graph beside a smaller one, so that clamped passes and rows past a
graph's n run; a one-graph gmc_train_step_f32 for the head kinds), checks that the batch has the table width / live
slots / overflow lists of its kind, that the query gives the kind's words, and that the probe saw exactly those words
launched - the fused sequence, then (no overflow lists) the gmc_set_fuse(0) sequence.  Workspace and gradient are
poisoned first.  P, the partition, the per-graph loss and the full gradient are compared with the float64 step; the
gradient per parameter row (stepcheck.row_error_ratio), never looser than the 1e-4 x max bar of the oracle tests.

Measured on the MI355X over the whole matrix (194 steps, worst case): P 6.8e-8 absolute (w16_val, n = 13); gradient
row ratio 2.2e-5 (w8_val, n = 256, both sequences).  The bars below are at most 10x those.
"""
import numpy as np
import pytest
import torch

from tests import stepcheck, util
from tests.stepcheck import ORACLE_BAR, P_TOL, ROW_FLOOR, ROW_TOL
from tests.test_lds_flavours import BOUNDARIES, KINDS, MATRIX, PER_CASES, expected_words, name

pytestmark = pytest.mark.gpu

FLAV = {"fwd1_fused", "bwd1_fused", "gather_w1", "agg_fwd", "agg_bwd", "dw1"}


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def graphs_of(kind, n, count, seed):
    W, slots, val, ovf, one, d, _n = KINDS[kind]
    big = util.near_regular(n, d, seed)
    graphs = {0: big}
    if ovf:
        util.add_hub(big, W + 4, seed)     # one overflow block
    if count == 2:
        n2 = max(3, min(n - 1, 2 * n // 3))
        if kind == "w8_ovf":
            n2 = max(n2, 200 - n)     # one long row per 200 rows keeps the 8-slot table
        graphs[1] = util.near_regular(n2, d, seed + 1)
    for i in range(2, count):         # (slice-group cases) many small graphs
        graphs[i] = util.near_regular(12, 3, seed + i)
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
    batch = util.batch_of(pkg, eng, ds)
    h = batch.host
    assert (h.n_max, h.ell_width, h.ell_slots, h.ovf_ptr is not None, h.vals is not None) == (n, W, slots, ovf, val)
    if ovf:
        assert h.ovf_max_blocks == 1
    want = expected_words(kind, *window(kind, n), per=per)
    query = pkg.hip.lds_flavours(batch.c, eng.Fp, one)
    assert query == want, ([name(w) for w in query], [name(w) for w in want])
    csrs = util.csrs_of(ds)
    seqs = [(1, want[:2])] + ([] if ovf or one else [(0, want[2:])])
    for fuse, words in seqs:
        got = stepcheck.run_step(pkg, eng, batch, fuse=fuse, entry="train_step" if one else "train_fwd_bwd")
        flav = [w for w in got.flavours if w]
        assert flav == words, ([name(w) for w in flav], [name(w) for w in words])
        assert all((w != 0) == (t in FLAV) for t, w in zip(got.tags, got.flavours)), got.tags
        res = stepcheck.compare_step(got, stepcheck.f64_step(csrs, params, got.S), p_tol=P_TOL, grad_bar=ORACLE_BAR,
                                     row_tol=ROW_TOL, row_floor=ROW_FLOOR, what=(kind, n, hidden, fuse))
        if stats is not None:
            stats.append((kind, n, hidden, fuse, res["p_err"], res["rows"]))
            print(f"flavour case {kind} n={n} hidden={hidden} fuse={fuse}: P {res['p_err']:.2e} rows {res['rows']:.2e}")


@pytest.mark.parametrize("kind,n,hidden,count", MATRIX, ids=[f"{k}-n{n}-h{h}" for k, n, h, c in MATRIX])
def test_flavour_matrix(pkg, kind, n, hidden, count):
    run_case(pkg, kind, n, hidden, count, stats=[])


@pytest.mark.parametrize("kind,n,hidden,count,per", PER_CASES, ids=[f"per{p}" for *_x, p in PER_CASES])
def test_slice_group_classes(pkg, kind, n, hidden, count, per):
    run_case(pkg, kind, n, hidden, count, per=per, stats=[])
