"""GPU tests of the semidefinite relaxation (csrc/sdp.hip through maxcut.sdp_relax / sdp_round / solve_sdp).  The rules of
include/gcnmaxcut_sdp.h are restated in tests/sdp_ref.py; V, the bits of value and every plane's bytes are compared with
it byte for byte - no assertion on them has a tolerance.

The small graphs: a 3-node path, 7-regular graphs of 70 and 300 nodes (a colour class crosses a 4-, 8- and 16-node tile
at every rank), a star with 70 leaves (a row of more than 64 entries), and one batch of all four.  The reference is
computed on the batch, once per case; every graph is also run alone and compared with its rows of the batch's result,
which is the batch independence and puts the single graphs against the reference too.

Measured on the MI355X: the file's 24 tests take 5.8 s alone; the slowest is the cycle of 2^20 nodes (2.0 s, most of it
the numpy restatement of 2^26 hashes), then the first byte test at 0.3 s.
"""
import functools
import itertools

import networkx as nx
import numpy as np
import pytest
import torch

from tests import sdp_ref as S
from tests import util

pytestmark = pytest.mark.gpu

RANKS = (16, 32, 64)
SWEEPS = (0, 1, 3)
WEIGHTS = ("unit", "signed", "real")
COSTS = (None, "integer", "real", "barrier")
KEYS = np.array([0x9E3779B97F4A7C15, 0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001], np.uint64)
PLANES = 8


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def weighted(g, kind, seed):
    g = nx.Graph(g)
    rng = np.random.RandomState(seed)
    for u, v in sorted(g.edges()):
        if kind == "signed":
            g[u][v]["weight"] = float(rng.choice([-1.0, 1.0]))
        elif kind == "real":   # full-mantissa float32
            g[u][v]["weight"] = float(np.float32(rng.uniform(0.1, 2.0)))
    return g


@functools.lru_cache(maxsize=None)
def small_graphs(kind):
    star = nx.star_graph(70)                                   # node 0: a row of 70 entries
    gs = (nx.path_graph(3), nx.random_regular_graph(7, 70, seed=70), nx.random_regular_graph(7, 300, seed=300), star)
    return tuple(weighted(g, kind, 11 + i) for i, g in enumerate(gs))


def handles(pkg, graphs):
    return [pkg.graph.from_networkx(g) for g in graphs]


def cost_of(kind, R, seed=3):
    rng = np.random.RandomState(seed)
    if kind is None:
        return None
    if kind == "integer":
        return rng.randint(-3, 4, (R, 2)).astype(np.float32)
    if kind == "real":
        return rng.uniform(-2.0, 2.0, (R, 2)).astype(np.float32)
    c = np.zeros((R, 2), np.float32)                           # a barrier: every third node is kept out of one class
    rows = np.arange(0, R, 3)
    c[rows, rng.randint(0, 2, rows.size)] = 1e6
    return c


def dev_keys(batch, keys):
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(batch.device)


def gpu_relax(pkg, batch, keys, rank, sweeps, terminals, cost, V=None):
    c = None if cost is None else torch.from_numpy(cost).to(batch.device)
    V, value = pkg.maxcut._sdp_relax_keys(batch, None if V is not None else dev_keys(batch, keys), rank, sweeps, terminals,
                                          c, V)
    return V, value


def gpu_round(pkg, batch, V, keys, first, planes, terminals):
    return pkg.maxcut._sdp_round_keys(batch, V, dev_keys(batch, keys), first, planes, terminals)


def same_bytes(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("terminals", (False, True))
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("rank", RANKS)
def test_bytes_of_V_value_and_planes(pkg, rank, weights, terminals):
    graphs = small_graphs(weights)
    hs = handles(pkg, graphs)
    batch = pkg.GraphBatch(hs)
    h = batch.host
    singles = [pkg.GraphBatch([x]) for x in hs]
    order = S.order_of(pkg, h, terminals)
    colours = S.colour_rows(h, terminals, *order)
    goff = [int(x) for x in h.goff]
    for kind in COSTS:
        cost = cost_of(kind, h.R)
        V = S.init(h, rank, terminals, KEYS)
        done = 0
        for sweeps in SWEEPS:
            for _ in range(sweeps - done):
                for rows in colours:
                    S.visit(h, V, rows, cost)
            done = sweeps
            value = S.value(h, V, cost)
            planes = S.round_planes(h, rank, terminals, V, KEYS, 5, PLANES)
            gV, gvalue = gpu_relax(pkg, batch, KEYS, rank, sweeps, terminals, cost)
            gplanes = gpu_round(pkg, batch, gV, KEYS, 5, PLANES, terminals)
            assert same_bytes(gV, V), (kind, sweeps, "V", float(np.abs(gV.cpu().numpy() - V).max()))
            assert same_bytes(gvalue, value), (kind, sweeps, "value", gvalue.cpu().numpy(), value)
            assert same_bytes(gplanes, planes), (kind, sweeps, "planes")
            assert np.isfinite(value).all() and set(np.unique(planes)) <= {0, 1}
            # every graph alone: its rows of the batch's result
            for g, one in enumerate(singles):
                lo, hi = goff[g], goff[g + 1]
                c1 = None if cost is None else cost[lo:hi]
                sV, svalue = gpu_relax(pkg, one, KEYS[g:g + 1], rank, sweeps, terminals, c1)
                splanes = gpu_round(pkg, one, sV, KEYS[g:g + 1], 5, PLANES, terminals)
                assert torch.equal(sV, gV[lo:hi]) and torch.equal(svalue.view(torch.int32), gvalue[g:g + 1].view(torch.int32))
                assert torch.equal(splanes, gplanes[:, lo:hi]), (kind, sweeps, g)


def test_warm_start_plane_windows_and_zero_cost(pkg):
    batch = pkg.GraphBatch(handles(pkg, small_graphs("real")))
    cost = cost_of("real", batch.R)
    for rank, terminals in itertools.product(RANKS, (False, True)):
        whole, value = gpu_relax(pkg, batch, KEYS, rank, 5, terminals, cost)
        first, _ = gpu_relax(pkg, batch, KEYS, rank, 2, terminals, cost)
        kept = first.clone()
        second, value2 = gpu_relax(pkg, batch, None, rank, 3, terminals, cost, V=first)
        assert torch.equal(first, kept)                                     # the state handed in is not modified
        assert torch.equal(second, whole) and torch.equal(value2.view(torch.int32), value.view(torch.int32))
        planes = gpu_round(pkg, batch, whole, KEYS, 0, 64, terminals)
        halves = torch.cat([gpu_round(pkg, batch, whole, KEYS, 0, 32, terminals),
                            gpu_round(pkg, batch, whole, KEYS, 32, 32, terminals)])
        assert torch.equal(planes, halves)
        assert 0 < int(planes.sum()) < planes.numel()
        zero, zvalue = gpu_relax(pkg, batch, KEYS, rank, 3, terminals, np.zeros((batch.R, 2), np.float32))
        none, nvalue = gpu_relax(pkg, batch, KEYS, rank, 3, terminals, None)
        assert torch.equal(zero, none) and torch.equal(zvalue.view(torch.int32), nvalue.view(torch.int32))
    # the public calls: seeded keys, the default rank, planes of the public rounding are windows of the same planes
    V, value = pkg.maxcut.sdp_relax(batch, sweeps=2, seed=9)
    assert tuple(V.shape) == (batch.R, 32)                                  # sqrt(2 * 300) + 1 = 25.5
    again, _ = pkg.maxcut.sdp_relax(batch, sweeps=1, seed=9, V=pkg.maxcut.sdp_relax(batch, sweeps=1, seed=9)[0])
    assert torch.equal(V, again)
    assert torch.equal(pkg.maxcut.sdp_round(batch, V, 10, seed=9)[:4], pkg.maxcut.sdp_round(batch, V, 4, seed=9))
    norms = V.double().norm(dim=1)
    assert float((norms - 1).abs().max()) < 1e-6


def circulant(pkg, n, offsets):
    u = np.arange(n, dtype=np.int64)
    src = np.concatenate([u for _ in offsets])
    dst = np.concatenate([(u + d) % n for d in offsets])
    return pkg.graph.from_edge_index(np.stack([src, dst]), n, pairs="once")


def test_a_4200_node_circulant(pkg):
    """Beyond one workgroup's graphs and several 256-row tiles of the value: ranks 16 and 64, two sweeps."""
    batch = pkg.GraphBatch([circulant(pkg, 4200, (1, 2, 5))])
    key = KEYS[1:2]
    for rank, terminals in ((16, True), (64, False)):
        V, value = S.relax(pkg, batch.host, rank, terminals, None, key, 2)
        gV, gvalue = gpu_relax(pkg, batch, key, rank, 2, terminals, None)
        assert same_bytes(gV, V) and same_bytes(gvalue, value), (rank, gvalue.cpu().numpy(), value)
        assert same_bytes(gpu_round(pkg, batch, gV, key, 0, 3, terminals), S.round_planes(batch.host, rank, terminals, V, key, 0, 3))


def test_a_cycle_of_2_to_the_20_nodes_at_rank_64(pkg):
    """The grid limits: one colour of the even cycle has 2^19 nodes, 131,072 four-node tiles in the x dimension."""
    n = 1 << 20
    batch = pkg.GraphBatch([circulant(pkg, n, (1,))])
    assert batch.refine_classes(2, False) == 2
    key = KEYS[:1]
    V, value = S.relax(pkg, batch.host, 64, False, None, key, 1)
    gV, gvalue = gpu_relax(pkg, batch, key, 64, 1, False, None)
    assert same_bytes(gV, V) and same_bytes(gvalue, value), (gvalue.cpu().numpy(), value)
    planes = gpu_round(pkg, batch, gV, key, 7, 2, False)
    assert same_bytes(planes, S.round_planes(batch.host, 64, False, V, key, 7, 2))


# ---- the solver --------------------------------------------------------------------------------------------------------------
def brute_force(g, cost):
    """The optimum of cut(S) - sum_v cost[v][S_v] over all 2^n partitions, in float64."""
    n = g.number_of_nodes()
    S_all = (np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1
    obj = np.zeros(1 << n)
    for u, v, w in g.edges(data="weight", default=1):
        obj += (S_all[:, u] != S_all[:, v]) * float(w)
    if cost is not None:
        obj -= np.where(S_all == 0, cost[None, :, 0], cost[None, :, 1]).sum(axis=1)
    return float(obj.max())


@pytest.mark.parametrize("with_cost", (False, True))
def test_solve_sdp_reaches_the_optimum_of_small_graphs(pkg, with_cost):
    sizes = (10, 11, 12, 13, 14, 10, 12, 14)
    graphs = [util.near_regular(n, 3 + i % 2, 500 + i, attrs=False) for i, n in enumerate(sizes)]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ei = np.concatenate([np.array([(u + ptr[i], v + ptr[i]) for u, v in g.edges()], np.int64).T
                         for i, g in enumerate(graphs)], axis=1)
    cost = np.random.RandomState(8).uniform(-1, 1, (int(ptr[-1]), 2)).astype(np.float32) if with_cost else None
    res = pkg.maxcut.solve_sdp(ei, ptr, pairs="once", seed=1, node_cost=cost)
    part = res.partition.cpu().numpy()
    assert part.shape == (int(ptr[-1]),) and set(np.unique(part)) <= {0, 1}
    cut, rounded, relaxed = (t.cpu().numpy().astype(np.float64) for t in (res.cut, res.rounded_cut, res.relaxed_value))
    for i, g in enumerate(graphs):
        lo, hi = int(ptr[i]), int(ptr[i + 1])
        c = None if cost is None else cost[lo:hi].astype(np.float64)
        mine = sum(float(part[lo + u] != part[lo + v]) for u, v in g.edges())
        if c is not None:
            spent = float(c[np.arange(hi - lo), part[lo:hi]].sum())
            assert abs(float(res.node_cost_sum[i]) - spent) < 1e-4
            mine -= spent
        best = brute_force(g, c)
        print(i, sizes[i], "optimum", best, "cut", cut[i], "rounded", rounded[i], "relaxed", relaxed[i])
        assert abs(cut[i] - mine) < 1e-4                                     # cut is the recount of partition
        assert abs(cut[i] - best) < 1e-4, (i, cut[i], best)
        assert rounded[i] <= cut[i] + 1e-4
    assert (res.node_cost_sum is None) == (cost is None)


def test_solve_sdp_beyond_one_workgroup(pkg):
    """4,200 nodes: scoring, search and pick go through the large annealing; with a cost the door refuses."""
    n = 4200
    u = np.arange(n, dtype=np.int64)
    ei = np.stack([np.concatenate([u, u, u]), np.concatenate([(u + 1) % n, (u + 2) % n, (u + 5) % n])])
    res = pkg.maxcut.solve_sdp(ei, num_nodes=n, pairs="once", sweeps=10, planes=8, anneal_sweeps=5, max_descent_sweeps=20)
    part = res.partition.cpu().numpy()
    recount = float((part[ei[0]] != part[ei[1]]).sum())
    assert float(res.cut[0]) == recount and float(res.rounded_cut[0]) <= recount <= 3 * n
    assert 0 < float(res.relaxed_value[0]) <= 3 * n        # every edge's term (1 - v_u . v_v) / 2 is at most 1
    with pytest.raises(NotImplementedError, match="node_cost"):
        pkg.maxcut.solve_sdp(ei, num_nodes=n, pairs="once", node_cost=np.zeros((n, 2), np.float32))
