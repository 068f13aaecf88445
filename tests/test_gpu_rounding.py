"""GPU tests of the rounding by conditional expectations (gmc_round_conditional_f32 and its Python API) against the
CPU restatement in tests/rounding_ref.py: class bytes and sweep counts byte for byte at descent 0 and 100, cuts (unit
weights exact, fp32 weights 1e-5 relative), the expected cut against float64, the guarantee, K = 3 against
gmc_refine_local_f32, reproducibility, batch independence, the optional outputs, round_dataset and decode_dataset."""
import ctypes as C
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import rounding_ref as CR
from tests.test_gpu_refine import run_refine
from tests.test_refine_host import handles_of, loop_graph
from tests.test_rounding_host import SLACK

pytestmark = pytest.mark.gpu

GARBAGE = -5
KS = (2, 3, 4, 8)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


class RawBatch:
    """The part of a GraphBatch the decoders read (goff, rowptr, lcol, vals, sizes), built straight from the handles:
    a graph of two nodes (K = 2 with nothing movable) is below what GraphBatch accepts."""

    def __init__(self, pkg, handles):
        hip = pkg.hip
        self.handles = handles
        self.device = torch.device("cuda")
        self.sizes = np.asarray([h.n for h in handles], np.int64)
        self.goff_host = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        eoff = np.concatenate([[0], np.cumsum([h.col.size for h in handles])]).astype(np.int64)
        self.B, self.R = len(handles), int(self.goff_host[-1])
        self.rowptr_host = np.concatenate([[0]] + [h.rowptr[1:].astype(np.int64) + eoff[g] for g, h in enumerate(handles)]).astype(np.int32)
        self.lcol_host = np.concatenate([h.col for h in handles]).astype(np.int32)
        unit = all(h.weight is None for h in handles)
        self.vals_host = None if unit else np.concatenate(
            [np.ones(h.col.size, np.float32) if h.weight is None else h.weight for h in handles]).astype(np.float32)
        dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
        self.goff, self.rowptr, self.lcol = dev(self.goff_host.astype(np.int32)), dev(self.rowptr_host), dev(self.lcol_host)
        self.vals = dev(self.vals_host)
        self.c = hip.GmcBatch(B=self.B, R=self.R, nnz=int(eoff[-1]), n_max=int(self.sizes.max()),
                              nnz_max=int(max(h.col.size for h in handles)), goff=hip.ptr(self.goff),
                              rowptr=hip.ptr(self.rowptr), lcol=hip.ptr(self.lcol), gcol=hip.ptr(self.lcol),
                              vals=hip.ptr(self.vals))
        self._orders = {}
        self._lib = hip.load()

    def ref(self):
        return C.byref(self.c)

    def refine_order(self, K=3):
        if K not in self._orders:
            order = np.zeros(max(self.R, 1), np.int32)
            cgoff = np.zeros(self.B + 1, np.int32)
            cptr = np.zeros(self.R + self.B, np.int32)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            go = self.goff_host.astype(np.int32)
            if K == 3:
                rc = self._lib.gmc_refine_order_host(self.B, p(go), p(self.rowptr_host), p(self.lcol_host), p(order),
                                                     p(cgoff), p(cptr), cptr.size)
            else:
                rc = self._lib.gmc_round_order_host(self.B, p(go), p(self.rowptr_host), p(self.lcol_host), K, p(order),
                                                    p(cgoff), p(cptr), cptr.size)
            assert rc == 0, rc
            self._orders[K] = tuple(torch.from_numpy(a).cuda() for a in (order, cgoff, cptr))
        return self._orders[K]


def run_round(pkg, batch, P, K, descent, want_expected=True, want_sweeps=True):
    """gmc_round_conditional_f32 with every output pre-filled with garbage."""
    hip = pkg.hip
    order, cgoff, cptr = batch.refine_order(K)
    Pd = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    assign = torch.full((batch.R,), GARBAGE, dtype=torch.int8, device="cuda")
    cut = torch.full((batch.B,), float("nan"), device="cuda")
    expected = torch.full((batch.B,), float("nan"), device="cuda")
    sweeps = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_round_conditional_f32(batch.ref(), p(Pd), K, p(order), p(cgoff), p(cptr), descent, p(assign),
                                              p(cut), p(expected) if want_expected else None,
                                              p(sweeps) if want_sweeps else None, hip.stream())
    hip.check(rc, "gmc_round_conditional_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut=cut, expected=expected, sweeps=sweeps).items()}


def path_graph(n):
    return nx.path_graph(n)


def hub40_graph(n, seed):
    """d = 7 regular with node 9 raised to degree 40"""
    g = R.regular_graph(n, 7, seed)
    rng = np.random.RandomState(seed)
    for u in rng.permutation(n):
        if g.degree(9) >= 40:
            break
        if int(u) != 9 and not g.has_edge(9, int(u)):
            g.add_edge(9, int(u))
    assert g.degree(9) == 40
    return g


def shapes(K):
    """name -> graphs of one batch, for K classes"""
    return {
        "n_equals_K": [nx.complete_graph(K)],
        "n_K_plus_1": [nx.complete_graph(K + 1)],
        "n65": [R.regular_graph(65, 4, 65 + K)],
        "path1030": [path_graph(1030)],
        "batch_60_97_K": [R.regular_graph(60, 5, 60 + K), CR.connected_gnp(97, 0.06, 97 + K), nx.complete_graph(K)],
        "hub40": [hub40_graph(300, 40 + K)],
        "self_loops": [loop_graph(120, 5, 18 + K)],
        "gnp200": [CR.connected_gnp(200, 0.05, 200 + K)],
    }


SHAPES = [(K, name) for K in KS for name in sorted(shapes(2))] + [(8, "n2048_d3"), (3, "n4096_d3")]


def graphs_of(K, name):
    if name == "n2048_d3":
        return [R.regular_graph(2048, 3, 2048)]
    if name == "n4096_d3":
        return [R.regular_graph(4096, 3, 4096)]
    return shapes(K)[name]


@functools.lru_cache(maxsize=None)
def reference(K, name, signed):
    """The case and its restatement, computed once: handles, P (terminal rows NaN) and per graph the class bytes and
    sweeps at descent 0 and 100, float64 cuts, the float64 expected cut and W_abs."""
    graphs = graphs_of(K, name)
    if signed:
        graphs = [CR.signed_weights(g, 7 * i + K) for i, g in enumerate(graphs)]
    hs = handles_of(graphs)
    seed = 31 * K + len(name) + (1 if signed else 0)
    Ps, per_graph = [], []
    for i, h in enumerate(hs):
        P = CR.softmax_rows(h.n, K, seed + i, scale=2.0)
        CR.check_case_inputs(K, h.n, h.rowptr, h.col, h.weight, P)
        a0 = CR.round_sequential(h.n, h.rowptr, h.col, h.weight, P, K)
        a100, s100 = CR.descent(h.n, h.rowptr, h.col, h.weight, a0, K, 100)
        per_graph.append(dict(a0=a0, a100=a100, s100=s100, c0=CR.cut(h.rowptr, h.col, h.weight, a0),
                              c100=CR.cut(h.rowptr, h.col, h.weight, a100),
                              expected=CR.expected_cut(h.n, h.rowptr, h.col, h.weight, P, K),
                              W_abs=CR.abs_weight(h.rowptr, h.col, h.weight)))
        P = P.copy()
        P[:K] = np.nan                                                 # the terminals' rows are never read
        Ps.append(P)
    return hs, np.concatenate(Ps), per_graph


def check_outputs(got, batch, per_graph, descent, signed):
    key_a, key_c = ("a0", "c0") if descent == 0 else ("a100", "c100")
    for g, ref in enumerate(per_graph):
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        assert (got["assign"][lo:hi] == ref[key_a]).all(), (g, int((got["assign"][lo:hi] != ref[key_a]).sum()))
        assert got["sweeps"][g] == (0 if descent == 0 else ref["s100"])
        err = abs(float(got["cut"][g]) - ref[key_c])
        print(f"graph {g}: cut {got['cut'][g]} (float64 {ref[key_c]}), expected {got['expected'][g]} "
              f"(float64 {ref['expected']}), W_abs {ref['W_abs']}")
        if signed:
            assert err <= 1e-5 * abs(ref[key_c]), (g, got["cut"][g], ref[key_c])
        else:
            assert float(got["cut"][g]) == ref[key_c]
        assert abs(float(got["expected"][g]) - ref["expected"]) <= SLACK * ref["W_abs"]
        assert ref[key_c] >= ref["expected"] - SLACK * ref["W_abs"]        # the guarantee (the bytes are the device's)


@pytest.mark.parametrize("signed", (False, True), ids=("unit", "signed"))
@pytest.mark.parametrize("K,name", SHAPES)
def test_rounding_matches_the_restatement(pkg, K, name, signed):
    hs, P, per_graph = reference(K, name, signed)
    batch = RawBatch(pkg, hs)
    for descent in (0, 100):
        got = run_round(pkg, batch, P, K, descent)
        check_outputs(got, batch, per_graph, descent, signed)
        again = run_round(pkg, batch, P, K, descent)                   # two runs are byte-equal
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), k
        # NULL expected / sweeps leave the other outputs unchanged
        bare = run_round(pkg, batch, P, K, descent, want_expected=False, want_sweeps=False)
        assert bare["assign"].tobytes() == got["assign"].tobytes() and bare["cut"].tobytes() == got["cut"].tobytes()
        assert np.isnan(bare["expected"]).all() and (bare["sweeps"] == GARBAGE).all()
        half = run_round(pkg, batch, P, K, descent, want_expected=False)
        assert half["assign"].tobytes() == got["assign"].tobytes() and half["sweeps"].tobytes() == got["sweeps"].tobytes()
    if K == 3 and min(h.n for h in hs) >= 3:
        # the score has the bits gmc_refine_local_f32(max_sweeps = 0) reports for the same bytes, and descent = 100 is
        # descent = 0 followed by gmc_refine_local_f32(100), sweep counts included
        r0 = run_round(pkg, batch, P, 3, 0)
        r100 = run_round(pkg, batch, P, 3, 100)
        scored = run_refine(pkg, batch, r0["assign"].reshape(1, -1), 0)
        assert scored["cut_all"][:, 0].tobytes() == r0["cut"].tobytes()
        refined = run_refine(pkg, batch, r0["assign"].reshape(1, -1), 100)
        assert (refined["assign"][0] == r100["assign"]).all()
        assert (refined["sweeps"][:, 0] == r100["sweeps"]).all()
        assert refined["cut_all"][:, 0].tobytes() == r100["cut"].tobytes()


@pytest.mark.parametrize("K", KS)
def test_a_graph_rounds_the_same_alone_and_inside_a_batch(pkg, K):
    hs, P, per_graph = reference(K, "batch_60_97_K", True)
    batch = RawBatch(pkg, hs)
    for descent in (0, 100):
        together = run_round(pkg, batch, P, K, descent)
        for g, h in enumerate(hs):
            lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
            alone = run_round(pkg, RawBatch(pkg, [h]), P[lo:hi], K, descent)
            assert alone["assign"].tobytes() == together["assign"][lo:hi].tobytes()
            for k in ("cut", "expected", "sweeps"):
                assert alone[k].tobytes() == together[k][g:g + 1].tobytes(), (k, g)


def small_model(pkg, K, specs, N, F, seed, epochs=3):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    from gcn_max_cut_amd.Training import TrainingNeural as T
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: [int(t) for t in np.random.RandomState(s).permutation(n)[:K]] for i, (n, d, s) in enumerate(specs)}
    ds = GE.process_graphs_from_folder(graphs, terms, N, number_classes=K)
    cfg = T.TrainingConfig(n_nodes=N, hidden_dim=F, number_classes=K, learning_rate=1e-2)
    torch.manual_seed(seed)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    for _ in range(epochs):
        T.train_single_epoch(ds, net, opt, embed, cfg, graphs_per_step=len(ds))
    net.eval()
    return net, ds


@pytest.mark.parametrize("K", (3, 2))
def test_round_dataset(pkg, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = small_model(pkg, K, [(60, 5, 61), (48, 6, 62), (100, 7, 63)], 128, 16, seed=K)
    assert net.engine().K == K and (K == 3 or net.engine().kway)
    for descent in (0, 100):
        results = TN.round_dataset(net, ds, descent_sweeps=descent)
        assert len(results) == len(ds)
        for res, (handle, a_pad, nx_g, _t) in zip(results, ds.values()):
            assert set(res) == {'nodes', 'simple_cut', 'simple_assignment', 'expected_cut', 'rounded_cut',
                                'rounded_assignment', 'descent_sweeps'}
            assert res["nodes"] == handle.n == len(res["rounded_assignment"])
            assert res["rounded_cut"] == TN.calculate_cut_value(res["rounded_assignment"], nx_g)
            assert res["simple_cut"] == TN.calculate_cut_value(res["simple_assignment"], nx_g)
            assert res["rounded_assignment"][:K] == list(range(K))     # terminals are fixed
            assert 0 <= min(res["rounded_assignment"]) and max(res["rounded_assignment"]) < K
            W_abs = nx_g.number_of_edges()
            assert res["rounded_cut"] >= res["expected_cut"] - SLACK * W_abs
            assert res["descent_sweeps"] == 0 if descent == 0 else 1 <= res["descent_sweeps"] <= 100
            with torch.no_grad():
                P = net(handle, a_pad)
            one, one_cut = TN.conditional_rounding(P, nx_g, descent_sweeps=descent)
            assert one == res["rounded_assignment"] and one_cut == res["rounded_cut"]
            h = handles_of([nx_g])[0]
            ref, ref_sweeps = CR.round_and_descend(h.n, h.rowptr, h.col, h.weight, P.cpu().numpy(), K, descent)
            assert ref.tolist() == res["rounded_assignment"] and ref_sweeps == res["descent_sweeps"]


def test_decode_dataset_with_rounding_keeps_the_other_keys(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = small_model(pkg, 3, [(60, 5, 71), (48, 6, 72)], 128, 16, seed=5)
    np.random.seed(11)
    plain = TN.decode_dataset(net, ds, 20, local_search_sweeps=10)
    state = np.random.get_state()[1].copy()
    np.random.seed(11)
    both = TN.decode_dataset(net, ds, 20, local_search_sweeps=10, rounding_descent_sweeps=0)
    assert (np.random.get_state()[1] == state).all()                   # the same uniforms drawn
    rounded = TN.round_dataset(net, ds, 0)
    for f, b, r in zip(plain, both, rounded):
        assert set(b) == set(f) | {'expected_cut', 'rounded_cut', 'rounded_assignment'}
        assert {k: b[k] for k in f} == f
        assert (b["expected_cut"], b["rounded_cut"], b["rounded_assignment"]) == \
            (r["expected_cut"], r["rounded_cut"], r["rounded_assignment"])
    with pytest.raises(ValueError, match="number_classes"):
        net2, ds2 = small_model(pkg, 2, [(40, 5, 73)], 64, 8, seed=6, epochs=1)
        TN.decode_dataset(net2, ds2, 4, rounding_descent_sweeps=0)     # decode_dataset stays 3-class
