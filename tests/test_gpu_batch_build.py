"""GPU checks of ``GraphBatch.from_edge_index`` (gmc_batch_build_csr / gmc_batch_build_table): a batch built on the device
from edge-index tensors holds, byte for byte, every array and every scalar of ``GraphBatch([from_networkx(g) ...])`` for
the same graphs - the yardstick, built once per case - on the cases of tests/batch_build_cases.py (the sizes at which each
kernel changes path), for every input form, and through the engine, the functional form and the colour orders.  The error
cases exercise the guards: a bad id is counted, never used as an index."""
import numpy as np
import pytest
import torch

from tests import batch_build_cases as BC

pytestmark = pytest.mark.gpu

ARRAYS = ("goff", "rowptr", "gcol", "lcol", "vals", "dinv", "ell", "ell_vals", "ovf_ptr", "ovf_ids", "ovf_vals")
STRUCT = ("B", "R", "nnz", "n_max", "uniform_n", "nnz_max", "ell_width", "ell_slots", "ovf_max_blocks")
HOST = ARRAYS[1:] + ("B", "R", "nnz", "n_max", "uniform_n", "nnz_max", "ell_width", "ell_slots", "ovf_max_blocks",
                     "max_degree")


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


_yardsticks = {}


def yardstick(pkg, name, allow_zero_degree=False):
    """GraphBatch(handles) of the case's graphs: built once, shared, never written."""
    key = (name, allow_zero_degree)
    if key not in _yardsticks:
        _yardsticks[key] = pkg.GraphBatch([pkg.from_networkx(g) for g in BC.graphs(name)],
                                          allow_zero_degree=allow_zero_degree)
    return _yardsticks[key]


def same_batch(got, want, what=""):
    for name in ARRAYS:
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), (what, name, a is None)
        if a is not None:
            assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, name, a.dtype, a.shape, b.dtype, b.shape)
            x, y = a.cpu().numpy(), b.cpu().numpy()
            if x.tobytes() != y.tobytes():
                bad = np.flatnonzero(x.ravel().view(np.uint8 if x.itemsize == 1 else f"u{x.itemsize}")
                                     != y.ravel().view(np.uint8 if y.itemsize == 1 else f"u{y.itemsize}"))
                raise AssertionError(f"{what}: {name} differs at {bad.size} of {x.size} places, first {bad[:8]}: "
                                     f"{x.ravel()[bad[:8]]} against {y.ravel()[bad[:8]]}")
    for name in STRUCT:
        assert getattr(got.c, name) == getattr(want.c, name), (what, name, getattr(got.c, name), getattr(want.c, name))
    for name in ("B", "R", "nnz", "n_max", "uniform_n"):
        assert getattr(got, name) == getattr(want, name), (what, name)
    assert got.sizes.dtype == want.sizes.dtype and np.array_equal(got.sizes, want.sizes), what
    assert got.goff_host.dtype == want.goff_host.dtype and np.array_equal(got.goff_host, want.goff_host), what
    for name in HOST:   # the lazy host copy: a BatchArrays in all but its construction
        a, b = getattr(got.host, name), getattr(want.host, name)
        if isinstance(b, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, "host", name)
        else:
            assert a == b and (a is None) == (b is None), (what, "host", name, a, b)
    assert np.array_equal(got.host.sizes, want.host.sizes) and np.array_equal(got.host.goff, want.host.goff)


def build(pkg, name, pairs="both", dtype=np.int64, where="cuda", order=None, **kw):
    ei, ptr, w = BC.edge_arrays(list(BC.graphs(name)), pairs, dtype)
    if order is not None:
        ei, w = ei[:, order], (None if w is None else w[order])
    ei = torch.from_numpy(np.ascontiguousarray(ei)).to(where)
    w = None if w is None else torch.from_numpy(np.ascontiguousarray(w)).to(where)
    return pkg.GraphBatch.from_edge_index(ei, ptr, edge_weight=w, pairs=pairs, **kw)


# ---- every case, byte for byte
@pytest.mark.parametrize("name", sorted(BC.CASES))
def test_device_build_equals_host_build(pkg, name):
    want = yardstick(pkg, name)
    got = build(pkg, name)
    same_batch(got, want, name)
    print(f"{name}: B {got.B} R {got.R} nnz {got.nnz} max degree {got.host.max_degree} W {got.c.ell_width} "
          f"slots {got.c.ell_slots} overflow blocks {got.c.ovf_max_blocks} weights {got.vals is not None}")


def test_cases_take_the_paths_they_are_there_for(pkg):
    facts = {name: yardstick(pkg, name) for name in BC.CASES}
    width = lambda n: (facts[n].c.ell_width, facts[n].c.ell_slots)
    assert width("reg7_n64") == (8, 7) and width("reg7_n65") == (8, 7) and width("reg8") == (8, 8)
    assert width("reg12") == (16, 12) and width("reg16") == (16, 16) and width("path3") == (8, 7)
    assert [facts[n].host.max_degree for n in ("star64", "star65", "star70", "star_wg", "star_wg1")] == \
        [64, 65, 70, BC.WG_SORT, BC.WG_SORT + 1]
    assert facts["star_wg"].ell is None and facts["star_wg1"].ell is None and facts["n4200"].ell is None
    assert facts["hub40"].ovf_ptr is not None and facts["hub40"].c.ovf_max_blocks == 4
    assert facts["hub128"].c.ovf_max_blocks == 15 and facts["hub128"].c.ell_width == 8
    assert facts["hub140"].ell is None and facts["hub140"].ovf_ptr is None
    assert facts["gnp300"].ell is None and 8 < facts["gnp300"].host.max_degree <= 64      # rows of the wave sort
    assert facts["real"].vals is not None and facts["real"].ovf_vals is not None
    assert facts["mixed_weights"].vals is not None and facts["all_ones"].vals is None
    assert tuple(facts["mixed"].sizes) == BC.MIXED


def test_empty_batch(pkg):
    want = pkg.GraphBatch([])
    got = pkg.GraphBatch.from_edge_index(torch.zeros((2, 0), dtype=torch.int64), np.asarray([0]))
    same_batch(got, want, "B = 0")
    assert got.handles() == []


def test_single_graph_by_num_nodes(pkg):
    ei, ptr, _w = BC.edge_arrays(list(BC.graphs("reg7_n65")))
    same_batch(pkg.GraphBatch.from_edge_index(torch.from_numpy(ei).cuda(), num_nodes=65), yardstick(pkg, "reg7_n65"), "num_nodes")


# ---- input forms
@pytest.mark.parametrize("name", ["mixed", "real", "hub40", "star70"])
def test_any_input_order_gives_the_same_bytes(pkg, name):
    want = yardstick(pkg, name)
    E = BC.edge_arrays(list(BC.graphs(name)))[0].shape[1]
    for seed in (1, 2, 3, 3):   # three orders, the last one twice
        same_batch(build(pkg, name, order=np.random.RandomState(seed).permutation(E)), want, f"{name} order {seed}")


@pytest.mark.parametrize("name", ["mixed", "mixed_weights", "loop"])
def test_input_forms(pkg, name):
    want = yardstick(pkg, name)
    for where in ("cpu", "cuda"):
        for dtype in (np.int32, np.int64):
            for pairs in ("both", "once"):
                same_batch(build(pkg, name, pairs, dtype, where), want, f"{name} {where} {dtype.__name__} {pairs}")
    ei, ptr, w = BC.edge_arrays(list(BC.graphs(name)))
    same_batch(pkg.GraphBatch.from_edge_index(ei, torch.from_numpy(ptr).cuda(), edge_weight=w), want, f"{name} numpy, ptr on the device")
    same_batch(pkg.GraphBatch.from_edge_index(ei.astype(np.int16), list(ptr), edge_weight=w), want, f"{name} int16, ptr a list")


def test_explicit_unit_weights_give_no_values(pkg):
    ei, ptr, _w = BC.edge_arrays(list(BC.graphs("mixed")), weights=True)
    got = pkg.GraphBatch.from_edge_index(ei, ptr, edge_weight=np.ones(ei.shape[1], np.float32))
    assert got.vals is None and got.ell_vals is None
    same_batch(got, yardstick(pkg, "mixed"), "explicit ones")


# ---- bad input: counted on the device, refused before the table stage
@pytest.fixture
def table_calls(pkg, monkeypatch):
    lib, calls = pkg.hip.load(), []
    real = lib.gmc_batch_build_table
    monkeypatch.setattr(lib, "gmc_batch_build_table", lambda *a: calls.append(1) or real(*a))
    return calls


def two_graphs():
    gs = [BC.regular(20, 3, 1), BC.regular(9, 4)]
    ei, ptr, _w = BC.edge_arrays(gs)
    return gs, ei, ptr


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_ids_out_of_range_are_refused(pkg, table_calls, dtype):
    _gs, ei, ptr = two_graphs()
    for value, count in ((29, 1), (-1, 1), (1 << 30, 1), ((1 << 40) if dtype is np.int64 else -(1 << 31), 1)):
        bad = ei.astype(dtype)
        bad[1, 5] = value
        with pytest.raises(ValueError, match=f"{count} entries with an id outside"):
            pkg.GraphBatch.from_edge_index(bad, ptr)
    bad = ei.astype(dtype)
    bad[0, 3], bad[1, 7], bad[0, 9] = 29, -5, 1 << 20
    with pytest.raises(ValueError, match="3 entries with an id outside"):
        pkg.GraphBatch.from_edge_index(torch.from_numpy(bad).cuda(), ptr)
    assert table_calls == []


def test_endpoints_in_two_graphs_are_refused(pkg, table_calls):
    _gs, ei, ptr = two_graphs()
    bad = np.concatenate([ei, np.asarray([[0, 20], [20, 0]])], axis=1)
    with pytest.raises(ValueError, match="2 entries whose endpoints lie in two graphs"):
        pkg.GraphBatch.from_edge_index(bad, ptr)
    assert table_calls == []


def test_repeated_entries_are_refused(pkg, table_calls):
    _gs, ei, ptr = two_graphs()
    with pytest.raises(ValueError, match="2 entries that repeat another entry"):
        pkg.GraphBatch.from_edge_index(np.concatenate([ei, ei[:, 4:6]], axis=1), ptr)
    assert table_calls == []


def test_a_missing_reverse_entry_is_refused(pkg, table_calls):
    _gs, ei, ptr = two_graphs()
    with pytest.raises(ValueError, match="1 entries whose reverse entry is missing"):
        pkg.GraphBatch.from_edge_index(np.delete(ei, 11, axis=1), ptr)
    with pytest.raises(ValueError, match=f"{ei.shape[1]} entries that repeat another entry"):
        pkg.GraphBatch.from_edge_index(ei, ptr, pairs="once")     # both directions listed, then flipped once more
    assert table_calls == []


def test_unequal_reverse_weights_are_refused(pkg, table_calls):
    _gs, ei, ptr = two_graphs()
    w = np.full(ei.shape[1], 0.5, np.float32)
    w[0] = 0.75
    with pytest.raises(ValueError, match="2 entries whose reverse entry is missing or carries another weight"):
        pkg.GraphBatch.from_edge_index(ei, ptr, edge_weight=w)
    assert table_calls == []


def test_zero_degree_nodes_are_refused_unless_allowed(pkg, table_calls):
    gs, ei, ptr = two_graphs()
    ptr = ptr.copy()
    ptr[-1] += 2                                  # two nodes without neighbours at the end of the last graph
    with pytest.raises(ValueError, match="2 nodes without neighbours"):
        pkg.GraphBatch.from_edge_index(ei, ptr)
    assert table_calls == []
    gs[1].add_nodes_from([9, 10])
    want = pkg.GraphBatch([pkg.from_networkx(g) for g in gs], allow_zero_degree=True)
    same_batch(pkg.GraphBatch.from_edge_index(ei, ptr, allow_zero_degree=True), want, "zero degree allowed")
    assert table_calls == [1]


# ---- end to end on (5, 300, 65, 257)
def test_engine_step_and_functional_give_the_same_bytes(pkg):
    want, got = yardstick(pkg, "mixed"), build(pkg, "mixed")
    N, F, K = 300, 12, 3
    init = torch.from_numpy(np.random.RandomState(7).uniform(-0.3, 0.3, 4096).astype(np.float32)).cuda()
    results = []
    for batch in (want, got):
        eng = pkg.FusedEngine(N, F, K)
        for v in eng.views().values():
            v.copy_(init[:v.numel()].view(v.shape))
        P, S, losses = eng.train_step(batch, lr=1e-2)
        results.append([t.cpu().numpy().tobytes() for t in (P, S, losses, eng.flat, eng.grad, eng.m, eng.v)])
    assert results[0] == results[1]
    Fn = pkg.functional
    results = []
    for batch in (want, got):
        W = [torch.from_numpy(np.random.RandomState(8 + i).uniform(-0.3, 0.3, shape).astype(np.float32)).cuda().requires_grad_()
             for i, shape in enumerate(((N, F), (F,), (F, 4), (4,)))]
        P = Fn.gcn_softmax(batch, *W)
        loss = Fn.cut_loss(batch, P, relaxed=True)
        loss.backward()
        results.append([t.detach().cpu().numpy().tobytes() for t in (P, loss, *(w.grad for w in W))])
    assert results[0] == results[1]


@pytest.mark.parametrize("name", ["mixed", "n4200"])
def test_colour_orders_and_handles(pkg, name):
    want, got = yardstick(pkg, name), build(pkg, name)
    assert "host" not in got.__dict__                    # not copied back until someone asks
    for K in (3, 4):
        for a, b in zip(got.refine_order(K), want.refine_order(K)):
            assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), K
        assert got.refine_classes(K) == want.refine_classes(K)
    assert "host" in got.__dict__
    handles = [pkg.from_networkx(g) for g in BC.graphs(name)]
    mine = got.handles()
    assert len(mine) == len(handles)
    for a, b in zip(mine, handles):
        assert a.n == b.n and a.rowptr.tobytes() == b.rowptr.tobytes() and a.col.tobytes() == b.col.tobytes()
        assert a.weight is None and b.weight is None


def test_handles_carry_each_graph_s_own_weights(pkg):
    got = build(pkg, "mixed_weights")
    for a, g in zip(got.handles(), BC.graphs("mixed_weights")):
        b = pkg.from_networkx(g)
        assert a.rowptr.tobytes() == b.rowptr.tobytes() and a.col.tobytes() == b.col.tobytes()
        assert (a.weight is None) == (b.weight is None)
        assert a.weight is None or a.weight.tobytes() == b.weight.tobytes()
