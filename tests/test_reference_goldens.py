"""Oracles AND product mirrors against fixtures produced by the reference's OWN code
(tests/golden/training.json, made by tests/golden/make_golden_training.py from
/root/reference/python/Training/TrainingNeural.py, DataGenerator/graphExtender.py, commons.py with an
inert ``dgl`` placeholder: GraphConv raises, from_networkx returns an opaque token).

After these tests the only parity-unpinned pieces of the hot path are ``GraphConv.forward`` and
``dgl.from_networkx`` (DGL 2.0.0 cannot run here).
"""
import contextlib
import copy
import io
import json
import os
import re

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import c_oracle as CO
from oracle import ref_dense as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def G():
    return json.load(open(os.path.join(HERE, "golden", "training.json")))


@pytest.fixture(scope="module")
def T(built):
    from gcn_max_cut_amd.Training import TrainingNeural
    return TrainingNeural


@pytest.fixture(scope="module")
def GE(built):
    from gcn_max_cut_amd.DataGenerator import graphExtender
    return graphExtender


def graph_of(n, edges):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    for u, v, w in edges:
        g.add_edge(int(u), int(v), weight=int(w) if float(w).is_integer() else w, capacity=1)
    return g


def dense_of(shape, trip):
    m = torch.zeros(*shape, dtype=torch.float32)
    for r, c, v in trip:
        m[r, c] = v
    return m


def hexes(a):
    return [np.float32(v).tobytes().hex() for v in np.asarray(a, np.float32).ravel()]


def test_fixture_is_from_the_reference_with_an_inert_dgl(G):
    assert "INERT" in G["dgl"] and "GraphConv.forward" in G["dgl"]
    assert len(G["loss"]) == 5 and set(G["train_model"]) == {"rise_then_stop", "plateau", "reset_counter", "runs_out"}


def test_training_config_matches_the_reference_dataclass(G, T):
    assert dict(T.TrainingConfig().__dict__) == G["config"]["defaults"]
    assert dict(T.TrainingConfig(n_nodes=300, hidden_dim=7).__dict__) == G["config"]["derived"]
    assert list(T.TrainingConfig.__dataclass_fields__) == G["config"]["fields"]


@pytest.mark.parametrize("idx", range(5))
def test_override_one_hot_loss_and_dLdP(G, T, idx):
    """TrainingNeural.py:87-106,154-176,291-309 + autograd: oracle (torch), oracle (C) and the product's
    host mirrors against the reference's own outputs - values bit for bit, incl. the tie rows, the
    saturated row and the straight-through residue ((1 + p) - p != 1 in fp32, Q6).  dL/dP is the autograd of the
    S S^T GEMM, whose last bit follows the accumulation order of the code path MKL picks for the CPU: the fixture
    holds the reference's dL/dP on each path, oracle and product must give the same bits, and those bits must be
    the reference's on one path."""
    c = G["loss"][idx]
    by_path = {isa: hexes(g) for isa, g in c["dL_dP_by_mkl_path"].items()}
    assert by_path["AVX512"] == hexes(c["dL_dP"])           # (the path the fixture's other values were recorded on)
    grads = {}
    n = c["n"]
    g = graph_of(n, c["edges"])
    a_ref = dense_of(c["adjacency_shape"], c["adjacency_nonzeros"])
    # the padded adjacency itself (commons.py:38-77 + graphExtender.py:28-48), three ways
    assert torch.equal(R.dense_adjacency(g, 1000), a_ref)
    from gcn_max_cut_amd import commons as PC
    from gcn_max_cut_amd.DataGenerator import graphExtender as PG
    assert torch.equal(PG.extend_matrix_torch_2(PC.adjacency_tensor(g, torch_dtype=torch.float32), 1000), a_ref)
    assert torch.equal(PG.extend_matrix_torch_2(PC.qubo_dict_to_torch(g, PC.gen_adj_matrix(g), torch_dtype=torch.float32), 1000), a_ref)

    P = np.asarray(c["P"], np.float32)
    for name, ov_f, hot_f, loss_f in (
            ("oracle", R.override_terminals, R.straight_through_one_hot, lambda s, a: R.cut_loss(s, a, c["C"])),
            ("product", T.override_fixed_nodes, T.apply_max_to_one_hot, lambda s, a: T.compute_loss(s, a, 0.0, c["C"], 1000.0))):
        h = torch.from_numpy(P.copy()).requires_grad_(True)
        ov = ov_f(h)
        hot = hot_f(ov)
        loss = loss_f(hot, a_ref)
        loss.backward()
        assert hexes(ov.detach()) == hexes(c["override"]), name
        assert [hexes(r) for r in ov.detach().numpy()[:3]] == c["override_hex"], name
        assert hexes(hot.detach()) == hexes(c["one_hot"]), name
        assert torch.argmax(hot.detach(), 1).tolist() == c["argmax"], name
        assert np.float32(loss.item()).tobytes().hex() == c["loss_hex"], name
        grads[name] = hexes(h.grad)
        assert grads[name] in by_path.values(), name
    assert grads["oracle"] == grads["product"]
    assert float(T.calculate_HC_vectorized(torch.tensor(c["one_hot"]), a_ref)) == c["HC"]
    # per-row form of the product (max_to_one_hot) on the tie rows: first maximum wins (:98)
    for r in (5, 6, 7, 8):
        assert hexes(T.max_to_one_hot(torch.from_numpy(P[r]))) == hexes(c["one_hot"][r])

    # the C oracle works on hard one-hots: argmax identical, loss and dL/dP equal up to the ~6e-8
    # straight-through residue the reference carries in its "1" entries
    rp, cl, vl = CO.csr_of(g)
    S, loss_c, GP = CO.loss_grad(rp, cl, vl, P, c["C"])
    assert S.tolist() == c["argmax"]
    assert abs(loss_c - c["loss"]) <= 1e-6 * max(1.0, abs(c["loss"]))
    ref_gp = np.asarray(c["dL_dP"], np.float32)
    assert np.abs(GP - ref_gp).max() <= 2e-7 * max(1.0, np.abs(ref_gp).max())
    # and the integer-valued identity the kernels rely on: loss == -C * cut(argmax partition)
    assert c["loss"] == -c["C"] * R.cut_value(c["argmax"], g)


def test_extend_matrix_helpers(G, T, GE):
    e = G["extend"]
    m = torch.tensor(e["input"])
    assert T.extend_matrix_torch(m, e["N"]).tolist() == e["extend_matrix_torch"]
    assert GE.extend_matrix_torch_2(m, e["N"]).tolist() == e["extend_matrix_torch_2"]
    assert T.extend_matrix_torch(m, 3).tolist() == e["extend_same_size"]
    assert str(T.extend_matrix_torch(m, e["N"]).dtype) == e["dtype"]
    assert str(T.extend_matrix_torch(m.double(), e["N"]).dtype) == e["dtype"]   # the reference allocates default-dtype zeros
    for fn, name in ((T.extend_matrix_torch, "extend_matrix_torch"), (GE.extend_matrix_torch_2, "extend_matrix_torch_2")):
        with pytest.raises(ValueError) as ei:
            fn(m, 2)
        assert str(ei.value) == e["too_small_error"][name]


def test_swap_graph_nodes(G, GE):
    for c in G["swap"]:
        for swap in (GE.swap_graph_nodes, R.swap_labels):
            g = graph_of(c["n"], c["edges_before"])
            swap(g, {k: v for k, v in c["mapping"]})
            got = [[u, v, float(d["weight"])] for u, v, d in g.edges(data=True)]
            assert got == c["edges_after"], swap.__name__          # same edges in the same iteration order
            assert list(g.nodes()) == c["nodes_after"]


def _extender_inputs(e):
    graphs = {i["name"]: graph_of(i["n"], i["edges"]) for i in e["inputs"]}
    terms = {i["name"]: list(i["terminals"]) for i in e["inputs"]}
    return graphs, terms


def test_process_graphs_from_folder_all_terminal_cases(G, GE, tmp_path, monkeypatch):
    """graphExtender.py:50-132: four terminal cases + the skip, the relabelled edge lists, the padded
    adjacency, the in-place sort of the terminal lists, the prints (Q11)."""
    monkeypatch.chdir(tmp_path)
    e = G["extender"]
    graphs, terms = _extender_inputs(e)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ds = GE.process_graphs_from_folder(graphs, terms, e["max_nodes"])
    assert buf.getvalue().splitlines() == e["stdout"]
    assert {k: list(v) for k, v in terms.items()} == e["terminals_after"]
    assert [int(k) for k in ds] == [it["key"] for it in e["items"]]
    for it in e["items"]:
        h, a_pad, g, t = ds[it["key"]]
        assert [[u, v, float(d["weight"])] for u, v, d in g.edges(data=True)] == it["edges_after"]
        assert list(a_pad.shape) == it["shape"] and str(a_pad.dtype) == it["dtype"] and t == it["terminals_entry"]
        assert torch.equal(a_pad.cpu(), dense_of(it["shape"], it["adjacency_nonzeros"]))
        # the handle standing where the DGLGraph is: 2|E| directed edges over the same structure
        assert h.number_of_nodes() == it["shape"][0] and h.number_of_edges() == len(it["adjacency_nonzeros"])
    # the torch oracle's restatement of the same function
    graphs, terms = _extender_inputs(e)
    ods = R.make_dataset(graphs, terms, e["max_nodes"])
    assert {k: list(v) for k, v in terms.items()} == e["terminals_after"]
    for it in e["items"]:
        assert torch.equal(ods[it["key"]][1], dense_of(it["shape"], it["adjacency_nonzeros"]))
        assert [[u, v, float(d["weight"])] for u, v, d in ods[it["key"]][2].edges(data=True)] == it["edges_after"]


def test_process_graphs_batch_flush_and_swallowed_error(G, GE, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    e = G["extender"]
    for bs, want in e["batch_flush"].items():
        graphs, terms = _extender_inputs(e)
        saved = []
        monkeypatch.setattr(GE, "save_object", lambda obj, filename: saved.append({"filename": filename, "keys": [int(k) for k in obj]}))
        with contextlib.redirect_stdout(io.StringIO()):
            ds = GE.process_graphs_from_folder(graphs, terms, 1000, save_batch_size=int(bs), output_filename_prefix="pfx")
        assert saved == want["saved"] and [int(k) for k in ds] == want["returned_keys"]
    buf = io.StringIO()
    g = {"a": graph_of(20, e["inputs"][0]["edges"])}
    with contextlib.redirect_stdout(buf):
        ds = GE.process_graphs_from_folder(g, {"a": [7, 13, 4]}, 10)     # pad < n: printed, swallowed
    assert [int(k) for k in ds] == e["too_small"]["returned_keys"]
    assert ("N should be greater than or equal to the original matrix size." in buf.getvalue()) == e["too_small"]["mentions_value_error"]


def test_gen_adj_matrix_and_qubo_dict_to_torch(G, built):
    from gcn_max_cut_amd import commons as PC
    for c in G["adjacency"]:
        g = graph_of(c["n"], c["edges"])
        q = PC.gen_adj_matrix(g)
        assert len(q) == c["dict_entries"]
        m = PC.qubo_dict_to_torch(g, q, torch_dtype=torch.float32)
        assert list(m.shape) == c["shape"] and str(m.dtype) == c["dtype"]
        assert torch.equal(m, dense_of(c["shape"], c["nonzeros"]))
        assert torch.equal(PC.adjacency_tensor(g, torch_dtype=torch.float32), m)


@pytest.mark.parametrize("name", ["rise_then_stop", "plateau", "reset_counter", "runs_out"])
def test_train_model_bookkeeping_trace(G, T, name, tmp_path, monkeypatch):
    """TrainingNeural.py:421-482 with train_single_epoch scripted: early stop (Q8), best loss, history,
    checkpoint names (Q9), prints - product and oracle restatement vs the reference's run."""
    monkeypatch.chdir(tmp_path)
    c = G["train_model"][name]
    it = iter(c["losses"])
    net = torch.nn.Linear(2, 2)
    embed = torch.nn.Embedding(4, 4)
    opt = torch.optim.Adam(list(net.parameters()) + list(embed.parameters()), lr=1e-3)
    saved = []
    monkeypatch.setattr(T, "train_single_epoch", lambda *a, **k: next(it))
    monkeypatch.setattr(T, "setup_model_and_optimizer", lambda cfg: (net, embed, opt))
    monkeypatch.setattr(torch, "save", lambda obj, f, *a, **k: saved.append(
        {"filename": f, "keys": list(obj.keys()), "epoch": int(obj["epoch"]), "loss_history": [float(x) for x in obj["loss_history"]]}))
    cfg = T.TrainingConfig(n_nodes=1000, **c["config"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        r_net, best, epoch, emb_w, hist = T.train_model({}, cfg)
    lines = [re.sub(r"Training completed in [0-9.]+ seconds", "Training completed in <T> seconds", ln) for ln in buf.getvalue().splitlines()]
    lines = [re.sub(r"^Device: .*", "Device: <D>", ln) for ln in lines]
    assert (float(best), int(epoch), [float(x) for x in hist]) == (c["best_loss"], c["final_epoch"], c["loss_history"])
    assert (r_net is net) == c["returns_same_net"] and (emb_w is embed.weight) == c["returns_embed_weight"]
    assert saved == c["saved"]
    assert lines == c["stdout"]
    stop, obest, ohist = R.early_stop_trace(c["losses"][:c["config"]["number_epochs"]], c["config"]["tolerance"], c["config"]["patience"])
    assert (obest, ohist) == (c["best_loss"], c["loss_history"])
    assert (stop if stop is not None else len(ohist) - 1) == c["final_epoch"]


def test_save_neural_model_checkpoint_layout(G, T, monkeypatch):
    c = G["save_neural_model"]
    net = torch.nn.Linear(2, 2)
    embed = torch.nn.Embedding(4, 4)
    opt = torch.optim.Adam(list(net.parameters()) + list(embed.parameters()), lr=1e-3)
    got = {}
    monkeypatch.setattr(torch, "save", lambda obj, f, *a, **k: got.update(
        filename=f, keys=list(obj.keys()), inputs_is_embed_weight=obj["inputs"] is embed.weight, epoch=obj["epoch"],
        loss_history=list(obj["loss_history"])))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        T.save_neural_model(net, opt, embed, 7, [-1.0, -2.0], T.TrainingConfig(), "some/path.pth")
    got["stdout"] = buf.getvalue().splitlines()
    assert got == c


def test_evaluate_optimal_partitioning_host_chain(G, T):
    """TrainingNeural.py:229-289 with a model object that returns stored probabilities (the GPU test in
    test_gpu_parity.py runs it on the real model): six model calls, ones-features for n < 30, binary
    threshold, legacy cut."""
    for c in G["optimal_partitioning"]:
        n = c["n"]
        g = graph_of(n, c["edges"])
        from gcn_max_cut_amd import commons as PC
        adj = PC.adjacency_tensor(g, torch_dtype=torch.float32)
        P = np.asarray(c["P"], np.float32)
        seen = []

        class Tok:
            def number_of_nodes(self):
                return n

        class Net:
            def eval(self):
                return self

            def __call__(self, tok, inputs):
                seen.append(list(inputs.shape))
                return torch.from_numpy(P.copy())

        best = T.GetOptimalNetValue(Net(), Tok(), torch.zeros(n, 1000), adj, {"s": 0, "t": 1, "u": 2})
        assert float(best) == c["best_loss"] and len(seen) == c["model_calls"] and seen[:1] == c["input_shapes"]
        binary = (T.override_fixed_nodes(torch.from_numpy(P.copy())) >= 0.5).float()
        assert binary.tolist() == c["binary"]
        assert float(T.calculateAllCut(adj, binary)) == c["calculate_all_cut_legacy"]
        assert T.generate_terminal_permutations({"s": 0, "t": 1, "u": 2}) == c["permutations"]
