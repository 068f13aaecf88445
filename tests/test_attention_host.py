"""CPU tests of the graph-attention first layer: the float64 restatement tests/attention_ref.py against torch.autograd
through an independent dense form of the same model, the layer with zero attention vectors (the mean over the terms), the
status codes and workspace sizes of the three gmc_att_* entry points, the kernels in the gfx950 code object, the ``layer1``
keyword with its environment switch and checkpoint, and the precondition of the GPU cases: on the float64 reference no
row of a case is near a tie, no unit near the relu kink and no score near the leaky relu's, so
tests/test_gpu_attention.py can demand identical partitions and judge every gradient entry."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import attention_ref as AR
from tests import kway_ref as KR
from tests import stepcheck, util
from tests import test_api_status as A
from tests.stepcheck import KEYS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOME, ODD, BIG = A.SOME, A.ODD, A.BIG
NEW = ("gmc_att_workspace_bytes", "gmc_att_forward", "gmc_att_train_fwd_bwd")


def golden_csrs(built):
    out = []
    for rec in json.load(open(os.path.join(GOLD, "graphs.json")))["graphs"]:
        out.append(KR.csr_of_handle(built.from_networkx(R.regular_graph(rec["n"], rec["d"], rec["seed"]))))
    return out


# ---- the restatement against torch.autograd through a dense form of the same model (attention_ref.dense_loss)
@pytest.mark.parametrize("loss", ("cut", "expected_cut"))
def test_restatement_gradients_equal_autograd_through_a_dense_form(built, loss):
    csrs = golden_csrs(built)
    params32 = AR.random_params(200, 16, 5)
    ref, _gaps = AR.f64_step(csrs, params32, 1.3, loss)
    P, grads = AR.dense_step(csrs, params32, 1.3, loss)
    assert np.abs(P - ref.P).max() <= 1e-12
    for k in AR.ATT_KEYS:
        want = ref.grads[k]
        assert np.abs(want).max() > 0, k
        err = float(np.abs(grads[k] - want).max() / np.abs(want).max())
        assert err <= 1e-10, (k, err)


def test_restatement_with_a_self_loop_and_an_isolated_node_equals_autograd(built):
    """The term-count matrix of the dense form has a 2 on the diagonal of a node with a self-loop edge (the edge is one
    more ordinary term) and a lone 1 for a node without neighbours."""
    for g in (AR.with_self_loop(30, 4, 4), AR.with_isolated_node(20, 3, 3)):
        csr = KR.csr_of_handle(built.from_networkx(g))
        params32 = AR.random_params(64, 8, 1)
        ref, _gaps = AR.f64_step([csr], params32, 1.0, "expected_cut")
        params = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for k, v in params32.items()}
        value, _P = AR.dense_loss(csr, params, 1.0, "expected_cut")
        value.backward()
        assert abs(float(value.detach()) - ref.loss[0]) <= 1e-10 * abs(ref.loss[0])
        for k in AR.ATT_KEYS:
            err = float(np.abs(params[k].grad.numpy() - ref.grads[k]).max() / np.abs(ref.grads[k]).max())
            assert err <= 1e-10, (k, err)
    rp, cl, _vl = KR.csr_of_handle(built.from_networkx(AR.with_isolated_node(20, 3, 3)))
    f = AR.f64_forward(rp, cl, None, AR.random_params(64, 8, 1))
    lone = np.nonzero(f["ti"] == 20)[0]
    assert lone.size == 1 and f["alpha"][lone[0]] == 1.0 and f["z"][lone[0]] == 0.0


def test_zero_attention_vectors_give_the_mean_over_the_terms(built):
    csrs = golden_csrs(built)
    params = AR.random_params(200, 16, 5)
    params["conv1.attn_src"][:] = 0
    params["conv1.attn_dst"][:] = 0
    W1, b1 = params["conv1.weight"].astype(np.float64), params["conv1.bias"].astype(np.float64)
    for rp, cl, vl in csrs:
        f = AR.f64_forward(rp, cl, vl, params)
        n = len(rp) - 1
        T = stepcheck.csr_mm(rp, cl, None if vl is None else vl.astype(np.float64), W1[:n])
        mean = (stepcheck.csr_mm(rp, cl, None, T) + T) / (np.diff(rp) + 1)[:, None]
        assert np.allclose(f["alpha"], 1.0 / (np.diff(rp) + 1)[f["ti"]], rtol=0, atol=1e-15)
        assert np.abs(f["pre"] - (mean + b1)).max() <= 1e-13


# ---- the library: symbols, status codes, workspace sizes, kernels
def test_library_exports_the_attention_symbols(built):
    hip = built.hip
    lib = hip.load()
    for name in NEW:
        assert name in hip.SYMBOLS
        getattr(lib, name)                       # AttributeError without the feature
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "gcnmaxcut.h")).read()
    assert "GMC_K_COUNT = 19" in header          # the new launches reuse tags: the tag list is pinned


def att_call(hip, entry, batch=None, model=None, nbytes=BIG, **a):
    lib = hip.load()
    b = None if batch is None else C.byref(hip.GmcBatch(**batch))
    m = None if model is None else C.byref(hip.GmcModel(**model))
    g = {**dict(a_src=SOME, a_dst=ODD, slope=0.2, ws=SOME, P=SOME, S=None, loss=SOME, grad=SOME), **a}
    if entry == "gmc_att_forward":
        return lib.gmc_att_forward(b, m, g["a_src"], g["a_dst"], g["slope"], 1.0, g["ws"], nbytes, g["P"], g["S"],
                                   g["loss"], None)
    return lib.gmc_att_train_fwd_bwd(b, m, g["a_src"], g["a_dst"], g["slope"], 1.0, g["ws"], nbytes, g["P"], g["S"],
                                     g["loss"], g["grad"], None)


@pytest.mark.parametrize("entry", NEW[1:])
def test_status_codes_of_the_attention_entry_points(built, entry):
    hip = built.hip
    lib = hip.load()
    training = entry == "gmc_att_train_fwd_bwd"
    bf = A.batch_fields()

    def code(**kw):
        kw.setdefault("batch", bf)
        kw.setdefault("model", A.model_fields())
        return att_call(hip, entry, **kw)

    # 1. the struct pointers and the attention vectors (which need no alignment: the default a_dst is odd)
    assert code(batch=None) == -1 and code(model=None) == -1 and code(a_src=None) == -1 and code(a_dst=None) == -1
    # 2. the structs
    assert code(batch={**bf, "abi": 100}) == -8 and code(model=A.model_fields(abi=100)) == -8
    assert code(batch={**bf, "abi": 100}, a_src=None) == -1                    # (1 before 2)
    for f in A.BATCH_PTRS:
        assert code(batch={**bf, f: None}) == -1, f
    for f in ("W1", "b1", "W2", "b2"):
        assert code(model=A.model_fields(**{f: None})) == -1, f
    for K in (2, 4, 8, 0):
        assert code(model=A.model_fields(K=K)) == -3, K                        # three classes only
    assert code(model=A.model_fields(N=0)) == -2 and code(batch={**bf, "R": -1}) == -2
    assert code(model=A.model_fields(F=30)) == -7 and code(model=A.model_fields(F=4100)) == -7
    assert code(model=A.model_fields(dropout_p=1.0)) == -2
    assert code(model=A.model_fields(dropout_p=0.5)) == -7                     # the attention sequence has no dropout
    assert code(model=A.model_fields(K=2, dropout_p=0.5)) == -3                # (K before dropout_p)
    assert code(batch={**bf, "n_max": 2}) == -6 and code(batch={**bf, "n_max": 4097}) == -6
    assert code(model=A.model_fields(N=48)) == -2                              # more nodes than rows of conv1.weight
    # 3. the slope
    for slope in (-0.1, 1.5, float("nan")):
        assert code(slope=slope) == -2, slope
    assert code(slope=0.0, nbytes=0) == -5 and code(slope=1.0, nbytes=0) == -5
    assert code(slope=-1.0, model=A.model_fields(dropout_p=0.5)) == -7         # (2 before 3)
    # 4. workspace and outputs
    assert code(ws=None) == -1 and code(P=None) == -1
    assert code(ws=None, slope=2.0) == -2                                      # (3 before 4)
    # 5. alignment
    assert code(model=A.model_fields(W1=ODD)) == -4 and code(model=A.model_fields(b1=ODD)) == -4
    if training:
        assert code(grad=None) == -1 and code(grad=ODD) == -4
        assert code(grad=ODD, nbytes=0) == -4                                  # (5 before 6)
        assert code(loss=None) == -1                                           # GMC_MODEL_GRAD_TAIL needs the losses
        assert code(loss=None, model=A.model_fields(flags=0), nbytes=0) == -5
    # 6. the workspace size
    for train_size in (0, 1):
        need = lib.gmc_att_workspace_bytes(C.byref(hip.GmcBatch(**bf)), C.byref(hip.GmcModel(**A.model_fields())),
                                           train_size)
        assert need > 256
        if bool(train_size) == training:
            assert code(nbytes=need - 1) == -5
    if not training:                                                           # returns before any launch
        assert code(batch={**bf, "B": 0, "R": 0, "nnz": 0, "n_max": 0}) == 0


def test_attention_workspace_sizes(built):
    hip = built.hip
    lib = hip.load()
    bf = A.batch_fields(n=100, B=6)                                            # R = nnz = 600
    b = hip.GmcBatch(**bf)

    def size(training, **kw):
        return int(lib.gmc_att_workspace_bytes(C.byref(b), C.byref(hip.GmcModel(**A.model_fields(**kw))), training))

    assert size(1, K=2) == 0 and size(1, K=4) == 0 and size(1, abi=100) == 0
    assert lib.gmc_att_workspace_bytes(None, None, 1) == 0
    up = lambda x: (x + 255) // 256 * 256   # noqa: E731
    R_, nnz, ld, F = 600, 600, 64, 36
    # forward: T and H [R,ld], Z0 [R,3], s_src, s_dst, alpha_self [R], alpha [nnz], each rounded up to 256 bytes
    fwd = 2 * up(R_ * ld * 4) + up(R_ * 3 * 4) + 3 * up(R_ * 4) + up(nnz * 4)
    assert size(0, F=F) == fwd
    # training adds G [R,ld], GY2 [R,4], the column partials [tiles,F,4], db2 partials [B,3], the dW1 scratch, ones / dz_self /
    # ds_src / ds_dst [R], dz [nnz] and the partials of da_src / da_dst [tiles,2,F]
    tiles = (R_ + 63) // 64
    fixed = (up(R_ * ld * 4) + up(R_ * 16) + up(tiles * F * 16) + up(6 * 3 * 4) + 4 * up(R_ * 4) + up(nnz * 4) +
             up(tiles * 2 * F * 4))
    trn = size(1, F=F)
    assert trn >= fwd + fixed and (trn - fwd - fixed) % 256 == 0              # (the rest: the dW1 chunk scratch)
    prev = lib.gmc_set_fuse(0)                                                 # the sequence does not depend on it
    try:
        assert size(1, F=F) == trn and size(0, F=F) == fwd
    finally:
        lib.gmc_set_fuse(prev)


KERNELS = {"att_scores_kernel": 1, "att_fwd_kernel": 2, "att_gy2_scale_kernel": 1, "att_edge_bwd_kernel": 4,
           "att_bwd_t_kernel": 2, "att_avec_part_kernel": 1, "att_avec_fold_kernel": 1}


def test_attention_kernels_are_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for kernel, forms in KERNELS.items():
        assert len([s for s in names if kernel in s]) == forms, (kernel, sorted(s for s in names if kernel in s))
    seen = dict.fromkeys(KERNELS, 0)
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
            for kernel in KERNELS:
                if kernel in fields.get(".name", ""):
                    seen[kernel] += 1
                    assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
                    assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
    assert seen == KERNELS


# ---- the layer1 keyword, the environment switch, the engine's layout, the checkpoint
def test_layer1_keyword_and_environment_switch(built, monkeypatch):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    hip = built.hip
    cfg = T.TrainingConfig(n_nodes=40, hidden_dim=6)
    monkeypatch.delenv(hip.LAYER1_ENV, raising=False)
    assert hip.layer1_name(None) == "graphconv" and hip.layer1_name("attention") == "attention"
    net, _e, opt = T.setup_model_and_optimizer(cfg)
    assert type(net) is T.GCNSoftmax and T.layer1_of(net) == "graphconv" and list(net.state_dict()) == list(KEYS)
    gat, _e, gopt = T.setup_model_and_optimizer(cfg, layer1="attention")
    assert type(gat) is T.GATSoftmax and T.layer1_of(gat) == "attention"
    assert {k: tuple(v.shape) for k, v in gat.state_dict().items()} == {
        "conv1.weight": (40, 6), "conv1.bias": (6,), "conv1.attn_src": (6,), "conv1.attn_dst": (6,),
        "conv2.weight": (6, 3), "conv2.bias": (3,)}
    assert len(gopt.param_groups[0]["params"]) == 7 and len(opt.param_groups[0]["params"]) == 5
    bound = (6 / (6 + 1)) ** 0.5                                               # xavier-uniform of a [hidden, 1] matrix
    for k in ("conv1.attn_src", "conv1.attn_dst"):
        a = gat.state_dict()[k]
        assert 0 < float(a.abs().max()) <= bound + 1e-7
    monkeypatch.setenv(hip.LAYER1_ENV, "attention")                            # read at call time
    assert type(T.setup_model_and_optimizer(cfg)[0]) is T.GATSoftmax
    assert type(T.setup_model_and_optimizer(cfg, layer1="graphconv")[0]) is T.GCNSoftmax
    monkeypatch.setenv(hip.LAYER1_ENV, "gat")
    with pytest.raises(ValueError, match="layer1"):
        T.setup_model_and_optimizer(cfg)
    monkeypatch.delenv(hip.LAYER1_ENV)
    with pytest.raises(ValueError, match="layer1"):
        T.setup_model_and_optimizer(cfg, layer1="gat")
    with pytest.raises(ValueError, match="layer1"):
        T.setup_model_and_optimizer(T.TrainingConfig(n_nodes=40, hidden_dim=6, number_classes=4), layer1="attention")
    with pytest.raises(ValueError, match="layer1"):
        T.train_single_epoch({}, net, opt, None, cfg, layer1="attention")      # the model was built with graphconv
    import inspect
    for fn in (T.setup_model_and_optimizer, T.train_model, T.train_single_epoch, T.load_neural_model):
        assert inspect.signature(fn).parameters["layer1"].default is None, fn
    assert "layer1" not in T.TrainingConfig.__dataclass_fields__


def test_default_initialisation_is_unchanged_by_the_keyword(built, monkeypatch):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.delenv(built.hip.LAYER1_ENV, raising=False)
    cfg = T.TrainingConfig(n_nodes=40, hidden_dim=6)
    torch.manual_seed(4)
    a = T.setup_model_and_optimizer(cfg)[0].state_dict()
    torch.manual_seed(4)
    b = T.setup_model_and_optimizer(cfg, layer1="graphconv")[0].state_dict()
    torch.manual_seed(4)
    w1 = torch.nn.init.xavier_uniform_(torch.empty(40, 6))
    assert all(torch.equal(a[k], b[k]) for k in KEYS) and torch.equal(a["conv1.weight"], w1)


def test_attention_engine_layout_and_constructor(built):
    """Six tensors in one flat buffer, in the order of the library's gradient (the hidden width padded to a multiple of 4 by
    the engine); the constructor's refusals come before any device memory is touched."""
    E = built.engine
    assert E.ATT_PARAM_ORDER == AR.ATT_KEYS and E.PARAM_ORDER == KEYS
    Fp = 8
    assert E.flat_layout(40, Fp, 3, attention=True) == ([0, 40 * Fp, 41 * Fp, 44 * Fp, 44 * Fp + 3, 45 * Fp + 3, 46 * Fp + 3],
                                                        46 * Fp + 3)
    assert E.flat_layout(40, Fp, 3) == ([0, 40 * Fp, 41 * Fp, 44 * Fp, 44 * Fp + 3], 44 * Fp + 3)
    cpu = torch.device("cpu")
    for K, kw in ((2, {}), (4, dict(kway=True)), (3, dict(kway=True))):
        with pytest.raises(ValueError, match="layer1"):
            E.FusedEngine(40, 6, K, device=cpu, attention=True, **kw)
    # nodes without neighbours: refused as DGL refuses them, unless the batch is built for the attention layer
    h = built.from_networkx(AR.with_isolated_node(20, 3, 3))
    with pytest.raises(built.DGLError):
        built.BatchArrays([h])
    b = built.BatchArrays([h], None, allow_zero_degree=True)
    assert b.R == 21 and b.dinv[20] == 1.0 and b.rowptr[21] == b.rowptr[20]


def test_checkpoint_round_trip_of_the_six_keys(built, tmp_path, monkeypatch):
    """train_model's bookkeeping with a scripted loss sequence (no GPU), layer1="attention": the checkpoint holds six
    keys and loads as a GATSoftmax without being told; a graphconv checkpoint keeps loading as a GCNSoftmax."""
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(built.hip.LAYER1_ENV, raising=False)
    for layer1, cls, keys in (("attention", T.GATSoftmax, 6), ("graphconv", T.GCNSoftmax, 4)):
        losses = iter([-10.0, -12.0])
        monkeypatch.setattr(T, "train_single_epoch", lambda *a, **k: next(losses))
        cfg = T.TrainingConfig(n_nodes=40, hidden_dim=6, number_epochs=2, save_directory=f"{layer1}.pth")
        net, best, epoch, _emb, hist = T.train_model({}, cfg, layer1=layer1)
        assert type(net) is cls and (best, epoch, hist) == (-12.0, 1, [-10.0, -12.0])
        ck = torch.load(f"final_{layer1}.pth", weights_only=False)
        assert len(ck["model"]) == keys and ("conv1.attn_src" in ck["model"]) == (layer1 == "attention")
        loaded, _inputs, _cfg = T.load_neural_model(f"final_{layer1}.pth", cfg)
        assert type(loaded) is cls
        for k, v in net.state_dict().items():
            assert torch.equal(v.cpu(), loaded.state_dict()[k].cpu()), k
    with pytest.raises(RuntimeError):                                          # told otherwise: the keys do not fit
        T.load_neural_model("final_attention.pth", cfg, layer1="graphconv")


# ---- the precondition of the GPU cases
@pytest.mark.parametrize("case", AR.CASES, ids=AR.case_id)
def test_gpu_cases_are_decided_on_the_float64_reference(built, case):
    handles = [built.from_networkx(g) for g in AR.case_graphs(case)]
    csrs = [KR.csr_of_handle(h) for h in handles]
    assert any(c[2] is not None for c in csrs) == (case.weights == "real")
    params = AR.case_params(case)
    ref, gaps = AR.f64_step(csrs, params, 1.3, case.loss)
    assert gaps["margin"] >= AR.MARGIN, (AR.case_id(case), gaps)
    assert gaps["kink"] >= AR.KINK, (AR.case_id(case), gaps)
    assert gaps["zgap"] >= AR.ZGAP, (AR.case_id(case), gaps)
    assert gaps["leak"] <= AR.CONDITION, (AR.case_id(case), gaps)
    p32, rows32 = AR.float32_yardstick(csrs, params, 1.3, case.loss, ref)
    assert rows32 <= AR.CONDITION, (AR.case_id(case), rows32)
    assert p32 <= stepcheck.PROB_TOL / 4, (AR.case_id(case), p32)             # (the probability bar of the GPU test stays below PROB_TOL)
    # stepcheck.near_tie_rows excuses nothing: with the reference's own decode as the device's, at the tightest bar
    off = 0
    for rp, _cl, _vl in csrs:
        n = len(rp) - 1
        P = ref.P[off:off + n]
        assert stepcheck.near_tie_rows(P, stepcheck.f64_partition(P.copy()), 0.0, AR.case_id(case)) == 0
        off += n
    if case.seed:                                                              # the first seed for which all of it holds
        for seed in range(case.seed):
            earlier = AR.case_params(case._replace(seed=seed))
            r, g = AR.f64_step(csrs, earlier, 1.3, case.loss)
            assert (g["margin"] < AR.MARGIN or g["kink"] < AR.KINK or g["zgap"] < AR.ZGAP or g["leak"] > AR.CONDITION or
                    AR.float32_yardstick(csrs, earlier, 1.3, case.loss, r)[1] > AR.CONDITION), (AR.case_id(case), seed)


def test_case_list_covers_the_promised_shapes(built):
    cases = AR.CASES
    for shape in AR.SHAPES:
        assert {(c.weights, c.loss) for c in cases if c.shape == shape} >= {("unit", "cut"), ("real", "expected_cut")}
    assert {AR.SHAPES[s][1] for s in AR.SHAPES} >= {4, 12, 260, 516}
    degs = {s: [np.diff(KR.csr_of_handle(built.from_networkx(g))[0]) for g in AR.case_graphs(AR.Case(s, "unit", "cut", 0))]
            for s in AR.SHAPES}
    assert [len(d) for d in degs["n3"]] == [3] and [len(d) for d in degs["n4"]] == [4]
    assert degs["deg0"][0].min() == 0
    assert degs["star70"][0].max() + 1 == 71 and degs["star140"][0].max() + 1 == 141   # terms of the hub rows
    assert [len(d) for d in degs["n65"]] == [65] and [len(d) for d in degs["n1030"]] == [1030]
    assert [len(d) for d in degs["batch3"]] == [60, 97, 5]
    assert (degs["d12"][0] == 12).all()
    loop = KR.csr_of_handle(built.from_networkx(AR.with_self_loop(30, 4, 4)))
    rows = np.repeat(np.arange(30), np.diff(loop[0]))
    assert ((rows == loop[1]).sum(), rows[rows == loop[1]].tolist()) == (1, [7])


def test_explicit_layer1_and_checkpoint_keys_beat_the_environment(built, tmp_path, monkeypatch):
    """With GCN_MAXCUT_LAYER1=attention set, an explicit layer1="graphconv" still builds a GCNSoftmax, and a checkpoint
    loads as what its keys say - told or not; without the keyword the environment decides."""
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.chdir(tmp_path)
    cfg = T.TrainingConfig(n_nodes=40, hidden_dim=6, number_epochs=1, save_directory="m.pth")
    monkeypatch.delenv(built.hip.LAYER1_ENV, raising=False)
    monkeypatch.setattr(T, "train_single_epoch", lambda *a, **k: -1.0)
    plain, *_ = T.train_model({}, cfg)                                         # a four-key checkpoint: final_m.pth
    assert type(plain) is T.GCNSoftmax
    os.rename("final_m.pth", "graphconv.pth")
    gat, *_ = T.train_model({}, cfg, layer1="attention")
    os.rename("final_m.pth", "attention.pth")
    monkeypatch.setenv(built.hip.LAYER1_ENV, "attention")
    assert type(T.train_model({}, cfg, layer1="graphconv")[0]) is T.GCNSoftmax
    assert type(T.train_model({}, cfg)[0]) is T.GATSoftmax
    for kw in ({}, {"layer1": "graphconv"}):
        loaded, _inputs, _cfg = T.load_neural_model("graphconv.pth", cfg, **kw)
        assert type(loaded) is T.GCNSoftmax
        for k, v in plain.state_dict().items():
            assert torch.equal(v.cpu(), loaded.state_dict()[k].cpu()), k
    monkeypatch.setenv(built.hip.LAYER1_ENV, "graphconv")
    for kw in ({}, {"layer1": "attention"}):
        loaded, _inputs, _cfg = T.load_neural_model("attention.pth", cfg, **kw)
        assert type(loaded) is T.GATSoftmax
        for k, v in gat.state_dict().items():
            assert torch.equal(v.cpu(), loaded.state_dict()[k].cpu()), k
    assert type(T.train_model({}, cfg, layer1="attention")[0]) is T.GATSoftmax


def test_layer1_through_train_from_pickle_and_train_multi_class(built, tmp_path, monkeypatch):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(built.hip.LAYER1_ENV, raising=False)
    monkeypatch.setattr(T, "train_single_epoch", lambda *a, **k: -1.0)
    monkeypatch.setattr(T, "open_file", lambda f: {})
    kw = dict(n_nodes=40, hidden_dim=6, number_epochs=1)
    assert type(T.train_from_pickle("x.pkl", "a", layer1="attention", **kw)[0]) is T.GATSoftmax
    assert type(T.train_from_pickle("x.pkl", "b", **kw)[0]) is T.GCNSoftmax
    assert type(T.train_multi_class("x.pkl", "c", num_classes=3, layer1="attention", **kw)[0]) is T.GATSoftmax
    assert type(T.train_multi_class("x.pkl", "d", num_classes=3, layer1="graphconv", **kw)[0]) is T.GCNSoftmax
    assert "conv1.attn_src" in torch.load("final_c.pth", weights_only=False)["model"]
    with pytest.raises(ValueError, match="layer1"):
        T.train_multi_class("x.pkl", "e", num_classes=2, layer1="attention", **kw)
    monkeypatch.setenv(built.hip.LAYER1_ENV, "attention")                      # the switch reaches them as well
    assert type(T.train_from_pickle("x.pkl", "f", **kw)[0]) is T.GATSoftmax
