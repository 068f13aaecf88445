"""CPU checks of one model per graph beyond 4096 nodes (include/gcnmaxcut.h, gmc_inst_large_*; engine.LargeInstanceEngine;
maxcut.solve_large): the status codes of the three entry points in the documented order (fake pointers: no call reaches a
launch), the workspace formula, the kernels' instantiations, the Python refusals, `subset` keeping the caller's class, and
the preconditions of the GPU cases of tests/test_gpu_large_instance.py on the float64 reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from tests import instance_ref as IR
from tests import large_instance_ref as LI
from tests import large_ref as LR
from tests import kway_ref as KR
from tests import plain_ref as PR
from tests import test_api_status as A
from tests import stepcheck, util
from tests.stepcheck import KEYS

SOME, ODD, BIG = A.SOME, A.ODD, A.BIG
LARGE = 1 << 20
ENTRIES = ("gmc_inst_large_forward", "gmc_inst_large_train_fwd_bwd")


# ---- status codes (fake pointers: no call reaches a launch)
def large_call(hip, entry, batch=None, model=None, nbytes=BIG, terminals=1, **a):
    lib = hip.load()
    b = None if batch is None else C.byref(hip.GmcBatch(**batch))
    m = None if model is None else C.byref(hip.GmcModel(**model))
    g = {**dict(ws=SOME, P=SOME, S=None, loss=SOME, grad=SOME), **a}
    if entry == "gmc_inst_large_forward":
        return lib.gmc_inst_large_forward(b, m, terminals, 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], None)
    return lib.gmc_inst_large_train_fwd_bwd(b, m, terminals, 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], g["grad"], None)


def imodel(**kw):
    return A.model_fields(**{"K": 4, "N": 120, "flags": 0, **kw})       # N = the batch's rows (2 graphs of 60)


@pytest.mark.parametrize("entry", ENTRIES)
def test_status_codes_of_the_large_instance_entry_points(built, entry):
    hip = built.hip
    lib = hip.load()
    training = entry == "gmc_inst_large_train_fwd_bwd"
    bf = A.batch_fields()
    assert entry in hip.SYMBOLS and "gmc_inst_large_workspace_bytes" in hip.SYMBOLS

    def code(**kw):
        kw.setdefault("batch", bf)
        kw.setdefault("model", imodel())
        return large_call(hip, entry, **kw)

    # 1. the structs and their abi word
    assert code(batch=None) == -1 and code(model=None) == -1
    assert code(batch={**bf, "abi": 100}) == -8 and code(model=imodel(abi=100)) == -8
    assert code(batch={**bf, "abi": 100, "goff": None}, model=imodel(K=9)) == -8
    # 2. pointers, the class count, the shapes - `terminals` among them -, the hidden width, dropout
    for f in A.BATCH_PTRS:
        assert code(batch={**bf, f: None}) == -1, f
    for f in ("W1", "b1", "W2", "b2"):
        assert code(model=imodel(**{f: None})) == -1, f
    assert code(batch={**bf, "goff": None}, model=imodel(K=9)) == -1
    for K in (1, 9, 0, -3):
        assert code(model=imodel(K=K)) == -3, K
        assert code(model=imodel(K=K), terminals=2) == -3, K                   # (the class count before the flag)
    for K in range(2, 9):
        assert code(model=imodel(K=K), nbytes=0) == -5, K
    for t in (-1, 2, 256):
        assert code(terminals=t) == -2, t
        assert code(terminals=t, model=imodel(F=30)) == -2, t                  # (the flag before F % 4)
    assert code(model=imodel(N=-1)) == -2 and code(batch={**bf, "R": -1}) == -2 and code(model=imodel(F=0)) == -2
    assert code(model=imodel(F=30)) == -7 and code(model=imodel(F=4100)) == -7
    assert code(model=imodel(F=30, dropout_p=1.0)) == -7                       # (F % 4 before dropout)
    assert code(model=imodel(dropout_p=1.0)) == -2
    assert code(model=imodel(dropout_p=0.5)) == -7
    assert code(model=imodel(K=1, dropout_p=0.5)) == -3
    assert code(model=imodel(W1_slab=ODD)) == -4
    # the graph size: n_max = K - 1 refused with terminals and accepted without; the upper bound is 2^20 for both
    assert code(batch={**bf, "n_max": 3}, terminals=1) == -6
    assert code(batch={**bf, "n_max": 3}, terminals=0, nbytes=0) == -5
    assert code(batch={**bf, "n_max": 0}, terminals=0) == -6                   # a graph needs one node
    assert code(batch={**bf, "n_max": 4}, nbytes=0) == -5
    assert code(model=imodel(dropout_p=0.5), batch={**bf, "n_max": 3}) == -7   # (dropout before the graph size)
    for t in (0, 1):
        for n_max in (4097, 5000, LARGE):
            big = {**bf, "R": n_max + 60, "nnz": n_max + 60, "n_max": n_max}
            assert code(batch=big, model=imodel(N=n_max + 60), terminals=t, nbytes=0) == -5, (t, n_max)
            assert code(batch=big, model=imodel(N=n_max + 60, K=8), terminals=t, nbytes=0) == -5, (t, n_max)
        assert code(batch={**bf, "n_max": LARGE + 1}, terminals=t) == -6
        assert code(batch={**bf, "n_max": LARGE + 1}, model=imodel(N=1000), terminals=t) == -6   # (graph size before N != R)
    # N != R: one W1 row per node of the batch
    assert code(model=imodel(N=1000)) == -2 and code(model=imodel(N=60)) == -2
    assert code(ws=None, model=imodel(N=1000)) == -2                           # (step 2 before step 4)
    # 4. workspace and outputs, 5. alignment, 6. the workspace size
    assert code(ws=None) == -1 and code(P=None) == -1
    assert code(P=ODD) == -4 and code(model=imodel(W2=ODD)) == -4 and code(model=imodel(W1=ODD)) == -4
    assert code(model=imodel(W1=ODD), ws=None) == -1 and code(model=imodel(W1=ODD), nbytes=0) == -4
    assert code(P=ODD, ws=None) == -1                                          # (step 4 before step 5)
    if training:
        assert code(grad=None) == -1 and code(grad=ODD) == -4
        assert code(grad=ODD, nbytes=0) == -4                                  # (step 5 before step 6)
    assert code(loss=None, nbytes=0) == -5 and code(S=SOME, nbytes=0) == -5    # loss and S are optional
    for train_size in (0, 1):
        need = lib.gmc_inst_large_workspace_bytes(C.byref(hip.GmcBatch(**bf)), C.byref(hip.GmcModel(**imodel())), train_size)
        assert need > 256
        if bool(train_size) == training:
            assert code(nbytes=need - 1) == -5
    # an empty batch launches nothing
    empty = {**bf, "B": 0, "R": 0, "nnz": 0, "n_max": 0}
    for t in (0, 1):
        assert code(batch=empty, model=imodel(N=0), terminals=t) == 0


def test_large_instance_workspace_is_the_instance_workspace_plus_the_head_scratch(built):
    hip = built.hip
    lib = hip.load()
    up = lambda x: (x + 255) // 256 * 256   # noqa: E731
    for n, B in ((100, 6), (5000, 1), (70000, 2)):
        b = hip.GmcBatch(**A.batch_fields(n=n, B=B))
        R_ = n * B
        for K in range(2, 9):
            for F in (32, 500):
                m = hip.GmcModel(**imodel(K=K, N=R_, F=F))
                for training in (0, 1):
                    inst = int(lib.gmc_inst_workspace_bytes(C.byref(b), C.byref(m), training))
                    large = int(lib.gmc_inst_large_workspace_bytes(C.byref(b), C.byref(m), training))
                    # the header: Sw [R], the head's tile partials [R / 256 + B + 1][K + 1], training: dinv o GZ [R,K]
                    extra = up(R_ * 4) + up((R_ // LR.T + B + 1) * (K + 1) * 4) + (up(R_ * K * 4) if training else 0)
                    assert inst > 0 and large == inst + extra, (n, B, K, F, training)
                    ld = (F + 31) // 32 * 32
                    want = 2 * up(R_ * ld * 4) + up(R_ * K * 4) + extra
                    if training:
                        want += up(R_ * K * 4) + up((R_ // 64 + B + 1) * F * (K + 1) * 4)
                    assert large == want, (n, B, K, F, training)
    # about 8 * ld bytes per node, as the header states: the two [R, ld] buffers are all that grows with F
    b = hip.GmcBatch(**A.batch_fields(n=70000, B=1))
    m = hip.GmcModel(**imodel(K=3, N=70000, F=64))
    per_node = lib.gmc_inst_large_workspace_bytes(C.byref(b), C.byref(m), 1) / 70000
    assert 8 * 64 <= per_node <= 8 * 64 + 4 * (3 * 3 + 1) + 4 * 4 + 1
    b = hip.GmcBatch(**A.batch_fields())
    assert lib.gmc_inst_large_workspace_bytes(None, None, 1) == 0
    assert lib.gmc_inst_large_workspace_bytes(C.byref(b), C.byref(hip.GmcModel(**imodel(K=9))), 1) == 0
    assert lib.gmc_inst_large_workspace_bytes(C.byref(b), C.byref(hip.GmcModel(**imodel(abi=100))), 1) == 0


# ---- the kernels
NEW_KERNELS = ("linst_hw2_kernel", "linst_prob_kernel", "linst_loss_kernel", "linst_fold_kernel", "linst_gy2_kernel")


def test_no_instantiation_of_the_new_kernels_is_missing_and_none_uses_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = [s for s in util.kernel_symbols(lib_path) if "linst_" in s]
    for K in range(2, 9):
        for kernel in ("linst_hw2_kernel", "linst_prob_kernel", "linst_fold_kernel", "linst_gy2_kernel"):
            assert any(f"{kernel}<{K}>" in s for s in names), (kernel, K)
        for soft in ("true", "false"):
            assert any(f"linst_loss_kernel<{K}, {soft}>" in s for s in names), (K, soft)
    seen = dict.fromkeys(NEW_KERNELS, 0)
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
            for kernel in NEW_KERNELS:
                if kernel in fields.get(".name", ""):
                    seen[kernel] += 1
                    assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
                    assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
    assert seen == {"linst_hw2_kernel": 7, "linst_prob_kernel": 7, "linst_loss_kernel": 14, "linst_fold_kernel": 7,
                    "linst_gy2_kernel": 7}


# ---- Python: size checks, refusals, subset
def test_large_instance_engine_size_checks_need_no_gpu(built):
    engine = built.engine
    assert issubclass(engine.LargeInstanceEngine, engine.InstanceEngine)
    engine.check_large_instance_sizes([5, 4097, LARGE], 3)
    engine.check_large_instance_sizes([12, 6, 3, 5000], 8, terminals=False)     # the minimum is waived without terminals
    with pytest.raises(ValueError, match="at least 8 nodes"):
        engine.check_large_instance_sizes([12, 6, 5000], 8)                     # ... and holds with them
    with pytest.raises(ValueError, match="at least one node"):
        engine.check_large_instance_sizes([12, 0], 2, terminals=False)
    with pytest.raises(ValueError, match=str(LARGE)):
        engine.check_large_instance_sizes([LARGE + 1], 2, terminals=False)
    # the one-workgroup engine keeps refusing, and may name the way out
    with pytest.raises(ValueError, match="beyond the one-workgroup head"):
        engine.check_instance_sizes([5000], 2, terminals=False)
    with pytest.raises(ValueError, match="train_model"):
        engine.check_instance_sizes([4097], 3)
    # the segmented Adam's bound: n_max * F / 4 float4 in tiles of 1024, plus the tiles of the small blocks, at most 65,535
    assert not engine.inst_adam_too_large(LARGE, 64, 3) and not engine.inst_adam_too_large(LARGE, 252, 3)
    assert engine.inst_adam_too_large(LARGE, 256, 3) and engine.inst_adam_too_large(70000, 4096, 8)
    assert not engine.inst_adam_too_large(4096, 4096, 8)
    some = C.c_void_p(4096)
    for n_max, F, K in ((LARGE, 256, 3), (70000, 4096, 8), (65535 * 1024, 4, 2)):   # the library agrees (GMC_ERR_SHAPE)
        assert engine.inst_adam_too_large(n_max, F, K)
        b = built.hip.GmcBatch(B=1, R=n_max, nnz=0, n_max=n_max, goff=4096)
        assert built.hip.load().gmc_inst_adam_f32(C.byref(b), F, K, some, some, some, some, 1e-3, 0.9, 0.999, 1e-8, 1, None,
                                                  None) == -2
    assert not engine.inst_adam_too_large(65534 * 1024, 4, 2)                       # 65,534 tiles of W1 and one of the rest
    for method in ("forward", "train_fwd_bwd", "workspace_bytes"):
        assert getattr(engine.LargeInstanceEngine, method) is getattr(engine.InstanceEngine, method)
    assert engine.LargeInstanceEngine._TRAIN == "gmc_inst_large_train_fwd_bwd"
    assert engine.InstanceEngine._TRAIN == "gmc_inst_train_fwd_bwd_t"


def test_solve_large_refusals_need_no_gpu(built):
    import inspect
    from gcn_max_cut_amd import maxcut
    for a, b in ((maxcut.solve, maxcut.solve_large), (maxcut.solve_batch, maxcut.solve_large_batch)):
        assert inspect.signature(a) == inspect.signature(b)
    ei = np.zeros((2, 0), np.int64)
    kw = dict(hidden_dim=8, epochs=1, learning_rate=0.01)
    with pytest.raises(ValueError, match="number_classes"):
        maxcut.solve_large(ei, num_nodes=5000, number_classes=9, **kw)
    with pytest.raises(ValueError, match="number_classes"):
        maxcut.solve_large(ei, num_nodes=5000, number_classes=1, **kw)
    with pytest.raises(ValueError, match="unknown loss"):
        maxcut.solve_large(ei, num_nodes=5000, loss="hinge", **kw)
    with pytest.raises(ValueError, match=str(LARGE)):
        maxcut.solve_large(ei, num_nodes=LARGE + 1, **kw)                       # (GraphBatch.from_edge_index's own bound)
    # solve keeps refusing 5000 nodes before it needs a GPU, names the old route and now the new one too
    with pytest.raises(ValueError, match=r"functional.*search_large_dataset\(\.\.\., terminals=False\)"):
        maxcut.solve(ei, num_nodes=5000, **kw)
    with pytest.raises(ValueError, match="solve_large"):
        maxcut.solve(ei, num_nodes=5000, **kw)
    with pytest.raises(ValueError, match="beyond the one-workgroup head"):
        maxcut.solve(ei, ptr=np.array([0, 10, 5010]), **kw)


class StubBatch:
    """What an engine's constructor and `subset` read of a GraphBatch, on the CPU."""

    def __init__(self, handles, values=None, device=None):
        self.sizes = [h.n for h in handles]
        self.B, self.R, self.n_max = len(handles), sum(self.sizes), max(self.sizes, default=0)
        self.goff_host = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.device = torch.device("cpu")


@pytest.mark.parametrize("cls", ("InstanceEngine", "LargeInstanceEngine"))
def test_subset_returns_an_engine_of_the_callers_class(built, monkeypatch, cls):
    engine = built.engine
    monkeypatch.setattr(engine, "GraphBatch", StubBatch)
    monkeypatch.setattr(engine.hip, "load", lambda: None)
    sizes = [5, 300, 4096] if cls == "InstanceEngine" else [5, 300, 4100]
    handles = [built.GraphHandle(*LR.circulant(n, 4)) for n in sizes]
    eng = getattr(engine, cls)(handles, 6, 3, torch.device("cpu"), terminals=False)
    assert type(eng) is getattr(engine, cls) and eng.Fp == 8
    eng.flat.copy_(torch.arange(eng.flat.numel(), dtype=torch.float32))
    eng.best_S.copy_(torch.arange(eng.R, dtype=torch.int32))
    eng.best_loss.copy_(torch.tensor([-1.0, -2.0, -3.0]))
    eng.step_count = 7
    sub = eng.subset([0, 2])
    assert type(sub) is type(eng) and sub.terminals is False and sub.step_count == 7
    assert sub.batch.sizes == [sizes[0], sizes[2]] and sub.best_loss.tolist() == [-1.0, -3.0]
    for g_sub, g in enumerate((0, 2)):
        for k in KEYS:
            assert torch.equal(sub.views(g_sub)[k], eng.views(g)[k]), (g, k)
    r2 = int(eng.batch.goff_host[2])
    assert sub.best_S.tolist() == list(range(5)) + list(range(r2, r2 + sizes[2]))
    # beyond the segmented Adam's bound the engine raises before it calls the library (there is none here), naming the bound
    monkeypatch.setattr(engine, "inst_adam_too_large", lambda n_max, F, K: (n_max, F, K) == (sizes[2], 8, 3))
    with pytest.raises(ValueError, match=r"segmented Adam's bound of 65535 tiles"):
        eng.adam_step(1e-3, running_only=True)
    if cls == "InstanceEngine":
        with pytest.raises(ValueError, match="beyond the one-workgroup head"):
            engine.InstanceEngine([built.GraphHandle(*LR.circulant(4097, 4))], 6, 3, torch.device("cpu"))


# ---- the reference is instance_ref's with terminals and plain_ref's without
def step_is_the_named_reference(loss):
    csr = LI.case_csrs(LI.Case("n255", 4, "real", loss, 1, 0))[0]
    p = KR.random_params(255, 20, 4, 3)
    with_t, ref = LI.step(csr, p, 1.3, loss, 1), IR.graph_step(csr, p, 1.3, loss)
    assert np.array_equal(with_t.P, ref.P) and with_t.loss == ref.loss[0]
    assert all(np.array_equal(with_t.grads[k], ref.grads[k]) for k in KEYS)
    without, (f, value, grads) = LI.step(csr, p, 1.3, loss, 0), PR.inst_step(csr, p, 1.3, loss)
    assert np.array_equal(without.P, f["P"]) and without.loss == value
    assert all(np.array_equal(without.grads[k], grads[k]) for k in KEYS)
    assert not np.array_equal(without.grads[KEYS[0]], with_t.grads[KEYS[0]])


# ---- the preconditions of the GPU cases
@pytest.mark.parametrize("case", LI.CASES + LI.COMPARE, ids=LI.case_id)
def test_gpu_cases_are_decided_on_the_float64_reference(built, case):
    sizes = LI.case_sizes(case)
    built.engine.check_large_instance_sizes(sizes, case.K, terminals=bool(case.terminals))   # a batch the engine takes
    if case in LI.COMPARE:
        built.engine.check_instance_sizes(sizes, case.K, terminals=bool(case.terminals))     # ... and InstanceEngine too
    r = LI.rules(case)
    what = (LI.case_id(case), r)
    if LI.is_big(case):
        assert r.gap >= LR.BIG_GAP and r.ties <= LR.MAX_TIES, what
    else:
        assert r.margin >= KR.MARGIN and r.gap >= KR.KINK and r.unsaturated >= LR.UNSATURATED, what
    assert r.ratio <= 0.5, what                                                # half of ROW_TOL, in units of ROW_TOL
    assert r.hub <= 0.5, what                                                  # half of P_TOL on every hub row
    assert stepcheck.ROW_TOL == 2e-4 and stepcheck.P_TOL == 5e-7


def test_case_list_covers_what_it_promises(built):
    for loss in ("cut", "expected_cut"):
        step_is_the_named_reference(loss)
    # every earlier seed of a case that records one misses a rule
    for spec, seed in LI.SEEDS.items():
        assert spec in LI._LIST, spec
        for earlier in range(seed):
            assert not LI.well_posed(LI.Case(*spec, earlier)), (spec, earlier)
    # the shapes the one-workgroup engine refuses are the ones meant to be beyond it
    refused = set()
    for c in LI.CASES:
        try:
            built.engine.check_instance_sizes(LI.case_sizes(c), c.K, c.loss, terminals=bool(c.terminals))
        except ValueError as e:
            assert "beyond the one-workgroup head" in str(e) and "LargeInstanceEngine" in str(e), (LI.case_id(c), e)
            refused.add(c.shape)
    assert refused == {"n4097", "k8n2500", "star4200", "hubring4201", "star4200hub0", "n70000", "n2^20"}
    shapes = {c.shape for c in LI.CASES}
    assert {"n255", "n256", "n257", "n515", "batch", "nK", "nK1", "path3", "n4097", "k8n2500", "star4200", "hubring4201",
            "star4200hub0", "n70000", "n2^20"} == shapes
    for field, values in (("K", (2, 3, 4, 8)), ("weights", ("unit", "real")), ("loss", ("cut", "expected_cut")),
                          ("terminals", (0, 1))):
        for v in values:
            assert sum(getattr(c, field) == v for c in LI.CASES) >= 5, (field, v)
    assert LI.case_sizes(LI.Case("batch", 3, "unit", "cut", 1, 0)) == [5, 700, 257]
    assert LI.case_sizes(LI.Case("path3", 8, "unit", "cut", 0, 0)) == [3]
    assert LI.case_sizes(LI.Case("mixed", 3, "unit", "cut", 1, 0)) == [5, 300, 65, 257]
    assert LI.HIDDEN == {2: 4, 3: 12, 4: 20, 5: 260, 8: 516}
    assert len(LI.COMPARE) == 16
    for c in LI.CASES:
        if c.shape in ("star4200", "hubring4201", "star4200hub0"):
            assert max(int(np.diff(rp).max()) for rp, _cl, _w in LI.case_csrs(c)) >= 4200   # a hub row
