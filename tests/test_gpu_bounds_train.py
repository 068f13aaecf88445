"""Guard-band tests of the forward and training entry points: every array of the batch and the model, every input,
output and the workspace - at exactly the size its query returns - comes from one arena with 4096-byte bands between
them (tests/arena.py); each case runs on plain tensors, on an arena filled 0xFF and on one filled 0x00, and
tests/bounds.run_case asserts the four byte equalities listed in tests/bounds.py.  Calls go straight through ctypes,
never through the engines (their workspace only grows, which is part of the gap these tests close).

Batches (tests/bounds.graphs_of): odd (n = 5, 67, 13), hub (a row of 70 entries, real weights, overflow lists), tile
(n = 257 + 8), trip (n = 1030).  Hidden widths 4, 20, 516; K in 2, 5, 8 on the K-class entry points (with terminals the
n = 5 graph of `odd` is replaced by n = 9 at K = 8: the header leaves a graph of fewer than K nodes to the caller).

Measured on the MI355X: 927 cases (3042 calls of entry points), no band touched, no pair of runs different.
Alone (-s prints the counts) the file's 74 tests take 5.6 s, library load and GPU start-up included; the slowest is
test_forward_and_train_fwd_bwd[gmc_forward-0-4-1] at 0.23 s (the first to touch the GPU), then
test_backward_from_gp_and_the_features_trio[4] at 0.19 s and test_instance_models[516-2] at 0.12 s.
DESIGN.md section 37 holds the case table.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bounds as B

pytestmark = pytest.mark.gpu

WIDTHS = (4, 20, 516)
CLASSES = (2, 5, 8)
LOSSES = (0, 2)                       # gmc_model.flags: GMC_LOSS_CUT, GMC_MODEL_LOSS_EXPECTED
HYPER = (1e-2, 0.9, 0.999, 1e-8)
CUT_C = 1.5


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    done = B.report_calls("bounds/train")
    yield built
    done()


def kind_for(kind, K, terminals=True):
    """`odd` with its n = 5 graph replaced by n = 9 where every graph must hold K = 8 terminals."""
    return "odd9" if kind == "odd" and terminals and K > 5 else kind


def grad_floats(h, N, F, K, flags, inst=False, att=False):
    if inst:
        return h.R * F + h.B * (F + F * K + K)
    return N * F + F + F * K + K + (2 * F if att else 0) + (flags & 1)


def model_call(pkg, entry, query, kind, F, K, training, *, flags=0, inst=False, terminals=None, cost=None, att=False,
               optional=True, slab=False, dropout=0.0, table=True, seed=3):
    """A case for the entry points of the shape (batch, model, [terminals, [node_cost]], [a_src, a_dst, slope], C,
    workspace, bytes, P, S, loss, [grad]).  cost: None = the entry point takes none; False = NULL; True = real costs."""
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    N = h.R if inst else h.n_max
    rng = np.random.RandomState(seed + F + K)
    arrs = B.model_arrays(N, F, K, seed, (h.R, h.B) if inst else None)
    node_cost = rng.uniform(-1, 1, (h.R, K)).astype(np.float32)
    a_src, a_dst = (rng.uniform(-1, 1, F).astype(np.float32) for _ in range(2))

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h, table)
        mc = B.device_model(pkg, mem, arrs, N, F, K, flags, slab, dropout)
        pre = []
        if terminals is not None:
            pre.append(int(terminals))
        if cost is not None:
            pre.append(p(mem.put("node_cost", node_cost)) if cost else None)
        if att:
            pre += [p(mem.put("a_src", a_src)), p(mem.put("a_dst", a_dst)), 0.2]
        nbytes = int(getattr(lib, query)(C.byref(bc), C.byref(mc), int(training)))
        assert nbytes > 0
        ws = mem.scratch("workspace", nbytes)
        P = mem.out("P", (h.R, K))
        S = mem.out("S", (h.R,), torch.int32) if optional else None
        loss = mem.out("loss", (h.B,)) if optional or flags & 1 else None
        args = [C.byref(bc), C.byref(mc), *pre, CUT_C, p(ws), nbytes, p(P), p(S), p(loss)]
        if training:
            args.append(p(mem.out("grad", (grad_floats(h, N, F, K, flags, inst, att),))))
        return getattr(lib, entry)(*args, B.stream(pkg))
    return case


# ---- the 3-class fused entry points ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", (1, 0))
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("entry,training", (("gmc_forward", 0), ("gmc_train_fwd_bwd", 1)))
def test_forward_and_train_fwd_bwd(pkg, entry, training, F, fuse):
    with B.util.fused(pkg, fuse):
        for slab in (False, True):
            for flags in LOSSES + ((1, 3) if training else ()):        # the tail slot with either loss
                for optional in (True, False):
                    if not optional and (training or flags):            # the loss kind only shows with S / loss there
                        continue
                    B.run_case(pkg, model_call(pkg, entry, "gmc_workspace_bytes", "odd", F, 3, training, flags=flags,
                                               slab=slab, optional=optional))
        for kind in ("hub", "trip", "tile"):
            B.run_case(pkg, model_call(pkg, entry, "gmc_workspace_bytes", kind, F, 3, training, slab=True))
        B.run_case(pkg, model_call(pkg, entry, "gmc_workspace_bytes", "odd", F, 3, training, dropout=0.5))
        B.run_case(pkg, model_call(pkg, entry, "gmc_workspace_bytes", "hub", F, 3, training, table=False))


def step_case(pkg, kind, F, loss_kind, slab, plain_entry=False):
    """gmc_train_step_loss_f32 (plain_entry: gmc_train_step_f32, its GMC_LOSS_CUT twin)."""
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    N = h.n_max
    count = N * F + F + F * 3 + 3
    arrs = B.model_arrays(N, F, 3, 5)
    flat = np.concatenate([arrs[k].ravel() for k in ("W1", "b1", "W2", "b2")])
    rng = np.random.RandomState(F)
    m0 = rng.uniform(-1e-3, 1e-3, count).astype(np.float32)
    v0 = rng.uniform(0, 1e-3, count).astype(np.float32)

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h)
        param = mem.state("param", flat)
        m, v = mem.state("m", m0), mem.state("v", v0)
        counter = mem.state("step_counter", np.asarray([4], np.int32))
        w1_slab = mem.state("w1_slab", B.util._slab_of(arrs["W1"])) if slab else None
        model = pkg.hip.GmcModel(N=N, F=F, K=3)
        nbytes = int(lib.gmc_workspace_bytes(C.byref(bc), C.byref(model), 1))
        ws = mem.scratch("workspace", nbytes)
        P, S, loss = mem.out("P", (h.R, 3)), mem.out("S", (h.R,), torch.int32), mem.out("loss", (h.B,))
        grad = mem.out("grad", (count,))
        head = [C.byref(bc), N, F, p(param), CUT_C]
        tail = [p(ws), nbytes, p(P), p(S), p(loss), p(grad), p(m), p(v), *HYPER, p(counter), p(w1_slab), B.stream(pkg)]
        if plain_entry:
            return lib.gmc_train_step_f32(*head, *tail)
        return lib.gmc_train_step_loss_f32(*head, loss_kind, *tail)
    return case


@pytest.mark.parametrize("F", WIDTHS)
def test_train_step(pkg, F):
    for loss_kind in (0, 1):
        for slab in (False, True):
            B.run_case(pkg, step_case(pkg, "odd", F, loss_kind, slab))
    B.run_case(pkg, step_case(pkg, "odd", F, 0, True, plain_entry=True))
    for kind in ("hub", "trip"):                       # (trip: a one-graph batch, whose head runs inside the backward)
        B.run_case(pkg, step_case(pkg, kind, F, 0, True))
        B.run_case(pkg, step_case(pkg, kind, F, 1, False))


def from_gp_case(pkg, kind, F, features, fn=False, K=3, dx=True):
    """A forward, then the backward for a caller's dLoss/dP from the same workspace: gmc_forward +
    gmc_backward_from_gp; features: gmc_forward_features + gmc_backward_features_from_gp on X [R, N] with a leading
    dimension rounded up to 4; fn: gmc_fn_forward + gmc_fn_backward (features: with X)."""
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    N = h.n_max
    ldx = (N + 3) // 4 * 4
    rng = np.random.RandomState(F + K)
    X = np.zeros((h.R, ldx), np.float32)
    X[:, :N] = rng.uniform(-1, 1, (h.R, N))
    GP = rng.uniform(-1, 1, (h.R, K)).astype(np.float32)

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h)
        mc = B.device_model(pkg, mem, B.model_arrays(N, F, K, 9), N, F, K)
        b, m = C.byref(bc), C.byref(mc)
        Xd = mem.put("X", X) if features else None
        P = mem.out("P", (h.R, K))
        grad = mem.out("grad", (N * F + F + F * K + K,))
        dX = mem.out("dX", (h.R, ldx)) if features and dx else None
        gp = mem.put("GP", GP)
        s = B.stream(pkg)
        if fn:
            nbytes = int(lib.gmc_fn_workspace_bytes(b, m, int(features)))
            ws = mem.scratch("workspace", nbytes)
            return [lib.gmc_fn_forward(b, m, p(Xd), ldx if features else 0, p(ws), nbytes, p(P), s),
                    lib.gmc_fn_backward(b, m, p(Xd), ldx if features else 0, p(ws), nbytes, p(P), p(gp), p(grad), p(dX),
                                        ldx if dX is not None else 0, s)]
        if features:
            nbytes = int(lib.gmc_workspace_bytes_features(b, m, 1))
            ws = mem.scratch("workspace", nbytes)
            S, loss = mem.out("S", (h.R,), torch.int32), mem.out("loss", (h.B,))
            return [lib.gmc_forward_features(b, m, p(Xd), ldx, CUT_C, p(ws), nbytes, p(P), p(S), p(loss), s),
                    lib.gmc_backward_features_from_gp(b, m, p(Xd), ldx, p(ws), nbytes, p(P), p(gp), p(grad), p(dX),
                                                      ldx if dX is not None else 0, s)]
        nbytes = int(lib.gmc_workspace_bytes(b, m, 1))
        ws = mem.scratch("workspace", nbytes)
        return [lib.gmc_forward(b, m, CUT_C, p(ws), nbytes, p(P), None, None, s),
                lib.gmc_backward_from_gp(b, m, p(ws), nbytes, p(P), p(gp), p(grad), s)]
    return case


def dx_pad(kind, dx):
    """dX is [R, N] with a leading dimension of N rounded up to 4: the columns from N on are no part of it."""
    return {"dX": B.host_batch(kind).n_max} if dx else None


@pytest.mark.parametrize("F", WIDTHS)
def test_backward_from_gp_and_the_features_trio(pkg, F):
    for fuse in (1, 0):
        with B.util.fused(pkg, fuse):
            for kind in ("odd", "hub"):
                B.run_case(pkg, from_gp_case(pkg, kind, F, False))
    for kind in ("odd", "hub"):
        for dx in (True, False):
            B.run_case(pkg, from_gp_case(pkg, kind, F, True, dx=dx), padded=dx_pad(kind, dx))


def forward_features_alone(pkg, kind, F, flags, optional):
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    N = h.n_max
    ldx = (N + 3) // 4 * 4
    X = np.zeros((h.R, ldx), np.float32)
    X[:, :N] = np.random.RandomState(F).uniform(-1, 1, (h.R, N))

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h)
        mc = B.device_model(pkg, mem, B.model_arrays(N, F, 3, 9), N, F, 3, flags)
        nbytes = int(lib.gmc_workspace_bytes_features(C.byref(bc), C.byref(mc), 0))      # the forward-only size
        ws = mem.scratch("workspace", nbytes)
        P = mem.out("P", (h.R, 3))
        S = mem.out("S", (h.R,), torch.int32) if optional else None
        loss = mem.out("loss", (h.B,)) if optional else None
        return lib.gmc_forward_features(C.byref(bc), C.byref(mc), p(mem.put("X", X)), ldx, CUT_C, p(ws), nbytes, p(P),
                                        p(S), p(loss), B.stream(pkg))
    return case


@pytest.mark.parametrize("F", WIDTHS)
def test_forward_features_with_the_forward_workspace(pkg, F):
    for flags in LOSSES:
        B.run_case(pkg, forward_features_alone(pkg, "odd", F, flags, True))
    B.run_case(pkg, forward_features_alone(pkg, "odd", F, 0, False))
    B.run_case(pkg, forward_features_alone(pkg, "hub", F, 2, True))


# ---- K classes: gmc_kway_*, gmc_large_*, the functional form ---------------------------------------------------------
@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("family,other", (("kway", "trip"), ("large", "tile")))
def test_kway_and_large(pkg, family, other, F, K):
    query = f"gmc_{family}_workspace_bytes"
    for entry, training in ((f"gmc_{family}_forward", 0), (f"gmc_{family}_train_fwd_bwd", 1)):
        for flags in LOSSES + ((3,) if training else ()):
            B.run_case(pkg, model_call(pkg, entry, query, kind_for("odd", K), F, K, training, flags=flags))
        if not training:
            B.run_case(pkg, model_call(pkg, entry, query, kind_for("odd", K), F, K, 0, optional=False))
        for kind in (other, "hub"):
            B.run_case(pkg, model_call(pkg, entry, query, kind, F, K, training, flags=2))


@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("F", WIDTHS)
def test_functional_forward_backward(pkg, F, K):
    for features in (False, True):
        for kind in ("odd", "hub", "tile"):
            B.run_case(pkg, from_gp_case(pkg, kind, F, features, fn=True, K=K), padded=dx_pad(kind, features))
    B.run_case(pkg, from_gp_case(pkg, "odd", F, True, fn=True, K=K, dx=False))


def fn_cut_loss_case(pkg, kind, K, terminals, loss_kind, want_gp):
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    Pm = np.random.RandomState(K).dirichlet(np.ones(K), h.R).astype(np.float32)

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h)
        nbytes = int(lib.gmc_fn_cut_loss_workspace_bytes(C.byref(bc), K))
        ws = mem.scratch("workspace", nbytes)
        loss = mem.out("loss", (h.B,))
        GP = mem.out("GP", (h.R, K)) if want_gp else None
        return lib.gmc_fn_cut_loss_f32(C.byref(bc), K, terminals, p(mem.put("P", Pm)), CUT_C, loss_kind, p(ws), nbytes,
                                       p(loss), p(GP), B.stream(pkg))
    return case


@pytest.mark.parametrize("K", CLASSES)
def test_fn_cut_loss(pkg, K):
    for terminals in (0, 1):
        for loss_kind in (0, 1):
            for want_gp in (True, False):
                B.run_case(pkg, fn_cut_loss_case(pkg, kind_for("odd", K, terminals), K, terminals, loss_kind, want_gp))
            for kind in ("hub", "tile"):
                B.run_case(pkg, fn_cut_loss_case(pkg, kind, K, terminals, loss_kind, True))


# ---- one model per graph -----------------------------------------------------------------------------------------------
INST = (("gmc_inst_forward", "gmc_inst_train_fwd_bwd", None, None),            # the plain form of the _t
        ("gmc_inst_forward_t", "gmc_inst_train_fwd_bwd_t", True, None),        # the _t of the _c
        ("gmc_inst_forward_c", "gmc_inst_train_fwd_bwd_c", True, True))        # the wide form: carries the matrix


@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("F", WIDTHS)
def test_instance_models(pkg, F, K):
    q = "gmc_inst_workspace_bytes"
    fwd, train = INST[2][:2]
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for cost in (False, True):
            for flags in LOSSES:
                B.run_case(pkg, model_call(pkg, fwd, q, odd, F, K, 0, flags=flags, inst=True, terminals=terminals, cost=cost))
                B.run_case(pkg, model_call(pkg, train, q, odd, F, K, 1, flags=flags, inst=True, terminals=terminals,
                                           cost=cost))
        B.run_case(pkg, model_call(pkg, fwd, q, odd, F, K, 0, inst=True, terminals=terminals, cost=True, optional=False))
    for kind in ("hub", "trip"):
        B.run_case(pkg, model_call(pkg, fwd, q, kind, F, K, 0, flags=2, inst=True, terminals=1, cost=True))
        B.run_case(pkg, model_call(pkg, train, q, kind, F, K, 1, flags=2, inst=True, terminals=1, cost=True))
    for fwd, train, with_t, _ in INST[:2]:                              # the narrower twins: one case each on `odd`
        t = 1 if with_t else None
        B.run_case(pkg, model_call(pkg, fwd, q, kind_for("odd", K), F, K, 0, inst=True, terminals=t))
        B.run_case(pkg, model_call(pkg, train, q, kind_for("odd", K), F, K, 1, inst=True, terminals=t))


@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("F", WIDTHS)
def test_large_instance_models(pkg, F, K):
    q = "gmc_inst_large_workspace_bytes"
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for flags in LOSSES:
            B.run_case(pkg, model_call(pkg, "gmc_inst_large_forward", q, odd, F, K, 0, flags=flags, inst=True,
                                       terminals=terminals))
            B.run_case(pkg, model_call(pkg, "gmc_inst_large_train_fwd_bwd", q, odd, F, K, 1, flags=flags, inst=True,
                                       terminals=terminals))
        B.run_case(pkg, model_call(pkg, "gmc_inst_large_forward", q, odd, F, K, 0, inst=True, terminals=terminals,
                                   optional=False))
    for kind in ("tile", "hub"):
        B.run_case(pkg, model_call(pkg, "gmc_inst_large_forward", q, kind, F, K, 0, flags=2, inst=True, terminals=1))
        B.run_case(pkg, model_call(pkg, "gmc_inst_large_train_fwd_bwd", q, kind, F, K, 1, flags=2, inst=True, terminals=1))


def inst_state_case(pkg, kind, which, F=20, K=5, stopped=False):
    """gmc_inst_keep_best_f32, gmc_inst_early_stop_f32 and gmc_inst_adam_f32 on the per-graph state of a batch."""
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    rng = np.random.RandomState(11)
    S = rng.randint(0, K, h.R).astype(np.int32)
    loss = -rng.uniform(1, 9, h.B).astype(np.float32)
    best_loss = np.where(np.arange(h.B) % 2 == 0, np.float32(np.inf), np.float32(-100.0)).astype(np.float32)
    count = h.R * F + h.B * (F + F * K + K)
    p0, g0 = (rng.uniform(-1, 1, count).astype(np.float32) for _ in range(2))
    m0 = rng.uniform(-1e-3, 1e-3, count).astype(np.float32)
    v0 = rng.uniform(0, 1e-3, count).astype(np.float32)

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h)
        s = B.stream(pkg)
        if which == "adam":
            stop = None
            if stopped is not None:
                stop = mem.put("stop_epoch", np.where(np.arange(h.B) % 2 == 1, 3 if stopped else -1, -1).astype(np.int32))
            return lib.gmc_inst_adam_f32(C.byref(bc), F, K, p(mem.state("param", p0)), p(mem.put("grad", g0)),
                                         p(mem.state("m", m0)), p(mem.state("v", v0)), *HYPER, 3, p(stop), s)
        Sd, ld = mem.put("S", S), mem.put("loss", loss)
        best = [p(mem.state("best_S", np.full(h.R, -3, np.int32))), p(mem.state("best_loss", best_loss)),
                p(mem.state("best_epoch", np.full(h.B, -1, np.int32)))]
        if which == "keep_best":
            return lib.gmc_inst_keep_best_f32(C.byref(bc), p(Sd), p(ld), 7, *best, s)
        prev = mem.state("prev_loss", (loss + np.where(np.arange(h.B) % 3 == 0, 0, 1)).astype(np.float32))
        stall = mem.state("stall", np.full(h.B, 1, np.int32))
        stop = mem.state("stop_epoch", np.where(np.arange(h.B) % 4 == 3, 2, -1).astype(np.int32))
        return lib.gmc_inst_early_stop_f32(C.byref(bc), p(Sd), p(ld), 7, 1e-4, 2, p(prev), p(stall), p(stop), *best, s)
    return case


def test_instance_state(pkg):
    for kind in ("odd", "tile", "trip"):
        for which in ("keep_best", "early_stop"):
            B.run_case(pkg, inst_state_case(pkg, kind, which))
    for F in WIDTHS:
        for K in CLASSES:
            for stopped in (None, False, True):
                B.run_case(pkg, inst_state_case(pkg, "odd", "adam", F, K, stopped))
        B.run_case(pkg, inst_state_case(pkg, "trip", "adam", F, 5, True))   # n * F beyond one 4096-float tile


# ---- the attention first layer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", WIDTHS)
def test_attention(pkg, F):
    q = "gmc_att_workspace_bytes"
    for flags in LOSSES:
        B.run_case(pkg, model_call(pkg, "gmc_att_forward", q, "odd", F, 3, 0, flags=flags, att=True))
    B.run_case(pkg, model_call(pkg, "gmc_att_forward", q, "odd", F, 3, 0, att=True, optional=False))
    for flags in LOSSES + (1, 3):
        B.run_case(pkg, model_call(pkg, "gmc_att_train_fwd_bwd", q, "odd", F, 3, 1, flags=flags, att=True))
    for kind in ("hub", "trip"):
        B.run_case(pkg, model_call(pkg, "gmc_att_forward", q, kind, F, 3, 0, flags=2, att=True))
        B.run_case(pkg, model_call(pkg, "gmc_att_train_fwd_bwd", q, kind, F, 3, 1, flags=2, att=True))


def test_the_check_can_fail(pkg):
    B.check_can_fail(pkg, model_call(pkg, "gmc_train_fwd_bwd", "gmc_workspace_bytes", "odd", 20, 3, 1), "grad")
    B.check_can_fail(pkg, model_call(pkg, "gmc_kway_forward", "gmc_kway_workspace_bytes", "odd", 20, 5, 0), "workspace")

