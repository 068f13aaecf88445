"""GPU tests of the relaxed loss (GMC_LOSS_EXPECTED_CUT, the expected cut under independent rounding) against the
float64 restatement of tests/expected_cut_ref.py: the head kernel and gmc_cut_loss_f32 on every neighbour walk (8- and
16-slot tables with padding slots, overflow blocks with and without padding, CSR rows, the second trip of the row loop,
unequal graphs, real-valued weights), the whole training step through both entries and both kernel sequences, the
trainer's launch paths, evaluate_model and the autograd op cut_loss.

Bars.  Loss: 5e-5 * C * (total edge weight) - five times the rounding of the longest add chain here (a degree-150 row
plus the block tree at 2^-24 per add, about 1e-5 relative).  GP, GY2, db2 and the gradients: stepcheck.ORACLE_BAR and
the row rules the existing step tests pass.  The relaxed loss has no near-tie rule: no case is excused.

Measured on the MI355X (the tests print each figure with -s), worst case per family:
  relaxed loss, head and gmc_cut_loss_f32   6.1e-5 absolute on a loss of -717 (one float32 ulp; bar 7.2e-2, hub150)
  GP / GY2 against float64                  1.2e-5 (hub150; bar 1.1e-2) / below it
  whole step, gradient row ratio            4.7e-5 (hub150, the row kernels; bar 2e-4), P 5.2e-8
  cut_loss through net(g, embed.weight)     dX 1.5e-7 (bar 1e-4), parameters at most 2.7e-5 (bar 4.3e-3)"""
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import expected_cut_ref as ER
from tests import stepcheck, util
from tests.stepcheck import KEYS, ORACLE_BAR, P_TOL, ROW_FLOOR, ROW_TOL

pytestmark = pytest.mark.gpu
HID = 16
LOSS_BAR = 5e-5
HARD, SOFT = 0, 1


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


# ---- batches: name -> (graphs, model rows N, (table width, overflow blocks of the largest graph > 0, weights))
def real_weights(specs, seed):
    graphs, _terms = util.weighted_copy(specs, seed)
    rng = np.random.RandomState(seed)
    for g in graphs.values():
        for u, v in g.edges():
            g[u][v]["weight"] = float(np.float32(g[u][v]["weight"] * rng.uniform(0.3, 1.0)))
    return list(graphs.values())


def graphs_of(name):
    if name == "n3":
        return [util.near_regular(3, 2, 1)]                            # terminals only
    if name == "n4":
        return [util.near_regular(4, 3, 2)]
    if name == "d7":
        return [util.near_regular(60, 7, 3)]                           # 8-slot table, one padding slot per row
    if name == "mixed":
        return [util.near_regular(61, 7, 4)]                           # rows of 6 and 7 neighbours
    if name == "d12":
        return [util.near_regular(50, 12, 5)]                          # 16-slot table, four padding slots per row
    if name == "hub40":
        return [util.with_hub(200, 7, 6, 40)]                          # overflow blocks (four full ones)
    if name == "hub43":
        return [util.with_hub(200, 7, 7, 43)]                          # ... the last of five padded with id n
    if name == "hub150":
        return [util.with_hub(200, 7, 8, 150)]                         # more than 15 blocks: no table, the CSR walk
    if name == "n1030":
        return [util.near_regular(1030, 7, 9)]                         # second trip of the 1024-thread row loop
    if name == "unequal":
        return [util.near_regular(60, 7, 10), util.near_regular(12, 3, 11), util.near_regular(33, 5, 12),
                util.near_regular(3, 2, 13)]
    if name == "weights":
        return real_weights([(60, 7, 14), (41, 6, 15)], 16)
    if name == "weights_hub":
        g = util.with_hub(200, 7, 17, 43)
        rng = np.random.RandomState(17)
        for u, v in g.edges():
            g[u][v]["weight"] = float(np.float32(rng.uniform(0.3, 3.0)))
        return [g]
    raise KeyError(name)


LAYOUT = {"n3": (8, False, False), "n4": (8, False, False), "d7": (8, False, False), "mixed": (8, False, False),
          "d12": (16, False, False), "hub40": (8, True, False), "hub43": (8, True, False), "hub150": (0, False, False),
          "n1030": (8, False, False), "unequal": (8, False, False), "weights": (8, False, True),
          "weights_hub": (8, True, True)}
NAMES = tuple(LAYOUT)
_BATCHES = {}


def batch_of(pkg, name):
    """(GraphBatch, csrs) of a case, built once per session; its layout is the one the case stands for."""
    if name not in _BATCHES:
        handles = [pkg.from_networkx(g) for g in graphs_of(name)]
        batch = pkg.GraphBatch(handles, None)
        h = batch.host
        W, ovf, weights = LAYOUT[name]
        assert (h.ell_width, h.ovf_max_blocks > 0, h.vals is not None) == (W, ovf, weights), name
        if name == "hub43":
            ids = h.ovf_ids.reshape(-1, 8)
            assert ids.shape[0] == 5 and (ids[-1] == 200).sum() == 5    # padding ids in the hub's last block
        if name == "d7":
            assert h.ell_slots == 7 and (h.ell >= 60).sum() == 60       # one padding slot in every row
        _BATCHES[name] = (batch, [(hd.rowptr, hd.col, hd.weight) for hd in handles])
    return _BATCHES[name]


def softmax64(rp, cl, Z0, b2):
    """float64 P of the head for pre-aggregation logits Z0: softmax(dinv o (A @ Z0) + b2)."""
    dinv = 1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(np.float64))
    Z = dinv[:, None] * stepcheck.csr_mm(rp, cl, None, Z0.astype(np.float64)) + b2.astype(np.float64)
    E = np.exp(Z - Z.max(1, keepdims=True))
    return E / E.sum(1, keepdims=True)


def run_head(pkg, batch, Z0, b2, Cc, kind):
    """One poisoned head launch under the probe; kind None: gmc_head_f32.  Returns numpy P, S, loss, db2, GY2."""
    lib, p = pkg.hip.load(), pkg.hip.ptr
    P = torch.full((batch.R, 3), float("nan"), device="cuda")
    S = torch.full((batch.R,), -1, dtype=torch.int32, device="cuda")
    loss = torch.full((batch.B,), float("nan"), device="cuda")
    db2 = torch.full((batch.B, 3), float("nan"), device="cuda")
    GY2 = torch.full((batch.R, 4), float("nan"), device="cuda")
    z, b = torch.from_numpy(Z0).cuda(), torch.from_numpy(b2).cuda()
    with pkg.hip.Probe(4) as probe:
        if kind is None:
            rc = lib.gmc_head_f32(batch.ref(), p(z), 1, p(b), float(Cc), p(P), p(S), p(loss), p(GY2), p(db2),
                                  pkg.hip.stream())
        else:
            rc = lib.gmc_head_loss_f32(batch.ref(), p(z), 1, p(b), float(Cc), kind, p(P), p(S), p(loss), p(GY2), p(db2),
                                       pkg.hip.stream())
        pkg.hip.check(rc, "gmc_head_loss_f32")
    assert [t for t, _ms in probe.records] == ["head"] and probe.flavours == [0]
    return [t.cpu().numpy() for t in (P, S, loss, db2, GY2)]


def run_cut_loss(pkg, batch, P, Cc, kind, want_gp=True):
    lib, p = pkg.hip.load(), pkg.hip.ptr
    Pd = torch.from_numpy(P).cuda()
    loss = torch.full((batch.B,), float("nan"), device="cuda")
    GP = torch.full((batch.R, 3), float("nan"), device="cuda") if want_gp else None
    with pkg.hip.Probe(4) as probe:
        pkg.hip.check(lib.gmc_cut_loss_f32(batch.ref(), p(Pd), float(Cc), kind, p(loss), p(GP), pkg.hip.stream()),
                      "gmc_cut_loss_f32")
    assert [t for t, _ms in probe.records] == ["head"]
    return loss.cpu().numpy(), (GP.cpu().numpy() if want_gp else None)


def within(got, ref, what, bar=ORACLE_BAR):
    ref = np.asarray(ref, np.float64)
    err = float(np.abs(np.asarray(got, np.float64) - ref).max()) if ref.size else 0.0
    lim = bar * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"{what}: err {err:.2e} bar {lim:.2e}")
    assert np.isfinite(np.asarray(got)).all() and err <= lim, (what, err, lim)


# ---- head and gmc_cut_loss_f32
@pytest.mark.parametrize("name", NAMES)
def test_head_and_cut_loss_on_every_walk(pkg, name):
    batch, csrs = batch_of(pkg, name)
    Cc = 1.7
    rng = np.random.RandomState(len(name) + batch.R)
    Z0 = rng.standard_normal((batch.R, 3)).astype(np.float32)
    b2 = (0.1 * rng.standard_normal(3)).astype(np.float32)
    old = run_head(pkg, batch, Z0, b2, Cc, None)
    hard = run_head(pkg, batch, Z0, b2, Cc, HARD)
    soft = run_head(pkg, batch, Z0, b2, Cc, SOFT)
    again = run_head(pkg, batch, Z0, b2, Cc, SOFT)
    for a, b in zip(old, hard):                                     # GMC_LOSS_CUT is today's head, bit for bit
        assert a.tobytes() == b.tobytes(), name
    assert old[0].tobytes() == soft[0].tobytes() and old[1].tobytes() == soft[1].tobytes(), name   # P and S
    for a, b in zip(soft, again):                                   # two runs give identical bytes
        assert a.tobytes() == b.tobytes(), name
    P, S = old[0], old[1]
    loss_h, gp_h = run_cut_loss(pkg, batch, P, Cc, HARD)
    loss_s, gp_s = run_cut_loss(pkg, batch, P, Cc, SOFT)
    loss_s2, gp_s2 = run_cut_loss(pkg, batch, P, Cc, SOFT)
    assert loss_s.tobytes() == loss_s2.tobytes() and gp_s.tobytes() == gp_s2.tobytes(), name
    assert loss_h.tobytes() == old[2].tobytes(), name               # the hard kind is the head's loss, bit for bit
    only_loss, none = run_cut_loss(pkg, batch, P, Cc, SOFT, want_gp=False)
    assert none is None and only_loss.tobytes() == loss_s.tobytes(), name

    off = 0
    for g, (rp, cl, vl) in enumerate(csrs):
        n = len(rp) - 1
        sl = slice(off, off + n)
        P64 = softmax64(rp, cl, Z0[sl], b2)
        assert np.abs(P[sl] - P64).max() <= P_TOL, name
        S64 = stepcheck.f64_partition(P64)
        assert stepcheck.near_tie_rows(P64, S[sl], 1e-6, name) == 0     # (random logits: no row near a tie)
        assert np.array_equal(S[sl], S64), name
        bar = LOSS_BAR * Cc * ER.total_weight([(rp, cl, vl)])
        # the relaxed loss and its gradient
        loss64, gp64 = ER.loss_and_gp(rp, cl, vl, P64, Cc)
        db64, gy64 = ER.head_from_p(rp, cl, P64, gp64)
        for what, got in (("head", soft[2][g]), ("cut_loss", loss_s[g])):
            print(f"{name} graph {g} {what}: relaxed loss {got:.6f} float64 {loss64:.6f} err {abs(got - loss64):.2e} bar {bar:.2e}")
            assert abs(float(got) - loss64) <= bar, (name, g, what, got, loss64)
        within(gp_s[sl], gp64, f"{name} graph {g} GP")
        within(soft[4][sl, :3], gy64, f"{name} graph {g} GY2")
        within(soft[3][g], db64, f"{name} graph {g} db2")
        dinv = 1.0 / np.sqrt(np.maximum(np.diff(rp), 1))
        assert np.allclose(soft[4][sl, 3], dinv, rtol=1e-6), name
        # the hard loss of the same partition
        hard64, hgp64 = ER.hard_loss_and_gp(rp, cl, vl, S64, Cc)
        assert abs(float(loss_h[g]) - hard64) <= bar, (name, g, loss_h[g], hard64)
        within(gp_h[sl], hgp64, f"{name} graph {g} hard GP")
        if vl is None:                                                  # unit weights: exact integers (times C)
            counts = np.round(hgp64 / Cc)
            assert np.abs(hgp64 / Cc - counts).max() < 1e-9, name
            assert np.array_equal(gp_h[sl], np.float32(Cc) * counts.astype(np.float32)), name
        hdb64, hgy64 = ER.head_from_p(rp, cl, P64, hgp64)
        within(hard[4][sl, :3], hgy64, f"{name} graph {g} hard GY2")
        off += n


def test_relaxed_loss_of_one_hot_rows_is_the_hard_loss(pkg):
    """P rows that are exactly one-hot: the relaxed loss and GP are the hard ones, exactly (unit weights)."""
    batch, csrs = batch_of(pkg, "hub43")
    rng = np.random.RandomState(3)
    S = rng.randint(0, 3, batch.R)
    S[:3] = [0, 1, 2]
    P = np.eye(3, dtype=np.float32)[S]
    P[:3] = np.float32(1.0 / 3)                                         # the override replaces them
    loss_s, gp_s = run_cut_loss(pkg, batch, P, 1.0, SOFT)
    loss_h, gp_h = run_cut_loss(pkg, batch, P, 1.0, HARD)
    ref, gp = ER.hard_loss_and_gp(*csrs[0], S, 1.0)
    assert float(loss_s[0]) == float(loss_h[0]) == ref
    assert np.array_equal(gp_s, gp_h) and np.array_equal(gp_s, gp.astype(np.float32))


# ---- the whole step
def model_for(name, seed=0):
    N = 1040 if name == "n1030" else 1000
    T, cfg, net, embed, opt, params = util.model(HID, n_nodes=N, seed=seed)
    return T, cfg, net, opt, params


def run_step(pkg, eng, batch, Cc, fuse, entry, loss):
    """stepcheck.run_step with the loss keyword: one poisoned step under the probe."""
    with util.fused(pkg, fuse):
        util.poison(eng, batch)
        with pkg.hip.Probe(64) as probe:
            if entry == "train_step":
                eng.m.zero_(); eng.v.zero_()
                eng.sync_step_dev()
                P, S, losses = eng.train_step(batch, 1e-3, Cc, loss=loss)
                grads = {k: v.cpu().numpy() / (1.0 - stepcheck.BETA1) for k, v in eng.views(eng.m).items()}
            else:
                P, S, losses = eng.train_fwd_bwd(batch, Cc, loss=loss)
                grads = {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()}
    tail = None if entry == "train_step" else float(eng.grad[eng.count])
    return stepcheck.Step(P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(), grads, tail,
                          [t for t, _ms in probe.records], list(probe.flavours))


def grad_rules(csrs, params):
    return dict(grad_bar=ORACLE_BAR, row_tol=ROW_TOL, row_floor=ROW_FLOOR, kinks=(1e-7, 3), csrs=csrs, params=params,
                sparse=True)


def check_relaxed_step(got, ref, csrs, params, Cc, what):
    p_err = float(np.abs(got.P - ref.P).max())
    assert p_err <= P_TOL, (what, p_err)
    off = 0
    for g, (rp, _cl, _vl) in enumerate(csrs):
        n = len(rp) - 1
        assert stepcheck.near_tie_rows(ref.P[off:off + n], got.S[off:off + n], 1e-6, what) >= 0
        bar = LOSS_BAR * Cc * ER.total_weight([csrs[g]])
        print(f"{what} graph {g}: loss {got.loss[g]:.6f} float64 {ref.loss[g]:.6f} bar {bar:.2e}")
        assert abs(float(got.loss[g]) - ref.loss[g]) <= bar, (what, g, got.loss[g], ref.loss[g])
        off += n
    if got.tail is not None:
        assert got.tail == float(got.loss.sum()), (what, got.tail)
    res = stepcheck.compare_grads(got.grads, ref.grads, what=what, **grad_rules(csrs, params))
    assert res["kink_cols"] is None or res["kink_cols"] <= 3, (what, res)
    print(f"{what}: P {p_err:.2e} rows {res['rows']:.2e}")


# name -> the kernel sequence of (the fused setting, gmc_set_fuse(0)): overflow lists are served by the fused kernels
# only, graphs past the LDS windows and batches without a table by the row kernels
STEP_CASES = {"d7": ("fused", "per_op"), "d12": ("fused", "per_op"), "hub43": ("fused", "rows"), "hub150": ("rows", "rows"),
              "unequal": ("fused", "per_op"), "weights": ("fused", "per_op"), "n1030": ("rows", "rows")}


@pytest.mark.parametrize("fuse", (1, 0), ids=("fused", "per_op"))
@pytest.mark.parametrize("entry", ("train_fwd_bwd", "train_step"))
@pytest.mark.parametrize("name", STEP_CASES)
def test_whole_step_against_float64(pkg, name, entry, fuse):
    batch, csrs = batch_of(pkg, name)
    _T, _cfg, net, _opt, params = model_for(name)
    eng = net.engine()
    Cc = 1.3
    got = run_step(pkg, eng, batch, Cc, fuse, entry, "expected_cut")
    W, ovf, weights = LAYOUT[name]
    path = STEP_CASES[name][0 if fuse else 1]
    query = pkg.hip.lds_flavours(batch.c, eng.Fp)                       # the fused sequence's words, then the per-op one's
    assert len(query) == {("fused", "per_op"): 6, ("fused", "rows"): 2, ("rows", "rows"): 0}[STEP_CASES[name]], query
    ran = [w for w in got.flavours if w]
    if path == "fused":
        assert got.tags[:3] == ["fwd1_fused", "head", "bwd1_fused"], got.tags
        assert ran == query[:2], (ran, query)
        words = [pkg.hip.flavour_fields(w) for w in ran]
        assert [w["kernel"] for w in words] == ["fwd1_lds", "bwd1_reg" if W == 8 else "bwd1_lds"], words
        assert all(w["OVF"] == int(ovf) and w["HAS_VAL"] == int(weights) and not w["HEAD"] for w in words), words
    else:
        assert got.tags[:3] == ["gather_w1", "agg_fwd", "head"], got.tags
        assert ran == (query[2:] if path == "per_op" else []), (ran, query)
    ref = ER.f64_step(csrs, params, Cc)
    check_relaxed_step(got, ref, csrs, params, Cc, f"{name} {entry} fuse={fuse}")
    assert not got.grads["conv1.weight"][batch.n_max:].any()            # rows past every graph's n: exactly 0
    # gmc_forward with the flag reports the same P, S and loss
    with util.fused(pkg, fuse):
        Pf, Sf, lf = (t.cpu().numpy() for t in eng.forward(batch, Cc, want_loss=True, loss="expected_cut"))
    if entry == "train_fwd_bwd":
        assert np.array_equal(Pf, got.P) and np.array_equal(Sf, got.S) and np.array_equal(lf, got.loss), name


def test_one_graph_relaxed_step_launches_the_head_on_its_own(pkg):
    """n = 200, d = 7: the hard one-graph train_step computes the head inside the backward launch (no head record,
    GMC_FLV_HEAD set); the relaxed one runs the stand-alone head (a GMC_K_HEAD record, GMC_FLV_HEAD clear)."""
    h = pkg.from_networkx(util.near_regular(200, 7, 21))
    batch, csrs = pkg.GraphBatch([h], None), [(h.rowptr, h.col, h.weight)]
    _T, _cfg, net, _opt, params = model_for("one")
    eng = net.engine()
    hard = run_step(pkg, eng, batch, 1.0, 1, "train_step", "cut")
    params = util.np_params(net.state_dict())                           # (the hard step moved them)
    soft = run_step(pkg, eng, batch, 1.0, 1, "train_step", "expected_cut")
    assert "head" not in hard.tags and pkg.hip.flavour_fields(hard.flavours[hard.tags.index("bwd1_fused")])["HEAD"] == 1
    assert soft.tags == ["fwd1_fused", "head", "bwd1_fused", "finish"], soft.tags
    word = pkg.hip.flavour_fields(soft.flavours[soft.tags.index("bwd1_fused")])
    assert word["kernel"] == "bwd1_reg" and word["HEAD"] == 0, word
    check_relaxed_step(soft, ER.f64_step(csrs, params, 1.0), csrs, params, 1.0, "one graph")


@pytest.mark.parametrize("name", ("d7", "hub43", "weights", "hub150"))
def test_loss_cut_through_the_new_entry_points_is_the_old_step_bit_for_bit(pkg, name):
    """gmc_train_step_loss_f32(GMC_LOSS_CUT) against gmc_train_step_f32 from the same state: P, S, loss, gradient and
    the updated parameters; train_fwd_bwd / forward with loss="cut" against the calls without the keyword."""
    batch, _csrs = batch_of(pkg, name)
    lib, p = pkg.hip.load(), pkg.hip.ptr
    outs = []
    for new in (False, True):
        _T, _cfg, net, _opt, _params = model_for(name, seed=4)
        eng = net.engine()
        util.poison(eng, batch)
        if new:
            P, S, loss = eng.train_step(batch, 1e-3, 1.3, loss="cut")
        else:
            ws, nbytes = eng._workspace(batch, True)
            P = torch.empty((batch.R, 3), device="cuda")
            S = torch.empty(batch.R, dtype=torch.int32, device="cuda")
            loss = torch.empty(batch.B, device="cuda")
            rc = lib.gmc_train_step_f32(batch.ref(), eng.N, eng.Fp, p(eng.flat), 1.3, p(ws), nbytes, p(P), p(S), p(loss),
                                        p(eng.grad), p(eng.m), p(eng.v), 1e-3, 0.9, 0.999, 1e-8, p(eng.step_dev), None,
                                        pkg.hip.stream())
            pkg.hip.check(rc, "gmc_train_step_f32")
        outs.append([t.cpu().numpy().tobytes() for t in (P, S, loss, eng.grad[:eng.count], eng.flat[:eng.count])])
        a = [t.cpu().numpy().tobytes() for t in eng.train_fwd_bwd(batch, 1.3)] + [eng.grad.cpu().numpy().tobytes()]
        b = [t.cpu().numpy().tobytes() for t in eng.train_fwd_bwd(batch, 1.3, loss="cut")] + [eng.grad.cpu().numpy().tobytes()]
        assert a == b, name
        a = [t.cpu().numpy().tobytes() for t in eng.forward(batch, 1.3, want_loss=True)]
        assert a == [t.cpu().numpy().tobytes() for t in eng.forward(batch, 1.3, want_loss=True, loss="cut")], name
    assert outs[0] == outs[1], name
    with pytest.raises(ValueError):
        eng.train_step(batch, 1e-3, loss="soft")
    with pytest.raises(ValueError):
        eng.forward(batch, loss="soft")


# ---- trainer
TRAIN_SPECS = [(60, 7, 31), (48, 6, 32), (34, 5, 33), (70, 7, 34)]


def train_epochs(pkg, path, epochs=3, dropout=0.0):
    """Epoch losses of FusedTrainer(loss="expected_cut") on four small graphs, two per step, on one launch path; also
    the first step's per-graph losses (at the initial parameters) and those parameters."""
    ds = util.product_dataset(TRAIN_SPECS)
    T, cfg, net, _embed, opt, params = util.model(HID, seed=6)
    net.dropout_frac = dropout
    net.train()
    tr = T.FusedTrainer(net, opt, cfg, graphs_per_step=2, loss="expected_cut")
    if path != "graph":
        tr.allow_graph = False
    if path == "copy":
        tr._poll = False
    losses, first = [], None
    for e in range(epochs):
        losses.append(tr.epoch(ds))
        if e == 0:
            torch.cuda.synchronize()
            direct = path == "direct" and tr._loss_host_dev is not None    # (the losses went straight to the pinned slots)
            first = tr._loss_host_np[0, :2].copy() if direct else tr._loss_slots[0, :2].cpu().numpy().copy()
    torch.cuda.synchronize()
    want = {"graph": tr._graph is not None, "direct": tr._graph is None,
            "copy": tr._graph is None and tr._loss_host_dev is None, "dropout": tr._graph is None}[path]
    assert want, path
    return losses, first, params, ds, net.engine().flat.cpu().numpy().copy()


def test_trainer_paths_agree_bit_for_bit_and_start_at_the_float64_loss(pkg):
    runs = {path: train_epochs(pkg, path) for path in ("graph", "direct", "copy")}
    losses, first, params, ds, flat = runs["graph"]
    for path in ("direct", "copy"):
        assert runs[path][0] == losses, (path, runs[path][0], losses)
        assert np.array_equal(runs[path][4], flat), path
    assert all(np.isfinite(losses)) and losses[2] < losses[0]            # (it descends: three epochs of Adam)
    csrs = util.csrs_of(ds)[:2]
    ref = ER.f64_step(csrs, params, 1.0)
    for path in runs:
        got = runs[path][1]
        for g in range(2):
            bar = LOSS_BAR * ER.total_weight([csrs[g]])
            print(f"trainer {path} first loss graph {g}: {got[g]:.6f} float64 {ref.loss[g]:.6f} bar {bar:.2e}")
            assert abs(float(got[g]) - ref.loss[g]) <= bar, (path, g)


def test_trainer_data_parallel_sequences_train_on_the_relaxed_loss(pkg):
    """The data-parallel sequence (train_fwd_bwd, all-reduce - a no-op without a process group -, device-stepped Adam),
    eager (DP) and with hipGraphs on either side of the all-reduce (DP_GRAPHS): the same three epochs as the fused
    step's, compared at the loss bar (the stand-alone Adam sweep need not be the fused one bit for bit)."""
    ref_losses, _first, _params, ds, ref_flat = train_epochs(pkg, "graph")
    bar = LOSS_BAR * ER.total_weight(util.csrs_of(ds))
    runs = {}
    for path in ("dp", "dp_graphs"):
        T, cfg, net, _embed, opt, _p = util.model(HID, seed=6)
        net.train()
        eng = net.engine()

        class WithoutFusedStep:          # an engine that offers only what the data-parallel sequence uses
            def __getattr__(self, name):
                if name == "train_step":
                    raise AttributeError(name)
                return getattr(eng, name)

            def __setattr__(self, name, value):   # (the trainer keeps the engine's step counts: they are the engine's)
                setattr(eng, name, value)

        tr = T.FusedTrainer(net, opt, cfg, graphs_per_step=2, engine=WithoutFusedStep(), loss="expected_cut")
        tr.dp = True
        tr._dp_graphs_env = path == "dp_graphs"
        runs[path] = ([tr.epoch(ds) for _ in range(3)], eng.flat.cpu().numpy().copy())
        assert (tr._dp_graph is not None) == (path == "dp_graphs") and tr._graph is None, path
        assert eng.step_count == 6 and int(eng.step_dev.item()) == 6, path
        for got, want in zip(runs[path][0], ref_losses):
            print(f"trainer {path}: epoch loss {got:.6f} fused step {want:.6f} bar {bar:.2e}")
            assert abs(got - want) <= bar, (path, got, want)
        assert np.abs(runs[path][1] - ref_flat).max() < 1e-6, path


def test_trainer_with_dropout_and_the_float64_step_under_the_restated_mask(pkg):
    losses, _first, _params, _ds, _flat = train_epochs(pkg, "dropout", dropout=0.3)
    assert all(np.isfinite(losses)), losses
    p, seed = 0.3, 0x5151_2323
    for name in ("d7", "hub43"):                                        # the LDS one-kernel-per-operation and the row sequence
        batch, csrs = batch_of(pkg, name)
        _T, _cfg, net, _opt, params = model_for(name, seed=8)
        eng = net.engine()
        goffs = [int(x) for x in batch.host.goff[:-1]]
        keeps = [util.dropout_keep(seed, g0 + np.arange(len(rp) - 1), np.arange(HID), p) for (rp, _c, _v), g0 in zip(csrs, goffs)]
        eng.set_dropout(p, seed)
        try:
            got = run_step(pkg, eng, batch, 1.0, None, "train_fwd_bwd", "expected_cut")
        finally:
            eng.set_dropout(0.0)
        ref = ER.f64_step(csrs, params, 1.0, keeps=keeps, p=p)
        check_relaxed_step(got, ref, csrs, params, 1.0, f"dropout {name}")


def test_evaluate_model_reports_the_relaxed_loss(pkg):
    ds = util.product_dataset(TRAIN_SPECS)
    T, cfg, net, _embed, _opt, params = util.model(HID, seed=6)
    cfg.C = 1.7
    out = T.evaluate_model(net, ds, cfg, loss="expected_cut")
    csrs = util.csrs_of(ds)
    ref = ER.f64_step(csrs, params, 1.7)
    bar = LOSS_BAR * 1.7 * ER.total_weight(csrs)
    print(f"evaluate_model relaxed: {out['total_loss']:.6f} float64 {ref.loss.sum():.6f} bar {bar:.2e}")
    assert abs(out["total_loss"] - float(ref.loss.sum())) <= bar and out["num_samples"] == 4
    assert abs(out["average_loss"] - float(ref.loss.sum()) / 4) <= bar
    hard = T.evaluate_model(net, ds, cfg)
    assert hard["total_loss"] == T.evaluate_model(net, ds, cfg, loss="cut")["total_loss"]
    assert hard["total_loss"] != out["total_loss"]


# ---- cut_loss as an autograd op
def test_cut_loss_backpropagates_to_the_embedding(pkg):
    """loss = cut_loss(g, net(g, embed.weight), C, relaxed=True); loss.backward(): the loss, embed.weight.grad (dX)
    and the parameter gradients against float64 autograd through oracle/ref_dense.py's forward and the definition."""
    from tests.test_gpu_dense_features import case, close, net_of
    c = case("n60_h32")
    assert c["closest"] > c["margin"], c["closest"]
    T, net = net_of(c)
    net.train()
    (g, _a_pad, nx_g, _t), = c["items"]
    n, Cc = g.number_of_nodes(), 1.7
    embed = torch.nn.Embedding(n, c["N"]).cuda()
    with torch.no_grad():
        embed.weight.copy_(torch.from_numpy(c["X"]))
    P = net(g, embed.weight)
    loss = T.cut_loss(g, P, Cc, relaxed=True)
    assert loss.dim() == 0 and loss.requires_grad
    (2.0 * loss).backward()                                             # grad_out = 2 reaches GP
    # float64
    leaf = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in c["params"].items()}
    Xl = torch.from_numpy(c["X"]).double().requires_grad_(True)
    P64 = R.forward(leaf, R.graph_from_networkx(nx_g), Xl)
    A = torch.zeros((n, n), dtype=torch.float64)
    for u, v, w in nx_g.edges(data="weight", default=1):
        A[u, v] = A[v, u] = float(w)
    Pt = torch.cat([torch.eye(3, dtype=torch.float64) + P64[:3] - P64[:3].detach(), P64[3:]])
    ref = -Cc * 0.5 * (A * (1.0 - Pt @ Pt.T)).sum()
    (2.0 * ref).backward()
    bar = LOSS_BAR * Cc * float(A.sum()) / 2
    print(f"cut_loss relaxed {float(loss.detach()):.6f} float64 {float(ref.detach()):.6f} bar {bar:.2e}")
    assert abs(float(loss.detach()) - float(ref.detach())) <= bar
    close(embed.weight.grad.cpu().numpy(), Xl.grad.numpy(), "cut_loss dX")
    named = dict(net.named_parameters())
    for k in KEYS:
        close(named[k].grad.cpu().numpy(), leaf[k].grad.numpy(), f"cut_loss {k}")
    # gmc_forward_features honours the flag: the same loss from the forward itself
    eng = net.engine()
    batch = T._dense_batch_of(g, eng.device)
    _P, _S, lf = eng.forward_features(batch, embed.weight, Cc, want_loss=True, loss="expected_cut")
    assert abs(float(lf[0]) - float(ref.detach())) <= bar
    assert float(eng.forward_features(batch, embed.weight, Cc, want_loss=True)[2][0]) == \
        float(T.cut_loss(g, P.detach(), Cc).detach())                   # (and without it the hard one)
    # the hard kind is the reference's chain: -C * cut of the argmax decode, straight-through gradient
    with torch.no_grad():
        Pd = net(g, embed.weight)
    Pl = Pd.clone().requires_grad_(True)
    hard = T.cut_loss(g, Pl, Cc)
    hard.backward()
    S = Pd.cpu().numpy().argmax(1)
    S[:3] = [0, 1, 2]
    ref_h, gp_h = ER.hard_loss_and_gp(g.rowptr, g.col, g.weight, S, Cc)
    assert abs(float(hard.detach()) - ref_h) <= bar
    close(Pl.grad.cpu().numpy(), gp_h, "cut_loss hard dP")
    with pytest.raises(ValueError):
        T.cut_loss(g, Pd[:10])
