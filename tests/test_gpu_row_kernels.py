"""GPU matrix of the row-kernel sequence (tests/test_row_kernels.py: ROW_MATRIX and the census that pins it) against
a float64 restatement of the training step on CSR segment sums (tests/stepcheck.py, f64_*_sparse).

Each case builds its batch (the n graph, then B - 1 graphs of 12 nodes), checks that it has the table / overflow
lists of its route and that the query gives it no LDS word, poisons workspace and gradient, and runs one
gmc_train_fwd_bwd under the probe: the tags are exactly the row sequence, every flavour word is 0.  P, the partition
(near-tie rule of stepcheck.f64_step), the loss (-C cut of the kernels' own partition), the gradient per parameter row
(never looser than the oracle bar) and the zero dW1 rows past n_max are compared with float64; gmc_forward's P, S and
loss are bitwise those of the training step.  Further: gmc_spmm_f32 per launch class, gmc_backward_from_gp with a dense
random dL/dP, three Adam steps of the largest advertised problem (N = 4096, hidden 2048, one 4096-node graph), and
dropout against the numpy restatement of the library's mask on both layouts.

Measured on the MI355X, worst case per family (P absolute / gradient row ratio; test_report prints them with -s):
  training step, ROW_MATRIX   P 5.4e-8 (n2328)   rows 2.2e-5 (b249, 32 dW1 chunks)
  backward_from_gp, dense GP                    rows 7.6e-5 (n2328, hidden 260)
  largest problem, 3 Adam steps P 6.1e-8        rows 9.5e-6
  dropout p = 0.3             P 4.7e-8           rows 2.2e-6 (slab), 7.8e-7 (rows)
  gmc_spmm_f32                                  rows 1.7e-6 (wide)
The bars below (the flavour matrix's) are at most 10x those.
"""
import networkx as nx
import numpy as np
import pytest
import torch

from tests import stepcheck, util
from tests.stepcheck import KEYS, ORACLE_BAR, P_TOL, ROW_FLOOR, ROW_TOL, SHORT
from tests.test_row_kernels import (DROPOUT_CASES, GP_CASES, ROW_MATRIX, USER_SPMM, dw1_chunks, launch_np, row_tags)

pytestmark = pytest.mark.gpu

MEASURED = {}


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


# ---- graphs
def big_graph(kind, n, seed):
    if kind == "gnp":
        g = nx.gnp_random_graph(n, 30.0 / n, seed=seed)
        assert min(d for _v, d in g.degree()) > 0
        return g
    g = util.near_regular(n, {"reg7": 7, "ovf8": 7, "hub": 7, "reg12": 12, "ovf16": 12}[kind], seed, attrs=False)
    if kind in ("ovf8", "ovf16", "hub"):
        util.add_hub(g, {"ovf8": 12, "ovf16": 20, "hub": 150}[kind], seed, attrs=False)
    return g


def build(pkg, kind, n, F, weights, B, N=None, seed=None):
    """(net, params, batch, csrs): the n graph and B - 1 graphs of 12 nodes, integer weights 1..3 when asked."""
    from gcn_max_cut_amd import graph as G
    from gcn_max_cut_amd.Training import TrainingNeural as T
    seed = 7 * n + F + B if seed is None else seed
    graphs = [big_graph(kind, n, seed)] + [util.near_regular(12, 3, seed + i, attrs=False) for i in range(1, B)]
    rng = np.random.RandomState(seed)
    for g in graphs:
        for u, v in g.edges():
            g[u][v]["weight"] = int(rng.randint(1, 4)) if weights else 1
    handles = [G.from_networkx(g) for g in graphs]
    N = N or min(4096, n + 40)
    torch.manual_seed(seed)
    net, _embed, _opt = T.setup_model_and_optimizer(T.TrainingConfig(n_nodes=N, hidden_dim=F))
    params = util.np_params(net.state_dict())
    batch = pkg.GraphBatch(handles, None, net.engine().device)
    csrs = [(h.rowptr, h.col, h.weight) for h in handles]
    return net, params, batch, csrs


# ---- comparisons
def check_grad(grads, g64, csrs, params, what, kinks_ok=True):
    """Every parameter row within ROW_TOL of the float64 gradient (keyed W1 / b1 / W2 / b2) and within the oracle bar.
    A layer-1 column whose float64 pre-activation lies within fp32 noise of 0 (a relu kink) may differ
    (test_gpu_wide_hidden's rule: at most three such columns).  Returns the worst row ratio."""
    res = stepcheck.compare_grads(grads, stepcheck.named(g64), what=what, **rules(csrs, params, kinks_ok))
    assert res["kink_cols"] is None or res["kink_cols"] <= 3, (what, res)
    return res["rows"]


def rules(csrs, params, kinks_ok=True):
    return dict(grad_bar=ORACLE_BAR, row_tol=ROW_TOL, row_floor=ROW_FLOOR, kinks=(1e-7, 3) if kinks_ok else None,
                csrs=csrs, params=params, sparse=True)


def record(family, p_err, ratio):
    a, b = MEASURED.get(family, (0.0, 0.0))
    MEASURED[family] = (max(a, p_err), max(b, ratio))
    print(f"row case {family}: P {p_err:.2e} rows {ratio:.2e}")


# ---- the matrix
@pytest.mark.parametrize("case", ROW_MATRIX, ids=[c[0] for c in ROW_MATRIX])
def test_row_matrix(pkg, case):
    cid, _route, kind, n, F, weights, B, fuse, (W, slots, blocks) = case
    net, params, batch, csrs = build(pkg, kind, n, F, weights, B)
    eng = net.engine()
    h = batch.host
    assert (h.n_max, h.ell_width, h.ovf_max_blocks, h.vals is not None) == (n, W, blocks, weights), cid
    if W:
        assert h.ell_slots == slots, cid
    words = pkg.hip.lds_flavours(batch.c, eng.Fp)
    assert words == [] if fuse else len(words) == 2, cid
    with util.fused(pkg, fuse):
        got = stepcheck.run_step(pkg, eng, batch)
        Pf, Sf, lossf = (t.cpu().numpy() for t in eng.forward(batch, want_loss=True))
    assert got.tags == row_tags(B), (cid, got.tags)
    assert not any(got.flavours), got.flavours
    assert np.array_equal(got.P, Pf) and np.array_equal(got.S, Sf) and np.array_equal(got.loss, lossf), cid
    ref = stepcheck.f64_step(csrs, params, got.S, sparse=True)
    assert not got.grads["conv1.weight"][n:].any(), cid          # rows past every graph's n: exactly 0
    res = stepcheck.compare_step(got, ref, p_tol=P_TOL, what=cid, **rules(csrs, params))
    assert res["kink_cols"] is None or res["kink_cols"] <= 3, (cid, res)
    p_err, ratio = res["p_err"], res["rows"]
    record(f"matrix F{launch_np(F)} B{'1' if B == 1 else 'fold' if dw1_chunks(B) > 1 else 'chunk1'}", p_err, ratio)
    record("matrix " + cid, p_err, ratio)


# ---- gmc_spmm_f32 per launch class (VARIANT 0 with weights and the W2 epilogue; spmm_rows_scalar)
@pytest.mark.parametrize("F,weights,epi", USER_SPMM, ids=[f"F{F}-{'val' if w else 'unit'}-{'epi' if e else 'plain'}"
                                                          for F, w, e in USER_SPMM])
def test_user_spmm(pkg, F, weights, epi):
    lib = pkg.hip.load()
    rng = np.random.RandomState(F + 2 * weights + epi)
    g = util.near_regular(300, 9, F, attrs=False)
    util.add_hub(g, 80, F, attrs=False)                           # one row of more than 64 neighbours
    from gcn_max_cut_amd import graph as G
    hd = G.from_networkx(g)
    rp, cl = hd.rowptr, hd.col
    n_src, n = 320, 300
    vl = rng.randint(1, 4, cl.size).astype(np.float32) if weights else None
    ldx = F + (4 if F % 4 == 0 else 0)
    X = rng.standard_normal((n_src, ldx)).astype(np.float32)
    scale = rng.uniform(0.1, 1.0, n).astype(np.float32)
    bias = rng.standard_normal(F).astype(np.float32) * 0.1
    W2 = rng.standard_normal((F, 3)).astype(np.float32)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = {k: dev(v) for k, v in dict(rp=rp, cl=cl, vl=vl, X=X, scale=scale, bias=bias, W2=W2).items()}
    Y = torch.full((n, ldx), float("nan"), device="cuda")
    Z0 = torch.full((n, 3), float("nan"), device="cuda") if epi else None
    p = pkg.hip.ptr
    rc = lib.gmc_spmm_f32(p(t["rp"]), p(t["cl"]), p(t["vl"]), p(t["scale"]), p(t["X"]), ldx, p(t["bias"]), 1, p(Y), ldx,
                          n, F, 0, p(t["W2"]) if epi else None, p(Z0), pkg.hip.stream())
    pkg.hip.check(rc, "gmc_spmm_f32")
    Y64 = np.maximum(scale[:, None].astype(np.float64) *
                     stepcheck.csr_mm(rp, cl, None if vl is None else vl.astype(np.float64), X[:, :F].astype(np.float64))
                     + bias, 0.0)
    Yg = Y.cpu().numpy()[:, :F].astype(np.float64)
    ratio = stepcheck.row_error_ratio(Yg, Y64, ROW_FLOOR)
    assert ratio <= ROW_TOL, ratio
    if epi:
        Z64 = scale[:, None] * (Y64 @ W2.astype(np.float64))
        zr = stepcheck.row_error_ratio(Z0.cpu().numpy(), Z64, ROW_FLOOR)
        assert zr <= ROW_TOL, zr
        ratio = max(ratio, zr)
    record(f"spmm_f32 F{launch_np(F) if F % 4 == 0 else 'scalar'}", 0.0, ratio)


# ---- gmc_backward_from_gp with a dense random dL/dP
@pytest.mark.parametrize("cid", GP_CASES)
def test_backward_from_gp_with_a_dense_gp(pkg, cid):
    _cid, _route, kind, n, F, weights, B, _fuse, _tab = next(c for c in ROW_MATRIX if c[0] == cid)
    net, params, batch, csrs = build(pkg, kind, n, F, weights, B)
    eng = net.engine()
    ws = torch.empty(eng.workspace_bytes(batch, True), dtype=torch.uint8, device=eng.device)
    ws.fill_(255)
    eng.grad.fill_(float("nan"))
    P, _S, _l = eng.forward(batch, ws=ws)
    rng = np.random.RandomState(n + F)
    GP = (rng.uniform(0.5, 2.0, (batch.R, 3)) * rng.choice([-1, 1], (batch.R, 3))).astype(np.float32)
    with pkg.hip.Probe(64) as probe:
        got = eng.backward_from_gp(batch, P, torch.from_numpy(GP).cuda(), ws=ws)
    assert [t for t, _ms in probe.records] == ["head"] + row_tags(B)[3:], probe.records
    grads = {k: v.cpu().numpy() for k, v in got.items()}
    W = [params[k] for k in KEYS]
    g64, off = None, 0
    Pn = P.cpu().numpy().astype(np.float64)
    for rp, cl, vl in csrs:
        m = len(rp) - 1
        f = stepcheck.f64_forward_sparse(rp, cl, vl, *W)
        assert np.abs(f["P"] - Pn[off:off + m]).max() <= P_TOL
        f["P"] = Pn[off:off + m]                              # the backward differentiates at the kernels' P
        g = stepcheck.f64_backward_sparse(f, GP[off:off + m].astype(np.float64), W[2], W[0].shape[0])
        g64 = g if g64 is None else {k: g64[k] + g[k] for k in g64}
        off += m
    ratio = check_grad(grads, g64, csrs, params, cid)
    record(f"backward_from_gp F{launch_np(F)}", 0.0, ratio)


# ---- the largest advertised problem: three Adam steps, each against float64 from the device's state
def test_largest_problem_three_adam_steps(pkg):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    cfg = T.TrainingConfig(n_nodes=4096)
    assert cfg.hidden_dim == 2048
    net, params, batch, csrs = build(pkg, "reg7", 4096, cfg.hidden_dim, False, 1, N=4096, seed=4096)
    eng = net.engine()
    lr, b1, b2, eps = cfg.learning_rate, 0.9, 0.999, 1e-8
    for t in (1, 2, 3):
        before = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.flat).items()}
        m0 = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.m).items()}
        v0 = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.v).items()}
        eng.sync_step_dev()
        with pkg.hip.Probe(64) as probe:
            P, S, loss = eng.train_step(batch, lr, betas=(b1, b2), eps=eps)
        assert [tg for tg, _ms in probe.records] == row_tags(1) + ["adam"], probe.records
        state = {k: v.astype(np.float32) for k, v in before.items()}
        ref = stepcheck.f64_step(csrs, state, S.cpu().numpy(), sparse=True)
        g64 = {k: ref.grads[key] for k, key in SHORT.items()}
        p_err = float(np.abs(P.cpu().numpy() - ref.P).max())
        assert p_err <= P_TOL, (t, p_err)
        assert np.array_equal(loss.cpu().numpy(), ref.loss), t
        grads = {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()}
        ratio = check_grad(grads, g64, csrs, state, f"adam step {t}")
        record("largest problem (grad)", p_err, ratio)
        after = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.flat).items()}
        m1 = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.m).items()}
        v1 = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.v).items()}
        for k, key in SHORT.items():
            g = g64[k].reshape(m0[key].shape)
            m64 = m0[key] + (g - m0[key]) * (1 - b1)
            v64 = b2 * v0[key] + (1 - b2) * g * g
            upd64 = -lr / (1 - b1 ** t) * m64 / (np.sqrt(v64) / np.sqrt(1 - b2 ** t) + eps)
            assert np.abs(m1[key] - m64).max() <= 1e-4 * np.abs(m64).max(), (t, key)
            assert np.abs(v1[key] - v64).max() <= 2e-4 * np.abs(v64).max(), (t, key)
            big = np.abs(m64) >= 1e-2 * np.abs(m64).max()      # (where g changed sign, m may be ~0: judged by m)
            rel = np.abs((after[key] - before[key]) - upd64)[big] / np.abs(upd64[big])
            assert big.any() and rel.max() < 0.02, (t, key, rel.max())


# ---- dropout against float64 with the restated mask
def f64_dropout_step(csrs, params, S_got, goffs, seed, p, C_=1.0):
    W1, b1, W2, b2 = (np.asarray(params[k], np.float64) for k in KEYS)
    Fh = W1.shape[1]
    Ps, losses, Hs, grad = [], [], [], None
    for (rp, cl, vl), g0 in zip(csrs, goffs):
        n = len(rp) - 1
        keep = util.dropout_keep(seed, g0 + np.arange(n), np.arange(Fh), p)
        f = stepcheck.f64_forward_sparse(rp, cl, vl, W1, b1, W2, b2)
        dinv = f["dinv"]
        Hd = f["H"] * keep / (1.0 - p)
        Z = dinv[:, None] * stepcheck.csr_mm(rp, cl, None, dinv[:, None] * Hd @ W2) + b2
        E = np.exp(Z - Z.max(1, keepdims=True))
        P = E / E.sum(1, keepdims=True)
        S = stepcheck.f64_partition(P)
        s_got = np.asarray(S_got[g0:g0 + n])
        diff = np.nonzero(s_got != S)[0]
        if diff.size:
            srt = np.sort(P[diff], axis=1)
            assert (srt[:, 2] - srt[:, 1]).max() < 1e-6, (diff, srt)
            S = s_got.astype(np.int64)
        f.update(P=P, H=Hd)
        loss, GP = stepcheck.f64_loss_and_gp_sparse(f, S, C_)
        gz = P * (GP - (GP * P).sum(1, keepdims=True))
        gy2 = stepcheck.csr_mm(rp, cl, None, dinv[:, None] * gz)
        dW2 = (dinv[:, None] * Hd).T @ gy2
        gg = np.where(Hd > 0, dinv[:, None] * (gy2 @ W2.T) / (1.0 - p), 0.0)
        gy1 = stepcheck.csr_mm(rp, cl, None, dinv[:, None] * gg)
        dW1 = np.zeros_like(W1)
        dW1[:n] = stepcheck.csr_mm(rp, cl, f["w"], dinv[:, None] * gy1)
        g = dict(W1=dW1, b1=gg.sum(0), W2=dW2, b2=gz.sum(0))
        grad = g if grad is None else {k: grad[k] + g[k] for k in grad}
        Ps.append(P); losses.append(loss); Hs.append((keep, f["pre"], Hd))
    return np.concatenate(Ps), np.asarray(losses), grad, Hs


def stored_h(ws, batch, F, fs):
    """H as the workspace holds it after gmc_forward (the backward reuses it for U): [R, F] from the row-major [R, ld]
    or the slab [slice][R][fs] layout (carve in api.hip: T0 first, then H, each 256-byte aligned)."""
    R = batch.R
    ld = (F + 31) // 32 * 32
    cols = (F + fs - 1) // fs * fs if fs else ld
    off = (R * cols * 4 + 255) // 256 * 256
    flat = ws[off:off + R * cols * 4].view(torch.float32).cpu().numpy()
    if not fs:
        return flat.reshape(R, ld)[:, :F]
    return flat.reshape(cols // fs, R, fs).transpose(1, 0, 2).reshape(R, cols)[:, :F]


def test_dropout_against_float64_with_the_restated_mask(pkg):
    p, seed = 0.3, 0x1234_5678_9ABC
    masks = {}
    for layout, kind, n, F, B in DROPOUT_CASES:
        net, params, batch, csrs = build(pkg, kind, n, F, False, B, seed=n + F)
        eng = net.engine()
        words = pkg.hip.lds_flavours(batch.c, eng.Fp)
        fs = 0 if layout == "rows" else words[-1] >> 3 & 0x7f
        assert (batch.host.ovf_max_blocks > 0) == (layout == "rows") and (fs > 0) == (layout == "slab")
        goffs = [int(x) for x in batch.host.goff[:-1]]
        eng.set_dropout(p, seed)
        try:
            # route 1: the training entry
            util.poison(eng, batch)
            with pkg.hip.Probe(64) as probe:
                P, S, loss = eng.train_fwd_bwd(batch)
            grads = {k: v.cpu().numpy().copy() for k, v in eng.views(eng.grad).items()}
            # route 2: gmc_forward, then gmc_backward_from_gp with the structured dL/dP of the kernels' partition
            ws = torch.empty(eng.workspace_bytes(batch, True), dtype=torch.uint8, device=eng.device)
            ws.fill_(255)
            P2, S2, loss2 = eng.forward(batch, want_loss=True, ws=ws)
            H = stored_h(ws, batch, F, fs)
            Sn = S2.cpu().numpy()
            GP = np.zeros((batch.R, 3), np.float32)
            for (rp, cl, vl), g0 in zip(csrs, goffs):
                m = len(rp) - 1
                rows = np.repeat(np.arange(m), np.diff(rp))
                np.add.at(GP, (g0 + rows, Sn[g0 + cl]), 1.0 if vl is None else vl)
            got2 = eng.backward_from_gp(batch, P2, torch.from_numpy(GP).cuda(), ws=ws)
            grads2 = {k: v.cpu().numpy() for k, v in got2.items()}
        finally:
            eng.set_dropout(0.0)
        if layout == "rows":
            assert [t for t, _ms in probe.records] == row_tags(B) and not any(probe.flavours), probe.records
        else:
            assert all(probe.flavours[i] for i, (t, _ms) in enumerate(probe.records)
                       if t in ("gather_w1", "agg_fwd", "agg_bwd", "dw1")), probe.records
        assert torch.equal(P, P2) and torch.equal(S, S2) and torch.equal(loss, loss2), layout
        P64, loss64, g64, Hs = f64_dropout_step(csrs, params, S.cpu().numpy(), goffs, seed, p)
        p_err = float(np.abs(P.cpu().numpy() - P64).max())
        assert p_err <= P_TOL, (layout, p_err)
        assert np.array_equal(loss.cpu().numpy(), loss64.astype(np.float32)), layout
        # the dropped positions are the numpy mask's (away from the relu kink), the kept ones carry 1 / (1 - p)
        for (keep, pre, Hd), g0 in zip(Hs, goffs):
            h = H[g0:g0 + len(pre)].astype(np.float64)
            live = np.abs(pre) > 1e-5
            assert np.array_equal((h != 0)[live], (keep & (pre > 0))[live]), layout
            assert np.abs(h - Hd).max() <= 1e-5 * max(1.0, np.abs(Hd).max()), layout
        masks[layout] = [k for k, _pre, _h in Hs]
        r1 = check_grad(grads, g64, csrs, params, layout + " train_fwd_bwd", kinks_ok=False)
        r2 = check_grad(grads2, g64, csrs, params, layout + " backward_from_gp", kinks_ok=False)
        record(f"dropout {layout}", p_err, max(r1, r2))
    assert all(np.array_equal(a, b) for a, b in zip(masks["rows"], masks["slab"]))


def test_report():
    """(prints the worst errors per family of this session's run; -s shows them)"""
    for fam, (p_err, ratio) in sorted(MEASURED.items()):
        print(f"MEASURED {fam}: P {p_err:.2e} rows {ratio:.2e}")
