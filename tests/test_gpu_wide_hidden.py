"""hidden_dim 1025..4096 on the GPU: TrainingConfig(n_nodes=1000, hidden_dim=2048) - and the derived default of
TrainingConfig(n_nodes=4096) - trains on the HIP path like any width up to 1024.  Every sequence (fused, one kernel per
operation, autograd, dropout, the reference's one-step-per-graph schedule, the batched and data-parallel trainer,
dense features) against the C oracle / float64 restatements, and a forward whose element offsets pass 2^31."""

import numpy as np
import pytest
import torch

from oracle import c_oracle as CO
from oracle import ref_dense as R
from tests import stepcheck, util

pytestmark = pytest.mark.gpu

PER_MASK = 3 << 29
WIDE = (1028, 2048, 2050, 4096)
MIX = [(1000, 7, 4001), (300, 8, 4002), (120, 12, 4003)]


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def dataset(case):
    if case == "mix":
        return util.product_dataset(MIX)
    if case == "weighted":
        return util.dataset_of(*util.weighted_copy(MIX, seed=7))
    if case == "hub":   # one degree-40 row: overflow lists (fused LDS kernels; the unfused sequence: row kernels)
        graphs = {0: util.with_hub(1000, 7, 4011, 40), 1: R.regular_graph(300, 7, 4012)}
        return util.dataset_of(graphs, {i: R.seeded_terminals(g.number_of_nodes(), 4013 + i) for i, g in graphs.items()})
    if case == "n270":  # 8 rows per thread at 64-column tiles
        return util.product_dataset([(270, 7, 4021), (200, 6, 4022)])
    assert case == "n530"  # 8 rows per thread at 32-column tiles
    return util.product_dataset([(530, 7, 4031), (500, 8, 4032)])


@pytest.mark.parametrize("case", ["mix", "weighted", "hub", "n270", "n530"])
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("hidden", WIDE)
def test_step_against_oracle(pkg, hidden, fuse, case):
    """One batched step: per-graph loss (or a documented near-tie), gradient <= 1e-4 of its largest entry, P within 1e-4
    of the C oracle and of the float64 restatement; the launches are the LDS flavours F = 1024 takes for this batch."""
    T, cfg, net, embed, opt, params = util.model(hidden)
    ds = dataset(case)
    with util.fused(pkg, fuse):
        # relu kinks (test_gpu_parity.test_relu_kink_is_the_only_gradient_mismatch): a dW1 column / db1 entry may be off
        # the bar only where the float64 pre-activation lies within fp32 noise of 0, at most three columns
        eng, got, _ = stepcheck.check_step_against_oracle(pkg, net, ds, params, kinks=(1e-7, 3))
        batch = util.batch_of(pkg, eng, ds)
        at1024 = pkg.hip.lds_flavours(batch.c, 1024)
        want = {w & ~PER_MASK for w in (at1024[:2] if fuse else at1024[2:])}
        assert {w & ~PER_MASK for w in got.flavours if w} == want, (got.tags, want)
        assert ("fwd1_fused" in got.tags) == bool(fuse and at1024) and ("bwd1_fused" in got.tags) == bool(fuse and at1024)
        P, S, _loss = eng.forward(batch, 1.0, want_loss=True)
    assert eng.F == hidden and eng.Fp % 4 == 0
    P64 = stepcheck.f64_step(util.csrs_of(ds), params, S.cpu().numpy()).P
    assert np.abs(P.cpu().numpy() - P64).max() < 1e-4


def test_adam_parity_on_the_reference_schedule_at_2048(pkg):
    """One Adam step per graph (graphs_per_step = 1), each step on its own: torch.optim.Adam, started from the device's
    parameters and moments and given the C oracle's gradient of that step, against the device's update (every entry
    whose gradient is >= 1 % of the largest: update within 2 %; moments 1e-4 / 2e-4 of their largest).  The one-graph
    backward computes the head (no head launch; the bwd1_reg flavour carries GMC_FLV_HEAD)."""
    T, cfg, net, embed, opt, params = util.model(2048)
    ds = util.product_dataset([(100, 7, 4041), (50, 6, 4042), (300, 8, 4043), (64, 8, 4044), (1000, 7, 4045)])
    eng = net.engine()
    csrs = util.csrs_of(ds)
    ct = CO.CTrainer(params, lr=cfg.learning_rate)
    batches = [pkg.GraphBatch([it[0]], None, eng.device) for it in ds.values()]
    checked = 0
    for t, (batch, csr) in enumerate(zip(batches, csrs), start=1):
        before = eng.flat[:eng.count].cpu().clone()
        m0, v0 = eng.m[:eng.count].cpu().clone(), eng.v[:eng.count].cpu().clone()
        ct.flat[:] = before.numpy()
        ct.m[:] = m0.numpy()
        ct.v[:] = v0.numpy()
        ct.t = t - 1
        eng.sync_step_dev()
        with pkg.hip.Probe(16) as pr:
            _, _, loss = eng.train_step(batch, cfg.learning_rate, cfg.C)
        assert "head" not in [tg for tg, _ms in pr.records], pr.records
        assert any(w >> 26 & 1 for w in pr.flavours if (w & 7) == 3), pr.flavours   # bwd1_reg<..., HEAD>
        ref_loss = ct.step([csr])
        assert eng.step_count == t == ct.t
        if float(loss[0]) != float(ref_loss[0]):
            continue   # a near-tie decoded differently: the next step starts re-synchronised
        p = before.clone().requires_grad_(True)
        topt = torch.optim.Adam([p], lr=cfg.learning_rate)
        topt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        p.grad = torch.from_numpy(ct.grad.copy())
        topt.step()
        g = ct.grad
        big = np.abs(g) >= 1e-2 * np.abs(g).max()
        upd = (eng.flat[:eng.count].cpu() - before).numpy()
        ref_upd = (p.detach() - before).numpy()
        rel = np.abs(upd - ref_upd)[big] / np.abs(ref_upd[big])
        assert big.sum() > 100 and rel.max() < 0.02, (t, rel.max())
        m, v = eng.m[:eng.count].cpu().numpy(), eng.v[:eng.count].cpu().numpy()
        tm, tv = topt.state[p]["exp_avg"].numpy(), topt.state[p]["exp_avg_sq"].numpy()
        assert np.abs(m - tm).max() <= 1e-4 * np.abs(tm).max()
        assert np.abs(v - tv).max() <= 2e-4 * np.abs(tv).max()
        checked += 1
    assert checked >= 3


def test_batched_and_data_parallel_trainer_at_2048(pkg):
    """FusedTrainer with graphs_per_step = 2: the single-GPU fused step (fold + Adam in one sweep, a replayed hipGraph)
    and the sequence a data-parallel rank runs (train_fwd_bwd -> all-reduce -> stand-alone Adam, the loss in the
    gradient's tail slot) end equal; the batched epochs follow the C oracle."""
    class WithoutFusedStep:          # an engine that offers only what the N > 1 branch uses
        def __init__(self, eng):
            self._eng = eng

        def __getattr__(self, name):
            if name == "train_step":
                raise AttributeError(name)
            return getattr(self._eng, name)

    ds = util.product_dataset([(1000, 7, 4051), (640, 6, 4052), (300, 8, 4053), (90, 11, 4054)])
    runs = []
    for variant in ("fused", "dp-sequence"):
        T, cfg, net, embed, opt, params = util.model(2048, seed=5)
        eng = net.engine()
        tr = T.FusedTrainer(net, opt, cfg, graphs_per_step=2,
                            engine=eng if variant == "fused" else WithoutFusedStep(eng))
        losses = [tr.epoch(ds) for _ in range(2)]
        assert (tr._graph is not None) == (variant == "fused")
        runs.append((losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, int(eng.step_count)))
    (la, pa, sa), (lb, pb, sb) = runs
    assert sa == sb == 4 and la == lb
    for k in pa:
        assert pa[k].shape == pb[k].shape and float((pa[k] - pb[k]).abs().max()) < 1e-6, k
    ct = CO.CTrainer(params, lr=cfg.learning_rate)
    csrs = util.csrs_of(ds)
    ref = [sum(float(ct.step(csrs[i:i + 2]).sum()) for i in (0, 2)) for _ in range(2)]
    for got, r in zip(la, ref):
        assert abs(got - r) <= 1e-3 * max(1.0, abs(r)), (la, ref)


def test_autograd_chain_and_dense_features_at_2048(pkg):
    """net(g, A) -> override_fixed_nodes -> apply_max_to_one_hot -> compute_loss -> backward equals the fused gradient;
    net(g, X) with random dense X under no_grad (the wide row SpMM with the fused W2 epilogue) equals ref_dense."""
    T, cfg, net, embed, opt, params = util.model(2048)
    ds = util.product_dataset([(300, 7, 4061)])
    (g, a_pad, nx_g, _t), = ds.values()
    net.train()
    P = net(g, a_pad)
    s = T.apply_max_to_one_hot(T.override_fixed_nodes(P))
    loss = T.compute_loss(s, a_pad, cfg.A, cfg.C, cfg.penalty)
    opt.zero_grad()
    loss.backward()
    auto = {k: dict(net.named_parameters())[k].grad.clone() for k in pkg.engine.PARAM_ORDER}
    eng = net.engine()
    _, _, fl = eng.train_fwd_bwd(pkg.GraphBatch([g], None, eng.device), cfg.C)
    assert abs(float(loss.detach()) - float(fl[0])) < 1e-3
    for k, v in eng.views(eng.grad).items():
        assert v.shape == auto[k].shape
        assert np.abs((v - auto[k]).cpu().numpy()).max() <= 1e-5 * max(1.0, float(auto[k].abs().max())), k

    ds = util.product_dataset([(60, 5, 4062)])
    (g, a_pad, nx_g, _t), = ds.values()
    torch.manual_seed(1)
    X = torch.randn(60, 1000)
    net.eval()
    with torch.no_grad():
        Pd = net(g, X.cuda()).cpu()
    tp = {k: torch.from_numpy(v) for k, v in params.items()}
    assert float((Pd - R.forward(tp, R.graph_from_networkx(nx_g), X)).abs().max()) < 1e-4


def test_dropout_at_2048(pkg):
    """p = 0.3 at hidden 2048: keep rate 1 - p with kept units scaled by 1/(1-p); the autograd gradient equals central
    differences with the mask held fixed; gmc_train_fwd_bwd and gmc_forward + gmc_backward_from_gp agree."""
    from gcn_max_cut_amd.Training import TrainingNeural as T
    p_drop, hidden = 0.3, 2048
    cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=hidden, dropout=p_drop)
    torch.manual_seed(0)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    ds = util.product_dataset([(80, 7, 4071), (60, 6, 4072)])
    (g, a_pad, nx_g, _t) = ds[0]
    eng = net.engine()
    net.train()
    # W1 = 0, b1 = 1 -> relu = 1 everywhere, H_dropped = mask / (1-p); W2[:, 0] = c -> log(P0/P1) = c * mean kept sum
    c = 5.0 / hidden
    with torch.no_grad():
        saved = eng.flat.clone()
        v = eng.views()
        v["conv1.weight"].zero_(); v["conv1.bias"].fill_(1.0); v["conv2.weight"].zero_(); v["conv2.weight"][:, 0] = c
        v["conv2.bias"].zero_()
        torch.manual_seed(11)
        P = net(g, a_pad).cpu().double()
        z = torch.log(P[:, 0] / P[:, 1])
        assert abs(float(z.mean()) / (c * hidden) - 1.0) < 0.01
        assert float(z.std()) > 1e-3
        eng.flat.copy_(saved)

    Wt = torch.from_numpy(np.random.RandomState(3).standard_normal((g.number_of_nodes(), 3)).astype(np.float32)).cuda()

    def loss_at(seed):
        torch.manual_seed(seed)
        return (net(g, a_pad) * Wt).sum()

    net.zero_grad()
    loss_at(21).backward()
    named = dict(net.named_parameters())
    # (steps: at 2048 columns the activations are small and a +-2e-2 step of a layer-1 parameter crosses relu kinks)
    for name, idx, eps in (("conv2.weight", (1500, 1), 2e-2), ("conv2.bias", (2,), 2e-2), ("conv1.bias", (1777,), 5e-3),
                           ("conv1.weight", (3, 2040), 5e-3)):
        prm = named[name]
        gval = float(prm.grad[idx])
        with torch.no_grad():
            old = float(prm[idx])
            prm[idx] = old + eps; lp = float(loss_at(21))
            prm[idx] = old - eps; lm = float(loss_at(21))
            prm[idx] = old
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - gval) <= 0.05 * max(abs(gval), abs(fd)) + 2e-3, (name, fd, gval)

    batch = pkg.GraphBatch([g], None, eng.device)
    torch.manual_seed(33)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    eng.set_dropout(p_drop, seed)
    eng.train_fwd_bwd(batch, 1.0)
    eng.set_dropout(0.0)
    fused = {k: gr.clone() for k, gr in eng.views(eng.grad).items()}
    net.zero_grad()
    torch.manual_seed(33)
    Pt = net(g, a_pad)
    T.compute_loss(T.apply_max_to_one_hot(T.override_fixed_nodes(Pt)), a_pad.cuda(), 0.0, 1.0, 1000.0).backward()
    for k, prm in named.items():
        r = fused[k]
        assert float((prm.grad - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max())), k


def test_forward_offsets_past_2_31(pkg):
    """1100 graphs of n = 1000 (d = 7) at hidden 2048: H is 2.25e9 elements.  P of the first and the last graphs (two
    different graphs, alternating through the batch) against the C oracle."""
    T, cfg, net, embed, opt, params = util.model(2048)
    ds = util.product_dataset([(1000, 7, 4081), (1000, 7, 4082)])
    items = list(ds.values())
    eng = net.engine()
    B = 1100
    batch = pkg.GraphBatch([items[i % 2][0] for i in range(B)], None, eng.device)
    assert batch.R * eng.Fp > 2 ** 31
    P, _S, _l = eng.forward(batch)
    P = P.cpu().numpy()
    eng._ws = None
    torch.cuda.empty_cache()
    W = [params[k] for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")]
    for i, rows in ((0, P[:1000]), (1, P[-1000:])):
        rp, cl, vl = CO.csr_of(items[i][2])
        assert np.abs(rows - CO.forward(rp, cl, vl, *W)["P"]).max() < 1e-4


def test_checkpoint_round_trip_at_2048(pkg, tmp_path, monkeypatch):
    """save_neural_model / load_neural_model keep the reference's logical shapes; the loaded model's next step equals
    the original's."""
    monkeypatch.chdir(tmp_path)
    T, cfg, net, embed, opt, params = util.model(2048)
    ds = util.product_dataset([(300, 7, 4091), (120, 6, 4092)])
    T.train_single_epoch(ds, net, opt, embed, cfg)
    T.save_neural_model(net, opt, embed, 1, [0.0], cfg, "m.pth")
    net2, _inputs, _cfg = T.load_neural_model("m.pth", cfg)
    sd, sd2 = net.state_dict(), net2.state_dict()
    assert tuple(sd2["conv1.weight"].shape) == (1000, 2048) and tuple(sd2["conv1.bias"].shape) == (2048,)
    assert tuple(sd2["conv2.weight"].shape) == (2048, 3) and tuple(sd2["conv2.bias"].shape) == (3,)
    for k, v in sd.items():
        assert torch.equal(v.cpu(), sd2[k].cpu()), k
    items = list(ds.values())
    out = []
    for n_ in (net, net2):
        e = n_.engine()
        _P, _S, loss = e.train_fwd_bwd(util.batch_of(pkg, e, items, weighted=False), cfg.C)
        out.append((loss.cpu().clone(), e.grad[:e.count].cpu().clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_default_hidden_of_a_4096_node_problem_is_accepted(pkg):
    """TrainingConfig(n_nodes=4096) derives hidden_dim = 2048: the engine takes it; 4097 and above stay refused."""
    from gcn_max_cut_amd.Training import TrainingNeural as T
    cfg = T.TrainingConfig(n_nodes=4096)
    assert cfg.hidden_dim == 2048
    eng = pkg.engine.FusedEngine(1000, cfg.hidden_dim, 3)
    assert eng.Fp == 2048
    del eng
    for F in (4096, 4093):
        assert pkg.engine.FusedEngine(10, F, 3).Fp == 4096
    with pytest.raises(ValueError, match="4096"):
        pkg.engine.FusedEngine(10, 4097, 3)
