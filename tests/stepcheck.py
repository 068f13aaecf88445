"""Is one training step right?  The GPU tests answer through this module: `run_step` runs one poisoned step on the
device, `f64_step` / `oracle_step` build the reference under the near-tie rule, `compare_step` judges - in plain numpy,
so that tests/test_stepcheck.py can hand it wrong answers without a GPU.  Each test passes its own bars as arguments;
the ones several files share are defined here once."""
import collections

import numpy as np

from oracle import c_oracle as CO
from tests import util

KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")
SHORT = dict(zip(("W1", "b1", "W2", "b2"), KEYS))

PROB_TOL = 1e-4         # absolute, probabilities against the float32 C oracle (north star)
ORACLE_BAR = 1e-4       # gradients: x max(1, max|reference tensor|)
P_TOL = 5e-7            # absolute, probabilities against float64
ROW_TOL = 2e-4          # per parameter row, relative to the row's own magnitude (never looser than ORACLE_BAR)
ROW_FLOOR = 1e-3        # ... or this fraction of the tensor's largest entry, for rows that are (near) zero
BETA1 = 0.9

Step = collections.namedtuple("Step", "P S loss grads tail tags flavours")
Ref = collections.namedtuple("Ref", "P loss grads near_ties")


def run_step(pkg, eng, batch, C=1.0, fuse=None, entry="train_fwd_bwd"):
    """One step of `entry` under the probe, workspace and gradient poisoned first: nothing may be read before it is
    written in the same step.  entry "train_step": gmc_train_step_f32 from zeroed Adam moments, so that m = (1 - beta1) g
    gives the gradient back; the loss tail is the gradient buffer's, so there is none."""
    with util.fused(pkg, fuse):
        util.poison(eng, batch)
        with pkg.hip.Probe(64) as probe:
            if entry == "train_step":
                eng.m.zero_(); eng.v.zero_()
                P, S, loss = eng.train_step(batch, 1e-3, C)
                grads = {k: v.cpu().numpy() / (1.0 - BETA1) for k, v in eng.views(eng.m).items()}
            else:
                assert entry == "train_fwd_bwd", entry
                P, S, loss = eng.train_fwd_bwd(batch, C)
                grads = {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()}
    tail = None if entry == "train_step" else float(eng.grad[eng.count])   # GMC_MODEL_GRAD_TAIL: the loss rides behind
    return Step(P.cpu().numpy(), S.cpu().numpy(), loss.cpu().numpy(), grads, tail, [t for t, _ms in probe.records],
                list(probe.flavours))


# ---- float64 restatement of one training step (forward, loss, backward) on a graph's CSR.
# Written from the algorithm the oracle documents (oracle/gcn_oracle.c: GraphConv norm='both' twice, softmax, terminal
# override + argmax, cut loss, straight-through dLoss/dP = C * A_val @ onehot(S)), on dense n x n operators.
def f64_forward(rp, cl, vl, W1, b1, W2, b2):
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    A = np.zeros((n, n))
    A[rows, cl] = 1.0                                   # structure: the aggregations carry no edge weight
    X = np.zeros((n, n))
    X[rows, cl] = 1.0 if vl is None else vl.astype(np.float64)   # features = the weighted adjacency
    dinv = 1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(np.float64))
    W1, b1, W2, b2 = (np.asarray(w, np.float64) for w in (W1, b1, W2, b2))
    T0 = dinv[:, None] * (X @ W1[:n])
    pre = dinv[:, None] * (A @ T0) + b1
    H = np.maximum(pre, 0.0)
    Z = dinv[:, None] * (A @ (dinv[:, None] * H @ W2)) + b2
    E = np.exp(Z - Z.max(1, keepdims=True))
    return dict(A=A, X=X, dinv=dinv, pre=pre, H=H, P=E / E.sum(1, keepdims=True))


def f64_partition(P):
    S = P.argmax(1)
    S[:3] = [0, 1, 2]
    return S


def f64_loss_and_gp(f, S, C=1.0):
    """loss = -C * cut(S), GP = C * A_val @ onehot(S)."""
    X = f["X"]
    cut = 0.5 * float((X * (S[:, None] != S[None, :])).sum())
    return -C * cut, C * X @ np.eye(3)[S]


def f64_backward(f, GP, W2, N):
    A, X, dinv, H, P = f["A"], f["X"], f["dinv"], f["H"], f["P"]
    W2 = np.asarray(W2, np.float64)
    gz = P * (GP - (GP * P).sum(1, keepdims=True))     # softmax backward
    gy2 = A @ (dinv[:, None] * gz)
    dW2 = (dinv[:, None] * H).T @ gy2
    g = np.where(H > 0, dinv[:, None] * (gy2 @ W2.T), 0.0)
    gy1 = A @ (dinv[:, None] * g)
    dW1 = np.zeros((N, H.shape[1]))
    dW1[:len(dinv)] = X @ (dinv[:, None] * gy1)
    return dict(W1=dW1, b1=g.sum(0), W2=dW2, b2=gz.sum(0))


# ---- the same float64 step on CSR segment sums: no n x n operator, for graphs of thousands of nodes and wide layers
def csr_mm(rp, cl, w, M, block=512):
    """CSR matrix (edge weights w; None = unit) times the dense float64 M, as per-row segment sums of M's rows."""
    n = len(rp) - 1
    out = np.zeros((n, M.shape[1]))
    live = np.nonzero(np.diff(rp))[0]
    if live.size == 0:
        return out
    starts = np.asarray(rp[:-1])[live]
    for c0 in range(0, M.shape[1], block):
        G = M[cl, c0:c0 + block]
        if w is not None:
            G = G * w[:, None]
        out[live, c0:c0 + block] = np.add.reduceat(G, starts, axis=0)
    return out


def f64_forward_sparse(rp, cl, vl, W1, b1, W2, b2):
    """f64_forward on the CSR: the aggregations carry no edge weight, the features (the weighted adjacency) do."""
    n = len(rp) - 1
    vw = None if vl is None else np.asarray(vl, np.float64)
    dinv = 1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(np.float64))
    W1, b1, W2, b2 = (np.asarray(w, np.float64) for w in (W1, b1, W2, b2))
    T0 = dinv[:, None] * csr_mm(rp, cl, vw, W1[:n])
    pre = dinv[:, None] * csr_mm(rp, cl, None, T0) + b1
    H = np.maximum(pre, 0.0)
    Z = dinv[:, None] * csr_mm(rp, cl, None, dinv[:, None] * H @ W2) + b2
    E = np.exp(Z - Z.max(1, keepdims=True))
    return dict(rp=rp, cl=cl, w=vw, dinv=dinv, pre=pre, H=H, P=E / E.sum(1, keepdims=True))


def f64_loss_and_gp_sparse(f, S, C=1.0):
    rp, cl, w = f["rp"], f["cl"], f["w"]
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    cut_w = (S[rows] != S[cl]).astype(np.float64)
    cut = 0.5 * float((cut_w if w is None else cut_w * w).sum())
    return -C * cut, C * csr_mm(rp, cl, w, np.eye(3)[S])


def f64_backward_sparse(f, GP, W2, N):
    rp, cl, w, dinv, H, P = f["rp"], f["cl"], f["w"], f["dinv"], f["H"], f["P"]
    W2 = np.asarray(W2, np.float64)
    gz = P * (GP - (GP * P).sum(1, keepdims=True))
    gy2 = csr_mm(rp, cl, None, dinv[:, None] * gz)
    dW2 = (dinv[:, None] * H).T @ gy2
    g = np.where(H > 0, dinv[:, None] * (gy2 @ W2.T), 0.0)
    gy1 = csr_mm(rp, cl, None, dinv[:, None] * g)
    dW1 = np.zeros((N, H.shape[1]))
    dW1[:len(dinv)] = csr_mm(rp, cl, w, dinv[:, None] * gy1)
    return dict(W1=dW1, b1=g.sum(0), W2=dW2, b2=gz.sum(0))


def named(short):
    """A gradient keyed W1 / b1 / W2 / b2 (the f64_backward forms) under the parameters' names."""
    return {SHORT[k]: v for k, v in short.items()}


# ---- the two references.  The near-tie rule, for both: the summation order of the kernels is not the reference's, so a
# row whose top-2 margin in the reference is below `tie` may decode either way - anywhere else the partitions must agree
# (AssertionError).  The reference loss and gradient are then those of the partition the kernels chose (`S_got`).
def near_tie_rows(P_ref, s_got, tie, where):
    diff = np.nonzero(s_got != f64_partition(P_ref))[0]
    if diff.size:
        srt = np.sort(P_ref[diff].astype(np.float64), axis=1)
        assert (srt[:, 2] - srt[:, 1]).max() < tie, (where, diff, srt)
    return diff.size


def f64_step(csrs, params, S_got, C=1.0, tie=1e-6, sparse=False):
    """Float64 reference of the batch: P, per-graph loss (rounded to float32 once), summed gradient.  `sparse`: the CSR
    restatement (same values, tests/test_row_kernels.py) instead of the dense one."""
    fwd, lgp, bwd = ((f64_forward_sparse, f64_loss_and_gp_sparse, f64_backward_sparse) if sparse else
                     (f64_forward, f64_loss_and_gp, f64_backward))
    W = [params[k] for k in KEYS]
    grad = None
    Ps, losses, off, near = [], [], 0, 0
    for i, (rp, cl, vl) in enumerate(csrs):
        n = len(rp) - 1
        f = fwd(rp, cl, vl, *W)
        S = np.asarray(S_got[off:off + n]).astype(np.int64)
        near += near_tie_rows(f["P"], S, tie, i)
        loss, GP = lgp(f, S, C)
        g = bwd(f, GP, W[2], W[0].shape[0])
        grad = g if grad is None else {k: grad[k] + g[k] for k in grad}
        Ps.append(f["P"])
        losses.append(loss)
        off += n
    return Ref(np.concatenate(Ps), np.asarray(losses).astype(np.float32), named(grad), near)


def flat_ref_grads(ct):
    """The CTrainer's flat gradient [W1 | b1 | W2 | b2] by parameter name."""
    return dict(zip(KEYS, np.split(ct.grad, np.cumsum([ct.N * ct.F, ct.F, ct.F * ct.K]))))


def oracle_step(csrs, params, S_got, C=1.0, tie=1e-6):
    """C-oracle reference of the batch (float32): P of orc_forward, losses and gradient of orc_train_step - or, where a
    row near-ties, the oracle's backward for the partition the kernels chose: same forward, GP from the kernels' S."""
    W = [params[k] for k in KEYS]
    N, F = W[0].shape
    ct = CO.CTrainer(params, Cc=C)
    loss = ct.step(csrs)
    Ps, differs, off = [], [], 0
    for i, (rp, cl, vl) in enumerate(csrs):
        n = len(rp) - 1
        Ps.append(CO.forward(rp, cl, vl, *W)["P"])
        differs.append(near_tie_rows(Ps[-1], np.asarray(S_got[off:off + n]), tie, i))
        off += n
    if not any(differs):
        grads = {k: g.reshape(np.shape(params[k])) for k, g in flat_ref_grads(ct).items()}
        return Ref(np.concatenate(Ps), loss, grads, 0)
    acc = [np.zeros_like(w) for w in W]
    off = 0
    for i, (rp, cl, vl) in enumerate(csrs):
        n = len(rp) - 1
        s_i = np.asarray(S_got[off:off + n])
        f = CO.forward(rp, cl, vl, *W)
        wv = np.ones(len(cl), np.float32) if vl is None else vl
        rows = np.repeat(np.arange(n), np.diff(rp))
        GP = np.zeros((n, 3), np.float32)
        np.add.at(GP, (rows, s_i[cl]), C * wv)                  # GP = C * A_val @ onehot(S)
        if differs[i]:
            loss[i] = np.float32(-C * 0.5 * float(wv[s_i[rows] != s_i[cl]].sum()))   # -C cut of the kernels' partition
        for a_, d_ in zip(acc, CO.backward(rp, cl, vl, N, W[2], f["H"], f["P"], GP)):
            a_ += d_
        off += n
    return Ref(np.concatenate(Ps), loss, dict(zip(KEYS, acc)), sum(differs))


# ---- judging
def row_scale(ref, floor):
    ref = np.abs(np.asarray(ref, np.float64).reshape(np.shape(ref)[0], -1))
    return np.maximum(ref.max(1), floor * max(ref.max(), 1e-30))


def row_error_ratio(got, ref, floor):
    """max over rows of |got - ref| / max(max |ref row|, floor * max |ref|): each parameter row (dW1 row j, a b1 entry,
    a dW2 row, a b2 entry) judged against its own magnitude; `floor` keeps rows that are exactly zero in the reference
    (rows past every graph's n) at a bar relative to the tensor."""
    got = np.asarray(got, np.float64).reshape(ref.shape[0], -1)
    ref = np.asarray(ref, np.float64).reshape(ref.shape[0], -1)
    return float((np.abs(got - ref).max(1) / row_scale(ref, floor)).max())


def kink_columns(csrs, params, noise=1e-7, sparse=False):
    """Columns f of layer 1 with a float64 pre-activation within fp32 accumulation noise of 0 (relu kinks: the kernels
    and the reference may take different sides, and then that column of dW1 and entry of db1 differ by design)."""
    W = [params[k].astype(np.float64) for k in KEYS]
    kink = np.zeros(W[1].shape[0], bool)
    for rp, cl, vl in csrs:
        pre = (f64_forward_sparse if sparse else f64_forward)(rp, cl, vl, *W)["pre"]
        kink |= (np.abs(pre) < noise).any(0)
    return kink


def compare_grads(got, ref, *, grad_bar, row_tol=None, row_floor=None, kinks=None, csrs=None, params=None, sparse=False,
                  what=None):
    """Every tensor finite and within grad_bar * max(1, max|ref|); with `row_tol`, every parameter row within row_tol of
    its own magnitude (row_error_ratio with `row_floor`) as well.  kinks = (noise, max_cols): where dW1 / db1 miss that,
    the columns that miss it must be kink columns (kink_columns of `csrs`, `params`; `sparse`: which restatement), at
    most max_cols of them, and the tensor without the kink columns must meet it.
    Returns rows (worst row ratio), bad_cols, kink_cols (how many columns qualify; None where the rule was not needed)."""
    worst, bad, kink = 0.0, set(), None
    for key in KEYS:
        r = np.asarray(ref[key], np.float64)
        g = np.asarray(got[key], np.float64).reshape(r.shape)
        assert np.isfinite(g).all(), (what, key)
        bar = grad_bar * max(1.0, float(np.abs(r).max()))
        err = np.abs(g - r)
        misses = err > bar
        if row_tol is not None:
            misses |= (err.reshape(r.shape[0], -1) > row_tol * row_scale(r, row_floor)[:, None]).reshape(r.shape)
        if kinks is not None and key in KEYS[:2] and misses.any():
            noise, max_cols = kinks
            if kink is None:
                kink = kink_columns(csrs, params, noise, sparse)
            cols = set(np.nonzero(misses.reshape(-1, r.shape[-1]).any(0))[0])
            assert cols <= set(np.nonzero(kink)[0]), (what, key, sorted(cols), np.nonzero(kink)[0])
            bad |= cols
            assert len(bad) <= max_cols, (what, key, sorted(bad))
            g, r = g[..., ~kink], r[..., ~kink]
        assert np.abs(g - r).max() <= bar, (what, key, float(np.abs(g - r).max()), bar)
        if row_tol is not None:
            ratio = row_error_ratio(g, r, row_floor)
            assert ratio <= row_tol, (what, key, ratio)
            worst = max(worst, ratio)
    return dict(rows=worst, bad_cols=sorted(bad), kink_cols=None if kink is None else int(kink.sum()))


def compare_step(got, ref, *, p_tol, grad_bar, what=None, **grad_rules):
    """A Step against a Ref: P within p_tol absolute, the float32 losses equal, the gradient's tail slot == loss.sum(),
    the gradient by compare_grads (its keyword rules).  Returns what callers assert further on or print: p_err, rows,
    near_ties, bad_cols, kink_cols."""
    p_err = float(np.abs(got.P - ref.P).max())
    assert p_err < p_tol, (what, p_err)
    assert got.loss.dtype == ref.loss.dtype == np.float32 and np.array_equal(got.loss, ref.loss), (what, got.loss, ref.loss)
    if got.tail is not None:
        assert got.tail == float(got.loss.sum()), (what, got.tail)
    return dict(compare_grads(got.grads, ref.grads, grad_bar=grad_bar, what=what, **grad_rules), p_err=p_err,
                near_ties=ref.near_ties)


def check_step_against_oracle(pkg, net, ds, params, C=1.0, fuse=None, weighted=True, **rules):
    """One batched step of the dataset through the C ABI against the C oracle at the oracle tests' bars: P within
    PROB_TOL, per-graph loss (== -cut of the partition the kernels chose), every gradient entry within ORACLE_BAR of
    the largest.  Returns (engine, Step, compare_step's result)."""
    eng = net.engine()
    got = run_step(pkg, eng, util.batch_of(pkg, eng, ds, weighted), C, fuse)
    csrs = util.csrs_of(ds)
    ref = oracle_step(csrs, params, got.S, C)
    return eng, got, compare_step(got, ref, p_tol=PROB_TOL, grad_bar=ORACLE_BAR, csrs=csrs, params=params, **rules)
