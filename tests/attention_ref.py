"""Float64 restatement of one training step of the model with a graph-attention first layer (include/gcnmaxcut.h,
gmc_att_*), in numpy, and the cases the GPU tests run.

Per graph, on local nodes; the terms of row i are its CSR entries plus one self term (a self-loop edge is one more
ordinary term):

    T = X @ W1[:n]                      s_src = T @ a_src,  s_dst = T @ a_dst
    z_ij = s_dst[i] + s_src[j]          e_ij = leaky_relu(z_ij, slope)
    alpha_ij = softmax over the terms of row i,   H = relu(sum_j alpha_ij T[j] + b1)
    Z = dinv o (A @ (dinv o H @ W2)) + b2,  P = softmax(Z)          (layer 2 and everything after it: tests/stepcheck.py)

and the hand-derived backward of the header.  The losses and their dLoss/dP are tests/kway_ref.py's at K = 3; the CSR
product is stepcheck.csr_mm.  tests/test_attention_host.py checks the gradients against torch.autograd through an
independent dense form of the same model.

The cases (`CASES`) live here so that the CPU test can assert, on this float64 reference, what lets the GPU test demand
identical partitions and judge every gradient entry: no top-2 margin below `MARGIN`, no layer-1 pre-activation within
`KINK` of the relu kink, no |z_ij| below `ZGAP` (the leaky-relu gradient jumps at 0).  A node without neighbours has
T = 0, so its one z_ii is exactly 0 in every arithmetic and for every seed; its alpha_ii is 1 and its de_ii = alpha (da -
alpha da) is exactly 0 on either side of the jump, so `zgap` is taken over the rows with more than one term.

One more precondition, `CONDITION`.  The gradient is judged per parameter row against the row's own magnitude
(stepcheck.ROW_TOL).  Some of these graphs make whole tensors or rows cancel: in a triangle every row has the same three
terms, and where all scores of a row have one sign its ds_dst is exactly 0, so da_dst is pure rounding noise in ANY float32
evaluation (the float64 value is 1e-18); a star's leaves are copies of one another.  `float32_yardstick` evaluates the same
formulas with torch in float32 on the CPU (an independent dense form, torch's own summation orders) against float64.  A
case whose yardstick already spends more than half of ROW_TOL leaves no room to judge a second float32 evaluation with
other summation orders at that bar, whatever computes it: such a seed is skipped like one with a near tie.  The figure comes
from torch on the CPU alone, never from the kernels.  The same bound holds for `leak`, the move of the float64 gradient under
ONE float32 rounding of the softmax backward (`float32_softmax_backward_error`): the row of a star's hub saturates, its
dLoss/dP is of the order of its degree, and half an ulp of that, handed to 140 identical leaves, is larger than whole
tensors of such a graph.  (With three nodes and the hard loss nearly every seed fails one of the two: hence a seed of 298.)"""
import collections

import networkx as nx
import numpy as np

from tests import kway_ref as KR
from tests import stepcheck, util
from tests.stepcheck import KEYS

SLOPE = 0.2
ATT_KEYS = KEYS + ("conv1.attn_src", "conv1.attn_dst")
MARGIN = 1e-5
KINK = 1e-6
ZGAP = 1e-6
# the float32 yardstick's worst parameter-row ratio a case may have: half of stepcheck.ROW_TOL (see below)
CONDITION = stepcheck.ROW_TOL / 2


def terms_of(rp, cl):
    """(row, column) of every term: the CSR entries in CSR order, then the self terms."""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    return np.concatenate([rows, np.arange(n)]), np.concatenate([np.asarray(cl, np.int64), np.arange(n)])


def scatter_rows(index, M, n):
    out = np.zeros((n,) + M.shape[1:])
    np.add.at(out, index, M)
    return out


def f64_forward(rp, cl, vl, params, slope=SLOPE):
    W1, b1, W2, b2, a_src, a_dst = (np.asarray(params[k], np.float64) for k in ATT_KEYS)
    rp, cl = np.asarray(rp), np.asarray(cl)
    n = len(rp) - 1
    vw = None if vl is None else np.asarray(vl, np.float64)
    dinv = 1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(np.float64))
    T = stepcheck.csr_mm(rp, cl, vw, W1[:n])
    s_src, s_dst = T @ a_src, T @ a_dst
    ti, tj = terms_of(rp, cl)
    z = s_dst[ti] + s_src[tj]
    e = np.where(z > 0, z, slope * z)
    m = np.full(n, -np.inf)
    np.maximum.at(m, ti, e)
    ex = np.exp(e - m[ti])
    alpha = ex / np.bincount(ti, ex, n)[ti]
    pre = scatter_rows(ti, alpha[:, None] * T[tj], n) + b1
    H = np.maximum(pre, 0.0)
    Z = dinv[:, None] * stepcheck.csr_mm(rp, cl, None, dinv[:, None] * H @ W2) + b2
    E = np.exp(Z - Z.max(1, keepdims=True))
    return dict(rp=rp, cl=cl, w=vw, dinv=dinv, T=T, ti=ti, tj=tj, z=z, alpha=alpha, pre=pre, H=H,
                P=E / E.sum(1, keepdims=True))


def f64_backward(f, GP, params, slope=SLOPE, gz_error=None):
    """The gradient by parameter name for a given dLoss/dP.  `gz_error`: added to the softmax backward's result (how an
    error there reaches the parameters: `float32_softmax_backward_error`)."""
    W1, _b1, W2, _b2, a_src, a_dst = (np.asarray(params[k], np.float64) for k in ATT_KEYS)
    rp, cl, w, dinv, T, ti, tj, z, alpha, H, P = (f[k] for k in ("rp", "cl", "w", "dinv", "T", "ti", "tj", "z", "alpha",
                                                                    "H", "P"))
    n = len(dinv)
    gz = P * (GP - (GP * P).sum(1, keepdims=True))
    if gz_error is not None:
        gz = gz + gz_error
    gy2 = stepcheck.csr_mm(rp, cl, None, dinv[:, None] * gz)
    dW2 = (dinv[:, None] * H).T @ gy2
    G = np.where(H > 0, dinv[:, None] * (gy2 @ W2.T), 0.0)
    da = (G[ti] * T[tj]).sum(1)
    de = alpha * (da - np.bincount(ti, alpha * da, n)[ti])
    dz = de * np.where(z > 0, 1.0, slope)
    ds_dst, ds_src = np.bincount(ti, dz, n), np.bincount(tj, dz, n)
    dT = scatter_rows(tj, alpha[:, None] * G[ti], n) + np.outer(ds_src, a_src) + np.outer(ds_dst, a_dst)
    dW1 = np.zeros(W1.shape)
    dW1[:n] = stepcheck.csr_mm(rp, cl, w, dT)          # X^T @ dT, X symmetric
    return {"conv1.weight": dW1, "conv1.bias": G.sum(0), "conv2.weight": dW2, "conv2.bias": gz.sum(0),
            "conv1.attn_src": ds_src @ T, "conv1.attn_dst": ds_dst @ T}


def float32_softmax_backward_error(P, GP):
    """One float32 rounding of the softmax backward p * (gp - p . gp): half an ulp of the row's largest |gp|, times p.  It
    is nothing beside the result - except in a row whose softmax has saturated (gp = p . gp up to rounding: the float64
    result is 1e-30, the float32 one this), and a hub's row saturates and has a |gp| of the order of its degree."""
    return 2.0 ** -24 * P * np.abs(GP).max(1, keepdims=True)


def worst_row_ratio(got, ref, row_floor=stepcheck.ROW_FLOOR):
    worst = 0.0
    for k in ATT_KEYS:
        r = np.asarray(ref[k], np.float64)
        r = r.reshape(r.shape[0], -1)
        worst = max(worst, stepcheck.row_error_ratio(np.asarray(got[k], np.float64).reshape(r.shape), r, row_floor))
    return worst


def f64_step(csrs, params, C=1.0, loss="cut", slope=SLOPE):
    """Float64 reference of one step of the batch: stepcheck.Ref(P, per-graph loss in float64, summed gradient by
    parameter name, 0) plus the figures of the precondition: (Ref, dict(margin, kink, zgap, leak)) - leak: the worst
    parameter-row ratio by which the gradient moves under `float32_softmax_backward_error`."""
    grad, leaked, Ps, losses = None, None, [], []
    gaps = dict(margin=np.inf, kink=np.inf, zgap=np.inf)
    for rp, cl, vl in csrs:
        f = f64_forward(rp, cl, vl, params, slope)
        if loss == "cut":
            value, GP = KR.hard_loss_and_gp(rp, cl, vl, KR.partition(f["P"], 3), 3, C)
        else:
            assert loss == "expected_cut", loss
            value, GP = KR.relaxed_loss_and_gp(rp, cl, vl, f["P"], C)
        g = f64_backward(f, GP, params, slope)
        grad = g if grad is None else {k: grad[k] + g[k] for k in grad}
        g = f64_backward(f, GP, params, slope, gz_error=float32_softmax_backward_error(f["P"], GP))
        leaked = g if leaked is None else {k: leaked[k] + g[k] for k in leaked}
        Ps.append(f["P"])
        losses.append(value)
        gaps["margin"] = min(gaps["margin"], KR.min_margin(f["P"], 3))
        gaps["kink"] = min(gaps["kink"], float(np.abs(f["pre"]).min()))
        several = (np.diff(rp) > 0)[f["ti"]]             # (a row whose only term is the self term: see `ZGAP`)
        if several.any():
            gaps["zgap"] = min(gaps["zgap"], float(np.abs(f["z"][several]).min()))
    gaps["leak"] = worst_row_ratio(leaked, grad)
    return stepcheck.Ref(np.concatenate(Ps), np.asarray(losses), grad, 0), gaps


def dense_loss(csr, params, Cc, loss, slope=SLOPE, dtype=None):
    """The scalar loss of one graph (and P) as torch operations on dense n x n operators, an independent form of the same
    model: masked dense softmax over the term-count matrix M = A + I, layer 2 as GraphConv(norm='both'), the relaxed loss
    written out, the hard loss as its straight-through surrogate sum(GP o P) with the constant GP = C * A_val @ onehot(S).
    `params`: torch tensors by name (requires_grad for a gradient); `dtype`: torch.float64 (default) or torch.float32."""
    import torch
    dtype = dtype or torch.float64
    rp, cl, vl = csr
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    A_, X = np.zeros((n, n)), np.zeros((n, n))
    np.add.at(A_, (rows, cl), 1.0)
    X[rows, cl] = 1.0 if vl is None else np.asarray(vl, np.float64)
    A_, X = torch.from_numpy(A_).to(dtype), torch.from_numpy(X).to(dtype)
    M = A_ + torch.eye(n, dtype=dtype)                            # how many terms of row i are node j
    dinv = A_.sum(1).clamp(min=1).rsqrt()
    W1, b1, W2, b2, a_src, a_dst = (params[k] for k in ATT_KEYS)
    T = X @ W1[:n]
    z = (T @ a_dst)[:, None] + (T @ a_src)[None, :]
    e = torch.nn.functional.leaky_relu(z, slope)
    alpha = torch.softmax(e + torch.log(M), dim=1)                # log 0 = -inf masks what is no term
    H = torch.relu(alpha @ T + b1)
    Z = dinv[:, None] * (A_ @ (dinv[:, None] * (H @ W2))) + b2
    P = torch.softmax(Z, dim=1)
    if loss == "cut":
        S = KR.partition(P.detach().numpy(), 3)
        GP = Cc * X @ torch.eye(3, dtype=dtype)[torch.from_numpy(S)]
        return (GP * P).sum(), P
    k = min(3, n)
    Pt = torch.cat([torch.eye(3, dtype=dtype)[:k] + P[:k] - P[:k].detach(), P[k:]])
    return -Cc / 2 * (X * (1 - Pt @ Pt.T)).sum(), P


def dense_step(csrs, params, Cc, loss, dtype=None):
    """(P, gradient by parameter name) of the batch through torch.autograd on the dense form, in `dtype`."""
    import torch
    dtype = dtype or torch.float64
    leaves = {k: torch.from_numpy(np.asarray(params[k])).to(dtype).requires_grad_(True) for k in ATT_KEYS}
    total, Ps = 0, []
    for csr in csrs:
        value, P = dense_loss(csr, leaves, Cc, loss, dtype=dtype)
        total = total + value
        Ps.append(P.detach().numpy())
    total.backward()
    return np.concatenate(Ps), {k: v.grad.numpy() for k, v in leaves.items()}


def float32_yardstick(csrs, params, Cc, loss, ref, row_floor=stepcheck.ROW_FLOOR):
    """What a float32 evaluation of the same formulas (torch, its own summation orders, on the CPU) gives on a case against
    the float64 Ref: (largest error of P, worst parameter-row ratio of the gradient over the six tensors)."""
    import torch
    P32, g32 = dense_step(csrs, params, Cc, loss, torch.float32)
    return float(np.abs(P32 - ref.P).max()), worst_row_ratio(g32, ref.grads, row_floor)


# ---- the cases of tests/test_gpu_attention.py
def star(leaves):
    g = nx.star_graph(leaves)                              # node 0 is the hub: leaves + 1 terms in its row
    nx.set_edge_attributes(g, 1, "weight")
    return g


def with_isolated_node(n, d, seed):
    g = util.near_regular(n, d, seed)
    g.add_node(n)                                          # degree 0: its only term is the self term
    return g


def with_self_loop(n, d, seed, node=7):
    g = util.near_regular(n, d, seed)
    g.add_edge(node, node, weight=1)
    return g


BUILDERS = {"reg": util.near_regular, "star": star, "iso": with_isolated_node, "loop": with_self_loop}
# shape -> (graph specs (builder, arguments...), hidden width, rows of conv1.weight)
SHAPES = {
    "n3": ([("reg", 3, 2, 1)], 16, 64),                              # every node is a terminal
    "n4": ([("reg", 4, 3, 2)], 16, 64),                              # one free node
    "deg0": ([("iso", 20, 3, 3)], 16, 64),                           # a node without neighbours: alpha_ii = 1
    "star70": ([("star", 70)], 16, 128),                             # the hub row has 71 terms: a second chunk of lanes
    "star140": ([("star", 140)], 16, 160),                           # 141 terms: a third
    "loop": ([("loop", 30, 4, 4)], 16, 64),                          # a self-loop edge: one more ordinary term
    "n65": ([("reg", 65, 7, 3)], 16, 128),                           # crosses one wave / one 64-row tile
    "n1030": ([("reg", 1030, 7, 4)], 16, 1040),                      # many tiles of the partial folds, second trip of the head
    "batch3": ([("reg", 60, 7, 5), ("reg", 97, 6, 6), ("reg", 5, 3, 7)], 16, 128),   # non-zero goff, mixed sizes
    "d12": ([("reg", 40, 12, 12)], 16, 64),                          # two batches of the 8-deep gather per row
    "h4": ([("reg", 70, 7, 8)], 4, 128),                             # column tail of a wave
    "h12": ([("reg", 70, 7, 9)], 12, 128),
    "h260": ([("reg", 70, 7, 10)], 260, 128),                        # more than one float4 pass per lane
    "h516": ([("reg", 70, 7, 11)], 516, 128),                        # a second column block; second slice of the hidden backward
}
Case = collections.namedtuple("Case", "shape weights loss seed")
# every shape with unit weights and the hard loss (its loss is then exactly -C * cut) and with real-valued weights and
# the relaxed loss, the wide layers the other way round as well.  The seeds are the first (from 0) for which the
# precondition above holds (tests/test_attention_host.py asserts it).
SEEDS = {("n3", "unit", "cut"): 298, ("star140", "unit", "cut"): 31, ("n1030", "unit", "cut"): 2, ("h260", "unit", "cut"): 7,
         ("h516", "unit", "cut"): 6, ("n3", "real", "expected_cut"): 3, ("star140", "real", "expected_cut"): 11,
         ("batch3", "real", "expected_cut"): 1, ("h260", "real", "expected_cut"): 1, ("h516", "real", "expected_cut"): 61,
         ("h260", "real", "cut"): 11, ("h516", "unit", "expected_cut"): 11}
CASES = [Case(s, w, l, SEEDS.get((s, w, l), 0))
         for s, w, l in ([(s, "unit", "cut") for s in SHAPES] + [(s, "real", "expected_cut") for s in SHAPES] +
                         [("h260", "real", "cut"), ("h516", "unit", "expected_cut")])]


def case_id(c):
    return f"{c.shape}-{c.weights}-{c.loss}"


def case_graphs(c):
    """The networkx graphs of a case: unit weights or real-valued float32 weights in [0.3, 3)."""
    graphs = []
    for i, (kind, *args) in enumerate(SHAPES[c.shape][0]):
        g = BUILDERS[kind](*args)
        if c.weights == "real":
            rng = np.random.RandomState(100 + 7 * i + len(args))
            for u, v in g.edges():
                g[u][v]["weight"] = float(np.float32(rng.uniform(0.3, 3.0)))
        graphs.append(g)
    return graphs


def random_params(N, F, seed):
    """float32 parameters by name (numpy: the same values with and without a GPU): kway_ref.random_params at K = 3 plus the
    attention vectors, uniform within the xavier bound of an [F, 1] matrix - the model's own initialisation."""
    p = KR.random_params(N, F, 3, seed)
    rng = np.random.RandomState(2000 + seed)
    bound = np.sqrt(6.0 / (F + 1))
    p["conv1.attn_src"] = rng.uniform(-bound, bound, F).astype(np.float32)
    p["conv1.attn_dst"] = rng.uniform(-bound, bound, F).astype(np.float32)
    return p


def case_params(c):
    _specs, hidden, N = SHAPES[c.shape]
    return random_params(N, hidden, c.seed)


def vector_rows(got, ref, grad_bar, row_tol, row_floor, what=None):
    """da_src / da_dst judged as parameter rows (each entry a row, as a bias entry is): stepcheck.compare_grads' two rules."""
    worst = 0.0
    for key in ATT_KEYS[4:]:
        r = np.asarray(ref[key], np.float64).reshape(-1, 1)
        g = np.asarray(got[key], np.float64).reshape(-1, 1)
        assert np.isfinite(g).all(), (what, key)
        bar = grad_bar * max(1.0, float(np.abs(r).max()))
        assert np.abs(g - r).max() <= bar, (what, key, float(np.abs(g - r).max()), bar)
        ratio = stepcheck.row_error_ratio(g, r, row_floor)
        assert ratio <= row_tol, (what, key, ratio)
        worst = max(worst, ratio)
    return worst
