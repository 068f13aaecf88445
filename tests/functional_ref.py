"""Float64 restatement of the functional form of the model (include/gcnmaxcut.h, gmc_fn_*; gcn_max_cut_amd.functional) and
the cases the GPU tests run.

Nothing of the model is restated twice: with the padded adjacency as features the forward and the backward are
stepcheck.f64_forward_sparse / f64_backward_sparse, the losses with terminals are kway_ref.hard_loss_and_gp /
relaxed_loss_and_gp.  What is added here is what those do not hold:

* dense features X [n, N]: layer 1's feature transform is X @ W1 (no edge weight anywhere in the layers), the backward
  gives dW1 = X^T @ U and dX = U @ W1^T (`forward`, `backward`);
* `terminals=False`: no node is forced - S is the plain argmax, Pt = P (`loss_and_gp`);
* `f32_eval`: the same formulas with every intermediate rounded to float32, in numpy's own order and with nothing of the
  library in it - what any float32 evaluation can promise on a case.

The cases (`CASES`) live here so that the CPU test (tests/test_functional_host.py) can assert on this reference what the
GPU test relies on: no layer-1 pre-activation within kway_ref.KINK of the relu kink, no argmax margin (of ANY row: without
terminals every row decodes) under kway_ref.MARGIN, no row whose largest probability is within large_ref.UNSATURATED of 1,
and `f32_eval` within HALF of each bar the GPU test asks - P_TOL for P, ORACLE_BAR and ROW_TOL / ROW_FLOOR for the gradients
and dX.  The seeds are the first from 0 for which all of that holds."""
import collections
import functools

import numpy as np

from tests import kway_ref as KR
from tests import large_ref as LR
from tests import stepcheck
from tests.stepcheck import KEYS

CC = 1.3
LOSSES = [(relaxed, terminals) for relaxed in (False, True) for terminals in (True, False)]


# ---- the losses
def loss_and_gp(csr, P, C=1.0, relaxed=False, terminals=True):
    """(loss, GP [n,K]) of probabilities P [n,K] in float64.  terminals: kway_ref's two functions; without: S = the plain
    argmax (first maximum), Pt = P."""
    rp, cl, vl = csr
    P = np.asarray(P, np.float64)
    K = P.shape[1]
    if terminals:
        if relaxed:
            return KR.relaxed_loss_and_gp(rp, cl, vl, P, C)
        return KR.hard_loss_and_gp(rp, cl, vl, KR.partition(P, K), K, C)
    if not relaxed:
        return KR.hard_loss_and_gp(rp, cl, vl, P.argmax(1), K, C)
    rp, cl, w, rows = KR._edges(rp, cl, vl)
    dots = (P[rows] * P[cl]).sum(1)
    return -C * 0.5 * float((w * (1.0 - dots)).sum()), C * stepcheck.csr_mm(rp, cl, w, P)


def brute_force_best_cut(csr, K):
    """The largest cut of any assignment of the graph's nodes to K classes (no node fixed), by enumeration."""
    rp, cl, w, rows = KR._edges(*csr)
    n = len(rp) - 1
    best = 0.0
    for code in range(K ** n):
        S = np.array([code // K ** i % K for i in range(n)])
        best = max(best, 0.5 * float((w * (S[rows] != S[cl])).sum()))
    return best


# ---- the model
def forward(csr, params, X=None):
    """stepcheck.f64_forward_sparse; with X [n,N]: the same layers on T0 = dinv o (X @ W1)."""
    rp, cl, vl = csr
    W1, b1, W2, b2 = (np.asarray(params[k], np.float64) for k in KEYS)
    if X is None:
        return stepcheck.f64_forward_sparse(rp, cl, vl, W1, b1, W2, b2)
    X = np.asarray(X, np.float64)
    dinv = 1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(np.float64))
    T0 = dinv[:, None] * (X @ W1)
    pre = dinv[:, None] * stepcheck.csr_mm(rp, cl, None, T0) + b1
    H = np.maximum(pre, 0.0)
    Z = dinv[:, None] * stepcheck.csr_mm(rp, cl, None, dinv[:, None] * H @ W2) + b2
    E = np.exp(Z - Z.max(1, keepdims=True))
    return dict(rp=rp, cl=cl, w=None, dinv=dinv, pre=pre, H=H, P=E / E.sum(1, keepdims=True), X=X)


def backward(f, GP, params):
    """(gradient by parameter name, dX or None) of sum(GP o P): stepcheck.f64_backward_sparse; with X its lines with
    dW1 = X^T @ U and dX = U @ W1^T, U = dinv o (A @ (dinv o g))."""
    W1, W2 = np.asarray(params[KEYS[0]], np.float64), np.asarray(params[KEYS[2]], np.float64)
    if "X" not in f:
        return stepcheck.named(stepcheck.f64_backward_sparse(f, GP, W2, W1.shape[0])), None
    rp, cl, dinv, H, P = f["rp"], f["cl"], f["dinv"], f["H"], f["P"]
    gz = P * (GP - (GP * P).sum(1, keepdims=True))
    gy2 = stepcheck.csr_mm(rp, cl, None, dinv[:, None] * gz)
    g = np.where(H > 0, dinv[:, None] * (gy2 @ W2.T), 0.0)
    U = dinv[:, None] * stepcheck.csr_mm(rp, cl, None, dinv[:, None] * g)
    return stepcheck.named(dict(W1=f["X"].T @ U, b1=g.sum(0), W2=(dinv[:, None] * H).T @ gy2, b2=gz.sum(0))), U @ W1.T


# ---- the same in float32: every intermediate rounded, numpy's own order (reduceat over the CSR rows)
def _mm32(rp, cl, w, M):
    f32 = np.float32
    G = M[cl] if w is None else (np.asarray(w, f32)[:, None] * M[cl]).astype(f32)
    out = np.zeros((len(rp) - 1, M.shape[1]), f32)
    live = np.nonzero(np.diff(rp))[0]
    if live.size:
        out[live] = np.add.reduceat(G, np.asarray(rp[:-1])[live], axis=0, dtype=f32)
    return out


def f32_eval(csr, params, X, gp_of):
    """(P, gradient by name, dX or None) in float32; gp_of(P32) -> GP (rounded to float32 here)."""
    f32 = np.float32
    rp, cl, vl = csr
    W1, b1, W2, b2 = (np.asarray(params[k], f32) for k in KEYS)
    d = (1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(f32))).astype(f32)[:, None]
    T0 = (d * (_mm32(rp, cl, vl, W1[:len(rp) - 1]) if X is None else (np.asarray(X, f32) @ W1).astype(f32))).astype(f32)
    H = np.maximum(((d * _mm32(rp, cl, None, T0)).astype(f32) + b1).astype(f32), 0).astype(f32)
    Z = ((d * _mm32(rp, cl, None, (d * (H @ W2).astype(f32)).astype(f32))).astype(f32) + b2).astype(f32)
    E = np.exp((Z - Z.max(1, keepdims=True)).astype(f32)).astype(f32)
    P = (E / E.sum(1, keepdims=True, dtype=f32)).astype(f32)
    GP = np.asarray(gp_of(P), f32)
    gz = (P * (GP - (GP * P).sum(1, keepdims=True, dtype=f32))).astype(f32)
    gy2 = _mm32(rp, cl, None, (d * gz).astype(f32))
    g = np.where(H > 0, d * (gy2 @ W2.T).astype(f32), 0).astype(f32)
    U = (d * _mm32(rp, cl, None, (d * g).astype(f32))).astype(f32)
    dW1 = np.zeros_like(W1)
    if X is None:
        dW1[:len(rp) - 1] = _mm32(rp, cl, vl, U)
    else:
        dW1 = (np.asarray(X, f32).T @ U).astype(f32)
    grads = {KEYS[0]: dW1, KEYS[1]: g.sum(0, dtype=f32), KEYS[2]: ((d * H).astype(f32).T @ gy2).astype(f32),
             KEYS[3]: gz.sum(0, dtype=f32)}
    return P, grads, None if X is None else (U @ W1.T).astype(f32)


# ---- judging (the bars are stepcheck's)
def grad_ratios(got, ref):
    """(worst |got - ref| / (ORACLE_BAR * max(1, max|ref|)), worst row ratio / ROW_TOL) over a dict of tensors: both at
    most 1 means within the bars."""
    worst_abs, worst_row = 0.0, 0.0
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        g = np.asarray(got[k], np.float64).reshape(r.shape)
        assert np.isfinite(g).all(), k
        worst_abs = max(worst_abs, float(np.abs(g - r).max()) / (stepcheck.ORACLE_BAR * max(1.0, float(np.abs(r).max()))))
        worst_row = max(worst_row, stepcheck.row_error_ratio(g, r, stepcheck.ROW_FLOOR) / stepcheck.ROW_TOL)
    return worst_abs, worst_row


# ---- the cases
# shape -> graph specs: ("circ", n, d, chord seed), ("star", leaves, hub); "K" / "K+1" in n: of the run's class count
SHAPES = {
    "nK": [("circ", "K", 3, None)],                   # every node a terminal (when there are terminals)
    "nK1": [("circ", "K+1", 3, None)],
    "n65": [("circ", 65, 7, 1)],                      # crosses one wave
    "n257": [("circ", 257, 7, 2)],                    # a second tile of one row
    "n300": [("circ", 300, 7, 3)],
    "star70": [("star", 70, 5)],                      # a row of 70 entries: the wave-per-row path
    "batch": [("circ", 5, 3, None), ("circ", 300, 7, 4), ("circ", 65, 6, None), ("circ", 257, 7, 5)],
    "n4200": [("circ", 4200, 7, 6)],                  # beyond the one-workgroup heads
}
# features: "adj" (the padded adjacency) or the N of dense features X (62: padded to 64 columns)
Case = collections.namedtuple("Case", "shape K hidden weights features seed")
CASES = [
    Case("nK", 2, 4, "unit", "adj", 0), Case("nK", 8, 12, "real", "adj", 0), Case("nK", 4, 36, "unit", 64, 0),
    Case("nK1", 3, 36, "unit", "adj", 0), Case("nK1", 4, 4, "real", 64, 0), Case("nK1", 8, 12, "unit", 62, 0),
    Case("n65", 2, 12, "real", "adj", 0), Case("n65", 8, 36, "unit", 62, 0),
    Case("n257", 3, 4, "real", 64, 0), Case("n257", 4, 12, "unit", "adj", 0),
    Case("n300", 2, 36, "unit", 62, 0), Case("n300", 8, 4, "real", "adj", 0),
    Case("star70", 3, 12, "unit", "adj", 0), Case("star70", 8, 4, "real", "adj", 0), Case("star70", 2, 12, "unit", 64, 1),
    Case("batch", 2, 12, "real", "adj", 0), Case("batch", 4, 36, "unit", 64, 1), Case("batch", 3, 4, "unit", "adj", 0),
    Case("batch", 4, 12, "real", 62, 0),
    Case("n4200", 3, 12, "unit", "adj", 0), Case("n4200", 8, 4, "real", "adj", 0), Case("n4200", 2, 36, "real", 64, 0),
]


def case_id(c):
    return f"{c.shape}-K{c.K}-h{c.hidden}-{c.weights}-{c.features}"


@functools.lru_cache(maxsize=None)
def case_csrs(c):
    """[(rowptr int32, col int32, weights float32 or None)] of a case (a GraphBatch takes graphs of at least 3 nodes)."""
    out = []
    for i, spec in enumerate(SHAPES[c.shape]):
        if spec[0] == "star":
            n, rp, col = LR.star(spec[1], spec[2])
        else:
            _kind, n, d, seed = spec
            n, rp, col = LR.circulant(max({"K": c.K, "K+1": c.K + 1}.get(n, n), 3), d, seed)
        w = LR.edge_weights(n, rp, col, 10 * c.seed + i) if c.weights == "real" else None
        out.append((rp.astype(np.int32), col.astype(np.int32), w))
    return out


def case_handles(pkg, c):
    return [pkg.GraphHandle(len(rp) - 1, rp, col, w) for rp, col, w in case_csrs(c)]


def case_rows(c):
    return sum(len(rp) - 1 for rp, _cl, _vl in case_csrs(c))


def case_params(c):
    """kway_ref.random_params; rows of conv1.weight: the largest graph rounded up to 4 (adjacency), or the features' N."""
    n_max = max(len(rp) - 1 for rp, _cl, _vl in case_csrs(c))
    N = (n_max + 3) // 4 * 4 if c.features == "adj" else c.features
    return KR.random_params(N, c.hidden, c.K, c.seed)


def case_features(c):
    """X [R, N] float32 for a case with dense features (None for the adjacency)."""
    if c.features == "adj":
        return None
    return np.random.RandomState(3000 + c.seed).uniform(-1.0, 1.0, (case_rows(c), c.features)).astype(np.float32)


def case_gp(c):
    """A dLoss/dP [R,K] drawn at random, not from a loss: the backward as a linear map."""
    return np.random.RandomState(4000 + c.seed).standard_normal((case_rows(c), c.K)).astype(np.float32)


def split(c, M):
    """Per-graph pieces of a [R, ...] array (None stays None)."""
    offs = np.cumsum([0] + [len(rp) - 1 for rp, _cl, _vl in case_csrs(c)])
    return [None if M is None else M[a:b] for a, b in zip(offs[:-1], offs[1:])]


Ref = collections.namedtuple("Ref", "P pre grads dX losses loss_gp loss_grads loss_dX")


@functools.lru_cache(maxsize=None)
def reference(c):
    """Float64 of a case: P [R,K], the layer-1 pre-activations, gradient and dX of sum(case_gp o P), and per loss variant of
    LOSSES at C = CC the per-graph losses [B], GP [R,K] and the gradient and dX of the summed loss."""
    csrs, params = case_csrs(c), case_params(c)
    fs = [forward(csr, params, X) for csr, X in zip(csrs, split(c, case_features(c)))]

    def total(gps):
        grads, dXs = None, []
        for f, gp in zip(fs, gps):
            g, dX = backward(f, np.asarray(gp, np.float64), params)
            grads = g if grads is None else {k: grads[k] + g[k] for k in g}
            dXs.append(dX)
        return grads, None if dXs[0] is None else np.concatenate(dXs)

    grads, dX = total(split(c, case_gp(c)))
    losses, loss_gp, loss_grads, loss_dX = {}, {}, {}, {}
    for variant in LOSSES:
        per = [loss_and_gp(csr, f["P"], CC, *variant) for csr, f in zip(csrs, fs)]
        losses[variant] = np.array([v for v, _gp in per])
        loss_gp[variant] = np.concatenate([gp for _v, gp in per])
        loss_grads[variant], loss_dX[variant] = total([gp for _v, gp in per])
    return Ref(np.concatenate([f["P"] for f in fs]), np.concatenate([f["pre"] for f in fs]), grads, dX, losses, loss_gp,
               loss_grads, loss_dX)


def f32_figures(c):
    """What `f32_eval` leaves of each bar on a case, as fractions of the bar: P, and for the random GP and every loss
    variant the gradient (absolute, per row) and dX (absolute, per row).  Returns {name: fraction}."""
    csrs, params, ref = case_csrs(c), case_params(c), reference(c)
    Xs, out = split(c, case_features(c)), {}

    def run(name, gp_ofs, ref_grads, ref_dX):
        P, grads, dXs = [], None, []
        for csr, X, gp_of in zip(csrs, Xs, gp_ofs):
            p, g, dX = f32_eval(csr, params, X, gp_of)
            P.append(p)
            grads = g if grads is None else {k: (grads[k] + g[k]).astype(np.float32) for k in g}
            dXs.append(dX)
        out["P"] = max(out.get("P", 0.0), float(np.abs(np.concatenate(P) - ref.P).max()) / stepcheck.P_TOL)
        out[f"{name} abs"], out[f"{name} row"] = grad_ratios(grads, ref_grads)
        if ref_dX is not None:
            out[f"{name} dX abs"], out[f"{name} dX row"] = grad_ratios({"dX": np.concatenate(dXs)}, {"dX": ref_dX})

    run("random", [lambda _p, gp=gp: gp for gp in split(c, case_gp(c))], ref.grads, ref.dX)
    for variant in LOSSES:
        run(f"relaxed={variant[0]} terminals={variant[1]}",
            [lambda p, csr=csr: loss_and_gp(csr, p, CC, *variant)[1] for csr in csrs], ref.loss_grads[variant],
            ref.loss_dX[variant])
    return out


def preconditions(c):
    """(smallest |layer-1 pre-activation|, smallest top-2 margin over ALL rows, smallest 1 - largest probability of a row)
    of a case in float64.  The last is large_ref's rule about the number format: a float32 P carries 1 - p_max to
    eps32 / (1 - p_max) only, and the softmax backward of a saturated row is made of that difference - a hub's logits are
    many times a leaf's, so the star gets there easily."""
    ref = reference(c)
    return float(np.abs(ref.pre).min()), KR.min_margin(ref.P, 0), float((1.0 - ref.P.max(1)).min())


def well_posed(c):
    gap, margin, unsaturated = preconditions(c)
    return gap >= KR.KINK and margin >= KR.MARGIN and unsaturated >= LR.UNSATURATED
