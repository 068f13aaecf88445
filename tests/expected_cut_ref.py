"""Float64 restatement of the relaxed loss (GMC_LOSS_EXPECTED_CUT, include/gcnmaxcut.h) on a graph's CSR, in numpy:

    Pt   = P with rows 0, 1, 2 replaced by e0, e1, e2            (override_fixed_nodes, straight-through)
    loss = -C/2 * sum_u sum_{v in N(u)} w_uv (1 - Pt_u . Pt_v)   (compute_loss on Pt, no one-hot step)
    GP_u = C * sum_{v in N(u)} w_uv Pt_v                         for every row u, rows 0..2 included

and the training step around it from tests/stepcheck.py's forward and backward (unchanged: everything after GP is
what the hard loss runs).  tests/test_expected_cut_host.py ties this to autograd through the package's own
compute_loss(override_fixed_nodes(P)); the GPU tests compare the kernels with it."""
import numpy as np

from tests import stepcheck
from tests.stepcheck import KEYS


def override(P):
    Pt = np.array(P, np.float64)
    Pt[:3] = np.eye(3)
    return Pt


def loss_and_gp(rp, cl, vl, P, C=1.0):
    """(loss, GP [n,3]) of the definition above; vl None = unit weights."""
    rp, cl = np.asarray(rp), np.asarray(cl)
    Pt = override(P)
    w = np.ones(len(cl)) if vl is None else np.asarray(vl, np.float64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    dots = (Pt[rows] * Pt[cl]).sum(1)
    return -C * 0.5 * float((w * (1.0 - dots)).sum()), C * stepcheck.csr_mm(rp, cl, w, Pt)


def hard_loss_and_gp(rp, cl, vl, S, C=1.0):
    """The hard loss of partition S on the same CSR: -C * cut(S), GP = C * A_val @ onehot(S)."""
    rp, cl = np.asarray(rp), np.asarray(cl)
    S = np.asarray(S).astype(np.int64)
    w = np.ones(len(cl)) if vl is None else np.asarray(vl, np.float64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return -C * 0.5 * float((w * (S[rows] != S[cl])).sum()), C * stepcheck.csr_mm(rp, cl, w, np.eye(3)[S])


def total_weight(csrs):
    """Sum of the undirected edge weights of the graphs: what the loss bars scale with."""
    return sum(0.5 * float(len(cl) if vl is None else np.abs(np.asarray(vl, np.float64)).sum()) for _rp, cl, vl in csrs)


def head_from_p(rp, cl, P, GP):
    """(db2, GY2 [n,3]) of the head's backward for a given dLoss/dP, at the given P: softmax backward and A @ (dinv o GZ)."""
    dinv = 1.0 / np.sqrt(np.maximum(np.diff(rp), 1).astype(np.float64))
    P = np.asarray(P, np.float64)
    gz = P * (GP - (GP * P).sum(1, keepdims=True))
    return gz.sum(0), stepcheck.csr_mm(rp, cl, None, dinv[:, None] * gz)


def f64_step(csrs, params, C=1.0, keeps=None, p=0.0):
    """Float64 reference of one relaxed training step of the batch: stepcheck.Ref(P, per-graph loss in float64, summed
    gradient by parameter name, 0).  keeps (optional): per graph the [n, F] mask of kept hidden units of dropout p - H
    becomes H o keep / (1 - p) before the layer-2 product, as the library applies it."""
    W = [np.asarray(params[k], np.float64) for k in KEYS]
    W1, b1, W2, b2 = W
    grad, Ps, losses = None, [], []
    for i, (rp, cl, vl) in enumerate(csrs):
        n = len(rp) - 1
        f = stepcheck.f64_forward_sparse(rp, cl, vl, *W)
        if keeps is not None:
            dinv = f["dinv"]
            Hd = f["H"] * keeps[i] / (1.0 - p)
            Z = dinv[:, None] * stepcheck.csr_mm(rp, cl, None, dinv[:, None] * Hd @ W2) + b2
            E = np.exp(Z - Z.max(1, keepdims=True))
            f.update(P=E / E.sum(1, keepdims=True), H=Hd)
        loss, GP = loss_and_gp(rp, cl, vl, f["P"], C)
        if keeps is None:
            g = stepcheck.f64_backward_sparse(f, GP, W2, W1.shape[0])
        else:   # the mask's factor rides on the hidden gradient (stepcheck's backward knows no dropout)
            dinv, P, Hd = f["dinv"], f["P"], f["H"]
            gz = P * (GP - (GP * P).sum(1, keepdims=True))
            gy2 = stepcheck.csr_mm(rp, cl, None, dinv[:, None] * gz)
            gg = np.where(Hd > 0, dinv[:, None] * (gy2 @ W2.T) / (1.0 - p), 0.0)
            gy1 = stepcheck.csr_mm(rp, cl, None, dinv[:, None] * gg)
            dW1 = np.zeros_like(W1)
            dW1[:n] = stepcheck.csr_mm(rp, cl, f["w"], dinv[:, None] * gy1)
            g = dict(W1=dW1, b1=gg.sum(0), W2=(dinv[:, None] * Hd).T @ gy2, b2=gz.sum(0))
        grad = g if grad is None else {k: grad[k] + g[k] for k in grad}
        Ps.append(f["P"])
        losses.append(loss)
    return stepcheck.Ref(np.concatenate(Ps), np.asarray(losses), stepcheck.named(grad), 0)
