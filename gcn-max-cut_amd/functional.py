"""The functional form of the model: differentiable probabilities and losses for any class count and graph size.

``GCNSoftmax.forward`` with gradients, ``FusedEngine.backward_from_gp`` and ``Training.cut_loss`` are the reference's
3-class model on graphs of up to 4096 nodes.  This module is the same open loop

    P = probabilities(net, g); loss = cut_loss(g, P, relaxed=True); loss.backward(); optimizer.step()

for ``number_classes`` 2..8 and graphs of up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes, over the gmc_fn_* entry points of
include/gcnmaxcut.h (csrc/functional.hip): :func:`gcn_softmax` is a ``torch.autograd.Function`` of the four parameter
tensors (and of dense features ``X``), :func:`cut_loss` one of the probabilities.  Everything between is torch's: a
caller's own loss on ``P``, any optimizer or scheduler, gradient clipping, a regulariser, learned embeddings.  It sits
beside the ``nn.Module`` as ``search_dataset`` sits beside ``decode_dataset``; nothing here touches a ``FusedEngine``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import hip
from .engine import MAX_HIDDEN, PARAM_ORDER, flat_layout, padded_features
from .graph import GraphBatch, GraphHandle


def _batch_of(g, device, structure_only: bool = False) -> GraphBatch:
    """``g`` as a device batch: a GraphBatch as it is, a GraphHandle as its cached one-graph batch (with its own edge
    weights; ``structure_only``: without, for dense features)."""
    if isinstance(g, GraphBatch):
        return g
    if not isinstance(g, GraphHandle):
        raise TypeError(f"expected a GraphHandle or a GraphBatch, got {type(g)}")
    from .Training.TrainingNeural import _dense_batch_of, graph_batch_of
    return _dense_batch_of(g, device) if structure_only else graph_batch_of(g, None, device)


def _check_classes(K: int) -> None:
    if not 2 <= K <= hip.KWAY_MAX_CLASSES:
        raise ValueError(f"number_classes must be in 2..{hip.KWAY_MAX_CLASSES}, got {K}")


class _GCNSoftmax(torch.autograd.Function):
    """softmax(conv2(relu(conv1(.)))) over gmc_fn_forward / gmc_fn_backward.  The call owns its flat parameter copy (hidden
    width padded to a multiple of 4: the pad columns are zero, their gradient entries exact zeros) and its workspace."""

    @staticmethod
    def forward(ctx, batch, X, W1, b1, W2, b2):
        device = hip.require_gpu()
        lib = hip.load()
        (N, F), K = W1.shape, W2.shape[1]
        Fp = (F + 3) // 4 * 4
        offs, count = flat_layout(N, Fp, K)
        flat = torch.zeros(count, dtype=torch.float32, device=device)
        views = {"conv1.weight": flat[offs[0]:offs[1]].view(N, Fp)[:, :F], "conv1.bias": flat[offs[1]:offs[2]][:F],
                 "conv2.weight": flat[offs[2]:offs[3]].view(Fp, K)[:F], "conv2.bias": flat[offs[3]:offs[4]]}
        for k, t in zip(PARAM_ORDER, (W1, b1, W2, b2)):
            views[k].copy_(t.detach())
        ctx.batch, ctx.shape, ctx.offs, ctx.count = batch, (N, F, Fp, K), offs, count
        ctx.like = [(t.device, t.dtype) for t in (W1, b1, W2, b2)]
        ctx.x_like = None if X is None else (X.device, X.dtype)
        P = torch.empty((batch.R, K), dtype=torch.float32, device=device)
        if batch.B == 0:   # nothing to launch (empty tensors have no device pointer to hand over)
            ctx.save_for_backward(P)
            return P
        if X is not None and tuple(X.shape) != (batch.R, N):
            raise ValueError(f"features must be [{batch.R}, {N}], got {tuple(X.shape)}")
        Xd = None if X is None else padded_features(X, batch.R, N, device)
        ctx.model = hip.GmcModel(N=N, F=Fp, K=K, W1=hip.ptr(flat), b1=hip.ptr(flat) + 4 * offs[1],
                                 W2=hip.ptr(flat) + 4 * offs[2], b2=hip.ptr(flat) + 4 * offs[3])
        need = int(lib.gmc_fn_workspace_bytes(batch.ref(), C.byref(ctx.model), int(X is not None)))
        ctx.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
        rc = lib.gmc_fn_forward(batch.ref(), C.byref(ctx.model), hip.ptr(Xd), 0 if Xd is None else Xd.shape[1],
                                hip.ptr(ctx.ws), ctx.ws.numel(), hip.ptr(P), hip.stream())
        hip.check(rc, "gmc_fn_forward")
        ctx.consumed = False   # (the backward turns the workspace's H into its own scratch)
        ctx.save_for_backward(P, flat, *(() if Xd is None else (Xd,)))
        return P

    @staticmethod
    def backward(ctx, gp):
        P, *rest = ctx.saved_tensors
        N, F, Fp, K = ctx.shape
        offs, batch = ctx.offs, ctx.batch
        need_x = ctx.x_like is not None and ctx.needs_input_grad[1]
        grad = torch.zeros(ctx.count, dtype=torch.float32, device=P.device)
        dX = None
        if batch.B:
            Xd = rest[1] if len(rest) > 1 else None
            GP = gp.to(P.device, torch.float32).contiguous()
            dX = torch.empty_like(Xd) if need_x else None
            if ctx.consumed:   # a second backward through a retained graph: the forward once more, into the same workspace
                rc = hip.load().gmc_fn_forward(batch.ref(), C.byref(ctx.model), hip.ptr(Xd), 0 if Xd is None else Xd.shape[1],
                                               hip.ptr(ctx.ws), ctx.ws.numel(), hip.ptr(torch.empty_like(P)), hip.stream())
                hip.check(rc, "gmc_fn_forward")
            ctx.consumed = True
            rc = hip.load().gmc_fn_backward(batch.ref(), C.byref(ctx.model), hip.ptr(Xd), 0 if Xd is None else Xd.shape[1],
                                            hip.ptr(ctx.ws), ctx.ws.numel(), hip.ptr(P), hip.ptr(GP), hip.ptr(grad),
                                            hip.ptr(dX), 0 if dX is None else dX.shape[1], hip.stream())
            hip.check(rc, "gmc_fn_backward")
        elif need_x:
            dX = torch.zeros((0, N), dtype=torch.float32, device=P.device)
        views = (grad[offs[0]:offs[1]].view(N, Fp)[:, :F], grad[offs[1]:offs[2]][:F], grad[offs[2]:offs[3]].view(Fp, K)[:F],
                 grad[offs[3]:offs[4]])
        grads = tuple(v.to(*like).clone() if need else None
                      for v, like, need in zip(views, ctx.like, ctx.needs_input_grad[2:]))
        return (None, None if dX is None else dX[:, :N].to(*ctx.x_like)) + grads


def gcn_softmax(g, W1: torch.Tensor, b1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor,
                X: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``P`` [R,K] = softmax(conv2(relu(conv1(.)))) for the graph(s) ``g`` - a GraphHandle (its own edge weights) or a
    GraphBatch - and the parameters ``W1`` [N,F], ``b1`` [F], ``W2`` [F,K], ``b2`` [K] of the two GraphConv layers, exactly
    what ``GCNSoftmax.forward`` returns: no terminals, no loss, no decode.  Differentiable in the four parameters and in
    ``X`` (gmc_fn_forward / gmc_fn_backward): K in 2..8, any hidden width 1..4096, graphs of up to
    ``hip.LARGE_MAX_GRAPH_NODES`` nodes.

    ``X`` None: the features are the padded adjacency with the graph's edge weights, N >= the largest graph.  Otherwise
    node features [R, N] (the rows of the batch's graphs stacked), any N: layer 1 then ignores edge weights, and ``X`` gets a
    gradient when it requires one (learned embeddings); constant ``X`` with parameter gradients is fine too."""
    if W1.dim() != 2 or W2.dim() != 2 or b1.shape != W1.shape[1:] or W2.shape[0] != W1.shape[1] or b2.shape != W2.shape[1:]:
        raise ValueError(f"parameters must be W1 [N,F], b1 [F], W2 [F,K], b2 [K], got {tuple(W1.shape)}, {tuple(b1.shape)}, "
                         f"{tuple(W2.shape)}, {tuple(b2.shape)}")
    _check_classes(W2.shape[1])
    if not 1 <= W1.shape[1] <= MAX_HIDDEN:
        raise ValueError(f"hidden_dim must be in 1..{MAX_HIDDEN} (include/gcnmaxcut.h: GMC_MAX_HIDDEN), got {W1.shape[1]}")
    device = hip.require_gpu()
    batch = _batch_of(g, device, structure_only=X is not None)
    if batch.B and int(batch.sizes.min()) < W2.shape[1]:
        raise ValueError(f"number_classes = {W2.shape[1]}: every graph needs at least {W2.shape[1]} nodes, got one with "
                         f"{int(batch.sizes.min())}")
    return _GCNSoftmax.apply(batch, X, W1, b1, W2, b2)


def probabilities(net, g, X: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`gcn_softmax` with the parameters of a ``GCNSoftmax`` of any ``number_classes``: what ``net(g, X)`` returns,
    differentiable whatever the class count and the graph's size.  ``X`` None stands for the padded adjacency."""
    return gcn_softmax(g, net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias, X)


class _CutLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, batch, C_, kind, terminals):
        device = hip.require_gpu()
        lib = hip.load()
        K = P.shape[1]
        ctx.like = (P.device, P.dtype)
        Pd = P.detach().to(device, torch.float32).contiguous()
        losses = torch.zeros(batch.B, dtype=torch.float32, device=device)
        GP = torch.zeros((batch.R, K), dtype=torch.float32, device=device)
        if batch.B:
            need = int(lib.gmc_fn_cut_loss_workspace_bytes(batch.ref(), K))
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
            rc = lib.gmc_fn_cut_loss_f32(batch.ref(), K, int(terminals), hip.ptr(Pd), C_, kind, hip.ptr(ws), ws.numel(),
                                         hip.ptr(losses), hip.ptr(GP), hip.stream())
            hip.check(rc, "gmc_fn_cut_loss_f32")
        ctx.save_for_backward(GP)
        return losses.sum().to(*ctx.like)

    @staticmethod
    def backward(ctx, grad_out):
        (GP,) = ctx.saved_tensors
        return (grad_out.to(GP.device, GP.dtype) * GP).to(*ctx.like), None, None, None, None


def cut_loss(g, P: torch.Tensor, C: float = 1.0, relaxed: bool = False, terminals: bool = True) -> torch.Tensor:
    """The scalar loss of probabilities ``P`` [n,K] on graph ``g`` (a GraphHandle with its own edge weights, or a GraphBatch
    with ``P`` [R,K]: then the sum over its graphs), K in 2..8, computed and differentiated on the device in O(edges)
    (gmc_fn_cut_loss_f32).  At K = 3 with ``terminals`` it is ``Training.cut_loss``.

    * ``relaxed=False``: ``-C * cut(S)`` of the argmax decode S (first maximum wins), with the straight-through gradient
      ``C * A_val @ onehot_K(S)``;
    * ``relaxed=True``: the expected cut under independent rounding, ``-C/2 * sum_uv w_uv (1 - Pt_u . Pt_v)`` with gradient
      ``C * A_val @ Pt``;
    * ``terminals=True``: nodes 0..K-1 of every graph are fixed to classes 0..K-1 (rows 0..K-1 of ``Pt`` are the unit
      vectors), as everywhere in the library; ``terminals=False``: no node is forced - unconstrained max-K-cut; a model
      trained that way is decoded by the plain argmax."""
    if P.dim() != 2:
        raise ValueError(f"P must be [rows, number_classes], got {tuple(P.shape)}")
    _check_classes(P.shape[1])
    device = hip.require_gpu()
    batch = _batch_of(g, device)
    if P.shape[0] != batch.R:
        raise ValueError(f"P must be [{batch.R}, {P.shape[1]}], got {tuple(P.shape)}")
    if terminals and batch.B and int(batch.sizes.min()) < P.shape[1]:
        raise ValueError(f"number_classes = {P.shape[1]}: with terminals every graph needs at least {P.shape[1]} nodes, got "
                         f"one with {int(batch.sizes.min())}")
    return _CutLoss.apply(P, batch, float(C), hip.LOSS_KINDS["expected_cut" if relaxed else "cut"], bool(terminals))
