"""TrainingNeural - drop-in API of ``python/Training/TrainingNeural.py`` on MI355X.

Same public names, signatures, return values, prints and checkpoint layout as the
reference module; the arithmetic of the hot loop (``train_single_epoch`` :341-390,
``GCNSoftmax.forward`` :79-85, ``evaluate_model`` :537-570) runs in the hand-written HIP
kernels of ``libgcnmaxcut_hip.so`` through :class:`gcn_max_cut_amd.engine.FusedEngine`.
There is no CPU fallback: without the HIP library and a GPU the compute entry points
raise :class:`gcn_max_cut_amd.hip.HipExtensionError`.  How an epoch's steps are launched (``FusedTrainer``, ``Launch``,
``launch_path``: re-exported here) is not reference API and lives in :mod:`gcn_max_cut_amd.trainer`.

Deliberately kept quirks: the features are the padded adjacency (Q1),
the loss pads to a hard-coded 1000 (Q2), the "best" state aliases the live parameters
(Q4), one Adam step per graph in dataset order (Q5), early-stop bookkeeping (Q8), save
names (Q9).  Extension (keyword-only / environment, default off): ``graphs_per_step`` > 1
switches to batched steps (one Adam step per batch of graphs, summed loss), and when
``torch.distributed`` is initialised each rank trains on its shard of every batch with one
RCCL all-reduce of the flat gradient per step.  ``loss="expected_cut"`` (or GCN_MAXCUT_LOSS=expected_cut) trains on
the relaxed loss - ``compute_loss`` of ``override_fixed_nodes(P)`` without the one-hot step, the expected cut of
independent rounding - instead of the reference's hard one; :func:`cut_loss` is either loss as a differentiable op.
``layer1="attention"`` (or GCN_MAXCUT_LAYER1=attention) builds a :class:`GATSoftmax`: the first layer is single-head graph
attention on the hand-written kernels of ``csrc/attention.hip`` instead of ``GraphConv(norm='both')``.
"""
from __future__ import annotations

import random  # noqa: F401  (reference namespace)
from dataclasses import dataclass
from itertools import chain, permutations
from time import time
from typing import Callable, Dict, List, Optional, Tuple  # noqa: F401

import numpy as np  # noqa: F401  (reference namespace)
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F  # noqa: F401

from .. import hip
from ..commons import open_file, save_object  # noqa: F401
from ..engine import PARAM_ORDER, FusedEngine, device_cut_loss, dp_active, shard_by_weight, shard_for_rank  # noqa: F401
from ..engine import InstanceEngine, check_instance_sizes, module_of
from ..graph import GraphBatch, GraphHandle
from ..trainer import FusedTrainer, Launch, _graphs_per_step, launch_path  # noqa: F401  (the launch machinery)

TORCH_DEVICE = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
TORCH_DTYPE = torch.float32
_LOSS_PAD = 1000  # TrainingNeural.py:171


@dataclass
class TrainingConfig:
    """Configuration class for training parameters (TrainingNeural.py:36-67)."""
    n_nodes: int = 1000
    dim_embedding: Optional[int] = None
    hidden_dim: Optional[int] = None
    dropout: float = 0.0
    number_classes: int = 3
    learning_rate: float = 0.001
    number_epochs: int = 1000
    tolerance: float = 1e-4
    patience: int = 20
    prob_threshold: float = 0.5
    A: float = 0.0
    C: float = 1.0
    penalty: float = 1000.0
    save_directory: Optional[str] = None
    save_frequency: int = 100

    def __post_init__(self):
        if self.dim_embedding is None:
            self.dim_embedding = self.n_nodes
        if self.hidden_dim is None:
            self.hidden_dim = self.dim_embedding // 2


# --------------------------------------------------------------------------- model
class GraphConv(nn.Module):
    """Parameter container with DGL ``GraphConv``'s layout and init (weight ``[in,out]``,
    xavier-uniform; bias zeros).  The arithmetic lives in the HIP library."""

    def __init__(self, in_feats: int, out_feats: int):
        super().__init__()
        self._in_feats, self._out_feats = in_feats, out_feats
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = nn.Parameter(torch.empty(out_feats))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        nn.init.zeros_(self.bias)

    def extra_repr(self):
        return f"in={self._in_feats}, out={self._out_feats}, normalization=both"


class _GCNForward(torch.autograd.Function):
    """softmax(conv2(relu(conv1(X)))) with a HIP backward, for callers that build their own loss from the
    probabilities (the reference's override/one-hot/compute_loss chain).  ``X`` None: the features are the padded
    adjacency (``net(g, a_pad)``).  Otherwise node features that are not (learned embeddings: ``net(g, embed.weight)``):
    the backward returns dX as well, and the three dense products of layer 1 (X @ W1, X^T @ U, U @ W1^T) run in the
    library's fp32 MFMA GEMM."""

    @staticmethod
    def forward(ctx, net, batch, X, *params):
        eng = net.engine()
        ctx.net, ctx.batch = net, batch
        ctx.dropout = eng.dropout_state()    # (p, seed) this forward runs with: the backward needs the same
        if X is None:
            ctx.ws = torch.empty(eng.workspace_bytes(batch, True), dtype=torch.uint8, device=eng.device)
            P, _, _ = eng.forward(batch, ws=ctx.ws)
            ctx.save_for_backward(P)
        else:
            ctx.ws = torch.empty(eng.workspace_bytes_features(batch, True), dtype=torch.uint8, device=eng.device)
            Xd = eng.pad_features(batch, X)      # (padded once when N % 4 != 0: the backward reads the same tensor)
            P, _, _ = eng.forward_features(batch, Xd, ws=ctx.ws)
            ctx.like = (X.device, X.dtype)
            ctx.save_for_backward(P, Xd)
        return P

    @staticmethod
    def backward(ctx, gp):
        P, *X = ctx.saved_tensors
        eng = ctx.net.engine()
        with eng.dropout(*ctx.dropout):
            if not X:
                g = eng.backward_from_gp(ctx.batch, P, gp.to(torch.float32), ws=ctx.ws)
                return (None, None, None) + tuple(g[k].clone() for k in PARAM_ORDER)
            # needs_input_grad: (net, batch, X, W1, b1, W2, b2).  GCNSoftmax.forward hands features over only when they
            # require grad, so through net(g, X) the dX GEMM always runs; want_dx = False is reached by callers of the
            # Function or of the engine whose features are constant
            g, dX = eng.backward_features_from_gp(ctx.batch, X[0], P, gp, ws=ctx.ws, want_dx=ctx.needs_input_grad[2])
            grads = tuple(g[k].clone() if need else None for k, need in zip(PARAM_ORDER, ctx.needs_input_grad[3:]))
            return (None, None, None if dX is None else dX.to(*ctx.like)) + grads


class GCNSoftmax(nn.Module):
    """Graph Convolutional Network with softmax output (TrainingNeural.py:69-85)."""

    def __init__(self, in_feats: int, hidden_size: int, num_classes: int, dropout: float, device):
        super().__init__()
        self.dropout_frac = dropout
        self.conv1 = GraphConv(in_feats, hidden_size).to(device)
        self.conv2 = GraphConv(hidden_size, num_classes).to(device)
        self._engine: Optional[FusedEngine] = None

    def engine(self) -> FusedEngine:
        """The fused engine owning this model's parameters (created on first use)."""
        if self._engine is None:
            w1, w2 = self.conv1.weight, self.conv2.weight
            self._engine = FusedEngine(w1.shape[0], w1.shape[1], w2.shape[1], hip.require_gpu(), kway=w2.shape[1] != 3)
        if not self._engine.owns(self):
            self._engine.adopt(self)
        return self._engine

    def forward(self, g, inputs):
        eng = self.engine()
        try:
            batch = graph_batch_of(g, inputs, eng.device)
        except NotImplementedError:
            return self._forward_dense_features(g, inputs)
        params = [dict(self.named_parameters())[k] for k in PARAM_ORDER]
        if eng.kway and torch.is_grad_enabled() and any(p.requires_grad for p in params):
            raise NotImplementedError(
                f"autograd through net(g, X) is implemented for number_classes = 3 only (this model has number_classes = "
                f"{eng.K}): train it with train_model / train_single_epoch, and call the model under torch.no_grad() "
                "for its probabilities")
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            eng._small_only(batch, "autograd through net(g, X)")
        # F.dropout(h, p=self.dropout_frac, training=self.training) (:82): a fresh mask per call in train mode;
        # the engine's dropout is 0 outside of such a call (evaluate_model, decode, the trainer's own steps)
        with eng.dropout(self.dropout_frac if self.training else 0.0):
            if torch.is_grad_enabled() and any(p.requires_grad for p in params):
                return _GCNForward.apply(self, batch, None, *params)
            P, _, _ = eng.forward(batch)
            return P

    def _forward_dense_features(self, g, inputs):
        """``net(g, X)`` for features with non-zeros off the graph's edges: inference when no gradient is asked
        for, the differentiable path when ``X`` requires grad (``embed.weight``); F.dropout applies in train mode."""
        eng = self.engine()
        params = [dict(self.named_parameters())[k] for k in PARAM_ORDER]
        differentiable = torch.is_grad_enabled() and inputs.requires_grad
        if torch.is_grad_enabled() and not inputs.requires_grad and any(p.requires_grad for p in params):
            raise NotImplementedError(
                "gradients with CONSTANT features are implemented for the reference's usage net(g, padded_adjacency) "
                "(TrainingNeural.py:373) only: call under torch.no_grad() for arbitrary constant features; features "
                "that require grad (learned embeddings, e.g. embed.weight) take the differentiable dense path")
        with eng.dropout(self.dropout_frac if self.training else 0.0):
            if differentiable:
                return _GCNForward.apply(self, _dense_batch_of(g, eng.device), inputs, *params)
            return _dense_forward(self, g, inputs)


class GATConv(nn.Module):
    """Parameter container of the attention first layer: ``weight`` [in,out] and ``bias`` as :class:`GraphConv`, plus the
    two attention vectors ``attn_src`` / ``attn_dst`` [out], each initialised xavier-uniform as an [out, 1] matrix from
    torch's generator.  The arithmetic lives in the HIP library (include/gcnmaxcut.h, gmc_att_*)."""

    def __init__(self, in_feats: int, out_feats: int):
        super().__init__()
        self._in_feats, self._out_feats = in_feats, out_feats
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = nn.Parameter(torch.empty(out_feats))
        self.attn_src = nn.Parameter(torch.empty(out_feats))
        self.attn_dst = nn.Parameter(torch.empty(out_feats))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        nn.init.zeros_(self.bias)
        for a in (self.attn_src, self.attn_dst):
            nn.init.xavier_uniform_(a.data.view(-1, 1))

    def extra_repr(self):
        return f"in={self._in_feats}, out={self._out_feats}, heads=1, self_loops=True, negative_slope={hip.ATTENTION_SLOPE}"


class GATSoftmax(GCNSoftmax):
    """:class:`GCNSoftmax` whose first layer is single-head graph attention on the graph with self-loops added, followed
    by relu (``layer1="attention"``; include/gcnmaxcut.h states the model).  Same constructor; three classes.  It trains
    through train_model / train_single_epoch (both losses) and answers ``net(g, a_pad)`` under ``torch.no_grad()``;
    dropout, dense features and autograd through ``net(g, X)`` are implemented for ``layer1="graphconv"`` only."""

    def __init__(self, in_feats: int, hidden_size: int, num_classes: int, dropout: float, device):
        super().__init__(in_feats, hidden_size, num_classes, dropout, device)
        self.conv1 = GATConv(in_feats, hidden_size).to(device)

    def engine(self) -> FusedEngine:
        if self._engine is None:
            w1, w2 = self.conv1.weight, self.conv2.weight
            self._engine = FusedEngine(w1.shape[0], w1.shape[1], w2.shape[1], hip.require_gpu(), attention=True)
        if not self._engine.owns(self):
            self._engine.adopt(self)
        return self._engine

    def forward(self, g, inputs):
        eng = self.engine()
        try:
            batch = graph_batch_of(g, inputs, eng.device)
        except NotImplementedError:
            raise NotImplementedError("dense node features are implemented for layer1 = 'graphconv' only (this model has "
                                      "layer1 = 'attention': its features are the padded adjacency)") from None
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(
                "autograd through net(g, X) is implemented for layer1 = 'graphconv' only (this model has layer1 = "
                "'attention'): train it with train_model / train_single_epoch, and call the model under torch.no_grad() "
                "for its probabilities")
        if self.training and self.dropout_frac > 0.0:
            raise NotImplementedError("dropout is implemented for layer1 = 'graphconv' only (this model has layer1 = "
                                      "'attention'): use dropout = 0")
        P, _, _ = eng.forward(batch)
        return P


def layer1_of(net) -> str:
    """``"attention"`` for a :class:`GATSoftmax`, else ``"graphconv"``."""
    return "attention" if isinstance(net, GATSoftmax) else "graphconv"


def _cached_batch(g: GraphHandle, key: tuple, vals, device) -> GraphBatch:
    """The single-graph device batch of ``g`` with edge values ``vals``, built once per ``key`` and kept on the handle."""
    if not isinstance(g, GraphHandle):
        raise TypeError(f"expected a GraphHandle (made by process_graphs_from_folder), got {type(g)}")
    b = g._cache.get(key)
    if b is None:
        b = g._cache[key] = GraphBatch([g], [vals], device)
    return b


def _dense_batch_of(g: GraphHandle, device) -> GraphBatch:
    """Single-graph device batch for features that are not the padded adjacency: the structure alone (layer 1 ignores
    edge values with such features, and the probabilities never read them)."""
    return _cached_batch(g, ("dense_batch", str(device)), None, device)


def _dense_forward(net: "GCNSoftmax", g: GraphHandle, inputs: torch.Tensor) -> torch.Tensor:
    """``net(g, X)`` for features that are NOT the padded adjacency (non-zeros off the edges), without a gradient:
    ``gmc_forward_features`` - the layer-1 feature transform is a genuine dense GEMM on the library's own fp32 MFMA
    kernel, everything after it the one-kernel-per-operation sequence.  The same entry point is the forward of the
    differentiable path (:class:`_GCNForward`); the engine's dropout setting applies."""
    eng = net.engine()
    P, _, _ = eng.forward_features(_dense_batch_of(g, eng.device), inputs)
    return P


def graph_batch_of(g: GraphHandle, inputs, device) -> GraphBatch:
    """Single-graph device batch for ``net(g, inputs)``, cached on the handle."""
    if not isinstance(g, GraphHandle):
        raise TypeError(f"expected a GraphHandle (made by process_graphs_from_folder), got {type(g)}")
    vals = g.edge_values(inputs)
    return _cached_batch(g, ("batch", None if vals is None else id(vals), str(device)), vals, device)


# --------------------------------------------------------------------------- the loss on the device
class _CutLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, batch, C, loss):
        losses, GP = device_cut_loss(batch, P, C, loss)
        ctx.save_for_backward(GP)
        ctx.like = (P.device, P.dtype)
        return losses.sum().to(*ctx.like)

    @staticmethod
    def backward(ctx, grad_out):
        (GP,) = ctx.saved_tensors
        return (grad_out.to(GP.device, GP.dtype) * GP).to(*ctx.like), None, None, None


def cut_loss(g, P, C: float = 1.0, relaxed: bool = False):
    """The scalar loss of probabilities ``P`` [n,3] on graph ``g`` (a GraphHandle with its own edge weights, or a
    GraphBatch with ``P`` [R,3]: then the sum over its graphs), computed and differentiated on the device in O(edges)
    (``gmc_cut_loss_f32``).  With ``A_pad`` the graph's padded adjacency it equals, in value and in ``dLoss/dP``,

    * ``relaxed=False``: ``compute_loss(apply_max_to_one_hot(override_fixed_nodes(P)), A_pad, C=C)`` - the reference's
      hard loss, ``-C * cut`` of the argmax decode with the straight-through gradient ``C * A_val @ onehot(S)``;
    * ``relaxed=True``: ``compute_loss(override_fixed_nodes(P), A_pad, C=C)`` - the expected cut under independent
      rounding, ``-C/2 * sum_uv w_uv (1 - Pt_u . Pt_v)`` with gradient ``C * A_val @ Pt``.

    Forward keeps ``GP = dLoss/dP``; backward returns ``grad_out * GP``.  So
    ``cut_loss(g, net(g, embed.weight), relaxed=True).backward()`` trains through the HIP forward and backward."""
    if P.dim() != 2 or P.shape[1] != 3:
        raise ValueError(f"cut_loss takes probabilities of number_classes = 3 columns, got {tuple(P.shape)}: a model with "
                         "another number_classes computes its loss inside train_model / evaluate_model")
    dev = hip.require_gpu()
    batch = g if isinstance(g, GraphBatch) else graph_batch_of(g, None, dev)
    if batch.B and batch.n_max > hip.MAX_GRAPH_NODES:
        raise ValueError(f"cut_loss is implemented for graphs of up to {hip.MAX_GRAPH_NODES} nodes, got one with "
                         f"{batch.n_max}: a larger graph trains through train_model and gets its loss and its argmax "
                         "partition from evaluate_model / simple_partition_assignment on net(g, None)")
    return _CutLoss.apply(P, batch, float(C), "expected_cut" if relaxed else "cut")


# --------------------------------------------------------------------------- loss helpers (torch ops)
def override_fixed_nodes(h):
    """Rows 0..K-1 <- e_0..e_{K-1} with straight-through gradient, K = the number of columns (TrainingNeural.py:87-94,
    where K is 3: rows 0,1,2 <- e0,e1,e2)."""
    k = min(h.shape[1], h.shape[0])
    eye = torch.eye(h.shape[1], dtype=h.dtype, device=h.device)[:k]
    head = eye + h[:k] - h[:k].detach()
    return torch.cat([head, h[k:].clone()], dim=0)


def max_to_one_hot(tensor):
    """One-hot of the first maximum, straight-through (TrainingNeural.py:96-102)."""
    hot = torch.zeros_like(tensor)
    hot[torch.argmax(tensor)] = 1.0
    return hot + tensor - tensor.detach()


def apply_max_to_one_hot(output):
    """Row-wise :func:`max_to_one_hot` without the Python loop (TrainingNeural.py:104-106)."""
    hot = F.one_hot(torch.argmax(output, dim=1), output.shape[1]).to(output.dtype)
    return hot + output - output.detach()


def extend_matrix_torch_training(matrix, N):
    size = matrix.shape[0]
    if N <= size:
        return matrix
    out = torch.zeros((N, N), dtype=matrix.dtype, device=matrix.device)
    out[:size, :size] = matrix
    return out


def extend_matrix_torch(matrix, N, torch_dtype=None, torch_device=None):
    """[n,n] -> [n,N] zero-padded (TrainingNeural.py:137-152)."""
    size = matrix.shape[0]
    if N < size:
        raise ValueError("N should be greater than or equal to the original matrix size.")
    out = torch.zeros(size, N, device=matrix.device)  # default dtype whatever the input's (as the reference)
    out[:size, :size] = matrix
    if torch_dtype is not None:
        out = out.type(torch_dtype)
    if torch_device is not None:
        out = out.to(torch_device)
    return out


def calculate_HC_vectorized(s, adjacency_matrix):
    """Total weight of cut edges, ``sum(A * (1 - pad(S S^T, 1000))) / 2`` (TrainingNeural.py:154-176)."""
    same = extend_matrix_torch(s @ s.T, _LOSS_PAD)
    return torch.sum(adjacency_matrix * (1 - same)) / 2


def compute_loss(s, adjacency_matrix, A: float = 0, C: float = 1, penalty: float = 1000):
    """``C * (-cut)``; ``A`` and ``penalty`` are accepted and unused (TrainingNeural.py:291-309)."""
    return C * (-1 * calculate_HC_vectorized(s, adjacency_matrix))


def terminal_independence_penalty(s, terminal_nodes: List[int]):
    total = 0
    for i, a in enumerate(terminal_nodes):
        for b in terminal_nodes[i + 1:]:
            total = total + torch.dot(s[a], s[b])
    return total


def find_ac_parameters(graph):
    top = max(dict(graph.degree()).values())
    return top + 1, top / 2


def generate_terminal_permutations(terminal_dict: Dict):
    keys = list(terminal_dict.keys())
    return [dict(zip(keys, perm)) for perm in permutations(terminal_dict.values())]


def calculate_all_cut_legacy(q_torch, s):
    if len(s) == 0:
        return 0
    total = 0
    for k in range(s.shape[1]):
        col = s[:, k].unsqueeze(0)
        total = total + (q_torch * (col != col.t()).float()).sum() / 2
    return total / 2


def evaluate_optimal_partitioning(net, dgl_graph, inputs, adjacency_matrix, terminal_dict: Dict):
    """TrainingNeural.py:253-289 (the permutations are generated but, as in the reference,
    never handed to the model)."""
    net.eval()
    best = float('inf')
    if dgl_graph.number_of_nodes() < 30:
        inputs = torch.ones((dgl_graph.number_of_nodes(), 30))
    with torch.no_grad():
        for _perm in generate_terminal_permutations(terminal_dict):
            probs = override_fixed_nodes(net(dgl_graph, inputs))
            value = calculate_all_cut_legacy(adjacency_matrix, (probs >= 0.5).float())
            if value < best:
                best = value
    return best


# --------------------------------------------------------------------------- training
def setup_model_and_optimizer(config: TrainingConfig, *, layer1: Optional[str] = None):
    """(model, embedding, optimizer) - TrainingNeural.py:311-339.  The embedding is never
    used by the forward (Q1) but is part of the optimizer, the checkpoint and the return
    value, as in the reference.  ``layer1``: ``"graphconv"`` (the reference's model), ``"attention"`` (a
    :class:`GATSoftmax`) or None = the environment's GCN_MAXCUT_LAYER1 (default graphconv)."""
    model_class = GATSoftmax if hip.layer1_name(layer1) == "attention" else GCNSoftmax
    if model_class is GATSoftmax and config.number_classes != 3:
        raise ValueError(f"number_classes = {config.number_classes}: layer1 = 'attention' is implemented for the 3-class "
                         "model only")
    net = model_class(config.dim_embedding, config.hidden_dim, config.number_classes,
                      config.dropout, TORCH_DEVICE)
    net = net.type(TORCH_DTYPE).to(TORCH_DEVICE)
    embed = nn.Embedding(config.n_nodes, config.dim_embedding).type(TORCH_DTYPE).to(TORCH_DEVICE)
    optimizer = torch.optim.Adam(chain(net.parameters(), embed.parameters()), lr=config.learning_rate)
    return net, embed, optimizer


def _setup(config: TrainingConfig, layer1: str):
    """:func:`setup_model_and_optimizer` for a RESOLVED ``layer1`` (a name, never None).  The keyword is left out only when
    it says what the function would choose by itself - the environment's value included - so that stand-ins of the function
    without the keyword keep working and an explicit ``"graphconv"``, or a checkpoint's own keys, beat
    GCN_MAXCUT_LAYER1=attention."""
    if layer1 == hip.layer1_name(None):
        return setup_model_and_optimizer(config)
    return setup_model_and_optimizer(config, layer1=layer1)


def _trainer_for(net, optimizer, config, graphs_per_step: Optional[int] = None,
                 loss: Optional[str] = None) -> FusedTrainer:
    gps = _graphs_per_step(graphs_per_step)
    loss = hip.loss_name(loss)   # (None: GCN_MAXCUT_LOSS, default "cut"; a bad name raises ValueError)
    tr = getattr(net, "_fused_trainer", None)
    if tr is None or tr.optimizer is not optimizer or tr.graphs_per_step != gps or tr.loss != loss:
        tr = FusedTrainer(net, optimizer, config, gps, loss=loss)
        net._fused_trainer = tr
    tr.config = config
    return tr


def train_single_epoch(dataset: Dict, net, optimizer, embed, config: TrainingConfig,
                       dataset_files: Optional[List[str]] = None, *,
                       graphs_per_step: Optional[int] = None, loss: Optional[str] = None,
                       layer1: Optional[str] = None) -> float:
    """One epoch, cumulative loss (TrainingNeural.py:341-390).  The device batches planned for ``dataset`` are
    kept from epoch to epoch while it looks unchanged (:meth:`FusedTrainer.prepare` says how that is decided);
    after editing a large dataset dict in place call ``net._fused_trainer.invalidate()``.  ``loss``: ``"cut"`` (the
    reference's), ``"expected_cut"`` (the relaxed loss) or None = the environment's GCN_MAXCUT_LOSS (default cut).
    ``layer1``: when given, the first layer ``net`` must have (the model itself was built by
    :func:`setup_model_and_optimizer`): another one is a ValueError."""
    if layer1 is not None and hip.layer1_name(layer1) != layer1_of(net):
        raise ValueError(f"layer1 = {layer1!r}, but the model was built with layer1 = {layer1_of(net)!r} "
                         "(setup_model_and_optimizer(config, layer1=...))")
    net.train()
    trainer = _trainer_for(net, optimizer, config, graphs_per_step, loss)
    if dataset_files is None:
        dataset_files = ['./nx_test_generated_graph_n200_300_d8_12_t500.pkl']
    cumulative_loss = 0.0
    for dataset_file in dataset_files:
        current = dataset if isinstance(dataset, dict) else open_file(dataset_file)
        cumulative_loss += trainer.epoch(current)
    return cumulative_loss


def _rank0() -> bool:
    """Data-parallel runs: every rank holds the same model, rank 0 alone prints and writes checkpoints
    (N processes writing ./epoch_*.pth at once would race on the same files)."""
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


def _checkpoint(net, optimizer, embed, epoch, loss_history, config) -> Dict:
    tr = getattr(net, "_fused_trainer", None)
    if tr is not None:
        tr.sync_optimizer_state()
    return {'epoch': epoch, 'model': net.state_dict(), 'optimizer': optimizer.state_dict(),
            'loss_history': loss_history, 'inputs': embed.weight, 'config': config}


def train_model(dataset: Dict, config: TrainingConfig, dataset_files: Optional[List[str]] = None, *,
                graphs_per_step: Optional[int] = None, loss: Optional[str] = None, layer1: Optional[str] = None) -> Tuple:
    """Main training function (TrainingNeural.py:392-484):
    returns ``(model, best_loss, final_epoch, embedding_weights, loss_history)``.  ``loss``: as for
    :func:`train_single_epoch`; ``layer1``: as for :func:`setup_model_and_optimizer`."""
    loss = hip.loss_name(loss)
    layer1 = hip.layer1_name(layer1)
    say = print if _rank0() else (lambda *a, **k: None)
    say(f"Starting training with {config.number_epochs} epochs")
    say(f"Model: {config.n_nodes} nodes, {config.number_classes} classes")
    say(f"Device: {TORCH_DEVICE}")

    net, embed, optimizer = _setup(config, layer1)
    best_loss, best_model_state = float('inf'), None
    loss_history: List[float] = []
    patience_counter, prev_loss = 0, float('inf')
    start_time = time()
    epoch = -1

    for epoch in range(config.number_epochs):
        cumulative_loss = train_single_epoch(dataset, net, optimizer, embed, config, dataset_files,
                                             graphs_per_step=graphs_per_step, loss=loss)
        loss_history.append(cumulative_loss)

        stalled = cumulative_loss > prev_loss or abs(prev_loss - cumulative_loss) <= config.tolerance
        if epoch > 0 and stalled:
            patience_counter += 1
            if patience_counter >= config.patience:
                say(f'Early stopping at epoch {epoch}')
                break
        else:
            patience_counter = 0

        if cumulative_loss < best_loss:
            best_loss = cumulative_loss
            best_model_state = net.state_dict()  # aliases the live parameters (Q4)
        prev_loss = cumulative_loss

        if epoch % config.save_frequency == 0:
            say(f'Epoch: {epoch}, Cumulative Loss: {cumulative_loss:.6f}')
            if config.save_directory and _rank0():
                torch.save(_checkpoint(net, optimizer, embed, epoch, loss_history, config),
                           f'./epoch_{epoch}_loss_{cumulative_loss:.4f}_{config.save_directory}')

    if best_model_state is not None:
        net.load_state_dict(best_model_state)

    say(f'Training completed in {time() - start_time:.2f} seconds')
    say(f'Best loss: {best_loss:.6f}')

    if config.save_directory and _rank0():
        final_filename = f'./final_{config.save_directory}'
        torch.save(_checkpoint(net, optimizer, embed, epoch, loss_history, config), final_filename)
        say(f'Final model saved to {final_filename}')

    return net, best_loss, epoch, embed.weight, loss_history


def instance_chunks(sizes: List[int], max_rows_per_chunk: int) -> List[range]:
    """Consecutive runs of a dataset's graphs with at most ``max_rows_per_chunk`` nodes each (a graph larger than that is
    a chunk of its own), in dataset order."""
    if max_rows_per_chunk < 1:
        raise ValueError(f"max_rows_per_chunk must be positive, got {max_rows_per_chunk}")
    chunks, start, rows = [], 0, 0
    for i, n in enumerate(sizes):
        if i > start and rows + n > max_rows_per_chunk:
            chunks.append(range(start, i))
            start, rows = i, 0
        rows += n
    if len(sizes) > start:
        chunks.append(range(start, len(sizes)))
    return chunks


def _solve_chunk_early_stopping(part: List, eng, config: TrainingConfig, loss: str, check_every: int,
                                compact_fraction: float) -> List[Dict]:
    """One chunk of :func:`solve_dataset` with per-graph early stopping: the results of ``part``'s graphs, in order."""
    from ..Testing.TestingNeuralNetwork import calculate_cut_value
    epochs = max(int(config.number_epochs), 0)
    alive = list(range(len(part)))            # positions in `part` of the engine's graphs, in batch order
    results: List[Optional[Dict]] = [None] * len(part)
    history = torch.empty((epochs, eng.B), dtype=torch.float32, device=eng.device)

    def archive(which: List[int], stop: Optional[torch.Tensor], ran: int) -> None:
        """Results of the engine's graphs ``which`` (batch positions) after ``ran`` epochs.  A stopped graph's state has
        not moved since its stop, so what is read here is what the stop left, whenever that was."""
        if not which:
            return
        P, _S, _l = eng.forward(config.C, loss=loss)
        P, hist = P.cpu(), history[:ran].cpu()
        best_S, best_loss, best_epoch = eng.best_S.cpu(), eng.best_loss.cpu(), eng.best_epoch.cpu()
        stop = eng.stopped() if stop is None else stop
        parameters = eng.parameters()
        goff = [0]
        for i in alive:
            goff.append(goff[-1] + part[i][0].n)
        for g in which:
            _handle, _a_pad, nx_graph, _terminals = part[alive[g]]
            stopped_epoch = int(stop[g]) if int(stop[g]) >= 0 else None
            kept = ran if stopped_epoch is None else stopped_epoch + 1
            partition = [int(x) for x in best_S[goff[g]:goff[g + 1]]]
            params = parameters[g]
            results[alive[g]] = {
                'best_loss': float(best_loss[g]), 'best_epoch': int(best_epoch[g]), 'partition': partition,
                'cut': calculate_cut_value(partition, nx_graph),
                'probabilities': P[goff[g]:goff[g + 1]].clone(),
                'loss_history': [float(x) for x in hist[:kept, g]],
                'model': (lambda params=params: module_of(params)),
                'stopped_epoch': stopped_epoch,
            }

    epoch = 0
    while epoch < epochs:
        _P, S, losses = eng.train_fwd_bwd(config.C, loss=loss)
        eng.adam_step(config.learning_rate, running_only=True)
        eng.early_stop(S, losses, epoch, config.tolerance, config.patience)
        history[epoch].copy_(losses)
        epoch += 1
        if check_every and epoch % check_every == 0 and epoch < epochs:
            stop = eng.stopped()
            done = [g for g in range(len(alive)) if int(stop[g]) >= 0]
            if len(done) == len(alive):
                break
            rows = [part[i][0].n for i in alive]
            if done and sum(rows[g] for g in done) >= compact_fraction * sum(rows):
                archive(done, stop, epoch)
                running = [g for g in range(len(alive)) if int(stop[g]) < 0]
                eng = eng.subset(running)
                history = history[:, running].contiguous()
                alive = [alive[g] for g in running]
    archive(list(range(len(alive))), None, epoch)
    return results


def solve_dataset(dataset: Dict, config: TrainingConfig, *, loss: Optional[str] = None,
                  max_rows_per_chunk: int = 1 << 18, early_stopping: bool = False, check_every: int = 64,
                  compact_fraction: float = 0.25, terminals: bool = True) -> List[Dict]:
    """Give every graph of ``dataset`` (the reference's items) ITS OWN model and train them all at once: the reference's
    architecture as the instance-wise solver it is - ``conv1.weight[i]`` is the embedding of node id i, which means
    something on the graph it was trained on only.  Graph g gets a ``GCNSoftmax(n_g, hidden_dim, number_classes)``,
    initialised as the reference initialises a model of ``n_nodes = n_g`` (graph by graph in dataset order from torch's
    generator); one launch sequence per step trains a whole chunk of them (:class:`gcn_max_cut_amd.engine.InstanceEngine`,
    gmc_inst_*), and nothing couples two graphs.

    ``config.number_classes`` (2..8), ``hidden_dim`` (ONE width for the call), ``learning_rate``, ``number_epochs`` and
    ``C`` are honoured; ``loss`` as for :func:`train_single_epoch`.  The dataset is cut into chunks of at most
    ``max_rows_per_chunk`` nodes, solved one after the other; every chunk runs ``number_epochs`` steps of
    train_fwd_bwd -> Adam -> keep_best.  By default there is no per-graph early stopping: ``tolerance`` and ``patience``
    are ignored (a graph that has converged costs its share of every later step).

    ``early_stopping=True`` stops every graph on its own by the reference's rule (``train_model``'s: the loss has stalled
    - risen, or moved by at most ``config.tolerance`` - ``config.patience`` epochs in a row; include/gcnmaxcut.h,
    gmc_inst_early_stop_f32), decided on the GPU.  A stopped graph is frozen at once: no Adam update, no keep-best, no
    state change (it still rides through the training launches).  Every ``check_every`` epochs (0: never) the host reads
    which graphs have stopped: when all have, the chunk ends; when the stopped ones hold at least ``compact_fraction`` of
    the current batch's nodes, their results are archived and the loop goes on with an engine over the running graphs
    alone (:meth:`InstanceEngine.subset`), so the number of rebuilds is logarithmic in the batch.  ``check_every = 64`` is
    a measured choice on ONE workload (faster than 16 and than 1 on every batch measured, because a
    rebuild costs about a millisecond per graph kept on the host); ``compact_fraction = 0.25`` is a provisional starting
    point, not a measured choice - 0.5 was faster where every graph stops early, and the fraction exists for batches in
    which some graphs run to the end, which were not measured.  No result depends on ``check_every``,
    ``compact_fraction`` or ``max_rows_per_chunk``, byte for byte.

    Returns one dict per graph, in dataset order: ``best_loss`` / ``best_epoch`` (the lowest loss of the graph over the
    epochs - measured before that epoch's update - and the first epoch that reached it), ``partition`` (the decode of
    that epoch, nodes 0..K-1 in classes 0..K-1), ``cut`` (``calculate_cut_value`` of it), ``probabilities`` (the LAST
    epoch's P [n_g, K], a CPU tensor), ``loss_history`` (the graph's loss per epoch) and ``model``: a zero-argument
    callable returning a ``GCNSoftmax`` with the graph's parameters after the last step (as train_model's "best" state
    aliases the live parameters), for ``evaluate_model``, ``round_dataset``, ``search_dataset`` and
    ``sampling_optimization`` on that graph.  With ``early_stopping=True``: ``loss_history`` ends at the stop epoch,
    inclusive (``stopped_epoch + 1`` entries; ``number_epochs`` for a graph that ran to the end), ``model`` holds the
    parameters as the stop left them (the update of the stop epoch applied, as in the reference), ``probabilities`` is
    the forward of exactly those parameters, the best comes from the epochs before the stop epoch, and a last key
    ``stopped_epoch`` (``None``: the graph ran to the end) is appended.

    ``terminals=False`` solves plain max-K-cut: no node is fixed - the head overrides no row, ``partition`` is the row
    argmax of the best epoch, both losses count every edge by its endpoints' own rows - and a graph needs one node,
    not number_classes.  Early stopping, chunking and every key work as with terminals.

    Refused: ``dropout > 0`` and ``layer1 = "attention"`` (NotImplementedError), a graph beyond the one-workgroup head
    (ValueError: ``train_model`` serves one large graph), a graph with fewer than number_classes nodes (ValueError;
    with terminals)."""
    from ..Testing.TestingNeuralNetwork import calculate_cut_value
    loss = hip.loss_name(loss)
    if config.dropout > 0:
        raise NotImplementedError(f"dropout = {config.dropout}: solve_dataset trains without dropout (the per-graph "
                                  "models run the K-class row-kernel sequence)")
    if hip.layer1_name(None) == "attention":
        raise NotImplementedError("layer1 = 'attention' (GCN_MAXCUT_LAYER1): solve_dataset is implemented for layer1 = "
                                  "'graphconv' only")
    K, F = int(config.number_classes), int(config.hidden_dim)
    items = list(dataset.values())
    sizes = [it[0].n for it in items]
    check_instance_sizes(sizes, K, loss, terminals=bool(terminals))
    if early_stopping and (check_every < 0 or not 0.0 <= compact_fraction <= 1.0):
        raise ValueError(f"check_every must be >= 0 and compact_fraction within 0..1, got {check_every}, {compact_fraction}")
    results: List[Dict] = []
    for chunk in instance_chunks(sizes, max_rows_per_chunk):
        part = [items[i] for i in chunk]
        handles = [it[0] for it in part]
        # (the keyword is passed only when it differs from the engine's default: an engine class put in this one's
        # place, as the host tests do, need not know it)
        plain = {} if terminals else {"terminals": False}
        eng = InstanceEngine(handles, F, K, values=[h.edge_values(it[1]) for h, it in zip(handles, part)], **plain)
        eng.reset_parameters()
        if early_stopping:
            results.extend(_solve_chunk_early_stopping(part, eng, config, loss, int(check_every), float(compact_fraction)))
            continue
        history = torch.empty((max(config.number_epochs, 0), eng.B), dtype=torch.float32, device=eng.device)
        P = None
        for epoch in range(config.number_epochs):
            P, S, losses = eng.train_fwd_bwd(config.C, loss=loss)
            eng.adam_step(config.learning_rate)
            eng.keep_best(S, losses, epoch)
            history[epoch].copy_(losses)
        history = history.cpu()
        best_S, best_loss, best_epoch = eng.best_S.cpu(), eng.best_loss.cpu(), eng.best_epoch.cpu()
        P = None if P is None else P.cpu()
        parameters = eng.parameters()
        goff = [0]
        for h in handles:
            goff.append(goff[-1] + h.n)
        for g, (_handle, _a_pad, nx_graph, _terminals) in enumerate(part):
            partition = [int(s) for s in best_S[goff[g]:goff[g + 1]]]
            params = parameters[g]
            results.append({
                'best_loss': float(best_loss[g]), 'best_epoch': int(best_epoch[g]), 'partition': partition,
                'cut': calculate_cut_value(partition, nx_graph),
                'probabilities': None if P is None else P[goff[g]:goff[g + 1]].clone(),
                'loss_history': [float(x) for x in history[:, g]],
                'model': (lambda params=params: module_of(params)),
            })
    return results


def train_from_pickle(dataset_filename: str, model_name: str, n_nodes: int = 1000, **kwargs) -> Tuple:
    """Train from a dataset pickle (TrainingNeural.py:486-513)."""
    graphs_per_step = kwargs.pop('graphs_per_step', None)
    loss = kwargs.pop('loss', None)
    layer1 = kwargs.pop('layer1', None)
    config = TrainingConfig(**{'n_nodes': n_nodes, 'save_directory': f'{model_name}.pth', **kwargs})
    print(f"Loading dataset from {dataset_filename}")
    dataset = open_file(dataset_filename)
    return train_model(dataset, config, graphs_per_step=graphs_per_step, loss=loss, layer1=layer1)


def train_multi_class(dataset_filename: str, model_name: str, num_classes: int = 3, **kwargs) -> Tuple:
    """TrainingNeural.py:515-535."""
    params = {'number_classes': num_classes, 'save_directory': f'{model_name}.pth', **kwargs}
    return train_from_pickle(dataset_filename, model_name, **params)


def evaluate_model(model, dataset: Dict, config: TrainingConfig, *, loss: Optional[str] = None) -> Dict:
    """Average / total loss over a dataset (TrainingNeural.py:537-570): forward, terminal
    override, argmax decode and cut loss for all graphs in one fused launch sequence.  ``loss``: as for
    :func:`train_single_epoch` (``"expected_cut"``: the relaxed loss of the same probabilities)."""
    loss_kw = {} if hip.loss_name(loss) == "cut" else {"loss": hip.loss_name(loss)}
    model.eval()
    items = list(dataset.values())
    if not items:
        return {'average_loss': 0, 'total_loss': 0.0, 'num_samples': 0}
    eng = model.engine()
    handles = [it[0] for it in items]
    vals = [h.edge_values(it[1]) for h, it in zip(handles, items)]
    batch = GraphBatch(handles, vals, eng.device)
    _, _, losses = eng.forward(batch, config.C, want_loss=True, **loss_kw)
    total = 0.0
    for value in losses.cpu().tolist():
        total += value
    return {'average_loss': total / len(items), 'total_loss': total, 'num_samples': len(items)}


def load_neural_model(model_path: str, config: TrainingConfig, *, layer1: Optional[str] = None):
    """(model, inputs, loaded_config) from a checkpoint (TrainingNeural.py:572-609).  A checkpoint with ``conv1.attn_src``
    among its keys loads as a :class:`GATSoftmax` without being told, any other as a :class:`GCNSoftmax`; ``layer1``
    (``"graphconv"`` / ``"attention"``) insists on one."""
    import torch.serialization
    try:
        torch.serialization.add_safe_globals([TrainingConfig])
        checkpoint = torch.load(model_path, map_location=TORCH_DEVICE)
    except Exception:
        try:
            checkpoint = torch.load(model_path, map_location=TORCH_DEVICE, weights_only=False)
        except Exception:
            with torch.serialization.safe_globals([TrainingConfig]):
                checkpoint = torch.load(model_path, map_location=TORCH_DEVICE)
    if layer1 is None:   # the checkpoint's own keys decide (not the environment: the weights are what they are)
        layer1 = "attention" if "conv1.attn_src" in checkpoint['model'] else "graphconv"
    layer1 = hip.layer1_name(layer1)
    net, embed, _ = _setup(config, layer1)
    net.load_state_dict(checkpoint['model'])
    return net, checkpoint.get('inputs', embed.weight), checkpoint.get('config', config)


def save_neural_model(model, optimizer, embed, epoch: int, loss_history: List,
                      config: TrainingConfig, model_path: str):
    """TrainingNeural.py:611-634."""
    torch.save(_checkpoint(model, optimizer, embed, epoch, loss_history, config), model_path)
    print(f'Model saved to {model_path}')


# --------------------------------------------------------------------------- legacy wrappers (:636-733)
def get_gnn_legacy(n_nodes: int, gnn_hypers: Dict, opt_params: Dict, torch_device, torch_dtype):
    return setup_model_and_optimizer(TrainingConfig(
        n_nodes=n_nodes, dim_embedding=gnn_hypers['dim_embedding'], hidden_dim=gnn_hypers['hidden_dim'],
        dropout=gnn_hypers['dropout'], number_classes=gnn_hypers['number_classes'],
        learning_rate=opt_params['lr']))


def hyperparameters_legacy(n: int = 80, d: int = 3, p=None, graph_type: str = 'reg',
                           number_epochs: int = int(1e5), learning_rate: float = 1e-4,
                           prob_threshold: float = 0.5, tol: float = 1e-4, patience: int = 100):
    dim_embedding = n
    return (n, d, p, graph_type, number_epochs, learning_rate, prob_threshold, tol, patience,
            dim_embedding, int(dim_embedding / 2))


def train_legacy_wrapper(model_name: str, filename: str = './testData/nx_generated_graph_n80_d3_t200.pkl',
                         n: int = 80):
    return train_from_pickle(filename, model_name, n_nodes=n, learning_rate=0.001, patience=20)


def train_2way_neural_legacy(model_name: str, filename: str = './testData/prepareDS.pkl'):
    return train_multi_class(filename, model_name, num_classes=2, n_nodes=4096,
                             learning_rate=0.001, patience=20, number_epochs=500)


get_gnn = get_gnn_legacy
hyperParameters = hyperparameters_legacy
train1 = train_legacy_wrapper
train_2wayNeural = train_2way_neural_legacy
FIndAC = find_ac_parameters
GetOptimalNetValue = evaluate_optimal_partitioning
calculateAllCut = calculate_all_cut_legacy
LoadNeuralModel = load_neural_model
