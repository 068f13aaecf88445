"""Fused HIP engine: forward / training step / Adam over the C-ABI library.

Holds the model's four GraphConv tensors as views of ONE flat fp32 buffer
``[W1 | b1 | W2 | b2]`` (so a single fused Adam sweep and a single RCCL all-reduce cover
them), the gradient / Adam-moment buffers of the same shape, and the scratch workspace.
All kernels are enqueued on torch's current HIP stream through ``gcnmaxcut.h``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import hip
from .graph import GraphBatch

PARAM_ORDER = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")
# the attention engine's flat buffer carries the two attention vectors of layer 1 behind the four GraphConv tensors
ATT_PARAM_ORDER = PARAM_ORDER + ("conv1.attn_src", "conv1.attn_dst")


def flat_layout(N: int, F: int, K: int, attention: bool = False) -> Tuple[List[int], int]:
    sizes = [N * F, F, F * K, K] + ([F, F] if attention else [])
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    return offs, offs[-1]


# widest hidden layer the kernels take (GMC_MAX_HIDDEN of include/gcnmaxcut.h; hidden_dim is padded to a multiple of 4)
MAX_HIDDEN = 4096


class FusedEngine:
    """One per model.  ``adopt`` re-homes a module's parameters into the flat buffer."""

    def __init__(self, N: int, F: int, K: int, device: Optional[torch.device] = None, *, kway: bool = False,
                 attention: bool = False):
        """``kway`` = True asks for the K-class engine (number_classes K in 2..8 through gmc_kway_*: the row-kernel sequence,
        ``[R,K]`` outputs, no fused step / slab / dropout / dense features).  It is required for K != 3 - a caller written
        for the 3-class engine's surface is told so instead of meeting NotImplementedError later - and allowed for K = 3,
        which then runs the same sequence.  ``GCNSoftmax.engine()`` passes it for models with number_classes != 3.

        ``attention`` = True asks for the attention engine: layer 1 is single-head graph attention (gmc_att_*: the
        row-kernel sequence of csrc/attention.hip), three classes, the flat buffer ``[W1 | b1 | W2 | b2 | a_src | a_dst]``.
        It offers forward, train_fwd_bwd and the Adam steps; the fused step, the slab copy, dropout, dense features and the
        caller-supplied dLoss/dP raise NotImplementedError naming ``layer1``.  ``GATSoftmax.engine()`` passes it."""
        self.device = device or hip.require_gpu()
        self.lib = hip.load()
        if not 2 <= K <= hip.KWAY_MAX_CLASSES:
            raise ValueError(f"number_classes must be in 2..{hip.KWAY_MAX_CLASSES}, got {K} (nodes 0..K-1 of every graph "
                             "are the terminals of classes 0..K-1)")
        if attention and (K != 3 or kway):
            raise ValueError(f"number_classes = {K}: layer1 = 'attention' is implemented for the 3-class model only "
                             "(FusedEngine(N, F, 3, attention=True))")
        if K != 3 and not kway:
            raise ValueError(f"number_classes = {K}: the fused engine is 3-class (the terminal override of "
                             "TrainingNeural.py:91-93 is 3-wide); FusedEngine(N, F, K, kway=True) is the K-class engine")
        if F < 1 or F > MAX_HIDDEN:
            raise ValueError(f"hidden_dim must be in 1..{MAX_HIDDEN} on this path (include/gcnmaxcut.h: GMC_MAX_HIDDEN), got {F}: "
                             f"TrainingConfig derives hidden_dim = n_nodes // 2 when none is given, so a model of n_nodes > "
                             f"{2 * MAX_HIDDEN + 1} needs an explicit hidden_dim")
        self.N, self.F, self.K = N, F, K
        # number_classes != 3: the K-class entry points (gmc_kway_*) - the one-kernel-per-operation row-kernel sequence
        # with [R,K] outputs.  The fused 3-way kernels, the slab copy of W1, dropout, dense features and the
        # caller-supplied dLoss/dP are 3-class only and raise NotImplementedError there.
        self.kway = bool(kway)
        # layer1 = "attention": the gmc_att_* entry points; six tensors in the flat buffer
        self.attention = bool(attention)
        self.param_order = ATT_PARAM_ORDER if self.attention else PARAM_ORDER
        # Any hidden_dim (TrainingNeural.py:42,66-67 accept any int; n_nodes=50 gives 25): the kernels work on 16-byte
        # column groups, so the flat buffer carries the hidden dimension padded to a multiple of 4 (Fp).  Pad columns of
        # W1 / entries of b1 / rows of W2 are 0 and stay 0 (their activations are relu(0), every gradient entry is an
        # exact 0, Adam of 0 is 0); the module's parameters and state_dict keep the logical shapes as views [:, :F].
        self.Fp = (F + 3) // 4 * 4
        self.offs, self.count = flat_layout(N, self.Fp, K, self.attention)
        # + 4 floats of tail: slot `count` carries the summed loss through the all-reduce
        self.flat = torch.zeros(self.count + 4, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.step_count = 0
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.device)  # device mirror of step_count
        self._dev_step = 0   # what step_dev holds (host shadow): replayed / device-stepped launches advance both
        self._ws: Optional[torch.Tensor] = None
        self._refresh_model()
        # slab copy of conv1.weight for the fused forward (gmc_model.W1_slab): used by the calls that ask for it
        # (FusedTrainer's steps), kept current by the fused Adam kernels, re-built when torch wrote the parameters
        self.w1_slab: Optional[torch.Tensor] = None
        self._slab_sig = None
        self._adopted: List = []
        self.slab_enabled = True   # False: no slab copy, the fused forward reads conv1.weight itself

    # ---- parameters
    def views(self, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The four tensors in the reference's (logical) shapes: views of ``buf`` (for hidden_dim % 4 != 0
        ``conv1.weight`` is a strided view of the padded rows).  The attention engine: six, with ``conv1.attn_src`` and
        ``conv1.attn_dst`` [F]."""
        p, F = self.padded_views(buf), self.F
        out = {"conv1.weight": p["conv1.weight"][:, :F], "conv1.bias": p["conv1.bias"][:F],
               "conv2.weight": p["conv2.weight"][:F], "conv2.bias": p["conv2.bias"]}
        if self.attention:
            out.update({k: p[k][:F] for k in ATT_PARAM_ORDER[4:]})
        return out

    def padded_views(self, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The same four tensors as the kernels see them: hidden dimension padded to Fp, contiguous."""
        buf = self.flat if buf is None else buf
        o, N, F, K = self.offs, self.N, self.Fp, self.K
        out = {"conv1.weight": buf[o[0]:o[1]].view(N, F), "conv1.bias": buf[o[1]:o[2]],
               "conv2.weight": buf[o[2]:o[3]].view(F, K), "conv2.bias": buf[o[3]:o[4]]}
        if self.attention:
            out.update({"conv1.attn_src": buf[o[4]:o[5]], "conv1.attn_dst": buf[o[5]:o[6]]})
        return out

    def _refresh_model(self) -> None:
        v = self.padded_views()
        self._model = hip.GmcModel(N=self.N, F=self.Fp, K=self.K, flags=hip.MODEL_GRAD_TAIL,
                                   W1=hip.ptr(v["conv1.weight"]), b1=hip.ptr(v["conv1.bias"]),
                                   W2=hip.ptr(v["conv2.weight"]), b2=hip.ptr(v["conv2.bias"]))

    # ---- slab copy of W1
    def _param_signature(self):
        # every torch-visible in-place write bumps the version counter of the tensor it went through: the flat
        # buffer (and its views) or an adopted nn.Parameter.  The library's kernels write through raw pointers
        # and bump nothing - they keep the slab current themselves.
        return (self.flat._version,) + tuple(p._version for p in self._adopted)

    def ensure_slab(self) -> int:
        """Device pointer of the slab copy of conv1.weight (gmc_model.W1_slab), re-built first when a torch
        operation wrote the parameters since it was last known to be current (optimizer.step(), load_state_dict,
        a broadcast, ...).  0 when the copy is switched off (``slab_enabled`` = False).  A write
        torch cannot see (``param.data`` arithmetic, foreign kernels) is picked up one step late: the Adam
        kernels refresh the copy from the row-major weights on every step."""
        if not self.slab_enabled:
            return 0
        self._three_way_only("the slab copy of conv1.weight")
        sig = self._param_signature()
        if self.w1_slab is None:
            self.w1_slab = torch.empty(int(self.lib.gmc_w1_slab_floats(self.N, self.Fp)), dtype=torch.float32,
                                       device=self.device)
            self._slab_sig = None
        if sig != self._slab_sig:
            rc = self.lib.gmc_w1_slab_f32(hip.ptr(self.flat), self.N, self.Fp, hip.ptr(self.w1_slab), hip.stream())
            hip.check(rc, "gmc_w1_slab_f32")
            self._slab_sig = sig
        return hip.ptr(self.w1_slab)

    def _three_way_only(self, what: str) -> None:
        if self.attention:
            raise NotImplementedError(f"{what} is implemented for layer1 = 'graphconv' only (this is the attention engine, "
                                      "layer1 = 'attention': forward, train_fwd_bwd and the Adam steps are what it offers)")
        if self.kway:
            raise NotImplementedError(f"{what} is implemented for the fused 3-class engine only (this is the K-class engine, "
                                      f"number_classes = {self.K}: forward, train_fwd_bwd and the Adam steps are what it "
                                      "offers)")

    def _entry(self, name: str, large: bool = False) -> str:
        """The library entry point of a call: gmc_<name>, gmc_kway_<name> for number_classes != 3, gmc_att_<name> for the
        attention engine; ``large``: gmc_large_<name>, for a batch that :meth:`needs_large`."""
        if large:
            return f"gmc_large_{name}"
        return f"gmc_att_{name}" if self.attention else f"gmc_kway_{name}" if self.kway else f"gmc_{name}"

    def needs_large(self, batch: GraphBatch, loss: str = "cut") -> bool:
        """Does this batch hold a graph too large for the engine's ordinary sequence (one workgroup per graph's head: more
        than ``hip.MAX_GRAPH_NODES`` nodes, fewer for the K-class engine at number_classes > 3)?  The library decides
        (gmc_large_required); the answer is kept with the batch.  Such a batch runs forward / train_fwd_bwd through
        gmc_large_* - several workgroups per graph, up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes - and nothing else."""
        key = (self.K, hip.loss_kind(loss))
        cache = batch.__dict__.setdefault("_needs_large", {})
        if key not in cache:
            model = hip.GmcModel(K=self.K, flags=hip.MODEL_LOSS_EXPECTED if key[1] else 0)
            rc = int(self.lib.gmc_large_required(batch.ref(), C.byref(model)))
            if rc < 0:
                hip.check(rc, "gmc_large_required")
            cache[key] = bool(rc)
        return cache[key]

    def _small_only(self, batch: GraphBatch, what: str) -> None:
        """NotImplementedError for what a batch that :meth:`needs_large` does not offer (either loss: the stricter one)."""
        if self.needs_large(batch, "expected_cut"):
            raise NotImplementedError(
                f"{what} is implemented for graphs of up to {hip.MAX_GRAPH_NODES} nodes only (fewer for number_classes > 3, "
                f"where the head's [n,K] tiles have to fit a CU's LDS): this batch has a graph of {batch.n_max} nodes, "
                f"number_classes = {self.K}.  Larger graphs (up to {hip.LARGE_MAX_GRAPH_NODES} nodes) offer forward and "
                "train_fwd_bwd with layer1 = 'graphconv', without dropout and with the padded adjacency as features")

    def _layer1_args(self) -> tuple:
        """What the gmc_att_* calls take behind the model struct: the two attention vectors and the slope."""
        if not self.attention:
            return ()
        v = self.padded_views()
        return hip.ptr(v["conv1.attn_src"]), hip.ptr(v["conv1.attn_dst"]), hip.ATTENTION_SLOPE

    def _check_terminals(self, batch: GraphBatch) -> None:
        if self.kway and batch.B and int(batch.sizes.min()) < self.K:
            raise ValueError(f"number_classes = {self.K}: every graph needs at least {self.K} nodes (nodes 0..{self.K - 1} "
                             f"are its terminals), got one with {int(batch.sizes.min())}")

    def _call_model(self, slab: bool = False, loss: str = "cut") -> hip.GmcModel:
        """A call's own gmc_model: a copy of the resident one (weights, dropout); ``slab``: with the (current) slab copy
        of W1; ``loss``: the loss the call computes (GMC_MODEL_LOSS_EXPECTED in the flags for ``expected_cut``).  The
        resident struct is never written for a call, so there is nothing to restore after one."""
        model = hip.GmcModel.from_buffer_copy(self._model)
        if slab:
            model.W1_slab = self.ensure_slab()
        if hip.loss_kind(loss):
            model.flags |= hip.MODEL_LOSS_EXPECTED
        return model

    def set_dropout(self, p: float, seed: Optional[int] = None) -> None:
        """F.dropout between the layers (TrainingNeural.py:82) for the next forward / training calls:
        ``p`` = 0 switches it off (eval mode, every reference configuration).  ``seed`` = None draws one
        from torch's CPU generator, so ``torch.manual_seed`` makes runs repeatable (the mask itself is the
        library's counter-based hash, not torch's random stream)."""
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"dropout probability has to be in [0, 1), got {p}")
        if p > 0.0:
            self._three_way_only("dropout")
        if p > 0.0 and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self._model.dropout_p = p
        self._model.dropout_seed_lo = (seed or 0) & 0xFFFFFFFF
        self._model.dropout_seed_hi = ((seed or 0) >> 32) & 0xFFFFFFFF

    def dropout_state(self) -> Tuple[float, int]:
        return float(self._model.dropout_p), (int(self._model.dropout_seed_hi) << 32) | int(self._model.dropout_seed_lo)

    @contextlib.contextmanager
    def dropout(self, p: float, seed: Optional[int] = None):
        """``with eng.dropout(p, seed):`` - :meth:`set_dropout` for the calls inside, the previous (p, seed) after them."""
        before = self.dropout_state()
        self.set_dropout(p, seed)
        try:
            yield
        finally:
            self.set_dropout(*before)

    def adopt(self, module: torch.nn.Module) -> None:
        """Make ``module.conv{1,2}.{weight,bias}`` (and the attention vectors) views of the flat buffer (values kept)."""
        named = dict(module.named_parameters())
        views = self.views()
        for k in self.param_order:
            p = named[k]
            if p.data_ptr() != views[k].data_ptr() or p.device != self.device or p.stride() != views[k].stride():
                views[k].copy_(p.detach().to(self.device, torch.float32))
                p.data = views[k]
        self._adopted = [named[k] for k in self.param_order]
        self._slab_sig = None

    def owns(self, module: torch.nn.Module) -> bool:
        named = dict(module.named_parameters())
        views = self.views()
        return all(named[k].data_ptr() == views[k].data_ptr() and named[k].stride() == views[k].stride()
                   for k in self.param_order)

    def make_batch(self, handles, values=None) -> GraphBatch:
        return GraphBatch(handles, values, self.device)

    # ---- scratch and outputs
    def _workspace(self, batch: GraphBatch, training: bool) -> Tuple[torch.Tensor, int]:
        need = self.workspace_bytes(batch, training)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return self._ws, self._ws.numel()

    def _outputs(self, batch: GraphBatch, out=None, want_loss: bool = True):
        """(P [R,K], S [R], losses [B]) of a call: the caller's ``out``, else fresh (S, losses only when ``want_loss``)."""
        if out is not None:
            return out
        P = torch.empty((batch.R, self.K), dtype=torch.float32, device=self.device)
        S = torch.empty(batch.R, dtype=torch.int32, device=self.device) if want_loss else None
        losses = torch.empty(batch.B, dtype=torch.float32, device=self.device) if want_loss else None
        return P, S, losses

    # ---- compute
    def workspace_bytes(self, batch: GraphBatch, training: bool) -> int:
        large = self.needs_large(batch, "expected_cut")   # (either loss: gmc_large_*'s scratch covers gmc_kway_*'s)
        if large:
            self._large_only_what_it_offers(batch)
        return max(256, int(getattr(self.lib, self._entry("workspace_bytes", large))(batch.ref(), C.byref(self._model),
                                                                                    int(training))))

    def _large_only_what_it_offers(self, batch: GraphBatch) -> None:
        if self.attention:
            self._small_only(batch, "layer1 = 'attention'")
        if self._model.dropout_p > 0.0:
            self._small_only(batch, "dropout")

    def forward(self, batch: GraphBatch, C_: float = 1.0, want_loss: bool = False,
                ws: Optional[torch.Tensor] = None, loss: str = "cut", terminals: bool = True):
        """P [R,K] (and S [R], loss [B] when ``want_loss``) - TrainingNeural.py:79-85.
        ``ws``: caller-owned scratch (kept alive for a later :meth:`backward_from_gp`).  ``loss``: ``"cut"`` (the
        reference's -C * cut of the argmax decode) or ``"expected_cut"`` (the relaxed loss: ``hip.LOSS_KINDS``).
        ``terminals=False``: the caller wants P alone - the plain softmax, the same bytes either way - for a decode
        without terminals, so a graph of fewer than number_classes nodes is no error here (the head gives such a graph
        min(n, K) terminals and reads nothing outside its rows; S and the loss still carry them).  The library's own
        bound stays: a batch whose LARGEST graph is below number_classes is refused (``ValueError``, gmc error -6)."""
        return self._forward(batch, None, C_, want_loss, ws, loss, check_terminals=bool(terminals))

    def _forward(self, batch: GraphBatch, X: Optional[torch.Tensor], C_: float, want_loss: bool,
                 ws: Optional[torch.Tensor], loss: str, check_terminals: bool = True):
        """:meth:`forward` (``X`` None: gmc_forward) and :meth:`forward_features` (gmc_forward_features)."""
        hip.loss_kind(loss)
        if X is not None:
            self._three_way_only("a forward through dense node features")
            self._small_only(batch, "a forward through dense node features")
        if check_terminals:
            self._check_terminals(batch)
        large = X is None and self.needs_large(batch, loss)
        if large:
            self._large_only_what_it_offers(batch)
        P, S, losses = self._outputs(batch, None, want_loss)
        Xd = None if X is None else self.pad_features(batch, X)
        if batch.B == 0:   # nothing to launch (empty tensors have no device pointer to hand over)
            return P, S, losses
        if ws is None:   # the engine's own scratch; the dense plan gets one of its own
            ws = (self._workspace(batch, False)[0] if X is None else
                  torch.empty(self.workspace_bytes_features(batch, False), dtype=torch.uint8, device=self.device))
        name, feat = ((self._entry("forward", large), self._layer1_args()) if X is None else
                      ("gmc_forward_features", (hip.ptr(Xd), Xd.shape[1])))
        model = self._call_model(loss=loss)
        rc = getattr(self.lib, name)(batch.ref(), C.byref(model), *feat, C_, hip.ptr(ws), ws.numel(), hip.ptr(P),
                                     hip.ptr(S), hip.ptr(losses), hip.stream())
        hip.check(rc, name)
        return P, S, losses

    def train_fwd_bwd(self, batch: GraphBatch, C_: float = 1.0, out=None, ws: Optional[torch.Tensor] = None,
                      slab: bool = False, loss: str = "cut"):
        """forward + loss + backward for the batch's summed loss; gradient lands in
        ``self.grad[:count]`` - TrainingNeural.py:373-385.  ``ws``: caller-owned scratch (a trainer
        whose launches are captured into a hipGraph must own it: the engine's own scratch moves
        whenever a later call needs more).  ``loss``: as for :meth:`forward`."""
        hip.loss_kind(loss)
        self._check_terminals(batch)
        P, S, losses = self._outputs(batch, out)
        if batch.B == 0:   # no graphs: zero gradient AND zero loss in the tail slot, nothing to launch
            self.grad[:self.count + 1].zero_()
            return P, S, losses
        large = self.needs_large(batch, loss)
        if large:
            self._large_only_what_it_offers(batch)
            if slab and self.slab_enabled:
                self._small_only(batch, "the slab copy of conv1.weight")
        ws, nbytes = (ws, ws.numel()) if ws is not None else self._workspace(batch, True)
        model = self._call_model(slab, loss)
        name = self._entry("train_fwd_bwd", large)
        rc = getattr(self.lib, name)(batch.ref(), C.byref(model), *self._layer1_args(), C_, hip.ptr(ws), nbytes, hip.ptr(P),
                                     hip.ptr(S), hip.ptr(losses), hip.ptr(self.grad), hip.stream())
        hip.check(rc, name)
        return P, S, losses

    def train_step(self, batch: GraphBatch, lr: float, C_: float = 1.0, out=None, betas=(0.9, 0.999),
                   eps: float = 1e-8, ws: Optional[torch.Tensor] = None, slab: bool = False,
                   loss_ptr: Optional[int] = None, loss: str = "cut"):
        """One whole optimizer step (forward, loss, backward, fused gradient fold + Adam) - the
        single-GPU form of the loop body of train_single_epoch (TrainingNeural.py:373-386).
        Replay-invariant: the step number is read from / advanced in device memory.  ``loss_ptr``: device-side
        address of pinned host memory (``hip.mapped_ptr``) that receives the per-graph losses instead of
        ``out[2]`` - each is stored as soon as it is final, before the backward kernels run.  ``loss``: as for
        :meth:`forward` (gmc_train_step_loss_f32; a one-graph ``expected_cut`` step launches the head on its own)."""
        kind = hip.loss_kind(loss)
        self._three_way_only("the fused train_step")
        self._small_only(batch, "the fused train_step")
        ws, nbytes = (ws, ws.numel()) if ws is not None else self._workspace(batch, True)
        P, S, losses = out if out is not None else self._outputs(batch)
        tail = (self.ensure_slab() if slab else None, hip.stream())
        rc = self.lib.gmc_train_step_loss_f32(batch.ref(), self.N, self.Fp, hip.ptr(self.flat), C_, kind, hip.ptr(ws),
                                              nbytes, hip.ptr(P), hip.ptr(S), loss_ptr or hip.ptr(losses),
                                              hip.ptr(self.grad), hip.ptr(self.m), hip.ptr(self.v), lr, betas[0],
                                              betas[1], eps, hip.ptr(self.step_dev), *tail)
        if not slab:
            self._slab_sig = None   # W1 moved, the copy did not
        hip.check(rc, "gmc_train_step_loss_f32")
        self.step_count += 1
        self._dev_step += 1
        return P, S, losses

    def backward_from_gp(self, batch: GraphBatch, P: torch.Tensor, GP: torch.Tensor,
                         ws: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Gradients for a caller-supplied dLoss/dP (autograd path); ``ws`` must be the
        (training-sized) workspace of the forward that produced ``P``."""
        return self._backward(batch, None, P, GP, ws, False)[0]

    def _backward(self, batch: GraphBatch, X: Optional[torch.Tensor], P: torch.Tensor, GP: torch.Tensor,
                  ws: Optional[torch.Tensor], want_dx: bool):
        """:meth:`backward_from_gp` (``X`` None: gmc_backward_from_gp) and :meth:`backward_features_from_gp`
        (gmc_backward_features_from_gp): (parameter gradients, dX or None)."""
        self._three_way_only("the backward from a caller's dLoss/dP")
        self._small_only(batch, "the backward from a caller's dLoss/dP")
        Xd = None if X is None else self.pad_features(batch, X)
        dX = torch.empty_like(Xd) if want_dx else None
        if batch.B == 0:
            self.grad[:self.count].zero_()
        else:
            if ws is None:
                ws = self._workspace(batch, True)[0]
            name, feat, dx = (("gmc_backward_from_gp", (), ()) if X is None else
                              ("gmc_backward_features_from_gp", (hip.ptr(Xd), Xd.shape[1]), (hip.ptr(dX), Xd.shape[1])))
            rc = getattr(self.lib, name)(batch.ref(), C.byref(self._model), *feat, hip.ptr(ws), ws.numel(), hip.ptr(P),
                                         hip.ptr(GP.to(torch.float32).contiguous()), hip.ptr(self.grad), *dx, hip.stream())
            hip.check(rc, name)
        return self.views(self.grad), (dX[:, :self.N] if want_dx else None)

    # ---- features that are not the padded adjacency (layer 1 is a dense GEMM: gmc_forward_features)
    def workspace_bytes_features(self, batch: GraphBatch, training: bool) -> int:
        self._three_way_only("a forward through dense node features")
        self._small_only(batch, "a forward through dense node features")
        return max(256, int(self.lib.gmc_workspace_bytes_features(batch.ref(), C.byref(self._model), int(training))))

    def pad_features(self, batch: GraphBatch, X: torch.Tensor) -> torch.Tensor:
        """``X`` [R, N] as the library takes it: fp32 on the device, 16-byte aligned rows - the columns padded with
        zeros to a multiple of 4 when N is not one.  A tensor this method returned passes through unchanged, so a
        caller that runs forward and backward on the same features pads them once."""
        return padded_features(X, batch.R, self.N, self.device)

    def forward_features(self, batch: GraphBatch, X: torch.Tensor, C_: float = 1.0, want_loss: bool = False,
                         ws: Optional[torch.Tensor] = None, loss: str = "cut"):
        """:meth:`forward` for node features ``X`` [R, N] that are not the padded adjacency (the rows of the batch's
        graphs stacked): the layer-1 feature transform is the library's fp32 MFMA GEMM.  ``ws``: caller-owned scratch
        of :meth:`workspace_bytes_features` bytes (kept alive for :meth:`backward_features_from_gp`).  ``loss``: as for
        :meth:`forward`."""
        return self._forward(batch, X, C_, want_loss, ws, loss)

    def backward_features_from_gp(self, batch: GraphBatch, X: torch.Tensor, P: torch.Tensor, GP: torch.Tensor,
                                  ws: torch.Tensor, want_dx: bool = True):
        """(parameter gradients, dX or None) for a caller-supplied dLoss/dP; ``ws``: the training-sized scratch of the
        :meth:`forward_features` call that produced ``P`` from the same ``X``.  ``want_dx`` = False skips the dX GEMM."""
        return self._backward(batch, X, P, GP, ws, want_dx)

    def adam_step(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8) -> None:
        """torch.optim.Adam.step over the flat buffer (TrainingNeural.py:386)."""
        self.step_count += 1
        rc = self.lib.gmc_adam_f32(hip.ptr(self.flat), hip.ptr(self.grad), hip.ptr(self.m),
                                   hip.ptr(self.v), self.count, lr, betas[0], betas[1], eps,
                                   self.step_count, hip.stream())
        hip.check(rc, "gmc_adam_f32")
        self._slab_sig = None   # W1 moved, the slab copy did not

    def adam_step_dev(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, slab: bool = False,
                      publish: Optional[Tuple[torch.Tensor, int]] = None) -> None:
        """Same update with the step number read from (and advanced in) device memory, so the
        launch can be captured into a hipGraph and replayed (``step_dev`` must equal
        ``step_count`` on entry; both advance by one).  ``slab``: the updated conv1.weight goes to the slab
        copy as well (which must be current: :meth:`ensure_slab`).  ``publish`` = (device floats, device-side
        address of pinned host memory): the values are stored there by the one-wave launch that also advances the
        step counter, in front of the Adam sweep (two launches for publish + Adam + tick instead of three)."""
        keep_slab = slab and self.slab_enabled
        if keep_slab:
            self._three_way_only("the slab copy of conv1.weight")
        if (self.kway or self.attention) and publish is not None:   # (the fused publish + Adam launch knows the N x F x 3 layout only)
            self.publish(*publish)
            publish = None
        bufs = (hip.ptr(self.flat), hip.ptr(self.grad), hip.ptr(self.m), hip.ptr(self.v))
        if publish is not None:
            name, (src, dst) = "gmc_publish_adam_devstep_model_f32", publish
            args = (hip.ptr(src), src.numel(), dst, *bufs, self.N, self.Fp, self.ensure_slab() if keep_slab else None)
        elif keep_slab:
            name, args = "gmc_adam_devstep_model_f32", (*bufs, self.N, self.Fp, self.ensure_slab())
        else:
            name, args = "gmc_adam_devstep_f32", (*bufs, self.count)
        rc = getattr(self.lib, name)(*args, lr, betas[0], betas[1], eps, hip.ptr(self.step_dev), hip.stream())
        if not keep_slab:
            self._slab_sig = None   # W1 moved, the slab copy did not
        hip.check(rc, name)
        self.step_count += 1
        self._dev_step += 1

    def sync_step_dev(self) -> None:
        """Make the device-side step counter equal ``step_count`` - a fill launch only when they differ
        (after host-stepped Adam launches); a trainer replaying its graph epoch after epoch never needs it."""
        if self._dev_step != self.step_count:
            self.step_dev.fill_(self.step_count)
            self._dev_step = self.step_count

    def sync_replicas(self, src: int = 0) -> None:
        """Data-parallel start-up: every rank takes rank ``src``'s parameters, Adam moments and step
        count, so that replicas built from different RNG states apply the all-reduced gradient to the
        SAME weights (the reference has one model; N replicas must be that one model)."""
        if not dp_active():
            return
        for buf in (self.flat, self.m, self.v):
            dist.broadcast(buf, src)
        step = torch.tensor([self.step_count], dtype=torch.int64, device=self.device)
        dist.broadcast(step, src)
        self.step_count = int(step.item())
        self._dev_step = -1
        self._slab_sig = None   # (a collective writes through raw pointers: no version counter moves)
        self.sync_step_dev()

    def publish(self, src: torch.Tensor, pinned_dst: int) -> None:
        """``src`` (device floats) -> pinned host memory at its device-side address ``pinned_dst``
        (``hip.mapped_ptr``), one system-scope store per value, on the current stream."""
        rc = self.lib.gmc_publish_f32(hip.ptr(src), src.numel(), pinned_dst, hip.stream())
        hip.check(rc, "gmc_publish_f32")

    def allreduce_grad(self, local_loss_sum: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """One RCCL all-reduce (sum) of [grad | loss] over xGMI when torch.distributed is up."""
        if local_loss_sum is not None:
            self.grad[self.count] = local_loss_sum
        if dp_active():
            dist.all_reduce(self.grad, op=dist.ReduceOp.SUM)
        return self.grad[self.count] if local_loss_sum is not None else None


def padded_features(X: torch.Tensor, R: int, N: int, device) -> torch.Tensor:
    """:meth:`FusedEngine.pad_features` for ``R`` rows and ``N`` columns (``functional.gcn_softmax`` pads the same way)."""
    ld = (N + 3) // 4 * 4
    if X.dim() != 2 or X.shape[0] != R or X.shape[1] not in (N, ld):
        raise ValueError(f"features must be [{R}, {N}], got {tuple(X.shape)}")
    X = X.detach().to(device, torch.float32)
    if X.shape[1] != ld:
        Xp = torch.zeros((R, ld), dtype=torch.float32, device=device)
        Xp[:, :N] = X
        return Xp
    X = X.contiguous()
    return X.clone() if X.data_ptr() % 16 else X


# ---- one model per graph ------------------------------------------------------------------------------------------------
def instance_layout(sizes: Sequence[int], F: int, K: int) -> Tuple[List[int], int]:
    """Offsets of the four blocks and the float count of the flat buffer of one model per graph (include/gcnmaxcut.h,
    gmc_inst_*): ``[W1 [R,F] | b1 [B,F] | W2 [B,F,K] | b2 [B,K]]`` for graphs of ``sizes`` nodes, R = sum(sizes).  ``F`` is
    the width the kernels see (a multiple of 4)."""
    R, B = int(sum(int(n) for n in sizes)), len(sizes)
    offs = [0]
    for s in (R * F, B * F, B * F * K, B * K):
        offs.append(offs[-1] + s)
    return offs, offs[-1]


def draw_instance_parameters(sizes: Sequence[int], F: int, K: int) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """The reference's ``GraphConv`` init for one model of ``n_nodes = n_g`` per graph: graph by graph in batch order,
    ``conv1.weight [n_g, F]`` and then ``conv2.weight [F, K]`` with ``nn.init.xavier_uniform_`` from torch's (CPU)
    generator - uniform within sqrt(6 / (n_g + F)) and sqrt(6 / (F + K)); the biases are zero.  CPU tensors."""
    out = []
    for n in sizes:
        w1, w2 = torch.empty(int(n), F), torch.empty(F, K)
        torch.nn.init.xavier_uniform_(w1)
        torch.nn.init.xavier_uniform_(w2)
        out.append((w1, w2))
    return out


def instance_too_large(n_max: int, K: int, loss: str = "cut") -> bool:
    """Is a graph of ``n_max`` nodes beyond what the one-workgroup head of gmc_kway_* / gmc_inst_* takes at ``K`` classes
    and this loss?  The library decides (gmc_large_required: host only, no GPU)."""
    if K == 3:   # (gmc_large_required answers for the fused 3-class entry points at K = 3; the bound here is gmc_kway_*'s)
        return n_max > hip.MAX_GRAPH_NODES
    model = hip.GmcModel(K=K, flags=hip.MODEL_LOSS_EXPECTED if hip.loss_kind(loss) else 0)
    rc = int(hip.load().gmc_large_required(C.byref(hip.GmcBatch(B=1, n_max=int(n_max))), C.byref(model)))
    if rc < 0:
        hip.check(rc, "gmc_large_required")
    return bool(rc)


class InstanceEngine:
    """One model PER GRAPH for a whole batch of graphs (gmc_inst_*): graph g of the batch has its own
    ``conv1.weight [n_g, F]`` (one embedding row per node), ``conv1.bias``, ``conv2.weight [F, K]`` and ``conv2.bias``, and
    one launch sequence trains all of them at once; nothing couples two graphs.  Owns the batch, the flat parameter
    buffer ``[W1 [R,F] | b1 [B,F] | W2 [B,F,K] | b2 [B,K]]`` with gradient and Adam moments of the same layout, and the best
    partition seen per graph, and the per-graph state of early stopping (``prev_loss``, ``stall``, ``stop_epoch``: -1 while
    a graph runs; include/gcnmaxcut.h, gmc_inst_early_stop_f32).  It does not touch :class:`FusedEngine`; number_classes
    2..8, both losses, layer1 = graphconv, no dropout, graphs within the one-workgroup head's bound.

    ``batch_handles``: the graphs' handles, or a ready :class:`GraphBatch` (``GraphBatch.from_edge_index`` builds one on
    the device; ``values`` must then be ``None``).  ``terminals=False``: plain max-K-cut - the head overrides no row, ``S``
    is the row argmax and both losses fix no node (gmc_inst_forward_t / gmc_inst_train_fwd_bwd_t with terminals = 0); a
    graph then needs one node, not K.  ``node_cost``: a [R, K] float32 tensor of per-node class costs (moved to the engine's device if it is elsewhere), indexed by
    batch row - both losses then train on ``cut - sum_v node_cost[v] . P_v`` (the hard loss: ``node_cost[v][S_v]``) through
    gmc_inst_forward_c / gmc_inst_train_fwd_bwd_c; ``subset`` keeps the rows of the graphs it keeps."""

    # the three entry points of include/gcnmaxcut.h the engine computes through (LargeInstanceEngine: gmc_inst_large_*)
    _WORKSPACE, _FORWARD, _TRAIN = "gmc_inst_workspace_bytes", "gmc_inst_forward_t", "gmc_inst_train_fwd_bwd_t"
    _FORWARD_COST, _TRAIN_COST = "gmc_inst_forward_c", "gmc_inst_train_fwd_bwd_c"   # (None: the sequence takes no cost)

    def __init__(self, batch_handles, F: int, K: int, device: Optional[torch.device] = None, *, values=None,
                 terminals: bool = True, node_cost: Optional[torch.Tensor] = None):
        if node_cost is not None and self._FORWARD_COST is None:
            raise NotImplementedError(f"{type(self).__name__} takes no node_cost: the per-node class costs enter the "
                                      "one-workgroup head of InstanceEngine only")
        if isinstance(batch_handles, GraphBatch) and device is not None and torch.device(device) != batch_handles.device:
            raise ValueError(f"the batch lives on {batch_handles.device}, the engine was asked for {torch.device(device)}")
        self.device = batch_handles.device if isinstance(batch_handles, GraphBatch) else device or hip.require_gpu()
        self.lib = hip.load()
        if not 2 <= K <= hip.KWAY_MAX_CLASSES:
            raise ValueError(f"number_classes must be in 2..{hip.KWAY_MAX_CLASSES}, got {K} (nodes 0..K-1 of every graph "
                             "are the terminals of classes 0..K-1)")
        if F < 1 or F > MAX_HIDDEN:
            raise ValueError(f"hidden_dim must be in 1..{MAX_HIDDEN} on this path (include/gcnmaxcut.h: GMC_MAX_HIDDEN), "
                             f"got {F}")
        self.terminals = bool(terminals)
        if isinstance(batch_handles, GraphBatch):
            if values is not None:
                raise ValueError("values come with handles: a ready GraphBatch already holds its edge weights")
            self._check_sizes(batch_handles.sizes, K)
            self._handles, self._values = None, None   # (subset() reads them from the batch when it needs them)
            self.batch = batch_handles
        else:
            handles = list(batch_handles)
            self._check_sizes([h.n for h in handles], K)
            self._handles, self._values = handles, None if values is None else list(values)   # (kept for subset())
            self.batch = GraphBatch(handles, values, self.device)
        self.F, self.K, self.Fp = F, K, (F + 3) // 4 * 4   # (the kernels see the hidden width padded to float4 columns)
        self.B, self.R = self.batch.B, self.batch.R
        self.offs, self.count = instance_layout(self.batch.sizes, self.Fp, K)
        self.flat = torch.zeros(self.count + 4, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.step_count = 0
        self.best_S = torch.zeros(self.R, dtype=torch.int32, device=self.device)
        self.best_loss = torch.full((self.B,), float("inf"), dtype=torch.float32, device=self.device)
        self.best_epoch = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
        self.prev_loss = torch.full((self.B,), float("inf"), dtype=torch.float32, device=self.device)
        self.stall = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.stop_epoch = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
        self._ws: Optional[torch.Tensor] = None
        if node_cost is not None:
            if (not isinstance(node_cost, torch.Tensor) or node_cost.dtype != torch.float32
                    or tuple(node_cost.shape) != (self.R, K)):
                raise ValueError(f"node_cost must be a [{self.R}, {K}] float32 tensor")
            node_cost = node_cost.to(self.device).contiguous()   # (a no-op for a tensor that is there already)
        self.node_cost = node_cost

    def _check_sizes(self, sizes: Sequence[int], K: int) -> None:
        check_instance_sizes(sizes, K, terminals=self.terminals)

    # ---- parameters
    def blocks(self, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The four stacked blocks as the kernels see them (hidden width padded to Fp): views of ``buf``."""
        buf = self.flat if buf is None else buf
        o, R, B, F, K = self.offs, self.R, self.B, self.Fp, self.K
        return {"conv1.weight": buf[o[0]:o[1]].view(R, F), "conv1.bias": buf[o[1]:o[2]].view(B, F),
                "conv2.weight": buf[o[2]:o[3]].view(B, F, K), "conv2.bias": buf[o[3]:o[4]].view(B, K)}

    def views(self, g: int, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Graph ``g``'s four tensors in the reference's shapes (``conv1.weight [n_g, F]``, ...): views of ``buf``
        (default the parameters; ``eng.grad``, ``eng.m``, ``eng.v`` have the same layout)."""
        b, F = self.blocks(buf), self.F
        r0, r1 = int(self.batch.goff_host[g]), int(self.batch.goff_host[g + 1])
        return {"conv1.weight": b["conv1.weight"][r0:r1, :F], "conv1.bias": b["conv1.bias"][g, :F],
                "conv2.weight": b["conv2.weight"][g, :F], "conv2.bias": b["conv2.bias"][g]}

    def reset_parameters(self) -> None:
        """:func:`draw_instance_parameters` into the flat buffer (padding columns and biases zero), Adam state, the kept
        partitions and the early-stopping state back to their start."""
        for buf in (self.flat, self.grad, self.m, self.v):
            buf.zero_()
        for g, (w1, w2) in enumerate(draw_instance_parameters(self.batch.sizes, self.F, self.K)):
            v = self.views(g)
            v["conv1.weight"].copy_(w1)
            v["conv2.weight"].copy_(w2)
        self.step_count = 0
        self.best_S.zero_()
        self.best_loss.fill_(float("inf"))
        self.best_epoch.fill_(-1)
        self.prev_loss.fill_(float("inf"))
        self.stall.zero_()
        self.stop_epoch.fill_(-1)

    def module(self, g: int):
        """A ``GCNSoftmax(n_g, F, K)`` holding COPIES of graph ``g``'s parameters: ``evaluate_model``, ``round_dataset``,
        ``search_dataset`` and ``sampling_optimization`` run on that graph with it as with any trained model.  (Building
        it leaves torch's random generator where it was.)"""
        return module_of({k: t.detach().cpu() for k, t in self.views(g).items()})

    def parameters(self) -> List[Dict[str, torch.Tensor]]:
        """CPU copies of every graph's four tensors, in batch order (one device-to-host copy of the flat buffer)."""
        flat = self.flat.cpu()
        return [{k: t.clone() for k, t in self.views(g, flat).items()} for g in range(self.B)]

    def _model(self, loss: str) -> hip.GmcModel:
        b = self.blocks()
        return hip.GmcModel(N=self.R, F=self.Fp, K=self.K, flags=hip.MODEL_LOSS_EXPECTED if hip.loss_kind(loss) else 0,
                            W1=hip.ptr(b["conv1.weight"]), b1=hip.ptr(b["conv1.bias"]), W2=hip.ptr(b["conv2.weight"]),
                            b2=hip.ptr(b["conv2.bias"]))

    # ---- compute
    def workspace_bytes(self, training: bool) -> int:
        model = hip.GmcModel(N=self.R, F=self.Fp, K=self.K)
        return max(256, int(getattr(self.lib, self._WORKSPACE)(self.batch.ref(), C.byref(model), int(training))))

    def _workspace(self, training: bool) -> torch.Tensor:
        need = self.workspace_bytes(training)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _outputs(self, out=None):
        if out is not None:
            return out
        return (torch.empty((self.R, self.K), dtype=torch.float32, device=self.device),
                torch.empty(self.R, dtype=torch.int32, device=self.device),
                torch.empty(self.B, dtype=torch.float32, device=self.device))

    def forward(self, C_: float = 1.0, loss: str = "cut", out=None):
        """(P [R,K], S [R], loss [B]) of every graph under its own model."""
        P, S, losses = self._outputs(out)
        if self.B == 0:
            return P, S, losses
        ws = self._workspace(False)
        name, cost = (self._FORWARD, ()) if self.node_cost is None else (self._FORWARD_COST, (hip.ptr(self.node_cost),))
        rc = getattr(self.lib, name)(self.batch.ref(), C.byref(self._model(loss)), int(self.terminals), *cost, C_,
                                     hip.ptr(ws), ws.numel(), hip.ptr(P), hip.ptr(S), hip.ptr(losses), hip.stream())
        hip.check(rc, name)
        return P, S, losses

    def train_fwd_bwd(self, C_: float = 1.0, loss: str = "cut", out=None):
        """forward + loss + backward of every graph's own loss; the gradient lands in ``self.grad[:count]``."""
        P, S, losses = self._outputs(out)
        if self.B == 0:
            self.grad.zero_()
            return P, S, losses
        ws = self._workspace(True)
        name, cost = (self._TRAIN, ()) if self.node_cost is None else (self._TRAIN_COST, (hip.ptr(self.node_cost),))
        rc = getattr(self.lib, name)(self.batch.ref(), C.byref(self._model(loss)), int(self.terminals), *cost, C_,
                                     hip.ptr(ws), ws.numel(), hip.ptr(P), hip.ptr(S), hip.ptr(losses),
                                     hip.ptr(self.grad), hip.stream())
        hip.check(rc, name)
        return P, S, losses

    def adam_step(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, running_only: bool = False) -> None:
        """torch.optim.Adam.step over the flat buffer: every instance shares the step number.  ``running_only``: the
        sweep cut by graph (gmc_inst_adam_f32) that neither reads nor writes anything of a graph whose ``stop_epoch`` is
        set; a running graph takes the same bits from either sweep."""
        self.step_count += 1
        if self.count == 0:
            return
        if running_only:
            if inst_adam_too_large(self.batch.n_max, self.Fp, self.K):
                raise ValueError(f"adam_step(running_only=True): a graph of {self.batch.n_max} nodes at hidden width "
                                 f"{self.Fp} is beyond the segmented Adam's bound of {INST_ADAM_MAX_TILES} tiles of "
                                 f"{hip.INST_ADAM_TILE_FLOATS} floats per graph (n_max * hidden_dim up to about 2^28)")
            rc = self.lib.gmc_inst_adam_f32(self.batch.ref(), self.Fp, self.K, hip.ptr(self.flat), hip.ptr(self.grad),
                                            hip.ptr(self.m), hip.ptr(self.v), lr, betas[0], betas[1], eps, self.step_count,
                                            hip.ptr(self.stop_epoch), hip.stream())
            hip.check(rc, "gmc_inst_adam_f32")
            return
        rc = self.lib.gmc_adam_f32(hip.ptr(self.flat), hip.ptr(self.grad), hip.ptr(self.m), hip.ptr(self.v), self.count,
                                   lr, betas[0], betas[1], eps, self.step_count, hip.stream())
        hip.check(rc, "gmc_adam_f32")

    def keep_best(self, S: torch.Tensor, losses: torch.Tensor, epoch: int) -> None:
        """For every graph whose loss is below its best so far (strictly: the first minimum wins, NaN never): its rows of
        ``S`` into ``best_S``, the loss into ``best_loss``, ``epoch`` into ``best_epoch`` (gmc_inst_keep_best_f32)."""
        if self.B == 0:
            return
        rc = self.lib.gmc_inst_keep_best_f32(self.batch.ref(), hip.ptr(S), hip.ptr(losses), int(epoch), hip.ptr(self.best_S),
                                             hip.ptr(self.best_loss), hip.ptr(self.best_epoch), hip.stream())
        hip.check(rc, "gmc_inst_keep_best_f32")

    def early_stop(self, S: torch.Tensor, losses: torch.Tensor, epoch: int, tolerance: float, patience: int) -> None:
        """:meth:`keep_best` behind the reference's tolerance / patience rule, per graph (gmc_inst_early_stop_f32; the
        rule is stated in include/gcnmaxcut.h): a graph whose loss has stalled ``patience`` epochs in a row gets
        ``stop_epoch[g] = epoch`` and is frozen from then on - no keep-best in that call or later, and
        ``adam_step(running_only=True)`` passes it by.  Nothing here waits for the device."""
        if self.B == 0:
            return
        rc = self.lib.gmc_inst_early_stop_f32(self.batch.ref(), hip.ptr(S), hip.ptr(losses), int(epoch), float(tolerance),
                                              int(patience), hip.ptr(self.prev_loss), hip.ptr(self.stall),
                                              hip.ptr(self.stop_epoch), hip.ptr(self.best_S), hip.ptr(self.best_loss),
                                              hip.ptr(self.best_epoch), hip.stream())
        hip.check(rc, "gmc_inst_early_stop_f32")

    def stopped(self) -> torch.Tensor:
        """Host copy of ``stop_epoch`` ([B] int32; -1: still running).  The one call here that synchronises."""
        return self.stop_epoch.cpu()

    def subset(self, keep: Sequence[int]) -> "InstanceEngine":
        """A new engine over the graphs ``keep`` of this one (indices into the batch, in ascending order: batch order is
        kept) that goes on where this one stands: their parameters, gradient, Adam moments, ``step_count``, best
        partition / loss / epoch and early-stopping state are carried across, block by block, by device-to-device
        indexing.  A graph's bytes do not depend on its batch, so its further steps are the ones it would have taken
        here."""
        keep = [int(g) for g in keep]
        if any(b <= a for a, b in zip(keep, keep[1:])) or (keep and not 0 <= keep[0] <= keep[-1] < self.B):
            raise ValueError(f"subset: graph indices must ascend within 0..{self.B - 1}, got {keep}")
        values = None if self._values is None else [self._values[g] for g in keep]
        if self._handles is None:   # built over a ready batch: its graphs as handles, edge weights included
            self._handles = self.batch.handles()
        gidx = torch.tensor(keep, dtype=torch.long, device=self.device)
        goff = self.batch.goff_host
        rows = [torch.arange(int(goff[g]), int(goff[g + 1]), device=self.device) for g in keep]
        ridx = torch.cat(rows) if rows else torch.zeros(0, dtype=torch.long, device=self.device)
        cost = {} if self.node_cost is None else {"node_cost": self.node_cost[ridx].contiguous()}
        sub = type(self)([self._handles[g] for g in keep], self.F, self.K, self.device, values=values,
                         terminals=self.terminals, **cost)
        for src, dst in ((self.flat, sub.flat), (self.grad, sub.grad), (self.m, sub.m), (self.v, sub.v)):
            a, b = self.blocks(src), sub.blocks(dst)
            b["conv1.weight"].copy_(a["conv1.weight"][ridx])
            for k in PARAM_ORDER[1:]:
                b[k].copy_(a[k][gidx])
        sub.step_count = self.step_count
        sub.best_S.copy_(self.best_S[ridx])
        for name in ("best_loss", "best_epoch", "prev_loss", "stall", "stop_epoch"):
            getattr(sub, name).copy_(getattr(self, name)[gidx])
        return sub


INST_ADAM_MAX_TILES = 65535   # gmc_inst_adam_f32: a graph's tiles are a grid dimension


def inst_adam_too_large(n_max: int, F: int, K: int) -> bool:
    """Would gmc_inst_adam_f32 refuse a graph of ``n_max`` nodes at hidden width ``F`` (a multiple of 4)?  Its grid has
    one y entry per tile of ``hip.INST_ADAM_TILE_FLOATS`` floats of the largest graph's W1 and of the three small blocks."""
    tile = hip.INST_ADAM_TILE_FLOATS
    w1_tiles = (int(n_max) * (F // 4) + tile // 4 - 1) // (tile // 4)
    small_tiles = (F + F * K + K + tile - 1) // tile
    return w1_tiles + small_tiles > INST_ADAM_MAX_TILES


class LargeInstanceEngine(InstanceEngine):
    """:class:`InstanceEngine` for graphs of up to ``hip.LARGE_MAX_GRAPH_NODES`` nodes (gmc_inst_large_*: several
    workgroups share a graph's head).  Same constructor, buffers and methods; ``forward`` and
    ``train_fwd_bwd`` run the large sequence for every graph of the batch, small ones included - on a batch
    :class:`InstanceEngine` takes the partitions are the same, and probabilities, losses and gradients agree to rounding.
    ``adam_step(running_only=True)`` keeps the segmented Adam's own bound (n_max * hidden_dim up to about 2^28) and
    raises ``ValueError`` beyond it; the plain ``adam_step`` has none.  About 16 * hidden_dim bytes per node for the
    parameters, gradient and moments and 8 * ld for the workspace (ld = hidden_dim rounded up to 32)."""

    _WORKSPACE, _FORWARD, _TRAIN = "gmc_inst_large_workspace_bytes", "gmc_inst_large_forward", "gmc_inst_large_train_fwd_bwd"
    _FORWARD_COST = _TRAIN_COST = None

    def _check_sizes(self, sizes: Sequence[int], K: int) -> None:
        check_large_instance_sizes(sizes, K, terminals=self.terminals)


def check_large_instance_sizes(sizes: Sequence[int], K: int, terminals: bool = True) -> None:
    """:func:`check_instance_sizes` for :class:`LargeInstanceEngine`: the same minimum, ``hip.LARGE_MAX_GRAPH_NODES`` nodes
    at most."""
    sizes = [int(n) for n in sizes]
    if sizes and not terminals and min(sizes) < 1:
        raise ValueError("every graph needs at least one node, got an empty one")
    if sizes and terminals and min(sizes) < K:
        raise ValueError(f"number_classes = {K}: every graph needs at least {K} nodes (nodes 0..{K - 1} "
                         f"are its terminals), got one with {min(sizes)}")
    if sizes and max(sizes) > hip.LARGE_MAX_GRAPH_NODES:
        raise ValueError(f"a graph of {max(sizes)} nodes is beyond the {hip.LARGE_MAX_GRAPH_NODES} nodes of the per-graph "
                         "models' large sequence (gmc_inst_large_*)")


def check_instance_sizes(sizes: Sequence[int], K: int, loss: str = "expected_cut", terminals: bool = True) -> None:
    """What one model per graph refuses of a batch's graph sizes: fewer than K nodes (the K-class engine's ValueError;
    waived with ``terminals=False``, where a graph needs one node), or a graph beyond the one-workgroup head (ValueError
    naming train_model; judged for the stricter loss by default)."""
    sizes = [int(n) for n in sizes]
    if sizes and not terminals and min(sizes) < 1:
        raise ValueError("every graph needs at least one node, got an empty one")
    if sizes and terminals and min(sizes) < K:
        raise ValueError(f"number_classes = {K}: every graph needs at least {K} nodes (nodes 0..{K - 1} "
                         f"are its terminals), got one with {min(sizes)}")
    if sizes and instance_too_large(max(sizes), K, loss):
        raise ValueError(f"a graph of {max(sizes)} nodes is beyond the one-workgroup head of the per-graph models "
                         f"(number_classes = {K}: {hip.MAX_GRAPH_NODES} nodes at most, fewer for number_classes > 3): one "
                         "large graph on its own is what train_model already serves (a model of n_nodes = n), and "
                         "LargeInstanceEngine / maxcut.solve_large train one model per graph up to "
                         f"{hip.LARGE_MAX_GRAPH_NODES} nodes")


def module_of(params: Dict[str, torch.Tensor]):
    """A ``GCNSoftmax`` with these four tensors (by parameter name) as its parameters, built without advancing torch's
    random generator."""
    from .Training.TrainingNeural import TORCH_DEVICE, TORCH_DTYPE, GCNSoftmax
    n, F = params["conv1.weight"].shape
    K = params["conv2.weight"].shape[1]
    with torch.random.fork_rng(devices=[]):
        net = GCNSoftmax(n, F, K, 0.0, TORCH_DEVICE).type(TORCH_DTYPE).to(TORCH_DEVICE)
    with torch.no_grad():
        named = dict(net.named_parameters())
        for k in PARAM_ORDER:
            named[k].copy_(params[k])
    return net


def device_cut_loss(batch: GraphBatch, P: torch.Tensor, C_: float = 1.0, loss: str = "cut", want_gp: bool = True,
                    device: Optional[torch.device] = None):
    """(loss [B], GP [R,3] or None) of given probabilities ``P`` [R,3] (gmc_cut_loss_f32): per-graph loss and
    dLoss/dP, O(edges) on the device - ``GP`` is what :meth:`FusedEngine.backward_from_gp` takes.  The loss has no
    parameters, so it needs no engine."""
    kind = hip.loss_kind(loss)
    device = device or hip.require_gpu()
    if P.dim() != 2 or tuple(P.shape) != (batch.R, 3):
        raise ValueError(f"P must be [{batch.R}, 3], got {tuple(P.shape)}")
    Pd = P.detach().to(device, torch.float32).contiguous()
    losses = torch.empty(batch.B, dtype=torch.float32, device=device)
    GP = torch.empty((batch.R, 3), dtype=torch.float32, device=device) if want_gp else None
    if batch.B == 0:
        return losses, GP
    rc = hip.load().gmc_cut_loss_f32(batch.ref(), hip.ptr(Pd), C_, kind, hip.ptr(losses), hip.ptr(GP), hip.stream())
    hip.check(rc, "gmc_cut_loss_f32")
    return losses, GP


def dp_active() -> bool:
    """Do steps run the data-parallel sequence (shard step -> all-reduce -> Adam)?  Yes with more than one
    rank; also with ONE rank when GCN_MAXCUT_DP_SINGLE_RANK=1 - a one-GPU box then exercises RCCL itself
    (communicator set-up, the collective on the launch stream, hipGraph capture beside its watchdog)."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or os.environ.get("GCN_MAXCUT_DP_SINGLE_RANK") == "1"


def shard_for_rank(n_items: int, rank: int, world: int) -> range:
    """Contiguous, balanced slice of the dataset for one rank."""
    base, extra = divmod(n_items, world)
    start = rank * base + min(rank, extra)
    return range(start, start + base + (1 if rank < extra else 0))


def shard_by_weight(weights: Sequence[int], rank: int, world: int) -> range:
    """Contiguous slice of a group of graphs for one rank, balanced by WORK instead of by count (SURVEY section 8e:
    "for mixed sizes balance by nnz"): ``weights[i]`` = directed edges of graph i.  Equal weights (the regular-graph
    workloads) give exactly :func:`shard_for_rank`.  Otherwise the partition into ``world`` contiguous runs with the
    smallest possible largest run: the smallest capacity for which filling rank after rank (a rank closes when the
    next graph would exceed it) needs at most ``world`` ranks, then that filling - a pure function of the weights, so
    every rank computes the same split without talking; trailing ranks may stay empty."""
    w = [int(x) for x in weights]
    n = len(w)
    if n == 0 or world <= 1 or min(w) == max(w):
        return shard_for_rank(n, rank, world)

    def cuts(cap):
        out, load = [0], 0
        for i, x in enumerate(w):
            if load and load + x > cap:
                out.append(i)
                load = 0
            load += x
        return out

    lo, hi = max(w), sum(w)
    while lo < hi:
        mid = (lo + hi) // 2
        if len(cuts(mid)) <= world:
            hi = mid
        else:
            lo = mid + 1
    starts = cuts(lo)
    starts += [n] * (world + 1 - len(starts))
    return range(starts[rank], starts[rank + 1])
