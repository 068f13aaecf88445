"""The launch machinery of training: how an epoch's optimizer steps reach the GPU.

:class:`FusedTrainer` keeps the device-resident state of one (model, optimizer) pair - the planned graph batches, the
pinned loss slots, the captured hipGraphs - and runs an epoch over one of the launch paths :func:`launch_path` chooses
(:class:`Launch`).  None of this is reference API: ``Training/TrainingNeural.py`` holds the reference's names and calls
into this module (it re-exports ``FusedTrainer``, ``Launch`` and ``launch_path``).  An engine is anything with the
:class:`gcn_max_cut_amd.engine.FusedEngine` surface the chosen path uses; ``hasattr`` tells the host stand-ins apart.
"""
from __future__ import annotations

import enum
import os
import warnings
from time import perf_counter, sleep, time
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import hip
from .engine import PARAM_ORDER, dp_active, shard_by_weight
from .graph import GraphBatch


def _graphs_per_step(explicit: Optional[int]) -> int:
    if explicit is not None:
        return max(1, int(explicit))
    return max(1, int(os.environ.get("GCN_MAXCUT_GRAPHS_PER_STEP", "1")))


_NOT_LANDED = np.uint32(0x7FC0DEAD)   # quiet-NaN payload no arithmetic produces: "this loss slot has not been written"
_SPIN_BEFORE_YIELD = 2048             # ~0.5 ms of looks before the polling loop starts yielding the core
_POLL_DEADLINE_S = 5.0


def _arm(bits: np.ndarray) -> None:
    """Mark every slot of a pinned loss buffer "not landed" before the launches that fill it.  The mark is a BIT
    PATTERN no kernel produces (`_NOT_LANDED`), so a loss that genuinely IS NaN (diverged weights) counts as landed
    and comes back as NaN at once - as `loss.item()` would (TrainingNeural.py:387-388)."""
    bits.fill(_NOT_LANDED)


class Launch(enum.Enum):
    """How :meth:`FusedTrainer.epoch` launches an epoch (chosen by :func:`launch_path`)."""
    DROPOUT = "dropout"       # eager one-kernel-per-operation sequence, a fresh dropout mask per step
    GRAPH = "graph"           # the whole epoch replayed from one hipGraph
    DIRECT = "direct"         # eager train_step launches storing the losses straight into the pinned host slots
    COPY = "copy"             # eager train_step launches, then a copy of the losses and a stream synchronisation
    DP = "dp"                 # data-parallel sequence (shard step -> all-reduce -> Adam), eager
    DP_GRAPHS = "dp_graphs"   # the same with hipGraphs on either side of the eager all-reduce


def launch_path(*, dp: bool, dropout: float, allow_graph: bool, fused_step: bool, steps: int, mapped: bool,
                poll: bool, dp_graphs: bool) -> Launch:
    """The launch path of one epoch, from its facts.  Dropout: a fresh mask per step (a replayed graph would repeat
    one).  Data-parallel: eager - as fast as graphs (0.246 against 0.249 ms per step on one rank over RCCL) and no
    stream capture beside RCCL's threads - unless GCN_MAXCUT_DP_GRAPHS=1 (``dp_graphs``).  An engine without the
    fused ``train_step`` runs the same sequence, whose all-reduce is then a no-op.  Otherwise the fused
    ``train_step``: several steps are captured once into a hipGraph (no per-launch host cost); ONE step runs eager
    when its losses can be stored into pinned slots (``mapped``) that the host watches (``poll``), so the host
    queues the next step behind this step's backward (0.2259 against 0.2288 ms for a graph replay per step)."""
    if dropout > 0.0:
        return Launch.DROPOUT
    if dp or not fused_step:
        return Launch.DP_GRAPHS if dp and allow_graph and dp_graphs else Launch.DP
    direct = mapped and poll
    if allow_graph and (steps > 1 or steps == 1 and not direct):
        return Launch.GRAPH
    return Launch.DIRECT if direct else Launch.COPY


class FusedTrainer:
    """Device-resident state of one (model, optimizer) pair: per-step graph batches, loss
    slots, and the bridge that exposes the fused Adam moments through the torch optimizer
    (so ``optimizer.state_dict()`` has the reference's layout)."""

    def __init__(self, net, optimizer, config, graphs_per_step: int = 1,
                 local_shard: bool = False, engine=None, loss: Optional[str] = None):
        self.net, self.optimizer, self.config = net, optimizer, config
        # "cut" (the reference's hard loss) or "expected_cut" (the relaxed one); None: GCN_MAXCUT_LOSS.  Every launch
        # path takes it; an engine is handed the keyword only when it is not the default (stand-ins without it work)
        self.loss = hip.loss_name(loss)
        self._loss_kw = {} if self.loss == "cut" else {"loss": self.loss}
        self.eng = engine if engine is not None else net.engine()
        self.graphs_per_step = graphs_per_step
        # local_shard: `dataset` already is this rank's shard (graphs_per_step of ITS graphs per
        # step); otherwise every rank holds the whole dataset and takes its slice of each group
        self.local_shard = local_shard
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        # dp: steps run the data-parallel sequence (shard step -> all-reduce -> Adam).  More than one rank, or a
        # single rank asked to (GCN_MAXCUT_DP_SINGLE_RANK=1: RCCL and the graphs around it on a one-GPU box)
        self.dp = dp_active()
        if self.dp:
            self.eng.sync_replicas(0)   # one model: rank 0's parameters / moments on every replica
        # what the engine offers: the fused step; scratch, slab copy of W1, device-stepped Adam (not host stand-ins)
        # (a number_classes != 3 engine has neither the fused step nor the slab copy: train_fwd_bwd -> Adam, eager)
        # (the attention engine - layer1 = "attention" - likewise: gmc_att_train_fwd_bwd -> Adam, eager, six tensors)
        self._attention = bool(getattr(self.eng, "attention", False))
        self._kway = bool(getattr(self.eng, "kway", False)) or self._attention
        self._fused_step = hasattr(self.eng, "train_step") and not self._kway
        self._slab = not self._kway
        self._hip = hasattr(self.eng, "adam_step_dev")
        # does the planned dataset hold a batch beyond the one-workgroup head (FusedEngine.needs_large)?  Decided per
        # DATASET in prepare(): every step of such a dataset then runs train_fwd_bwd -> Adam, eager, without the slab copy
        # (the path the K-class engine takes), so that an epoch's losses come back one way
        self._large = False
        self._dp_graphs_env = os.environ.get("GCN_MAXCUT_DP_GRAPHS", "0") == "1"
        self._plan_key = None
        self._ws: Optional[torch.Tensor] = None   # scratch of this trainer's steps (captured graphs point into it)
        self._graph_key = None
        self._poll = True           # watch the pinned loss slots instead of a stream sync (off after a deadline hit)
        self._dp_graph = None       # (per-step forward/backward hipGraphs, Adam hipGraph) of a data-parallel rank
        self._dp_graph_key = None
        # False: eager launches only (per-kernel probing; an engine off the GPU has no hipGraphs)
        self.allow_graph = self.eng.device.type == "cuda"
        self._graph = None          # hipGraph of one whole epoch (single GPU)
        self._graph_steps = 0
        self._batches: List[GraphBatch] = []
        self._loss_slots: Optional[torch.Tensor] = None
        self._loss_host: Optional[torch.Tensor] = None
        self._step_host: Optional[torch.Tensor] = None
        self._out = None
        self.last_enqueue_s = 0.0
        self.deadline_hits = 0      # epochs whose losses did not land within the polling deadline (see _landed)

    def invalidate(self) -> None:
        """Forget the planned batches (and the captured hipGraphs with them): the next epoch walks the dataset
        again.  Call it after editing a dataset dict in a way :meth:`prepare` cannot see (see there)."""
        self._plan_key = None
        self._graph = None
        self._dp_graph = None

    def prepare(self, dataset: Dict) -> None:
        """Plan the device batches for ``dataset`` once and keep them while it is the same dataset.  "The same" is
        decided cheaply per epoch (the reference re-reads ``dataset.items()`` every epoch, TrainingNeural.py:371; a
        full walk per 0.2 ms step would cost more than the step): the dict object and its length, plus - for every
        item of a small dataset (<= 32 items), else for the first, the last and six evenly spaced items - the
        identity of the graph handle and of the adjacency tensor and the tensor's in-place version counter.
        Replacing or editing an item those probes miss needs :meth:`invalidate`."""
        probe = None
        if dataset:
            n_items = len(dataset)
            if n_items <= 32 or not hasattr(dataset, "__reversed__"):
                picked = list(dataset.values()) if n_items <= 32 else [next(iter(dataset.values()))]
            else:
                keys = list(dataset)   # (a list of 160 ints: ~1 us)
                picked = [dataset[keys[(n_items - 1) * j // 7]] for j in range(8)]
            probe = tuple((id(it[0]), id(it[1]), getattr(it[1], "_version", 0)) for it in picked)
        key = (id(dataset), len(dataset), self.graphs_per_step, self.world, probe)
        if key == self._plan_key:
            return
        items = list(dataset.values())
        gps, dev = self.graphs_per_step, self.eng.device
        self._batches = []
        stride = gps if self.local_shard else gps * self.world
        for start in range(0, len(items), stride):
            group = items[start:start + stride]
            # this rank's contiguous share of the group, balanced by directed edges (== by count for equal graphs)
            mine = group if self.local_shard else [group[i] for i in shard_by_weight(
                [it[0].number_of_edges() for it in group], self.rank, self.world)]
            handles = [it[0] for it in mine]
            vals = [h.edge_values(it[1]) for h, it in zip(handles, mine)]
            self._batches.append(self.eng.make_batch(handles, vals))
        self._large = hasattr(self.eng, "needs_large") and any(self.eng.needs_large(b, self.loss)
                                                                 for b in self._batches if b.B)
        rmax = max((b.R for b in self._batches), default=0)
        bmax = max((b.B for b in self._batches), default=0)
        self._out = (torch.empty((rmax, int(getattr(self.eng, "K", 3))), dtype=torch.float32, device=dev),
                     torch.empty(rmax, dtype=torch.int32, device=dev))
        self._loss_slots = torch.zeros((len(self._batches), max(bmax, 1)), dtype=torch.float32, device=dev)
        self._step_loss = torch.zeros(len(self._batches), dtype=torch.float32, device=dev)
        # pinned landing buffer of the per-graph losses: the copy is enqueued behind the epoch's
        # kernels (inside the replayed hipGraph on one GPU), the host then waits on one event
        self._loss_host = (torch.empty_like(self._loss_slots, device="cpu").pin_memory()
                           if dev.type == "cuda" else None)
        self._loss_host_np = self._loss_host.numpy() if self._loss_host is not None else None   # (shares the pinned memory)
        self._loss_host_bits = self._loss_host_np.view(np.uint32) if self._loss_host_np is not None else None
        self._loss_rows = ([(self._loss_host_bits[i, :b.B], self._loss_host_np[i, :b.B])   # (bits, values) of each step
                            for i, b in enumerate(self._batches) if b.B] if self._loss_host is not None else [])
        # device-side address of that pinned buffer (None when the runtime cannot map it, or polling is off): the
        # steps store their per-graph losses straight into it (one system-scope store each, as soon as the value is
        # final), so the host has a step's loss while its backward is still running and no copy node trails the graph
        self._loss_host_dev = hip.mapped_ptr(self._loss_host) if self._loss_host is not None and self._poll else None
        self._step_host = (torch.empty_like(self._step_loss, device="cpu").pin_memory()
                           if dev.type == "cuda" else None)
        self._step_host_np = self._step_host.numpy() if self._step_host is not None else None
        self._step_host_bits = self._step_host_np.view(np.uint32) if self._step_host_np is not None else None
        # data-parallel steps: the all-reduced loss of a step (the gradient's tail slot) is published to this pinned
        # buffer by a one-wave launch BEFORE the step's Adam launches, so the host has it while Adam still runs
        self._step_host_dev = hip.mapped_ptr(self._step_host) if self._step_host is not None and self._poll else None
        # private scratch, sized for the largest step: the engine's own scratch is re-allocated whenever a
        # later call (evaluate_model on a bigger batch, another trainer) needs more, which would leave a
        # captured hipGraph replaying into freed memory
        if self._hip and self._batches:
            drop = 0.0 if self._kway else float(getattr(self.net, "dropout_frac", 0.0) or 0.0)   # (K-class: no dropout)
            with self.eng.dropout(drop, 0):   # the dropout sequence needs a little more scratch: size for it
                need = max((self.eng.workspace_bytes(b, True) for b in self._batches if b.B), default=0)
            if need and (self._ws is None or self._ws.numel() < need):
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self._plan_key = key
        self._graph = None
        self._dp_graph = None

    def _hyper(self):
        """(lr, betas, eps) of the step: the optimizer's first param group, as ``optimizer.step()`` would use
        (TrainingNeural.py:337,386); the config's learning rate when the optimizer carries none."""
        groups = getattr(self.optimizer, "param_groups", None)
        if groups:
            g = groups[0]
            return float(g.get("lr", self.config.learning_rate)), tuple(g.get("betas", (0.9, 0.999))), float(g.get("eps", 1e-8))
        return float(self.config.learning_rate), (0.9, 0.999), 1e-8

    def _dropout(self) -> float:
        """p of F.dropout for this epoch's steps (TrainingNeural.py:82): the model's, in train mode."""
        return float(getattr(self.net, "dropout_frac", 0.0)) if getattr(self.net, "training", False) else 0.0

    def epoch(self, dataset: Dict) -> float:
        """One pass over the dataset; returns the cumulative loss (one host sync)."""
        t_entry = perf_counter()
        if self._attention and self._dropout() > 0.0:
            raise NotImplementedError("dropout is implemented for layer1 = 'graphconv' only (this model has layer1 = "
                                      "'attention'): train it with dropout = 0")
        if self._kway and self._dropout() > 0.0:
            raise NotImplementedError(f"dropout is implemented for number_classes = 3 only (this model has number_classes "
                                      f"= {self.eng.K}): train it with dropout = 0")
        self.prepare(dataset)
        drop = self._dropout()
        path = launch_path(dp=self.dp, dropout=drop, allow_graph=self.allow_graph,
                           fused_step=self._fused_step and not self._large,
                           steps=len(self._batches), mapped=self._loss_host_dev is not None, poll=self._poll,
                           dp_graphs=self._dp_graphs_env and not self._kway and not self._large)
        if path is Launch.DROPOUT:
            self._run_dropout(drop)
        elif path is Launch.DP or path is Launch.DP_GRAPHS:
            self._run_dp(graphs=path is Launch.DP_GRAPHS)
        elif path is Launch.GRAPH:
            self._run_graph()
        else:
            self._run_eager(direct=path is Launch.DIRECT)
        self.last_enqueue_s = perf_counter() - t_entry   # host time to queue the epoch's launches (bench.py reports it)
        if path is Launch.DROPOUT:
            return float(self._step_loss.cpu().numpy().sum(dtype=np.float64))
        if path is Launch.DP or path is Launch.DP_GRAPHS:
            return self._step_losses()
        return self._slot_losses(copy=path is Launch.COPY)

    # ---- launch paths (launch_path says which one an epoch takes)
    def _run_dropout(self, drop: float) -> None:
        """The one-kernel-per-operation sequence with a fresh dropout mask per step."""
        eng, cfg = self.eng, self.config
        lr, betas, eps = self._hyper()
        tail = eng.grad[eng.count:eng.count + 1]
        for i, batch in enumerate(self._batches):
            eng.set_dropout(drop)
            if batch.B == 0:
                eng.grad[:eng.count + 1].zero_()
            else:
                eng.train_fwd_bwd(batch, cfg.C, out=(self._out[0], self._out[1], self._loss_slots[i]), ws=self._ws,
                                  **self._loss_kw)
            if self.dp:
                eng.allreduce_grad()
            self._step_loss[i:i + 1].copy_(tail)
            eng.adam_step(lr, betas, eps)
        eng.set_dropout(0.0)

    def _run_eager(self, direct: bool) -> None:
        """Eager train_step launches; ``direct``: the losses are stored straight into the pinned host slots, so the
        host is back as soon as the loss kernels have run and queues the next step behind this step's backward."""
        if direct:
            _arm(self._loss_host_bits)
        self.eng.sync_step_dev()
        self._train_steps(self._loss_host_dev if direct else None)

    def _run_graph(self) -> None:
        """Replay the epoch's hipGraph (captured on the first epoch, which itself runs eager)."""
        eng = self.eng
        if self._poll:
            _arm(self._loss_host_bits)
        eng.sync_step_dev()   # (no launch while this trainer's replays are the only thing stepping the optimizer)
        # the captured launches carry lr / betas / eps / C and the scratch pointer as kernel arguments
        key = (self._hyper(), float(self.config.C), self._ws.data_ptr() if self._ws is not None else 0)
        if self._graph is not None and key != self._graph_key:
            self._graph = None
        self._graph_key = key
        if self._graph is None:
            self._train_steps(None)               # eager epoch: sizes the workspace, warms the kernels
            graph = torch.cuda.CUDAGraph()
            before = eng.step_count
            with torch.cuda.graph(graph):
                self._train_steps(self._loss_host_dev)
                if self._loss_host_dev is None:   # the graph ends with the copy of the losses
                    self._loss_host.copy_(self._loss_slots, non_blocking=True)
            eng.step_count = eng._dev_step = before   # capture enqueued nothing
            self._graph, self._graph_steps = graph, len(self._batches)
            self._loss_host.copy_(self._loss_slots, non_blocking=True)   # this (eager) epoch's losses
            return
        eng.ensure_slab()   # (a launch only when torch wrote the parameters since the last replay)
        self._graph.replay()
        eng.step_count += self._graph_steps
        eng._dev_step += self._graph_steps

    def _train_steps(self, loss_dev: Optional[int]) -> None:
        """One fused train_step launch per step; ``loss_dev``: device address of the pinned slots that get the losses."""
        eng, cfg = self.eng, self.config
        lr, betas, eps = self._hyper()
        row_bytes = self._loss_slots.shape[1] * 4
        for i, batch in enumerate(self._batches):
            eng.train_step(batch, lr, cfg.C, out=(self._out[0], self._out[1], self._loss_slots[i]), betas=betas, eps=eps,
                           ws=self._ws, slab=True, loss_ptr=loss_dev + i * row_bytes if loss_dev else None,
                           **self._loss_kw)

    def _run_dp(self, graphs: bool) -> None:
        """Shard step, ONE RCCL all-reduce of [gradient | loss], Adam.  The step's loss rides in the all-reduce (the
        slot after the gradient, GMC_MODEL_GRAD_TAIL) and reaches pinned slot i ahead of the step's Adam: fused into
        the Adam launch (eager), a publish launch (``graphs``), or a device copy when the slots are not mapped."""
        eng, cfg = self.eng, self.config
        tail = eng.grad[eng.count:eng.count + 1]
        last = len(self._batches) - 1
        lr, betas, eps = self._hyper()
        slab = self._slab and not self._large
        publish = self._step_host_dev
        if self._poll and self._step_host is not None:
            _arm(self._step_host_bits)
        if graphs:
            fwd_bwd, adam = self._dp_graphs()
            eng.sync_step_dev()
            eng.ensure_slab()   # (a launch only when torch wrote the parameters since the last step)
        for i, batch in enumerate(self._batches):
            if batch.B == 0:
                # this rank's shard of the step is empty (last group smaller than the world): it
                # contributes a zero gradient and a ZERO loss - the tail slot still holds the previous
                # step's all-reduced loss and would otherwise be added once more per empty rank
                eng.grad[:eng.count + 1].zero_()
            elif graphs:
                fwd_bwd[i].replay()                   # forward + loss + backward + gradient fold of my shard
            elif self._hip:
                eng.train_fwd_bwd(batch, cfg.C, out=(self._out[0], self._out[1], self._loss_slots[i]), ws=self._ws,
                                  slab=slab, **self._loss_kw)
            else:
                eng.train_fwd_bwd(batch, cfg.C, out=(self._out[0], self._out[1], self._loss_slots[i]), **self._loss_kw)
            eng.allreduce_grad()                      # ONE RCCL all-reduce of [gradient | loss] per step, eager
            if not publish and i != last:             # (the last step's slot is read in place: _step_losses)
                self._step_loss[i:i + 1].copy_(tail)
            if graphs:
                if publish:
                    eng.publish(tail, publish + 4 * i)
                adam.replay()                         # Adam, step number read from / advanced in device memory
                eng.step_count += 1
                eng._dev_step += 1
            elif self._hip:
                eng.sync_step_dev()                   # (a launch only after host-stepped updates)
                # keeps the slab copy of W1 current; with `publish`: loss store + counter tick + Adam in two launches
                eng.adam_step_dev(lr, betas, eps, slab=slab,
                                  publish=(tail, publish + 4 * i) if publish else None)
            else:
                eng.adam_step(lr, betas, eps)

    def _dp_graphs(self):
        eng, cfg = self.eng, self.config
        hyper = self._hyper()
        key = (hyper, float(cfg.C), self._ws.data_ptr() if self._ws is not None else 0)
        if self._dp_graph is not None and self._dp_graph_key == key:
            return self._dp_graph
        lr, betas, eps = hyper
        fb = []
        for i, batch in enumerate(self._batches):
            if batch.B == 0:
                fb.append(None)
                continue
            out = (self._out[0], self._out[1], self._loss_slots[i])
            eng.train_fwd_bwd(batch, cfg.C, out=out, ws=self._ws, slab=True, **self._loss_kw)   # eager once: warms the kernels
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                eng.train_fwd_bwd(batch, cfg.C, out=out, ws=self._ws, slab=True, **self._loss_kw)
            fb.append(g)
        before, flat, m, v = eng.step_count, eng.flat.clone(), eng.m.clone(), eng.v.clone()
        eng.sync_step_dev()
        eng.adam_step_dev(lr, betas, eps, slab=True)                # eager once (state restored below)
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            eng.adam_step_dev(lr, betas, eps, slab=True)
        eng.flat.copy_(flat); eng.m.copy_(m); eng.v.copy_(v)
        eng.step_count = before
        eng._dev_step = -1                                          # (the capture pass counted on the host only)
        eng.sync_step_dev()
        self._dp_graph, self._dp_graph_key = (fb, ga), key
        return self._dp_graph

    # ---- the epoch's loss (one host sync)
    def _slot_losses(self, copy: bool) -> float:
        """Cumulative loss of a single-GPU epoch: the reference adds one float per optimizer step (loss.item(),
        :388), each the sum of that step's per-graph losses.  ``copy``: the losses are still in the device slots."""
        if self._loss_host is None:
            host = self._loss_slots.cpu().numpy()
            rows = [host[i, :b.B] for i, b in enumerate(self._batches)]
        elif not copy and self._poll:
            rows = self._landed(self._loss_rows)   # (each step's sum is taken while the later steps still run)
        else:
            if copy:
                self._loss_host.copy_(self._loss_slots, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            rows = [values for _bits, values in self._loss_rows]
        total = 0.0
        for values in rows:
            total += float(values.sum(dtype=np.float32))
        return total

    def _step_losses(self) -> float:
        """Cumulative loss of a data-parallel epoch: the sum of the steps' all-reduced losses."""
        if not self._batches:
            return 0.0
        eng, last = self.eng, len(self._batches) - 1
        tail = eng.grad[eng.count:eng.count + 1]
        if self._step_host is None:
            self._step_loss[last:last + 1].copy_(tail)
            return float(sum(self._step_loss.cpu().tolist()))
        if not self._step_host_dev:
            if last == 0:   # one step per epoch: its loss goes from the gradient's tail slot to the host
                self._step_host.copy_(tail, non_blocking=True)
            else:
                self._step_loss[last:last + 1].copy_(tail)
                self._step_host.copy_(self._step_loss, non_blocking=True)
        if self._poll:
            host, = self._landed([(self._step_host_bits, self._step_host_np)])
        else:
            torch.cuda.current_stream().synchronize()
            host = self._step_host_np
        return float(host.sum(dtype=np.float64))

    def _landed(self, rows):
        """Yield the values of each (bits, values) row of pinned host slots (``bits`` armed with :func:`_arm`) as soon
        as every slot of it holds a loss.  The losses are stored there by the loss kernels or by a copy behind the
        epoch's launches: the host watches that memory instead of sleeping in hipStreamSynchronize (whose wake-up
        costs ~10 us per step of a 0.25 ms step).  After ~0.5 ms of spinning the loop yields the core between looks
        (RCCL's proxy threads and the other ranks' hosts share it).  Slots that have not landed within
        `_POLL_DEADLINE_S` hand over to the stream synchronisation - which reports whatever went wrong on the device,
        and after which the slots hold the result - and polling is switched off for the rest of the run with ONE
        warning (e.g. pinned memory that is not host-coherent: every epoch would otherwise pay the deadline)."""
        deadline, synced = None, False
        for bits, values in rows:
            spins = 0
            while not synced and (bits[-1] == _NOT_LANDED or bits[0] == _NOT_LANDED or (bits == _NOT_LANDED).any()):
                spins += 1
                if spins > _SPIN_BEFORE_YIELD and spins & 63 == 0:
                    sleep(0)
                    now = time()
                    deadline = deadline or now + _POLL_DEADLINE_S
                    if now > deadline:
                        torch.cuda.current_stream().synchronize()   # (raises if the device faulted)
                        self.deadline_hits += 1
                        self._poll = False
                        warnings.warn("GCN max-cut: the step's losses did not reach the pinned host buffer within "
                                      f"{_POLL_DEADLINE_S:.0f} s of polling; falling back to stream synchronisation for "
                                      "the rest of this run (is the pinned memory host-coherent? HIP_HOST_COHERENT=0 "
                                      "breaks zero-copy stores)")
                        synced = True
            yield values

    def sync_optimizer_state(self) -> None:
        """Expose step / exp_avg / exp_avg_sq of the fused Adam through ``optimizer.state``."""
        if self.eng.step_count == 0:
            return
        named = dict(self.net.named_parameters())
        mv, vv = self.eng.views(self.eng.m), self.eng.views(self.eng.v)
        for k in getattr(self.eng, "param_order", PARAM_ORDER):
            self.optimizer.state[named[k]] = {
                'step': torch.tensor(float(self.eng.step_count)),
                'exp_avg': mv[k], 'exp_avg_sq': vv[k]}
