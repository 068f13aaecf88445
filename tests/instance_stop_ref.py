"""Restatement, in numpy and Python, of per-graph early stopping for one model per graph (include/gcnmaxcut.h,
gmc_inst_early_stop_f32 and gmc_inst_adam_f32):

* `reference_loop`: the reference's own loop (`train_model`, TrainingNeural.py:429-444) for ONE graph, transcribed
  literally in Python floats - what the rule is restated from;
* `StopRule`: the rule for a batch, call by call as the device runs it, composed with `instance_ref.KeepBest` (a graph
  that may not take part in keep-best is shown a NaN loss, which never wins);
* `segments` / `adam_f64_masked`: the flat layout cut by graph and a float64 Adam step that passes stopped graphs by;
* `SEQUENCES`: the made-up loss sequences both the host test and the GPU test feed, with what they must give."""
import collections

import numpy as np

from tests import instance_ref as IR

INF, NAN = float("inf"), float("nan")


# ---- the reference, literally (one graph, Python floats of float32 losses)
def reference_loop(losses, tolerance, patience):
    """(stopped_epoch or None, best_loss, best_epoch, patience_counter, prev_loss) of train_model's loop over
    ``losses``."""
    best_loss, best_epoch = float('inf'), -1
    patience_counter, prev_loss = 0, float('inf')
    stopped = None
    for epoch, cumulative_loss in enumerate(float(np.float32(x)) for x in losses):
        stalled = cumulative_loss > prev_loss or abs(prev_loss - cumulative_loss) <= tolerance
        if epoch > 0 and stalled:
            patience_counter += 1
            if patience_counter >= patience:
                stopped = epoch
                break
        else:
            patience_counter = 0
        if cumulative_loss < best_loss:
            best_loss, best_epoch = cumulative_loss, epoch
        prev_loss = cumulative_loss
    return stopped, best_loss, best_epoch, patience_counter, prev_loss


# ---- the rule for a batch
class StopRule:
    """prev_loss / stall / stop_epoch and, through ``keep`` (an `instance_ref.KeepBest`), best_S / best_loss / best_epoch
    of a batch under the rule of include/gcnmaxcut.h."""

    def __init__(self, goff, tolerance, patience):
        self.keep = IR.KeepBest(goff)
        B = len(self.keep.best_loss)
        self.tolerance, self.patience = float(tolerance), int(patience)
        self.prev_loss = np.full(B, np.inf, np.float32)
        self.stall = np.zeros(B, np.int32)
        self.stop_epoch = np.full(B, -1, np.int32)

    best_S = property(lambda self: self.keep.best_S)
    best_loss = property(lambda self: self.keep.best_loss)
    best_epoch = property(lambda self: self.keep.best_epoch)

    def update(self, S, loss, epoch):
        loss = np.asarray(loss, np.float32)
        shown = loss.copy()                       # what keep-best sees: NaN for a graph that is stopped or stops now
        for g in range(len(loss)):
            if self.stop_epoch[g] >= 0:
                shown[g] = np.nan
                continue
            L, p = float(loss[g]), float(self.prev_loss[g])
            if epoch > 0 and (L > p or abs(p - L) <= self.tolerance):
                self.stall[g] += 1
                if self.stall[g] >= self.patience:
                    self.stop_epoch[g] = epoch
                    shown[g] = np.nan
                    continue
            else:
                self.stall[g] = 0
            self.prev_loss[g] = loss[g]
        self.keep.update(S, shown, epoch)

    def state(self):
        """The six arrays as bytes, in the order the entry point takes them."""
        return tuple(a.tobytes() for a in (self.prev_loss, self.stall, self.stop_epoch, self.best_S, self.best_loss,
                                           self.best_epoch))


def replay(history, tolerance, patience):
    """(stopped_epoch or None, best_loss, best_epoch) the rule gives one graph whose losses were ``history``."""
    rule = StopRule([0, 1], tolerance, patience)
    for e, L in enumerate(history):
        rule.update(np.full(1, e, np.int32), [L], e)
    stop = int(rule.stop_epoch[0])
    return (stop if stop >= 0 else None), float(rule.best_loss[0]), int(rule.best_epoch[0])


# ---- the flat layout cut by graph, and Adam over the running graphs
def segments(sizes, F, K):
    """Per graph, the indices of its floats in the flat [W1 | b1 | W2 | b2] buffer (W1 rows, b1, W2, b2: ascending)."""
    offs = IR.flat_offsets(sizes, F, K)
    out, r0 = [], 0
    for g, n in enumerate(sizes):
        out.append(np.concatenate([np.arange(offs[0] + r0 * F, offs[0] + (r0 + n) * F),
                                   np.arange(offs[1] + g * F, offs[1] + (g + 1) * F),
                                   np.arange(offs[2] + g * F * K, offs[2] + (g + 1) * F * K),
                                   np.arange(offs[3] + g * K, offs[3] + (g + 1) * K)]))
        r0 += n
    return out


def adam_f64_masked(sizes, F, K, param, grad, m, v, t, lr, stopped):
    """(param, m, v) in float64 after Adam step number t over the graphs whose ``stopped`` entry is false; the others'
    floats - and whatever their gradient holds, NaN included - stay out of it."""
    param, m, v = (np.array(a, np.float64) for a in (param, m, v))
    for seg, off in zip(segments(sizes, F, K), stopped):
        if off:
            continue
        m1, v1, upd = IR.adam_f64(m[seg], v[seg], np.asarray(grad, np.float64)[seg], t, lr)
        m[seg], v[seg] = m1, v1
        param[seg] += upd
    return param, m, v


# ---- made-up loss sequences (seven epochs each), grouped by the (tolerance, patience) of their calls
# Seq: losses, the stop epoch (None: runs on), best_loss, best_epoch
Seq = collections.namedtuple("Seq", "name losses stop best_loss best_epoch")
F32 = lambda x: float(np.float32(x))   # noqa: E731
SEQUENCES = {
    (0.25, 2): [
        Seq("rising", [-5, -4, -3, -2, -1, 0, 1], 2, -5.0, 0),
        Seq("flat", [-5] * 7, 2, -5.0, 0),
        Seq("improving by less than the tolerance", [-10, -10.125, -10.25, -10.375, -10.5, -10.625, -10.75], 2, -10.125, 1),
        # -10.0 and -10.25 are float32 values whose difference is exactly the tolerance: <= holds, a stall
        Seq("improving by exactly the tolerance", [-10, -10.25, -10.5, -10.75, -11, -11.25, -11.5], 2, -10.25, 1),
        Seq("improving by more than the tolerance", [-10, -10.5, -11, -11.5, -12, -12.5, -13], None, -13.0, 6),
        # a NaN loss neither stalls nor wins, and the epoch after it compares against NaN: no stall either
        Seq("NaN", [-5, NAN, NAN, -6, -6, -6, -6], 5, -6.0, 3),
        # inf after inf: inf - inf is NaN, no stall; inf after -3 has risen: a stall
        Seq("+inf", [INF, INF, -3, INF, INF, -4, -4], None, -4.0, 5),
        Seq("a stopped graph ignores a later new minimum", [-5, -5, -5, -100, -200, -300, -400], 2, -5.0, 0),
    ],
    (1e-4, 3): [
        Seq("a stall run broken one short of patience", [-5, -5, -5, -6, -6, -6, -6], 6, -6.0, 3),
        # epochs 2 and 3 stall and still enter the best (lower, within the tolerance); epoch 4 stops and does not
        Seq("a lower loss within the tolerance at the stop epoch", [-5, -6, -6.00001, -6.00002, -6.00003, -7, -7], 4,
            F32(-6.00002), 3),
    ],
    (1e-4, 1): [
        Seq("patience = 1", [-5, -6, -6.00001, -9, -9, -9, -9], 2, -6.0, 1),
    ],
    # an infinite tolerance makes every epoch a stall - but for epoch 0, which never is one
    (INF, 1): [
        Seq("epoch 0 never stalls", [-5, -7, -9, -11, -13, -15, -17], 1, -5.0, 0),
    ],
}
EPOCHS = 7
