"""Shared parts of the bounds tests (tests/test_gpu_bounds_*.py): the four batches, a memory source that hands every
device buffer of a call out either as a plain torch tensor or from a guard-band arena (tests/arena.py), and the runner
that makes one case's calls three times - plain, arena filled 0xFF, arena filled 0x00 - and asserts, in this order:

 1. every call returned GMC_OK in all three runs;
 2. no band of either arena was touched (nothing written outside a buffer);
 3. every input buffer still holds, byte for byte, what was uploaded (the header's `const`);
 4. every output of the 0xFF run equals the 0x00 run equals the plain run, byte for byte (a read beyond a buffer that
    reaches a result would make the NaN / 255 run and the 0 run differ).

A case is a function ``case(lib, mem)`` that obtains EVERY piece of device memory from ``mem`` - the batch's arrays, the
model's, inputs, outputs and the workspace at exactly the size the query returns - and returns the status codes of its
calls.  No assertion here has a tolerance: every one is an equality of bytes.
"""
import ctypes as C
import functools

import numpy as np
import torch

from tests import arena as A
from tests import util

CALLS = {"cases": 0, "calls": 0}          # what the process made so far (each case's calls are made three times)


def report_calls(label):
    """For a module-scoped fixture: ``done = report_calls(label)`` at set-up, ``done()`` at tear-down prints the cases
    and calls the module's tests made in between (shown with -s; DESIGN.md section 37 quotes them)."""
    before = dict(CALLS)
    return lambda: print(f"\n{label}: {CALLS['cases'] - before['cases']} cases, {CALLS['calls'] - before['calls']} calls")


# ---- the batches -------------------------------------------------------------------------------------------------------
def _real_weights(g, seed):
    """Full-mantissa float32 weights in 0.1 .. 2, one per undirected edge (so equal on both entries of an edge)."""
    rng = np.random.RandomState(seed)
    for u, v in g.edges():
        g[u][v]["weight"] = float(np.float32(rng.uniform(0.1, 2.0)))
    return g


@functools.lru_cache(maxsize=None)
def graphs_of(kind):
    """odd: n = 5, 67, 13 (R = 85: nothing a multiple of 4; 67 crosses a wave), 3-regular or nearest, unit weights.
    hub: n = 131 with node 5 raised to degree 70 (a row of more than 64 entries, overflow lists in the table) plus
    n = 9, real weights.  tile: n = 257 plus n = 8 (crosses the 256-row tiles of csrc/large.hip).  trip: n = 1030, d = 3
    (the second trip of a 1024-thread head's row loop).  pins: n = 67 (unit weights) plus the hub graph (real weights),
    for the contraction at K = 8."""
    if kind in ("odd", "odd9"):   # odd9 (R = 89): for 8 terminals per graph, which the n = 5 graph cannot hold
        return tuple(util.near_regular(n, 3, 100 + n, attrs=False) for n in ((5 if kind == "odd" else 9), 67, 13))
    if kind == "hub":
        big = util.add_hub(util.near_regular(131, 3, 231, attrs=False), 70, 7, attrs=False)
        return (_real_weights(big, 1), _real_weights(util.near_regular(9, 3, 109, attrs=False), 2))
    if kind == "tile":
        return (util.near_regular(257, 3, 357, attrs=False), util.near_regular(8, 3, 108, attrs=False))
    if kind == "trip":
        return (util.near_regular(1030, 3, 1130, attrs=False),)
    if kind == "pins":            # the n = 67 graph of `odd` and the hub graph: room for 8 pinned classes in each
        return (graphs_of("odd")[1], graphs_of("hub")[0])
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def host_batch(kind):
    """gcn-max-cut_amd/graph.py's BatchArrays (host numpy, the table and overflow lists included) of a batch."""
    import gcn_max_cut_amd as pkg
    hs = [pkg.graph.from_networkx(g) for g in graphs_of(kind)]
    h = pkg.graph.BatchArrays(hs)
    h.handles = hs
    assert int(np.diff(h.rowptr).min()) > 0
    if kind == "hub":
        assert h.max_degree == 70 and h.ovf_ptr is not None and h.vals is not None and h.ovf_vals is not None
    return h


BATCH_ARRAYS = ("goff", "rowptr", "gcol", "lcol", "vals", "dinv", "ell", "ell_vals", "ovf_ptr", "ovf_ids", "ovf_vals")


def device_batch(pkg, mem, h, table=True, nnz_max=None):
    """The gmc_batch of host arrays `h` with every array taken from `mem` (table: with the ELL table and the overflow
    lists; nnz_max: overstated, the global-CSR variant of the chain searches)."""
    t = {}
    for name in BATCH_ARRAYS:
        a = getattr(h, name)
        if a is None or (not table and name.startswith(("ell", "ovf"))):
            t[name] = None
            continue
        if name == "goff":
            a = a.astype(np.int32)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        t[name] = mem.put("batch." + name, a)
    p = pkg.hip.ptr
    c = pkg.hip.GmcBatch(B=h.B, R=h.R, nnz=h.nnz, n_max=h.n_max, uniform_n=h.uniform_n,
                         nnz_max=h.nnz_max if nnz_max is None else nnz_max,
                         ell_width=h.ell_width if table else 0, ell_slots=h.ell_slots if table else 0,
                         ovf_max_blocks=h.ovf_max_blocks if table else 0, **{k: p(v) for k, v in t.items()})
    mem.keep.append(c)
    return c


def model_arrays(N, F, K, seed, per_graph=None):
    """W1, b1, W2, b2 of a seeded model; per_graph = (R, B): the stacked blocks of one model per graph."""
    rng = np.random.RandomState(seed)
    u = lambda *s: rng.uniform(-0.5, 0.5, s).astype(np.float32)
    if per_graph:
        R, B = per_graph
        return dict(W1=u(R, F), b1=u(B, F), W2=u(B, F, K), b2=u(B, K))
    return dict(W1=u(N, F), b1=u(F), W2=u(F, K), b2=u(K))


def device_model(pkg, mem, arrs, N, F, K, flags=0, slab=False, dropout=0.0):
    t = {k: mem.put("model." + k, v) for k, v in arrs.items()}
    s = mem.put("model.W1_slab", util._slab_of(arrs["W1"])) if slab else None
    p = pkg.hip.ptr
    m = pkg.hip.GmcModel(N=N, F=F, K=K, flags=flags, W1=p(t["W1"]), b1=p(t["b1"]), W2=p(t["W2"]), b2=p(t["b2"]),
                         dropout_p=dropout, dropout_seed_lo=12345, dropout_seed_hi=678, W1_slab=p(s))
    mem.keep.append(m)
    return m


# ---- the memory source ---------------------------------------------------------------------------------------------------
_ITEM = {torch.float32: 4, torch.int32: 4, torch.int8: 1, torch.uint8: 1, torch.int16: 2, torch.int64: 8,
         torch.float64: 8}


class Mem:
    """Hands out device buffers: `put` uploads a host array as an INPUT (checked unchanged afterwards), `state` uploads
    one the call updates in place (an output), `out` gives an uninitialised output, `scratch` uninitialised memory that
    is not compared (the workspace).  arena = None: plain torch tensors, uninitialised ones filled 0xFF."""

    def __init__(self, arena=None):
        self.arena = arena
        self.inputs, self.outputs, self.sizes, self.keep = {}, {}, [], []

    def _name(self, name, table):
        assert name not in table, name
        return name

    def _take(self, name, what, dtype=None):
        if isinstance(what, np.ndarray):
            nbytes = what.nbytes
        else:
            what = tuple(int(s) for s in (what if isinstance(what, (tuple, list)) else (what,)))
            nbytes = int(np.prod(what, dtype=np.int64)) * _ITEM[dtype]
        self.sizes.append(nbytes)
        if self.arena is not None:
            return self.arena.take(name, what, dtype)
        if isinstance(what, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(what)).cuda()
        return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda").view(dtype).reshape(what)

    def put(self, name, array):
        t = self._take(self._name(name, self.inputs), array)
        self.inputs[name] = (t, np.ascontiguousarray(array).tobytes())
        return t

    def state(self, name, array):
        t = self._take(self._name(name, self.outputs), array)
        self.outputs[name] = t
        return t

    def out(self, name, shape, dtype=torch.float32):
        t = self._take(self._name(name, self.outputs), shape, dtype)
        self.outputs[name] = t
        return t

    def scratch(self, name, nbytes):
        t = self._take(name, (int(nbytes),), torch.uint8)
        self.keep.append(t)               # (a plain tensor nobody holds would be freed and its block handed out again)
        return t


def bytes_of(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def _first_difference(a, b):
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    if x.size != y.size:
        return f"sizes {x.size} and {y.size}"
    bad = np.flatnonzero(x != y)
    return f"{bad.size} bytes differ, the first at byte {int(bad[0])}"


def run_case(pkg, case, unwritten=(), padded=None):
    """One case, three times; the assertions of the module docstring.  `unwritten`: outputs the call documents as left
    alone in part - the entries behind the kept ones of a build with refused entries - whose bytes depend on the fill:
    they are compared between the plain and the 0xFF run only, both pre-filled 0xFF.  `padded`: {name: N} for a 2-D
    output [rows, ld] whose matrix is the first N columns: those are compared, and the pad columns must still hold the
    fill in every run (they are outside the matrix, so the call must not write them either)."""
    padded = padded or {}
    lib = pkg.hip.load()
    runs = []
    for fill in (None,) + A.FILLS:
        arena = None if fill is None else A.Arena("cuda", fill, A.capacity_for(runs[0][0].sizes))
        mem = Mem(arena)
        torch.cuda.synchronize()
        rcs = case(lib, mem)
        torch.cuda.synchronize()
        runs.append((mem, list(rcs) if isinstance(rcs, (list, tuple)) else [rcs]))
    CALLS["cases"] += 1
    CALLS["calls"] += 3 * len(runs[0][1])
    tags = ("plain", "0xFF", "0x00")
    for tag, (mem, rcs) in zip(tags, runs):
        assert all(rc == 0 for rc in rcs), (tag, rcs)
    for tag, (mem, rcs) in zip(tags[1:], runs[1:]):
        assert mem.arena.check() == [], (tag, mem.arena.check())
    for tag, (mem, rcs) in zip(tags, runs):
        for name, (t, want) in mem.inputs.items():
            got = bytes_of(t)
            assert got == want, (tag, "input changed", name, _first_difference(got, want))
    plain, ff, zero = (m for m, _ in runs)
    assert set(plain.outputs) == set(ff.outputs) == set(zero.outputs)
    for name in plain.outputs:
        ta, tb, tc = plain.outputs[name], ff.outputs[name], zero.outputs[name]
        if name in padded:
            n = padded[name]
            for t, fill in ((ta, 0xFF), (tb, 0xFF), (tc, 0x00)):
                pad = t[:, n:].contiguous().reshape(-1).view(torch.uint8)
                assert bool((pad == fill).all()), ("a pad column was written", name)
            ta, tb, tc = (t[:, :n].contiguous() for t in (ta, tb, tc))
        a, b, c = bytes_of(ta), bytes_of(tb), bytes_of(tc)
        if name not in unwritten:
            assert b == c, ("0xFF run != 0x00 run: a read beyond a buffer", name, _first_difference(b, c))
        assert a == b, ("plain run != 0xFF run: not reproducible", name, _first_difference(a, b))
    return runs


def check_can_fail(pkg, case, buffer):
    """After a clean call, one byte of a band set through the arena's own tensor is reported with the buffer's name and
    the offset - the check of run_case can fail."""
    lib = pkg.hip.load()
    probe = Mem(None)
    case(lib, probe)
    torch.cuda.synchronize()
    arena = A.Arena("cuda", 0xFF, A.capacity_for(probe.sizes))
    mem = Mem(arena)
    rcs = case(lib, mem)
    torch.cuda.synchronize()
    assert all(rc == 0 for rc in (rcs if isinstance(rcs, (list, tuple)) else [rcs])) and arena.check() == []
    name, start, end = next(r for r in arena.regions if r[0] == buffer)
    arena.mem[end + 3] = 0x12
    assert arena.check() == [(buffer, "after", end - start + 3, 1)]
    arena.mem[end + 3] = 0xFF
    arena.mem[start - 16:start - 12] = 0
    assert arena.check() == [(buffer, "before", -16, 4)]


def stream(pkg):
    return pkg.hip.stream()
