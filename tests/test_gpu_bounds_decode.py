"""Guard-band tests of the decoders: the one-workgroup samplers, local search, annealing, rounding, evolution, tabu and
balanced search, and the four decoders for graphs beyond one workgroup.  As in tests/test_gpu_bounds_train.py every
array of the batch, every input (probabilities, keys, uniforms, orders, schedules, node costs, size bounds), every
output and the workspace at exactly its query's size comes from one arena with 4096-byte bands (tests/arena.py); each
case runs on plain tensors and on arenas filled 0xFF and 0x00 and tests/bounds.run_case asserts the byte equalities.

The class planes [cands, R] are int8 with R = 85 / 89 / 140 (odd, not a multiple of 4); cands in 1, 3, 70 (70: past one
wave and past cp = 64); K in 2, 5, 8 (row strides of 8, 20 and 32 bytes); terminals 0 and 1; node_cost NULL and real;
optional outputs present and NULL.  Iteration counts are tiny: 3 sweeps, 20 tabu / balance iterations, 2 generations,
5 samples.  A narrower twin (the `_t` of a `_c`, the plain form of a `_t`) gets one case on `odd`.

Measured on the MI355X: 696 cases (2088 calls), no band touched, no pair of runs different.  Alone (-s prints the
counts) the file's 69 tests take 4.1 s, library load and GPU start-up included; the slowest is
test_samplers[gmc_decode_sample_f32] at 0.12 s (the first to touch the GPU), then test_chain_searches[balance-8-70] at
0.05 s.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import bounds as B

pytestmark = pytest.mark.gpu

CLASSES = (2, 5, 8)
CANDS = (1, 3, 70)
SEED = 0xFEEDC0DE1234567
TENURE = (3, 0, 10)
LEVELS = (-np.log((np.arange(1024) + 0.5) / 1024)).astype(np.float32)
SWEEPS, ITERATIONS, GENERATIONS, SAMPLES = 3, 20, 2, 5
I32, I8 = torch.int32, torch.int8


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    done = B.report_calls("bounds/decode")
    yield built
    done()


def kind_for(kind, K, terminals=True):
    return "odd9" if kind == "odd" and terminals and K > 5 else kind


@functools.lru_cache(maxsize=None)
def orders(kind, K, terminals):
    """gmc_order_host_t's arrays at exactly the documented sizes: order [R - first * B], cgoff [B + 1], cptr
    [cgoff[B]], and max_classes."""
    import gcn_max_cut_amd as pkg
    h = B.host_batch(kind)
    order = np.zeros(h.R, np.int32)
    cgoff = np.zeros(h.B + 1, np.int32)
    cptr = np.zeros(h.R + h.B, np.int32)
    classes = C.c_int32(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg.hip.load().gmc_order_host_t(h.B, ptr(h.goff.astype(np.int32)), ptr(h.rowptr), ptr(h.lcol), K, int(terminals),
                                         ptr(order), ptr(cgoff), ptr(cptr), cptr.size, C.byref(classes))
    assert rc == 0, rc
    first = K if terminals else 0
    return order[:h.R - first * h.B].copy(), cgoff, cptr[:int(cgoff[-1])].copy(), int(classes.value)


@functools.lru_cache(maxsize=None)
def inputs(kind, K, cands):
    """Seeded inputs of a (batch, K, cands): probabilities, keys, start partitions, node costs, a schedule."""
    h = B.host_batch(kind)
    rng = np.random.RandomState(1000 * K + cands)
    A = rng.randint(0, K, (cands, h.R)).astype(np.int8)
    for g in range(h.B):
        lo, n = int(h.goff[g]), int(h.sizes[g])
        m = min(K, n)
        A[:, lo:lo + m] = np.arange(m)                      # (harmless without terminals: any class is a start)
    return dict(P=rng.dirichlet(np.ones(K), h.R).astype(np.float32), gkey=rng.randint(1, 2 ** 62, h.B).astype(np.uint64),
                assign=A, cost=rng.uniform(-1, 1, (h.R, K)).astype(np.float32),
                inv_temp=np.linspace(0.5, 3.0, SWEEPS).astype(np.float32))


def chain_shape(kind, K, nnz_max):
    """(chains per workgroup, staged CSR) the two chain searches take for these batches: four chains over the CSR staged
    in LDS; two for `trip` at K = 8, whose [n, K] table leaves room for no more; four over the global CSR when nnz_max
    is overstated.  (The one-chain shape needs a graph beyond these batches: tests/test_gpu_tabu.py runs it.)
    tests/test_bounds_host.py holds the same table against the host query, without a GPU."""
    if nnz_max is not None:
        return (4, 0)
    return (2, 1) if kind == "trip" and K == 8 else (4, 1)


def put_orders(mem, kind, K, terminals):
    order, cgoff, cptr, classes = orders(kind, K, bool(terminals))
    return [mem.put("order", order), mem.put("cgoff", cgoff), mem.put("cptr", cptr)], classes


def picks(mem, h, cands, idx="best_idx"):
    return [mem.out("cut_all", (h.B, cands)), mem.out("best_assign", (h.R,), I32), mem.out("best_cut", (h.B,)),
            mem.out(idx, (h.B,), I32)]


def decoder_case(pkg, entry, kind, K, terminals, cands, cost=None, optional=True, table=True, nnz_max=None):
    """One call of a decoder.  terminals / cost: None = the entry point has no such argument (a narrower twin);
    cost False = NULL."""
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    data = inputs(kind, K, cands)
    t_eff = 1 if terminals is None else terminals
    name = entry.replace("gmc_", "").replace("_f32", "")
    for suffix in ("_c", "_t"):
        name = name[:-2] if name.endswith(suffix) else name

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h, table, nnz_max)
        s = B.stream(pkg)
        pre = [K] if "kway" in entry or "round" in entry or "large" in entry else []
        tc = ([] if terminals is None else [terminals]) + \
             ([] if cost is None else [p(mem.put("node_cost", data["cost"])) if cost else None])
        b = C.byref(bc)
        opt = lambda nm, shape, dt=I32: p(mem.out(nm, shape, dt)) if optional else None
        if name in ("decode_sample", "decode_sample_seeded", "kway_decode_sample_seeded", "large_sample_seeded"):
            P = p(mem.put("P", data["P"]))
            if name == "decode_sample":
                uoff = np.concatenate([[0], np.cumsum(SAMPLES * (h.sizes - 3))]).astype(np.int64)
                src = [p(mem.put("uniforms", np.random.RandomState(5).uniform(0, 1, int(uoff[-1])))),
                       p(mem.put("uoff", uoff))]
            else:
                src = [p(mem.put("gkey", data["gkey"].view(np.int64)))]
            all_ = p(mem.out("assign_all", (SAMPLES, h.R), I8)) if optional or "kway" not in name and "large" not in name \
                else None
            ws = []
            if name == "large_sample_seeded":
                nbytes = int(lib.gmc_large_search_workspace_bytes(b, K, SAMPLES))
                assert nbytes > 0
                ws = [p(mem.scratch("workspace", nbytes)), nbytes]
            outs = [p(t) for t in picks(mem, h, SAMPLES, "best_iter")]
            return getattr(lib, entry)(b, P, *pre, *tc, *src, SAMPLES, all_, *ws, *outs, s)
        if name in ("round_conditional", "large_round_conditional"):
            o, classes = put_orders(mem, kind, K, t_eff)
            ws = []
            if name.startswith("large"):
                nbytes = int(lib.gmc_large_round_workspace_bytes(b, K))
                assert nbytes > 0
                ws = [classes, SWEEPS, p(mem.scratch("workspace", nbytes)), nbytes]
            else:
                ws = [SWEEPS]
            return getattr(lib, entry)(b, p(mem.put("P", data["P"])), *pre, *tc, *[p(x) for x in o], *ws,
                                       p(mem.out("assign", (h.R,), I8)), p(mem.out("cut", (h.B,))),
                                       opt("expected", (h.B,), torch.float32), opt("sweeps", (h.B,)), s)
        if name == "large_local_search":
            o, classes = put_orders(mem, kind, K, t_eff)
            nbytes = int(lib.gmc_large_round_workspace_bytes(b, K))
            return getattr(lib, entry)(b, *pre, *tc, *[p(x) for x in o], classes, SWEEPS, p(mem.scratch("workspace", nbytes)),
                                       nbytes, p(mem.state("assign", data["assign"][0].copy())), p(mem.out("cut", (h.B,))),
                                       opt("sweeps", (h.B,)), s)
        assign = mem.state("assign", data["assign"]) if name != "kway_evolve" else None
        if name == "refine_local":
            o, _ = put_orders(mem, kind, 3, 1)
            return lib.gmc_refine_local_f32(b, *[p(x) for x in o], cands, p(assign), SWEEPS,
                                            *[p(t) for t in picks(mem, h, cands)], opt("sweeps", (h.B, cands)), s)
        if name in ("refine_anneal", "kway_refine_anneal", "large_anneal"):
            o, classes = put_orders(mem, kind, K, t_eff)
            assert lib.gmc_refine_anneal_staged(b) in (0, 1)
            sched = [p(mem.put("inv_temp", data["inv_temp"])), SWEEPS, p(mem.put("levels", LEVELS)), SEED, SWEEPS]
            ws, mc = [], []
            if name == "large_anneal":
                nbytes = int(lib.gmc_large_search_workspace_bytes(b, K, cands))
                assert nbytes > 0
                ws, mc = [p(mem.scratch("workspace", nbytes)), nbytes], [classes]
            return getattr(lib, entry)(b, *pre, *tc, *[p(x) for x in o], *mc, cands, p(assign), *sched, *ws,
                                       *[p(t) for t in picks(mem, h, cands)], opt("snap_sweep", (h.B, cands)),
                                       opt("sweeps", (h.B, cands)), s)
        if name == "kway_evolve":
            o, _ = put_orders(mem, kind, K, 1)
            pop = np.zeros((2,) + data["assign"].shape, np.int8)
            pop[0] = data["assign"]
            pop[1] = -7
            return lib.gmc_kway_evolve_f32(b, K, *[p(x) for x in o], cands, p(mem.state("pop", pop)),
                                           p(mem.out("cut", (2, h.B, cands))), GENERATIONS, 2,
                                           p(mem.put("inv_temp", data["inv_temp"])), SWEEPS, p(mem.put("levels", LEVELS)), SEED,
                                           SWEEPS, p(mem.out("best_assign", (h.R,), I32)), p(mem.out("best_cut", (h.B,))),
                                           p(mem.out("best_idx", (h.B,), I32)),
                                           opt("history", (GENERATIONS + 1, h.B), torch.float32), s)
        if name in ("kway_tabu", "kway_balance"):
            shape = int(getattr(lib, f"gmc_{name}_shape")(b, K))
            assert (shape & 15, shape >> 4) == chain_shape(kind, K, nnz_max), (kind, K, nnz_max, shape)
            bounds = []
            if name == "kway_balance":
                lo = np.maximum(h.sizes[:, None] // K - 2, 0).repeat(K, 1).astype(np.int32)
                hi = (h.sizes[:, None] // K + 3).repeat(K, 1).astype(np.int32)
                bounds = [p(mem.put("size_lo", lo)), p(mem.put("size_hi", hi))]
            extra = [opt("best_iter", (h.B, cands)), opt("moves", (h.B, cands))]
            if name == "kway_balance":
                extra += [opt("repairs", (h.B, cands)), opt("feasible", (h.B,))]
            return getattr(lib, entry)(b, *pre, *tc, cands, p(assign), *bounds, ITERATIONS, *TENURE, SEED,
                                       *[p(t) for t in picks(mem, h, cands)], *extra, s)
        raise KeyError(entry)
    return case


# ---- the 3-class decoders ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("gmc_decode_sample_f32", "gmc_decode_sample_seeded_f32"))
def test_samplers(pkg, entry):
    for kind in ("odd", "hub", "trip"):
        B.run_case(pkg, decoder_case(pkg, entry, kind, 3, None, SAMPLES))


@pytest.mark.parametrize("cands", CANDS)
@pytest.mark.parametrize("entry", ("gmc_refine_local_f32", "gmc_refine_anneal_f32"))
def test_refine_and_anneal(pkg, entry, cands):
    for optional in (True, False):
        B.run_case(pkg, decoder_case(pkg, entry, "odd", 3, None, cands, optional=optional))
    for kind in ("hub", "trip"):
        B.run_case(pkg, decoder_case(pkg, entry, kind, 3, None, cands))


# ---- K classes, terminals, node costs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", CLASSES)
def test_round_conditional(pkg, K):
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for cost in (False, True):
            for optional in (True, False):
                B.run_case(pkg, decoder_case(pkg, "gmc_round_conditional_c_f32", odd, K, terminals, 1, cost, optional))
        for kind in ("hub", "trip"):
            B.run_case(pkg, decoder_case(pkg, "gmc_round_conditional_c_f32", kind, K, terminals, 1, True))
    B.run_case(pkg, decoder_case(pkg, "gmc_round_conditional_t_f32", kind_for("odd", K), K, 1, 1))
    B.run_case(pkg, decoder_case(pkg, "gmc_round_conditional_f32", kind_for("odd", K), K, None, 1))


@pytest.mark.parametrize("K", CLASSES)
def test_kway_sampler(pkg, K):
    e = "gmc_kway_decode_sample_seeded_c_f32"
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for cost in (False, True):
            for optional in (True, False):
                B.run_case(pkg, decoder_case(pkg, e, odd, K, terminals, SAMPLES, cost, optional))
        for kind in ("hub", "trip"):
            B.run_case(pkg, decoder_case(pkg, e, kind, K, terminals, SAMPLES, True))
    B.run_case(pkg, decoder_case(pkg, "gmc_kway_decode_sample_seeded_t_f32", kind_for("odd", K), K, 1, SAMPLES))
    B.run_case(pkg, decoder_case(pkg, "gmc_kway_decode_sample_seeded_f32", kind_for("odd", K), K, None, SAMPLES))


@pytest.mark.parametrize("cands", CANDS)
@pytest.mark.parametrize("K", CLASSES)
def test_kway_anneal(pkg, K, cands):
    e = "gmc_kway_refine_anneal_c_f32"
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for cost in (False, True):
            B.run_case(pkg, decoder_case(pkg, e, odd, K, terminals, cands, cost))
        B.run_case(pkg, decoder_case(pkg, e, odd, K, terminals, cands, True, optional=False))
        for kind in ("hub", "trip"):
            B.run_case(pkg, decoder_case(pkg, e, kind, K, terminals, cands, True))
    if cands == 3:
        B.run_case(pkg, decoder_case(pkg, "gmc_kway_refine_anneal_t_f32", kind_for("odd", K), K, 1, cands))
        B.run_case(pkg, decoder_case(pkg, "gmc_kway_refine_anneal_f32", kind_for("odd", K), K, None, cands))


@pytest.mark.parametrize("cands", CANDS)
@pytest.mark.parametrize("K", CLASSES)
def test_evolve(pkg, K, cands):
    for optional in (True, False):
        B.run_case(pkg, decoder_case(pkg, "gmc_kway_evolve_f32", kind_for("odd", K), K, None, cands, optional=optional))
    for kind in ("hub", "trip"):
        B.run_case(pkg, decoder_case(pkg, "gmc_kway_evolve_f32", kind, K, None, cands))


@pytest.mark.parametrize("cands", CANDS)
@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("search", ("tabu", "balance"))
def test_chain_searches(pkg, search, K, cands):
    """Every LDS shape gmc_kway_*_shape reports for these batches - asserted per case against chain_shape - and the
    global-CSR variant (nnz_max overstated)."""
    e = f"gmc_kway_{search}_c_f32"
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for cost in (False, True):
            B.run_case(pkg, decoder_case(pkg, e, odd, K, terminals, cands, cost))
        B.run_case(pkg, decoder_case(pkg, e, odd, K, terminals, cands, True, optional=False))
        for kind in ("hub", "trip"):
            for nnz_max in (None, 1 << 24):
                B.run_case(pkg, decoder_case(pkg, e, kind, K, terminals, cands, True, nnz_max=nnz_max))
        B.run_case(pkg, decoder_case(pkg, e, odd, K, terminals, cands, True, nnz_max=1 << 24))
    if cands == 3:
        B.run_case(pkg, decoder_case(pkg, f"gmc_kway_{search}_f32", kind_for("odd", K), K, 1, cands))


# ---- graphs beyond one workgroup ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("what", ("round_conditional", "local_search", "sample_seeded"))
def test_large_decoders(pkg, what, K):
    e = f"gmc_large_{what}_t_f32"
    cands = SAMPLES if what == "sample_seeded" else 1
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for optional in (True, False):
            B.run_case(pkg, decoder_case(pkg, e, odd, K, terminals, cands, optional=optional))
        for kind in ("tile", "hub"):
            B.run_case(pkg, decoder_case(pkg, e, kind, K, terminals, cands))
    B.run_case(pkg, decoder_case(pkg, f"gmc_large_{what}_f32", kind_for("odd", K), K, None, cands))


@pytest.mark.parametrize("cands", CANDS)
@pytest.mark.parametrize("K", CLASSES)
def test_large_anneal(pkg, K, cands):
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for optional in (True, False):
            B.run_case(pkg, decoder_case(pkg, "gmc_large_anneal_t_f32", odd, K, terminals, cands, optional=optional))
        for kind in ("tile", "hub"):
            B.run_case(pkg, decoder_case(pkg, "gmc_large_anneal_t_f32", kind, K, terminals, cands))
    if cands == 3:
        B.run_case(pkg, decoder_case(pkg, "gmc_large_anneal_f32", kind_for("odd", K), K, None, cands))


def test_the_check_can_fail(pkg):
    B.check_can_fail(pkg, decoder_case(pkg, "gmc_kway_tabu_c_f32", "odd", 5, 1, 3, True), "assign")
    B.check_can_fail(pkg, decoder_case(pkg, "gmc_large_anneal_t_f32", "odd", 5, 0, 3), "workspace")

