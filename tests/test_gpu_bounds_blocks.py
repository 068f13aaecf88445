"""Guard-band tests of the stand-alone heads and products (gmc_head_f32, gmc_head_loss_f32, gmc_cut_loss_f32,
gmc_dense_hw2_f32, gmc_row_weight_sums_f32) and of the builders (gmc_batch_build_csr, gmc_batch_build_table,
gmc_contract_map, gmc_contract_entries): every buffer from one arena with 4096-byte bands, each case on plain tensors
and on arenas filled 0xFF and 0x00, the byte equalities of tests/bounds.run_case.

The builders get an edge-index input with an odd number of entries and a self-loop (accepted: kept once), and one with
a duplicate, an id out of range and an entry across two graphs (counted in the report, never used as an index; the
arrays then hold fewer than E entries, so their tails stay as they were and are compared per fill).
The contraction runs K = 2, 3, 5, 8 wherever a batch's graphs can hold a pin of every class (INFEASIBLE lists the
three pairs that cannot, with the reason); `pins` and `trip` carry K = 8.

Measured on the MI355X: 107 cases (390 calls), no band touched, no pair of runs different.  Alone (-s prints the
counts) the file's 36 tests take 2.6 s, library load and GPU start-up included; the slowest is test_heads[odd] at 0.12 s
(the first to touch the GPU), every other test at most 0.03 s.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import bounds as B

pytestmark = pytest.mark.gpu

WIDTHS = (4, 20, 516)
CUT_C = 1.5
I32 = torch.int32


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    done = B.report_calls("bounds/blocks")
    yield built
    done()


def head_case(pkg, kind, entry, loss_kind, z_parts, training, table=True):
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    rng = np.random.RandomState(z_parts)
    Z0 = rng.uniform(-1, 1, (z_parts, h.R, 3)).astype(np.float32)
    b2 = rng.uniform(-1, 1, 3).astype(np.float32)

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h, table)
        outs = [p(mem.out("P", (h.R, 3))), p(mem.out("S", (h.R,), I32)), p(mem.out("loss", (h.B,))),
                p(mem.out("GY2", (h.R, 4))) if training else None, p(mem.out("db2part", (h.B, 3))) if training else None]
        kind_arg = [] if entry == "gmc_head_f32" else [loss_kind]
        return getattr(lib, entry)(C.byref(bc), p(mem.put("Z0", Z0)), z_parts, p(mem.put("b2", b2)), CUT_C, *kind_arg,
                                   *outs, B.stream(pkg))
    return case


@pytest.mark.parametrize("kind", ("odd", "hub", "trip"))
def test_heads(pkg, kind):
    for training in (True, False):
        for z_parts in (1, 3):
            for loss_kind in (0, 1):
                B.run_case(pkg, head_case(pkg, kind, "gmc_head_loss_f32", loss_kind, z_parts, training))
        B.run_case(pkg, head_case(pkg, kind, "gmc_head_f32", 0, 1, training))
        B.run_case(pkg, head_case(pkg, kind, "gmc_head_loss_f32", 1, 1, training, table=False))


def cut_loss_case(pkg, kind, loss_kind, want_gp, table=True):
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    Pm = np.random.RandomState(3).dirichlet(np.ones(3), h.R).astype(np.float32)

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h, table)
        return lib.gmc_cut_loss_f32(C.byref(bc), p(mem.put("P", Pm)), CUT_C, loss_kind, p(mem.out("loss", (h.B,))),
                                    p(mem.out("GP", (h.R, 3))) if want_gp else None, B.stream(pkg))
    return case


@pytest.mark.parametrize("kind", ("odd", "hub", "trip"))
def test_cut_loss(pkg, kind):
    for loss_kind in (0, 1):
        for want_gp in (True, False):
            B.run_case(pkg, cut_loss_case(pkg, kind, loss_kind, want_gp))
        B.run_case(pkg, cut_loss_case(pkg, kind, loss_kind, True, table=False))


@pytest.mark.parametrize("F", WIDTHS)
def test_dense_hw2(pkg, F):
    p = pkg.hip.ptr
    for rows in (1, 85, 257):                       # one row, an odd count, past a 256-row tile
        for ldh in (F, F + 4):
            rng = np.random.RandomState(rows + ldh)
            H = rng.uniform(-1, 1, (rows, ldh)).astype(np.float32).reshape(-1)[:(rows - 1) * ldh + F].copy()
            dinv = rng.uniform(0.1, 1, rows).astype(np.float32)
            W2 = rng.uniform(-1, 1, (F, 3)).astype(np.float32)

            def case(lib, mem):                      # (H ends with its last row's F-th float: no pad behind it)
                return lib.gmc_dense_hw2_f32(p(mem.put("H", H)), ldh, p(mem.put("dinv", dinv)), p(mem.put("W2", W2)),
                                             p(mem.out("Z0", (rows, 3))), rows, F, B.stream(pkg))
            B.run_case(pkg, case)


@pytest.mark.parametrize("kind", ("odd", "hub", "tile"))
def test_row_weight_sums(pkg, kind):
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    for weighted in (False, True):
        vals = h.vals if h.vals is not None else np.random.RandomState(1).uniform(0.1, 2, h.nnz).astype(np.float32)

        def case(lib, mem):
            return lib.gmc_row_weight_sums_f32(h.R, p(mem.put("rowptr", h.rowptr)), p(mem.put("gcol", h.gcol)),
                                               p(mem.put("vals", vals)) if weighted else None, p(mem.out("out", (h.R,))),
                                               B.stream(pkg))
        B.run_case(pkg, case)


# ---- the builders ------------------------------------------------------------------------------------------------------
def entries_of(kind, faults):
    """Directed entries of a batch in a seeded shuffle, plus one self-loop (so E is odd); faults: also a duplicate, an
    id out of range and an entry across two graphs."""
    h = B.host_batch(kind)
    rows = np.repeat(np.arange(h.R, dtype=np.int32), np.diff(h.rowptr))
    src, dst = rows, h.gcol.copy()
    w = h.vals if h.vals is not None else np.ones(h.nnz, np.float32)
    loop = int(h.goff[1]) - 1                                        # the last row of the first graph
    src, dst, w = np.append(src, loop), np.append(dst, loop), np.append(w, np.float32(1.0))
    if faults:
        src = np.append(src, [src[0], h.R, 0]).astype(np.int32)
        dst = np.append(dst, [dst[0], 1, h.R - 1]).astype(np.int32)
        w = np.append(w, [w[0], 1.0, 1.0]).astype(np.float32)
    perm = np.random.RandomState(7).permutation(src.size)
    assert faults or src.size % 2 == 1
    return h, src[perm].astype(np.int32), dst[perm].astype(np.int32), w[perm].astype(np.float32)


def build_case(pkg, kind, weighted, faults):
    """gmc_batch_build_csr, then gmc_batch_build_table on its output, sized as GraphBatch.from_edge_index sizes them
    (the host twin says how many entries are kept and how many overflow blocks there are)."""
    h, src, dst, w = entries_of(kind, faults)
    p = pkg.hip.ptr
    E = src.size
    hs = list(h.handles)
    if not faults:                                                   # the host twin with the self-loop, for the table's sizes
        g = B.graphs_of(kind)[0].copy()
        g.add_edge(int(h.sizes[0]) - 1, int(h.sizes[0]) - 1, weight=1.0)
        hs[0] = pkg.graph.from_networkx(g)
    twin = pkg.graph.BatchArrays(hs)
    Wd, blocks = twin.ell_width, 0 if twin.ovf_ptr is None else int(twin.ovf_ptr[-1])
    with_vals = weighted and (twin.vals is not None)

    def case(lib, mem):
        goff = mem.put("goff", h.goff.astype(np.int32))
        nbytes = int(lib.gmc_batch_build_workspace_bytes(h.B, h.R, E))
        assert nbytes > 0
        ws = mem.scratch("workspace", nbytes)
        rowptr, lcol, gcol = mem.out("rowptr", (h.R + 1,), I32), mem.out("lcol", (E,), I32), mem.out("gcol", (E,), I32)
        vals = mem.out("vals", (E,)) if weighted else None
        dinv, report = mem.out("dinv", (h.R,)), mem.out("report", (20,), I32)
        s = B.stream(pkg)
        rcs = [lib.gmc_batch_build_csr(h.B, h.R, E, p(goff), p(mem.put("src", src)), p(mem.put("dst", dst)),
                                       p(mem.put("w", w)) if weighted else None, p(rowptr), p(lcol), p(gcol), p(vals),
                                       p(dinv), p(report), p(ws), nbytes, s)]
        if not faults and Wd:
            ell = mem.out("ell", (h.R, Wd), torch.int16)
            ell_vals = mem.out("ell_vals", (h.R, Wd)) if with_vals else None
            ovf = [mem.out("ovf_ptr", (h.R + 1,), I32), mem.out("ovf_ids", (8 * blocks,), torch.int16),
                   mem.out("ovf_vals", (8 * blocks,)) if with_vals else None] if blocks else [None, None, None]
            rcs.append(lib.gmc_batch_build_table(h.B, h.R, h.n_max, p(goff), p(rowptr), p(lcol), p(vals) if with_vals else None,
                                                 Wd, twin.ell_slots, p(ell), p(ell_vals), *[p(x) for x in ovf], blocks,
                                                 p(ws), nbytes, s))
        return rcs
    return case


@pytest.mark.parametrize("kind", ("odd", "hub", "tile"))
def test_batch_build(pkg, kind):
    for weighted in (False, True):
        runs = B.run_case(pkg, build_case(pkg, kind, weighted, False))
        rep = runs[1][0].outputs["report"].cpu().numpy()
        assert not rep[:5].any() and rep[17] == entries_of(kind, False)[1].size, rep
        # with faults the arrays hold fewer than E entries: their tails keep the fill
        runs = B.run_case(pkg, build_case(pkg, kind, weighted, True), unwritten=("lcol", "gcol", "vals"))
        rep = runs[1][0].outputs["report"].cpu().numpy()
        assert rep[0] == 1 and rep[1] == 1 and rep[2] == 1, rep


def contract_case(pkg, kind, K):
    """gmc_contract_map, then gmc_contract_entries sized by the host twin (gcn-max-cut_amd/graph.py: contract)."""
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    pins, classes, E_out = [], [], 0
    for g, hd in enumerate(h.handles):           # every class twice in a graph of 60 nodes or more, else once
        vals = None if h.vals is None else h.vals[int(h.rowptr[h.goff[g]]):int(h.rowptr[h.goff[g + 1]])]
        hh = pkg.graph.GraphHandle(hd.n, hd.rowptr, hd.col, vals)
        count = 2 * K if hd.n >= 60 else K
        cls = np.arange(count) % K
        if hd.n >= 60:                           # the first seeded draw the rule accepts
            draws = (np.random.RandomState(100 * K + seed).permutation(hd.n)[:count] for seed in range(100))
        else:                                    # a small graph: every K-subset in order, so "none" means there is none
            draws = (np.asarray(c) for c in itertools.combinations(range(hd.n), count))
        for nodes in draws:
            try:
                E_out += pkg.graph.contract(hh, nodes, cls, K).handle.col.size
                break
            except ValueError:
                continue
        else:
            assert hd.n < 60, (kind, K)
            return None, 0                       # no admissible pin set exists (INFEASIBLE lists these pairs)
        pins.append(nodes + int(h.goff[g]))
        classes.append(cls)
    pins = np.concatenate(pins + [pins[0][:1]]).astype(np.int32)     # (a repeated identical pin is harmless: P is odd)
    classes = np.concatenate(classes + [classes[0][:1]]).astype(np.int32)

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h, table=False)
        nbytes = int(lib.gmc_contract_workspace_bytes(h.B, h.R, h.nnz, K))
        assert nbytes > 0
        ws = mem.scratch("workspace", nbytes)
        node_map, goff_out = mem.out("node_map", (h.R,), I32), mem.out("goff_out", (h.B + 1,), I32)
        report = mem.out("report", (8,), I32)
        s = B.stream(pkg)
        rcs = [lib.gmc_contract_map(C.byref(bc), K, pins.size, p(mem.put("pin_node", pins)), p(mem.put("pin_class", classes)),
                                    p(node_map), p(goff_out), p(report), p(ws), nbytes, s)]
        rcs.append(lib.gmc_contract_entries(C.byref(bc), K, p(node_map), p(goff_out), E_out,
                                            p(mem.out("src_out", (E_out,), I32)), p(mem.out("dst_out", (E_out,), I32)),
                                            p(mem.out("w_out", (E_out,))), p(mem.out("fixed_cut", (h.B,))), p(ws), nbytes, s))
        return rcs
    return case, E_out


# K = 2, 5, 8 (and 3, the reference's): every class is pinned in every graph and needs a pinned node with a free
# neighbour, so the small graphs cannot hold the larger class counts - those (batch, K) pairs are listed, each with
# the reason, and `pins` (n = 67 and the hub graph) and `trip` carry K = 8 instead.
CONTRACT = tuple((kind, K) for K in (2, 3, 5, 8) for kind in ("odd9", "hub", "tile", "pins", "trip"))
INFEASIBLE = {
    ("odd9", 8): "n = 9 has one free node left beside 8 pins: eight classes cannot each have a free neighbour",
    ("hub", 8): "its n = 9 graph, as above",
    ("tile", 8): "its n = 8 graph has no free node left beside 8 pins",
}


@pytest.mark.parametrize("kind,K", CONTRACT)
def test_contract(pkg, kind, K):
    case, E_out = contract_case(pkg, kind, K)
    assert (case is None) == ((kind, K) in INFEASIBLE), (kind, K)
    if case is None:
        return
    runs = B.run_case(pkg, case)
    rep = runs[1][0].outputs["report"].cpu().numpy()
    assert not rep[:6].any() and rep[6] == E_out, (rep, E_out)          # the outputs were sized exactly


def test_the_check_can_fail(pkg):
    B.check_can_fail(pkg, head_case(pkg, "odd", "gmc_head_f32", 0, 1, True), "GY2")
    B.check_can_fail(pkg, build_case(pkg, "odd", True, False), "goff")

