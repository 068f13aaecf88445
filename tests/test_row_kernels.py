"""Census of the row-kernel sequence (CPU only).

plan() in csrc/api.hip runs a batch on the row kernels (Plan.fs == 0) when its largest graph does not fit a CU's LDS
(n_max past the last window, up to GMC_MAX_GRAPH_NODES = 4096), when the batch has no ELL table (dense graphs, rows of
more than 15 overflow blocks), and when it has overflow lists that the LDS kernels cannot take (between and past the
overflow windows, with edge weights, under gmc_set_fuse(0) or dropout).  This module pins that sequence:

- what is instantiated: the row-family kernel symbols of the gfx950 code objects inside the built library;
- what is reachable: the dispatch of spmm.hip / dw1.hip / head.hip / dropout.hip stated here as literal tables,
  independently of the library;
- reachable <= instantiated, instantiated - reachable == DEAD (each with its reason);
- ROW_MATRIX (run by tests/test_gpu_row_kernels.py) covers every reachable instantiation and every route into the row
  sequence, and the query gives no LDS word for any of its batches;
- the sparse float64 step equals the dense one of tests/stepcheck.py; the numpy dropout mask is the kernel's hash.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest

from tests import stepcheck, util
from tests.test_lds_flavours import batch_struct

FAMILIES = ("spmm_rows_v4", "spmm_rows_wide", "spmm_rows_scalar", "dw1_gather_kernel", "fold_chunks_kernel",
            "hidden_bwd_kernel", "colsum_reduce_kernel", "head_kernel", "head_bwd_kernel", "dropout_kernel",
            "hw2_rows_kernel")
HEAD_LDS_LIMIT = 64 * 1024   # head.hip: above this the head kernel's dynamic LDS needs hipFuncSetAttribute


# ---- the dispatch, stated independently of the library
def launch_np(F):
    """spmm.hip launch_np: 256-column passes per lane, or the 1024-column blocks of spmm_rows_wide."""
    return 1 if F <= 256 else 2 if F <= 512 else 4 if F <= 1024 else "wide"


def spmm(F, has_val, epi, variant):
    np_ = launch_np(F)
    if np_ == "wide":
        return f"spmm_rows_wide<2,8,{int(has_val)},{int(epi)},{variant}>"
    return f"spmm_rows_v4<{np_},2,8,{int(has_val)},{int(epi)},0,{variant}>"


def dw1_np(F):
    return 1 if F <= 256 else 2 if F <= 512 else 4


def dw1_chunks(B):
    """gmc_dw1_chunks(B, lds = false): about eight graphs per chunk, at most 32 - one chunk (no fold) up to B = 8."""
    return 1 if B <= 4 else min(32, (B + 7) // 8)


def head_lds_bytes(n_max):
    return 4 * (7 * (n_max + 4) + 64)


def row_step(F, weights, table_w, B, dropout=False):
    """Kernels of a training step (gmc_train_fwd_bwd) on the row sequence, in launch order, with their probe tags:
    W1 gather (VARIANT 1, HAS_VAL = the batch has weights, no epilogue), aggregation + relu (+ W2 epilogue without
    dropout; with it: dropout and hw2_rows), head, hidden backward, colsum, backward aggregation, dW1 (+ fold)."""
    out = [("gather_w1", spmm(F, weights, False, 1))]
    if dropout:
        out += [("agg_fwd", spmm(F, False, False, 0)), (None, "dropout_kernel"), (None, "hw2_rows_kernel")]
    else:
        out += [("agg_fwd", spmm(F, False, True, 0))]
    out += [("head", f"head_kernel<{table_w}>"), ("hidden_bwd", "hidden_bwd_kernel"), ("colsum", "colsum_reduce_kernel"),
            ("agg_bwd", spmm(F, False, False, 0)), ("dw1", f"dw1_gather_kernel<{dw1_np(F)}>")]
    if dw1_chunks(B) > 1:
        out += [("dw1_fold", "fold_chunks_kernel")]
    return out


def row_tags(B):
    return ["gather_w1", "agg_fwd", "head", "hidden_bwd", "colsum", "agg_bwd", "dw1"] + \
        (["dw1_fold"] if dw1_chunks(B) > 1 else [])


def user_spmm(F, weights, epi, vec=True):
    """gmc_spmm_f32: VARIANT 0 with or without weights and W2 epilogue; F % 4 != 0 or unaligned: spmm_rows_scalar."""
    return spmm(F, weights, epi, 0) if vec else f"spmm_rows_scalar<{int(weights)}>"


F_CLASSES = (4, 256, 512, 1024, 4096)   # one F per launch_np / dw1_np class


def reachable():
    out = set()
    for F in F_CLASSES:
        for weights in (False, True):
            for table_w in (0, 8, 16):
                for B in (1, 9):
                    for dropout in (False, True):
                        out |= {k for _t, k in row_step(F, weights, table_w, B, dropout)}
            for epi in (False, True):
                out.add(user_spmm(F, weights, epi))
            out.add(user_spmm(F, weights, False, vec=False))
    out.add("head_bwd_kernel")   # gmc_backward_from_gp
    return out


# ---- instantiations that no call can select.  Must stay empty unless an entry has a reason.
DEAD = {}


def instantiated(lib_path):
    out = set()
    for line in util.kernel_symbols(lib_path):
        m = re.search(r"::(\w+)(<[^>]*>)?\(", line)
        if not m or m.group(1) not in FAMILIES:
            continue
        args = ""
        if m.group(2):
            a = [{"true": "1", "false": "0"}.get(t.strip(), t.strip()) for t in m.group(2)[1:-1].split(",")]
            args = "<" + ",".join(a) + ">"
        out.add(m.group(1) + args)
    return out


# ---- the GPU matrix (tests/test_gpu_row_kernels.py).  Graph kinds:
#   reg7 / reg12   near-regular of that degree: table of 8 slots (7 live) / 16 slots (12 live);
#   ovf8 / ovf16   reg7 + one hub of degree 12 / reg12 + one hub of degree 20: one overflow block;
#   gnp            G(n, p) of mean degree ~30: no table (choose_width 0);
#   hub            reg7 + one hub of degree 150: 18 overflow blocks > 15, no table.
# B > 1: the n graph, then B - 1 graphs of 12 nodes (degree 3).  Columns:
#   (id, route, kind, n, F, weights, B, fuse, (table W, live slots, overflow blocks) of the batch)
ROW_MATRIX = [
    ("w8_past", "past the last 8-slot window", "reg7", 1021, 256, False, 2, 1, (8, 7, 0)),
    ("w16_past", "past the last 16-slot window", "reg12", 1009, 260, True, 6, 1, (16, 12, 0)),
    ("ovf8_gap275", "w8_ovf gap 275", "ovf8", 275, 512, False, 2, 1, (8, 8, 1)),
    ("ovf8_gap536", "w8_ovf gap 536", "ovf8", 536, 516, False, 5, 1, (8, 8, 1)),
    ("ovf8_1007", "w8_ovf past 1006", "ovf8", 1007, 1024, False, 3, 1, (8, 8, 1)),
    ("ovf16_1005", "w16_ovf past 1004", "ovf16", 1005, 1028, True, 12, 1, (16, 16, 1)),
    ("ovf8_weighted", "weights with overflow lists", "ovf8", 300, 128, True, 2, 1, (8, 8, 1)),
    ("ovf8_unfused", "overflow lists under gmc_set_fuse(0)", "ovf8", 300, 64, False, 2, 0, (8, 8, 1)),
    ("n2327", "head LDS <= 64 KiB, last", "reg7", 2327, 2048, False, 1, 1, (8, 7, 0)),
    ("n2328", "head LDS > 64 KiB, first", "reg7", 2328, 260, True, 9, 1, (8, 7, 0)),
    ("n4096", "GMC_MAX_GRAPH_NODES", "reg7", 4096, 4096, False, 1, 1, (8, 7, 0)),
    ("gnp", "dense: no table", "gnp", 1500, 1024, True, 2, 1, (0, 0, 0)),
    ("gnp_small", "dense: no table, inside the windows", "gnp", 300, 4096, True, 1, 1, (0, 0, 0)),
    ("hub", "more than 15 overflow blocks: no table", "hub", 1500, 516, False, 2, 1, (0, 0, 0)),
    ("b249", "32 dW1 chunks", "reg7", 1100, 512, True, 249, 1, (8, 7, 0)),
]
ROUTES = {"past the last 8-slot window", "past the last 16-slot window", "w8_ovf gap 275", "w8_ovf gap 536",
          "w8_ovf past 1006", "w16_ovf past 1004", "weights with overflow lists", "overflow lists under gmc_set_fuse(0)",
          "head LDS <= 64 KiB, last", "head LDS > 64 KiB, first", "GMC_MAX_GRAPH_NODES", "dense: no table",
          "dense: no table, inside the windows", "more than 15 overflow blocks: no table", "32 dW1 chunks"}
# gmc_spmm_f32 cases of the GPU module: (F, weights, W2 epilogue); F = 6 takes spmm_rows_scalar
USER_SPMM = [(F, w, e) for F in (256, 512, 1024, 2048) for w in (False, True) for e in (False, True)] + \
            [(6, False, False), (6, True, False)]
# gmc_backward_from_gp with a dense random dL/dP: one NP 1, one NP 4 and one wide case of ROW_MATRIX
GP_CASES = ["w8_past", "ovf8_1007", "ovf16_1005", "n2328"]
# dropout (p = 0.3) on the row sequence and the LDS one-kernel-per-operation sequence: (id, kind, n, F, B)
# (the same n and F, so that the two layouts' masks can be compared entry by entry; overflow lists + dropout: rows)
DROPOUT_CASES = [("rows", "ovf8", 400, 100, 2), ("slab", "reg7", 400, 100, 2)]


def matrix_kernels():
    out = set()
    for _id, _r, kind, n, F, weights, B, _fuse, (W, _s, _o) in ROW_MATRIX:
        out |= {k for _t, k in row_step(F, weights, W, B)}
    out |= {user_spmm(F, w, e, vec=F % 4 == 0) for F, w, e in USER_SPMM}
    out |= {k for _c, _k, _n, F, B in DROPOUT_CASES[:1] for _t, k in row_step(F, False, 8, B, dropout=True)}
    out.add("head_bwd_kernel")
    return out


@pytest.fixture(scope="module")
def hip(built):
    built.hip.load()
    return built.hip


# ---- tests
def test_reachable_row_kernels_are_instantiated_and_the_rest_is_listed_dead(hip):
    inst = instantiated(hip.LIB_PATH)
    reach = reachable()
    assert not reach - inst, sorted(reach - inst)
    assert sorted(inst - reach) == sorted(DEAD), sorted(inst - reach)
    assert all(DEAD.values())
    count = {f: sum(1 for k in reach if k.startswith(f + "<") or k == f) for f in FAMILIES}
    assert count == {"spmm_rows_v4": 18, "spmm_rows_wide": 6, "spmm_rows_scalar": 2, "dw1_gather_kernel": 3,
                     "fold_chunks_kernel": 1, "hidden_bwd_kernel": 1, "colsum_reduce_kernel": 1, "head_kernel": 3,
                     "head_bwd_kernel": 1, "dropout_kernel": 1, "hw2_rows_kernel": 1}, count


def test_no_w1_gather_has_a_w2_epilogue_and_no_tuning_case_is_shipped(hip):
    inst = instantiated(hip.LIB_PATH)
    assert not [k for k in inst if k.startswith("spmm_rows_v4") and k.endswith(",1,0,1>")]
    assert not [k for k in inst if k.startswith("spmm_rows_wide") and k.endswith(",1,1>")]
    assert {k.split(",")[1] + k.split(",")[2] + k.split(",")[5] for k in inst if k.startswith("spmm_rows_v4")} == {"280"}


def test_dispatch_tables():
    assert [launch_np(F) for F in (4, 256, 260, 512, 516, 1024, 1028, 4096)] == [1, 1, 2, 2, 4, 4, "wide", "wide"]
    assert [dw1_np(F) for F in (256, 260, 512, 516, 1024, 1028, 4096)] == [1, 2, 2, 4, 4, 4, 4]
    assert [dw1_chunks(B) for B in (1, 4, 5, 8, 9, 248, 249, 1000)] == [1, 1, 1, 1, 2, 31, 32, 32]
    assert max(n for n in range(3, 4097) if head_lds_bytes(n) <= HEAD_LDS_LIMIT) == 2327


def test_matrix_covers_every_reachable_kernel_and_route():
    assert matrix_kernels() == reachable(), (sorted(reachable() - matrix_kernels()), sorted(matrix_kernels() - reachable()))
    assert {r for _i, r, *_x in ROW_MATRIX} == ROUTES
    assert len({c[0] for c in ROW_MATRIX}) == len(ROW_MATRIX)
    Bs = [c[6] for c in ROW_MATRIX]
    assert min(Bs) <= 4 and any(5 <= B <= 8 for B in Bs) and any(1 < dw1_chunks(B) < 32 for B in Bs)
    assert dw1_chunks(max(Bs)) == 32
    Fs = {c[4] for c in ROW_MATRIX}
    assert {256, 260, 512, 516, 1024, 1028, 2048, 4096} <= Fs
    ns = {c[3] for c in ROW_MATRIX}
    assert {1021, 1009, 275, 536, 1007, 1005, 2327, 2328, 4096} <= ns
    assert {c[0] for c in ROW_MATRIX if c[4] <= 256} and {c[0] for c in ROW_MATRIX if c[4] > 1024 and c[5]}
    for i in GP_CASES:
        assert i in {c[0] for c in ROW_MATRIX}
    assert {launch_np(c[4]) for c in ROW_MATRIX if c[0] in GP_CASES} == {1, 2, 4, "wide"}


@pytest.mark.parametrize("case", ROW_MATRIX, ids=[c[0] for c in ROW_MATRIX])
def test_matrix_batches_get_no_lds_words(hip, case):
    """The query (host only) gives the batch of each case no LDS word of the sequence it runs: the row kernels.  Under
    gmc_set_fuse(0) the fused pair may stay (the batch is not run fused); the one-kernel-per-operation part is empty."""
    _id, _route, _kind, n, F, weights, B, fuse, (W, slots, blocks) = case
    b = batch_struct(hip, W, slots, weights, blocks, n, B)
    if not W:
        b.ell = None
    words = hip.lds_flavours(b, F)
    if fuse:
        assert words == [], [hip.flavour_fields(w) for w in words]
    else:
        assert len(words) == 2, [hip.flavour_fields(w) for w in words]   # fused only: the unfused sequence has no words


def _graph_csr(n, deg, seed):
    import networkx as nx
    g = nx.random_regular_graph(deg, n, seed=seed)
    rows, cols = [], []
    for u, v in g.edges():
        rows += [u, v]
        cols += [v, u]
    order = np.lexsort((cols, rows))
    rows, cols = np.asarray(rows)[order], np.asarray(cols)[order]
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols.astype(np.int32)


@pytest.mark.parametrize("weighted", [False, True])
def test_sparse_float64_step_equals_the_dense_one(weighted):
    rng = np.random.RandomState(7)
    N, F = 60, 24
    params = {"conv1.weight": rng.standard_normal((N, F)) * 0.3, "conv1.bias": rng.standard_normal(F) * 0.1,
              "conv2.weight": rng.standard_normal((F, 3)) * 0.3, "conv2.bias": rng.standard_normal(3) * 0.1}
    csrs = []
    for n, d, s in ((40, 5, 1), (57, 6, 2), (12, 3, 3)):
        rp, cl = _graph_csr(n, d, s)
        vl = None
        if weighted:   # symmetric integer weights
            w = {}
            for r in range(n):
                for e in range(rp[r], rp[r + 1]):
                    w.setdefault((min(r, cl[e]), max(r, cl[e])), float(rng.randint(1, 4)))
            vl = np.asarray([w[(min(r, cl[e]), max(r, cl[e]))] for r in range(n) for e in range(rp[r], rp[r + 1])],
                            np.float32)
        csrs.append((rp, cl, vl))
        W = [params[k] for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")]
        fd, fs = stepcheck.f64_forward(rp, cl, vl, *W), stepcheck.f64_forward_sparse(rp, cl, vl, *W)
        for k in ("dinv", "H", "P"):
            assert np.abs(fd[k] - fs[k]).max() <= 1e-12 * max(1.0, np.abs(fd[k]).max()), k
        S = stepcheck.f64_partition(fd["P"])
        (ld, gd), (ls, gs) = stepcheck.f64_loss_and_gp(fd, S), stepcheck.f64_loss_and_gp_sparse(fs, S)
        assert ld == ls and np.array_equal(gd, gs)
    S_all = np.concatenate([stepcheck.f64_partition(stepcheck.f64_forward_sparse(rp, cl, vl, *W)["P"]) for rp, cl, vl in csrs])
    Pd, lossd, gd, _ties = stepcheck.f64_step(csrs, params, S_all)
    Ps, losss, gs, _ties = stepcheck.f64_step(csrs, params, S_all, sparse=True)
    assert np.abs(Pd - Ps).max() <= 1e-12 and np.array_equal(lossd, losss)
    for k in gd:
        assert np.abs(gd[k] - gs[k]).max() <= 1e-12 * max(1.0, np.abs(gd[k]).max()), k
    assert np.array_equal(stepcheck.kink_columns(csrs, params, noise=1e-2), stepcheck.kink_columns(csrs, params, noise=1e-2,
                                                                                          sparse=True))


def test_dropout_mask_restatement():
    """splitmix64 of (seed, batch row, column) as csrc/dropout.hip states it, in numpy: known values of the
    finaliser, a keep rate of 1 - p, no correlation between neighbouring rows / columns, a different mask per seed."""
    # splitmix64's finaliser on the first outputs of the splitmix64 stream with seed 0 (gamma 0x9E3779B97F4A7C15)
    gamma = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        z = np.asarray([gamma * np.uint64(k) for k in (1, 2, 3)], np.uint64)
    assert [int(x) for x in util.mix64(z)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = util.dropout_uniform(12345, np.arange(2000), np.arange(500))
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u * np.float32(16777216.0), np.floor(u * np.float32(16777216.0)))   # 24-bit grid
    p = 0.3
    keep = util.dropout_keep(12345, np.arange(2000), np.arange(500), p)
    assert abs(keep.mean() - (1 - p)) < 3e-3
    k = keep.astype(np.float64) - keep.mean()
    assert abs((k[1:] * k[:-1]).mean()) / k.var() < 0.01 and abs((k[:, 1:] * k[:, :-1]).mean()) / k.var() < 0.01
    other = util.dropout_keep(12346, np.arange(2000), np.arange(500), p)
    assert abs((keep == other).mean() - (p * p + (1 - p) * (1 - p))) < 3e-3
    # the stream hashes the BATCH row: a graph's mask depends on where it sits in the batch
    at0 = util.dropout_keep(9, np.arange(100), np.arange(64), p)
    at50 = util.dropout_keep(9, np.arange(100) + 50, np.arange(64), p)
    assert not np.array_equal(at0, at50) and np.array_equal(at0[50:], at50[:50])


def test_graph_size_bound_is_checked_before_any_launch(hip):
    """n_max = 4097 is refused with GMC_ERR_GRAPH_SIZE by the argument checks of gmc_forward / gmc_train_fwd_bwd
    (before any HIP call); 4096 passes them and stops at the workspace size."""
    lib = hip.load()
    some = C.c_void_p(4096)
    model = hip.GmcModel(N=4097, F=2048, K=3, W1=4096, b1=4096, W2=4096, b2=4096)
    for n, want in ((4097, -6), (4096, -5), (2, -6)):
        b = batch_struct(hip, 8, 7, False, 0, n, 1)
        assert lib.gmc_forward(C.byref(b), C.byref(model), 1.0, some, 16, some, None, None, None) == want, n
        assert lib.gmc_train_fwd_bwd(C.byref(b), C.byref(model), 1.0, some, 16, some, some, some, some, None) == want, n
    model.N = 4096
    b = batch_struct(hip, 8, 7, False, 0, 4096, 1)
    assert lib.gmc_forward(C.byref(b), C.byref(model), 1.0, some, 16, some, None, None, None) == -5   # GMC_ERR_WORKSPACE
    assert math.isfinite(lib.gmc_workspace_bytes(C.byref(b), C.byref(model), 1))
