"""CPU checks of the batch build from edge-index tensors (include/gcnmaxcut.h, gmc_batch_build_*; graph.from_edge_index,
GraphBatch.from_edge_index): the host twin against from_networkx byte for byte on every case of tests/batch_build_cases.py,
every Python-level refusal (raised before the library or a GPU is asked for), every status code of the three entry points
(fake pointers, one thing wrong per call: no call reaches a launch), the workspace size, and the kernels in the gfx950 code
object without scratch."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from tests import batch_build_cases as BC
from tests import util

SOME, BIG = 4096, 1 << 40   # a fake device address (never dereferenced: the calls fail first), a generous size


# ---- the host twin
def same_handle(a, b):
    assert a.n == b.n
    for name in ("rowptr", "col"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    assert (a.weight is None) == (b.weight is None)
    if a.weight is not None:
        assert a.weight.dtype == b.weight.dtype == np.float32 and a.weight.tobytes() == b.weight.tobytes()


@pytest.mark.parametrize("name", sorted(BC.CASES))
def test_host_twin_equals_from_networkx(built, name):
    for g in BC.graphs(name):
        want = built.from_networkx(g)
        for pairs in ("both", "once"):
            for dtype in (np.int64, np.int32):
                ei, ptr, w = BC.edge_arrays([g], pairs, dtype)
                same_handle(built.from_edge_index(ei, int(ptr[-1]), w, pairs=pairs), want)
        ei, ptr, w = BC.edge_arrays([g])
        perm = np.random.RandomState(1).permutation(ei.shape[1])
        same_handle(built.from_edge_index(torch.from_numpy(ei[:, perm]), int(ptr[-1]),
                                          None if w is None else torch.from_numpy(w[perm])), want)


def test_host_twin_drops_unit_weights_and_keeps_real_ones(built):
    g = BC.graphs("all_ones")[0]
    ei, ptr, w = BC.edge_arrays([g])
    assert w is not None and np.all(w == 1.0)
    assert built.from_edge_index(ei, int(ptr[-1]), w).weight is None
    assert built.from_networkx(g).weight is None
    ei, ptr, w = BC.edge_arrays([BC.graphs("real")[0]])
    assert built.from_edge_index(ei, int(ptr[-1]), w).weight is not None


def test_host_twin_refuses_bad_entries(built):
    ei, ptr, _w = BC.edge_arrays([BC.regular(20, 3, 1)])
    n = int(ptr[-1])
    bad = ei.copy(); bad[1, 0] = n
    with pytest.raises(ValueError, match="1 entries with an id outside"):
        built.from_edge_index(bad, n)
    with pytest.raises(ValueError, match="2 repeated entries"):
        built.from_edge_index(np.concatenate([ei, ei[:, :2]], axis=1), n)
    with pytest.raises(ValueError, match="1 entries whose reverse is missing"):
        built.from_edge_index(ei[:, 1:], n)
    w = np.ones(ei.shape[1], np.float32); w[0] = 2.0
    with pytest.raises(ValueError, match="whose reverse is missing or carries another weight"):
        built.from_edge_index(ei, n, w)
    with pytest.raises(ValueError, match="pairs must be"):
        built.from_edge_index(ei, n, pairs="twice")
    with pytest.raises(ValueError, match=r"edge_index must be \[2, E\]"):
        built.from_edge_index(ei.T, n)
    with pytest.raises(ValueError, match="must hold integers"):
        built.from_edge_index(ei.astype(np.float32), n)


# ---- the Python-level refusals of the device constructor: ValueError, whether or not there is a GPU
def test_python_level_checks_come_before_the_library(built):
    make = built.GraphBatch.from_edge_index
    ei, ptr, _w = BC.edge_arrays([BC.regular(20, 3, 1), BC.regular(9, 4)])
    E = ei.shape[1]
    with pytest.raises(ValueError, match=r"edge_index must be \[2, E\]"):
        make(ei.T, ptr)
    with pytest.raises(ValueError, match=r"edge_index must be \[2, E\]"):
        make(ei[0], ptr)
    with pytest.raises(ValueError, match="edge_index must hold integers"):
        make(torch.from_numpy(ei).float(), ptr)
    with pytest.raises(ValueError, match=r"edge_weight must be \[E = "):
        make(ei, ptr, edge_weight=np.ones(E + 1, np.float32))
    with pytest.raises(ValueError, match="edge_weight must hold real numbers"):
        make(ei, ptr, edge_weight=np.ones(E, np.complex64))
    with pytest.raises(ValueError, match="exactly one of ptr"):
        make(ei)
    with pytest.raises(ValueError, match="exactly one of ptr"):
        make(ei, ptr, num_nodes=29)
    with pytest.raises(ValueError, match=r"ptr must be \[B \+ 1\]"):
        make(ei, ptr.reshape(1, -1))
    with pytest.raises(ValueError, match="ptr must hold integers"):
        make(ei, ptr.astype(np.float64))
    with pytest.raises(ValueError, match="ptr must ascend from 0"):
        make(ei, np.asarray([0, 29, 20]))
    with pytest.raises(ValueError, match="ptr must ascend from 0"):
        make(ei, ptr + 1)
    with pytest.raises(ValueError, match="graph with 2 nodes"):
        make(ei, np.asarray([0, 20, 22, 29]))
    with pytest.raises(ValueError, match=f"graph with {(1 << 20) + 1} nodes"):
        make(ei, num_nodes=(1 << 20) + 1)
    with pytest.raises(ValueError, match="too large for int32"):
        make(ei, np.arange(0, (1 << 31) + (1 << 20), 1 << 20))
    with pytest.raises(ValueError, match="pairs must be"):
        make(ei, ptr, pairs="twice")
    with pytest.raises(ValueError, match="describes no graph"):
        make(ei, np.asarray([0]))
    if not torch.cuda.is_available():   # and there is no CPU fallback behind them
        with pytest.raises(built.hip.HipExtensionError):
            make(ei, ptr)


def test_int32_limit_of_the_entries_is_checked_before_the_library(built):
    class Huge:   # stands for an edge_index of 2^30 entries: only its shape and dtype are looked at before the refusal
        shape, dtype = (2, 1 << 30), torch.int64
    with pytest.raises(ValueError, match="too large for int32"):
        built.GraphBatch.from_edge_index(Huge(), num_nodes=1 << 20, pairs="once")
    Huge.shape = (2, 1 << 31)
    with pytest.raises(ValueError, match="too large for int32"):
        built.GraphBatch.from_edge_index(Huge(), num_nodes=1 << 20)


# ---- status codes and sizes
def csr_args(**kw):
    a = dict(B=2, R=29, E=100, goff=SOME, src=SOME, dst=SOME, w=None, rowptr=SOME, lcol=SOME, gcol=SOME, vals=None,
             dinv=SOME, report=SOME, ws=SOME, ws_bytes=BIG)
    a.update(kw)
    return [a[k] for k in ("B", "R", "E", "goff", "src", "dst", "w", "rowptr", "lcol", "gcol", "vals", "dinv", "report", "ws",
                           "ws_bytes")] + [None]


def table_args(**kw):
    a = dict(B=2, R=29, n_max=20, goff=SOME, rowptr=SOME, lcol=SOME, vals=None, W=8, NS=7, ell=SOME, ell_vals=None,
             ovf_ptr=None, ovf_ids=None, ovf_vals=None, ovf_blocks=0, ws=SOME, ws_bytes=BIG)
    a.update(kw)
    return [a[k] for k in ("B", "R", "n_max", "goff", "rowptr", "lcol", "vals", "W", "NS", "ell", "ell_vals", "ovf_ptr",
                           "ovf_ids", "ovf_vals", "ovf_blocks", "ws", "ws_bytes")] + [None]


def test_argument_errors_need_no_gpu(built):
    lib = built.hip.load()
    csr, table = lib.gmc_batch_build_csr, lib.gmc_batch_build_table
    NULL, SHAPE, WORKSPACE, GRAPH_SIZE = -1, -2, -5, -6
    for name in ("goff", "src", "dst", "rowptr", "lcol", "gcol", "dinv", "report", "ws"):
        assert csr(*csr_args(**{name: None})) == NULL, name
    assert csr(*csr_args(w=SOME)) == NULL                        # weights in, no room for them out
    assert csr(*csr_args(B=-1)) == SHAPE
    assert csr(*csr_args(R=-1)) == SHAPE and csr(*csr_args(R=1)) == SHAPE   # fewer rows than graphs
    assert csr(*csr_args(E=-1)) == SHAPE and csr(*csr_args(E=1 << 31)) == SHAPE
    assert csr(*csr_args(B=-1, goff=None)) == NULL               # pointers first, as everywhere in the library
    need = lib.gmc_batch_build_workspace_bytes(2, 29, 100)
    assert csr(*csr_args(ws_bytes=need - 1)) == WORKSPACE
    assert csr(*csr_args(B=0, R=0, E=0)) == 0                    # nothing to do, nothing launched
    assert csr(*csr_args(B=0, R=0, E=0, src=None, dst=None, lcol=None, gcol=None)) == 0
    assert csr(*csr_args(B=0, R=0, E=0, ws_bytes=0)) == WORKSPACE

    for name in ("goff", "rowptr", "lcol", "ell", "ws"):
        assert table(*table_args(**{name: None})) == NULL, name
    assert table(*table_args(vals=SOME)) == NULL                 # weights without ell_vals
    assert table(*table_args(ovf_ptr=SOME)) == NULL              # ovf_ptr without the lists
    assert table(*table_args(ovf_ptr=SOME, ovf_ids=SOME, vals=SOME, ell_vals=SOME)) == NULL   # ... without ovf_vals
    for W in (0, 7, 9, 12, 32, -8):
        assert table(*table_args(W=W)) == SHAPE, W
    assert table(*table_args(NS=0)) == SHAPE and table(*table_args(NS=9)) == SHAPE
    assert table(*table_args(W=16, NS=17)) == SHAPE
    assert table(*table_args(B=-1)) == SHAPE and table(*table_args(R=1)) == SHAPE
    assert table(*table_args(ovf_blocks=-1)) == SHAPE
    assert table(*table_args(n_max=2)) == GRAPH_SIZE and table(*table_args(n_max=65532)) == GRAPH_SIZE
    assert table(*table_args(W=7, n_max=2)) == SHAPE             # sizes before the graph size
    assert table(*table_args(ws_bytes=need - 1)) == WORKSPACE
    assert table(*table_args(B=0, R=0)) == 0


def test_workspace_size_is_positive_and_monotone(built):
    size = built.hip.load().gmc_batch_build_workspace_bytes
    assert size(0, 0, 0) > 0 and size(1, 3, 4) > 0
    assert size(-1, 3, 4) == 0 and size(1, -3, 4) == 0 and size(1, 3, -4) == 0 and size(1, 3, 1 << 31) == 0
    rows = [3, 4, 100, 1023, 1024, 1025, 4096, 1 << 16, 1 << 20, (1 << 20) + 1, 160000]
    for E in (0, 10, 1 << 20, (1 << 31) - 1):
        sizes = [size(1, R, E) for R in sorted(rows)]
        assert sizes == sorted(sizes) and len(set(sizes)) > len(sizes) // 2, sizes
        assert all(s % 16 == 0 for s in sizes)
    for R in rows:
        by_e = [size(1, R, E) for E in (0, 10, 1 << 20, (1 << 31) - 1)]
        assert by_e == sorted(by_e), by_e          # (the workspace holds per-row words only: it does not grow with E)
        assert size(1, R, 0) <= 17 * R + 4096      # the 'about 16 bytes per row' of the header
    assert len(built.hip.BB_REPORT) < built.hip.BB_REPORT_WORDS == 20


# ---- the kernels
KERNELS = {"bb_init_kernel": 1, "bb_count_kernel": 1, "bb_scan_sums_kernel": 2, "bb_scan_top_kernel": 1,
           "bb_scan_add_kernel": 2, "bb_scatter_kernel": 2, "bb_sort_group_kernel": 2, "bb_sort_wave_kernel": 2,
           "bb_sort_wg_kernel": 2, "bb_sort_global_kernel": 2, "bb_validate_kernel": 2, "bb_ovf_fill_kernel": 2,
           "bb_arrange_kernel": 4}


def test_every_kernel_is_in_the_code_object_and_none_uses_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = [s for s in util.kernel_symbols(lib_path) if "bb_" in s]
    for W in (8, 16):
        for weights in ("true", "false"):
            assert any(f"bb_arrange_kernel<{W}, {weights}>" in s for s in names), (W, weights)
    for kernel in ("bb_scatter_kernel", "bb_sort_group_kernel", "bb_sort_wave_kernel", "bb_sort_wg_kernel",
                   "bb_sort_global_kernel", "bb_validate_kernel", "bb_ovf_fill_kernel"):
        for weights in ("true", "false"):
            assert any(f"{kernel}<{weights}>" in s for s in names), (kernel, weights)
    seen = dict.fromkeys(KERNELS, 0)
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
            for kernel in KERNELS:
                if kernel in fields.get(".name", ""):
                    seen[kernel] += 1
                    assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
                    assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
                    assert int(fields[".group_segment_fixed_size"]) <= 48 * 1024, fields[".name"]
    assert seen == KERNELS


def test_the_c_abi_declares_the_three_entry_points(built):
    for name in ("gmc_batch_build_workspace_bytes", "gmc_batch_build_csr", "gmc_batch_build_table"):
        assert name in built.hip.SYMBOLS and hasattr(built.hip.load(), name)
    assert C.sizeof(built.hip.GmcBatch) == C.sizeof(built.hip.GmcBatch())   # no struct change
    assert built.hip.ABI_VERSION == 200
