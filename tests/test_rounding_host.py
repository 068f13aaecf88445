"""CPU checks of the rounding by conditional expectations (include/gcnmaxcut.h, gmc_round_order_host /
gmc_round_conditional_f32): the restatement's own properties (the class-parallel form equals the sequential one, the
rounded cut is not below the expected cut, the argmax decode does fall below it), the host colouring from K, the entry
points' argument checks (no GPU needed), the kernels' presence in the gfx950 code object and the Python refusals."""
import ctypes as C
import subprocess

import networkx as nx
import numpy as np
import pytest

from oracle import ref_dense as R
from tests import refine_ref as RR
from tests import rounding_ref as CR
from tests import util
from tests.test_refine_host import gnp_graph, handles_of, host_order, hub_graph, loop_graph
from tests.test_seeded_sampler_host import golden_graphs

# The slack of the guarantee, in units of the graph's absolute edge weight W_abs.  An fp32 decision loses at most
# 2 (deg + 1) 2^-24 of a node's absolute weighted degree, a softmax row is off 1 by a few 2^-24; summed over the nodes
# that is below 1e-5 W_abs for degrees up to 40.  5e-5 is the bar tests/test_gpu_kway.py uses for relaxed losses.
SLACK = 5e-5


def test_case_inputs_stay_clear_of_denormals():
    cases = CR.cases()
    assert len(cases) == 48 and {c[0] for c in cases} == {2, 3, 4, 8}
    assert any(c[4] is None for c in cases) and any(c[4] is not None and (c[4] < 0).any() and (c[4] > 0).any() for c in cases)
    for case in cases:
        CR.check_case_inputs(*case)


def test_class_parallel_form_equals_the_sequential_one():
    for K, n, rowptr, col, w, P in CR.cases():
        seq = CR.round_sequential(n, rowptr, col, w, P, K)
        assert (seq[:K] == np.arange(K)).all() and seq.min() >= 0 and seq.max() < K
        assert (CR.round_by_classes(n, rowptr, col, w, P, K) == seq).all(), (K, n)
        poisoned = P.copy()
        poisoned[:K] = np.nan                                          # the terminals' rows are never read
        assert (CR.round_sequential(n, rowptr, col, w, poisoned, K) == seq).all()


def test_rounded_cut_is_not_below_the_expected_cut_and_argmax_is():
    margins, below = [], 0
    for K, n, rowptr, col, w, P in CR.cases():
        W_abs = CR.abs_weight(rowptr, col, w)
        expected = CR.expected_cut(n, rowptr, col, w, P, K)
        rounded = CR.round_sequential(n, rowptr, col, w, P, K)
        c0 = CR.cut(rowptr, col, w, rounded)
        assert c0 >= expected - SLACK * W_abs, (K, n, c0, expected)
        margins.append((c0 - expected) / W_abs)
        refined, sweeps = CR.descent(n, rowptr, col, w, rounded, K, 100)
        assert 1 <= sweeps < 100 and (refined[:K] == np.arange(K)).all()
        # after the descent the cut is no smaller
        assert CR.cut(rowptr, col, w, refined) >= c0
        same, none = CR.descent(n, rowptr, col, w, rounded, K, 0)
        assert none == 0 and (same == rounded).all()
        if CR.cut(rowptr, col, w, CR.argmax_assignment(P, K)) < expected - SLACK * W_abs:
            below += 1
    print(f"smallest margin {min(margins):+.4f} W_abs; argmax below the expected cut on {below} of {len(margins)} cases")
    assert below >= 1                                                  # the inequality is not vacuous


def order_from_K(ba, K, cap=None):
    from gcn_max_cut_amd import hip
    order = np.full(max(ba.R, 1), -7, np.int32)
    cgoff = np.full(ba.B + 1, -7, np.int32)
    cptr = np.full(ba.R + ba.B if cap is None else cap, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    go = ba.goff.astype(np.int32)
    rc = hip.load().gmc_round_order_host(ba.B, p(go), p(ba.rowptr), p(ba.lcol), K, p(order), p(cgoff), p(cptr), cptr.size)
    return rc, order, cgoff, cptr


ORDER_BATCHES = {
    "golden": golden_graphs,
    "hub": lambda: [hub_graph(400, 7, 5)],
    "gnp": lambda: [gnp_graph(800, 0.01, 4)],
    "self_loops": lambda: [loop_graph(200, 6, 6)],
    "mixed": lambda: [nx.complete_graph(8), R.regular_graph(50, 6, 7), nx.complete_graph(9), R.regular_graph(100, 3, 9)],
}


@pytest.mark.parametrize("name", sorted(ORDER_BATCHES))
def test_round_order_host(built, name):
    from gcn_max_cut_amd.graph import BatchArrays
    hs = handles_of(ORDER_BATCHES[name]())
    ba = BatchArrays(hs)
    want = host_order(ba)
    got = order_from_K(ba, 3)
    assert want[0] == got[0] == 0
    for a, b in zip(want[1:], got[1:]):                                # K = 3: gmc_refine_order_host, array for array
        assert a.dtype == b.dtype and (a == b).all()
    ref3 = RR.order_of_batch(hs)
    for a, b in zip(ref3, CR.order_of_batch(hs, 3)):
        assert (a == b).all()
    for K in (2, 5):
        if min(h.n for h in hs) < K:
            continue
        rc, order, cgoff, cptr = order_from_K(ba, K)
        assert rc == 0
        ref_order, ref_cgoff, ref_cptr = CR.order_of_batch(hs, K)
        moving = ba.R - K * ba.B
        assert (order[:moving] == ref_order).all() and (order[moving:] == -7).all()
        assert (cgoff == ref_cgoff).all()
        assert (cptr[:cgoff[-1]] == ref_cptr).all() and (cptr[cgoff[-1]:] == -7).all()


def test_round_order_host_status_codes(built):
    from gcn_max_cut_amd.graph import BatchArrays
    lib = built.hip.load()
    null = C.c_void_p(None)
    some = (C.c_int32 * 16)()
    assert lib.gmc_round_order_host(1, null, some, some, 4, some, some, some, 16) == -1       # GMC_ERR_NULL
    assert lib.gmc_round_order_host(1, some, some, some, 4, some, some, null, 16) == -1
    for K in (-1, 0, 1, 9):
        assert lib.gmc_round_order_host(1, some, some, some, K, some, some, some, 16) == -3   # GMC_ERR_CLASSES
    assert lib.gmc_round_order_host(-1, some, some, some, 4, some, some, some, 16) == -2      # GMC_ERR_SHAPE
    goff = (C.c_int32 * 2)(0, 3)                                                               # a three-node graph
    assert lib.gmc_round_order_host(1, goff, some, some, 4, some, some, some, 16) == -6       # fewer than K nodes
    assert lib.gmc_round_order_host(1, goff, some, some, 3, some, some, some, 16) == 0
    assert lib.gmc_round_order_host(1, goff, some, some, 2, some, some, some, 16) == 0
    goff = (C.c_int32 * 2)(0, 4097)
    assert lib.gmc_round_order_host(1, goff, some, some, 2, some, some, some, 16) == -6
    ba = BatchArrays(handles_of([R.regular_graph(60, 5, 1), nx.complete_graph(5)]))
    assert order_from_K(ba, 5, cap=ba.R + ba.B - 1)[0] == -2
    assert order_from_K(ba, 5, cap=ba.R + ba.B)[0] == 0
    assert order_from_K(ba, 6)[0] == -6
    zero = (C.c_int32 * 1)(0)
    assert lib.gmc_round_order_host(0, zero, some, some, 2, some, some, some, 0) == 0         # an empty batch


def test_round_entry_point_checks_arguments_without_a_gpu(built):
    hip = built.hip
    lib = hip.load()
    null, some = C.c_void_p(None), C.c_void_p(4096)                    # (never dereferenced: the calls fail first)
    fields = dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096)
    batch = lambda **kw: C.byref(hip.GmcBatch(**{**fields, **kw}))

    def f(b, P=some, K=3, order=some, cgoff=some, cptr=some, sweeps_max=10, assign=some, cut=some, expected=some,
          sweeps=some):
        return lib.gmc_round_conditional_f32(b, P, K, order, cgoff, cptr, sweeps_max, assign, cut, expected, sweeps, None)
    # 1. NULL pointers (before the abi word is read); expected and sweeps are the ones that may be NULL
    assert f(None) == -1
    for name in ("P", "order", "cgoff", "cptr", "assign", "cut"):
        assert f(batch(), **{name: null}) == -1, name
        assert f(batch(abi=100), **{name: null}) == -1, name
    # 2. the abi word, before the batch's pointers, the class count and the shapes
    assert f(batch(abi=100)) == -8
    assert f(batch(abi=100, lcol=None), K=9, sweeps_max=-1) == -8
    # 3. the batch's own pointers, before the class count
    for name in ("goff", "rowptr", "lcol"):
        assert f(batch(**{name: None}), K=9) == -1, name
    # 4. the class count, before the shapes
    for K in (-3, 0, 1, 9, 100):
        assert f(batch(), K=K, sweeps_max=-1) == -3, K
    # 5. shapes, before the graph size
    assert f(batch(n_max=2), sweeps_max=-1) == -2
    assert f(batch(n_max=2, B=-1)) == -2
    # 6. graph size
    assert f(batch(n_max=2)) == -6
    assert f(batch(n_max=7), K=8) == -6
    assert f(batch(n_max=4097)) == -6
    # an empty batch: nothing launched, whatever the optional outputs
    assert f(batch(B=0, R=0, n_max=0)) == 0
    assert f(batch(B=0, R=0, n_max=0), expected=null, sweeps=null) == 0
    assert {"gmc_round_order_host", "gmc_round_conditional_f32"} <= set(hip.SYMBOLS)


def test_round_kernels_are_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for K in range(2, 9):
        assert any(f"round_conditional_kernel<{K}>(" in s for s in names), (K, sorted(names))
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if "round_conditional_kernel" not in entry or ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
            if "round_conditional_kernel" not in fields.get(".name", ""):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0
            assert int(fields[".vgpr_spill_count"]) == 0
    assert seen == 7


def test_python_refusals(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = R.regular_graph(20, 3, 1)
    for K in (1, 9):
        with pytest.raises(ValueError, match="number_classes"):
            TN.conditional_rounding(np.full((20, K), 1.0 / K, np.float32), g)
    with pytest.raises(ValueError, match="at least 5 nodes"):
        TN.conditional_rounding(np.full((4, 5), 0.2, np.float32), nx.complete_graph(4))
    with pytest.raises(ValueError, match="descent_sweeps"):
        TN.conditional_rounding(np.full((20, 3), 1.0 / 3, np.float32), g, descent_sweeps=-1)
    with pytest.raises(ValueError, match="rows"):
        TN.conditional_rounding(np.full((19, 3), 1.0 / 3, np.float32), g)
    with pytest.raises(ValueError, match="descent_sweeps"):
        TN.round_dataset(None, {}, descent_sweeps=-1)
    with pytest.raises(ValueError, match="rounding_descent_sweeps"):
        TN.decode_dataset(None, {}, 4, rounding_descent_sweeps=-1)
