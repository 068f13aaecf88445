"""CPU checks of the annealing over decoded partitions (include/gcnmaxcut.h, gmc_refine_anneal_f32): the vectorised
restatement against its one-node-at-a-time definition, the hash and the level index against hand-worked integers, the
level table and the schedule, the entry point's argument checks (no GPU needed), the kernel's presence in the gfx950
code object, and the quality the restatement reaches on the CPU."""
import ctypes as C
import subprocess

import networkx as nx
import numpy as np
import pytest

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import refine_ref as RR
from tests import util
from tests.test_refine_host import handles_of, loop_graph


def dyadic_weights(h, seed):
    """One multiple of 1/8 in 1/8 .. 4 per undirected edge, as the CSR's fp32 values."""
    rng = np.random.RandomState(seed)
    w = np.zeros(h.col.size, np.float32)
    rows = np.repeat(np.arange(h.n), np.diff(h.rowptr))
    key = {}
    for e, (a, b) in enumerate(zip(rows, h.col)):
        w[e] = key.setdefault((min(a, b), max(a, b)), rng.randint(1, 33) / 8.0)
    return w


SMALL = {
    "n3": lambda: (nx.complete_graph(3), None),
    "n4": lambda: (nx.complete_graph(4), None),
    "regular": lambda: (R.regular_graph(40, 5, 1), None),
    "self_loops": lambda: (loop_graph(36, 4, 2), None),
    "dyadic": lambda: (R.regular_graph(30, 6, 3), 4),
}


@pytest.mark.parametrize("case", sorted(SMALL))
def test_vectorised_restatement_equals_the_sequential_definition(case):
    g, wseed = SMALL[case]()
    h = handles_of([g])[0]
    w = None if wseed is None else dyadic_weights(h, wseed)
    rng = np.random.RandomState(len(case))
    cands = 5
    A = rng.randint(0, 3, (cands, h.n)).astype(np.int8)
    if h.n > 6:
        A[1, 5] = 3                                                    # a byte of no class: counts for nothing, moves
    inv_t, table = AR.schedule(12), AR.levels()
    for max_descent in (0, 100):
        out, snap, sweeps = AR.anneal(h.n, h.rowptr, h.col, w, A, inv_t, table, 9, max_descent)
        for i in range(cands):
            a, sn, sw = AR.sequential(h.n, h.rowptr, h.col, w, A[i].tolist(), inv_t, table, 9, max_descent, cand=i)
            assert out[i].tolist() == a and snap[i] == sn and sweeps[i] == sw, (case, i)
        assert (out[:, :3] == A[:, :3]).all()
        if h.n > 6 and max_descent:
            assert 0 <= out[1, 5] <= 2
    # the candidate's index is part of the random stream, its place in the array is not
    out2, snap2, _ = AR.anneal(h.n, h.rowptr, h.col, w, A[3:], inv_t, table, 9, 100, cand_ids=[3, 4])
    assert (out2 == out[3:]).all() and (snap2 == snap[3:]).all()
    # no annealing sweeps: the local search
    plain, _snap, sw0 = AR.anneal(h.n, h.rowptr, h.col, w, A, inv_t[:0], table, 9, 100)
    ref, ref_sw = RR.refine(h.n, h.rowptr, h.col, w, A, 100)
    assert (plain == ref).all() and (sw0 == ref_sw).all() and (_snap == 0).all()


def test_hash_and_level_index_against_hand_worked_integers():
    M = (1 << 64) - 1
    # mix64(0) = 0; mix64(1) worked step by step
    assert AR.mix64_int(0) == 0
    z = 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    assert z == 0xBF58476D1CE4E5B9
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    assert AR.mix64_int(1) == z == 0x5692161D100B05E5
    # splitmix64's first output for seed 0 is mix64(GOLD): the published value
    assert AR.mix64_int(AR.GOLD) == 0xE220A8397B1DCDAF
    # seed 0, candidate 0, sweep 0, node 0: ctr = 0, h = mix64(GOLD * 1), top 10 bits
    assert AR.level_index(0, 0, 0, 0) == 0xE220A8397B1DCDAF >> 54 == 904
    # the fields of the counter do not overlap: node 4095 of sweep 0 is not node 0 of sweep 1
    assert (2 << 32 | 5 << 12 | 7) + 1 == 0x0000000200005008
    assert AR.level_index(3, 2, 5, 7) == AR.mix64_int(3 + AR.GOLD * 0x0000000200005008) >> 54
    # numpy form == integer form, high seed bits and the largest fields included
    for seed in (0, 1, (1 << 64) - 1, 0x123456789ABCDEF0):
        for cand, s, v in ((0, 0, 3), (200, 99, 4095), (1000, (1 << 20) - 1, 17)):
            got = AR.level_indices(seed, [cand], s, [v])
            assert got.shape == (1, 1) and int(got[0, 0]) == AR.level_index(seed, cand, s, v)
            assert 0 <= int(got[0, 0]) < 1024
    # the restatement's mix64 is the one tests/util.py states for the dropout mask
    zs = np.array([0, 1, AR.GOLD, M], np.uint64)
    assert [int(x) for x in util.mix64(zs)] == [AR.mix64_int(int(x)) for x in zs]


def test_levels_and_schedule(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    lv = TN.anneal_levels()
    assert lv.dtype == np.float32 and lv.shape == (1024,) == (built.hip.ANNEAL_LEVELS,)
    assert (np.diff(lv) < 0).all() and lv[-1] > 0
    assert lv[0] == np.float32(-np.log(0.5 / 1024)) and lv[-1] == np.float32(-np.log(1023.5 / 1024))
    assert (lv == AR.levels()).all()
    inv = TN.anneal_schedule(100)
    assert inv.dtype == np.float32 and inv.shape == (100,)
    assert (np.diff(inv) > 0).all()
    assert inv[0] == np.float32(1 / 1.5) and abs(inv[-1] - 1 / 0.15) <= 1e-6 * (1 / 0.15)
    assert (inv == AR.schedule(100)).all()
    one = TN.anneal_schedule(1)
    assert one.shape == (1,) and one[0] == np.float32(1 / 1.5)
    assert TN.anneal_schedule(0).shape == (0,)
    scaled = TN.anneal_schedule(30, 2.0, 0.1, scale=2.0)
    assert scaled[0] == np.float32(0.25) and abs(scaled[-1] - 5.0) <= 1e-6 * 5.0
    assert (scaled == AR.schedule(30, 2.0, 0.1, 2.0)).all()
    with pytest.raises(ValueError):
        TN.anneal_schedule(-1)
    with pytest.raises(ValueError):
        TN.anneal_schedule(10, t_end=0.0)


def test_anneal_entry_point_checks_arguments_without_a_gpu(built):
    hip = built.hip
    lib = hip.load()
    null, some = C.c_void_p(None), C.c_void_p(4096)                    # (never dereferenced: the calls fail first)
    mk = lambda **kw: hip.GmcBatch(**{**dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096), **kw})
    b = mk()

    def f(batch, order=some, cgoff=some, cptr=some, cands=4, assign=some, inv_temp=some, sweeps=10, levels=some,
          descent=10, cut_all=some, best_assign=some, best_cut=some, best_idx=some):
        return lib.gmc_refine_anneal_f32(batch, order, cgoff, cptr, cands, assign, inv_temp, sweeps, levels, 7, descent,
                                         cut_all, best_assign, best_cut, best_idx, null, null, None)
    for name in ("order", "cgoff", "cptr", "assign", "inv_temp", "levels", "cut_all", "best_assign", "best_cut", "best_idx"):
        assert f(C.byref(b), **{name: null}) == -1, name                # GMC_ERR_NULL
    assert f(None) == -1
    assert f(C.byref(mk(lcol=None))) == -1
    assert f(C.byref(mk(abi=100))) == -8                               # GMC_ERR_ABI
    assert f(C.byref(b), cands=0) == -2                                # GMC_ERR_SHAPE
    assert f(C.byref(b), sweeps=-1) == -2
    assert f(C.byref(b), descent=-1) == -2
    assert f(C.byref(b), sweeps=1 << 20) == -2                         # the counter keeps 20 bits for the sweep
    assert f(C.byref(mk(n_max=4097))) == -6                            # GMC_ERR_GRAPH_SIZE
    assert f(C.byref(mk(n_max=2))) == -6
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096)
    assert f(C.byref(empty)) == 0                                      # nothing launched
    assert f(C.byref(empty), sweeps=0, inv_temp=null, levels=null) == 0   # no annealing: neither table is needed
    assert f(C.byref(empty), sweeps=(1 << 20) - 1) == 0
    assert hip.KERNEL_TAGS[-1] == "anneal" and hip.KERNEL_TAGS.index("anneal") == 16
    assert hip.KERNEL_TAGS.index("refine") == 15
    assert "gmc_refine_anneal_f32" in hip.SYMBOLS


def test_staging_follows_the_lds_budget(built):
    """gmc_refine_anneal_staged (host query): n = 1000, d = 7 keeps its CSR in LDS, n = 4096 and a weighted n = 1000
    batch of degree 12 do not; bad arguments are refused."""
    hip = built.hip
    lib = hip.load()
    q = lambda **kw: lib.gmc_refine_anneal_staged(C.byref(hip.GmcBatch(**kw)))
    assert q(n_max=1000, nnz_max=7000) == 1
    assert q(n_max=1000, nnz_max=7000, vals=4096) == 0
    assert q(n_max=500, nnz_max=3500, vals=4096) == 1
    assert q(n_max=1000, nnz_max=12000) == 1
    assert q(n_max=4096, nnz_max=4096 * 7) == 0
    assert q(n_max=3, nnz_max=6) == 1
    assert q(n_max=3, nnz_max=0) == 0
    assert q(n_max=2) == -6 and q(n_max=4097) == -6 and q(abi=100, n_max=10) == -8
    assert lib.gmc_refine_anneal_staged(None) == -1


def test_anneal_kernel_is_in_the_code_object_without_scratch(built):
    """gmc_refine_anneal_f32 runs the K-class annealing kernel at K = 3: that instantiation is in the code object once,
    without scratch, and no 3-class annealing kernel stands beside it."""
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    assert sum("anneal_k_kernel<3>" in s for s in names) == 1, sorted(names)
    assert not any("anneal_kernel" in s or "anneal_pick_kernel" in s for s in names), sorted(names)
    assert sum("refine_local_kernel" in s for s in names) == 1
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if not ("anneal_k_kernel" in entry and ".name:" in entry):
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
            if "anneal_k_kernelILi3E" not in fields.get(".name", ""):   # the mangled <3>
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0
            assert int(fields[".vgpr_spill_count"]) == 0
    assert seen == 1


@pytest.mark.parametrize("graph_seed", [100, 101])
def test_worst_annealed_candidate_beats_the_best_local_search_candidate(graph_seed):
    """7-regular, n = 500, 201 uniform random candidates (nodes 0..2 fixed), 100 sweeps from T = 1.5 to 0.15, seed 1:
    the worst annealed cut exceeds the best local-search cut over the same candidates (no tolerance)."""
    g = nx.random_regular_graph(7, 500, seed=graph_seed)
    h = handles_of([g])[0]
    A = np.random.RandomState(0).randint(0, 3, (201, 500)).astype(np.int8)
    A[:, :3] = [0, 1, 2]
    local, _sw = RR.refine(h.n, h.rowptr, h.col, None, A, 100)
    local_cuts = AR.cuts_f32(h.rowptr, h.col, None, local)
    out, snap, sweeps = AR.anneal(h.n, h.rowptr, h.col, None, A, AR.schedule(100), AR.levels(), 1, 100)
    cuts = AR.cuts_f32(h.rowptr, h.col, None, out)
    print(f"seed {graph_seed}: local search best {local_cuts.max()} mean {local_cuts.mean():.1f}; "
          f"annealed best {cuts.max()} mean {cuts.mean():.1f} worst {cuts.min()}")
    assert cuts.min() > local_cuts.max()
    assert (cuts >= AR.cuts_f32(h.rowptr, h.col, None, A)).all()
    assert (sweeps < 100).all() and (out[:, :3] == A[:, :3]).all()
    for a in out[:5]:
        assert RR.best_single_move_gain(h.n, h.rowptr, h.col, None, a.tolist()) == 0
