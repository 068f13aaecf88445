"""CPU checks of the seeded post-processing sampler (include/gcnmaxcut.h, gmc_decode_sample_seeded_f32): the product's
host forms against the restatement of tests/seeded_ref.py, statistics of the draw rule itself, the entry point's
argument checks (no GPU needed), the kernel's presence in the gfx950 code object and the probe tag."""
import ctypes as C
import itertools
import json
import os
import subprocess

import networkx as nx
import numpy as np
import pytest
import torch

from tests import refine_ref as RR
from tests import seeded_ref as SR
from tests import util

SEEDS = (0, 1, 12345, 2 ** 63 + 5)


def golden_graphs():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graphs.json")
    out = []
    for rec in json.load(open(path))["graphs"]:
        g = nx.Graph()
        g.add_nodes_from(range(rec["n"]))
        g.add_weighted_edges_from((u, v, w) for u, v, w, _cap in rec["edges"])
        out.append(g)
    return out


def softmax_rows(n, seed):
    rng = np.random.RandomState(seed)
    logits = rng.standard_normal((n, 3)) * 2.0
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def test_host_forms_equal_the_restatement(built):
    from gcn_max_cut_amd.graph import from_networkx
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    graphs = golden_graphs()
    assert len(graphs) >= 5
    for seed in SEEDS:
        indices = list(range(len(graphs))) + [159, 2 ** 31 + 7]
        got = TN.sample_keys(seed, indices)
        assert got.dtype == np.uint64 and (got == SR.keys(seed, indices)).all()
        assert len(set(got.tolist())) == len(indices)
        for index, g in enumerate(graphs):
            n = g.number_of_nodes()
            P = softmax_rows(n, 100 + index)
            P[3] = [0.25, 0.25, 0.25]                                 # a row whose sum stays below some draws
            h = from_networkx(g)
            key = SR.keys(seed, [index])[0]
            for it in (0, 1, 5, 199, 2 ** 31 - 1):
                want = SR.assignments(P, key, 1, first_iter=it)[0]
                got_a = TN.assign_partitions_seeded(P, seed, graph_index=index, iteration=it)
                assert got_a == want.tolist(), (seed, index, it)
                assert TN.calculate_cut_value(got_a, g) == RR.cut(h.rowptr, h.col, h.weight, want)
    P = softmax_rows(40, 1)
    assert TN.assign_partitions_seeded(P, -1) == TN.assign_partitions_seeded(P, 2 ** 64 - 1)   # masked to 64 bits
    assert TN.assign_partitions_seeded(P, 3, 2, 1) != TN.assign_partitions_seeded(P, 3, 2, 0)
    assert TN.assign_partitions_seeded(P[:3], 3) == [0, 1, 2]
    with pytest.raises(ValueError):
        TN.sample_keys(0, [-1])
    with pytest.raises(ValueError):
        TN.assign_partitions_seeded(P, 0, iteration=-1)


STAT_SEEDS = (0, 1, 7, 12345, 2 ** 63 + 5)
STAT_INDICES = (0, 1, 159)
# a condition on the rule, not a tuned bar: the worst figure over exactly these seeds and indices is 2.8
STAT_BOUND = 4.5


def test_statistics_of_the_draw_rule():
    """64 iterations x nodes 3..1029, every row (0.2, 0.3, 0.5): class counts within 4.5 sigma of N p; the lag-1
    correlations of u - 1/2 along nodes and along iterations as z-scores (mean product * 12 * sqrt(count): the product
    of two independent centred uniforms has standard deviation 1/12) below 4.5; iterations pairwise different; the
    streams of two graphs share no uniform."""
    iters, n = 64, 1030
    P = np.tile(np.array([0.2, 0.3, 0.5], np.float32), (n, 1))
    c0 = float(P[0, 0])
    c1 = c0 + float(P[0, 1])
    probs = (c0, c1 - c0, 1.0 - c1)
    worst = 0.0
    streams = {}
    for seed, index in itertools.product(STAT_SEEDS, STAT_INDICES):
        key = SR.keys(seed, [index])[0]
        a = SR.assignments(P, key, iters)[:, 3:]
        h = SR.hashes(key, iters, n)[:, 3:]
        u = SR.uniforms(key, iters, n)[:, 3:]
        assert u.shape == (64, 1027) and (u >= 0).all() and (u < 1).all()
        N = a.size
        for k, p in enumerate(probs):
            z = abs(int((a == k).sum()) - N * p) / np.sqrt(N * p * (1 - p))
            worst = max(worst, z)
            assert z <= STAT_BOUND, (seed, index, "class", k, z)
        c = u - 0.5
        for name, prod in (("nodes", c[:, :-1] * c[:, 1:]), ("iterations", c[:-1, :] * c[1:, :])):
            z = abs(float(prod.mean())) * 12.0 * np.sqrt(prod.size)
            worst = max(worst, z)
            assert z < STAT_BOUND, (seed, index, name, z)
        assert len({row.tobytes() for row in a}) == iters            # the 64 samples are pairwise different
        assert len({row.tobytes() for row in h}) == iters
        streams[seed, index] = h
    for seed in STAT_SEEDS:
        assert np.intersect1d(streams[seed, 0].ravel(), streams[seed, 1].ravel()).size == 0
    print(f"worst figure {worst:.2f}")


def test_seeded_entry_point_checks_arguments_without_a_gpu(built):
    hip = built.hip
    lib = hip.load()
    null, some = C.c_void_p(None), C.c_void_p(4096)                    # (never dereferenced: the calls fail first)
    fields = dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096)
    batch = lambda **kw: C.byref(hip.GmcBatch(**{**fields, **kw}))

    def f(b, P=some, gkey=some, iters=8, assign_all=some, cut_all=some, best_assign=some, best_cut=some,
          best_iter=some):
        return lib.gmc_decode_sample_seeded_f32(b, P, gkey, iters, assign_all, cut_all, best_assign, best_cut,
                                                best_iter, None)
    # 1. NULL pointers (before the abi word is read); assign_all is the only one that may be NULL
    assert f(None) == -1
    for name in ("P", "gkey", "cut_all", "best_assign", "best_cut", "best_iter"):
        assert f(batch(), **{name: null}) == -1, name
        assert f(batch(abi=100), **{name: null}) == -1, name
    # 2. the abi word, before the batch's pointers and the shapes
    assert f(batch(abi=100)) == -8
    assert f(batch(abi=100, lcol=None), iters=0) == -8
    # 3. the batch's own pointers, before the shapes
    for name in ("goff", "rowptr", "lcol"):
        assert f(batch(**{name: None}), iters=0) == -1, name
    # 4. shapes, before the graph size
    assert f(batch(n_max=2), iters=0) == -2
    assert f(batch(n_max=2, B=-1)) == -2
    # 5. graph size
    assert f(batch(n_max=2)) == -6
    assert f(batch(n_max=65536)) == -6
    # 6. an empty batch: nothing launched - with or without assign_all
    assert f(batch(B=0, R=0, n_max=0)) == 0
    assert f(batch(B=0, R=0, n_max=0), assign_all=null) == 0
    assert "gmc_decode_sample_seeded_f32" in hip.SYMBOLS


def test_seeded_kernels_are_in_the_code_object_without_scratch(built):
    """gmc_decode_sample_seeded_f32 runs the K-class sampler's two kernels at K = 3: each instantiation is in the code
    object once, without scratch, and no 3-class sampler kernel stands beside them."""
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for kernel in ("sample_seeded_k_kernel<3>", "sample_seeded_k_pick_kernel<3>"):
        assert sum(kernel + "(" in s for s in names) == 1, sorted(names)
    assert not any("sample_seeded_kernel" in s or "sample_seeded_pick_kernel" in s for s in names), sorted(names)
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if "sample_seeded_k_" not in entry or ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
            name = fields.get(".name", "")
            if "sample_seeded_k_kernelILi3E" not in name and "sample_seeded_k_pick_kernelILi3E" not in name:   # <3>
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0
            assert int(fields[".vgpr_spill_count"]) == 0
    assert seen == 2


def test_probe_tag():
    from gcn_max_cut_amd import hip
    assert hip.PROBE_TAGS.index("sample") == 18                        # GMC_K_SAMPLE
    assert hip.PROBE_TAGS.index("gemm") == 17 and hip.KERNEL_TAGS[-1] == "anneal" and "sample" not in hip.KERNEL_TAGS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gcnmaxcut.h")).read()
    assert "GMC_K_SAMPLE = 18" in header and "GMC_K_COUNT = 19" in header


def test_environment_switch_is_read_at_call_time(built, monkeypatch):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    monkeypatch.delenv(TN.SAMPLE_SEED_ENV, raising=False)
    assert TN._sample_seed(None) is None and TN._sample_seed(5) == 5 and TN._sample_seed(-1) == 2 ** 64 - 1
    monkeypatch.setenv(TN.SAMPLE_SEED_ENV, "12345")
    assert TN._sample_seed(None) == 12345 and TN._sample_seed(7) == 7  # the argument wins
    monkeypatch.setenv(TN.SAMPLE_SEED_ENV, "twelve")
    with pytest.raises(ValueError, match=TN.SAMPLE_SEED_ENV):
        TN._sample_seed(None)
    assert TN.SAMPLE_SEED_ENV.encode() not in open(built.hip.LIB_PATH, "rb").read()   # Python only


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_seeded_post_processing_has_no_cpu_fallback(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = golden_graphs()[0]
    P = softmax_rows(g.number_of_nodes(), 0)
    with pytest.raises(built.hip.HipExtensionError):
        TN.post_processing_optimization(P, g, 10, seed=1)
    with pytest.raises(built.hip.HipExtensionError):
        TN.post_processing_optimization(torch.from_numpy(P), g, 10, seed=1, graph_index=3)
