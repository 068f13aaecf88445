"""CPU-side checks of the semidefinite relaxation (include/gcnmaxcut_sdp.h, csrc/sdp.hip, maxcut.sdp_*): the ledger of the
second header, the argument checks (all answered before any HIP call), the properties of the rule itself on its numpy
restatement tests/sdp_ref.py - the value never falls, float32 stays at float64's side, the best of 64 hyperplanes
reaches the Goemans-Williamson ratio of the relaxed value - and the kernels' code object notes (no scratch).
"""
import ast
import ctypes as C
import functools
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest

from tests import sdp_ref as S
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gcnmaxcut_sdp.h")
BOUNDS = "test_gpu_bounds_sdp"

# the ledger of include/gcnmaxcut_sdp.h, as tests/test_bounds_host.py keeps the main header's
COVERED = {
    "gmc_sdp_relax_f32": (BOUNDS, "test_relax_and_round"),
    "gmc_sdp_round_f32": (BOUNDS, "test_relax_and_round"),
}
EXEMPT = {"gmc_sdp_workspace_bytes": "a size query"}


def declarations(path=HEADER):
    code = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"(?:^|\n)\s*(?:int|size_t)\s+(gmc_\w+)\s*\(([^;{]*?)\)\s*;", code))


def test_ledger_of_the_second_header(built):
    names = declarations()
    assert names == sorted(built.hip.SDP_SYMBOLS) and len(names) == 3
    lib = built.hip.load()
    for name in names:
        assert hasattr(lib, name), name
        assert (name in COVERED) != (name in EXEMPT), name
    assert set(COVERED) | set(EXEMPT) == set(names)
    # the main header and its table gain no name
    main = declarations(os.path.join(ROOT, "include", "gcnmaxcut.h"))
    assert not set(names) & set(main) and not set(names) & set(built.hip.SYMBOLS)
    for name, (module, fn) in COVERED.items():
        tree = ast.parse(open(os.path.join(ROOT, "tests", module + ".py")).read())
        assert fn in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (name, fn)
    # the size query takes no device pointer: the struct's scalars only
    b = built.hip.GmcBatch(B=3, R=1000, n_max=600)
    assert lib.gmc_sdp_workspace_bytes(C.byref(b), 16) == 4 * 8 == lib.gmc_sdp_workspace_bytes(C.byref(b), 64)
    assert lib.gmc_sdp_workspace_bytes(C.byref(b), 48) == 0 and lib.gmc_sdp_workspace_bytes(None, 16) == 0
    assert lib.gmc_sdp_workspace_bytes(C.byref(built.hip.GmcBatch(abi=100, B=3, R=1000)), 16) == 0
    assert lib.gmc_sdp_workspace_bytes(C.byref(built.hip.GmcBatch(B=-1, R=10)), 16) == 0


def test_argument_checks_answer_before_any_hip_call(built):
    lib = built.hip.load()
    some = C.c_void_p(4096)          # (never dereferenced: the calls fail first)
    G = built.hip.GmcBatch
    good = dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096, gcol=4096)

    def relax(batch=None, rank=16, terminals=0, order=some, gkey=some, init=1, sweeps=1, classes=3, V=some, value=some,
              ws=some, ws_bytes=1 << 20):
        b = C.byref(batch if batch is not None else G(**good))
        return lib.gmc_sdp_relax_f32(b, rank, terminals, None, order, some, some, classes, gkey, init, sweeps, V, value, ws,
                                     ws_bytes, None)

    def rounding(batch=None, rank=16, terminals=0, V=some, gkey=some, first=0, planes=4, assign=some):
        b = C.byref(batch if batch is not None else G(**good))
        return lib.gmc_sdp_round_f32(b, rank, terminals, V, gkey, first, planes, assign, None)

    assert lib.gmc_sdp_relax_f32(None, 16, 0, None, some, some, some, 3, some, 1, 1, some, some, some, 64, None) == -1
    assert relax(order=None) == -1 and relax(V=None) == -1 and relax(value=None) == -1 and relax(ws=None) == -1
    assert relax(gkey=None) == -1                                  # init = 1 needs the keys
    assert relax(batch=G(abi=100, **good)) == -8
    assert relax(batch=G(**dict(good, gcol=None))) == -1
    for bad in (0, 8, 17, 48, 128, -16):
        assert relax(rank=bad) == -2 and rounding(rank=bad) == -2
    assert relax(sweeps=-1) == -2 and relax(classes=-1) == -2 and relax(terminals=2) == -2 and relax(init=2) == -2
    assert relax(batch=G(**dict(good, B=-1))) == -2
    assert relax(batch=G(**dict(good, n_max=0))) == -6 and relax(batch=G(**dict(good, n_max=1)), terminals=1) == -6
    assert relax(batch=G(**dict(good, n_max=(1 << 20) + 1))) == -6
    assert relax(V=C.c_void_p(4100)) == -4 and relax(ws=C.c_void_p(4104)) == -4
    assert relax(ws_bytes=15) == -5 and relax(batch=G(**dict(good, R=-1))) == -5
    assert relax(batch=G(**dict(good, B=0, R=0, n_max=0))) == 0    # nothing to do, nothing launched
    # NULL comes before the abi word, the abi word before the shape, the shape before the size
    assert relax(batch=G(abi=100, **good), V=None, rank=5) == -1 and relax(batch=G(abi=100, **good), rank=5) == -8
    assert relax(batch=G(**dict(good, n_max=0)), rank=5) == -2 and relax(batch=G(**dict(good, n_max=0)), ws_bytes=0) == -6

    assert lib.gmc_sdp_round_f32(None, 16, 0, some, some, 0, 4, some, None) == -1
    assert rounding(V=None) == -1 and rounding(gkey=None) == -1 and rounding(assign=None) == -1
    assert rounding(batch=G(abi=100, **good)) == -8 and rounding(batch=G(**dict(good, rowptr=None))) == -1
    assert rounding(first=-1) == -2 and rounding(planes=-1) == -2 and rounding(first=(1 << 31) - 2, planes=2) == -2
    assert rounding(terminals=-1) == -2 and rounding(batch=G(**dict(good, n_max=1)), terminals=1) == -6
    assert rounding(V=C.c_void_p(4100)) == -4
    assert rounding(planes=0) == 0 and rounding(batch=G(**dict(good, B=0, R=0, n_max=0))) == 0


def test_python_refusals(built):
    mc = built.maxcut
    assert [mc._sdp_rank(None, n) for n in (3, 112, 113, 480, 481, 1984, 1985, 2048, 1 << 20)] == \
        [16, 16, 32, 32, 64, 64, 64, 64, 64]
    assert "2,048" in mc.sdp_relax.__doc__ and "certificate" in mc.solve_sdp.__doc__
    for bad in (8, 48, 128):
        with pytest.raises(ValueError, match="rank"):
            mc._sdp_rank(bad, 100)
    assert "relaxed_value" in mc.SdpResult.__dataclass_fields__ and "rounded_cut" in mc.SdpResult.__dataclass_fields__


# ---- the rule itself, on the restatement ---------------------------------------------------------------------------------
SWEEPS = 50
CASES = tuple((n, rank, kind) for n, rank in ((60, 16), (200, 32)) for kind in ("unit", "signed", "cost"))


def host_batch(pkg, graphs):
    return pkg.graph.BatchArrays([pkg.graph.from_networkx(g) for g in graphs])


@functools.lru_cache(maxsize=None)
def relaxed(n, rank, kind):
    """(h, cost, keys, float32 (V, value, trace), float64 (V, value, trace)) of one 7-regular case, computed once."""
    import gcn_max_cut_amd as pkg
    g = nx.random_regular_graph(7, n, seed=n)
    if kind == "signed":
        rng = np.random.RandomState(n)
        for u, v in g.edges():
            g[u][v]["weight"] = float(rng.choice([-1.0, 1.0]))
    h = host_batch(pkg, [g])
    cost = np.random.RandomState(5).uniform(-1, 1, (n, 2)).astype(np.float32) if kind == "cost" else None
    keys = np.array([0x0123456789ABCDEF + n], np.uint64)
    f32 = S.relax(pkg, h, rank, False, cost, keys, SWEEPS, values=True)
    f64 = S.relax(pkg, h, rank, False, cost, keys, SWEEPS, dtype=np.float64, values=True)
    return h, cost, keys, f32, f64


@pytest.mark.parametrize("n,rank,kind", CASES)
def test_the_value_never_falls(built, n, rank, kind):
    _, _, _, f32, f64 = relaxed(n, rank, kind)
    for trace in (f32[2], f64[2]):
        steps = np.diff(np.array([float(v[0]) for v in trace]))
        assert steps.size == SWEEPS and steps.min() >= 0.0, (steps.min(), int(steps.argmin()))


# the worst of the six cases, as DESIGN.md section 38 records them; the bar is four times that
WORST_DV, WORST_REL = 2.2e-7, 8.6e-8


def test_float32_against_float64(built):
    worst_dv = worst_rel = 0.0
    for case in CASES:
        _, _, _, f32, f64 = relaxed(*case)
        dv = float(np.abs(f32[0].astype(np.float64) - f64[0]).max())
        rel = abs(float(f32[1][0]) - float(f64[1][0])) / abs(float(f64[1][0]))
        print(case, "max |V32 - V64|", dv, "relative value difference", rel)
        worst_dv, worst_rel = max(worst_dv, dv), max(worst_rel, rel)
    print("worst", worst_dv, worst_rel)
    assert worst_dv <= 4 * WORST_DV and worst_rel <= 4 * WORST_REL, (worst_dv, worst_rel)


@pytest.mark.parametrize("n,rank", ((60, 16), (200, 32)))
def test_best_of_64_planes_reaches_the_gw_ratio(built, n, rank):
    """Unit weights only: the bound of Goemans and Williamson needs non-negative weights."""
    h, _, keys, f32, _ = relaxed(n, rank, "unit")
    planes = S.round_planes(h, rank, False, f32[0], keys, 0, 64)
    cuts = np.array([S.cut_of(h, planes[m])[0] for m in range(64)])
    value = float(f32[1][0])
    print(n, rank, "value", value, "best", cuts.max() / value, "mean", cuts.mean() / value)
    assert cuts.max() >= 0.878 * value
    # and a plane's bytes do not depend on the window it is asked in
    assert (S.round_planes(h, rank, False, f32[0], keys, 40, 3) == planes[40:43]).all()


def test_the_restatement_follows_the_header():
    """The pieces a reader can check by hand: the butterfly's order, the init's integers, terminals, the plane tag."""
    x = np.array([1e8, 1.0, -1e8, 1.0], np.float32)
    assert S.butterfly(x)[0] == np.float32(np.float32(1e8) + np.float32(-1e8)) + (np.float32(1) + np.float32(1))
    r = np.random.RandomState(1).normal(size=(5, 3, 64)).astype(np.float32) * np.float32(1e3)
    for width in (16, 32, 64):     # the halving sum the restatement uses is entry 0 of the butterfly, bit for bit
        assert (S.total(r[..., :width]) == S.butterfly(r[..., :width])[..., 0]).all()
    text = " ".join(open(HEADER).read().split())
    assert "0x9E3779B97F4A7C15" in text and f"0x{int(S.PLANE_TAG):016X}ULL" in text

    class One:
        B, R, goff = 1, 3, np.array([0, 3])
    V = S.init(One, 16, True, np.array([7], np.uint64))
    assert V[0].tolist() == [1.0] + [0.0] * 15 and V[1].tolist() == [-1.0] + [0.0] * 15 and not np.signbit(V[1, 1:]).any()
    i = int(S.mix64(np.array([7], np.uint64) + S.GOLD * np.array([2 * 16 + 3 + 1], np.uint64))[0]) >> 40
    row = S.init(One, 16, False, np.array([7], np.uint64))[2]
    assert abs(float(np.linalg.norm(row.astype(np.float64))) - 1.0) < 1e-6 and np.sign(row[3]) == np.sign(i - (1 << 23))
    hs = S.normals(np.uint64(7), 16, 5, 2)
    assert hs.shape == (2, 16) and np.abs(hs).max() < 6 * (1 << 20) and (hs == np.round(hs)).all()


KERNELS = ("sdp_init_kernel", "sdp_visit_kernel", "sdp_value_kernel", "sdp_round_kernel")


def test_kernels_are_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for kernel in KERNELS:
        for rank in (16, 32, 64):
            assert sum(f"{kernel}<{rank}>(" in s for s in names) == 1, (kernel, rank)
    assert sum("sdp_fold_kernel(" in s for s in names) == 1
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            if not any(k in fields.get(".name", "") for k in KERNELS + ("sdp_fold_kernel",)):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
            assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
    assert seen == 3 * len(KERNELS) + 1
