"""Guard-band tests of include/gcnmaxcut_bifurcation.h's two device entry points, in the manner of
tests/test_gpu_bounds_dense.py: the matrices W [B][n][ld] at exactly that size, node costs [B * n][2], the pump table
[steps], the planes x and y at exactly gmc_dense_sb_state_bytes, assign [cands][B * n] and the workspace at exactly
gmc_dense_sb_workspace_bytes come from one arena with 4096-byte bands (tests/arena.py); each case runs on plain tensors
and on arenas filled 0xFF and 0x00, and tests/bounds.run_case asserts the byte equalities (every status GMC_OK, no band
touched, no input changed, the three runs' outputs equal).  The workspace is handed out holding the fill - poisoned, not
zeroed: a sign byte read before it is written would make the 0xFF run and the 0x00 run differ.

n = 2, 63, 65, 130 and 257; ld = n (the last row ends the buffer) and ld > n (rows that are not 16-byte aligned); B = 1
and 3; cands = 1, 5, 17, 65 (a partial column tile of each width, cs > cands); node_cost NULL and given; steps 0 (pump
NULL), 1 and 3 (both sign planes written and read); every tile of the step kernel."""
import numpy as np
import pytest
import torch

from tests import bifurcation_ref as BR
from tests import bounds as B
from tests import dense_ref as DR

pytestmark = pytest.mark.gpu
I8 = torch.int8


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    done = B.report_calls("bounds/bifurcation")
    yield built
    done()
    built.hip.load().gmc_debug_set_sb_tile(0)


def sb_case(pkg, n, problems, cands, pad=0, cost=False, steps=3):
    p = pkg.hip.ptr
    square = np.stack([DR.weights_of("real", n, 11 * n + b) for b in range(problems)])
    W = np.zeros((problems, n, n + pad), np.float32)
    W[:, :, :n] = square
    R = problems * n
    x0 = np.concatenate([BR.init(n, cands, 5, 0.1)[0] for _ in range(problems)])
    y0 = np.concatenate([BR.init(n, cands, 5, 0.1)[1] for _ in range(problems)])
    if steps == 0:
        x0 = np.random.RandomState(n).choice([-1.0, -0.0, 0.0, 0.5], size=x0.shape).astype(np.float32)
    c0 = float(np.float32(4.0 * BR.scale_c0(square)))

    def case(lib, mem):
        t_w = mem.put("W", W)
        t_cost = mem.put("node_cost", DR.cost_of("real", R, n)) if cost else None
        t_pump = mem.put("pump", BR.pump_table(steps)) if steps else None
        assert int(lib.gmc_dense_sb_state_bytes(problems, n, cands)) == x0.nbytes
        if steps:
            x, y = mem.state("x", x0), mem.state("y", y0)
        else:                                            # left untouched: inputs
            x, y = mem.put("x", x0), mem.put("y", y0)
        assign = mem.out("assign", (cands, R), I8)
        need = int(lib.gmc_dense_sb_workspace_bytes(problems, n, cands))
        ws = mem.scratch("workspace", need)
        return lib.gmc_dense_sb_f32(problems, n, p(t_w), n + pad, p(t_cost), cands, p(x), p(y), p(t_pump), steps, c0,
                                    1.25, p(ws), need, p(assign), B.stream(pkg))
    return case


def init_case(pkg, n, problems, cands):
    p = pkg.hip.ptr

    def case(lib, mem):
        x = mem.out("x", (problems * n, cands))
        y = mem.out("y", (problems * n, cands))
        return lib.gmc_dense_sb_init_f32(problems, n, cands, 0x1234567, 0.1, p(x), p(y), B.stream(pkg))
    return case


@pytest.mark.parametrize("n", (2, 63, 65, 130, 257))
def test_dense_sb(pkg, n):
    lib = pkg.hip.load()
    for tile in (0, 1, 2, 3):
        lib.gmc_debug_set_sb_tile(tile)
        B.run_case(pkg, sb_case(pkg, n, 1, 17))
        B.run_case(pkg, sb_case(pkg, n, 3, 5, pad=3, cost=True))
    lib.gmc_debug_set_sb_tile(0)
    B.run_case(pkg, sb_case(pkg, n, 1, 1, pad=1, cost=True, steps=1))
    B.run_case(pkg, sb_case(pkg, n, 3, 65, pad=5))
    B.run_case(pkg, sb_case(pkg, n, 1, 65, cost=True, steps=0))
    B.run_case(pkg, sb_case(pkg, n, 3, 5, pad=2, steps=0))


@pytest.mark.parametrize("n", (2, 63, 65, 130, 257))
def test_dense_sb_init(pkg, n):
    for problems, cands in ((1, 1), (3, 5), (1, 65)):
        B.run_case(pkg, init_case(pkg, n, problems, cands))


def test_the_check_can_fail(pkg):
    B.check_can_fail(pkg, sb_case(pkg, 65, 3, 17, cost=True), "x")
    B.check_can_fail(pkg, sb_case(pkg, 63, 1, 5), "workspace")
