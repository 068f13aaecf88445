"""Guard-band tests of include/gcnmaxcut_dense.h's entry point, in the manner of tests/test_gpu_bounds_temper.py: the
matrices W [B][n][ld] at exactly that size, node costs [B * n][2], the order [B * n], the schedule [anneal_sweeps], the
level table, assign [cands][B * n], score_all / snap_sweep / sweeps [B][cands], moves [B][cands] int64, best_assign
[B * n], best_score / best_idx [B] and the workspace at exactly gmc_dense_anneal_workspace_bytes come from one arena with
4096-byte bands (tests/arena.py); each case runs on plain tensors and on arenas filled 0xFF and 0x00, and
tests/bounds.run_case asserts the byte equalities (every status GMC_OK, no band touched, no input changed, the three runs'
outputs equal).

n = 2, 63, 65, 130 and 257 (nothing a multiple of the lane stride but 64 itself, which tests/test_gpu_dense.py has); ld = n
(the last row ends the buffer) and ld > n; B = 1 and 3; cands = 1, 3, 5 (the last workgroup of a problem has idle waves);
node_cost and order NULL and given; the optional outputs given and NULL; anneal_sweeps 0 (schedule and table NULL) and
3; max_descent_sweeps 0 and 3."""
import numpy as np
import pytest
import torch

from tests import anneal_ref as AR
from tests import bounds as B
from tests import dense_ref as DR

pytestmark = pytest.mark.gpu
I32, I8, I64 = torch.int32, torch.int8, torch.int64
SEED = 0x1234567


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    done = B.report_calls("bounds/dense")
    yield built
    done()


def dense_case(pkg, n, problems, cands, pad=0, cost=False, order=False, optional=True, sweeps=3, descent=3):
    p = pkg.hip.ptr
    square = np.stack([DR.weights_of("real", n, 9 * n + b) for b in range(problems)])
    W = np.zeros((problems, n, n + pad), np.float32)
    W[:, :, :n] = square
    R = problems * n
    assign = np.random.RandomState(n + cands).randint(0, 2, (cands, R)).astype(np.int8)
    perm = np.concatenate([np.random.RandomState(3 + b).permutation(n) for b in range(problems)]).astype(np.int32)
    inv_temp = AR.schedule(sweeps, scale=DR.rms_field(square))

    def case(lib, mem):
        t_w = mem.put("W", W)
        t_cost = mem.put("node_cost", DR.cost_of("real", R, n)) if cost else None
        t_order = mem.put("order", perm) if order else None
        t_inv = mem.put("inv_temp", inv_temp) if sweeps else None
        t_levels = mem.put("levels", AR.levels()) if sweeps else None
        state = mem.state("assign", assign)
        score_all = mem.out("score_all", (problems, cands))
        best_assign = mem.out("best_assign", (R,), I32)
        best_score = mem.out("best_score", (problems,))
        best_idx = mem.out("best_idx", (problems,), I32)
        extra = [mem.out(name, (problems, cands), dt) if optional else None
                 for name, dt in (("snap_sweep", I32), ("sweeps", I32), ("moves", I64))]
        need = int(lib.gmc_dense_anneal_workspace_bytes(problems, n, cands))
        assert need == 16
        ws = mem.scratch("workspace", need)
        return lib.gmc_dense_anneal_f32(problems, n, p(t_w), n + pad, p(t_cost), p(t_order), cands, p(state), p(t_inv),
                                        sweeps, p(t_levels), SEED, descent, p(ws), need, p(score_all), p(best_assign),
                                        p(best_score), p(best_idx), *(p(e) for e in extra), B.stream(pkg))
    return case


@pytest.mark.parametrize("n", (2, 63, 65, 130, 257))
def test_dense_anneal(pkg, n):
    for problems, cands in ((1, 1), (3, 3), (1, 5)):
        B.run_case(pkg, dense_case(pkg, n, problems, cands))
        B.run_case(pkg, dense_case(pkg, n, problems, cands, pad=3, cost=True, order=True))
    B.run_case(pkg, dense_case(pkg, n, 3, 5, cost=True, optional=False))
    B.run_case(pkg, dense_case(pkg, n, 1, 3, order=True, sweeps=0))
    B.run_case(pkg, dense_case(pkg, n, 3, 1, pad=1, cost=True, descent=0, optional=False))


def test_the_check_can_fail(pkg):
    B.check_can_fail(pkg, dense_case(pkg, 65, 3, 5, cost=True, order=True), "assign")
    B.check_can_fail(pkg, dense_case(pkg, 63, 1, 3), "W")
