"""Guard-band tests of include/gcnmaxcut_temper.h's entry point, in the manner of tests/test_gpu_bounds_decode.py: the
batch's arrays, the order arrays at exactly gmc_order_host_t's sizes, node costs, the ladder [rungs], the level table,
state and best [cands][R], best_score / best_round / rung_out / swaps [B][cands] and the workspace at exactly
gmc_kway_temper_workspace_bytes come from one arena with 4096-byte bands (tests/arena.py); each case runs on plain
tensors and on arenas filled 0xFF and 0x00, and tests/bounds.run_case asserts the byte equalities (every status GMC_OK,
no band touched, no input changed, the three runs' outputs equal - so no word of the workspace is read before the call
wrote it).

Batches `odd` (R = 85 / 89), `hub` (a row of 70 entries, real weights) and `trip` (n = 1030); K = 2, 5, 8; terminals 0
and 1; node_cost NULL and real; rungs 1 and 3 with cands = rungs and 2 rungs (B * cands * 4 no multiple of 16: the
planes' padding is in play); rounds 0, 1 and 4 (both planes read and written); the optional outputs given and NULL; the
global-CSR variant (nnz_max overstated)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bounds as B
from tests.test_gpu_bounds_decode import LEVELS, SEED, inputs, kind_for, put_orders

pytestmark = pytest.mark.gpu
I32, I8 = torch.int32, torch.int8
CLASSES = (2, 5, 8)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    done = B.report_calls("bounds/temper")
    yield built
    done()


def temper_case(pkg, kind, K, terminals, rungs, copies, rounds, cost=False, optional=True, nnz_max=None):
    h = B.host_batch(kind)
    p = pkg.hip.ptr
    cands = rungs * copies
    data = inputs(kind, K, cands)
    ladder = np.linspace(0.5, 3.0, rungs).astype(np.float32)

    def case(lib, mem):
        bc = B.device_batch(pkg, mem, h, False, nnz_max)
        ords, _classes = put_orders(mem, kind, K, terminals)
        t_cost = mem.put("node_cost", data["cost"]) if cost else None
        t_ladder, t_levels = mem.put("ladder", ladder), mem.put("levels", LEVELS)
        state = mem.state("state", data["assign"])
        best = mem.out("best", (cands, h.R), I8)
        best_score = mem.out("best_score", (h.B, cands))
        extra = [mem.out(name, (h.B, cands), I32) if optional else None for name in ("best_round", "rung_out", "swaps")]
        need = int(lib.gmc_kway_temper_workspace_bytes(C.byref(bc), cands))
        assert need == 4 * ((h.B * cands * 4 + 15) // 16 * 16)
        ws = mem.scratch("workspace", need)
        return lib.gmc_kway_temper_f32(C.byref(bc), K, terminals, p(t_cost), *(p(o) for o in ords), cands, rungs,
                                       p(t_ladder), rounds, 2, p(t_levels), SEED, p(state), p(best), p(best_score),
                                       *(p(e) for e in extra), p(ws), need, B.stream(pkg))
    return case


@pytest.mark.parametrize("K", CLASSES)
def test_temper(pkg, K):
    for terminals in (1, 0):
        odd = kind_for("odd", K, terminals)
        for rungs, copies in ((1, 1), (3, 1), (3, 2)):
            for rounds in (0, 1, 4):
                B.run_case(pkg, temper_case(pkg, odd, K, terminals, rungs, copies, rounds, cost=bool(rounds & 1)))
        B.run_case(pkg, temper_case(pkg, odd, K, terminals, 3, 1, 4, cost=True, optional=False))
        B.run_case(pkg, temper_case(pkg, odd, K, terminals, 3, 2, 4, nnz_max=1 << 24))
        for kind in ("hub", "trip"):
            B.run_case(pkg, temper_case(pkg, kind, K, terminals, 3, 1, 3, cost=kind == "hub"))
    B.run_case(pkg, temper_case(pkg, "hub", K, 1, 3, 2, 2, cost=True, nnz_max=1 << 24))


def test_the_check_can_fail(pkg):
    B.check_can_fail(pkg, temper_case(pkg, "odd", 5, 1, 3, 2, 2, cost=True), "best")
    B.check_can_fail(pkg, temper_case(pkg, "hub", 2, 0, 3, 1, 3), "workspace")
