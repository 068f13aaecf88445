"""Guard-band tests of include/gcnmaxcut_sdp.h's two entry points, in the manner of tests/test_gpu_bounds_decode.py: the
batch's arrays, the order arrays at exactly gmc_order_host_t's sizes, keys, node costs, V [R][rank], value [B], assign
[planes][R] and the workspace at exactly gmc_sdp_workspace_bytes come from one arena with 4096-byte bands
(tests/arena.py); each case runs on plain tensors and on arenas filled 0xFF and 0x00, and tests/bounds.run_case asserts
the byte equalities (every status GMC_OK, no band touched, no input changed, the three runs' outputs equal).

Batches `odd` (R = 85: nothing a multiple of a tile), `hub` (a row of 70 entries, real weights) and `trip` (n = 1030:
several workgroups per colour at every rank); ranks 16, 32, 64; terminals 0 and 1; node_cost NULL and real; init = 1 and
the warm start (V an in/out state); 5 planes from plane 3.

Measured on the MI355X: 72 cases (432 calls), no band touched, no pair of runs different; the file's 10 tests take 2.4 s
alone, library load and GPU start-up included (slowest: test_relax_and_round[odd-16], 0.13 s, the first to touch the GPU).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import bounds as B

pytestmark = pytest.mark.gpu

RANKS = (16, 32, 64)
KINDS = ("odd", "hub", "trip")
SWEEPS, FIRST_PLANE, PLANES = 2, 3, 5


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    done = B.report_calls("bounds/sdp")
    yield built
    done()


@functools.lru_cache(maxsize=None)
def orders(kind, terminals):
    """gmc_order_host_t(K = 2)'s arrays at exactly the documented sizes, and max_classes."""
    import gcn_max_cut_amd as pkg
    h = B.host_batch(kind)
    order = np.zeros(h.R, np.int32)
    cgoff = np.zeros(h.B + 1, np.int32)
    cptr = np.zeros(h.R + h.B, np.int32)
    classes = C.c_int32(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg.hip.load().gmc_order_host_t(h.B, ptr(h.goff.astype(np.int32)), ptr(h.rowptr), ptr(h.lcol), 2, int(terminals),
                                         ptr(order), ptr(cgoff), ptr(cptr), cptr.size, C.byref(classes))
    assert rc == 0, rc
    first = 2 if terminals else 0
    return order[:h.R - first * h.B].copy(), cgoff, cptr[:int(cgoff[-1])].copy(), int(classes.value)


@functools.lru_cache(maxsize=None)
def inputs(kind, rank):
    h = B.host_batch(kind)
    rng = np.random.RandomState(100 * rank + len(kind))
    keys = rng.randint(0, 1 << 62, h.B).astype(np.uint64).view(np.int64)
    cost = rng.uniform(-1.5, 1.5, (h.R, 2)).astype(np.float32)
    V = rng.normal(size=(h.R, rank)).astype(np.float32)
    V /= np.linalg.norm(V, axis=1, keepdims=True).astype(np.float32)
    return keys, cost, V


def relax_case(pkg, kind, rank, terminals, cost, warm):
    """gmc_sdp_relax_f32, then gmc_sdp_round_f32 on its V - both on the same memory source."""
    h = B.host_batch(kind)
    order, cgoff, cptr, classes = orders(kind, terminals)
    keys, costs, start = inputs(kind, rank)
    p = pkg.hip.ptr

    def case(lib, mem):
        b = B.device_batch(pkg, mem, h, table=False)
        t_order, t_cgoff, t_cptr = mem.put("order", order), mem.put("cgoff", cgoff), mem.put("cptr", cptr)
        t_keys = mem.put("gkey", keys)
        t_cost = mem.put("node_cost", costs) if cost else None
        V = mem.state("V", start) if warm else mem.out("V", (h.R, rank))
        value = mem.out("value", (h.B,))
        need = int(lib.gmc_sdp_workspace_bytes(C.byref(b), rank))
        assert need == 4 * ((h.R // 256 + h.B + 1 + 3) // 4 * 4)
        ws = mem.scratch("workspace", need)
        rcs = [lib.gmc_sdp_relax_f32(C.byref(b), rank, terminals, p(t_cost), p(t_order), p(t_cgoff), p(t_cptr), classes,
                                     None if warm else p(t_keys), 0 if warm else 1, SWEEPS, p(V), p(value), p(ws), need,
                                     B.stream(pkg))]
        assign = mem.out("assign", (PLANES, h.R), torch.int8)
        rcs.append(lib.gmc_sdp_round_f32(C.byref(b), rank, terminals, p(V), p(t_keys), FIRST_PLANE, PLANES, p(assign),
                                         B.stream(pkg)))
        return rcs
    return case


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("kind", KINDS)
def test_relax_and_round(pkg, kind, rank):
    for terminals in (0, 1):
        for cost in (False, True):
            for warm in (False, True):
                B.run_case(pkg, relax_case(pkg, kind, rank, terminals, cost, warm))


def test_the_check_can_fail(pkg):
    B.check_can_fail(pkg, relax_case(pkg, "odd", 16, 0, True, False), "V")
    B.check_can_fail(pkg, relax_case(pkg, "hub", 64, 1, False, True), "assign")
