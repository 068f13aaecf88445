"""Hidden widths 1028..4096 (GMC_MAX_HIDDEN) on the host side (CPU only): the flavour query, the ABI's bound and the
workspace size.

Wide F is a runtime slice count of the LDS-tiled kernels that F <= 1024 already uses - no new instantiation: every word
of a wide-F launch, GMC_FLV_PER cleared, is one that F = 1024 gives for the same batch, and one the code object has.
"""
import ctypes as C

import pytest

from tests.test_lds_flavours import PER_MASK, batch_struct, instantiated_flavours, name

WIDE = (1028, 2048, 2052, 4096)


@pytest.fixture(scope="module")
def hip(built):
    built.hip.load()
    return built.hip


def sweep():
    """The batches of test_lds_flavours.reachable_flavours: both table widths, every ell_slots value, weights, overflow
    lists, one-graph steps, every n_max in 1..2100."""
    for W in (8, 16):
        combos = [(s, False, 0) for s in range(0, W + 1)]
        combos += [(s, True, 0) for s in (0, W - 1, W)]
        combos += [(W, val, b) for val in (False, True) for b in (1, 64, 4095, 4096)]
        for slots, val, blocks in combos:
            for one, B in ((False, 2), (True, 1), (True, 2)):
                for n in range(1, 2101):
                    yield (W, slots, val, blocks, n, B), one


def test_wide_flavours_are_the_words_of_f1024_and_instantiated(hip):
    inst = instantiated_flavours(hip.LIB_PATH)
    served = 0
    for args, one in sweep():
        b = batch_struct(hip, *args)
        base = {w & ~PER_MASK for w in hip.lds_flavours(b, 1024, one)}
        for F in WIDE:
            got = hip.lds_flavours(b, F, one)
            assert all(w > 0 for w in got), (args, one, F, got)
            # the same launches as F = 1024: the LDS path where (and only where) F = 1024 takes it
            assert {w & ~PER_MASK for w in got} == base, (args, one, F, [name(w) for w in got])
            assert {w & ~PER_MASK for w in got} <= inst, (args, one, F, [name(w) for w in got])
            served += bool(got)
    assert served > 0


def test_wide_flavours_keep_the_one_graph_head(hip):
    """The reference schedule at hidden 2048: the one-graph backward still computes the head (GMC_FLV_HEAD)."""
    b = batch_struct(hip, 8, 7, False, 0, 1000, 1)
    words = hip.lds_flavours(b, 2048, True)
    assert words[1] >> 26 & 1, [name(w) for w in words]


def _model(hip, F, N=1000):
    some = C.c_void_p(4096)
    return hip.GmcModel(N=N, F=F, K=3, W1=some, b1=some, W2=some, b2=some)


def test_abi_bound_is_4096(hip):
    """check() refuses F = 4100 with GMC_ERR_UNSUPPORTED and passes F = 4096 (the call then fails on its NULL P,
    before any device memory is touched); the query refuses 4100 as a bad shape; the message names the bound."""
    lib = hip.load()
    b = batch_struct(hip, 8, 7, False, 0, 1000, 2)
    some = C.c_void_p(4096)
    assert lib.gmc_forward(C.byref(b), C.byref(_model(hip, 4100)), 1.0, some, 1 << 20, None, None, None, None) == -7
    assert lib.gmc_forward(C.byref(b), C.byref(_model(hip, 4096)), 1.0, some, 1 << 20, None, None, None, None) == -1
    assert lib.gmc_forward(C.byref(b), C.byref(_model(hip, 2052)), 1.0, some, 1 << 20, None, None, None, None) == -1
    assert lib.gmc_train_fwd_bwd(C.byref(b), C.byref(_model(hip, 4100)), 1.0, some, 1 << 20, some, None, None, some,
                                 None) == -7
    assert lib.gmc_backward_from_gp(C.byref(b), C.byref(_model(hip, 4100)), some, 1 << 20, some, some, some, None) == -7
    words = (C.c_int32 * 8)()
    assert lib.gmc_lds_flavours(C.byref(b), 4100, 0, words, 8) == -2
    assert lib.gmc_lds_flavours(C.byref(b), 4096, 0, words, 8) == 6
    assert b"4096" in lib.gmc_error_string(-7)


def _align(x):
    return (x + 255) // 256 * 256


def test_workspace_bytes_past_2_31_elements(hip):
    """1100 graphs of n = 1000 at F = 4096: R * F = 4.5e9 elements.  gmc_workspace_bytes equals the sum of its regions
    (api.hip: carve) in Python integers: T0, H [R, 4096] each (the 16-column slab: n = 1000 gives FS = 16), Z0
    [groups][R][3] (4 slices per group: 64 groups), GY2 [R, 4], column partials [max(tiles, chunks), F, 4] (256-row
    tiles; one dW1 chunk at 256 slices), db2 partials [B, 3], dW1 partials [chunks, n_max, F]."""
    lib = hip.load()
    B, n, F, N = 1100, 1000, 4096, 1000
    b = batch_struct(hip, 8, 7, False, 0, n, B)
    R = n * B
    assert R * F > 2 ** 31
    fs, slices = 16, 4096 // 16
    groups = slices // 4
    tiles = (R + 255) // 256
    chunks = 1
    fwd = [R * F, R * F, groups * R * 3]
    train = fwd + [R * 4, max(tiles, chunks) * F * 4, B * 3, chunks * n * F]
    assert lib.gmc_workspace_bytes(C.byref(b), C.byref(_model(hip, F, N)), 0) == sum(_align(4 * x) for x in fwd)
    assert lib.gmc_workspace_bytes(C.byref(b), C.byref(_model(hip, F, N)), 1) == sum(_align(4 * x) for x in train)
    # the row kernels' layout (no ELL table): leading dimension F rounded up to 32, one Z0 partial, tiles of 64 rows,
    # dW1 partials of the row kernel: min(32, ceil(B / 8)) chunks of [N, F]
    b.ell = None
    ld = F
    rchunks = min(32, (B + 7) // 8)
    train = [R * ld, R * ld, R * 3, R * 4, ((R + 63) // 64) * F * 4, B * 3, rchunks * N * F]
    assert lib.gmc_workspace_bytes(C.byref(b), C.byref(_model(hip, F, N)), 1) == sum(_align(4 * x) for x in train)
