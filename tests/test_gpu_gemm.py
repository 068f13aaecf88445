"""gmc_gemm_f32 alone against a float64 numpy product: the three forms (NN, TN, NT) of the one fp32 MFMA tile loop at
every edge of its 64 x 64 x 16 block tile, packed and padded leading dimensions, with and without the row scale.

Bound per element: |got - ref| <= (K + 4) * 2^-24 * sum_k |a_k b_k| * |scale| - the forward-error bound of an fp32 fma
sum of K products in any order plus the epilogue's rounding; derived, not measured.  A misplaced or missing element is
off by whole products, so the bound catches indexing faults too.  Operand padding and the band around C hold NaN: a
read of padding poisons the result, a write beyond the edge shows in the band."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TM, TN, TK = 64, 64, 16      # the kernel's block tile (csrc/gemm_mfma.hip)
FORMS = {"NN": (0, 0), "TN": (1, 0), "NT": (0, 1)}
EDGE = lambda T: (1, T - 1, T, T + 1, 2 * T + 3)
K_EDGE = (1, 2, 3, TK - 1, TK + 1, 2 * TK + 5)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def up4(n):
    return (n + 3) // 4 * 4


def stored(m, pad):
    """A host matrix on the device, rows of up4(cols) + pad floats, the padding NaN; (buffer, view of the data, ld)."""
    rows, cols = m.shape
    ld = up4(cols) + pad
    buf = torch.full((rows, ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :cols] = torch.from_numpy(np.ascontiguousarray(m))
    return buf, ld


def run(pkg, form, M, Nc, K, pad, use_scale, seed):
    """One GEMM call; returns (got [M, Nc] float32, ref float64, bound float64, whole C buffer, its data mask)."""
    hip = pkg.hip
    ta, tb = FORMS[form]
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = rng.standard_normal((K, Nc)).astype(np.float32)
    s = rng.uniform(0.1, 2.0, M).astype(np.float32) * rng.choice([-1.0, 1.0], M).astype(np.float32)
    A, lda = stored(a.T if ta else a, pad)
    B, ldb = stored(b.T if tb else b, pad)
    ldc = up4(Nc) + pad
    Cbuf = torch.full((M + 2, ldc), float("nan"), dtype=torch.float32, device="cuda")   # a NaN band on every side
    scale = torch.from_numpy(s).cuda() if use_scale else None
    rc = hip.load().gmc_gemm_f32(ta, tb, M, Nc, K, hip.ptr(A), lda, hip.ptr(B), ldb, hip.ptr(scale),
                                 Cbuf.data_ptr() + 4 * ldc, ldc, hip.stream())
    hip.check(rc, "gmc_gemm_f32")
    whole = Cbuf.cpu().numpy()
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    sc = s.astype(np.float64)[:, None] if use_scale else 1.0
    ref = sc * (a64 @ b64)
    bound = (K + 4) * 2.0 ** -24 * (np.abs(a64) @ np.abs(b64)) * np.abs(sc)
    inside = np.zeros(whole.shape, bool)
    inside[1:M + 1, :Nc] = True
    return whole[1:M + 1, :Nc], ref, bound, whole, inside


def check(pkg, form, M, Nc, K, pad, use_scale, seed=0):
    got, ref, bound, whole, inside = run(pkg, form, M, Nc, K, pad, use_scale, seed)
    what = (form, M, Nc, K, pad, use_scale)
    assert np.isnan(whole[~inside]).all(), ("write beyond the edge of C", what)
    assert np.isfinite(got).all(), ("padding read or element not written", what)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f"gemm {what}: max err / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("use_scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("pad", [0, 4], ids=["packed", "padded"])
@pytest.mark.parametrize("form", list(FORMS))
def test_tile_edges(pkg, form, pad, use_scale):
    """M, Nc and K each at 1, T-1, T, T+1, 2T+3 (K: 1, 2, 3, TK-1, TK+1, 2TK+5) in turn, the other two at sizes that
    are no multiple of the tile."""
    for M in EDGE(TM):
        check(pkg, form, M, 70, 21, pad, use_scale, seed=M)
    for Nc in EDGE(TN):
        check(pkg, form, 70, Nc, 21, pad, use_scale, seed=100 + Nc)
    for K in K_EDGE:
        check(pkg, form, 65, 66, K, pad, use_scale, seed=200 + K)


@pytest.mark.parametrize("form,M,Nc,K", [("NN", 4096, 4, 8), ("NN", 3, 4096, 1000), ("TN", 70, 40, 4096),
                                         ("NT", 70, 40, 4096), ("NN", 1000, 500, 1000)])
def test_extreme_aspect_shapes(pkg, form, M, Nc, K):
    check(pkg, form, M, Nc, K, 0, True, seed=7)


@pytest.mark.parametrize("form", list(FORMS))
def test_two_runs_give_equal_bytes(pkg, form):
    a = run(pkg, form, 131, 67, 1000, 4, True, seed=3)[0]
    b = run(pkg, form, 131, 67, 1000, 4, True, seed=3)[0]
    assert a.tobytes() == b.tobytes()


def test_probe_names_the_launch(pkg):
    with pkg.hip.Probe(4) as p:
        run(pkg, "NN", 8, 8, 8, 0, False, seed=1)
    assert [t for t, _ms in p.records] == ["gemm"]
