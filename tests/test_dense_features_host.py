"""CPU-side checks of the dense-feature entry points (features that are not the padded adjacency): the library exports
them, they refuse bad arguments before any HIP call, and the GEMM kernels are in the gfx950 code object without
scratch.  The arithmetic is tested on the GPU (tests/test_gpu_gemm.py, tests/test_gpu_dense_features.py)."""
import ctypes as C
import subprocess

from tests import util

NEW = ("gmc_gemm_f32", "gmc_workspace_bytes_features", "gmc_forward_features", "gmc_backward_features_from_gp")
NULL_, SHAPE, ALIGN, WORKSPACE, UNSUPPORTED, ABI = -1, -2, -4, -5, -7, -8


def test_library_exports_the_dense_feature_symbols(built):
    hip = built.hip
    lib = hip.load()
    for name in NEW:
        assert name in hip.SYMBOLS
        getattr(lib, name)                       # AttributeError without the feature
    assert hip.PROBE_TAGS.index("gemm") == 17     # GMC_K_GEMM
    assert hip.PROBE_TAGS[:17] == hip.KERNEL_TAGS


def test_gemm_rejects_bad_arguments_without_a_gpu(built):
    lib = built.hip.load()
    null, some, odd = C.c_void_p(None), C.c_void_p(4096), C.c_void_p(4100)   # (never dereferenced: the calls fail first)

    def f(ta=0, tb=0, M=8, Nc=8, K=8, A=some, lda=8, B=some, ldb=8, scale=null, Cp=some, ldc=8):
        return lib.gmc_gemm_f32(ta, tb, M, Nc, K, A, lda, B, ldb, scale, Cp, ldc, None)

    assert f(A=null) == NULL_ and f(B=null) == NULL_ and f(Cp=null) == NULL_
    assert f(M=-1) == SHAPE and f(Nc=-1) == SHAPE and f(K=-1) == SHAPE
    assert f(lda=4) == SHAPE and f(ldb=4) == SHAPE and f(ldc=4) == SHAPE
    assert f(ta=1, M=16, lda=8) == SHAPE          # A stored [K, M]: lda >= M
    assert f(tb=1, K=16, lda=16, ldb=8) == SHAPE  # B stored [Nc, K]: ldb >= K
    assert f(ta=1, tb=1) == UNSUPPORTED
    assert f(A=odd) == ALIGN and f(B=odd) == ALIGN and f(Cp=odd) == ALIGN
    assert f(K=7, lda=7) == ALIGN and f(Nc=7, ldb=7, ldc=8) == ALIGN and f(Nc=7, ldb=8, ldc=7) == ALIGN
    assert f(M=0) == 0 and f(Nc=0) == 0           # nothing to do, nothing launched


def _structs(hip, **model_kw):
    some = 4096
    b = hip.GmcBatch(B=1, R=60, nnz=300, n_max=60, uniform_n=60, nnz_max=300, goff=some, rowptr=some, gcol=some,
                     lcol=some, dinv=some)
    kw = dict(N=1000, F=32, K=3, W1=some, b1=some, W2=some, b2=some)
    kw.update(model_kw)
    return b, hip.GmcModel(**kw)


def test_feature_entry_points_reject_bad_arguments_without_a_gpu(built):
    hip = built.hip
    lib = hip.load()
    null, some, odd = C.c_void_p(None), C.c_void_p(4096), C.c_void_p(4100)
    b, m = _structs(hip)
    need_f = lib.gmc_workspace_bytes_features(C.byref(b), C.byref(m), 0)
    need_t = lib.gmc_workspace_bytes_features(C.byref(b), C.byref(m), 1)
    assert 0 < need_f < need_t
    assert need_f >= 2 * 60 * 32 * 4              # T0 and H, row-major
    assert lib.gmc_workspace_bytes_features(None, C.byref(m), 1) == 0

    def fwd(bb=b, mm=m, X=some, ldx=1000, ws=some, nbytes=1 << 30, P=some):
        return lib.gmc_forward_features(C.byref(bb), C.byref(mm), X, ldx, 1.0, ws, nbytes, P, None, None, None)

    def bwd(bb=b, mm=m, X=some, ldx=1000, ws=some, nbytes=1 << 30, P=some, GP=some, grad=some, dX=null, lddx=0):
        return lib.gmc_backward_features_from_gp(C.byref(bb), C.byref(mm), X, ldx, ws, nbytes, P, GP, grad, dX, lddx,
                                                 None)

    for call in (fwd, bwd):
        assert call(X=null) == NULL_ and call(ws=null) == NULL_ and call(P=null) == NULL_
        assert call(bb=hip.GmcBatch(abi=100)) == ABI and call(mm=hip.GmcModel(abi=100)) == ABI
        assert call(ldx=996) == SHAPE                        # ldx < N
        assert call(mm=_structs(hip, N=0)[1]) == SHAPE
        assert call(X=odd) == ALIGN and call(ldx=1002) == ALIGN
        assert call(mm=_structs(hip, F=30)[1]) == UNSUPPORTED   # the hidden width is padded by the caller
    assert lib.gmc_forward_features(None, C.byref(m), some, 1000, 1.0, some, 1 << 30, some, None, None, None) == NULL_
    assert fwd(nbytes=need_f - 1) == WORKSPACE and bwd(nbytes=need_t - 1) == WORKSPACE
    assert bwd(GP=null) == NULL_ and bwd(grad=null) == NULL_
    assert bwd(grad=odd) == ALIGN
    assert bwd(dX=some, lddx=996) == SHAPE
    assert bwd(dX=odd, lddx=1000) == ALIGN and bwd(dX=some, lddx=1002) == ALIGN
    # errors come in the order NULL, ABI, SHAPE, ALIGN, WORKSPACE
    assert fwd(bb=hip.GmcBatch(abi=100), X=null) == NULL_
    assert fwd(bb=hip.GmcBatch(abi=100), ldx=996) == ABI
    assert fwd(ldx=996, X=odd) == SHAPE
    assert fwd(X=odd, nbytes=0) == ALIGN
    # a graph may have more nodes than the features have columns here (gmc_forward: GMC_ERR_SHAPE)
    small = _structs(hip, N=48)[1]
    assert fwd(mm=small, ldx=48, nbytes=0) == WORKSPACE
    assert lib.gmc_forward(C.byref(b), C.byref(small), 1.0, some, 1 << 30, some, None, None, None) == SHAPE
    # an empty batch launches nothing
    empty = hip.GmcBatch(B=0, R=0, goff=4096, rowptr=4096, gcol=4096, lcol=4096, dinv=4096)
    assert fwd(bb=empty) == 0


def test_dense_workspace_is_the_row_major_plan(built):
    """The dense plan has its own size query: row-major [R, ld] buffers T0 and H (ld = F rounded up to 32 floats)
    and Z0 [R, 3], each rounded up to 256 bytes; dropout adds the scaled copy of W2 to the training size."""
    hip = built.hip
    lib = hip.load()
    b, m = _structs(hip, F=36)
    up = lambda n: (n + 255) // 256 * 256
    assert lib.gmc_workspace_bytes_features(C.byref(b), C.byref(m), 0) == 2 * up(60 * 64 * 4) + up(60 * 3 * 4)
    plain = lib.gmc_workspace_bytes_features(C.byref(b), C.byref(m), 1)
    m.dropout_p = 0.3
    assert lib.gmc_workspace_bytes_features(C.byref(b), C.byref(m), 1) == plain + up(36 * 3 * 4)


def test_gemm_kernels_are_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    forms = [s for s in names if "gemm_mfma_kernel" in s]
    assert len(forms) == 3, sorted(forms)            # NN, TN, NT: one template, three instantiations
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if "gemm_mfma_kernel" in entry and ".name:" in entry:
                fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
                if "gemm_mfma_kernel" not in fields.get(".name", ""):
                    continue
                seen += 1
                assert int(fields[".private_segment_fixed_size"]) == 0
                assert int(fields[".vgpr_spill_count"]) == 0
    assert seen == 3
