"""An empty batch (B = R = 0) through the C ABI itself: the engine answers B == 0 in Python, so these are the only calls
that reach the entry points' own empty-batch case - which zeroes the gradient, with the slot behind it exactly when
gmc_train_fwd_bwd is told of one (GMC_MODEL_GRAD_TAIL), and launches nothing else.  N = 8, F = 4."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
N, F = 8, 4
COUNT = N * F + F + F * 3 + 3
SENTINEL = 7.25


@pytest.fixture(scope="module")
def ctx(built):
    hip = built.hip
    dev = hip.require_gpu()
    one_i, one_f = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float32, device=dev)
    torch.manual_seed(3)
    param = torch.randn(COUNT + 4, device=dev)   # (the engine's buffers carry four floats of tail as well)
    keep = [one_i, one_f, param]

    def model(flags):
        o = [0, N * F, N * F + F, N * F + F + F * 3]
        return hip.GmcModel(N=N, F=F, K=3, flags=flags, W1=param.data_ptr(), b1=param.data_ptr() + 4 * o[1],
                            W2=param.data_ptr() + 4 * o[2], b2=param.data_ptr() + 4 * o[3])

    batch = hip.GmcBatch(B=0, R=0, goff=hip.ptr(one_i), rowptr=hip.ptr(one_i), gcol=hip.ptr(one_i), lcol=hip.ptr(one_i),
                         dinv=hip.ptr(one_f))
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    return dict(hip=hip, lib=hip.load(), dev=dev, batch=batch, model=model, ws=ws, one=one_f, param=param, keep=keep)


def hip_ptr(ctx, name):
    return ctx["hip"].ptr(ctx[name])


def grad_after(ctx, call):
    """The count + 4 floats of a sentinel-filled gradient buffer after ``call(grad pointer)`` returned GMC_OK."""
    grad = torch.full((COUNT + 4,), SENTINEL, dtype=torch.float32, device=ctx["dev"])
    assert call(ctx["hip"].ptr(grad)) == 0
    torch.cuda.synchronize()
    return grad.cpu()


def assert_zeroed(grad, n):
    assert (grad[:n] == 0).all(), f"first {n} floats are not all zero"
    assert (grad[n:] == SENTINEL).all(), f"floats beyond the first {n} changed: {grad[n:].tolist()}"


@pytest.mark.parametrize("flags,zeroed", ((1, COUNT + 1), (0, COUNT), (3, COUNT + 1), (2, COUNT)))
def test_train_fwd_bwd_zeroes_the_tail_slot_only_when_told_of_one(ctx, flags, zeroed):
    hip, lib, P = ctx["hip"], ctx["lib"], hip_ptr(ctx, "one")
    m = ctx["model"](flags)
    grad = grad_after(ctx, lambda g: lib.gmc_train_fwd_bwd(C.byref(ctx["batch"]), C.byref(m), 1.0, hip.ptr(ctx["ws"]),
                                                           ctx["ws"].numel(), P, None, P, g, hip.stream()))
    assert_zeroed(grad, zeroed)


@pytest.mark.parametrize("dense", (False, True), ids=("plain", "features"))
def test_backward_from_gp_never_zeroes_the_tail_slot(ctx, dense):
    hip, lib, one = ctx["hip"], ctx["lib"], hip_ptr(ctx, "one")
    m = ctx["model"](hip.MODEL_GRAD_TAIL)   # (the flag is gmc_train_fwd_bwd's: these two calls have no loss to put there)
    head = (C.byref(ctx["batch"]), C.byref(m))
    ws = (hip.ptr(ctx["ws"]), ctx["ws"].numel())
    if dense:
        call = lambda g: lib.gmc_backward_features_from_gp(*head, one, N, *ws, one, one, g, None, 0, hip.stream())
    else:
        call = lambda g: lib.gmc_backward_from_gp(*head, *ws, one, one, g, hip.stream())
    assert_zeroed(grad_after(ctx, call), COUNT)


@pytest.mark.parametrize("kind", (0, 1), ids=("cut", "expected_cut"))
def test_train_step_of_an_empty_batch_is_an_adam_step_on_a_zero_gradient(ctx, kind):
    """Zero moments and a zero gradient: Adam leaves parameters and moments as they are, bit for bit, and the device
    step counter advances by exactly one."""
    hip, lib, dev, one = ctx["hip"], ctx["lib"], ctx["dev"], hip_ptr(ctx, "one")
    param = ctx["param"].clone()
    mom, var = torch.zeros_like(param), torch.zeros_like(param)
    counter = torch.full((1,), 5, dtype=torch.int32, device=dev)
    grad = grad_after(ctx, lambda g: lib.gmc_train_step_loss_f32(
        C.byref(ctx["batch"]), N, F, hip.ptr(param), 1.0, kind, hip.ptr(ctx["ws"]), ctx["ws"].numel(), one, None, one, g,
        hip.ptr(mom), hip.ptr(var), 1e-3, 0.9, 0.999, 1e-8, hip.ptr(counter), None, hip.stream()))
    assert_zeroed(grad, COUNT)                     # (the step's model has no tail slot)
    assert torch.equal(param.view(torch.int32), ctx["param"].view(torch.int32))
    assert not mom.view(torch.int32).any() and not var.view(torch.int32).any()
    assert int(counter.item()) == 6
