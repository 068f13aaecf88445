"""The Adam family, gmc_w1_slab_f32 and gmc_publish_f32 alone (csrc/adam.hip, csrc/w1_slab.hip) against a float64 step
from the same float32 state (tests/blocks_ref.py: adam_ref and the bounds bm, bv, bp derived there).

  counts   1 .. 7 (tail only / one float4 + tail), 1023 .. 1025, and 2048 blocks x 256 threads x 4 floats = 2,097,152
           (every thread one trip), + 1 (tail), + 4 (the first float4 of a second trip), + 1027, 3 x that + 5
  steps    1, 2, 3, 1000 (gmc_adam_f32); a device counter starting at 0, 1, 999 (the devstep forms); three calls in a
           row, each judged from the device's state before it
  state    a third of the parameters exactly 0, a third ~1e-4, a third ~1 (p's own rounding must not hide an error of
           the update); gradients of scales 1e-6 .. 1e3 with blocks of exact zeros; blocks of m = v = 0
  buffers  p, g, m, v, the slab and the counter lie between NaN bands (sentinels for the counter); g must not change

gmc_adam_devstep_model_f32 and gmc_publish_adam_devstep_model_f32 must give the bytes of gmc_adam_devstep_f32 on the
same buffers, keep the slab copy equal to the slab of the updated W1 (pad columns as gmc_w1_slab_f32 left them), and
advance the counter by exactly one - the publishing form BEFORE its sweep, which then uses the counter as it stands.

Measured on the MI355X, worst err / bound (-s prints every call; the module takes 4.4 s, its largest case 0.9 s):
                                   m      v      p      (bm = 3u(|m| + |g|), bv = 5u v, bp: tests/blocks_ref.py)
  gmc_adam_f32, counts and steps   0.324  0.552  0.997
  gmc_adam_devstep_f32, counts     0.324  0.552  0.997
  devstep from 0 / 1 / 999         0.299  0.524  0.948
  three devsteps in a row          0.306  0.535  0.981
  model and publishing forms       0.308  0.539  0.986
p's ratio is its own final rounding (u |p| of parameters of size 1); the float32 restatement on the CPU gives 0.319,
0.552 and 0.997, and 0.25 over the parameters that start at exactly 0, where only the update's error shows.
"""
import numpy as np
import pytest
import torch

from tests import blocks_ref as BR
from tests.blocks_ref import BAND
from tests.util import _slab_of

pytestmark = pytest.mark.gpu

FULL = 2048 * 256 * 4                     # elements of one trip of the largest grid
COUNTS = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, FULL, FULL + 1, FULL + 4, FULL + 1027, 3 * FULL + 5)
MODELS = ((1, 4), (3, 20), (5, 16), (1000, 72), (64, 500))
SLABS = ((1, 4), (3, 12), (3, 20), (1000, 16), (1000, 72), (64, 500), (4096, 4), (3, 4096), (4096, 500))
SENTINEL = -7777
H = BR.HYPER
HYPER = (H["lr"], H["beta1"], H["beta2"], H["eps"])


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


class State:
    """p, g, m, v on the device between NaN bands, a step counter between sentinels, optionally a slab buffer."""

    def __init__(self, st, start=0, slab_floats=0):
        self.n = st["p"].size
        self.t = {k: torch.from_numpy(BR.banded(st[k])[0]).cuda() for k in "pgmv"}
        self.counter = torch.tensor([SENTINEL, start, SENTINEL], dtype=torch.int32, device="cuda")
        self.slab = torch.full((slab_floats + 2 * BAND,), float("nan"), device="cuda") if slab_floats else None

    def ptr(self, k):
        return self.t[k].data_ptr() + 4 * BAND

    def ptrs(self):
        return tuple(self.ptr(k) for k in "pgmv")

    def counter_ptr(self):
        return self.counter.data_ptr() + 4

    def slab_ptr(self):
        return None if self.slab is None else self.slab.data_ptr() + 4 * BAND

    def wholes(self):
        torch.cuda.synchronize()
        return tuple(self.t[k].cpu().numpy() for k in "pmvg")

    def host_state(self):
        """The float32 state as it stands on the device (for the next step's reference)."""
        torch.cuda.synchronize()
        return {k: self.t[k].cpu().numpy()[BAND:BAND + self.n].copy() for k in "pgmv"}

    def steps(self):
        c = self.counter.cpu().numpy()
        assert c[0] == SENTINEL and c[2] == SENTINEL, c
        return int(c[1])


def adam(pkg, s, step):
    pkg.hip.check(pkg.hip.load().gmc_adam_f32(*s.ptrs(), s.n, *HYPER, step, pkg.hip.stream()), "gmc_adam_f32")


def devstep(pkg, s):
    rc = pkg.hip.load().gmc_adam_devstep_f32(*s.ptrs(), s.n, *HYPER, s.counter_ptr(), pkg.hip.stream())
    pkg.hip.check(rc, "gmc_adam_devstep_f32")


def devstep_model(pkg, s, N, F):
    rc = pkg.hip.load().gmc_adam_devstep_model_f32(*s.ptrs(), N, F, s.slab_ptr(), *HYPER, s.counter_ptr(),
                                                   pkg.hip.stream())
    pkg.hip.check(rc, "gmc_adam_devstep_model_f32")


def build_slab(pkg, s, N, F):
    rc = pkg.hip.load().gmc_w1_slab_f32(s.ptr("p"), N, F, s.slab_ptr(), pkg.hip.stream())
    pkg.hip.check(rc, "gmc_w1_slab_f32")


def report(what, worst):
    print(f"adam {what}: max err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def model_count(N, F):
    return N * F + F + 3 * F + 3


@pytest.mark.parametrize("count", COUNTS)
def test_counts_both_entry_points(pkg, count):
    st = BR.adam_problem(count)
    ref = BR.adam_ref(st, 2, **H)
    s = State(st)
    adam(pkg, s, 2)
    report(f"gmc_adam_f32 count {count}", BR.judge_adam(ref, *s.wholes(), ("adam_f32", count)))
    s = State(st, start=1)
    devstep(pkg, s)
    report(f"gmc_adam_devstep_f32 count {count}", BR.judge_adam(ref, *s.wholes(), ("devstep", count)))
    assert s.steps() == 2


@pytest.mark.parametrize("step", (1, 2, 3, 1000))
def test_steps_of_adam_f32(pkg, step):
    st = BR.adam_problem(1027, f"steps {step}")
    s = State(st)
    adam(pkg, s, step)
    report(f"gmc_adam_f32 step {step}", BR.judge_adam(BR.adam_ref(st, step, **H), *s.wholes(), ("adam_f32 step", step)))


@pytest.mark.parametrize("start", (0, 1, 999))
def test_devstep_reads_the_counter_and_advances_it_by_one(pkg, start):
    st = BR.adam_problem(1027, f"devstep {start}")
    s = State(st, start=start)
    devstep(pkg, s)
    report(f"devstep from {start}", BR.judge_adam(BR.adam_ref(st, start + 1, **H), *s.wholes(), ("devstep from", start)))
    assert s.steps() == start + 1


@pytest.mark.parametrize("start", (0, 999))
def test_three_devsteps_in_a_row(pkg, start):
    """The counter is never touched by the host: each call is judged as step start + k from the device's state before it."""
    st = BR.adam_problem(FULL // 64 + 3, f"three {start}")
    s = State(st, start=start)
    for k in (1, 2, 3):
        before = s.host_state()
        devstep(pkg, s)
        report(f"devstep {start} + {k}", BR.judge_adam(BR.adam_ref(before, start + k, **H), *s.wholes(), ("three", start, k)))
        assert s.steps() == start + k


def check_slab(s, N, F, what):
    """The slab buffer against the slab of W1 as it now stands in p; the NaN band behind gmc_w1_slab_floats untouched."""
    torch.cuda.synchronize()
    W1 = s.t["p"].cpu().numpy()[BAND:BAND + N * F].reshape(N, F)
    whole = s.slab.cpu().numpy()
    BR.judge_slab(W1, whole, what=what)
    assert np.array_equal(whole[BAND:-BAND].reshape(-1, N, 16), _slab_of(W1)), what


@pytest.mark.parametrize("with_slab", (False, True), ids=("noslab", "slab"))
@pytest.mark.parametrize("N,F", MODELS)
def test_devstep_model_equals_devstep_and_keeps_the_slab(pkg, N, F, with_slab):
    lib = pkg.hip.load()
    count = model_count(N, F)
    floats = int(lib.gmc_w1_slab_floats(N, F))
    assert floats == BR.slab_floats(N, F)
    st = BR.adam_problem(count, f"model {N} {F}")
    plain = State(st, start=4)
    devstep(pkg, plain)
    report(f"model {N}x{F} (plain devstep)", BR.judge_adam(BR.adam_ref(st, 5, **H), *plain.wholes(), ("model", N, F)))
    s = State(st, start=4, slab_floats=floats if with_slab else 0)
    if with_slab:
        build_slab(pkg, s, N, F)
        check_slab(s, N, F, ("built", N, F))
    devstep_model(pkg, s, N, F)
    for a, b in zip(plain.wholes(), s.wholes()):
        assert a.tobytes() == b.tobytes()
    assert s.steps() == plain.steps() == 5
    if with_slab:
        check_slab(s, N, F, ("after the step", N, F))


@pytest.mark.parametrize("publish_n", (1, 3, 64, 65))
def test_publishing_form_ticks_first_and_equals_the_model_call(pkg, publish_n):
    lib, hip = pkg.hip.load(), pkg.hip
    N, F = 5, 16
    floats = BR.slab_floats(N, F)
    st = BR.adam_problem(model_count(N, F), f"publish {publish_n}")
    plain = State(st, start=6, slab_floats=floats)
    build_slab(pkg, plain, N, F)
    devstep_model(pkg, plain, N, F)
    s = State(st, start=6, slab_floats=floats)
    build_slab(pkg, s, N, F)
    values = (np.arange(publish_n, dtype=np.float32) - 3.5) * 0.25
    src = torch.from_numpy(BR.banded(values)[0]).cuda()
    host = torch.full((publish_n + 8,), float("nan")).pin_memory()
    dst = hip.mapped_ptr(host)
    assert dst, "pinned host memory must be mapped into the device"
    rc = lib.gmc_publish_adam_devstep_model_f32(src.data_ptr() + 4 * BAND, publish_n, dst, *s.ptrs(), N, F, s.slab_ptr(),
                                                *HYPER, s.counter_ptr(), hip.stream())
    hip.check(rc, "gmc_publish_adam_devstep_model_f32")
    torch.cuda.current_stream().synchronize()
    got = host.numpy()
    assert np.array_equal(got[:publish_n], values) and np.isnan(got[publish_n:]).all()
    assert s.steps() == plain.steps() == 7
    for a, b in zip(plain.wholes(), s.wholes()):
        assert a.tobytes() == b.tobytes()
    assert plain.slab.cpu().numpy().tobytes() == s.slab.cpu().numpy().tobytes()
    check_slab(s, N, F, ("publishing form", publish_n))
    report(f"publishing form n {publish_n}", BR.judge_adam(BR.adam_ref(st, 7, **H), *s.wholes(), ("publish", publish_n)))


@pytest.mark.parametrize("N,F", SLABS)
def test_w1_slab(pkg, N, F):
    rng = np.random.RandomState(N + F)
    W1 = rng.standard_normal((N, F)).astype(np.float32)
    src = torch.from_numpy(BR.banded(W1.ravel())[0]).cuda()
    floats = int(pkg.hip.load().gmc_w1_slab_floats(N, F))
    assert floats == BR.slab_floats(N, F)
    slab = torch.full((floats + 2 * BAND,), float("nan"), device="cuda")
    rc = pkg.hip.load().gmc_w1_slab_f32(src.data_ptr() + 4 * BAND, N, F, slab.data_ptr() + 4 * BAND, pkg.hip.stream())
    pkg.hip.check(rc, "gmc_w1_slab_f32")
    torch.cuda.synchronize()
    whole = slab.cpu().numpy()
    BR.judge_slab(W1, whole, what=("slab", N, F))
    assert np.array_equal(whole[BAND:-BAND].reshape(-1, N, 16), _slab_of(W1))


@pytest.mark.parametrize("n", (1, 63, 64, 65, 200))
def test_publish(pkg, n):
    hip = pkg.hip
    values = np.random.RandomState(n).standard_normal(n).astype(np.float32)
    src = torch.from_numpy(BR.banded(values)[0]).cuda()
    host = torch.full((n + 8,), float("nan")).pin_memory()
    dst = hip.mapped_ptr(host)
    assert dst, "pinned host memory must be mapped into the device"
    hip.check(hip.load().gmc_publish_f32(src.data_ptr() + 4 * BAND, n, dst, hip.stream()), "gmc_publish_f32")
    torch.cuda.current_stream().synchronize()
    got = host.numpy()
    assert np.array_equal(got[:n], values) and np.isnan(got[n:]).all()
