"""CPU restatement of the discrete simulated bifurcation of dense two-class instances (include/gcnmaxcut_bifurcation.h,
gmc_dense_sb_f32 and gmc_dense_sb_init_f32), written from the header's text in numpy float32: the signs, the k-ascending
fmaf chain of the force (a product with -1, 0 or +1 is exact, so every step of the chain is one rounded float32 addition),
the separately rounded operations of the update, the walls, the class bytes and the seeded start.  x and y are held as the
header lays them out, [n, cands] per problem and [B * n, cands] for a call.

Also here: the cases tests/test_gpu_bifurcation.py runs and tests/test_bifurcation_host.py checks for wall hits."""
import numpy as np

from tests import dense_ref as DR

F32 = np.float32
ZERO = F32(0)
MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix64(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def init(n, cands, seed, amplitude, cand_ids=None):
    """(x, y) [n, cands] float32 of one problem: the seeded start."""
    ids = range(cands) if cand_ids is None else cand_ids
    t = np.zeros((n, len(ids)), F32)
    for j, cand in enumerate(ids):
        for v in range(n):
            h = mix64(seed + GOLD * (((int(cand) << 32) | v) + 1))
            t[v, j] = F32(h >> 40)                       # 24 bits: exact
    t = t - F32(8388608.0)
    u = t * F32(2.0 ** -23)
    return np.zeros_like(u), (F32(amplitude) * u).astype(F32)


def signs(x):
    return np.where(x > 0, F32(1), np.where(x < 0, F32(-1), ZERO)).astype(F32)


def force(Wz, s):
    """Step 2: f [n, cands] float32 = the chain fmaf(W[v][u], s_u, f_v) over u ascending, from +0."""
    f = np.zeros(s.shape, F32)
    cols = np.ascontiguousarray(Wz.T)                    # cols[u] is W[:, u]
    for u in range(Wz.shape[0]):
        f = f + cols[u][:, None] * s[u][None, :]         # the product is exact: one rounding per step, as fmaf
    return f


def run(W, cost, x, y, pump, c0, dt, tally=None):
    """One problem: W [n, ld], cost [n, 2] or None, x / y [n, cands] -> (x, y, class bytes [cands, n] int8) after
    len(pump) steps.  tally: a dict that gains the wall hits `up` and `down`."""
    Wz = DR._square(W)
    x, y = np.array(x, F32, copy=True), np.array(y, F32, copy=True)
    c0, dt = F32(c0), F32(dt)
    g = None if cost is None else (np.asarray(cost, F32)[:, 0] - np.asarray(cost, F32)[:, 1])[:, None]
    for a in np.asarray(pump, F32):
        f = force(Wz, signs(x))
        if g is not None:
            f = f + g
        p = a * x
        q = c0 * f
        r = p + q
        m = dt * r
        y = y - m
        m2 = dt * y
        x = x + m2
        up, down = x > 1, x < -1
        x = np.where(up, F32(1), np.where(down, F32(-1), x)).astype(F32)
        y = np.where(up | down, ZERO, y).astype(F32)
        if tally is not None:
            tally["up"] = tally.get("up", 0) + int(up.sum())
            tally["down"] = tally.get("down", 0) + int(down.sum())
    return x, y, (x < 0).T.astype(np.int8)


def run_batch(W, cost, x, y, pump, c0, dt, tally=None):
    """The whole call: W [B, n, ld], cost [B * n, 2] or None, x / y [B * n, cands] -> x, y [B * n, cands], assign
    [cands, B * n]."""
    B, n = W.shape[0], W.shape[1]
    outs = [run(W[b], None if cost is None else cost[b * n:(b + 1) * n], x[b * n:(b + 1) * n], y[b * n:(b + 1) * n], pump,
                c0, dt, tally) for b in range(B)]
    return (np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]),
            np.concatenate([o[2] for o in outs], axis=1))


def pump_table(steps):
    """The linear ramp of a0 - a(t) from 1 to 0, float32 (Testing.dense_bifurcation's)."""
    return np.linspace(1.0, 0.0, steps).astype(F32) if steps > 1 else np.ones(steps, F32)


def scale_c0(W):
    return 0.5 / DR.rms_field(W)


def descend(Wz, cost, S, sweeps=100):
    """Single-move descent of the states S [cands, n] (0 / 1) in float64: a node moves while that raises obj."""
    W64 = Wz.astype(np.float64)
    c = np.zeros((Wz.shape[0], 2)) if cost is None else np.asarray(cost, np.float64)
    S = S.copy()
    for _ in range(sweeps):
        moved = False
        for v in range(Wz.shape[0]):
            same = (W64[v][None, :] * (S == S[:, v:v + 1])).sum(axis=1)
            diff = (W64[v][None, :] * (S != S[:, v:v + 1])).sum(axis=1)
            own, other = c[v][S[:, v]], c[v][1 - S[:, v]]
            gain = (same - other) - (diff - own)          # obj after the move minus obj before
            go = gain > 0
            S[go, v] = 1 - S[go, v]
            moved |= bool(go.any())
        if not moved:
            break
    return S


def objective(Wz, cost, S):
    """obj(S) [cands] float64."""
    W64 = np.triu(Wz.astype(np.float64), 1)
    cut = np.einsum("cu,uv,cv->c", S.astype(np.float64), W64, 1.0 - S) + np.einsum("cu,uv,cv->c", 1.0 - S, W64,
                                                                                   S.astype(np.float64))
    if cost is None:
        return cut
    return cut - np.asarray(cost, np.float64)[np.arange(S.shape[1])[None, :], S].sum(axis=1)


# ---- the cases of tests/test_gpu_bifurcation.py (tests/test_bifurcation_host.py asserts the walls are hit in them) ---------
SEED = 0x13579BDF
#        n   B cands pad weights cost    steps
CASES = [(2, 1, 1, 0, "pm1", None, 37),
         (15, 1, 15, 5, "int", "int", 2),
         (16, 3, 16, 0, "real", "real", 37),
         (17, 1, 17, 5, "pm1", None, 37),
         (63, 1, 64, 0, "int", "int", 1),
         (64, 1, 65, 5, "real", None, 37),
         (65, 3, 200, 5, "real", "real", 2),
         (65, 1, 65, 0, "pm1", "zero", 37),
         (130, 1, 200, 5, "int", "int", 37),
         (130, 3, 17, 0, "real", "real", 37),
         (64, 1, 16, 0, "int", None, 0),
         (17, 3, 1, 5, "real", "int", 0)]
INTEGER = ("pm1", "int")
RUN = dict(dt=1.25, amplitude=0.1)                      # c0 = 4 * scale_c0(W): the walls are hit within 37 steps


def is_integer_case(case):
    return case[4] in INTEGER and case[5] in (None, "zero", "int")


def case_inputs(case):
    n, B, cands, pad, weights, cost_kind, steps = case
    square = np.stack([DR.weights_of(weights, n, 700 * n + b) for b in range(B)])
    c0 = float(F32(4.0 * scale_c0(square)))
    x = np.concatenate([init(n, cands, SEED, RUN["amplitude"])[0] for _ in range(B)])
    y = np.concatenate([init(n, cands, SEED, RUN["amplitude"])[1] for _ in range(B)])
    if steps == 0:                                      # a state with every kind of position, zeros included
        rng = np.random.RandomState(n)
        x = rng.choice([-1.0, -0.25, -0.0, 0.0, 0.5, 1.0], size=x.shape).astype(F32)
    return dict(W=DR.padded(square, n + pad), square=square, cost=DR.cost_of(cost_kind, B * n, 5 * n + 2), x=x, y=y,
                pump=pump_table(steps), c0=c0, dt=RUN["dt"])
