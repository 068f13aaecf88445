"""Float64 references, derived per-element bounds and float32 restatements of the library's building blocks
(include/gcnmaxcut.h, "building blocks"): gmc_spmm_f32, gmc_dense_hw2_f32, the Adam family, gmc_w1_slab_f32.  Plain
numpy: tests/test_blocks_host.py (CPU) and the GPU modules test_gpu_spmm / test_gpu_dense_hw2 / test_gpu_adam import it.

Every bound is derived from the kernel's chain of operations, with u = 2^-24 (round to nearest, fp32), never from a
measurement.  A misplaced, missing or doubled element is off by whole terms, so the bounds catch indexing faults too.

SpMM Y (csrc/spmm.hip: gather_rows + the epilogue of spmm_rows_v4 / _wide; spmm_rows_scalar):
    acc = 0; for e in CSR order: acc = fma(v_e, x_e, acc)   (acc += x_e without weights)        d_r roundings
    y = fma(acc, s_r, bias_c); relu                                                             1 rounding
    bound_Y[r,c] = (d_r + 3) u (|s_r| sum_e |v_e| |X[col_e,c]| + |bias_c|);  relu is 1-Lipschitz.
SpMM Z0 (the W2 epilogue): z_k = s_r * sum_c y_c W2[c,k], the F products summed per lane, then over the wave
    bound_Z[r,k] = |s_r| ((F + 3) u sum_c |Y64[r,c]| |W2[c,k]| + sum_c bound_Y[r,c] |W2[c,k]|)
    (an F-term sum in any order, the rounding of "* s", and Y's own error carried through).
H@W2 (csrc/dense_mfma.hip): z = dinv_r * (a k-ordered fma chain of F products, 4 per MFMA step)
    bound[r,k] = (F + 3) u |dinv_r| sum_c |H[r,c]| |W2[c,k]|.
Adam (csrc/adam.hip, adam1), against a float64 step from the same float32 p, g, m, v:
    m' = m + (g - m) c1                                   one subtraction, one product, one add;  c1 = fl(1 - beta1)
    v' = fma(c2 g, g, v b2)                               two products and an fma;  c2 = fl(1 - beta2), b2 = fl(beta2)
    denom = sqrt(v') / fl(sqrt(bc2)) + fl(eps)            root, division, add
    p' = p - fl(lr / bc1) * (m' / denom)                  division, product, subtraction
    bm = 3u (|m| + |g|);  bv = 5u v'_64;
    bp = u max(|p_ref|, |p_got|) + 16u |update| + (step_size / denom) bm
    The update's share with a correctly rounded division and root is 10u (three rounded constants, half of v's 5u
    through the root, root, division, add, division, product); the 16 leaves each of the two divisions and the root
    2 ulp.  The final subtraction is the u max(|p|) term, m's error reaches p through step_size / denom.
    The library is built with -O3 and no fast-math flag (csrc/Makefile), so hipcc's default
    -fhip-fp32-correctly-rounded-divide-sqrt holds: adam.hip's gfx950 ISA has, per element, the v_div_scale_f32 /
    v_div_fmas_f32 / v_div_fixup_f32 sequence for both divisions (no bare v_rcp_f32 product) and a v_sqrt_f32 followed
    by its fma correction - established by compiling csrc/adam.hip to assembly (hipcc -S, same flags) and reading
    adam_kernel.  Contraction (fma for "m + (g - m) c1" and "p - s (m / denom)") only removes roundings.
    The float32 restatement below (adam_f32, no contraction) over steps 1, 2, 3, 10, 1000, 100000 and gradient scales
    1e-6 .. 1e3 reaches 0.32 of bm (0.96u of the 3u), 0.55 of bv (2.8u of the 5u) and 0.997 of bp; p's ratio is
    dominated by its own final rounding, which is why a third of the tests' parameters are exactly 0 and a third tiny:
    over the parameters that start at 0 ("p0") it is 0.25 (tests/test_blocks_host.py prints them).
"""
import zlib

import numpy as np

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)     # torch.optim.Adam's defaults, as the trainer uses them


class Rejected(AssertionError):
    """What the checker raises for an answer that is outside its bound or touched memory it must not."""


def seed_of(name):
    return zlib.crc32(str(name).encode()) & 0x7fffffff


def up4(n):
    return (n + 3) // 4 * 4


def fma32(a, b, c):
    """fl32(a * b + c) of float32 operands: the product of two float32 is exact in float64."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


# ---- the checker ------------------------------------------------------------------------------------------------------
def embed(data, ld, band=1):
    """data [rows, cols] inside a NaN buffer [rows + 2 band, ld]: (whole, mask of the data elements)."""
    rows, cols = data.shape
    whole = np.full((rows + 2 * band, ld), np.nan, F32)
    inside = np.zeros(whole.shape, bool)
    whole[band:band + rows, :cols] = data
    inside[band:band + rows, :cols] = True
    return whole, inside


def judge(whole, inside, ref, bound, what):
    """The whole buffer as the kernel left it against the float64 reference: everything outside `inside` is still NaN,
    every data element is finite and within `bound` of `ref`.  Returns the worst err / bound; raises Rejected."""
    whole = np.asarray(whole)
    if not np.isnan(whole[~inside]).all():
        raise Rejected((what, "a write outside the data (NaN band or padding)"))
    got = whole[inside].reshape(ref.shape).astype(F64)
    if not np.isfinite(got).all():
        raise Rejected((what, "an element never written, or NaN padding read"))
    err = np.abs(got - ref)
    if (err > bound).any():
        at = np.unravel_index(np.argmax(err - bound), err.shape)
        raise Rejected((what, "bound exceeded", tuple(int(i) for i in at), float(err[at]), float(bound[at])))
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def judge_exact(whole, inside, want, what):
    """As judge, for data that must be reproduced bit for bit."""
    whole = np.asarray(whole)
    if not np.isnan(whole[~inside]).all():
        raise Rejected((what, "a write outside the data (NaN band or padding)"))
    got = whole[inside].reshape(want.shape)
    if not np.array_equal(got, np.asarray(want, F32)):
        raise Rejected((what, "differs", int((got != want).sum())))


# ---- SpMM ---------------------------------------------------------------------------------------------------------------
def spmm_case(name, rows, F, **kw):
    """One gmc_spmm_f32 call: `rows` = entries per row; ldx = F + padx, ldy = F + pady unless given; xoff = floats X's
    pointer is moved by (1: a pointer that is not 16-byte aligned)."""
    c = dict(name=name, rows=list(rows), F=F, vals=True, scale=True, bias=True, relu=1, epi=False, padx=4, pady=8,
             ldx=None, ldy=None, group_rows=0, xoff=0)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def spmm_problem(c):
    """The operands of a case, seeded by its name.  Rectangular (n_src > n_rows), sorted rows, source row 0 referenced
    by no entry and NaN (idle lanes of the kernel point at it), signed real weights with exact zeros among them, X's
    leading-dimension padding NaN."""
    rng = np.random.RandomState(seed_of(c["name"]))
    lens = np.asarray(c["rows"], np.int64)
    n, F = lens.size, c["F"]
    n_src = max(n + 8, 208)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = np.zeros(max(nnz, 1), np.int32)
    for r, d in enumerate(lens):
        col[rowptr[r]:rowptr[r + 1]] = np.sort(rng.choice(np.arange(1, n_src), int(d), replace=False))
    vals = None
    if c["vals"]:
        vals = rng.standard_normal(max(nnz, 1)).astype(F32)
        vals[rng.rand(vals.size) < 0.1] = 0.0
    ldx = c["ldx"] or F + c["padx"]
    ldy = c["ldy"] or F + c["pady"]
    X = np.full((n_src, ldx), np.nan, F32)
    X[1:, :F] = rng.standard_normal((n_src - 1, F))
    scale = (rng.uniform(0.1, 2.0, max(n, 1)) * rng.choice([-1.0, 1.0], max(n, 1))).astype(F32) if c["scale"] else None
    bias = (0.5 * rng.standard_normal(F)).astype(F32) if c["bias"] else None
    W2 = rng.standard_normal((F, 3)).astype(F32) if c["epi"] else None
    return dict(case=c, n=n, F=F, n_src=n_src, rowptr=rowptr, col=col, vals=vals, X=X, ldx=ldx, ldy=ldy, scale=scale,
                bias=bias, W2=W2, relu=c["relu"])


def spmm_ref(pr):
    """(Y64, bound_Y, Z64 or None, bound_Z or None) of a problem."""
    n, F, rp, col = pr["n"], pr["F"], pr["rowptr"], pr["col"]
    X = pr["X"][:, :F].astype(F64)
    s = pr["scale"].astype(F64)[:n] if pr["scale"] is not None else np.ones(n)
    b = pr["bias"].astype(F64) if pr["bias"] is not None else np.zeros(F)
    Y, bY = np.zeros((n, F)), np.zeros((n, F))
    for r in range(n):
        e = slice(rp[r], rp[r + 1])
        xs = X[col[e]]
        v = pr["vals"][e].astype(F64)[:, None] if pr["vals"] is not None else np.ones((xs.shape[0], 1))
        Y[r] = s[r] * (v * xs).sum(0) + b
        bY[r] = (xs.shape[0] + 3) * U * (abs(s[r]) * (np.abs(v) * np.abs(xs)).sum(0) + np.abs(b))
    if pr["relu"]:
        Y = np.maximum(Y, 0.0)
    if pr["W2"] is None:
        return Y, bY, None, None
    W = pr["W2"].astype(F64)
    Z = s[:, None] * (Y @ W)
    bZ = np.abs(s)[:, None] * ((F + 3) * U * (np.abs(Y) @ np.abs(W)) + bY @ np.abs(W))
    return Y, bY, Z, bZ


def spmm_f32(pr, order="scale, bias, relu"):
    """Float32 restatement: the sequential CSR-order sum and the epilogue, (Y, Z or None).  `order` other than the
    kernel's gives the wrong answers of tests/test_blocks_host.py: "scale after bias" (s * (acc + bias)),
    "relu before bias"."""
    n, F, rp, col = pr["n"], pr["F"], pr["rowptr"], pr["col"]
    X = pr["X"][:, :F]
    s = pr["scale"][:n] if pr["scale"] is not None else np.ones(n, F32)
    b = pr["bias"] if pr["bias"] is not None else np.zeros(F, F32)
    Y = np.zeros((n, F), F32)
    for r in range(n):
        acc = np.zeros(F, F32)
        for e in range(rp[r], rp[r + 1]):
            acc = fma32(pr["vals"][e], X[col[e]], acc) if pr["vals"] is not None else acc + X[col[e]]
        if order == "scale, bias, relu":
            y = fma32(acc, s[r], b)
            Y[r] = np.maximum(y, F32(0)) if pr["relu"] else y
        elif order == "scale after bias":
            y = (acc + b) * s[r]
            Y[r] = np.maximum(y, F32(0)) if pr["relu"] else y
        elif order == "relu before bias":
            Y[r] = np.maximum(acc * s[r], F32(0)) + b
        else:
            raise ValueError(order)
    if pr["W2"] is None:
        return Y, None
    prod = Y[:, :, None] * pr["W2"][None]                                   # [n, F, 3], each product rounded
    Z = np.cumsum(prod, axis=1, dtype=F32)[:, -1, :] * s[:, None]
    return Y, Z.astype(F32)


def judge_spmm(pr, Ywhole, Zwhole, what=None):
    """The Y buffer [(n + 2), ldy] (one NaN row either side) and, with W2, the Z0 buffer [(n + 2), 3] of a call."""
    what = what or pr["case"]["name"]
    n, F = pr["n"], pr["F"]
    Y64, bY, Z64, bZ = spmm_ref(pr)
    inside = np.zeros(np.shape(Ywhole), bool)
    inside[1:n + 1, :F] = True
    out = {"Y": judge(Ywhole, inside, Y64, bY, (what, "Y"))}
    if Z64 is not None:
        zin = np.zeros(np.shape(Zwhole), bool)
        zin[1:n + 1] = True
        out["Z0"] = judge(Zwhole, zin, Z64, bZ, (what, "Z0"))
    return out


def spmm_wholes(pr, Y, Z):
    """A restatement's (Y, Z) laid into NaN buffers the way the GPU module lays out the device buffers."""
    Yw = embed(Y, pr["ldy"])[0]
    return Yw, None if Z is None else embed(Z, 3)[0]


# ---- H @ W2 -------------------------------------------------------------------------------------------------------------
def dense_case(n, F, pad=0, kind="real"):
    return dict(name=f"hw2 n{n} F{F} pad{pad} {kind}", n=n, F=F, pad=pad, kind=kind)


def dense_problem(c):
    """H [n, ldh] with NaN padding (ldh = F rounded up to 4, + pad), dinv of both signs, W2 [F, 3].  kind "int": small
    asymmetric integers and dinv = +-2, exact in fp32."""
    rng = np.random.RandomState(seed_of(c["name"]))
    n, F = c["n"], c["F"]
    ldh = up4(F) + c["pad"]
    H = np.full((n, ldh), np.nan, F32)
    if c["kind"] == "int":
        H[:, :F] = np.arange(n * F).reshape(n, F) % 7 - 3
        W2 = (np.arange(F * 3).reshape(F, 3) % 5 - 2).astype(F32)
        dinv = np.where(np.arange(n) % 3 == 0, -2.0, 2.0).astype(F32)
    else:
        H[:, :F] = rng.standard_normal((n, F))
        W2 = rng.standard_normal((F, 3)).astype(F32)
        dinv = (rng.uniform(0.1, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    return dict(case=c, n=n, F=F, ldh=ldh, H=H, W2=W2, dinv=dinv)


def dense_ref(pr):
    H, W, d = pr["H"][:, :pr["F"]].astype(F64), pr["W2"].astype(F64), pr["dinv"].astype(F64)[:, None]
    return d * (H @ W), (pr["F"] + 3) * U * np.abs(d) * (np.abs(H) @ np.abs(W))


def dense_f32(pr, F_used=None):
    """Float32 restatement: a k-ordered fma chain, then the row scale.  F_used < F drops the tail (a wrong answer)."""
    H, W = pr["H"], pr["W2"]
    acc = np.zeros((pr["n"], 3), F32)
    for k in range(pr["F"] if F_used is None else F_used):
        acc = fma32(H[:, k:k + 1], W[k:k + 1, :], acc)
    return acc * pr["dinv"][:, None]


def judge_dense(pr, Zwhole, what=None):
    """The Z0 buffer [(n + 2), 3] of a call; "int" cases must be exact."""
    what = what or pr["case"]["name"]
    ref, bound = dense_ref(pr)
    inside = np.zeros(np.shape(Zwhole), bool)
    inside[1:pr["n"] + 1] = True
    if pr["case"]["kind"] == "int":
        judge_exact(Zwhole, inside, ref.astype(F32), what)
        return 0.0
    return judge(Zwhole, inside, ref, bound, what)


# ---- Adam ---------------------------------------------------------------------------------------------------------------
BAND = 64      # floats of NaN either side of p, g, m, v (256 bytes: the kernel's base pointer stays 16-byte aligned)


def adam_problem(count, name=None):
    """p, g, m, v of `count` elements: a third of the parameters exactly 0, a third of size 1e-4, a third of size 1
    (interleaved); gradients of scales 1e-6 .. 1e3 with a block of exact zeros; a block of m = v = 0 beside non-zero
    moments.  The blocks are placed by position so that every count has them."""
    rng = np.random.RandomState(seed_of(name or f"adam {count}"))
    i = np.arange(count)
    p = rng.standard_normal(count) * np.choose(i % 3, [0.0, 1e-4, 1.0])
    gs = 10.0 ** rng.randint(-6, 4, count)
    g = rng.standard_normal(count) * gs
    g[(i % 16) >= 12] = 0.0                                   # a block of exact zeros in every 16
    m = 0.1 * gs * rng.standard_normal(count)
    v = (0.1 * gs * rng.standard_normal(count)) ** 2
    fresh = (i % 32) < 8                                      # a block without history in every 32
    m[fresh], v[fresh] = 0.0, 0.0
    return dict(p=p.astype(F32), g=g.astype(F32), m=m.astype(F32), v=v.astype(F32))


def adam_ref(st, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """One float64 Adam step number t from the float32 state st = dict(p, g, m, v)."""
    p, g, m, v = (st[k].astype(F64) for k in "pgmv")
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    m1 = m + (g - m) * (1.0 - beta1)
    v1 = beta2 * v + (1.0 - beta2) * g * g
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    step_size = lr / bc1
    update = step_size * m1 / denom
    return dict(p=p - update, m=m1, v=v1, update=update, reach=step_size / denom, g=st["g"], zero=st["p"] == 0,
                bm=3 * U * (np.abs(m) + np.abs(g)), bv=5 * U * v1)


def adam_f32(st, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wrong=None):
    """Float32 restatement of adam1 with the host's double-precision bias corrections: dict(p, m, v).  `wrong`:
    "eps inside the root", "float32 bias corrections" (the wrong answers of tests/test_blocks_host.py)."""
    p, g, m, v = (st[k].astype(F32) for k in "pgmv")
    if wrong == "float32 bias corrections":
        bc1 = F32(1) - F32(beta1) ** F32(t)
        bc2 = F32(1) - F32(beta2) ** F32(t)
        step_size, bc2_sqrt = F32(lr) / bc1, np.sqrt(bc2)
    else:
        with np.errstate(divide="ignore"):     # (step 0, a wrong answer: lr / 0 as the device would compute it)
            step_size, bc2_sqrt = F32(F64(lr) / F64(1.0 - beta1 ** t)), F32(np.sqrt(1.0 - beta2 ** t))
    c1, b2, c2, epsf = F32(1.0 - beta1), F32(beta2), F32(1.0 - beta2), F32(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        m1 = m + (g - m) * c1
        v1 = fma32(c2 * g, g, v * b2)
        if wrong == "eps inside the root":
            denom = np.sqrt(v1 / (bc2_sqrt * bc2_sqrt) + epsf)
        else:
            denom = np.sqrt(v1) / bc2_sqrt + epsf
        p1 = p - step_size * (m1 / denom)
    return dict(p=p1.astype(F32), m=m1.astype(F32), v=v1.astype(F32))


def banded(a, band=BAND):
    """A 1-d array inside NaN bands: (whole, mask)."""
    whole = np.full(a.size + 2 * band, np.nan, F32)
    whole[band:band + a.size] = a
    inside = np.zeros(whole.size, bool)
    inside[band:band + a.size] = True
    return whole, inside


def judge_adam(ref, pw, mw, vw, gw, what):
    """The four banded buffers after a step against adam_ref's result: bands NaN, g unchanged, m, v, p within their
    bounds (p's uses the value the kernel gave).  Returns the worst ratios {"p", "m", "v"} and "p0": p's over the parameters
    that started at exactly 0."""
    n = ref["p"].size
    inside = np.zeros(np.shape(pw), bool)
    inside[BAND:BAND + n] = True
    judge_exact(gw, inside, ref["g"], (what, "g changed"))
    out = {"m": judge(mw, inside, ref["m"], ref["bm"], (what, "m")),
           "v": judge(vw, inside, ref["v"], ref["bv"], (what, "v"))}
    got = np.asarray(pw)[inside].astype(F64)
    with np.errstate(invalid="ignore"):
        bp = U * np.maximum(np.abs(ref["p"]), np.abs(got)) + 16 * U * np.abs(ref["update"]) + ref["reach"] * ref["bm"]
    bp = np.where(np.isfinite(bp), bp, 0.0)
    out["p"] = judge(pw, inside, ref["p"], bp, (what, "p"))
    z = ref["zero"] & (bp > 0)                      # where p started at 0 its own rounding hides nothing of the update
    out["p0"] = float((np.abs(got - ref["p"])[z] / bp[z]).max()) if z.any() else 0.0
    return out


def adam_wholes(res, g):
    return tuple(banded(a)[0] for a in (res["p"], res["m"], res["v"], g))


# ---- the slab copy of conv1.weight ---------------------------------------------------------------------------------
def slab_floats(N, F):
    return (F + 15) // 16 * N * 16


def slab_index(row, col, N):
    """gmc::slab16_index: element (row, col) of W1 [N, F] in the layout [ceil(F/16)][N][16]."""
    return ((col >> 4) * N + row) * 16 + (col & 15)


def slab_f32(W1):
    """The slab copy by the index formula, flat, pad columns zero."""
    N, F = W1.shape
    out = np.zeros(slab_floats(N, F), F32)
    r, c = np.meshgrid(np.arange(N), np.arange(F), indexing="ij")
    out[slab_index(r, c, N)] = W1
    return out


def judge_slab(W1, whole, band=BAND, what="slab"):
    """A banded slab buffer against W1: exact, pad columns exactly zero, bands NaN."""
    want = slab_f32(np.asarray(W1, F32))
    inside = np.zeros(np.shape(whole), bool)
    inside[band:band + want.size] = True
    judge_exact(whole, inside, want, what)
