"""The rules of include/gcnmaxcut_sdp.h restated in numpy, written from the header's text: init, visit, value and
hyperplanes of the low-rank max-cut relaxation, every product and sum a float32 operation of its own, so the GPU tests
compare bytes.  ``dtype=np.float64`` runs the same rules in float64 (the same start: the init's integers are exact).

A batch is anything with ``B, R, goff, rowptr, gcol, vals`` (vals None: unit weights) - gcn-max-cut_amd/graph.py's
BatchArrays; the order arrays are gmc_order_host_t's for K = 2 (:func:`order_of`).
"""
import ctypes as C

import numpy as np

U = np.uint64
GOLD = U(0x9E3779B97F4A7C15)
PLANE_TAG = U(0x53445020504C414E)
TILE = 256


def mix64(z):
    z = np.array(z, U)   # (a copy: the steps below work in place)
    with np.errstate(over="ignore"):
        z ^= z >> U(30)
        z *= U(0xBF58476D1CE4E5B9)
        z ^= z >> U(27)
        z *= U(0x94D049BB133111EB)
        z ^= z >> U(31)
    return z


def butterfly(x):
    """x[..., i] += x[..., i ^ d] for d = n/2 .. 1 over the last axis (n a power of two); every entry: the total."""
    n = x.shape[-1]
    idx = np.arange(n)
    d = n // 2
    while d >= 1:
        x = x + x[..., idx ^ d]
        d //= 2
    return x


def total(x):
    """Entry 0 of :func:`butterfly` (the same additions: for i < d, i ^ d is i + d), without the other lanes' work."""
    n = x.shape[-1]
    while n > 1:
        n //= 2
        x = x[..., :n] + x[..., n:2 * n]
    return x[..., 0]


def order_of(pkg, h, terminals):
    """(order, cgoff, cptr, max_classes) of gmc_order_host_t(K = 2, terminals) for the host batch h."""
    classes = C.c_int32(-1)
    order = np.zeros(max(h.R, 1), np.int32)
    cgoff = np.zeros(h.B + 1, np.int32)
    cptr = np.zeros(h.R + h.B, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    go32 = np.ascontiguousarray(h.goff, np.int32)
    rc = pkg.hip.load().gmc_order_host_t(h.B, ptr(go32), ptr(h.rowptr), ptr(h.lcol), 2, int(terminals), ptr(order),
                                         ptr(cgoff), ptr(cptr), cptr.size, C.byref(classes))
    assert rc == 0, rc
    return order, cgoff, cptr, int(classes.value)


def colour_rows(h, terminals, order, cgoff, cptr, max_classes):
    """Per colour 0 .. max_classes - 1 the batch rows a launch visits (every graph's nodes of that colour)."""
    first = 2 if terminals else 0
    goff = np.asarray(h.goff, np.int64)
    out = []
    for c in range(max_classes):
        rows = []
        for g in range(h.B):
            k0 = int(cgoff[g])
            n = int(goff[g + 1] - goff[g])
            if c >= int(cgoff[g + 1]) - k0 - 1 or n < max(first, 1):
                continue
            r = order[int(cptr[k0 + c]):int(cptr[k0 + c + 1])].astype(np.int64)
            l = r - goff[g]
            rows.append(r[(l >= first) & (l < n)])
        out.append(np.concatenate(rows) if rows else np.zeros(0, np.int64))
    return out


def init(h, rank, terminals, gkey, dtype=np.float32):
    """Rule 1: V [R][rank]."""
    V = np.zeros((h.R, rank), dtype)
    goff = np.asarray(h.goff, np.int64)
    t = np.zeros((1, rank), dtype)
    t[0, 0] = 1
    for g in range(h.B):
        r0, n = int(goff[g]), int(goff[g + 1] - goff[g])
        for lo in range(0, n, 1 << 13):   # (in pieces that stay in cache: a 2^20-node graph has 2^26 counters)
            ls = np.arange(lo, min(n, lo + (1 << 13)), dtype=U)
            ctr = ls[:, None] * U(rank) + np.arange(rank, dtype=U)[None, :] + U(1)
            with np.errstate(over="ignore"):
                i = mix64(np.array([gkey[g]], U) + GOLD * ctr) >> U(40)
            x = (i.astype(np.int64) - (1 << 23)).astype(dtype)
            s = total(x * x)[:, None]
            with np.errstate(invalid="ignore", divide="ignore"):
                V[r0 + lo:r0 + lo + ls.size] = np.where(s == 0, t, x / np.sqrt(s))
        if terminals:
            V[r0], V[r0 + 1] = t[0], -t[0]
            V[r0 + 1, 1:] = 0.0
    return V


def _entries(h, rows):
    """Yields (index into rows, entry id, neighbour row) position by position along the CSR rows, diagonal skipped."""
    start = h.rowptr[rows].astype(np.int64)
    deg = h.rowptr[rows + 1].astype(np.int64) - start
    for j in range(int(deg.max()) if rows.size else 0):
        act = np.flatnonzero(deg > j)
        e = start[act] + j
        u = h.gcol[e].astype(np.int64)
        keep = u != rows[act]
        if act.size == rows.size and keep.all():
            yield slice(None), e, u          # (every row has this entry: no gather and scatter of the accumulator)
        else:
            yield act[keep], e[keep], u[keep]


def _weights(h, e, dtype):
    return np.ones(e.size, dtype) if h.vals is None else h.vals[e].astype(dtype)


def visit(h, V, rows, cost):
    """Rule 2 for the rows of one colour, in place."""
    dtype = V.dtype.type
    g = np.zeros((rows.size, V.shape[1]), dtype)
    if cost is not None:
        g[:, 0] = cost[rows, 0].astype(dtype) - cost[rows, 1].astype(dtype)
    for idx, e, u in _entries(h, rows):
        g[idx] = g[idx] + _weights(h, e, dtype)[:, None] * V[u]
    n = np.sqrt(total(g * g))
    ok = (n != 0) & np.isfinite(n)
    V[rows[ok]] = -(g[ok] / n[ok, None])


def value(h, V, cost):
    """Rule 3: value [B]."""
    dtype = V.dtype.type
    rows = np.arange(h.R, dtype=np.int64)
    p = np.zeros(h.R, dtype)
    for idx, e, u in _entries(h, rows):
        d = np.cumsum(V[rows[idx]] * V[u], axis=1, dtype=dtype)[:, -1]   # (accumulate: strictly k ascending, one rounding each)
        p[idx] = p[idx] + _weights(h, e, dtype) * (dtype(1) - d)
    x = dtype(0.25) * p
    if cost is not None:
        c0, c1 = cost[:, 0].astype(dtype), cost[:, 1].astype(dtype)
        x = x - ((c0 + c1) * dtype(0.5) + ((c0 - c1) * dtype(0.5)) * V[:, 0])
    out = np.zeros(h.B, dtype)
    goff = np.asarray(h.goff, np.int64)
    for g in range(h.B):
        r0, n = int(goff[g]), int(goff[g + 1] - goff[g])
        tiles = (n + TILE - 1) // TILE
        pad = np.zeros(tiles * TILE, dtype)
        pad[:n] = x[r0:r0 + n]
        waves = total(pad.reshape(tiles, TILE // 64, 64))
        tile = np.zeros(tiles, dtype)
        for w in range(TILE // 64):
            tile = tile + waves[:, w]
        s = dtype(0)
        for t in range(tiles):
            s = s + tile[t]
        out[g] = s
    return out


def relax(pkg, h, rank, terminals, cost, gkey, sweeps, V=None, dtype=np.float32, values=False):
    """gmc_sdp_relax_f32: (V, value); V None: init = 1.  values: the value after every sweep too (a list)."""
    order, cgoff, cptr, classes = order_of(pkg, h, terminals)
    colours = colour_rows(h, terminals, order, cgoff, cptr, classes)
    V = init(h, rank, terminals, gkey, dtype) if V is None else V.astype(dtype).copy()
    trace = [value(h, V, cost)] if values else None
    for _ in range(sweeps):
        for rows in colours:
            visit(h, V, rows, cost)
        if values:
            trace.append(value(h, V, cost))
    if values:
        return V, trace[-1], trace
    return V, value(h, V, cost)


def normals(gkey_g, rank, first_plane, planes):
    """Rule 4: h [planes][rank] float32 of one graph."""
    m = np.arange(first_plane, first_plane + planes, dtype=U)[:, None, None]
    j = np.arange(12, dtype=U)[None, :, None]
    k = np.arange(rank, dtype=U)[None, None, :]
    with np.errstate(over="ignore"):
        d = mix64((np.array([gkey_g], U) ^ PLANE_TAG) + GOLD * ((m * U(12) + j) * U(64) + k + U(1))) >> U(44)
    return (d.sum(axis=1).astype(np.int64) - 6 * (1 << 20)).astype(np.float32)


def round_planes(h, rank, terminals, V, gkey, first_plane, planes):
    """gmc_sdp_round_f32: assign [planes][R] int8."""
    out = np.zeros((planes, h.R), np.int8)
    goff = np.asarray(h.goff, np.int64)
    for g in range(h.B):
        r0, n = int(goff[g]), int(goff[g + 1] - goff[g])
        hs = normals(gkey[g], rank, first_plane, planes)
        p = np.stack([np.cumsum(hs[m][None, :] * V[r0:r0 + n], axis=1, dtype=np.float32)[:, -1] for m in range(planes)])
        out[:, r0:r0 + n] = np.where((p >= 0) == (hs[:, :1] >= 0), 0, 1)
        if terminals:
            out[:, r0], out[:, r0 + 1] = 0, 1
    return out


def cut_of(h, assign):
    """The cut of a class array [R] per graph in float64 (every undirected edge once)."""
    rows = np.repeat(np.arange(h.R), np.diff(h.rowptr))
    w = np.ones(rows.size) if h.vals is None else h.vals.astype(np.float64)
    cross = (assign[rows] != assign[h.gcol]) * w
    run = np.concatenate([[0.0], np.cumsum(cross)])
    e = h.rowptr[np.asarray(h.goff, np.int64)]
    return 0.5 * (run[e[1:]] - run[e[:-1]])
