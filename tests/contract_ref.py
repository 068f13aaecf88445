"""The contraction of pinned nodes (include/gcnmaxcut.h, "pinning any nodes to classes") restated in plain numpy, one
row and one addition at a time, in the sum orders the header fixes:

* a free node's merged weight to a class: float32, from +0, the entries in ascending neighbour id;
* ``fixed_cut``: per pinned row the entries to pinned nodes of another class and a larger id, from +0 in ascending id;
  per tile of 256 rows a butterfly (distances 32 .. 1) over each quarter of 64 and the quarters in order; the tiles from
  +0 in order.

Graphs are ``(n, rowptr, col, weight or None)`` with sorted rows, as a ``GraphHandle`` holds them."""
import itertools

import numpy as np

f32 = np.float32


class BadPins(ValueError):
    pass


def fold(t):
    """fixed_cut of one graph from its per-row sums."""
    total = f32(0)
    for start in range(0, len(t), 256):
        tile = [f32(x) for x in t[start:start + 256]] + [f32(0)] * max(0, start + 256 - len(t))
        quarters = []
        for q in range(4):
            v = tile[64 * q:64 * q + 64]
            for d in (32, 16, 8, 4, 2, 1):
                v = [f32(v[i] + v[i ^ d]) for i in range(64)]
            quarters.append(v[0])
        total = f32(total + f32(f32(f32(quarters[0] + quarters[1]) + quarters[2]) + quarters[3]))
    return total


def contract(graph, pins, K):
    """``pins``: {node: class}.  Returns a dict: ``graph`` (the contracted (n', rowptr, col, weight or None)), ``node_map``
    [n] int32, ``fixed_cut`` float32, ``pinned`` [n] bool."""
    n, rowptr, col, weight = graph
    cls = np.full(n, -1, np.int64)
    for u, c in pins.items():
        assert 0 <= u < n and 0 <= c < K
        cls[u] = c
    free = cls < 0
    if set(cls[~free].tolist()) != set(range(K)):
        raise BadPins("a class without a pinned node")
    if not free.any():
        raise BadPins("no free node")
    rank = np.cumsum(free) - 1
    node_map = np.where(free, K + rank, cls).astype(np.int32)
    entries = {}          # (row', col') -> weight
    t = np.zeros(n, f32)
    for u in range(n):
        sums, touched = [f32(0)] * K, [False] * K
        for e in range(rowptr[u], rowptr[u + 1]):
            x = int(col[e])
            w = f32(1) if weight is None else f32(weight[e])
            if free[u] and free[x]:
                entries[(int(node_map[u]), int(node_map[x]))] = w
            elif free[u]:
                sums[cls[x]] = f32(sums[cls[x]] + w)
                touched[cls[x]] = True
            elif not free[x] and x > u and cls[x] != cls[u]:
                t[u] = f32(t[u] + w)
        for c in range(K):
            if touched[c]:
                entries[(int(node_map[u]), c)] = sums[c]
                entries[(c, int(node_map[u]))] = sums[c]
    n_out = K + int(free.sum())
    keys = sorted(entries)
    if {r for r, _c in keys} != set(range(n_out)):
        raise BadPins("a node without neighbours in the contracted graph")
    out_rowptr = np.zeros(n_out + 1, np.int32)
    for r, _c in keys:
        out_rowptr[r + 1] += 1
    out_rowptr = np.cumsum(out_rowptr).astype(np.int32)
    out_col = np.asarray([c for _r, c in keys], np.int32)
    out_w = np.asarray([entries[k] for k in keys], f32)
    return dict(graph=(n_out, out_rowptr, out_col, None if bool(np.all(out_w == 1.0)) else out_w), node_map=node_map,
                fixed_cut=fold(t), pinned=~free)


def cut_of(graph, partitions):
    """The cut (float64) of every row of ``partitions`` [m, n] on ``graph``: every undirected edge once."""
    n, rowptr, col, weight = graph
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    w = np.ones(col.size) if weight is None else weight.astype(np.float64)
    partitions = np.atleast_2d(partitions)
    return ((partitions[:, rows] != partitions[:, col]) * w).sum(axis=1) / 2


def assignments(n, pins, K):
    """Every partition [m, n] of n nodes into K classes that honours ``pins``."""
    free = [u for u in range(n) if u not in pins]
    out = np.zeros((K ** len(free), n), np.int64)
    for u, c in pins.items():
        out[:, u] = c
    for i, combo in enumerate(itertools.product(range(K), repeat=len(free))):
        out[i, free] = combo
    return out


def drawn_graph(n, chords, seed, weights="unit"):
    """A ring of n nodes with ``chords`` random chords; weights: unit, integer (1..4), signed (-3..3 without 0) or real."""
    rng = np.random.RandomState(seed)
    edges = {(i, (i + 1) % n) if i < (i + 1) % n else ((i + 1) % n, i) for i in range(n)}
    while len(edges) < n + chords and len(edges) < n * (n - 1) // 2:
        u, v = sorted(rng.randint(0, n, 2).tolist())
        if u != v:
            edges.add((u, v))
    return from_edges(n, sorted(edges), seed, weights)


def from_edges(n, edges, seed, weights="unit"):
    rng = np.random.RandomState(seed + 1000)
    if weights == "unit":
        w = np.ones(len(edges), f32)
    elif weights == "integer":
        w = rng.randint(1, 5, len(edges)).astype(f32)
    elif weights == "signed":
        w = rng.choice([-3, -2, -1, 1, 2, 3], len(edges)).astype(f32)
    else:
        w = rng.uniform(0.25, 2.0, len(edges)).astype(f32)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    loops = e[:, 0] == e[:, 1]
    rows = np.concatenate([e[:, 0], e[~loops, 1]])
    cols = np.concatenate([e[:, 1], e[~loops, 0]])
    ww = np.concatenate([w, w[~loops]])
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return n, rowptr, cols[order].astype(np.int32), (None if weights == "unit" else ww[order])


def usable(graph, pins, K):
    """Do the pins give every class a pinned node with a free neighbour, and leave a free node?"""
    n, rowptr, col, _w = graph
    if len(pins) >= n:
        return False
    ok = [False] * K
    for u, c in pins.items():
        ok[c] = ok[c] or any(int(x) not in pins for x in col[rowptr[u]:rowptr[u + 1]])
    return all(ok)


def drawn_pins(graph, K, count, seed):
    """``count`` pins (at least one per class) on random nodes of the graph, redrawn until they are usable."""
    n, rowptr, col, _w = graph
    if count == n - 1:   # all but one: the free node is the one with most neighbours, which carry every class
        free = int(np.argmax(np.diff(rowptr)))
        around = [int(x) for x in col[rowptr[free]:rowptr[free + 1]] if x != free]
        assert len(around) >= K, "no node with K neighbours"
        classes = np.random.RandomState(seed).randint(0, K, n)
        classes[around] = np.arange(len(around)) % K
        return {u: int(classes[u]) for u in range(n) if u != free}
    for attempt in range(1000):
        rng = np.random.RandomState(seed * 1000 + attempt)
        nodes = rng.permutation(n)[:count]
        classes = np.concatenate([np.arange(K), rng.randint(0, K, count - K)])
        pins = {int(u): int(c) for u, c in zip(nodes, classes)}
        if usable(graph, pins, K):
            return pins
    raise AssertionError("no usable pins drawn")
