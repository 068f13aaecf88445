"""Census of the LDS-tiled kernel flavours (CPU only).

The hot path is a family of template instantiations per kernel (fwd1_lds, bwd1_lds / bwd1_reg, spmm_lds, dw1_lds), and
the host picks one per batch from n_max, the table width W, the live slots, edge weights, overflow lists and - for a
one-graph gmc_train_step_f32 - whether the head runs inside the backward.  This module pins that choice:

- what is instantiated: the kernel symbols of the gfx950 code objects inside the built library;
- what is reachable: gmc_lds_flavours (the host-only query whose words the launchers dispatch on) over every n_max in
  1..2100, both table widths, every ell_slots value, weights on / off, overflow lists with small and boundary block
  counts, one-graph steps on / off, several hidden widths;
- reachable <= instantiated, instantiated - reachable == DEAD (each with its reason), reachable == the words of the GPU
  matrix (MATRIX, run by tests/test_gpu_flavours.py);
- BOUNDARIES: the n_max windows of every (FS, ACC) class per batch kind, as literal numbers, and an independent Python
  statement of which words each kind selects inside a window.  A change of pick_fs or of the dispatch has to edit
  these tables.
"""
import ctypes as C
import re

import pytest

from tests import util

PER_MASK = 3 << 29
KERNEL_IDS = {"fwd1_lds": 1, "bwd1_lds": 2, "bwd1_reg": 3, "spmm_lds": 4, "dw1_lds": 5}


def word(kernel, FS, W, ACC, NS, val=0, ovf=0, head=0, epi=0, shared=0, per=1):
    """A flavour word (include/gcnmaxcut.h, GMC_FLV_*)."""
    return (KERNEL_IDS[kernel] | FS << 3 | W << 10 | ACC << 15 | NS << 19 | val << 24 | ovf << 25 | head << 26 |
            epi << 27 | shared << 28 | {1: 0, 2: 1, 4: 2, 8: 3}[per] << 29)


def name(w):
    f = {"FS": w >> 3 & 0x7f, "W": w >> 10 & 0x1f, "ACC": w >> 15 & 0xf, "NS": w >> 19 & 0x1f}
    kid = {v: k for k, v in KERNEL_IDS.items()}.get(w & 7, "?")
    flags = [t for t, b in (("VAL", 24), ("OVF", 25), ("HEAD", 26), ("EPI", 27), ("SHARED", 28)) if w >> b & 1]
    per = 1 << (w >> 29 & 3)
    return f"{kid}<FS{f['FS']} W{f['W']} ACC{f['ACC']} NS{f['NS']}{''.join(' ' + t for t in flags)}>" + \
        (f" x{per}" if per > 1 else "")


# ---- batch kinds: what the GPU matrix builds, and the gmc_batch fields that make the library pick their flavours
# kind: (W, ell_slots, weights, overflow, one-graph train_step, degree of the regular graphs, smallest n_max)
KINDS = {
    "w8_ns7": (8, 7, False, False, False, 7, 8),
    "w8_ns8": (8, 8, False, False, False, 8, 9),
    "w8_val": (8, 7, True, False, False, 7, 8),       # integer weights 1..3
    "w8_ovf": (8, 8, False, True, False, 7, 101),     # one hub row of degree 12 (one overflow block); a table of 8
                                                      # slots allows one long row per 200 rows: R >= 200
    "w16_ns10": (16, 10, False, False, False, 10, 11),
    "w16_ns12": (16, 12, False, False, False, 12, 13),
    "w16_ns14": (16, 14, False, False, False, 14, 15),
    "w16_ns16": (16, 16, False, False, False, 16, 17),
    "w16_val": (16, 12, True, False, False, 12, 13),
    "w16_ovf": (16, 16, False, True, False, 12, 21),  # one hub row of degree 20
    "head_ns7": (8, 7, False, False, True, 7, 8),     # ONE graph per step: the head inside the backward
    "head_ns8": (8, 8, False, False, True, 8, 9),
}

# ---- boundary table: per kind, the (FS, ACC) windows of n_max in which the kind selects its flavours (n_max < 3 is
# refused before any kernel; past the last window the batch takes the row kernels).  Head kinds: only the windows in
# which the head rides in the backward (between them, ACC = 8: the plain one-graph backward of the w8 kinds).
_W8 = [(64, 4, 3, 256), (64, 8, 257, 275), (32, 4, 276, 512), (32, 8, 513, 538), (16, 4, 539, 1020)]
_W16 = [(64, 4, 3, 256), (64, 8, 257, 282), (32, 4, 283, 512), (32, 8, 513, 551), (16, 4, 552, 1008)]
BOUNDARIES = {
    "w8_ns7": _W8, "w8_ns8": _W8, "w8_val": _W8,
    # overflow lists: the descriptors and blocks have to fit behind the kernels' own LDS (ovf_fits)
    "w8_ovf": [(64, 4, 3, 256), (64, 8, 257, 274), (32, 4, 276, 512), (32, 8, 513, 534), (16, 4, 539, 1006)],
    "w16_ns10": _W16, "w16_ns12": _W16, "w16_ns14": _W16, "w16_ns16": _W16, "w16_val": _W16,
    "w16_ovf": [(64, 4, 3, 256), (64, 8, 257, 282), (32, 4, 283, 512), (32, 8, 513, 551), (16, 4, 552, 1004)],
    "head_ns7": [(64, 4, 3, 256), (32, 4, 276, 512), (16, 4, 539, 1020)],
    "head_ns8": [(64, 4, 3, 256), (32, 4, 276, 512), (16, 4, 539, 1020)],
}
# slices per workgroup item (GMC_FLV_PER) of the fused forward / the SpMM: 4 when that still gives half a workgroup
# per CU, else 2, else 1 - a function of B, the slice count and the device's CU count (256 without a device), not of
# n_max alone; pinned by PER_CASES below with batch sizes that give the same class for 256..304 CUs.


def expected_words(kind, FS, ACC, per=1):
    """The flavour words a training step of a batch of this kind makes inside an (FS, ACC) window: fused sequence,
    then (no overflow lists) the gmc_set_fuse(0) sequence - W1 gather, aggregation + W2 epilogue, backward
    aggregation, dW1.  Stated here independently of the library's dispatch."""
    W, slots, val, ovf, one, _d, _n = KINDS[kind]
    v, o = int(val), int(ovf)
    ns = W if (val or ovf) else slots
    bwd = "bwd1_reg" if W == 8 else "bwd1_lds"
    head = int(one and ACC == 4)
    out = [word("fwd1_lds", FS, W, ACC, ns, v, o, per=per), word(bwd, FS, W, ACC, ns, v, o, head=head)]
    if not ovf:
        agg_ns = slots   # the aggregations never apply the weights: unit-weight gathers over the live slots
        out += [word("spmm_lds", FS, W, ACC, W, v, shared=1, per=per), word("spmm_lds", FS, W, ACC, agg_ns, epi=1, per=per),
                word("spmm_lds", FS, W, ACC, agg_ns, per=per), word("dw1_lds", FS, W, ACC, ns, v)]
    return out


# ---- instantiations that no batch can select (removed from the dispatch: their launch branch returns
# GMC_ERR_UNSUPPORTED and the code object no longer carries them).  Must stay empty unless an entry has a reason.
DEAD = {}

# ---- the GPU matrix (tests/test_gpu_flavours.py): every kind at both ends of each window, plus the slice-group
# classes 2 and 4.  (kind, n_max, hidden, graphs): hidden < FS or not a multiple of FS at every slice width, 500 once
# per FS; `graphs` = 2 (the n_max graph and a smaller one) or 1 (head kinds).
_HIDDEN = {(64, "lo"): 20, (64, "hi"): 100, (32, "lo"): 20, (32, "hi"): 72, (16, "lo"): 12, (16, "hi"): 52}


def _matrix():
    rows = []
    for kind, wins in BOUNDARIES.items():
        graphs = 1 if KINDS[kind][4] else 2
        for FS, ACC, lo, hi in wins:
            for end, n in (("lo", max(lo, KINDS[kind][6])), ("hi", hi)):
                hidden = _HIDDEN[(FS, end)]
                if kind == "w8_ns7" and end == "hi" and (FS, ACC) in ((64, 8), (32, 8), (16, 4)):
                    hidden = 500
                rows.append((kind, n, hidden, graphs))
    return rows


MATRIX = _matrix()
# slice-group classes beyond 1 (two-graph batches never reach them): one n = 600 graph plus small ones, hidden 128
# (8 slices of 16 columns): 40 graphs -> 2 slices per item, 96 graphs -> 4
PER_CASES = [("w8_ns7", 600, 128, 40, 2), ("w8_ns7", 600, 128, 96, 4)]


# ---- helpers
def batch_struct(hip, W, slots, val, ovf_blocks, n, B):
    """A host-filled gmc_batch: dummy non-NULL pointers (the query only tests them against NULL)."""
    some = 4096
    return hip.GmcBatch(B=B, R=n * B, nnz=n * B, n_max=n, uniform_n=0, nnz_max=n, goff=some, rowptr=some, gcol=some,
                        lcol=some, vals=some if val else None, dinv=some, ell=some, ell_vals=some if val else None,
                        ell_width=W, ell_slots=slots, ovf_ptr=some if ovf_blocks else None,
                        ovf_ids=some if ovf_blocks else None, ovf_max_blocks=ovf_blocks)


def kind_struct(hip, kind, n, B=None):
    W, slots, val, ovf, one, _d, _n = KINDS[kind]
    return batch_struct(hip, W, slots, val, 1 if ovf else 0, n, B or (1 if one else 2))


def instantiated_flavours(lib_path):
    """Template arguments of every LDS-tiled kernel in the library's gfx950 code objects, as flavour words (GMC_FLV_PER
    clear)."""
    words = set()
    for line in sorted(util.kernel_symbols(lib_path)):
        m = re.search(r"\b(fwd1_lds|bwd1_lds|bwd1_reg|spmm_lds|dw1_lds)_kernel<([^>]*)>", line)
        if not m:
            continue
        a = [1 if t == "true" else 0 if t == "false" else int(t) for t in (x.strip() for x in m.group(2).split(","))]
        k = m.group(1)
        if k in ("fwd1_lds", "bwd1_lds"):            # <FS, W, ACC, HAS_VAL, NS, OVF>
            words.add(word(k, a[0], a[1], a[2], a[4], a[3], a[5]))
        elif k == "bwd1_reg":                        # <FS, ACC, HAS_VAL, NS, OVF, HEAD>
            words.add(word(k, a[0], 8, a[1], a[3], a[2], a[4], head=a[5]))
        elif k == "spmm_lds":                        # <FS, W, ACC, EPI, HAS_VAL, SHARED, NS>
            words.add(word(k, a[0], a[1], a[2], a[6], a[4], epi=a[3], shared=a[5]))
        else:                                        # dw1_lds <FS, W, ACC, HAS_VAL, NS>
            words.add(word(k, a[0], a[1], a[2], a[4], a[3]))
    return words


def reachable_flavours(hip):
    """Union of the query's words over the sweep (GMC_FLV_PER clear), and every word's n_max range."""
    seen = {}
    for W in (8, 16):
        combos = [(s, False, 0) for s in range(0, W + 1)]                       # every ell_slots value, unit weights
        combos += [(s, True, 0) for s in (0, W - 1, W)]                         # edge weights
        combos += [(W, val, b) for val in (False, True) for b in (1, 64, 4095, 4096)]   # overflow lists
        for slots, val, blocks in combos:
            for one, B in ((False, 2), (True, 1), (True, 2)):
                for F in (4, 20, 100, 1024):
                    for n in range(1, 2101):
                        for w in hip.lds_flavours(batch_struct(hip, W, slots, val, blocks, n, B), F, one):
                            assert w > 0, (W, slots, val, blocks, one, B, F, n)
                            lo, hi = seen.get(w & ~PER_MASK, (n, n))
                            seen[w & ~PER_MASK] = (min(lo, n), max(hi, n))
    return seen


@pytest.fixture(scope="module")
def hip(built):
    built.hip.load()
    return built.hip


@pytest.fixture(scope="module")
def reachable(hip):
    return reachable_flavours(hip)


def matrix_words():
    words = set()
    for kind, n, hidden, graphs in MATRIX:
        FS, ACC = next((fs, acc) for fs, acc, lo, hi in BOUNDARIES[kind] if lo <= n <= hi)
        words |= {w & ~PER_MASK for w in expected_words(kind, FS, ACC)}
    return words


# ---- tests
def test_reachable_flavours_are_instantiated_and_the_rest_is_listed_dead(hip, reachable):
    inst = instantiated_flavours(hip.LIB_PATH)
    reach = set(reachable)
    missing = reach - inst
    assert not missing, sorted(name(w) for w in missing)
    unexplained = {name(w) for w in inst - reach} ^ set(DEAD)
    assert not unexplained, sorted(unexplained)
    assert all(DEAD.values())
    # per family (reported in the pull request that introduced this census)
    count = {k: sum(1 for w in reach if w & 7 == v) for k, v in KERNEL_IDS.items()}
    assert count == {"fwd1_lds": 50, "bwd1_lds": 30, "bwd1_reg": 26, "spmm_lds": 80, "dw1_lds": 40}, count


def test_no_sixteen_column_flavour_runs_eight_rows_per_thread(reachable):
    """A 16-column tile stops fitting the 160 KiB of LDS at n_max = 1021 (8-slot table) / 1009 (16 slots), before
    ACC = 8 could start at 1025: those instantiations were dead weight of the code object and are gone."""
    assert not [name(w) for w in reachable if w >> 3 & 0x7f == 16 and w >> 15 & 0xf == 8]
    assert max(hi for w, (lo, hi) in reachable.items() if w >> 3 & 0x7f == 16) == 1020


def test_gpu_matrix_covers_exactly_the_reachable_flavours(reachable):
    got = matrix_words()
    assert got == set(reachable), (sorted(name(w) for w in set(reachable) - got), sorted(name(w) for w in got - set(reachable)))


def test_matrix_cases_sit_at_both_ends_of_every_window(reachable):
    """Each reachable word's highest n_max is a matrix case; its lowest is one too, or the smallest graph its kind can
    be built as (KINDS)."""
    by_word = {}
    for kind, n, hidden, graphs in MATRIX:
        FS, ACC = next((fs, acc) for fs, acc, lo, hi in BOUNDARIES[kind] if lo <= n <= hi)
        for w in expected_words(kind, FS, ACC):
            by_word.setdefault(w & ~PER_MASK, set()).add((kind, n))
    for w, (lo, hi) in reachable.items():
        ns = {n for _k, n in by_word[w]}
        assert max(ns) == hi, (name(w), hi, sorted(ns))
        assert min(ns) == max(lo, 3) or all(min(ns) == KINDS[k][6] for k, n in by_word[w] if n == min(ns)), \
            (name(w), lo, sorted(ns))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_boundary_table(hip, kind):
    """For every n_max in 1..2100 the query gives exactly the kind's words of the window n_max lies in (head kinds
    outside their windows: the plain one-graph backward below n = 1021), nothing outside the windows."""
    wins = BOUNDARIES[kind]
    one = KINDS[kind][4]
    for n in range(1, 2101):
        got = hip.lds_flavours(kind_struct(hip, kind, n), 128, one)
        win = next(((fs, acc) for fs, acc, lo, hi in wins if lo <= n <= hi), None)
        if win is not None:
            assert got == expected_words(kind, *win), (kind, n, [name(w) for w in got])
        elif n < 3:   # (refused by every entry point before the query matters)
            assert got == expected_words(kind, 64, 4), (kind, n, [name(w) for w in got])
        elif one and n <= 1020:   # ACC = 8 between the head windows: the backward runs without the head
            plain = "w8_ns7" if KINDS[kind][1] == 7 else "w8_ns8"
            fs, acc = next((fs, acc) for fs, acc, lo, hi in BOUNDARIES[plain] if lo <= n <= hi)
            assert acc == 8 and got == expected_words(plain, fs, acc), (kind, n, [name(w) for w in got])
        else:   # past the last window, or (overflow lists) between windows: the lists do not fit - row kernels
            assert got == [] and (n > 1000 or KINDS[kind][3]), (kind, n, [name(w) for w in got])


def test_slice_group_classes(hip):
    """Two graphs never group slices; PER_CASES reach 2 and 4 (the fused forward and the three SpMMs carry the class)."""
    for n in (3, 256, 257, 538, 539, 1020):
        for F in (4, 128, 1024):
            assert all(w >> 29 == 0 for w in hip.lds_flavours(batch_struct(hip, 8, 7, False, 0, n, 2), F, False)), (n, F)
    for kind, n, hidden, B, per in PER_CASES:
        got = hip.lds_flavours(kind_struct(hip, kind, n, B), hidden, False)
        assert [1 << (w >> 29 & 3) for w in got] == [per, 1, per, per, per, 1], [name(w) for w in got]


def test_query_arguments(hip):
    lib = hip.load()
    b = batch_struct(hip, 8, 7, False, 0, 100, 2)
    words = (C.c_int32 * 2)()
    assert lib.gmc_lds_flavours(C.byref(b), 128, 0, words, 2) == 6           # count of all, writes the first two
    assert list(words) == hip.lds_flavours(b, 128)[:2]
    assert lib.gmc_lds_flavours(None, 128, 0, words, 2) == -1                # GMC_ERR_NULL
    assert lib.gmc_lds_flavours(C.byref(b), 130, 0, words, 2) == -2          # F % 4
    b.ell = None                                                              # no table: row kernels
    assert hip.lds_flavours(b, 128) == []
    b.abi = 199
    assert lib.gmc_lds_flavours(C.byref(b), 128, 0, words, 2) == -8          # GMC_ERR_ABI
