"""The argument handling of the six fused entry points, pinned against a recording (CPU only).

``tests/golden/api_status.json`` holds what the library returned BEFORE the entry points were moved onto one call
record and one preamble (tests/golden/make_golden_api_status.py wrote it with the library of that commit):

* status: the code of every entry point for a grid of calls with exactly ONE thing wrong (plus the empty batch of the
  two forwards, which returns GMC_OK without a launch).  Pointers are fake non-NULL addresses: no call reaches a launch.
* workspace: gmc_workspace_bytes / gmc_workspace_bytes_features over forward / training x dropout x loss flag x
  fused on / off x shapes that take each plan.  The slice-group count depends on the device's CU count (256 without a
  device): the batch sizes give the same count for 256..304 CUs (the generator checks that), as PER_CASES of
  tests/test_lds_flavours.py do.

The grid lives here (`status_grid`, `workspace_grid`); the generator imports it, so the two cannot drift apart.
"""
import ctypes as C
import json
import math
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_status.json")
SOME, ODD = 4096, 4100          # fake device addresses: 16-byte aligned / not (never dereferenced)
N, F, BIG = 1000, 32, 1 << 40
ENTRIES = ("gmc_forward", "gmc_train_fwd_bwd", "gmc_train_step_loss_f32", "gmc_backward_from_gp",
           "gmc_forward_features", "gmc_backward_features_from_gp")
DENSE = ("gmc_forward_features", "gmc_backward_features_from_gp")
BATCH_PTRS = ("goff", "rowptr", "gcol", "lcol", "dinv")


def batch_fields(n=60, B=2, W=8, slots=7, ovf_blocks=0, table=True):
    """Fields of a host-filled gmc_batch of B graphs of n nodes (as tests/test_lds_flavours.py builds them)."""
    kw = dict(B=B, R=n * B, nnz=n * B, n_max=n, uniform_n=0, nnz_max=n, goff=SOME, rowptr=SOME, gcol=SOME, lcol=SOME,
              dinv=SOME, ell_width=W, ell_slots=slots)
    if table:
        kw.update(ell=SOME)
    if ovf_blocks:
        kw.update(ovf_ptr=SOME, ovf_ids=SOME, ovf_max_blocks=ovf_blocks)
    return kw


def model_fields(**kw):
    return {**dict(N=N, F=F, K=3, flags=1, W1=SOME, b1=SOME, W2=SOME, b2=SOME), **kw}   # flags: GMC_MODEL_GRAD_TAIL


def call(hip, entry, batch=None, model=None, nbytes=BIG, **a):
    """One call of ``entry``.  ``batch`` / ``model``: field dicts, or None for a NULL struct pointer; ``a`` overrides the
    other arguments (None = NULL).  gmc_train_step_loss_f32 has no model struct: it takes N, F and W1_slab of ``model``
    and its parameter pointer from ``a``."""
    lib = hip.load()
    b = None if batch is None else C.byref(hip.GmcBatch(**batch))
    m = None if model is None else C.byref(hip.GmcModel(**model))
    g = {**dict(ws=SOME, P=SOME, S=None, loss=SOME, grad=SOME, GP=SOME, X=SOME, ldx=N, dX=None, lddx=0, param=SOME,
                mom=SOME, var=SOME, counter=SOME, kind=0), **a}
    if entry == "gmc_forward":
        return lib.gmc_forward(b, m, 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], None)
    if entry == "gmc_train_fwd_bwd":
        return lib.gmc_train_fwd_bwd(b, m, 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], g["grad"], None)
    if entry == "gmc_train_step_loss_f32":
        return lib.gmc_train_step_loss_f32(b, model["N"], model["F"], g["param"], 1.0, g["kind"], g["ws"], nbytes, g["P"],
                                           g["S"], g["loss"], g["grad"], g["mom"], g["var"], 1e-3, 0.9, 0.999, 1e-8,
                                           g["counter"], model.get("W1_slab"), None)
    if entry == "gmc_backward_from_gp":
        return lib.gmc_backward_from_gp(b, m, g["ws"], nbytes, g["P"], g["GP"], g["grad"], None)
    if entry == "gmc_forward_features":
        return lib.gmc_forward_features(b, m, g["X"], g["ldx"], 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], None)
    return lib.gmc_backward_features_from_gp(b, m, g["X"], g["ldx"], g["ws"], nbytes, g["P"], g["GP"], g["grad"],
                                             g["dX"], g["lddx"], None)


def status_grid(hip):
    """[(name, thunk)]: every case has exactly one thing wrong, or is an empty batch that launches nothing."""
    lib = hip.load()
    cases = []
    for entry in ENTRIES:
        step, dense = entry == "gmc_train_step_loss_f32", entry in DENSE
        training, backward = entry != "gmc_forward" and entry != "gmc_forward_features", "backward" in entry

        def add(name, entry=entry, **kw):
            kw.setdefault("batch", batch_fields())
            kw.setdefault("model", model_fields())
            cases.append((f"{entry}:{name}", lambda: call(hip, entry, **kw)))

        def bat(**kw):
            return {**batch_fields(), **kw}

        # -- the batch struct
        add("batch=NULL", batch=None)
        add("batch.abi", batch=bat(abi=100))
        for f in BATCH_PTRS:
            add(f"batch.{f}=NULL", batch=bat(**{f: None}))
        for f in ("B", "R", "nnz"):
            add(f"batch.{f}=-1", batch=bat(**{f: -1}))
        add("batch.n_max=2", batch=bat(n_max=2))
        add("batch.n_max=4097", batch=bat(n_max=4097))
        if not dense:   # (with features of their own a graph may have more nodes than conv1.weight has rows)
            add("batch.n_max>N", model=model_fields(N=48))
        # -- the model: a struct, or N / F / param / w1_slab of the step
        for n in (0, -1):
            add(f"model.N={n}", model=model_fields(N=n))
        for f in (0, -4, 30, 4100):
            add(f"model.F={f}", model=model_fields(F=f))
        add("model.W1_slab odd", model=model_fields(W1_slab=ODD))
        if step:
            for kind in (2, -1):
                add(f"loss_kind={kind}", kind=kind)
            for p in ("param", "mom", "var", "counter"):
                add(f"{p}=NULL", **{p: None})
            for p in ("param", "mom", "var"):
                add(f"{p} odd", **{p: ODD})
        else:
            add("model=NULL", model=None)
            add("model.abi", model=model_fields(abi=100))
            for f in ("W1", "b1", "W2", "b2"):
                add(f"model.{f}=NULL", model=model_fields(**{f: None}))
            add("model.K=2", model=model_fields(K=2))
            for p in (-0.25, 1.0, math.nan):
                add(f"model.dropout_p={p}", model=model_fields(dropout_p=p))
        # -- the features
        if dense:
            add("X=NULL", X=None)
            add("X odd", X=ODD)
            add("ldx<N", ldx=N - 4)
            add("ldx%4", ldx=N + 2)
            add("model.W1 odd", model=model_fields(W1=ODD))
        # -- workspace and outputs
        add("workspace=NULL", ws=None)
        add("P=NULL", P=None)
        if backward:
            add("GP=NULL", GP=None)
        if training:
            add("grad=NULL", grad=None)
            add("grad odd", grad=ODD)
        if entry == "gmc_train_fwd_bwd":
            add("loss=NULL with GMC_MODEL_GRAD_TAIL", loss=None)
        if entry == "gmc_backward_features_from_gp":
            add("dX odd", dX=ODD, lddx=N)
            add("lddx<N", dX=SOME, lddx=N - 4)
            add("lddx%4", dX=SOME, lddx=N + 2)
        # -- the workspace one byte short: the fused LDS plan, the row kernels (no table), and with dropout
        for tag, bf, mf in (("lds", batch_fields(), model_fields()),
                            ("rows", batch_fields(table=False, B=6), model_fields()),
                            ("dropout", batch_fields(), model_fields(dropout_p=0.0 if step else 0.5))):
            size = lib.gmc_workspace_bytes_features if dense else lib.gmc_workspace_bytes
            need = size(C.byref(hip.GmcBatch(**bf)), C.byref(hip.GmcModel(**mf)), int(training))
            assert need > 256
            add(f"workspace one byte short ({tag})", batch=bf, model=mf, nbytes=need - 1)
        if not training:   # the forwards return before any launch (the training calls zero the gradient: GPU tests)
            add("empty batch", batch=bat(B=0, R=0, nnz=0, n_max=0))
    return cases


# (name, batch fields, hidden width): one shape per plan
SHAPES = [(f"lds n={n}", batch_fields(n=n), 128) for n in (100, 260, 400, 520, 800)]   # each (FS, ACC) window, W = 8
SHAPES += [(f"lds16 n={n}", batch_fields(n=n, W=16, slots=12), 128) for n in (100, 270, 400, 530, 800)]   # ... W = 16
SHAPES += [
    ("lds narrow", batch_fields(n=100), 20),
    ("lds 2 slices per group", batch_fields(n=600, B=40), 128),
    ("lds 4 slices per group", batch_fields(n=600, B=96), 128),
    ("lds one graph", batch_fields(n=300, B=1), 500),
    ("overflow lists", batch_fields(n=200, slots=8, ovf_blocks=1), 128),
    ("overflow lists that do not fit", batch_fields(n=275, slots=8, ovf_blocks=1), 128),
    ("rows: too large for LDS", batch_fields(n=2000), 128),
    ("rows: too large, many graphs", batch_fields(n=1500, B=40), 64),
    ("rows: no table", batch_fields(n=100, B=6, table=False), 36),
    ("wide", batch_fields(n=100), 4096),
]


def workspace_grid(hip):
    """[(name, thunk)] over both size queries (the dense plan is gmc_workspace_bytes_features')."""
    lib = hip.load()
    cases = []
    for shape, bf, width in SHAPES:
        for query in ("gmc_workspace_bytes", "gmc_workspace_bytes_features"):
            for training in (0, 1):
                for p in (0.0, 0.5):
                    for flags in (0, 1, 2, 3):   # GMC_MODEL_GRAD_TAIL | GMC_MODEL_LOSS_EXPECTED
                        def size(query=query, bf=bf, width=width, training=training, p=p, flags=flags):
                            m = hip.GmcModel(**model_fields(N=4096, F=width, flags=flags, dropout_p=p))
                            return int(getattr(lib, query)(C.byref(hip.GmcBatch(**bf)), C.byref(m), training))
                        cases.append((f"{query}:{shape}:F={width}:training={training}:p={p}:flags={flags}", size))
    return cases


def record(hip):
    """What the loaded library answers over both grids; the second workspace pass runs with gmc_set_fuse(0)."""
    lib = hip.load()
    out = {"status": {k: f() for k, f in status_grid(hip)}, "workspace": {k: f() for k, f in workspace_grid(hip)}}
    prev = lib.gmc_set_fuse(0)
    try:
        out["workspace_unfused"] = {k: f() for k, f in workspace_grid(hip)}
    finally:
        lib.gmc_set_fuse(prev)
    return out


@pytest.fixture(scope="module")
def recorded(built):
    return record(built.hip)


@pytest.mark.parametrize("section", ("status", "workspace", "workspace_unfused"))
def test_entry_points_answer_as_recorded(recorded, section):
    want = json.load(open(GOLDEN))[section]
    got = recorded[section]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_grid_covers_every_entry_point_and_every_code(recorded):
    """The recording is not vacuous: every entry point, every status code the preamble can give, every plan."""
    status = recorded["status"]
    assert {k.split(":")[0] for k in status} == set(ENTRIES)
    assert set(status.values()) == {0, -1, -2, -3, -4, -5, -6, -7, -8, -9}
    assert all(v < 0 or k.endswith(":empty batch") for k, v in status.items())    # nothing reached a launch
    sizes = recorded["workspace"]
    assert len(set(sizes.values())) > len(SHAPES) and min(sizes.values()) > 0
