#!/usr/bin/env python3
"""Generates tests/golden/api_status.json: what the fused entry points return over the grids of
tests/test_api_status.py (status codes of calls with one thing wrong, workspace sizes per plan).

Run it on the CPU with the library of the commit whose behaviour is to be kept, NEVER with the code under test:

    GCN_MAXCUT_LIB=/path/to/that/libgcnmaxcut_hip.so python tests/golden/make_golden_api_status.py

Only recorded results are written.  Before writing it checks that no call of the status grid got as far as a launch
(without a device a launch fails with a positive HIP error) and that every LDS shape of the workspace grid has the same
number of slice groups for 256..304 compute units, so the recording holds on a machine with a GPU.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
import gcn_max_cut_amd as pkg  # noqa: E402
from tests import test_api_status as A  # noqa: E402


def check_cu_independent(hip):
    """gmc_lds_slices_per_group halves 4 -> 2 -> 1 while B * ceil(slices / per) < CUs / 2: no product may lie in
    [256 / 2, 304 / 2)."""
    for shape, bf, width in A.SHAPES:
        words = hip.lds_flavours(hip.GmcBatch(**bf), width)
        if not words:
            continue   # row kernels: no slice groups
        slices = -(-width // hip.flavour_fields(words[0])["FS"])
        for per in (4, 2):
            items = bf["B"] * -(-slices // per)
            assert not 128 <= items < 152, (shape, per, items)


def main():
    hip = pkg.hip
    if not os.environ.get("GCN_MAXCUT_LIB"):
        sys.exit("set GCN_MAXCUT_LIB to the library of the commit to record (not the code under test)")
    check_cu_independent(hip)
    out = A.record(hip)
    bad = {k: v for k, v in out["status"].items() if v > 0 or (v == 0 and not k.endswith(":empty batch"))}
    assert not bad, f"calls that reached a launch: {bad}"
    for cus in (256, 304):   # the test hook re-splits items only; the sizes must not move with it either
        prev = hip.load().gmc_debug_set_device_cus(cus)
        again = {k: f() for k, f in A.workspace_grid(hip)}
        hip.load().gmc_debug_set_device_cus(prev)
        assert again == out["workspace"], cus
    out["library"] = "libgcnmaxcut_hip.so of the commit before the entry points moved onto one preamble"
    with open(A.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{A.GOLDEN}: {len(out['status'])} status cases, {2 * len(out['workspace'])} workspace sizes")


if __name__ == "__main__":
    main()
