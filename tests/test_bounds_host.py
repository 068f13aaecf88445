"""The ledger of the bounds tests: every name include/gcnmaxcut.h exports is in exactly one of three sets -

  COVERED           called by a guard-band test (tests/test_gpu_bounds_*.py), named here;
  BANDED_ELSEWHERE  a building block whose own test already runs it between bands, named here;
  EXEMPT            takes no device pointer, with the reason.

so an entry point added to the header fails this test until someone decides where its memory is checked.  An EXEMPT
function may only have pointer parameters that are host memory: the two host structs (gmc_batch / gmc_model: only their
scalars are read by such a function), any pointer of a function whose name says `_host`, or a parameter listed in
HOST_POINTERS with the words of the header's comment that say so (the words must be there).  CPU only.
"""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gcnmaxcut.h")

TRAIN, DECODE, BLOCKS = "test_gpu_bounds_train", "test_gpu_bounds_decode", "test_gpu_bounds_blocks"

COVERED = {
    # forward and training
    "gmc_forward": (TRAIN, "test_forward_and_train_fwd_bwd"),
    "gmc_train_fwd_bwd": (TRAIN, "test_forward_and_train_fwd_bwd"),
    "gmc_train_step_f32": (TRAIN, "test_train_step"),
    "gmc_train_step_loss_f32": (TRAIN, "test_train_step"),
    "gmc_backward_from_gp": (TRAIN, "test_backward_from_gp_and_the_features_trio"),
    "gmc_forward_features": (TRAIN, "test_forward_features_with_the_forward_workspace"),
    "gmc_backward_features_from_gp": (TRAIN, "test_backward_from_gp_and_the_features_trio"),
    "gmc_kway_forward": (TRAIN, "test_kway_and_large"),
    "gmc_kway_train_fwd_bwd": (TRAIN, "test_kway_and_large"),
    "gmc_large_forward": (TRAIN, "test_kway_and_large"),
    "gmc_large_train_fwd_bwd": (TRAIN, "test_kway_and_large"),
    "gmc_fn_forward": (TRAIN, "test_functional_forward_backward"),
    "gmc_fn_backward": (TRAIN, "test_functional_forward_backward"),
    "gmc_fn_cut_loss_f32": (TRAIN, "test_fn_cut_loss"),
    "gmc_inst_forward": (TRAIN, "test_instance_models"),
    "gmc_inst_train_fwd_bwd": (TRAIN, "test_instance_models"),
    "gmc_inst_forward_t": (TRAIN, "test_instance_models"),
    "gmc_inst_train_fwd_bwd_t": (TRAIN, "test_instance_models"),
    "gmc_inst_forward_c": (TRAIN, "test_instance_models"),
    "gmc_inst_train_fwd_bwd_c": (TRAIN, "test_instance_models"),
    "gmc_inst_keep_best_f32": (TRAIN, "test_instance_state"),
    "gmc_inst_early_stop_f32": (TRAIN, "test_instance_state"),
    "gmc_inst_adam_f32": (TRAIN, "test_instance_state"),
    "gmc_inst_large_forward": (TRAIN, "test_large_instance_models"),
    "gmc_inst_large_train_fwd_bwd": (TRAIN, "test_large_instance_models"),
    "gmc_att_forward": (TRAIN, "test_attention"),
    "gmc_att_train_fwd_bwd": (TRAIN, "test_attention"),
    # stand-alone heads and products
    "gmc_head_f32": (BLOCKS, "test_heads"),
    "gmc_head_loss_f32": (BLOCKS, "test_heads"),
    "gmc_cut_loss_f32": (BLOCKS, "test_cut_loss"),
    "gmc_dense_hw2_f32": (BLOCKS, "test_dense_hw2"),
    "gmc_row_weight_sums_f32": (BLOCKS, "test_row_weight_sums"),
    # builders
    "gmc_batch_build_csr": (BLOCKS, "test_batch_build"),
    "gmc_batch_build_table": (BLOCKS, "test_batch_build"),
    "gmc_contract_map": (BLOCKS, "test_contract"),
    "gmc_contract_entries": (BLOCKS, "test_contract"),
    # one-workgroup decoders
    "gmc_decode_sample_f32": (DECODE, "test_samplers"),
    "gmc_decode_sample_seeded_f32": (DECODE, "test_samplers"),
    "gmc_refine_local_f32": (DECODE, "test_refine_and_anneal"),
    "gmc_refine_anneal_f32": (DECODE, "test_refine_and_anneal"),
    "gmc_refine_anneal_staged": (DECODE, "test_refine_and_anneal"),
    "gmc_round_conditional_f32": (DECODE, "test_round_conditional"),
    "gmc_round_conditional_t_f32": (DECODE, "test_round_conditional"),
    "gmc_round_conditional_c_f32": (DECODE, "test_round_conditional"),
    "gmc_kway_decode_sample_seeded_f32": (DECODE, "test_kway_sampler"),
    "gmc_kway_decode_sample_seeded_t_f32": (DECODE, "test_kway_sampler"),
    "gmc_kway_decode_sample_seeded_c_f32": (DECODE, "test_kway_sampler"),
    "gmc_kway_refine_anneal_f32": (DECODE, "test_kway_anneal"),
    "gmc_kway_refine_anneal_t_f32": (DECODE, "test_kway_anneal"),
    "gmc_kway_refine_anneal_c_f32": (DECODE, "test_kway_anneal"),
    "gmc_kway_evolve_f32": (DECODE, "test_evolve"),
    "gmc_kway_tabu_f32": (DECODE, "test_chain_searches"),
    "gmc_kway_tabu_c_f32": (DECODE, "test_chain_searches"),
    "gmc_kway_balance_f32": (DECODE, "test_chain_searches"),
    "gmc_kway_balance_c_f32": (DECODE, "test_chain_searches"),
    # decoders beyond one workgroup
    "gmc_large_round_conditional_f32": (DECODE, "test_large_decoders"),
    "gmc_large_round_conditional_t_f32": (DECODE, "test_large_decoders"),
    "gmc_large_local_search_f32": (DECODE, "test_large_decoders"),
    "gmc_large_local_search_t_f32": (DECODE, "test_large_decoders"),
    "gmc_large_sample_seeded_f32": (DECODE, "test_large_decoders"),
    "gmc_large_sample_seeded_t_f32": (DECODE, "test_large_decoders"),
    "gmc_large_anneal_f32": (DECODE, "test_large_anneal"),
    "gmc_large_anneal_t_f32": (DECODE, "test_large_anneal"),
}

BANDED_ELSEWHERE = {
    "gmc_spmm_f32": ("test_gpu_spmm", "test_against_float64"),
    "gmc_gemm_f32": ("test_gpu_gemm", "test_tile_edges"),
    "gmc_adam_f32": ("test_gpu_adam", "test_counts_both_entry_points"),
    "gmc_adam_devstep_f32": ("test_gpu_adam", "test_counts_both_entry_points"),
    "gmc_adam_devstep_model_f32": ("test_gpu_adam", "test_devstep_model_equals_devstep_and_keeps_the_slab"),
    "gmc_w1_slab_f32": ("test_gpu_adam", "test_w1_slab"),
    # their source is device memory between NaN bands there; the target is mapped host memory
    "gmc_publish_f32": ("test_gpu_adam", "test_publish"),
    "gmc_publish_adam_devstep_model_f32": ("test_gpu_adam", "test_publishing_form_ticks_first_and_equals_the_model_call"),
}

EXEMPT = {
    "gmc_version": "no argument",
    "gmc_error_string": "a code in, a static string out",
    "gmc_set_fuse": "a switch",
    "gmc_probe_begin": "the timing probe: host state only",
    "gmc_probe_end": "the timing probe: writes host arrays",
    "gmc_probe_flavours": "the timing probe: writes a host array",
    "gmc_lds_flavours": "host query: the batch's pointers are only tested against NULL",
    "gmc_ell_arrange_host": "host routine on host arrays",
    "gmc_ell_slots_for": "host routine on a host array",
    "gmc_w1_slab_floats": "a size",
    "gmc_host_device_pointer": "maps pinned host memory; launches nothing",
    "gmc_workspace_bytes": "a size query", "gmc_workspace_bytes_features": "a size query",
    "gmc_kway_workspace_bytes": "a size query", "gmc_large_workspace_bytes": "a size query",
    "gmc_fn_workspace_bytes": "a size query", "gmc_fn_cut_loss_workspace_bytes": "a size query",
    "gmc_inst_workspace_bytes": "a size query", "gmc_inst_large_workspace_bytes": "a size query",
    "gmc_att_workspace_bytes": "a size query", "gmc_large_round_workspace_bytes": "a size query",
    "gmc_large_search_workspace_bytes": "a size query", "gmc_batch_build_workspace_bytes": "a size query",
    "gmc_contract_workspace_bytes": "a size query",
    "gmc_large_required": "host query on the structs' scalars",
    "gmc_kway_tabu_fits": "host query on the batch's scalars", "gmc_kway_tabu_shape": "host query on the batch's scalars",
    "gmc_kway_balance_fits": "host query on the batch's scalars",
    "gmc_kway_balance_shape": "host query on the batch's scalars",
    "gmc_refine_order_host": "host routine on host arrays", "gmc_round_order_host": "host routine on host arrays",
    "gmc_large_round_order_host": "host routine on host arrays", "gmc_order_host_t": "host routine on host arrays",
}

# pointer parameters of EXEMPT functions that are host memory, with the words of the header (comments, whitespace
# collapsed) that say so
HOST_POINTERS = {
    ("gmc_ell_slots_for", "rowptr"): "for a batch with R rows (host pointer)",
    ("gmc_probe_end", "tags"): "(tag, milliseconds) pairs (host pointers)",
    ("gmc_probe_end", "ms"): "(tag, milliseconds) pairs (host pointers)",
    ("gmc_probe_flavours", "words"): "Writes up to `max` words (host pointer)",
    ("gmc_lds_flavours", "words"): "HOST query (no HIP call",
    ("gmc_host_device_pointer", "pinned_host"): "the device-side address of such memory (hipHostGetDevicePointer",
    ("gmc_host_device_pointer", "device_ptr"): "the device-side address of such memory (hipHostGetDevicePointer",
}
HOST_STRUCTS = ("const gmc_batch *", "const gmc_model *")


def declarations():
    """name -> [(type, parameter name)] of every function the header declares (comments stripped)."""
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"(?:^|\n)\s*(?:int|size_t|const char \*)\s*\*?\s*(gmc_\w+)\s*\(([^;{]*?)\)\s*;", code):
        params = []
        for raw in m.group(2).split(","):
            raw = " ".join(raw.split())
            if raw in ("void", ""):
                continue
            pm = re.match(r"(.*?)(\w+)$", raw)
            params.append((pm.group(1).strip(), pm.group(2)))
        out[m.group(1)] = params
    return out, " ".join(text.split())


def test_every_exported_name_is_in_exactly_one_set():
    decl, _ = declarations()
    import gcn_max_cut_amd as pkg
    assert set(decl) == set(pkg.hip.SYMBOLS)                              # the parse found what the binding declares
    sets = (COVERED, BANDED_ELSEWHERE, EXEMPT)
    for name in decl:
        where = [k for k, s in enumerate(sets) if name in s]
        assert len(where) == 1, (name, "in no set" if not where else "in more than one set")
    for s in sets:
        assert not set(s) - set(decl), ("not in the header", sorted(set(s) - set(decl)))


def test_exempt_functions_take_no_device_pointer():
    decl, flat = declarations()
    for name, reason in EXEMPT.items():
        assert reason
        for ctype, pname in decl[name]:
            if "*" not in ctype:
                continue
            if ctype in HOST_STRUCTS or "_host" in name:
                continue
            words = HOST_POINTERS.get((name, pname))
            assert words, (name, pname, "a pointer parameter that nothing marks as host memory")
            assert " ".join(words.split()) in flat, (name, pname, "the header no longer says", words)


def test_named_tests_exist():
    for table in (COVERED, BANDED_ELSEWHERE):
        for name, (module, fn) in table.items():
            path = os.path.join(ROOT, "tests", module + ".py")
            assert os.path.exists(path), (name, module)
            tree = ast.parse(open(path).read())
            assert fn in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (name, module, fn)


def _scalars_only(pkg, h, nnz_max=None):
    """A gmc_batch for the host queries: the scalars of `h`, and 1 for every array it has (the queries only test the
    pointers against NULL)."""
    from tests import bounds as B
    there = {k: (1 if getattr(h, k) is not None else None) for k in B.BATCH_ARRAYS}
    return pkg.hip.GmcBatch(B=h.B, R=h.R, nnz=h.nnz, n_max=h.n_max, uniform_n=h.uniform_n,
                            nnz_max=h.nnz_max if nnz_max is None else nnz_max, ell_width=h.ell_width,
                            ell_slots=h.ell_slots, ovf_max_blocks=h.ovf_max_blocks, **there)


def test_the_batches_reach_the_edges_they_are_there_for():
    """What DESIGN.md section 37 says of the bounds tests' batches, from the host queries: `tile` picks the ACC = 8
    flavours of the fused kernels and `odd` the ACC = 4 ones; the chain searches run four chains per workgroup over the
    staged CSR, two for `trip` at K = 8, four over the global CSR with nnz_max overstated - the table
    tests/test_gpu_bounds_decode.chain_shape asserts for every case it runs."""
    import ctypes as C
    import gcn_max_cut_amd as pkg
    from tests import bounds as B
    from tests.test_gpu_bounds_decode import chain_shape
    lib = pkg.hip.load()
    for kind, acc in (("tile", 8), ("odd", 4), ("odd9", 4)):
        for F in (4, 20, 516):
            for one_graph in (False, True):
                words = [pkg.hip.flavour_fields(w) for w in pkg.hip.lds_flavours(_scalars_only(pkg, B.host_batch(kind)), F,
                                                                              one_graph)]
                assert [w["kernel"] for w in words[:2]] == ["fwd1_lds", "bwd1_reg"], (kind, F, words)
                assert all(w["ACC"] == acc for w in words), (kind, F, words)
    seen = set()
    for kind in ("odd", "odd9", "hub", "trip"):
        h = B.host_batch(kind)
        for K in (2, 5, 8):
            for nnz_max in (None, 1 << 24):
                for query in (lib.gmc_kway_tabu_shape, lib.gmc_kway_balance_shape):
                    s = int(query(C.byref(_scalars_only(pkg, h, nnz_max)), K))
                    assert (s & 15, s >> 4) == chain_shape(kind, K, nnz_max), (kind, K, nnz_max, s)
                    seen.add((s & 15, s >> 4))
    assert seen == {(4, 1), (2, 1), (4, 0)}
