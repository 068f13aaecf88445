"""ctypes binding of ``libgcnmaxcut_hip.so`` (declared in ``include/gcnmaxcut.h``).

This is the only door from the Python host code to the compute path.  There is no
CPU fallback: if the shared library is missing, or no HIP device is visible, every
compute entry point raises (see :func:`require_gpu`).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GCN_MAXCUT_LIB") or os.path.join(_PKG, "lib", "libgcnmaxcut_hip.so")

MAX_GRAPH_NODES = 4096
# GMC_LARGE_MAX_GRAPH_NODES: what a graph of a batch may have (gmc_large_*: several workgroups share a graph's head); the
# fused, K-class and attention sequences, the one-workgroup decoders and the cut_loss op stay at MAX_GRAPH_NODES
LARGE_MAX_GRAPH_NODES = 1 << 20
ANNEAL_LEVELS = 1024  # GMC_ANNEAL_LEVELS: entries of the level table gmc_refine_anneal_f32 reads
MODEL_GRAD_TAIL = 1   # gmc_model.flags: grad has a tail slot that receives the batch's loss sum
MODEL_LOSS_EXPECTED = 2   # gmc_model.flags: loss and gradient are GMC_LOSS_EXPECTED_CUT
# GMC_LOSS_*: the reference's hard loss (-C * cut of the argmax decode) and the relaxed one (the expected cut of
# independent rounding: compute_loss on override_fixed_nodes(P) without the one-hot step)
LOSS_KINDS = {"cut": 0, "expected_cut": 1}
LOSS_ENV = "GCN_MAXCUT_LOSS"
# layer 1 of the model: the reference's GraphConv(norm='both'), or single-head graph attention (gmc_att_*: GATSoftmax)
LAYER1_KINDS = ("graphconv", "attention")
LAYER1_ENV = "GCN_MAXCUT_LAYER1"
ATTENTION_SLOPE = 0.2  # negative slope of the attention scores' leaky relu (the GAT paper's)
INST_ADAM_TILE_FLOATS = 4096   # GMC_INST_ADAM_TILE_FLOATS: floats of a graph's W1 one workgroup of gmc_inst_adam_f32 takes
KWAY_MAX_CLASSES = 8  # GMC_KWAY_MAX_CLASSES: number_classes the gmc_kway_* entry points take (2..8; 3 also has the fused path)
# GMC_BB_*: the int32 words of the report gmc_batch_build_csr leaves on the device (word k is BB_REPORT[k])
BB_REPORT = ("out_of_range", "cross_graph", "duplicate", "asymmetric", "zero_degree", "max_degree", "rows_over_8",
             "rows_over_16", "excess_8", "excess_16", "row_blocks_8", "row_blocks_16", "graph_blocks_8", "graph_blocks_16",
             "blocks_8", "blocks_16", "non_unit", "nnz", "nnz_max")
BB_REPORT_WORDS = 20  # GMC_BB_REPORT_WORDS
# GMC_CT_*: the int32 words of the report gmc_contract_map leaves on the device (word k is CT_REPORT[k]); any of the first
# CT_BAD_WORDS non-zero is bad input
CT_REPORT = ("pin_out_of_range", "pin_class", "pin_conflict", "graphs_missing_class", "graphs_no_free", "bare_terminals",
             "nnz", "pinned")
CT_BAD_WORDS = 6
CT_REPORT_WORDS = 8  # GMC_CT_REPORT_WORDS
ABI_VERSION = 200    # GMC_VERSION of include/gcnmaxcut.h these struct layouts follow (checked at load and per call)


class HipExtensionError(RuntimeError):
    """The HIP extension (or a GPU to run it on) is not available."""


class GmcBatch(C.Structure):
    _fields_ = [
        ("abi", C.c_int32), ("B", C.c_int32), ("R", C.c_int32), ("nnz", C.c_int32), ("n_max", C.c_int32),
        ("uniform_n", C.c_int32), ("nnz_max", C.c_int32),
        ("goff", C.c_void_p), ("rowptr", C.c_void_p), ("gcol", C.c_void_p), ("lcol", C.c_void_p),
        ("vals", C.c_void_p), ("dinv", C.c_void_p),
        ("ell", C.c_void_p), ("ell_vals", C.c_void_p), ("ell_width", C.c_int32), ("ell_slots", C.c_int32),
        ("ovf_ptr", C.c_void_p), ("ovf_ids", C.c_void_p), ("ovf_vals", C.c_void_p), ("ovf_max_blocks", C.c_int32),
    ]

    def __init__(self, **kw):
        kw.setdefault("abi", ABI_VERSION)
        super().__init__(**kw)


class GmcModel(C.Structure):
    _fields_ = [
        ("abi", C.c_int32), ("N", C.c_int32), ("F", C.c_int32), ("K", C.c_int32), ("flags", C.c_int32),
        ("W1", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p),
        ("dropout_p", C.c_float), ("dropout_seed_lo", C.c_uint32), ("dropout_seed_hi", C.c_uint32),
        ("W1_slab", C.c_void_p),
    ]

    def __init__(self, **kw):
        kw.setdefault("abi", ABI_VERSION)
        super().__init__(**kw)


def loss_kind(name: Optional[str]) -> int:
    """GMC_LOSS_* of a loss name; ``None`` reads the environment switch GCN_MAXCUT_LOSS (default ``cut``).  The
    library itself reads no environment."""
    if name is None:
        name = os.environ.get(LOSS_ENV) or "cut"
    try:
        return LOSS_KINDS[name]
    except (KeyError, TypeError):
        raise ValueError(f"unknown loss {name!r}: expected one of {sorted(LOSS_KINDS)}") from None


def loss_name(name: Optional[str]) -> str:
    """The canonical name of a loss (``None``: the environment's)."""
    kind = loss_kind(name)
    return next(k for k, v in LOSS_KINDS.items() if v == kind)


def layer1_name(name: Optional[str]) -> str:
    """The canonical name of a first layer; ``None`` reads the environment switch GCN_MAXCUT_LAYER1 (default
    ``graphconv``) at call time.  The library itself reads no environment."""
    if name is None:
        name = os.environ.get(LAYER1_ENV) or "graphconv"
    if name not in LAYER1_KINDS:
        raise ValueError(f"unknown layer1 {name!r}: expected one of {sorted(LAYER1_KINDS)}")
    return name


def _api() -> dict:
    """name -> (restype, argtypes) of every symbol include/gcnmaxcut.h declares: the one place an entry point is
    added to (tests check the .so exports all of them)."""
    vp, i32, i64, f32, f64, sz, i = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t, C.c_int
    B, M = C.POINTER(GmcBatch), C.POINTER(GmcModel)
    adam = [f64, f64, f64, f64]   # lr, beta1, beta2, eps
    return {
        "gmc_version": (i, []),
        "gmc_error_string": (C.c_char_p, [i]),
        "gmc_spmm_f32": (i, [vp, vp, vp, vp, vp, i64, vp, i, vp, i64, i32, i32, i32, vp, vp, vp]),
        "gmc_dense_hw2_f32": (i, [vp, i64, vp, vp, vp, i32, i32, vp]),
        "gmc_head_f32": (i, [B, vp, i32, vp, f32, vp, vp, vp, vp, vp, vp]),
        "gmc_head_loss_f32": (i, [B, vp, i32, vp, f32, i32, vp, vp, vp, vp, vp, vp]),
        "gmc_cut_loss_f32": (i, [B, vp, f32, i32, vp, vp, vp]),
        "gmc_adam_f32": (i, [vp, vp, vp, vp, i64, *adam, i32, vp]),
        "gmc_adam_devstep_f32": (i, [vp, vp, vp, vp, i64, *adam, vp, vp]),
        "gmc_adam_devstep_model_f32": (i, [vp, vp, vp, vp, i32, i32, vp, *adam, vp, vp]),
        "gmc_publish_f32": (i, [vp, i32, vp, vp]),
        "gmc_publish_adam_devstep_model_f32": (i, [vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, *adam, vp, vp]),
        "gmc_host_device_pointer": (i, [vp, C.POINTER(vp)]),
        "gmc_w1_slab_floats": (sz, [i32, i32]),
        "gmc_w1_slab_f32": (i, [vp, i32, i32, vp, vp]),
        "gmc_workspace_bytes": (sz, [B, M, i]),
        "gmc_forward": (i, [B, M, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_train_fwd_bwd": (i, [B, M, f32, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_train_step_f32": (i, [B, i32, i32, vp, f32, vp, sz, vp, vp, vp, vp, vp, vp, *adam, vp, vp, vp]),
        "gmc_train_step_loss_f32": (i, [B, i32, i32, vp, f32, i32, vp, sz, vp, vp, vp, vp, vp, vp, *adam, vp, vp, vp]),
        "gmc_backward_from_gp": (i, [B, M, vp, sz, vp, vp, vp, vp]),
        "gmc_workspace_bytes_features": (sz, [B, M, i]),
        "gmc_forward_features": (i, [B, M, vp, i64, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_backward_features_from_gp": (i, [B, M, vp, i64, vp, sz, vp, vp, vp, vp, i64, vp]),
        "gmc_kway_workspace_bytes": (sz, [B, M, i]),
        "gmc_kway_forward": (i, [B, M, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_kway_train_fwd_bwd": (i, [B, M, f32, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_large_workspace_bytes": (sz, [B, M, i]),
        "gmc_large_forward": (i, [B, M, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_large_train_fwd_bwd": (i, [B, M, f32, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_large_required": (i, [B, M]),
        "gmc_fn_workspace_bytes": (sz, [B, M, i]),
        "gmc_fn_forward": (i, [B, M, vp, i64, vp, sz, vp, vp]),
        "gmc_fn_backward": (i, [B, M, vp, i64, vp, sz, vp, vp, vp, vp, i64, vp]),
        "gmc_fn_cut_loss_workspace_bytes": (sz, [B, i32]),
        "gmc_fn_cut_loss_f32": (i, [B, i32, i32, vp, f32, i32, vp, sz, vp, vp, vp]),
        "gmc_inst_workspace_bytes": (sz, [B, M, i]),
        "gmc_inst_forward": (i, [B, M, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_inst_train_fwd_bwd": (i, [B, M, f32, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_inst_keep_best_f32": (i, [B, vp, vp, i32, vp, vp, vp, vp]),
        "gmc_inst_early_stop_f32": (i, [B, vp, vp, i32, f64, i32, vp, vp, vp, vp, vp, vp, vp]),
        "gmc_inst_adam_f32": (i, [B, i32, i32, vp, vp, vp, vp, *adam, i32, vp, vp]),
        "gmc_att_workspace_bytes": (sz, [B, M, i]),
        "gmc_att_forward": (i, [B, M, vp, vp, f32, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_att_train_fwd_bwd": (i, [B, M, vp, vp, f32, f32, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_gemm_f32": (i, [i32, i32, i32, i32, i32, vp, i64, vp, i64, vp, vp, i64, vp]),
        "gmc_set_fuse": (i, [i]),
        "gmc_probe_begin": (i, [i32]),
        "gmc_probe_end": (i, [vp, vp, i32]),
        "gmc_probe_flavours": (i, [vp, i32]),
        "gmc_lds_flavours": (i, [B, i32, i32, vp, i32]),
        "gmc_ell_arrange_host": (i, [i32, vp, vp, vp, vp, i32, vp, vp]),
        "gmc_ell_slots_for": (i, [i32, vp, i32]),
        "gmc_decode_sample_f32": (i, [B, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "gmc_decode_sample_seeded_f32": (i, [B, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "gmc_refine_order_host": (i, [i32, vp, vp, vp, vp, vp, vp, i32]),
        "gmc_refine_local_f32": (i, [B, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
        "gmc_refine_anneal_f32": (i, [B, vp, vp, vp, i32, vp, vp, i32, vp, C.c_uint64, i32, vp, vp, vp, vp, vp, vp, vp]),
        "gmc_refine_anneal_staged": (i, [B]),
        "gmc_round_order_host": (i, [i32, vp, vp, vp, i32, vp, vp, vp, i32]),
        "gmc_round_conditional_f32": (i, [B, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "gmc_kway_decode_sample_seeded_f32": (i, [B, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
        "gmc_kway_refine_anneal_f32": (i, [B, i32, vp, vp, vp, i32, vp, vp, i32, vp, C.c_uint64, i32, vp, vp, vp, vp, vp,
                                           vp, vp]),
        "gmc_kway_evolve_f32": (i, [B, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp, i32, vp, C.c_uint64, i32, vp, vp, vp,
                                    vp, vp]),
        "gmc_kway_tabu_f32": (i, [B, i32, i32, i32, vp, i32, i32, i32, i32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]),
        "gmc_kway_tabu_fits": (i, [B, i32]),
        "gmc_kway_tabu_shape": (i, [B, i32]),
        "gmc_kway_balance_f32": (i, [B, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, C.c_uint64, vp, vp, vp, vp, vp, vp,
                                     vp, vp, vp]),
        "gmc_kway_balance_fits": (i, [B, i32]),
        "gmc_kway_balance_shape": (i, [B, i32]),
        "gmc_large_round_order_host": (i, [i32, vp, vp, vp, i32, vp, vp, vp, i32, vp]),
        "gmc_large_round_workspace_bytes": (sz, [B, i32]),
        "gmc_large_round_conditional_f32": (i, [B, vp, i32, vp, vp, vp, i32, i32, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_large_local_search_f32": (i, [B, i32, vp, vp, vp, i32, i32, vp, sz, vp, vp, vp, vp]),
        "gmc_large_search_workspace_bytes": (sz, [B, i32, i32]),
        "gmc_large_sample_seeded_f32": (i, [B, vp, i32, vp, i32, vp, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_large_anneal_f32": (i, [B, i32, vp, vp, vp, i32, i32, vp, vp, i32, vp, C.c_uint64, i32, vp, sz, vp, vp, vp,
                                     vp, vp, vp, vp]),
        "gmc_batch_build_workspace_bytes": (sz, [i32, i32, i64]),
        "gmc_batch_build_csr": (i, [i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "gmc_batch_build_table": (i, [i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, sz, vp]),
        "gmc_contract_workspace_bytes": (sz, [i32, i32, i64, i32]),
        "gmc_contract_map": (i, [B, i32, i64, vp, vp, vp, vp, vp, vp, sz, vp]),
        "gmc_contract_entries": (i, [B, i32, vp, vp, i64, vp, vp, vp, vp, vp, sz, vp]),
        # the terminals optional: the entry points above with `terminals` (0 or 1) after the class count / the model
        "gmc_order_host_t": (i, [i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp]),
        "gmc_round_conditional_t_f32": (i, [B, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "gmc_kway_decode_sample_seeded_t_f32": (i, [B, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
        "gmc_kway_refine_anneal_t_f32": (i, [B, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, C.c_uint64, i32, vp, vp, vp, vp,
                                             vp, vp, vp]),
        "gmc_large_round_conditional_t_f32": (i, [B, vp, i32, i32, vp, vp, vp, i32, i32, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_large_local_search_t_f32": (i, [B, i32, i32, vp, vp, vp, i32, i32, vp, sz, vp, vp, vp, vp]),
        "gmc_large_sample_seeded_t_f32": (i, [B, vp, i32, i32, vp, i32, vp, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_large_anneal_t_f32": (i, [B, i32, i32, vp, vp, vp, i32, i32, vp, vp, i32, vp, C.c_uint64, i32, vp, sz, vp, vp,
                                       vp, vp, vp, vp, vp]),
        "gmc_inst_forward_t": (i, [B, M, i32, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_inst_train_fwd_bwd_t": (i, [B, M, i32, f32, vp, sz, vp, vp, vp, vp, vp]),
        # one model per graph for graphs of up to LARGE_MAX_GRAPH_NODES nodes
        "gmc_inst_large_workspace_bytes": (sz, [B, M, i]),
        "gmc_inst_large_forward": (i, [B, M, i32, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_inst_large_train_fwd_bwd": (i, [B, M, i32, f32, vp, sz, vp, vp, vp, vp, vp]),
        # per-node class costs: the `_t` entry points with `node_cost` ([R][K] or NULL) after `terminals`
        "gmc_round_conditional_c_f32": (i, [B, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "gmc_kway_decode_sample_seeded_c_f32": (i, [B, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "gmc_kway_refine_anneal_c_f32": (i, [B, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, C.c_uint64, i32, vp, vp, vp,
                                             vp, vp, vp, vp]),
        "gmc_inst_forward_c": (i, [B, M, i32, vp, f32, vp, sz, vp, vp, vp, vp]),
        "gmc_inst_train_fwd_bwd_c": (i, [B, M, i32, vp, f32, vp, sz, vp, vp, vp, vp, vp]),
        "gmc_row_weight_sums_f32": (i, [i32, vp, vp, vp, vp, vp]),
        # the two chain searches with `node_cost` after `terminals`
        "gmc_kway_tabu_c_f32": (i, [B, i32, i32, vp, i32, vp, i32, i32, i32, i32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]),
        "gmc_kway_balance_c_f32": (i, [B, i32, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, C.c_uint64, vp, vp, vp, vp, vp,
                                       vp, vp, vp, vp]),
    }


def _sdp_api() -> dict:
    """name -> (restype, argtypes) of every symbol include/gcnmaxcut_sdp.h declares (the semidefinite relaxation: a
    header and a table of its own, so ``SYMBOLS`` stays the mirror of include/gcnmaxcut.h)."""
    vp, i32, sz, i = C.c_void_p, C.c_int32, C.c_size_t, C.c_int
    B = C.POINTER(GmcBatch)
    return {
        "gmc_sdp_workspace_bytes": (sz, [B, i32]),
        "gmc_sdp_relax_f32": (i, [B, i32, i32, vp, vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, sz, vp]),
        "gmc_sdp_round_f32": (i, [B, i32, i32, vp, vp, i32, i32, vp, vp]),
    }


def _temper_api() -> dict:
    """name -> (restype, argtypes) of every symbol include/gcnmaxcut_temper.h declares (parallel tempering over decoded
    partitions: a header and a table of its own, as the semidefinite relaxation has)."""
    vp, i32, sz, i = C.c_void_p, C.c_int32, C.c_size_t, C.c_int
    B = C.POINTER(GmcBatch)
    return {
        "gmc_kway_temper_workspace_bytes": (sz, [B, i32]),
        "gmc_kway_temper_f32": (i, [B, i32, i32, vp, vp, vp, vp, i32, i32, vp, i32, i32, vp, C.c_uint64, vp, vp, vp, vp, vp,
                                    vp, vp, sz, vp]),
    }


def _dense_api() -> dict:
    """name -> (restype, argtypes) of every symbol include/gcnmaxcut_dense.h declares (annealing of dense two-class
    instances on cached local fields: a header and a table of its own, as the tempering has)."""
    vp, i32, i64, sz, i = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_int
    return {
        "gmc_dense_anneal_workspace_bytes": (sz, [i32, i32, i32]),
        "gmc_dense_anneal_f32": (i, [i32, i32, vp, i64, vp, vp, i32, vp, vp, i32, vp, C.c_uint64, i32, vp, sz, vp, vp, vp,
                                     vp, vp, vp, vp, vp]),
    }


def _bifurcation_api() -> dict:
    """name -> (restype, argtypes) of every symbol include/gcnmaxcut_bifurcation.h declares (discrete simulated
    bifurcation of dense two-class instances: a header and a table of its own, as the dense annealing has)."""
    vp, i32, i64, sz, i, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_int, C.c_float
    return {
        "gmc_dense_sb_state_bytes": (sz, [i32, i32, i32]),
        "gmc_dense_sb_workspace_bytes": (sz, [i32, i32, i32]),
        "gmc_dense_sb_init_f32": (i, [i32, i32, i32, C.c_uint64, f32, vp, vp, vp]),
        "gmc_dense_sb_f32": (i, [i32, i32, vp, i64, vp, i32, vp, vp, vp, i32, f32, f32, vp, sz, vp, vp]),
    }


_API = _api()
SYMBOLS = tuple(_API)
_BIFURCATION_API = _bifurcation_api()
BIFURCATION_SYMBOLS = tuple(_BIFURCATION_API)
_SDP_API = _sdp_api()
SDP_SYMBOLS = tuple(_SDP_API)
_TEMPER_API = _temper_api()
TEMPER_SYMBOLS = tuple(_TEMPER_API)
_DENSE_API = _dense_api()
DENSE_SYMBOLS = tuple(_DENSE_API)
TEMPER_MAX_RUNGS = 256   # GMC_TEMPER_MAX_RUNGS: the longest ladder gmc_kway_temper_f32 takes
SDP_RANKS = (16, 32, 64)   # the ranks gmc_sdp_relax_f32 / gmc_sdp_round_f32 take

_lib: Optional[C.CDLL] = None


def _declare(lib: C.CDLL) -> None:
    for name, (restype, argtypes) in (list(_API.items()) + list(_SDP_API.items()) + list(_TEMPER_API.items())
                                      + list(_DENSE_API.items()) + list(_BIFURCATION_API.items())):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    lib.gmc_debug_set_device_cus.argtypes = [C.c_int]   # test hook (not part of gcnmaxcut.h)
    lib.gmc_debug_set_device_cus.restype = C.c_int


def load() -> C.CDLL:
    """dlopen the in-tree library (no compute; works without a GPU)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionError(
                f"{LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        lib.gmc_version.restype = C.c_int
        have = int(lib.gmc_version())
        if have != ABI_VERSION:   # struct layouts and signatures are chosen by VERSION, never by sniffing symbols
            raise HipExtensionError(
                f"{LIB_PATH} reports gmc_version() = {have}, this binding is written for {ABI_VERSION} "
                f"(include/gcnmaxcut.h): rebuild the library (`python -c 'import __graft_entry__ as g; g.build()'`)")
        _declare(lib)
        _lib = lib
    return _lib


def require_gpu() -> torch.device:
    """The compute path needs the HIP library *and* a visible GPU; fail loudly otherwise."""
    load()
    if not torch.cuda.is_available():
        raise HipExtensionError(
            "no HIP device visible: the GCN max-cut compute path runs only on a GPU "
            "(MI355X/gfx950); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    msg = load().gmc_error_string(rc).decode()
    if rc < 0:
        raise ValueError(f"{what}: {msg} (gmc error {rc})")
    raise RuntimeError(f"{what}: HIP error {rc}: {msg}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipExtensionError("tensor is not on a HIP device")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


def mapped_ptr(t: torch.Tensor) -> Optional[int]:
    """Device-side address of a PINNED host tensor (kernels may store into it; the host polls it), or None when
    the library / runtime cannot map it."""
    lib = load()
    if not (t.device.type == "cpu" and t.is_pinned() and t.is_contiguous()):
        return None
    out = C.c_void_p()
    if lib.gmc_host_device_pointer(C.c_void_p(t.data_ptr()), C.byref(out)) != 0 or not out.value:
        return None
    return int(out.value)


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


KERNEL_TAGS = ("gather_w1", "agg_fwd", "head", "hidden_bwd", "colsum", "agg_bwd", "dw1", "dw1_fold",
               "adam", "spmm_user", "dense_mfma", "bwd1_fused", "fwd1_fused", "decode", "finish",
               "refine", "anneal")
# the tags after those (GMC_K_GEMM = 17 on): what Probe names a record by
PROBE_TAGS = KERNEL_TAGS + ("gemm", "sample")


FLAVOUR_KERNELS = {1: "fwd1_lds", 2: "bwd1_lds", 3: "bwd1_reg", 4: "spmm_lds", 5: "dw1_lds"}   # GMC_FLV_KERNEL


def flavour_fields(word: int) -> dict:
    """The bit fields of a flavour word (include/gcnmaxcut.h, GMC_FLV_*)."""
    return dict(kernel=FLAVOUR_KERNELS.get(word & 7, "?"), FS=word >> 3 & 0x7f, W=word >> 10 & 0x1f,
                ACC=word >> 15 & 0xf, NS=word >> 19 & 0x1f, HAS_VAL=word >> 24 & 1, OVF=word >> 25 & 1,
                HEAD=word >> 26 & 1, EPI=word >> 27 & 1, SHARED=word >> 28 & 1, PER=1 << (word >> 29 & 3))


def lds_flavours(batch_struct: GmcBatch, F: int, one_graph_step: bool = False) -> list:
    """Flavour words of the LDS-tiled launches of a training step (gmc_lds_flavours; host only, no GPU):
    the fused sequence (fwd1, bwd1), then - batches without overflow lists - the gmc_set_fuse(0) sequence."""
    words = (C.c_int32 * 8)()
    n = load().gmc_lds_flavours(C.byref(batch_struct), int(F), int(bool(one_graph_step)), words, 8)
    if n < 0:
        check(n, "gmc_lds_flavours")
    return [int(words[i]) for i in range(n)]


class Probe:
    """``with Probe(capacity) as p: ...`` then ``p.records`` = [(kernel_tag, ms), ...]:
    per-launch HIP-event timings recorded by the library on the launch stream, and ``p.flavours`` = the
    flavour word of each of those launches (0 for kernels outside the LDS-tiled families)."""

    def __init__(self, capacity: int):
        self.capacity, self.records, self.flavours = capacity, [], []

    def __enter__(self):
        check(load().gmc_probe_begin(self.capacity), "gmc_probe_begin")
        return self

    def __exit__(self, *exc):
        tags = (C.c_int32 * self.capacity)()
        ms = (C.c_float * self.capacity)()
        n = load().gmc_probe_end(tags, ms, self.capacity)
        if n < 0:
            raise RuntimeError(f"gmc_probe_end failed ({n})")
        self.records = [(PROBE_TAGS[tags[i]], float(ms[i])) for i in range(min(n, self.capacity))]
        words = (C.c_int32 * self.capacity)()
        m = load().gmc_probe_flavours(words, self.capacity)
        if m != n:
            raise RuntimeError(f"gmc_probe_flavours returned {m}, gmc_probe_end {n}")
        self.flavours = [int(words[i]) for i in range(min(n, self.capacity))]
        return False
