"""ctypes binding of libglove_hip.so (C ABI: include/glove_hip.h), of libglove_eval_hip.so (include/glove_eval_hip.h,
include/glove_eval_sim_hip.h, include/glove_eval_cluster_hip.h), of libglove_prep_hip.so (include/glove_cooc_stream_hip.h,
include/glove_text_hip.h, include/glove_vectors_hip.h, include/glove_cooc_options_hip.h) and of libglove_factor_hip.so
(include/glove_factor_hip.h, include/glove_factor_dense_hip.h, include/glove_factor_graph_hip.h).

This is the only way the host loop reaches the GPU kernels.  There is no CPU fallback: if the
shared library is missing or a call fails, an exception is raised.  torch is used here only
as the owner of device memory and streams (`tensor.data_ptr()`, `current_stream().cuda_stream`).
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from trainer.optimizers import BY_CODE, OPTIMIZERS, names

logger = logging.getLogger(__name__)

PKG_DIR = Path(__file__).resolve().parent.parent
LIB_PATH = PKG_DIR / "lib" / "libglove_hip.so"
EVAL_LIB_PATH = PKG_DIR / "lib" / "libglove_eval_hip.so"      # include/glove_eval_hip.h: scoring finished embeddings, a library of its own

PREP_LIB_PATH = PKG_DIR / "lib" / "libglove_prep_hip.so"      # include/glove_cooc_stream_hip.h: counting a corpus chunk by chunk, a library of its own
FACTOR_LIB_PATH = PKG_DIR / "lib" / "libglove_factor_hip.so"  # include/glove_factor_hip.h: the count-based baselines (trainer.svd), a library of its own

GLOVE_ABI_VERSION = 15
GLOVE_EVAL_ABI_VERSION = 1
GLOVE_EVAL_SIM_ABI_VERSION = 1      # include/glove_eval_sim_hip.h: the same library's second header, versioned on its own
GLOVE_EVAL_CLUSTER_ABI_VERSION = 1  # include/glove_eval_cluster_hip.h: the third header (spherical k-means), likewise
GLOVE_EVAL_CROSS_ABI_VERSION = 1    # include/glove_eval_cross_hip.h: the fourth header (neighbours across two tables, CSLS), likewise
GLOVE_COOC_STREAM_ABI_VERSION = 1   # include/glove_cooc_stream_hip.h (libglove_prep_hip.so)
COOC_MERGE_TILE = 2048              # GLOVE_COOC_MERGE_TILE: merged positions one workgroup of glove_cooc_merge_u64 owns
GLOVE_TEXT_ABI_VERSION = 1          # include/glove_text_hip.h: the same library's second header (tokenizing), versioned on its own
TEXT_TILE_BYTES = 4096              # GLOVE_TEXT_TILE_BYTES: bytes of a block one workgroup of glove_text_tokenize_u8 owns
TEXT_MAX_TOKEN = 65535              # GLOVE_TEXT_MAX_TOKEN: bytes of a token its hash covers; the longest length a `where` word holds
GLOVE_VECTORS_ABI_VERSION = 1       # include/glove_vectors_hip.h: the same library's third header (word-vector files), versioned on its own
VECTORS_TILE_BYTES = 4096           # GLOVE_VECTORS_TILE_BYTES: bytes of a block one workgroup of glove_vectors_lines_u8 owns
VECTORS_MAX_SPAN = 65535            # GLOVE_VECTORS_MAX_SPAN: the longest token length a fallback span holds
VECTORS_MAX_D = 65536               # GLOVE_VECTORS_MAX_D: the most numbers per record / columns of a table
GLOVE_COOC_OPTIONS_ABI_VERSION = 1  # include/glove_cooc_options_hip.h: the same library's fourth header (token filter, window weightings), versioned on its own
FILTER_TILE = 4096                  # GLOVE_FILTER_TILE: tokens of a block one workgroup of glove_token_filter_i32 owns
WINDOW_WEIGHTINGS = {"harmonic": 0, "uniform": 1, "dynamic": 2}      # GLOVE_WINDOW_*
GLOVE_PHRASES_ABI_VERSION = 1       # include/glove_phrases_hip.h: the same library's fifth header (phrase detection), versioned on its own
PHRASE_TILE = 1024                  # GLOVE_PHRASE_TILE: tokens of a block one workgroup of glove_phrase_join_u8 owns
PHRASE_SELECT_TILE = 1024           # GLOVE_PHRASE_SELECT_TILE: keys of a table one workgroup of glove_phrase_select owns
GLOVE_FACTOR_ABI_VERSION = 1        # include/glove_factor_hip.h (libglove_factor_hip.so)
FACTOR_CHUNK = 512                  # GLOVE_FACTOR_CHUNK: nonzeros of a row one lane group of glove_csr_spmm_f32 sums
GLOVE_FACTOR_DENSE_ABI_VERSION = 1  # include/glove_factor_dense_hip.h: the same library's second header (dense tables), versioned on its own
GRAM_CHUNK = 1024                   # GLOVE_GRAM_CHUNK: rows of one float32 fmaf chain of glove_gram_f64
GRAM_SLICE = 16384                  # GLOVE_GRAM_SLICE: rows whose chunk partials one float64 slice partial adds
GLOVE_FACTOR_GRAPH_ABI_VERSION = 1  # include/glove_factor_graph_hip.h: the same library's third header (retrofitting), versioned on its own
GLOVE_FACTOR_ALIGN_ABI_VERSION = 1  # include/glove_factor_align_hip.h: the same library's fourth header (cross-covariance of row pairs), versioned on its own
REWEIGHT_KINDS = {"none": 0, "sqrt": 1, "log1p": 2, "ppmi": 3}      # GLOVE_REWEIGHT_*
HEAD_REGRESSION, HEAD_LOGISTIC = 0, 1      # glove_hyper.head
OPTIMIZER_CODES = {o.name: o.code for o in OPTIMIZERS.values()}      # glove_hyper.optimizer (GLOVE_OPT_*): trainer/optimizers.py holds what every name needs
ROW_WISE_OPTIMIZERS = names(lambda o: o.row_wise)      # slot 1 of R and C is ONE float per row (float[rows]), not shaped like the table
STEP_AUTO, STEP_TWO_LAUNCH, STEP_FUSED_ONE_PASS, STEP_FUSED_THREE_LAUNCH, STEP_FUSED_TWIN, STEP_TAGGED = 0, 1, 2, 3, 4, 5   # glove_hyper.step_form (2: tests / comparisons only)
TAGGED_STEP_MAX_BATCH = 2048      # GLOVE_STEP_AUTO takes the tagged step up to this batch size on step-tagged tables
DEFAULT_CHUNK_CAP = 32
RECORDS_AT_BUILD_MAX = 4096     # batches up to this size get their chunk records inside glove_plan_build
HEAVY_CHUNKS = 8          # ids with more chunks than this are reduced by a whole workgroup


RUN_WORDS_MIN_CHUNKS = 98304    # chunks of a side from which a resident plan of the fused regime keeps run words instead of records (6 chunks per lane group)
FUSED_STEP_BYTES = 96 << 20    # GLOVE_FUSED_STEP_BYTES (include/glove_hip.h): touched ids x row bytes x 4 beyond which the fused step pays (tests/test_abi.py holds the two together)


def auto_chunk_cap(B: int, V: int, d: int | None = None) -> int:
    """Chunk length used when the caller does not choose one.  Short chunks shorten the dependent
    chain of the gather passes (fewer partner-row round trips per chunk) and win while a batch holds
    few pairs per id; long chunks mean fewer partial rows and win for dense batches (bench.py --chunk-cap,
    V = 10000: B = 131072: 8 / 16 / 24 / 32 -> 22.4 / 21.2 / 22.3 / 23.3 us per step; B = 1048576: 16 -> 59.4, 32 -> 53.8).
    Tables beyond the L2s (`d` given: V x d x 4 B >= 32 MB) take the fused step at realistic batch sizes, which is bandwidth-bound
    and likes long chunks (V = 400 k, d = 300, B = 1 M: 8 / 16 / 32 -> 746 / 734 / 722 us per step)."""
    if d is not None and V * d * 4 >= (32 << 20):       # (round 5: V = 50 k, d = 300 — 61 MB — cap 8 / 16 / 32 -> 96.3 / 92.6 / 91.7 us per step)
        return 32
    return 16 if B <= 20 * V else 32

# every symbol include/glove_hip.h declares
EXPORTED_SYMBOLS = (
    "glove_abi_version", "glove_plan_workspace_bytes", "glove_plan_build", "glove_plan_fill_records", "glove_step_workspace_bytes",
    "glove_passes_f32", "glove_rowpass_f32", "glove_colpass_f32", "glove_apply_adagrad_f32",
    "glove_dense_grad_f32", "glove_dense_adagrad_f32", "glove_dense_adam_f32", "glove_step_adagrad_f32",
    "glove_steps_adagrad_f32", "glove_step_adam_f32", "glove_steps_adam_f32", "glove_eval_f32", "glove_eval_logistic_f32", "glove_topk_workspace_bytes", "glove_topk_cosine_f32",
    "glove_cooc_workspace_bytes", "glove_cooccurrence_i32", "glove_dense_grad_layout",
    "glove_pack_grad_f32", "glove_passes_packing_f32", "glove_pack_rest_f32", "glove_loss_partials_f32", "glove_combine_packed_f32", "glove_apply_packed_adagrad_f32",
    "glove_gather_rows_f32", "glove_canonicalize_f32", "glove_rowside_step_adagrad_f32",
    "glove_count_packed_f32",
    "glove_masters_workspace_bytes", "glove_masters_build", "glove_epoch_deal_workspace_bytes", "glove_epoch_deal",
    "glove_plan_sorted_workspace_bytes", "glove_plan_chunk_bound", "glove_plan_build_sorted", "glove_step_sparse_f32",
    "glove_rowside_step_f32",
)

# every symbol include/glove_eval_hip.h declares
EVAL_EXPORTED_SYMBOLS = ("glove_eval_abi_version", "glove_analogy_workspace_bytes", "glove_analogy_topk_f32")
# every symbol include/glove_eval_sim_hip.h declares (the same library)
EVAL_SIM_EXPORTED_SYMBOLS = ("glove_eval_sim_abi_version", "glove_cosmul_workspace_bytes", "glove_cosmul_topk_f32",
                             "glove_pair_cosine_f32")
# every symbol include/glove_eval_cluster_hip.h declares (the same library)
EVAL_CLUSTER_EXPORTED_SYMBOLS = ("glove_eval_cluster_abi_version", "glove_kmeans_workspace_bytes", "glove_kmeans_assign_f32",
                                 "glove_kmeans_update_f32")
KMEANS_MAX_CLUSTERS = 4096
# every symbol include/glove_eval_cross_hip.h declares (the same library)
EVAL_CROSS_EXPORTED_SYMBOLS = ("glove_eval_cross_abi_version", "glove_cross_topk_workspace_bytes", "glove_cross_topk_f32",
                               "glove_topk_mean_f32")
# every symbol include/glove_cooc_stream_hip.h declares (libglove_prep_hip.so)
PREP_EXPORTED_SYMBOLS = ("glove_cooc_stream_abi_version", "glove_cooc_chunk_workspace_bytes", "glove_cooc_chunk_keys_i32",
                         "glove_cooc_merge_workspace_bytes", "glove_cooc_merge_u64", "glove_cooc_finalize_workspace_bytes",
                         "glove_cooc_finalize")
# every symbol include/glove_text_hip.h declares (the same library)
TEXT_EXPORTED_SYMBOLS = ("glove_text_abi_version", "glove_text_tokenize_workspace_bytes", "glove_text_tokenize_u8",
                         "glove_text_block_vocab_workspace_bytes", "glove_text_block_vocab",
                         "glove_text_vocab_merge_workspace_bytes", "glove_text_vocab_merge", "glove_text_token_ids_i32")
# every symbol include/glove_vectors_hip.h declares (the same library)
VECTORS_EXPORTED_SYMBOLS = ("glove_vectors_abi_version", "glove_vectors_lines_workspace_bytes", "glove_vectors_lines_u8",
                            "glove_vectors_parse_f32", "glove_vectors_format_workspace_bytes", "glove_vectors_format_f32")
# every symbol include/glove_cooc_options_hip.h declares (the same library)
COOC_OPTIONS_EXPORTED_SYMBOLS = ("glove_cooc_options_abi_version", "glove_token_filter_workspace_bytes", "glove_token_filter_i32",
                                 "glove_cooc_finalize_weighted_workspace_bytes", "glove_cooc_finalize_weighted")
# every symbol include/glove_phrases_hip.h declares (the same library)
PHRASES_EXPORTED_SYMBOLS = ("glove_phrases_abi_version", "glove_phrase_bigram_workspace_bytes", "glove_phrase_bigram_keys_i32",
                            "glove_phrase_select_workspace_bytes", "glove_phrase_select", "glove_phrase_join_workspace_bytes",
                            "glove_phrase_join_u8")
# every symbol include/glove_factor_hip.h declares (libglove_factor_hip.so)
FACTOR_EXPORTED_SYMBOLS = ("glove_factor_abi_version", "glove_csr_spmm_workspace_bytes", "glove_csr_spmm_f32",
                           "glove_csr_row_sums_f64", "glove_coo_reweight_f32")
# every symbol include/glove_factor_dense_hip.h declares (the same library)
FACTOR_DENSE_EXPORTED_SYMBOLS = ("glove_factor_dense_abi_version", "glove_gram_workspace_bytes", "glove_col_sums_f64",
                                 "glove_gram_f64", "glove_rows_transform_f32")
# every symbol include/glove_factor_graph_hip.h declares (the same library)
FACTOR_GRAPH_EXPORTED_SYMBOLS = ("glove_factor_graph_abi_version", "glove_retrofit_rows_f32")
# every symbol include/glove_factor_align_hip.h declares (the same library)
FACTOR_ALIGN_EXPORTED_SYMBOLS = ("glove_factor_align_abi_version", "glove_cross_gram_workspace_bytes", "glove_cross_gram_f64")

_fp = C.c_void_p  # device pointers travel as integers


class GloveTables(C.Structure):
    _fields_ = [("V", C.c_int32), ("d", C.c_int32), ("V_row", C.c_int32), ("d_model", C.c_int32),
                ("R", _fp), ("C", _fp), ("br", _fp), ("bc", _fp),
                ("s1_R", _fp), ("s1_C", _fp), ("s1_br", _fp), ("s1_bc", _fp),
                ("s2_R", _fp), ("s2_C", _fp), ("s2_br", _fp), ("s2_bc", _fp),
                ("scalars", _fp), ("step", _fp), ("R_ver", _fp), ("R_tag", _fp), ("C_tag", _fp)]


class GloveHyper(C.Structure):
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double),
                ("l2_reg", C.c_float), ("reg_mult", C.c_float), ("learning_rate", C.c_float),
                ("epsilon", C.c_float), ("inv_batch", C.c_float), ("sides", C.c_int32),
                ("head", C.c_int32), ("neg_factor", C.c_float), ("step_form", C.c_int32),
                ("optimizer", C.c_int32), ("momentum", C.c_float), ("nesterov", C.c_int32), ("rho", C.c_float),
                ("sweep_sides", C.c_int32)]


class GlovePlan(C.Structure):
    _fields_ = [("B", C.c_int64), ("chunk_cap", C.c_int32), ("cap_chunks", C.c_int32),
                ("cap_uniq", C.c_int32), ("heavy_chunks", C.c_int32), ("cap_heavy", C.c_int32),
                ("V_row", C.c_int32), ("counts", _fp), ("host_counts", C.c_int32 * 8),
                ("r_partner", _fp), ("r_w", _fp), ("r_y", _fp), ("r_to_c", _fp),
                ("r_chunk_id", _fp), ("r_chunk_start", _fp), ("r_uniq_slot", _fp), ("r_uniq_rec", _fp),
                ("c_partner", _fp), ("c_perm", _fp), ("c_w", _fp), ("c_y", _fp),
                ("c_chunk_id", _fp), ("c_chunk_start", _fp), ("c_uniq_slot", _fp), ("c_uniq_rec", _fp), ("heavy", _fp),
                ("r_crec", _fp), ("c_crec", _fp), ("r_mark", _fp), ("c_mark", _fp),
                ("r_chunk_hw", _fp), ("c_chunk_hw", _fp)]


class GlovePairs(C.Structure):
    _fields_ = [("id", _fp), ("partner", _fp), ("w", _fp), ("y", _fp)]


class GlovePackedList(C.Structure):
    _fields_ = [("entries", _fp), ("ids", _fp), ("header", _fp), ("n", C.c_int32), ("side", C.c_int32)]


class GloveHipError(RuntimeError):
    pass


_lib = None


def _open(p: Path, protos: dict, optional: bool = False) -> C.CDLL:
    """dlopen a built library and declare its prototypes (`optional`: symbols an older build lacks are left out)."""
    if not p.exists():
        raise GloveHipError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % p)
    lib = C.CDLL(str(p))
    for name, (res, args) in protos.items():
        if optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    return lib


def load_library(path: os.PathLike | None = None, any_abi: bool = False) -> C.CDLL:
    """dlopen libglove_hip.so and declare the prototypes.  Raises if it is not built.  `path` / `any_abi`: explicit
    arguments of the A/B tools (tools/ab_kernels.py), which load other builds of the library — older ones included —
    beside the shipped one; nothing in the product passes them and no environment variable is read."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    P = C.POINTER
    sz, i32, i64, vp = C.c_size_t, C.c_int32, C.c_int64, C.c_void_p
    protos = {
        "glove_abi_version": (C.c_int, []),
        "glove_plan_workspace_bytes": (sz, [i64, i32]),
        "glove_plan_build": (C.c_int, [vp, vp, vp, vp, i64, i32, P(GlovePlan), vp, sz, vp]),
        "glove_plan_fill_records": (C.c_int, [P(GlovePlan), vp]),
        "glove_masters_workspace_bytes": (sz, [i64]),
        "glove_masters_build": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, P(GlovePairs), P(GlovePairs), vp, vp, vp, sz, vp]),
        "glove_epoch_deal_workspace_bytes": (sz, [i64, i64]),
        "glove_epoch_deal": (C.c_int, [P(GlovePairs), P(GlovePairs), vp, i64, i64, C.c_uint64, C.c_uint64, P(GlovePairs),
                                       P(GlovePairs), vp, sz, vp]),
        "glove_plan_sorted_workspace_bytes": (sz, [i64, i32]),
        "glove_plan_chunk_bound": (i32, [i64, i32, i32]),
        "glove_plan_build_sorted": (C.c_int, [P(GlovePairs), P(GlovePairs), i64, i64, i32, i32, P(GlovePlan), vp, vp, sz, vp]),
        "glove_step_workspace_bytes": (sz, [i64, i32, i32]),
        "glove_passes_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp]),
        "glove_rowpass_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp]),
        "glove_colpass_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp]),
        "glove_apply_adagrad_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, vp]),
        "glove_dense_grad_layout": (sz, [i32, i32, i32, vp]),
        "glove_dense_grad_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, vp]),
        "glove_dense_adagrad_f32": (C.c_int, [P(GloveTables), P(GloveHyper), vp, vp, vp]),
        "glove_dense_adam_f32": (C.c_int, [P(GloveTables), P(GloveHyper), vp, vp, vp]),
        "glove_step_adagrad_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, vp]),
        "glove_steps_adagrad_f32": (C.c_int, [P(P(GlovePlan)), i32, P(GloveTables), P(GloveHyper), vp, sz, vp, vp]),
        "glove_step_adam_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, vp, vp]),
        "glove_step_sparse_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, vp, vp]),
        "glove_steps_adam_f32": (C.c_int, [P(P(GlovePlan)), i32, P(GloveTables), P(GloveHyper), vp, sz, vp, vp, vp]),
        "glove_pack_grad_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, i64, vp]),
        "glove_passes_packing_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, i64, vp]),
        "glove_pack_rest_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, i64, vp]),
        "glove_loss_partials_f32": (C.c_int, [P(GlovePlan), P(GloveTables), vp, sz, vp, vp]),
        "glove_combine_packed_f32": (C.c_int, [P(GlovePackedList), i32, P(GloveTables), vp, vp, i64, vp]),
        "glove_count_packed_f32": (C.c_int, [P(GlovePackedList), i32, P(GloveTables), vp, vp, i64, vp]),
        "glove_apply_packed_adagrad_f32": (C.c_int, [P(GlovePackedList), i32, P(GloveTables), P(GloveHyper), vp, vp, vp, vp, i64, vp]),
        "glove_gather_rows_f32": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp]),
        "glove_canonicalize_f32": (C.c_int, [P(GloveTables), vp]),
        "glove_rowside_step_adagrad_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp]),
        "glove_rowside_step_f32": (C.c_int, [P(GlovePlan), P(GloveTables), P(GloveHyper), vp, sz, vp, vp]),
        "glove_eval_f32": (C.c_int, [vp, vp, vp, vp, i64, P(GloveTables), vp, vp]),
        "glove_eval_logistic_f32": (C.c_int, [vp, vp, vp, vp, i64, P(GloveTables), vp, vp]),
        "glove_topk_workspace_bytes": (sz, [i32, i32, i32]),
        "glove_topk_cosine_f32": (C.c_int, [vp, i32, i32, vp, i32, i32, vp, vp, vp, sz, vp]),
        "glove_cooc_workspace_bytes": (sz, [i64, i32]),
        "glove_cooccurrence_i32": (C.c_int, [vp, i64, i32, i32, vp, vp, vp, vp, vp, i64, vp, sz, vp]),
    }
    lib = _open(Path(path) if path else LIB_PATH, protos, optional=bool(path and any_abi))
    if lib.glove_abi_version() != GLOVE_ABI_VERSION and not (path and any_abi):
        raise GloveHipError("ABI mismatch: library %d, binding %d" % (lib.glove_abi_version(), GLOVE_ABI_VERSION))
    if path is None:
        _lib = lib
    return lib


_eval_lib = None


def eval_cross_prototypes() -> dict:
    """name -> (result, arguments) of every function include/glove_eval_cross_hip.h declares."""
    sz, i32, vp = C.c_size_t, C.c_int32, C.c_void_p
    return {
        "glove_eval_cross_abi_version": (C.c_int, []),
        "glove_cross_topk_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "glove_cross_topk_f32": (C.c_int, [vp, i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
        "glove_topk_mean_f32": (C.c_int, [vp, i32, i32, vp, vp]),
    }


def load_eval_library(path: os.PathLike | None = None) -> C.CDLL:
    """dlopen libglove_eval_hip.so (include/glove_eval_hip.h, include/glove_eval_sim_hip.h, include/glove_eval_cluster_hip.h,
    include/glove_eval_cross_hip.h) and declare the prototypes, at the first call that needs it:
    training never loads it.  Raises if it is not built, like load_library."""
    global _eval_lib
    if _eval_lib is not None and path is None:
        return _eval_lib
    sz, i32, vp = C.c_size_t, C.c_int32, C.c_void_p
    protos = {
        "glove_eval_abi_version": (C.c_int, []),
        "glove_analogy_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "glove_analogy_topk_f32": (C.c_int, [vp, i32, i32, vp, i32, i32, vp, vp, vp, sz, vp]),
        "glove_eval_sim_abi_version": (C.c_int, []),
        "glove_cosmul_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "glove_cosmul_topk_f32": (C.c_int, [vp, i32, i32, vp, i32, i32, C.c_float, vp, vp, vp, sz, vp]),
        "glove_pair_cosine_f32": (C.c_int, [vp, i32, i32, vp, i32, vp, vp]),
        "glove_eval_cluster_abi_version": (C.c_int, []),
        "glove_kmeans_workspace_bytes": (sz, [i32, i32, i32, i32]),
        "glove_kmeans_assign_f32": (C.c_int, [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, sz, vp]),
        "glove_kmeans_update_f32": (C.c_int, [vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, sz, vp]),
    }
    protos.update(eval_cross_prototypes())
    lib = _open(Path(path) if path else EVAL_LIB_PATH, protos)
    if lib.glove_eval_abi_version() != GLOVE_EVAL_ABI_VERSION:
        raise GloveHipError("ABI mismatch: eval library %d, binding %d" % (lib.glove_eval_abi_version(), GLOVE_EVAL_ABI_VERSION))
    if lib.glove_eval_sim_abi_version() != GLOVE_EVAL_SIM_ABI_VERSION:
        raise GloveHipError("ABI mismatch: eval library (similarity entry points) %d, binding %d"
                            % (lib.glove_eval_sim_abi_version(), GLOVE_EVAL_SIM_ABI_VERSION))
    if lib.glove_eval_cluster_abi_version() != GLOVE_EVAL_CLUSTER_ABI_VERSION:
        raise GloveHipError("ABI mismatch: eval library (clustering entry points) %d, binding %d"
                            % (lib.glove_eval_cluster_abi_version(), GLOVE_EVAL_CLUSTER_ABI_VERSION))
    if lib.glove_eval_cross_abi_version() != GLOVE_EVAL_CROSS_ABI_VERSION:
        raise GloveHipError("ABI mismatch: eval library (cross-table entry points) %d, binding %d"
                            % (lib.glove_eval_cross_abi_version(), GLOVE_EVAL_CROSS_ABI_VERSION))
    if path is None:
        _eval_lib = lib
    return lib


_prep_lib = None


def load_prep_library(path: os.PathLike | None = None) -> C.CDLL:
    """dlopen libglove_prep_hip.so (include/glove_cooc_stream_hip.h, include/glove_text_hip.h, include/glove_vectors_hip.h, include/glove_cooc_options_hip.h, include/glove_phrases_hip.h) and declare the prototypes, at the first call that needs
    it: training never loads it.  Raises if it is not built, like load_library."""
    global _prep_lib
    if _prep_lib is not None and path is None:
        return _prep_lib
    sz, i32, i64, vp = C.c_size_t, C.c_int32, C.c_int64, C.c_void_p
    protos = {
        "glove_cooc_stream_abi_version": (C.c_int, []),
        "glove_cooc_chunk_workspace_bytes": (sz, [i64, i32]),
        "glove_cooc_chunk_keys_i32": (C.c_int, [vp, i64, i64, i32, i32, vp, vp, vp, i64, vp, sz, vp]),
        "glove_cooc_merge_workspace_bytes": (sz, [i64, i64]),
        "glove_cooc_merge_u64": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, sz, vp]),
        "glove_cooc_finalize_workspace_bytes": (sz, [i64]),
        "glove_cooc_finalize": (C.c_int, [vp, vp, vp, i64, i32, i32, i64, vp, vp, vp, vp, vp, i64, vp, sz, vp]),
        "glove_text_abi_version": (C.c_int, []),
        "glove_text_tokenize_workspace_bytes": (sz, [i64]),
        "glove_text_tokenize_u8": (C.c_int, [vp, i64, vp, vp, vp, vp, vp, i64, vp, sz, vp]),
        "glove_text_block_vocab_workspace_bytes": (sz, [i64]),
        "glove_text_block_vocab": (C.c_int, [vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, i64, vp, sz, vp]),
        "glove_text_vocab_merge_workspace_bytes": (sz, [i64, i64]),
        "glove_text_vocab_merge": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, sz, vp]),
        "glove_text_token_ids_i32": (C.c_int, [vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp]),
        "glove_vectors_abi_version": (C.c_int, []),
        "glove_vectors_lines_workspace_bytes": (sz, [i64, i64]),
        "glove_vectors_lines_u8": (C.c_int, [vp, i64, vp, vp, vp, i64, vp, sz, vp]),
        "glove_vectors_parse_f32": (C.c_int, [vp, i64, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
        "glove_vectors_format_workspace_bytes": (sz, [i64, i32]),
        "glove_vectors_format_f32": (C.c_int, [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp, sz, vp]),
        "glove_cooc_options_abi_version": (C.c_int, []),
        "glove_token_filter_workspace_bytes": (sz, [i64]),
        "glove_token_filter_i32": (C.c_int, [vp, i64, i64, vp, i32, C.c_uint64, vp, vp, i64, vp, sz, vp]),
        "glove_cooc_finalize_weighted_workspace_bytes": (sz, [i64]),
        "glove_cooc_finalize_weighted": (C.c_int, [vp, vp, vp, i64, i32, i32, i64, i32, vp, vp, vp, vp, vp, i64, vp, sz, vp]),
        "glove_phrases_abi_version": (C.c_int, []),
        "glove_phrase_bigram_workspace_bytes": (sz, [i64]),
        "glove_phrase_bigram_keys_i32": (C.c_int, [vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, sz, vp]),
        "glove_phrase_select_workspace_bytes": (sz, [i64]),
        "glove_phrase_select": (C.c_int, [vp, vp, vp, i64, vp, i32, i64, i64, C.c_double, vp, vp, vp, vp, i64, vp, sz, vp]),
        "glove_phrase_join_workspace_bytes": (sz, [i64]),
        "glove_phrase_join_u8": (C.c_int, [vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, i32, vp, vp, vp, vp, sz, vp]),
    }
    lib = _open(Path(path) if path else PREP_LIB_PATH, protos)
    if lib.glove_cooc_stream_abi_version() != GLOVE_COOC_STREAM_ABI_VERSION:
        raise GloveHipError("ABI mismatch: prep library %d, binding %d"
                            % (lib.glove_cooc_stream_abi_version(), GLOVE_COOC_STREAM_ABI_VERSION))
    if lib.glove_text_abi_version() != GLOVE_TEXT_ABI_VERSION:
        raise GloveHipError("ABI mismatch: prep library (text entry points) %d, binding %d"
                            % (lib.glove_text_abi_version(), GLOVE_TEXT_ABI_VERSION))
    if lib.glove_vectors_abi_version() != GLOVE_VECTORS_ABI_VERSION:
        raise GloveHipError("ABI mismatch: prep library (word-vector entry points) %d, binding %d"
                            % (lib.glove_vectors_abi_version(), GLOVE_VECTORS_ABI_VERSION))
    if lib.glove_cooc_options_abi_version() != GLOVE_COOC_OPTIONS_ABI_VERSION:
        raise GloveHipError("ABI mismatch: prep library (counting-option entry points) %d, binding %d"
                            % (lib.glove_cooc_options_abi_version(), GLOVE_COOC_OPTIONS_ABI_VERSION))
    if lib.glove_phrases_abi_version() != GLOVE_PHRASES_ABI_VERSION:
        raise GloveHipError("ABI mismatch: prep library (phrase entry points) %d, binding %d"
                            % (lib.glove_phrases_abi_version(), GLOVE_PHRASES_ABI_VERSION))
    if path is None:
        _prep_lib = lib
    return lib


_factor_lib = None


def factor_prototypes() -> dict:
    """name -> (result, arguments) of every function include/glove_factor_hip.h declares."""
    sz, i32, i64, vp, f64 = C.c_size_t, C.c_int32, C.c_int64, C.c_void_p, C.c_double
    return {
        "glove_factor_abi_version": (C.c_int, []),
        "glove_csr_spmm_workspace_bytes": (sz, [i32, i64, i32]),
        "glove_csr_spmm_f32": (C.c_int, [vp, vp, vp, i32, i32, i64, vp, i32, vp, vp, sz, vp]),
        "glove_csr_row_sums_f64": (C.c_int, [vp, vp, i32, i64, vp, vp, sz, vp]),
        "glove_coo_reweight_f32": (C.c_int, [vp, vp, vp, i64, i32, vp, vp, f64, f64, vp, vp]),
    }


def factor_dense_prototypes() -> dict:
    """name -> (result, arguments) of every function include/glove_factor_dense_hip.h declares."""
    sz, i32, i64, vp = C.c_size_t, C.c_int32, C.c_int64, C.c_void_p
    return {
        "glove_factor_dense_abi_version": (C.c_int, []),
        "glove_gram_workspace_bytes": (sz, [i64, i32]),
        "glove_col_sums_f64": (C.c_int, [vp, i64, i32, vp, vp, sz, vp]),
        "glove_gram_f64": (C.c_int, [vp, i64, i32, vp, vp, vp, sz, vp]),
        "glove_rows_transform_f32": (C.c_int, [vp, i64, i32, vp, i32, vp, vp, vp]),
    }


def factor_graph_prototypes() -> dict:
    """name -> (result, arguments) of every function include/glove_factor_graph_hip.h declares."""
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    return {
        "glove_factor_graph_abi_version": (C.c_int, []),
        "glove_retrofit_rows_f32": (C.c_int, [vp, vp, vp, i32, i64, vp, i32, vp, vp, vp, i32, C.c_float, vp]),
    }


def factor_align_prototypes() -> dict:
    """name -> (result, arguments) of every function include/glove_factor_align_hip.h declares."""
    sz, i32, i64, vp = C.c_size_t, C.c_int32, C.c_int64, C.c_void_p
    return {
        "glove_factor_align_abi_version": (C.c_int, []),
        "glove_cross_gram_workspace_bytes": (sz, [i64, i32]),
        "glove_cross_gram_f64": (C.c_int, [vp, i32, vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, sz, vp]),
    }


def load_factor_library(path: os.PathLike | None = None) -> C.CDLL:
    """dlopen libglove_factor_hip.so (include/glove_factor_hip.h, include/glove_factor_dense_hip.h,
    include/glove_factor_graph_hip.h, include/glove_factor_align_hip.h) and declare the
    prototypes, at the first call that needs it: training never loads it.  Raises if it is not built, like load_library."""
    global _factor_lib
    if _factor_lib is not None and path is None:
        return _factor_lib
    lib = _open(Path(path) if path else FACTOR_LIB_PATH,
                dict(factor_prototypes(), **factor_dense_prototypes(), **factor_graph_prototypes(),
                     **factor_align_prototypes()))
    if lib.glove_factor_abi_version() != GLOVE_FACTOR_ABI_VERSION:
        raise GloveHipError("ABI mismatch: factor library %d, binding %d"
                            % (lib.glove_factor_abi_version(), GLOVE_FACTOR_ABI_VERSION))
    if lib.glove_factor_dense_abi_version() != GLOVE_FACTOR_DENSE_ABI_VERSION:
        raise GloveHipError("ABI mismatch: factor library (dense entry points) %d, binding %d"
                            % (lib.glove_factor_dense_abi_version(), GLOVE_FACTOR_DENSE_ABI_VERSION))
    if lib.glove_factor_graph_abi_version() != GLOVE_FACTOR_GRAPH_ABI_VERSION:
        raise GloveHipError("ABI mismatch: factor library (graph entry points) %d, binding %d"
                            % (lib.glove_factor_graph_abi_version(), GLOVE_FACTOR_GRAPH_ABI_VERSION))
    if lib.glove_factor_align_abi_version() != GLOVE_FACTOR_ALIGN_ABI_VERSION:
        raise GloveHipError("ABI mismatch: factor library (alignment entry points) %d, binding %d"
                            % (lib.glove_factor_align_abi_version(), GLOVE_FACTOR_ALIGN_ABI_VERSION))
    if path is None:
        _factor_lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        names = {-1: "GLOVE_E_BADARG", -2: "GLOVE_E_WORKSPACE"}
        raise GloveHipError("%s failed: %s" % (what, names.get(rc, "hipError %d" % rc)))


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise GloveHipError("device tensor expected (the HIP path has no CPU fallback)")


def _require(t, dtype, n=None):
    """The kernels read raw pointers: a wrong dtype (torch's default int64 ids), a strided view or a short buffer
    would be silently misread."""
    if t is None:
        return
    if not t.is_cuda:
        raise GloveHipError("device tensor expected (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise GloveHipError("expected a %s tensor, got %s" % (dtype, t.dtype))
    if not t.is_contiguous():
        raise GloveHipError("expected a contiguous tensor")
    if n is not None and t.numel() != n:
        raise GloveHipError("expected %d elements, got %d" % (n, t.numel()))


def row_width(rows: int, d: int) -> int:
    """Floats per stored table row (the row stride the kernels take) for an embedding size `d`: rows start on 16-byte
    boundaries at least; when the padding costs at most d / 12 floats they start on 64-byte boundaries, and on 128-byte lines
    for tables beyond the Infinity Cache (>= 128 MB: what the fused twin form also looks at).  d = 300: 304 floats (1,216 B =
    19 x 64) on a 60 MB table, 320 (1,280 B = 10 lines) on a 480 MB one; 64 and 128 stay as they are, 50 becomes 52.
    Measured on the same batches (tools/exp_row_stride.py, one process): V = 400 k, B = 1 M: 1,200-byte rows 622 - 628 us per step,
    1,216 B 608 - 609, 1,280 B 602 — 6.7 % more bytes per row and 3.7 % less time: rows that start mid-line cost two partial
    lines per access, on the write side two partial write-backs; V = 50 k (cache-resident): 101.5 / 99.8 - 100.4 / 101.7 - 103.0.
    The padding columns are zero and stay zero (glove_tables.d_model keeps lambda / d on the model's size)."""
    base = (int(d) + 3) // 4 * 4
    if os.environ.get("GLOVE_ROW_ALIGN") == "4":        # experiments (tools/): the former rule
        return base
    for align, ok in ((32, int(rows) * int(d) * 4 >= (128 << 20)), (16, True)):
        cand = (int(d) + align - 1) // align * align
        if ok and cand - int(d) <= int(d) // 12:
            return cand
    return base


def _plain_view(name, rows):
    """DeviceTables.R / br / C / bc: see there."""
    def get(self) -> torch.Tensor:
        self.canonicalize()
        return getattr(self, "_" + name)[:getattr(self, rows)]

    def put(self, value):               # `tables.R += x` and `tables.R = tensor` write into the buffer the kernels see
        view = get(self)
        if value.data_ptr() != view.data_ptr():
            view.copy_(value)
    return property(get, put)


class DeviceTables:
    """The five variables + optimizer slots as device buffers (reference model_utils.py:31-39)."""

    NAMES = ("R", "C", "br", "bc")

    def __init__(self, V: int, d: int, optimizer: str, device="cuda:0", seed: int | None = None,
                 V_row: int | None = None, V_col: int | None = None):
        """`d`: --embedding-size, any positive int.  Rows are stored aligned: `self.d` is the row stride
        (`row_width`: d rounded up to a multiple of 4, 16 or 32 floats — what the kernels and workspace queries take),
        `self.d_model` the reference's embedding size; the padding columns are zero and stay zero (glove_tables.d_model).
        `V_row` < V: this process holds only a shard of the row table (row ids handed to the kernels
        are then local indices into the shard).  `V_col` < V: it also holds only a shard of the col table
        (trainer.stepper.ShardedStepper, which runs the passes against fetched col rows); such tables go through
        TablesView, the plain kernels expect V col rows."""
        if d <= 0:
            raise ValueError("embedding size must be positive, got %d" % d)
        if optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be one of %s (Keras names), got %r" % (", ".join(OPTIMIZERS), optimizer))
        self.V, self.d_model, self.optimizer, self.device = int(V), int(d), optimizer, torch.device(device)
        self.V_row = int(V if V_row is None else V_row)
        self.V_col = int(V if V_col is None else V_col)
        self.d = row_width(self.V, d)        # (by the whole vocabulary, not this rank's shard: every rank takes the same stride)
        if not 0 < self.V_row <= self.V or not 0 < self.V_col <= self.V:
            raise ValueError("V_row and V_col must be in (0, V]")
        gen = torch.Generator(device="cpu")
        if seed is not None:
            gen.manual_seed(seed)
        else:
            gen.seed()   # the reference is unseeded (train_utils.py:26-27)

        def uni(*shape):  # Keras Embedding default: U(-0.05, 0.05)
            return ((torch.rand(*shape, generator=gen, dtype=torch.float32) - 0.5) * 0.1).to(self.device)

        def table(rows):
            t = torch.zeros(rows, self.d, dtype=torch.float32, device=self.device)
            t[:, :self.d_model] = uni(rows, self.d_model)
            return t

        self._R, self._C = table(self.V_row), table(self.V_col)
        self._br, self._bc = uni(self.V_row), uni(self.V_col)
        self.R_ver = None           # uint8[V_row] once enable_twin() has doubled R and br (glove_tables.R_ver)
        self.R_tag = self.C_tag = None    # once enable_tags() has doubled both tables (glove_tables.R_tag)
        spec = OPTIMIZERS[optimizer]                   # the slot layout and the scalars at step 0: the name's record
        self.scalars = torch.tensor(spec.scalars, dtype=torch.float32, device=self.device)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.s1, self.s2 = {}, {}
        for n in self.NAMES:
            w = getattr(self, n)
            # (row-wise: one accumulator per row — float[rows] for R and C as for br and bc)
            self.s1[n] = torch.full(w.shape[:1] if spec.row_wise else w.shape, spec.slot1_init, dtype=torch.float32, device=self.device)
            if spec.slot2:
                self.s2[n] = torch.zeros_like(w)
        self._struct = None

    # ---- the row table may be twinned (glove_tables.R_ver): R / br are the plain views [V_row, ...]; reading them
    # (or handing the tables to anything but the Adagrad step) first brings the table back to its plain form
    R, br = _plain_view("R", "V_row"), _plain_view("br", "V_row")
    C, bc = _plain_view("C", "V_col"), _plain_view("bc", "V_col")

    def enable_tags(self):
        """Second copies of BOTH tables + a step tag per row (glove_tables.R_tag / C_tag): what the tagged step
        (GLOVE_STEP_TAGGED) needs to read pre-step rows while it updates rows in the same launch.  For the latency-bound
        regime — small tables: costs (V_row + V) x d x 4 B of HBM."""
        if self.R_tag is not None or not OPTIMIZERS[self.optimizer].tagged or self.R_ver is not None:
            return                               # (Adam: the twins flip as a whole every step — scalars[3] —, the tags stay zero)
        if self.V_col != self.V or 2 * max(self.V_row, self.V) * self.d * 4 >= 1 << 32:
            return                               # a sharded col table goes through views; 32-bit row offsets
        for name in ("_R", "_br", "_C", "_bc"):
            old = getattr(self, name)
            new = torch.zeros((2 * old.shape[0],) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
            new[:old.shape[0]].copy_(old)
            setattr(self, name, new)
        self.R_tag = torch.zeros(self.V_row, dtype=torch.int64, device=self.device)
        self.C_tag = torch.zeros(self.V, dtype=torch.int64, device=self.device)
        self._struct = None

    def maybe_enable_tags(self, batch_size: int):
        """The policy: batches the library steps in the tagged form (at most TAGGED_STEP_MAX_BATCH pairs) on tables small enough
        that the step is a latency chain (both tables within the caches: 64 MB)."""
        small = batch_size <= TAGGED_STEP_MAX_BATCH and (self.V_row + self.V) * self.d * 4 <= (64 << 20)
        spec = OPTIMIZERS[self.optimizer]
        if small and spec.tagged and (not spec.tagged_sweeps or 2 * batch_size <= self.V_row + self.V):
            self.enable_tags()

    def enable_twin(self):
        """Second copy of the row table + per-row version bytes: lets the fused step write a row's update beside the old
        row instead of through a partial-row slot (GLOVE_STEP_FUSED_TWIN).  Costs V_row x d x 4 B of HBM."""
        if self.R_ver is not None or not OPTIMIZERS[self.optimizer].twinned or self.R_tag is not None:
            return
        if 2 * self.V_row * self.d * 4 >= 1 << 32:
            return                               # 32-bit row offsets: the table cannot be doubled
        for name in ("_R", "_br"):
            old = getattr(self, name)
            new = torch.zeros((2 * old.shape[0],) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
            new[:old.shape[0]].copy_(old)
            setattr(self, name, new)
        self.R_ver = torch.zeros(self.V_row, dtype=torch.uint8, device=self.device)
        self._struct = None

    def maybe_enable_twin(self):
        """The policy: row tables of 32 MB and more — where batches reach the fused step's regime — get the twin (128 MB until round 5).
        Measured per step, three-launch form -> twin form with its id triage: V = 400 k, d = 300: 678 -> 627 us;
        V = 2 M, d = 128: 578 -> 539 us (the passes pay ~20 us each for looking up which copy of a row is current, the
        apply launch shrinks from 95 to 15 us); V = 50 k, d = 300 (Infinity-Cache resident): no gain, not enabled."""
        # (round 4, tools/ab_step_forms.py: on the 61 MB table of V = 50 k, d = 300 — Infinity-Cache resident — the three-launch
        # form beats the twin form 101.0 to 103.2 us; on tables beyond the cache the twin form wins by 4 - 11 %)
        # (round 5: without a triage launch — the list of unfinished ids rides in the col-side launch — and without the streaming
        # cache policy on tables the caches hold, the twin form also wins on the 61 MB table: V = 50 k, d = 300, B = 131,072
        # 96.2 -> 92.9 us per step, B = 65,536 64.9 -> 64.4, B = 1 M 295.0 -> 292.6: tools/ab_step_forms.py,
        # profiles/r05_exp_twin_form_on_cache_resident_tables.txt; below 32 MB nothing was measured: not enabled)
        if OPTIMIZERS[self.optimizer].twinned and self.V_row * self.d * 4 >= (32 << 20):
            self.enable_twin()

    def canonicalize(self):
        """Versions back to 0 (a no-op without a twin; one sweep over V_row bytes plus the rows whose second copy was
        current).  Called by every accessor except the Adagrad step's."""
        # `_twin_dirty` is sticky: once a step that may flip versions has been issued (possibly inside a captured graph
        # that is replayed without any further Python call), every reader pays this one small launch
        if (self.R_ver is not None or self.R_tag is not None) and getattr(self, "_twin_dirty", False):
            _check(load_library().glove_canonicalize_f32(C.byref(self.struct(twin_ok=True)), _stream()),
                   "glove_canonicalize_f32")

    def struct(self, twin_ok=False) -> GloveTables:
        """`twin_ok`: the caller is the Adagrad step, which understands a twinned table (and says so through
        `_twin_dirty` when it may leave one behind: GloveHip.step_adagrad)."""
        if not twin_ok:
            self.canonicalize()
        if self._struct is None:
            s = GloveTables()
            s.V, s.d, s.V_row = self.V, self.d, (0 if self.V_row == self.V else self.V_row)
            s.d_model = 0 if self.d_model == self.d else self.d_model
            for n in self.NAMES:
                setattr(s, n, _ptr(getattr(self, "_" + n)))
                setattr(s, "s1_" + n, _ptr(self.s1[n]))
                setattr(s, "s2_" + n, _ptr(self.s2.get(n)))
            s.scalars, s.step, s.R_ver = _ptr(self.scalars), _ptr(self.step), _ptr(self.R_ver)
            s.R_tag, s.C_tag = _ptr(self.R_tag), _ptr(self.C_tag)
            self._struct = s
        return self._struct

    def embeddings(self, name: str) -> torch.Tensor:
        """R or C without the alignment padding: [rows, d_model] (a view)."""
        return getattr(self, name)[:, :self.d_model]

    # ---- (de)serialisation used by the checkpoint code and the tests: logical shapes [rows, d_model]
    # (a slot need not be shaped like its variable: RowWiseAdagrad's slot 1 of R and C is float[rows] — 1-D arrays pass whole)
    def _logical(self, x):
        return (x[:, :self.d_model] if x.dim() == 2 else x).cpu()

    def _store(self, dst, src):
        if dst.dim() == 2:
            dst[:, :self.d_model].copy_(src)
        else:
            dst.copy_(src)

    def state_dict(self) -> dict:
        self.canonicalize()             # (also settles scalars[3], the current copy of tables the one-launch Adam step flips)
        out = {"V": self.V, "d": self.d_model, "V_row": self.V_row, "optimizer": self.optimizer,
               "scalars": self.scalars.cpu(), "global_step": self.step.cpu()}
        for n in self.NAMES:
            out[n] = self._logical(getattr(self, n))
            out["slot1_" + n] = self._logical(self.s1[n])
            if n in self.s2:
                out["slot2_" + n] = self._logical(self.s2[n])
        return out

    def load_state_dict(self, sd: dict):
        if (sd["V"], sd["d"], sd["optimizer"], sd.get("V_row", sd["V"])) != (self.V, self.d_model, self.optimizer, self.V_row):
            raise ValueError("checkpoint is for V=%s d=%s %s, model is V=%d d=%d %s" % (
                sd["V"], sd["d"], sd["optimizer"], self.V, self.d_model, self.optimizer))
        self.canonicalize()
        self.scalars.copy_(sd["scalars"])
        self.step.copy_(sd["global_step"])
        for n in self.NAMES:
            self._store(getattr(self, n), sd[n])
            self._store(self.s1[n], sd["slot1_" + n])
            if n in self.s2:
                self._store(self.s2[n], sd["slot2_" + n])

    # ---- row-sharded tables (BASELINE config 5): row u lives on rank u % world at local index u // world
    ROW_SIDE = ("R", "br")

    COL_SIDE = ("C", "bc")

    def _sharded_names(self):
        return self.ROW_SIDE + (self.COL_SIDE if self.V_col < self.V else ())

    def gather_whole(self, x, dist, world: int):
        """A table sharded by id % world (this rank's shard `x`) as the whole [V, ...] array, on every rank (collective)."""
        per = (self.V + world - 1) // world
        pad = torch.zeros((per,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        pad[:x.shape[0]] = x
        parts = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(parts, pad)
        return torch.stack(parts, 1).reshape((per * world,) + tuple(x.shape[1:]))[:self.V]

    def gather_by_owner(self, x, dist, world: int):
        """A table sharded by id % world as [world * ceil(V / world), ...]: rank after rank, each shard padded to the same
        length — row (v % world) * per + v // world holds id v (the numbering of NonzeroStream(cols_by_owner=world))."""
        per = (self.V + world - 1) // world
        pad = torch.zeros((per,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        pad[:x.shape[0]] = x
        parts = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(parts, pad)
        return torch.cat(parts, 0)

    def gathered_state_dict(self, dist, world: int, relabel=None) -> dict:
        """state_dict() of the WHOLE model: the shards of all ranks (the row side; the col side too when it is sharded) are
        all-gathered and interleaved back into [V, ...] arrays, so the checkpoint has the same format as an unsharded
        run's (collective).
        `relabel`: int64[V], the bijection the run's ids were renamed by (trainer.owner_map): row relabel[u] of every table
        here — sharded or replicated — is token u; the dict comes out in vocabulary order (row u is token u), as it always is."""
        out = self.state_dict()
        out["V_row"] = self.V
        sharded = self._sharded_names()
        names = None if relabel is None else self._relabel_index(relabel)
        for n in (sharded if names is None else self.NAMES):
            for key, x in ((n, getattr(self, n)), ("slot1_" + n, self.s1[n]), ("slot2_" + n, self.s2.get(n))):
                if x is None:
                    continue
                whole = self._logical(self.gather_whole(x, dist, world) if n in sharded else x)
                out[key] = whole if names is None else whole[names]
        return out

    def load_whole_state_dict(self, sd: dict, world: int, rank: int, relabel=None):
        """Takes this rank's rows out of a whole-model state dict (the inverse of gathered_state_dict).
        `relabel`: the bijection this run's ids are renamed by: token u goes to row relabel[u] of every table, and the shard
        is cut from that order."""
        if sd.get("V_row", sd["V"]) != sd["V"]:
            raise ValueError("the checkpoint holds a row shard, not the whole model")
        mine = dict(sd, V_row=self.V_row)
        sharded = self._sharded_names()
        tokens = None
        if relabel is not None:
            names = self._relabel_index(relabel)
            tokens = torch.empty_like(names)
            tokens[names] = torch.arange(self.V, dtype=torch.int64)        # row p holds token tokens[p]
        for n in (sharded if tokens is None else self.NAMES):
            for key in (n, "slot1_" + n, "slot2_" + n):
                if key in sd:
                    whole = sd[key] if tokens is None else sd[key][tokens]
                    mine[key] = whole[rank::world] if n in sharded else whole
        self.load_state_dict(mine)

    def _relabel_index(self, relabel) -> torch.Tensor:
        names = torch.as_tensor(relabel, dtype=torch.int64).cpu()
        if names.numel() != self.V:
            raise ValueError("relabel names %d ids, the vocabulary has %d" % (names.numel(), self.V))
        return names

    @property
    def global_bias(self) -> float:
        return float(self.scalars[0].item())

    @property
    def global_step(self) -> int:
        return int(self.step.item())


class TablesView:
    """A glove_tables struct over buffers picked by the caller: the tables of `base` with some of them replaced
    (a fetched block as the col table, a col shard standing on the row side, ...).  Offers what the wrappers use:
    struct(), d, V, V_row, device, optimizer."""

    def __init__(self, base: "DeviceTables", V: int, V_row: int, keep=(), **replace):
        self.d, self.d_model, self.device, self.optimizer = base.d, base.d_model, base.device, base.optimizer
        self.V, self.V_row = int(V), int(V_row)
        self._keep = (base, keep, replace)                      # the struct holds raw pointers: keep the owners alive
        src = base.struct()
        s = GloveTables()
        for name, _ in GloveTables._fields_:
            setattr(s, name, getattr(src, name))
        s.V, s.V_row = self.V, (0 if self.V_row == self.V else self.V_row)
        s.R_ver = s.R_tag = s.C_tag = None            # views are plain: base.struct() above made the tables canonical
        for name, tensor in replace.items():
            _require(tensor, torch.float32)
            setattr(s, name, tensor.data_ptr())
        self._struct = s

    def struct(self) -> GloveTables:
        return self._struct


class Plan:
    """Device-resident dedup index of one batch (see glove_plan in include/glove_hip.h)."""

    INT_FIELDS = ("r_partner", "r_to_c", "r_chunk_id", "r_chunk_start", "r_uniq_slot", "r_uniq_rec",
                  "c_partner", "c_perm", "c_chunk_id", "c_chunk_start", "c_uniq_slot", "c_uniq_rec", "heavy")

    def __init__(self, B: int, V: int, chunk_cap: int, device, cap_chunks: int | None = None,
                 cap_uniq: int | None = None, V_row: int = 0, records: bool | None = None, links: bool = True,
                 own_pairs: bool = True, run_words: bool = False, _no_pairs_ok: bool = False):
        """`own_pairs=False` (a plan with chunk records that glove_plan_build_sorted refills from a dealt epoch): no pair
        arrays of its own — the records carry partner / w / y, the step functions read nothing else."""
        self.B, self.V, self.chunk_cap, self.V_row = int(B), int(V), int(chunk_cap), int(V_row or 0)
        self.cap_chunks = int(B if cap_chunks is None else cap_chunks)
        self.cap_uniq = int(min(B, V) if cap_uniq is None else cap_uniq)
        dev = torch.device(device)
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        n = max(self.B, 1)
        self.heavy_chunks = HEAVY_CHUNKS
        self.cap_heavy = 2 * self.B // (self.heavy_chunks * self.chunk_cap) + 2
        self.counts = torch.zeros(8, **i32)
        self.host_counts = [-1] * 8      # unknown until the build has been synchronised
        self.heavy = torch.zeros(self.cap_heavy, **i32)
        # per-chunk records: carried by small (per-step) plans right away, added to big ones when compacted
        # (`records=True`: a staging plan of a big batch on big tables, refilled every step and stepped in a fused form)
        self.r_crec = self.c_crec = None
        if self.B > 0 and (self.B <= RECORDS_AT_BUILD_MAX if records is None else records):
            # (uninitialised: a build writes every record slot a step reads — the poisoned-plan tests — and a capacity-sized
            # record array is hundreds of MB per side at B = 1 M: zero-filling it cost more than the build)
            self.r_crec, self.c_crec = (torch.empty(self.cap_chunks * self.rec_dwords, **i32) for _ in range(2))
        if not own_pairs and self.r_crec is None and not _no_pairs_ok:
            raise ValueError("a plan without pair arrays of its own needs chunk records")
        self.r_partner, self.c_partner = (torch.empty(n, **i32), torch.empty(n, **i32)) if own_pairs else (None, None)
        # c_perm / r_to_c link the two sorted orders; no kernel reads them: `links=False` (the per-step plans of a
        # reshuffled epoch) leaves them out and the build skips the join of its two sorts
        self.r_to_c, self.c_perm = (torch.empty(n, **i32), torch.empty(n, **i32)) if links else (None, None)
        self.r_w, self.r_y = (torch.empty(n, **f32), torch.empty(n, **f32)) if own_pairs else (None, None)
        self.c_w, self.c_y = (torch.empty(n, **f32), torch.empty(n, **f32)) if own_pairs else (None, None)
        self.r_chunk_id, self.c_chunk_id = (torch.empty(max(self.cap_chunks, 1), **i32) for _ in range(2))
        self.r_chunk_start, self.c_chunk_start = (torch.zeros(self.cap_chunks + 1, **i32) for _ in range(2))
        self.r_uniq_slot, self.c_uniq_slot = (torch.zeros(self.cap_uniq + 1, **i32) for _ in range(2))
        self.r_uniq_rec, self.c_uniq_rec = (torch.zeros(4 * max(self.cap_uniq, 1), **i32) for _ in range(2))
        # bitmaps of the batch's ids (glove_plan.r_mark / c_mark): small batches carry them — the one-launch Adam step's sweep
        # over all rows leaves the batch's rows alone by them
        # per-chunk run words (glove_plan.r_chunk_hw): the fused step forms on a plan that keeps pair arrays instead of records
        self.r_chunk_hw = self.c_chunk_hw = None
        if run_words:
            self.r_chunk_hw, self.c_chunk_hw = (torch.zeros(max(self.cap_chunks, 1), **i32) for _ in range(2))
        self.r_mark = self.c_mark = None
        if 0 < self.B <= TAGGED_STEP_MAX_BATCH:
            self.r_mark = torch.zeros(((max(self.V_row, 0) or self.V) + 31) // 32, **i32)
            self.c_mark = torch.zeros((self.V + 31) // 32, **i32)
        self._struct = None

    @property
    def fusable(self) -> bool:
        """The plan carries what the fused step forms read the id layout from: chunk records, or run words beside pair arrays."""
        return self.r_crec is not None or (getattr(self, "r_chunk_hw", None) is not None and
                                           (self.r_partner is not None or getattr(self, "borrows", False)))

    @property
    def rec_dwords(self) -> int:
        """int32 per chunk record in memory (glove_common.h rec_stride_q): whole 128-byte lines — header + block 0 of 8 pairs
        + 16 bytes of padding fill the first, the other blocks follow packed."""
        capP = (self.chunk_cap + 7) // 8 * 8
        return (8 + 6 * (capP // 8 - 1) + 7) // 8 * 8 * 4

    def records(self, side: str, n_chunks: int) -> torch.Tensor:
        """The first n_chunks records of a side ('r' / 'c') in their packed form [n_chunks, 4 + 3 capP]: header {id, pairs, position
        of the id, first-chunk flag | chunks behind}, then capP / 8 blocks of {partner[8] | w[8] | y[8]} (tests and tools)."""
        capP = (self.chunk_cap + 7) // 8 * 8
        raw = getattr(self, side + "_crec")[:n_chunks * self.rec_dwords].view(n_chunks, self.rec_dwords)
        return torch.cat([raw[:, :28], raw[:, 32:32 + 24 * (capP // 8 - 1)]], dim=1)

    def struct(self) -> GlovePlan:
        if self._struct is None:
            s = GlovePlan()
            s.r_crec, s.c_crec = _ptr(self.r_crec), _ptr(self.c_crec)
            s.r_mark, s.c_mark = _ptr(getattr(self, "r_mark", None)), _ptr(getattr(self, "c_mark", None))
            s.r_chunk_hw, s.c_chunk_hw = _ptr(getattr(self, "r_chunk_hw", None)), _ptr(getattr(self, "c_chunk_hw", None))
            s.B, s.chunk_cap, s.cap_chunks, s.cap_uniq = self.B, self.chunk_cap, self.cap_chunks, self.cap_uniq
            s.heavy_chunks, s.cap_heavy, s.V_row = self.heavy_chunks, self.cap_heavy, getattr(self, "V_row", 0)
            s.counts = _ptr(self.counts)
            for i in range(8):
                s.host_counts[i] = self.host_counts[i]
            s.r_w, s.r_y = _ptr(self.r_w), _ptr(self.r_y)
            s.c_w, s.c_y = _ptr(self.c_w), _ptr(self.c_y)
            for n in self.INT_FIELDS:
                setattr(s, n, _ptr(getattr(self, n)))
            self._struct = s
        return self._struct

    def compact(self, lib=None, d: int | None = None, records: bool | None = None) -> "Plan":
        """Exact-size copy (one host sync): used when plans of a static stream stay resident.  With `lib`
        (the loaded C library) the copy also gets its per-chunk records; `d` (floats per table row) tells whether
        the batch is one the library steps in its fused form, which reads the id layout from the records.
        `records`: True / False overrides the rule below (tests and A/B tools)."""
        nc_r, nu_r, nc_c, nu_c, n_heavy, n_mapped = (int(x) for x in self.counts.tolist()[:6])
        if n_mapped:
            logger.warning("%d ids outside [0, %d) were treated as id 0 (the unknown token)", n_mapped, self.V)
        out = Plan.__new__(Plan)
        out.B, out.V, out.chunk_cap, out.V_row = self.B, self.V, self.chunk_cap, self.V_row
        out.cap_chunks, out.cap_uniq = max(nc_r, nc_c), max(nu_r, nu_c)
        out.counts = self.counts.clone()
        most = 0                 # the most chunks of one id (uniq_rec = {id, first chunk, chunks, pairs}); same sync as above
        if self.B > 0:
            most = int(max(self.r_uniq_rec[2:4 * nu_r:4].max().item() if nu_r else 0,
                           self.c_uniq_rec[2:4 * nu_c:4].max().item() if nu_c else 0))
        out.host_counts = [nc_r, nu_r, nc_c, nu_c, n_heavy, -1, most, -1]
        out.heavy_chunks, out.cap_heavy = self.heavy_chunks, max(n_heavy, 1)
        out.heavy = self.heavy[:max(n_heavy, 1)].clone()
        out.r_partner, out.r_w, out.r_y, out.r_to_c = self.r_partner, self.r_w, self.r_y, self.r_to_c
        out.c_partner, out.c_perm, out.c_w, out.c_y = self.c_partner, self.c_perm, self.c_w, self.c_y
        out.r_chunk_id = self.r_chunk_id[:max(out.cap_chunks, 1)].clone()
        out.c_chunk_id = self.c_chunk_id[:max(out.cap_chunks, 1)].clone()
        out.r_chunk_start = self.r_chunk_start[:out.cap_chunks + 1].clone()
        out.c_chunk_start = self.c_chunk_start[:out.cap_chunks + 1].clone()
        out.r_uniq_slot = self.r_uniq_slot[:out.cap_uniq + 1].clone()
        out.c_uniq_slot = self.c_uniq_slot[:out.cap_uniq + 1].clone()
        out.r_uniq_rec = self.r_uniq_rec[:4 * max(out.cap_uniq, 1)].clone()
        out.c_uniq_rec = self.c_uniq_rec[:4 * max(out.cap_uniq, 1)].clone()
        out._struct = None
        out.r_mark, out.c_mark = self.r_mark, self.c_mark
        out.r_chunk_hw = None if self.r_chunk_hw is None else self.r_chunk_hw[:max(out.cap_chunks, 1)].clone()
        out.c_chunk_hw = None if self.c_chunk_hw is None else self.c_chunk_hw[:max(out.cap_chunks, 1)].clone()
        out.r_crec = out.c_crec = None
        # records pad every chunk to the cap: worth it for the latency they save unless the chunks are nearly
        # empty (V = 400 k, B = 1 M: 2.6 pairs per 16-slot chunk -> 7 % more traffic, measured slower)
        fused = d is not None and (nu_r + nu_c) * d * 16 >= FUSED_STEP_BYTES
        if records is None:
            # (small batches always: the tagged step of the latency-bound regime reads nothing but the records)
            records = out.B <= TAGGED_STEP_MAX_BATCH or 4 * out.B >= out.chunk_cap * max(nc_r, nc_c)
            # a fused step reads the id layout from the records or from the run words; with the words it takes the pair fields
            # from the plan's arrays, a group's chunks at a time (V = 400 k, d = 300: 579 against 586 us per step; V = 2 M,
            # d = 128: 509 against 525), and the plan costs 40 instead of 190 B per nonzero
            # (that pays when a lane group owns many chunks — 12 at these sizes — so that the two trips up front are shared; at
            # V = 50 k, d = 300, B = 131,072 a group owns 2 and the records win, 98 against 104 us)
            if fused:
                records = out.r_chunk_hw is None or max(nc_r, nc_c) < RUN_WORDS_MIN_CHUNKS
        if not fused or records:
            out.r_chunk_hw = out.c_chunk_hw = None
        if lib is not None and out.B > 0 and records:
            n = max(out.cap_chunks, 1) * out.rec_dwords
            out.r_crec = torch.empty(n, dtype=torch.int32, device=self.counts.device)
            out.c_crec = torch.empty(n, dtype=torch.int32, device=self.counts.device)
            _check(lib.glove_plan_fill_records(C.byref(out.struct()), _stream()), "glove_plan_fill_records")
        return out

    def nbytes(self) -> int:
        n = sum(getattr(self, f).numel() * 4 for f in self.INT_FIELDS + ("r_w", "r_y", "c_w", "c_y", "counts", "r_mark", "c_mark", "r_chunk_hw", "c_chunk_hw") if getattr(self, f, None) is not None)
        return n + sum(t.numel() * 4 for t in (self.r_crec, self.c_crec) if t is not None)


class Pairs:
    """One sorted order of a set of nonzeros as four device arrays (glove_pairs): the pair's id on the order's own side,
    its id on the other side, glove_weight, glove_value."""

    def __init__(self, n: int, device):
        dev = torch.device(device)
        self.n = int(n)
        self.id = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)
        self.partner = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)
        self.w = torch.empty(max(self.n, 1), dtype=torch.float32, device=dev)
        self.y = torch.empty(max(self.n, 1), dtype=torch.float32, device=dev)
        self._struct = None

    def struct(self) -> GlovePairs:
        if self._struct is None:
            s = GlovePairs()
            s.id, s.partner, s.w, s.y = _ptr(self.id), _ptr(self.partner), _ptr(self.w), _ptr(self.y)
            self._struct = s
        return self._struct

    def arrays(self, lo: int = 0, hi: int | None = None):
        hi = self.n if hi is None else hi
        return self.id[lo:hi], self.partner[lo:hi], self.w[lo:hi], self.y[lo:hi]


class Masters:
    """A rank's nonzeros in their two master orders (glove_masters_build): row-major, col-major and the link between them."""

    def __init__(self, row_major: Pairs, col_major: Pairs, link: torch.Tensor, mapped: int):
        self.row_major, self.col_major, self.link, self.mapped = row_major, col_major, link, mapped
        self.n = row_major.n


class PlanBlock:
    """Staging plans that glove_plan_build_sorted refills together: the plans, a host array of their structs and the same
    array in device memory (the kernels read the structs from there: one launch covers the whole block)."""

    def __init__(self, plans: list):
        self.plans = list(plans)
        n = len(self.plans)
        # the plans' counts side by side in ONE tensor: a whole block's counts come back to the host in one copy
        self.counts = torch.zeros(n, 8, dtype=torch.int32, device=self.plans[0].counts.device)
        self.counts_host = torch.zeros(n, 8, dtype=torch.int32).pin_memory() if self.counts.is_cuda else torch.zeros(n, 8, dtype=torch.int32)
        for i, p in enumerate(self.plans):
            p.counts = self.counts[i]
            p._struct = None
        self.host = (GlovePlan * n)()
        for i, p in enumerate(self.plans):
            self.host[i] = p.struct()
        raw = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8)
        self.dev = raw.to(self.plans[0].counts.device)

    def __len__(self):
        return len(self.plans)

    def fetch_counts(self):
        """Starts the copy of every plan's counts to pinned host memory (on the current stream: behind the build that wrote them)."""
        self.counts_host.copy_(self.counts, non_blocking=True)

    def adopt_counts(self, n: int):
        """The fetched counts of the first n plans become their host counts: the step then sizes its grids by what the batch
        holds, like a resident plan's (call once the copy has completed).  The structs a BUILD reads (`host`) keep -1."""
        got = self.counts_host[:n].tolist()
        for p, c in zip(self.plans[:n], got):
            p.host_counts = [c[0], c[1], c[2], c[3], c[4], -1, -1, -1]
            st = p.struct()
            for i in range(8):
                st.host_counts[i] = p.host_counts[i]


def make_hyper(l2_reg=0.01, reg_mult=2.0, learning_rate=0.001, epsilon=1e-7, beta1=0.9, beta2=0.999,
               batch_size=None, inv_batch=None, sides=0, head=HEAD_REGRESSION, neg_factor=1.0,
               step_form=STEP_AUTO, optimizer="Adagrad", momentum=0.0, nesterov=False, rho=None, sweep_sides=0) -> GloveHyper:
    """`sides`: 0/3 both sides, 1 row side only, 2 col side only; `head`: HEAD_REGRESSION (GloVe) or
    HEAD_LOGISTIC (pos/neg logistic matrix factorisation, with `neg_factor`); `sweep_sides`: the sides whose unlisted rows
    the touched-rows apply sweeps under Adam / RMSprop / Nadam (0 = `sides`) — see glove_hyper in the header."""
    h = GloveHyper()
    h.sides, h.head, h.neg_factor, h.step_form, h.sweep_sides = sides, head, neg_factor, step_form, sweep_sides
    spec = OPTIMIZERS[optimizer] if isinstance(optimizer, str) else BY_CODE[int(optimizer)]     # (a name or its code)
    h.optimizer = spec.code     # set here once: the wrappers hand the struct on as it is
    if rho is None:                     # the optimizer's own Keras default
        rho = spec.rho
    h.momentum, h.nesterov, h.rho = momentum, int(bool(nesterov)), rho
    h.beta1, h.beta2 = beta1, beta2
    h.l2_reg, h.reg_mult, h.learning_rate, h.epsilon = l2_reg, reg_mult, learning_rate, epsilon
    h.inv_batch = inv_batch if inv_batch is not None else 1.0 / batch_size
    return h


def staging_records(B: int, V_row: int, V: int, d: int) -> bool | None:
    """Whether a staging plan (refilled on the device every step: a reshuffled epoch) should carry chunk records from its
    build: yes where the library will take a fused step form for it (glove_step.hip pick_step_form judges such a plan by
    the most ids its batch can hold), otherwise the Plan's own rule (small batches)."""
    return True if min(V_row + V, 2 * B) * ((d + 3) // 4 * 4) * 16 >= FUSED_STEP_BYTES else None


def _step_struct(tables, plans, hyper):
    """The tables as the Adagrad step may see them: a twinned row table stays twinned between steps.  Marks the tables
    as possibly twinned when one of the plans can take the twin form (the rule of glove_step.hip pick_step_form), so
    that the next reader of R / br brings them home first."""
    if getattr(tables, "R_tag", None) is not None:
        # step-tagged tables: the tagged step leaves rows in their second copies (the rule of glove_step.hip pick_step_form;
        # Adam: adam_one_launch)
        form = hyper.step_form
        if form == STEP_TAGGED or (form == STEP_AUTO and any(p.r_crec is not None and p.B <= TAGGED_STEP_MAX_BATCH for p in plans)):
            tables._twin_dirty = True
        return tables.struct(twin_ok=True)
    if getattr(tables, "R_ver", None) is None:
        return tables.struct()
    form = hyper.step_form
    for plan in plans:
        hc = plan.host_counts
        ids = hc[1] + hc[3] if hc[1] >= 0 and hc[3] >= 0 else min(tables.V_row + tables.V, 2 * plan.B)
        fused = plan.fusable and ids * tables.d * 16 >= FUSED_STEP_BYTES
        if form == STEP_FUSED_TWIN or (form == STEP_AUTO and fused):
            tables._twin_dirty = True
            break
    return tables.struct(twin_ok=True)


def _same_optimizer(tables, hyper):
    """The record of `tables.optimizer`, for the entry points that take the optimizer from glove_hyper.optimizer: a hyper made
    for another name would silently apply that one to these tables' slots."""
    spec = OPTIMIZERS[tables.optimizer]
    if hyper.optimizer != spec.code:
        raise GloveHipError("%s tables, but the hyper names optimizer code %d: make_hyper(optimizer=...)" % (tables.optimizer, hyper.optimizer))
    return spec


class KMeansResult(NamedTuple):
    """What GloveHip.kmeans returns: the winning run's last assignment [n] int32, its cosines [n], the centroids [K,d]
    that produced them, the assign passes it ran, whether two successive assignments agreed, its objective (the sum of
    the cosines, float64 on the host), and of all restarts the objectives and the last assignments."""
    assign: torch.Tensor
    cos: torch.Tensor
    centroids: torch.Tensor
    iterations: int
    converged: bool
    objective: float
    objectives: list
    assignments: list


class GloveHip:
    """Thin object wrapper over the C ABI; one instance per process/GPU."""

    def __init__(self, device="cuda:0", lib_path=None, any_abi=False):
        self.lib = load_library(lib_path, any_abi)
        self.device = torch.device(device)
        self._plan_ws = None
        self._step_ws = None
        self.ws_generation = 0      # counts reallocations of the shared workspaces: a captured hipGraph holds their raw pointers

    # ---- workspaces (grown on demand, never inside a captured region)
    def _ws(self, attr: str, nbytes: int) -> torch.Tensor:
        cur = getattr(self, attr)
        if cur is None or cur.numel() < nbytes:
            cur = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            setattr(self, attr, cur)
            self.ws_generation += 1
        return cur

    def step_workspace(self, plan: Plan, d: int) -> torch.Tensor:
        return self._ws("_step_ws", self.lib.glove_step_workspace_bytes(plan.B, plan.cap_chunks, d))

    # ---- index build
    def build_plan(self, row, col, w, y, V: int, chunk_cap: int | None = DEFAULT_CHUNK_CAP, compact=False,
                   into: Plan | None = None, ws: torch.Tensor | None = None, d: int | None = None,
                   V_row: int = 0, records: bool | None = None, links: bool = True, run_words: bool | None = None) -> Plan:
        """Builds the dedup index of one batch on the device.  `V_row`: rows of this rank's row-table shard when the
        row ids are shard-local (ids outside it count as id 0, like col ids outside [0, V)).  `run_words`: the per-chunk run words a
        fused step needs of a plan without records (default: when `d` says the batch can reach the fused regime).  `into`: a full-capacity Plan of the same
        (B, V, chunk_cap) to refill — a caller that indexes a fresh batch every step avoids ~20 tensor
        allocations per step this way.  `ws`: scratch of glove_plan_workspace_bytes(B, V) bytes (default: one
        shared buffer, fine for builds issued on one stream).  `records`: see Plan (default: small batches only)."""
        B = int(row.numel())
        _require(row, torch.int32, B); _require(col, torch.int32, B)
        _require(w, torch.float32, B); _require(y, torch.float32, B)
        if not chunk_cap:
            chunk_cap = auto_chunk_cap(B, V, d)
        if into is not None:
            if (into.B, into.V, into.chunk_cap) != (B, V, chunk_cap) or into.cap_chunks < B:
                raise ValueError("`into` must be an uncompacted plan of the same batch size, vocabulary and chunk cap")
            plan = into
        else:
            if run_words is None:
                run_words = d is not None and min((V_row or V) + V, 2 * B) * ((d + 3) // 4 * 4) * 16 >= FUSED_STEP_BYTES
            plan = Plan(B, V, chunk_cap, row.device, V_row=V_row, records=records, links=links, run_words=bool(run_words))
        if ws is None:      # builds that run concurrently on different streams each bring their own scratch
            ws = self._ws("_plan_ws", self.lib.glove_plan_workspace_bytes(B, V))
        _check(self.lib.glove_plan_build(_ptr(row), _ptr(col), _ptr(w), _ptr(y), B, V, C.byref(plan.struct()),
                                         _ptr(ws), ws.numel(), _stream()), "glove_plan_build")
        return plan.compact(self.lib, d) if compact else plan

    # ---- epochs dealt from id-sorted master orders (include/glove_hip.h)
    def build_masters(self, row, col, w, y, V: int, V_row: int = 0) -> Masters:
        """The rank's nonzeros sorted once: row-major and col-major orders + the link between them (one host sync for the
        count of ids that were mapped to 0)."""
        n = int(row.numel())
        _require(row, torch.int32, n); _require(col, torch.int32, n)
        _require(w, torch.float32, n); _require(y, torch.float32, n)
        dev = row.device
        rm, cm = Pairs(n, dev), Pairs(n, dev)
        link = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        mapped = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(self.lib.glove_masters_workspace_bytes(n), 256), dtype=torch.uint8, device=dev)
        _check(self.lib.glove_masters_build(_ptr(row), _ptr(col), _ptr(w), _ptr(y), n, V, V_row, C.byref(rm.struct()),
                                            C.byref(cm.struct()), _ptr(link), _ptr(mapped), _ptr(ws), ws.numel(), _stream()),
               "glove_masters_build")
        n_mapped = int(mapped.item())
        if n_mapped:
            logger.warning("%d ids outside their table were treated as id 0 (the unknown token)", n_mapped)
        del ws
        return Masters(rm, cm, link, n_mapped)

    def deal_workspace(self, n: int, B: int, device) -> torch.Tensor:
        return torch.empty(max(self.lib.glove_epoch_deal_workspace_bytes(n, B), 256), dtype=torch.uint8, device=device)

    def deal_epoch(self, masters: Masters, B: int, key: int, row_side: Pairs, col_side: Pairs, ws: torch.Tensor) -> None:
        """One epoch of `masters` under the bijection the 128-bit `key` determines, into row_side / col_side: batch k =
        positions [k B, (k + 1) B) of both, sorted by row id / by col id."""
        if row_side.n != masters.n or col_side.n != masters.n:
            raise GloveHipError("epoch buffers must hold %d pairs" % masters.n)
        _check(self.lib.glove_epoch_deal(C.byref(masters.row_major.struct()), C.byref(masters.col_major.struct()),
                                         _ptr(masters.link), masters.n, B, key & (2 ** 64 - 1), (key >> 64) & (2 ** 64 - 1),
                                         C.byref(row_side.struct()), C.byref(col_side.struct()), _ptr(ws), ws.numel(), _stream()),
               "glove_epoch_deal")

    def staging_plan(self, B: int, V: int, chunk_cap: int, device, V_row: int = 0, records: bool = True, run_words: bool = False,
                     borrow: bool = False) -> Plan:
        """A plan for glove_plan_build_sorted to refill: capacity for any batch of B pairs (an id of p pairs has at most
        p / chunk_cap + 1 chunks), chunk records carrying the pair fields, or pair arrays of its own without records
        (`run_words`: with the per-chunk run words the fused step forms need in that case; `borrow`: no pair arrays either —
        build_plans_sorted points the plan at the batch's positions in the epoch's arrays, which must outlive its steps)."""
        cap_uniq = min(B, max(V, V_row or 0))
        cap_chunks = int(self.lib.glove_plan_chunk_bound(B, cap_uniq, chunk_cap))
        words = run_words and not records
        plan = Plan(B, V, chunk_cap, device, cap_chunks=cap_chunks, cap_uniq=cap_uniq, V_row=V_row, records=bool(records),
                    links=False, own_pairs=not records and not (borrow and words), run_words=words,
                    _no_pairs_ok=bool(borrow and words))
        plan.borrows = bool(borrow and words)
        return plan

    def build_plans_sorted(self, row_side: Pairs, col_side: Pairs, first_batch: int, block: PlanBlock, n: int,
                           V: int, ws: torch.Tensor) -> None:
        """The indexes of batches first_batch .. first_batch + n - 1 of a dealt epoch into the first n plans of `block`."""
        B = block.plans[0].B
        if n < 0 or n > len(block) or (first_batch + n) * B > row_side.n:
            raise GloveHipError("batches %d .. %d of %d pairs do not lie inside the epoch" % (first_batch, first_batch + n - 1, B))
        _check(self.lib.glove_plan_build_sorted(C.byref(row_side.struct()), C.byref(col_side.struct()), first_batch * B, B, n, V,
                                                block.host, _ptr(block.dev), _ptr(ws), ws.numel(), _stream()),
               "glove_plan_build_sorted")
        if getattr(block.plans[0], "borrows", False):
            # plans that borrow their pair fields: batch j lies sorted at positions [(first_batch + j) B, ...) of the epoch's arrays
            base = [(t.data_ptr(), t) for t in (row_side.partner, row_side.w, row_side.y, col_side.partner, col_side.w, col_side.y)]
            for j in range(n):
                st, off = block.plans[j].struct(), 4 * (first_batch + j) * B
                st.r_partner, st.r_w, st.r_y = (base[k][0] + off for k in range(3))
                st.c_partner, st.c_w, st.c_y = (base[k][0] + off for k in range(3, 6))
                block.plans[j].lent = (row_side, col_side)          # (keeps the epoch's arrays alive as long as the plan points at them)

    # ---- passes
    def _plan_call(self, name, plan, tables, hyper, ws, *tail):
        """An entry point of the shape (plan, tables, hyper, ws, ws_bytes, <tail>, stream), with the shared step workspace by default."""
        ws = self.step_workspace(plan, tables.d) if ws is None else ws
        _check(getattr(self.lib, name)(C.byref(plan.struct()), C.byref(tables.struct()), C.byref(hyper), _ptr(ws), ws.numel(),
                                       *tail, _stream()), name)

    def passes(self, plan, tables, hyper, ws=None):
        """Both gather passes (row side and col side) in one launch."""
        self._plan_call("glove_passes_f32", plan, tables, hyper, ws)

    def rowpass(self, plan, tables, hyper, ws=None):
        self._plan_call("glove_rowpass_f32", plan, tables, hyper, ws)

    def colpass(self, plan, tables, hyper, ws=None):
        self._plan_call("glove_colpass_f32", plan, tables, hyper, ws)

    def rowside_step(self, plan, tables, hyper, ws=None):
        """The row side of a step, applied in place where a lane group holds an id completely (hyper.sides = 1); the
        col pass of the step must have run already: it gathers the old rows."""
        self._plan_call("glove_rowside_step_adagrad_f32", plan, tables, hyper, ws)

    def rowside_step_opt(self, plan, tables, hyper, G_flat=None, ws=None):
        """The row side of a step under the optimizer `tables.optimizer` names (hyper.sides = 1; glove_rowside_step_f32).
        G_flat: a dense gradient buffer of these tables (all zero between calls) — the names with a `row_scratch` in
        trainer/optimizers.py mark or sum the row ids in it."""
        _same_optimizer(tables, hyper)
        self._plan_call("glove_rowside_step_f32", plan, tables, hyper, ws, _ptr(G_flat))

    def apply_adagrad(self, plan, tables, hyper, loss_out=None, ws=None):
        self._plan_call("glove_apply_adagrad_f32", plan, tables, hyper, ws, _ptr(loss_out))

    def dense_grad(self, plan, tables, hyper, G_flat, ws=None):
        self._plan_call("glove_dense_grad_f32", plan, tables, hyper, ws, _ptr(G_flat))

    def dense_adagrad(self, tables, hyper, G_flat, loss_out=None):
        _check(self.lib.glove_dense_adagrad_f32(C.byref(tables.struct()), C.byref(hyper), _ptr(G_flat),
                                                _ptr(loss_out), _stream()), "glove_dense_adagrad_f32")

    def dense_adam(self, tables, hyper, G_flat, loss_out=None):
        _check(self.lib.glove_dense_adam_f32(C.byref(tables.struct()), C.byref(hyper), _ptr(G_flat),
                                             _ptr(loss_out), _stream()), "glove_dense_adam_f32")

    def grad_layout(self, tables) -> dict:
        """Float offsets of the sections of the flat dense-gradient buffer."""
        offs = (C.c_int64 * 5)()
        total = self.lib.glove_dense_grad_layout(tables.V_row, tables.V, tables.d, C.cast(offs, C.c_void_p))
        return dict(G_R=offs[0], G_br=offs[1], G_C=offs[2], G_bc=offs[3], tail=offs[4], total=int(total))

    def dense_grad_buffer(self, tables) -> torch.Tensor:
        return torch.zeros(self.grad_layout(tables)["total"], dtype=torch.float32, device=tables.device)

    # ---- touched-rows exchange (include/glove_hip.h "touched-rows exchange")
    def packed_list(self, buf: torch.Tensor, with_header=True, ids: torch.Tensor | None = None, n: int = -1,
                    side: int = -1) -> GlovePackedList:
        """One list inside `buf` ([entries, d + 4] float32, contiguous): header in entry 0 and the count read from it on
        the device (with_header), or a bare run of `n` entries, optionally with explicit owner-local `ids`."""
        _require(buf, torch.float32)
        stride = buf.shape[-1]
        lst = GlovePackedList()
        lst.entries = buf.data_ptr() + (4 * stride if with_header else 0)
        lst.header = buf.data_ptr() if with_header else None
        if ids is not None:
            _require(ids, torch.int32)
            if ids.numel() < n:
                raise GloveHipError("%d ids for %d entries" % (ids.numel(), n))
        lst.ids = _ptr(ids)
        lst.n, lst.side = n, side
        return lst

    def pack_grad(self, plan, tables, hyper, packed: torch.Tensor, ws=None):
        """The plan's summed gradients (hyper.sides) as one packed list: packed is [capacity, d + 4] float32."""
        self._packing_call("glove_pack_grad_f32", plan, tables, hyper, packed, ws)

    def _packing_call(self, name, plan, tables, hyper, packed, ws):
        _require(packed, torch.float32)
        if packed.dim() != 2 or packed.shape[1] != tables.d + 4:
            raise GloveHipError("packed buffer must be [entries, d + 4]")
        self._plan_call(name, plan, tables, hyper, ws, _ptr(packed), packed.shape[0])

    def passes_packing(self, plan, tables, hyper, packed: torch.Tensor, ws=None):
        """The passes of hyper.sides; ids one lane group holds completely land in the packed list right away."""
        self._packing_call("glove_passes_packing_f32", plan, tables, hyper, packed, ws)

    def pack_rest(self, plan, tables, hyper, packed: torch.Tensor, ws=None):
        """Completes the list passes_packing started (the other ids, the header)."""
        self._packing_call("glove_pack_rest_f32", plan, tables, hyper, packed, ws)

    def loss_partials(self, plan, tables, out4: torch.Tensor, ws=None):
        """out4 = {sum e, sum w diff^2, sum |r|^2+|c|^2, sum b^2} of the plan's last row pass (a list header's floats 2..5)."""
        _require(out4, torch.float32, 4)
        ws = self.step_workspace(plan, tables.d) if ws is None else ws
        _check(self.lib.glove_loss_partials_f32(C.byref(plan.struct()), C.byref(tables.struct()), _ptr(ws), ws.numel(),
                                                _ptr(out4), _stream()), "glove_loss_partials_f32")

    def combine_packed(self, lst: GlovePackedList, tag: int, tables, G_flat, mark, capacity: int):
        _require(G_flat, torch.float32)
        _require(mark, torch.int32)
        if mark.numel() < tables.V_row + tables.V:
            raise GloveHipError("mark needs V_row + V entries")
        _check(self.lib.glove_combine_packed_f32(C.byref(lst), tag, C.byref(tables.struct()), _ptr(G_flat), _ptr(mark),
                                                 capacity, _stream()), "glove_combine_packed_f32")

    def count_packed(self, lists, tables, G_flat, mark, capacity: int = 0):
        """Optional before the combines: ids only one list touches are then applied straight from their entry."""
        arr = (GlovePackedList * len(lists))(*lists)
        _check(self.lib.glove_count_packed_f32(arr, len(lists), C.byref(tables.struct()), _ptr(G_flat), _ptr(mark), capacity,
                                               _stream()), "glove_count_packed_f32")

    def apply_packed(self, lists, tables, hyper, G_flat, mark, tail=None, loss_out=None, capacity: int = 0):
        arr = (GlovePackedList * len(lists))(*lists)
        _check(self.lib.glove_apply_packed_adagrad_f32(arr, len(lists), C.byref(tables.struct()), C.byref(hyper),
                                                       _ptr(G_flat), _ptr(mark), _ptr(tail), _ptr(loss_out), capacity,
                                                       _stream()), "glove_apply_packed_adagrad_f32")

    def gather_rows(self, W, bias, ids, rows, biases):
        for x in (W, bias, rows, biases):
            _require(x, torch.float32)
        _require(ids, torch.int32)
        n = int(ids.numel())
        if rows.numel() < n * W.shape[1] or biases.numel() < n:
            raise GloveHipError("gather_rows: output buffers too small")
        _check(self.lib.glove_gather_rows_f32(_ptr(W), _ptr(bias), _ptr(ids), n, W.shape[1], _ptr(rows), _ptr(biases),
                                              _stream()), "glove_gather_rows_f32")

    # ---- whole steps
    def step(self, plan, tables, hyper, G_flat=None, loss_out=None, ws=None):
        """One whole single-GPU step of `tables.optimizer` through the entry point its record names (trainer/optimizers.py).
        G_flat: the dense gradient buffer of the names whose record says `step_buffer`."""
        entry = OPTIMIZERS[tables.optimizer].entry
        if entry == "adagrad":
            self.step_adagrad(plan, tables, hyper, loss_out, ws)
        else:
            (self.step_adam if entry == "adam" else self.step_sparse)(plan, tables, hyper, G_flat, loss_out, ws)

    def steps(self, plans, tables, hyper, G_flat=None, loss_out=None, ws=None):
        """len(plans) consecutive steps: ONE host call where the name has a chained entry point, otherwise one call per plan."""
        entry = OPTIMIZERS[tables.optimizer].entry
        if entry == "adagrad":
            self.steps_adagrad(plans, tables, hyper, loss_out, ws)
        elif entry == "adam":
            self.steps_adam(plans, tables, hyper, G_flat, loss_out, ws)
        else:
            for plan in plans:
                self.step_sparse(plan, tables, hyper, G_flat, loss_out, ws)

    def step_adagrad(self, plan, tables, hyper, loss_out=None, ws=None):
        ws = self.step_workspace(plan, tables.d) if ws is None else ws
        _check(self.lib.glove_step_adagrad_f32(C.byref(plan.struct()), C.byref(_step_struct(tables, (plan,), hyper)), C.byref(hyper),
                                               _ptr(ws), ws.numel(), _ptr(loss_out), _stream()),
               "glove_step_adagrad_f32")

    def steps_adagrad(self, plans, tables, hyper, loss_out=None, ws=None):
        """len(plans) consecutive Adagrad steps from one host call (the launch loop runs in C; on step-tagged tables consecutive
        small batches go out as a chain: ONE launch per step, glove_steps_adagrad_f32)."""
        if not plans:
            return
        if ws is None:
            big = max(plans, key=lambda p: self.lib.glove_step_workspace_bytes(p.B, p.cap_chunks, tables.d))
            ws = self.step_workspace(big, tables.d)
        arr = (C.POINTER(GlovePlan) * len(plans))(*[C.pointer(p.struct()) for p in plans])
        _check(self.lib.glove_steps_adagrad_f32(arr, len(plans), C.byref(_step_struct(tables, plans, hyper)), C.byref(hyper), _ptr(ws),
                                                ws.numel(), _ptr(loss_out), _stream()), "glove_steps_adagrad_f32")

    def step_adam(self, plan, tables, hyper, G_flat, loss_out=None, ws=None):
        ws = self.step_workspace(plan, tables.d) if ws is None else ws
        _check(self.lib.glove_step_adam_f32(C.byref(plan.struct()), C.byref(_step_struct(tables, (plan,), hyper)), C.byref(hyper),
                                            _ptr(ws), ws.numel(), _ptr(G_flat), _ptr(loss_out), _stream()),
               "glove_step_adam_f32")

    def step_sparse(self, plan, tables, hyper, G_flat=None, loss_out=None, ws=None):
        """One step under the optimizer `tables.optimizer` names (glove_step_sparse_f32 takes every name of trainer/optimizers.py;
        inside the library those with an entry point of their own go there).  G_flat: the dense gradient buffer of the names
        whose record says `step_buffer`.  `hyper` must have been made for the same name (make_hyper(optimizer=...))."""
        ws = self.step_workspace(plan, tables.d) if ws is None else ws
        spec = _same_optimizer(tables, hyper)
        struct = _step_struct(tables, (plan,), hyper) if spec.chained else tables.struct()      # (own entry points: they know tagged / twinned tables)
        _check(self.lib.glove_step_sparse_f32(C.byref(plan.struct()), C.byref(struct), C.byref(hyper), _ptr(ws), ws.numel(),
                                              _ptr(G_flat), _ptr(loss_out), _stream()), "glove_step_sparse_f32")

    def steps_adam(self, plans, tables, hyper, G_flat, loss_out=None, ws=None):
        """len(plans) consecutive Adam steps from one host call (on twinned tables consecutive small batches go out as a chain:
        ONE launch per step, glove_steps_adam_f32)."""
        if not plans:
            return
        if ws is None:
            big = max(plans, key=lambda p: self.lib.glove_step_workspace_bytes(p.B, p.cap_chunks, tables.d))
            ws = self.step_workspace(big, tables.d)
        arr = (C.POINTER(GlovePlan) * len(plans))(*[C.pointer(p.struct()) for p in plans])
        _check(self.lib.glove_steps_adam_f32(arr, len(plans), C.byref(_step_struct(tables, plans, hyper)), C.byref(hyper), _ptr(ws),
                                             ws.numel(), _ptr(G_flat), _ptr(loss_out), _stream()),
               "glove_steps_adam_f32")

    # ---- eval / predict
    def eval_sums(self, row, col, w, y, tables, sums=None) -> torch.Tensor:
        n = int(row.numel())
        _require(row, torch.int32, n); _require(col, torch.int32, n)
        _require(w, torch.float32, n); _require(y, torch.float32, n)
        _require(sums, torch.float64)
        if sums is None:
            sums = torch.zeros(4, dtype=torch.float64, device=tables.device)
        _check(self.lib.glove_eval_f32(_ptr(row), _ptr(col), _ptr(w), _ptr(y), int(row.numel()),
                                       C.byref(tables.struct()), _ptr(sums), _stream()), "glove_eval_f32")
        return sums

    def eval_sums_logistic(self, row, col, pos, neg, tables, sums=None) -> torch.Tensor:
        n = int(row.numel())
        _require(row, torch.int32, n); _require(col, torch.int32, n)
        _require(pos, torch.float32, n); _require(neg, torch.float32, n)
        _require(sums, torch.float64)
        if sums is None:
            sums = torch.zeros(6, dtype=torch.float64, device=tables.device)
        _check(self.lib.glove_eval_logistic_f32(_ptr(row), _ptr(col), _ptr(pos), _ptr(neg), int(row.numel()),
                                                C.byref(tables.struct()), _ptr(sums), _stream()),
               "glove_eval_logistic_f32")
        return sums

    def topk_cosine(self, R: torch.Tensor, query_ids: torch.Tensor, k: int):
        _require(R, torch.float32); _require(query_ids, torch.int32)
        V, d = R.shape
        n = int(query_ids.numel())
        sims = torch.empty(n, k, dtype=torch.float32, device=R.device)
        idx = torch.empty(n, k, dtype=torch.int32, device=R.device)
        ws = torch.empty(self.lib.glove_topk_workspace_bytes(n, V, k), dtype=torch.uint8, device=R.device)
        _check(self.lib.glove_topk_cosine_f32(_ptr(R), V, d, _ptr(query_ids), n, k, _ptr(sims), _ptr(idx),
                                              _ptr(ws), ws.numel(), _stream()), "glove_topk_cosine_f32")
        return sims, idx

    def _analogy_batches(self, W: torch.Tensor, abc: torch.Tensor, k: int, batch: int, sizes: str, entry: str, *extra):
        """What analogy_topk and analogy_cosmul_topk share: the checks, the outputs, one workspace of `sizes`(batch
        questions) bytes and the walk of the questions through `entry` in batches; `extra` goes between k and the outputs."""
        _require(W, torch.float32); _require(abc, torch.int32)
        if W.dim() != 2 or abc.dim() != 2 or abc.shape[1] != 3:
            raise GloveHipError("expected W [V,d] and abc [n,3]")
        if batch < 1:
            raise GloveHipError("batch must be positive, got %d" % batch)
        lib = load_eval_library()
        V, d = W.shape
        n = int(abc.shape[0])
        sims = torch.empty(n, k, dtype=torch.float32, device=W.device)
        idx = torch.empty(n, k, dtype=torch.int32, device=W.device)
        ws = torch.empty(max(getattr(lib, sizes)(min(batch, n), V, d, k), 256), dtype=torch.uint8, device=W.device)
        for s in range(0, max(n, 1), batch):      # (n == 0: one call, which checks the sizes and launches nothing)
            m = min(batch, n - s)
            _check(getattr(lib, entry)(_ptr(W), V, d, _ptr(abc[s:s + m]), m, k, *extra, _ptr(sims[s:s + m]), _ptr(idx[s:s + m]),
                                       _ptr(ws), ws.numel(), _stream()), entry)
        return sims, idx

    def analogy_topk(self, W: torch.Tensor, abc: torch.Tensor, k: int, batch: int = 1024):
        """3CosAdd word analogies (include/glove_eval_hip.h): for the questions abc [n,3] = (a, b, c) the k rows of W [V,d]
        closest by cosine to w^_b - w^_a + w^_c, a, b and c themselves left out -> (sims, idx) [n,k], descending, ties to
        the lower id.  The scores of `batch` questions are a [batch, V] matrix in the workspace: the questions are walked
        in batches of that size through one workspace.  The ids of abc must lie in [0, V): the kernels do not look."""
        return self._analogy_batches(W, abc, k, batch, "glove_analogy_workspace_bytes", "glove_analogy_topk_f32")

    def analogy_cosmul_topk(self, W: torch.Tensor, abc: torch.Tensor, k: int, eps: float = 1e-3, batch: int = 1024):
        """3CosMul word analogies (include/glove_eval_sim_hip.h): for the questions abc [n,3] = (a, b, c) the k rows v of
        W [V,d] with the largest s(b, v) s(c, v) / (s(a, v) + eps), s = (1 + cos) / 2, a, b and c themselves left out ->
        (scores, idx) [n,k], descending, ties to the lower id.  Walks the questions in batches through one workspace like
        analogy_topk; a question's scores do not depend on its batch.  The ids of abc must lie in [0, V)."""
        return self._analogy_batches(W, abc, k, batch, "glove_cosmul_workspace_bytes", "glove_cosmul_topk_f32", float(eps))

    def pair_cosine(self, W: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
        """The cosine of the rows pairs[i,0] and pairs[i,1] of W [V,d] -> [n] (include/glove_eval_sim_hip.h), the norms
        clamped as in the PREDICT path.  The ids must lie in [0, V)."""
        _require(W, torch.float32); _require(pairs, torch.int32)
        if W.dim() != 2 or pairs.dim() != 2 or pairs.shape[1] != 2:
            raise GloveHipError("expected W [V,d] and pairs [n,2]")
        lib = load_eval_library()
        V, d = W.shape
        n = int(pairs.shape[0])
        out = torch.empty(n, dtype=torch.float32, device=W.device)
        _check(lib.glove_pair_cosine_f32(_ptr(W), V, d, _ptr(pairs), n, _ptr(out), _stream()), "glove_pair_cosine_f32")
        return out

    # ---- neighbours across two tables, by cosine or CSLS (include/glove_eval_cross_hip.h): what trainer.align drives
    def cross_topk(self, Q: torch.Tensor, qid: torch.Tensor, T: torch.Tensor, k: int, q_pen: torch.Tensor | None = None,
                   t_pen: torch.Tensor | None = None, batch: int = 1024):
        """For the rows qid [n] of Q [Vq, d] the k rows of T [Vt, d] with the largest cosine -> (scores, idx) [n, k],
        descending, ties to the lower id; with q_pen [n] and t_pen [Vt] (both or neither) the score is CSLS's
        2 cos - q_pen[q] - t_pen[v].  The scores of `batch` queries are a [batch, Vt] matrix in the workspace: the queries
        are walked in batches of that size through one workspace, and a query's result does not depend on its batch.  The
        ids must lie in [0, Vq): the kernels do not look."""
        _require(Q, torch.float32); _require(T, torch.float32); _require(qid, torch.int32)
        if Q.dim() != 2 or T.dim() != 2 or qid.dim() != 1 or Q.shape[1] != T.shape[1]:
            raise GloveHipError("expected Q [Vq, d], T [Vt, d] of one row stride and qid [n]")
        if batch < 1:
            raise GloveHipError("batch must be positive, got %d" % batch)
        if (q_pen is None) != (t_pen is None):
            raise GloveHipError("CSLS takes both penalty arrays, nearest neighbours neither")
        lib = load_eval_library()
        (Vq, d), Vt, n = Q.shape, int(T.shape[0]), int(qid.numel())
        _require(q_pen, torch.float32, n); _require(t_pen, torch.float32, Vt)
        sims = torch.empty(n, k, dtype=torch.float32, device=Q.device)
        idx = torch.empty(n, k, dtype=torch.int32, device=Q.device)
        ws = torch.empty(max(lib.glove_cross_topk_workspace_bytes(min(batch, n), Vt, d, k), 256), dtype=torch.uint8, device=Q.device)
        for s in range(0, max(n, 1), batch):      # (n == 0: one call, which checks the sizes and launches nothing)
            m = min(batch, n - s)
            _check(lib.glove_cross_topk_f32(_ptr(Q), Vq, _ptr(qid[s:s + m]), m, _ptr(T), Vt, d, k,
                                            None if q_pen is None else _ptr(q_pen[s:s + m]), _ptr(t_pen), _ptr(sims[s:s + m]),
                                            _ptr(idx[s:s + m]), _ptr(ws), ws.numel(), _stream()), "glove_cross_topk_f32")
        return sims, idx

    def topk_mean(self, sims: torch.Tensor) -> torch.Tensor:
        """The mean of each row of sims [n, k] -> [n]: a float32 sum in position order, one division by k."""
        _require(sims, torch.float32)
        if sims.dim() != 2 or sims.shape[1] < 1:
            raise GloveHipError("expected sims [n, k >= 1], got %s" % (tuple(sims.shape),))
        lib = load_eval_library()
        n, k = int(sims.shape[0]), int(sims.shape[1])
        out = torch.empty(n, dtype=torch.float32, device=sims.device)
        _check(lib.glove_topk_mean_f32(_ptr(sims), n, k, _ptr(out), _stream()), "glove_topk_mean_f32")
        return out

    def csls_penalty(self, A: torch.Tensor, ids: torch.Tensor, B: torch.Tensor, knn: int = 10, batch: int = 1024) -> torch.Tensor:
        """The mean cosine of each row A[ids] to its `knn` nearest rows of B -> [n]: topk_mean of cross_topk's scores."""
        return self.topk_mean(self.cross_topk(A, ids, B, knn, batch=batch)[0])

    # ---- spherical k-means (include/glove_eval_cluster_hip.h)
    def _kmeans_args(self, W, ids, centroids, assign=None):
        _require(W, torch.float32); _require(ids, torch.int32); _require(centroids, torch.float32)
        if W.dim() != 2 or ids.dim() != 1 or centroids.dim() != 2 or centroids.shape[1] != W.shape[1]:
            raise GloveHipError("expected W [V,d], ids [n] and centroids [K,d] of W's row stride")
        if assign is not None:
            _require(assign, torch.int32, int(ids.numel()))
            if assign.dim() != 1:
                raise GloveHipError("expected assign [n]")
        return int(W.shape[0]), int(W.shape[1]), int(ids.numel()), int(centroids.shape[0])

    def kmeans_workspace(self, n: int, V: int, d: int, K: int, device) -> torch.Tensor:
        """The one workspace of kmeans_assign and kmeans_update for these sizes."""
        need = load_eval_library().glove_kmeans_workspace_bytes(n, V, d, K)
        if need == 0:
            raise GloveHipError("k-means takes d %% 4 == 0 up to 1024, 0 <= n <= 65535 * 128 and 1 <= K <= %d: got n = %d, "
                                "V = %d, d = %d, K = %d" % (KMEANS_MAX_CLUSTERS, n, V, d, K))
        return torch.empty(need, dtype=torch.uint8, device=device)

    def kmeans_assign(self, W: torch.Tensor, ids: torch.Tensor, centroids: torch.Tensor, ws: torch.Tensor | None = None):
        """The closest of the centroids [K,d] by cosine for every point W[ids[i]] -> (assign [n] int32, cos [n]): ties to
        the lower centroid, a zero row to cluster 0 with cosine 0.  The ids must lie in [0, V): the kernels do not look."""
        V, d, n, K = self._kmeans_args(W, ids, centroids)
        lib = load_eval_library()
        ws = self.kmeans_workspace(n, V, d, K, W.device) if ws is None else ws
        assign = torch.empty(n, dtype=torch.int32, device=W.device)
        cos = torch.empty(n, dtype=torch.float32, device=W.device)
        _check(lib.glove_kmeans_assign_f32(_ptr(W), V, d, _ptr(ids), n, _ptr(centroids), K, _ptr(assign), _ptr(cos),
                                           _ptr(ws), ws.numel(), _stream()), "glove_kmeans_assign_f32")
        return assign, cos

    def kmeans_update(self, W: torch.Tensor, ids: torch.Tensor, assign: torch.Tensor, centroids: torch.Tensor,
                      ws: torch.Tensor | None = None):
        """The unit-length sums of each cluster's unit rows -> (centroids [K,d], counts [K] int32); an empty cluster keeps
        its row of `centroids`.  Bitwise repeatable (a fixed summation order, no float atomics)."""
        V, d, n, K = self._kmeans_args(W, ids, centroids, assign)
        lib = load_eval_library()
        ws = self.kmeans_workspace(n, V, d, K, W.device) if ws is None else ws
        if n == 0:                      # the library leaves its outputs untouched: every cluster is empty
            return centroids.clone(), torch.zeros(K, dtype=torch.int32, device=W.device)
        out = torch.empty_like(centroids)
        counts = torch.empty(K, dtype=torch.int32, device=W.device)
        _check(lib.glove_kmeans_update_f32(_ptr(W), V, d, _ptr(ids), n, _ptr(assign), _ptr(centroids), K, _ptr(out),
                                           _ptr(counts), _ptr(ws), ws.numel(), _stream()), "glove_kmeans_update_f32")
        return out, counts

    def kmeans(self, W: torch.Tensor, ids: torch.Tensor, K: int, seed: int = 0, restarts: int = 1, iterations: int = 100,
               init: torch.Tensor | None = None) -> KMeansResult:
        """Spherical k-means of the points W[ids[i]] into K clusters (include/glove_eval_cluster_hip.h).  Run r of
        `restarts` starts from the unit rows of the points sorted(numpy.random.default_rng([seed, r]).choice(n, K,
        replace=False)); `init` [K,d] gives the one run's initial centroids instead.  A run assigns, stops when the
        assignment repeats (converged) or after `iterations` assign passes, and otherwise updates; its result is the
        last assignment with the centroids that produced it.  The run with the largest sum of cosines wins, ties to the
        lower r.  One workspace serves every call; the host compares successive assignments."""
        _require(W, torch.float32); _require(ids, torch.int32)
        if W.dim() != 2 or ids.dim() != 1:
            raise GloveHipError("expected W [V,d] and ids [n]")
        n = int(ids.numel())
        if iterations < 1 or restarts < 1:
            raise GloveHipError("iterations and restarts must be positive, got %d and %d" % (iterations, restarts))
        if init is not None:
            if restarts != 1:
                raise GloveHipError("explicit initial centroids make one run: restarts must be 1, got %d" % restarts)
            if init.dim() != 2 or init.shape[0] != K:
                raise GloveHipError("expected init [K,d]")
        elif not 1 <= K <= n:
            raise GloveHipError("K must lie in [1, n = %d] to draw the initial centroids from the points, got %d" % (n, K))
        ws = self.kmeans_workspace(n, int(W.shape[0]), int(W.shape[1]), K, W.device)
        best, objectives, assignments = None, [], []
        for r in range(restarts):
            if init is not None:
                cents = init
            else:
                rows = np.sort(np.random.default_rng([seed, r]).choice(n, K, replace=False))
                X = W[ids[torch.from_numpy(rows).to(ids.device)].long()]
                cents = (X * torch.rsqrt(torch.clamp((X * X).sum(dim=1, keepdim=True), min=1e-12))).contiguous()
            previous, converged, t = None, False, 0
            while True:
                t += 1
                assign, cos = self.kmeans_assign(W, ids, cents, ws)
                converged = previous is not None and torch.equal(assign, previous)
                if converged or t == iterations:
                    break
                cents, _ = self.kmeans_update(W, ids, assign, cents, ws)
                previous = assign
            objective = float(cos.cpu().numpy().astype(np.float64).sum())
            objectives.append(objective)
            assignments.append(assign)
            if best is None or objective > best.objective:
                best = KMeansResult(assign, cos, cents, t, converged, objective, objectives, assignments)
        return best

    # ---- count-based baselines (include/glove_factor_hip.h): what trainer.svd drives
    def _csr_args(self, row_ptr, col_idx, val, n_rows: int):
        _require(row_ptr, torch.int64, n_rows + 1); _require(val, torch.float32)
        nnz = int(val.numel())
        if col_idx is not None:
            _require(col_idx, torch.int32, nnz)
        return nnz

    def csr_spmm(self, row_ptr: torch.Tensor, col_idx: torch.Tensor, val: torch.Tensor, n_rows: int, n_cols: int,
                 B: torch.Tensor, ws: torch.Tensor | None = None) -> torch.Tensor:
        """Y [n_rows, l] = A B for the CSR matrix A (row_ptr int64 [n_rows + 1] from 0 to nnz, col_idx int32, val float32)
        and B [n_cols, l] float32, l % 4 == 0 up to 1024.  Bitwise repeatable (a fixed summation order, no float
        atomics); a row without nonzeros comes back as zeros.  The columns must lie in [0, n_cols)."""
        nnz = self._csr_args(row_ptr, col_idx, val, n_rows)
        _require(B, torch.float32)
        if B.dim() != 2 or B.shape[0] != n_cols:
            raise GloveHipError("expected B [n_cols = %d, l], got %s" % (n_cols, tuple(B.shape)))
        lib, l = load_factor_library(), int(B.shape[1])
        need = lib.glove_csr_spmm_workspace_bytes(n_rows, nnz, l)
        if need == 0 or l == 0:
            raise GloveHipError("csr_spmm takes 1 <= n_rows, nnz <= 2^31 - 1 and l %% 4 == 0 in [4, 1024]: got n_rows = %d, "
                                "nnz = %d, l = %d" % (n_rows, nnz, l))
        ws = torch.empty(need, dtype=torch.uint8, device=B.device) if ws is None else ws
        Y = torch.empty(n_rows, l, dtype=torch.float32, device=B.device)
        _check(lib.glove_csr_spmm_f32(_ptr(row_ptr), _ptr(col_idx), _ptr(val), n_rows, n_cols, nnz, _ptr(B), l, _ptr(Y),
                                      _ptr(ws), ws.numel(), _stream()), "glove_csr_spmm_f32")
        return Y

    def csr_row_sums(self, row_ptr: torch.Tensor, val: torch.Tensor, n_rows: int) -> torch.Tensor:
        """The sum of every CSR row's values in float64 [n_rows] (the marginals), in a fixed order."""
        nnz = self._csr_args(row_ptr, None, val, n_rows)
        lib = load_factor_library()
        need = lib.glove_csr_spmm_workspace_bytes(n_rows, nnz, 0)
        if need == 0:
            raise GloveHipError("csr_row_sums takes 1 <= n_rows and nnz <= 2^31 - 1: got n_rows = %d, nnz = %d" % (n_rows, nnz))
        ws = torch.empty(need, dtype=torch.uint8, device=val.device)
        sums = torch.empty(n_rows, dtype=torch.float64, device=val.device)
        _check(lib.glove_csr_row_sums_f64(_ptr(row_ptr), _ptr(val), n_rows, nnz, _ptr(sums), _ptr(ws), ws.numel(), _stream()),
               "glove_csr_row_sums_f64")
        return sums

    def coo_reweight(self, row: torch.Tensor, col: torch.Tensor, val: torch.Tensor, kind: str, row_sums=None,
                     col_weights=None, total: float = 0.0, log_shift: float = 0.0, out: torch.Tensor | None = None) -> torch.Tensor:
        """The entrywise transform `kind` (none, sqrt, log1p, ppmi) of a COO table's float32 values, computed in float64:
        ppmi is max(0, log(x total / (row_sums[row] col_weights[col])) - log_shift) with float64 marginals.  `out` may be
        `val` itself.  The ids must index the marginals: the kernel does not look."""
        if kind not in REWEIGHT_KINDS:
            raise GloveHipError("kind must be one of %s, got %r" % (", ".join(REWEIGHT_KINDS), kind))
        _require(val, torch.float32)
        nnz = int(val.numel())
        _require(row, torch.int32, nnz); _require(col, torch.int32, nnz)
        _require(row_sums, torch.float64); _require(col_weights, torch.float64)
        if kind == "ppmi" and (row is None or col is None or row_sums is None or col_weights is None):
            raise GloveHipError("ppmi needs row, col, row_sums and col_weights")
        out = torch.empty_like(val) if out is None else out
        _require(out, torch.float32, nnz)
        _check(load_factor_library().glove_coo_reweight_f32(_ptr(row), _ptr(col), _ptr(val), nnz, REWEIGHT_KINDS[kind],
                                                            _ptr(row_sums), _ptr(col_weights), float(total), float(log_shift),
                                                            _ptr(out), _stream()), "glove_coo_reweight_f32")
        return out

    # ---- post-processing of a finished table (include/glove_factor_dense_hip.h): what trainer.postprocess drives
    def _dense_args(self, X: torch.Tensor, what: str):
        _require(X, torch.float32)
        if X.dim() != 2:
            raise GloveHipError("%s: expected a table [n, d], got %s" % (what, tuple(X.shape)))
        n, d = int(X.shape[0]), int(X.shape[1])
        lib = load_factor_library()
        need = lib.glove_gram_workspace_bytes(n, d)
        if need == 0:
            raise GloveHipError("%s takes 1 <= n <= 2^31 - 1 and d %% 4 == 0 in [4, 1024]: got n = %d, d = %d" % (what, n, d))
        return lib, n, d, need

    def col_sums(self, X: torch.Tensor, ws: torch.Tensor | None = None) -> torch.Tensor:
        """The column sums of X [n, d] float32 in float64 [d], in a fixed order (bitwise repeatable)."""
        lib, n, d, need = self._dense_args(X, "col_sums")
        ws = torch.empty(need, dtype=torch.uint8, device=X.device) if ws is None else ws
        sums = torch.empty(d, dtype=torch.float64, device=X.device)
        _check(lib.glove_col_sums_f64(_ptr(X), n, d, _ptr(sums), _ptr(ws), ws.numel(), _stream()), "glove_col_sums_f64")
        return sums

    def gram(self, X: torch.Tensor, mean: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> torch.Tensor:
        """G [d, d] float64 = X~^T X~ for X [n, d] float32, X~ = the float32 difference X - mean (mean float32 [d], or
        None: X itself): float32 fmaf chains over chunks of GRAM_CHUNK rows, added in float64.  Exactly symmetric and
        bitwise repeatable (no float atomics)."""
        lib, n, d, need = self._dense_args(X, "gram")
        _require(mean, torch.float32, d)
        ws = torch.empty(need, dtype=torch.uint8, device=X.device) if ws is None else ws
        G = torch.empty(d, d, dtype=torch.float64, device=X.device)
        _check(lib.glove_gram_f64(_ptr(X), n, d, _ptr(mean), _ptr(G), _ptr(ws), ws.numel(), _stream()), "glove_gram_f64")
        return G

    def rows_transform(self, X: torch.Tensor, T: torch.Tensor, shift: torch.Tensor | None = None,
                       out: torch.Tensor | None = None) -> torch.Tensor:
        """Y [n, m] float32 = X T^T - shift for X [n, d] and T [m, d] float32 (m % 4 == 0 up to 1024; shift float32 [m]
        or None): a k-ordered fmaf chain per entry, the shift subtracted once.  `out` must not be X."""
        lib, n, d, _ = self._dense_args(X, "rows_transform")
        _require(T, torch.float32)
        if T.dim() != 2 or T.shape[1] != d:
            raise GloveHipError("expected T [m, d = %d], got %s" % (d, tuple(T.shape)))
        m = int(T.shape[0])
        if m < 4 or m > 1024 or m % 4:
            raise GloveHipError("rows_transform takes m %% 4 == 0 in [4, 1024]: got m = %d" % m)
        _require(shift, torch.float32, m)
        Y = torch.empty(n, m, dtype=torch.float32, device=X.device) if out is None else out
        _require(Y, torch.float32, n * m)
        _check(lib.glove_rows_transform_f32(_ptr(X), n, d, _ptr(T), m, _ptr(shift), _ptr(Y), _stream()),
               "glove_rows_transform_f32")
        return Y

    # ---- the cross-covariance of row pairs (include/glove_factor_align_hip.h): what trainer.align fits its map on
    def cross_gram(self, X: torch.Tensor, xid: torch.Tensor, Y: torch.Tensor, yid: torch.Tensor,
                   x_scale: torch.Tensor | None = None, y_scale: torch.Tensor | None = None,
                   ws: torch.Tensor | None = None) -> torch.Tensor:
        """M [d, d] float64 = sum over the pairs p of the outer product of X[xid[p]] x_scale[xid[p]] and
        Y[yid[p]] y_scale[yid[p]] (float32 products; a null scale leaves the row as it is) for X [Vx, d] and Y [Vy, d]
        float32 of one row stride: float32 fmaf chains over chunks of GRAM_CHUNK pairs, added in float64.  Bitwise
        repeatable (no float atomics).  The ids must lie in [0, Vx) and [0, Vy): the kernels do not look."""
        _require(X, torch.float32); _require(Y, torch.float32); _require(xid, torch.int32)
        if X.dim() != 2 or Y.dim() != 2 or X.shape[1] != Y.shape[1] or xid.dim() != 1:
            raise GloveHipError("cross_gram: expected X [Vx, d], Y [Vy, d] of one row stride and xid, yid [n]")
        (Vx, d), Vy, n = X.shape, int(Y.shape[0]), int(xid.numel())
        _require(yid, torch.int32, n)
        _require(x_scale, torch.float32, Vx); _require(y_scale, torch.float32, Vy)
        lib = load_factor_library()
        need = lib.glove_cross_gram_workspace_bytes(n, d)
        if need == 0 or Vx < 1 or Vy < 1:
            raise GloveHipError("cross_gram takes 1 <= n <= 2^31 - 1 pairs and d %% 4 == 0 in [4, 1024]: got n = %d, d = %d" % (n, d))
        ws = torch.empty(need, dtype=torch.uint8, device=X.device) if ws is None else ws
        M = torch.empty(d, d, dtype=torch.float64, device=X.device)
        _check(lib.glove_cross_gram_f64(_ptr(X), Vx, _ptr(Y), Vy, d, _ptr(xid), _ptr(yid), n, _ptr(x_scale), _ptr(y_scale),
                                        _ptr(M), _ptr(ws), ws.numel(), _stream()), "glove_cross_gram_f64")
        return M

    # ---- retrofitting to a lexicon (include/glove_factor_graph_hip.h): what trainer.retrofit drives
    def retrofit_rows(self, row_ptr: torch.Tensor, col_idx: torch.Tensor, beta: torch.Tensor | None,
                      rows: torch.Tensor | None, Q_hat: torch.Tensor, Q_in: torch.Tensor, Q_out: torch.Tensor,
                      alpha: float = 1.0) -> torch.Tensor:
        """One retrofitting update of the listed rows (`rows` int32, or None: every row) of the table [n, d]:
        Q_out[i] = (alpha w_i Q_hat[i] + sum_p beta[p] Q_in[col_idx[p]]) / (alpha w_i + w_i) over the positions p of row i
        of the square CSR graph (row_ptr int64 [n + 1], col_idx int32 [nnz], beta float32 [nnz] or None: all 1), w_i the sum
        of the row's weights; a listed row without positions is copied from Q_in, an unlisted one is not touched.  The
        summation order is the header's: bitwise repeatable.  Q_out may be Q_in (the in-place sweep) when no listed row is
        a column of another listed row — the kernel does not look; Q_out must not be Q_hat.  -> Q_out."""
        _require(Q_hat, torch.float32); _require(Q_in, torch.float32); _require(Q_out, torch.float32)
        if Q_hat.dim() != 2 or Q_in.shape != Q_hat.shape or Q_out.shape != Q_hat.shape:
            raise GloveHipError("expected three tables [n, d] of one shape, got %s, %s and %s"
                                % (tuple(Q_hat.shape), tuple(Q_in.shape), tuple(Q_out.shape)))
        n, d = int(Q_hat.shape[0]), int(Q_hat.shape[1])
        if n < 1 or n > 2 ** 31 - 1 or d < 4 or d > 1024 or d % 4:
            raise GloveHipError("retrofit_rows takes 1 <= n <= 2^31 - 1 and d %% 4 == 0 in [4, 1024]: got n = %d, d = %d" % (n, d))
        _require(row_ptr, torch.int64, n + 1); _require(col_idx, torch.int32)
        if row_ptr is None or col_idx is None:
            raise GloveHipError("retrofit_rows needs row_ptr and col_idx")
        nnz = int(col_idx.numel())
        _require(beta, torch.float32, nnz); _require(rows, torch.int32)
        n_list = n if rows is None else int(rows.numel())
        alpha = float(alpha)
        if not (np.isfinite(alpha) and alpha >= 0.0):
            raise GloveHipError("alpha must be finite and not negative, got %r" % alpha)
        if n_list > n:
            raise GloveHipError("%d rows listed for a table of %d" % (n_list, n))
        _check(load_factor_library().glove_retrofit_rows_f32(_ptr(row_ptr), _ptr(col_idx), _ptr(beta), n, nnz, _ptr(rows),
                                                             n_list, _ptr(Q_hat), _ptr(Q_in), _ptr(Q_out), d, alpha, _stream()),
               "glove_retrofit_rows_f32")
        return Q_out

    # ---- data prep
    def cooccurrence(self, tokens: torch.Tensor, V: int, context: int, cap: int | None = None):
        """(row i32, col i32, count i64, value f64) sorted by (row, col): the symmetrised window
        co-occurrence table of reference src/data/text8.py:84-108 (one host sync for the size)."""
        _require(tokens, torch.int32)
        n = int(tokens.numel())
        cap = int(cap if cap is not None else max(1, 2 * context * n))
        dev = tokens.device
        row = torch.empty(cap, dtype=torch.int32, device=dev)
        col = torch.empty(cap, dtype=torch.int32, device=dev)
        cnt = torch.empty(cap, dtype=torch.int64, device=dev)
        val = torch.empty(cap, dtype=torch.float64, device=dev)
        nnz = torch.zeros(1, dtype=torch.int64, device=dev)
        ws = torch.empty(self.lib.glove_cooc_workspace_bytes(n, context), dtype=torch.uint8, device=dev)
        _check(self.lib.glove_cooccurrence_i32(_ptr(tokens), n, V, context, _ptr(row), _ptr(col), _ptr(cnt), _ptr(val),
                                               _ptr(nnz), cap, _ptr(ws), ws.numel(), _stream()),
               "glove_cooccurrence_i32")
        m = int(nnz.item())
        if m > cap:
            raise GloveHipError("co-occurrence table has %d entries, capacity %d" % (m, cap))
        return row[:m], col[:m], cnt[:m], val[:m]

    # ---- data prep, chunk by chunk (include/glove_cooc_stream_hip.h): what trainer.cooccur.CoocAccumulator drives
    def _bytes(self, n: int, what: str) -> torch.Tensor:
        if n == 0:
            raise GloveHipError("%s: sizes out of range" % what)
        return torch.empty(n, dtype=torch.uint8, device=self.device)

    def cooc_chunk_keys_enqueue(self, tokens, n_own: int, V: int, context: int, keys_out, counts_out, n_out, ws=None):
        """glove_cooc_chunk_keys_i32 on the current stream, nothing read back: tokens [n_total] int32 (own positions, then
        the halo), keys_out / counts_out int64 [cap] (a key's bits are those of the header's uint64), n_out int64 [>= 2]."""
        lib = load_prep_library()
        _require(tokens, torch.int32); _require(keys_out, torch.int64); _require(n_out, torch.int64)
        _require(counts_out, torch.int64, int(keys_out.numel()))
        n_total = int(tokens.numel())
        if ws is None:
            ws = self._bytes(lib.glove_cooc_chunk_workspace_bytes(n_total, context), "glove_cooc_chunk_workspace_bytes")
        _check(lib.glove_cooc_chunk_keys_i32(_ptr(tokens), int(n_own), n_total, V, context, _ptr(keys_out), _ptr(counts_out),
                                             _ptr(n_out), int(keys_out.numel()), _ptr(ws), ws.numel(), _stream()),
               "glove_cooc_chunk_keys_i32")

    def cooc_merge_enqueue(self, keys_a, counts_a, n_a, keys_b, counts_b, n_b, keys_out, counts_out, n_out, ws=None):
        """glove_cooc_merge_u64 on the current stream, nothing read back; n_a, n_b, n_out are int64 device tensors."""
        lib = load_prep_library()
        for k, c in ((keys_a, counts_a), (keys_b, counts_b), (keys_out, counts_out)):
            _require(k, torch.int64); _require(c, torch.int64, int(k.numel()))
        for t in (n_a, n_b, n_out):
            _require(t, torch.int64)
        cap_a, cap_b = int(keys_a.numel()), int(keys_b.numel())
        if ws is None:
            ws = self._bytes(lib.glove_cooc_merge_workspace_bytes(cap_a, cap_b), "glove_cooc_merge_workspace_bytes")
        _check(lib.glove_cooc_merge_u64(_ptr(keys_a), _ptr(counts_a), _ptr(n_a), cap_a, _ptr(keys_b), _ptr(counts_b), _ptr(n_b),
                                        cap_b, _ptr(keys_out), _ptr(counts_out), _ptr(n_out), int(keys_out.numel()),
                                        _ptr(ws), ws.numel(), _stream()), "glove_cooc_merge_u64")

    def cooc_finalize_enqueue(self, keys, counts, n, V: int, context: int, min_count: int, row, col, cnt, val, nnz, ws=None,
                              weighting: str = "harmonic"):
        """glove_cooc_finalize on the current stream, nothing read back; n and nnz are int64 device tensors (nnz [>= 2]).
        Another `weighting` than the default ("uniform", "dynamic") goes to glove_cooc_finalize_weighted
        (include/glove_cooc_options_hip.h); the workspace is the same."""
        lib = load_prep_library()
        if weighting not in WINDOW_WEIGHTINGS:
            raise GloveHipError("weighting must be one of %s, got %r" % (sorted(WINDOW_WEIGHTINGS), weighting))
        _require(keys, torch.int64); _require(counts, torch.int64, int(keys.numel())); _require(n, torch.int64)
        cap = int(row.numel())
        _require(row, torch.int32); _require(col, torch.int32, cap); _require(cnt, torch.int64, cap)
        _require(val, torch.float64, cap); _require(nnz, torch.int64)
        if ws is None:
            ws = self._bytes(lib.glove_cooc_finalize_workspace_bytes(int(keys.numel())), "glove_cooc_finalize_workspace_bytes")
        if weighting != "harmonic":
            _check(lib.glove_cooc_finalize_weighted(_ptr(keys), _ptr(counts), _ptr(n), int(keys.numel()), V, context,
                                                    int(min_count), WINDOW_WEIGHTINGS[weighting], _ptr(row), _ptr(col), _ptr(cnt),
                                                    _ptr(val), _ptr(nnz), cap, _ptr(ws), ws.numel(), _stream()),
                   "glove_cooc_finalize_weighted")
            return
        _check(lib.glove_cooc_finalize(_ptr(keys), _ptr(counts), _ptr(n), int(keys.numel()), V, context, int(min_count),
                                       _ptr(row), _ptr(col), _ptr(cnt), _ptr(val), _ptr(nnz), cap, _ptr(ws), ws.numel(),
                                       _stream()), "glove_cooc_finalize")

    def cooc_chunk_keys(self, tokens: torch.Tensor, n_own: int, V: int, context: int, cap: int | None = None):
        """(keys int64, counts int64): the distinct (row, col, distance) keys of a chunk, ascending, and how often each
        occurred.  tokens [n_own + halo]: a pair belongs to the chunk that owns its left position (one host sync for the size)."""
        cap = int(cap if cap is not None else max(1, 2 * context * int(n_own)))
        keys = torch.empty(cap, dtype=torch.int64, device=tokens.device)
        counts = torch.empty(cap, dtype=torch.int64, device=tokens.device)
        n_out = torch.zeros(2, dtype=torch.int64, device=tokens.device)
        self.cooc_chunk_keys_enqueue(tokens, n_own, V, context, keys, counts, n_out)
        m = int(n_out[0].item())
        if m > cap:
            raise GloveHipError("the chunk has %d distinct keys, capacity %d" % (m, cap))
        return keys[:m], counts[:m]

    def cooc_merge(self, keys_a, counts_a, keys_b, counts_b, keys_out=None, counts_out=None):
        """The ascending union of two strictly ascending key tables, counts of shared keys summed -> (keys, counts), views
        of `keys_out` / `counts_out` (default: fresh ones that hold both inputs).  One host sync for the size."""
        n_a, n_b = int(keys_a.numel()), int(keys_b.numel())
        if keys_out is None:
            keys_out = torch.empty(max(1, n_a + n_b), dtype=torch.int64, device=keys_a.device)
            counts_out = torch.empty_like(keys_out)
        sizes = torch.tensor([n_a, n_b, 0, 0], dtype=torch.int64).to(keys_a.device)
        self.cooc_merge_enqueue(keys_a, counts_a, sizes[0:1], keys_b, counts_b, sizes[1:2], keys_out, counts_out, sizes[2:4])
        m = int(sizes[2].item())
        if m > keys_out.numel():
            raise GloveHipError("the merged table has %d keys, capacity %d" % (m, keys_out.numel()))
        return keys_out[:m], counts_out[:m]

    def cooc_finalize(self, keys, counts, V: int, context: int, min_count: int = 0, cap: int | None = None,
                      weighting: str = "harmonic"):
        """(row i32, col i32, count i64, value f64) sorted by (row, col) from a key table: what `cooccurrence` returns for
        the corpus the keys were counted from, bit for bit, cut to the pairs with count >= min_count (one host sync).
        weighting "uniform": value = count; "dynamic": value = sum_k n_k (context - k + 1) / context."""
        n = int(keys.numel())
        cap = int(cap if cap is not None else max(1, n))
        dev = keys.device
        row = torch.empty(cap, dtype=torch.int32, device=dev)
        col = torch.empty(cap, dtype=torch.int32, device=dev)
        cnt = torch.empty(cap, dtype=torch.int64, device=dev)
        val = torch.empty(cap, dtype=torch.float64, device=dev)
        sizes = torch.tensor([n, 0, 0], dtype=torch.int64).to(dev)
        self.cooc_finalize_enqueue(keys, counts, sizes[0:1], V, context, min_count, row, col, cnt, val, sizes[1:3],
                                   weighting=weighting)
        m = int(sizes[1].item())
        if m > cap:
            raise GloveHipError("co-occurrence table has %d entries, capacity %d" % (m, cap))
        return row[:m], col[:m], cnt[:m], val[:m]

    # ---- removing tokens before the window is laid (include/glove_cooc_options_hip.h): what trainer.cooccur.filter_blocks drives
    def token_filter_enqueue(self, ids, pos0: int, thresholds, seed: int, ids_out, n_out, ws=None):
        """glove_token_filter_i32 on the current stream, nothing read back: ids int32 [n], thresholds int32 [V] (the bits of
        the header's uint32), ids_out int32 [cap], n_out an int64 device tensor ([>= 2] where the block may be empty)."""
        lib = load_prep_library()
        _require(ids, torch.int32); _require(thresholds, torch.int32); _require(ids_out, torch.int32); _require(n_out, torch.int64)
        n = int(ids.numel())
        if ws is None:
            ws = self._bytes(lib.glove_token_filter_workspace_bytes(n), "glove_token_filter_workspace_bytes")
        _check(lib.glove_token_filter_i32(_ptr(ids), n, int(pos0), _ptr(thresholds), int(thresholds.numel()),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(ids_out), _ptr(n_out), int(ids_out.numel()),
                                          _ptr(ws), ws.numel(), _stream()), "glove_token_filter_i32")

    def token_filter(self, ids: torch.Tensor, pos0: int, thresholds, seed: int = 0):
        """The ids that survive the keep rule of include/glove_cooc_options_hip.h, in stream order: the token at index i
        has the global position pos0 + i.  thresholds: uint32 [V] as a numpy array, or its bits as an int32 device tensor
        (one host sync for the size)."""
        if isinstance(thresholds, np.ndarray):
            thresholds = torch.from_numpy(np.ascontiguousarray(thresholds, np.uint32).view(np.int32).copy()).to(ids.device)
        out = torch.empty(max(1, int(ids.numel())), dtype=torch.int32, device=ids.device)
        n_out = torch.zeros(2, dtype=torch.int64, device=ids.device)
        self.token_filter_enqueue(ids, pos0, thresholds, seed, out, n_out)
        return out[:int(n_out[0].item())]

    # ---- tokenizing and numbering a corpus (include/glove_text_hip.h): what trainer.cooccur drives with --tokenizer device.
    # Hashes and vocabulary keys travel as int64 tensors whose bits are the header's uint64.
    def text_tokenize_enqueue(self, block, start, length, hashes, n_tokens, n_long, ws=None):
        """glove_text_tokenize_u8 on the current stream, nothing read back: block uint8 [n_bytes]; start / length int32
        [cap], hashes int64 [cap]; n_tokens and n_long int64 device tensors ([>= 2] each where the block may be empty)."""
        lib = load_prep_library()
        _require(block, torch.uint8); _require(start, torch.int32); _require(length, torch.int32, int(start.numel()))
        _require(hashes, torch.int64, int(start.numel())); _require(n_tokens, torch.int64); _require(n_long, torch.int64)
        n_bytes = int(block.numel())
        if ws is None:
            ws = self._bytes(lib.glove_text_tokenize_workspace_bytes(n_bytes), "glove_text_tokenize_workspace_bytes")
        _check(lib.glove_text_tokenize_u8(_ptr(block) if n_bytes else None, n_bytes, _ptr(start), _ptr(length), _ptr(hashes),
                                          _ptr(n_tokens), _ptr(n_long), int(start.numel()), _ptr(ws), ws.numel(), _stream()),
               "glove_text_tokenize_u8")

    def text_block_vocab_enqueue(self, hashes, start, length, n_tokens, base_offset: int, keys, counts, where, n_out, ws=None):
        """glove_text_block_vocab on the current stream, nothing read back; n_tokens int64 [>= 1], n_out int64 [>= 2]."""
        lib = load_prep_library()
        cap_tokens, cap_out = int(hashes.numel()), int(keys.numel())
        _require(hashes, torch.int64); _require(start, torch.int32, cap_tokens); _require(length, torch.int32, cap_tokens)
        _require(keys, torch.int64); _require(counts, torch.int64, cap_out); _require(where, torch.int64, cap_out)
        _require(n_tokens, torch.int64); _require(n_out, torch.int64)
        if ws is None:
            ws = self._bytes(lib.glove_text_block_vocab_workspace_bytes(cap_tokens), "glove_text_block_vocab_workspace_bytes")
        _check(lib.glove_text_block_vocab(_ptr(hashes), _ptr(start), _ptr(length), _ptr(n_tokens), cap_tokens, int(base_offset),
                                          _ptr(keys), _ptr(counts), _ptr(where), _ptr(n_out), cap_out, _ptr(ws), ws.numel(),
                                          _stream()), "glove_text_block_vocab")

    def text_vocab_merge_enqueue(self, a, n_a, b, n_b, out, n_out, ws=None):
        """glove_text_vocab_merge on the current stream, nothing read back: a, b, out are (keys, counts, where) triples of
        int64 tensors, n_a, n_b, n_out int64 device tensors."""
        lib = load_prep_library()
        for triple in (a, b, out):
            for t in triple:
                _require(t, torch.int64, int(triple[0].numel()))
        for t in (n_a, n_b, n_out):
            _require(t, torch.int64)
        cap_a, cap_b = int(a[0].numel()), int(b[0].numel())
        if ws is None:
            ws = self._bytes(lib.glove_text_vocab_merge_workspace_bytes(cap_a, cap_b), "glove_text_vocab_merge_workspace_bytes")
        _check(lib.glove_text_vocab_merge(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(n_a), cap_a, _ptr(b[0]), _ptr(b[1]), _ptr(b[2]),
                                          _ptr(n_b), cap_b, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(n_out),
                                          int(out[0].numel()), _ptr(ws), ws.numel(), _stream()), "glove_text_vocab_merge")

    def text_token_ids_enqueue(self, block, start, length, hashes, n_tokens, kept, ids, n_mismatch):
        """glove_text_token_ids_i32 on the current stream, nothing read back: kept = (keys int64 [n_kept] ascending as
        uint64, ids int32 [n_kept], offsets int64 [n_kept + 1], bytes uint8); ids int32 [cap]; n_mismatch int64 [>= 2]."""
        lib = load_prep_library()
        kept_keys, kept_id, kept_off, kept_bytes = kept
        cap, n_kept = int(hashes.numel()), int(kept_keys.numel())
        _require(block, torch.uint8); _require(hashes, torch.int64); _require(start, torch.int32, cap)
        _require(length, torch.int32, cap); _require(ids, torch.int32, cap); _require(n_tokens, torch.int64)
        _require(kept_keys, torch.int64); _require(kept_id, torch.int32, n_kept); _require(kept_off, torch.int64, n_kept + 1)
        _require(kept_bytes, torch.uint8); _require(n_mismatch, torch.int64)
        _check(lib.glove_text_token_ids_i32(_ptr(block) if block.numel() else None, int(block.numel()), _ptr(start), _ptr(length),
                                            _ptr(hashes), _ptr(n_tokens), cap, _ptr(kept_keys) if n_kept else None,
                                            _ptr(kept_id) if n_kept else None, _ptr(kept_off),
                                            _ptr(kept_bytes) if n_kept else None, n_kept, _ptr(ids), _ptr(n_mismatch), _stream()),
               "glove_text_token_ids_i32")

    def text_tokenize(self, block: torch.Tensor):
        """(start int32, length int32, hashes int64, n_long): the whitespace-separated tokens of a block of bytes, in order
        (one host sync for the sizes).  n_long: tokens longer than TEXT_MAX_TOKEN bytes, which their hash does not cover."""
        cap = (int(block.numel()) + 1) // 2         # the most tokens the bytes can hold
        start = torch.empty(cap, dtype=torch.int32, device=block.device)
        length = torch.empty_like(start)
        hashes = torch.empty(cap, dtype=torch.int64, device=block.device)
        sizes = torch.zeros(4, dtype=torch.int64, device=block.device)
        self.text_tokenize_enqueue(block, start, length, hashes, sizes[0:2], sizes[2:4])
        m, n_long = (int(v) for v in sizes[0:3:2].tolist())
        return start[:m], length[:m], hashes[:m], n_long

    def text_block_vocab(self, hashes, start, length, base_offset: int = 0):
        """(keys, counts, where) of a block's tokens: the distinct hashes ascending (as uint64), how often each occurred,
        and ((base_offset + start of the first occurrence) << 16) | min(length, TEXT_MAX_TOKEN).  One host sync."""
        n = int(hashes.numel())
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=hashes.device)
        counts, where = torch.empty_like(keys), torch.empty_like(keys)
        sizes = torch.tensor([n, 0, 0], dtype=torch.int64).to(hashes.device)
        self.text_block_vocab_enqueue(hashes, start, length, sizes[0:1], base_offset, keys, counts, where, sizes[1:3])
        m = int(sizes[1].item())
        return keys[:m], counts[:m], where[:m]

    def text_vocab_merge(self, keys_a, counts_a, where_a, keys_b, counts_b, where_b, keys_out=None, counts_out=None,
                         where_out=None):
        """The ascending union of two vocabularies, counts summed and the smaller `where` kept for shared keys ->
        (keys, counts, where), views of the outputs (default: fresh ones that hold both inputs).  One host sync."""
        n_a, n_b = int(keys_a.numel()), int(keys_b.numel())
        if keys_out is None:
            keys_out = torch.empty(max(1, n_a + n_b), dtype=torch.int64, device=keys_a.device)
            counts_out, where_out = torch.empty_like(keys_out), torch.empty_like(keys_out)
        sizes = torch.tensor([n_a, n_b, 0, 0], dtype=torch.int64).to(keys_a.device)
        self.text_vocab_merge_enqueue((keys_a, counts_a, where_a), sizes[0:1], (keys_b, counts_b, where_b), sizes[1:2],
                                      (keys_out, counts_out, where_out), sizes[2:4])
        m = int(sizes[2].item())
        if m > keys_out.numel():
            raise GloveHipError("the merged vocabulary has %d keys, capacity %d" % (m, keys_out.numel()))
        return keys_out[:m], counts_out[:m], where_out[:m]

    def text_token_ids(self, block, start, length, hashes, kept):
        """(ids int32, n_mismatch): every token's id from the kept table (see text_token_ids_enqueue), 0 where its hash
        is not kept; n_mismatch counts tokens whose hash is kept but whose bytes are another word's (one host sync)."""
        ids = torch.empty(int(hashes.numel()), dtype=torch.int32, device=hashes.device)
        sizes = torch.tensor([int(hashes.numel()), 0, 0], dtype=torch.int64).to(hashes.device)
        self.text_token_ids_enqueue(block, start, length, hashes, sizes[0:1], kept, ids, sizes[1:3])
        return ids, int(sizes[1].item())

    # ---- phrase detection (include/glove_phrases_hip.h): what trainer.phrases drives.  Bigram keys travel as int64 tensors
    # whose bits are the header's uint64 (an id is below 2^31, so they are the same numbers).
    def phrase_bigram_keys_enqueue(self, block, start, length, ids, n_tokens, keys_out, counts_out, n_out, ws=None):
        """glove_phrase_bigram_keys_i32 on the current stream, nothing read back: block uint8 [n_bytes]; start / length / ids
        int32 [cap_tokens]; n_tokens int64 [>= 1]; keys_out / counts_out int64 [cap]; n_out int64 [>= 2]."""
        lib = load_prep_library()
        cap_tokens = int(start.numel())
        _require(block, torch.uint8); _require(start, torch.int32); _require(length, torch.int32, cap_tokens)
        _require(ids, torch.int32, cap_tokens); _require(n_tokens, torch.int64); _require(keys_out, torch.int64)
        _require(counts_out, torch.int64, int(keys_out.numel())); _require(n_out, torch.int64)
        if ws is None:
            ws = self._bytes(lib.glove_phrase_bigram_workspace_bytes(cap_tokens), "glove_phrase_bigram_workspace_bytes")
        _check(lib.glove_phrase_bigram_keys_i32(_ptr(block) if block.numel() else None, int(block.numel()), _ptr(start),
                                                _ptr(length), _ptr(ids), _ptr(n_tokens), cap_tokens, _ptr(keys_out),
                                                _ptr(counts_out), _ptr(n_out), int(keys_out.numel()), _ptr(ws), ws.numel(),
                                                _stream()), "glove_phrase_bigram_keys_i32")

    def phrase_select_enqueue(self, keys, counts, n, unigram, total_tokens: int, min_count: int, threshold: float, keys_out,
                              counts_out, score_out, n_out, ws=None):
        """glove_phrase_select on the current stream, nothing read back: keys / counts int64 [cap_keys], n int64 [>= 1],
        unigram int64 [V]; keys_out / counts_out int64 [cap_out], score_out float64 [cap_out], n_out int64 [>= 2]."""
        lib = load_prep_library()
        cap_keys, cap_out = int(keys.numel()), int(keys_out.numel())
        _require(keys, torch.int64); _require(counts, torch.int64, cap_keys); _require(n, torch.int64)
        _require(unigram, torch.int64); _require(keys_out, torch.int64); _require(counts_out, torch.int64, cap_out)
        _require(score_out, torch.float64, cap_out); _require(n_out, torch.int64)
        if ws is None:
            ws = self._bytes(lib.glove_phrase_select_workspace_bytes(cap_keys), "glove_phrase_select_workspace_bytes")
        _check(lib.glove_phrase_select(_ptr(keys), _ptr(counts), _ptr(n), cap_keys, _ptr(unigram), int(unigram.numel()),
                                       int(total_tokens), int(min_count), float(threshold), _ptr(keys_out), _ptr(counts_out),
                                       _ptr(score_out), _ptr(n_out), cap_out, _ptr(ws), ws.numel(), _stream()),
               "glove_phrase_select")

    def phrase_join_enqueue(self, block, start, length, ids, n_tokens, phrase_keys, n_phrases, delimiter: int, carry, joined,
                            n_joined, ws=None):
        """glove_phrase_join_u8 on the current stream, nothing read back: block uint8 [n_bytes], rewritten in place; start /
        length / ids int32 [cap_tokens]; n_tokens, n_phrases int64 [>= 1]; phrase_keys, joined int64 [cap_phrases]; carry
        int32 [1]; n_joined int64 [>= 2]."""
        lib = load_prep_library()
        cap_tokens, cap_phrases = int(start.numel()), int(phrase_keys.numel())
        _require(block, torch.uint8); _require(start, torch.int32); _require(length, torch.int32, cap_tokens)
        _require(ids, torch.int32, cap_tokens); _require(n_tokens, torch.int64); _require(phrase_keys, torch.int64)
        _require(n_phrases, torch.int64); _require(carry, torch.int32, 1); _require(joined, torch.int64, cap_phrases)
        _require(n_joined, torch.int64)
        if ws is None:
            ws = self._bytes(lib.glove_phrase_join_workspace_bytes(cap_tokens), "glove_phrase_join_workspace_bytes")
        _check(lib.glove_phrase_join_u8(_ptr(block) if block.numel() else None, int(block.numel()), _ptr(start), _ptr(length),
                                        _ptr(ids), _ptr(n_tokens), cap_tokens, _ptr(phrase_keys) if cap_phrases else None,
                                        _ptr(n_phrases), cap_phrases, int(delimiter), _ptr(carry),
                                        _ptr(joined) if cap_phrases else None, _ptr(n_joined), _ptr(ws), ws.numel(), _stream()),
               "glove_phrase_join_u8")

    def phrase_bigram_keys(self, block, start, length, ids, cap: int | None = None):
        """(keys int64, counts int64): the distinct bigram keys (id << 32 | next id) of a block's plain adjacent pairs of
        kept words, ascending, and how often each occurs (one host sync for the size)."""
        n = int(start.numel())
        cap = int(cap if cap is not None else max(1, n))
        keys = torch.empty(cap, dtype=torch.int64, device=block.device)
        counts = torch.empty_like(keys)
        sizes = torch.tensor([n, 0, 0], dtype=torch.int64).to(block.device)
        self.phrase_bigram_keys_enqueue(block, start, length, ids, sizes[0:1], keys, counts, sizes[1:3])
        m = int(sizes[1].item())
        if m > cap:
            raise GloveHipError("the block has %d distinct bigrams, capacity %d" % (m, cap))
        return keys[:m], counts[:m]

    def phrase_select(self, keys, counts, unigram, total_tokens: int, min_count: int, threshold: float, cap: int | None = None):
        """(keys int64, counts int64, scores float64): the bigrams with count >= min_count and
        (count - min_count) / unigram[a] / unigram[b] * total_tokens > threshold, keys ascending (one host sync)."""
        n = int(keys.numel())
        cap = int(cap if cap is not None else max(1, n))
        out_keys = torch.empty(cap, dtype=torch.int64, device=keys.device)
        out_counts = torch.empty_like(out_keys)
        scores = torch.empty(cap, dtype=torch.float64, device=keys.device)
        sizes = torch.tensor([n, 0, 0], dtype=torch.int64).to(keys.device)
        if n == 0:                       # (a zero-element tensor has no address to hand over)
            keys = counts = torch.zeros(1, dtype=torch.int64, device=out_keys.device)
        self.phrase_select_enqueue(keys, counts, sizes[0:1], unigram, total_tokens, min_count, threshold, out_keys, out_counts,
                                   scores, sizes[1:3])
        m = int(sizes[1].item())
        if m > cap:
            raise GloveHipError("%d phrases are accepted, capacity %d" % (m, cap))
        return out_keys[:m], out_counts[:m], scores[:m]

    def phrase_join(self, block, start, length, ids, phrase_keys, delimiter: int, carry, joined) -> int:
        """Rewrites `block` in place: the single space of every chosen pair becomes `delimiter`; carry (int32 [1]) takes the
        greedy rule from block to block, joined[j] grows by the joins of phrase_keys[j].  -> the block's joins (one host
        sync)."""
        sizes = torch.tensor([int(start.numel()), int(phrase_keys.numel()), 0, 0], dtype=torch.int64).to(block.device)
        self.phrase_join_enqueue(block, start, length, ids, sizes[0:1], phrase_keys, sizes[1:2], delimiter, carry, joined,
                                 sizes[2:4])
        return int(sizes[2].item())

    # ---- reading and writing word-vector text files (include/glove_vectors_hip.h): what trainer.vectors drives
    def vectors_lines_enqueue(self, block, line_start, line_fields, n_lines, ws=None):
        """glove_vectors_lines_u8 on the current stream, nothing read back: block uint8 [n_bytes]; line_start / line_fields
        int32 [cap]; n_lines an int64 device tensor ([>= 2] where the block may be empty)."""
        lib = load_prep_library()
        cap = int(line_start.numel())
        _require(block, torch.uint8); _require(line_start, torch.int32); _require(line_fields, torch.int32, cap)
        _require(n_lines, torch.int64)
        n_bytes = int(block.numel())
        if ws is None:
            ws = self._bytes(lib.glove_vectors_lines_workspace_bytes(n_bytes, cap), "glove_vectors_lines_workspace_bytes")
        _check(lib.glove_vectors_lines_u8(_ptr(block) if n_bytes else None, n_bytes, _ptr(line_start), _ptr(line_fields),
                                          _ptr(n_lines), cap, _ptr(ws), ws.numel(), _stream()), "glove_vectors_lines_u8")

    def vectors_parse_enqueue(self, block, line_start, n_lines, d: int, vec, word_len, fb_index, fb_span, n_fallback):
        """glove_vectors_parse_f32 on the current stream, nothing read back: vec float32 [cap_lines, ld] (ld % 4 == 0), word_len
        int32 [cap_lines], fb_index / fb_span int64 [cap_fb], n_lines int64 [>= 1], n_fallback int64 [>= 2]."""
        lib = load_prep_library()
        cap_lines, cap_fb = int(line_start.numel()), int(fb_index.numel())
        _require(block, torch.uint8); _require(line_start, torch.int32); _require(word_len, torch.int32, cap_lines)
        _require(vec, torch.float32); _require(fb_index, torch.int64); _require(fb_span, torch.int64, cap_fb)
        _require(n_lines, torch.int64); _require(n_fallback, torch.int64)
        if vec.dim() != 2 or vec.shape[0] != cap_lines:
            raise GloveHipError("vec must be [%d, ld], got %s" % (cap_lines, tuple(vec.shape)))
        _check(lib.glove_vectors_parse_f32(_ptr(block) if block.numel() else None, int(block.numel()), _ptr(line_start), _ptr(n_lines),
                                           cap_lines, int(d), int(vec.shape[1]), _ptr(vec), _ptr(word_len),
                                           _ptr(fb_index) if cap_fb else None, _ptr(fb_span) if cap_fb else None, _ptr(n_fallback),
                                           cap_fb, _stream()), "glove_vectors_parse_f32")

    def vectors_format_enqueue(self, W, d: int, precision: int, word_bytes, word_off, out, row_off, host_row, n_host_rows, ws=None):
        """glove_vectors_format_f32 on the current stream, nothing read back: W float32 [n_rows, ld]; word_bytes uint8, word_off
        int64 [n_rows + 1]; out uint8 [cap_out]; row_off int64 [n_rows + 1]; host_row uint8 [n_rows]; n_host_rows int64 [>= 2]."""
        lib = load_prep_library()
        _require(W, torch.float32)
        if W.dim() != 2:
            raise GloveHipError("W must be [n_rows, ld], got %s" % (tuple(W.shape),))
        n_rows, ld = int(W.shape[0]), int(W.shape[1])
        _require(word_bytes, torch.uint8); _require(word_off, torch.int64, n_rows + 1); _require(out, torch.uint8)
        _require(row_off, torch.int64, n_rows + 1); _require(host_row, torch.uint8, n_rows); _require(n_host_rows, torch.int64)
        if ws is None:
            ws = self._bytes(lib.glove_vectors_format_workspace_bytes(n_rows, int(d)), "glove_vectors_format_workspace_bytes")
        _check(lib.glove_vectors_format_f32(_ptr(W) if n_rows else None, n_rows, int(d), ld, int(precision), _ptr(word_bytes),
                                            _ptr(word_off), _ptr(out) if out.numel() else None, _ptr(row_off),
                                            _ptr(host_row) if n_rows else None, _ptr(n_host_rows), int(out.numel()), _ptr(ws),
                                            ws.numel(), _stream()), "glove_vectors_format_f32")

    def vectors_lines(self, block: torch.Tensor):
        """(line_start int32, line_fields int32): the records of a block of bytes, in order — the offset of each record's word
        and its number of fields, the word included (one host sync for the size)."""
        cap = (int(block.numel()) + 1) // 2         # the most records the bytes can hold
        line_start = torch.empty(cap, dtype=torch.int32, device=block.device)
        line_fields = torch.empty_like(line_start)
        sizes = torch.zeros(2, dtype=torch.int64, device=block.device)
        self.vectors_lines_enqueue(block, line_start, line_fields, sizes)
        m = int(sizes[0].item())
        return line_start[:m], line_fields[:m]

    def vectors_parse(self, block: torch.Tensor, line_start: torch.Tensor, d: int):
        """(vec float32 [m, ld], word_len int32 [m], fb_index int64, fb_span int64): fields 1 .. d of every record as
        np.float32(float(token)), ld = d rounded up to a multiple of four with zero padding columns.  The tokens the device does
        not parse (and does not write) are listed, sorted by fb_index = record * ld + column, with
        fb_span = (byte offset << 16) | min(length, VECTORS_MAX_SPAN).  One host sync, a second one where the list was too short."""
        m, ld = int(line_start.numel()), (int(d) + 3) // 4 * 4
        line_start = line_start.contiguous()
        vec = torch.empty((m, ld), dtype=torch.float32, device=block.device)
        word_len = torch.empty(m, dtype=torch.int32, device=block.device)
        sizes = torch.tensor([m, 0, 0], dtype=torch.int64).to(block.device)
        cap_fb = 4096
        while True:
            fb_index = torch.empty(cap_fb, dtype=torch.int64, device=block.device)
            fb_span = torch.empty_like(fb_index)
            self.vectors_parse_enqueue(block, line_start, sizes[0:1], d, vec, word_len, fb_index, fb_span, sizes[1:3])
            k = int(sizes[1].item())
            if k <= cap_fb:
                break
            cap_fb = k
        order = torch.argsort(fb_index[:k])
        return vec, word_len, fb_index[:k][order], fb_span[:k][order]

    def vectors_format(self, W: torch.Tensor, d: int, precision: int, word_bytes: torch.Tensor, word_off: torch.Tensor, cap_out: int):
        """(out uint8 [size], row_off int64 [n_rows + 1], host_row uint8 [n_rows]): the text `word v1 ... vd\\n` of every row,
        values as "%.*f" % (precision, x); rows that hold a NaN, an infinity or |x| >= 2^31 have length 0 and host_row 1.  Raises
        where the text does not fit cap_out (a row takes at most its word + d (precision + 13) + 1 bytes).  One host sync."""
        n_rows = int(W.shape[0])
        out = torch.empty(int(cap_out), dtype=torch.uint8, device=W.device)
        row_off = torch.empty(n_rows + 1, dtype=torch.int64, device=W.device)
        host_row = torch.empty(n_rows, dtype=torch.uint8, device=W.device)
        sizes = torch.zeros(2, dtype=torch.int64, device=W.device)
        self.vectors_format_enqueue(W, d, precision, word_bytes, word_off, out, row_off, host_row, sizes)
        size = int(row_off[n_rows].item())
        if size > cap_out:
            raise GloveHipError("the text takes %d bytes, capacity %d" % (size, cap_out))
        return out[:size], row_off, host_row
