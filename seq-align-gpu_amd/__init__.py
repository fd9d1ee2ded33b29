"""ctypes binding of libswg (include/swg.h, include/swg_host.h).

This package is plumbing for tests and bench.py: the product is the C-ABI
library next to this file.  Nothing here computes an alignment; if libswg.so
is missing the import fails loudly, and `Context()` raises when there is no
GPU (the library has no CPU backend).

The directory name has a hyphen (it is the name the build contract gives), so
it is imported through `swg_loader.load()` at the repo root, as module
`seq_align_gpu_amd`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libswg.so")
DATA_DIR = os.path.join(_HERE, "data")
CLI_PATH = os.path.join(_HERE, "bin", "smith_waterman")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libswg.so is not built: run `python seq-align-gpu_amd/build.py` "
        "(or __graft_entry__.build()); there is no Python/CPU fallback")

lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)

SWG_OK, SWG_ERR_ARG, SWG_ERR_HIP, SWG_ERR_NOMEM = 0, -1, -2, -3
SWG_ERR_STATE, SWG_ERR_RESIDUE, SWG_ERR_IO, SWG_ERR_NODEVICE = -4, -5, -6, -7

# every symbol declared in include/swg.h and include/swg_host.h
ABI_SYMBOLS = [
    "swg_create", "swg_destroy", "swg_last_error", "swg_global_error", "swg_abi_version", "swg_prune_last",
    "swg_set_option", "swg_set_scoring", "swg_set_query", "swg_set_query_pssm", "swg_db_pack", "swg_db_pack_shard", "swg_db_pack_shards", "swg_db_upload", "swg_db_view",
    "swg_db_free", "swg_db_save", "swg_db_load", "swg_db_count", "swg_db_total_count", "swg_db_residues",
    "swg_db_packed_bytes", "swg_db_order", "swg_search", "swg_search_begin", "swg_search_end", "swg_search_multi",
    "swg_search_multi_pssm", "swg_search_lists", "swg_search_lists_pssm", "swg_search_gapless", "swg_search_gapless_multi",
    "swg_search_gapless_multi_pssm", "swg_search_above", "swg_search_gapless_above", "swg_search_above_multi", "swg_search_above_multi_pssm",
    "swg_search_gapless_above_multi", "swg_search_gapless_above_multi_pssm", "swg_fill_batches16", "swg_align_hits", "swg_align_ops_bound", "swg_align_hits_multi",
    "swg_align_hits_multi_pssm", "swg_align_ops_bound_multi", "swg_align_bounds", "swg_align_bounds_multi",
    "swg_align_bounds_multi_pssm", "swg_align_stats", "swg_align_stats_multi", "swg_align_stats_multi_pssm", "swg_align_hsps",
    "swg_align_hsps_multi", "swg_align_hsps_multi_pssm", "swg_align_hsps_host", "swg_comp_adjust", "swg_comp_adjust_multi",
    "swg_comp_adjust_multi_pssm", "swg_comp_adjust_host", "swg_hit_key",
    "swg_key_hit", "swg_topk_merge_keys",
    "swg_group_create", "swg_group_destroy", "swg_group_size", "swg_group_last_error", "swg_group_set_option",
    "swg_group_set_scoring", "swg_group_set_query", "swg_group_set_query_pssm", "swg_group_load", "swg_group_search",
    "swg_group_align_hits", "swg_group_align_ops_bound", "swg_group_select",
    "swg_letter_index", "swg_index_letter", "swg_scoring_init", "swg_scoring_add",
    "swg_scoring_load_matrix", "swg_query_sanitize", "swg_seqs_read", "swg_seqs_free",
    "swg_seqs_to_indices", "swg_synth_db", "swg_synth_query", "swg_synth_db_similar", "swg_synth_db_family", "swg_synth_db_shard",
    "swg_synth_free", "swg_host_threads", "swg_pssm_load", "swg_pssm_free",
    "swg_db_composition", "swg_calibrate", "swg_calibrate_multi", "swg_calibrate_multi_pssm", "swg_evalue", "swg_bitscore",
    "swg_evalue_min_score", "swg_synth_db_iid", "swg_gumbel_fit_hist",
    "swg_matrix_lambda", "swg_pssm_from_paths", "swg_pssm_from_paths_ex", "swg_pssm_save", "swg_pssm_build", "swg_pssm_build_multi", "swg_pssm_build_multi_pssm",
    "swg_mask_params_default", "swg_mask_tables", "swg_seg_mask", "swg_seg_mask_segments", "swg_db_sequence", "swg_db_mask",
    "swg_db_mask_info", "swg_seg_mask_flat",
    "swg_codon_table", "swg_translate_seq", "swg_translate_flat", "swg_translate_hit", "swg_translate_coords", "swg_db_translate",
    "swg_db_translate_info",
]


class SwgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libswg error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("reserved", C.c_int * 7)]


class Hit(C.Structure):
    _fields_ = [("score", C.c_int32), ("index", C.c_uint32)]


class Alignment(C.Structure):
    _fields_ = [("score", C.c_int32), ("index", C.c_uint32), ("q_begin", C.c_uint32), ("q_end", C.c_uint32),
                ("d_begin", C.c_uint32), ("d_end", C.c_uint32), ("n_ops", C.c_uint32), ("reserved", C.c_uint32)]


class AlignCounts(C.Structure):
    _fields_ = [("n_ident", C.c_uint32), ("n_match", C.c_uint32), ("n_gap_open", C.c_uint32), ("n_gap", C.c_uint32)]


class EvalueParams(C.Structure):
    """swg_evalue_params: the Gumbel fit of a calibrated query and the (lambda, K) read off it."""
    _fields_ = [("lambda_", C.c_double), ("K", C.c_double), ("mu", C.c_double), ("lq", C.c_uint32), ("n_seqs", C.c_uint32),
                ("seq_len", C.c_uint32), ("status", C.c_int32)]

    def as_dict(self):
        return {"lambda": self.lambda_, "K": self.K, "mu": self.mu, "lq": self.lq, "n_seqs": self.n_seqs, "seq_len": self.seq_len,
                "status": self.status}

    @classmethod
    def of(cls, p):
        """From a dict as as_dict gives it (or an EvalueParams, returned as it is)."""
        if isinstance(p, cls):
            return p
        return cls(float(p["lambda"]), float(p["K"]), float(p["mu"]), int(p["lq"]), int(p["n_seqs"]), int(p["seq_len"]), int(p["status"]))


class PssmInfo(C.Structure):
    """swg_pssm_info: what a PSSM construction reports per query."""
    _fields_ = [("lambda_", C.c_double), ("n_distinct", C.c_double), ("n_rows", C.c_uint32), ("n_observed", C.c_uint32),
                ("n_clamped", C.c_uint32), ("n_purged", C.c_uint32)]

    def as_dict(self):
        return {"lambda": self.lambda_, "n_distinct": self.n_distinct, "n_rows": self.n_rows, "n_observed": self.n_observed,
                "n_clamped": self.n_clamped, "n_purged": self.n_purged}


PSSM_PSEUDOCOUNT_DEFAULT = 10.0


class MaskParams(C.Structure):
    """swg_mask_params: the window, the residue index written, and the two entropy bounds in bits."""
    _fields_ = [("window", C.c_int32), ("replace", C.c_int32), ("trigger", C.c_double), ("extend", C.c_double)]


class MaskInfo(C.Structure):
    """swg_mask_info: what swg_db_mask made a database with, what it covered, and what it took."""
    _fields_ = [("params", MaskParams), ("residues_masked", C.c_uint64), ("sequences_masked", C.c_uint64), ("segments", C.c_uint64),
                ("kernel_ms", C.c_double), ("host_image_ms", C.c_double)]

    def as_dict(self):
        return {"window": self.params.window, "replace": self.params.replace, "trigger": self.params.trigger,
                "extend": self.params.extend, "residues_masked": self.residues_masked, "sequences_masked": self.sequences_masked,
                "segments": self.segments, "kernel_ms": self.kernel_ms, "host_image_ms": self.host_image_ms}


MASK_REPLACE_DEFAULT = 24  # swg_letter_index('X')


class TranslateParams(C.Structure):
    """swg_translate_params: the residue index of each of the 64 codons (TCAG order) and of a codon with a non-base."""
    _fields_ = [("codon", C.c_int8 * 64), ("unknown", C.c_int8)]


class TranslateInfo(C.Structure):
    """swg_translate_info: what swg_db_translate made a database with, what it wrote, and what it took."""
    _fields_ = [("params", TranslateParams), ("codons", C.c_uint64), ("stops", C.c_uint64), ("unknown_codons", C.c_uint64),
                ("kernel_ms", C.c_double), ("host_image_ms", C.c_double)]

    def as_dict(self):
        return {"codon": np.array(self.params.codon[:], dtype=np.int8), "unknown": int(self.params.unknown), "codons": self.codons,
                "stops": self.stops, "unknown_codons": self.unknown_codons, "kernel_ms": self.kernel_ms,
                "host_image_ms": self.host_image_ms}


TRANSLATE_UNKNOWN_DEFAULT = 24  # swg_letter_index('X')


class Stats(C.Structure):
    _fields_ = [
        ("cells", C.c_uint64), ("cells_padded", C.c_uint64), ("bytes_alg", C.c_uint64),
        ("n_rescored", C.c_uint64), ("fill_ms", C.c_double), ("rescore_ms", C.c_double),
        ("topk_ms", C.c_double), ("total_ms", C.c_double), ("path_bits", C.c_int32),
        ("cols_per_wave", C.c_int32), ("waves", C.c_int32), ("passes", C.c_int32),
        ("workgroups", C.c_int32), ("engine", C.c_int32), ("group_lanes", C.c_int32),
        ("streams", C.c_int32), ("long_pairs", C.c_int32), ("long_cols_per_lane", C.c_int32),
        ("long_streams", C.c_int32), ("work_queue", C.c_int32), ("classes_overlapped", C.c_int32),
        ("fill_launches", C.c_int32),
        ("cell_form", C.c_int32),
        ("split_rows", C.c_int32),
        ("fill_f16_launches", C.c_int32),
        ("fill_f16_ms", C.c_double),
        ("cells_f16", C.c_uint64),
        ("last_pass_cols", C.c_int32),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("reserved")}


class Batch16(C.Structure):
    _fields_ = [("db_idx_t", C.c_void_p), ("max_len", C.c_size_t), ("vector_size", C.c_size_t),
                ("max_scores", C.c_void_p)]


class Scoring(C.Structure):
    _fields_ = [("gap_open", C.c_int), ("gap_extend", C.c_int), ("match", C.c_int),
                ("mismatch", C.c_int), ("sub", (C.c_int8 * 32) * 32), ("set", C.c_uint32 * 32)]

    def table(self):
        return np.ctypeslib.as_array(self.sub).reshape(32, 32).copy()


class Seqs(C.Structure):
    _fields_ = [("n", C.c_size_t), ("names", C.c_void_p), ("name_off", C.POINTER(C.c_uint64)),
                ("seq", C.c_void_p), ("seq_off", C.POINTER(C.c_uint64))]


def _sig(name, restype, argtypes):
    f = getattr(lib, name)
    f.restype = restype
    f.argtypes = argtypes
    return f


_vp = C.c_void_p
_sig("swg_create", C.c_int, [C.POINTER(Config), C.POINTER(_vp)])
_sig("swg_destroy", None, [_vp])
_sig("swg_last_error", C.c_char_p, [_vp])
_sig("swg_global_error", C.c_char_p, [])
_sig("swg_abi_version", C.c_int, [])
_sig("swg_set_option", C.c_int, [_vp, C.c_char_p, C.c_long])
_sig("swg_set_scoring", C.c_int, [_vp, _vp, C.c_int, C.c_int])
_sig("swg_set_query", C.c_int, [_vp, _vp, C.c_size_t])
_sig("swg_set_query_pssm", C.c_int, [_vp, _vp, C.c_size_t])
_sig("swg_db_pack", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("swg_db_pack_shard", C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(_vp)])
_sig("swg_db_pack_shards", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.POINTER(_vp)])
_sig("swg_db_upload", C.c_int, [_vp, _vp])
_sig("swg_db_view", C.c_int, [_vp, _vp, _vp, C.c_size_t, C.POINTER(_vp)])
_sig("swg_db_free", None, [_vp])
_sig("swg_db_save", C.c_int, [_vp, C.c_char_p])
_sig("swg_db_load", C.c_int, [C.c_char_p, C.POINTER(_vp)])
_sig("swg_db_count", C.c_size_t, [_vp])
_sig("swg_db_total_count", C.c_size_t, [_vp])
_sig("swg_db_residues", C.c_uint64, [_vp])
_sig("swg_db_packed_bytes", C.c_uint64, [_vp])
_sig("swg_db_order", C.POINTER(C.c_uint32), [_vp])
_sig("swg_search", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(Stats)])
_sig("swg_search_begin", C.c_int, [_vp, _vp, C.c_int, C.c_size_t, C.POINTER(C.c_int)])
_sig("swg_search_end", C.c_int, [_vp, C.c_int, _vp, _vp, C.POINTER(C.c_size_t), C.POINTER(Stats)])
_sig("swg_search_multi", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, C.POINTER(Stats)])
_sig("swg_search_multi_pssm", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, C.POINTER(Stats)])
_sig("swg_search_gapless", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(Stats)])
for _name in ("swg_search_above", "swg_search_gapless_above"):
    _sig(_name, C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(Stats)])
for _name in ("swg_search_above_multi", "swg_search_above_multi_pssm", "swg_search_gapless_above_multi", "swg_search_gapless_above_multi_pssm"):
    _sig(_name, C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.POINTER(Stats)])
_sig("swg_search_gapless_multi", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, C.POINTER(Stats)])
_sig("swg_search_gapless_multi_pssm", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, C.POINTER(Stats)])
_sig("swg_search_lists", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.POINTER(Stats)])
_sig("swg_search_lists_pssm", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.POINTER(Stats)])
_sig("swg_fill_batches16", C.c_int, [_vp, C.POINTER(Batch16), C.c_size_t, C.POINTER(C.c_double)])
_sig("swg_align_hits", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t])
_sig("swg_align_ops_bound", C.c_size_t, [_vp, _vp])
_sig("swg_align_hits_multi", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t])
_sig("swg_align_hits_multi_pssm", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t])
_sig("swg_align_ops_bound_multi", C.c_size_t, [_vp, _vp, C.c_size_t])
_sig("swg_hit_key", C.c_uint64, [C.c_int32, C.c_uint32])
_sig("swg_key_hit", None, [C.c_uint64, C.POINTER(Hit)])
_sig("swg_topk_merge_keys", C.c_size_t, [_vp, C.c_size_t, C.c_size_t, _vp])
_sig("swg_align_bounds", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp])
_sig("swg_align_bounds_multi", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp])
_sig("swg_align_bounds_multi_pssm", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp])
_sig("swg_group_align_hits", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t])
_sig("swg_group_align_ops_bound", C.c_size_t, [_vp])
_sig("swg_group_select", C.c_int, [_vp, _vp, C.c_size_t])
_sig("swg_group_create", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("swg_group_destroy", None, [_vp])
_sig("swg_group_size", C.c_int, [_vp])
_sig("swg_group_last_error", C.c_char_p, [_vp])
_sig("swg_group_set_option", C.c_int, [_vp, C.c_char_p, C.c_long])
_sig("swg_group_set_scoring", C.c_int, [_vp, _vp, C.c_int, C.c_int])
_sig("swg_group_set_query", C.c_int, [_vp, _vp, C.c_size_t])
_sig("swg_group_set_query_pssm", C.c_int, [_vp, _vp, C.c_size_t])
_sig("swg_group_load", C.c_int, [_vp, _vp, _vp, C.c_size_t])
_sig("swg_group_search", C.c_int, [_vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(Stats)])
_sig("swg_letter_index", C.c_int, [C.c_int])
_sig("swg_index_letter", C.c_int, [C.c_int])
_sig("swg_scoring_init", None, [C.POINTER(Scoring)])
_sig("swg_scoring_add", C.c_int, [C.POINTER(Scoring), C.c_int, C.c_int, C.c_int])
_sig("swg_scoring_load_matrix", C.c_int, [C.POINTER(Scoring), C.c_char_p, C.c_char_p, C.c_size_t])
_sig("swg_query_sanitize", None, [C.POINTER(Scoring), _vp, C.c_size_t])
_sig("swg_seqs_read", C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(Seqs), C.c_char_p, C.c_size_t])
_sig("swg_seqs_free", None, [C.POINTER(Seqs)])
_sig("swg_seqs_to_indices", C.c_int, [C.POINTER(Seqs), _vp, C.c_char_p])
_sig("swg_synth_db", C.c_int, [C.c_uint64, C.c_size_t, C.c_double, C.c_double, C.c_uint32,
                               C.c_uint32, C.POINTER(_vp), C.POINTER(_vp)])
_sig("swg_synth_query", None, [C.c_uint64, C.c_size_t, _vp])
_sig("swg_synth_db_similar", C.c_int, [C.c_uint64, C.c_size_t, C.c_double, C.c_double, C.c_uint32,
                                       C.c_uint32, _vp, C.c_size_t, C.c_double, C.c_double,
                                       C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_size_t)])
_sig("swg_synth_db_family", C.c_int, [C.c_uint64, C.c_size_t, C.c_double, C.c_double, C.c_uint32,
                                      C.c_uint32, _vp, C.c_size_t, C.c_double, C.c_double, C.c_double,
                                      C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_size_t)])
_sig("swg_synth_db_shard", C.c_int, [C.c_uint64, C.c_size_t, C.c_double, C.c_double, C.c_uint32, C.c_uint32,
                                     _vp, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_int,
                                     C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)])
_sig("swg_synth_free", None, [_vp])
_sig("swg_pssm_load", C.c_int, [C.c_char_p, C.POINTER(Scoring), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_size_t),
                                C.c_char_p, C.c_size_t])
_sig("swg_pssm_free", None, [_vp, _vp])
# test hook, declared in csrc/swg_host_internal.h (not part of the public ABI)
_sig("swg_debug_fail_alloc", None, [C.c_int])
_sig("swg_align_stats", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, _vp])
_sig("swg_align_stats_multi", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp])
_sig("swg_align_stats_multi_pssm", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp])
_sig("swg_align_hsps", C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t])
_sig("swg_align_hsps_multi", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t])
_sig("swg_align_hsps_multi_pssm", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t])
_sig("swg_align_hsps_host", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_uint32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp])
_sig("swg_debug_bounds_last", C.c_int, [_vp, _vp])
_sig("swg_comp_adjust", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp])
_sig("swg_comp_adjust_multi", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, _vp])
_sig("swg_comp_adjust_multi_pssm", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, _vp])
_sig("swg_comp_adjust_host", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_int, _vp, C.POINTER(C.c_double)])
_sig("swg_debug_comp_last", C.c_int, [_vp, _vp])
_sig("swg_debug_sort_count", C.c_ulong, [])
_sig("swg_debug_engine", C.c_int, [_vp, C.c_size_t, C.c_int, C.c_int, _vp])
_sig("swg_debug_plan", C.c_int, [_vp, C.c_size_t, C.c_int, _vp])
_sig("swg_debug_plan_f16", C.c_int, [_vp, C.c_size_t, C.c_int, C.c_long, _vp])
_sig("swg_debug_plan_gapless", C.c_int, [_vp, C.c_size_t, C.c_int, _vp])
_sig("swg_debug_plan_forced", C.c_int, [_vp, C.c_size_t, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_long, C.c_int, _vp])
_sig("swg_debug_plan_streams", C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_long, C.c_long, C.c_long, C.c_long, _vp])
_sig("swg_debug_plan_systolic", C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_long, C.c_long, _vp])
_sig("swg_debug_systolic_variants", C.c_int, [C.c_int, _vp, C.c_size_t])
_sig("swg_debug_plan_batch", C.c_int, [_vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, _vp])
_sig("swg_debug_plan_lists", C.c_int, [_vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, _vp])
_sig("swg_debug_launch_log", None, [C.c_int])
_sig("swg_debug_launch_log_read", C.c_size_t, [_vp, C.c_size_t])
_sig("swg_debug_split", C.c_int, [_vp, C.c_size_t, C.c_uint64, _vp])
_sig("swg_debug_list_plan", C.c_int, [C.c_size_t, C.c_uint32, C.c_int, _vp, _vp])
_sig("swg_debug_pair_tokens", C.c_int, [_vp, _vp, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_size_t)])
_sig("swg_debug_view_ranks", C.c_int, [_vp, _vp, C.c_size_t, _vp, C.POINTER(C.c_size_t)])
_sig("swg_debug_list_jobs", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp])
_sig("swg_prune_last", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_bound", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp])
_sig("swg_debug_prune_plan", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_plan_above", C.c_int, [_vp, _vp])
_sig("swg_debug_above_multi_route", C.c_int, [C.c_long, C.c_int, C.c_int])
_sig("swg_debug_prune_stages", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)])
_sig("swg_debug_prune_kmer", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp])
_sig("swg_debug_prune_kmer_choice", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_kmer_read", C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_size_t, _vp])
_sig("swg_debug_prune_kmer_seg", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp])
_sig("swg_debug_prune_kmer_choice_seg", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_kmer_seg_read", C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp])
_sig("swg_debug_prune_kmer_refine", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp])
_sig("swg_debug_prune_refine_choice", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_refine_read", C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp])
_sig("swg_debug_prune_stages3", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)])
_sig("swg_debug_prune_kmer_refine3", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp])
_sig("swg_debug_prune_refine3_choice", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_kmer_refine4", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp])
_sig("swg_debug_prune_table_bits", C.c_int, [_vp, _vp, C.c_size_t, C.c_int])
_sig("swg_debug_prune_tables", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_tables4", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_kmer_refine5", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp])
_sig("swg_debug_prune_refine5_read", C.c_int, [_vp, _vp, C.c_size_t, _vp])
_sig("swg_debug_prune_tables5", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_refine5_choice", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_stages6", C.c_int, [_vp, _vp, C.c_size_t, _vp])
_sig("swg_debug_prune_refine4_read", C.c_int, [_vp, _vp, C.c_size_t, _vp])
_sig("swg_debug_prune_refine4_choice", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_gate_choice", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_gate", C.c_int, [_vp, _vp])
_sig("swg_debug_prune_stages5", C.c_int, [_vp, _vp, C.c_size_t, _vp])
_sig("swg_debug_prune_stages4", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)])
_sig("swg_debug_list_deal", C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_uint64, C.c_uint64, _vp, C.c_size_t, C.POINTER(C.c_size_t)])
_sig("swg_debug_calib_iters", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)])
_sig("swg_db_composition", C.c_int, [_vp, _vp, _vp])
_sig("swg_calibrate", C.c_int, [_vp, _vp, C.c_int, _vp])
_sig("swg_calibrate_multi", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_int, _vp])
_sig("swg_calibrate_multi_pssm", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_int, _vp])
_sig("swg_evalue", C.c_double, [_vp, C.c_uint64, C.c_int32])
_sig("swg_bitscore", C.c_double, [_vp, C.c_int32])
_sig("swg_evalue_min_score", C.c_int32, [_vp, C.c_uint64, C.c_double])
_sig("swg_synth_db_iid", C.c_int, [C.c_uint64, C.c_size_t, C.c_uint32, _vp, C.POINTER(_vp), C.POINTER(_vp)])
_sig("swg_gumbel_fit_hist", C.c_int, [_vp, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)])
_sig("swg_matrix_lambda", C.c_int, [_vp, _vp, C.POINTER(C.c_double)])
_sig("swg_pssm_from_paths", C.c_int, [_vp, _vp, C.c_double, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp])
_sig("swg_pssm_from_paths_ex", C.c_int, [_vp, _vp, C.c_double, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                         _vp, _vp, _vp])
_sig("swg_pssm_save", C.c_int, [C.c_char_p, _vp, _vp, C.c_size_t])
_sig("swg_pssm_build", C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_double, _vp, _vp, _vp])
_sig("swg_pssm_build_multi", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_double, _vp, _vp, _vp])
_sig("swg_pssm_build_multi_pssm", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_double, _vp, _vp, _vp])
_sig("swg_mask_params_default", None, [_vp])
_sig("swg_mask_tables", C.c_int, [_vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
_sig("swg_seg_mask", C.c_int, [_vp, C.c_size_t, _vp, _vp, C.POINTER(C.c_size_t)])
_sig("swg_seg_mask_segments", C.c_int, [_vp, C.c_size_t, _vp, _vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)])
_sig("swg_seg_mask_flat", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp])
_sig("swg_db_sequence", C.c_int, [_vp, C.c_uint32, _vp, C.c_size_t, C.POINTER(C.c_size_t)])
_sig("swg_db_mask", C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)])
_sig("swg_db_mask_info", C.c_int, [_vp, _vp])
_sig("swg_debug_mask_fail_alloc", None, [C.c_int])
_sig("swg_codon_table", C.c_int, [C.c_int, _vp])
_sig("swg_translate_seq", C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp])
_sig("swg_translate_flat", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, _vp])
_sig("swg_translate_hit", None, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int)])
_sig("swg_translate_coords", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)])
_sig("swg_db_translate", C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)])
_sig("swg_db_translate_info", C.c_int, [_vp, _vp])
_sig("swg_translate_tile_codons", C.c_uint, [])
TRANSLATE_TILE_CODONS = int(lib.swg_translate_tile_codons())  # codons of a frame per tile of the translation kernel


def _check(rc, ctx=None):
    if rc != SWG_OK:
        msg = lib.swg_last_error(ctx) if ctx else lib.swg_global_error()
        raise SwgError(rc, (msg or b"").decode("utf-8", "replace"))


def _i8(a):
    a = np.ascontiguousarray(a, dtype=np.int8)
    return a, a.ctypes.data_as(_vp)


def _pssm(pssm):
    """(lq, 32) int8 PSSM -> (array, pointer, lq); values must already be int8."""
    a = np.asarray(pssm)
    if a.ndim != 2 or a.shape[1] != 32:
        raise ValueError("a PSSM is an (lq, 32) array, got shape %s" % (a.shape,))
    if a.dtype != np.int8 and a.size and (a.min() < -128 or a.max() > 127):
        raise ValueError("PSSM values must fit int8")
    p, pp = _i8(a)
    return p, pp, a.shape[0]


def _lists(lists):
    """Candidate lists (one sequence of original indices per query) -> (flat uint32, offsets uint64[n + 1])."""
    arrs = [np.ascontiguousarray(l, dtype=np.uint32).reshape(-1) for l in lists]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([a.size for a in arrs])
    flat = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint32)
    if flat.size == 0:
        flat = np.zeros(1, dtype=np.uint32)           # (empty lists are lists: never a NULL pointer)
    return np.ascontiguousarray(flat, dtype=np.uint32), off


# ---------------------------------------------------------------------------
# host helpers
# ---------------------------------------------------------------------------
def letters_to_indices(s):
    """Reference letters_to_index over a string; raises on an illegal letter."""
    out = np.empty(len(s), dtype=np.int8)
    for i, ch in enumerate(s):
        v = lib.swg_letter_index(ord(ch))
        if v < 0:
            raise SwgError(SWG_ERR_RESIDUE, "illegal residue %r" % ch)
        out[i] = v
    return out


def load_scoring(name_or_path, gap_open=-2, gap_extend=-1):
    """Scoring struct from a matrix file (bundled name like 'BLOSUM62' or a path)."""
    path = name_or_path
    if not os.path.exists(path):
        path = os.path.join(DATA_DIR, name_or_path + ".txt")
    sc = Scoring()
    lib.swg_scoring_init(C.byref(sc))
    err = C.create_string_buffer(512)
    rc = lib.swg_scoring_load_matrix(C.byref(sc), path.encode(), err, 512)
    if rc != SWG_OK:
        raise SwgError(rc, err.value.decode())
    sc.gap_open, sc.gap_extend = gap_open, gap_extend
    return sc


def read_pssm(path, scoring):
    """PSI-BLAST ASCII PSSM (swg_pssm_load) -> (pssm int8[lq, 32], query residue indices int8[lq]).  Residues the
    file has no column for score as `scoring` (a Scoring) scores them against each position's residue."""
    pp, qp, n = _vp(), _vp(), C.c_size_t(0)
    err = C.create_string_buffer(512)
    rc = lib.swg_pssm_load(path.encode(), C.byref(scoring), C.byref(pp), C.byref(qp), C.byref(n), err, 512)
    if rc != SWG_OK:
        raise SwgError(rc, err.value.decode())
    try:
        lq = n.value
        pssm = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_int8)), shape=(lq * 32,)).reshape(lq, 32).copy()
        query = np.ctypeslib.as_array(C.cast(qp, C.POINTER(C.c_int8)), shape=(lq,)).copy()
    finally:
        lib.swg_pssm_free(pp, qp)
    return pssm, query


def read_seqs(path, max_records=0):
    """-> (names list, residue letters bytes, offsets uint64[n+1])."""
    s = Seqs()
    err = C.create_string_buffer(512)
    rc = lib.swg_seqs_read(path.encode(), max_records, C.byref(s), err, 512)
    if rc != SWG_OK:
        raise SwgError(rc, err.value.decode())
    try:
        n = s.n
        seq_off = np.ctypeslib.as_array(s.seq_off, shape=(n + 1,)).copy()
        name_off = np.ctypeslib.as_array(s.name_off, shape=(n + 1,)).copy()
        seq = C.string_at(s.seq, int(seq_off[n])) if n else b""
        raw = C.string_at(s.names, int(name_off[n])) if n else b""
        names = [raw[int(name_off[i]):int(name_off[i + 1]) - 1].decode("utf-8", "replace") for i in range(n)]
        idx = np.empty(len(seq), dtype=np.int8)
        bad = C.create_string_buffer(2)
        rc = lib.swg_seqs_to_indices(C.byref(s), idx.ctypes.data_as(_vp), bad)
        if rc != SWG_OK:
            raise SwgError(rc, "illegal residue %r" % bad.value)
    finally:
        lib.swg_seqs_free(C.byref(s))
    return names, seq, idx, seq_off


class _Owned:
    """A buffer malloc'ed by the library, released with swg_synth_free when the last array over it dies."""

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes
        self.buf = (C.c_uint8 * nbytes).from_address(ptr.value)

    def __del__(self):
        if self.ptr is not None:
            lib.swg_synth_free(self.ptr)
            self.ptr = None


def _take(ptr, nbytes, dtype):
    """numpy array over a library-owned buffer WITHOUT copying it (a 10M-sequence database is 3.8 GB);
    the buffer is freed when the array (and every view of it) is gone."""
    if not nbytes:
        lib.swg_synth_free(ptr)
        return np.zeros(0, dtype=dtype)
    owner = _Owned(ptr, nbytes)
    arr = np.frombuffer(owner.buf, dtype=dtype)     # keeps owner.buf alive ...
    _OWNERS[id(owner.buf)] = owner                  # ... and the owner lives as long as its buffer does
    import weakref
    weakref.finalize(arr, _OWNERS.pop, id(owner.buf), None)
    return arr


_OWNERS = {}


def synth_db(seed, n, median=290.0, sigma_ln=0.75, min_len=20, max_len=5000, query=None,
             fraction=0.0, subst=0.05, subst_hi=None):
    """Synthetic database -> (flat int8, offsets uint64[n+1][, n_planted]).
    subst_hi: the planted sequences are a family of relatives, each with its own substitution rate
    from [subst, subst_hi]."""
    flat, off = _vp(), _vp()
    if query is None or fraction <= 0.0:
        _check(lib.swg_synth_db(seed, n, median, sigma_ln, min_len, max_len, C.byref(flat), C.byref(off)))
        planted = None
    else:
        q, qp = _i8(query)
        npl = C.c_size_t(0)
        if subst_hi is not None:
            _check(lib.swg_synth_db_family(seed, n, median, sigma_ln, min_len, max_len, qp, len(q),
                                           fraction, subst, subst_hi, C.byref(flat), C.byref(off), C.byref(npl)))
        else:
            _check(lib.swg_synth_db_similar(seed, n, median, sigma_ln, min_len, max_len, qp, len(q),
                                            fraction, subst, C.byref(flat), C.byref(off), C.byref(npl)))
        planted = npl.value
    offsets = _take(off, (n + 1) * 8, np.uint64)
    residues = _take(flat, int(offsets[n]), np.int8)
    return (residues, offsets) if planted is None else (residues, offsets, planted)


def _freq(freq):
    """A composition (32 weights by residue index) -> (array, pointer); None -> (None, None): the built-in table."""
    if freq is None:
        return None, None
    f = np.ascontiguousarray(freq, dtype=np.float64)
    if f.shape != (32,):
        raise ValueError("freq is 32 weights by residue index, got shape %s" % (f.shape,))
    return f, f.ctypes.data_as(_vp)


def synth_db_iid(seed, n, length, freq=None):
    """n sequences of exactly `length` residues, i.i.d. from freq (32 weights by residue index; None: the built-in
    table) -> (flat int8, offsets uint64[n+1]) (swg_synth_db_iid: what a calibration scores against)."""
    f, fp = _freq(freq)
    flat, off = _vp(), _vp()
    _check(lib.swg_synth_db_iid(seed, n, length, fp, C.byref(flat), C.byref(off)))
    offsets = _take(off, (n + 1) * 8, np.uint64)
    return _take(flat, int(offsets[n]), np.int8), offsets


def gumbel_fit_hist(hist):
    """Maximum-likelihood Gumbel fit of a histogram of integer scores (swg_gumbel_fit_hist) -> dict(lambda, mu, n_iter,
    status); status 0 a fit, 1 fewer than two distinct scores, 2 not converged."""
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    lam, mu, it = C.c_double(0), C.c_double(0), C.c_int(0)
    rc = lib.swg_gumbel_fit_hist(h.ctypes.data_as(_vp) if h.size else None, h.size, C.byref(lam), C.byref(mu), C.byref(it))
    if rc < 0:
        _check(rc)
    return {"lambda": lam.value, "mu": mu.value, "n_iter": it.value, "status": rc}


def matrix_lambda(sub, freq=None):
    """The scale of a substitution matrix under a background (swg_matrix_lambda): the positive root of
    sum P_a P_b exp(lambda sub[a][b]) = 1.  freq: 32 weights by residue index (None: the built-in table)."""
    if isinstance(sub, Scoring):
        sub = sub.table()
    s, sp = _i8(np.asarray(sub).reshape(32, 32))
    f, fp = _freq(freq)
    lam = C.c_double(0)
    _check(lib.swg_matrix_lambda(sp, fp, C.byref(lam)))
    return lam.value


def pssm_from_paths(sub, query, flat, offsets, alignments, freq=None, pseudocount=PSSM_PSEUDOCOUNT_DEFAULT, want_values=False,
                    blocks=False, purge=0):
    """The PSSM of `query` (table indices) from its hits' alignments on the host (swg_pssm_from_paths, the twin of
    Context.build_pssm): alignments is what align_hits returns with want_ops=True -- dicts whose "index" is an index
    into flat / offsets -> (pssm int8[lq, 32], values float64[lq, 32] or None, info dict).  blocks, purge: the model's
    options "pssm_blocks" and "pssm_purge" (swg_pssm_from_paths_ex); both off, the old entry point is called."""
    if isinstance(sub, Scoring):
        sub = sub.table()
    s, sp = _i8(np.asarray(sub).reshape(32, 32))
    q, qp = _i8(query)
    fl, flp = _i8(flat)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    f, fp = _freq(freq)
    n = len(alignments)
    stride = max((a["n_ops"] for a in alignments), default=0) + 1
    al = (Alignment * max(n, 1))()
    ops = C.create_string_buffer(max(1, n * stride))
    for i, a in enumerate(alignments):
        for name, _ in Alignment._fields_:
            if name != "reserved":
                setattr(al[i], name, int(a[name]))
        ops[i * stride:i * stride + len(a["ops"])] = a["ops"].encode()
    pssm = np.zeros((q.size, 32), dtype=np.int8)
    values = np.zeros((q.size, 32), dtype=np.float64) if want_values else None
    info = PssmInfo()
    head = (sp, fp, float(pseudocount), qp, q.size, flp, off.ctypes.data_as(_vp), C.cast(al, _vp), C.cast(ops, _vp), stride, n)
    tail = (pssm.ctypes.data_as(_vp), values.ctypes.data_as(_vp) if want_values else None, C.byref(info))
    if not blocks and not purge:
        _check(lib.swg_pssm_from_paths(*head, *tail))
    else:
        _check(lib.swg_pssm_from_paths_ex(*head, int(blocks), int(purge), *tail))
    return pssm, values, info.as_dict()


def write_pssm(path, pssm, query):
    """The ASCII PSSM file read_pssm reads (swg_pssm_save): the 20 standard columns of pssm int8[lq, 32] and the query's
    residues (table indices)."""
    p, pp, lq = _pssm(pssm)
    q, qp = _i8(query)
    if q.size != lq:
        raise ValueError("query: %d residues for a PSSM of %d rows" % (q.size, lq))
    _check(lib.swg_pssm_save(os.fsencode(path), pp, qp, lq))


def evalue(params, db_residues, score):
    """E = K lq db_residues exp(-lambda score) of a calibrated query (a dict from Context.calibrate*); NaN without a fit."""
    return lib.swg_evalue(C.byref(EvalueParams.of(params)), int(db_residues), int(score))


def bitscore(params, score):
    """(lambda score - ln K) / ln 2; NaN without a fit."""
    return lib.swg_bitscore(C.byref(EvalueParams.of(params)), int(score))


def evalue_min_score(params, db_residues, E):
    """The smallest score S >= 1 with evalue(params, db_residues, S) <= E; -1 without a fit or for E <= 0."""
    return lib.swg_evalue_min_score(C.byref(EvalueParams.of(params)), int(db_residues), float(E))


def synth_db_shard(seed, n, shard_rank, shard_count, median=290.0, sigma_ln=0.75, min_len=20, max_len=5000,
                   query=None, fraction=0.0, subst=0.05):
    """One shard (global bins b % shard_count == shard_rank) of the database synth_db(seed, n, ...) would
    return, without generating the rest -> dict(flat, offsets[n_local+1], index[n_local] global indices,
    n_total, residues_total, planted)."""
    flat, off, idx = _vp(), _vp(), _vp()
    nl, tot, npl = C.c_size_t(0), C.c_uint64(0), C.c_size_t(0)
    if query is not None and fraction > 0.0:
        q, qp = _i8(query)
        lq = len(q)
    else:
        qp, lq, fraction = None, 0, 0.0
    _check(lib.swg_synth_db_shard(seed, n, median, sigma_ln, min_len, max_len, qp, lq, fraction, subst,
                                  shard_rank, shard_count, C.byref(flat), C.byref(off), C.byref(idx),
                                  C.byref(nl), C.byref(tot), C.byref(npl)))
    n_local = nl.value
    offsets = _take(off, (n_local + 1) * 8, np.uint64)
    index = _take(idx, n_local * 4, np.uint32)
    residues = _take(flat, int(offsets[n_local]), np.int8)
    return dict(flat=residues, offsets=offsets, index=index, n_total=n, residues_total=int(tot.value),
                planted=int(npl.value))


def debug_list_plan(lq, n_pairs_guess, n_cu=256, main=(32, 16, 4)):
    """Test hook: geometry of the int16 re-run of the pairs the f16 cells flagged (no device needed)
    -> dict(K, G, W, passes)."""
    m = np.asarray(main, dtype=np.int32)
    out = np.zeros(4, dtype=np.int32)
    _check(lib.swg_debug_list_plan(lq, n_pairs_guess, n_cu, m.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return {"K": int(out[0]), "G": int(out[1]), "W": int(out[2]), "passes": int(out[3])}


def debug_prune_bound(rows, query, flat, offsets):
    """Test hook (no device needed): the host mirror of the pruning bound.  rows: the 32 x 32 table with `query` the
    index query, or an (lq, 32) PSSM with query None.  -> (colmax uint8[32], U uint64[n]) for the sequences
    flat[offsets[i] .. offsets[i+1])."""
    r, rp = _i8(rows)
    lq = r.size // 32
    qp = None
    if query is not None:
        q, qp = _i8(query)
        lq = q.size
    f, fp = _i8(flat)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = off.size - 1
    cm = np.zeros(32, dtype=np.uint8)
    u = np.zeros(max(n, 1), dtype=np.uint64)
    _check(lib.swg_debug_prune_bound(rp, qp, lq, fp, off.ctypes.data_as(_vp), n, cm.ctypes.data_as(_vp), u.ctypes.data_as(_vp)))
    return cm, u[:n]


KMER_CLASSES = 22
# residue index -> class of the k-mer bound: 0 padding, 1..20 the standard amino acids in index order, 21 the rest
KMER_CLASS = [0] + [0] * 31
_std = sorted(ord(ch) - ord("A") + 1 for ch in "ACDEFGHIKLMNPQRSTVWY")
for _r in range(1, 32):
    KMER_CLASS[_r] = _std.index(_r) + 1 if _r in _std else KMER_CLASSES - 1
del _std, _r


def _prune_kmer_mirror(hook, rows, query, gap_open, gap_extend, which, flat, offsets, table_shape):
    """The marshalling of the three k-mer mirror hooks: `which` is the hook's own arguments between the gap scores and
    the sequences ((k,), (k, S) or (S2,)), table_shape the table to hand it (None: none).  -> (table or None, U uint64[n])."""
    r, rp = _i8(rows)
    lq = r.size // 32
    qp = None
    if query is not None:
        q, qp = _i8(query)
        lq = q.size
    f, fp = _i8(flat)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = off.size - 1
    t = np.zeros(table_shape, dtype=np.uint16) if table_shape is not None else None
    u = np.zeros(max(n, 1), dtype=np.uint64)
    _check(hook(rp, qp, lq, int(gap_open), int(gap_extend), *which, fp, off.ctypes.data_as(_vp), n,
                t.ctypes.data_as(_vp) if t is not None else None, u.ctypes.data_as(_vp)))
    return t, u[:n]


def debug_prune_kmer(rows, query, gap_open, gap_extend, k, flat, offsets, table=True):
    """Test hook (no device needed): the host mirror of the k-mer bound, k = 4 or 5.  rows / query as debug_prune_bound
    takes them.  -> (table uint16[22^k] or None, U_k uint64[n]): the local score of every class block against the query,
    and the bound of each sequence flat[offsets[i] .. offsets[i+1]) summed as the device sums it -- over the sequence's
    token rows (two reset rows first), in blocks of 4 rows, or of 5 over every whole 20 rows and of 4 over the rest.  A
    residue 0 in a sequence is a padding row (the shorter sequence of a pair, filled up to the longer one's length)."""
    return _prune_kmer_mirror(lib.swg_debug_prune_kmer, rows, query, gap_open, gap_extend, (int(k),), flat, offsets,
                              (KMER_CLASSES ** int(k),) if table and k in (4, 5) else None)


def debug_prune_kmer_choice(forced=0, pruned=1, lq=3000, pair_rows=1900000000, table_rate=0, fill_rate=0):
    """Test hook (no device needed): the bound a search cuts by (swg_prune_kmer_choice) -> 0 (not pruned: nothing is
    built), 1 (colmax), 4 or 5, with option prune_segments = 1 (the unsegmented bound; debug_prune_kmer_choice_seg has
    the segments).  forced: option prune_kmer; rates in table cells and fill pair rows per second, 0: the library's own
    for this lq."""
    a = np.array([forced, pruned, lq, pair_rows, table_rate, fill_rate], dtype=np.int64)
    out = np.zeros(1, dtype=np.int64)
    _check(lib.swg_debug_prune_kmer_choice(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return int(out[0])


KMER_MAX_SEGMENTS = 32
KMER_TABLE_BUDGET = 96 << 20   # bytes: the largest table of the k-mer bound a context builds (it admits k = 5 in 8 segments)


def debug_prune_kmer_seg(rows, query, gap_open, gap_extend, k, segments, flat, offsets, table=True):
    """Test hook (no device needed): debug_prune_kmer over `segments` (1..32) segments of the query's columns, each
    ceil(lq / segments) wide.  -> (table uint16[22^k, segments] or None, U uint64[n]): every class block's best cell
    within each segment, and the bound of each sequence with its blocks taken in order.  One segment is
    debug_prune_kmer."""
    S = int(segments)
    return _prune_kmer_mirror(lib.swg_debug_prune_kmer_seg, rows, query, gap_open, gap_extend, (int(k), S), flat, offsets,
                              (KMER_CLASSES ** int(k), S) if table and k in (4, 5) and 1 <= S <= KMER_MAX_SEGMENTS else None)


def debug_prune_kmer_choice_seg(forced=0, segments=0, pruned=1, lq=3000, pair_rows=1900000000, table_rate=0, fill_rate=0):
    """Test hook (no device needed): debug_prune_kmer_choice with option prune_segments -> (k, S, the table's bytes,
    whether a context builds that table: False beyond KMER_TABLE_BUDGET); (0, 0, 0, True) where nothing is pruned,
    (1, 1, 0, True) for the colmax bound."""
    a = np.array([forced, pruned, lq, pair_rows, table_rate, fill_rate, segments], dtype=np.int64)
    out = np.zeros(4, dtype=np.int64)
    _check(lib.swg_debug_prune_kmer_choice_seg(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return int(out[0]), int(out[1]), int(out[2]), bool(out[3])


KMER_REFINE_SEGMENTS = 128    # the second level's most
KMER_REFINE3_SEGMENTS = 256   # the third level's


def debug_prune_kmer_refine(rows, query, gap_open, gap_extend, segments, flat, offsets, table=True):
    """Test hook (no device needed): the second- and third-level bounds' host mirror -- debug_prune_kmer_seg at k = 4 over
    the `segments` (32, 64, 128; 256: the third level's, swg_debug_prune_kmer_refine3) segments the refine kernel walks.
    -> (table uint16[22^4, segments] or None, U uint64[n])."""
    S = int(segments)
    hook = lib.swg_debug_prune_kmer_refine3 if S == KMER_REFINE3_SEGMENTS else lib.swg_debug_prune_kmer_refine
    return _prune_kmer_mirror(hook, rows, query, gap_open, gap_extend, (S,), flat, offsets,
                              (KMER_CLASSES ** 4, S) if table and S in (32, 64, 128, 256) else None)


def debug_prune_kmer_refine4(rows, query, gap_open, gap_extend, segments, flat, offsets):
    """Test hook (no device needed): the fourth-level bound's host mirror -- k = 5 over `segments` (128 or 256) segments,
    the blocks taken as debug_prune_kmer takes k = 5.  There is no table (22^5 x 256 entries): the mirror computes the
    entries of the blocks the sequences hold.  -> U uint64[n]."""
    r, rp = _i8(rows)
    lq = r.size // 32
    qp = None
    if query is not None:
        q, qp = _i8(query)
        lq = q.size
    f, fp = _i8(flat)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = off.size - 1
    u = np.zeros(max(n, 1), dtype=np.uint64)
    _check(lib.swg_debug_prune_kmer_refine4(rp, qp, lq, int(gap_open), int(gap_extend), int(segments), fp, off.ctypes.data_as(_vp), n,
                                            u.ctypes.data_as(_vp)))
    return u[:n]


REFINE5_EXPLICIT = 1   # N of the fifth level's walk: the segments between two chains' ends taken one by one


def debug_prune_kmer_refine5(rows, query, gap_open, gap_extend, segments, flat, offsets, explicit=0):
    """Test hook (no device needed): the host mirror of a fifth-level bound -- the fourth level's blocks over
    `segments` (256) segments, the query columns jumped over between two blocks charged at -gap_extend each.  explicit: N
    of the walk (0: REFINE5_EXPLICIT; `segments` or more: the exact form).  -> U uint64[n], or None where the level is
    off (gap_extend = 0, or second entries that are no bytes)."""
    r, rp = _i8(rows)
    lq = r.size // 32
    qp = None
    if query is not None:
        q, qp = _i8(query)
        lq = q.size
    f, fp = _i8(flat)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = off.size - 1
    u = np.zeros(max(n, 1), dtype=np.uint64)
    on = C.c_int(0)
    _check(lib.swg_debug_prune_kmer_refine5(rp, qp, lq, int(gap_open), int(gap_extend), int(segments), int(explicit), fp, off.ctypes.data_as(_vp), n,
                                            u.ctypes.data_as(_vp), C.byref(on)))
    return u[:n] if on.value else None


def debug_prune_table_bits(rows, query, k=4):
    """Test hook (no device needed): the width of the k-mer tables' entries for this query (rows / query as
    debug_prune_bound takes them) at k = 4 or 5 under option prune_table_bits = 0 -> 8 where k x the largest colmax entry
    is at most 255, else 16."""
    r, rp = _i8(rows)
    lq = r.size // 32
    qp = None
    if query is not None:
        q, qp = _i8(query)
        lq = q.size
    rc = lib.swg_debug_prune_table_bits(rp, qp, lq, int(k))
    if rc < 0:
        _check(rc)
    return rc


def debug_prune_refine3_choice(forced=0, segments=0, refine=0, refine3=0, table_bits=8, pruned=1, lq=3000, pair_rows=1900000000,
                               table_rate=0, fill_rate=0):
    """Test hook (no device needed): debug_prune_refine_choice with option prune_refine3 and the tables' entry width
    -> (k, S, S2, S3): S3 = 256 with a third level, 0 without."""
    a = np.array([forced, pruned, lq, pair_rows, table_rate, fill_rate, segments, refine, refine3, table_bits], dtype=np.int64)
    out = np.zeros(4, dtype=np.int64)
    _check(lib.swg_debug_prune_refine3_choice(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


KMER_REFINE4_SEGMENTS = 256   # the fourth level's, of the k = 5 table
PRUNE_REFINE4_FORCED = 5256   # option "prune_refine4": (k, S) = (5, 256) as 1000 k + S


def debug_prune_refine4_choice(forced=0, segments=0, refine=0, refine3=0, refine4=0, table_bits=8, table_bits5=8, pruned=1, lq=3000,
                               pair_rows=1900000000, table_rate=0, fill_rate=0):
    """Test hook (no device needed): debug_prune_refine3_choice with option prune_refine4 and the k = 5 tables' entry width
    -> (k, S, S2, S3, S4): S4 = 256 with a fourth level, 0 without."""
    a = np.array([forced, pruned, lq, pair_rows, table_rate, fill_rate, segments, refine, refine3, table_bits, refine4, table_bits5], dtype=np.int64)
    out = np.zeros(5, dtype=np.int64)
    _check(lib.swg_debug_prune_refine4_choice(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return tuple(int(v) for v in out)


PRUNE_REFINE5_FORCED = 5256   # option "prune_refine5": both k = 5 tables in 256 segments


def debug_prune_refine5_choice(forced=0, segments=0, refine=0, refine3=0, refine4=0, refine5=0, table_bits=8, table_bits5=8, admitted=True,
                               fixed=False, pruned=1, lq=3000, pair_rows=1900000000, table_rate=0, fill_rate=0):
    """Test hook (no device needed): debug_prune_refine4_choice with option prune_refine5 and whether the query and scoring
    admit the fifth level (gap_extend < 0 and second entries that are bytes); fixed: a caller's threshold (search_above)
    -> (k, S, S2, S3, S4, S5): S5 = 256 with a fifth level, 0 without."""
    a = np.array([forced, pruned, lq, pair_rows, table_rate, fill_rate, segments, refine, refine3, table_bits, refine4, table_bits5, refine5,
                  1 if admitted else 0, 1 if fixed else 0], dtype=np.int64)
    out = np.zeros(6, dtype=np.int64)
    _check(lib.swg_debug_prune_refine5_choice(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return tuple(int(v) for v in out)


def debug_prune_gate_choice(forced=0, segments=0, gate=0, pruned=1, lq=3000, pair_rows=1900000000, table_rate=0, fill_rate=0):
    """Test hook (no device needed): debug_prune_kmer_choice_seg with option prune_gate (0 automatic, 1 off, 2 wherever
    the first level is a segmented k-mer bound) -> (k, S, gate): whether the first level's launch waits for a threshold
    and leaves out the pairs whose colmax bound is below it (swg_prune_gate_choice)."""
    a = np.array([forced, pruned, lq, pair_rows, table_rate, fill_rate, segments, 0, gate], dtype=np.int64)
    out = np.zeros(3, dtype=np.int64)
    _check(lib.swg_debug_prune_gate_choice(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return int(out[0]), int(out[1]), bool(out[2])


def debug_prune_refine_choice(forced=0, segments=0, refine=0, pruned=1, lq=3000, pair_rows=1900000000, table_rate=0, fill_rate=0):
    """Test hook (no device needed): debug_prune_kmer_choice_seg with option prune_refine -> (k, S, S2): the first-level
    bound and the segments of the second level's table, 0 without one."""
    a = np.array([forced, pruned, lq, pair_rows, table_rate, fill_rate, segments, refine], dtype=np.int64)
    out = np.zeros(3, dtype=np.int64)
    _check(lib.swg_debug_prune_refine_choice(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return int(out[0]), int(out[1]), int(out[2])


def prune_list(bounds, begin, end, threshold):
    """The list of a stage cut pair by pair, restated in numpy: the ids of the pairs of [begin, end) whose
    bound reaches the threshold, ascending."""
    b = np.asarray(bounds)[begin:end]
    return (begin + np.nonzero(b >= threshold)[0]).astype(np.uint32)


PRUNE_PLAN_KEYS = ("mode", "k", "want_scores", "gap_open", "gap_extend", "bits", "use_diag", "n_classes", "work_queue", "both_forms",
                   "gapless", "batch", "range_pairs", "groups", "prune_head", "n_segments")


def debug_prune_plan(**ask):
    """Test hook (no device needed): what a search decides about pruning (swg_prune_plan).  Keyword arguments as
    PRUNE_PLAN_KEYS; the defaults describe a hits-only search that is pruned: mode 1, k 100, gaps (-2, -1), 16-bit lane
    groups off the work queue, one class, one form, 1 000 000 pairs in 8 segments on 1024 lane groups, prune_head 4.
    -> (pruned, head pairs; 0: the stages are the segments)."""
    d = dict(mode=1, k=100, want_scores=0, gap_open=-2, gap_extend=-1, bits=16, use_diag=1, n_classes=1, work_queue=1, both_forms=0,
             gapless=0, batch=0, range_pairs=1000000, groups=1024, prune_head=4, n_segments=8)
    unknown = set(ask) - set(d)
    if unknown:
        raise TypeError("debug_prune_plan: unknown arguments %s" % sorted(unknown))
    d.update(ask)
    a = np.array([int(d[k]) for k in PRUNE_PLAN_KEYS], dtype=np.int64)
    out = np.zeros(2, dtype=np.int64)
    _check(lib.swg_debug_prune_plan(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return bool(out[0]), int(out[1])


PRUNE_PLAN_ABOVE_KEYS = ("mode", "gap_open", "gap_extend", "bits", "use_diag", "n_classes", "work_queue", "both_forms", "gapless", "batch",
                         "range_pairs", "groups", "n_segments", "prune_head")


def debug_prune_plan_above(**ask):
    """Test hook (no device needed): what a search_above decides about pruning (swg_prune_plan under a caller's
    threshold).  Keyword arguments as PRUNE_PLAN_ABOVE_KEYS; the defaults describe one that is pruned: mode 1, gaps (-2, -1),
    16-bit lane groups off the work queue, one class, one form, 1 000 000 pairs in 8 segments on 1024 lane groups.
    -> (pruned, head pairs: always 0)."""
    d = dict(mode=1, gap_open=-2, gap_extend=-1, bits=16, use_diag=1, n_classes=1, work_queue=1, both_forms=0, gapless=0, batch=0,
             range_pairs=1000000, groups=1024, n_segments=8, prune_head=4)
    unknown = set(ask) - set(d)
    if unknown:
        raise TypeError("debug_prune_plan_above: unknown arguments %s" % sorted(unknown))
    d.update(ask)
    a = np.array([int(d[k]) for k in PRUNE_PLAN_ABOVE_KEYS], dtype=np.int64)
    out = np.zeros(2, dtype=np.int64)
    _check(lib.swg_debug_prune_plan_above(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp)))
    return bool(out[0]), int(out[1])


def debug_above_multi_route(option=0, admitted=True, single_pruned=False):
    """Test hook (no device needed): the route search_above_multi takes (swg_above_multi_route) under option "above_batch"
    for a batch that plan_batch admits to the one launch or not, where swg_search_above of its longest query on the
    database would be pruned or not.  -> 1 (one launch per class) or 2 (one query after another); an option outside
    0..2 raises SwgError."""
    rc = lib.swg_debug_above_multi_route(int(option), 1 if admitted else 0, 1 if single_pruned else 0)
    if rc < 0:
        _check(rc)
    return rc


# a stage's fourth word: (bit, name) in queue order (the third level's walk is bit 5, queued between the second's and the list)
PRUNE_STAGE_QUEUED = ("threshold", "prefix_cut", "gate", "refine", "list")
_PRUNE_STAGE_BITS = ((0, "threshold"), (7, "bound"), (1, "prefix_cut"), (2, "gate"), (3, "refine"), (5, "refine3"), (6, "refine4"), (8, "refine5"),
                     (4, "list"))


def debug_prune_stages(segments, head_pairs=0, fixed=False, refine=0, prefix_cut=False, refine3=0, refine4=0, gate=False, refine5=0):
    """Test hook (no device needed): the stages of a pruned fill over the pair ranges `segments` [(begin, end), ...] and
    what is queued in front of each (swg_prune_stages) -> [(begin, end, segment index, names in queue order: those of
    PRUNE_STAGE_QUEUED, and "refine3" then "refine4" in front of "list"), ...].  head_pairs, fixed (a caller's threshold),
    refine, refine3 and refine4 (the second, third and fourth levels' segments, 0: none) and prefix_cut are the plan's.
    gate (the plan's: swg_debug_prune_stages5): "bound", the first level's gated launch, sits behind "threshold" on the
    stage that first has one.  refine5 (the fifth level's segments: swg_debug_prune_stages6): "refine5" behind "refine4"."""
    head = [head_pairs, fixed, refine, prefix_cut, refine3, refine4] + ([1 if gate else 0, refine5] if refine5 else [1] if gate else [])
    a = np.array(head + [len(segments)] + [int(v) for sg in segments for v in sg], dtype=np.int64)
    out = np.zeros((2 * len(segments) + 1, 4), dtype=np.int64)
    n = C.c_size_t(0)
    hook = lib.swg_debug_prune_stages6 if refine5 else lib.swg_debug_prune_stages5 if gate else lib.swg_debug_prune_stages4
    _check(hook(a.ctypes.data_as(_vp), out.ctypes.data_as(_vp), out.shape[0], C.byref(n)))
    return [(int(b), int(e), int(sg), tuple(name for i, name in _PRUNE_STAGE_BITS if int(qd) >> i & 1))
            for b, e, sg, qd in out[:n.value]]


LAUNCH_FAMILIES = ("dyn", "lists", "q32", "qq", "streams", "systolic")


def debug_systolic_variants(bits):
    """Test hook: [(K, max_waves)] of the systolic fill's instantiations for 16- or 32-bit cells, in the library's order
    (the first is the default)."""
    out = np.zeros((16, 2), dtype=np.int32)
    n = lib.swg_debug_systolic_variants(bits, out.ctypes.data_as(_vp), 16)
    assert 0 < n <= 16
    return [(int(k), int(w)) for k, w in out[:n]]


def debug_launch_log(on):
    """Test hook: clears the launch log and switches it on or off (off by default)."""
    lib.swg_debug_launch_log(1 if on else 0)


def debug_launch_log_read():
    """Test hook: the fill-kernel launches since the log was switched on, in launch order, as dicts: family (one of
    LAUNCH_FAMILIES: the launcher), K (columns per lane of the instantiation launched), G (lanes per group), W, form (the
    cells: 0 packed int16, 1 wide, 2 packed f16, 3 gapless), edges (the instantiation of one pass of several), fma (the
    f16 cells' pairing) / exact (the int32 cells' recurrence): the same flag under the name that fits the family,
    workgroups, grid_rows, list (1: the launch works off a device-side list -- a re-run of what an earlier launch
    flagged -- or the lists' row table, not off a range of the database).  Raises if the log overflowed."""
    seen = lib.swg_debug_launch_log_read(None, 0)              # how many launches there were: as many rows are asked for
    out = np.zeros((max(seen, 1), 10), dtype=np.int32)
    lib.swg_debug_launch_log_read(out.ctypes.data_as(_vp), seen)
    kept = int(np.count_nonzero(out[:seen, 1]))                # (a record's K is never 0: rows beyond the log's bound stay empty)
    if kept < seen:
        raise SwgError(SWG_ERR_STATE, "launch log: %d launches, %d kept" % (seen, kept))
    keys = ("family", "K", "G", "W", "form", "edges", "flag", "workgroups", "grid_rows", "list")
    recs = []
    for row in out[:seen]:
        r = dict(zip(keys, (int(v) for v in row)))
        r["family"] = LAUNCH_FAMILIES[r["family"]]
        r["fma"] = r["exact"] = r.pop("flag")
        recs.append(r)
    return recs


def synth_query(seed, lq):
    out = np.empty(lq, dtype=np.int8)
    lib.swg_synth_query(seed, lq, out.ctypes.data_as(_vp))
    return out


def hit_key(score, index):
    return int(lib.swg_hit_key(int(score), int(index)))


def key_hit(key):
    h = Hit()
    lib.swg_key_hit(int(key), C.byref(h))
    return int(h.score), int(h.index)


def topk_merge_keys(keys, k):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = (Hit * max(k, 1))()
    m = lib.swg_topk_merge_keys(keys.ctypes.data_as(_vp), keys.size, k, C.cast(out, _vp))
    return [(int(out[i].score), int(out[i].index)) for i in range(m)]


def mask_params(window=12, trigger=2.2, extend=2.5, replace=MASK_REPLACE_DEFAULT):
    return MaskParams(int(window), int(replace), float(trigger), float(extend))


def mask_tables(window=12, trigger=2.2, extend=2.5, replace=MASK_REPLACE_DEFAULT):
    """The integers of the masking rule: (T int32[65], threshold of `trigger`, threshold of `extend`) (swg_mask_tables)."""
    p = mask_params(window, trigger, extend, replace)
    T = np.zeros(65, dtype=np.int32)
    t1, t2 = C.c_int64(0), C.c_int64(0)
    _check(lib.swg_mask_tables(C.byref(p), T.ctypes.data_as(_vp), C.byref(t1), C.byref(t2)))
    return T, t1.value, t2.value


def align_hsps_host(sub, gap_open, gap_extend, seq, max_hsps, min_score=1, query=None, pssm=None, want_ops=True, want_counts=False):
    """The alignments of one pair on the host (swg_align_hsps_host, the twin of Context.align_hsps): sub int8[32, 32], one of
    query (table indices) and pssm (int8[lq, 32]), seq table indices -> the list of alignments as align_hsps gives it
    (index 0)."""
    t = np.ascontiguousarray(sub, dtype=np.int8) if sub is not None else None
    q = np.ascontiguousarray(query, dtype=np.int8) if query is not None else None
    p = np.ascontiguousarray(pssm, dtype=np.int8) if pssm is not None else None
    d = np.ascontiguousarray(seq, dtype=np.int8)
    lq = q.size if q is not None else (p.shape[0] if p is not None else 0)
    per, stride = max(int(max_hsps), 1), lq + d.size + 1
    out = (Alignment * per)()
    cnt = (AlignCounts * per)() if want_counts else None
    ops = C.create_string_buffer(per * stride) if want_ops else None
    n = C.c_uint32(0)
    _check(lib.swg_align_hsps_host(t.ctypes.data_as(_vp) if t is not None else None, int(gap_open), int(gap_extend),
                                   q.ctypes.data_as(_vp) if q is not None else None, p.ctypes.data_as(_vp) if p is not None else None, lq,
                                   d.ctypes.data_as(_vp), d.size, int(max_hsps), int(min_score), C.cast(out, _vp),
                                   C.cast(cnt, _vp) if want_counts else None, C.cast(ops, _vp) if want_ops else None, stride, C.byref(n)))
    res = []
    for r in range(n.value):
        a = {f: int(getattr(out[r], f)) for f, _ in Alignment._fields_ if f != "reserved"}
        if want_counts:
            a.update((f, int(getattr(cnt[r], f))) for f, _ in AlignCounts._fields_)
        if want_ops:
            a["ops"] = ops.raw[r * stride:r * stride + a["n_ops"]].decode()
        res.append(a)
    return res


# swg_comp_result, as a numpy record; COMP_UNWRITTEN is the status the Python layer puts into a record before the call, so
# that a hit the handle does not hold (which the library does not write) can be told from one it adjusted
COMP_DTYPE = np.dtype([("adj_score", "<i4"), ("scaled_score", "<i4"), ("ratio16", "<u4"), ("status", "<i4"), ("lambda_hit", "<f8")])
COMP_UNWRITTEN = -1
COMP_SCALE_DEFAULT = 32
COMP_CLASSES = ((16, 4), (16, 8), (32, 8), (64, 8), (64, 16), (64, 32))     # the fill kernel's (lanes, columns per lane)
COMP_COLS = 2048                                                           # its column limit: beyond it the host route


def _comp_records(n):
    out = np.zeros(max(n, 1), dtype=COMP_DTYPE)
    out["status"] = COMP_UNWRITTEN
    return out


def comp_adjust_host(sub, gap_open, gap_extend, seq, query=None, pssm=None, freq=None, scale=COMP_SCALE_DEFAULT):
    """Composition-based score adjustment of one pair on the host (swg_comp_adjust_host, the twin of Context.comp_adjust):
    sub int8[32, 32], one of query (table indices) and pssm (int8[lq, 32]), seq table indices, freq the background (None:
    the built-in table), scale the F of the rule -> (record of COMP_DTYPE, lambda_std)."""
    t = np.ascontiguousarray(sub, dtype=np.int8) if sub is not None else None
    q = np.ascontiguousarray(query, dtype=np.int8) if query is not None else None
    p = np.ascontiguousarray(pssm, dtype=np.int8) if pssm is not None else None
    d = np.ascontiguousarray(seq, dtype=np.int8)
    lq = q.size if q is not None else (p.shape[0] if p is not None else 0)
    f, fp = _freq(freq)
    out = _comp_records(1)
    lam = C.c_double(0.0)
    _check(lib.swg_comp_adjust_host(t.ctypes.data_as(_vp) if t is not None else None, int(gap_open), int(gap_extend),
                                    q.ctypes.data_as(_vp) if q is not None else None, p.ctypes.data_as(_vp) if p is not None else None, lq,
                                    d.ctypes.data_as(_vp), d.size, fp, int(scale), out.ctypes.data_as(_vp), C.byref(lam)))
    return out[0], lam.value


def seg_mask(seq, window=12, trigger=2.2, extend=2.5, replace=MASK_REPLACE_DEFAULT, want_segments=False):
    """The low-complexity mask of one sequence of table indices (swg_seg_mask, the host twin of Database.mask): a bool
    array, True where the position is masked; with want_segments also the number of kept runs.  The sequence is not
    changed: np.where(mask, replace, seq) is what a masked database holds."""
    a, ap = _i8(seq)
    p = mask_params(window, trigger, extend, replace)
    m = np.zeros(max(1, a.size), dtype=np.uint8)
    nm, ns = C.c_size_t(0), C.c_size_t(0)
    _check(lib.swg_seg_mask_segments(ap, a.size, C.byref(p), m.ctypes.data_as(_vp), C.byref(nm), C.byref(ns)))
    mask = m[:a.size].astype(bool)
    assert int(mask.sum()) == nm.value
    return (mask, ns.value) if want_segments else mask


def debug_mask_fail_alloc(n):
    """Test hook: the n-th device allocation of the next Database.mask finds no memory (0 disarms)."""
    lib.swg_debug_mask_fail_alloc(int(n))


def seg_mask_flat(flat, offsets, window=12, trigger=2.2, extend=2.5, replace=MASK_REPLACE_DEFAULT):
    """swg_seg_mask over a whole database laid end to end, on every core -> (masked copy of flat, {counts})."""
    a = np.array(flat, dtype=np.int8, order="C")
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    p = mask_params(window, trigger, extend, replace)
    tot = np.zeros(3, dtype=np.uint64)
    _check(lib.swg_seg_mask_flat(a.ctypes.data_as(_vp), off.ctypes.data_as(_vp), off.size - 1, C.byref(p), tot.ctypes.data_as(_vp)))
    return a, {"residues_masked": int(tot[0]), "sequences_masked": int(tot[1]), "segments": int(tot[2])}


def codon_table(ncbi_id):
    """NCBI genetic code 1, 2, 3, 4, 5, 6 or 11 as int8[64] residue indices in TCAG order (swg_codon_table)."""
    p = TranslateParams()
    _check(lib.swg_codon_table(int(ncbi_id), C.byref(p)))
    return np.array(p.codon[:], dtype=np.int8)


def translate_params(code=1, unknown=TRANSLATE_UNKNOWN_DEFAULT):
    """swg_translate_params of `code`: an NCBI id, or a 64-entry array of residue indices.  Values are passed as they are:
    the library refuses what is outside 1..31."""
    p = TranslateParams()
    if np.ndim(code) == 0:
        _check(lib.swg_codon_table(int(code), C.byref(p)))
    else:
        t = np.asarray(code)
        if t.shape != (64,) or t.min() < -128 or t.max() > 127:
            raise ValueError("a codon table is 64 residue indices")
        p.codon[:] = [int(v) for v in t]
    if not -128 <= int(unknown) <= 127:
        raise ValueError("unknown is a residue index")
    p.unknown = int(unknown)
    return p


def translate_seq(nt, code=1, unknown=TRANSLATE_UNKNOWN_DEFAULT):
    """The six frames of one nucleotide sequence of residue indices (swg_translate_seq, the host twin of
    Database.translate): six int8 arrays, frames 0..2 of the forward strand, then of the reverse complement."""
    a, ap = _i8(nt)
    p = translate_params(code, unknown)
    outs = [np.zeros(a.size // 3, dtype=np.int8) for _ in range(6)]
    ptrs = (_vp * 6)(*[o.ctypes.data_as(_vp) for o in outs])
    lens = (C.c_size_t * 6)()
    _check(lib.swg_translate_seq(ap, a.size, C.byref(p), ptrs, lens))
    return [o[:lens[g]].copy() for g, o in enumerate(outs)]


def translate_flat(flat, offsets, code=1, unknown=TRANSLATE_UNKNOWN_DEFAULT):
    """swg_translate_seq over a whole database laid end to end, on every core -> (flat, offsets) of its 6 n frames,
    frame g of sequence i at 6 i + g (swg_translate_flat)."""
    a, ap = _i8(flat)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    p = translate_params(code, unknown)
    out = np.zeros(2 * int(off[-1] - off[0]) if off.size > 1 else 0, dtype=np.int8)
    out_off = np.zeros(6 * (off.size - 1) + 1, dtype=np.uint64)
    _check(lib.swg_translate_flat(ap, off.ctypes.data_as(_vp), off.size - 1, C.byref(p), out.ctypes.data_as(_vp), out_off.ctypes.data_as(_vp)))
    return out[:int(out_off[-1])], out_off


def translate_hit(index):
    """A hit's index in a translated database -> (index of the nucleotide record, frame 0..5) (swg_translate_hit)."""
    i, f = C.c_uint32(0), C.c_int(0)
    lib.swg_translate_hit(int(index), C.byref(i), C.byref(f))
    return i.value, f.value


def translate_coords(frame, nt_len, d_begin, d_end):
    """The nucleotides that residues [d_begin, d_end) of `frame` cover: (nt_begin, nt_end), 0-based and half-open on
    the forward strand (swg_translate_coords)."""
    b, e = C.c_uint32(0), C.c_uint32(0)
    _check(lib.swg_translate_coords(int(frame), int(nt_len), int(d_begin), int(d_end), C.byref(b), C.byref(e)))
    return b.value, e.value


# ---------------------------------------------------------------------------
# database + context
# ---------------------------------------------------------------------------
class Database:
    """Host-packed database shard (swg_db); `upload(ctx)` makes it resident."""

    def __init__(self, flat=None, offsets=None, shard_rank=0, shard_count=1, path=None, index=None, n_total=None):
        """flat/offsets: the whole database, of which bins b % shard_count == shard_rank are kept; or, with
        index (global index of every sequence given) and n_total, a shard that was cut elsewhere."""
        self.handle = None
        if path is not None:            # load a packed-database file written by save()
            h = _vp()
            _check(lib.swg_db_load(path.encode(), C.byref(h)))
            self.handle = h
            return
        self._flat, fp = _i8(flat)
        self._off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = self._off.size - 1
        h = _vp()
        if index is not None:
            ix = np.ascontiguousarray(index, dtype=np.uint32)
            assert ix.size == n
            _check(lib.swg_db_pack_shard(fp, self._off.ctypes.data_as(_vp), n, ix.ctypes.data_as(_vp),
                                         int(n_total), C.byref(h)))
        else:
            _check(lib.swg_db_pack(fp, self._off.ctypes.data_as(_vp), n, shard_rank, shard_count, C.byref(h)))
        self.handle = h
        self._flat = None  # the library copied what it needs

    @classmethod
    def pack_shards(cls, flat, offsets, shard_count):
        """All shards of one database from ONE global sort (what swg_group_load uses) -> [Database] * shard_count."""
        f, fp = _i8(flat)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        hs = (_vp * shard_count)()
        _check(lib.swg_db_pack_shards(fp, off.ctypes.data_as(_vp), off.size - 1, shard_count, hs))
        out = []
        for h in hs:
            d = cls.__new__(cls)
            d.handle = _vp(h)
            out.append(d)
        return out

    count = property(lambda self: lib.swg_db_count(self.handle))
    total_count = property(lambda self: lib.swg_db_total_count(self.handle))
    residues = property(lambda self: lib.swg_db_residues(self.handle))
    packed_bytes = property(lambda self: lib.swg_db_packed_bytes(self.handle))

    def order(self):
        if self.count == 0:                 # a shard may hold nothing (fewer bins than shards)
            return np.zeros(0, dtype=np.uint32)
        return np.ctypeslib.as_array(lib.swg_db_order(self.handle), shape=(self.count,)).copy()

    def debug_plan(self, lq, n_cu=256, f16_pair=None):
        """Test hook: the cost model's first choice for this database and a query of lq residues (no device needed).
        f16_pair None: for the int16 cells; 0 (auto), 1 (v_perm_b32) or 2 (fma): for the packed-f16 cells with that
        pairing option, which adds the plan's pairing (fma, long_fma: 1 = v_pk_fma_f16) and the workgroup's LDS bytes."""
        out = np.zeros(16, dtype=np.int32)
        if f16_pair is None:
            _check(lib.swg_debug_plan(self.handle, lq, n_cu, out.ctypes.data_as(_vp)))
        else:
            _check(lib.swg_debug_plan_f16(self.handle, lq, n_cu, f16_pair, out.ctypes.data_as(_vp)))
        keys = ("classes", "K", "G", "W", "passes", "workgroups", "long_pairs", "long_K", "long_G", "long_W", "long_workgroups", "est_us",
                "last_pass_cols") + (() if f16_pair is None else ("fma", "lds_bytes", "long_fma"))
        return dict(zip(keys, (int(v) for v in out)))

    def debug_plan_forced(self, lq, cols=0, group=0, waves=0, form=0, f16_pair=0, last_pass=True, n_cu=256):
        """Test hook: the planner's answer for a forced geometry (options cols_per_wave, group_lanes, max_waves; long_split
        -1) on cells of `form` (0 int16 or wide, 2 packed f16, 3 gapless), no device needed -> debug_plan's dict with fma,
        lds_bytes and last_pass_cols for every form and "planned"; no plan is an answer: planned False, classes 0."""
        out = np.zeros(16, dtype=np.int32)
        _check(lib.swg_debug_plan_forced(self.handle, lq, n_cu, cols, group, waves, form, f16_pair, 1 if last_pass else 0,
                                         out.ctypes.data_as(_vp)))
        keys = ("classes", "K", "G", "W", "passes", "workgroups", "long_pairs", "long_K", "long_G", "long_W", "long_workgroups", "est_us",
                "last_pass_cols", "fma", "lds_bytes", "long_fma")
        d = dict(zip(keys, (int(v) for v in out)))
        d["planned"] = d["classes"] > 0
        return d

    def debug_plan_streams(self, sub, query, cols=0, group=0, waves=0, workgroups=0, n_cu=256):
        """Test hook: what a search of `query` under the 32 x 32 table `sub` plans with options engine = 2, work_queue = 0,
        f16 = 0, long_split = -1, cols_per_wave, group_lanes, max_waves and workgroups (no device needed) -> dict(planned,
        classes, K, G, W, passes, workgroups, streams, wide: the wide form of the int16 cells)."""
        t, tp = _i8(np.asarray(sub, dtype=np.int8).reshape(32, 32))
        q, qp = _i8(query)
        out = np.zeros(8, dtype=np.int32)
        _check(lib.swg_debug_plan_streams(self.handle, tp, qp, q.size, n_cu, cols, group, waves, workgroups, out.ctypes.data_as(_vp)))
        d = dict(zip(("classes", "K", "G", "W", "passes", "workgroups", "streams", "wide"), (int(v) for v in out)))
        d["planned"] = d["classes"] > 0
        return d

    def debug_plan_systolic(self, sub, query, gap_open, gap_extend, force_bits=0, cols=0, max_waves=0, workgroups=0, f16=1, n_cu=256):
        """Test hook: what a search of `query` under `sub` and the gap scores plans with option engine = 1 and force_bits,
        cols_per_wave, max_waves, workgroups, f16 (no device needed) -> dict(planned, K, W, passes, workgroups, f16: the
        packed-f16 cells, variant_max_waves, bits, rescore: an int32 re-score follows, and its rescore_K / _W / _passes)."""
        t, tp = _i8(np.asarray(sub, dtype=np.int8).reshape(32, 32))
        q, qp = _i8(query)
        out = np.zeros(12, dtype=np.int32)
        _check(lib.swg_debug_plan_systolic(self.handle, tp, qp, q.size, gap_open, gap_extend, n_cu, force_bits, cols, max_waves, workgroups,
                                           f16, out.ctypes.data_as(_vp)))
        keys = ("planned", "K", "W", "passes", "workgroups", "f16", "variant_max_waves", "bits", "rescore", "rescore_K", "rescore_W",
                "rescore_passes")
        d = dict(zip(keys, (int(v) for v in out)))
        d["planned"] = bool(d["planned"])
        return d

    _BATCH_PLAN_KEYS = ("batch", "K", "G", "W", "per_cu", "qq", "lds_bytes", "classes")

    def debug_plan_batch(self, lq_max, n_queries, form=2, qq=True, cols=0, group=0, batch_geometry=0, n_cu=256):
        """Test hook: what search_multi launches for n_queries queries, the longest of lq_max columns, on cells of `form`
        (0 packed int16, 2 packed f16: the hook has no scoring system) with options qq, cols_per_wave, group_lanes and
        batch_geometry, under engine = 2, no device needed -> dict(batch: launched as one batch -- False: one query after
        another, and the rest zero --, K, G, W, per_cu: workgroups per CU, qq: two queries per lane, lds_bytes of a
        workgroup, classes)."""
        out = np.zeros(8, dtype=np.int32)
        _check(lib.swg_debug_plan_batch(self.handle, lq_max, n_queries, n_cu, form, 1 if qq else 0, cols, group, batch_geometry,
                                        out.ctypes.data_as(_vp)))
        d = dict(zip(self._BATCH_PLAN_KEYS, (int(v) for v in out)))
        d["batch"], d["qq"] = bool(d["batch"]), bool(d["qq"])
        return d

    def debug_plan_lists(self, lists, lq_max, form=2, cols=0, group=0, batch_geometry=0, n_cu=256, lengths=None):
        """Test hook: the same for search_lists and one candidate list per query: the job table (debug_list_jobs) is
        described to the library by its pairs' lengths.  lengths: residues of every sequence by original index (default: of
        the sequences this database was packed from)."""
        if lengths is None:
            lengths = np.diff(self._off.astype(np.int64))
        slots, _ = self.debug_list_jobs(lists)
        order = self.order()
        lens = np.zeros(slots.size, dtype=np.uint32)
        held = slots != 0xFFFFFFFF
        lens[held] = np.asarray(lengths, dtype=np.int64)[order[slots[held]]]
        out = np.zeros(8, dtype=np.int32)
        _check(lib.swg_debug_plan_lists(lens.ctypes.data_as(_vp), lens.size // 2, lq_max, n_cu, form, cols, group, batch_geometry,
                                        out.ctypes.data_as(_vp)))
        d = dict(zip(self._BATCH_PLAN_KEYS, (int(v) for v in out)))
        d["batch"], d["qq"] = bool(d["batch"]), bool(d["qq"])
        return d

    def debug_plan_gapless(self, lq, n_cu=256):
        """Test hook: what search_gapless would plan for a query of lq residues with default options (no device needed):
        route 1 = the gapless cells, 0 = the gapped machinery with the gaps priced out; the fill's geometry either way."""
        out = np.zeros(6, dtype=np.int32)
        _check(lib.swg_debug_plan_gapless(self.handle, lq, n_cu, out.ctypes.data_as(_vp)))
        return dict(zip(("route", "K", "G", "W", "workgroups", "passes"), (int(v) for v in out)))

    def debug_engine(self, lq, n_cu=256, form=2):
        """Test hook: the cost model's estimates of both engines for this database and a query of lq residues (no device
        needed) -> dict(diag_us, systolic_us, systolic_K, systolic: the model picks the systolic engine)."""
        out = np.zeros(4, dtype=np.int32)
        _check(lib.swg_debug_engine(self.handle, lq, n_cu, form, out.ctypes.data_as(_vp)))
        return {"diag_us": int(out[0]), "systolic_us": int(out[1]), "systolic_K": int(out[2]), "systolic": bool(out[3])}

    def debug_split(self, lq, qbound):
        """Test hook: the both-forms cut (a query of lq columns that can score qbound at best) -> rows, first pair of the
        f16 part in the sorted order, residues of the f16 part (no device needed)."""
        out = np.zeros(3, dtype=np.uint64)
        _check(lib.swg_debug_split(self.handle, lq, qbound, out.ctypes.data_as(_vp)))
        return {"rows": int(out[0]), "first_pair": int(out[1]), "residues_f16": int(out[2])}

    def debug_pair_tokens(self, ctx, from_host):
        """Test hook: the pair-token image (uint32 dwords) built on the device or by the host builder."""
        n = C.c_size_t(0)
        _check(lib.swg_debug_pair_tokens(ctx.handle, self.handle, 1 if from_host else 0, None, 0, C.byref(n)), ctx.handle)
        out = np.zeros(n.value, dtype=np.uint32)
        _check(lib.swg_debug_pair_tokens(ctx.handle, self.handle, 1 if from_host else 0, out.ctypes.data_as(_vp),
                                         out.size, C.byref(n)), ctx.handle)
        return out

    def debug_view_ranks(self, indices):
        """Test hook: the sorted ranks (slots of this database; of its parent database for a view) that view(ctx,
        indices) would select, ascending (no device needed)."""
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        out = np.zeros(max(ix.size, 1), dtype=np.uint32)
        n = C.c_size_t(0)
        _check(lib.swg_debug_view_ranks(self.handle, ix.ctypes.data_as(_vp), ix.size, out.ctypes.data_as(_vp), C.byref(n)))
        return out[:n.value].copy()

    def debug_list_jobs(self, lists):
        """Test hook: the job table search_lists builds from one candidate list per query (no device needed) ->
        (slots uint32: the job database's slots as slots of this database -- of its parent for a view --, ~0 = the empty
        slot that ends an odd list; prefix uint64[n + 1]: row i's pairs are [prefix[i], prefix[i + 1]))."""
        flat, off = _lists(lists)
        n = C.c_size_t(0)
        prefix = np.zeros(len(lists) + 1, dtype=np.uint64)
        _check(lib.swg_debug_list_jobs(self.handle, flat.ctypes.data_as(_vp), off.ctypes.data_as(_vp), len(lists), None, 0,
                                       C.byref(n), prefix.ctypes.data_as(_vp)))
        slots = np.zeros(max(n.value, 1), dtype=np.uint32)
        _check(lib.swg_debug_list_jobs(self.handle, flat.ctypes.data_as(_vp), off.ctypes.data_as(_vp), len(lists),
                                       slots.ctypes.data_as(_vp), slots.size, C.byref(n), prefix.ctypes.data_as(_vp)))
        return slots[:n.value].copy(), prefix

    def debug_list_deal(self, lists, per_wg, resident):
        """Test hook: the workgroups of search_lists' one launch over these lists, dealt by work (no device needed): an
        (n, 2) array of (row, index within the row) per workgroup, for per_wg lane groups per workgroup and `resident`
        workgroups on the chip."""
        flat, off = _lists(lists)
        n = C.c_size_t(0)
        args = (self.handle, flat.ctypes.data_as(_vp), off.ctypes.data_as(_vp), len(lists), per_wg, resident)
        _check(lib.swg_debug_list_deal(*args, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 2), dtype=np.uint32)
        _check(lib.swg_debug_list_deal(*args, out.ctypes.data_as(_vp), out.shape[0], C.byref(n)))
        return out[:n.value].copy()

    def view(self, ctx, indices):
        """The sequences with the listed ORIGINAL indices (any order, duplicates collapse, those of other shards
        ignored) as a Database of its own that reads this one's resident bytes (swg_db_view).  Scores stay indexed by
        original index and only the selected entries are written.  Either object may be closed first."""
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        h = _vp()
        _check(lib.swg_db_view(ctx.handle, self.handle, ix.ctypes.data_as(_vp), ix.size, C.byref(h)), ctx.handle)
        v = Database.__new__(Database)
        v.handle = h
        return v

    def composition(self, ctx):
        """Residue counts of this resident database, shard or view: uint64[32] by residue index (swg_db_composition)."""
        counts = np.zeros(32, dtype=np.uint64)
        _check(lib.swg_db_composition(ctx.handle, self.handle, counts.ctypes.data_as(_vp)), ctx.handle)
        return counts

    def mask(self, ctx, window=12, trigger=2.2, extend=2.5, replace=MASK_REPLACE_DEFAULT):
        """A masked copy of this resident root database, made on the device (swg_db_mask): the same sequences, order
        and original indices, with `replace` at every position of a low-complexity region.  A Database of its own."""
        p = mask_params(window, trigger, extend, replace)
        h = _vp()
        _check(lib.swg_db_mask(ctx.handle, self.handle, C.byref(p), C.byref(h)), ctx.handle)
        m = Database.__new__(Database)
        m.handle = h
        return m

    def mask_info(self):
        """What Database.mask made this database with and what it covered (swg_db_mask_info)."""
        info = MaskInfo()
        _check(lib.swg_db_mask_info(self.handle, C.byref(info)))
        return info.as_dict()

    def translate(self, ctx, code=1, unknown=TRANSLATE_UNKNOWN_DEFAULT):
        """The six-frame translation of this resident root NUCLEOTIDE database, made on the device (swg_db_translate):
        frame g of sequence i is sequence 6 i + g of the result.  code: an NCBI id or 64 residue indices in TCAG order.
        A Database of its own."""
        p = translate_params(code, unknown)
        h = _vp()
        _check(lib.swg_db_translate(ctx.handle, self.handle, C.byref(p), C.byref(h)), ctx.handle)
        t = Database.__new__(Database)
        t.handle = h
        return t

    def translate_info(self):
        """What Database.translate made this database with and what it wrote (swg_db_translate_info)."""
        info = TranslateInfo()
        _check(lib.swg_db_translate_info(self.handle, C.byref(info)))
        return info.as_dict()

    def sequence(self, i):
        """The table indices of the sequence with ORIGINAL index i, from the host image (swg_db_sequence)."""
        n = C.c_size_t(0)
        rc = lib.swg_db_sequence(self.handle, int(i), None, 0, C.byref(n))
        if rc != SWG_OK and n.value == 0:
            _check(rc)
        out = np.zeros(n.value, dtype=np.int8)
        if n.value:
            _check(lib.swg_db_sequence(self.handle, int(i), out.ctypes.data_as(_vp), out.size, C.byref(n)))
        return out

    def save(self, path):
        _check(lib.swg_db_save(self.handle, path.encode()))

    def upload(self, ctx):
        _check(lib.swg_db_upload(ctx.handle, self.handle), ctx.handle)
        return self

    def close(self):
        if self.handle:
            lib.swg_db_free(self.handle)
            self.handle = None

    __del__ = close


class Context:
    """swg_ctx: one GPU, one query, one scoring system."""

    def __init__(self, device=0):
        self.handle = None
        self._lq = 0        # length of the query last set (build_pssm sizes its output by it)
        cfg = Config()
        cfg.device = device
        h = _vp()
        _check(lib.swg_create(C.byref(cfg), C.byref(h)))
        self.handle = h

    def set_option(self, key, value):
        _check(lib.swg_set_option(self.handle, key.encode(), int(value)), self.handle)

    def set_scoring(self, sub, gap_open, gap_extend):
        if isinstance(sub, Scoring):
            sub = sub.table()
        s, sp = _i8(np.asarray(sub).reshape(32, 32))
        _check(lib.swg_set_scoring(self.handle, sp, int(gap_open), int(gap_extend)), self.handle)

    def set_query(self, idx):
        q, qp = _i8(idx)
        _check(lib.swg_set_query(self.handle, qp, q.size), self.handle)
        self._lq = q.size

    def set_query_pssm(self, pssm):
        """A position-specific query: pssm int8[lq, 32], row i = query position i's scores by residue index."""
        p, pp, lq = _pssm(pssm)
        _check(lib.swg_set_query_pssm(self.handle, pp, lq), self.handle)
        self._lq = lq

    def search(self, db, want_scores=True, k=0, _fn=None):
        """-> (scores int32[total] or None, hits [(score, index)], stats dict)."""
        scores = np.zeros(db.total_count, dtype=np.int32) if want_scores else None
        hits = (Hit * max(k, 1))()
        nh = C.c_size_t(0)
        st = Stats()
        rc = (_fn or lib.swg_search)(self.handle, db.handle, scores.ctypes.data_as(_vp) if want_scores else None,
                                     C.cast(hits, _vp) if k else None, k, C.byref(nh), C.byref(st))
        _check(rc, self.handle)
        return scores, [(int(hits[i].score), int(hits[i].index)) for i in range(nh.value)], st.as_dict()

    def search_gapless(self, db, want_scores=True, k=0):
        """The gapless prefilter score (best ungapped diagonal segment) of the context's query against db, shaped like
        search; the gap scores of set_scoring are not read (swg_search_gapless)."""
        return self.search(db, want_scores, k, _fn=lib.swg_search_gapless)

    def search_above(self, db, min_score, cap=None, gapless=False):
        """Every sequence of db that scores at least min_score (>= 1) against the context's query: -> (hits [(score,
        index)] -- the best min(cap, n_total) in the library's order --, n_total, stats dict).  cap None: room for every
        sequence of db; cap 0: a pure count.  gapless: the gapless prefilter score (swg_search_above,
        swg_search_gapless_above)."""
        cap = db.count if cap is None else int(cap)
        hits = (Hit * max(cap, 1))()
        nh, nt = C.c_size_t(0), C.c_uint64(0)
        st = Stats()
        fn = lib.swg_search_gapless_above if gapless else lib.swg_search_above
        rc = fn(self.handle, db.handle, int(min_score), C.cast(hits, _vp) if cap else None, cap, C.byref(nh), C.byref(nt), C.byref(st))
        _check(rc, self.handle)
        a = np.frombuffer(hits, dtype=np.dtype([("score", np.int32), ("index", np.uint32)]), count=nh.value)
        return list(zip(a["score"].tolist(), a["index"].tolist())), int(nt.value), st.as_dict()

    def calibrate(self, freq=None, gapless=False):
        """The context's query scored against random sequences and fitted on the device (swg_calibrate) -> dict(lambda, K,
        mu, lq, n_seqs, seq_len, status), what evalue / bitscore / evalue_min_score take.  freq: 32 weights by residue
        index (None: the built-in table; Database.composition's counts: the database's own)."""
        f, fp = _freq(freq)
        p = EvalueParams()
        _check(lib.swg_calibrate(self.handle, fp, int(bool(gapless)), C.byref(p)), self.handle)
        return p.as_dict()

    def calibrate_multi(self, queries, freq=None, gapless=False):
        """calibrate for a list of index queries -> list of dicts; the context's own query is kept (swg_calibrate_multi)."""
        nq = len(queries)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if nq else np.zeros(1), dtype=np.int8)
        return self._calibrate_multi(lib.swg_calibrate_multi, qflat, qoff, freq, gapless)

    def calibrate_multi_pssm(self, pssms, freq=None, gapless=False):
        """calibrate_multi with position-specific queries: pssms as search_multi_pssm takes them."""
        nq = len(pssms)
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if nq else np.zeros((1, 32)), dtype=np.int8)
        return self._calibrate_multi(lib.swg_calibrate_multi_pssm, pflat, qoff, freq, gapless)

    def _calibrate_multi(self, fn, qflat, qoff, freq, gapless):
        nq = len(qoff) - 1
        f, fp = _freq(freq)
        out = (EvalueParams * max(nq, 1))()
        _check(fn(self.handle, qflat.ctypes.data_as(_vp), qoff.ctypes.data_as(_vp), nq, fp, int(bool(gapless)), C.cast(out, _vp)), self.handle)
        return [out[i].as_dict() for i in range(nq)]

    def debug_calib_iters(self):
        """Newton steps of each query's fit in the last calibrate* call (tests)."""
        n = C.c_size_t(0)
        _check(lib.swg_debug_calib_iters(self.handle, None, 0, C.byref(n)), self.handle)
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        _check(lib.swg_debug_calib_iters(self.handle, out.ctypes.data_as(_vp), n.value, C.byref(n)), self.handle)
        return out[:n.value].tolist()

    def search_above_multi(self, db, queries, min_scores, cap=None, gapless=False):
        """search_above for a list of index queries, each with its own least score (min_scores: a list, or one int for all):
        -> (hits: list of lists of (score, index) -- per query the best min(cap, n_total[i]) in the library's order --,
        n_total: list of int, stats dict).  cap None: room for every sequence of db; cap 0: counts only.  gapless: the
        gapless prefilter score.  The context's own query is kept (swg_search_above_multi,
        swg_search_gapless_above_multi)."""
        nq = len(queries)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if nq else np.zeros(0), dtype=np.int8)
        fn = lib.swg_search_gapless_above_multi if gapless else lib.swg_search_above_multi
        return self._above_multi(fn, db, qflat, qoff, min_scores, cap)

    def search_above_multi_pssm(self, db, pssms, min_scores, cap=None, gapless=False):
        """search_above_multi with position-specific queries: pssms as search_multi_pssm takes them."""
        nq = len(pssms)
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if nq else np.zeros((0, 32)), dtype=np.int8)
        fn = lib.swg_search_gapless_above_multi_pssm if gapless else lib.swg_search_above_multi_pssm
        return self._above_multi(fn, db, pflat, qoff, min_scores, cap)

    def _above_multi(self, fn, db, qflat, qoff, min_scores, cap):
        nq = len(qoff) - 1
        ms = np.full(nq, min_scores, dtype=np.int32) if np.isscalar(min_scores) else np.ascontiguousarray(min_scores, dtype=np.int32)
        if ms.shape != (nq,):
            raise ValueError("min_scores: %s for %d queries" % (ms.shape, nq))
        ms = np.concatenate([ms, np.zeros(1, dtype=np.int32)])    # (never an empty buffer)
        cap = db.count if cap is None else int(cap)
        hits = np.zeros(max(nq * cap, 1), dtype=np.dtype([("score", np.int32), ("index", np.uint32)]))
        nh = np.zeros(max(nq, 1), dtype=np.uintp)
        nt = np.zeros(max(nq, 1), dtype=np.uint64)
        st = Stats()
        rc = fn(self.handle, db.handle, qflat.ctypes.data_as(_vp), qoff.ctypes.data_as(_vp), nq, ms.ctypes.data_as(_vp),
                hits.ctypes.data_as(_vp) if cap else None, cap, nh.ctypes.data_as(_vp), nt.ctypes.data_as(_vp), C.byref(st))
        _check(rc, self.handle)
        out = []
        for i in range(nq):
            a = hits[i * cap:i * cap + int(nh[i])]
            out.append(list(zip(a["score"].tolist(), a["index"].tolist())))
        return out, [int(v) for v in nt[:nq]], st.as_dict()

    def search_gapless_multi(self, db, queries, k=0, want_scores=True):
        """search_gapless for a list of index queries, shaped like search_multi; the context's own query is kept."""
        nq = len(queries)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if nq else np.zeros(0), dtype=np.int8)
        return self._multi(lib.swg_search_gapless_multi, db, qflat, qoff, k, want_scores)

    def search_gapless_multi_pssm(self, db, pssms, k=0, want_scores=True):
        """search_gapless for a list of (lq, 32) int8 PSSMs, shaped like search_multi_pssm."""
        nq = len(pssms)
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if nq else np.zeros((0, 32)), dtype=np.int8)
        return self._multi(lib.swg_search_gapless_multi_pssm, db, pflat, qoff, k, want_scores)

    def search_multi(self, db, queries, k=0, want_scores=True):
        """Several queries (list of index arrays) against db in one pass -> (scores int32[nq, total] or None,
        hits: list of lists, stats dict)."""
        nq = len(queries)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if nq else np.zeros(0), dtype=np.int8)
        return self._multi(lib.swg_search_multi, db, qflat, qoff, k, want_scores)

    def search_multi_pssm(self, db, pssms, k=0, want_scores=True):
        """search_multi with position-specific queries: pssms is a list of (lq, 32) int8 arrays (as set_query_pssm
        takes one); the context's own query is left as it was."""
        nq = len(pssms)
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if nq else np.zeros((0, 32)), dtype=np.int8)
        return self._multi(lib.swg_search_multi_pssm, db, pflat, qoff, k, want_scores)

    def search_lists(self, db, queries, lists, k=0, want_scores=True, fill=0):
        """Every query against its own candidate list (original indices, any order, duplicates allowed, possibly empty)
        in one pass -> (scores: list of int32 arrays parallel to each list, or None; hits: list of lists; stats dict).
        Entries the library ignores (another shard's, outside a view) keep `fill`."""
        nq = len(queries)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if nq else np.zeros(0), dtype=np.int8)
        return self._lists_call(lib.swg_search_lists, db, qflat, qoff, lists, k, want_scores, fill)

    def search_lists_pssm(self, db, pssms, lists, k=0, want_scores=True, fill=0):
        """search_lists with position-specific queries: pssms as search_multi_pssm takes them."""
        nq = len(pssms)
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if nq else np.zeros((0, 32)), dtype=np.int8)
        return self._lists_call(lib.swg_search_lists_pssm, db, pflat, qoff, lists, k, want_scores, fill)

    def _lists_call(self, fn, db, qflat, qoff, lists, k, want_scores, fill):
        nq = len(qoff) - 1
        if len(lists) != nq:
            raise ValueError("lists: %d for %d queries" % (len(lists), nq))
        cflat, coff = _lists(lists)
        scores = np.full(max(int(coff[nq]), 1), fill, dtype=np.int32) if want_scores else None
        hits = (Hit * max(k * nq, 1))()
        nh = (C.c_size_t * max(nq, 1))()
        st = Stats()
        rc = fn(self.handle, db.handle, qflat.ctypes.data_as(_vp), qoff.ctypes.data_as(_vp), nq, cflat.ctypes.data_as(_vp),
                coff.ctypes.data_as(_vp), scores.ctypes.data_as(_vp) if want_scores else None, C.cast(hits, _vp) if k else None, k,
                C.cast(nh, _vp), C.byref(st))
        _check(rc, self.handle)
        out = [[(int(hits[i * k + j].score), int(hits[i * k + j].index)) for j in range(nh[i])] for i in range(nq)]
        per = [scores[int(coff[i]):int(coff[i + 1])].copy() for i in range(nq)] if want_scores else None
        return per, out, st.as_dict()

    def _multi(self, fn, db, qflat, qoff, k, want_scores):
        nq = len(qoff) - 1
        scores = np.zeros((nq, db.total_count), dtype=np.int32) if want_scores else None
        hits = (Hit * max(k * nq, 1))()
        nh = (C.c_size_t * max(nq, 1))()
        st = Stats()
        rc = fn(self.handle, db.handle, qflat.ctypes.data_as(_vp), qoff.ctypes.data_as(_vp), nq,
                scores.ctypes.data_as(_vp) if want_scores else None, C.cast(hits, _vp) if k else None, k,
                C.cast(nh, _vp), C.byref(st))
        _check(rc, self.handle)
        out = [[(int(hits[i * k + j].score), int(hits[i * k + j].index)) for j in range(nh[i])] for i in range(nq)]
        return scores, out, st.as_dict()

    def search_begin(self, db, k=0, want_scores=False):
        """Queue a search; returns a ticket for search_end / search_end_keys."""
        t = C.c_int(-1)
        _check(lib.swg_search_begin(self.handle, db.handle, 1 if want_scores else 0, k, C.byref(t)), self.handle)
        return (t.value, db, k, want_scores)

    def search_end(self, ticket):
        t, db, k, want_scores = ticket
        scores = np.zeros(db.total_count, dtype=np.int32) if want_scores else None
        hits = (Hit * max(k, 1))()
        nh = C.c_size_t(0)
        st = Stats()
        _check(lib.swg_search_end(self.handle, t, scores.ctypes.data_as(_vp) if want_scores else None,
                                  C.cast(hits, _vp) if k else None, C.byref(nh), C.byref(st)), self.handle)
        return scores, [(int(hits[i].score), int(hits[i].index)) for i in range(nh.value)], st.as_dict()

    def search_end_keys(self, ticket):
        """As search_keys, for a search queued with search_begin."""
        t, db, k, _ = ticket
        hits = (Hit * max(k, 1))()
        nh = C.c_size_t(0)
        st = Stats()
        _check(lib.swg_search_end(self.handle, t, None, C.cast(hits, _vp), C.byref(nh), C.byref(st)), self.handle)
        return self._hit_keys(hits, k, nh.value), st.as_dict()

    def align_hits(self, db, hits, want_ops=True, ops_stride=None):
        """Alignments of the given hits [(score, index)] -> list of dicts with score, index,
        q_begin, q_end, d_begin, d_end and (want_ops) the path as a string of M/I/D."""
        n = len(hits)
        arr = (Hit * max(n, 1))()
        for i, (sc, ix) in enumerate(hits):
            arr[i].score, arr[i].index = int(sc), int(ix)
        out = (Alignment * max(n, 1))()
        stride = int(ops_stride if ops_stride is not None else lib.swg_align_ops_bound(self.handle, db.handle))
        ops = C.create_string_buffer(max(1, n * stride)) if want_ops else None
        _check(lib.swg_align_hits(self.handle, db.handle, C.cast(arr, _vp), n, C.cast(out, _vp),
                                  C.cast(ops, _vp) if want_ops else None, stride), self.handle)
        res = []
        for i in range(n):
            a = {f: int(getattr(out[i], f)) for f, _ in Alignment._fields_ if f != "reserved"}
            if want_ops:
                a["ops"] = ops.raw[i * stride:i * stride + a["n_ops"]].decode()
            res.append(a)
        return res

    def align_hits_multi(self, db, queries, hits, want_ops=True, ops_stride=None):
        """Alignments of a batch's hits in one call: queries as search_multi takes them, hits the list of lists of
        (score, index) it returns -> list of lists of align_hits' dicts.  The context's own query is left as it was."""
        qoff = np.zeros(len(queries) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if len(queries) else np.zeros(0), dtype=np.int8)
        return self._align_multi(lib.swg_align_hits_multi, db, qflat, qoff, hits, want_ops, ops_stride)

    def align_hits_multi_pssm(self, db, pssms, hits, want_ops=True, ops_stride=None):
        """align_hits_multi with position-specific queries: pssms as search_multi_pssm takes them."""
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(len(rows) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 32)), dtype=np.int8)
        return self._align_multi(lib.swg_align_hits_multi_pssm, db, pflat, qoff, hits, want_ops, ops_stride)

    def build_pssm(self, db, hits, query_residues=None, freq=None, pseudocount=PSSM_PSEUDOCOUNT_DEFAULT, want_values=False):
        """The PSSM of the context's query from its hits [(score, index)], built on the device (swg_pssm_build) -> (pssm
        int8[lq, 32], values float64[lq, 32] or None, info dict).  query_residues: None for an index query; the query's
        residues when the context's query is a PSSM (the next iteration of a profile search)."""
        n = len(hits)
        arr = (Hit * max(n, 1))()
        for i, (sc, ix) in enumerate(hits):
            arr[i].score, arr[i].index = int(sc), int(ix)
        lq = self._lq                   # (the library writes as many rows as the context's query has)
        qr, qrp = (None, None) if query_residues is None else _i8(query_residues)
        if qr is not None and qr.size != lq:
            raise ValueError("query_residues: %d residues for a query of %d positions" % (qr.size, lq))
        f, fp = _freq(freq)
        pssm = np.zeros((max(lq, 1), 32), dtype=np.int8)
        values = np.zeros((max(lq, 1), 32), dtype=np.float64) if want_values else None
        info = PssmInfo()
        _check(lib.swg_pssm_build(self.handle, db.handle, C.cast(arr, _vp), n, qrp, fp, float(pseudocount), pssm.ctypes.data_as(_vp),
                                  values.ctypes.data_as(_vp) if want_values else None, C.byref(info)), self.handle)
        return pssm[:lq], (values[:lq] if want_values else None), info.as_dict()

    def build_pssm_multi(self, db, queries, hits, freq=None, pseudocount=PSSM_PSEUDOCOUNT_DEFAULT, want_values=False):
        """build_pssm for a batch: queries as search_multi takes them, hits the list of lists of (score, index) that
        search_multi or search_above_multi returns -> (pssms: list of int8[lq_i, 32], ready for search_multi_pssm; values:
        list of float64[lq_i, 32] or None; infos: list of dicts).  The context's own query is kept (swg_pssm_build_multi)."""
        return self._build_pssm_multi(db, None, queries, hits, freq, pseudocount, want_values)

    def build_pssm_multi_pssm(self, db, pssms, queries, hits, freq=None, pseudocount=PSSM_PSEUDOCOUNT_DEFAULT, want_values=False):
        """build_pssm_multi with position-specific queries: pssms score the alignments, queries are their residues."""
        return self._build_pssm_multi(db, pssms, queries, hits, freq, pseudocount, want_values)

    def _build_pssm_multi(self, db, pssms, queries, hits, freq, pseudocount, want_values):
        nq = len(queries)
        if len(hits) != nq or (pssms is not None and len(pssms) != nq):
            raise ValueError("hits / pssms: one row per query (%d queries)" % nq)
        qoff = np.zeros(nq + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        total = int(qoff[nq])
        qflat = np.ascontiguousarray(np.concatenate(queries) if nq else np.zeros(1), dtype=np.int8)
        k = max((len(row) for row in hits), default=0)
        arr = (Hit * max(nq * k, 1))()
        nh = (C.c_size_t * max(nq, 1))()
        for i, row in enumerate(hits):
            nh[i] = len(row)
            for j, (sc, ix) in enumerate(row):
                arr[i * k + j].score, arr[i * k + j].index = int(sc), int(ix)
        f, fp = _freq(freq)
        out = np.zeros((max(total, 1), 32), dtype=np.int8)
        values = np.zeros((max(total, 1), 32), dtype=np.float64) if want_values else None
        info = (PssmInfo * max(nq, 1))()
        tail = (C.cast(arr, _vp), k, C.cast(nh, _vp), fp, float(pseudocount), out.ctypes.data_as(_vp),
                values.ctypes.data_as(_vp) if want_values else None, C.cast(info, _vp))
        if pssms is None:
            rc = lib.swg_pssm_build_multi(self.handle, db.handle, qflat.ctypes.data_as(_vp), qoff.ctypes.data_as(_vp), nq, *tail)
        else:
            rows = [_pssm(p)[0] for p in pssms]
            if [r.shape[0] for r in rows] != [len(q) for q in queries]:
                raise ValueError("pssms and queries differ in length")
            pflat = np.ascontiguousarray(np.concatenate(rows) if nq else np.zeros((1, 32)), dtype=np.int8)
            rc = lib.swg_pssm_build_multi_pssm(self.handle, db.handle, pflat.ctypes.data_as(_vp), qflat.ctypes.data_as(_vp),
                                               qoff.ctypes.data_as(_vp), nq, *tail)
        _check(rc, self.handle)
        cut = [(int(qoff[i]), int(qoff[i + 1])) for i in range(nq)]
        return ([out[a:b].copy() for a, b in cut], [values[a:b].copy() for a, b in cut] if want_values else None,
                [info[i].as_dict() for i in range(nq)])

    def align_bounds(self, db, hits):
        """align_hits(db, hits, want_ops=False) from a forward pass alone (swg_align_bounds: no traceback is run)."""
        n = len(hits)
        arr = (Hit * max(n, 1))()
        for i, (sc, ix) in enumerate(hits):
            arr[i].score, arr[i].index = int(sc), int(ix)
        out = (Alignment * max(n, 1))()
        _check(lib.swg_align_bounds(self.handle, db.handle, C.cast(arr, _vp), n, C.cast(out, _vp)), self.handle)
        return [{f: int(getattr(out[i], f)) for f, _ in Alignment._fields_ if f != "reserved"} for i in range(n)]

    def align_bounds_multi(self, db, queries, hits):
        """align_hits_multi(db, queries, hits, want_ops=False) from a forward pass alone (swg_align_bounds_multi)."""
        qoff = np.zeros(len(queries) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if len(queries) else np.zeros(0), dtype=np.int8)
        return self._align_multi(lib.swg_align_bounds_multi, db, qflat, qoff, hits, False, None, bounds=True)

    def align_bounds_multi_pssm(self, db, pssms, hits):
        """align_bounds_multi with position-specific queries: pssms as search_multi_pssm takes them."""
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(len(rows) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 32)), dtype=np.int8)
        return self._align_multi(lib.swg_align_bounds_multi_pssm, db, pflat, qoff, hits, False, None, bounds=True)

    def align_stats(self, db, hits):
        """align_bounds(db, hits) plus the counts of a tabular report's line (swg_align_stats): each dict also has n_ident,
        n_match, n_gap_open and n_gap of the path align_hits would spell -- still from a forward pass alone."""
        n = len(hits)
        arr = (Hit * max(n, 1))()
        for i, (sc, ix) in enumerate(hits):
            arr[i].score, arr[i].index = int(sc), int(ix)
        out = (Alignment * max(n, 1))()
        cnt = (AlignCounts * max(n, 1))()
        _check(lib.swg_align_stats(self.handle, db.handle, C.cast(arr, _vp), n, C.cast(out, _vp), C.cast(cnt, _vp)), self.handle)
        return [self._stats_dict(out[i], cnt[i]) for i in range(n)]

    def align_stats_multi(self, db, queries, hits):
        """align_bounds_multi(db, queries, hits) plus align_stats' four counts per hit (swg_align_stats_multi)."""
        qoff = np.zeros(len(queries) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if len(queries) else np.zeros(0), dtype=np.int8)
        return self._align_multi(lib.swg_align_stats_multi, db, qflat, qoff, hits, False, None, bounds=True, stats=True)

    def align_stats_multi_pssm(self, db, pssms, hits):
        """align_stats_multi with position-specific queries; identity is counted against each PSSM's consensus (the lowest
        residue index in 1..31 whose score is the row's maximum over 1..31)."""
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(len(rows) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 32)), dtype=np.int8)
        return self._align_multi(lib.swg_align_stats_multi_pssm, db, pflat, qoff, hits, False, None, bounds=True, stats=True)

    def comp_adjust(self, db, hits, freq=None):
        """Composition-based score adjustment of the context's query's hits [(score, index)] (swg_comp_adjust) -> (records
        of COMP_DTYPE parallel to hits, lambda_std).  A hit the handle does not hold keeps status COMP_UNWRITTEN.  The scale
        F is option "comp_scale"; alignments and counts stay those of the unadjusted scores."""
        n = len(hits)
        arr = (Hit * max(n, 1))()
        for i, (sc, ix) in enumerate(hits):
            arr[i].score, arr[i].index = int(sc), int(ix)
        f, fp = _freq(freq)
        out = _comp_records(n)
        lam = np.zeros(1, dtype=np.float64)
        _check(lib.swg_comp_adjust(self.handle, db.handle, C.cast(arr, _vp), n, fp, out.ctypes.data_as(_vp), lam.ctypes.data_as(_vp)),
               self.handle)
        return out[:n], float(lam[0])

    def comp_adjust_multi(self, db, queries, hits, freq=None):
        """comp_adjust for a batch: queries as search_multi takes them, hits one list of (score, index) per query -> (list of
        record arrays, one per query, parallel to its hits; lambda_std float64[n_queries]).  The context's own query is
        kept (swg_comp_adjust_multi)."""
        qoff = np.zeros(len(queries) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if len(queries) else np.zeros(1), dtype=np.int8)
        return self._comp_multi(lib.swg_comp_adjust_multi, db, qflat, qoff, hits, freq)

    def comp_adjust_multi_pssm(self, db, pssms, hits, freq=None):
        """comp_adjust_multi with position-specific queries: pssms as search_multi_pssm takes them."""
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(len(rows) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((1, 32)), dtype=np.int8)
        return self._comp_multi(lib.swg_comp_adjust_multi_pssm, db, pflat, qoff, hits, freq)

    def _comp_multi(self, fn, db, qflat, qoff, hits, freq):
        nq = len(qoff) - 1
        if len(hits) != nq:
            raise ValueError("hits: %d rows for %d queries" % (len(hits), nq))
        k = max((len(row) for row in hits), default=0)
        arr = (Hit * max(nq * k, 1))()
        nh = (C.c_size_t * max(nq, 1))()
        for i, row in enumerate(hits):
            nh[i] = len(row)
            for j, (sc, ix) in enumerate(row):
                arr[i * k + j].score, arr[i * k + j].index = int(sc), int(ix)
        f, fp = _freq(freq)
        out = _comp_records(nq * k)
        lam = np.zeros(max(nq, 1), dtype=np.float64)
        _check(fn(self.handle, db.handle, qflat.ctypes.data_as(_vp), qoff.ctypes.data_as(_vp), nq, C.cast(arr, _vp), k, C.cast(nh, _vp), fp,
                  out.ctypes.data_as(_vp), lam.ctypes.data_as(_vp)), self.handle)
        return [out[i * k:i * k + len(row)].copy() for i, row in enumerate(hits)], lam[:nq]

    def debug_comp_last(self):
        """What the last comp_adjust* call of this context did (swg_debug_comp_last) -> dict: pairs on the fill kernel, pairs
        on the host route, launches of the fill kernel, its column limit, the scale, and the pairs of each instantiation
        (G, K), narrowest first."""
        out = np.zeros(12, dtype=np.uint32)
        _check(lib.swg_debug_comp_last(self.handle, out.ctypes.data_as(_vp)), self.handle)
        res = dict(zip(("kernel_pairs", "host_pairs", "launches", "column_limit", "scale"), (int(v) for v in out[:5])))
        res["class_pairs"] = dict(zip(COMP_CLASSES, (int(v) for v in out[5:11])))
        return res

    def align_hsps(self, db, hits, max_hsps, min_score=1, want_ops=True, want_counts=False):
        """Every non-overlapping alignment of each hit at or above min_score, at most max_hsps of them, best first
        (swg_align_hsps) -> per hit the list of its alignments: align_hits' dicts, with align_stats' four counts when
        want_counts.  The first of a hit's alignments is align_hits' one."""
        n = len(hits)
        arr = (Hit * max(n, 1))()
        for i, (sc, ix) in enumerate(hits):
            arr[i].score, arr[i].index = int(sc), int(ix)
        stride = int(lib.swg_align_ops_bound(self.handle, db.handle))
        return self._align_hsps(lambda *tail: lib.swg_align_hsps(self.handle, db.handle, C.cast(arr, _vp), n, *tail),
                                [n], n, stride, max_hsps, min_score, want_ops, want_counts)[0]

    def align_hsps_multi(self, db, queries, hits, max_hsps, min_score=1, want_ops=True, want_counts=False):
        """align_hsps for a batch: queries and hits as align_hits_multi takes them -> per query, per hit, the list of its
        alignments.  The context's own query is left as it was."""
        qoff = np.zeros(len(queries) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        qflat = np.ascontiguousarray(np.concatenate(queries) if len(queries) else np.zeros(0), dtype=np.int8)
        return self._align_hsps_multi(lib.swg_align_hsps_multi, db, qflat, qoff, hits, max_hsps, min_score, want_ops, want_counts)

    def align_hsps_multi_pssm(self, db, pssms, hits, max_hsps, min_score=1, want_ops=True, want_counts=False):
        """align_hsps_multi with position-specific queries; identity is counted against each PSSM's consensus."""
        rows = [_pssm(p)[0] for p in pssms]
        qoff = np.zeros(len(rows) + 1, dtype=np.uint64)
        qoff[1:] = np.cumsum([r.shape[0] for r in rows])
        pflat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 32)), dtype=np.int8)
        return self._align_hsps_multi(lib.swg_align_hsps_multi_pssm, db, pflat, qoff, hits, max_hsps, min_score, want_ops, want_counts)

    def _align_hsps_multi(self, fn, db, qflat, qoff, hits, max_hsps, min_score, want_ops, want_counts):
        nq = len(qoff) - 1
        if len(hits) != nq:
            raise ValueError("hits: %d rows for %d queries" % (len(hits), nq))
        k = max((len(row) for row in hits), default=0)
        arr = (Hit * max(nq * k, 1))()
        nh = (C.c_size_t * max(nq, 1))()
        for i, row in enumerate(hits):
            nh[i] = len(row)
            for j, (sc, ix) in enumerate(row):
                arr[i * k + j].score, arr[i * k + j].index = int(sc), int(ix)
        stride = int(lib.swg_align_ops_bound_multi(db.handle, qoff.ctypes.data_as(_vp), nq))
        return self._align_hsps(lambda *tail: fn(self.handle, db.handle, qflat.ctypes.data_as(_vp), qoff.ctypes.data_as(_vp), nq,
                                                 C.cast(arr, _vp), k, C.cast(nh, _vp), *tail),
                                [len(row) for row in hits], k, stride, max_hsps, min_score, want_ops, want_counts)

    def _align_hsps(self, call, row_lens, k, stride, max_hsps, min_score, want_ops, want_counts):
        """The outputs of one swg_align_hsps* call over rows of k hit slots, row i holding row_lens[i] hits."""
        per = max(int(max_hsps), 1)                     # (a refused max_hsps still needs buffers to hand over)
        slots = max(len(row_lens) * k, 1)
        out = (Alignment * (slots * per))()
        nout = (C.c_uint32 * slots)()
        cnt = (AlignCounts * (slots * per))() if want_counts else None
        ops = C.create_string_buffer(max(1, slots * per * stride)) if want_ops else None
        _check(call(int(max_hsps), int(min_score), C.cast(out, _vp), C.cast(nout, _vp), C.cast(cnt, _vp) if want_counts else None,
                    C.cast(ops, _vp) if want_ops else None, stride), self.handle)
        raw = ops.raw if want_ops else None
        res = []
        for i, nrow in enumerate(row_lens):
            row = []
            for j in range(nrow):
                s = i * k + j
                als = []
                for r in range(int(nout[s])):
                    e = s * per + r
                    a = self._stats_dict(out[e], cnt[e]) if want_counts else \
                        {f: int(getattr(out[e], f)) for f, _ in Alignment._fields_ if f != "reserved"}
                    if want_ops:
                        a["ops"] = raw[e * stride:e * stride + a["n_ops"]].decode()
                    als.append(a)
                row.append(als)
            res.append(row)
        return res

    @staticmethod
    def _stats_dict(al, cnt):
        a = {f: int(getattr(al, f)) for f, _ in Alignment._fields_ if f != "reserved"}
        a.update((f, int(getattr(cnt, f))) for f, _ in AlignCounts._fields_)
        return a

    def prune_last(self):
        """What the search last ended on this context left out (swg_prune_last) -> dict: pruned (bool), threshold (the
        last T), pairs_skipped, pair_rows_skipped and pair_rows (rows in whole 4-row token blocks)."""

        class _Info(C.Structure):
            _fields_ = [("pairs_skipped", C.c_uint64), ("pair_rows_skipped", C.c_uint64), ("pair_rows", C.c_uint64),
                        ("threshold", C.c_uint32), ("pruned", C.c_int32)]

        i = _Info()
        _check(lib.swg_prune_last(self.handle, C.cast(C.byref(i), _vp)), self.handle)
        return {"pruned": bool(i.pruned), "threshold": int(i.threshold), "pairs_skipped": int(i.pairs_skipped),
                "pair_rows_skipped": int(i.pair_rows_skipped), "pair_rows": int(i.pair_rows)}

    def debug_prune_kmer_read(self, db, k=None, bounds=False):
        """Test hook: what the k-mer bound left on the device, once everything queued has run -> dict: k (what the search
        last begun cut by; 0: not pruned), builds (table builds of this context so far), pairs (of db), table (the
        context's table of `k`, uint16[22^k], when k is given) and bounds (uint32 per pair of the search last begun on db,
        when asked for)."""
        info = np.zeros(3, dtype=np.uint64)
        t = np.zeros(KMER_CLASSES ** int(k), dtype=np.uint16) if k else None
        n = 0
        if bounds:  # (a first call for the number of pairs)
            _check(lib.swg_debug_prune_kmer_read(self.handle, db.handle, 0, None, None, 0, info.ctypes.data_as(_vp)), self.handle)
            n = int(info[2])
        b = np.zeros(max(n, 1), dtype=np.uint32) if bounds else None
        _check(lib.swg_debug_prune_kmer_read(self.handle, db.handle, int(k or 0), t.ctypes.data_as(_vp) if t is not None else None,
                                             b.ctypes.data_as(_vp) if b is not None else None, n, info.ctypes.data_as(_vp)), self.handle)
        return {"k": int(info[0]), "builds": int(info[1]), "pairs": int(info[2]), "table": t, "bounds": None if b is None else b[:int(info[2])]}

    def debug_prune_kmer_seg_read(self, db, k=None, segments=1, bounds=False):
        """Test hook: debug_prune_kmer_read for a table of `segments` segments -> the same dict, table uint16[22^k,
        segments], plus segments (what the search last begun cut by)."""
        info = np.zeros(4, dtype=np.uint64)
        S = int(segments)
        t = np.zeros((KMER_CLASSES ** int(k), S), dtype=np.uint16) if k else None
        n = 0
        if bounds:  # (a first call for the number of pairs)
            _check(lib.swg_debug_prune_kmer_seg_read(self.handle, db.handle, 0, 0, None, None, 0, info.ctypes.data_as(_vp)), self.handle)
            n = int(info[2])
        b = np.zeros(max(n, 1), dtype=np.uint32) if bounds else None
        _check(lib.swg_debug_prune_kmer_seg_read(self.handle, db.handle, int(k or 0), S, t.ctypes.data_as(_vp) if t is not None else None,
                                                 b.ctypes.data_as(_vp) if b is not None else None, n, info.ctypes.data_as(_vp)), self.handle)
        return {"k": int(info[0]), "builds": int(info[1]), "pairs": int(info[2]), "segments": int(info[3]), "table": t,
                "bounds": None if b is None else b[:int(info[2])]}

    def debug_prune_refine_read(self, db, segments=None, arrays=True):
        """Test hook: the second level and the lists of the search last begun -> dict: k, segments, refine (its S2, 0:
        none), builds / refine_builds (table builds queued so far, first / second level), table uint16[22^4, segments]
        (only when `segments` is given: 64 | 128 the second level's, 256 the third's; widened where the device keeps
        bytes), bounds uint32[pairs] as the search left them, stages: a list of (begin, end, T,
        list) per stage cut pair by pair, list being the pair ids its launches took.  arrays = False: the counters only
        (before the database's first pruned search there are no bounds to read)."""
        info = np.zeros(7, dtype=np.uint64)
        _check(lib.swg_debug_prune_refine_read(self.handle, db.handle, 0, None, None, None, 0, None, 0, info.ctypes.data_as(_vp)), self.handle)
        n = int(info[2])
        if not arrays:
            return {"k": int(info[0]), "builds": int(info[1]), "pairs": n, "segments": int(info[3]), "refine": int(info[4]),
                    "refine_builds": int(info[5]), "table": None, "bounds": None, "stages": []}
        S = int(segments or 0)
        t = np.zeros((KMER_CLASSES ** 4, S), dtype=np.uint16) if S else None
        b = np.zeros(max(n, 1), dtype=np.uint32)
        l = np.zeros(max(n, 1), dtype=np.uint32)
        st = np.zeros((256, 4), dtype=np.uint32)
        _check(lib.swg_debug_prune_refine_read(self.handle, db.handle, S, t.ctypes.data_as(_vp) if t is not None else None, b.ctypes.data_as(_vp),
                                               l.ctypes.data_as(_vp), n, st.ctypes.data_as(_vp), 256, info.ctypes.data_as(_vp)), self.handle)
        stages = [(int(r[0]), int(r[1]), int(r[2]), l[int(r[0]):int(r[0]) + int(r[3])].copy()) for r in st[:int(info[6])]]
        return {"k": int(info[0]), "builds": int(info[1]), "pairs": n, "segments": int(info[3]), "refine": int(info[4]),
                "refine_builds": int(info[5]), "table": t, "bounds": b[:n], "stages": stages}

    def debug_prune_tables(self):
        """Test hook: the third level and the k-mer tables' entry widths (swg_debug_prune_tables) -> dict: refine3 (S3 of
        the search last begun, 0: none), refine3_builds, bits: the entry bits of the tables that hold the current query
        and scoring (0: none) -- first4, first5, second, third --, auto_bits (what prune_table_bits = 0 gives at k = 4)."""
        out = np.zeros(7, dtype=np.int64)
        _check(lib.swg_debug_prune_tables(self.handle, out.ctypes.data_as(_vp)), self.handle)
        return {"refine3": int(out[0]), "refine3_builds": int(out[1]),
                "bits": dict(zip(("first4", "first5", "second", "third"), (int(v) for v in out[2:6]))), "auto_bits": int(out[6])}

    def debug_prune_tables4(self):
        """Test hook: the fourth level (swg_debug_prune_tables4) -> dict: refine4 (S4 of the search last begun, 0: none),
        refine4_builds, bits (of the fourth table if it holds the current query and scoring, else 0), refused (its
        allocation failed once on this context)."""
        out = np.zeros(4, dtype=np.int64)
        _check(lib.swg_debug_prune_tables4(self.handle, out.ctypes.data_as(_vp)), self.handle)
        return {"refine4": int(out[0]), "refine4_builds": int(out[1]), "bits": int(out[2]), "refused": bool(out[3])}

    def debug_prune_tables5(self):
        """Test hook: the fifth level (swg_debug_prune_tables5) -> dict: refine5 (S5 of the search last begun, 0: none),
        refine5_builds (of its second table), bits (of that table if it holds the current query and scoring, else 0),
        refused (its allocation failed once on this context)."""
        out = np.zeros(4, dtype=np.int64)
        _check(lib.swg_debug_prune_tables5(self.handle, out.ctypes.data_as(_vp)), self.handle)
        return {"refine5": int(out[0]), "refine5_builds": int(out[1]), "bits": int(out[2]), "refused": bool(out[3])}

    def debug_prune_refine5_read(self, blocks):
        """Test hook: rows of the fifth level's second table -> uint16[len(blocks), 256] (as debug_prune_refine4_read)."""
        b = np.ascontiguousarray(blocks, dtype=np.uint32)
        out = np.zeros((max(b.size, 1), KMER_REFINE4_SEGMENTS), dtype=np.uint16)
        _check(lib.swg_debug_prune_refine5_read(self.handle, b.ctypes.data_as(_vp), b.size, out.ctypes.data_as(_vp)), self.handle)
        return out[:b.size]

    def debug_prune_gate(self):
        """Test hook: whether the search last begun took the gate in front of the first level (option prune_gate)."""
        out = np.zeros(1, dtype=np.int64)
        _check(lib.swg_debug_prune_gate(self.handle, out.ctypes.data_as(_vp)), self.handle)
        return bool(out[0])

    def debug_prune_refine4_read(self, blocks):
        """Test hook: rows of the fourth level's table -> uint16[len(blocks), 256]: the entries of the class blocks
        `blocks` (indices below 22^5, first class most significant)."""
        b = np.ascontiguousarray(blocks, dtype=np.uint32)
        out = np.zeros((max(b.size, 1), KMER_REFINE4_SEGMENTS), dtype=np.uint16)
        _check(lib.swg_debug_prune_refine4_read(self.handle, b.ctypes.data_as(_vp), b.size, out.ctypes.data_as(_vp)), self.handle)
        return out[:b.size]

    def debug_bounds_last(self):
        """What the last align_bounds* call of this context did (swg_debug_bounds_last) -> dict: pairs on the bounds kernel,
        pairs on the fallback (the traceback's kernel), launches of the bounds kernel, its column limit."""
        out = np.zeros(4, dtype=np.uint32)
        _check(lib.swg_debug_bounds_last(self.handle, out.ctypes.data_as(_vp)), self.handle)
        return dict(zip(("kernel_pairs", "fallback_pairs", "launches", "column_limit"), (int(v) for v in out)))

    def _align_multi(self, fn, db, qflat, qoff, hits, want_ops, ops_stride, bounds=False, stats=False):
        nq = len(qoff) - 1
        if len(hits) != nq:
            raise ValueError("hits: %d rows for %d queries" % (len(hits), nq))
        k = max((len(row) for row in hits), default=0)
        arr = (Hit * max(nq * k, 1))()
        nh = (C.c_size_t * max(nq, 1))()
        for i, row in enumerate(hits):
            nh[i] = len(row)
            for j, (sc, ix) in enumerate(row):
                arr[i * k + j].score, arr[i * k + j].index = int(sc), int(ix)
        out = (Alignment * max(nq * k, 1))()
        stride = 0 if bounds else int(ops_stride if ops_stride is not None else
                                      lib.swg_align_ops_bound_multi(db.handle, qoff.ctypes.data_as(_vp), nq))
        ops = C.create_string_buffer(max(1, nq * k * stride)) if want_ops else None
        args = (self.handle, db.handle, qflat.ctypes.data_as(_vp), qoff.ctypes.data_as(_vp), nq, C.cast(arr, _vp), k,
                C.cast(nh, _vp), C.cast(out, _vp))
        if stats:
            cnt = (AlignCounts * max(nq * k, 1))()
            _check(fn(*args, C.cast(cnt, _vp)), self.handle)
            return [[self._stats_dict(out[i * k + j], cnt[i * k + j]) for j in range(len(row))] for i, row in enumerate(hits)]
        _check(fn(*args) if bounds else fn(*args, C.cast(ops, _vp) if want_ops else None, stride), self.handle)
        raw = ops.raw if want_ops else None          # (one copy: .raw copies the whole buffer on every access)
        res = []
        for i, row in enumerate(hits):
            r = []
            for j in range(len(row)):
                h = i * k + j
                a = {f: int(getattr(out[h], f)) for f, _ in Alignment._fields_ if f != "reserved"}
                if want_ops:
                    a["ops"] = raw[h * stride:h * stride + a["n_ops"]].decode()
                r.append(a)
            res.append(r)
        return res

    @staticmethod
    def _hit_keys(hits, k, n):
        a = np.frombuffer(hits, dtype=np.dtype([("score", "<i4"), ("index", "<u4")]), count=max(k, 1))[:k]
        keys = (a["score"].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - a["index"].astype(np.uint64))
        keys[n:] = 0
        return keys

    def search_keys(self, db, k):
        """Top-K of this shard as uint64 sort keys (score << 32 | ~index), zero-padded to k, plus
        stats: the form the multi-GPU merge exchanges (no per-hit Python objects)."""
        hits = (Hit * max(k, 1))()
        nh = C.c_size_t(0)
        st = Stats()
        _check(lib.swg_search(self.handle, db.handle, None, C.cast(hits, _vp), k, C.byref(nh), C.byref(st)),
               self.handle)
        a = np.frombuffer(hits, dtype=np.dtype([("score", "<i4"), ("index", "<u4")]), count=max(k, 1))[:k]
        keys = (a["score"].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - a["index"].astype(np.uint64))
        keys[nh.value:] = 0
        return keys, st.as_dict()

    def fill_batches16(self, batches):
        """batches: list of (db_idx_t int8[max_len,16], vector_size) -> list of int16[vector_size]."""
        arr = (Batch16 * len(batches))()
        keep, outs = [], []
        for i, (d, vs) in enumerate(batches):
            d = np.ascontiguousarray(d, dtype=np.int8)
            o = np.zeros(16, dtype=np.int16)
            keep.append(d)
            outs.append(o)
            arr[i].db_idx_t = d.ctypes.data
            arr[i].max_len = d.shape[0]
            arr[i].vector_size = vs
            arr[i].max_scores = o.ctypes.data
        secs = C.c_double(0)
        _check(lib.swg_fill_batches16(self.handle, arr, len(batches), C.byref(secs)), self.handle)
        return [o[:vs].copy() for o, (_, vs) in zip(outs, batches)], secs.value

    def close(self):
        if self.handle:
            lib.swg_destroy(self.handle)
            self.handle = None

    __del__ = close


class Group:
    """swg_group: several GPUs in one process, shards merged with one RCCL all-reduce."""

    def __init__(self, devices, force_collective=False):
        self.handle = None
        devs = (C.c_int * len(devices))(*devices)
        h = _vp()
        _check(lib.swg_group_create(C.cast(devs, _vp), len(devices), 1 if force_collective else 0, C.byref(h)))
        self.handle = h
        self.n = len(devices)
        self.total = 0

    def _chk(self, rc):
        if rc != SWG_OK:
            raise SwgError(rc, (lib.swg_group_last_error(self.handle) or b"").decode("utf-8", "replace"))

    def set_option(self, key, value):
        self._chk(lib.swg_group_set_option(self.handle, key.encode(), int(value)))

    def set_scoring(self, sub, gap_open, gap_extend):
        if isinstance(sub, Scoring):
            sub = sub.table()
        s, sp = _i8(np.asarray(sub).reshape(32, 32))
        self._chk(lib.swg_group_set_scoring(self.handle, sp, int(gap_open), int(gap_extend)))

    def set_query(self, idx):
        q, qp = _i8(idx)
        self._chk(lib.swg_group_set_query(self.handle, qp, q.size))

    def set_query_pssm(self, pssm):
        p, pp, lq = _pssm(pssm)
        self._chk(lib.swg_group_set_query_pssm(self.handle, pp, lq))

    def load(self, flat, offsets):
        f, fp = _i8(flat)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._chk(lib.swg_group_load(self.handle, fp, o.ctypes.data_as(_vp), o.size - 1))
        self.total = o.size - 1

    def search(self, want_scores=True, k=0):
        scores = np.zeros(self.total, dtype=np.int32) if want_scores else None
        hits = (Hit * max(k, 1))()
        nh = C.c_size_t(0)
        st = (Stats * self.n)()
        self._chk(lib.swg_group_search(self.handle, scores.ctypes.data_as(_vp) if want_scores else None,
                                       C.cast(hits, _vp) if k else None, k, C.byref(nh), st))
        return scores, [(int(hits[i].score), int(hits[i].index)) for i in range(nh.value)], [s.as_dict() for s in st]

    def select(self, indices):
        """Restrict search / align_hits to the listed original indices (every device takes a view of its shard);
        None returns to the whole database."""
        if indices is None:
            self._chk(lib.swg_group_select(self.handle, None, 0))
            return
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        keep = ix if ix.size else np.zeros(1, dtype=np.uint32)   # (an empty list is a list: never a NULL pointer)
        self._chk(lib.swg_group_select(self.handle, keep.ctypes.data_as(_vp), ix.size))

    def align_hits(self, hits):
        """Alignments of hits of a group search (see Context.align_hits)."""
        n = len(hits)
        arr = (Hit * max(n, 1))()
        for i, (sc, ix) in enumerate(hits):
            arr[i].score, arr[i].index = int(sc), int(ix)
        out = (Alignment * max(n, 1))()
        stride = int(lib.swg_group_align_ops_bound(self.handle))
        ops = C.create_string_buffer(max(1, n * stride))
        self._chk(lib.swg_group_align_hits(self.handle, C.cast(arr, _vp), n, C.cast(out, _vp), C.cast(ops, _vp), stride))
        res = []
        for i in range(n):
            a = {f: int(getattr(out[i], f)) for f, _ in Alignment._fields_ if f != "reserved"}
            a["ops"] = ops.raw[i * stride:i * stride + a["n_ops"]].decode()
            res.append(a)
        return res

    def close(self):
        if self.handle:
            lib.swg_group_destroy(self.handle)
            self.handle = None

    __del__ = close
