"""ctypes binding of the C-ABI in include/msv.h (libmsv_hip.so, built in-tree).

There is no fallback: if the shared library is missing the import of the device path fails
loudly with a message saying how to build it.
"""
from __future__ import annotations

import ctypes as C
import os

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
# MSV_LIB_PATH: another build of the same library (tools/ab.py compares two builds in one process
# run); unset in every test and product run.
LIB_PATH = os.environ.get("MSV_LIB_PATH") or os.path.join(LIB_DIR, "libmsv_hip.so")

STATUS = {
    0: "MSV_OK",
    1: "MSV_ERR_INVALID_ARGUMENT",
    2: "MSV_ERR_IO",
    3: "MSV_ERR_PARSE",
    4: "MSV_ERR_BAD_RESIDUE",
    5: "MSV_ERR_SEQUENCE_TOO_LONG",
    6: "MSV_ERR_UNSUPPORTED_MODEL",
    7: "MSV_ERR_NO_DEVICE",
    8: "MSV_ERR_HIP",
    9: "MSV_ERR_OUT_OF_MEMORY",
    10: "MSV_ERR_RCCL",
    11: "MSV_ERR_NO_CONVERGENCE",
}
MSV_OK = 0
MSV_ERR_BAD_RESIDUE = 4

# Every symbol include/msv.h declares (checked by tests/test_capi.py).
EXPORTED = [
    "msv_status_string", "msv_version", "msv_device_count",
    "msv_hmm_read", "msv_hmm_destroy", "msv_hmm_model_length", "msv_hmm_name", "msv_hmm_stats",
    "msv_hmm_match_emissions", "msv_hmm_insert_emissions", "msv_hmm_transitions", "msv_hmm_msv_scores",
    "msv_sequence_transitions",
    "msv_fasta_read", "msv_fasta_destroy", "msv_fasta_count", "msv_fasta_rejected", "msv_fasta_codes",
    "msv_fasta_offsets", "msv_fasta_header", "msv_encode_residues",
    "msv_profile_create", "msv_profile_create_from_hmm", "msv_profile_destroy", "msv_profile_describe",
    "msv_profile_reserve_length", "msv_score_batch", "msv_score_batch_device", "msv_profile_check",
    "msv_order_longest_first", "msv_variant_count", "msv_variant_name", "msv_profile_set_variant",
    "msv_score_grid", "msv_score_grid_device", "msv_pvalues", "msv_pvalues_device",
    "msv_shard_bounds", "msv_lazy_bound_table", "msv_score_batch_multi",
    "msv_fasta_parse_device", "msv_fasta_read_device", "msv_fasta_device_destroy", "msv_fasta_device_count",
    "msv_fasta_device_rejected", "msv_fasta_device_residues", "msv_fasta_device_codes", "msv_fasta_device_offsets",
    "msv_fasta_device_header_spans", "msv_fasta_device_text", "msv_fasta_device_download",
    "msv_fasta_device_max_length", "msv_score_fasta_device", "msv_fasta_device_device",
    "msv_score_batch_async", "msv_profile_wait", "msv_profile_bind_stream",
    "msv_multi_create", "msv_multi_score_batch", "msv_multi_destroy",
    "msv_host_alloc", "msv_host_free", "msv_profile_variant_for",
    "msv_filter_select_device", "msv_hmm_viterbi_scores", "msv_vit_cpu_score", "msv_vit_profile_create",
    "msv_vit_profile_create_from_hmm", "msv_vit_profile_destroy", "msv_vit_profile_reserve_length",
    "msv_vit_profile_describe", "msv_vit_variant_count", "msv_vit_variant_name", "msv_vit_profile_set_variant",
    "msv_vit_score_batch_device", "msv_vit_score_batch", "msv_vit_profile_check", "msv_vit_filter_batch",
    "msv_vit_profile_bind_stream",
    "msv_vit_cpu_trace", "msv_vit_trace_plan_count", "msv_vit_trace_plan_name", "msv_vit_trace_plan_capacity",
    "msv_vit_trace_plan_cell", "msv_vit_trace_sequence_bytes", "msv_vit_trace_chunk_cuts", "msv_vit_trace_batch",
    "msv_vit_traces_count", "msv_vit_traces_domains", "msv_vit_traces_ops", "msv_vit_traces_copy",
    "msv_vit_traces_free", "msv_vit_trace_describe", "msv_vit_traces_stats",
    "msv_fwd_cpu_score", "msv_fwd_cpu_score_batch", "msv_fwd_pvalues", "msv_fwd_scan_constants",
    "msv_fwd_profile_create", "msv_fwd_profile_create_from_hmm", "msv_fwd_profile_destroy",
    "msv_fwd_profile_reserve_length", "msv_fwd_profile_describe", "msv_fwd_variant_count", "msv_fwd_variant_name",
    "msv_fwd_profile_set_variant", "msv_fwd_score_batch_device", "msv_fwd_profile_bind_stream",
    "msv_fwd_score_batch", "msv_fwd_profile_check", "msv_fwd_pvalues_device", "msv_fwd_filter_batch",
    "msv_dom_cpu_decode", "msv_dom_cpu_decode_batch", "msv_dom_regions", "msv_dom_scan_constants",
    "msv_dom_sequence_bytes", "msv_dom_profile_create", "msv_dom_profile_create_from_hmm", "msv_dom_profile_destroy",
    "msv_dom_profile_reserve_length", "msv_dom_profile_describe", "msv_dom_variant_count", "msv_dom_variant_name",
    "msv_dom_profile_set_variant", "msv_dom_profile_bind_stream", "msv_dom_profile_check",
    "msv_dom_score_batch_device", "msv_dom_score_batch", "msv_dom_decode_batch_device", "msv_dom_decode_batch",
    "msv_dom_result_count", "msv_dom_result_residues", "msv_dom_result_regions", "msv_dom_result_copy",
    "msv_dom_result_free", "msv_dom_result_stats",
    "msv_aln_cpu_decode", "msv_aln_oa", "msv_aln_cpu_align", "msv_aln_item_bytes", "msv_aln_align_batch",
    "msv_aln_result_count", "msv_aln_result_domains", "msv_aln_result_ops", "msv_aln_result_copy",
    "msv_aln_result_posteriors", "msv_aln_result_free", "msv_aln_describe", "msv_aln_result_stats",
    "msv_aln_cpu_null2", "msv_aln_null2_correction", "msv_aln_bias_scores", "msv_aln_align_batch_opts",
    "msv_aln_result_null2", "msv_aln_result_null2_stats",
    "msv_hmm_compo", "msv_background_frequencies",
    "msv_bf_cpu_score", "msv_bf_cpu_score_batch", "msv_bf_pvalues", "msv_bf_device_table", "msv_bf_profile_create",
    "msv_bf_profile_create_from_hmm", "msv_bf_profile_destroy", "msv_bf_profile_describe", "msv_bf_score_batch",
    "msv_bf_score_batch_device", "msv_bf_profile_bind_stream", "msv_bf_profile_check", "msv_bf_filter_select_device",
    "msv_bf_pvalues_device", "msv_fwd_filter_batch_opts",
    "msv_dom_is_multidomain", "msv_spl_cpu_forward", "msv_spl_sample", "msv_spl_cluster", "msv_spl_item_bytes",
    "msv_spl_sample_batch", "msv_spl_result_count", "msv_spl_result_segments", "msv_spl_result_copy",
    "msv_spl_result_matrix", "msv_spl_result_stats", "msv_spl_result_free", "msv_spl_describe",
    "msv_cal_lambda", "msv_cal_thresholds", "msv_cal_codes_of_draws", "msv_cal_generate", "msv_cal_fit_location",
    "msv_cal_fit_gumbel", "msv_cal_tau", "msv_cal_cpu_calibrate", "msv_cal_workspace_bytes",
    "msv_cal_generate_device", "msv_cal_fit_device", "msv_cal_calibrate",
    "msv_emit_tables", "msv_emit_generate", "msv_emit_result_count", "msv_emit_result_residues",
    "msv_emit_result_domains", "msv_emit_result_ops", "msv_emit_result_chunks", "msv_emit_result_copy",
    "msv_emit_result_free", "msv_emit_path_score", "msv_emit_workspace_bytes", "msv_emit_profile_create",
    "msv_emit_profile_destroy", "msv_emit_profile_bind_stream", "msv_emit_batch_device", "msv_emit_batch",
    "msv_emit_describe", "msv_emit_profile_times",
]
CAL_FIT_LOCATION, CAL_FIT_GUMBEL, CAL_FIT_TAU = 0, 1, 2  # msv.h msv_cal_fit_mode
BF_GUMBEL, BF_EXPONENTIAL = 0, 1  # msv.h MSV_BF_*: the tail of a filtered P-value


class MSVError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        self.name = STATUS.get(status, f"MSV_ERR_{status}")
        super().__init__(f"{what}: {self.name}" if what else self.name)


class KernelInfo(C.Structure):
    _fields_ = [
        ("model_length", C.c_uint32),
        ("lanes_per_group", C.c_uint32),
        ("states_per_lane", C.c_uint32),
        ("waves_per_block", C.c_uint32),
        ("lds_rows", C.c_uint32),
        ("lds_bytes", C.c_uint32),
        ("blocks", C.c_uint32),
        ("max_length", C.c_uint32),
        ("device", C.c_int),
        ("variant", C.c_char * 64),
        ("latency_variant", C.c_char * 64),
        ("latency_blocks", C.c_uint32),
        ("latency_max_n", C.c_uint64),
        ("mid_variant", C.c_char * 64),
        ("mid_blocks", C.c_uint32),
        ("mid_max_n", C.c_uint64),
        ("coop_variant", C.c_char * 64),
        ("coop_blocks", C.c_uint32),
        ("coop_max_n", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["variant"] = self.variant.decode()
        d["latency_variant"] = self.latency_variant.decode()
        d["mid_variant"] = self.mid_variant.decode()
        d["coop_variant"] = self.coop_variant.decode()
        return d


class VitInfo(C.Structure):
    _fields_ = [
        ("model_length", C.c_uint32),
        ("states_per_lane", C.c_uint32),
        ("transitions_in_registers", C.c_uint32),
        ("match_in_lds", C.c_uint32),
        ("insert_scores", C.c_uint32),
        ("waves_per_block", C.c_uint32),
        ("blocks", C.c_uint32),
        ("lds_bytes", C.c_uint32),
        ("max_length", C.c_uint32),
        ("device", C.c_int),
        ("variant", C.c_char * 64),
        ("scratch_bytes", C.c_uint32),
        ("waves_per_sequence", C.c_uint32),
    ]

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["variant"] = self.variant.decode()
        return d


class FwdInfo(C.Structure):
    _fields_ = [
        ("model_length", C.c_uint32),
        ("states_per_lane", C.c_uint32),
        ("match_in_lds", C.c_uint32),
        ("insert_scores", C.c_uint32),
        ("waves_per_block", C.c_uint32),
        ("blocks", C.c_uint32),
        ("lds_bytes", C.c_uint32),
        ("scratch_bytes", C.c_uint32),
        ("max_length", C.c_uint32),
        ("device", C.c_int),
        ("variant", C.c_char * 64),
    ]

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["variant"] = self.variant.decode()
        return d


class DomInfo(C.Structure):
    """msv_dom_info: append-only, struct_size first (set before the call)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("model_length", C.c_uint32),
        ("states_per_lane", C.c_uint32),
        ("match_in_lds", C.c_uint32),
        ("insert_scores", C.c_uint32),
        ("waves_per_block", C.c_uint32),
        ("blocks", C.c_uint32),
        ("backward_blocks", C.c_uint32),
        ("lds_bytes", C.c_uint32),
        ("backward_lds_bytes", C.c_uint32),
        ("scratch_bytes", C.c_uint32),
        ("max_length", C.c_uint32),
        ("device", C.c_int),
        ("variant", C.c_char * 64),
    ]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(DomInfo)

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_ if f != "struct_size"}
        d["variant"] = self.variant.decode()
        return d


class DomStats(C.Structure):
    _fields_ = [("chunks", C.c_uint64), ("record_bytes", C.c_uint64), ("forward_ms", C.c_float),
                ("backward_ms", C.c_float), ("regions_ms", C.c_float), ("reserved", C.c_uint32)]


class AlnInfo(C.Structure):
    """msv_aln_info: append-only, struct_size first (set before the call)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("states_per_lane", C.c_uint32),
        ("pointer_words", C.c_uint32),
        ("forward_blocks", C.c_uint32),
        ("backward_blocks", C.c_uint32),
        ("fill_blocks", C.c_uint32),
        ("forward_scratch_bytes", C.c_uint32),
        ("backward_scratch_bytes", C.c_uint32),
        ("fill_scratch_bytes", C.c_uint32),
        ("walk_scratch_bytes", C.c_uint32),
        ("forward_lds_bytes", C.c_uint32),
        ("backward_lds_bytes", C.c_uint32),
        ("fill_lds_bytes", C.c_uint32),
        ("walk_lds_bytes", C.c_uint32),
        ("default_workspace_bytes", C.c_uint64),
        ("variant", C.c_char * 64),
        ("null2_row_block", C.c_uint32),
        ("null2_partial_scratch_bytes", C.c_uint32),
        ("null2_finish_scratch_bytes", C.c_uint32),
        ("null2_partial_lds_bytes", C.c_uint32),
        ("null2_finish_lds_bytes", C.c_uint32),
        ("reserved", C.c_uint32),
    ]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(AlnInfo)

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_ if f != "struct_size"}
        d["variant"] = self.variant.decode()
        return d


class AlnStats(C.Structure):
    _fields_ = [("chunks", C.c_uint64), ("matrix_bytes", C.c_uint64), ("forward_ms", C.c_float),
                ("backward_ms", C.c_float), ("fill_ms", C.c_float), ("walk_ms", C.c_float)]


class AlnOptions(C.Structure):
    """msv_aln_options: append-only, struct_size first (set on construction)."""
    _fields_ = [("struct_size", C.c_uint64), ("workspace_bytes", C.c_uint64), ("keep_posteriors", C.c_int32),
                ("null2", C.c_int32)]

    def __init__(self, workspace_bytes=0, keep_posteriors=0, null2=0):
        super().__init__(C.sizeof(AlnOptions), workspace_bytes, keep_posteriors, null2)


class AlnNull2Stats(C.Structure):
    """msv_aln_null2_stats: append-only, struct_size first (set before the call)."""
    _fields_ = [("struct_size", C.c_uint32), ("row_block", C.c_uint32), ("null2_ms", C.c_float),
                ("partial_ms", C.c_float), ("slab_bytes", C.c_uint64)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(AlnNull2Stats)


class SplOptions(C.Structure):
    """msv_spl_options: append-only, struct_size first (set on construction)."""
    _fields_ = [("struct_size", C.c_uint64), ("workspace_bytes", C.c_uint64), ("seed", C.c_uint64),
                ("n_samples", C.c_uint32), ("seed_set", C.c_int32), ("keep_matrix", C.c_int32),
                ("reserved", C.c_int32), ("stream", C.c_void_p)]

    def __init__(self, workspace_bytes=0, seed=42, n_samples=200, keep_matrix=0, stream=None):
        super().__init__(C.sizeof(SplOptions), workspace_bytes, seed, n_samples, 1, keep_matrix, 0, stream)


class SplClusterOptions(C.Structure):
    """msv_spl_cluster_options: append-only, struct_size first; fractions as integer ratios."""
    _fields_ = [("struct_size", C.c_uint64), ("min_overlap_num", C.c_uint32), ("min_overlap_den", C.c_uint32),
                ("max_diagdiff", C.c_uint32), ("min_posterior_num", C.c_uint32), ("min_posterior_den", C.c_uint32),
                ("min_endpointp_num", C.c_uint32), ("min_endpointp_den", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(SplClusterOptions)


class SplStats(C.Structure):
    """msv_spl_stats: append-only, struct_size first (set before the call)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_samples", C.c_uint32), ("seed", C.c_uint64),
                ("chunks", C.c_uint64), ("matrix_bytes", C.c_uint64), ("truncated", C.c_uint64),
                ("forward_ms", C.c_float), ("sample_ms", C.c_float)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(SplStats)


class SplInfo(C.Structure):
    """msv_spl_info: append-only, struct_size first (set before the call)."""
    _fields_ = [("struct_size", C.c_uint32), ("states_per_lane", C.c_uint32), ("forward_blocks", C.c_uint32),
                ("forward_scratch_bytes", C.c_uint32), ("sample_scratch_bytes", C.c_uint32),
                ("forward_lds_bytes", C.c_uint32), ("sample_lds_bytes", C.c_uint32), ("reserved", C.c_uint32),
                ("default_workspace_bytes", C.c_uint64), ("variant", C.c_char * 64)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(SplInfo)

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_ if f not in ("struct_size", "reserved")}
        d["variant"] = self.variant.decode()
        return d


class CalOptions(C.Structure):
    """msv_cal_options: append-only, struct_size first (set on construction); index = sample set."""
    _fields_ = [("struct_size", C.c_uint64), ("n", C.c_uint64 * 3), ("length", C.c_uint64 * 3), ("tail", C.c_double),
                ("seed", C.c_uint64), ("seed_set", C.c_int32), ("insert_mode", C.c_int32),
                ("workspace_bytes", C.c_uint64), ("scores", C.c_void_p * 3)]

    def __init__(self, n=(0, 0, 0), length=(0, 0, 0), tail=0.0, seed=42, insert_mode=0, workspace_bytes=0):
        super().__init__(C.sizeof(CalOptions), (C.c_uint64 * 3)(*n), (C.c_uint64 * 3)(*length), tail,
                         seed & (2 ** 64 - 1), 1, insert_mode, workspace_bytes)


class CalReport(C.Structure):
    """msv_cal_report: append-only, struct_size first (set before the call)."""
    _fields_ = [("struct_size", C.c_uint32), ("ran", C.c_uint32), ("lambda_", C.c_double),
                ("location", C.c_double * 3), ("gmu", C.c_double), ("glam", C.c_double),
                ("iterations", C.c_uint32), ("reserved", C.c_uint32), ("chunks", C.c_uint64 * 3),
                ("n", C.c_uint64 * 3), ("length", C.c_uint64 * 3), ("seed", C.c_uint64), ("tail", C.c_double)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(CalReport)

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_ if f not in ("struct_size", "reserved")}
        for f in ("location", "chunks", "n", "length"):
            d[f] = list(d[f])
        return d


class EmitOptions(C.Structure):
    """msv_emit_options: append-only, struct_size first (set on construction)."""
    _fields_ = [("struct_size", C.c_uint64), ("length", C.c_uint64), ("max_length", C.c_uint64),
                ("length_set", C.c_int32), ("unihit", C.c_int32), ("insert_mode", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, length=400, multihit=True, insert_mode=0, max_length=None):
        super().__init__(C.sizeof(EmitOptions), int(length), int(max_length or 0), 1, 0 if multihit else 1,
                         insert_mode, 0)


class EmitTotals(C.Structure):
    """msv_emit_totals: the record the scan launch writes."""
    _fields_ = [("residues", C.c_uint64), ("domains", C.c_uint64), ("ops", C.c_uint64), ("truncated", C.c_uint64),
                ("overflow", C.c_uint64)]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


class EmitTruth(C.Structure):
    """msv_emit_truth: the truth buffers of a device call (device pointers, capacities in elements)."""
    _fields_ = [("d_domain_offsets", C.c_void_p), ("d_domains", C.c_void_p), ("domains_capacity", C.c_uint64),
                ("d_ops", C.c_void_p), ("ops_capacity", C.c_uint64), ("d_truncated", C.c_void_p)]


class EmitInfo(C.Structure):
    """msv_emit_info: append-only, struct_size first (set before the call)."""
    _fields_ = [("struct_size", C.c_uint32), ("model_length", C.c_uint32), ("block", C.c_uint32),
                ("scan_block", C.c_uint32), ("count_vgprs", C.c_uint32), ("place_vgprs", C.c_uint32),
                ("scan_vgprs", C.c_uint32), ("count_scratch_bytes", C.c_uint32), ("place_scratch_bytes", C.c_uint32),
                ("scan_scratch_bytes", C.c_uint32), ("count_lds_bytes", C.c_uint32), ("place_lds_bytes", C.c_uint32),
                ("scan_lds_bytes", C.c_uint32), ("device", C.c_int), ("table_bytes", C.c_uint64),
                ("length", C.c_uint64), ("max_length", C.c_uint64), ("unihit", C.c_int32), ("insert_mode", C.c_int32),
                ("default_workspace_bytes", C.c_uint64)]

    def __init__(self):
        super().__init__()
        self.struct_size = C.sizeof(EmitInfo)

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "struct_size"}


# msv_cal_fit, the fit kernel's record, as a numpy structured dtype (40 bytes)
CAL_FIT_DTYPE = [("mu", "<f8"), ("lambda_", "<f8"), ("gmu", "<f8"), ("glam", "<f8"), ("iterations", "<u4"),
                 ("status", "<u4")]

# msv_spl_segment and msv_spl_envelope as numpy structured dtypes
SEGMENT_DTYPE = [("i_from", "<u4"), ("i_to", "<u4"), ("k_from", "<u4"), ("k_to", "<u4")]
SPLIT_ENVELOPE_DTYPE = [("i_from", "<u4"), ("i_to", "<u4"), ("k_from", "<u4"), ("k_to", "<u4"), ("count", "<u4"),
                        ("prob", "<f4")]

# msv_aln_item as a numpy structured dtype
ITEM_DTYPE = [("seq", "<u4"), ("i_from", "<u4"), ("i_to", "<u4")]

# msv_dom_region as a numpy structured dtype
REGION_DTYPE = [("seq", "<u4"), ("i_from", "<u4"), ("i_to", "<u4"), ("expected_domains", "<f4"), ("mass", "<f4")]


class VitDomain(C.Structure):
    """msv_vit_domain; DOMAIN_DTYPE is the same record as a numpy structured dtype."""
    _fields_ = [
        ("seq", C.c_uint32),
        ("i_from", C.c_uint32),
        ("i_to", C.c_uint32),
        ("k_from", C.c_uint32),
        ("k_to", C.c_uint32),
        ("ops_len", C.c_uint32),
        ("ops_begin", C.c_uint64),
    ]


DOMAIN_DTYPE = [("seq", "<u4"), ("i_from", "<u4"), ("i_to", "<u4"), ("k_from", "<u4"), ("k_to", "<u4"),
                ("ops_len", "<u4"), ("ops_begin", "<u8")]


class VitTraceInfo(C.Structure):
    _fields_ = [
        ("plan", C.c_char * 64),
        ("states_per_lane", C.c_uint32),
        ("lanes_per_sequence", C.c_uint32),
        ("capacity", C.c_uint32),
        ("scratch_bytes", C.c_uint32),
        ("words_per_lane", C.c_uint32),
        ("blocks", C.c_uint32),
        ("lds_bytes", C.c_uint32),
        ("reserved", C.c_uint32),
        ("default_workspace_bytes", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved"}
        d["plan"] = self.plan.decode()
        return d


class VitTraceStats(C.Structure):
    _fields_ = [("chunks", C.c_uint64), ("pointer_bytes", C.c_uint64), ("fill_ms", C.c_float),
                ("walk_ms", C.c_float)]


class BfInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("model_length", C.c_uint32),
        ("residues_per_lane", C.c_uint32),
        ("residues_per_trip", C.c_uint32),
        ("waves_per_block", C.c_uint32),
        ("blocks", C.c_uint32),
        ("lds_bytes", C.c_uint32),
        ("scratch_bytes", C.c_uint32),
        ("vgprs", C.c_uint32),
        ("device", C.c_int),
        ("table", C.c_float * 26),
        ("variant", C.c_char * 64),
    ]

    def as_dict(self) -> dict:
        d = {f: getattr(self, f) for f, _ in self._fields_ if f != "struct_size"}
        d["variant"] = self.variant.decode()
        d["table"] = [float(x) for x in self.table]
        return d


class SearchOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint64), ("bias_filter", C.c_int32), ("reserved", C.c_int32),
                ("bias_profile", C.c_void_p)]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MSV HIP library is not built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C hmm_fasta_viterbi_amd/csrc`.")
    # One HIP runtime per process: torch ships its own libamdhip64 (soname libamdhip64.so.7, the
    # same soname /opt/rocm's has).  Loading torch first makes our DT_NEEDED bind to torch's copy,
    # so streams, events and device pointers from torch are valid handles for this library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, u64, u32, f32 = C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_float
    fp = C.POINTER(C.c_float)
    sig = {
        "msv_status_string": (C.c_char_p, [C.c_int]),
        "msv_version": (C.c_char_p, []),
        "msv_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "msv_hmm_read": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "msv_hmm_destroy": (None, [vp]),
        "msv_hmm_model_length": (sz, [vp]),
        "msv_hmm_name": (C.c_char_p, [vp]),
        "msv_hmm_stats": (None, [vp, fp]),
        "msv_hmm_match_emissions": (fp, [vp]),
        "msv_hmm_insert_emissions": (fp, [vp]),
        "msv_hmm_transitions": (fp, [vp]),
        "msv_hmm_msv_scores": (C.c_int, [vp, fp, fp, fp, fp]),
        "msv_sequence_transitions": (None, [u64, fp, fp]),
        "msv_fasta_read": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "msv_fasta_destroy": (None, [vp]),
        "msv_fasta_count": (sz, [vp]),
        "msv_fasta_rejected": (sz, [vp]),
        "msv_fasta_codes": (C.POINTER(C.c_uint8), [vp]),
        "msv_fasta_offsets": (C.POINTER(C.c_uint64), [vp]),
        "msv_fasta_header": (C.c_char_p, [vp, sz]),
        "msv_encode_residues": (C.c_int, [C.c_char_p, sz, vp]),
        "msv_profile_create": (C.c_int, [C.c_int, vp, u32, f32, f32, f32, C.POINTER(vp)]),
        "msv_profile_create_from_hmm": (C.c_int, [C.c_int, vp, C.POINTER(vp)]),
        "msv_profile_destroy": (None, [vp]),
        "msv_profile_describe": (C.c_int, [vp, C.POINTER(KernelInfo)]),
        "msv_profile_variant_for": (C.c_char_p, [vp, C.c_uint64]),
        "msv_profile_reserve_length": (C.c_int, [vp, u64]),
        "msv_score_batch": (C.c_int, [vp, vp, vp, u64, vp, vp]),
        "msv_host_alloc": (C.c_int, [sz, C.POINTER(vp)]),
        "msv_host_free": (C.c_int, [vp]),
        "msv_score_batch_device": (C.c_int, [vp, vp, u64, vp, u64, vp, vp, vp]),
        "msv_score_batch_async": (C.c_int, [vp, vp, vp, u64, vp, C.POINTER(C.c_uint64)]),
        "msv_profile_wait": (C.c_int, [vp, u64]),
        "msv_profile_bind_stream": (C.c_int, [vp, vp]),
        "msv_multi_create": (C.c_int, [vp, C.c_uint32, C.POINTER(vp)]),
        "msv_multi_score_batch": (C.c_int, [vp, vp, vp, u64, vp]),
        "msv_multi_destroy": (None, [vp]),
        "msv_profile_check": (C.c_int, [vp, vp]),
        "msv_order_longest_first": (C.c_int, [vp, vp, u64, vp, vp]),
        "msv_variant_count": (C.c_int, []),
        "msv_variant_name": (C.c_char_p, [C.c_int]),
        "msv_profile_set_variant": (C.c_int, [vp, C.c_char_p]),
        "msv_score_grid": (C.c_int, [vp, C.c_uint32, vp, vp, u64, vp, vp]),
        "msv_score_grid_device": (C.c_int, [vp, C.c_uint32, vp, u64, vp, u64, vp, vp, vp]),
        "msv_pvalues": (C.c_int, [vp, vp, u64, C.c_float, C.c_float, vp]),
        "msv_shard_bounds": (C.c_int, [vp, u64, C.c_uint32, vp]),
        "msv_lazy_bound_table": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_int, vp]),
        "msv_fasta_parse_device": (C.c_int, [C.c_int, vp, u64, vp, vp]),
        "msv_fasta_read_device": (C.c_int, [C.c_int, C.c_char_p, vp, vp]),
        "msv_fasta_device_destroy": (None, [vp]),
        "msv_fasta_device_count": (u64, [vp]),
        "msv_fasta_device_device": (C.c_int, [vp]),
        "msv_fasta_device_rejected": (u64, [vp]),
        "msv_fasta_device_residues": (u64, [vp]),
        "msv_fasta_device_codes": (vp, [vp]),
        "msv_fasta_device_offsets": (vp, [vp]),
        "msv_fasta_device_header_spans": (vp, [vp]),
        "msv_fasta_device_text": (vp, [vp]),
        "msv_fasta_device_download": (C.c_int, [vp, vp, vp, vp]),
        "msv_fasta_device_max_length": (u64, [vp]),
        "msv_score_fasta_device": (C.c_int, [vp, vp, vp]),
        "msv_score_batch_multi": (C.c_int, [vp, C.c_uint32, vp, vp, u64, vp]),
        "msv_pvalues_device": (C.c_int, [C.c_int, vp, vp, u64, C.c_float, C.c_float, vp, vp]),
        "msv_filter_select_device": (C.c_int, [C.c_int, vp, vp, vp, u64, f32, f32, C.c_double, vp, vp, vp, vp]),
        "msv_hmm_viterbi_scores": (C.c_int, [vp, C.c_int, vp, vp, vp, fp, fp, fp]),
        "msv_vit_cpu_score": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, fp]),
        "msv_vit_profile_create": (C.c_int, [C.c_int, vp, vp, vp, u32, f32, f32, f32, C.POINTER(vp)]),
        "msv_vit_profile_create_from_hmm": (C.c_int, [C.c_int, vp, C.c_int, C.POINTER(vp)]),
        "msv_vit_profile_destroy": (None, [vp]),
        "msv_vit_profile_reserve_length": (C.c_int, [vp, u64]),
        "msv_vit_profile_describe": (C.c_int, [vp, C.POINTER(VitInfo)]),
        "msv_vit_variant_count": (C.c_int, []),
        "msv_vit_variant_name": (C.c_char_p, [C.c_int]),
        "msv_vit_profile_set_variant": (C.c_int, [vp, C.c_char_p]),
        "msv_vit_score_batch_device": (C.c_int, [vp, vp, u64, vp, u64, vp, vp, vp, vp]),
        "msv_vit_profile_bind_stream": (C.c_int, [vp, vp]),
        "msv_vit_score_batch": (C.c_int, [vp, vp, vp, u64, vp, vp]),
        "msv_vit_profile_check": (C.c_int, [vp, vp]),
        "msv_vit_filter_batch": (C.c_int, [vp, vp, vp, vp, u64, f32, f32, C.c_double, vp, vp, vp,
                                           C.POINTER(C.c_uint64)]),
        "msv_vit_cpu_trace": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, fp, C.POINTER(u32),
                                        C.POINTER(u64), vp, vp]),
        "msv_vit_trace_plan_count": (C.c_int, []),
        "msv_vit_trace_plan_name": (C.c_char_p, [C.c_int]),
        "msv_vit_trace_plan_capacity": (u32, [C.c_int]),
        "msv_vit_trace_plan_cell": (C.c_int, [C.c_int, u32] + [C.POINTER(u32)] * 5),
        "msv_vit_trace_sequence_bytes": (u64, [C.c_int, u64]),
        "msv_vit_trace_chunk_cuts": (C.c_int, [vp, u64, u64, vp, C.POINTER(u64)]),
        "msv_vit_trace_batch": (C.c_int, [vp, vp, vp, u64, vp, u64, u64, C.POINTER(vp)]),
        "msv_vit_traces_count": (u64, [vp]),
        "msv_vit_traces_domains": (u64, [vp]),
        "msv_vit_traces_ops": (u64, [vp]),
        "msv_vit_traces_copy": (C.c_int, [vp, vp, vp, vp, vp]),
        "msv_vit_traces_free": (None, [vp]),
        "msv_vit_trace_describe": (C.c_int, [vp, C.POINTER(VitTraceInfo)]),
        "msv_vit_traces_stats": (C.c_int, [vp, C.POINTER(VitTraceStats)]),
        "msv_fwd_cpu_score": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, C.POINTER(C.c_double)]),
        "msv_fwd_cpu_score_batch": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, vp, u64, vp]),
        "msv_fwd_pvalues": (C.c_int, [vp, vp, u64, f32, f32, vp]),
        "msv_fwd_scan_constants": (C.c_int, [vp, u32, u32, vp, vp, vp]),
        "msv_fwd_profile_create": (C.c_int, [C.c_int, vp, vp, vp, u32, f32, f32, f32, C.POINTER(vp)]),
        "msv_fwd_profile_create_from_hmm": (C.c_int, [C.c_int, vp, C.c_int, C.POINTER(vp)]),
        "msv_fwd_profile_destroy": (None, [vp]),
        "msv_fwd_profile_reserve_length": (C.c_int, [vp, u64]),
        "msv_fwd_profile_describe": (C.c_int, [vp, C.POINTER(FwdInfo)]),
        "msv_fwd_variant_count": (C.c_int, []),
        "msv_fwd_variant_name": (C.c_char_p, [C.c_int]),
        "msv_fwd_profile_set_variant": (C.c_int, [vp, C.c_char_p]),
        "msv_fwd_score_batch_device": (C.c_int, [vp, vp, u64, vp, u64, vp, vp, vp, vp]),
        "msv_fwd_profile_bind_stream": (C.c_int, [vp, vp]),
        "msv_fwd_score_batch": (C.c_int, [vp, vp, vp, u64, vp, vp]),
        "msv_fwd_profile_check": (C.c_int, [vp, vp]),
        "msv_fwd_pvalues_device": (C.c_int, [C.c_int, vp, vp, u64, f32, f32, vp, vp]),
        "msv_fwd_filter_batch": (C.c_int, [vp, vp, vp, vp, vp, u64, vp, C.c_double, C.c_double, vp, vp, vp, vp, vp,
                                           vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "msv_dom_cpu_decode": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), vp, vp, vp]),
        "msv_dom_cpu_decode_batch": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, vp, u64, vp, vp, vp, vp, vp]),
        "msv_dom_regions": (C.c_int, [vp, vp, vp, u64, f32, f32, C.POINTER(u32), vp]),
        "msv_dom_scan_constants": (C.c_int, [vp, u32, u32, vp, vp, vp]),
        "msv_dom_sequence_bytes": (u64, [u64]),
        "msv_dom_profile_create": (C.c_int, [C.c_int, vp, vp, vp, u32, f32, f32, f32, C.POINTER(vp)]),
        "msv_dom_profile_create_from_hmm": (C.c_int, [C.c_int, vp, C.c_int, C.POINTER(vp)]),
        "msv_dom_profile_destroy": (None, [vp]),
        "msv_dom_profile_reserve_length": (C.c_int, [vp, u64]),
        "msv_dom_profile_describe": (C.c_int, [vp, C.POINTER(DomInfo)]),
        "msv_dom_variant_count": (C.c_int, []),
        "msv_dom_variant_name": (C.c_char_p, [C.c_int]),
        "msv_dom_profile_set_variant": (C.c_int, [vp, C.c_char_p]),
        "msv_dom_profile_bind_stream": (C.c_int, [vp, vp]),
        "msv_dom_profile_check": (C.c_int, [vp, vp]),
        "msv_dom_score_batch_device": (C.c_int, [vp, vp, u64, vp, u64, vp, vp, vp, vp]),
        "msv_dom_score_batch": (C.c_int, [vp, vp, vp, u64, vp, vp]),
        "msv_dom_decode_batch_device": (C.c_int, [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp]),
        "msv_dom_decode_batch": (C.c_int, [vp, vp, vp, u64, vp, u64, f32, f32, u64, C.POINTER(vp)]),
        "msv_dom_result_count": (u64, [vp]),
        "msv_dom_result_residues": (u64, [vp]),
        "msv_dom_result_regions": (u64, [vp]),
        "msv_dom_result_copy": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "msv_dom_result_free": (None, [vp]),
        "msv_dom_result_stats": (C.c_int, [vp, C.POINTER(DomStats)]),
        "msv_aln_cpu_decode": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, u64, C.POINTER(C.c_double),
                                         vp, vp, vp, vp, vp]),
        "msv_aln_oa": (C.c_int, [vp, vp, vp, vp, vp, vp, u32, f32, f32, f32, u64, u64, C.POINTER(f32),
                                 C.POINTER(u32), C.POINTER(u64), vp, vp, vp]),
        "msv_aln_cpu_align": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, u64, C.POINTER(C.c_double),
                                        C.POINTER(f32), C.POINTER(u32), C.POINTER(u64), vp, vp, vp]),
        "msv_aln_item_bytes": (u64, [u32, u64]),
        "msv_aln_align_batch": (C.c_int, [vp, vp, vp, u64, vp, u64, u64, C.c_int, C.POINTER(vp)]),
        "msv_aln_result_count": (u64, [vp]),
        "msv_aln_result_domains": (u64, [vp]),
        "msv_aln_result_ops": (u64, [vp]),
        "msv_aln_result_copy": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "msv_aln_result_posteriors": (C.c_int, [vp, u64, vp, vp, vp, vp, vp]),
        "msv_aln_result_free": (None, [vp]),
        "msv_aln_describe": (C.c_int, [vp, C.POINTER(AlnInfo)]),
        "msv_aln_result_stats": (C.c_int, [vp, C.POINTER(AlnStats)]),
        "msv_aln_cpu_null2": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, u64, vp, C.POINTER(C.c_double)]),
        "msv_aln_null2_correction": (C.c_int, [vp, vp, u64, C.POINTER(f32)]),
        "msv_aln_bias_scores": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, vp, u64, f32, f32, vp, vp, vp, vp, vp, vp]),
        "msv_aln_align_batch_opts": (C.c_int, [vp, vp, vp, u64, vp, u64, C.POINTER(AlnOptions), C.POINTER(vp)]),
        "msv_aln_result_null2": (C.c_int, [vp, vp, vp]),
        "msv_aln_result_null2_stats": (C.c_int, [vp, C.POINTER(AlnNull2Stats)]),
        "msv_hmm_compo": (fp, [vp]),
        "msv_background_frequencies": (fp, []),
        "msv_bf_cpu_score": (C.c_int, [vp, vp, u32, vp, u64, C.POINTER(C.c_double)]),
        "msv_bf_cpu_score_batch": (C.c_int, [vp, vp, u32, vp, vp, u64, vp]),
        "msv_bf_pvalues": (C.c_int, [vp, vp, vp, u64, f32, f32, C.c_int, vp]),
        "msv_bf_device_table": (C.c_int, [vp, vp, u32, vp]),
        "msv_bf_profile_create": (C.c_int, [C.c_int, vp, vp, u32, C.POINTER(vp)]),
        "msv_bf_profile_create_from_hmm": (C.c_int, [C.c_int, vp, C.POINTER(vp)]),
        "msv_bf_profile_destroy": (None, [vp]),
        "msv_bf_profile_describe": (C.c_int, [vp, C.POINTER(BfInfo)]),
        "msv_bf_score_batch": (C.c_int, [vp, vp, vp, u64, vp, vp]),
        "msv_bf_score_batch_device": (C.c_int, [vp, vp, u64, vp, u64, vp, vp, vp, vp]),
        "msv_bf_profile_bind_stream": (C.c_int, [vp, vp]),
        "msv_bf_profile_check": (C.c_int, [vp, vp]),
        "msv_bf_filter_select_device": (C.c_int, [C.c_int, vp, vp, vp, vp, u64, f32, f32, C.c_double, vp, vp, vp, vp]),
        "msv_bf_pvalues_device": (C.c_int, [C.c_int, vp, vp, vp, u64, f32, f32, C.c_int, vp, vp]),
        "msv_fwd_filter_batch_opts": (C.c_int, [vp, vp, vp, vp, vp, u64, vp, C.c_double, C.c_double,
                                                C.POINTER(SearchOptions), vp, vp, vp, vp, vp, vp,
                                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp, vp,
                                                C.POINTER(C.c_uint64)]),
        "msv_dom_is_multidomain": (C.c_int, [vp, vp, u64, u32, u32, f32, C.POINTER(C.c_int)]),
        "msv_spl_cpu_forward": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, u64, C.POINTER(C.c_double),
                                          vp, vp, vp, vp, vp]),
        "msv_spl_sample": (C.c_int, [vp, vp, vp, vp, vp, u32, f32, f32, f32, u64, u64, u32, u32, u32, u32,
                                     C.POINTER(u32), C.POINTER(u64), C.POINTER(C.c_int), vp, vp, vp]),
        "msv_spl_cluster": (C.c_int, [vp, u64, u32, C.POINTER(SplClusterOptions), C.POINTER(u32), vp]),
        "msv_spl_item_bytes": (u64, [u32, u64]),
        "msv_spl_sample_batch": (C.c_int, [vp, vp, vp, u64, vp, u64, C.POINTER(SplOptions), C.POINTER(vp)]),
        "msv_spl_result_count": (u64, [vp]),
        "msv_spl_result_segments": (u64, [vp]),
        "msv_spl_result_copy": (C.c_int, [vp, vp, vp, vp]),
        "msv_spl_result_matrix": (C.c_int, [vp, u64, vp, vp, vp, vp]),
        "msv_spl_result_stats": (C.c_int, [vp, C.POINTER(SplStats)]),
        "msv_spl_result_free": (None, [vp]),
        "msv_spl_describe": (C.c_int, [vp, C.POINTER(SplInfo)]),
        "msv_cal_lambda": (C.c_int, [vp, u32, vp, C.POINTER(C.c_double)]),
        "msv_cal_thresholds": (C.c_int, [vp, vp]),
        "msv_cal_codes_of_draws": (C.c_int, [vp, vp, u64, vp]),
        "msv_cal_generate": (C.c_int, [vp, u64, u32, u64, u64, u64, vp, vp]),
        "msv_cal_fit_location": (C.c_int, [vp, u64, u64, C.c_double, C.POINTER(C.c_double)]),
        "msv_cal_fit_gumbel": (C.c_int, [vp, u64, u64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(u32)]),
        "msv_cal_tau": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
        "msv_cal_cpu_calibrate": (C.c_int, [vp, u32, C.POINTER(CalOptions), vp, C.POINTER(CalReport)]),
        "msv_cal_workspace_bytes": (u64, [u64, u64]),
        "msv_cal_generate_device": (C.c_int, [C.c_int, vp, u64, u32, u64, u64, u64, vp, vp, vp]),
        "msv_cal_fit_device": (C.c_int, [C.c_int, vp, u64, u64, C.c_int, C.c_double, C.c_double, vp, vp]),
        "msv_cal_calibrate": (C.c_int, [vp, vp, vp, vp, C.POINTER(CalOptions), vp, C.POINTER(CalReport)]),
        "msv_emit_tables": (C.c_int, [vp, C.POINTER(EmitOptions), vp, vp, vp, vp, vp]),
        "msv_emit_generate": (C.c_int, [vp, C.POINTER(EmitOptions), u64, u64, u64, C.POINTER(vp)]),
        "msv_emit_result_count": (u64, [vp]),
        "msv_emit_result_residues": (u64, [vp]),
        "msv_emit_result_domains": (u64, [vp]),
        "msv_emit_result_ops": (u64, [vp]),
        "msv_emit_result_chunks": (u64, [vp]),
        "msv_emit_result_copy": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "msv_emit_result_free": (None, [vp]),
        "msv_emit_path_score": (C.c_int, [vp, vp, vp, u32, f32, f32, f32, vp, u64, vp, u32, vp,
                                          C.POINTER(C.c_double)]),
        "msv_emit_workspace_bytes": (u64, [u64, u64, u64, u64, C.c_int]),
        "msv_emit_profile_create": (C.c_int, [C.c_int, vp, C.POINTER(EmitOptions), C.POINTER(vp)]),
        "msv_emit_profile_destroy": (None, [vp]),
        "msv_emit_profile_bind_stream": (C.c_int, [vp, vp]),
        "msv_emit_batch_device": (C.c_int, [vp, u64, u64, u64, vp, u64, vp, C.POINTER(EmitTruth),
                                            C.POINTER(EmitTotals), vp]),
        "msv_emit_batch": (C.c_int, [vp, u64, u64, u64, C.c_int, u64, vp, C.POINTER(vp)]),
        "msv_emit_describe": (C.c_int, [vp, C.POINTER(EmitInfo)]),
        "msv_emit_profile_times": (C.c_int, [vp, fp, fp, fp]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("MSV_LIB_PATH") and not hasattr(L, name):
            continue  # an older build under A/B timing may predate an entry point
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status: int, what: str = "") -> None:
    if status != MSV_OK:
        raise MSVError(status, what)
