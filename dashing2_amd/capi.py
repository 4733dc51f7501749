"""ctypes mirror of include/d2g.h.  No computation happens here: every method forwards to the
C ABI of libd2g.so (HIP kernels + x86 host half).  Missing library => ImportError-like failure,
never a silent fallback."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("D2G_LIB") or os.path.join(_HERE, "libd2g.so")
_lib = None

SIMILARITY, CONTAINMENT, SYMMETRIC_CONTAINMENT, POISSON_LLR, INTERSECTION, UNION_SIZE = range(6)
K2_SCHEDULES = ("classic", "merged", "planes-emit")     # D2G_K2_MERGE = 0, 1, 2: the bit-sliced prepare's schedule (CmpSet.sparse_detail)
CMP_AUTO, CMP_DIRECT, CMP_BITSLICE, CMP_PLANES = 0, 1, 2, 3
# bit-sliced pair kernel: VALU operations per pair and 32-register group = (id planes of the group) + this (one v_bcnt)
BITSLICE_OPS_PER_GROUP_EXTRA = 1


TIME_K1, TIME_K2, TIME_K2PREP, TIME_K3, TIME_K0 = 2, 4, 8, 16, 32          # include/d2g.h D2G_TIME_*
TIME_KNN = 64
TIME_DEDUP = 128
TIME_FILTER = 256
TIME_KSET = 512
TIME_SCREEN = 1024
TIME_EDIT = 2048
TIME_EDIT_NEAR = 4096
TIME_EDIT_DEDUP = 8192
EDIT_MAX_LEN = 65535                                                     # include/d2g.h D2G_EDIT_MAX_LEN
EDIT_BAND_MAX = 31                                                       # include/d2g.h D2G_EDIT_BAND_MAX


class D2GError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        name = lib().d2g_strerror(status).decode() if _lib is not None else str(status)
        super().__init__(f"d2g error {status} ({name}){': ' + detail if detail else ''}")


def build(jobs=8):
    """Compile libd2g.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", f"-j{jobs}", "-C", os.path.join(_HERE, "csrc")])
    return LIB_PATH


_u64, _sz, _dbl, _int, _f32 = C.c_uint64, C.c_size_t, C.c_double, C.c_int, C.c_float
_vp, _cp = C.c_void_p, C.c_char_p
_pu64, _pu32, _pdbl, _pf32, _pu8 = (C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double),
                                    C.POINTER(C.c_float), C.POINTER(C.c_uint8))

# name: (restype, argtypes) -- must cover every d2g_* declared in include/d2g.h (tested)
SIGNATURES = {
    "d2g_version": (_int, []),
    "d2g_strerror": (_cp, [_int]),
    "d2g_device_count": (_int, []),
    "d2g_ctx_create": (_int, [_int, C.POINTER(_vp)]),
    "d2g_ctx_destroy": (None, [_vp]),
    "d2g_last_error": (_cp, [_vp]),
    "d2g_ctx_device": (_int, [_vp]),
    "d2g_ctx_reload_tuning": (_int, [_vp]),
    "d2g_ctx_tuning": (_int, [_vp, C.c_char_p, _sz]),
    "d2g_sync": (_int, [_vp, _vp]),
    "d2g_malloc": (_int, [_vp, _sz, C.POINTER(_vp)]),
    "d2g_free": (_int, [_vp, _vp]),
    "d2g_malloc_host": (_int, [_vp, _sz, C.POINTER(_vp)]),
    "d2g_host_register": (_int, [_vp, _vp, _sz]),
    "d2g_host_unregister": (_int, [_vp, _vp]),
    "d2g_free_host": (_int, [_vp, _vp]),
    "d2g_memcpy_h2d": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "d2g_memcpy_d2h": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "d2g_set_timing": (_int, [_vp, _int]),
    "d2g_kernel_ms": (_int, [_vp, _cp, _int, C.POINTER(_int), C.POINTER(_f32), C.POINTER(_f32)]),
    "d2g_wang_hash": (_u64, [_u64]),
    "d2g_wang_hash_inverse": (_u64, [_u64]),
    "d2g_oph_kmer_ids": (_int, [_vp, _sz, _sz, _sz, _vp]),
    "d2g_seed_mask": (_u64, [_u64]),
    "d2g_oph_xor_const": (_u64, []),
    "d2g_oph_m": (_sz, [_sz]),
    "d2g_oph_card": (_dbl, [_pu64, _sz]),
    "d2g_oph_signatures": (_int, [_pu64, _sz, _pdbl]),
    "d2g_oph_finalize": (_int, [_pu64, _sz, _sz, _sz, _pdbl, _pdbl, _int]),
    "d2g_densify": (_int, [_pdbl, _sz, _sz, C.POINTER(_sz), _int]),
    "d2g_epilogue_gtlt": (_f32, [_u64, _u64, _sz, _dbl, _dbl, _int, _int]),
    "d2g_epilogue_neq": (_f32, [_u64, _sz, _dbl, _dbl, _int, _int]),
    "d2g_epilogue_ut": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _int, _int, _int, _int, _vp]),
    "d2g_epilogue_lut": (_int, [_sz, _int, _int, _int, _pf32]),
    "d2g_regs_truncate": (_int, [_vp, _sz, _sz, _int, _int, _vp, _vp, _vp, _int, C.c_char_p, _sz]),
    "d2g_epilogue_trunc_neq": (_f32, [_u64, _sz, _int, _dbl, _dbl, _int, _int]),
    "d2g_epilogue_trunc_gtlt": (_f32, [_u64, _u64, _sz, _vp, _dbl, _dbl, _int, _int]),
    "d2g_epilogue_trunc_ut": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _int, _int, _int, _vp, _int, _vp]),
    "d2g_epilogue_trunc_rect": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz, _sz, _int, _int, _int, _vp, _int, _vp]),
    "d2g_seqpack_create": (_int, [_int, C.POINTER(_vp)]),
    "d2g_seqpack_create_alphabet": (_int, [_int, _int, C.POINTER(_vp)]),
    "d2g_seqpack_alphabet": (_int, [_vp]),
    "d2g_alphabet_size": (_int, [_int]),
    "d2g_alphabet_max_k": (_int, [_int]),
    "d2g_alphabet_code": (_int, [_int, _int]),
    "d2g_alphabet_name": (C.c_char_p, [_int]),
    "d2g_key_bits": (_int, [_int, _int]),
    "d2g_oph_plan_create_alphabet": (_int, [_vp, _vp, _vp, _sz, _vp, _sz, _int, _int, C.POINTER(_vp)]),
    "d2g_sketcher_set_alphabet": (_int, [_vp, _int]),
    "d2g_kmer_filter_create_alphabet": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _int, _int, C.POINTER(_vp)]),
    "d2g_seqpack_destroy": (None, [_vp]),
    "d2g_seqpack_clear": (None, [_vp]),
    "d2g_seqpack_add_path": (_int, [_vp, _cp]),
    "d2g_seqpack_add_fastx": (_int, [_vp, _cp, _sz]),
    "d2g_seqpack_add_sequence": (_int, [_vp, _cp, _sz]),
    "d2g_seqpack_ngenomes": (_sz, [_vp]),
    "d2g_seqpack_nruns": (_sz, [_vp]),
    "d2g_seqpack_packed_bytes": (_sz, [_vp]),
    "d2g_seqpack_packed": (_pu8, [_vp]),
    "d2g_seqpack_run_start": (_pu64, [_vp]),
    "d2g_seqpack_run_len": (_pu32, [_vp]),
    "d2g_seqpack_genome_run_off": (_pu64, [_vp]),
    "d2g_seqpack_nkmers": (_u64, [_vp, _sz]),
    "d2g_seqpack_nbases": (_u64, [_vp]),
    "d2g_oph_sketch": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, _vp]),
    "d2g_oph_plan_create": (_int, [_vp, _vp, _vp, _sz, _vp, _sz, _int, C.POINTER(_vp)]),
    "d2g_oph_plan_create_windowed": (_int, [_vp, _vp, _vp, _sz, _vp, _sz, _int, _int, C.POINTER(_vp)]),
    "d2g_run_emissions": (_u64, [_u64, _int, _int]),
    "d2g_sketcher_set_window": (_int, [_vp, _int]),
    "d2g_oph_plan_destroy": (None, [_vp]),
    "d2g_oph_plan_nkmers": (_u64, [_vp]),
    "d2g_oph_plan_nbases": (_u64, [_vp]),
    "d2g_oph_sketch_dev": (_int, [_vp, _vp, _vp, _int, _u64, _sz, _vp, _vp]),
    "d2g_oph_count_dev": (_int, [_vp, _vp, _vp, _int, _u64, _sz, _vp, _vp, _vp]),
    "d2g_oph_sketch_counts": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, _vp, _vp]),
    "d2g_sketcher_run_counts": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, _vp, _vp]),
    "d2g_oph_sketch_mincount": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, C.c_uint32, _vp, _vp]),
    "d2g_sketcher_run_mincount": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, C.c_uint32, _vp, _vp]),
    "d2g_oph_sketch_mincount_dev": (_int, [_vp, _vp, _vp, _int, _u64, _sz, C.c_uint32, _vp, _vp]),
    "d2g_kmer_filter_create_dev": (_int, [_vp, _vp, _vp, _int, _vp, C.POINTER(_vp)]),
    "d2g_kmer_filter_create": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _int, _int, C.POINTER(_vp)]),
    "d2g_kmer_filter_create_windowed": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _int, _int, _int, C.POINTER(_vp)]),
    "d2g_kmer_filter_destroy": (None, [_vp]),
    "d2g_kmer_filter_info": (_int, [_vp, _vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_sz)]),
    "d2g_kmer_filter_contains": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "d2g_screen_create": (_int, [_vp, _vp, _sz, _sz, _int, _int, _u64, _sz, C.POINTER(_vp)]),
    "d2g_screen_destroy": (None, [_vp]),
    "d2g_screen_table_slots": (_int, [_u64, C.POINTER(_u64)]),
    "d2g_screen_reset": (_int, [_vp, _vp]),
    "d2g_screen_info": (_int, [_vp, _vp, C.POINTER(_u64), C.POINTER(_sz), C.POINTER(_sz)]),
    "d2g_screen_fed": (_int, [_vp, _vp, _sz, C.POINTER(_u64)]),
    "d2g_screen_set_fed": (_int, [_vp, _vp, _sz, _u64]),
    "d2g_screen_add_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "d2g_sketcher_run_screen": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _vp, _vp]),
    "d2g_screen_result": (_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "d2g_screen_key_counts": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "d2g_epilogue_contain": (_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "d2g_mem_info": (_int, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "d2g_seqpack_add_file": (_int, [_vp, _cp]),
    "d2g_oph_plan_set_filter": (_int, [_vp, _vp]),
    "d2g_sketcher_set_filter": (_int, [_vp, _vp]),
    "d2g_sketcher_create": (_int, [_vp, C.POINTER(_vp)]),
    "d2g_sketcher_destroy": (None, [_vp]),
    "d2g_sketcher_run": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, _vp]),
    "d2g_sketcher_run_bmh": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, C.c_double, _vp, _vp]),
    "d2g_bmh_sketch_dev": (_int, [_vp, _vp, _vp, _int, _u64, _sz, C.c_double, _vp, _vp, _vp]),
    "d2g_bmh_sketch": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, C.c_double, _vp, _vp]),
    "d2g_kmer_count": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, C.c_double, _vp, _vp, _sz, _vp]),
    "d2g_kmer_distinct": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _vp]),
    "d2g_kmer_sets": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, C.c_double, _vp, _vp, _sz, _vp, _vp]),
    "d2g_sketcher_run_sets": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, C.c_double, _vp, _vp, _sz, _vp, _vp]),
    "d2g_kmer_sets_dev": (_int, [_vp, _vp, _vp, _int, _u64, C.c_double, _vp, _vp, _sz, _vp, _vp, _vp]),
    "d2g_kset_check": (_int, [_vp, _vp, _vp, _sz, C.c_char_p, _sz]),
    "d2g_kset_create": (_int, [_vp, _vp, _vp, _vp, _sz, C.POINTER(_vp)]),
    "d2g_kset_create_dev": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, C.POINTER(_vp)]),
    "d2g_kset_destroy": (None, [_vp]),
    "d2g_kset_size": (_sz, [_vp]),
    "d2g_kset_device_bytes": (_sz, [_vp]),
    "d2g_kset_slice_bits": (_int, [_vp]),
    "d2g_kset_isz_ut_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "d2g_kset_isz_rect_dev": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp]),
    "d2g_seqrecs_create": (_int, [C.POINTER(_vp)]),
    "d2g_seqrecs_destroy": (None, [_vp]),
    "d2g_seqrecs_add_path": (_int, [_vp, _cp]),
    "d2g_seqrecs_add_fastx": (_int, [_vp, _cp, _sz]),
    "d2g_seqrecs_nrecords": (_sz, [_vp]),
    "d2g_seqrecs_name": (C.c_char_p, [_vp, _sz]),
    "d2g_seqrecs_bytes": (_pu8, [_vp]),
    "d2g_seqrecs_off": (_pu64, [_vp]),
    "d2g_seqset_check": (_int, [_vp, _vp, _sz, _u64, C.c_char_p, _sz]),
    "d2g_seqset_recode_map": (_int, [_vp, _u64, _vp]),
    "d2g_seqset_create": (_int, [_vp, _vp, _vp, _sz, _u64, C.POINTER(_vp)]),
    "d2g_seqset_destroy": (None, [_vp]),
    "d2g_seqset_nrecords": (_sz, [_vp]),
    "d2g_seqset_device_bytes": (_sz, [_vp]),
    "d2g_seqset_alphabet_size": (_int, [_vp]),
    "d2g_seqset_strip_blocks": (_int, [_vp, _vp]),
    "d2g_edit_ut_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "d2g_edit_rect_dev": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp]),
    "d2g_edit_ut": (_int, [_vp, _vp, _sz, _sz, _vp]),
    "d2g_edit_rect": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _vp]),
    "d2g_edit_band_max": (_int, []),
    "d2g_edit_near_dev": (_int, [_vp, _vp, _sz, _sz, C.c_uint32, _vp, _vp]),
    "d2g_edit_within_dev": (_int, [_vp, _vp, _sz, _sz, _sz, C.c_uint32, _sz, _vp, _vp, _vp, _sz, _vp]),
    "d2g_edit_dedup_dev": (_int, [_vp, _vp, C.c_uint32, _vp, _sz, _vp]),
    "d2g_edit_dedup": (_int, [_vp, _vp, C.c_uint32, _sz, _vp]),
    "d2g_edit_knn": (_int, [_vp, _vp, _sz, _sz, _sz, C.c_uint32, _sz, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "d2g_epilogue_exact": (_f32, [_u64, _dbl, _dbl, _int, _int]),
    "d2g_epilogue_exact_ut": (_int, [_vp, _vp, _sz, _sz, _sz, _int, _int, _int, _vp]),
    "d2g_epilogue_exact_rect": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _sz, _int, _int, _int, _vp]),
    "d2g_sketcher_run_distinct": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _vp]),
    "d2g_sketcher_ingest_fasta": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int]),
    "d2g_sketcher_ingested_runs": (_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64)]),
    "d2g_seqpack_add_path_by_record": (_int, [_vp, C.c_char_p]),
    "d2g_seqpack_add_fastx_by_record": (_int, [_vp, C.c_char_p, _sz]),
    "d2g_seqpack_name": (C.c_char_p, [_vp, _sz]),
    "d2g_bmh_sketch_cs": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, _u64, C.c_double, _vp, _vp]),
    "d2g_bmh_sketch_cs_dev": (_int, [_vp, _vp, _vp, _int, _u64, _sz, _u64, C.c_double, _vp, _vp, _vp]),
    "d2g_sketcher_run_bmh_cs": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _sz, _u64, C.c_double, _vp, _vp]),
    "d2g_countsketch_table": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _u64, _vp]),
    "d2g_countsketch_cells": (_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _int, _int, _u64, _u64, C.c_double, _vp, _vp, _sz, _vp, _vp]),
    "d2g_countsketch_lds_cells": (_int, []),
    "d2g_countsketch_stats": (_int, [_vp, _vp, _vp, _vp]),
    "d2g_bmh_check_weights": (_int, [_vp, _vp, _sz, _sz, _dbl, C.c_char_p, _sz]),
    "d2g_xxh3_64": (_u64, [_vp, _sz]),
    "d2g_bed_parse": (_int, [C.c_char_p, _sz, _int, _vp, _vp, _vp, _sz, _vp, C.c_char_p, _sz]),
    "d2g_interval_plan_create": (_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "d2g_interval_plan_destroy": (None, [_vp]),
    "d2g_interval_plan_npositions": (_u64, [_vp]),
    "d2g_interval_oph_sketch": (_int, [_vp, _vp, _sz, _vp]),
    "d2g_interval_oph_sketch_dev": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "d2g_interval_bmh_sketch": (_int, [_vp, _vp, _int, _sz, _vp, _vp]),
    "d2g_interval_runs": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "d2g_bmh_from_weighted": (_int, [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "d2g_bmh_from_weighted_ids": (_int, [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "d2g_ut_count": (_sz, [_sz, _sz, _sz]),
    "d2g_cmp_set_create_dev": (_int, [_vp, _vp, _sz, _sz, _int, _vp, C.POINTER(_vp)]),
    "d2g_cmp_set_create": (_int, [_vp, _vp, _sz, _sz, _int, C.POINTER(_vp)]),
    "d2g_cmp_set_update_dev": (_int, [_vp, _vp, _vp, _vp]),
    "d2g_cmp_set_planes": (_int, [_vp, _vp, _vp, C.POINTER(C.c_uint), C.POINTER(_int), C.POINTER(_f32)]),
    "d2g_cmp_set_status": (_int, [_vp, _vp, _vp]),
    "d2g_cmp_set_sparse_info": (_int, [_vp, _vp, _vp, _vp]),
    "d2g_cmp_set_debug_pairs": (_int, [_vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "d2g_cmp_set_sparse_detail": (_int, [_vp, _vp, _vp, _vp]),
    "d2g_cmp_set_fill_detail": (_int, [_vp, _vp, _vp]),
    "d2g_sparse_bin_geometry": (_int, [_sz, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(_int)]),
    "d2g_warmup": (_int, [_vp, _int]),
    "d2g_device_name": (_int, [_int, C.c_char_p, _sz]),
    "d2g_comm_unique_id": (_int, [_vp]),
    "d2g_comm_create": (_int, [_vp, _vp, _int, _int, C.POINTER(_vp)]),
    "d2g_comm_create_all": (_int, [C.POINTER(_vp), _int, C.POINTER(_vp)]),
    "d2g_comm_destroy": (None, [_vp]),
    "d2g_comm_rank": (_int, [_vp]),
    "d2g_comm_world": (_int, [_vp]),
    "d2g_comm_is_rccl": (_int, [_vp]),
    "d2g_bcast_sigs": (_int, [C.POINTER(_vp), C.POINTER(_vp), _int, _vp, _sz, _sz, C.POINTER(_vp)]),
    "d2g_allpairs_create": (_int, [_vp, _vp, _sz, _sz, C.POINTER(_vp)]),
    "d2g_allpairs_destroy": (None, [_vp]),
    "d2g_allpairs_rows_held": (_int, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "d2g_allpairs_rows_computed": (_int, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "d2g_allpairs_prepare_dev": (_int, [_vp, _vp, _vp]),
    "d2g_allpairs_prepare_all": (_int, [C.POINTER(_vp), _int, C.POINTER(_vp), C.POINTER(_vp)]),
    "d2g_allpairs_operand": (_vp, [_vp]),
    "d2g_allpairs_status": (_int, [_vp, _vp]),
    "d2g_allpairs_chunks": (_int, [_vp]),
    "d2g_allpairs_set_phase_timing": (_int, [_vp, _int]),
    "d2g_allpairs_phase_times": (_int, [_vp, _int, C.POINTER(_int), _vp, _vp, _vp, _vp]),
    "d2g_allpairs_sparse_info": (_int, [_vp, _vp]),
    "d2g_allpairs_step_lut_dev": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "d2g_allpairs_step_eqcount_dev": (_int, [_vp, _vp, _vp, _vp]),
    "d2g_allpairs_step_all": (_int, [C.POINTER(_vp), _int, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "d2g_allpairs_enqueue_lut_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _int]),
    "d2g_operand_layout": (_int, [_sz, _sz, C.POINTER(_sz), C.POINTER(_sz)]),
    "d2g_cmp_set_export_operand_dev": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "d2g_cmp_set_from_planes_dev": (_int, [_vp, _sz, _sz, _vp, _vp, C.POINTER(_vp)]),
    "d2g_pack_column_slices_dev": (_int, [_vp, _vp, _sz, _sz, _int, _vp, _vp]),
    "d2g_cmp_set_destroy": (None, [_vp]),
    "d2g_cmp_set_algo": (_int, [_vp]),
    "d2g_cmp_eqcount_ut_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "d2g_cmp_lut_ut_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "d2g_cmp_ut_prefill_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "d2g_cmp_ut_announce_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "d2g_cmp_set_forget": (_int, [_vp, _vp]),
    "d2g_cmp_gtlt_ut_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "d2g_cmp_eqcount_rect_dev": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp]),
    "d2g_cmp_gtlt_rect_dev": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp, _vp]),
    "d2g_cmp_eqcount_ut": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _int, _vp]),
    "d2g_cmp_dist_ut": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _int, _int, _int, _int, _int, _vp]),
    "d2g_ut_partition": (_int, [_sz, _int, C.POINTER(_sz)]),
    "d2g_cmp_set_create_codes_dev": (_int, [_vp, _vp, _sz, _sz, _int, _vp, C.POINTER(_vp)]),
    "d2g_cmp_set_create_codes": (_int, [_vp, _vp, _sz, _sz, _int, C.POINTER(_vp)]),
    "d2g_cmp_set_operand_bytes": (_sz, [_vp]),
    "d2g_cmp_set_id_bits": (_int, [_vp]),
    "d2g_cmp_dist_trunc_ut": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _int, _int, _int, _int, _int, _vp]),
    "d2g_cmp_knn_dev": (_int, [_vp, _vp, _sz, _sz, _sz, C.c_uint32, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    "d2g_knn_finish": (_int, [_vp, _vp, _vp, _sz, _sz, _vp, _sz, _int, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(_sz)]),
    "d2g_cmp_set_knn": (_int, [_vp, _vp, _sz, _sz, _vp, _int, _sz, _dbl, _sz, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "d2g_cmp_knn": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _int, _int, _int, _int, _sz, _dbl, _sz, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "d2g_cmp_dedup_dev": (_int, [_vp, _vp, C.c_uint32, _vp, _vp, _sz, _vp]),
    "d2g_dedup_clusters": (_int, [_vp, _sz, _vp, _vp, C.POINTER(_sz)]),
    "d2g_cmp_set_dedup": (_int, [_vp, _vp, _vp, _dbl, _sz, _vp]),
    "d2g_cmp_dedup": (_int, [_vp, _vp, _sz, _sz, _int, _int, _int, _int, _dbl, _sz, _vp]),
}


def sparse_info_dict(a):
    """info4 of d2g_cmp_set_sparse_info / d2g_allpairs_sparse_info as a dict"""
    return {"sorted_operand": bool(a[0]), "tiles_listed": int(a[1]), "dense_decided_by_prepare": bool(a[2] & 1), "dense_kernel_ran": bool(a[2] & 2),
            "tiles_and_pair_list": bool(a[2] & 4), "callers_order_kept": bool(a[2] & 8), "ordering_skipped": bool(a[2] & 16), "pairs_listed": int(a[3])}


def lib():
    """Load libd2g.so (once).  Raises if the extension has not been built: no fallback."""
    global _lib
    if _lib is None:
        # torch wheels bundle their own HIP/HSA runtime; two runtimes in one process cannot both own
        # the GPU.  If torch is going to be used next to libd2g (bench, dist), load it FIRST so that
        # libd2g's libamdhip64.so.7 dependency resolves to the copy that is already mapped.
        if os.environ.get("D2G_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(dashing2_amd has no CPU fallback)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                f = getattr(l, name)
            except AttributeError:
                if os.environ.get("D2G_LIB"):      # another build selected for an A/B measurement may predate a symbol: the call fails where it is made
                    continue
                raise
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def _np_ptr(a):
    return a.ctypes.data if a is not None else None


class _Runs:
    """The nine leading arguments of every sketch entry point -- packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k,
    canon -- as `args`, from a SeqPack (anything with arrays() and k), a tuple (packed, run_start, run_len, genome_run_off, k) of host
    arrays, or (None, runs, k) for the stream a sketcher ingested last (packed == NULL).  Holds the arrays for the call."""

    def __init__(self, src, canon):
        if hasattr(src, "arrays"):
            src = tuple(src.arrays()) + (src.k,)
        elif src[0] is None:
            src = (None,) + tuple(src[1][:3]) + (src[2],)
        packed, rs, rl, go, self.k = src
        self.packed = None if packed is None else np.ascontiguousarray(packed, np.uint8)
        self.rs, self.rl, self.go = np.ascontiguousarray(rs, np.uint64), np.ascontiguousarray(rl, np.uint32), np.ascontiguousarray(go, np.uint64)
        self.n = self.go.size - 1
        self.args = (_np_ptr(self.packed), 0 if packed is None else self.packed.size, _np_ptr(self.rs), _np_ptr(self.rl), self.rs.size,
                     _np_ptr(self.go), self.n, self.k, int(canon))

    @property
    def nkmers(self):
        """k-mers of all runs: the most entries an exact count can return"""
        return int(self.rl.astype(np.int64).sum()) - (self.k - 1) * self.rl.size if self.rl.size else 0


# ---------------------------------------------------------------- host-side primitives
def wang_hash(x):
    return int(lib().d2g_wang_hash(x & 0xFFFFFFFFFFFFFFFF))


def wang_hash_inverse(x):
    return int(lib().d2g_wang_hash_inverse(x & 0xFFFFFFFFFFFFFFFF))


SCREEN_MAX_KEYS = 1 << 30                                               # include/d2g.h D2G_SCREEN_MAX_KEYS


def run_emissions(length, k, w=0):
    """k-mers a run of `length` valid bases emits under (k, w): its k-mers, or its window positions when w > k (host, no GPU)"""
    return int(lib().d2g_run_emissions(int(length), int(k), int(w)))


def countsketch_lds_cells():
    """L: count-sketch tables of up to this many cells are accumulated in LDS (host, no GPU)"""
    return int(lib().d2g_countsketch_lds_cells())


def screen_table_slots(ndistinct):
    """slots of the table of a screen with that many distinct keys (host, no GPU); D2GError beyond SCREEN_MAX_KEYS"""
    s = _u64()
    rc = lib().d2g_screen_table_slots(ndistinct, C.byref(s))
    if rc:
        raise D2GError(rc)
    return int(s.value)


def epilogue_contain(matches, matchsums, S):
    """contain's table from the device's integer sums -> (coverage f32, depth f32), shaped like matches (host, no GPU)"""
    m = np.ascontiguousarray(matches, np.uint32)
    s = np.ascontiguousarray(matchsums, np.uint32)
    cov, dep = np.empty(m.shape, np.float32), np.empty(m.shape, np.float32)
    rc = lib().d2g_epilogue_contain(_np_ptr(m), _np_ptr(s), m.size, S, _np_ptr(cov), _np_ptr(dep))
    if rc:
        raise D2GError(rc)
    return cov, dep


def oph_kmer_ids(regs, S):
    """regs u64 [n][m] -> ids u64 [n][S]: the masked k-mer behind each of the first S registers (DHasher::inverse)"""
    regs = np.ascontiguousarray(regs, np.uint64)
    n, m = regs.shape
    ids = np.empty((n, S), np.uint64)
    rc = lib().d2g_oph_kmer_ids(_np_ptr(regs), n, m, S, _np_ptr(ids))
    if rc:
        raise D2GError(rc)
    return ids


def seed_mask(seed):
    return int(lib().d2g_seed_mask(seed))


def oph_xor_const():
    return int(lib().d2g_oph_xor_const())


def oph_m(S):
    return int(lib().d2g_oph_m(S))


def oph_finalize(regs, S, nthreads=1):
    """regs u64 [n][m] -> (sigs f64 [n][S], cards f64 [n])  (x87 host arithmetic in libd2g)"""
    regs = np.ascontiguousarray(regs, np.uint64)
    n, m = regs.shape
    sigs = np.empty((n, S), np.float64)
    cards = np.empty(n, np.float64)
    rc = lib().d2g_oph_finalize(regs.ctypes.data_as(_pu64), n, m, S, sigs.ctypes.data_as(_pdbl),
                                cards.ctypes.data_as(_pdbl), nthreads)
    if rc:
        raise D2GError(rc)
    return sigs, cards


def densify(sigs, nthreads=1):
    sigs = np.ascontiguousarray(sigs, np.float64).copy()
    n, S = sigs.shape
    nf = _sz()
    rc = lib().d2g_densify(sigs.ctypes.data_as(_pdbl), n, S, C.byref(nf), nthreads)
    if rc:
        raise D2GError(rc)
    return sigs, nf.value


def epilogue_lut(S, measure=SIMILARITY, k=31, multiset_space=False):
    lut = np.empty(S + 1, np.float32)
    rc = lib().d2g_epilogue_lut(S, measure, k, int(multiset_space), lut.ctypes.data_as(_pf32))
    if rc:
        raise D2GError(rc)
    return lut


def host_epilogue_ut(ca, cb, cards, N, S, r0, r1, measure=SIMILARITY, k=31, multiset_space=False, nthreads=0):
    """integer counts of rows [r0,r1) -> float32 values (libd2g x87 host arithmetic, OpenMP)"""
    ca = np.ascontiguousarray(ca, np.uint32)
    cb = None if cb is None else np.ascontiguousarray(cb, np.uint32)
    cards = np.ascontiguousarray(cards, np.float64)
    out = np.empty(ca.size, np.float32)
    rc = lib().d2g_epilogue_ut(_np_ptr(ca), _np_ptr(cb), _np_ptr(cards), N, S, r0, r1, measure, k, int(multiset_space),
                               nthreads or (os.cpu_count() or 1), _np_ptr(out))
    if rc:
        raise D2GError(rc)
    return out


def epilogue_gtlt(gt, lt, S, lhc, rhc, measure=SIMILARITY, k=31):
    return float(lib().d2g_epilogue_gtlt(gt, lt, S, lhc, rhc, measure, k))


def epilogue_neq(neq, S, lhc, rhc, measure=SIMILARITY, k=31):
    return float(lib().d2g_epilogue_neq(neq, S, lhc, rhc, measure, k))


# ---- truncated registers (--fastcmp <4|2|1>, --bbit-sigs)
_CODE_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _longdouble_ptr(b):
    """one x87 long double as a pointer (ctypes would round it to a double on the way in)"""
    assert np.finfo(np.longdouble).nmant == 63, "np.longdouble is not the x87 80-bit format here"
    a = np.array([b], np.longdouble)
    return a, a.ctypes.data


def regs_truncate(sigs, regbytes, bbit=False, nthreads=1, with_minmax=False):
    """double signatures [n][S] -> (codes [n][S] of regbytes, a, b) with a, b np.longdouble (0, 0 for b-bit codes);
    with_minmax: also (minreg, maxreg) of the setsketch method"""
    sigs = np.ascontiguousarray(sigs, np.float64)
    assert sigs.ndim == 2
    n, S = sigs.shape
    codes = np.zeros((n, S), _CODE_DTYPES.get(regbytes, np.uint32))
    assert np.finfo(np.longdouble).nmant == 63, "np.longdouble is not the x87 80-bit format here"
    ab = np.zeros(2, np.longdouble)
    mm = np.zeros(2, np.float64)
    err = C.create_string_buffer(256)
    rc = lib().d2g_regs_truncate(_np_ptr(sigs), n, S, regbytes, int(bool(bbit)), _np_ptr(codes), _np_ptr(ab), _np_ptr(mm), nthreads, err, 256)
    if rc:
        raise D2GError(rc, err.value.decode())
    return (codes, ab[0], ab[1], float(mm[0]), float(mm[1])) if with_minmax else (codes, ab[0], ab[1])


def epilogue_trunc_neq(neq, S, regbytes, lhc, rhc, measure=SIMILARITY, k=31):
    return float(lib().d2g_epilogue_trunc_neq(neq, S, regbytes, lhc, rhc, measure, k))


def epilogue_trunc_gtlt(gt, lt, S, b, lhc, rhc, measure=SIMILARITY, k=31):
    keep, pb = _longdouble_ptr(b)
    return float(lib().d2g_epilogue_trunc_gtlt(gt, lt, S, pb, lhc, rhc, measure, k))


def host_epilogue_trunc_ut(ca, cb, cards, N, S, r0, r1, measure=SIMILARITY, k=31, regbytes=1, b=None, nthreads=0):
    """counts of rows [r0,r1) of truncated codes -> float32: b None = ca is neq of b-bit codes, else (ca, cb) = (gt, lt)"""
    ca = np.ascontiguousarray(ca, np.uint32)
    cb = None if cb is None else np.ascontiguousarray(cb, np.uint32)
    cards = np.ascontiguousarray(cards, np.float64)
    out = np.empty(ca.size, np.float32)
    keep, pb = (None, None) if b is None else _longdouble_ptr(b)
    rc = lib().d2g_epilogue_trunc_ut(_np_ptr(ca), _np_ptr(cb), _np_ptr(cards), N, S, r0, r1, measure, k, regbytes, pb,
                                     nthreads or (os.cpu_count() or 1), _np_ptr(out))
    if rc:
        raise D2GError(rc)
    return out


def host_epilogue_trunc_rect(ca, cb, cards, N, S, a0, a1, b0, b1, measure=SIMILARITY, k=31, regbytes=1, b=None, nthreads=0):
    """the same over the row-major block rows [a0,a1) x columns [b0,b1)"""
    ca = np.ascontiguousarray(ca, np.uint32)
    cb = None if cb is None else np.ascontiguousarray(cb, np.uint32)
    cards = np.ascontiguousarray(cards, np.float64)
    out = np.empty((a1 - a0, b1 - b0), np.float32)
    keep, pb = (None, None) if b is None else _longdouble_ptr(b)
    rc = lib().d2g_epilogue_trunc_rect(_np_ptr(ca), _np_ptr(cb), _np_ptr(cards), N, S, a0, a1, b0, b1, measure, k, regbytes, pb,
                                       nthreads or (os.cpu_count() or 1), _np_ptr(out))
    if rc:
        raise D2GError(rc)
    return out


def epilogue_exact(isz, lhcard, rhcard, measure=SIMILARITY, k=31):
    """the exact branch of compare() (--set, --countdict): intersection size and the two cardinalities -> float32"""
    return float(lib().d2g_epilogue_exact(int(isz), lhcard, rhcard, measure, k))


def host_epilogue_exact_ut(isz, cards, N, r0, r1, measure=SIMILARITY, k=31, nthreads=0):
    """exact intersection sizes (uint64) of rows [r0,r1) of the condensed upper triangle -> float32"""
    isz = np.ascontiguousarray(isz, np.uint64)
    cards = np.ascontiguousarray(cards, np.float64)
    out = np.empty(isz.size, np.float32)
    rc = lib().d2g_epilogue_exact_ut(_np_ptr(isz), _np_ptr(cards), N, r0, r1, measure, k, nthreads or (os.cpu_count() or 1), _np_ptr(out))
    if rc:
        raise D2GError(rc)
    return out


def host_epilogue_exact_rect(isz, cards, N, a0, a1, b0, b1, measure=SIMILARITY, k=31, nthreads=0):
    """the same over the row-major block rows [a0,a1) x columns [b0,b1)"""
    isz = np.ascontiguousarray(isz, np.uint64)
    cards = np.ascontiguousarray(cards, np.float64)
    out = np.empty((a1 - a0, b1 - b0), np.float32)
    rc = lib().d2g_epilogue_exact_rect(_np_ptr(isz), _np_ptr(cards), N, a0, a1, b0, b1, measure, k, nthreads or (os.cpu_count() or 1),
                                       _np_ptr(out))
    if rc:
        raise D2GError(rc)
    return out


XXH3_MAX_LEN = 240


def xxh3_64(data):
    """XXH3_64bits (seed 0) of at most XXH3_MAX_LEN bytes; host only"""
    data = bytes(data)
    if len(data) > XXH3_MAX_LEN:
        raise ValueError("d2g_xxh3_64 covers inputs of at most 240 bytes")
    return int(lib().d2g_xxh3_64(data, len(data)))


def bed_parse(buf, trim_chr=True):
    """the data lines of a BED buffer -> (chrhash, start, stop) uint64 arrays; host only.  Raises ValueError with the library's words
    for a line without a tab, a gzip magic, a chromosome name of more than 240 bytes"""
    buf = bytes(buf)
    cap = buf.count(b"\n") + 1
    h, a, b = (np.zeros(cap, np.uint64) for _ in range(3))
    n = _sz()
    err = C.create_string_buffer(512)
    rc = lib().d2g_bed_parse(buf, len(buf), int(bool(trim_chr)), _np_ptr(h), _np_ptr(a), _np_ptr(b), cap, C.addressof(n), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode(errors="replace"))
    return h[:n.value].copy(), a[:n.value].copy(), b[:n.value].copy()


def kset_check(keys, counts, set_off):
    """the host-side check of Context.kset without a device: raises D2GError for a set_off that is not monotone, a set whose keys are
    not strictly ascending (unsorted or duplicated), and a count of 0"""
    keys = np.ascontiguousarray(keys, np.uint64)
    counts = None if counts is None else np.ascontiguousarray(counts, np.uint32)
    set_off = np.ascontiguousarray(set_off, np.uint64)
    assert keys.size >= int(set_off.max(initial=0)) and (counts is None or counts.size == keys.size)
    err = C.create_string_buffer(256)
    rc = lib().d2g_kset_check(_np_ptr(keys), _np_ptr(counts), _np_ptr(set_off), set_off.size - 1, err, 256)
    if rc:
        raise D2GError(rc, err.value.decode())


def _seq_arrays(records):
    """a list of byte strings -> (bytes u8, off u64[n + 1])"""
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
    return np.frombuffer(b"".join(bytes(r) for r in records), np.uint8).copy(), off


def seqset_check(data, off):
    """the host-side check of Context.seqset without a device: raises D2GError (INVALID) for an off that does not begin at 0, decreases
    or does not end at the byte count, and (UNSUPPORTED) for a record of more than EDIT_MAX_LEN symbols"""
    data = np.ascontiguousarray(data, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    err = C.create_string_buffer(256)
    rc = lib().d2g_seqset_check(_np_ptr(data), _np_ptr(off), off.size - 1, data.size, err, 256)
    if rc:
        raise D2GError(rc, err.value.decode())


def seqset_recode_map(data):
    """-> (map u8[256], sigma): the dense code of every byte value that occurs in `data`, in order of byte value"""
    data = np.ascontiguousarray(data, np.uint8)
    m = np.zeros(256, np.uint8)
    return m, int(lib().d2g_seqset_recode_map(_np_ptr(data), data.size, _np_ptr(m)))


def bmh_check_weights(weights, set_off, S, scale=1.0):
    """the host-side checks of Context.bmh_from_weighted / _ids without a device: raises D2GError for a NaN weight, a weight above
    2^53, a set_off that is not monotone, and a non-empty set whose total weight is too small for S (its bound would not stay finite)"""
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    set_off = np.ascontiguousarray(set_off, np.uint64)
    assert w is None or w.size >= int(set_off.max(initial=0))
    err = C.create_string_buffer(256)
    rc = lib().d2g_bmh_check_weights(_np_ptr(w), _np_ptr(set_off), set_off.size - 1, S, scale, err, 256)
    if rc:
        raise D2GError(rc, err.value.decode())


class KnnOverflow(ValueError):
    """d2g_knn_finish met rows whose true count exceeds the slots they were given"""
    def __init__(self, rows):
        self.rows = rows
        super().__init__(f"{rows} row(s) hold more candidates than their slots: re-run them with a cap that fits")


def knn_finish(rowcnt, ids, counts, cap, lut, isdist=False):
    """candidate lists (rowcnt [n], ids / counts [n][cap]) -> CSR (indptr u64 [n+1], indices u32, data f32) in the reference's order"""
    rowcnt = np.ascontiguousarray(rowcnt, np.uint32)
    ids = np.ascontiguousarray(ids, np.uint32)
    counts = np.ascontiguousarray(counts, np.uint32)
    lut = np.ascontiguousarray(lut, np.float32)
    n = rowcnt.size
    assert ids.size >= n * cap and counts.size >= n * cap
    indptr = np.zeros(n + 1, np.uint64)
    need, over = _sz(), _sz()
    rc = lib().d2g_knn_finish(_np_ptr(rowcnt), _np_ptr(ids), _np_ptr(counts), n, cap, _np_ptr(lut), lut.size - 1, int(bool(isdist)),
                              _np_ptr(indptr), None, None, 0, C.byref(need), C.byref(over))
    if over.value:
        raise KnnOverflow(over.value)
    if rc not in (0, -4):
        raise D2GError(rc)
    indices = np.empty(need.value, np.uint32)
    data = np.empty(need.value, np.float32)
    if need.value:
        rc = lib().d2g_knn_finish(_np_ptr(rowcnt), _np_ptr(ids), _np_ptr(counts), n, cap, _np_ptr(lut), lut.size - 1, int(bool(isdist)),
                                  _np_ptr(indptr), _np_ptr(indices), _np_ptr(data), need.value, None, None)
        if rc:
            raise D2GError(rc)
    return indptr, indices, data


def dedup_clusters(assign):
    """assign [N] (the representative of every sketch) -> (indptr u64 [C+1], indices u32 [N]): clusters in creation order, the
    representative first, then the members in input order"""
    assign = np.ascontiguousarray(assign, np.uint32)
    n = assign.size
    indptr = np.zeros(n + 1, np.uint64)
    indices = np.empty(n, np.uint32)
    nc = _sz()
    rc = lib().d2g_dedup_clusters(_np_ptr(assign), n, _np_ptr(indptr), _np_ptr(indices), C.byref(nc))
    if rc:
        raise D2GError(rc)
    return indptr[:nc.value + 1].copy(), indices


def operand_layout(N, S):
    """-> (u32 words per 32-register group, number of groups) of the bit-sliced operand"""
    gw, ng = _sz(), _sz()
    rc = lib().d2g_operand_layout(N, S, C.byref(gw), C.byref(ng))
    if rc:
        raise D2GError(rc)
    return int(gw.value), int(ng.value)


def sparse_bin_geometry(N):
    """-> dict(cshift, nch, nbins, binned_ok): the output bins of the sparse path's pair list for a set of N sketches (no GPU needed)"""
    cs, nch, nb, ok = C.c_uint32(), C.c_uint32(), C.c_uint32(), _int()
    rc = lib().d2g_sparse_bin_geometry(N, C.byref(cs), C.byref(nch), C.byref(nb), C.byref(ok))
    if rc:
        raise D2GError(rc)
    return {"cshift": cs.value, "nch": nch.value, "nbins": nb.value, "binned_ok": bool(ok.value)}


def ut_count(N, r0=0, r1=None):
    return int(lib().d2g_ut_count(N, r0, N if r1 is None else r1))


def ut_partition(N, nparts):
    b = (_sz * (nparts + 1))()
    rc = lib().d2g_ut_partition(N, nparts, b)
    if rc:
        raise D2GError(rc)
    return [int(x) for x in b]


# ---------------------------------------------------------------- alphabets (K1a)
ALPHABET_DNA, ALPHABET_PROTEIN20, ALPHABET_PROTEIN_3BIT, ALPHABET_PROTEIN_14, ALPHABET_PROTEIN_6 = 0, 2, 3, 4, 5


def alphabet_size(alphabet):
    """symbols of the alphabet (4 for DNA; 0 for an unknown id)"""
    return int(lib().d2g_alphabet_size(alphabet))


def alphabet_max_k(alphabet):
    """the largest k whose key fits 64 bits (32 for DNA; 0 for an unknown id)"""
    return int(lib().d2g_alphabet_max_k(alphabet))


def alphabet_code(alphabet, byte):
    """code of a byte (an int, or a one-character str / bytes) under the alphabet, -1 for anything that ends a run"""
    return int(lib().d2g_alphabet_code(alphabet, byte if isinstance(byte, int) else ord(byte)))


def alphabet_name(alphabet):
    return lib().d2g_alphabet_name(alphabet).decode()


def key_bits(k, alphabet=ALPHABET_DNA):
    """bits of the widest key of (k, alphabet): 2k for DNA, the bit length of A^k - 1 for a protein alphabet"""
    return int(lib().d2g_key_bits(k, alphabet))


# ---------------------------------------------------------------- ingest
class SeqPack:
    """FASTA/FASTQ -> packed run stream (d2g_seqpack_*).  alphabet: ALPHABET_DNA (2 bits per base) or a protein alphabet (one byte per
    residue, K1a) -- the stream then belongs to a Sketcher / a plan / a filter under the same alphabet."""

    def __init__(self, k, alphabet=ALPHABET_DNA):
        self.k = k
        self.alphabet = alphabet
        self._h = None
        h = _vp()
        rc = lib().d2g_seqpack_create_alphabet(k, alphabet, C.byref(h))
        if rc:
            raise D2GError(rc)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_seqpack_destroy(self._h)
            self._h = None

    __del__ = close

    def clear(self):
        """forget the content, keep the allocations"""
        lib().d2g_seqpack_clear(self._h)

    def add_path(self, path):
        rc = lib().d2g_seqpack_add_path(self._h, os.fsencode(path))
        if rc:
            raise D2GError(rc, str(path))

    def add_file(self, path):
        """one genome from ONE file, its name taken as it stands (spaces included)"""
        rc = lib().d2g_seqpack_add_file(self._h, os.fsencode(path))
        if rc:
            raise D2GError(rc, str(path))

    def add_path_by_record(self, path):
        rc = lib().d2g_seqpack_add_path_by_record(self._h, os.fsencode(path))
        if rc:
            raise D2GError(rc, str(path))

    def add_fastx_by_record(self, buf):
        rc = lib().d2g_seqpack_add_fastx_by_record(self._h, buf, len(buf))
        if rc:
            raise D2GError(rc, "add_fastx_by_record")

    def name(self, g):
        return lib().d2g_seqpack_name(self._h, g).decode()

    def add_fastx(self, data: bytes):
        rc = lib().d2g_seqpack_add_fastx(self._h, data, len(data))
        if rc:
            raise D2GError(rc)

    def add_sequence(self, seq: bytes):
        rc = lib().d2g_seqpack_add_sequence(self._h, seq, len(seq))
        if rc:
            raise D2GError(rc)

    @property
    def ngenomes(self):
        return int(lib().d2g_seqpack_ngenomes(self._h))

    @property
    def nruns(self):
        return int(lib().d2g_seqpack_nruns(self._h))

    @property
    def nbases(self):
        return int(lib().d2g_seqpack_nbases(self._h))

    def nkmers(self, g):
        return int(lib().d2g_seqpack_nkmers(self._h, g))

    def arrays(self):
        """-> (packed u8, run_start u64, run_len u32, genome_run_off u64) as numpy copies"""
        l = lib()
        nb = l.d2g_seqpack_packed_bytes(self._h)
        nr, ng = self.nruns, self.ngenomes
        packed = np.ctypeslib.as_array(l.d2g_seqpack_packed(self._h), shape=(nb,)).copy()
        rs = np.ctypeslib.as_array(l.d2g_seqpack_run_start(self._h), shape=(nr,)).copy() if nr else np.empty(0, np.uint64)
        rl = np.ctypeslib.as_array(l.d2g_seqpack_run_len(self._h), shape=(nr,)).copy() if nr else np.empty(0, np.uint32)
        go = np.ctypeslib.as_array(l.d2g_seqpack_genome_run_off(self._h), shape=(ng + 1,)).copy()
        return packed, rs, rl, go


# ---------------------------------------------------------------- device context
class Context:
    """One GPU (d2g_ctx).  Raises D2GError when no gfx950 device is usable."""

    def __init__(self, device=0):
        self._h = None
        h = _vp()
        rc = lib().d2g_ctx_create(device, C.byref(h))
        if rc:
            raise D2GError(rc, f"d2g_ctx_create(device={device})")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc:
            raise D2GError(rc, lib().d2g_last_error(self._h).decode())

    def sync(self, stream=None):
        self._check(lib().d2g_sync(self._h, stream))

    def reload_tuning(self):
        """the D2G_* switches are read once, at context creation: read them again (tests that change one between calls)"""
        self._check(lib().d2g_ctx_reload_tuning(self._h))

    def tuning(self):
        """-> dict of the D2G_* switches this context resolved (only those that were set)"""
        import json
        n = lib().d2g_ctx_tuning(self._h, None, 0)
        if n < 0:
            self._check(n)
        buf = C.create_string_buffer(n + 1)
        lib().d2g_ctx_tuning(self._h, buf, n + 1)
        return json.loads(buf.value.decode())

    def set_timing(self, on=True):
        """True / False, or an OR of TIME_K1 / TIME_K2 / TIME_K2PREP / TIME_K3 (time only what is reported: an event pair in
        the stream costs a few microseconds of device time per launch)"""
        self._check(lib().d2g_set_timing(self._h, int(on)))

    def kernel_ms(self, which, reset=True):
        """-> (count, avg_ms, last_ms) of the launches logged since the last reset"""
        n, avg, last = _int(), _f32(), _f32()
        self._check(lib().d2g_kernel_ms(self._h, which.encode(), int(reset), C.byref(n), C.byref(avg), C.byref(last)))
        return int(n.value), float(avg.value), float(last.value)

    # -- K1 ------------------------------------------------------------------
    def oph_sketch(self, packed, run_start, run_len, genome_run_off, k, S, canon=True, xormask=0):
        """host arrays -> regs u64 [n][m]"""
        return self._oph_sketch((packed, run_start, run_len, genome_run_off, k), S, canon, xormask)

    def _oph_sketch(self, src, S, canon, xormask):
        r = _Runs(src, canon)
        regs = np.empty((r.n, oph_m(S)), np.uint64)
        self._check(lib().d2g_oph_sketch(self._h, *r.args, xormask, S, _np_ptr(regs)))
        return regs

    def oph_sketch_seqpack(self, sp: SeqPack, S, canon=True, xormask=0):
        return self._oph_sketch(sp, S, canon, xormask)

    def oph_sketch_counts(self, packed, run_start, run_len, genome_run_off, k, S, canon=True, xormask=0):
        """host arrays -> (regs u64 [n][m], counts u32 [n][m]): K1, then how often the k-mer behind each register occurred"""
        return self._oph_sketch_counts((packed, run_start, run_len, genome_run_off, k), S, canon, xormask)

    def _oph_sketch_counts(self, src, S, canon, xormask):
        r = _Runs(src, canon)
        regs = np.empty((r.n, oph_m(S)), np.uint64)
        counts = np.empty((r.n, oph_m(S)), np.uint32)
        self._check(lib().d2g_oph_sketch_counts(self._h, *r.args, xormask, S, _np_ptr(regs), _np_ptr(counts)))
        return regs, counts

    def oph_sketch_counts_seqpack(self, sp: SeqPack, S, canon=True, xormask=0):
        return self._oph_sketch_counts(sp, S, canon, xormask)

    def oph_sketch_mincount_seqpack(self, sp: SeqPack, S, mincount, canon=True, xormask=0, counts=False):
        """One-Permutation registers over the k-mers seen at least `mincount` times (sketch -m; mincount < 2: the plain sketch)
        -> regs u64 [n][m], or (regs, counts u32 [n][m]) with counts=True"""
        r = _Runs(sp, canon)
        regs = np.empty((r.n, oph_m(S)), np.uint64)
        cnts = np.empty((r.n, oph_m(S)), np.uint32) if counts else None
        self._check(lib().d2g_oph_sketch_mincount(self._h, *r.args, xormask, S, mincount, _np_ptr(regs), _np_ptr(cnts)))
        return (regs, cnts) if counts else regs

    def oph_sketch_mincount_dev(self, plan, packed_dev_ptr, S, mincount, regs_dev_ptr, canon=True, xormask=0, stream=None):
        """the device-resident form; synchronises `stream`.  Counts: oph_count_dev over regs_dev_ptr"""
        self._check(lib().d2g_oph_sketch_mincount_dev(self._h, plan._h, packed_dev_ptr, int(canon), xormask, S, mincount, regs_dev_ptr, stream))

    def sketcher(self):
        return Sketcher(self)

    # -- K3 (--multiset: exact k-mer counts -> BagMinHash) ---------------------
    def bmh_sketch_seqpack(self, sp: "SeqPack", S, canon=True, xormask=0, count_threshold=0.0):
        """-> (sig float64[n][S], total_weight float64[n])"""
        r = _Runs(sp, canon)
        sig = np.empty((r.n, S), np.float64)
        tw = np.empty(r.n, np.float64)
        self._check(lib().d2g_bmh_sketch(self._h, *r.args, xormask, S, count_threshold, _np_ptr(sig), _np_ptr(tw)))
        return sig, tw

    def bmh_sketch_dev(self, plan, packed_dev_ptr, S, sig_dev_ptr, tw_dev_ptr, canon=True, xormask=0, count_threshold=0.0,
                       stream=None):
        self._check(lib().d2g_bmh_sketch_dev(self._h, plan._h, packed_dev_ptr, int(canon), xormask, S, count_threshold,
                                             sig_dev_ptr, tw_dev_ptr, stream))

    # -- K3k (--multiset -c <cells>: count-sketch -> BagMinHash) --------------------
    def bmh_sketch_cs_seqpack(self, sp: "SeqPack", S, cells, canon=True, xormask=0, count_threshold=0.0):
        """-> (sig float64[n][S], total_weight float64[n]) over the cells with |count| >= count_threshold"""
        r = _Runs(sp, canon)
        sig = np.empty((r.n, S), np.float64)
        tw = np.empty(r.n, np.float64)
        self._check(lib().d2g_bmh_sketch_cs(self._h, *r.args, xormask, S, cells, count_threshold, _np_ptr(sig), _np_ptr(tw)))
        return sig, tw

    def bmh_sketch_cs_dev(self, plan, packed_dev_ptr, S, cells, sig_dev_ptr, tw_dev_ptr, canon=True, xormask=0, count_threshold=0.0,
                          stream=None):
        self._check(lib().d2g_bmh_sketch_cs_dev(self._h, plan._h, packed_dev_ptr, int(canon), xormask, S, cells, count_threshold,
                                                sig_dev_ptr, tw_dev_ptr, stream))

    def countsketch_table(self, sp: "SeqPack", cells, canon=True, xormask=0):
        """-> int32[n][cells]: the signed tables (small tables only)"""
        r = _Runs(sp, canon)
        tab = np.empty((r.n, cells), np.int32)
        self._check(lib().d2g_countsketch_table(self._h, *r.args, xormask, cells, _np_ptr(tab)))
        return tab

    def countsketch_cells(self, sp: "SeqPack", cells, canon=True, xormask=0, count_threshold=0.0, cap=None):
        """-> (ids uint64[total], weights float64[total], set_off uint64[n+1], totals uint64[n]): the kept cells of every input, ascending"""
        r = _Runs(sp, canon)
        if cap is None:
            cap = sum(min(cells, sp.nkmers(g)) for g in range(r.n)) if hasattr(sp, "nkmers") else r.nkmers
        ids, w = np.empty(max(cap, 1), np.uint64), np.empty(max(cap, 1), np.float64)
        off, tot = np.zeros(r.n + 1, np.uint64), np.zeros(r.n, np.uint64)
        self._check(lib().d2g_countsketch_cells(self._h, *r.args, xormask, cells, count_threshold, _np_ptr(ids), _np_ptr(w), cap,
                                                _np_ptr(off), _np_ptr(tot)))
        return ids[:int(off[-1])].copy(), w[:int(off[-1])].copy(), off, tot

    def countsketch_stats(self):
        """-> (largest table in bytes, groups, batches) of the count-sketch calls on this context"""
        b, g, n = _u64(), _u64(), _u64()
        self._check(lib().d2g_countsketch_stats(self._h, C.byref(b), C.byref(g), C.byref(n)))
        return int(b.value), int(g.value), int(n.value)

    def kmer_count(self, packed, run_start, run_len, genome_run_off, k, canon=True, xormask=0, count_threshold=0.0):
        """host arrays (any run table over `packed`) -> list over genomes of (keys uint64[nd], counts uint32[nd]), each sorted by key"""
        return self._kmer_count((packed, run_start, run_len, genome_run_off, k), canon, xormask, count_threshold)

    def _kmer_count(self, src, canon, xormask, count_threshold):
        r = _Runs(src, canon)
        cap = r.nkmers
        keys = np.empty(max(cap, 1), np.uint64)
        counts = np.empty(max(cap, 1), np.uint32)
        off = np.zeros(r.n + 1, np.uint64)
        self._check(lib().d2g_kmer_count(self._h, *r.args, xormask, count_threshold, _np_ptr(keys), _np_ptr(counts), cap, _np_ptr(off)))
        out = []
        for g in range(r.n):
            k_, c_ = keys[int(off[g]):int(off[g + 1])], counts[int(off[g]):int(off[g + 1])]
            o = np.argsort(k_, kind="stable")
            out.append((k_[o].copy(), c_[o].copy()))
        return out

    def kmer_count_seqpack(self, sp: "SeqPack", canon=True, xormask=0, count_threshold=0.0):
        """-> list over genomes of (keys uint64[nd], counts uint32[nd]), each sorted by key"""
        return self._kmer_count(sp, canon, xormask, count_threshold)

    def kmer_sets_seqpack(self, sp: "SeqPack", canon=True, xormask=0, count_threshold=0.0, counts=True):
        """the exact k-mer sets, sorted on the device -> (keys uint64[total], counts uint32[total] or None, set_off uint64[n+1],
        cards uint64[n][2] = (distinct keys, sum of the counts))"""
        return _kmer_sets(self, lib().d2g_kmer_sets, self._h, _Runs(sp, canon), xormask, count_threshold, counts)

    def kmer_sets_dev(self, plan, packed_dev_ptr, keys_dev_ptr, counts_dev_ptr, cap, set_off_dev_ptr, cards_dev_ptr, canon=True, xormask=0,
                      count_threshold=0.0, stream=None):
        """the device-resident form; synchronises `stream`"""
        self._check(lib().d2g_kmer_sets_dev(self._h, plan._h, packed_dev_ptr, int(canon), xormask, count_threshold, keys_dev_ptr, counts_dev_ptr,
                                            cap, set_off_dev_ptr, cards_dev_ptr, stream))

    def kset(self, keys, counts, set_off):
        """host arrays (sorted sets, e.g. loaded files) -> KSet; refuses unsorted or duplicated keys"""
        keys = np.ascontiguousarray(keys, np.uint64)
        counts = None if counts is None else np.ascontiguousarray(counts, np.uint32)
        set_off = np.ascontiguousarray(set_off, np.uint64)
        h = _vp()
        self._check(lib().d2g_kset_create(self._h, _np_ptr(keys), _np_ptr(counts), _np_ptr(set_off), set_off.size - 1, C.byref(h)))
        return KSet(self, h)

    def kset_dev(self, keys_dev_ptr, counts_dev_ptr, set_off_dev_ptr, nsets, stream=None):
        """the device arrays of kmer_sets_dev -> KSet (copied)"""
        h = _vp()
        self._check(lib().d2g_kset_create_dev(self._h, keys_dev_ptr, counts_dev_ptr, set_off_dev_ptr, nsets, stream, C.byref(h)))
        return KSet(self, h)

    def seqset(self, records=None, data=None, off=None):
        """a list of byte strings (or their concatenation and off[n + 1]) -> SeqSet, resident and recoded on the device"""
        if records is not None:
            data, off = _seq_arrays(records)
        data = np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        h = _vp()
        self._check(lib().d2g_seqset_create(self._h, _np_ptr(data), _np_ptr(off), off.size - 1, data.size, C.byref(h)))
        return SeqSet(self, h)

    def kmer_distinct_seqpack(self, sp: "SeqPack", canon=True, xormask=0):
        """-> uint64[n]: exact number of distinct masked k-mers per genome"""
        r = _Runs(sp, canon)
        out = np.zeros(r.n, np.uint64)
        self._check(lib().d2g_kmer_distinct(self._h, *r.args, xormask, _np_ptr(out)))
        return out

    def bmh_from_weighted(self, ids, weights, set_off, S):
        """-> (sig float64[nsets][S], total_weight float64[nsets])"""
        ids = np.ascontiguousarray(ids, np.uint64)
        w = None if weights is None else np.ascontiguousarray(weights, np.float64)
        set_off = np.ascontiguousarray(set_off, np.uint64)
        ns = set_off.size - 1
        sig = np.empty((ns, S), np.float64)
        tw = np.empty(ns, np.float64)
        self._check(lib().d2g_bmh_from_weighted(self._h, _np_ptr(ids), None if w is None else _np_ptr(w), _np_ptr(set_off),
                                                ns, S, _np_ptr(sig), _np_ptr(tw)))
        return sig, tw

    def bmh_from_weighted_ids(self, ids, weights, set_off, S):
        """-> (sig, total_weight, owner uint64[nsets][S]): owner = position within its set of the element that set the register"""
        ids = np.ascontiguousarray(ids, np.uint64)
        w = None if weights is None else np.ascontiguousarray(weights, np.float64)
        set_off = np.ascontiguousarray(set_off, np.uint64)
        ns = set_off.size - 1
        sig = np.empty((ns, S), np.float64)
        tw = np.empty(ns, np.float64)
        own = np.empty((ns, S), np.uint64)
        self._check(lib().d2g_bmh_from_weighted_ids(self._h, _np_ptr(ids), None if w is None else _np_ptr(w), _np_ptr(set_off),
                                                    ns, S, _np_ptr(sig), _np_ptr(tw), _np_ptr(own)))
        return sig, tw, own

    def oph_plan(self, run_start, run_len, genome_run_off, k, w=0, alphabet=ALPHABET_DNA):
        """launch plan over a run table; w > k: a windowed one (K1w) -- every *_dev call over it walks minimizers; a protein alphabet
        (K1a): every *_dev call over it reads a byte-per-residue stream (no window with it)"""
        run_start = np.ascontiguousarray(run_start, np.uint64)
        run_len = np.ascontiguousarray(run_len, np.uint32)
        genome_run_off = np.ascontiguousarray(genome_run_off, np.uint64)
        h = _vp()
        if alphabet != ALPHABET_DNA:
            if w > k:
                raise ValueError("a window (w > k) with a protein alphabet: the windowed walker is DNA only")
            self._check(lib().d2g_oph_plan_create_alphabet(self._h, _np_ptr(run_start), _np_ptr(run_len), run_start.size,
                                                           _np_ptr(genome_run_off), genome_run_off.size - 1, k, alphabet, C.byref(h)))
            return OphPlan(self, h, genome_run_off.size - 1)
        self._check(lib().d2g_oph_plan_create_windowed(self._h, _np_ptr(run_start), _np_ptr(run_len), run_start.size,
                                                       _np_ptr(genome_run_off), genome_run_off.size - 1, k, w, C.byref(h)))
        return OphPlan(self, h, genome_run_off.size - 1)

    # -- K1i (interval sets: sketch / cmp --bed) --------------------------------
    def interval_plan(self, chrhash, start, stop, file_off):
        """launch plan over the lines of n BED files: file f owns lines [file_off[f], file_off[f + 1])"""
        chrhash, start, stop, file_off = (np.ascontiguousarray(x, np.uint64) for x in (chrhash, start, stop, file_off))
        assert chrhash.size == start.size == stop.size
        h = _vp()
        self._check(lib().d2g_interval_plan_create(self._h, _np_ptr(chrhash), _np_ptr(start), _np_ptr(stop), chrhash.size, _np_ptr(file_off),
                                                   file_off.size - 1, C.byref(h)))
        return IntervalPlan(self, h, file_off.size - 1)

    def interval_oph_sketch(self, plan, S):
        """-> regs uint64[n][m]"""
        regs = np.empty((plan.n, oph_m(S)), np.uint64)
        self._check(lib().d2g_interval_oph_sketch(self._h, plan._h, S, _np_ptr(regs)))
        return regs

    def interval_oph_sketch_dev(self, plan, S, regs_dev_ptr, stream=None):
        """the same into device memory [n][m] on `stream`; does not synchronise"""
        self._check(lib().d2g_interval_oph_sketch_dev(self._h, plan._h, S, regs_dev_ptr, stream))

    def interval_bmh_sketch(self, plan, S, normalize=False):
        """--multiset -> (sig float64[n][S], total_weight float64[n])"""
        sig = np.empty((plan.n, S), np.float64)
        tw = np.empty(plan.n, np.float64)
        self._check(lib().d2g_interval_bmh_sketch(self._h, plan._h, int(bool(normalize)), S, _np_ptr(sig), _np_ptr(tw)))
        return sig, tw

    # -- K1s (contain: reads screened against a k-mer database) ----------------
    def screen(self, keys, k, canon=True, xormask=0, nrows=1):
        """keys u64 [nrefs][S] (masked, a .kmer64 payload) -> Screen with nrows rows of counters"""
        keys = np.ascontiguousarray(keys, np.uint64)
        nrefs, S = keys.shape
        h = _vp()
        self._check(lib().d2g_screen_create(self._h, _np_ptr(keys), nrefs, S, k, int(canon), xormask, nrows, C.byref(h)))
        return Screen(self, h, nrefs, S, k, canon, nrows)

    def mem_info(self):
        """-> (free, total) bytes of device memory"""
        f, t = _sz(), _sz()
        self._check(lib().d2g_mem_info(self._h, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    # -- K1f (--filterset: k-mers every sketch skips) ---------------------------
    def kmer_filter(self, sp: "SeqPack", canon=True, w=0):
        """the k-mers of ALL genomes of `sp` as one device-resident set (host-pointer form; synchronises); w > k: its minimizers"""
        r = _Runs(sp, canon)
        h = _vp()
        if getattr(sp, "alphabet", ALPHABET_DNA) != ALPHABET_DNA:      # K1a: the pack's alphabet; there is no canonical form (canon is not looked at)
            if w > sp.k:
                raise ValueError("a window (w > k) with a protein alphabet: the windowed walker is DNA only")
            self._check(lib().d2g_kmer_filter_create_alphabet(self._h, *r.args[:5], r.args[7], sp.alphabet, C.byref(h)))
            return KmerFilter(self, h, sp.k, False)
        self._check(lib().d2g_kmer_filter_create_windowed(self._h, *r.args[:5], *r.args[7:], w, C.byref(h)))      # no genomes: all runs feed one set
        return KmerFilter(self, h, sp.k, bool(canon))

    def kmer_filter_dev(self, plan, packed_dev_ptr, canon=True, stream=None):
        """the same from a plan and a device-resident packed stream; enqueues on `stream`"""
        h = _vp()
        self._check(lib().d2g_kmer_filter_create_dev(self._h, plan._h, packed_dev_ptr, int(canon), stream, C.byref(h)))
        return KmerFilter(self, h, None, bool(canon))

    def oph_sketch_dev(self, plan, packed_dev_ptr, S, regs_dev_ptr, canon=True, xormask=0, stream=None):
        self._check(lib().d2g_oph_sketch_dev(self._h, plan._h, packed_dev_ptr, int(canon), xormask, S, regs_dev_ptr, stream))

    def oph_count_dev(self, plan, packed_dev_ptr, S, regs_dev_ptr, counts_dev_ptr, canon=True, xormask=0, stream=None):
        """counts u32 [n][m] of the k-mers whose id equals the register they map to, for any registers; does not synchronise"""
        self._check(lib().d2g_oph_count_dev(self._h, plan._h, packed_dev_ptr, int(canon), xormask, S, regs_dev_ptr, counts_dev_ptr, stream))

    # -- K2 ------------------------------------------------------------------
    def cmp_set(self, sig_bits_host, algo=CMP_AUTO):
        a = np.ascontiguousarray(sig_bits_host)
        assert a.dtype.itemsize == 8 and a.ndim == 2
        h = _vp()
        self._check(lib().d2g_cmp_set_create(self._h, _np_ptr(a), a.shape[0], a.shape[1], algo, C.byref(h)))
        return CmpSet(self, h, a.shape[0], a.shape[1])

    def cmp_set_dev(self, dev_ptr, N, S, algo=CMP_AUTO, stream=None):
        h = _vp()
        self._check(lib().d2g_cmp_set_create_dev(self._h, dev_ptr, N, S, algo, stream, C.byref(h)))
        return CmpSet(self, h, N, S)

    def cmp_set_codes(self, codes_host):
        """set of truncated codes (uint8 / uint16 / uint32 [N][S]): (gt, lt) and equality counts only"""
        a = np.ascontiguousarray(codes_host)
        assert a.ndim == 2 and a.dtype in (np.uint8, np.uint16, np.uint32)
        h = _vp()
        self._check(lib().d2g_cmp_set_create_codes(self._h, _np_ptr(a), a.shape[0], a.shape[1], a.dtype.itemsize, C.byref(h)))
        return CmpSet(self, h, a.shape[0], a.shape[1])

    def cmp_set_codes_dev(self, dev_ptr, N, S, regbytes, stream=None):
        h = _vp()
        self._check(lib().d2g_cmp_set_create_codes_dev(self._h, dev_ptr, N, S, regbytes, stream, C.byref(h)))
        return CmpSet(self, h, N, S)

    def cmp_dist_trunc_ut(self, sigs, cards, measure=SIMILARITY, k=31, regbytes=1, bbit=False, r0=0, r1=None, nthreads=1):
        """truncate + upload + count + epilogue: float32 values of rows [r0,r1) from (densified) double signatures"""
        a = np.ascontiguousarray(sigs, np.float64)
        assert a.ndim == 2
        cards = np.ascontiguousarray(cards, np.float64)
        N, S = a.shape
        r1 = N if r1 is None else r1
        out = np.empty(ut_count(N, r0, r1), np.float32)
        self._check(lib().d2g_cmp_dist_trunc_ut(self._h, _np_ptr(a), _np_ptr(cards), N, S, r0, r1, measure, k, regbytes,
                                                int(bool(bbit)), nthreads, _np_ptr(out)))
        return out

    def cmp_set_from_planes(self, N, S, planes_dev_ptr, meta_dev_ptr):
        h = _vp()
        self._check(lib().d2g_cmp_set_from_planes_dev(self._h, N, S, planes_dev_ptr, meta_dev_ptr, C.byref(h)))
        return CmpSet(self, h, N, S)

    def pack_column_slices_dev(self, rows_dev_ptr, n, S, W, out_dev_ptr, stream=None):
        self._check(lib().d2g_pack_column_slices_dev(self._h, rows_dev_ptr, n, S, W, out_dev_ptr, stream))

    def cmp_eqcount_ut(self, sig_bits_host, r0=0, r1=None, algo=CMP_AUTO):
        a = np.ascontiguousarray(sig_bits_host)
        assert a.dtype.itemsize == 8 and a.ndim == 2
        N, S = a.shape
        r1 = N if r1 is None else r1
        out = np.empty(ut_count(N, r0, r1), np.uint32)
        self._check(lib().d2g_cmp_eqcount_ut(self._h, _np_ptr(a), N, S, r0, r1, algo, _np_ptr(out)))
        return out

    def cmp_dist_ut(self, sig_bits_host, cards, measure=SIMILARITY, k=31, multiset_space=False, r0=0, r1=None,
                    algo=CMP_AUTO, nthreads=1):
        a = np.ascontiguousarray(sig_bits_host)
        assert a.dtype.itemsize == 8 and a.ndim == 2
        cards = np.ascontiguousarray(cards, np.float64)
        N, S = a.shape
        r1 = N if r1 is None else r1
        out = np.empty(ut_count(N, r0, r1), np.float32)
        self._check(lib().d2g_cmp_dist_ut(self._h, _np_ptr(a), _np_ptr(cards), N, S, r0, r1, measure, k,
                                          int(multiset_space), algo, nthreads, _np_ptr(out)))
        return out

    def cmp_knn(self, sig_bits_host, K=0, threshold=0.0, measure=SIMILARITY, k=31, multiset_space=False, r0=0, r1=None,
                algo=CMP_AUTO, cap=0, band_rows=0):
        """nearest neighbours of rows [r0,r1): top-K (all ties with the K-th best kept) or every pair at / beyond `threshold`;
        returns CSR (indptr u64, indices u32, data f32), best first inside a row"""
        a = np.ascontiguousarray(sig_bits_host)
        assert a.dtype.itemsize == 8 and a.ndim == 2
        N, S = a.shape
        r1 = N if r1 is None else r1
        return _knn_csr(self, r1 - r0, K, lambda ip, ix, dt, oc, need: lib().d2g_cmp_knn(
            self._h, _np_ptr(a), N, S, r0, r1, measure, k, int(multiset_space), algo, K, float(threshold), cap, band_rows, ip, ix, dt, oc, need))

    def cmp_dedup(self, sig_bits_host, threshold, measure=SIMILARITY, k=31, multiset_space=False, algo=CMP_AUTO, band_rows=0):
        """greedy clustering in input order (cmp --greedy): -> assign u32 [N], the representative of every sketch"""
        a = np.ascontiguousarray(sig_bits_host)
        assert a.dtype.itemsize == 8 and a.ndim == 2
        N, S = a.shape
        out = np.empty(N, np.uint32)
        self._check(lib().d2g_cmp_dedup(self._h, _np_ptr(a), N, S, measure, k, int(multiset_space), algo, float(threshold), band_rows, _np_ptr(out)))
        return out

    # -- raw device memory (tests / bench without torch) ------------------------
    def malloc(self, nbytes):
        p = _vp()
        self._check(lib().d2g_malloc(self._h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr):
        self._check(lib().d2g_free(self._h, ptr))

    def h2d(self, dptr, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        self._check(lib().d2g_memcpy_h2d(self._h, dptr, _np_ptr(arr), arr.nbytes, stream))

    def d2h(self, arr, dptr, stream=None):
        assert arr.flags["C_CONTIGUOUS"]
        self._check(lib().d2g_memcpy_d2h(self._h, _np_ptr(arr), dptr, arr.nbytes, stream))


def _knn_csr(ctx, nrows, K, call):
    """runs call(indptr, indices, data, out_cap, &needed) with a first guess of the output size and once more if it was short"""
    indptr = np.zeros(nrows + 1, np.uint64)
    guess = max(1, nrows * (2 * K + 16 if K else 64))
    for _ in range(2):
        indices, data = np.empty(guess, np.uint32), np.empty(guess, np.float32)
        need = _sz()
        rc = call(_np_ptr(indptr), _np_ptr(indices), _np_ptr(data), guess, C.byref(need))
        if rc != -4:        # D2G_ERR_NOMEM with `need` set: the arrays were too small
            break
        guess = need.value
    ctx._check(rc)
    return indptr, indices[:need.value].copy(), data[:need.value].copy()


def _kmer_sets(ctx, fn, handle, r, xormask, count_threshold, counts):
    """d2g_kmer_sets / d2g_sketcher_run_sets over the runs `r` -> (keys, counts or None, set_off, cards)"""
    cap = r.nkmers
    keys = np.empty(max(cap, 1), np.uint64)
    cnts = np.empty(max(cap, 1), np.uint32) if counts else None
    off = np.zeros(r.n + 1, np.uint64)
    cards = np.zeros((r.n, 2), np.uint64)
    ctx._check(fn(handle, *r.args, xormask, count_threshold, _np_ptr(keys), _np_ptr(cnts), cap, _np_ptr(off), _np_ptr(cards)))
    total = int(off[r.n])
    return keys[:total], (cnts[:total] if counts else None), off, cards


class Sketcher:
    """persistent K1 front end (d2g_sketcher): reuses device buffers across calls"""

    def __init__(self, ctx):
        self.ctx = ctx
        self._h = None
        h = _vp()
        ctx._check(lib().d2g_sketcher_create(ctx._h, C.byref(h)))
        self._h = h

    def set_filter(self, filt):
        """attach a KmerFilter (None detaches): every run* of this sketcher skips its k-mers.  The sketcher keeps it alive."""
        self.ctx._check(lib().d2g_sketcher_set_filter(self._h, filt._h if filt is not None else None))
        self._filter = filt

    def set_window(self, w):
        """K1w: every later run* of this sketcher walks the minimizers of windows of w bases when w > its k; 0 or w <= k: off"""
        self.ctx._check(lib().d2g_sketcher_set_window(self._h, int(w)))

    def set_alphabet(self, alphabet):
        """K1a: every later run* of this sketcher reads its stream as one byte per residue of this protein alphabet (a SeqPack made
        with the same one); ALPHABET_DNA switches back"""
        self.ctx._check(lib().d2g_sketcher_set_alphabet(self._h, int(alphabet)))

    def _ingested(self, runs, k):
        """the source of a run table over the stream ingested last (k: default the k of the ingest)"""
        return (None, runs, self.k if k is None else k)

    def _run_screen(self, src, screen, genome_row, canon):
        r = _Runs(src, canon)
        rows = np.ascontiguousarray(genome_row, np.uint32)
        assert rows.size == r.n
        self.ctx._check(lib().d2g_sketcher_run_screen(self._h, *r.args, screen._h, _np_ptr(rows)))

    def run_screen(self, sp, screen, genome_row, canon=True):
        """the k-mers of genome g of the pack count towards row genome_row[g] of the Screen; synchronises"""
        self._run_screen(sp, screen, genome_row, canon)

    def run_screen_ingested(self, runs, screen, genome_row, canon=True, k=None):
        """run_screen over the stream ingested last (packed == NULL)"""
        self._run_screen(self._ingested(runs, k), screen, genome_row, canon)

    def run_distinct(self, sp, canon=True, xormask=0):
        """-> distinct k-mers per genome, u64 [n] (exact)"""
        r = _Runs(sp, canon)
        nd = np.zeros(r.n, np.uint64)
        self.ctx._check(lib().d2g_sketcher_run_distinct(self._h, *r.args, xormask, _np_ptr(nd)))
        return nd

    def run_sets(self, sp, canon=True, xormask=0, count_threshold=0.0, counts=True):
        """the exact k-mer sets, sorted on the device, through this sketcher's buffers -> as Context.kmer_sets_seqpack"""
        return _kmer_sets(self.ctx, lib().d2g_sketcher_run_sets, self._h, _Runs(sp, canon), xormask, count_threshold, counts)

    def run(self, sp, S, canon=True, xormask=0):
        r = _Runs(sp, canon)
        regs = np.empty((r.n, oph_m(S)), np.uint64)
        self.ctx._check(lib().d2g_sketcher_run(self._h, *r.args, xormask, S, _np_ptr(regs)))
        return regs

    def run_counts(self, sp, S, canon=True, xormask=0):
        """-> (regs u64 [n][m], counts u32 [n][m])"""
        r = _Runs(sp, canon)
        regs = np.empty((r.n, oph_m(S)), np.uint64)
        counts = np.empty((r.n, oph_m(S)), np.uint32)
        self.ctx._check(lib().d2g_sketcher_run_counts(self._h, *r.args, xormask, S, _np_ptr(regs), _np_ptr(counts)))
        return regs, counts

    def run_counts_ingested(self, runs, S, canon=True, xormask=0, k=None):
        """run_counts over the stream ingested last (packed == NULL)"""
        return self.run_counts(self._ingested(runs, k), S, canon, xormask)

    def run_mincount(self, sp, S, mincount, canon=True, xormask=0, counts=False):
        """registers over the k-mers seen at least `mincount` times (mincount < 2: run / run_counts) -> regs u64 [n][m], or
        (regs, counts u32 [n][m]) with counts=True"""
        r = _Runs(sp, canon)
        regs = np.empty((r.n, oph_m(S)), np.uint64)
        cnts = np.empty((r.n, oph_m(S)), np.uint32) if counts else None
        self.ctx._check(lib().d2g_sketcher_run_mincount(self._h, *r.args, xormask, S, mincount, _np_ptr(regs), _np_ptr(cnts)))
        return (regs, cnts) if counts else regs

    def run_mincount_ingested(self, runs, S, mincount, canon=True, xormask=0, counts=False, k=None):
        """run_mincount over the stream ingested last (packed == NULL)"""
        return self.run_mincount(self._ingested(runs, k), S, mincount, canon, xormask, counts)

    def run_bmh(self, sp, S, canon=True, xormask=0, count_threshold=0.0):
        r = _Runs(sp, canon)
        sig = np.empty((r.n, S), np.float64)
        tw = np.empty(r.n, np.float64)
        self.ctx._check(lib().d2g_sketcher_run_bmh(self._h, *r.args, xormask, S, count_threshold, _np_ptr(sig), _np_ptr(tw)))
        return sig, tw

    def run_bmh_cs(self, sp, S, cells, canon=True, xormask=0, count_threshold=0.0):
        """K3k through this sketcher's buffers, filter, window and alphabet -> as Context.bmh_sketch_cs_seqpack"""
        r = _Runs(sp, canon)
        sig = np.empty((r.n, S), np.float64)
        tw = np.empty(r.n, np.float64)
        self.ctx._check(lib().d2g_sketcher_run_bmh_cs(self._h, *r.args, xormask, S, cells, count_threshold, _np_ptr(sig), _np_ptr(tw)))
        return sig, tw

    # -- K0: FASTA bytes -> packed run stream on the GPU ------------------------------------------
    def ingest_fasta(self, buffers, k, genome_nfiles=None, pinned=None):
        """buffers: list of bytes-like FASTA inputs; genome_nfiles: files per genome (default one each).  The bytes are laid out
        16-byte aligned in ONE host buffer (`pinned`: a PinnedArray to reuse, else a plain numpy array) and parsed on the
        device.  Raises D2GError(D2G_ERR_UNSUPPORTED) for inputs only the host parser handles.
        -> (run_start u64, run_len u32, genome_run_off u64, genome_nkmers u64, nbases)"""
        nf = len(buffers)
        lens = np.array([len(b) for b in buffers], np.uint64)
        offs = np.zeros(nf, np.uint64)
        pos = 0
        for i in range(nf):
            offs[i] = pos
            pos += (int(lens[i]) + 15) // 16 * 16
        total = max(pos, 16)
        raw = pinned.array[:total] if pinned is not None else np.empty(total, np.uint8)
        for i, b in enumerate(buffers):
            raw[int(offs[i]):int(offs[i]) + int(lens[i])] = np.frombuffer(b, np.uint8)
        gn = np.ones(nf, np.uint64) if genome_nfiles is None else np.asarray(genome_nfiles, np.uint64)
        gfo = np.concatenate([[0], np.cumsum(gn)]).astype(np.uint64)
        n = gfo.size - 1
        self.ingest_raw(raw, pos, offs, lens, gfo, k)
        return self.ingested_runs(n)

    def ingest_raw(self, raw, raw_bytes, file_off, file_len, genome_file_off, k):
        file_off = np.ascontiguousarray(file_off, np.uint64)
        file_len = np.ascontiguousarray(file_len, np.uint64)
        genome_file_off = np.ascontiguousarray(genome_file_off, np.uint64)
        self.k = k
        self.ctx._check(lib().d2g_sketcher_ingest_fasta(self._h, _np_ptr(raw), raw_bytes, _np_ptr(file_off), _np_ptr(file_len), file_off.size,
                                                        _np_ptr(genome_file_off), genome_file_off.size - 1, k))

    def ingested_runs(self, n):
        rs, rl, go, nk = _vp(), _vp(), _vp(), _vp()
        nrun, nb = _sz(), _u64()
        self.ctx._check(lib().d2g_sketcher_ingested_runs(self._h, C.byref(rs), C.byref(rl), C.byref(nrun), C.byref(go), C.byref(nk), C.byref(nb)))
        nr = nrun.value

        def arr(p, cnt, dt):
            if not cnt:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(cnt * np.dtype(dt).itemsize,)).view(dt).copy()
        return arr(rs, nr, np.uint64), arr(rl, nr, np.uint32), arr(go, n + 1, np.uint64), arr(nk, n, np.uint64), int(nb.value)

    def run_ingested(self, runs, S, canon=True, xormask=0, k=None):
        """K1 over the stream ingested last (packed == NULL): -> regs u64 [n][m].  `runs` may be any run table inside the stream's
        extent, and k any k its runs allow (default: the k of the ingest)"""
        return self.run(self._ingested(runs, k), S, canon, xormask)

    def run_bmh_ingested(self, runs, S, canon=True, xormask=0, count_threshold=0.0):
        return self.run_bmh(self._ingested(runs, None), S, canon, xormask, count_threshold)

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_sketcher_destroy(self._h)
            self._h = None

    __del__ = close


class PinnedArray:
    """page-locked host bytes (d2g_malloc_host) as a numpy uint8 array: uploads from it are one DMA"""

    def __init__(self, ctx, nbytes):
        self.ctx, self._p = ctx, _vp()
        ctx._check(lib().d2g_malloc_host(ctx._h, nbytes, C.byref(self._p)))
        self.array = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            lib().d2g_free_host(self.ctx._h, self._p)
            self._p = None

    __del__ = close


class KmerFilter:
    """Device-resident set of the raw 2-bit k-mers of a filter input (d2g_kmer_filter)."""

    def __init__(self, ctx, h, k, canon):
        self.ctx, self._h, self.k, self.canon = ctx, h, k, canon

    def info(self):
        """-> (k-mer occurrences put in, distinct keys held, bytes of the device table); synchronises"""
        no, nd, tb = _u64(), _u64(), _sz()
        self.ctx._check(lib().d2g_kmer_filter_info(self.ctx._h, self._h, C.byref(no), C.byref(nd), C.byref(tb)))
        return int(no.value), int(nd.value), int(tb.value)

    def contains(self, kmers):
        """membership of raw 2-bit k-mers (canonical ones for a canon filter) through the device probe the walker uses -> bool [n]"""
        kmers = np.ascontiguousarray(kmers, np.uint64)
        out = np.zeros(kmers.size, np.uint8)
        self.ctx._check(lib().d2g_kmer_filter_contains(self.ctx._h, self._h, _np_ptr(kmers), kmers.size, _np_ptr(out)))
        return out.astype(bool)

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_kmer_filter_destroy(self._h)
            self._h = None

    __del__ = close


class Screen:
    """Device-resident k-mer database with rows of hit counters (d2g_screen)."""

    def __init__(self, ctx, h, nrefs, S, k, canon, nrows):
        self.ctx, self._h, self.nrefs, self.S, self.k, self.canon, self.nrows = ctx, h, nrefs, S, k, canon, nrows

    def info(self):
        """-> (distinct keys, bytes of the table, bytes of the counters)"""
        nd, tb, cb = _u64(), _sz(), _sz()
        self.ctx._check(lib().d2g_screen_info(self.ctx._h, self._h, C.byref(nd), C.byref(tb), C.byref(cb)))
        return int(nd.value), int(tb.value), int(cb.value)

    def reset(self):
        self.ctx._check(lib().d2g_screen_reset(self.ctx._h, self._h))

    def fed(self, row):
        n = _u64()
        self.ctx._check(lib().d2g_screen_fed(self.ctx._h, self._h, row, C.byref(n)))
        return int(n.value)

    def set_fed(self, row, nkmers):
        self.ctx._check(lib().d2g_screen_set_fed(self.ctx._h, self._h, row, nkmers))

    def add_dev(self, plan, packed_dev_ptr, genome_row, stream=None):
        rows = np.ascontiguousarray(genome_row, np.uint32)
        assert rows.size == plan.n
        self.ctx._check(lib().d2g_screen_add_dev(self.ctx._h, self._h, plan._h, packed_dev_ptr, _np_ptr(rows), stream))

    def result(self, row0=0, nrows=None):
        """-> (matches u32 [nrows][nrefs], matchsums u32 [nrows][nrefs]); synchronises"""
        nrows = self.nrows - row0 if nrows is None else nrows
        m = np.zeros((nrows, self.nrefs), np.uint32)
        s = np.zeros((nrows, self.nrefs), np.uint32)
        self.ctx._check(lib().d2g_screen_result(self.ctx._h, self._h, row0, nrows, _np_ptr(m), _np_ptr(s)))
        return m, s

    def key_counts(self, row):
        """-> (distinct masked keys u64 [D] ascending, the row's count of each u32 [D])"""
        D = self.info()[0]
        keys, cnt = np.zeros(D, np.uint64), np.zeros(D, np.uint32)
        self.ctx._check(lib().d2g_screen_key_counts(self.ctx._h, self._h, row, _np_ptr(keys), _np_ptr(cnt)))
        return keys, cnt

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_screen_destroy(self._h)
            self._h = None

    __del__ = close


class KSet:
    """Device-resident sorted exact k-mer sets with their slice table (d2g_kset)."""

    def __init__(self, ctx, h):
        self.ctx, self._h = ctx, h
        self.N = int(lib().d2g_kset_size(h))

    @property
    def device_bytes(self):
        return int(lib().d2g_kset_device_bytes(self._h))

    @property
    def slice_bits(self):
        return int(lib().d2g_kset_slice_bits(self._h))

    def isz_ut_dev(self, r0, r1, out_dev_ptr, stream=None):
        self.ctx._check(lib().d2g_kset_isz_ut_dev(self.ctx._h, self._h, r0, r1, out_dev_ptr, stream))

    def isz_rect_dev(self, a0, a1, b0, b1, out_dev_ptr, stream=None):
        self.ctx._check(lib().d2g_kset_isz_rect_dev(self.ctx._h, self._h, a0, a1, b0, b1, out_dev_ptr, stream))

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_kset_destroy(self._h)
            self._h = None

    __del__ = close


class SeqSet:
    """Device-resident records, recoded to dense symbol codes, for exact edit distances (d2g_seqset, K2h)."""

    def __init__(self, ctx, h):
        self.ctx, self._h = ctx, h
        self.N = int(lib().d2g_seqset_nrecords(h))

    @property
    def device_bytes(self):
        return int(lib().d2g_seqset_device_bytes(self._h))

    @property
    def alphabet_size(self):
        return int(lib().d2g_seqset_alphabet_size(self._h))

    @property
    def strip_blocks(self):
        return int(lib().d2g_seqset_strip_blocks(self.ctx._h, self._h))

    def edit_ut_dev(self, r0, r1, out_dev_ptr, stream=None):
        self.ctx._check(lib().d2g_edit_ut_dev(self.ctx._h, self._h, r0, r1, out_dev_ptr, stream))

    def edit_rect_dev(self, a0, a1, b0, b1, out_dev_ptr, stream=None):
        self.ctx._check(lib().d2g_edit_rect_dev(self.ctx._h, self._h, a0, a1, b0, b1, out_dev_ptr, stream))

    def edit_ut(self, r0=0, r1=None):
        """-> uint32[d2g_ut_count(N, r0, r1)] (host-pointer form; synchronises)"""
        r1 = self.N if r1 is None else r1
        out = np.zeros(ut_count(self.N, r0, r1), np.uint32)
        self.ctx._check(lib().d2g_edit_ut(self.ctx._h, self._h, r0, r1, _np_ptr(out)))
        return out

    def edit_rect(self, a0, a1, b0, b1):
        out = np.zeros((a1 - a0, b1 - b0), np.uint32)
        self.ctx._check(lib().d2g_edit_rect(self.ctx._h, self._h, a0, a1, b0, b1, _np_ptr(out)))
        return out

    def near_dev(self, T, close_dev_ptr, r0=0, r1=None, stream=None):
        """d2g_edit_near_dev: closeness T + 1 - min(d, T + 1) of rows [r0, r1) x all N columns, u32 row-major in device memory"""
        r1 = self.N if r1 is None else r1
        self.ctx._check(lib().d2g_edit_near_dev(self.ctx._h, self._h, r0, r1, T, close_dev_ptr, stream))

    def within_dev(self, rowcnt_dev_ptr, ids_dev_ptr, close_dev_ptr, cap, K=0, T=0, r0=0, r1=None, band_rows=0, stream=None):
        """d2g_edit_within_dev: per-row selection on the device over closeness (K == 0: every j with d <= T)"""
        r1 = self.N if r1 is None else r1
        self.ctx._check(lib().d2g_edit_within_dev(self.ctx._h, self._h, r0, r1, K, T, cap, rowcnt_dev_ptr, ids_dev_ptr, close_dev_ptr,
                                                  band_rows, stream))

    def knn(self, K=0, T=0, r0=0, r1=None, cap=0, band_rows=0):
        """d2g_edit_knn: CSR (indptr, indices, data) of rows [r0, r1), data = the distances as float32.  K == 0: every record within T
        edits; K >= 1: the K nearest of all records with every tie of the K-th (T is only the bound the search starts from)"""
        r1 = self.N if r1 is None else r1
        return _knn_csr(self.ctx, r1 - r0, K, lambda ip, ix, dt, oc, need: lib().d2g_edit_knn(
            self.ctx._h, self._h, r0, r1, K, T, cap, band_rows, ip, ix, dt, oc, need))

    def dedup_dev(self, assign_dev_ptr, T, band_rows=0, stream=None):
        """d2g_edit_dedup_dev: greedy clustering by edit distance; assign[i] = the representative of record i, u32 [N] in device memory"""
        self.ctx._check(lib().d2g_edit_dedup_dev(self.ctx._h, self._h, T, assign_dev_ptr, band_rows, stream))

    def dedup(self, T, band_rows=0):
        """d2g_edit_dedup -> uint32[N] (host-pointer form; synchronises)"""
        out = np.zeros(self.N, np.uint32)
        self.ctx._check(lib().d2g_edit_dedup(self.ctx._h, self._h, T, band_rows, _np_ptr(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_seqset_destroy(self._h)
            self._h = None

    __del__ = close


class SeqRecs:
    """FASTA/FASTQ -> raw records (d2g_seqrecs_*): the record walk of SeqPack.add_*_by_record, the sequence bytes kept as they are."""

    def __init__(self):
        self._h = None
        h = _vp()
        rc = lib().d2g_seqrecs_create(C.byref(h))
        if rc:
            raise D2GError(rc)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_seqrecs_destroy(self._h)
            self._h = None

    __del__ = close

    def add_path(self, path):
        rc = lib().d2g_seqrecs_add_path(self._h, os.fsencode(path))
        if rc:
            raise D2GError(rc, str(path))

    def add_fastx(self, buf):
        rc = lib().d2g_seqrecs_add_fastx(self._h, buf, len(buf))
        if rc:
            raise D2GError(rc, "add_fastx")

    @property
    def nrecords(self):
        return int(lib().d2g_seqrecs_nrecords(self._h))

    def name(self, g):
        return lib().d2g_seqrecs_name(self._h, g).decode()

    def arrays(self):
        """-> (bytes u8, off u64[n + 1]) as numpy copies"""
        n = self.nrecords
        off = np.ctypeslib.as_array(lib().d2g_seqrecs_off(self._h), shape=(n + 1,)).copy()
        nb = int(off[n])
        data = np.ctypeslib.as_array(lib().d2g_seqrecs_bytes(self._h), shape=(nb,)).copy() if nb else np.empty(0, np.uint8)
        return data, off

    def records(self):
        data, off = self.arrays()
        return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(self.nrecords)]


class OphPlan:
    def __init__(self, ctx, h, n):
        self.ctx, self._h, self.n = ctx, h, n

    def set_filter(self, filt):
        """attach a KmerFilter (None detaches): oph_sketch_dev, oph_count_dev and bmh_sketch_dev on this plan skip its k-mers"""
        self.ctx._check(lib().d2g_oph_plan_set_filter(self._h, filt._h if filt is not None else None))
        self._filter = filt

    @property
    def nkmers(self):
        return int(lib().d2g_oph_plan_nkmers(self._h))

    @property
    def nbases(self):
        return int(lib().d2g_oph_plan_nbases(self._h))

    def close(self):
        if self._h:
            lib().d2g_oph_plan_destroy(self._h)
            self._h = None

    __del__ = close


class IntervalPlan:
    def __init__(self, ctx, h, n):
        self.ctx, self._h, self.n = ctx, h, n

    @property
    def npositions(self):
        return int(lib().d2g_interval_plan_npositions(self._h))

    def runs(self, normalize=False):
        """the sweep behind --multiset (host only) -> (hash, lo, hi uint64[nruns], weight float64[nruns], run_off uint64[n + 1])"""
        off = np.zeros(self.n + 1, np.uint64)
        nr = _sz()
        self.ctx._check(lib().d2g_interval_runs(self._h, int(bool(normalize)), None, None, None, None, 0, _np_ptr(off), C.addressof(nr)))
        n = max(int(nr.value), 1)
        h, lo, hi, w = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.float64)
        self.ctx._check(lib().d2g_interval_runs(self._h, int(bool(normalize)), _np_ptr(h), _np_ptr(lo), _np_ptr(hi), _np_ptr(w), n, _np_ptr(off),
                                                C.addressof(nr)))
        k = int(nr.value)
        return h[:k], lo[:k], hi[:k], w[:k], off

    def close(self):
        if self._h:
            lib().d2g_interval_plan_destroy(self._h)
            self._h = None

    __del__ = close


class CmpSet:
    """Device-resident prepared signature matrix (d2g_cmp_set)."""

    def __init__(self, ctx, h, N, S, owned=True):
        self.ctx, self._h, self.N, self.S, self._owned = ctx, h, N, S, owned

    @property
    def algo(self):
        return int(lib().d2g_cmp_set_algo(self._h))

    @property
    def operand_bytes(self):
        return int(lib().d2g_cmp_set_operand_bytes(self._h))

    @property
    def id_bits(self):
        """width of the set's per-column id words: 16 or 32 (0: the set keeps no ids)"""
        return int(lib().d2g_cmp_set_id_bits(self._h))

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                lib().d2g_cmp_set_destroy(self._h)
            self._h = None

    __del__ = close

    def export_operand_dev(self, planes_out_ptr, meta_out_ptr, stream=None):
        self.ctx._check(lib().d2g_cmp_set_export_operand_dev(self.ctx._h, self._h, planes_out_ptr, meta_out_ptr, stream))

    def update_dev(self, dev_ptr, stream=None):
        self.ctx._check(lib().d2g_cmp_set_update_dev(self.ctx._h, self._h, dev_ptr, stream))

    def status(self, stream=None):
        """synchronises; raises D2GError(D2G_ERR_INTERNAL) if the asynchronous prepare overflowed"""
        self.ctx._check(lib().d2g_cmp_set_status(self.ctx._h, self._h, stream))

    def sparse_info(self, stream=None):
        """-> dict of the sparse path's last upper-triangle launch (synchronises)"""
        a = np.zeros(4, np.uint32)
        self.ctx._check(lib().d2g_cmp_set_sparse_info(self.ctx._h, self._h, stream, a.ctypes.data))
        return sparse_info_dict(a)

    def sparse_detail(self, stream=None):
        """-> dict of the last prepare's first look (its decision and raw sums), list form and schedule -- "classic", "merged" (column plan and planes
        inside launches of the ordering: D2G_K2_MERGE=1) or "planes-emit" (the planes behind the pair-list kernel's workgroups: D2G_K2_MERGE=2); "merge" is
        the same as the switch's number -- with the kernels it enqueued, the transpose included (synchronises; zeros without a sparse path)"""
        a = np.zeros(10, np.uint64)
        self.ctx._check(lib().d2g_cmp_set_sparse_detail(self.ctx._h, self._h, stream, a.ctypes.data))
        return {"looked": bool(a[0]), "looked_dense": bool(a[1]), "entries": int(a[2]), "family_pairs": int(a[3]), "shared_values": int(a[4]),
                "planes": int(a[5]), "binned": bool(a[6]), "bin_cshift": int(a[7]), "schedule": K2_SCHEDULES[min(int(a[8]), 2)], "merge": int(a[8]), "prepare_kernels": int(a[9])}

    def fill_detail(self):
        """-> dict of what became of the output announced to the last prepare, in 32 KB pieces: "announced", "rank" (written by the rank kernel's own
        threads), "riders" (carried by the prepare's other kernels), "launch" (left to the launch); host bookkeeping, nothing is synchronised"""
        a = np.zeros(4, np.uint64)
        self.ctx._check(lib().d2g_cmp_set_fill_detail(self.ctx._h, self._h, a.ctypes.data))
        return {"announced": int(a[0]), "rank": int(a[1]), "riders": int(a[2]), "launch": int(a[3])}

    def debug_pairs(self, cap=1 << 24, stream=None):
        """-> (pairs [n][2] uint32: the pair list of the last prepare (i < j), roots [N] uint32: the family root of every sketch)"""
        buf = np.empty(cap, np.uint64)
        roots = np.empty(self.N, np.uint32)
        n = _sz()
        self.ctx._check(lib().d2g_cmp_set_debug_pairs(self.ctx._h, self._h, stream, buf.ctypes.data, cap, C.byref(n), roots.ctypes.data))
        e = buf[:n.value]
        e = e[e != np.uint64(0xFFFFFFFFFFFFFFFF)]                     # empty slots (two outsiders of one value in one segment)
        return np.stack([(e & np.uint64(0xFFFFFFFF)).astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32)], axis=1), roots

    def planes(self, stream=None):
        """-> (max shared values per column + 1, max id planes of a group, mean id planes); zeros for DIRECT"""
        md, nb, mean = C.c_uint(), _int(), _f32()
        self.ctx._check(lib().d2g_cmp_set_planes(self.ctx._h, self._h, stream, C.byref(md), C.byref(nb), C.byref(mean)))
        return int(md.value), int(nb.value), float(mean.value)

    def eqcount_ut_dev(self, out_dev_ptr, r0=0, r1=None, stream=None):
        r1 = self.N if r1 is None else r1
        self.ctx._check(lib().d2g_cmp_eqcount_ut_dev(self.ctx._h, self._h, r0, r1, out_dev_ptr, stream))

    def lut_ut_dev(self, lut_dev_ptr, out_dev_ptr, r0=0, r1=None, stream=None):
        r1 = self.N if r1 is None else r1
        self.ctx._check(lib().d2g_cmp_lut_ut_dev(self.ctx._h, self._h, r0, r1, lut_dev_ptr, out_dev_ptr, stream))

    def prefill_ut_dev(self, out_dev_ptr, r0=0, r1=None, lut_dev_ptr=None, stream=None):
        """the fill of the NEXT upper-triangle launch into `out`, enqueued now on `stream` (counts when no table is given)"""
        r1 = self.N if r1 is None else r1
        if lut_dev_ptr is None:
            self.ctx._check(lib().d2g_cmp_ut_prefill_dev(self.ctx._h, self._h, r0, r1, out_dev_ptr, None, None, stream))
        else:
            self.ctx._check(lib().d2g_cmp_ut_prefill_dev(self.ctx._h, self._h, r0, r1, None, lut_dev_ptr, out_dev_ptr, stream))

    def forget(self):
        """the set's next prepare decides as the first prepare of a new set does (measurements)"""
        self.ctx._check(lib().d2g_cmp_set_forget(self.ctx._h, self._h))

    def announce_ut_dev(self, out_dev_ptr, r0=0, r1=None, lut_dev_ptr=None):
        """the output of the NEXT upper-triangle launch, told ahead of the update_dev that precedes it: the prepare carries the fill"""
        r1 = self.N if r1 is None else r1
        if lut_dev_ptr is None:
            self.ctx._check(lib().d2g_cmp_ut_announce_dev(self.ctx._h, self._h, r0, r1, out_dev_ptr, None, None))
        else:
            self.ctx._check(lib().d2g_cmp_ut_announce_dev(self.ctx._h, self._h, r0, r1, None, lut_dev_ptr, out_dev_ptr))

    def gtlt_ut_dev(self, gt_dev_ptr, lt_dev_ptr, r0=0, r1=None, stream=None):
        r1 = self.N if r1 is None else r1
        self.ctx._check(lib().d2g_cmp_gtlt_ut_dev(self.ctx._h, self._h, r0, r1, gt_dev_ptr, lt_dev_ptr, stream))

    def eqcount_rect_dev(self, out_dev_ptr, a0, a1, b0, b1, stream=None):
        self.ctx._check(lib().d2g_cmp_eqcount_rect_dev(self.ctx._h, self._h, a0, a1, b0, b1, out_dev_ptr, stream))

    def knn_dev(self, rowcnt_dev_ptr, ids_dev_ptr, counts_dev_ptr, cap, K=0, min_count=0, cls_dev_ptr=None, r0=0, r1=None,
                band_rows=0, stream=None):
        """d2g_cmp_knn_dev: per-row selection on the device (K == 0: threshold mode with min_count as the threshold)"""
        r1 = self.N if r1 is None else r1
        self.ctx._check(lib().d2g_cmp_knn_dev(self.ctx._h, self._h, r0, r1, K, min_count, cls_dev_ptr, cap, rowcnt_dev_ptr, ids_dev_ptr,
                                              counts_dev_ptr, band_rows, stream))

    def knn(self, lut, isdist=False, K=0, threshold=0.0, r0=0, r1=None, cap=0, band_rows=0):
        """d2g_cmp_set_knn: CSR (indptr, indices, data) of rows [r0,r1) for the value table lut[S+1]"""
        lut = np.ascontiguousarray(lut, np.float32)
        assert lut.size == self.S + 1
        r1 = self.N if r1 is None else r1
        return _knn_csr(self.ctx, r1 - r0, K, lambda ip, ix, dt, oc, need: lib().d2g_cmp_set_knn(
            self.ctx._h, self._h, r0, r1, _np_ptr(lut), int(bool(isdist)), K, float(threshold), cap, band_rows, ip, ix, dt, oc, need))

    def dedup_dev(self, assign_dev_ptr, min_count, cls_dev_ptr=None, band_rows=0, stream=None):
        """d2g_cmp_dedup_dev: greedy clustering of the whole set on the device, assign_dev_ptr = u32 [N]"""
        self.ctx._check(lib().d2g_cmp_dedup_dev(self.ctx._h, self._h, min_count, cls_dev_ptr, assign_dev_ptr, band_rows, stream))

    def dedup(self, lut, threshold, band_rows=0):
        """d2g_cmp_set_dedup: -> assign u32 [N] for the non-decreasing value table lut[S+1]"""
        lut = np.ascontiguousarray(lut, np.float32)
        assert lut.size == self.S + 1
        out = np.empty(self.N, np.uint32)
        self.ctx._check(lib().d2g_cmp_set_dedup(self.ctx._h, self._h, _np_ptr(lut), float(threshold), band_rows, _np_ptr(out)))
        return out

    def gtlt_rect_dev(self, gt_dev_ptr, lt_dev_ptr, a0, a1, b0, b1, stream=None):
        self.ctx._check(lib().d2g_cmp_gtlt_rect_dev(self.ctx._h, self._h, a0, a1, b0, b1, gt_dev_ptr, lt_dev_ptr, stream))

    # host-returning helpers built on the raw device-memory calls
    def eqcount_ut(self, r0=0, r1=None):
        r1 = self.N if r1 is None else r1
        out = np.empty(ut_count(self.N, r0, r1) if r0 <= r1 <= self.N else 0, np.uint32)
        d = self.ctx.malloc(max(out.nbytes, 4))
        try:
            self.eqcount_ut_dev(d, r0, r1)
            if out.size:
                self.ctx.d2h(out, d)
        finally:
            self.ctx.free(d)
        return out

    def gtlt_ut(self, r0=0, r1=None):
        r1 = self.N if r1 is None else r1
        n = ut_count(self.N, r0, r1)
        gt, lt = np.empty(n, np.uint32), np.empty(n, np.uint32)
        if n == 0:
            return gt, lt
        dg, dl = self.ctx.malloc(gt.nbytes), self.ctx.malloc(lt.nbytes)
        try:
            self.gtlt_ut_dev(dg, dl, r0, r1)
            self.ctx.d2h(gt, dg)
            self.ctx.d2h(lt, dl)
        finally:
            self.ctx.free(dg)
            self.ctx.free(dl)
        return gt, lt

    def gtlt_rect(self, a0, a1, b0, b1):
        gt, lt = np.empty((a1 - a0, b1 - b0), np.uint32), np.empty((a1 - a0, b1 - b0), np.uint32)
        if gt.size == 0:
            return gt, lt
        dg, dl = self.ctx.malloc(gt.nbytes), self.ctx.malloc(lt.nbytes)
        try:
            self.gtlt_rect_dev(dg, dl, a0, a1, b0, b1)
            self.ctx.d2h(gt, dg)
            self.ctx.d2h(lt, dl)
        finally:
            self.ctx.free(dg)
            self.ctx.free(dl)
        return gt, lt

    def eqcount_rect(self, a0, a1, b0, b1):
        out = np.empty((a1 - a0, b1 - b0), np.uint32)
        if out.size == 0:
            return out
        d = self.ctx.malloc(out.nbytes)
        try:
            self.eqcount_rect_dev(d, a0, a1, b0, b1)
            self.ctx.d2h(out, d)
        finally:
            self.ctx.free(d)
        return out

    def lut_ut(self, lut, r0=0, r1=None):
        r1 = self.N if r1 is None else r1
        lut = np.ascontiguousarray(lut, np.float32)
        out = np.empty(ut_count(self.N, r0, r1), np.float32)
        if out.size == 0:
            return out
        dl, d = self.ctx.malloc(lut.nbytes), self.ctx.malloc(out.nbytes)
        try:
            self.ctx.h2d(dl, lut)
            self.lut_ut_dev(dl, d, r0, r1)
            self.ctx.d2h(out, d)
        finally:
            self.ctx.free(dl)
            self.ctx.free(d)
        return out


# ---------------------------------------------------------------- multi-GPU (RCCL communicator + row-sharded engine)
COMM_ID_BYTES = 128


def comm_unique_id():
    """128 opaque bytes (ncclGetUniqueId) rank 0 hands to every rank"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().d2g_comm_unique_id(buf)
    if rc:
        raise D2GError(rc, "d2g_comm_unique_id (RCCL not loadable?)")
    return buf.raw


class Comm:
    def __init__(self, ctx, h):
        self.ctx, self._h = ctx, h

    @classmethod
    def create(cls, ctx, rank=0, world=1, unique_id=None):
        h = _vp()
        ctx._check(lib().d2g_comm_create(ctx._h, unique_id, rank, world, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def create_all(cls, ctxs):
        """one process, one communicator per context: RCCL clique over distinct devices, loopback transport otherwise"""
        n = len(ctxs)
        arr = (_vp * n)(*[c._h for c in ctxs])
        out = (_vp * n)()
        ctxs[0]._check(lib().d2g_comm_create_all(arr, n, out))
        return [cls(c, _vp(out[i])) for i, c in enumerate(ctxs)]

    rank = property(lambda self: int(lib().d2g_comm_rank(self._h)))
    world = property(lambda self: int(lib().d2g_comm_world(self._h)))
    is_rccl = property(lambda self: bool(lib().d2g_comm_is_rccl(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_comm_destroy(self._h)
            self._h = None

    __del__ = close


class AllPairs:
    """one rank of the row-sharded all-pairs engine (d2g_allpairs)"""

    def __init__(self, ctx, comm, N, S):
        self.ctx, self.comm, self.N, self.S = ctx, comm, N, S
        self._h = None
        h = _vp()
        ctx._check(lib().d2g_allpairs_create(ctx._h, comm._h, N, S, C.byref(h)))
        self._h = h
        a, b = _sz(), _sz()
        lib().d2g_allpairs_rows_held(h, C.byref(a), C.byref(b))
        self.rows_held = (a.value, b.value)
        lib().d2g_allpairs_rows_computed(h, C.byref(a), C.byref(b))
        self.rows_computed = (a.value, b.value)
        self.r0, self.r1 = self.rows_computed

    def prepare_dev(self, rows_ptr, stream=None):
        self.ctx._check(lib().d2g_allpairs_prepare_dev(self._h, rows_ptr, stream))

    def operand(self):
        """the gathered operand as a (non-owning) CmpSet"""
        return CmpSet(self.ctx, _vp(lib().d2g_allpairs_operand(self._h)), self.N, self.S, owned=False)

    def status(self, stream=None):
        """synchronises; raises if ANY rank's sharded prepare overflowed its rank table (results invalid everywhere)"""
        self.ctx._check(lib().d2g_allpairs_status(self._h, stream))

    @property
    def chunks(self):
        return lib().d2g_allpairs_chunks(self._h)

    PHASE_NAMES = ("pack", "x1", "prepare", "x2", "derive", "pair", "order", "fill")

    def set_phase_timing(self, on=True):
        """bracket every phase of the next prepare/step with timing events (switch off again for timed runs)"""
        self.ctx._check(lib().d2g_allpairs_set_phase_timing(self._h, int(bool(on))))

    def phase_times(self):
        """synchronises; -> [{"phase", "chunk", "start_ms", "ms"}] of the last step enqueued with phase timing on"""
        cap = 64
        kind, chunk = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        start, dur = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        n = _int()
        self.ctx._check(lib().d2g_allpairs_phase_times(self._h, cap, C.byref(n), kind.ctypes.data, chunk.ctypes.data,
                                                       start.ctypes.data, dur.ctypes.data))
        return [{"phase": self.PHASE_NAMES[int(kind[i])], "chunk": int(chunk[i]), "start_ms": float(start[i]), "ms": float(dur[i])}
                for i in range(n.value)]

    def sparse_info(self):
        """-> dict of the sparse-tile path in this rank's last pair phase (synchronises the device); keys as CmpSet.sparse_info"""
        a = np.zeros(4, np.uint32)
        self.ctx._check(lib().d2g_allpairs_sparse_info(self._h, a.ctypes.data))
        return sparse_info_dict(a)

    def step_lut_dev(self, rows_ptr, lut_ptr, out_ptr, stream=None):
        self.ctx._check(lib().d2g_allpairs_step_lut_dev(self._h, rows_ptr, lut_ptr, out_ptr, stream))

    def step_eqcount_dev(self, rows_ptr, out_ptr, stream=None):
        self.ctx._check(lib().d2g_allpairs_step_eqcount_dev(self._h, rows_ptr, out_ptr, stream))

    def enqueue_lut_dev(self, rows_ptr, lut_ptr, out_ptr, stream=None, input_ready=False):
        self.ctx._check(lib().d2g_allpairs_enqueue_lut_dev(self._h, rows_ptr, lut_ptr, out_ptr, stream, int(input_ready)))

    def close(self):
        if getattr(self, "_h", None):
            lib().d2g_allpairs_destroy(self._h)
            self._h = None

    __del__ = close


def allpairs_step_all(engs, rows_ptrs, lut_ptrs, out_ptrs, streams=None):
    """single-process multi-rank step: every collective phase is issued for all ranks inside one group"""
    n = len(engs)
    E = (_vp * n)(*[e._h for e in engs])
    R = (_vp * n)(*rows_ptrs)
    L = (_vp * n)(*lut_ptrs) if lut_ptrs is not None else None
    O = (_vp * n)(*out_ptrs)
    St = (_vp * n)(*(streams or [None] * n))
    engs[0].ctx._check(lib().d2g_allpairs_step_all(E, n, R, L, O, St))


def allpairs_prepare_all(engs, rows_ptrs, streams=None):
    n = len(engs)
    E = (_vp * n)(*[e._h for e in engs])
    R = (_vp * n)(*rows_ptrs)
    St = (_vp * n)(*(streams or [None] * n))
    engs[0].ctx._check(lib().d2g_allpairs_prepare_all(E, n, R, St))


def bcast_sigs(ctxs, comms, sig_bits_host):
    """-> list of device pointers (one per context) holding the whole matrix (d2g_bcast_sigs)"""
    a = np.ascontiguousarray(sig_bits_host, np.uint64)
    N, S = a.shape
    n = len(ctxs)
    Cx = (_vp * n)(*[c._h for c in ctxs])
    Cm = (_vp * n)(*[c._h for c in comms])
    out = (_vp * n)()
    ctxs[0]._check(lib().d2g_bcast_sigs(Cx, Cm, n, _np_ptr(a), N, S, out))
    return [int(out[i]) for i in range(n)]
