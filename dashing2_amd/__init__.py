"""dashing2_amd -- MI355X-native implementation of dashing2's two data-parallel hot paths.

The product is ``libd2g.so`` (hand-written HIP kernels for gfx950 + an x86 host half) behind
the C ABI declared in ``include/d2g.h``, and the ``dashing2`` drop-in CLI built from
``dashing2_amd/host``.  This Python package is only a thin ctypes mirror of that C ABI, used
by the tests, ``bench.py`` and the multi-GPU launcher (``dashing2_amd.dist``); it never
re-implements any part of the path and it fails loudly when the shared object is missing.
"""
from .capi import (  # noqa: F401
    D2GError, Context, CmpSet, SeqPack, Comm, AllPairs, lib, build, LIB_PATH,
    comm_unique_id, allpairs_step_all, allpairs_prepare_all, bcast_sigs,
    SIMILARITY, CONTAINMENT, SYMMETRIC_CONTAINMENT, POISSON_LLR, INTERSECTION, UNION_SIZE,
    CMP_AUTO, CMP_DIRECT, CMP_BITSLICE, CMP_PLANES, BITSLICE_OPS_PER_GROUP_EXTRA, TIME_K1, TIME_K2, TIME_K2PREP, TIME_K3, TIME_K0, PinnedArray,
    wang_hash, seed_mask, oph_xor_const, oph_m, oph_finalize, densify, epilogue_lut,
    epilogue_gtlt, epilogue_neq, host_epilogue_ut, operand_layout, sparse_bin_geometry, ut_count, ut_partition,
    regs_truncate, epilogue_trunc_neq, epilogue_trunc_gtlt, host_epilogue_trunc_ut, host_epilogue_trunc_rect,
    knn_finish, KnnOverflow, TIME_KNN, dedup_clusters, TIME_DEDUP, bmh_check_weights, wang_hash_inverse, oph_kmer_ids,
    KmerFilter, TIME_FILTER,
    Screen, TIME_SCREEN, epilogue_contain, screen_table_slots, SCREEN_MAX_KEYS, run_emissions,
    KSet, TIME_KSET, epilogue_exact, host_epilogue_exact_ut, host_epilogue_exact_rect, kset_check,
    ALPHABET_DNA, ALPHABET_PROTEIN20, ALPHABET_PROTEIN_3BIT, ALPHABET_PROTEIN_14, ALPHABET_PROTEIN_6,
    alphabet_size, alphabet_max_k, alphabet_code, alphabet_name, key_bits,
    countsketch_lds_cells,
    IntervalPlan, xxh3_64, bed_parse, XXH3_MAX_LEN,
    SeqSet, SeqRecs, TIME_EDIT, TIME_EDIT_NEAR, TIME_EDIT_DEDUP, EDIT_MAX_LEN, EDIT_BAND_MAX, seqset_check, seqset_recode_map,
)

__all__ = [
    "D2GError", "Context", "CmpSet", "SeqPack", "Comm", "AllPairs", "lib", "build", "LIB_PATH",
    "comm_unique_id", "allpairs_step_all", "allpairs_prepare_all", "bcast_sigs",
    "SIMILARITY", "CONTAINMENT", "SYMMETRIC_CONTAINMENT", "POISSON_LLR", "INTERSECTION", "UNION_SIZE",
    "CMP_AUTO", "CMP_DIRECT", "CMP_BITSLICE", "CMP_PLANES", "BITSLICE_OPS_PER_GROUP_EXTRA", "TIME_K1", "TIME_K2", "TIME_K2PREP", "TIME_K3", "TIME_K0", "PinnedArray",
    "wang_hash", "seed_mask", "oph_xor_const", "oph_m", "oph_finalize", "densify", "epilogue_lut",
    "epilogue_gtlt", "epilogue_neq", "host_epilogue_ut", "operand_layout", "sparse_bin_geometry", "ut_count", "ut_partition",
    "regs_truncate", "epilogue_trunc_neq", "epilogue_trunc_gtlt", "host_epilogue_trunc_ut", "host_epilogue_trunc_rect",
    "knn_finish", "KnnOverflow", "TIME_KNN", "dedup_clusters", "TIME_DEDUP", "bmh_check_weights", "wang_hash_inverse", "oph_kmer_ids",
    "KmerFilter", "TIME_FILTER",
    "Screen", "TIME_SCREEN", "epilogue_contain", "screen_table_slots", "SCREEN_MAX_KEYS", "run_emissions",
    "KSet", "TIME_KSET", "epilogue_exact", "host_epilogue_exact_ut", "host_epilogue_exact_rect", "kset_check",
    "ALPHABET_DNA", "ALPHABET_PROTEIN20", "ALPHABET_PROTEIN_3BIT", "ALPHABET_PROTEIN_14", "ALPHABET_PROTEIN_6",
    "alphabet_size", "alphabet_max_k", "alphabet_code", "alphabet_name", "key_bits",
    "countsketch_lds_cells",
    "IntervalPlan", "xxh3_64", "bed_parse", "XXH3_MAX_LEN",
    "SeqSet", "SeqRecs", "TIME_EDIT", "TIME_EDIT_NEAR", "TIME_EDIT_DEDUP", "EDIT_MAX_LEN", "EDIT_BAND_MAX", "seqset_check", "seqset_recode_map",
]
