"""ctypes binding of ``csrc/libmirge_native.so`` (C ABI: ``include/mirge_native.h``).

This is the whole boundary between the Python host code and the HIP kernels: plain pointers and
sizes, numpy buffers in and out.  There is no fallback: if the shared library is missing, or no
MI355X is visible, the first call raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import weakref
import os
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .seqio import FlatSeqs

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIRGE_NATIVE_SO: A/B builds of the same library when tuning kernels (never a different backend)
SO_PATH = os.environ.get("MIRGE_NATIVE_SO") or os.path.join(_HERE, "csrc", "libmirge_native.so")

# Every entry point of include/mirge_native.h, in the header's order and spelling without the parameter names (tests/test_ffi_signatures.py
# holds the two together): the one statement of the ABI on this side.  bind() turns it into restype / argtypes.
_PROTOTYPES = """
const char* mirge_last_error();
int mirge_device_count();
int mirge_ctx_create(int, void*, mirge_ctx**);
void mirge_ctx_destroy(mirge_ctx*);
int mirge_ctx_sync(mirge_ctx*);
int mirge_ctx_pool_stats(mirge_ctx*, int64_t*);
int mirge_lib_create(mirge_ctx*, const char*, const int64_t*, int64_t, mirge_lib**);
int mirge_lib_create_packed(mirge_ctx*, const uint64_t*, int64_t, const uint64_t*, int64_t, const uint32_t*, int64_t, uint64_t, int32_t, uint64_t, mirge_lib**);
int mirge_lib_packed_sizes(const mirge_lib*, int64_t*, int32_t*);
int mirge_lib_packed_copy(const mirge_lib*, uint64_t*, uint64_t*, uint32_t*);
void mirge_lib_destroy(mirge_lib*);
int64_t mirge_lib_n_refs(const mirge_lib*);
int64_t mirge_lib_device_bytes(const mirge_lib*);
int mirge_lib_prepare(mirge_lib*, int32_t);
int mirge_gz_inflate(const uint8_t*, int64_t, uint8_t*, int64_t, int64_t*, int32_t);
int mirge_gz_inflate_progress(const uint8_t*, int64_t, uint8_t*, int64_t, int64_t*, int32_t, int64_t*);
int mirge_reads_pack(mirge_ctx*, const char*, const int64_t*, int64_t, mirge_reads**);
int mirge_reads_parse(mirge_ctx*, const char*, int64_t, int32_t, int32_t, mirge_reads**, int64_t*);
int32_t mirge_reads_iupac_seen(const mirge_reads*);
int mirge_reads_parse_trim(mirge_ctx*, const char*, int64_t, int32_t, int32_t, const mirge_trim*, mirge_reads**, int64_t*);
int mirge_reads_parse_umi(mirge_ctx*, const char*, int64_t, int32_t, int32_t, const mirge_trim*, const mirge_umi*, mirge_reads**, int64_t*, mirge_reads**);
int mirge_umi_cluster(mirge_ctx*, const mirge_reads*, int32_t, int32_t, uint8_t*, int64_t*);
int mirge_umi_cluster_stats(int64_t*);
int mirge_kmer_correct(mirge_ctx*, const mirge_reads*, int32_t, int32_t, int32_t, mirge_reads**, uint32_t*, uint32_t*);
int mirge_kmer_correct_stats(int64_t*);
int mirge_kmer_correct_ratio(mirge_ctx*, const mirge_reads*, int32_t, int32_t, int32_t, int32_t, mirge_reads**, uint32_t*, uint32_t*);
int mirge_kmer_correct_ratio_stats(int64_t*);
int mirge_adapter_infer(mirge_ctx*, const mirge_reads*, mirge_adapter*, const uint32_t*, int64_t, uint64_t*, uint64_t*);
int mirge_reads_concat(mirge_ctx*, const mirge_reads* const*, int32_t, mirge_reads**);
void mirge_reads_destroy(mirge_reads*);
int64_t mirge_reads_count(const mirge_reads*);
int64_t mirge_reads_total_bases(const mirge_reads*);
int32_t mirge_reads_n_samples(const mirge_reads*);
int32_t mirge_reads_group_counts(const mirge_reads*, int64_t*, int32_t);
int mirge_reads_unpack(mirge_ctx*, const mirge_reads*, char*, int64_t*);
int mirge_collapse(mirge_ctx*, const mirge_reads*, const int32_t*, int32_t, mirge_reads**, int64_t*);
int mirge_collapse_weighted(mirge_ctx*, const mirge_reads*, const int32_t*, int32_t, const uint32_t*, mirge_reads**, int64_t*);
int mirge_collapse_merge(mirge_ctx*, const mirge_reads* const*, int32_t, mirge_reads**, int64_t*);
int mirge_collapse_fetch(mirge_ctx*, const mirge_reads*, uint32_t*, int64_t*);
int mirge_collapse_order(mirge_ctx*, const mirge_reads*, int64_t*);
int mirge_collapse_order_sorted(mirge_ctx*, const mirge_reads*, int64_t*);
int mirge_collapse_nonzero(mirge_ctx*, const mirge_reads*, int64_t*);
int mirge_reads_set_counts(mirge_ctx*, mirge_reads*, const uint32_t*, int32_t);
int mirge_cascade_run(mirge_ctx*, const mirge_reads*, const mirge_lib* const*, const mirge_policy*, int32_t, mirge_result**);
int mirge_cascade_prepare(mirge_ctx*, const mirge_reads*, const mirge_lib* const*, const mirge_policy*, int32_t);
int mirge_cascade_walks(mirge_ctx*, int32_t*);
int mirge_cascade_wg_times(mirge_ctx*, uint32_t*, int32_t, int32_t*, int32_t*);
int mirge_collapse_cascade(mirge_ctx*, const mirge_reads*, const mirge_lib* const*, const mirge_policy*, int32_t, mirge_reads**, int64_t*, mirge_result**);
int mirge_result_fetch(mirge_ctx*, const mirge_result*, int8_t*, int32_t*, int32_t*, int8_t*);
void mirge_result_destroy(mirge_result*);
int mirge_count_join(mirge_ctx*, const mirge_reads*, const mirge_result*, int32_t, int32_t, int64_t, int64_t*, int64_t*, int64_t*);
int mirge_count_join_host(mirge_ctx*, const int8_t*, const int32_t*, const uint32_t*, int64_t, int32_t, int32_t, int32_t, int32_t, int64_t, int64_t*, int64_t*, int64_t*);
int mirge_annotation_csv(const char*, const char*, const char*, const char*, const int64_t*, const int8_t*, const int32_t*, const uint32_t*, int32_t, const int64_t*,
    int64_t, int32_t, const int32_t*, int32_t, const char* const*, const int64_t* const*, const int64_t*);
int mirge_annotation_csv_device(mirge_ctx*, const mirge_reads*, const mirge_result*, const char*, const char*, const char*, const int64_t*, int64_t, int32_t,
    const int32_t*, int32_t, const char* const*, const int64_t* const*, const int64_t*);
int mirge_reads_range_sample(mirge_ctx*, const mirge_reads*, int32_t, uint64_t*);
int mirge_reads_range_split(mirge_ctx*, const mirge_reads*, const uint64_t*, int32_t, char*, int64_t*, uint32_t*, int64_t*);
int mirge_annotation_csv_device_sizes(mirge_ctx*, const mirge_reads*, const mirge_result*, const int64_t*, int64_t, int32_t, const int32_t*, int32_t, const char* const*,
    const int64_t* const*, const int64_t*, int64_t*);
int mirge_annotation_csv_device_at(mirge_ctx*, const mirge_reads*, const mirge_result*, const char*, const char*, int64_t, int64_t, const int64_t*, int64_t, int32_t,
    const int32_t*, int32_t, const char* const*, const int64_t* const*, const int64_t*);
int mirge_variant_tally(mirge_ctx*, const mirge_reads*, const mirge_result*, int32_t, int32_t, const int32_t*, int64_t, const char*, const int64_t*, int64_t,
    const uint8_t*, const double*, int64_t*, int64_t*, int8_t*, int8_t*);
int mirge_isomir_type(mirge_ctx*, const mirge_reads*, const mirge_result*, int32_t, int32_t, const int32_t*, int64_t, const char*, const int32_t*, const int32_t*,
    const int32_t*, int64_t, const char*, const int32_t*, int64_t, const int32_t*, int64_t, void*);
int mirge_gff_write(const char*, const char*, const char*, const void*, int64_t, const char*, const int64_t*, const uint32_t*, int32_t, const int32_t*, const char*,
    const int64_t*, int64_t, const int32_t*, const char*, const int64_t*, int64_t, const int64_t*, int64_t);
int mirge_gff_write_device(mirge_ctx*, const mirge_reads*, const mirge_result*, int32_t, int32_t, const int32_t*, int64_t, const char*, const int32_t*, const int32_t*,
    const int32_t*, int64_t, const char*, const int32_t*, int64_t, const int32_t*, const char*, const int64_t*, int64_t, const int32_t*, const char*, const int64_t*,
    int64_t, const int64_t*, const char*, const char*, const char*, int64_t*);
int mirge_genome_create(mirge_ctx*, const char*, const int64_t*, int64_t, mirge_genome**);
int mirge_genome_create_packed(mirge_ctx*, const uint8_t*, int64_t, const uint64_t*, const uint64_t*, const uint8_t*, int64_t, mirge_genome**);
void mirge_genome_destroy(mirge_genome*);
int mirge_genome_align_counts(mirge_ctx*, const mirge_genome*, const char*, const int64_t*, int64_t, int32_t, int32_t, int32_t, int32_t, int32_t, uint32_t*);
int mirge_genome_align_loci(mirge_ctx*, const mirge_genome*, const char*, const int64_t*, int64_t, int32_t, int32_t, int32_t, int32_t, int32_t, int64_t, int32_t,
    uint64_t*, mirge_loci**);
int mirge_genome_align_loci_strata(mirge_ctx*, const mirge_genome*, const char*, const int64_t*, int64_t, int32_t, int32_t, int32_t, int32_t, int32_t, int64_t, int32_t,
    int32_t, uint64_t*, mirge_loci**);
int64_t mirge_loci_count(const mirge_loci*);
int mirge_loci_fetch(const mirge_loci*, uint32_t*, uint32_t*, uint64_t*, uint8_t*, uint8_t*);
void mirge_loci_destroy(mirge_loci*);
int mirge_loci_cluster(mirge_ctx*, int64_t, const uint32_t*, const uint64_t*, const uint8_t*, const uint32_t*, int64_t, const int32_t*, const int64_t*, int64_t,
    const uint8_t*, int32_t, int32_t, int32_t*, int64_t*, uint32_t*, uint8_t*, uint64_t*, uint64_t*, int64_t*, uint32_t*);
int mirge_cluster_diagonals(mirge_ctx*, const char*, const int64_t*, int64_t, const char*, const int64_t*, int64_t, const uint32_t*, int32_t*, int32_t*, int32_t*,
    uint8_t*);
int mirge_cluster_pileup(mirge_ctx*, const char*, const int64_t*, int64_t, const int64_t*, const int64_t*, int64_t, const int32_t*, const int64_t*, int32_t*, int32_t*,
    int64_t*, int64_t*, int64_t);
int mirge_genome_fetch(mirge_ctx*, const mirge_genome*, int64_t, const uint32_t*, const int64_t*, const int64_t*, const uint8_t*, const uint8_t*, const int64_t*, char*);
int mirge_sam_write_device(mirge_ctx*, const mirge_reads*, const mirge_result*, const int64_t*, int32_t, const int32_t*, int32_t, const mirge_sam_pass*, int32_t,
    const char*, const char*, int64_t, int64_t*, int64_t*);
int mirge_bam_write_device(mirge_ctx*, const mirge_reads*, const mirge_result*, const int64_t*, int32_t, const int32_t*, int32_t, const mirge_sam_pass*, int32_t,
    const int32_t*, const int64_t*, int32_t, const char*, const char*, const char*, int64_t, int32_t, int64_t*, int64_t*, int64_t*);
int mirge_bam_huffman_probe(mirge_ctx*, const uint32_t*, int32_t, int32_t, uint8_t*);
int mirge_coverage_runs(mirge_ctx*, int64_t, const int32_t*, const int64_t*, const int32_t*, const uint32_t*, const uint8_t*, int32_t, uint8_t*, int32_t*, int64_t*,
    int64_t*, int64_t*, int64_t*);
int mirge_coverage_write_device(mirge_ctx*, const mirge_reads*, const mirge_result*, const int64_t*, int32_t, const int32_t*, int32_t, const mirge_sam_pass*, int32_t,
    const int32_t*, const int64_t*, int32_t, const char*, const int64_t*, int32_t, const char*, const char*, int64_t*, int64_t*, int64_t*, int64_t*, int64_t*);
int mirge_bigwig_from_intervals(mirge_ctx*, int64_t, const int32_t*, const int64_t*, const int32_t*, const uint32_t*, const uint8_t*, int32_t, int32_t, const char*,
    const int64_t*, const int64_t*, const int32_t*, const char*, const char*, int64_t*, int64_t*);
int mirge_bigwig_write_device(mirge_ctx*, const mirge_reads*, const mirge_result*, const int64_t*, int32_t, const int32_t*, int32_t, const mirge_sam_pass*, int32_t,
    const int32_t*, const int64_t*, int32_t, const char*, const int64_t*, const int64_t*, const int32_t*, int32_t, const char*, const char*, int64_t*, int64_t*);
int mirge_bgzf_write(mirge_ctx*, const uint8_t*, int64_t, int64_t, const char*, const char*, int64_t*);
int mirge_sam_write_device_bgzf(mirge_ctx*, const mirge_reads*, const mirge_result*, const int64_t*, int32_t, const int32_t*, int32_t, const mirge_sam_pass*, int32_t,
    const char*, const char*, int64_t, int64_t*, int64_t*, const char*, int64_t, int64_t*);
int mirge_coverage_write_device_bgzf(mirge_ctx*, const mirge_reads*, const mirge_result*, const int64_t*, int32_t, const int32_t*, int32_t, const mirge_sam_pass*,
    int32_t, const int32_t*, const int64_t*, int32_t, const char*, const int64_t*, int32_t, const char*, const char*, int64_t*, int64_t*, int64_t*, int64_t*, int64_t*,
    const char*, const char*, int64_t, int64_t*);
int mirge_trf_hits_run(mirge_ctx*, const mirge_reads*, const mirge_result*, int32_t, const mirge_lib*, const mirge_policy*, int32_t, const mirge_lib*,
    const mirge_policy*, const int64_t*, int64_t, const int32_t*, mirge_trf_hits**);
int64_t mirge_trf_hits_count(const mirge_trf_hits*);
int mirge_trf_hits_fetch(const mirge_trf_hits*, uint32_t*, uint32_t*, int32_t*, uint8_t*, uint8_t*, uint8_t*);
void mirge_trf_hits_destroy(mirge_trf_hits*);
int mirge_trf_assign(mirge_ctx*, const mirge_reads*, const mirge_result*, int64_t, const int64_t*, const int32_t*, const int32_t*, int64_t, const int64_t*, int64_t,
    const int64_t*, const char*, const int32_t*, const int32_t*, const int32_t*, int32_t*, int32_t*);
int mirge_trf_row_counts(mirge_ctx*, const mirge_reads*, const int64_t*, int64_t, uint32_t*);
int mirge_trf_cluster(mirge_ctx*, const mirge_reads*, int64_t, const int64_t*, const int64_t*, const int32_t*, const double*, const int32_t*, int64_t, const double*,
    float*, float*, int32_t*, int32_t*, int32_t*, int32_t*, int32_t*, int32_t*);
int mirge_qc_create(mirge_ctx*, mirge_qc**);
void mirge_qc_destroy(mirge_qc*);
int mirge_reads_parse_trim_qc(mirge_ctx*, const char*, int64_t, int32_t, int32_t, const mirge_trim*, mirge_qc*, mirge_reads**, int64_t*);
int mirge_qc_fetch(mirge_ctx*, const mirge_qc*, int64_t*, int32_t*);
int mirge_qc_class_profile(mirge_ctx*, const mirge_reads*, const mirge_result*, int32_t, int64_t*);
int mirge_fqout_create(mirge_ctx*, const char*, const char*, int64_t, mirge_fqout**);
int mirge_reads_parse_trim_out(mirge_ctx*, const char*, int64_t, int32_t, int32_t, const mirge_trim*, mirge_qc*, mirge_fqout*, mirge_reads**, int64_t*);
int mirge_fqout_finish(mirge_ctx*, mirge_fqout*, int64_t*);
void mirge_fqout_destroy(mirge_fqout*);
int mirge_nearest_scan(mirge_ctx*, const char*, const int64_t*, int64_t, const char*, const int64_t*, int64_t, int32_t*, int32_t*, int32_t*, int32_t*);
int mirge_nearest_unmapped(mirge_ctx*, const mirge_reads*, const mirge_result*, const char*, const int64_t*, int64_t, int32_t, mirge_nearest**);
int64_t mirge_nearest_count(const mirge_nearest*);
int mirge_nearest_fetch(const mirge_nearest*, uint32_t*, int32_t*, int32_t*, int32_t*, int32_t*);
int mirge_nearest_stats(const mirge_nearest*, int64_t*);
void mirge_nearest_destroy(mirge_nearest*);
int mirge_ctx_timer_start(mirge_ctx*);
int mirge_ctx_timer_stop(mirge_ctx*, double*);
int mirge_ctx_profile_enable(mirge_ctx*, int32_t);
int mirge_ctx_profile_only(mirge_ctx*, const char*);
int mirge_ctx_profile_units(mirge_ctx*, int32_t);
int mirge_ctx_profile_reset(mirge_ctx*);
int32_t mirge_ctx_profile_count(mirge_ctx*);
int mirge_ctx_profile_get(mirge_ctx*, int32_t, char*, int32_t, int64_t*, double*, double*);
"""
# name -> (return type, parameter types)
SIGNATURES = {name: (ret, tuple(params.split(", ")) if params else ())
              for ret, name, params in re.findall(r"(\S[^;()]*?) (mirge_\w+)\(([^)]*)\);", " ".join(_PROTOTYPES.split()))}
EXPORTS = list(SIGNATURES)


class MirgePolicy(C.Structure):
    """``mirge_policy`` of include/mirge_native.h."""
    _fields_ = [(n, C.c_int32) for n in (
        "mode", "mm", "seedlen", "maxtotal", "trim5", "trim3", "ttail", "len_lt", "len_gt", "reserved")]


class MirgeTrim(C.Structure):
    """``mirge_trim`` of include/mirge_native.h: the cutadapt modifier chain of digest.py:59-101."""
    _fields_ = [("nextseq_cutoff", C.c_int32), ("quality_front", C.c_int32), ("quality_back", C.c_int32),
                ("phred_base", C.c_int32), ("adapter", C.c_char_p), ("adapter_len", C.c_int32), ("min_overlap", C.c_int32),
                ("error_rate", C.c_double), ("trim_n", C.c_int32), ("n_cut", C.c_int32), ("cut", C.c_int32 * 2),
                ("count_per_modifier", C.c_int32), ("adapter_front", C.c_int32), ("adapter2", C.c_char_p),
                ("adapter2_len", C.c_int32), ("adapter2_front", C.c_int32), ("times", C.c_int32), ("no_indels", C.c_int32),
                ("match_read_wildcards", C.c_int32), ("no_adapter_wildcards", C.c_int32), ("action_none", C.c_int32),
                ("adapter_anchored", C.c_int32), ("adapter2_anchored", C.c_int32), ("linked", C.c_int32), ("linked_required", C.c_int32)]

    @staticmethod
    def make(adapter: Optional[str] = None, quality_back: int = -1, quality_front: int = 0, nextseq: int = -1,
             phred_base: int = 33, min_overlap: int = 3, error_rate: float = 0.12, trim_n: bool = False,
             cut: Sequence[int] = (), count_per_modifier: bool = True, front: bool = False,
             adapter2: Optional[str] = None, front2: bool = False, times: int = 1, indels: bool = True,
             read_wildcards: bool = False, adapter_wildcards: bool = True, action: str = "trim",
             anchored: bool = False, anchored2: bool = False, linked: bool = False, front_required: bool = True,
             back_required: bool = False) -> "MirgeTrim":
        t = MirgeTrim()
        t.nextseq_cutoff, t.quality_front, t.quality_back, t.phred_base = nextseq, quality_front, quality_back, phred_base
        a = adapter.encode() if adapter else None
        t.adapter, t.adapter_len = a, (len(a) if a else 0)
        t.min_overlap, t.error_rate, t.trim_n = min_overlap, error_rate, 1 if trim_n else 0
        cut = [int(x) for x in cut]
        t.n_cut = len(cut)
        for k, v in enumerate(cut[:2]):
            t.cut[k] = v
        t.count_per_modifier = 1 if count_per_modifier else 0
        t.adapter_front = 1 if front else 0
        a2 = adapter2.encode() if adapter2 else None
        t.adapter2, t.adapter2_len, t.adapter2_front = a2, (len(a2) if a2 else 0), 1 if front2 else 0
        t.times, t.no_indels = int(times), 0 if indels else 1
        t.match_read_wildcards, t.no_adapter_wildcards = 1 if read_wildcards else 0, 0 if adapter_wildcards else 1
        if action not in ("trim", "none"):
            raise NotImplementedError("--action mask / lowercase change the letters of a read, not its bounds: not part of the MI355X path")
        t.action_none = 1 if action == "none" else 0
        t.adapter_anchored, t.adapter2_anchored = 1 if anchored else 0, 1 if anchored2 else 0
        t.linked = 1 if linked else 0
        t.linked_required = (1 if front_required else 0) | (2 if back_required else 0)
        return t


class MirgeUmi(C.Structure):
    """``mirge_umi`` of include/mirge_native.h: ``-umi f,b`` [``--qiagenumi``] [``-udd``] (digest.py:164-205,305-315,334-365)."""
    _fields_ = [("front", C.c_int32), ("back", C.c_int32), ("qiagen", C.c_int32), ("dedup", C.c_int32)]

    @staticmethod
    def make(front: int, back: int, qiagen: bool = False, dedup: bool = False, cluster: Optional[str] = None) -> "MirgeUmi":
        """``cluster="directional"`` (with ``dedup``): ``--umi-cluster directional``, ``dedup == 2`` in the struct"""
        if cluster not in (None, "none", "directional"):
            raise ValueError(f"cluster={cluster!r}: None or 'directional'")
        directional = cluster == "directional"
        if directional and not dedup:
            raise ValueError("cluster='directional' needs dedup (-udd)")
        if directional and not 1 <= int(front) + int(back) <= 32:
            raise ValueError("cluster='directional' takes UMIs of 1 to 32 letters (front + back)")
        u = MirgeUmi()
        u.front, u.back, u.qiagen, u.dedup = int(front), int(back), 1 if qiagen else 0, (2 if directional else 1) if dedup else 0
        return u

    @property
    def cluster(self) -> Optional[str]:
        return "directional" if self.dedup == 2 else None


class SamPass(C.Structure):
    """``mirge_sam_pass`` of include/mirge_native.h"""
    _fields_ = [("lib", C.c_void_p), ("trim5", C.c_int32), ("trim3", C.c_int32), ("n_refs", C.c_int64), ("chrom_of_ref", C.c_void_p),
                ("minus", C.c_void_p), ("seg_ptr", C.c_void_p), ("seg_s", C.c_void_p), ("seg_e", C.c_void_p), ("cds_lo", C.c_void_p),
                ("cds_hi", C.c_void_p), ("n_chrom", C.c_int64), ("chrom_data", C.c_void_p), ("chrom_off", C.c_void_p)]


class MirgeAdapter(C.Structure):
    """``mirge_adapter`` of include/mirge_native.h: what ``mirge_adapter_infer`` found (``-a auto``)"""
    _fields_ = [("seq", C.c_char * 40), ("len", C.c_int32), ("left_steps", C.c_int32), ("spread", C.c_int32), ("pad", C.c_int32),
                ("support", C.c_uint64), ("eligible", C.c_uint64), ("seed_sum", C.c_uint64), ("candidates", C.c_uint64),
                ("seed", C.c_uint32), ("start", C.c_uint32)]

    FIELDS = ("seq", "len", "left_steps", "spread", "support", "eligible", "seed_sum", "candidates", "seed", "start")

    def as_dict(self) -> dict:
        return {k: (self.seq.decode() if k == "seq" else int(getattr(self, k))) for k in self.FIELDS}


_SCALARS = {"void": None, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
_STRUCTS = {"mirge_policy": MirgePolicy, "mirge_trim": MirgeTrim, "mirge_umi": MirgeUmi, "mirge_sam_pass": SamPass,
            "mirge_adapter": MirgeAdapter}
_ELEMENTS = {"char": "uint8", "void": None, "float": "float32", "double": "float64",
             **{t + "_t": t for t in ("int8", "uint8", "int32", "uint32", "int64", "uint64")}}  # C element type -> dtype (None: any)


class _ArrayPtr:
    """The ``argtypes`` entry of a pointer to numbers or bytes: None (NULL); a numpy array of exactly the element type (``void``: any),
    C-contiguous and, unless the pointer is const, writeable; ``bytes`` for a const pointer to bytes; else whatever ``c_void_p``
    takes -- a ``c_void_p``, ``byref(x)``, a ctypes array -- unchecked."""

    def __init__(self, ctype: str, elem: str, const: bool):
        self.ctype, self.dtype, self.const = ctype, _ELEMENTS[elem] and np.dtype(_ELEMENTS[elem]), const
        self.bytes_ok = const and elem in ("char", "uint8_t", "void")

    def from_param(self, a):
        if isinstance(a, np.ndarray):
            flags = a.flags
            if (self.dtype is not None and a.dtype != self.dtype) or not flags.c_contiguous or not (self.const or flags.writeable):
                raise TypeError(f"{self.ctype} takes a C-contiguous{'' if self.const else ', writeable'} array of dtype "
                                f"{'any' if self.dtype is None else self.dtype.name}; this one is {a.dtype.name}")
            return C.c_void_p(a.ctypes.data)
        if isinstance(a, str) or (isinstance(a, bytes) and not self.bytes_ok):
            raise TypeError(f"{self.ctype} takes no {type(a).__name__}")
        return C.c_void_p.from_param(a)


@functools.lru_cache(maxsize=None)
def _ctype(t: str):
    """the ctypes type of a parameter or return type as the header spells it (one object per spelling)"""
    elem = t.replace("const ", "").split("*")[0]
    if "*" not in t:
        return _SCALARS[t]
    if t.count("*") > 1 or (elem.startswith("mirge_") and elem not in _STRUCTS):
        return C.c_void_p  # opaque handles, out-handles and arrays of pointers
    return C.POINTER(_STRUCTS[elem]) if elem in _STRUCTS else _ArrayPtr(t, elem, t.startswith("const "))  # (KeyError: a type of no kind)


def bind(lib: C.CDLL) -> C.CDLL:
    """Declare ``restype`` and ``argtypes`` of every entry point of SIGNATURES that ``lib`` has; one it lacks (an older A/B build named
    by MIRGE_NATIVE_SO) is skipped and fails when it is called."""
    for name, (ret, params) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = C.c_char_p if ret == "const char*" else _ctype(ret)
            fn.argtypes = [_ctype(t) for t in params]
    return lib


_lib = None
_live = []  # weak references to every wrapper, closed in dependency order at interpreter exit


def load() -> C.CDLL:
    """Load the shared library (once).  Raises if it was not built -- there is no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  mirge3.0_amd has no CPU fallback.")
    _lib = bind(C.CDLL(SO_PATH))
    return _lib


def _track(obj):
    _live.append(weakref.ref(obj))
    if len(_live) > 4096:  # long-running callers create two handles per sample: drop the dead references
        _live[:] = [r for r in _live if r() is not None]


def _shutdown():
    """Close device handles before the interpreter and the HIP runtime tear down: result/read sets,
    then libraries, then contexts (a handle freed after its context is gone would crash at exit)."""
    objs = [r() for r in _live]
    objs = [o for o in objs if o is not None]
    for kind in (CascadeResult, ReadQc, TrimmedOut, DeviceReads, DeviceLibrary, DeviceGenome, Context):
        for o in objs:
            if isinstance(o, kind):
                try:
                    o.close()
                except Exception:
                    pass


import atexit  # noqa: E402
atexit.register(_shutdown)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().mirge_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def gz_inflate(data, threads: int = 0) -> Optional[np.ndarray]:
    """The text of a whole .gz file (``data``: its bytes) inflated on all host cores (``mirge_gz_inflate``), or None when the
    file is not of a kind that route takes -- the caller then inflates it serially.  Verified against the file's CRC-32."""
    buf = np.frombuffer(data, dtype=np.uint8)
    if buf.size < 18:
        return None
    isize = int.from_bytes(bytes(buf[-4:]), "little")  # the LAST member's length mod 2^32: exact for a one-member file below 4 GiB
    # room: that length, or -- the file may hold several members (merged lanes, BGZF), whose lengths only the members know --
    # twelve times the compressed size (FASTQ deflates 4-6 x; untouched pages of the buffer cost nothing).  Too little room is
    # reported (-2) and the caller streams the file instead.
    cap = max(isize, 12 * buf.size) + 65536
    if cap > (1 << 37):
        return None
    try:
        out = np.empty(cap, dtype=np.uint8)
    except MemoryError:  # (a host that does not overcommit): the streamed route needs pieces only
        return None
    n = C.c_int64(0)
    rc = load().mirge_gz_inflate(buf, buf.size, out, cap, C.byref(n), threads or gz_threads())
    if rc != 0:
        return None
    return out[: n.value]


# The text buffer of the last finished GzInflation, kept for the next one: a fresh buffer costs a sample its page faults while it
# inflates (the inflater's floor, profiles/README.md round 4) and an munmap of half a gigabyte when it is dropped -- 0.03-0.05 s of
# a 0.15 s sample.  One buffer, at most MIRGE_GZ_KEEP_BYTES (default 16 GiB of address space; what a sample touched stays resident).
_gz_kept: list = []          # (popped and appended by read-ahead threads: list.pop / append are atomic, the emptiness test is not)
_GZ_KEEP_BYTES = int(os.environ.get("MIRGE_GZ_KEEP_BYTES", str(16 << 30)))
import threading as _threading
_gz_keep_lock = _threading.Lock()


def gz_threads() -> int:
    """host threads one inflation takes: MIRGE_GZ_THREADS, else the cores divided among the ranks of this node (one process per GPU:
    eight samples inflate side by side), at most 64 (beyond, nothing is gained)"""
    env = os.environ.get("MIRGE_GZ_THREADS")
    if env:
        return max(1, int(env))
    ranks = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1))
    return max(1, min(64, (os.cpu_count() or 1) // ranks))


class GzInflation:
    """``mirge_gz_inflate_progress`` running on a thread of its own: ``out[:done()]`` is text that will not change any more, whole
    before ``wait()`` returns -- True when the file was inflated and its CRC-32 matched, False when this route does not take the
    file (then whatever was read ahead must be dropped and the file inflated the serial way)."""

    def __init__(self, data, threads: int = 0):
        import threading
        self.buf = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        self.out = None
        self.ok = None
        self._n = C.c_int64(0)
        self._progress = C.c_int64(0)
        self._thread = None
        if self.buf.size < 18:
            self.ok = False
            return
        isize = int.from_bytes(bytes(self.buf[-4:]), "little")
        cap = max(isize, 12 * int(self.buf.size)) + 65536  # (see gz_inflate)
        if cap > (1 << 37):
            self.ok = False
            return
        try:
            kept = _gz_kept.pop()
        except IndexError:  # none kept, or another read-ahead thread took it between a test and the pop
            kept = None
        if kept is not None and kept.size >= cap:
            self.out = kept
            cap = int(kept.size)
        else:
            del kept
            try:
                self.out = np.empty(cap, dtype=np.uint8)
            except MemoryError:
                self.ok = False
                return
        lib = load()

        def run():
            rc = lib.mirge_gz_inflate_progress(self.buf, self.buf.size, self.out, cap, C.byref(self._n), threads or gz_threads(),
                                               C.byref(self._progress))
            self.ok = rc == 0

        # (not a daemon: the interpreter waits for it at exit -- a fraction of a second -- instead of freeing the buffers under it)
        self._thread = threading.Thread(target=run, name="mirge-gz-inflate", daemon=False)
        self._thread.start()

    def done(self) -> int:
        """bytes of ``out`` that are final so far"""
        return int(self._progress.value)

    def running(self) -> bool:
        return self._thread is not None and self._thread.is_alive()

    def wait(self) -> bool:
        if self._thread is not None:
            self._thread.join()
        return bool(self.ok)

    def text(self) -> np.ndarray:
        """the whole text (after ``wait()`` returned True)"""
        return self.out[: self._n.value]

    def release(self):
        """the caller is done with ``out`` and every view of it: the buffer is kept for the next inflation"""
        self.wait()
        out, self.out = self.out, None
        if out is not None and out.size <= _GZ_KEEP_BYTES:
            with _gz_keep_lock:
                if not _gz_kept:
                    _gz_kept.append(out)


class Context:
    """One GPU + one HIP stream (``mirge_ctx``)."""

    def __init__(self, device: int = 0, stream: int = 0):
        lib = load()
        if lib.mirge_device_count() <= 0:
            raise RuntimeError("no HIP device visible: mirge3.0_amd needs an MI355X (no CPU fallback)")
        self._h = C.c_void_p()
        _check(lib.mirge_ctx_create(device, C.c_void_p(stream), C.byref(self._h)), "mirge_ctx_create")
        self.device = device
        _track(self)

    def close(self):
        if self._h:
            # whatever still lives in this context goes first -- results, read sets, libraries: their device blocks belong to the
            # context's pool, and a handle destroyed after its context (a reference kept by a traceback, a cycle the collector
            # reaches late) would free into released memory
            objs = [o for o in (r() for r in _live) if o is not None and getattr(o, "ctx", None) is self]
            for kind in (CascadeResult, ReadQc, TrimmedOut, DeviceReads, DeviceLibrary, DeviceGenome):
                for o in objs:
                    if isinstance(o, kind):
                        o.close()
            load().mirge_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(load().mirge_ctx_sync(self._h), "mirge_ctx_sync")

    def pool_stats(self):
        """(bytes the pool has from the driver, blocks handed out and not back, blocks in the free list): host bookkeeping only"""
        out = (C.c_int64 * 3)()
        _check(load().mirge_ctx_pool_stats(self._h, out), "mirge_ctx_pool_stats")
        return int(out[0]), int(out[1]), int(out[2])

    # ---- measurement
    def timer_start(self):
        _check(load().mirge_ctx_timer_start(self._h), "mirge_ctx_timer_start")

    def timer_stop(self) -> float:
        ms = C.c_double()
        _check(load().mirge_ctx_timer_stop(self._h, C.byref(ms)), "mirge_ctx_timer_stop")
        return ms.value

    def profile(self, on: bool):
        _check(load().mirge_ctx_profile_enable(self._h, bool(on)), "profile_enable")

    def profile_only(self, substr: str = ""):
        """bracket only the launches whose name contains ``substr`` ('' = all)"""
        _check(load().mirge_ctx_profile_only(self._h, substr.encode()), "profile_only")

    def profile_units(self, on: bool):
        """False: bracketed cascade launches are timed, their per-pass read counts are not copied back any more"""
        _check(load().mirge_ctx_profile_units(self._h, bool(on)), "profile_units")

    def profile_reset(self):
        _check(load().mirge_ctx_profile_reset(self._h), "profile_reset")

    def profile_records(self):
        """[(kernel name, launches, total ms, units)]"""
        lib = load()
        out = []
        for i in range(lib.mirge_ctx_profile_count(self._h)):
            name = C.create_string_buffer(64)
            launches, ms, units = C.c_int64(), C.c_double(), C.c_double()
            _check(lib.mirge_ctx_profile_get(self._h, i, name, 64, C.byref(launches), C.byref(ms), C.byref(units)), "profile_get")
            out.append((name.value.decode(), launches.value, ms.value, units.value))
        return out


class DeviceLibrary:
    """A reference library packed and indexed in HBM (``mirge_lib``)."""

    def __init__(self, ctx: Context, seqs: FlatSeqs):
        self.ctx = ctx
        self._h = C.c_void_p()
        packed = getattr(seqs, "packed", None)
        if packed is not None:  # a cached library (libcache.PackedSeqs): the image itself, no letters, no packing
            T = np.ascontiguousarray(packed["T"], dtype=np.uint64)
            inv = np.ascontiguousarray(packed["inv"], dtype=np.uint64)
            rs = np.ascontiguousarray(packed["ref_start"], dtype=np.uint32)
            _check(load().mirge_lib_create_packed(ctx._h, T, T.shape[0], inv, inv.shape[0], rs, len(seqs), packed["total"], packed["kmax"],
                                                  packed["valid_positions"], C.byref(self._h)), "mirge_lib_create_packed")
        else:
            data = np.ascontiguousarray(seqs.data, dtype=np.uint8)
            off = np.ascontiguousarray(seqs.offsets, dtype=np.int64)
            _check(load().mirge_lib_create(ctx._h, data, off, len(seqs), C.byref(self._h)), "mirge_lib_create")
        _track(self)

    def packed_image(self) -> dict:
        """the library's packed image (2-bit text, invalid-base bitmap, reference starts) for the cache next to the index"""
        sizes = (C.c_int64 * 4)()
        kmax = C.c_int32()
        _check(load().mirge_lib_packed_sizes(self._h, sizes, C.byref(kmax)), "mirge_lib_packed_sizes")
        T = np.empty(int(sizes[0]), dtype=np.uint64)
        inv = np.empty(int(sizes[1]), dtype=np.uint64)
        rs = np.empty(self.n_refs + 1, dtype=np.uint32)
        _check(load().mirge_lib_packed_copy(self._h, T, inv, rs), "mirge_lib_packed_copy")
        return {"T": T, "inv": inv, "ref_start": rs, "total": int(sizes[2]), "kmax": int(kmax.value), "valid_positions": int(sizes[3])}

    @property
    def n_refs(self) -> int:
        return load().mirge_lib_n_refs(self._h)

    @property
    def device_bytes(self) -> int:
        return load().mirge_lib_device_bytes(self._h)

    def prepare(self, k: int):
        _check(load().mirge_lib_prepare(self._h, k), "mirge_lib_prepare")

    def close(self):
        if self._h:
            load().mirge_lib_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceGenome:
    """The genome of the A-to-I report's filter in HBM (``mirge_genome``): from ASCII references (``seqs``) or from bowtie's own
    reference files as they are (``packed`` = the bytes of ``.4.ebwt``, ``records`` = the ``(off, len, first)`` arrays of
    ``.3.ebwt``, ``ebwt.read_records``)."""

    def __init__(self, ctx: Context, seqs: Optional[FlatSeqs] = None, packed: Optional[np.ndarray] = None, records=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        if seqs is not None:
            data = np.ascontiguousarray(seqs.data, dtype=np.uint8)
            off = np.ascontiguousarray(seqs.offsets, dtype=np.int64)
            _check(load().mirge_genome_create(ctx._h, data, off, len(seqs), C.byref(self._h)), "mirge_genome_create")
        else:
            pk = np.ascontiguousarray(packed, dtype=np.uint8)
            ro, rl, rf = (np.ascontiguousarray(a, dtype=t) for a, t in zip(records, (np.uint64, np.uint64, np.uint8)))
            _check(load().mirge_genome_create_packed(ctx._h, pk, pk.shape[0], ro, rl, rf, ro.shape[0], C.byref(self._h)),
                   "mirge_genome_create_packed")
        _track(self)

    def align_counts(self, seqs: FlatSeqs, n_mm: int, seedlen: int = 28, maxtotal: int = 2, trim5: int = 0, trim3: int = 2) -> np.ndarray:
        """``mirge_genome_align_counts`` -> uint32 [n, 3]: every query's alignments with 0, 1, 2 mismatches"""
        n = len(seqs)
        out = np.zeros((max(n, 1), 3), dtype=np.uint32)
        data = np.ascontiguousarray(seqs.data, dtype=np.uint8)
        off = np.ascontiguousarray(seqs.offsets, dtype=np.int64)
        _check(load().mirge_genome_align_counts(self.ctx._h, self._h, data if data.size else None, off, n, n_mm, seedlen, maxtotal, trim5,
                                                trim3, out), "mirge_genome_align_counts")
        return out[:n]

    def align_loci(self, seqs: FlatSeqs, n_mm: int, seedlen: int = 28, maxtotal: int = 2, trim5: int = 0, trim3: int = 0,
                   max_loci: int = 0, norc: bool = False, strata: bool = False) -> dict:
        """``mirge_genome_align_loci`` -> ``query`` (uint32), ``ref`` (uint32), ``off`` (uint64, 0-based in the reference),
        ``strand`` (uint8, 1 = '-'), ``mm`` (uint8) per reported alignment in (ref, off, query, strand) order, and ``totals``
        (uint64 per query: its valid alignments, reported or capped by ``max_loci``).  ``strata``
        (``mirge_genome_align_loci_strata``): only each query's best stratum -- fewest seed mismatches -- is reported, and
        ``max_loci`` counts that stratum"""
        lib = load()
        n = len(seqs)
        totals = np.zeros(max(n, 1), dtype=np.uint64)
        data = np.ascontiguousarray(seqs.data, dtype=np.uint8)
        off = np.ascontiguousarray(seqs.offsets, dtype=np.int64)
        h = C.c_void_p()
        head = (self.ctx._h, self._h, data if data.size else None, off, n, n_mm, seedlen, maxtotal, trim5, trim3, max_loci, bool(norc))
        if strata:
            _check(lib.mirge_genome_align_loci_strata(*head, 1, totals, C.byref(h)), "mirge_genome_align_loci_strata")
        else:
            _check(lib.mirge_genome_align_loci(*head, totals, C.byref(h)), "mirge_genome_align_loci")
        try:
            m = lib.mirge_loci_count(h)
            out = dict(query=np.zeros(m, np.uint32), ref=np.zeros(m, np.uint32), off=np.zeros(m, np.uint64),
                       strand=np.zeros(m, np.uint8), mm=np.zeros(m, np.uint8))
            if m:
                _check(lib.mirge_loci_fetch(h, *(out[k] for k in ("query", "ref", "off", "strand", "mm"))), "mirge_loci_fetch")
        finally:
            lib.mirge_loci_destroy(h)
        out["totals"] = totals[:n]
        return out

    def fetch(self, ref, start, length, minus, rna) -> List[str]:
        """``mirge_genome_fetch``: the windows ``[start, start + length)`` (0-based) of references ``ref`` as text: 'N' where the
        genome holds no base, reverse-complemented where ``minus``, 'U' for 'T' where ``rna``"""
        ref = np.ascontiguousarray(ref, dtype=np.uint32)
        start, length = (np.ascontiguousarray(a, dtype=np.int64) for a in (start, length))
        minus, rna = (np.ascontiguousarray(a, dtype=np.uint8) for a in (minus, rna))
        n = ref.shape[0]
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(length, out=off[1:])
        out = np.zeros(max(int(off[n]), 1), dtype=np.uint8)
        _check(load().mirge_genome_fetch(self.ctx._h, self._h, n, ref, start, length, minus, rna, off, out), "mirge_genome_fetch")
        text = out.tobytes().decode("ascii")
        return [text[a:b] for a, b in zip(off[:-1].tolist(), off[1:].tolist())]

    def close(self):
        if self._h:
            load().mirge_genome_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceReads:
    """A device-resident packed read set (``mirge_reads``), optionally with a count matrix."""

    def __init__(self, ctx: Context, handle: C.c_void_p):
        self.ctx = ctx
        self._h = handle
        _track(self)

    @staticmethod
    def pack(ctx: Context, reads: FlatSeqs) -> "DeviceReads":
        data = np.ascontiguousarray(reads.data, dtype=np.uint8)
        off = np.ascontiguousarray(reads.offsets, dtype=np.int64)
        h = C.c_void_p()
        _check(load().mirge_reads_pack(ctx._h, data, off, len(reads), C.byref(h)), "mirge_reads_pack")
        return DeviceReads(ctx, h)

    @staticmethod
    def parse(ctx: Context, text, fmt: int = 0, min_len: int = 0, trim: Optional["MirgeTrim"] = None):
        """FASTQ / single-line FASTA / one-sequence-per-line TEXT (bytes or a uint8 array) -> (DeviceReads of the
        records with len >= min_len, number of records seen).  Parsed -- and, with ``trim``, trimmed (quality, 3'
        adapter, N ends, cuts: ``mirge_reads_parse_trim``) -- on the GPU: no per-read host work."""
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(text, dtype=np.uint8)
        h = C.c_void_p()
        nrec = C.c_int64()
        _check(load().mirge_reads_parse_trim(ctx._h, buf if buf.size else None, buf.size, fmt, min_len, trim, C.byref(h), C.byref(nrec)),
               "mirge_reads_parse")
        return DeviceReads(ctx, h), int(nrec.value)

    @staticmethod
    def parse_qc(ctx: Context, text, fmt: int, min_len: int, trim: Optional["MirgeTrim"], qc: Optional["ReadQc"]):
        """``parse`` that also adds the text's records to ``qc`` (``mirge_reads_parse_trim_qc``, ``--read-qc``); ``qc`` None: exactly ``parse``"""
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(text, dtype=np.uint8)
        h = C.c_void_p()
        nrec = C.c_int64()
        _check(load().mirge_reads_parse_trim_qc(ctx._h, buf if buf.size else None, buf.size, fmt, min_len, trim, None if qc is None else qc._h,
                                                C.byref(h), C.byref(nrec)), "mirge_reads_parse_trim_qc")
        if qc is not None:
            qc.fed += 1
        return DeviceReads(ctx, h), int(nrec.value)

    @staticmethod
    def parse_out(ctx: Context, text, fmt: int, min_len: int, trim: Optional["MirgeTrim"], qc: Optional["ReadQc"], out: Optional["TrimmedOut"]):
        """``parse_qc`` that also appends the text's trimmed records to ``out`` (``mirge_reads_parse_trim_out``, ``--trimmed-out``); ``out`` None:
        exactly ``parse_qc``.  A call that fails leaves no file of the sample."""
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(text, dtype=np.uint8)
        h = C.c_void_p()
        nrec = C.c_int64()
        fq = None
        if out is not None:
            fq = out.handle_for(fmt or (3 if not buf.size else (1 if buf[0] == 64 else (2 if buf[0] == 62 else 3))))
        _check(load().mirge_reads_parse_trim_out(ctx._h, buf if buf.size else None, buf.size, fmt, min_len, trim, None if qc is None else qc._h, fq,
                                                 C.byref(h), C.byref(nrec)), "mirge_reads_parse_trim_out")
        if qc is not None:
            qc.fed += 1
        return DeviceReads(ctx, h), int(nrec.value)

    @staticmethod
    def parse_umi(ctx: Context, text, fmt: int, min_len: int, trim: Optional["MirgeTrim"], umi: "MirgeUmi"):
        """``parse`` with the reference's UMI handling (``mirge_reads_parse_umi``) -> (raw INSERTS, records seen, the
        distinct UMI-tagged reads with their counts -- a collapse result -- or None without ``-udd``).  With ``-udd``
        the inserts are one per distinct tagged read, in the order the tagged reads first appeared."""
        buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(text, dtype=np.uint8)
        h, ht = C.c_void_p(), C.c_void_p()
        nrec = C.c_int64()
        _check(load().mirge_reads_parse_umi(ctx._h, buf if buf.size else None, buf.size, fmt, min_len, trim, umi, C.byref(h), C.byref(nrec),
                                            C.byref(ht)), "mirge_reads_parse_umi")
        return DeviceReads(ctx, h), int(nrec.value), (DeviceReads(ctx, ht) if ht.value else None)

    @staticmethod
    def concat(ctx: Context, parts: Sequence["DeviceReads"]) -> "DeviceReads":
        """Raw read sets appended in the order given (one per sample, before the joint collapse)."""
        arr = (C.c_void_p * len(parts))(*[p._h for p in parts])
        h = C.c_void_p()
        _check(load().mirge_reads_concat(ctx._h, arr, len(parts), C.byref(h)), "mirge_reads_concat")
        return DeviceReads(ctx, h)

    def __len__(self) -> int:
        return load().mirge_reads_count(self._h)

    @property
    def n_samples(self) -> int:
        return load().mirge_reads_n_samples(self._h)

    def group_counts(self) -> np.ndarray:
        """reads per storage group: width classes (up to 31, 64, 128, 255 nt, longer) without an ambiguous call, then the same with an N"""
        out = np.zeros(16, dtype=np.int64)
        n = load().mirge_reads_group_counts(self._h, out, 16)
        return out[:n]

    @property
    def iupac_seen(self) -> bool:
        """some read held an IUPAC ambiguity code other than N (packed and printed as N)"""
        return load().mirge_reads_iupac_seen(self._h) == 1

    @staticmethod
    def merge(ctx: "Context", parts: Sequence["DeviceReads"]) -> "DeviceReads":
        """The sample matrix of several samples from their per-sample dictionaries (``mirge_collapse_merge``): unique reads of the
        union, one count column per part, all on the device."""
        arr = (C.c_void_p * len(parts))(*[p._h for p in parts])
        h, nu = C.c_void_p(), C.c_int64()
        _check(load().mirge_collapse_merge(ctx._h, arr, len(parts), C.byref(h), C.byref(nu)), "mirge_collapse_merge")
        return DeviceReads(ctx, h)

    def unpack(self) -> FlatSeqs:
        n = len(self)
        off = np.zeros(n + 1, dtype=np.int64)
        data = np.empty(max(load().mirge_reads_total_bases(self._h), 1), dtype=np.uint8)
        _check(load().mirge_reads_unpack(self.ctx._h, self._h, data, off), "mirge_reads_unpack")
        return FlatSeqs(data[:off[-1]].copy(), off)

    def collapse(self, sample_ids: Optional[np.ndarray] = None, n_samples: int = 1,
                 weights: Optional[np.ndarray] = None) -> "DeviceReads":
        """``weights`` (uint32 per read): read i stands for that many copies (``mirge_collapse_weighted``)."""
        sid = None if sample_ids is None else np.ascontiguousarray(sample_ids, dtype=np.int32)
        h = C.c_void_p()
        nu = C.c_int64()
        if weights is None:
            _check(load().mirge_collapse(self.ctx._h, self._h, sid, n_samples, C.byref(h), C.byref(nu)), "mirge_collapse")
        else:
            w = np.ascontiguousarray(weights, dtype=np.uint32)
            if w.shape[0] != len(self):
                raise ValueError("one weight per read")
            _check(load().mirge_collapse_weighted(self.ctx._h, self._h, sid, n_samples, w, C.byref(h), C.byref(nu)), "mirge_collapse_weighted")
        return DeviceReads(self.ctx, h)

    def counts(self) -> Tuple[np.ndarray, np.ndarray]:
        """(counts [U, S] uint32, first_index [U] int64) of a collapse result."""
        n, S = len(self), self.n_samples
        cnt = np.zeros((n, max(S, 1)), dtype=np.uint32)
        first = np.zeros(n, dtype=np.int64)
        _check(load().mirge_collapse_fetch(self.ctx._h, self._h, cnt, first), "mirge_collapse_fetch")
        return cnt, first

    def umi_cluster(self, front: int, back: int) -> np.ndarray:
        """``mirge_umi_cluster`` on a one-column collapse result (distinct UMI-tagged reads with their counts) -> uint8 [U], handle
        order: 1 = the read founds a molecule under the directional method (UMI = first ``front`` + last ``back`` letters)"""
        n = len(self)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        nf = C.c_int64()
        _check(load().mirge_umi_cluster(self.ctx._h, self._h, front, back, out, C.byref(nf)), "mirge_umi_cluster")
        out = out[:n]
        if int(out.sum()) != nf.value:
            raise RuntimeError("mirge_umi_cluster: the founder count and the flags differ")
        return out

    def kmer_correct(self, k_start: int, k_end: int, threshold: int, ratio: int = 0):
        """``mirge_kmer_correct_ratio`` on a one-column collapse result -> (the corrected dictionary, a collapse result whose first indices are
        this one's; uint32 [U]: the handle index there of every read of this one; uint32 [U]: bit ``k - k_start`` set iff the read, or the
        read it had become, was corrected in the round of ``k``).  ``ratio`` >= 2: the relative threshold of ``--kmer-ratio``; 0: none,
        exactly ``mirge_kmer_correct``"""
        n = len(self)
        final_of = np.zeros(max(n, 1), dtype=np.uint32)
        mask = np.zeros(max(n, 1), dtype=np.uint32)
        h = C.c_void_p()
        if not -2 ** 31 <= int(ratio) < 2 ** 31:
            raise RuntimeError("mirge_kmer_correct_ratio: the ratio is 0 (none) or 2 .. 2^31 - 1")
        _check(load().mirge_kmer_correct_ratio(self.ctx._h, self._h, k_start, k_end, threshold, ratio, C.byref(h), final_of, mask),
               "mirge_kmer_correct_ratio")
        return DeviceReads(self.ctx, h), final_of[:n], mask[:n]

    def adapter_infer(self, probes=None):
        """``mirge_adapter_infer`` on a one-column collapse result of UNTRIMMED reads (``-a auto``) -> the fields of ``mirge_adapter`` as a
        dict (``seq`` empty: no adapter); with ``probes`` (12-mer codes, first letter most significant) -> (that dict, uint64 sums,
        uint64 masks of the probed codes)"""
        out = MirgeAdapter()
        if probes is None:
            _check(load().mirge_adapter_infer(self.ctx._h, self._h, C.byref(out), None, 0, None, None), "mirge_adapter_infer")
            return out.as_dict()
        codes = np.ascontiguousarray(probes, dtype=np.uint32)
        n = int(codes.shape[0])
        sums, masks = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        _check(load().mirge_adapter_infer(self.ctx._h, self._h, C.byref(out), codes if n else None, n, sums, masks), "mirge_adapter_infer")
        return out.as_dict(), sums[:n], masks[:n]

    def first_appearance_order(self) -> np.ndarray:
        """Indices of the unique reads in the order their first copy appeared in the raw reads (``mirge_collapse_order``)."""
        order = np.zeros(len(self), dtype=np.int64)
        _check(load().mirge_collapse_order(self.ctx._h, self._h, order), "mirge_collapse_order")
        return order

    def sorted_order(self) -> np.ndarray:
        """Indices of the unique reads in the order of the sorted sequences (Python string order: the index of the reference's
        outer-joined sample matrix, digest.py:243), from a radix sort on the device (``mirge_collapse_order_sorted``)."""
        order = np.zeros(len(self), dtype=np.int64)
        _check(load().mirge_collapse_order_sorted(self.ctx._h, self._h, order), "mirge_collapse_order_sorted")
        return order

    def range_sample(self, k: int = 256) -> np.ndarray:
        """k evenly spaced quantiles of the dictionary's first-word sort keys (``mirge_reads_range_sample``): what a rank puts
        into the pool the sharded run's range splitters are chosen from (``multigpu.choose_splitters``)"""
        out = np.zeros(k, dtype=np.uint64)
        _check(load().mirge_reads_range_sample(self.ctx._h, self._h, k, out), "mirge_reads_range_sample")
        return out

    def range_split(self, splitters: np.ndarray):
        """The dictionary ordered by (owner range, handle index) -> (FlatSeqs, counts [U, S] uint32, bounds int64 [n_parts + 1]);
        range q = keys in [splitters[q-1], splitters[q]) = rows bounds[q] .. bounds[q+1] (``mirge_reads_range_split``)."""
        sp = np.ascontiguousarray(splitters, dtype=np.uint64)
        n_parts = int(sp.shape[0]) + 1
        n, S = len(self), max(self.n_samples, 1)
        off = np.zeros(n + 1, dtype=np.int64)
        data = np.empty(max(load().mirge_reads_total_bases(self._h), 1), dtype=np.uint8)
        cnt = np.zeros((n, S), dtype=np.uint32)
        bounds = np.zeros(n_parts + 1, dtype=np.int64)
        _check(load().mirge_reads_range_split(self.ctx._h, self._h, sp if sp.size else None, n_parts, data, off, cnt if cnt.size else None,
                                              bounds), "mirge_reads_range_split")
        return FlatSeqs(data[:off[-1]], off), cnt, bounds

    def nonzero_per_sample(self) -> np.ndarray:
        """unique reads with a count, per sample column (``mirge_collapse_nonzero``)"""
        out = np.zeros(max(self.n_samples, 1), dtype=np.int64)
        _check(load().mirge_collapse_nonzero(self.ctx._h, self._h, out), "mirge_collapse_nonzero")
        return out

    def set_counts(self, counts: np.ndarray):
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(len(self), -1)
        _check(load().mirge_reads_set_counts(self.ctx._h, self._h, counts, counts.shape[1]), "mirge_reads_set_counts")

    def close(self):
        if self._h:
            load().mirge_reads_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def umi_cluster_stats() -> dict:
    """``mirge_umi_cluster_stats``: what this thread's last directional clustering saw"""
    out = np.zeros(5, dtype=np.int64)
    _check(load().mirge_umi_cluster_stats(out), "mirge_umi_cluster_stats")
    return dict(zip(("tagged", "eligible", "linked", "rounds", "slots"), (int(x) for x in out)))


KMER_CORRECT_TALLIES = ("eligible", "suspect", "corrected", "uncorrectable", "unsupported", "ambiguous", "distinct", "slots")


def kmer_correct_stats() -> list:
    """``mirge_kmer_correct_stats``: one dict per round of this thread's last ``mirge_kmer_correct``"""
    out = np.zeros(8 * 24, dtype=np.int64)
    rounds = load().mirge_kmer_correct_stats(out)
    if rounds < 0:
        _check(rounds, "mirge_kmer_correct_stats")
    return [dict(zip(KMER_CORRECT_TALLIES, (int(x) for x in out[8 * r:8 * r + 8]))) for r in range(rounds)]


def kmer_correct_ratio_stats() -> list:
    """``mirge_kmer_correct_ratio_stats``: per round of this thread's last ``kmer_correct`` a dict ``above`` (distinct k-mers with a sum
    above the threshold) and ``dominated`` (those of them a neighbouring k-mer dominates); zeros when that call had no ratio"""
    out = np.zeros(2 * 24, dtype=np.int64)
    rounds = load().mirge_kmer_correct_ratio_stats(out)
    if rounds < 0:
        _check(rounds, "mirge_kmer_correct_ratio_stats")
    return [{"above": int(out[2 * r]), "dominated": int(out[2 * r + 1])} for r in range(rounds)]


QC_VIEW_WORDS = 92467  # MIRGE_QC_VIEW_WORDS of csrc/kernels_qc.hpp: the 64-bit words of one view's tables (mirge_qc_fetch)


class ReadQc:
    """The ``--read-qc`` accumulator of ONE sample (``mirge_qc``): the tables of the ``raw`` and the ``trimmed`` view on the device, fed by
    ``DeviceReads.parse_qc`` piece by piece"""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()
        _check(load().mirge_qc_create(ctx._h, C.byref(self._h)), "mirge_qc_create")
        self.fed = 0  # pieces that went in
        _track(self)

    def reset(self):
        """empty tables again (a sample whose text is parsed a second time from its start)"""
        self.close()
        _check(load().mirge_qc_create(self.ctx._h, C.byref(self._h)), "mirge_qc_create")
        self.fed = 0

    def fetch(self):
        """-> (int64 [2][QC_VIEW_WORDS]: raw, trimmed, in the layout include/mirge_native.h documents; True when a FASTQ piece went in)"""
        out = np.zeros((2, QC_VIEW_WORDS), dtype=np.int64)
        has_q = C.c_int32()
        _check(load().mirge_qc_fetch(self.ctx._h, self._h, out, C.byref(has_q)), "mirge_qc_fetch")
        return out, bool(has_q.value)

    def close(self):
        if self._h:
            load().mirge_qc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrimmedOut:
    """The ``--trimmed-out`` writer of ONE sample (``mirge_fqout``), fed by ``DeviceReads.parse_out`` piece by piece.  The file's name depends
    on the input format (``trimmed_out.file_name``), which the first piece tells: the native writer is created then, in ``directory``.
    ``mode``: ``plain`` | ``gz`` (BGZF with a ``.gzi``); ``block_bytes`` <= 0: MIRGE_BGZF_BLOCK_BYTES."""
    STATS = ("records", "written", "stream_bytes", "file_bytes", "members", "stored", "fixed", "dynamic")

    def __init__(self, ctx: Context, directory, sample: str, mode: str = "plain", block_bytes: int = 0):
        if mode not in ("plain", "gz"):
            raise ValueError(f"mode={mode!r}: plain or gz")
        self.ctx, self.directory, self.sample, self.mode, self.block_bytes = ctx, str(directory), str(sample), mode, int(block_bytes)
        self._h = C.c_void_p()
        self.fmt = 0
        self.path = None  # the file's final name, once known
        _track(self)

    def handle_for(self, fmt: int):
        """the native writer, created for input format ``fmt`` (1 FASTQ, 2 FASTA, 3 one sequence per line) on first use"""
        if not self._h:
            from . import trimmed_out
            self.fmt = int(fmt)
            self.path = os.path.join(self.directory, trimmed_out.file_name(self.sample, self.fmt, self.mode))
            gzi = (self.path + ".gzi").encode() if self.mode == "gz" else None
            _check(load().mirge_fqout_create(self.ctx._h, self.path.encode(), gzi, self.block_bytes, C.byref(self._h)), "mirge_fqout_create")
        return self._h

    def reset(self):
        """nothing written yet again: the files reopened, the offsets 0 (a sample whose text is parsed a second time from its start)"""
        self.close()
        self.fmt, self.path = 0, None

    def finish(self) -> dict:
        """the rest of the stream, the files renamed to their names -> STATS as a dict (plus ``path``); a sample without a piece: an empty file"""
        out = np.zeros(8, dtype=np.int64)
        _check(load().mirge_fqout_finish(self.ctx._h, self.handle_for(self.fmt or 3), out), "mirge_fqout_finish")
        self.close()
        return {**{k: int(v) for k, v in zip(self.STATS, out)}, "path": self.path}

    def close(self):
        """without ``finish``: the ``.tmp`` files are removed"""
        if self._h:
            load().mirge_fqout_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def qc_class_profile(ctx: "Context", uniq: "DeviceReads", res: "CascadeResult") -> np.ndarray:
    """``mirge_qc_class_profile`` -> int64 [S][n_pass + 1][257][5][2]: per sample, class (pass; n_pass: unmapped), min(length, 256), first
    letter (A C G T N) the raw reads and the unique reads with a count > 0"""
    out = np.zeros((max(uniq.n_samples, 1), res.n_pass + 1, 257, 5, 2), dtype=np.int64)
    _check(load().mirge_qc_class_profile(ctx._h, uniq._h, res._h, res.n_pass, out), "mirge_qc_class_profile")
    return out


class CascadeResult:
    """Device-resident per-read annotation (``mirge_result``)."""

    def __init__(self, ctx: Context, handle: C.c_void_p, reads: DeviceReads, n_pass: int):
        self.ctx, self._h, self.reads, self.n_pass = ctx, handle, reads, n_pass
        _track(self)

    def fetch(self):
        """(pass int8, ref int32, off int32, mm int8) in the read set's order; -1 = unannotated."""
        n = len(self.reads)
        ps = np.empty(n, dtype=np.int8)
        ref = np.empty(n, dtype=np.int32)
        off = np.empty(n, dtype=np.int32)
        mm = np.empty(n, dtype=np.int8)
        _check(load().mirge_result_fetch(self.ctx._h, self._h, ps, ref, off, mm), "mirge_result_fetch")
        return ps, ref, off, mm

    def close(self):
        if self._h:
            load().mirge_result_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cascade_args(libs: Sequence[Optional[DeviceLibrary]], policies: Sequence[MirgePolicy]):
    """The two C arrays ``mirge_cascade_run`` takes, built once by callers that run many read sets through one
    library set (this sits on the host's critical path between the collapse's sync and the first pass)."""
    n_pass = len(policies)
    arr = (C.c_void_p * n_pass)(*[(lb._h if lb is not None else C.c_void_p(0)) for lb in libs])
    pol = (MirgePolicy * n_pass)(*policies)
    return arr, pol, n_pass


def cascade_run(ctx: Context, reads: DeviceReads, libs: Sequence[Optional[DeviceLibrary]],
                policies: Sequence[MirgePolicy], prepared=None) -> CascadeResult:
    arr, pol, n_pass = prepared if prepared is not None else cascade_args(libs, policies)
    h = C.c_void_p()
    _check(load().mirge_cascade_run(ctx._h, reads._h, arr, pol, n_pass, C.byref(h)), "mirge_cascade_run")
    return CascadeResult(ctx, h, reads, n_pass)


def cascade_prepare(ctx: Context, reads: DeviceReads, libs: Sequence[Optional[DeviceLibrary]],
                    policies: Sequence[MirgePolicy], prepared=None) -> None:
    """Build the probe / plan tables a cascade over ``reads`` needs now (``mirge_cascade_prepare``) and wait for them."""
    arr, pol, n_pass = prepared if prepared is not None else cascade_args(libs, policies)
    _check(load().mirge_cascade_prepare(ctx._h, reads._h, arr, pol, n_pass), "mirge_cascade_prepare")


def cascade_walks(ctx: "Context"):
    """(walks over the bulk one-word group's list, passes answered by a whole-read lookup inside another pass's walk, passes) of
    the ctx's current cascade configuration (``mirge_cascade_walks``)."""
    w = (C.c_int32 * 3)()
    _check(load().mirge_cascade_walks(ctx._h, w), "mirge_cascade_walks")
    return int(w[0]), int(w[1]), int(w[2])


def cascade_wg_times(ctx: "Context"):
    """milliseconds every workgroup of the last profiled bulk-cascade launch took (``mirge_cascade_wg_times``), or None"""
    g, khz = C.c_int32(0), C.c_int32(0)
    _check(load().mirge_cascade_wg_times(ctx._h, None, 0, C.byref(g), C.byref(khz)), "mirge_cascade_wg_times")
    if g.value <= 0:
        return None
    t = np.zeros(g.value, dtype=np.uint32)
    _check(load().mirge_cascade_wg_times(ctx._h, t, g.value, C.byref(g), C.byref(khz)), "mirge_cascade_wg_times")
    return t.astype(np.float64) / max(khz.value, 1)


def collapse_cascade(ctx: Context, raw: DeviceReads, libs: Sequence[Optional[DeviceLibrary]],
                     policies: Sequence[MirgePolicy], prepared=None) -> Tuple[DeviceReads, CascadeResult]:
    """One sample: collapse + cascade in one call (``mirge_collapse_cascade``) -> (unique reads, annotation)."""
    arr, pol, n_pass = prepared if prepared is not None else cascade_args(libs, policies)
    hu, hr = C.c_void_p(), C.c_void_p()
    nu = C.c_int64()
    _check(load().mirge_collapse_cascade(ctx._h, raw._h, arr, pol, n_pass, C.byref(hu), C.byref(nu), C.byref(hr)),
           "mirge_collapse_cascade")
    uniq = DeviceReads(ctx, hu)
    return uniq, CascadeResult(ctx, hr, uniq, n_pass)


def count_join(ctx: Context, uniq: DeviceReads, res: CascadeResult, exact_pass: int, iso_pass: int,
               n_mirna: int):
    """-> (class_sums [n_pass, S], exact [n_mirna, S], iso [n_mirna, S]) int64."""
    S = uniq.n_samples
    cls = np.zeros((res.n_pass, S), dtype=np.int64)
    ex = np.zeros((max(n_mirna, 1), S), dtype=np.int64)
    iso = np.zeros((max(n_mirna, 1), S), dtype=np.int64)
    _check(load().mirge_count_join(ctx._h, uniq._h, res._h, exact_pass, iso_pass, n_mirna, cls, ex, iso), "mirge_count_join")
    return cls, ex[:n_mirna], iso[:n_mirna]


def count_join_host(ctx: Context, ps: np.ndarray, ref: np.ndarray, counts: np.ndarray, n_pass: int,
                    exact_pass: int, iso_pass: int, n_mirna: int):
    """``count_join`` from host arrays (pass int8 [n], ref int32 [n], counts uint32 [n, S])."""
    ps = np.ascontiguousarray(ps, dtype=np.int8)
    ref = np.ascontiguousarray(ref, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(ps.shape[0], -1)
    S = counts.shape[1]
    cls = np.zeros((n_pass, S), dtype=np.int64)
    ex = np.zeros((max(n_mirna, 1), S), dtype=np.int64)
    iso = np.zeros((max(n_mirna, 1), S), dtype=np.int64)
    _check(load().mirge_count_join_host(ctx._h, ps, ref, counts, ps.shape[0], S, n_pass, exact_pass, iso_pass, n_mirna, cls, ex, iso),
           "mirge_count_join_host")
    return cls, ex[:n_mirna], iso[:n_mirna]


TALLY_POSITIONS = 32


def variant_tally(ctx: Context, uniq: DeviceReads, res: CascadeResult, exact_pass: int, iso_pass: int,
                  fam_of_ref: np.ndarray, targets: FlatSeqs, retained: Optional[np.ndarray], freq: np.ndarray,
                  per_read: bool = True):
    """``mirge_variant_tally`` (config 5 / rows a16, N1) -> dict: n_seqs, seq_true, count_true, canon, kept_exact
    [n_fam, S]; census [n_fam, 32, 4, 4, 3, S]; diag, state [n reads] (handle order) when ``per_read``.
    Canonical sequences of up to 32 nt (A/C/G/T/U), member reads of up to 64 nt: a longer canonical sequence, one with another
    character, or a read of more than 64 nt that is a member of a family's list raises ``RuntimeError`` -- nothing is dropped."""
    n_fam, S, n = len(targets), uniq.n_samples, len(uniq)
    fam_of_ref = np.ascontiguousarray(fam_of_ref, dtype=np.int32)
    tdata = np.ascontiguousarray(targets.data, dtype=np.uint8)
    toff = np.ascontiguousarray(targets.offsets, dtype=np.int64)
    freq = np.ascontiguousarray(freq, dtype=np.float64)
    assert freq.shape[0] == S
    ret = None if retained is None else np.ascontiguousarray(retained, dtype=np.uint8)
    assert ret is None or ret.shape[0] == n
    tabs = np.empty((5, max(n_fam, 1), S), dtype=np.int64)  # every cell is written by the call
    cen = np.empty((max(n_fam, 1), TALLY_POSITIONS, 4, 4, 3, S), dtype=np.int64)
    diag = np.empty(max(n, 1), dtype=np.int8) if per_read else None
    state = np.empty(max(n, 1), dtype=np.int8) if per_read else None
    if n_fam == 0:
        tabs = np.zeros((5, 0, S), dtype=np.int64)
    _check(load().mirge_variant_tally(ctx._h, uniq._h, res._h, exact_pass, iso_pass, fam_of_ref, fam_of_ref.shape[0],
                                      tdata if tdata.size else None, toff, n_fam, ret, freq, tabs if n_fam else np.zeros(1, np.int64),
                                      cen, diag, state), "mirge_variant_tally")
    out = dict(zip(("n_seqs", "seq_true", "count_true", "canon", "kept_exact"), tabs[:, :n_fam]))
    out["census"] = cen[:n_fam]
    if per_read:
        out["diag"], out["state"] = diag[:n], state[:n]
    return out


def annotation_csv(mapped_path, unmapped_path, header: str, seqs: FlatSeqs, ps: np.ndarray, ref: np.ndarray,
                   counts: np.ndarray, rows: np.ndarray, col_of_pass: Sequence[int], n_name_cols: int,
                   names_by_pass: Sequence[Optional[FlatSeqs]]):
    """``mapped.csv`` / ``unmapped.csv`` (mirge/__main__.py:164-173) from flat arrays; ``names_by_pass[p]`` = the
    reference names of pass p's library as a FlatSeqs (None: the pass has none)."""
    n_pass, col, nd, no, nn, keep = _name_tables(col_of_pass, names_by_pass)
    data = np.ascontiguousarray(seqs.data, dtype=np.uint8)
    off = np.ascontiguousarray(seqs.offsets, dtype=np.int64)
    ps = np.ascontiguousarray(ps, dtype=np.int8)
    ref = np.ascontiguousarray(ref, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(ps.shape[0], -1)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    enc = lambda x: None if x is None else str(x).encode()
    _check(load().mirge_annotation_csv(enc(mapped_path), enc(unmapped_path), header.encode(), data if data.size else None, off, ps, ref, counts,
                                       counts.shape[1], rows, rows.shape[0], n_pass, col, n_name_cols, nd, no, nn), "mirge_annotation_csv")


def _name_tables(col_of_pass, names_by_pass):
    """ctypes views of the per-pass reference-name tables the CSV formatters take (+ the arrays that must outlive the call)"""
    n_pass = len(col_of_pass)
    col = (C.c_int32 * n_pass)(*[int(x) for x in col_of_pass])
    keep = []
    nd, no, nn = (C.c_void_p * n_pass)(), (C.c_void_p * n_pass)(), (C.c_int64 * n_pass)()
    for p in range(n_pass):
        fs = names_by_pass[p]
        if fs is None:
            nd[p], no[p], nn[p] = None, None, 0
            continue
        d = np.ascontiguousarray(fs.data, dtype=np.uint8)
        o = np.ascontiguousarray(fs.offsets, dtype=np.int64)
        keep += [d, o]
        nd[p], no[p], nn[p] = d.ctypes.data if d.size else None, o.ctypes.data, len(fs)
    return n_pass, col, nd, no, nn, keep


def annotation_csv_device_sizes(ctx: "Context", uniq: "DeviceReads", res: "CascadeResult", rows: np.ndarray, col_of_pass: Sequence[int],
                                n_name_cols: int, names_by_pass: Sequence[Optional[FlatSeqs]]):
    """(bytes in mapped.csv, bytes in unmapped.csv) the listed rows take (``mirge_annotation_csv_device_sizes``): a rank's stretch of
    a sharded run's files; None when a reference name needs CSV quoting (the run then takes rank 0's host route)."""
    n_pass, col, nd, no, nn, keep = _name_tables(col_of_pass, names_by_pass)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.zeros(2, dtype=np.int64)
    rc = load().mirge_annotation_csv_device_sizes(ctx._h, uniq._h, res._h, rows if rows.size else None, rows.shape[0], n_pass, col, n_name_cols,
                                                  nd, no, nn, out)
    if rc == -4:
        return None
    _check(rc, "mirge_annotation_csv_device_sizes")
    return int(out[0]), int(out[1])


def annotation_csv_device_at(ctx: "Context", uniq: "DeviceReads", res: "CascadeResult", mapped_path, unmapped_path, mapped_off: int,
                             unmapped_off: int, rows: np.ndarray, col_of_pass: Sequence[int], n_name_cols: int,
                             names_by_pass: Sequence[Optional[FlatSeqs]]):
    """The listed rows' text at the given byte offsets of the two EXISTING files (``mirge_annotation_csv_device_at``)."""
    n_pass, col, nd, no, nn, keep = _name_tables(col_of_pass, names_by_pass)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    _check(load().mirge_annotation_csv_device_at(ctx._h, uniq._h, res._h, str(mapped_path).encode(), str(unmapped_path).encode(), mapped_off,
                                                 unmapped_off, rows if rows.size else None, rows.shape[0], n_pass, col, n_name_cols, nd, no, nn),
           "mirge_annotation_csv_device_at")


def annotation_csv_device(ctx: "Context", uniq: "DeviceReads", res: "CascadeResult", mapped_path, unmapped_path, header: str,
                          rows: np.ndarray, col_of_pass: Sequence[int], n_name_cols: int,
                          names_by_pass: Sequence[Optional[FlatSeqs]]) -> bool:
    """``mapped.csv`` / ``unmapped.csv`` formatted on the GPU from the device-resident reads, counts and annotation
    (``mirge_annotation_csv_device``).  False: a reference name needs CSV quoting -- call ``annotation_csv`` instead."""
    n_pass, col, nd, no, nn, keep = _name_tables(col_of_pass, names_by_pass)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    enc = lambda x: None if x is None else str(x).encode()
    rc = load().mirge_annotation_csv_device(ctx._h, uniq._h, res._h, enc(mapped_path), enc(unmapped_path), header.encode(),
                                            rows if rows.size else None, rows.shape[0], n_pass, col, n_name_cols, nd, no, nn)
    if rc == -4:
        return False
    _check(rc, "mirge_annotation_csv_device")
    return True


def loci_cluster(ctx: Context, ref, off, strand, query, qlen, qcount, ref_skip, threshold: int, minus_first_only: bool = True) -> dict:
    """``mirge_loci_cluster``: records sorted by (ref, off) -> ``cluster`` (int32 per record, -1 = dropped) and the cluster table
    ``ref``, ``strand``, ``start`` (0-based), ``end`` (exclusive), ``reads``, ``members`` in (ref, strand, start) order"""
    ref, query = (np.ascontiguousarray(a, dtype=np.uint32) for a in (ref, query))
    off = np.ascontiguousarray(off, dtype=np.uint64)
    strand, ref_skip = (np.ascontiguousarray(a, dtype=np.uint8) for a in (strand, ref_skip))
    qlen = np.ascontiguousarray(qlen, dtype=np.int32)
    qcount = np.ascontiguousarray(qcount, dtype=np.int64)
    n = ref.shape[0]
    m = max(n, 1)
    cluster = np.full(m, -1, dtype=np.int32)
    tab = dict(ref=np.zeros(m, np.uint32), strand=np.zeros(m, np.uint8), start=np.zeros(m, np.uint64), end=np.zeros(m, np.uint64),
               reads=np.zeros(m, np.int64), members=np.zeros(m, np.uint32))
    nc = C.c_int64(0)
    _check(load().mirge_loci_cluster(ctx._h, n, ref, off, strand, query, qlen.shape[0], qlen, qcount, ref_skip.shape[0], ref_skip, threshold,
                                     bool(minus_first_only), cluster, C.byref(nc),
                                     *(tab[k] for k in ("ref", "strand", "start", "end", "reads", "members"))), "mirge_loci_cluster")
    out = {k: v[:nc.value] for k, v in tab.items()}
    out["cluster"] = cluster[:n]
    return out


TRF_TYPES = ("tRF-whole", "5'-half", "5'-tRF", "3'-half", "3'-tRF", "i-tRF", "tRF-1")  # csrc/kernels_trf.hpp: MIRGE_TRF_*
TRF_NO_DIST = 100


def trf_hits(ctx: Context, uniq: DeviceReads, res: CascadeResult, mature_pass: int, mature_lib: DeviceLibrary, mature_pol: MirgePolicy,
             primary_pass: int, primary_lib: DeviceLibrary, primary_pol: MirgePolicy, rows, anticodon) -> dict:
    """``mirge_trf_hits_run``: every best-stratum alignment of the tRNA reads ``rows`` (handle indices of ``uniq``) -> ``row`` (uint32,
    index into ``rows``), ``ref`` (uint32), ``off`` (int32, 0-based), ``mm``, ``cls`` (0 mature, 1 primary), ``type`` (index into
    ``TRF_TYPES``) per window, sorted by (row, ref, off).  ``anticodon``: 0-based anticodon start of every mature reference."""
    lib = load()
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    anticodon = np.ascontiguousarray(anticodon, dtype=np.int32)
    if anticodon.shape[0] != mature_lib.n_refs:
        raise ValueError("one anticodon start per mature reference")
    h = C.c_void_p()
    _check(lib.mirge_trf_hits_run(ctx._h, uniq._h, res._h, mature_pass, mature_lib._h, mature_pol, primary_pass, primary_lib._h, primary_pol,
                                  rows if rows.size else None, rows.shape[0], anticodon if anticodon.size else None, C.byref(h)),
           "mirge_trf_hits_run")
    try:
        m = lib.mirge_trf_hits_count(h)
        out = dict(row=np.zeros(m, np.uint32), ref=np.zeros(m, np.uint32), off=np.zeros(m, np.int32), mm=np.zeros(m, np.uint8),
                   cls=np.zeros(m, np.uint8), type=np.zeros(m, np.uint8))
        if m:
            _check(lib.mirge_trf_hits_fetch(h, *(out[k] for k in ("row", "ref", "off", "mm", "cls", "type"))), "mirge_trf_hits_fetch")
    finally:
        lib.mirge_trf_hits_destroy(h)
    return out


def trf_assign(ctx: Context, uniq: DeviceReads, res: CascadeResult, read, tref, start, ref_ptr, strings: Sequence[bytes], c_start, c_end,
               rank):
    """``mirge_trf_assign``: per report row (``read`` = handle index, ``tref`` = index into the CSR ``ref_ptr`` over the predefined
    tRFs or -1, ``start`` 1-based) -> (``dist`` int32, ``trf`` int32 index or -1).  ``strings``: the tRFs' dashed strings."""
    read = np.ascontiguousarray(read, dtype=np.int64)
    tref, start = (np.ascontiguousarray(a, dtype=np.int32) for a in (tref, start))
    ref_ptr = np.ascontiguousarray(ref_ptr, dtype=np.int64)
    c_start, c_end, rank = (np.ascontiguousarray(a, dtype=np.int32) for a in (c_start, c_end, rank))
    n, n_trf = read.shape[0], len(strings)
    str_off = np.zeros(n_trf + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=str_off[1:])
    blob = np.frombuffer(b"".join(strings) or b"\0", dtype=np.uint8)
    dist, trf = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    _check(load().mirge_trf_assign(ctx._h, uniq._h, res._h, n, read, tref, start, max(ref_ptr.shape[0] - 1, 0), ref_ptr, n_trf, str_off, blob,
                                   c_start, c_end, rank, dist, trf), "mirge_trf_assign")
    return dist[:n], trf[:n]


TRF_CLUSTER_MAXCOL = 256  # csrc/kernels_trf.hpp: MIRGE_TRF_CL_MAXCOL


def trf_gauss(max_tlen: int) -> np.ndarray:
    """the reference's ``guass_func`` (mirge2_tRF_a2i.py:137) with dc = 3.0 for every distance two points of a template of ``max_tlen``
    columns can have, by Python's ``math.exp``: the device looks the values up"""
    import math
    return np.asarray([math.exp(-(float(d) / 3.0) ** 2) for d in range(2 * int(max_tlen) + 1)], dtype=np.float64)


def trf_cluster(ctx: Context, uniq: DeviceReads, grp_ptr, read, off, rp100k, tlen, gauss=None) -> dict:
    """``mirge_trf_cluster``: groups of points (CSR ``grp_ptr``; per point ``read`` = handle index, ``off`` = 0-based offset in the
    template, ``rp100k``; per group ``tlen``) -> per point ``rho`` / ``delta`` (float32), ``nneigh`` / ``order`` / ``cl`` / ``halo`` /
    ``centre`` (int32), per group ``nclust``: see include/mirge_native.h"""
    grp_ptr, read = (np.ascontiguousarray(a, dtype=np.int64) for a in (grp_ptr, read))
    off, tlen = (np.ascontiguousarray(a, dtype=np.int32) for a in (off, tlen))
    rp100k = np.ascontiguousarray(rp100k, dtype=np.float64)
    n_grp, n = grp_ptr.shape[0] - 1, read.shape[0]
    if n_grp < 0 or int(grp_ptr[-1]) != n or off.shape[0] != n or rp100k.shape[0] != n or tlen.shape[0] != n_grp:
        raise ValueError("trf_cluster: the arrays do not fit the group table")
    if gauss is None:
        gauss = trf_gauss(int(tlen.max()) if n_grp else 1)
    gauss = np.ascontiguousarray(gauss, dtype=np.float64)
    out = dict(rho=np.zeros(max(n, 1), np.float32), delta=np.zeros(max(n, 1), np.float32))
    for k in ("nneigh", "order", "cl", "halo", "centre"):
        out[k] = np.zeros(max(n, 1), np.int32)
    out["nclust"] = np.zeros(max(n_grp, 1), np.int32)
    _check(load().mirge_trf_cluster(ctx._h, uniq._h, n_grp, grp_ptr, read, off, rp100k, tlen, gauss.shape[0], gauss,
                                    *(out[k] for k in ("rho", "delta", "nneigh", "order", "cl", "halo", "nclust", "centre"))), "mirge_trf_cluster")
    return {k: (a[:n_grp] if k == "nclust" else a[:n]) for k, a in out.items()}


def trf_row_counts(ctx: Context, uniq: DeviceReads, rows) -> np.ndarray:
    """``mirge_trf_row_counts``: the count matrix of the reads ``rows`` alone -> uint32 [len(rows), samples]"""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.zeros((rows.shape[0], max(uniq.n_samples, 1)), dtype=np.uint32)
    if rows.size:
        _check(load().mirge_trf_row_counts(ctx._h, uniq._h, rows, rows.shape[0], out), "mirge_trf_row_counts")
    return out


NEAREST_STATS = ("unmapped", "short", "long", "considered", "reported")


def _flat_ascii(seqs) -> Tuple[np.ndarray, np.ndarray, int]:
    """sequences (``FlatSeqs`` or strings) -> (bytes as uint8, never empty; int64 offsets; their number)"""
    flat = seqs if isinstance(seqs, FlatSeqs) else FlatSeqs.from_list(list(seqs))
    data = np.ascontiguousarray(flat.data, dtype=np.uint8)
    return (data if data.size else np.zeros(1, np.uint8)), np.ascontiguousarray(flat.offsets, dtype=np.int64), len(flat)


def nearest_scan(ctx: Context, queries, targets) -> dict:
    """``mirge_nearest_scan``: for EVERY query (``FlatSeqs`` or strings) against the targets in order -> ``dist``, ``hairpin``, ``start``,
    ``end`` (int32; all -1 for a query outside 12 .. 64 letters or targets without a base); ``h[start:end]`` is the matched substring."""
    q, q_off, n = _flat_ascii(queries)
    t, t_off, n_t = _flat_ascii(targets)
    out = {k: np.full(max(n, 1), -1, np.int32) for k in ("dist", "hairpin", "start", "end")}
    _check(load().mirge_nearest_scan(ctx._h, q, q_off, n, t, t_off, n_t, out["dist"], out["hairpin"], out["start"], out["end"]), "mirge_nearest_scan")
    return {k: a[:n] for k, a in out.items()}


def nearest_unmapped(ctx: Context, uniq: DeviceReads, res: CascadeResult, targets, K: int) -> Tuple[dict, dict]:
    """``mirge_nearest_unmapped``: the rows of ``uniq`` that ``res`` left unannotated, 12 .. 64 nt long, with D <= min(K, length // 8) ->
    ({``row`` (uint32 handle index, ascending), ``dist``, ``hairpin``, ``start``, ``end`` (int32)}, {name of ``NEAREST_STATS``: int})"""
    lib = load()
    t, t_off, n_t = _flat_ascii(targets)
    h = C.c_void_p()
    _check(lib.mirge_nearest_unmapped(ctx._h, uniq._h, res._h, t, t_off, n_t, int(K), C.byref(h)), "mirge_nearest_unmapped")
    try:
        m = lib.mirge_nearest_count(h)
        out = dict(row=np.zeros(m, np.uint32), **{k: np.zeros(m, np.int32) for k in ("dist", "hairpin", "start", "end")})
        if m:
            _check(lib.mirge_nearest_fetch(h, *(out[k] for k in ("row", "dist", "hairpin", "start", "end"))), "mirge_nearest_fetch")
        st = np.zeros(len(NEAREST_STATS), np.int64)
        _check(lib.mirge_nearest_stats(h, st), "mirge_nearest_stats")
    finally:
        lib.mirge_nearest_destroy(h)
    return out, dict(zip(NEAREST_STATS, (int(x) for x in st)))


def bam_huffman_probe(ctx: Context, counts, max_bits: int) -> np.ndarray:
    """``mirge_bam_huffman_probe``: the code lengths (uint8 per symbol) that ``MIRGE_BAM_DEFLATE=dynamic``'s builder gives ``counts``
    under the limit ``max_bits``"""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    out = np.zeros(max(counts.shape[0], 1), dtype=np.uint8)
    _check(load().mirge_bam_huffman_probe(ctx._h, counts, counts.shape[0], max_bits, out), "mirge_bam_huffman_probe")
    return out[:counts.shape[0]]


PILEUP_MAXREAD, PILEUP_MAXCLUSTER = 64, 128  # csrc/kernels_pileup.hpp
PILEUP_FLAG_GAP, PILEUP_FLAG_NONE = 1, 2


def cluster_diagonals(ctx: Context, reads: FlatSeqs, clusters: FlatSeqs, row_cluster) -> dict:
    """``mirge_cluster_diagonals``: per row ``diag`` (cluster index - read index of the best ungapped local diagonal), ``score``,
    ``identity`` (equal bases over the whole overlap on that diagonal) and ``flag`` (PILEUP_FLAG_GAP: a gapped alignment could
    tie or win, PILEUP_FLAG_NONE: nothing scores)"""
    row_cluster = np.ascontiguousarray(row_cluster, dtype=np.uint32)
    n = len(reads)
    m = max(n, 1)
    out = dict(diag=np.zeros(m, np.int32), score=np.zeros(m, np.int32), identity=np.zeros(m, np.int32), flag=np.zeros(m, np.uint8))
    rd, ro = np.ascontiguousarray(reads.data, dtype=np.uint8), np.ascontiguousarray(reads.offsets, dtype=np.int64)
    cd, co = np.ascontiguousarray(clusters.data, dtype=np.uint8), np.ascontiguousarray(clusters.offsets, dtype=np.int64)
    _check(load().mirge_cluster_diagonals(ctx._h, rd if rd.size else None, ro, n, cd if cd.size else None, co, len(clusters), row_cluster,
                                          *(out[k] for k in ("diag", "score", "identity", "flag"))), "mirge_cluster_diagonals")
    return {k: v[:n] for k, v in out.items()}


def cluster_pileup(ctx: Context, reads: FlatSeqs, c_len, row_start, diag, count) -> dict:
    """``mirge_cluster_pileup``: rows ``[row_start[k], row_start[k + 1])`` are cluster k's -> ``head`` / ``tail`` (int32 per
    cluster), ``col_off`` (int64 [clusters + 1]) and ``tally`` (int64 [columns, 5]: A, T, C, G, other)"""
    c_len, row_start, count = (np.ascontiguousarray(a, dtype=np.int64) for a in (c_len, row_start, count))
    diag = np.ascontiguousarray(diag, dtype=np.int32)
    nc = c_len.shape[0]
    # the columns the call will write, from the same diagonals it is given (it checks them and fails on a smaller array): no
    # worst-case array of 126 spare columns per cluster
    lens = np.diff(np.ascontiguousarray(reads.offsets, dtype=np.int64))
    k = np.repeat(np.arange(nc), np.diff(row_start))
    pad_h, pad_t = np.zeros(nc, np.int64), np.zeros(nc, np.int64)
    if diag.shape[0] == k.shape[0] == lens.shape[0] and nc:
        np.maximum.at(pad_h, k, -diag.astype(np.int64))
        np.maximum.at(pad_t, k, lens + diag - c_len[k])
    cap = int((c_len + pad_h + pad_t).sum())
    head, tail = np.zeros(max(nc, 1), np.int32), np.zeros(max(nc, 1), np.int32)
    col_off = np.zeros(nc + 1, np.int64)
    tally = np.empty((max(cap, 1), 5), np.int64)
    rd, ro = np.ascontiguousarray(reads.data, dtype=np.uint8), np.ascontiguousarray(reads.offsets, dtype=np.int64)
    _check(load().mirge_cluster_pileup(ctx._h, rd if rd.size else None, ro, len(reads), c_len, row_start, nc, diag, count, head, tail, col_off,
                                       tally, cap), "mirge_cluster_pileup")
    return dict(head=head[:nc], tail=tail[:nc], col_off=col_off, tally=tally[:int(col_off[nc])])
