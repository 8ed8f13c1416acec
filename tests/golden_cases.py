"""The parity contract: every C++-path golden VCF of the reference's tests/run.py that the
scan/combine hot path produces, with the loader/query parameters run.py used for it
(reference tests/run.py:184-870 for the parameters, :935-947 for the vcf attribute order).

Each case: name, callsets json, vid json, query overrides, golden file, mode.
mode "query"  = gt_mpi_gather --produce-Broad-GVCF with vcf_attributes_order
mode "load"   = the loader's in-line combine (produce_combined_vcf): all schema attributes,
                one interval = the column partition.
"""
VCF_ATTRIBUTES_ORDER = ["END", "REF", "ALT", "BaseQRankSum", "ClippingRankSum", "MQRankSum", "ReadPosRankSum",
                        "MQ", "RAW_MQ", "MQ0", "DP", "GT", "GQ", "SB", "AD", "PL", "PGT", "PID", "MIN_DP",
                        "DP_FORMAT", "FILTER"]

FULL = [{"range_list": [{"low": 0, "high": 1000000000}]}]


def _r(lo, hi=1000000000):
    return [{"range_list": [{"low": lo, "high": hi}]}]


HT = "t0_haploid_triploid_1_2_3_triploid_deletion"

CASES = [
    # name, callsets, vid, query overrides, golden, mode
    ("t0_1_2_vcf_at_0", "t0_1_2.json", "vid.json", {"query_column_ranges": FULL}, "t0_1_2_vcf_at_0", "query"),
    ("t0_1_2_vcf_at_multiple_positions", "t0_1_2.json", "vid.json",
     {"query_column_ranges": [[12000, 12142, 12144, 12160, 12290, 12294, 14000, 17384, 18000]]},
     "t0_1_2_vcf_at_multiple_positions", "query"),
    ("t0_1_2_vcf_sites_only_at_0", "t0_1_2.json", "vid.json", {"query_column_ranges": FULL, "sites_only_query": True},
     "t0_1_2_vcf_sites_only_at_0", "query"),
    ("t0_1_2_vcf_at_12150", "t0_1_2.json", "vid.json", {"query_column_ranges": _r(12150)}, "t0_1_2_vcf_at_12150", "query"),
    ("t0_1_2_vcf_at_0_with_FILTER", "t0_1_2.json", "vid.json", {"query_column_ranges": FULL, "produce_FILTER_field": True},
     "t0_1_2_vcf_at_0_with_FILTER", "query"),
    ("t0_1_2_vcf_at_0_phased_GT_vid", "t0_1_2.json", "vid_phased_GT.json", {"query_column_ranges": FULL}, "t0_1_2_vcf_at_0", "query"),
    ("t0_1_2_loading", "t0_1_2.json", "vid.json", {}, "t0_1_2_loading", "load"),
    ("t0_1_2_as_array_loading", "t0_1_2_as_array.json", "vid_as_array.json", {}, "t0_1_2_loading", "load"),
    ("t0_overlapping_loading", "t0_overlapping.json", "vid.json", {}, "t0_overlapping", "load"),
    ("t0_overlapping_at_12202", "t0_overlapping.json", "vid.json", {"query_column_ranges": _r(12202)}, "t0_overlapping_at_12202", "query"),
    ("t0_overlapping_at_12202_partition_loading", "t0_overlapping.json", "vid.json", {"partition_begin": 12202},
     "t0_overlapping_at_12202", "load"),
    ("t6_7_8_vcf_at_0", "t6_7_8.json", "vid.json", {"query_column_ranges": FULL}, "t6_7_8_vcf_at_0", "query"),
    ("t6_7_8_loading", "t6_7_8.json", "vid.json", {}, "t6_7_8_loading", "load"),
    ("t6_7_8_vcf_sites_only_at_0", "t6_7_8.json", "vid.json", {"query_column_ranges": FULL, "sites_only_query": True},
     "t6_7_8_vcf_sites_only_at_0", "query"),
    ("t6_7_8_vcf_at_8029500", "t6_7_8.json", "vid.json", {"query_column_ranges": _r(8029500)}, "t6_7_8_vcf_at_8029500", "query"),
    ("t6_7_8_vcf_at_8029500-8029500", "t6_7_8.json", "vid.json", {"query_column_ranges": _r(8029500, 8029500)},
     "t6_7_8_vcf_at_8029500-8029500", "query"),
    ("t6_7_8_vcf_at_0_phased_GT_vid", "t6_7_8.json", "vid_phased_GT.json", {"query_column_ranges": FULL}, "t6_7_8_vcf_at_0", "query"),
    ("t6_7_8_new_field_gatk", "t6_7_8.json", "vid_MLEAC_MLEAF.json", {}, "t6_7_8_new_field_gatk.vcf", "load"),
    ("info_ops0", "info_ops.json", "vid_info_ops0.json", {}, "info_ops0.vcf", "load"),
    ("info_ops1", "info_ops.json", "vid_info_ops1.json", {}, "info_ops1.vcf", "load"),
    ("t0_1_2_DS_ID_vcf_at_0", "t0_1_2.json", "vid_DS_ID.json", {}, "t0_1_2_DS_ID_vcf_at_0", "load"),
    ("t0_with_missing_PL_SB_fields_t1", "t0_with_missing_PL_SB_fields_t1.json", "vid.json", {},
     "t0_with_missing_PL_SB_fields_t1.vcf", "load"),
    ("t0_1_2_all_asa_loading", "t0_1_2_all_asa.json", "vid_all_asa.json", {}, "t0_1_2_all_asa_loading", "load"),
    ("t0_1_2_combined", "t0_1_2_combined.json", "vid.json", {"query_column_ranges": FULL}, "t0_1_2_combined", "query"),
    ("t0_1_2_combined_loading", "t0_1_2_combined.json", "vid.json", {}, "t0_1_2_combined", "load"),
    (HT + "_loading", HT + ".json", "vid_DS_ID_phased_GT.json", {}, HT + "_loading", "load"),
    (HT + "_vcf", HT + ".json", "vid_DS_ID_phased_GT.json", {"query_column_ranges": FULL}, HT + "_vcf", "query"),
    (HT + "_vcf_produce_GT", HT + ".json", "vid_DS_ID_phased_GT.json", {"query_column_ranges": FULL, "produce_GT_field": True},
     HT + "_vcf_produce_GT", "query"),
    (HT + "_vcf_produce_GT_for_min_value_PL", HT + ".json", "vid_DS_ID_phased_GT.json",
     {"query_column_ranges": FULL, "produce_GT_field": True, "produce_GT_with_min_PL_value_for_spanning_deletions": True},
     HT + "_vcf_produce_GT_for_min_value_PL", "query"),
    (HT + "_vcf_sites_only", HT + ".json", "vid_DS_ID_phased_GT.json", {"query_column_ranges": FULL, "sites_only_query": True},
     HT + "_vcf_sites_only", "query"),
    ("min_PL_spanning_deletion_load_stdout", "min_PL_spanning_deletion.json", "vid_phased_GT.json", {},
     "min_PL_spanning_deletion_load_stdout", "load"),
    ("min_PL_spanning_deletion_vcf_no_min_PL", "min_PL_spanning_deletion.json", "vid_phased_GT.json",
     {"query_column_ranges": FULL, "produce_GT_field": True}, "min_PL_spanning_deletion_vcf_no_min_PL", "query"),
    ("min_PL_spanning_deletion_vcf", "min_PL_spanning_deletion.json", "vid_phased_GT.json",
     {"query_column_ranges": FULL, "produce_GT_field": True, "produce_GT_with_min_PL_value_for_spanning_deletions": True},
     "min_PL_spanning_deletion_vcf", "query"),
]

# Goldens of the hot path that are NOT covered yet, with the reason (kept visible on purpose).
UNCOVERED = {
}


# ---- the reference's java_vcf goldens: htsjdk's text of the BCF2 stream GenomicsDBFeatureReader opens -----------------------------------
# (reference tests/run.py:184-870; run.py:947 gives java_vcf the vcf_attributes_order like vcf.)  The stream is opened with is_bcf,
# use_missing_values_only_not_vector_end and without IDX keys (GenomicsDBQueryStream.java:39-41) and printed by tests/tools/htsjdk_text.py.
# The reference's spark_* goldens belong to its Spark input format and differ from their twins in the #CHROM line: out of scope.
ASA_VCF_ATTRIBUTES = VCF_ATTRIBUTES_ORDER + ["AS_RAW_MQ", "AS_RAW_MQRankSum"]      # run.py:55 (asa_vcf_attributes)

JAVA_CASES = [
    # name, callsets, vid, query overrides, java golden, C++ text twin (a golden of the same query, None when the reference has none)
    ("java_t0_1_2_vcf_at_0", "t0_1_2.json", "vid.json", {"query_column_ranges": FULL}, "java_t0_1_2_vcf_at_0", "t0_1_2_vcf_at_0"),
    ("java_t0_1_2_vcf_at_0_phased_GT_vid", "t0_1_2.json", "vid_phased_GT.json", {"query_column_ranges": FULL}, "java_t0_1_2_vcf_at_0",
     "t0_1_2_vcf_at_0"),
    ("java_t0_1_2_vcf_at_multiple_positions", "t0_1_2.json", "vid.json",
     {"query_column_ranges": [[12000, 12142, 12144, 12160, 12290, 12294, 14000, 17384, 18000]]},
     "java_t0_1_2_vcf_at_multiple_positions", "t0_1_2_vcf_at_multiple_positions"),
    ("java_t0_1_2_vcf_sites_only_at_0", "t0_1_2.json", "vid.json", {"query_column_ranges": FULL, "sites_only_query": True},
     "java_t0_1_2_vcf_sites_only_at_0", "t0_1_2_vcf_sites_only_at_0"),
    ("java_t0_1_2_vcf_at_12150", "t0_1_2.json", "vid.json", {"query_column_ranges": _r(12150)}, "java_t0_1_2_vcf_at_12150", "t0_1_2_vcf_at_12150"),
    ("java_t6_7_8_vcf_at_0", "t6_7_8.json", "vid.json", {"query_column_ranges": FULL}, "java_t6_7_8_vcf_at_0", "t6_7_8_vcf_at_0"),
    ("java_t6_7_8_vcf_at_8029500", "t6_7_8.json", "vid.json", {"query_column_ranges": _r(8029500)}, "java_t6_7_8_vcf_at_8029500",
     "t6_7_8_vcf_at_8029500"),
    ("java_t6_7_8_vcf_at_8029501", "t6_7_8.json", "vid.json", {"query_column_ranges": _r(8029501, 8029501)}, "java_t6_7_8_vcf_at_8029501", None),
    (HT + "_java_vcf", HT + ".json", "vid_DS_ID_phased_GT.json", {"query_column_ranges": FULL}, HT + "_java_vcf", HT + "_vcf"),
    (HT + "_java_vcf_produce_GT", HT + ".json", "vid_DS_ID_phased_GT.json", {"query_column_ranges": FULL, "produce_GT_field": True},
     HT + "_java_vcf_produce_GT", HT + "_vcf_produce_GT"),
    (HT + "_java_vcf_produce_GT_for_min_PL", HT + ".json", "vid_DS_ID_phased_GT.json",
     {"query_column_ranges": FULL, "produce_GT_field": True, "produce_GT_with_min_PL_value_for_spanning_deletions": True},
     HT + "_java_vcf_produce_GT_for_min_PL", HT + "_vcf_produce_GT_for_min_value_PL"),
    (HT + "_java_vcf_sites_only", HT + ".json", "vid_DS_ID_phased_GT.json", {"query_column_ranges": FULL, "sites_only_query": True},
     HT + "_java_vcf_sites_only", HT + "_vcf_sites_only"),
    ("t0_1_2_all_asa_java_query_vcf", "t0_1_2_all_asa.json", "vid_all_asa.json", {"query_column_ranges": FULL, "attributes": ASA_VCF_ATTRIBUTES},
     "t0_1_2_all_asa_java_query_vcf", "t0_1_2_all_asa_loading"),
]

# the rows the reference asks for as a contig interval (run.py:470-485): contig, 1-based begin, end - what GATK's query(chr, start, end)
# passes to jniGenomicsDBInit.  The column interval of the same records is the row's own query.
JAVA_CONTIG_INTERVALS = {
    "java_t6_7_8_vcf_at_8029500": ("1", 8029501, 8029510),
    "java_t6_7_8_vcf_at_8029501": ("1", 8029502, 8029502),
}

# goldens of a query over three arrays (run.py:337-365, chromosome_intervals 1:1-12160, 1:12161-12200, 1:12201-18000): one stream per
# column partition, imported on its own and asked for the part of the query columns inside it (GenomicsDBFeatureIterator.java:114-118),
# their records back to back under the first stream's header
JAVA_MULTI_ARRAY_CASES = [
    # name (= golden), callsets, vid, column partitions, query columns
    ("java_genomicsdb_importer_from_vcfs_t0_1_2_multi_contig_vcf_0_18000", "t0_1_2.json", "vid_phased_GT.json",
     [(0, 12159), (12160, 12199), (12200, 17999)], (0, 18000)),
    ("java_genomicsdb_importer_from_vcfs_t0_1_2_multi_contig_vcf_12150_18000", "t0_1_2.json", "vid_phased_GT.json",
     [(0, 12159), (12160, 12199), (12200, 17999)], (12150, 17999)),       # contig interval 1:12151-18000
]

# Java goldens that are NOT reproduced from the device's stream: name -> reason, with the first differing record
JAVA_UNCOVERED = {
}


# ---- gt_mpi_gather --print-calls(the reference's "calls" goldens, tests/run.py:184-720) ----------------------------------------
CALLS_ATTRIBUTES = ["REF", "ALT", "BaseQRankSum", "MQ", "RAW_MQ", "MQ0", "ClippingRankSum", "MQRankSum", "ReadPosRankSum", "DP", "GT", "GQ",
                    "SB", "AD", "PL", "DP_FORMAT", "MIN_DP", "PID", "PGT"]   # run.py:50 (the query template's "attributes")
CALLS_ATTRIBUTES_DS_ID = CALLS_ATTRIBUTES + ["DS", "ID"]


def _rl(*pairs):
    return [{"range_list": [{"low": lo, "high": hi} for lo, hi in pairs]}]


CALLS_CASES = [
    # name (= golden file), callsets, vid, query_column_ranges, attributes
    ("t0_1_2_calls_at_0", "t0_1_2.json", "vid.json", FULL, CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_multiple_positions", "t0_1_2.json", "vid.json", [[12000, 12142, 12144, 12160, 12290, 12294, 14000, 17384, 18000]], CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_12100", "t0_1_2.json", "vid.json", _rl((12100, 12100)), CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_12100_12141", "t0_1_2.json", "vid.json", _rl((12100, 12100), (12141, 12141)), CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_12100_12141_12150", "t0_1_2.json", "vid.json", _rl((12100, 12100), (12141, 12141), (12150, 12150)), CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_12100_12141_to_12150", "t0_1_2.json", "vid.json", _rl((12100, 12100), (12141, 12150)), CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_12100_12141_to_12150_12300_17384", "t0_1_2.json", "vid.json", _rl((12100, 12100), (12141, 12150), (12300, 12300), (17384, 17384)),
     CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_0_with_PL_only", "t0_1_2.json", "vid.json", FULL, ["PL"]),
    ("t0_1_2_calls_at_12150", "t0_1_2.json", "vid.json", _r(12150), CALLS_ATTRIBUTES),
    ("t6_7_8_calls_at_0", "t6_7_8.json", "vid.json", FULL, CALLS_ATTRIBUTES),
    ("t6_7_8_calls_at_8029500", "t6_7_8.json", "vid.json", _r(8029500), CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_0_phased_GT", "t0_1_2.json", "vid_phased_GT.json", FULL, CALLS_ATTRIBUTES),
    ("t0_1_2_calls_at_12150_phased_GT", "t0_1_2.json", "vid_phased_GT.json", _r(12150), CALLS_ATTRIBUTES),
    ("t6_7_8_calls_at_0_phased_GT", "t6_7_8.json", "vid_phased_GT.json", FULL, CALLS_ATTRIBUTES),
    ("t6_7_8_calls_at_8029500_phased_GT", "t6_7_8.json", "vid_phased_GT.json", _r(8029500), CALLS_ATTRIBUTES),
    ("test_new_fields_MLEAC_only.json", "t6_7_8.json", "vid_MLEAC_MLEAF.json", FULL, ["MLEAC"]),
    ("t0_1_2_DS_ID_calls_at_0", "t0_1_2.json", "vid_DS_ID.json", FULL, CALLS_ATTRIBUTES_DS_ID),
    ("t0_1_2_DS_ID_calls_at_0_phased_GT", "t0_1_2.json", "vid_DS_ID_phased_GT.json", FULL, CALLS_ATTRIBUTES_DS_ID),
    ("t0_with_missing_PL_SB_fields_t1_calls.json", "t0_with_missing_PL_SB_fields_t1.json", "vid.json", FULL, CALLS_ATTRIBUTES),
]
