"""The reference's ten "variants" goldens (gt_mpi_gather without a mode flag, tests/run.py:935-942): each shares callsets, vid file, column
ranges and attributes with the "calls" query of the same run.py entry (:195-720), so the table is derived from CALLS_CASES by name."""
from golden_cases import CALLS_CASES

VARIANTS_GOLDENS = [
    "t0_1_2_variants_at_0", "t0_1_2_variants_at_12150", "t6_7_8_variants_at_0", "t6_7_8_variants_at_8029500",
    "t0_1_2_variants_at_0_phased_GT", "t0_1_2_variants_at_12150_phased_GT", "t6_7_8_variants_at_0_phased_GT", "t6_7_8_variants_at_8029500_phased_GT",
    "t0_1_2_DS_ID_variants_at_0", "t0_1_2_DS_ID_variants_at_0_phased_GT",
]
_calls = {c[0]: c for c in CALLS_CASES}
# name (= golden file), callsets, vid, query_column_ranges, attributes
VARIANTS_CASES = [(name,) + _calls[name.replace("_variants_", "_calls_")][1:] for name in VARIANTS_GOLDENS]
