"""genomicsdb_amd - MI355X-native variant-combine engine (scan + BroadCombinedGVCF hot path of GenomicsDB).

Python here is plumbing over the C ABI in include/genomicsdb_amd.h (libgenomicsdb_amd.so); the work happens in
the HIP kernels.  Mirrors the reference's caller-facing objects:
  GenomicsDBQueryStream  ~ com.intel.genomicsdb.reader.GenomicsDBQueryStream (JNI stream over GenomicsDBBCFGenerator)
  CombineEngine          ~ VariantQueryProcessor::scan_and_operate + BroadCombinedGVCFOperator on one column partition
"""
from .api import CombineEngine, GenomicsDBQueryStream, GenomicsDBException, import_cells, StreamImporter, chromosome_intervals, merge_cells, merge_cell_files, MERGE_FILES_STAT_NAMES, split_files, input_histogram, histogram_text, vcfdiff, index_vcf, INDEX_STAT_NAMES, bgzf_compress, bgzf_decompress, inflate_tiles, BGZF_EOF  # noqa: F401
