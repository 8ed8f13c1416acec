import ctypes
import json
import os

from . import _lib

INT64_MAX = 2**63 - 1


class GenomicsDBException(RuntimeError):
    pass


def _check(ok, what):
    if not ok:
        raise GenomicsDBException("%s: %s" % (what, _lib.last_error()))


class _DevicePage:
    """an HBM page as an object torch can alias (CUDA array interface, version 2; ROCm builds of torch honour it)"""

    def __init__(self, addr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(addr), False), "version": 2}


class _DeviceArray:
    """a typed HBM array as an object torch can alias, like _DevicePage"""

    def __init__(self, addr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": typestr, "data": (int(addr), False), "version": 2}


# gdbamd dtype codes (include/genomicsdb_amd.h) <-> names, CUDA-array-interface type strings
COLUMN_DTYPES = {"int8": 1, "int16": 2, "int32": 3, "int64": 4, "float32": 5, "uint8": 6}
_COLUMN_TYPESTR = {1: "|i1", 2: "<i2", 3: "<i4", 4: "<i8", 5: "<f4", 6: "|u1"}


class GenomicsDBQueryStream:
    """Byte stream of the combined gVCF (header first), the Python face of the six JNI entry points."""

    def __init__(self, loader_json_file=None, query_json_file=None, chr="", start=0, end=0, rank=0, buffer_capacity=1048576,
                 segment_size=1048576, is_bcf=False, produce_header_only=False, query_json=None, cells=None,
                 use_missing_values_only_not_vector_end=False, keep_idx_fields_in_bcf_header=True, output_format=None, index=False):
        """output_format (the reference's vcf_output_format: "", "bu", "z", "b") overrides is_bcf when given.
        index=True ("z" / "b" only): the .tbi / .csi of the stream's bytes is built on the device while the pages are
        there; write_index(path) writes it once the stream has been read to its end"""
        self._open(loader_json_file, query_json_file, chr, start, end, rank, buffer_capacity, segment_size, is_bcf, produce_header_only, query_json, cells,
                   use_missing_values_only_not_vector_end, keep_idx_fields_in_bcf_header, output_format)
        if index:
            try:
                self.enable_index()
            except Exception:
                self.close()
                raise

    def _open(self, loader_json_file, query_json_file, chr, start, end, rank, buffer_capacity, segment_size, is_bcf, produce_header_only, query_json, cells,
              use_missing_values_only_not_vector_end, keep_idx_fields_in_bcf_header, output_format):
        L = _lib.lib()
        if output_format is not None:
            fmt = output_format.encode()
            if query_json is not None:
                txt = query_json if isinstance(query_json, str) else json.dumps(query_json)
                if isinstance(cells, tuple):
                    self._cells = None
                    self._h = L.gdb_mi355_init_from_memory_output_format(txt.encode(), ctypes.cast(cells[0], ctypes.c_char_p), cells[1], buffer_capacity, int(produce_header_only),
                                                                         fmt, int(use_missing_values_only_not_vector_end), int(keep_idx_fields_in_bcf_header))
                else:
                    self._cells = bytes(cells or b"")
                    self._h = L.gdb_mi355_init_from_memory_output_format(txt.encode(), self._cells, len(self._cells), buffer_capacity, int(produce_header_only), fmt,
                                                                         int(use_missing_values_only_not_vector_end), int(keep_idx_fields_in_bcf_header))
            else:
                self._h = L.gdb_mi355_init_output_format((loader_json_file or "").encode(), (query_json_file or "").encode(), chr.encode(), start, end, rank, buffer_capacity,
                                                         segment_size, fmt, int(produce_header_only), int(use_missing_values_only_not_vector_end), int(keep_idx_fields_in_bcf_header))
            _check(self._h, "GenomicsDBQueryStream init")
            return
        if query_json is not None:
            txt = query_json if isinstance(query_json, str) else json.dumps(query_json)
            if isinstance(cells, tuple):      # (host address, nbytes): cells that already lie in native memory (synthetic generator)
                self._cells = None
                self._h = L.gdb_mi355_init_from_memory_format(txt.encode(), ctypes.cast(cells[0], ctypes.c_char_p), cells[1], buffer_capacity, int(produce_header_only),
                                                              int(is_bcf), int(use_missing_values_only_not_vector_end), int(keep_idx_fields_in_bcf_header))
            else:
                self._cells = bytes(cells or b"")
                self._h = L.gdb_mi355_init_from_memory_format(txt.encode(), self._cells, len(self._cells), buffer_capacity, int(produce_header_only),
                                                              int(is_bcf), int(use_missing_values_only_not_vector_end), int(keep_idx_fields_in_bcf_header))
        else:
            self._h = L.gdb_mi355_init((loader_json_file or "").encode(), (query_json_file or "").encode(), chr.encode(), start, end, rank,
                                       buffer_capacity, segment_size, int(is_bcf), int(produce_header_only), int(use_missing_values_only_not_vector_end),
                                       int(keep_idx_fields_in_bcf_header))
        _check(self._h, "GenomicsDBQueryStream init")

    def read(self, n=-1):
        L = _lib.lib()
        chunks = []
        want = n if n >= 0 else None
        while want is None or want > 0:
            k = 1 << 20 if want is None else min(want, 1 << 20)
            buf = ctypes.create_string_buffer(k)
            got = L.gdb_mi355_read(self._h, buf, 0, k)
            if got < 0:
                raise GenomicsDBException("read: " + _lib.last_error())
            if got == 0:
                break
            chunks.append(buf.raw[:got])
            if want is not None:
                want -= got
        return b"".join(chunks)

    def read_into(self, addr, n):
        """up to n bytes of the stream into host memory at `addr` (e.g. a pinned torch tensor's data_ptr()); returns the count"""
        got = _lib.lib().gdb_mi355_read(self._h, addr, 0, n)
        if got < 0:
            raise GenomicsDBException("read: " + _lib.last_error())
        return got

    def stream_stats(self):
        st = _lib.StreamStats()
        _check(_lib.lib().gdb_mi355_get_stream_stats(self._h, ctypes.byref(st)) == 0, "stream_stats")
        return st

    def enable_index(self):
        """build the index of the stream's bytes on the device ("z" / "b" only, before the header has been read to its end)"""
        if _lib.lib().gdb_mi355_enable_index(self._h) != 0:
            raise GenomicsDBException("enable_index: " + _lib.last_error())

    def write_index(self, path):
        """the .tbi ("z") / .csi ("b") of the bytes this stream has handed out, to `path`; only once the stream has been read
        to its end.  -> dict of gdb_mi355_index_stats"""
        st = _lib.OutputIndexStats()
        if _lib.lib().gdb_mi355_write_index(self._h, os.fsencode(path), ctypes.byref(st)) != 0:
            raise GenomicsDBException("write_index: " + _lib.last_error())
        return {k: getattr(st, k) for k, _ in st._fields_}

    def skip(self, n):
        return _lib.lib().gdb_mi355_skip(self._h, n)

    def available(self):
        return _lib.lib().gdb_mi355_get_num_bytes_available(self._h)

    def close(self):
        if self._h:
            _lib.lib().gdb_mi355_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CombineEngine:
    """One column partition on one GPU: stage cells (or adopt device columns), run query intervals."""

    def __init__(self, query_json, device=0, is_bcf=False, use_missing_values_only_not_vector_end=False, output_format=None):
        L = _lib.lib()
        txt = query_json if isinstance(query_json, str) else json.dumps(query_json)
        if output_format is not None:
            self._e = L.gdbamd_engine_create_output_format(txt.encode(), device, output_format.encode(), int(use_missing_values_only_not_vector_end))
        else:
            self._e = L.gdbamd_engine_create_format(txt.encode(), device, int(is_bcf), int(use_missing_values_only_not_vector_end))
        _check(self._e, "CombineEngine create")
        self._keep = []

    @property
    def header(self):
        L = _lib.lib()
        n = L.gdbamd_engine_header(self._e, None, 0)
        buf = ctypes.create_string_buffer(n)
        L.gdbamd_engine_header(self._e, buf, n)
        return buf.raw[:n]

    def fields(self):
        L = _lib.lib()
        out = []
        for f in range(L.gdbamd_engine_num_fields(self._e)):
            et, var, num = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            L.gdbamd_engine_field_info(self._e, f, ctypes.byref(et), ctypes.byref(var), ctypes.byref(num))
            out.append({"name": L.gdbamd_engine_field_name(self._e, f).decode(), "elem": et.value, "var": bool(var.value), "num": num.value})
        return out

    def stage_cells(self, cells):
        cells = bytes(cells)
        _check(_lib.lib().gdbamd_engine_stage_cells(self._e, cells, len(cells)) == 0, "stage_cells")

    def stage_cells_begin(self):
        _check(_lib.lib().gdbamd_engine_stage_cells_begin(self._e) == 0, "stage_cells_begin")

    def stage_cells_append(self, ptr, nbytes):
        """ptr: host address (int / ctypes pointer) of `nbytes` of cells continuing the column-major order"""
        _check(_lib.lib().gdbamd_engine_stage_cells_append(self._e, ptr, nbytes) == 0, "stage_cells_append")

    def stage_cells_end(self):
        _check(_lib.lib().gdbamd_engine_stage_cells_end(self._e) == 0, "stage_cells_end")

    # ---- arrays larger than the staging budget: column windows streamed through HBM (see include/genomicsdb_amd.h) ----
    def open_array(self, directory):
        _check(_lib.lib().gdbamd_engine_open_array(self._e, str(directory).encode()) == 0, "open_array")

    def open_memory_cells(self, cells):
        """cells: bytes, or (host address, nbytes); kept alive by this object"""
        if isinstance(cells, tuple):
            addr, n = cells
        else:
            self._keep.append(bytes(cells))
            addr, n = ctypes.cast(ctypes.c_char_p(self._keep[-1]), ctypes.c_void_p).value, len(self._keep[-1])
        _check(_lib.lib().gdbamd_engine_open_memory_cells(self._e, addr, n) == 0, "open_memory_cells")

    def open_cell_callback(self, next_chunk):
        """next_chunk() -> (host address, nbytes) of the next whole-column chunk (valid until the next call) or None at the end"""
        def _fn(_user, pp, pn):
            r = next_chunk()
            if r is None:
                return 0
            pp[0], pn[0] = r[0], r[1]
            return 1
        cb = _lib.CELL_CHUNK_FN(_fn)
        self._keep.append(cb)
        _check(_lib.lib().gdbamd_engine_open_cell_callback(self._e, cb, None) == 0, "open_cell_callback")

    def cover(self, column):
        """stage windows until `column` is covered; returns (lo, hi): the query positions the staged fragment serves"""
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        _check(_lib.lib().gdbamd_engine_cover(self._e, column, ctypes.byref(lo), ctypes.byref(hi)) == 0, "cover")
        return lo.value, hi.value

    def adopt_device_fragment(self, ncells, row_ptr, begin_ptr, end_ptr, cols, reference_cell_bytes, keepalive=None):
        """cols: list of (data_ptr, off_ptr_or_0) device addresses, one per plan field."""
        arr = (_lib.DeviceColumn * len(cols))()
        for i, (d, o) in enumerate(cols):
            arr[i].data = d
            arr[i].off = o or None
        self._keep = [arr, keepalive]
        _check(_lib.lib().gdbamd_engine_adopt_device_fragment(self._e, ncells, row_ptr, begin_ptr, end_ptr, arr, len(cols), reference_cell_bytes) == 0,
               "adopt_device_fragment")

    def staged_info(self):
        n, b = ctypes.c_int64(), ctypes.c_uint64()
        _check(_lib.lib().gdbamd_engine_staged_info(self._e, ctypes.byref(n), ctypes.byref(b)) == 0, "staged_info")
        return n.value, b.value

    def set_reference(self, begin, bases):
        _check(_lib.lib().gdbamd_engine_set_reference(self._e, begin, bases, len(bases)) == 0, "set_reference")

    def print_calls(self, mode=0):
        """`gt_mpi_gather --print-calls` (mode 0: the JSON document of the cells of the query's column intervals, VariantCallPrintOperator),
        `--print-csv` (1) or `--print-AC` (2); bytes"""
        L = _lib.lib()
        L.gdbamd_engine_print_cells.restype = ctypes.c_int64
        L.gdbamd_engine_print_cells.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64]
        n = L.gdbamd_engine_print_cells(self._e, mode, None, 0)
        _check(n >= 0, "print_calls")
        buf = ctypes.create_string_buffer(max(1, n))
        _check(L.gdbamd_engine_print_cells(self._e, mode, buf, n) == n, "print_calls")
        return buf.raw[:n]

    def query_variants(self):
        """`gt_mpi_gather` without a mode flag / GenomicsDB::query_variants: the calls of the query's column intervals grouped into variants
        (same begin, end, REF and set of ALT), GT and allele-length fields of multi-call variants in merged allele order, as the reference's
        JSON document (print_variants' default format); selected, grouped and formatted on the device; bytes"""
        L = _lib.lib()
        L.gdbamd_engine_query_variants.restype = ctypes.c_int64
        L.gdbamd_engine_query_variants.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        n = L.gdbamd_engine_query_variants(self._e, None, 0)
        _check(n >= 0, "query_variants")
        buf = ctypes.create_string_buffer(max(1, n))
        _check(L.gdbamd_engine_query_variants(self._e, buf, n) == n, "query_variants")
        return buf.raw[:n]

    def print_csv(self):
        return self.print_calls(1)

    def print_allele_counts(self):
        return self.print_calls(2)

    def column_histogram(self, hist_begin, hist_end, bin_size, counts=None):
        """ColumnHistogramOperator on the device: numpy uint64 counts[(hist_end - hist_begin) // bin_size + 1] of the staged begin-cells by
        begin column (counts given: added to, for arrays streamed in windows)"""
        import numpy as np
        nbins = (hist_end - hist_begin) // bin_size + 1
        acc = counts is not None
        if counts is None:
            counts = np.zeros(nbins, dtype=np.uint64)
        assert counts.dtype == np.uint64 and counts.size == nbins and counts.flags["C_CONTIGUOUS"]
        L = _lib.lib()
        L.gdbamd_engine_column_histogram.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
        _check(L.gdbamd_engine_column_histogram(self._e, hist_begin, hist_end, bin_size, counts.ctypes.data, nbins, int(acc)) == 0, "column_histogram")
        return counts

    def split_point(self, begin, end, max_columns):
        """last column of the first piece of [begin, end] that can be run on its own with byte-identical output"""
        pe = ctypes.c_int64()
        _check(_lib.lib().gdbamd_engine_split_point(self._e, begin, end, max_columns, ctypes.byref(pe)) == 0, "split_point")
        return pe.value

    def save_fragment(self, path, compress=False):
        """the staged fragment as a columnar file; compress: DEFLATE tiles that are inflated on the device when the file is read"""
        fn = _lib.lib().gdbamd_engine_save_fragment_compressed if compress else _lib.lib().gdbamd_engine_save_fragment
        _check(fn(self._e, str(path).encode()) == 0, "save_fragment")

    def load_fragment(self, path):
        _check(_lib.lib().gdbamd_engine_load_fragment(self._e, str(path).encode()) == 0, "load_fragment")

    def run_interval(self, begin=0, end=INT64_MAX - 1, arena_bytes=1 << 30, fetch=True, host_cap=None):
        L = _lib.lib()
        st = _lib.IntervalStats()
        n = ctypes.c_uint64()
        if fetch:
            cap = host_cap or (1 << 26)
            while True:
                buf = ctypes.create_string_buffer(cap)
                rc = L.gdbamd_engine_run_interval(self._e, begin, end, arena_bytes, buf, cap, ctypes.byref(n), ctypes.byref(st))
                _check(rc == 0, "run_interval")
                if n.value <= cap:
                    return buf.raw[:n.value], st
                cap = n.value
        rc = L.gdbamd_engine_run_interval(self._e, begin, end, arena_bytes, None, 0, ctypes.byref(n), ctypes.byref(st))
        _check(rc == 0, "run_interval")
        return None, st

    def run_intervals(self, intervals, arena_bytes=1 << 30, lanes=2, fetch=False, host_cap=1 << 26):
        """several (begin, end) column intervals of the staged fragment, up to `lanes` in flight at a time on device pipelines that share
        the fragment (gdbamd_engine_run_intervals).  fetch=False: pages stay in HBM, returns the per-interval statistics in interval
        order; fetch=True: returns [(body bytes, statistics)]"""
        L = _lib.lib()
        n = len(intervals)
        b = (ctypes.c_int64 * max(1, n))(*[iv[0] for iv in intervals])
        e = (ctypes.c_int64 * max(1, n))(*[iv[1] for iv in intervals])
        st = (_lib.IntervalStats * max(1, n))()
        if not fetch:
            _check(L.gdbamd_engine_run_intervals(self._e, n, b, e, arena_bytes, lanes, st, None, None, None) == 0, "run_intervals")
            return [st[i] for i in range(n)]
        caps = [host_cap] * n
        while True:
            bufs = [ctypes.create_string_buffer(c) for c in caps]
            ptrs = (ctypes.c_char_p * max(1, n))(*[ctypes.cast(x, ctypes.c_char_p) for x in bufs])
            cap = (ctypes.c_uint64 * max(1, n))(*caps)
            lens = (ctypes.c_uint64 * max(1, n))()
            _check(L.gdbamd_engine_run_intervals(self._e, n, b, e, arena_bytes, lanes, st, ptrs, cap, lens) == 0, "run_intervals")
            if all(lens[i] <= caps[i] for i in range(n)):
                return [(bufs[i].raw[:lens[i]], st[i]) for i in range(n)]
            caps = [max(caps[i], lens[i]) for i in range(n)]

    def lane_footprint(self, interval_columns, arena_bytes=1 << 30):
        """HBM bytes a new lane pipeline of run_intervals takes at this query's sample count (gdbamd_engine_lane_footprint)"""
        n = ctypes.c_uint64(0)
        _check(_lib.lib().gdbamd_engine_lane_footprint(self._e, interval_columns, arena_bytes, ctypes.byref(n)) == 0, "lane_footprint")
        return n.value

    def release_lanes(self):
        """frees the lane pipelines run_intervals created (their HBM comes back; the next call creates them again)"""
        _check(_lib.lib().gdbamd_engine_release_lanes(self._e) == 0, "release_lanes")

    def pages(self, begin=0, end=INT64_MAX - 1, arena_bytes=1 << 30):
        """the VCF body of one column interval page by page, left in HBM: yields (device address, nbytes); an address is valid
        until the next page is asked for"""
        L = _lib.lib()
        _check(L.gdbamd_engine_prepare_interval(self._e, begin, end) == 0, "prepare_interval")
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        while True:
            rc = L.gdbamd_engine_next_page(self._e, arena_bytes, ctypes.byref(p), ctypes.byref(n))
            _check(rc >= 0, "next_page")
            if rc == 0:
                return
            yield p.value, n.value

    def page_tensors(self, begin=0, end=INT64_MAX - 1, arena_bytes=1 << 30, device=None):
        """pages() as torch uint8 tensors that alias the HBM page (no copy); a tensor is valid until the next page is asked for"""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        for addr, n in self.pages(begin, end, arena_bytes):
            yield torch.as_tensor(_DevicePage(addr, n), device=dev)

    def record_tensors(self, begin=0, end=INT64_MAX - 1, fields=None, arena_bytes=1 << 30, device=None, stats=None):
        """The combined records of one column interval page by page as typed torch tensors that alias HBM (decoded on the device from the
        BCF2 page; the engine's output format must be "bu").  Yields a dict name -> tensor: contig int32[R], pos / end / column int64[R],
        qual float32[R], n_allele int32[R], alleles uint8[total] with alleles_off int64[R + 1], and per entry of `fields` - name ->
        dtype name ("int8", "int16", "int32", "float32", None: the field's own), or name -> (dtype, width) - a FORMAT field as [R, N, W],
        an INFO field as [R, W]; GT comes with GT_phase uint8[R, N, W].  Sentinels are BCF's for the dtype (missing -128 / -32768 /
        -2**31 / 0x7F800001 as bits, end-of-vector the next value up; GT: -1 is missing).  A tensor is valid until the next iteration:
        clone what has to live longer.  stats: a list that receives one dict of gdbamd_columns_stats per page."""
        import torch
        L = _lib.lib()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        names = list(fields or {})
        req = (_lib.ColumnRequest * max(1, len(names)))()
        for i, name in enumerate(names):
            spec = (fields[name], 0) if not isinstance(fields[name], (tuple, list)) else fields[name]
            if spec[0] is not None and spec[0] not in COLUMN_DTYPES:
                raise GenomicsDBException("record_tensors: field %s: unknown dtype %r" % (name, spec[0]))
            req[i].name, req[i].dtype, req[i].width = name.encode(), COLUMN_DTYPES.get(spec[0], 0), int(spec[1])
        _check(L.gdbamd_engine_columns_select(self._e, req, len(names)) == 0, "record_tensors")
        cols = (_lib.Column * (8 + 2 * len(names)))()
        n, st = ctypes.c_int(), _lib.ColumnsStats()
        for _ in self.pages(begin, end, arena_bytes):
            _check(L.gdbamd_engine_page_columns(self._e, cols, len(cols), ctypes.byref(n), ctypes.byref(st)) == 0, "record_tensors")
            out = {}
            for c in cols[:n.value]:
                shape = tuple(c.shape[:c.ndim])
                tdtype = getattr(torch, [k for k, v in COLUMN_DTYPES.items() if v == c.dtype][0])
                if 0 in shape:
                    out[c.name.decode()] = torch.empty(shape, dtype=tdtype, device=dev)
                else:
                    out[c.name.decode()] = torch.as_tensor(_DeviceArray(c.dev_ptr, shape, _COLUMN_TYPESTR[c.dtype]), device=dev)
            if stats is not None:
                stats.append({"records": st.records, "bytes_read": st.bytes_read, "bytes_written": st.bytes_written, "ms_measure": st.ms_measure,
                              "ms_site": st.ms_site, "ms_scatter": st.ms_scatter, "width": {name: st.width[i] for i, name in enumerate(names)}})
            yield out

    def close(self):
        if self._e:
            _lib.lib().gdbamd_engine_destroy(self._e)
            self._e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pin_host_memory(addr, nbytes):
    """page-lock the caller's host range so that staging copies out of it are DMA transfers (gdbamd_pin_host_memory)"""
    _check(_lib.lib().gdbamd_pin_host_memory(addr, nbytes) == 0, "pin_host_memory")


def unpin_host_memory(addr):
    _check(_lib.lib().gdbamd_unpin_host_memory(addr) == 0, "unpin_host_memory")


IMPORT_STAT_NAMES = ("num_files", "num_records", "num_cells", "num_spanning_cells", "num_bytes", "num_deferred_values", "num_batches", "text_bytes",
                     "ms_index", "ms_measure", "ms_write", "ms_sort_gather", "s_read", "s_h2d", "s_deferred", "s_d2h", "s_total",
                     "compressed_bytes", "num_device_members", "num_host_inflated_files", "ms_inflate", "bytes_h2d")
INFLATE_MODES = {"auto": 0, "host": 1, "device": 2}


def import_cells(vid_mapping_file, callset_mapping_file, file_root="", treat_deletions_as_intervals=True, column_begin=0, column_end=2**63 - 2,
                 device=None, text_budget_bytes=0, stats=None, inflate="auto", streams=None, lb_callset_row_idx=0, ub_callset_row_idx=2**63 - 2):
    """(g)VCFs of a callset mapping -> begin-cells (bytes, reference binary cell layout, column-major) of one column partition:
    the conversion step of the reference's vcf2tiledb (vcf2binary.cc:991-1196).
    device=None: host code, no device needed.  device=<int>: the conversion runs on that GPU (kernels/gdb_import.hip) and gives
    the same bytes; text_budget_bytes is the record text per batch (0: default) and `stats`, a dict, receives IMPORT_STAT_NAMES.
    inflate (device path only): "auto" - bgzip'ed (BGZF) files cross the link compressed and are inflated on the device
    (kernels/gdb_inflate.hip), every other file goes through zlib on the host; "host" - zlib for every file; "device" - a file that
    is not BGZF is an error.  A BGZF member with a bad stream, ISIZE or CRC32 refuses the import.
    BCF2 (device path only): a file whose content - plain, BGZF or gzip - begins with 'BCF\\2\\1' or 'BCF\\2\\2' is imported as BCF2 and
    gives the cells of the same records as VCF text; compressed BCF2 is inflated on the host (inflate="device" refuses it), and the
    host importer refuses a BCF2 file by name.  streams (device path only): {name: bytes} - a callset whose "filename" equals a name is
    read from those bytes (VCF text or BCF2, plain or gzip) instead of a file; a name that no callset uses is an error.
    CSV cell files (device path only): a "filename" that the callset mapping also lists under "sorted_csv_files" / "unsorted_csv_files"
    is read as the reference loader's CSV input, one line = one cell (csrc/core/gdb_import_csv.hpp); from a file or from streams=.
    lb_callset_row_idx / ub_callset_row_idx (the loader JSON keys of an incremental import, host and device path): only the callsets
    whose row_idx lies inside are converted - clamped as the reference does (negative -> 0, swapped when reversed, capped at the
    mapping's largest row).  A file or stream without such a callset is not opened and not counted in stats["num_files"] (which the
    host path fills too); merge_cells puts the batch next to the cells an array already holds."""
    if inflate not in INFLATE_MODES:
        raise ValueError("inflate=%r: one of %s" % (inflate, sorted(INFLATE_MODES)))
    if streams is not None and device is None:
        raise ValueError("streams= needs device=: the host importer reads files only")
    L = _lib.lib()
    p = ctypes.c_void_p()
    n = ctypes.c_uint64()
    nc = ctypes.c_int64()
    if device is None:
        nf = ctypes.c_int64()
        rc = L.gdbamd_import_cells_rows(os.fsencode(vid_mapping_file), os.fsencode(callset_mapping_file), os.fsencode(file_root or ""), 1 if treat_deletions_as_intervals else 0,
                                        column_begin, column_end, ctypes.byref(p), ctypes.byref(n), ctypes.byref(nc), int(lb_callset_row_idx), int(ub_callset_row_idx),
                                        ctypes.byref(nf))
        if rc == 0 and stats is not None:
            stats.update({"num_files": nf.value, "num_cells": nc.value, "num_bytes": n.value})
    else:
        st = (ctypes.c_double * len(IMPORT_STAT_NAMES))()
        items = [(os.fsencode(k), bytes(v)) for k, v in (streams or {}).items()]
        ns = len(items)
        names = (ctypes.c_char_p * max(ns, 1))(*[k for k, _ in items])
        data = (ctypes.c_void_p * max(ns, 1))(*[ctypes.cast(ctypes.c_char_p(v), ctypes.c_void_p) for _, v in items])      # (items keeps the bytes alive)
        sizes = (ctypes.c_uint64 * max(ns, 1))(*[len(v) for _, v in items])
        rc = L.gdbamd_import_cells_device_rows(os.fsencode(vid_mapping_file), os.fsencode(callset_mapping_file), os.fsencode(file_root or ""),
                                                  1 if treat_deletions_as_intervals else 0, column_begin, column_end, ctypes.byref(p), ctypes.byref(n), ctypes.byref(nc),
                                                  int(device), int(text_budget_bytes), INFLATE_MODES[inflate], st, len(IMPORT_STAT_NAMES), ns, names, data, sizes,
                                               int(lb_callset_row_idx), int(ub_callset_row_idx))
        if rc == 0 and stats is not None:
            stats.update({k: (float(v) if k[:2] in ("ms", "s_") else int(v)) for k, v in zip(IMPORT_STAT_NAMES, st)})
    _check(rc == 0, "import_cells")
    try:
        return ctypes.string_at(p.value, n.value), nc.value
    finally:
        L.gdbamd_free(p)


STREAM_IMPORT_STAT_NAMES = ("num_batches", "num_records", "num_cells", "num_bytes", "max_pending_cells", "max_pending_bytes", "num_deferred_values",
                            "num_spanning_cells", "ms_order", "ms_classify", "ms_sort_gather", "ms_compact", "s_h2d", "s_d2h")


class StreamImporter:
    """The reference's GenomicsDBImporter protocol on one GPU (csrc/api/genomicsdb_importer.h, kernels/gdb_import_stream.hip): buffer
    streams of VCF text or BCF2 records are imported batch by batch, with bounded device memory.

        imp = StreamImporter(loader_json)                 # a path, or a dict / JSON text
        imp.add_buffer_stream(name, is_bcf, capacity, header_bytes)       # once per stream
        used = imp.setup(callsets_json)                   # -> per stream its index among the sources of the callset mapping, -1: unused
        while not imp.done:
            cells, exhausted = imp.import_batch()         # cells of this batch (column-major), [(stream, 0), ...] to refill
            for idx, _ in exhausted:
                imp.write(idx, whole_records)             # b"" (or no write) ends the stream
        imp.finish()                                      # the loader's outputs, as vcf2tiledb makes them

    The batches' cells, concatenated, are import_cells() of the same records.  A batch hands over every pending cell whose column is
    strictly below W, the smallest last column over the streams that have not ended, and reports the streams whose last column is not
    above W.  Errors (GenomicsDBException) name the stream and the record or byte offset; after one, the importer can only be closed."""

    def __init__(self, loader_json, rank=0, device=0):
        import json
        self._L = _lib.lib()
        self._n = 0
        self._max = 0
        text = json.dumps(loader_json) if isinstance(loader_json, dict) else loader_json
        self._h = self._L.gdbamd_importer_create(os.fsencode(text), int(rank), int(device))
        _check(self._h, "StreamImporter")

    def _handle(self):
        if not self._h:
            raise GenomicsDBException("StreamImporter is closed")
        return self._h

    def add_buffer_stream(self, name, is_bcf, capacity, init=b""):
        init = bytes(init)
        _check(self._L.gdbamd_importer_add_buffer_stream(self._handle(), os.fsencode(name), 1 if is_bcf else 0, int(capacity), init, len(init)) == 0, "add_buffer_stream")
        self._n += 1
        return self._n - 1

    def setup(self, callsets_json=""):
        import json
        text = json.dumps(callsets_json) if isinstance(callsets_json, dict) else (callsets_json or "")
        n = ctypes.c_int64()
        _check(self._L.gdbamd_importer_setup_loader(self._handle(), text.encode(), ctypes.byref(n)) == 0, "setup_loader")
        self._max = n.value
        out = []
        for i in range(self._n):
            f = ctypes.c_int64()
            _check(self._L.gdbamd_importer_stream_file_idx(self._h, i, ctypes.byref(f)) == 0, "stream_file_idx")
            out.append(f.value)
        return out

    @property
    def max_identifiers(self):
        return self._max

    def write(self, idx, data, partition_idx=0):
        data = bytes(data)
        _check(self._L.gdbamd_importer_write(self._handle(), int(idx), int(partition_idx), data, len(data)) == 0, "write_data_to_buffer_stream")

    def import_batch(self):
        p = ctypes.c_void_p()
        n = ctypes.c_uint64()
        pairs = (ctypes.c_int64 * (2 * max(self._max, 1)))()
        ne = ctypes.c_int64()
        _check(self._L.gdbamd_importer_import_batch(self._handle(), ctypes.byref(p), ctypes.byref(n), pairs, ctypes.byref(ne)) == 0, "import_batch")
        try:
            cells = ctypes.string_at(p.value, n.value)
        finally:
            self._L.gdbamd_free(p)
        return cells, [(pairs[2 * i], pairs[2 * i + 1]) for i in range(ne.value)]

    @property
    def done(self):
        r = self._L.gdbamd_importer_is_done(self._handle())
        _check(r >= 0, "is_done")
        return r == 1

    def finish(self):
        _check(self._L.gdbamd_importer_finish(self._handle()) == 0, "finish")

    def stats(self):
        st = (ctypes.c_double * len(STREAM_IMPORT_STAT_NAMES))()
        _check(self._L.gdbamd_importer_stats(self._handle(), st) == 0, "stats")
        return {k: (float(v) if k[:2] in ("ms", "s_") else int(v)) for k, v in zip(STREAM_IMPORT_STAT_NAMES, st)}

    def close(self):
        if self._h:
            self._L.gdbamd_importer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chromosome_intervals(loader_json, rank=0):
    """{"contigs": [{name: [begin, end]}, ...]}: the 1-based contig intervals that column partition `rank` of the loader JSON (a path, a
    dict or JSON text) covers - what the reference's jniGetChromosomeIntervalsForColumnPartition returns; -> the JSON text"""
    import json
    text = json.dumps(loader_json) if isinstance(loader_json, dict) else loader_json
    p = ctypes.c_void_p()
    L = _lib.lib()
    _check(L.gdbamd_chromosome_intervals_for_column_partition(os.fsencode(text), int(rank), ctypes.byref(p)) == 0, "chromosome_intervals")
    try:
        return ctypes.string_at(p.value).decode()
    finally:
        L.gdbamd_free(p)


SPLIT_STAT_NAMES = ("num_files", "num_record_lines", "num_lines_written", "text_bytes_in", "text_bytes_out", "compressed_bytes_out", "num_batches", "ms_index",
                    "ms_classify", "ms_scan_gather", "ms_deflate", "s_read", "s_h2d", "s_d2h_write", "s_index_build", "s_total", "ms_inflate", "ms_index_kernels")


def split_files(vid_mapping_file, callset_mapping_file, partitions, results_directory=None, file_root="", produce=None, device=0, text_budget_bytes=0, stats=None,
                output_filename=None, extra_files=(), inflate="auto", index_on_device=False):
    """vcf2tiledb --split-files on GPU `device` (kernels/gdb_split.hip): every (g)VCF text file of the callset mapping (plain, gzip or
    BGZF), then `extra_files`, cut into one BGZF file + .tbi per column partition in one pass per file.  partitions: [(begin, end)]
    per partition index, as the loader JSON's column_partitions give them with derived ends (column_partition()).  A partition's
    file holds every '#' line and, verbatim and in file order, every record line whose interval [col, tend] overlaps it (tend from
    INFO END, else col + len(REF) - 1); a line that spans partitions goes to each.  produce: one partition index, None for all.
    Outputs: <results_directory or the input's directory>/partition_<p>_<basename>, or what the callset mapping's
    "split_files_paths" names; output_filename names the output of exactly one input and one partition.
    -> {(original filename, partition index): output path}.  BCF2 and CSV inputs are refused by name; a line error names file
    and line and leaves no output of that input.  index_on_device: each output's .tbi is built on the GPU while the output is written
    (kernels/gdb_index.hip), from its text that is still in device memory and the blocks just deflated, instead of by the host builder
    re-reading the finished file; the files are the same, byte for byte.  `stats`, a dict, receives SPLIT_STAT_NAMES (s_index_build:
    wall clock of index building on either path, ms_index_kernels: its device share)."""
    if inflate not in INFLATE_MODES:
        raise ValueError("inflate=%r: one of %s" % (inflate, sorted(INFLATE_MODES)))
    L = _lib.lib()
    parts = [(int(b), int(e)) for b, e in partitions]
    n = len(parts)
    begins = (ctypes.c_int64 * max(n, 1))(*[b for b, _ in parts])
    ends = (ctypes.c_int64 * max(n, 1))(*[e for _, e in parts])
    extra = [os.fsencode(p) for p in extra_files]
    extra_arr = (ctypes.c_char_p * max(len(extra), 1))(*extra)
    st = (ctypes.c_double * len(SPLIT_STAT_NAMES))()
    out = ctypes.c_void_p()
    rc = L.gdbamd_split_files_device_index(os.fsencode(vid_mapping_file), os.fsencode(callset_mapping_file), os.fsencode(file_root or ""), n, begins, ends,
                                     -1 if produce is None else int(produce), os.fsencode(results_directory or ""), os.fsencode(output_filename or ""), int(device),
                                     int(text_budget_bytes), INFLATE_MODES[inflate], len(extra), extra_arr, st, len(SPLIT_STAT_NAMES), ctypes.byref(out),
                                           1 if index_on_device else 0)
    _check(rc == 0, "split_files")
    try:
        text = ctypes.string_at(out.value).decode()
    finally:
        L.gdbamd_free(out)
    if stats is not None:
        stats.update({k: (float(v) if k[:2] in ("ms", "s_") else int(v)) for k, v in zip(SPLIT_STAT_NAMES, st)})
    result = {}
    for line in text.splitlines():
        original, p, path = line.split("\t")
        result[(original, int(p))] = path
    return result


INDEX_STAT_NAMES = tuple(name for name, _ in _lib.IndexStats._fields_)


def index_vcf(path, device=0, text_budget_bytes=0, stats=None):
    """<path>.tbi of a bgzipped VCF, built on GPU `device` (kernels/gdb_index.hip): the file the host builder writes, byte for byte.  The
    file crosses the link compressed and is inflated and indexed on the device in batches of whole lines of about text_budget_bytes
    (0: 64 MiB); the result does not depend on where the batches are cut.  Refused: a file that is not BGZF from its first byte to its
    last (the error names the byte offset), a member with a bad stream, ISIZE or CRC32, a record with POS < 1 or POS / END >= 2^31 (file
    and 1-based line); after an error no .tbi exists.  -> the index path.  `stats`, a dict, receives INDEX_STAT_NAMES."""
    L = _lib.lib()
    st = _lib.IndexStats()
    rc = L.gdbamd_index_vcf_device(os.fsencode(path), int(device), int(text_budget_bytes), ctypes.byref(st))
    _check(rc == 0, "index_vcf")
    if stats is not None:
        stats.update({k: getattr(st, k) for k in INDEX_STAT_NAMES})
    return os.fspath(path) + ".tbi"


HISTOGRAM_STAT_NAMES = tuple(name for name, _ in _lib.HistogramStats._fields_)


def input_histogram(vid_mapping_file, callset_mapping_file, max_histogram_range, num_bins, file_root="", column_begin=0, column_end=2**63 - 2,
                    lb_callset_row_idx=0, ub_callset_row_idx=2**63 - 2, device=0, text_budget_bytes=0, inflate="auto", streams=None, stats=None):
    """vcf_histogram on GPU `device` (kernels/gdb_histogram.hip): one pass over every input file of the callset mapping ((g)VCF text -
    plain, gzip or BGZF - and BCF2; `streams`, {filename: bytes}, gives files from memory as for import_cells) counts the records per
    bin of a uniform histogram over the columns [0, max_histogram_range]: size_of_bin = ceil((max_histogram_range + 1) / num_bins),
    bin = column // size_of_bin.  A record counts iff its column (contig offset + POS - 1) lies in [column_begin, column_end], once
    per callset of its file whose row lies in the row bounds.  -> numpy uint64 array of num_bins counts.  CSV cell files are refused
    by name; a counted column above max_histogram_range and a line the splitter would refuse raise an error that names file and
    1-based line / record.  `stats`, a dict, receives HISTOGRAM_STAT_NAMES."""
    import numpy as np
    if inflate not in INFLATE_MODES:
        raise ValueError("inflate=%r: one of %s" % (inflate, sorted(INFLATE_MODES)))
    if int(num_bins) < 0:
        raise ValueError("num_bins=%r is negative" % (num_bins,))
    L = _lib.lib()
    items = [(os.fsencode(k), bytes(v)) for k, v in (streams or {}).items()]
    ns = len(items)
    names = (ctypes.c_char_p * max(ns, 1))(*[k for k, _ in items])
    data = (ctypes.c_void_p * max(ns, 1))(*[ctypes.cast(ctypes.c_char_p(v), ctypes.c_void_p) for _, v in items])      # (items keeps the bytes alive)
    sizes = (ctypes.c_uint64 * max(ns, 1))(*[len(v) for _, v in items])
    counts = np.zeros(max(int(num_bins), 1), dtype=np.uint64)
    st = _lib.HistogramStats()
    rc = L.gdbamd_input_histogram(os.fsencode(vid_mapping_file), os.fsencode(callset_mapping_file), os.fsencode(file_root or ""), int(max_histogram_range), int(num_bins),
                                  int(column_begin), int(column_end), int(lb_callset_row_idx), int(ub_callset_row_idx), int(device), int(text_budget_bytes),
                                  INFLATE_MODES[inflate], ns, names, data, sizes, counts.ctypes.data, ctypes.byref(st))
    _check(rc == 0, "input_histogram")
    if stats is not None:
        stats.update({k: getattr(st, k) for k in HISTOGRAM_STAT_NAMES})
    return counts


def histogram_text(counts, max_histogram_range):
    """Histogram::print of the reference for the counts of input_histogram: "Histogram: [", one "lo,hi,count" line per non-zero
    bin, "]"; -> str"""
    import numpy as np
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    L = _lib.lib()
    n = L.gdbamd_histogram_text(counts.ctypes.data, counts.size, int(max_histogram_range), None, 0)
    if n < 0:
        raise ValueError("histogram_text: no bin, or a negative max_histogram_range")
    buf = ctypes.create_string_buffer(n + 1)
    L.gdbamd_histogram_text(counts.ctypes.data, counts.size, int(max_histogram_range), buf, n)
    return buf.raw[:n].decode()


VCFDIFF_STAT_NAMES = tuple(name for name, _ in _lib.VcfDiffStats._fields_)


def vcfdiff(gold, test, threshold=1e-5, regions="", device=0, text_budget_bytes=0, stats=None):
    """vcfdiff on GPU `device` (kernels/gdb_vcfdiff.hip): the VCF text files `gold` and `test` (plain, gzip or BGZF) compared record by
    record, the order of ALT alleles (AD / PL / AF and the like are compared through the allele permutation), of INFO keys, FORMAT keys
    and sample columns and float noise below `threshold` aside; DESIGN.md, "Comparing two VCFs", has the rule.  regions: chr | chr:pos |
    chr:from-to | chr:from- , comma separated.  -> {"compared": pairs compared, "events": [...]}: in order, every event that is not a
    clean COMPARED pair, with its kind, the 1-based line numbers, the lines, the flag names and the field names per mask.  BCF2 input,
    differing sample names and more than 64 INFO or FORMAT names are refused; a line error names file and 1-based line.  `stats`, a
    dict, receives VCFDIFF_STAT_NAMES."""
    import json
    L = _lib.lib()
    p = ctypes.c_void_p()
    st = _lib.VcfDiffStats()
    rc = L.gdbamd_vcfdiff(os.fsencode(gold), os.fsencode(test), float(threshold), os.fsencode(regions or ""), int(device), int(text_budget_bytes), ctypes.byref(p),
                          ctypes.byref(st))
    _check(rc == 0, "vcfdiff")
    if stats is not None:
        stats.update({k: getattr(st, k) for k in VCFDIFF_STAT_NAMES})
    try:
        return json.loads(ctypes.string_at(p.value).decode())
    finally:
        L.gdbamd_free(p)


MERGE_STAT_NAMES = ("num_streams", "cells_in", "cells_out", "bytes_out", "tile", "ms_keys", "ms_rank", "ms_scan", "ms_gather", "s_h2d", "s_d2h", "s_total")


def merge_cells(streams, device=0, stats=None):
    """k >= 1 streams of begin-cells (bytes; each in column-major (column, row) order, as import_cells or a cells.bin gives them) ->
    (bytes, ncells) of the one stream in that order, merged on GPU `device` (kernels/gdb_merge.hip): how the batch of an incremental
    import joins the cells an array already holds.  Only each cell's 24-byte header is read.  Raises, with nothing returned, for a
    size chain that runs past its stream's end, a stream that is not sorted, a negative row and a row that two streams share.
    `stats`, a dict, receives MERGE_STAT_NAMES ("tile": output cells per workgroup of the rank kernel)."""
    L = _lib.lib()
    items = [bytes(s) for s in streams]
    k = len(items)
    if k == 0:
        raise ValueError("merge_cells: at least one stream")
    data = (ctypes.c_void_p * k)(*[ctypes.cast(ctypes.c_char_p(v), ctypes.c_void_p) for v in items])      # (items keeps the bytes alive)
    sizes = (ctypes.c_uint64 * k)(*[len(v) for v in items])
    p = ctypes.c_void_p()
    n = ctypes.c_uint64()
    nc = ctypes.c_int64()
    st = (ctypes.c_double * len(MERGE_STAT_NAMES))()
    rc = L.gdbamd_merge_cells(k, data, sizes, ctypes.byref(p), ctypes.byref(n), ctypes.byref(nc), int(device), st, len(MERGE_STAT_NAMES))
    _check(rc == 0, "merge_cells")
    if stats is not None:
        stats.update({name: (float(v) if name[:2] in ("ms", "s_") else int(v)) for name, v in zip(MERGE_STAT_NAMES, st)})
    try:
        # (ctypes.string_at takes a C int: a merged array of 2 GiB and more goes the long way)
        return (ctypes.string_at(p.value, n.value) if n.value < (1 << 31) else bytes((ctypes.c_ubyte * n.value).from_address(p.value))), nc.value
    finally:
        L.gdbamd_free(p)


MERGE_FILES_STAT_NAMES = MERGE_STAT_NAMES + ("rounds", "carried_cells", "grown", "window_bytes", "device_bytes_peak", "pinned_bytes", "s_read", "s_write", "s_wait_device")


def merge_cell_files(sources, output, device=0, window_bytes=0, stats=None):
    """merge_cells from files to a file, for arrays larger than device memory: `sources` mixes paths (str: files of begin-cells, read
    window by window) and bytes; their cells go to the file `output` in (column, row) order, byte for byte what merge_cells gives,
    through <output>.merge.tmp.  `window_bytes` caps the input cell bytes resident on GPU `device` over all sources (0: derived from
    the free device memory); device memory is about 8.7 times that, whatever the sources' lengths.  Raises as merge_cells does, with
    cell indices and byte offsets counted from the start of the source, and then leaves neither file.  Returns the number of cells.
    `stats`, a dict, receives MERGE_FILES_STAT_NAMES ("rounds", "carried_cells" summed over them, "grown": rounds that had to double
    a source's share of the window)."""
    L = _lib.lib()
    items = [os.fsencode(s) if isinstance(s, (str, os.PathLike)) else bytes(s) for s in sources]
    is_path = [isinstance(s, (str, os.PathLike)) for s in sources]
    k = len(items)
    if k == 0:
        raise ValueError("merge_cell_files: at least one source")
    paths = (ctypes.c_char_p * k)(*[v if p else None for v, p in zip(items, is_path)])
    data = (ctypes.c_void_p * k)(*[None if p else ctypes.cast(ctypes.c_char_p(v), ctypes.c_void_p) for v, p in zip(items, is_path)])      # (items keeps the bytes alive)
    sizes = (ctypes.c_uint64 * k)(*[0 if p else len(v) for v, p in zip(items, is_path)])
    st = (ctypes.c_double * len(MERGE_FILES_STAT_NAMES))()
    n = L.gdbamd_merge_cell_files(k, paths, data, sizes, os.fsencode(output), int(device), int(window_bytes), st, len(MERGE_FILES_STAT_NAMES))
    _check(n >= 0, "merge_cell_files")
    if stats is not None:
        stats.update({name: (float(v) if name[:2] in ("ms", "s_") else int(v)) for name, v in zip(MERGE_FILES_STAT_NAMES, st)})
    return n


def bgzf_compress(data, vcf_text=False):
    """BGZF blocks (no EOF block) of `data`, deflated by the device kernels (kernels/gdb_bgzf.hip); returns (bytes, kernel ms).
    vcf_text: the anchored kernel of the "z" stream (matches begin at tabs / newlines) instead of the byte-level one"""
    L = _lib.lib()
    data = bytes(data)
    cap = L.gdbamd_bgzf_bound(len(data))
    dst = ctypes.create_string_buffer(cap)
    n = ctypes.c_uint64()
    ms = ctypes.c_float()
    _check(L.gdbamd_bgzf_compress_mode(data, len(data), dst, cap, ctypes.byref(n), ctypes.byref(ms), 1 if vcf_text else 0) == 0, "bgzf_compress")
    return dst.raw[:n.value], ms.value


def bgzf_decompress(data, device=0):
    """the bytes of a whole BGZF buffer, inflated and verified (stream, ISIZE, CRC32 per member) by the device kernel of
    kernels/gdb_inflate.hip; returns (bytes, kernel ms).  A bad member raises an error that names its byte offset."""
    L = _lib.lib()
    data = bytes(data)
    n = ctypes.c_uint64()
    ms = ctypes.c_float()
    _check(L.gdbamd_bgzf_decompress(data, len(data), None, 0, ctypes.byref(n), None, int(device)) == 0, "bgzf_decompress")
    dst = ctypes.create_string_buffer(max(n.value, 1))
    _check(L.gdbamd_bgzf_decompress(data, len(data), dst, n.value, ctypes.byref(n), ctypes.byref(ms), int(device)) == 0, "bgzf_decompress")
    return dst.raw[:n.value], ms.value


TILE_BYTES = 8192


def inflate_tiles(streams, wants, device=0, fill=0xA5):
    """N independent raw DEFLATE streams through the tile inflater of compressed fragment files (k_inflate_tiles, with the launch
    shape and buffer sizes of the fragment reader): stream i must inflate to exactly wants[i] <= 8192 bytes.  The streams are
    concatenated without padding.  Returns (status, out): status[i] = 0 or the TileErr of csrc/core/gdb_tile_inflate.hpp, out =
    N slots of 8192 bytes, each prefilled with `fill` before the launch.  A diagnostic: the engine path does not use it."""
    L = _lib.lib()
    streams = [bytes(s) for s in streams]
    n = len(streams)
    if len(wants) != n:
        raise ValueError("inflate_tiles: one size per stream")
    if n == 0:
        return b"", b""
    offs = (ctypes.c_uint64 * (n + 1))()
    for i, s in enumerate(streams):
        offs[i + 1] = offs[i] + len(s)
    want = (ctypes.c_uint32 * n)(*[int(w) for w in wants])
    out = ctypes.create_string_buffer(n * TILE_BYTES)
    status = ctypes.create_string_buffer(n)
    _check(L.gdbamd_inflate_tiles(b"".join(streams), offs, want, n, int(fill) & 0xFF, out, status, int(device)) == 0, "inflate_tiles")
    return status.raw[:n], out.raw[:n * TILE_BYTES]


BGZF_EOF = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])
