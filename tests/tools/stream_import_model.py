"""A model of the streaming importer's batch protocol ("Importing buffer streams batch by batch"), written from the
rules and from nothing else: it reads no code of the product.  Tests run a caller's loop against the device and against this model
and compare, batch by batch, W, the cells handed over, the exhausted lists and the pending cells.

The rules.  Every used stream s has last_s, the column of its last delivered record: -inf before its first record, +inf once it has
ended; every record counts, also one that the partition filters out.  A batch takes what was written, W = min last_s, and hands over
every pending cell with column < W (strictly: the stream that defines W may still deliver at W), in (column, row) order, ties in
delivery order.  The unfinished used streams with last_s <= W are reported exhausted, in index order.  A reported stream that gets no
bytes before the next batch has ended.  Cells behind column_end are dropped.  A cell that begins before column_begin and reaches it is
a candidate of its row; the row keeps the candidate of its latest record at or before column_begin (any record there counts, also one
that makes no cell), superseded candidates are dropped in every batch, and the chosen ones go out in the first batch with
W > column_begin.

The caller of the model and of the device is the same loop: every used stream gets its first write before the first batch (a stream
without writes gets none); after a batch every reported stream gets its next write, or none when it has no more.

Input: streams = [None | [write, ...]], None: a stream that no callset uses; write = [record, ...]; record = (column, [(row, end, size)])
with one (row, end, size) per imported sample of the stream: the cell's END column and its size in bytes."""

NEG_INF = float("-inf")
POS_INF = float("inf")


def align16(n):
    return (n + 15) & ~15


class StreamOrderError(Exception):
    def __init__(self, stream, record):
        Exception.__init__(self, "stream %d record %d goes back" % (stream, record))
        self.stream, self.record = stream, record      # record: 1-based over the stream


def run(streams, column_begin=0, column_end=2**63 - 2):
    """-> list of batches: {"W", "cells": [(column, row, size)], "exhausted": [stream], "pending_cells", "pending_bytes"}; the
    pending figures are what the batch held before it handed anything over: the cells it carried over (each rounded up to 16 bytes,
    as they sit in the pool) plus the cells of the new writes (packed)"""
    n = len(streams)
    used = [s is not None for s in streams]
    last = [NEG_INF] * n
    ended = [not u for u in used]
    reported = list(used)
    next_write = [0] * n
    records = [0] * n
    row_best = {}
    pending = []          # [column, row, size, tag] in delivery order; tag None: a cell inside the partition
    seq = 0
    batches = []
    while True:
        held_cells = len(pending)
        held_bytes = sum(align16(p[2]) for p in pending)
        for s in range(n):
            if ended[s] or not reported[s]:
                continue
            write = streams[s][next_write[s]] if next_write[s] < len(streams[s]) else []
            next_write[s] += 1
            if not write:
                ended[s] = True
                last[s] = POS_INF
                continue
            for col, cells in write:
                seq += 1
                records[s] += 1
                if col < last[s]:
                    raise StreamOrderError(s, records[s])
                last[s] = col
                if col <= column_end and col <= column_begin:
                    for row, _, _ in cells:
                        if row not in row_best or row_best[row] < (col, seq):
                            row_best[row] = (col, seq)
                if col > column_end:
                    continue
                for row, end, size in cells:
                    if col < column_begin:
                        if end < column_begin:
                            continue
                        pending.append([col, row, size, (col, seq)])
                    else:
                        pending.append([col, row, size, None])
                    held_cells += 1
                    held_bytes += size
        W = min([last[s] for s in range(n) if not ended[s]] or [POS_INF])
        out, keep = [], []
        for p in pending:
            col, row, size, tag = p
            if tag is not None:
                if row_best.get(row) != tag:
                    continue
                (out if W > column_begin else keep).append(p)
            else:
                (out if col < W else keep).append(p)
        out.sort(key=lambda p: (p[0], p[1]))      # stable: ties stay in delivery order
        pending = keep
        exhausted = [s for s in range(n) if not ended[s] and last[s] <= W]
        reported = [s in exhausted for s in range(n)]
        batches.append({"W": W, "cells": [(p[0], p[1], p[2]) for p in out], "exhausted": exhausted, "pending_cells": held_cells, "pending_bytes": held_bytes,
                        "spanning": sum(1 for p in out if p[3] is not None)})
        if all(ended) and not pending:
            return batches


def pending_bound(streams, column_begin=0, column_end=2**63 - 2):
    """(cells, bytes) that no batch can exceed, whatever the order of the writes.  A stream is refilled only when last_s <= W, so what a
    batch holds of a stream lies in the stream's latest write or at the column the stream had reached before it; on top of that come
    the chosen partition-begin candidates that wait for W to pass column_begin: at most one per row."""
    cells = nbytes = 0
    cand_rows = {}
    for writes in streams:
        if writes is None:
            continue
        best_c = best_b = 0
        before = []          # (column, size) of the cells of earlier writes
        last_col = None
        for write in writes:
            c = b = 0
            for col, recs in write:
                if col > column_end:
                    continue
                for row, end, size in recs:
                    if col < column_begin and end < column_begin:
                        continue
                    c += 1
                    b += align16(size)
                    if col < column_begin:
                        cand_rows[row] = max(cand_rows.get(row, 0), align16(size))
            c += sum(1 for col, _ in before if col == last_col)
            b += sum(sz for col, sz in before if col == last_col)
            best_c, best_b = max(best_c, c), max(best_b, b)
            for col, recs in write:
                if col <= column_end:
                    before += [(col, align16(size)) for row, end, size in recs if not (col < column_begin and end < column_begin)]
                last_col = col
        cells += best_c
        nbytes += best_b
    return cells + len(cand_rows), nbytes + sum(cand_rows.values())
