"""A numpy restatement of ``streaming_amd.collate``'s pad and pack, the yardstick of the GPU tests.

Input: per row, what the reference's decode gives -- a numpy array, or the exception it raised.
Output: what ``pad_ragged`` / ``pack_ragged`` must give for those rows, built one row at a time
the way ``default_collate`` over per-sample decodes would. ``tests/test_collate.py`` pins it to the
rows the reference itself recorded (``tests/golden/dynamic/items.json``)."""

import numpy as np


def row_elems(row, dtype=None):
    """(flattened elements or None, status) of one row: status 1 for a row whose decode raised,
    2 for a row of another dtype than ``dtype`` (when given)."""
    if isinstance(row, BaseException):
        return None, 1
    if dtype is not None and row.dtype != np.dtype(dtype):
        return None, 2
    return np.ascontiguousarray(row).reshape(-1), 0


def padded_length(rows, multiple_of=1, dtype=None):
    longest = max([e.size for e, s in (row_elems(r, dtype) for r in rows) if s == 0], default=0)
    return max(1, -(-longest // multiple_of)) * multiple_of


def pad_ref(rows, length, out_dtype, *, dtype=None, pad_value=0, side='right', truncate='right'):
    """(dense out_dtype[rows, length], lengths int64[rows], status uint8[rows])."""
    out = np.full((len(rows), length), pad_value, np.dtype(out_dtype))
    lengths = np.zeros(len(rows), np.int64)
    status = np.zeros(len(rows), np.uint8)
    for i, row in enumerate(rows):
        e, status[i] = row_elems(row, dtype)
        if e is None or e.size == 0:
            continue
        e = e[:length] if truncate == 'right' else e[max(0, e.size - length):]
        lengths[i] = e.size
        if side == 'right':
            out[i, :e.size] = e.astype(out_dtype)
        else:
            out[i, length - e.size:] = e.astype(out_dtype)
    return out, lengths, status


def pack_ref(rows, out_dtype, *, dtype=None):
    """(values out_dtype[sum of counts], offsets int64[rows + 1], status uint8[rows])."""
    parts, offsets = [], np.zeros(len(rows) + 1, np.int64)
    status = np.zeros(len(rows), np.uint8)
    for i, row in enumerate(rows):
        e, status[i] = row_elems(row, dtype)
        n = 0 if e is None else e.size
        offsets[i + 1] = offsets[i] + n
        if n:
            parts.append(e.astype(out_dtype))
    values = np.concatenate(parts) if parts else np.zeros(0, np.dtype(out_dtype))
    return values, offsets, status


def golden_rows(items, column):
    """The arrays the reference recorded for ``column`` of a golden set's items.json."""
    return [np.frombuffer(bytes.fromhex(it[column]['hex']), it[column]['dtype']).reshape(
        it[column]['shape']) for it in items]
