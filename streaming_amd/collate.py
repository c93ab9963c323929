"""Dense and packed typed batches from variable-length columns, on the device.

A variable-length column leaves the decoder as a :class:`~streaming_amd.decoder.RaggedColumn`:
packed bytes plus byte offsets, and for a dynamic ndarray (``ndarray``, ``ndarray:<dtype>``) each
row still starts with its header (``NDArray.decode``, ``encodings.py:270-305``). This is the token
column of an LLM dataset, stored as ``ndarray:int32`` / ``ndarray:uint16`` or as ``bytes`` read
with ``numpy.frombuffer``. :func:`pad_ragged` turns such a column into ``dtype[rows, L]`` plus
lengths, :func:`pack_ragged` into the rows' values back to back (aligned, headers stripped) plus
element offsets, the ``cu_seqlens`` form -- what ``default_collate`` after a per-sample decode,
or a per-row loop over :meth:`NdarrayMeta.row`, would build one row at a time. Both run the
``mdsx_ragged_*`` kernels of libmdsx.so; there is no CPU path.

Every row gets a status byte: 0 good; 1 the reference's decode raises for it (or, for a plain
``bytes`` row, its length is not a whole number of elements); 2 a well-formed row of a fully
dynamic ``ndarray`` column whose dtype is not the one asked for. Rows with a non-zero status
have no elements. Multi-dimensional rows are flattened (C order: their value bytes in memory
order).

Conversions: ``out_dtype`` equal to the source dtype (a bit copy), or integer widening --
``int8 / uint8 / int16 / uint16 -> int32 / int64`` and ``int32 / uint32 -> int64``, sign- or
zero-extended as the source says. Anything else (floats, ``uint64 -> int64``, narrowing) is a
``ValueError``.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Mapping, Optional, Union

import numpy as np
import torch

from streaming_amd import _native
from streaming_amd.encodings import VALUE_DTYPES, parse_encoding

__all__ = ['PaddedColumn', 'PackedColumn', 'Pad', 'Pack', 'pad_ragged', 'pack_ragged',
           'collate_columns', 'padded_length']

_DTYPE_IDS = {name: i for i, name in VALUE_DTYPES.items()}
_SIDES = {'right': _native.SIDE_RIGHT, 'left': _native.SIDE_LEFT}
_WIDEN = {
    'int8': ('int32', 'int64'), 'uint8': ('int32', 'int64'),
    'int16': ('int32', 'int64'), 'uint16': ('int32', 'int64'),
    'int32': ('int64',), 'uint32': ('int64',),
}


def _dtype_name(dtype: Any) -> str:
    if isinstance(dtype, torch.dtype):
        name = str(dtype).split('.')[-1]
    else:
        try:
            name = dtype if isinstance(dtype, str) and dtype in _DTYPE_IDS else np.dtype(dtype).name
        except TypeError:
            name = str(dtype)
    if name not in _DTYPE_IDS:
        raise ValueError(f'collate: {dtype!r} is not a value dtype ({", ".join(_DTYPE_IDS)})')
    return name


def check_conversion(dtype: Any, out_dtype: Any) -> tuple[str, str]:
    """The (source, destination) dtype names of an allowed conversion; ``ValueError`` otherwise."""
    src = _dtype_name(dtype)
    dst = src if out_dtype is None else _dtype_name(out_dtype)
    if dst != src and dst not in _WIDEN.get(src, ()):
        raise ValueError(f'collate: {src} -> {dst} is not allowed (equal dtypes, or integer '
                         f'widening to int32 / int64)')
    return src, dst


def pad_bits(pad_value: Any, dtype: Any) -> int:
    """``pad_value`` as the bit pattern of one ``dtype`` element (converted with numpy);
    ``ValueError`` when the dtype cannot hold it."""
    dt = np.dtype(_dtype_name(dtype))
    if dt.kind in 'iu':
        try:
            exact = int(pad_value)
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f'collate: pad_value {pad_value!r} is not an integer ({dt.name})')
        info = np.iinfo(dt)
        if exact != pad_value or not info.min <= exact <= info.max:
            raise ValueError(f'collate: pad_value {pad_value!r} is not representable as {dt.name}')
        arr = np.array([exact], dt)
    else:
        with np.errstate(over='ignore'):
            arr = np.array([pad_value], np.float64).astype(dt)
        if np.isfinite(float(pad_value)) and not np.isfinite(arr[0]):
            raise ValueError(f'collate: pad_value {pad_value!r} is not representable as {dt.name}')
    return int(arr.view(f'u{dt.itemsize}')[0])


def padded_length(longest: int, multiple_of: int = 1) -> int:
    """The row length chosen when ``length`` is None: the longest row, rounded up to
    ``multiple_of`` (at least one multiple: a batch of empty rows still has a column)."""
    if multiple_of < 1:
        raise ValueError('collate: multiple_of must be positive')
    return max(1, -(-int(longest) // multiple_of)) * multiple_of


def _row_model(encoding: str, dtype: Any) -> tuple[int, str]:
    """(row model, source dtype name) of a ragged column of ``encoding`` read as ``dtype``."""
    info = parse_encoding(encoding)
    if info.name == 'ndarray':
        if info.size is not None:
            raise ValueError(f'collate: {encoding!r} is a fixed-size column (already a tensor)')
        if info.dtype is not None:
            if dtype is not None and _dtype_name(dtype) != info.dtype:
                raise ValueError(f'collate: dtype {dtype!r} given for a column of {encoding!r}')
            return _native.ROWS_NDARRAY_STATIC, info.dtype
        if dtype is None:
            raise ValueError("collate: `dtype` is required for an 'ndarray' column (the rows "
                             'carry their own)')
        return _native.ROWS_NDARRAY_DYN, _dtype_name(dtype)
    if info.name == 'str':
        raise ValueError(f'collate: {encoding!r} columns are not collated (byte and dynamic '
                         f'ndarray columns are)')
    if dtype is None:
        raise ValueError(f'collate: `dtype` is required to read a {encoding!r} column as elements')
    return _native.ROWS_PLAIN, _dtype_name(dtype)


@dataclass
class PaddedColumn:
    """A ragged column as ``values[rows, L]``: row i's ``lengths[i]`` elements at the ``side`` end
    of the row, the rest ``pad_value``. ``status``: uint8[rows], see the module docstring."""
    values: torch.Tensor
    lengths: torch.Tensor
    status: torch.Tensor
    side: str = 'right'

    def __len__(self) -> int:
        return int(self.values.shape[0])

    def mask(self) -> torch.Tensor:
        """bool[rows, L]: True on the elements that are data (``arange(L) < lengths`` for
        ``side='right'``; the last ``lengths`` positions for ``'left'``)."""
        width = self.values.shape[1]
        pos = torch.arange(width, device=self.lengths.device)
        if self.side == 'left':
            return pos[None, :] >= (width - self.lengths)[:, None]
        return pos[None, :] < self.lengths[:, None]

    def tensors(self) -> list[torch.Tensor]:
        return [self.values, self.lengths, self.status]


@dataclass
class PackedColumn:
    """A ragged column as typed ``values[sum of lengths]`` with ``offsets`` int64[rows + 1] in
    ELEMENTS (``cu_seqlens``): row i is ``values[offsets[i]:offsets[i + 1]]``. ``shape``:
    int64[rows, max_ndim] padded with 1 (``ndarray_meta``), when asked for."""
    values: torch.Tensor
    offsets: torch.Tensor
    status: torch.Tensor
    shape: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return int(self.offsets.numel()) - 1

    def tensors(self) -> list[torch.Tensor]:
        return [t for t in (self.values, self.offsets, self.status, self.shape) if t is not None]


@dataclass
class Pad:
    """The keyword arguments of :func:`pad_ragged`, for a ``collate`` spec."""
    dtype: Any = None
    out_dtype: Any = None
    length: Optional[int] = None
    multiple_of: int = 1
    pad_value: Any = 0
    side: str = 'right'
    truncate: str = 'right'
    check: bool = True

    def __post_init__(self) -> None:
        if self.side not in _SIDES or self.truncate not in _SIDES:
            raise ValueError("collate: side and truncate are 'right' or 'left'")
        if self.multiple_of < 1:
            raise ValueError('collate: multiple_of must be positive')
        if self.length is not None and self.length < 1:
            raise ValueError('collate: length must be positive')
        if self.dtype is not None:
            _, dst = check_conversion(self.dtype, self.out_dtype)
            pad_bits(self.pad_value, dst)
        elif self.out_dtype is not None:
            pad_bits(self.pad_value, self.out_dtype)

    def apply(self, col: Any, encoding: str) -> PaddedColumn:
        return pad_ragged(col, encoding, dtype=self.dtype, out_dtype=self.out_dtype,
                          length=self.length, multiple_of=self.multiple_of,
                          pad_value=self.pad_value, side=self.side, truncate=self.truncate,
                          check=self.check)


@dataclass
class Pack:
    """The keyword arguments of :func:`pack_ragged`, for a ``collate`` spec."""
    dtype: Any = None
    out_dtype: Any = None
    check: bool = True
    shapes: bool = False

    def __post_init__(self) -> None:
        if self.dtype is not None:
            check_conversion(self.dtype, self.out_dtype)
        elif self.out_dtype is not None:
            _dtype_name(self.out_dtype)

    def apply(self, col: Any, encoding: str) -> PackedColumn:
        return pack_ragged(col, encoding, dtype=self.dtype, out_dtype=self.out_dtype,
                           check=self.check, shapes=self.shapes)


def _source(col: Any, who: str) -> tuple[torch.device, int, Optional[int]]:
    for t in (col.values, col.offsets):
        if t.device.type != 'cuda':
            raise ValueError(f'{who}: the column is not on the GPU ({t.device}); the collate '
                             f'kernels read decoded device tensors only')
    if col.offsets.dtype != torch.int64 or not col.offsets.is_contiguous() or \
            not col.values.is_contiguous():
        raise ValueError(f'{who}: a RaggedColumn of contiguous values and int64 offsets expected')
    vals = col.values.data_ptr() if col.values.numel() else None
    return col.offsets.device, len(col), vals


def _raise_first_bad(status: torch.Tensor, who: str) -> None:
    bad = torch.nonzero(status)[:1].reshape(-1)
    i = int(bad[0])
    code = int(status[i])
    what = {1: "malformed (the reference's decode raises, or not a whole number of elements)",
            2: 'of another dtype than asked for'}.get(code, 'bad')
    raise ValueError(f'{who}: row {i} has status {code}: {what}')


def pad_ragged(col: Any, encoding: str, *, dtype: Any = None, out_dtype: Any = None,
               length: Optional[int] = None, multiple_of: int = 1, pad_value: Any = 0,
               side: str = 'right', truncate: str = 'right', check: bool = True,
               out: Optional[torch.Tensor] = None) -> PaddedColumn:
    """The rows of ragged column ``col`` (of ``encoding``) as ``out_dtype[rows, L]``
    (``mdsx_ragged_pad``: one launch that parses each row's header itself).

    ``dtype``: taken from ``ndarray:<dtype>``; required for ``ndarray`` (rows of another dtype get
    status 2) and for ``bytes`` (the row bytes read as elements, as ``numpy.frombuffer`` would).
    ``length``: L; None: the longest row, rounded up to ``multiple_of``. ``side``: the end of the
    row the elements sit at; ``truncate``: ``'right'`` keeps the first L elements of a longer row,
    ``'left'`` the last. ``pad_value`` is converted to ``out_dtype`` on the host (``ValueError``
    when it cannot hold it). ``check``: raise ``ValueError`` naming the first row with a non-zero
    status; without it such rows come out all pad with length 0 and their status set.
    ``out``: a contiguous ``out_dtype[rows, L]`` device tensor to write instead of a new one (it
    sets ``length``); every byte of it is written, and none outside it.

    Host syncs: with ``length`` given and ``check=False`` none (one launch, nothing read back);
    with ``length=None`` one, which reads the sizing pass's record (longest row and bad count:
    ``mdsx_ragged_elems``); with ``length`` given and ``check=True`` one, which reads the bad
    count. (Naming the bad row, when there is one, reads once more.)
    """
    if side not in _SIDES or truncate not in _SIDES:
        raise ValueError("pad_ragged: side and truncate are 'right' or 'left'")
    if multiple_of < 1:
        raise ValueError('pad_ragged: multiple_of must be positive')
    if length is not None and length < 1:
        raise ValueError('pad_ragged: length must be positive')
    model, src = _row_model(encoding, dtype)
    src, dst = check_conversion(src, out_dtype)
    bits = pad_bits(pad_value, dst)
    dev, rows, vals = _source(col, 'pad_ragged')
    if out is not None:
        if out.dtype != getattr(torch, dst) or out.device != dev or out.dim() != 2 or \
                out.shape[0] != rows or out.shape[1] < 1 or not out.is_contiguous():
            raise ValueError(f'pad_ragged: `out` must be a contiguous {dst}[{rows}, L] tensor on '
                             f'{dev}')
        if length is not None and length != out.shape[1]:
            raise ValueError('pad_ragged: `length` differs from the width of `out`')
        length = int(out.shape[1])
    lib = _native.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    status = torch.empty(rows, dtype=torch.uint8, device=dev)
    lengths = torch.empty(rows, dtype=torch.int64, device=dev)
    record = None
    if length is None:
        record = torch.zeros(3, dtype=torch.int64, device=dev)
        _native.raise_for_code(
            lib.mdsx_ragged_elems(vals, col.offsets.data_ptr(), rows, model, _DTYPE_IDS[src],
                                  lengths.data_ptr(), status.data_ptr(), record.data_ptr(),
                                  stream), 'mdsx_ragged_elems')
        longest, _, nbad = (int(x) for x in record.cpu())  # sizes the batch (host sync)
        if check and nbad:
            _raise_first_bad(status, 'pad_ragged')
        length = padded_length(longest, multiple_of)
        record = None
    elif check:
        record = torch.zeros(1, dtype=torch.int64, device=dev)
    values = out if out is not None else torch.empty((rows, int(length)),
                                                     dtype=getattr(torch, dst), device=dev)
    _native.raise_for_code(
        lib.mdsx_ragged_pad(vals, col.offsets.data_ptr(), rows, model, _DTYPE_IDS[src],
                            _DTYPE_IDS[dst], values.data_ptr() if rows else None, int(length),
                            _SIDES[side], _SIDES[truncate], bits, lengths.data_ptr(),
                            status.data_ptr(), record.data_ptr() if record is not None else None,
                            stream), 'mdsx_ragged_pad')
    if record is not None and int(record.item()):  # the bad count (host sync)
        _raise_first_bad(status, 'pad_ragged')
    return PaddedColumn(values, lengths, status, side)


def pack_ragged(col: Any, encoding: str, *, dtype: Any = None, out_dtype: Any = None,
                check: bool = True, shapes: bool = False) -> PackedColumn:
    """The rows of ragged column ``col`` (of ``encoding``) back to back as ``out_dtype[sum of
    lengths]`` with int64 element offsets [rows + 1] (``mdsx_ragged_elems`` then
    ``mdsx_ragged_pack``). ``dtype`` / ``out_dtype`` / ``check``: as :func:`pad_ragged`.
    ``shapes``: also the rows' shapes (``ndarray_meta``, int64[rows, max_ndim] padded with 1).

    Host syncs: always one, which reads the total (and the bad count) to size ``values``;
    ``shapes=True`` adds ``ndarray_meta``'s one.
    """
    model, src = _row_model(encoding, dtype)
    src, dst = check_conversion(src, out_dtype)
    dev, rows, vals = _source(col, 'pack_ragged')
    lib = _native.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    status = torch.empty(rows, dtype=torch.uint8, device=dev)
    counts = torch.empty(rows, dtype=torch.int64, device=dev)
    record = torch.zeros(3, dtype=torch.int64, device=dev)
    _native.raise_for_code(
        lib.mdsx_ragged_elems(vals, col.offsets.data_ptr(), rows, model, _DTYPE_IDS[src],
                              counts.data_ptr(), status.data_ptr(), record.data_ptr(), stream),
        'mdsx_ragged_elems')
    _, total, nbad = (int(x) for x in record.cpu())  # sizes the values (host sync)
    if check and nbad:
        _raise_first_bad(status, 'pack_ragged')
    values = torch.empty(total, dtype=getattr(torch, dst), device=dev)
    offsets = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    ws = torch.zeros(int(lib.mdsx_gather_workspace_bytes(rows)), dtype=torch.uint8, device=dev)
    _native.raise_for_code(
        lib.mdsx_ragged_pack(vals, col.offsets.data_ptr(), rows, model, _DTYPE_IDS[src],
                             _DTYPE_IDS[dst], counts.data_ptr(),
                             values.data_ptr() if total else None, total, offsets.data_ptr(),
                             ws.data_ptr(), ws.numel(), stream), 'mdsx_ragged_pack')
    shape = None
    if shapes:
        if model == _native.ROWS_PLAIN:
            raise ValueError('pack_ragged: shapes=True needs an ndarray column')
        from streaming_amd.decoder import ndarray_meta
        shape = ndarray_meta(col, _DTYPE_IDS[src] if model == _native.ROWS_NDARRAY_STATIC
                             else 0).shape
    return PackedColumn(values, offsets, status, shape)


def collate_columns(columns: Mapping[str, Any], spec: Mapping[str, Union[Pad, Pack]],
                    encodings: Mapping[str, str]) -> dict[str, Any]:
    """``columns`` with every column named in ``spec`` replaced by its padded / packed form; the
    others are the same objects (shared, not copied)."""
    out = dict(columns)
    for name, how in spec.items():
        if name not in columns:
            raise KeyError(f'collate: no column {name!r} in the batch ({", ".join(columns)})')
        if not isinstance(how, (Pad, Pack)):
            raise TypeError(f'collate: column {name!r}: a Pad(...) or Pack(...) expected')
        if not hasattr(columns[name], 'offsets'):
            raise ValueError(f'collate: column {name!r} ({encodings[name]!r}) is not a ragged '
                             f'column')
        out[name] = how.apply(columns[name], encodings[name])
    return out
