"""Device-backed MDS shard reader with the reference ``Reader`` / ``MDSReader`` interface.

The reference reader (``streaming/base/format/base/reader.py:31-400``,
``streaming/base/format/mds/reader.py:19-149``) decodes ONE sample per call with Python file
I/O and numpy. :class:`MDSReader` keeps that interface -- ``from_json``, ``validate``,
``get_sample_data``, ``decode_sample``, ``get_item``, fancy ``__getitem__``, ``__len__``,
``size`` and the cache bookkeeping (``evict``, ``set_up_local``, size queries) -- but decodes
the WHOLE shard on the GPU the first time any sample is asked for (:meth:`decode_shard`, through
libmdsx.so), then serves samples from the decoded columns:

* :meth:`decode_shard` -> device tensors (``DecodedBatch``): the hot path.
* :meth:`get_item` -> a dict of host objects with the reference's types (Python ``int`` for
  ``int``, numpy scalars, read-only ndarrays, ``bytes``, ``str``), materialised from one D2H copy
  of the decoded shard. ``str`` rows are produced by ``bytes.decode('utf-8')`` of the
  device-gathered bytes, so invalid UTF-8 raises the same ``UnicodeDecodeError``.
* :meth:`decode_sample` decodes one sample's bytes on the device as a one-sample shard.

A missing shard file raises ``FileNotFoundError`` from ``open`` exactly as the reference does
(the caller's prepare-and-retry loop, ``dataset.py:1274-1291``, depends on it).
"""

from __future__ import annotations

import itertools
import json
import os
import sys
import threading
from copy import deepcopy
from dataclasses import dataclass
from typing import Any, Iterator, Optional, Sequence, Union

import numpy as np
import torch

from streaming_amd import _native
from streaming_amd.array import Array
from streaming_amd.cache import DecodedShardCache, default_cache
from streaming_amd.decoder import (DecodedBatch, Plan, RaggedColumn, _check, _status_error,
                                   output_bytes, stage_shards)
from streaming_amd.encodings import (host_object_decode, is_mds_encoding_safe,
                                     ndarray_dyn_decode, parse_encoding)
from streaming_amd.writer import bytes_to_int

__all__ = ['FileInfo', 'Reader', 'JointReader', 'MDSReader', 'get_plan', 'reader_from_json',
           'pack_samples', 'packed_bytes']

_plan_lock = threading.Lock()
_plans: dict[tuple, Plan] = {}


def get_plan(column_names, column_encodings, column_sizes) -> Plan:
    """Compiled plan for a schema (one per distinct schema per process)."""
    key = (tuple(column_names), tuple(column_encodings),
           tuple(int(s) if s else 0 for s in column_sizes))
    with _plan_lock:
        plan = _plans.get(key)
        if plan is None:
            plan = Plan(column_names, column_encodings, column_sizes)
            _plans[key] = plan
    return plan


def packed_bytes(lengths: Sequence[int]) -> int:
    """Bytes of the buffer :func:`pack_samples` fills for samples of these lengths."""
    m = len(lengths)
    table = (12 * m + 63) // 64 * 64
    return table + 2 * _native.SAMPLE_SLACK + int(sum(int(n) for n in lengths))


def pack_samples(datas: Sequence[bytes], out: Optional[np.ndarray] = None
                 ) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The input of ``mdsx_decode_samples_*`` for the samples ``datas``, in ONE host buffer (one
    H2D): the table -- ``uint64[m]`` offsets, then ``uint32[m]`` lengths, padded to 64 bytes --
    then 64 zero bytes, the samples' bytes back to back (every source alignment occurs; an empty
    sample takes no bytes), and 64 zero bytes: the slack the kernels' aligned loads may read
    before the first sample and after the last.

    Returns ``(buffer, offsets, lengths)``; ``offsets`` (each sample's first byte in ``buffer``)
    and ``lengths`` are views of ``buffer``'s table. ``out``: a uint8 array of
    ``packed_bytes([len(d) for d in datas])`` bytes to fill (a pinned staging buffer)."""
    m = len(datas)
    lens = [len(d) for d in datas]
    if any(n >= 1 << 32 for n in lens):
        raise ValueError('pack_samples: a sample of 4 GiB or more')
    total = packed_bytes(lens)
    if out is None:
        out = np.empty(total, np.uint8)
    if out.dtype != np.uint8 or out.ndim != 1 or out.size != total:
        raise ValueError(f'pack_samples: `out` must be a uint8 array of {total} bytes')
    table = (12 * m + 63) // 64 * 64
    first = table + _native.SAMPLE_SLACK
    offsets = out[:8 * m].view(np.uint64)
    lengths = out[8 * m:12 * m].view(np.uint32)
    lengths[:] = lens
    offsets[:] = first + np.cumsum(lengths, dtype=np.uint64) - lengths
    out[12 * m:first] = 0
    end = first + int(sum(lens))
    if end > first:
        out[first:end] = np.frombuffer(b''.join(datas), np.uint8)
    out[end:] = 0
    return out, offsets, lengths


@dataclass
class FileInfo:
    """File validation info (base/reader.py:17-28)."""
    basename: str
    bytes: int
    hashes: dict[str, str]


class Reader(Array):
    """Random access to the samples of a shard (base/reader.py:31-330)."""

    def __init__(self, dirname: str, split: Optional[str], compression: Optional[str],
                 hashes: list[str], samples: int, size_limit: Optional[Union[int, str]]) -> None:
        if size_limit:
            if isinstance(size_limit, str):
                size_limit = bytes_to_int(size_limit)
            if size_limit < 0:
                raise ValueError(f'`size_limit` must be greater than zero, instead, ' +
                                 f'found as {size_limit}.')
        self.dirname = dirname
        self.split = split or ''
        self.compression = compression
        self.hashes = hashes
        self.samples = samples
        self.size_limit = size_limit
        self.file_pairs: list[tuple[FileInfo, Optional[FileInfo]]] = []

    def validate(self, allow_unsafe_types: bool) -> None:
        pass

    @property
    def size(self) -> int:
        return self.samples

    def __len__(self) -> int:
        return self.samples

    def _path(self, basename: str) -> str:
        return os.path.join(self.dirname, self.split, basename)

    def _evict_raw(self) -> int:
        size = 0
        for raw_info, _ in self.file_pairs:
            filename = self._path(raw_info.basename)
            if os.path.exists(filename):
                os.remove(filename)
                size += raw_info.bytes
        return size

    def _evict_zip(self) -> int:
        size = 0
        for _, zip_info in self.file_pairs:
            if zip_info:
                filename = self._path(zip_info.basename)
                if os.path.exists(filename):
                    os.remove(filename)
                    size += zip_info.bytes
        return size

    def evict(self) -> int:
        return self._evict_raw() + self._evict_zip()

    def set_up_local(self, listing: set[str], safe_keep_zip: bool) -> int:
        """Normalise which of raw/zip are present; return cache bytes (base/reader.py:136-225)."""
        raw_present = sum(1 for raw, _ in self.file_pairs if raw and self._path(raw.basename) in
                          listing)
        zip_present = sum(1 for _, z in self.file_pairs if z and self._path(z.basename) in listing)
        has_raw = raw_present == len(self.file_pairs) and raw_present > 0
        if 0 < raw_present < len(self.file_pairs):
            self._evict_raw()
        has_zip = zip_present == len(self.file_pairs) and zip_present > 0
        if 0 < zip_present < len(self.file_pairs):
            self._evict_zip()
        if self.compression:
            if safe_keep_zip:
                if has_raw and not has_zip:
                    has_raw = False
                    self._evict_raw()
            elif has_raw and has_zip:
                has_zip = False
                self._evict_raw()
        elif has_zip:
            raise ValueError('Shard is invalid: compression was not used, but has a ' +
                             'compressed form.')
        size = 0
        if has_raw:
            size += self.get_raw_size()
        if has_zip:
            size += self.get_zip_size() or 0
        return size

    def get_raw_size(self) -> int:
        return sum(info.bytes for info, _ in self.file_pairs)

    def get_zip_size(self) -> Optional[int]:
        size = 0
        for _, info in self.file_pairs:
            if info is None:
                return None
            size += info.bytes
        return size

    def get_max_size(self) -> int:
        return self.get_raw_size() + (self.get_zip_size() or 0)

    def get_persistent_size(self, keep_zip: bool) -> int:
        if self.compression and keep_zip:
            return self.get_max_size()
        return self.get_raw_size()

    def decode_sample(self, data: bytes) -> dict[str, Any]:
        raise NotImplementedError

    def get_sample_data(self, idx: int) -> bytes:
        raise NotImplementedError

    def get_item(self, idx: int) -> dict[str, Any]:
        data = self.get_sample_data(idx)
        return self.decode_sample(data)

    def __iter__(self) -> Iterator[dict[str, Any]]:
        for i in range(len(self)):
            yield self[i]


class JointReader(Reader):
    """A shard stored as one file (base/reader.py:323-361)."""

    def __init__(self, dirname: str, split: Optional[str], compression: Optional[str],
                 hashes: list[str], raw_data: FileInfo, samples: int,
                 size_limit: Optional[Union[int, str]], zip_data: Optional[FileInfo]) -> None:
        super().__init__(dirname, split, compression, hashes, samples, size_limit)
        self.raw_data = raw_data
        self.zip_data = zip_data
        self.file_pairs.append((raw_data, zip_data))


class _HostShard:
    """Host copy of one decoded shard, for per-sample ``get_item``."""

    def __init__(self, plan: Plan, decoded: DecodedBatch) -> None:
        self.fixed: dict[str, np.ndarray] = {}
        self.ragged: dict[str, tuple[np.ndarray, np.ndarray]] = {}
        self.getters: Optional[list] = None  # MDSReader._getters, built on first use
        self.nbytes = 0
        for col in plan.columns:
            out = decoded.columns[col.name]
            if isinstance(out, RaggedColumn):
                vals, offs = out.values.cpu().numpy(), out.offsets.cpu().numpy()
                self.ragged[col.name] = (vals, offs)
                self.nbytes += vals.nbytes + offs.nbytes
            else:
                rows = out.shape[0]
                raw = out.reshape(rows, -1).view(torch.uint8).cpu().numpy()
                raw.setflags(write=False)
                self.fixed[col.name] = raw
                self.nbytes += raw.nbytes


class _Decoded:
    """A cache entry: one decoded shard, its kernel status and (once asked for) its host copy."""

    def __init__(self, decoded: DecodedBatch, status: _native.Status, nbytes: int) -> None:
        self.decoded = decoded
        self.status = status
        self.nbytes = nbytes
        self.host: Optional[_HostShard] = None


_reader_keys = itertools.count()


class MDSReader(JointReader):
    """Random access to the samples of an MDS shard, decoded on the GPU.

    Same constructor as the reference (mds/reader.py:39-57) plus ``device`` and ``cache``.

    Decoded shards live in ``cache`` (a bounded LRU shared by the readers of a process unless one
    is given, :mod:`streaming_amd.cache`), never beyond it: a shard dropped from the cache, or
    released by :meth:`evict` / :meth:`release`, is decoded again from its file on next use. Like
    the reference, which re-opens the shard file for every sample, :meth:`get_item` raises
    ``FileNotFoundError`` once the file is gone (``StreamingDataset.get_item`` then re-prepares
    the shard and retries, ``dataset.py:1274-1291``), even if a decoded copy is still cached.
    """

    def __init__(self,
                 dirname: str,
                 split: Optional[str],
                 column_encodings: list[str],
                 column_names: list[str],
                 column_sizes: list[Optional[int]],
                 compression: Optional[str],
                 hashes: list[str],
                 raw_data: FileInfo,
                 samples: int,
                 size_limit: Optional[Union[int, str]],
                 zip_data: Optional[FileInfo],
                 device: Union[str, torch.device, None] = None,
                 cache: Optional[DecodedShardCache] = None) -> None:
        super().__init__(dirname, split, compression, hashes, raw_data, samples, size_limit,
                         zip_data)
        self.column_encodings = column_encodings
        self.column_names = column_names
        self.column_sizes = column_sizes
        self.device = device
        self._infos = [parse_encoding(e) for e in column_encodings]
        self._lock = threading.Lock()
        self._cache = cache
        self._key = next(_reader_keys)

    def __getstate__(self) -> dict[str, Any]:
        # pickled into spawned DataLoader workers: no lock, and the decoded shards stay behind
        # (a given cache travels as an empty cache with the same bound, shared by the readers
        # pickled with it)
        state = self.__dict__.copy()
        del state['_lock']
        return state

    def __setstate__(self, state: dict[str, Any]) -> None:
        self.__dict__.update(state)
        self._lock = threading.Lock()
        self._key = next(_reader_keys)

    @classmethod
    def from_json(cls, dirname: str, split: Optional[str], obj: dict[str, Any],
                  device: Union[str, torch.device, None] = None,
                  cache: Optional[DecodedShardCache] = None) -> 'MDSReader':
        """Initialize from an ``index.json`` shard entry (mds/reader.py:59-86)."""
        args = deepcopy(obj)
        if args['version'] != 2:
            raise ValueError(f'Unsupported streaming data version: {args["version"]}. '
                             f'Expected version 2.')
        del args['version']
        if args['format'] != 'mds':
            raise ValueError(f'Unsupported data format: {args["format"]}. Expected to be `mds`.')
        del args['format']
        args['dirname'] = dirname
        args['split'] = split
        for key in ['raw_data', 'zip_data']:
            arg = args[key]
            args[key] = FileInfo(**arg) if arg else None
        return cls(**args, device=device, cache=cache)

    def validate(self, allow_unsafe_types: bool) -> None:
        """Reject unsafe encodings unless allowed (mds/reader.py:88-101)."""
        if not allow_unsafe_types:
            for column_id, encoding in enumerate(self.column_encodings):
                if not is_mds_encoding_safe(encoding):
                    name = self.column_names[column_id]
                    raise ValueError(f'Column {name} contains an unsafe type: {encoding}. To ' +
                                     f'proceed anyway, set ``allow_unsafe_types=True``.')

    @property
    def plan(self) -> Plan:
        return get_plan(self.column_names, self.column_encodings, self.column_sizes)

    def _filename(self) -> str:
        name = self.__dict__.get('_fname')
        if name is None:  # (the directory and basename are fixed at construction)
            name = self._fname = self._path(self.raw_data.basename)
        return name

    def read_shard_bytes(self) -> bytes:
        """The raw shard file (FileNotFoundError if it is not in the local cache)."""
        with open(self._filename(), 'rb', 0) as fp:
            return fp.read()

    @property
    def cache(self) -> DecodedShardCache:
        return self._cache if self._cache is not None else default_cache()

    def _decode_entry(self) -> _Decoded:
        """This shard's cache entry, decoding the file on a miss (FileNotFoundError if absent)."""

        def create() -> tuple[_Decoded, int]:
            _native.check_fork()
            _native.require_gpu()
            data = self.read_shard_bytes()
            plan = self.plan
            batch = stage_shards([data], [self.samples], plan, device=self.device)
            from streaming_amd.decoder import BatchDecoder
            dec = BatchDecoder(plan, batch)
            out = dec.run()
            status = dec.status()  # waits for the decode
            nbytes = output_bytes(plan, out)
            return _Decoded(out, status, nbytes), nbytes, str(batch.device)  # bound per device

        with self._lock:
            return self.cache.get_or_create(self._key, create)

    def decode_shard(self, check: bool = True) -> DecodedBatch:
        """Decode every sample of this shard on the GPU (cached, bounded). Device tensors.

        With ``check`` a malformed shard raises (IndexError for an empty sample, ValueError for a
        range or header error); without it the rows that decoded are returned as they are."""
        entry = self._decode_entry()
        if check and entry.status.code != 0:
            raise _status_error(entry.status, self.plan)
        return entry.decoded

    def release(self) -> None:
        """Drop the decoded shard (device and host copies) from the cache."""
        with self._lock:
            self.cache.discard(self._key)

    def evict(self) -> int:
        """Remove the shard files from the local cache (base/reader.py:128-134) and drop the
        decoded copy, so the next access re-reads the file (or raises FileNotFoundError)."""
        self.release()
        return super().evict()

    def get_sample_data(self, idx: int) -> bytes:
        """Raw bytes of sample ``idx`` (mds/reader.py:128-149): file offsets table + range."""
        offset = (1 + idx) * 4
        with open(self._filename(), 'rb', 0) as fp:
            fp.seek(offset)
            pair = fp.read(8)
            begin, end = np.frombuffer(pair, np.uint32)
            fp.seek(begin)
            data = fp.read(end - begin)
        if not data:
            raise IndexError(
                f'Relative sample index {idx} is not present in the {self.raw_data.basename} file.')
        return data

    def _row_fits(self, idx: int) -> bool:
        """Whether sample ``idx`` passes the whole-shard decode's per-sample checks (decode_kernel,
        swave_decode_kernel): its offsets pair inside the file after the offsets table, its u32
        size heads and every column inside the sample (bytes after the last column allowed)."""
        size = os.stat(self._filename()).st_size
        with open(self._filename(), 'rb', 0) as fp:
            fp.seek((1 + idx) * 4)
            begin, end = (int(x) for x in np.frombuffer(fp.read(8), np.uint32))
            if not (4 + 4 * (self.samples + 1) <= begin <= end <= size):
                return False
            fp.seek(begin)
            data = fp.read(end - begin)
        need, pos = 0, 0
        for size_ in self.column_sizes:
            if size_:
                need += int(size_)
            else:
                if pos + 4 > len(data):
                    return False
                need += 4 + int(np.frombuffer(data[pos:pos + 4], np.uint32)[0])
                pos += 4
        return 0 < need <= len(data)

    def _check_row(self, entry: _Decoded, idx: int) -> None:
        """The batch path (``order.DeviceSampleGather``) on a shard whose decode reported an
        error: raise only if sample ``idx`` is one the decode refused (the reference raises only
        when a bad sample is read, mds/reader.py:145-148) -- the reference's own exception for it
        where the reference raises one (``get_item`` reproduces it), else ValueError: the batch
        path does not hand out the clipped values the reference would. A
        shard-level (header) error raises for every sample."""
        st = entry.status
        if st.code not in (_native.MDSX_E_EMPTY, _native.MDSX_E_BOUNDS):
            raise _status_error(st, self.plan)
        if self._row_fits(idx):
            return
        self.get_item(idx)  # raises what the reference raises for this sample, if anything
        raise ValueError(f'MDS sample {idx} of {self.raw_data.basename} does not fit its layout '
                         '(the reference would hand out clipped values; the batch path refuses).')

    def _materialize(self, host: _HostShard, idx: int) -> dict[str, Any]:
        getters = host.getters
        if getters is None:
            getters = host.getters = self._getters(host)
        return {name: get(idx) for name, get in getters}

    def _getters(self, host: _HostShard) -> list[tuple[str, Any]]:
        """Per column, a function of the sample index returning its reference value (the
        branches of :meth:`_value` resolved once per host shard, the fixed columns viewed as
        their dtype once): the per-sample cost is one call per column."""
        out = []
        for col, enc, info in zip(self.plan.columns, self.column_encodings, self._infos):
            name = info.name if info is not None else None
            if col.is_fixed:
                raw = host.fixed[col.name]
                if info is not None and info.dtype is not None and info.size == raw.shape[1]:
                    if name == 'int':
                        typed = raw.view(info.dtype).reshape(-1)
                        get = (lambda t: lambda i: int(t[i]))(typed)
                    elif info.shape == ():
                        get = raw.view(info.dtype).reshape(-1).__getitem__
                    else:
                        get = raw.view(info.dtype).reshape((raw.shape[0], ) +
                                                           tuple(info.shape)).__getitem__
                else:
                    get = (lambda r, e, f: lambda i: self._value(e, f, r[i], fixed=True))(
                        raw, enc, info)
            else:
                values, offsets = host.ragged[col.name]
                offs = offsets.tolist()  # (python ints: cheaper slicing than numpy scalars)
                # the list's own memory (a pointer + an int object per row) counts against the
                # host bound like the arrays (MDSX_DECODED_HOST_BYTES)
                host.nbytes += len(offs) * (8 + sys.getsizeof(offs[-1] if offs else 0))
                if name == 'bytes':
                    get = (lambda v, o: lambda i: v[o[i]:o[i + 1]].tobytes())(values, offs)
                elif name == 'str':
                    get = (lambda v, o: lambda i: v[o[i]:o[i + 1]].tobytes().decode('utf-8'))(
                        values, offs)
                else:
                    get = (lambda v, o, e, f: lambda i: self._value(
                        e, f, v[o[i]:o[i + 1]].tobytes(), fixed=False))(values, offs, enc, info)
            out.append((col.name, get))
        return out

    @staticmethod
    def _value(encoding: str, info, raw, fixed: bool) -> Any:
        """Reference value type of one decoded column value (encodings.py:62-397)."""
        name = info.name if info is not None else None
        if fixed and info is not None and info.size == len(raw) and info.dtype is not None:
            arr = raw.view(info.dtype)
            if name == 'int':
                return int(arr[0])
            if info.shape == ():
                return arr[0]
            return arr.reshape(info.shape)
        data = raw.tobytes() if isinstance(raw, np.ndarray) else raw
        if name == 'bytes':
            return data
        if name == 'str':
            return data.decode('utf-8')
        if name == 'ndarray':
            return ndarray_dyn_decode(info, data)
        if name == 'int':
            return int(np.frombuffer(data, np.int64)[0])
        if info is not None and info.dtype is not None and info.shape == ():
            return np.frombuffer(data, info.dtype)[0]
        return host_object_decode(encoding, data)

    def get_item(self, idx: int) -> dict[str, Any]:
        """Sample ``idx`` as a dict of host objects, from the device-decoded shard."""
        if not (0 <= idx < self.samples):
            raise IndexError(
                f'Relative sample index {idx} is not present in the {self.raw_data.basename} file.')
        os.stat(self._filename())  # FileNotFoundError once evicted, as the reference's open()
        entry = self.cache.lookup(self._key) or self._decode_entry()
        if entry.status.code != 0:
            # the whole-shard decode reported a sample that does not fit its range or columns (or
            # a header error): every sample of this shard takes the reference's own per-sample
            # path, get_sample_data + decode_sample (base/reader.py:310-320), whose slices clip
            # where the whole-shard decode refuses (mdsx_decode_sample)
            return self.decode_sample(self.get_sample_data(idx))
        host = entry.host
        if host is None:
            with self._lock:
                if entry.host is None:
                    h = _HostShard(self.plan, entry.decoded)
                    h.getters = self._getters(h)  # (adds the offsets lists' bytes)
                    entry.host = h
                    self.cache.set_host_bytes(self._key, h.nbytes)
                host = entry.host
        return self._materialize(host, idx)

    def decode_sample(self, data: bytes) -> dict[str, Any]:
        """Decode one sample's bytes on the device (mds/reader.py:103-126), each column handed the
        slice the reference hands it: a size head larger than the bytes left, or a sample shorter
        than its fixed columns, gives a shorter slice, which the column's decoder returns (bytes),
        decodes (str: UnicodeDecodeError on a cut sequence) or rejects as numpy does (int,
        scalars, static ndarrays); a size head cut short raises ValueError (mdsx_decode_sample)."""
        _native.check_fork()
        _native.require_gpu()
        plan = self.plan
        n = len(data)
        dev = torch.device(self.device or 'cuda')
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        host = torch.zeros(n + 128, dtype=torch.uint8)  # 64 readable bytes before and after
        if n:
            host[64:64 + n] = torch.from_numpy(np.frombuffer(data, np.uint8).copy())
        buf = host.to(dev)
        values = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        ncols = len(plan.columns)
        meta = torch.zeros(2 * ncols + 1, dtype=torch.int64, device=dev)
        rc = _native.lib().mdsx_decode_sample(plan.handle, buf.data_ptr() + 64, n,
                                              values.data_ptr(), meta.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            _check(rc, 'mdsx_decode_sample')
        m = meta.cpu().tolist()  # (syncs the stream)
        vals = values.cpu().numpy()
        vals.setflags(write=False)  # (views of it are read-only, as np.frombuffer's)
        if m[-1]:  # `size, = np.frombuffer(data[idx:idx + 4], np.uint32)` on a short head
            vi = sum(1 for c in plan.columns[:m[-1] - 1] if not c.is_fixed)  # its head's index
            if 4 * vi >= n:
                raise ValueError('not enough values to unpack (expected 1, got 0)')
            raise ValueError('buffer size must be a multiple of element size')
        sample = {}
        for c, (col, enc, info) in enumerate(zip(plan.columns, self.column_encodings,
                                                 self._infos)):
            raw = vals[m[2 * c]:m[2 * c] + m[2 * c + 1]]
            if col.is_fixed and len(raw) == col.row_bytes:
                sample[col.name] = self._value(enc, info, raw, fixed=True)
            else:  # ragged, or a fixed column clipped short: its decoder sees the short slice
                sample[col.name] = self._value(enc, info, raw.tobytes(), fixed=False)
        return sample


    def decode_samples(self, datas: Sequence[bytes]) -> tuple[DecodedBatch, np.ndarray]:
        """Decode many samples' bytes on the device, each sliced as :meth:`decode_sample` slices
        one (mds/reader.py:103-126), into a device batch of ``len(datas)`` rows with the columns
        the whole-shard decode gives (fixed tensors; :class:`RaggedColumn`, with ``flags`` for
        ``str``): ``mdsx_decode_samples_sizes`` + ``mdsx_decode_samples_copy``, one H2D of the
        packed samples (:func:`pack_samples`) and one host sync (the ragged totals, read with the
        status).

        Returns the batch and the host ``int32[m]`` status of each row (``_native.SAMPLE_*``):
        ``OK``; ``CLIPPED`` -- a ragged slice shorter than its head, handed out as the reference
        hands it out (a ``str`` row's flag then says whether ``bytes.decode`` raises on the
        clipped slice); ``SHORT_HEAD`` / ``SHORT_FIXED`` -- the reference's numpy decode raises
        (the row's fixed columns are zero, its ragged slices as clipped)."""
        _native.check_fork()
        _native.require_gpu()
        plan = self.plan
        m = len(datas)
        if m == 0:
            raise ValueError('decode_samples: no samples')
        dev = torch.device(self.device or 'cuda')
        if dev.type != 'cuda':  # host addresses must never reach the kernels
            raise ValueError(f'decode_samples: device {dev} is not a GPU')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        lib = _native.lib()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            total = packed_bytes([len(d) for d in datas])
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            pack_samples(datas, out=host.numpy())
            buf = host.to(dev, non_blocking=True)  # (`host` outlives the copy: the sync below)
            base = buf.data_ptr()
            table = (base, total, base, base + 8 * m, m)
            nvar = plan.num_var
            lens = torch.zeros((max(nvar, 1), m + 1), dtype=torch.int64, device=dev)
            status = torch.zeros((m, 2), dtype=torch.int32, device=dev)
            _check(lib.mdsx_decode_samples_sizes(plan.handle, *table, lens.data_ptr(),
                                                 status.data_ptr(), stream.cuda_stream),
                   'mdsx_decode_samples_sizes')
            offs = torch.cumsum(lens, 1)
            # the one sync: the totals that size the value buffers, and the status
            head = torch.cat([offs[:, -1], status.view(torch.int64).reshape(-1)]).cpu().numpy()
            caps = head[:max(nvar, 1)]
            st = head[max(nvar, 1):].view(np.int32).reshape(m, 2)[:, 0].copy()
            if (st < 0).any():
                raise RuntimeError(f'decode_samples: sample {int(np.argmax(st < 0))} lies outside '
                                   'the packed buffer')
            outs = (_native.ColumnOut * max(len(plan.columns), 1))()
            cols: dict[str, Union[torch.Tensor, RaggedColumn]] = {}
            vi = 0
            for col in plan.columns:
                o = outs[col.index]
                if col.is_fixed:
                    raw = torch.zeros((m, col.row_bytes), dtype=torch.uint8, device=dev)
                    o.data, o.offsets, o.flags, o.capacity = raw.data_ptr(), None, None, 0
                    dtype, shape = col.tensor_view()
                    cols[col.name] = raw.view(dtype).reshape((m, ) + shape)
                else:
                    cap = int(caps[vi])
                    vals = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
                    flags = torch.zeros(m, dtype=torch.uint8, device=dev) \
                        if col.kind == _native.KIND_STR else None
                    o.data = vals.data_ptr() if cap else None
                    o.offsets = offs[vi].data_ptr()
                    o.flags = flags.data_ptr() if flags is not None else None
                    o.capacity = cap
                    cols[col.name] = RaggedColumn(vals[:cap], offs[vi], flags)
                    vi += 1
            _check(lib.mdsx_decode_samples_copy(plan.handle, *table, outs, stream.cuda_stream),
                   'mdsx_decode_samples_copy')
        return DecodedBatch(cols, m, stream=stream), st


def reader_from_json(dirname: str, split: Optional[str], obj: dict[str, Any],
                     device: Union[str, torch.device, None] = None,
                     cache: Optional[DecodedShardCache] = None) -> MDSReader:
    """Reader for an index.json shard entry (format/__init__.py:29-42); MDS only."""
    assert obj['version'] == 2
    if obj['format'] != 'mds':
        raise ValueError(f'streaming_amd decodes MDS shards only, got format {obj["format"]!r}')
    return MDSReader.from_json(dirname, split, obj, device=device, cache=cache)


def load_index(dirname: str, split: Optional[str] = None) -> dict[str, Any]:
    filename = os.path.join(dirname, split or '', 'index.json')
    with open(filename) as f:
        obj = json.load(f)
    if obj['version'] != 2:
        raise ValueError(f'Unsupported streaming data version: {obj["version"]}. ' +
                         f'Expected version 2.')
    return obj
