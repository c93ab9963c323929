"""GPU parity of the collate kernels (``mdsx_ragged_elems`` / ``mdsx_ragged_pad`` /
``mdsx_ragged_pack``; ``streaming_amd.collate``): every comparison is bit-exact against the numpy
restatement ``tests/collate_ref.py`` (pinned to the reference's recorded rows by
``tests/test_collate.py``) over per-row truth from the recorded items or the oracle's
``mds_decode``."""

import numpy as np
import pytest
import torch

from oracle import mds_oracle
from streaming_amd.collate import Pack, PackedColumn, Pad, PaddedColumn, pack_ragged, pad_ragged
from streaming_amd.decoder import Plan, RaggedColumn, decode_batch, stage_shards
from streaming_amd.encodings import VALUE_DTYPES
from streaming_amd.local import LocalDataset
from streaming_amd.order import DeviceSampleGather
from streaming_amd.plugin import device_iter
from tests import collate_ref as cr
from tests import golden_util as gu
from tests.standin_dataset import StandInDataset

pytestmark = pytest.mark.gpu

_IDS = {v: k for k, v in VALUE_DTYPES.items()}
SIDES = [(s, t) for s in ('right', 'left') for t in ('right', 'left')]


@pytest.fixture(scope='module', autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X (torch.cuda.is_available() is False)')


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _same_padded(got: PaddedColumn, want):
    dense, lengths, status = want
    assert tuple(got.values.shape) == dense.shape
    assert str(got.values.dtype).split('.')[-1] == dense.dtype.name
    assert (got.status.cpu().numpy() == status).all()
    assert (got.lengths.cpu().numpy() == lengths).all()
    if _bytes(got.values) != dense.tobytes():
        g = np.frombuffer(_bytes(got.values), np.uint8).reshape(dense.shape[0], -1)
        w = np.frombuffer(dense.tobytes(), np.uint8).reshape(dense.shape[0], -1)
        r, c = np.argwhere(g != w)[0]
        raise AssertionError(f'padded values differ first at row {r}, byte {c}')


def _same_packed(got: PackedColumn, want):
    values, offsets, status = want
    assert (got.status.cpu().numpy() == status).all()
    assert (got.offsets.cpu().numpy() == offsets).all()
    assert str(got.values.dtype).split('.')[-1] == values.dtype.name
    assert got.values.numel() == values.size
    assert _bytes(got.values) == values.tobytes()


def _ragged(rows):
    offs = np.zeros(len(rows) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    vals = np.frombuffer(b''.join(rows), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
    return RaggedColumn(torch.from_numpy(vals.copy()).cuda(), torch.from_numpy(offs).cuda())


def _header(dtype_id, shape, code, static):
    h = b'' if static else bytes([dtype_id])
    h += bytes([(len(shape) << 2) | code])
    sdt = ('<u1', '<u2', '<u4', '<u8')[code]
    return h + np.asarray(shape, dtype=sdt).tobytes()


def _truth(rows, encoding):
    """Per row what the oracle's decode gives: the array, or the exception it raises."""
    out = []
    for row in rows:
        try:
            out.append(mds_oracle.mds_decode(encoding, row))
        except Exception as e:  # the reference's decode raises on this row
            out.append(e)
    return out


# ---- 1. the golden `dynamic` set ---------------------------------------------------------------

@pytest.fixture(scope='module')
def dynamic():
    idx = gu.index('dynamic')
    info0 = idx['shards'][0]
    plan = Plan(info0['column_names'], info0['column_encodings'], info0['column_sizes'])
    data = [gu.shard_bytes('dynamic', s) for s in idx['shards']]
    decoded = decode_batch(plan, stage_shards(data, [s['samples'] for s in idx['shards']], plan))
    items = gu.items('dynamic')
    return decoded, plan, items, {c: cr.golden_rows(items, c) for c in ('d0', 'd1', 'd2')}


@pytest.mark.parametrize('column,dtype', [('d1', 'int16'), ('d2', 'float32')])
@pytest.mark.parametrize('length', [16, None])
def test_golden_pad(dynamic, column, dtype, length):
    decoded, _, _, rows = dynamic
    sizes = np.array([r.size for r in rows[column]])
    if length == 16:
        assert (sizes < 16).any() and (sizes == 16).any() and (sizes > 16).any()
    width = length or cr.padded_length(rows[column], 8)
    for side, truncate in SIDES:
        got = pad_ragged(decoded[column], f'ndarray:{dtype}', length=length, multiple_of=8,
                         pad_value=-3, side=side, truncate=truncate)
        assert not got.status.any().item()
        _same_padded(got, cr.pad_ref(rows[column], width, dtype, pad_value=-3, side=side,
                                     truncate=truncate))
        mask = got.mask().cpu().numpy()
        pos = np.arange(width)[None, :]
        n = np.minimum(sizes, width)[:, None]
        assert (mask == (pos < n if side == 'right' else pos >= width - n)).all()


def test_golden_mixed_dtypes(dynamic):
    decoded, _, items, rows = dynamic
    other = np.array([it['d0']['dtype'] != 'int16' for it in items])
    assert other.sum() == 182
    for length in (16, None):
        got = pad_ragged(decoded['d0'], 'ndarray', dtype='int16', length=length, check=False)
        status = got.status.cpu().numpy()
        assert (status[other] == 2).all() and (status[~other] == 0).all()
        width = length or cr.padded_length(rows['d0'], dtype='int16')
        _same_padded(got, cr.pad_ref(rows['d0'], width, 'int16', dtype='int16'))
    first = int(np.argmax(other))
    for call in (lambda: pad_ragged(decoded['d0'], 'ndarray', dtype='int16', length=16),
                 lambda: pad_ragged(decoded['d0'], 'ndarray', dtype='int16'),
                 lambda: pack_ragged(decoded['d0'], 'ndarray', dtype='int16')):
        with pytest.raises(ValueError, match=f'row {first} has status 2'):
            call()
    _same_packed(pack_ragged(decoded['d0'], 'ndarray', dtype='int16', check=False),
                 cr.pack_ref(rows['d0'], 'int16', dtype='int16'))


@pytest.mark.parametrize('column,dtype', [('d1', 'int16'), ('d2', 'float32')])
def test_golden_pack(dynamic, column, dtype):
    decoded, _, items, rows = dynamic
    got = pack_ragged(decoded[column], f'ndarray:{dtype}', shapes=True)
    assert not got.status.any().item()
    _same_packed(got, cr.pack_ref(rows[column], dtype))
    assert _bytes(got.values) == b''.join(bytes.fromhex(it[column]['hex']) for it in items)
    assert (got.offsets.cpu().numpy() == np.concatenate(
        [[0], np.cumsum([r.size for r in rows[column]])])).all()
    shape = got.shape.cpu().numpy()
    for i, r in enumerate(rows[column]):
        assert tuple(shape[i, :r.ndim]) == r.shape and (shape[i, r.ndim:] == 1).all()


# ---- 2. edge geometry --------------------------------------------------------------------------

VALUE_BYTES = [0, 1, 15, 16, 17, 1008, 1024, 1040, 4080, 4096, 4112]
ROW_BYTES = [2, 14, 16, 18, 100, 1016, 1024, 4096]  # width x item (1024: four rows per wave below it)
EDGE_DTYPES = {1: 'uint8', 2: 'int16', 4: 'float32', 8: 'int64'}
GUARD = 256
SENTINEL = 0xA5


def _edge_rows(item, count, seed):
    """`count` rows of ndarray:<dtype>: value byte counts around one chunk, one 64-lane step, one
    unrolled wave_copy batch and (one row of 40,000 bytes) more than one destination segment;
    shape dtype codes 0..3 and ndim 0..3 in turn, so the value bytes start at every residue."""
    rng = np.random.default_rng(seed)
    dtid = _IDS[EDGE_DTYPES[item]]
    sizes = [VALUE_BYTES[i % len(VALUE_BYTES)] for i in range(count)]
    if count > 2:
        sizes[count // 2] = 40_000
    rows = []
    for i, nbytes in enumerate(sizes):
        numel = nbytes // item
        code, ndim = i % 4, (i // 4) % 4
        if ndim == 0 and numel != 1:
            ndim = 1 + i % 3
        while numel >= 1 << (8 << code):
            code += 1
        shape = [numel] + [1] * (ndim - 1) if ndim else []
        rows.append(_header(dtid, shape[::-1] if i % 2 else shape, code, True) +
                    rng.bytes(numel * item))
    return rows


def _residues(rows, truth):
    start, seen = 0, set()
    for row, t in zip(rows, truth):
        seen.add((start + len(row) - t.nbytes) % 16)
        start += len(row)
    return seen


@pytest.mark.parametrize('count', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('item', [1, 2, 4, 8])
def test_edge_geometry(item, count):
    dtype = EDGE_DTYPES[item]
    enc = f'ndarray:{dtype}'
    rows = _edge_rows(item, count, 100 * item + count)
    truth = _truth(rows, enc)
    assert not any(isinstance(t, Exception) for t in truth)
    if count >= 63:
        assert _residues(rows, truth) == set(range(16))
    col = _ragged(rows)
    sizes = np.array([t.size for t in truth])
    pad_value = {1: 0x3C, 2: -2, 4: 1.5, 8: -(1 << 40) - 5}[item]
    for row_bytes in ROW_BYTES:
        if row_bytes % item:
            continue
        width = row_bytes // item
        if count > 2:  # rows both shorter and longer than the width
            assert (sizes < width).any() and (sizes > width).any()
        for side, truncate in SIDES:
            # dst: a slice of a larger buffer, item-aligned but not chunk-aligned
            buf = torch.full((GUARD + item + count * row_bytes + GUARD,), SENTINEL,
                             dtype=torch.uint8, device='cuda')
            lo = GUARD + item
            out = buf[lo:lo + count * row_bytes].view(getattr(torch, dtype)).view(count, width)
            got = pad_ragged(col, enc, pad_value=pad_value, side=side, truncate=truncate,
                             check=False, out=out)
            assert got.values.data_ptr() == out.data_ptr()
            _same_padded(got, cr.pad_ref(truth, width, dtype, pad_value=pad_value, side=side,
                                         truncate=truncate))
            host = buf.cpu().numpy()
            assert (host[:lo] == SENTINEL).all() and (host[lo + count * row_bytes:] ==
                                                      SENTINEL).all(), (row_bytes, side, truncate)
    # the longest row sets the width: rows of more than one destination segment
    _same_padded(pad_ragged(col, enc, multiple_of=64),
                 cr.pad_ref(truth, cr.padded_length(truth, 64), dtype))
    if count > 2:
        width = int(sizes.max()) - 3
        assert width * item > 32768  # several destination segments per row
        _same_padded(pad_ragged(col, enc, length=width, pad_value=pad_value, side='left',
                                truncate='left'),
                     cr.pad_ref(truth, width, dtype, pad_value=pad_value, side='left',
                                truncate='left'))
        # rows of exactly two segments in a chunk-aligned tensor: the spare segment is empty
        _same_padded(pad_ragged(col, enc, length=16384 // item, pad_value=pad_value),
                     cr.pad_ref(truth, 16384 // item, dtype, pad_value=pad_value))
    _same_packed(pack_ragged(col, enc), cr.pack_ref(truth, dtype))


def test_empty_column():
    col = _ragged([])
    got = pad_ragged(col, 'ndarray:int16', multiple_of=8)
    assert tuple(got.values.shape) == (0, 8) and got.lengths.numel() == 0
    packed = pack_ragged(col, 'ndarray:int16')
    assert packed.values.numel() == 0 and packed.offsets.cpu().tolist() == [0]


# ---- 3. malformed rows -------------------------------------------------------------------------

def _malformed_rows(static):
    rng = np.random.default_rng(11 if static is None else len(static))
    rows = []
    for i in range(3000):
        name = static or VALUE_DTYPES[list(VALUE_DTYPES)[i % len(VALUE_DTYPES)]]
        dtid = _IDS[name]
        item = np.dtype(name).itemsize
        ndim = int(rng.integers(0, 5))
        shape = [int(rng.integers(0, 5)) for _ in range(ndim)]
        code = int(rng.integers(0, 4))
        numel = int(np.prod(shape)) if ndim else 1
        body = rng.bytes(numel * item)
        kind = i % 10
        if kind == 0:      # value bytes one item short / long
            body = body[:-item] if body else body + rng.bytes(item)
        elif kind == 1:    # truncated shape
            hdr = _header(dtid, shape, code, static)
            rows.append(hdr[:max(0, len(hdr) - 1 - int(rng.integers(0, 3)))])
            continue
        elif kind == 2 and static is None:  # unknown dtype id
            rows.append(bytes([int(rng.choice([0, 1, 7, 10, 19, 35, 67, 255]))]) +
                        _header(dtid, shape, code, True) + body)
            continue
        elif kind == 3:    # ragged byte count (not a multiple of the item size)
            body = body + b'\x00' if item > 1 else body
        elif kind == 4:    # a zero dim with a huge other dim (empty array, numpy accepts)
            shape = [0, 2**40 + 3] if code == 3 else [0, 200]
            body = b''
        elif kind == 5:    # product overflows intp
            shape, code, body = [2**40, 2**40], 3, rng.bytes(16)
        rows.append(_header(dtid, shape, code, static) + body)
    rows += [b'', b'\x00', b'\x04', bytes([_IDS['float64'], 0]) + b'\x00' * 8]
    return rows


@pytest.mark.parametrize('static', [None, 'int16', 'uint8'])
def test_malformed_rows(static):
    rows = _malformed_rows(static)
    enc = f'ndarray:{static}' if static else 'ndarray'
    dtype = static or 'int16'
    truth = _truth(rows, enc)
    want_status = np.array([1 if isinstance(t, Exception) else 2 if t.dtype.name != dtype else 0
                            for t in truth], np.uint8)
    nbad = int((want_status != 0).sum())
    assert 0 < nbad < len(rows)
    kw = {'dtype': dtype} if static is None else {}
    for length in (8, None):
        got = pad_ragged(_ragged(rows), enc, length=length, pad_value=77, check=False, **kw)
        assert (got.status.cpu().numpy() == want_status).all()
        width = length or cr.padded_length(truth, dtype=dtype)
        _same_padded(got, cr.pad_ref(truth, width, dtype, dtype=dtype, pad_value=77))
        bad = torch.from_numpy(want_status != 0).cuda()
        assert (got.values[bad] == 77).all().item() and not got.lengths[bad].any().item()
    _same_packed(pack_ragged(_ragged(rows), enc, check=False, **kw),
                 cr.pack_ref(truth, dtype, dtype=dtype))
    first = int(np.argmax(want_status != 0))
    with pytest.raises(ValueError, match=f'row {first} has status {want_status[first]}'):
        pad_ragged(_ragged(rows), enc, length=8, **kw)


# ---- 4. plain bytes as elements ----------------------------------------------------------------

def test_bytes_columns_as_elements(tmp_path):
    from streaming_amd.writer import MDSWriter
    rng = np.random.default_rng(5)
    samples = []
    for i in range(300):
        n = 0 if i % 11 == 0 else int(rng.integers(1, 400))
        a = rng.integers(-2**62, 2**62, n, dtype=np.int64).tobytes()
        b = rng.integers(0, 2**16, n, dtype=np.uint16).tobytes()
        if i % 7 == 3:  # not a whole number of elements
            a, b = a + b'\x01' * (1 + i % 7), b + b'\x02'
        samples.append({'a': a, 'b': b})
    with MDSWriter(columns={'a': 'bytes', 'b': 'bytes'}, out=str(tmp_path), size_limit=1 << 16) as w:
        for s in samples:
            w.write(s)
    batch = LocalDataset(str(tmp_path)).decode_all()
    for name, dtype in (('a', 'int64'), ('b', 'uint16')):
        item = np.dtype(dtype).itemsize
        truth = [ValueError('ragged') if len(s[name]) % item else np.frombuffer(s[name], dtype)
                 for s in samples]
        status = np.array([isinstance(t, Exception) for t in truth], np.uint8)
        assert 0 < status.sum() < len(samples)
        got = pad_ragged(batch[name], 'bytes', dtype=dtype, multiple_of=16, check=False)
        _same_padded(got, cr.pad_ref(truth, cr.padded_length(truth, 16), dtype))
        assert (got.status.cpu().numpy() == status).all()
        empty = np.array([len(s[name]) == 0 for s in samples])
        assert empty.any() and not got.status.cpu().numpy()[empty].any()
        assert not got.lengths.cpu().numpy()[empty].any()
        _same_padded(pad_ragged(batch[name], 'bytes', dtype=dtype, length=33, side='left',
                                truncate='left', check=False),
                     cr.pad_ref(truth, 33, dtype, side='left', truncate='left'))
        _same_packed(pack_ragged(batch[name], 'bytes', dtype=dtype, check=False),
                     cr.pack_ref(truth, dtype))
        with pytest.raises(ValueError, match='row 3 has status 1'):
            pack_ragged(batch[name], 'bytes', dtype=dtype)


# ---- 5. widening -------------------------------------------------------------------------------

WIDEN = [('uint8', 'int64'), ('int16', 'int32'), ('uint16', 'int64'), ('int32', 'int64'),
         ('uint32', 'int64'), ('int8', 'int32'), ('uint8', 'int32'), ('int16', 'int64'),
         ('uint16', 'int32'), ('int8', 'int64')]


@pytest.mark.parametrize('src,dst', WIDEN)
def test_widening(src, dst):
    rng = np.random.default_rng(len(src) * 10 + len(dst))
    info = np.iinfo(src)
    item = np.dtype(src).itemsize
    arrays = []
    for i, nbytes in enumerate(VALUE_BYTES * 6 + [40_000]):
        a = rng.integers(info.min, int(info.max) + 1, nbytes // item, dtype=np.int64).astype(src)
        if a.size:
            a[0], a[-1] = info.min, info.max  # negative / above the signed range of the source
        arrays.append(a)
    rows = [_header(_IDS[src], [a.size] if i % 3 else [a.size, 1], 2, True) + a.tobytes()
            for i, a in enumerate(arrays)]
    enc = f'ndarray:{src}'
    truth = _truth(rows, enc)
    for t, a in zip(truth, arrays):
        assert t.reshape(-1).tobytes() == a.tobytes()
    col = _ragged(rows)
    for width in (7, 100, 700):  # rows of the four-per-wave and of the segment form
        for side, truncate in (('right', 'right'), ('left', 'left')):
            want = cr.pad_ref(truth, width, dst, pad_value=-1, side=side, truncate=truncate)
            _same_padded(pad_ragged(col, enc, out_dtype=dst, length=width, pad_value=-1,
                                    side=side, truncate=truncate), want)
    want = cr.pack_ref(truth, dst)
    assert (want[0] == np.concatenate(arrays).astype(dst)).all()
    _same_packed(pack_ragged(col, enc, out_dtype=dst), want)
    small = [i for i, a in enumerate(arrays) if a.nbytes <= 17]  # short rows only: the grouped pack
    assert len(small) >= 30
    _same_packed(pack_ragged(_ragged([rows[i] for i in small]), enc, out_dtype=dst),
                 cr.pack_ref([truth[i] for i in small], dst))


# ---- 6. batch and loader -----------------------------------------------------------------------

def test_batch_collate_after_gather(dynamic):
    _, plan, _, rows = dynamic
    ds = LocalDataset(gu.GOLDEN + '/dynamic')
    ids = np.random.default_rng(3).permutation(200)[:150]
    batch = DeviceSampleGather(ds.shards).gather(ids)
    out = batch.collate({'d1': Pad(length=16, pad_value=-1), 'd2': Pack()}, ds.shards[0].plan)
    assert out.rows == batch.rows and out.stream is not None
    assert out['e'] is batch['e'] and out['d0'] is batch['d0']
    _same_padded(out['d1'], cr.pad_ref([rows['d1'][i] for i in ids], 16, 'int16', pad_value=-1))
    _same_packed(out['d2'], cr.pack_ref([rows['d2'][i] for i in ids], 'float32'))
    listed = {t.data_ptr() for t in out.tensors()}
    for t in (out['d1'].values, out['d1'].lengths, out['d1'].status, out['d2'].values,
              out['d2'].offsets, out['d2'].status, out['e'].values):
        assert t.data_ptr() in listed
    with pytest.raises(KeyError):
        batch.collate({'nope': Pad()}, plan)


def test_device_iter_collate(dynamic):
    _, _, _, rows = dynamic
    ds = LocalDataset(gu.GOLDEN + '/dynamic')
    ids = np.random.default_rng(4).permutation(200)
    spec = {'d1': Pad(length=24, side='left', truncate='left', out_dtype='int32'),
            'd2': Pad(multiple_of=8)}
    plain = list(device_iter(StandInDataset(ds.shards, lambda e, s: ids), 16))
    again = list(device_iter(StandInDataset(ds.shards, lambda e, s: ids), 16, collate=None))
    made = list(device_iter(StandInDataset(ds.shards, lambda e, s: ids), 16, collate=spec))
    assert len(plain) == len(made) == len(again) == 13
    seen = 0
    for b, a, m in zip(plain, again, made):
        assert (m.sample_ids == b.sample_ids).all() and m.rows == b.rows
        got = ids[seen:seen + b.rows]
        assert (b.sample_ids == got).all()
        seen += b.rows
        _same_padded(m['d1'], cr.pad_ref([rows['d1'][i] for i in got], 24, 'int32', side='left',
                                         truncate='left'))
        r2 = [rows['d2'][i] for i in got]
        _same_padded(m['d2'], cr.pad_ref(r2, cr.padded_length(r2, 8), 'float32'))
        for name in ('d0', 'd1', 'd2', 'e'):  # without `collate`: the batches as before
            assert isinstance(a[name], RaggedColumn)
            assert torch.equal(a[name].values, b[name].values)
            assert torch.equal(a[name].offsets, b[name].offsets)
        assert torch.equal(m['e'].values, b['e'].values)
    assert seen == 200
    got = list(ds.iter_batches(ids, 64, collate={'d1': Pack()}))
    assert [g.rows for g in got] == [64, 64, 64, 8]
    _same_packed(got[1]['d1'], cr.pack_ref([rows['d1'][i] for i in ids[64:128]], 'int16'))


# ---- 7. no host sync ---------------------------------------------------------------------------

def test_pad_with_length_and_no_check_does_not_sync(dynamic):
    decoded, _, _, rows = dynamic
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        got = pad_ragged(decoded['d1'], 'ndarray:int16', length=16, check=False)
        wide = pad_ragged(decoded['d1'], 'ndarray:int16', out_dtype='int64', length=600,
                          check=False)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _same_padded(got, cr.pad_ref(rows['d1'], 16, 'int16'))
    _same_padded(wide, cr.pad_ref(rows['d1'], 600, 'int64'))
    with pytest.raises(RuntimeError):  # the mode does catch a sync: `length=None` reads one back
        try:
            torch.cuda.set_sync_debug_mode('error')
            pad_ragged(decoded['d1'], 'ndarray:int16', check=False)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
