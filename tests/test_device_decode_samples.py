"""Device batches under malformed='reference' and the batched sample decode behind them
(MDSReader.decode_samples: mdsx_decode_samples_sizes / mdsx_decode_samples_copy).

A batch serves every sample as the reference's loader serves it -- the clipped values recorded in
tests/golden/malformed/outcomes.json from the real reference -- and raises only where the
reference raises. Decoded rows are compared as bytes against the value records: bytes by hex, str
as UTF-8, int as int64 little-endian, scalars and arrays by hex. The kernels are compared, row by
row and over the whole of every output tensor, with the oracle's slices of the same bytes."""
import json
import os
import warnings

import numpy as np
import pytest

from oracle import mds_oracle
from streaming_amd import _native
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

HERE = os.path.join(gu.GOLDEN, 'malformed')
OUTCOMES = json.load(open(os.path.join(HERE, 'outcomes.json')))
CASES = sorted(OUTCOMES)


def _record_bytes(rec):
    if rec['t'] == 'bytes':
        return bytes.fromhex(rec['hex'])
    if rec['t'] == 'str':
        return rec['v'].encode('utf-8')
    if rec['t'] == 'int':
        return int(rec['v']).to_bytes(8, 'little', signed=True)
    assert rec['t'] in ('np', 'ndarray'), rec
    return bytes.fromhex(rec['hex'])


def _host(batch):
    """Every column of a device batch on the host: (values, offsets, flags) or raw rows."""
    import torch
    from streaming_amd.decoder import RaggedColumn
    out = {}
    for name, col in batch.columns.items():
        if isinstance(col, RaggedColumn):
            out[name] = (col.values.cpu().numpy(), col.offsets.cpu().numpy(),
                         col.flags.cpu().numpy() if col.flags is not None else None)
        else:
            out[name] = col.reshape(col.shape[0], -1).view(torch.uint8).cpu().numpy()
    return out


def _row_bytes(host, k):
    row = {}
    for name, col in host.items():
        if isinstance(col, tuple):
            vals, offs, _ = col
            row[name] = vals[offs[k]:offs[k + 1]].tobytes()
        else:
            row[name] = col[k].tobytes()
    return row


def _want_bytes(outcome):
    return {name: _record_bytes(rec) for name, rec in outcome['value'].items()}


def _batch(ds, ids, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')  # numpy's uint32 wrap of end - begin
        batches = list(ds.iter_batches(ids, len(ids), **kw))
    assert len(batches) == 1 and len(batches[0]) == len(ids)
    return batches[0]


def _dataset(case):
    from streaming_amd import LocalDataset
    return LocalDataset(os.path.join(HERE, case), decoded_cache_bytes=1 << 20)


# ---- 1. the fixtures ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_reference_batches_equal_the_recorded_outcomes(case):
    ds = _dataset(case)
    outcomes = OUTCOMES[case]
    for i, want in enumerate(outcomes):  # one sample per batch
        if 'exc' in want:
            with pytest.raises(Exception) as e:
                _batch(ds, [i], malformed='reference')
            assert type(e.value).__name__ == want['exc'], (case, i)
        else:
            got = _row_bytes(_host(_batch(ds, [i], malformed='reference')), 0)
            assert got == _want_bytes(want), (case, i)
    # one batch of every sample whose outcome is a value (twice over: repeated ids)
    good = [i for i, o in enumerate(outcomes) if 'value' in o]
    ids = good + good[::-1]
    host = _host(_batch(ds, ids, malformed='reference'))
    for k, i in enumerate(ids):
        assert _row_bytes(host, k) == _want_bytes(outcomes[i]), (case, i)
    for col in host.values():  # every recorded str is well formed
        assert not isinstance(col, tuple) or col[2] is None or not col[2].any()
    # a batch of all ids: the exception of the first raising sample in BATCH order
    for ids in (list(range(len(outcomes))), list(range(len(outcomes)))[::-1]):
        first = next((outcomes[i]['exc'] for i in ids if 'exc' in outcomes[i]), None)
        if first is None:
            _batch(ds, ids, malformed='reference')
        else:
            with pytest.raises(Exception) as e:
                _batch(ds, ids, malformed='reference')
            assert type(e.value).__name__ == first, (case, ids)


def test_reference_mode_serves_what_strict_mode_refuses():
    """The samples the issue names: strict raises ValueError, the reference returns values."""
    for case, i in (('head_over_last', 2), ('last_past_file', 5), ('file_cut', 5),
                    ('end_before_begin', 2)):
        ds = _dataset(case)
        assert 'value' in OUTCOMES[case][i]
        with pytest.raises(ValueError):
            _batch(ds, [i])
        got = _row_bytes(_host(_batch(ds, [i], malformed='reference')), 0)
        assert got == _want_bytes(OUTCOMES[case][i]), (case, i)


# ---- the kernels against the oracle's slices ----------------------------------------------------
def _reader(names, encodings, sizes):
    from streaming_amd.reader import FileInfo, MDSReader
    return MDSReader('.', None, list(encodings), list(names), list(sizes), None, [],
                     FileInfo('none.mds', 0, {}), 0, None, None)


def _oracle(names, encodings, sizes):
    info = {'raw_data': {'basename': 'none.mds'}, 'column_names': list(names),
            'column_encodings': list(encodings), 'column_sizes': list(sizes), 'samples': 0}
    return mds_oracle.OracleMDSReader(None, None, info, data=b'')


def _value_bytes(v):
    return _record_bytes(gu.value_record(v))


def _expected_status(oracle, data):
    """MDSX_SAMPLE_* of one sample's bytes, from the layout alone (mds/reader.py:103-126)."""
    heads = [s for s in oracle.column_sizes if not s]
    if 4 * len(heads) > len(data):
        return _native.SAMPLE_SHORT_HEAD
    declared = iter(np.frombuffer(data[:4 * len(heads)], np.uint32).tolist())
    sizes = [s or next(declared) for s in oracle.column_sizes]
    parts = oracle.split_sample(data)
    if any(s and len(p) < s for p, s in zip(parts, oracle.column_sizes)):
        return _native.SAMPLE_SHORT_FIXED
    if any(len(p) < s for p, s in zip(parts, sizes)):
        return _native.SAMPLE_CLIPPED
    return _native.SAMPLE_OK


def _check_against_oracle(reader, oracle, datas):
    """decode_samples(datas), one call: the status / str flag says the reference raises exactly
    where the oracle raises, every other row equals the oracle's values, and every output tensor
    as a whole is the oracle's slices of every row, in order, and nothing else."""
    batch, status = reader.decode_samples(datas)
    assert len(batch) == len(datas) and status.shape == (len(datas), )
    host = _host(batch)
    names = oracle.column_names
    str_cols = [n for n, e in zip(names, oracle.column_encodings) if e == 'str']
    parts = []  # the oracle's slices per row (None: a size head cut short)
    for k, data in enumerate(datas):
        try:
            want = oracle.decode_sample(data)
        except Exception:  # noqa: BLE001 -- the outcome is the exception
            want = None
        try:
            parts.append(oracle.split_sample(data))
        except ValueError:
            parts.append(None)
        flagged = any(host[n][2][k] for n in str_cols)
        raises = status[k] >= 2 or (status[k] == _native.SAMPLE_CLIPPED and flagged)
        assert raises == (want is None), (k, len(data), int(status[k]), flagged)
        assert status[k] == _expected_status(oracle, data), (k, len(data))
        assert (status[k] == _native.SAMPLE_SHORT_HEAD) == (parts[k] is None), k
        if want is not None:
            assert _row_bytes(host, k) == {n: _value_bytes(v) for n, v in want.items()}, k
    for c, (name, size) in enumerate(zip(names, oracle.column_sizes)):
        if size:  # a row whose fixed columns are not all whole stays zero
            want_rows = b''.join(
                p[c] if p is not None and all(len(q) == s for q, s in zip(p, oracle.column_sizes)
                                              if s) else bytes(size) for p in parts)
            assert host[name].tobytes() == want_rows, name
        else:  # the values are the clipped slices back to back: no byte more, none disturbed
            vals, offs, flags = host[name]
            lens = [len(p[c]) if p is not None else 0 for p in parts]
            assert offs.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist(), name
            assert vals.tobytes() == b''.join(p[c] for p in parts if p is not None), name
            if flags is not None:
                assert flags.tolist() == [
                    int(p is not None and not mds_oracle.utf8_is_valid(p[c])) for p in parts], name
    return status, host


# ---- 2. every cut of every sample, one launch ---------------------------------------------------
def _junk_after():
    info = json.load(open(os.path.join(HERE, 'junk_after', 'index.json')))['shards'][0]
    o = mds_oracle.OracleMDSReader(os.path.join(HERE, 'junk_after'), None, info)
    from streaming_amd.reader import MDSReader
    r = MDSReader.from_json(os.path.join(HERE, 'junk_after'), None, info)
    return r, o, [o.get_sample_data(i) for i in range(info['samples'])]


def test_cut_sweep_in_one_launch():
    r, o, samples = _junk_after()
    datas = [d[:cut] for d in samples for cut in range(len(d) + 1)]
    assert len(datas) == sum(len(d) + 1 for d in samples) > 300
    status, _ = _check_against_oracle(r, o, datas)
    assert set(status.tolist()) == {0, 1, 2, 3}


def test_single_rows():
    r, o, samples = _junk_after()
    for datas in ([samples[2]], [samples[2][:-1]], [b'']):
        status, _ = _check_against_oracle(r, o, datas)
        assert status.tolist() == [0 if datas[0] == samples[2] else 1 if datas[0] else 2]
    with pytest.raises(ValueError):
        r.decode_samples([])


# ---- 3. copy boundaries -------------------------------------------------------------------------
NAMES3, ENCS3, SIZES3 = ('a', 'n', 's', 'x'), ('bytes', 'int', 'str', 'ndarray:float32:4'), \
    (None, 8, None, 16)


def _sample3(i, alen, with_x=True):
    a = bytes((7 * i + j) % 251 + 1 for j in range(alen))
    s = ('€あ￮' * (alen // 9 + 1))[:alen // 3 + 1].encode('utf-8')  # 3-byte points
    x = (np.arange(4, dtype=np.float32) + i).tobytes() if with_x else b''
    return (np.array([len(a), len(s)], np.uint32).tobytes() + a +
            int(-i - 1).to_bytes(8, 'little', signed=True) + s + x)


@pytest.mark.parametrize('with_x', [True, False])
def test_copy_boundaries(with_x):
    """`a` of lengths around wave_copy's 16-byte chunk and its 64-lane step; each sample whole and
    cut at its last 1-4 bytes, tightly packed sources, adjacent destinations. With the fixed tail
    x the cuts fall inside it (SHORT_FIXED; 16 bytes further they fall inside the 3-byte code
    points of s as well); without it, inside s (CLIPPED: the flag decides)."""
    ncol = 4 if with_x else 3
    schema = NAMES3[:ncol], ENCS3[:ncol], SIZES3[:ncol]
    r, o = _reader(*schema), _oracle(*schema)
    datas = []
    for i, alen in enumerate((0, 1, 15, 16, 17, 1023, 1024, 1041)):
        d = _sample3(i, alen, with_x)
        assert o.decode_sample(d)['a'] == d[8:8 + alen]
        datas += [d[:len(d) - cut] for cut in (0, 1, 2, 3, 4) + ((16, 17, 18, 19, 20) * with_x)]
    status, host = _check_against_oracle(r, o, datas)
    assert set(status.tolist()) == ({0, 3} if with_x else {0, 1, 3})
    flags = host['s'][2]
    assert flags.any() and not flags.all()  # cuts inside a code point, and between two


# ---- 4. the widest plan -------------------------------------------------------------------------
def test_widest_plan():
    names = [f'c{i:02d}' for i in range(_native.MAX_COLUMNS)]
    encs, sizes = ['str'] * len(names), [None] * len(names)
    r, o = _reader(names, encs, sizes), _oracle(names, encs, sizes)
    texts = [('zé€' * (i % 5) + str(i)).encode('utf-8') for i in range(len(names))]
    d = np.array([len(t) for t in texts], np.uint32).tobytes() + b''.join(texts)
    datas = [d, d[:4 * 37 + 2], d[:len(d) - 1], d]
    status, _ = _check_against_oracle(r, o, datas)
    assert status.tolist() == [0, 2, 1, 0]


# ---- 5. strict mode is what it was --------------------------------------------------------------
def test_strict_mode_unchanged():
    """The default, and malformed='strict', on config_c_small: the batches the gather of the
    decoded shards gives (the only path before the option existed), byte for byte; and
    the same ValueError on a sample the reference clips."""
    from streaming_amd import LocalDataset
    from streaming_amd.decoder import gather_sources
    ds = LocalDataset(os.path.join(gu.GOLDEN, 'config_c_small'))
    rng = np.random.default_rng(3)
    ids = rng.permutation(len(ds))[:96]
    g = ds.sample_gather
    assert g.malformed == 'strict'
    shard, local = g.locate(ids)
    for lo in (0, 48):
        want = _host(gather_sources([s.decode_shard() for s in ds.shards], shard[lo:lo + 48],
                                    local[lo:lo + 48]))
        for kw in ({}, {'malformed': 'strict'}, {'malformed': 'reference'}):
            got = _host(list(ds.iter_batches(ids, 48, **kw))[lo // 48])
            assert got.keys() == want.keys()
            for name in want:
                for x, y in zip(got[name] if isinstance(got[name], tuple) else (got[name], ),
                                want[name] if isinstance(want[name], tuple) else (want[name], )):
                    assert (x is None and y is None) or np.array_equal(x, y), (kw, name)
    bad = _dataset('head_over_last')
    for kw in ({}, {'malformed': 'strict'}):
        with pytest.raises(ValueError, match='the batch path refuses'):
            next(iter(bad.iter_batches([2], 1, **kw)))
