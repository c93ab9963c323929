"""Collate without a GPU: the argument checks of ``mdsx_ragged_elems`` / ``mdsx_ragged_pad`` /
``mdsx_ragged_pack`` (all made before any HIP call), the ``Pad`` / ``Pack`` validation, and the
numpy restatement (``tests/collate_ref.py``) pinned to the rows the reference recorded."""

import ctypes

import numpy as np
import pytest

from streaming_amd import _native
from streaming_amd.collate import (Pack, Pad, check_conversion, pad_bits, padded_length,
                                   pad_ragged)
from streaming_amd.encodings import VALUE_DTYPES
from tests import collate_ref as cr
from tests import golden_util as gu

_IDS = {v: k for k, v in VALUE_DTYPES.items()}
OK, E_ARG, E_ENC = _native.MDSX_OK, _native.MDSX_E_ARG, _native.MDSX_E_ENCODING

# host memory the checks never read: every rejection below happens before a launch, and
# rows == 0 launches nothing
_buf = ctypes.create_string_buffer(4096)
P = ctypes.addressof(_buf)


def _elems(values=P, offsets=P, rows=4, model=1, src=_IDS['int16'], count=P, status=P, record=P):
    return _native.lib().mdsx_ragged_elems(values, offsets, rows, model, src, count, status,
                                           record, None)


def _pad(values=P, offsets=P, rows=4, model=1, src=_IDS['int16'], dst=_IDS['int16'], out=P,
         width=8, side=0, truncate=0, bits=0, out_len=P, status=P, bad=None):
    return _native.lib().mdsx_ragged_pad(values, offsets, rows, model, src, dst, out, width, side,
                                         truncate, bits, out_len, status, bad, None)


def _pack(values=P, offsets=P, rows=4, model=1, src=_IDS['int16'], dst=_IDS['int16'], count=P,
          out=P, capacity=16, out_offsets=P, ws=P, ws_bytes=4096):
    return _native.lib().mdsx_ragged_pack(values, offsets, rows, model, src, dst, count, out,
                                          capacity, out_offsets, ws, ws_bytes, None)


ALLOWED = [(s, d) for s in ('int8', 'uint8', 'int16', 'uint16') for d in ('int32', 'int64')] + \
          [('int32', 'int64'), ('uint32', 'int64')] + [(n, n) for n in _IDS]
REFUSED = [('float32', 'int32'), ('int32', 'float32'), ('float16', 'float32'),
           ('uint64', 'int64'), ('int64', 'int32'), ('int32', 'int16'), ('int16', 'uint16'),
           ('uint8', 'int16'), ('uint8', 'uint32'), ('int32', 'uint64'), ('int64', 'uint64')]


def test_rows_zero_is_ok_and_launches_nothing():
    assert _elems(rows=0, values=None, count=None, status=None) == OK
    assert _pad(rows=0, values=None, out=None, out_len=None, status=None) == OK
    assert _pack(rows=0, values=None, count=None, out=None, capacity=0, ws=None,
                 ws_bytes=0) == OK


@pytest.mark.parametrize('null', ['values', 'offsets', 'count', 'status', 'record'])
def test_elems_null_pointers(null):
    assert _elems(**{null: None}) == E_ARG


@pytest.mark.parametrize('null', ['values', 'offsets', 'out', 'out_len', 'status'])
def test_pad_null_pointers(null):
    assert _pad(**{null: None}) == E_ARG


@pytest.mark.parametrize('null', ['values', 'offsets', 'count', 'out', 'out_offsets', 'ws'])
def test_pack_null_pointers(null):
    assert _pack(**{null: None}) == E_ARG


def test_pack_small_workspace():
    need = int(_native.lib().mdsx_gather_workspace_bytes(4))
    assert _pack(ws_bytes=need - 1) == E_ARG


@pytest.mark.parametrize('bad', [0, 1, 7, 10, 19, 35, 67, 255, -8])
def test_unknown_dtype_ids(bad):
    assert _elems(src=bad) == E_ENC
    assert _pad(src=bad) == E_ENC and _pad(dst=bad) == E_ENC
    assert _pack(src=bad) == E_ENC and _pack(dst=bad) == E_ENC


@pytest.mark.parametrize('model', [-1, 3])
def test_unknown_row_model(model):
    assert _elems(model=model) == E_ARG and _pad(model=model) == E_ARG
    assert _pack(model=model) == E_ARG


@pytest.mark.parametrize('src,dst', REFUSED)
def test_refused_conversions(src, dst):
    assert _pad(src=_IDS[src], dst=_IDS[dst]) == E_ARG
    assert _pack(src=_IDS[src], dst=_IDS[dst]) == E_ARG
    with pytest.raises(ValueError):
        check_conversion(src, dst)
    with pytest.raises(ValueError):
        Pad(dtype=src, out_dtype=dst)
    with pytest.raises(ValueError):
        Pack(dtype=src, out_dtype=dst)


@pytest.mark.parametrize('src,dst', ALLOWED)
def test_allowed_conversions(src, dst):
    # accepted by the host checks: rows == 0 passes them all and launches nothing
    assert _pad(src=_IDS[src], dst=_IDS[dst], rows=0) == OK
    assert _pack(src=_IDS[src], dst=_IDS[dst], rows=0) == OK
    assert check_conversion(src, dst) == (src, dst)
    assert Pad(dtype=src, out_dtype=dst).out_dtype == dst
    assert Pack(dtype=src, out_dtype=dst).out_dtype == dst
    assert check_conversion(src, None) == (src, src)


def test_pad_width_limits():
    assert _pad(width=0) == E_ARG
    assert _pad(width=0, rows=0) == E_ARG
    assert _pad(width=1 << 31) == E_ARG                  # x 2 bytes = 2^32
    assert _pad(width=1 << 29, dst=_IDS['int64'], src=_IDS['int64']) == E_ARG
    assert _pad(width=1 << 32, src=_IDS['uint8'], dst=_IDS['uint8']) == E_ARG
    assert _pad(width=(1 << 31) - 1, rows=0) == OK      # 2^32 - 2 bytes
    assert _pad(side=2) == E_ARG and _pad(truncate=-1) == E_ARG
    assert _pad(out=P + 1) == E_ARG                      # dst not aligned to its item


def test_pad_value_bits():
    assert pad_bits(0, 'int32') == 0
    assert pad_bits(-1, 'int16') == 0xFFFF
    assert pad_bits(-100, 'int64') == (1 << 64) - 100
    assert pad_bits(65535, 'uint16') == 65535
    assert pad_bits(1.0, 'float32') == 0x3F800000
    assert pad_bits(float('inf'), 'float16') == 0x7C00
    assert pad_bits(np.int64(7), 'uint8') == 7
    for value, dtype in [(-1, 'uint16'), (70000, 'int16'), (256, 'uint8'), (-129, 'int8'),
                         (1 << 63, 'int64'), (1.5, 'int32'), (1e39, 'float32'),
                         (70000.0, 'float16'), ('x', 'int32')]:
        with pytest.raises(ValueError):
            pad_bits(value, dtype)
    with pytest.raises(ValueError):
        Pad(dtype='uint16', pad_value=-1)
    with pytest.raises(ValueError):
        Pad(dtype='uint8', out_dtype='int32', pad_value=1 << 31)
    assert Pad(dtype='uint8', out_dtype='int32', pad_value=-100).pad_value == -100


def test_pad_and_pack_validation():
    for kw in ({'side': 'middle'}, {'truncate': 'both'}, {'multiple_of': 0}, {'length': 0},
               {'dtype': 'complex64'}, {'out_dtype': 'bool'}):
        with pytest.raises(ValueError):
            Pad(**kw)
    with pytest.raises(ValueError):
        Pack(dtype='str')
    assert [padded_length(n, 8) for n in (0, 1, 8, 9, 300)] == [8, 8, 8, 16, 304]
    assert [padded_length(n) for n in (0, 1, 300)] == [1, 1, 300]
    assert padded_length(300, 128) == 384
    with pytest.raises(ValueError):
        padded_length(3, 0)


class _Host:
    """A ragged column that is not on the GPU."""

    def __init__(self):
        import torch
        self.values = torch.zeros(4, dtype=torch.uint8)
        self.offsets = torch.tensor([0, 4], dtype=torch.int64)

    def __len__(self):
        return 1


def test_encoding_rules_and_host_columns():
    col = _Host()
    for enc, kw in [('ndarray', {}), ('bytes', {}), ('str', {'dtype': 'uint8'}),
                    ('ndarray:int16', {'dtype': 'int32'}), ('ndarray:int16:3,4', {}),
                    ('ndarray:int16', {'out_dtype': 'float32'})]:
        with pytest.raises(ValueError):
            pad_ragged(col, enc, length=4, **kw)
    with pytest.raises(ValueError, match='not on the GPU'):  # refused before any device call
        pad_ragged(col, 'ndarray:int16', length=4)


# ---- the restatement against the reference's recorded rows -------------------------------------

def test_restatement_matches_the_recorded_rows():
    items = gu.items('dynamic')
    rows = cr.golden_rows(items, 'd1')
    assert len(rows) == 200 and all(r.dtype == np.int16 for r in rows)
    sizes = np.array([r.size for r in rows])
    assert ((sizes < 16).sum(), (sizes == 16).sum(), (sizes > 16).sum()) == (143, 3, 54)
    for side in ('right', 'left'):
        for truncate in ('right', 'left'):
            dense, lengths, status = cr.pad_ref(rows, 16, 'int16', pad_value=-7, side=side,
                                                truncate=truncate)
            assert dense.shape == (200, 16) and not status.any()
            pad = np.int16(-7).tobytes()
            for i, it in enumerate(items):
                raw = bytes.fromhex(it['d1']['hex'])
                kept = raw[:32] if truncate == 'right' else raw[max(0, len(raw) - 32):]
                fill = pad * (16 - len(kept) // 2)
                want = kept + fill if side == 'right' else fill + kept
                assert dense[i].tobytes() == want, (side, truncate, i)
                assert lengths[i] == len(kept) // 2
    # d0: eleven dtypes mixed; asking for int16 gives status 2 on the others
    d0 = cr.golden_rows(items, 'd0')
    _, lengths, status = cr.pad_ref(d0, 8, 'int16', dtype='int16')
    other = np.array([it['d0']['dtype'] != 'int16' for it in items])
    assert other.sum() == 182 and (status == np.where(other, 2, 0)).all()
    assert not lengths[other].any()
    # pack: the recorded bytes back to back
    values, offsets, status = cr.pack_ref(rows, 'int16')
    assert values.tobytes() == b''.join(bytes.fromhex(it['d1']['hex']) for it in items)
    assert (np.diff(offsets) == sizes).all() and offsets[0] == 0 and not status.any()


def test_restatement_statuses_and_widening():
    rows = [np.array([[1, -2], [3, -4]], np.int16), ValueError('bad'), np.zeros(0, np.int16),
            np.array([5], np.int16), np.array([1.5], np.float32)]
    dense, lengths, status = cr.pad_ref(rows, 3, 'int64', dtype='int16', pad_value=9,
                                        side='left', truncate='left')
    assert dense.tolist() == [[-2, 3, -4], [9, 9, 9], [9, 9, 9], [9, 9, 5], [9, 9, 9]]
    assert lengths.tolist() == [3, 0, 0, 1, 0] and status.tolist() == [0, 1, 0, 0, 2]
    values, offsets, status = cr.pack_ref(rows, 'int32', dtype='int16')
    assert values.tolist() == [1, -2, 3, -4, 5] and values.dtype == np.int32
    assert offsets.tolist() == [0, 4, 4, 4, 5, 5] and status.tolist() == [0, 1, 0, 0, 2]
    assert cr.padded_length(rows, 4, dtype='int16') == 4
