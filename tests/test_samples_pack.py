"""The host side of the batched sample decode (mdsx_decode_samples_*), no GPU: the packed input
buffer of MDSReader.decode_samples, and the `malformed` option of the device batch path."""
import inspect

import numpy as np
import pytest

from streaming_amd import LocalDataset, _native
from streaming_amd.order import DeviceSampleGather
from streaming_amd.plugin import device_iter
from streaming_amd.reader import pack_samples, packed_bytes

SLACK = 64


def _samples():
    rng = np.random.default_rng(7)
    lens = [3, 0, 70, 1, 0, 0, 4096, 17, 64, 0]
    return [rng.integers(1, 256, n, dtype=np.uint8).tobytes() for n in lens]


def test_slack_constant_matches_the_header():
    assert _native.SAMPLE_SLACK == SLACK
    assert (_native.SAMPLE_OK, _native.SAMPLE_CLIPPED, _native.SAMPLE_SHORT_HEAD,
            _native.SAMPLE_SHORT_FIXED) == (0, 1, 2, 3)


def test_pack_offsets_lengths_and_bytes():
    datas = _samples()
    buf, offs, lens = pack_samples(datas)
    m = len(datas)
    assert buf.dtype == np.uint8 and buf.size == packed_bytes([len(d) for d in datas])
    assert offs.dtype == np.uint64 and lens.dtype == np.uint32
    assert lens.tolist() == [len(d) for d in datas]
    # back to back, in order: an empty sample takes no bytes
    assert offs.tolist() == (int(offs[0]) + np.cumsum([0] + [len(d) for d in datas[:-1]])).tolist()
    for d, o, n in zip(datas, offs.tolist(), lens.tolist()):
        assert buf[o:o + n].tobytes() == d
    # the table the kernels read is the head of the same buffer
    assert np.shares_memory(offs, buf) and np.shares_memory(lens, buf)
    assert buf[:8 * m].view(np.uint64).tolist() == offs.tolist()
    assert buf[8 * m:12 * m].view(np.uint32).tolist() == lens.tolist()


def test_pack_slack_at_both_ends():
    datas = _samples()
    buf, offs, lens = pack_samples(datas)
    m = len(datas)
    first, end = int(offs[0]), int(offs[-1]) + int(lens[-1])
    # 64 zero bytes between the table and the first sample, and after the last
    assert first - 12 * m >= SLACK and not buf[first - SLACK:first].any()
    assert buf.size - end == SLACK and not buf[end:].any()


def test_pack_into_a_given_buffer_overwrites_all_of_it():
    datas = _samples()
    want, _, _ = pack_samples(datas)
    out = np.full(want.size, 0xAB, np.uint8)
    got, offs, _ = pack_samples(datas, out=out)
    assert got is out and np.array_equal(out, want) and np.shares_memory(offs, out)
    with pytest.raises(ValueError):
        pack_samples(datas, out=np.empty(want.size + 1, np.uint8))


@pytest.mark.parametrize('datas', [[b''], [b'', b''], [b'x'], []])
def test_pack_degenerate(datas):
    buf, offs, lens = pack_samples(datas)
    assert lens.tolist() == [len(d) for d in datas]
    assert buf.size == packed_bytes(lens.tolist())
    data0 = buf.size - SLACK - sum(len(d) for d in datas)
    assert all(o >= data0 and o + n <= buf.size - SLACK for o, n in zip(offs.tolist(),
                                                                        lens.tolist()))
    assert data0 >= 12 * len(datas) + SLACK


def test_malformed_option():
    assert DeviceSampleGather([]).malformed == 'strict'
    assert DeviceSampleGather([], malformed='reference').malformed == 'reference'
    with pytest.raises(ValueError):
        DeviceSampleGather([], malformed='bogus')
    for fn in (DeviceSampleGather.__init__, LocalDataset.iter_batches, device_iter):
        assert inspect.signature(fn).parameters['malformed'].default == 'strict', fn
