"""Collate throughput: ragged token columns to padded / packed typed batches on the device
(``streaming_amd.collate``: mdsx_ragged_pad, mdsx_ragged_elems + mdsx_ragged_pack).

    python scripts/bench_collate.py --shapes a,a256,b,c --steps 20

Shapes (an ``ndarray:<dtype>`` column, one-dimensional rows of U[lo, hi] tokens):
  a     4096 rows x U[1024, 8192] int32, padded to 8192   (a256: the same with 256 rows)
  b     the same as uint16, widened to int64
  c     1,000,000 rows x U[32, 256] uint16, padded to 256
Per shape, in one process and alternated step by step: the pad (``pad_ragged``, which allocates
its outputs; ``pad_launch`` is the bare ``mdsx_ragged_pad`` call into pre-sized outputs, as the
probe is a bare call), the pack, ``mdsx_copy_probe`` over
the pad's algorithmic bytes (half of R + W copied: the same bytes read plus written), and the
composition available without these kernels -- ``ndarray_meta`` + a torch byte-index gather
``values[data_offset[:, None] + arange(L * item)]``, masked and viewed (for pack: that, then a
boolean select). Outputs are verified against the torch composition before timing. Device
events, median of ``--steps`` steps after ``--warmup``. Prints one JSON line.

Algorithmic bytes: R = value bytes + headers + 8 (rows + 1) offsets; pad W = rows x L x dst item +
9 rows; pack W = sum of lengths x dst item + 8 (rows + 1) + rows.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from streaming_amd import _native  # noqa: E402
from streaming_amd.collate import pack_ragged, pad_ragged  # noqa: E402
from streaming_amd.decoder import RaggedColumn, ndarray_meta  # noqa: E402
from streaming_amd.encodings import VALUE_DTYPES  # noqa: E402

HBM_PEAK_GBS = 8000.0
SHAPES = {
    'a': (4096, 1024, 8192, 'int32', 'int32', 8192),
    'a256': (256, 1024, 8192, 'int32', 'int32', 8192),
    'b': (4096, 1024, 8192, 'uint16', 'int64', 8192),
    'c': (1_000_000, 32, 256, 'uint16', 'uint16', 256),
}
_IDS = {v: k for k, v in VALUE_DTYPES.items()}


def make_column(rows, lo, hi, dtype, seed, dev):
    """An ``ndarray:<dtype>`` column of one-dimensional rows: [1 << 2 | 1][n: u16][values]."""
    rng = np.random.default_rng(seed)
    item = np.dtype(dtype).itemsize
    n = rng.integers(lo, hi + 1, rows)
    offs = np.zeros(rows + 1, np.int64)
    offs[1:] = np.cumsum(3 + n * item)
    buf = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
    buf[offs[:-1]] = (1 << 2) | 1
    buf[offs[:-1] + 1] = n & 0xFF
    buf[offs[:-1] + 2] = n >> 8
    return RaggedColumn(torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev)), n


def torch_pad(col, src, dst, length):
    """What a user can do without per-row syncs: header parse on the device, then a byte-index
    gather, masked and viewed."""
    meta = ndarray_meta(col, _IDS[src])
    item = np.dtype(src).itemsize
    pos = torch.arange(length * item, device=col.values.device)
    idx = (meta.data_offset[:, None] + pos[None, :]).clamp_(max=col.values.numel() - 1)
    live = pos[None, :] < (meta.numel * item)[:, None]
    dense = torch.where(live, col.values[idx], 0).view(getattr(torch, src))
    if dst != src:
        signed = dense.view(torch.int16) if src == 'uint16' else dense
        dense = signed.to(getattr(torch, dst))
        if src == 'uint16':
            dense &= 0xFFFF
    return dense, meta.numel.clamp(max=length)


def torch_pack(col, src, dst, length):
    dense, lengths = torch_pad(col, src, dst, length)
    mask = torch.arange(length, device=dense.device)[None, :] < lengths[:, None]
    if dense.dtype == torch.uint16:  # torch has no boolean select for it: the same bits
        dense = dense.view(torch.int16)
    return dense[mask]


def timed(fn, events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    events.append((e0, e1))


def run_shape(name, steps, warmup, dev):
    rows, lo, hi, src, dst, length = SHAPES[name]
    lib = _native.lib()
    enc = f'ndarray:{src}'
    col, n = make_column(rows, lo, hi, src, 17, dev)
    sitem, ditem = np.dtype(src).itemsize, np.dtype(dst).itemsize
    r_bytes = int(col.values.numel()) + 8 * (rows + 1)
    w_pad = rows * length * ditem + 9 * rows
    w_pack = int(n.sum()) * ditem + 8 * (rows + 1) + rows
    probe_bytes = ((r_bytes + w_pad) // 2 + 15) & ~15
    psrc = torch.empty(probe_bytes, dtype=torch.uint8, device=dev)
    pdst = torch.empty(probe_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out_dtype = None if dst == src else dst

    def pad():
        return pad_ragged(col, enc, out_dtype=out_dtype, length=length, check=False)

    out = torch.empty((rows, length), dtype=getattr(torch, dst), device=dev)
    out_len = torch.empty(rows, dtype=torch.int64, device=dev)
    out_status = torch.empty(rows, dtype=torch.uint8, device=dev)

    def pad_launch():
        _native.raise_for_code(
            lib.mdsx_ragged_pad(col.values.data_ptr(), col.offsets.data_ptr(), rows,
                                _native.ROWS_NDARRAY_STATIC, _IDS[src], _IDS[dst], out.data_ptr(),
                                length, _native.SIDE_RIGHT, _native.SIDE_RIGHT, 0,
                                out_len.data_ptr(), out_status.data_ptr(), None, stream),
            'mdsx_ragged_pad')

    def pack():
        return pack_ragged(col, enc, out_dtype=out_dtype, check=False)

    def probe():
        _native.raise_for_code(lib.mdsx_copy_probe(psrc.data_ptr(), pdst.data_ptr(), probe_bytes,
                                                   stream), 'mdsx_copy_probe')

    # parity with the torch composition (bit patterns)
    got, want = pad(), torch_pad(col, src, dst, length)
    if not torch.equal(got.values.view(torch.uint8), want[0].contiguous().view(torch.uint8)) or \
            not torch.equal(got.lengths, want[1]) or got.status.any().item():
        raise SystemExit(f'PARITY FAILURE: pad, shape {name}')
    packed = pack()
    if not torch.equal(packed.values.view(torch.uint8),
                       torch_pack(col, src, dst, length).contiguous().view(torch.uint8)) or \
            not torch.equal(packed.offsets[1:], torch.cumsum(want[1], 0)):
        raise SystemExit(f'PARITY FAILURE: pack, shape {name}')
    del got, want, packed
    fns = {'pad': pad, 'pad_launch': pad_launch, 'pack': pack, 'copy_probe': probe,
           'torch_pad': lambda: torch_pad(col, src, dst, length),
           'torch_pack': lambda: torch_pack(col, src, dst, length)}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    events = {k: [] for k in fns}
    torch.cuda.synchronize()
    for _ in range(steps):  # alternated: every step runs each of them once
        for k, fn in fns.items():
            timed(fn, events[k])
    torch.cuda.synchronize()
    ms = {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in events.items()}
    pad_gbs = (r_bytes + w_pad) / ms['pad'] / 1e6
    pack_gbs = (r_bytes + w_pack) / ms['pack'] / 1e6
    return {
        'shape': name, 'rows': rows, 'tokens': [lo, hi], 'src': src, 'dst': dst, 'L': length,
        'read_bytes': r_bytes, 'pad_write_bytes': w_pad, 'pack_write_bytes': w_pack,
        'ms': ms,
        'pad_over_copy_probe': ms['pad'] / ms['copy_probe'],
        'pad_launch_over_copy_probe': ms['pad_launch'] / ms['copy_probe'],
        'pad_over_torch': ms['pad'] / ms['torch_pad'],
        'pack_over_torch': ms['pack'] / ms['torch_pack'],
        'pad_GBps': pad_gbs, 'pad_hbm_frac': pad_gbs / HBM_PEAK_GBS,
        'pad_launch_GBps': (r_bytes + w_pad) / ms['pad_launch'] / 1e6,
        'pack_GBps': pack_gbs, 'pack_hbm_frac': pack_gbs / HBM_PEAK_GBS,
        'copy_probe_GBps': 2 * probe_bytes / ms['copy_probe'] / 1e6,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='a,a256,b,c')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if args.steps < 20 or args.warmup < 3:
        raise SystemExit('at least 3 warm-up and 20 timed steps')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    results = [run_shape(s, args.steps, args.warmup, dev) for s in args.shapes.split(',')]
    print(json.dumps({
        'metric': 'collate: ragged ndarray column to padded / packed typed batch, HBM-resident',
        'version': _native.lib().mdsx_version().decode(),
        'device': torch.cuda.get_device_name(0),
        'steps': args.steps, 'warmup': args.warmup,
        'parity': 'ndarray_meta + torch byte-index gather, bit patterns',
        'pack_includes': 'its one host sync (the total sizes the values)',
        'shapes': results,
    }))


if __name__ == '__main__':
    main()
