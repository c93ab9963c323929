"""Device batches over a shard with clipped samples: the time
of one 256-row ``DeviceSampleGather.gather`` under ``malformed='reference'`` with 1, 16 and 256
clipped rows in the batch, against the same batch in strict mode over the unedited shard and
against the same 256 samples read one by one through ``MDSReader.get_item`` (on a malformed shard:
``get_sample_data`` + ``decode_sample``, one launch and one sync per sample).

A synthetic {b: bytes, n: int, s: str} shard is written to a temp directory; an edited copy per
count raises the ``s`` size head of that many of the batch's samples 5 bytes past the sample (the
reference hands out the clipped text: tests/golden/malformed ``head_over_last``). Every shard is
decoded (cached) before the clock starts; each figure is the median over ``--reps`` gathers, each
ended by a device synchronise. The same-run copy ceiling (bench.py ``copy_ceiling``) is reported
beside them. Prints one JSON object (and writes it to ``--out``).
"""

import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from streaming_amd import LocalDataset, MDSWriter, _native  # noqa: E402
from streaming_amd.order import DeviceSampleGather  # noqa: E402


def write_shard(out, samples, seed):
    rng = np.random.default_rng(seed)
    with MDSWriter(out=out, columns={'b': 'bytes', 'n': 'int', 's': 'str'},
                   size_limit=1 << 30) as w:
        for i in range(samples):
            b = rng.integers(0, 256, int(rng.integers(1024, 3073)), dtype=np.uint8).tobytes()
            s = rng.integers(97, 123, int(rng.integers(256, 1025)), dtype=np.uint8).tobytes()
            w.write({'b': b, 'n': i, 's': s.decode()})


def clip_rows(src_dir, dst_dir, rows):
    """A copy of the one-shard dataset whose samples ``rows`` have their `s` head 5 bytes past
    the sample."""
    shutil.copytree(src_dir, dst_dir)
    info = json.load(open(os.path.join(dst_dir, 'index.json')))['shards']
    assert len(info) == 1
    path = os.path.join(dst_dir, info[0]['raw_data']['basename'])
    raw = bytearray(open(path, 'rb').read())
    n = int(np.frombuffer(raw[:4], np.uint32)[0])
    offs = np.frombuffer(raw[4:4 + 4 * (n + 1)], np.uint32).astype(np.int64)
    for i in rows:
        at = int(offs[i]) + 4  # heads: b, s
        head = int(np.frombuffer(raw[at:at + 4], np.uint32)[0])
        raw[at:at + 4] = np.uint32(head + 5).tobytes()
    with open(path, 'wb') as f:
        f.write(raw)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'reps': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=4096)
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--clipped', type=int, nargs='+', default=[1, 16, 256])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--item-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    import bench
    tmp = tempfile.mkdtemp(prefix='mdsx_malformed_')
    res = {'library': _native.lib().mdsx_version().decode(), 'rows': args.rows,
           'shard_samples': args.samples, 'device': torch.cuda.get_device_name(0)}
    try:
        clean = os.path.join(tmp, 'clean')
        write_shard(clean, args.samples, seed=11)
        ids = np.random.default_rng(5).permutation(args.samples)[:args.rows]
        ds = LocalDataset(clean, decoded_cache_bytes=1 << 34)
        res['shard_bytes'] = os.path.getsize(ds.shards[0]._filename())
        strict = DeviceSampleGather(ds.shards)
        want = strict.gather(ids)
        res['strict_clean'] = timed(lambda: strict.gather(ids), args.reps)
        ref = DeviceSampleGather(ds.shards, malformed='reference')
        res['reference_clean'] = timed(lambda: ref.gather(ids), args.reps)
        res['get_item_clean'] = timed(lambda: [ds.shards[0].get_item(int(i)) for i in ids],
                                      args.item_reps)
        for k in args.clipped:
            d = os.path.join(tmp, f'clip{k}')
            clip_rows(clean, d, [int(i) for i in ids[:k]])
            dk = LocalDataset(d, decoded_cache_bytes=1 << 34)
            g = DeviceSampleGather(dk.shards, malformed='reference')
            got = g.gather(ids)
            # the clipped text is all that is left of the sample: the whole text, as written
            same = all(torch.equal(got[c].values, want[c].values) and
                       torch.equal(got[c].offsets, want[c].offsets) for c in ('b', 's')) and \
                torch.equal(got['n'], want['n'])
            entry = {'equals_clean_batch': bool(same),
                     'reference_batch': timed(lambda: g.gather(ids), args.reps),
                     'get_item_loop': timed(
                         lambda: [dk.shards[0].get_item(int(i)) for i in ids], args.item_reps)}
            try:
                DeviceSampleGather(dk.shards).gather(ids)
                entry['strict_raises'] = None
            except ValueError as e:
                entry['strict_raises'] = type(e).__name__
            res[f'clipped_{k}'] = entry
        buf = types.SimpleNamespace(buffer=torch.empty(256 << 20, dtype=torch.uint8,
                                                       device='cuda').random_(0, 256))
        res['copy_probe'] = bench.copy_ceiling(buf)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
