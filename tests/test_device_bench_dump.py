"""A plain benchmark run on the GPU at a small size (``--shards 2``): the result line's fields,
``--steps`` as the number of timed steps, and ``--dump-outputs`` against a decode of the same
seeded workload made here."""

import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHARDS = 2


def test_plain_run_line_and_dumped_outputs(tmp_path, capsys):
    import bench
    from streaming_amd.decoder import BatchDecoder
    out = tmp_path / 'dump'
    args = ['--gpus', '1', '--steps', '4', '--warmup', '2', '--shards', str(SHARDS),
            '--dump-outputs', str(out)]
    assert bench.main(args) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line['metric'] == bench.METRIC and line['unit'] == 'samples/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'u8'
    assert line['steps'] == 4 and line['warmup'] == 2 and line['full'] is False
    assert sum(b['steps'] for b in line['blocks']) == 4
    assert line['ms_per_step'] > 0
    rows = line['config']['samples_per_gpu']
    assert line['value'] == pytest.approx(rows / (line['ms_per_step'] / 1e3), rel=1e-9)
    assert line['cpu_baseline'] is None and 'config_c' not in line
    assert line['roofline']['copy_ceiling_same_run'] is None

    synth, _ = bench.build_workload('B', list(range(SHARDS)))
    dec = BatchDecoder(synth.plan, synth.batch)
    want = dec.run()
    dec.check()
    assert want.rows == rows
    files = sorted(p.name for p in out.iterdir())
    assert files == ['B_id.npy', 'B_x.npy', 'B_x.rows.npy']
    got = {p.name[2:-4]: np.load(p) for p in out.iterdir()}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 * 10**6
    assert np.array_equal(got['id'], want['id'].cpu().numpy().astype(np.float64))
    picked = got['x.rows'].astype(np.int64)
    assert len(picked) > 1000 and picked.max() < rows
    bits = want['x'].view(torch.int32)[torch.from_numpy(picked).cuda()].cpu().numpy()
    assert np.array_equal(got['x'].astype(np.int32), bits.reshape(len(picked), -1))
