"""bench.py --dump-outputs: what the timed path returned for its last step, as float32 / float64 .npy files within the size
limit (a fixed, seeded sample of the envs above it); and a plain run on the GPU end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(n, points=8, seed=0):
    rng = np.random.default_rng(seed)
    obs = {'position': rng.standard_normal((n, 4, 3)).astype(np.float32),
           'body_mask': (rng.random((n, 4)) > 0.5).astype(np.float32),
           'point_cloud': rng.standard_normal((n, 4, points, 3)).astype(np.float32),
           'num_steps': rng.integers(0, 2 ** 40, n, dtype=np.int64)}
    return obs, rng.standard_normal(n).astype(np.float32), (rng.random(n) > 0.5).astype(np.uint8)


def test_every_output_is_written_exactly_in_float(tmp_path):
    obs, r, d = _outputs(16)
    bench.dump_outputs(str(tmp_path), obs, r, d)
    got = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))}
    assert sorted(got) == sorted(['obs_' + k for k in obs] + ['reward', 'done'])
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
    for k, v in obs.items():
        assert np.array_equal(got['obs_' + k], v), k
    assert got['obs_num_steps'].dtype == np.float64            # integers beyond 2^24 stay exact
    assert np.array_equal(got['reward'], r) and np.array_equal(got['done'], d)


def test_large_outputs_are_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 200000)
    obs, r, d = _outputs(1000)
    written = []
    for run in range(2):
        out = os.path.join(str(tmp_path), str(run))
        bench.dump_outputs(out, obs, r, d, rank=1, world_size=2)
        written.append({f: np.load(os.path.join(out, f)) for f in os.listdir(out)})
        assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 200000 // 2
    a, b = written
    assert sorted(a) == sorted(b) and all(np.array_equal(a[f], b[f]) for f in a)
    idx = a['env_index_rank1.npy'].astype(np.int64) - 1000          # global env ids of rank 1
    assert len(idx) > 0 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a['obs_point_cloud_rank1.npy'], obs['point_cloud'][idx])
    assert np.array_equal(a['reward_rank1.npy'], r[idx])


@pytest.mark.gpu
def test_a_plain_run_prints_its_line_and_dumps_the_last_step(tmp_path):
    out = os.path.join(str(tmp_path), 'dump')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--envs-per-gpu', '64', '--dump-outputs', out],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-3000:]
    got = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in got, k
    assert got['steps'] == 3 and got['value'] > 0 and got['ms_per_step'] > 0
    assert 'cpu_baseline' not in got and 'legs' not in got       # the other legs belong to --full
    files = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    for k in ('obs_position', 'obs_body_mask', 'obs_point_cloud', 'reward', 'done'):
        assert files[k].shape[0] == 64, k
    assert files['obs_point_cloud'].shape[1:] == (4, 256, 3)
    assert all(v.dtype in (np.float32, np.float64) for v in files.values())
    assert np.isfinite(files['obs_position']).all() and set(np.unique(files['done'])) <= {0.0, 1.0}
