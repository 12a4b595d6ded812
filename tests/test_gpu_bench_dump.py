"""bench.py --dump-outputs: the arrays a plain run writes are the reference chain's, whatever the clock did.

The timed steps start from the cold state after exactly --warmup sweeps (the time-based warm-up runs before the
chain is set up), so the fields after the last timed step are those of warmup + steps sweeps of the seed-0 chain:
the oracle gives them bit for bit.  L=64 is written whole (and runs on the temporal-block kernel), L=2048 has more
than bench.DUMP_SITES sites and is written as the fixed sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('L', [64, 2048])
def test_dump_outputs_is_the_oracle_chain(L, tmp_path, oracle_lib):
    import bench
    warm, steps = 2, 3
    out = str(tmp_path / 'dump')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warm),
           '--warmup-s', '0.05', '--L', str(L), '--dump-outputs', out]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([s for s in p.stdout.splitlines() if s.startswith('{')][-1])
    assert line['steps'] == steps and line['warmup'] == warm and line['ms_per_step'] > 0
    assert abs(line['value'] - L * L / (line['ms_per_step'] * 1e-3)) < 1e-6 * line['value']
    assert line['cpu_baseline'] is None and line['roofline']['copy_ceiling_GBps'] is None  # a plain run

    phi, n = np.zeros((L, L)), np.zeros((2, L, L), dtype=np.int64)
    g = np.random.default_rng(0)
    threads = min(16, os.cpu_count() or 1)
    oracle_lib.villain_neighborhood_mt(L, 0.5, 1, phi, n, warm, g, threads)
    ref = oracle_lib.villain_neighborhood_mt(L, 0.5, 1, phi, n, steps, g, threads)
    idx = bench.dump_sample(L * L)
    assert (idx.size == L * L) == (L == 64)
    got = {k: np.load(os.path.join(out, k + '.npy')) for k in ('phi', 'n', 'accepted')}
    assert sorted(os.listdir(out)) == ['accepted.npy', 'n.npy', 'phi.npy']
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert (got['phi'].reshape(-1) == phi.reshape(-1)[idx]).all()
    assert (got['n'].reshape(2, -1) == n.reshape(2, -1)[:, idx]).all()
    assert got['accepted'].tolist() == [float(s.accepted) for s in ref]
