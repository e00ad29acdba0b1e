"""GPU: the plain bench.py run — the headline alone, --steps timed steps, `ms_per_step` — and --dump-outputs, whose
files are the same on every run with the same arguments (seeded inputs), so that two builds compare output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(*argv):
  env = dict(os.environ)
  env.pop('WORLD_SIZE', None)
  p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), env=env, stdout=subprocess.PIPE,
                     stderr=subprocess.PIPE, text=True, timeout=600)
  assert p.returncode == 0, p.stderr[-3000:]
  lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, p.stdout
  return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_plain_line_is_the_headline_alone_and_dumps_are_reproducible(tmp_path):
  args = ['--lanes', '8192', '--steps', '12', '--warmup', '4']
  lines = [_run(*args, '--dump-outputs', str(tmp_path / d)) for d in ('a', 'b')]
  for line in lines:
    assert line['metric'] == 'env-steps/sec' and line['unit'] == 'env-steps/s' and line['higher_is_better'] is True
    assert line['steps'] == 12 and line['ms_per_step'] > 0 and line['dtype'] == 'int32'
    assert line['config']['workload'].startswith('deep_sea/10') and line['roofline']['alg_bytes'] == 3621 * 8192
    assert not {'also', 'cpu_baseline', 'host'} & set(line) and 'box_fill_GBps' not in line['roofline']
  assert lines[0]['episodes_finished'] == lines[1]['episodes_finished'] > 0
  shapes = {'step_type': (8192,), 'reward': (8192,), 'discount': (8192,), 'observation': (8192, 30, 30)}
  assert sorted(os.listdir(tmp_path / 'a')) == sorted(f'{k}.npy' for k in shapes)
  for k, shape in shapes.items():
    a, b = np.load(tmp_path / 'a' / f'{k}.npy'), np.load(tmp_path / 'b' / f'{k}.npy')
    assert a.dtype == np.float32 and a.shape == shape and np.array_equal(a, b), k
  st, obs = np.load(tmp_path / 'a' / 'step_type.npy'), np.load(tmp_path / 'a' / 'observation.npy')
  assert set(np.unique(st)) <= {0.0, 1.0, 2.0} and set(np.unique(obs)) <= {0.0, 1.0}
  # the sweep's plain line: its headline schedule alone, the lanes of every segment in the dump
  sweep = [_run('--workload', 'sweep', '--lanes', '8192', '--steps', '10', '--warmup', '2', '--dump-outputs', str(tmp_path / d))
           for d in ('s1', 's2')]
  assert sweep[0]['steps'] == 10 and sweep[0]['ms_per_step'] > 0 and 'pipelined' not in sweep[0]
  assert sweep[0]['episodes_finished'] == sweep[1]['episodes_finished']
  for k in shapes:
    a, b = np.load(tmp_path / 's1' / f'{k}.npy'), np.load(tmp_path / 's2' / f'{k}.npy')
    assert np.array_equal(a, b), k
  assert np.load(tmp_path / 's1' / 'reward.npy').shape == (sweep[0]['config']['global_lanes'],)
