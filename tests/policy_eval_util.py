"""The contract of evaluate_policy restated in numpy, for the CPU and the GPU tests: per lane, over [T, B] step types and
float64 rewards in step order,

    acc = done = total = 0.0; n = 0
    if type_t != FIRST: acc += r_t; total += r_t
    if type_t == LAST:  done += acc; acc = 0.0; n += 1

Lanes that take no part in an update keep their bits (np.where, never `+ 0.0`)."""
import glob
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_DIR = os.path.join(ROOT, 'tests', 'golden', '.tools', 'policy_rollout')
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FIXTURE_DIR, '*.npz')))


def load(name):
  with np.load(os.path.join(FIXTURE_DIR, name + '.npz')) as z:
    g = {k: z[k] for k in z.files}
  return json.loads(str(g['meta'])), g


def host_loop(step_type, reward):
  """(episodes int32 [B], return_sum f64 [B], episode_return_sum f64 [B]) of step_type [T, B] and reward [T, B] (any
  float dtype, widened to float64; the value on a FIRST step is not looked at)."""
  step_type = np.asarray(step_type)
  reward = np.asarray(reward).astype(np.float64)
  T, B = step_type.shape
  acc, done, total, n = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B, np.int32)
  for t in range(T):
    live, last = step_type[t] != 0, step_type[t] == 2
    r = np.where(live, reward[t], 0.0)
    acc = np.where(live, acc + r, acc)
    total = np.where(live, total + r, total)
    done = np.where(last, done + acc, done)
    acc = np.where(last, 0.0, acc)
    n = n + last.astype(np.int32)
  return n, total, done


def bits(x):
  return np.ascontiguousarray(x, np.float64).view(np.uint64)
