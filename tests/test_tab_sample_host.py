"""CPU: sample_policy / evaluate_sampled_policy (fused softmax rollouts of deep_sea and catch from a table of logits;
bsx_<family>_policy_sample, bsx_<family>_policy_sample_evaluate) without a GPU — the rule the kernel compiles
(bsuite_amd/csrc/bsx_tab_sample.h, through gcc) against a numpy float64 restatement with one rounding per operation, against
utils.observations.gumbel_select and, for three actions, against the rule of the physics families (bsx_gumbel_select through
tests/csrc/gumbel_shim.c); masked, NaN and infinite logits; the distribution of the drawn actions at the lanes, seeds and call
indices of the GPU test; every refusal of the Python entry points, all before any GPU use; the C ABI's declarations, bindings,
exports and argument checks; and the built library: ONE new kernel inside the kernel budget, paid for by the two single-family
group advances that became one kernel, inside the resource conditions, with no store and no barrier inside the loops of its
returns-only branches."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import _native
from bsuite_amd.environments import base, cartpole, catch, deep_sea
from bsuite_amd.utils import observations, wrappers
from oracle import stream
from tests import tab_sample_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bsuite_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
SHIM = os.path.join(ROOT, 'tests', 'csrc', 'tab_sample_shim.c')
GUMBEL_SHIM = os.path.join(ROOT, 'tests', 'csrc', 'gumbel_shim.c')
SAMPLE = dict(deep_sea='bsx_deep_sea_policy_sample', catch='bsx_catch_policy_sample')
SAMPLE_EVAL = dict(deep_sea='bsx_deep_sea_policy_sample_evaluate', catch='bsx_catch_policy_sample_evaluate')
CALLS = ('sample_policy', 'evaluate_sampled_policy')
BETAS = [0.25, 1.0, 4.0]
GCC = ['gcc', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off']

_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ------------------------------------------------------------------------------------------ bsx_tab_sample.h, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  d = tmp_path_factory.mktemp('tab_sample')
  so = str(d / 'tab_sample_shim.so')
  subprocess.check_call(GCC + ['-O2', '-shared', '-fPIC', SHIM, '-o', so])
  lib = ctypes.CDLL(so)
  P, I64, I32, U64, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double
  for name, args in (('shim_select_n', [I64, I32, P, P, P, P, P]), ('shim_select_3', [I64, P, P, P, P]),
                     ('shim_table_actions', [I64, I32, I32, P, P, U64, U64, U64, F64, P])):
    getattr(lib, name).restype = None
    getattr(lib, name).argtypes = args
  lib.shim_lds_bytes.restype = ctypes.c_int32
  lib.shim_stream_sample.restype = ctypes.c_uint32
  # the existing shim of the physics families' rule: bsx_gumbel_select
  so3 = str(d / 'gumbel_shim.so')
  subprocess.check_call(GCC + ['-O2', '-shared', '-fPIC', GUMBEL_SHIM, '-o', so3])
  lib.three = ctypes.CDLL(so3)
  lib.three.shim_select.restype = None
  lib.three.shim_select.argtypes = [I64, P, P, P, P, P]
  return lib


def _select_n(lib, logits, words, beta):
  logits, words = np.ascontiguousarray(logits, np.float32), np.ascontiguousarray(words, np.uint32)
  n_cases, n = logits.shape
  assert words.shape == (n_cases, n)
  beta = np.ascontiguousarray(np.broadcast_to(beta, (n_cases,)), np.float64)
  z, action = np.full((n_cases, n), 7.0, np.float64), np.full(n_cases, -1, np.int32)
  lib.shim_select_n(n_cases, n, _ptr(logits), _ptr(words), _ptr(beta), _ptr(z), _ptr(action))
  return z, action


def _select_3_of_the_physics_families(lib, logits, words, beta):
  logits, words = np.ascontiguousarray(logits, np.float32), np.ascontiguousarray(words, np.uint32)
  beta = np.ascontiguousarray(np.broadcast_to(beta, (logits.shape[0],)), np.float64)
  z, action = np.empty(logits.shape, np.float64), np.full(logits.shape[0], -1, np.int32)
  lib.three.shim_select(logits.shape[0], _ptr(logits), _ptr(words), _ptr(beta), _ptr(z), _ptr(action))
  mine = np.full(logits.shape[0], -1, np.int32)
  lib.shim_select_3(logits.shape[0], _ptr(logits), _ptr(words), _ptr(beta), _ptr(mine))
  np.testing.assert_array_equal(mine, action)
  return action


def _words(rng, n_cases, n):
  w = rng.randint(0, 1 << 32, (n_cases, n), dtype=np.uint64).astype(np.uint32)
  w[0], w[1] = 0, 0xFFFFFFFF                                                                      # the ends of the u grid
  w[2], w[3] = (0, 0xFFFFFFFF, 0)[:n], (0xFFFFFFFF, 0, 0xFFFFFFFF)[:n]
  return w


def test_the_shim_compiles_the_kernels_header(shim):
  assert shim.shim_stream_sample() == tu.STREAM_SAMPLE == 3 and shim.shim_lds_bytes() == 12288
  text = open(os.path.join(CSRC, 'bsx_tab_sample.h')).read()
  assert 'BSX_HD int32_t bsx_gumbel_select_n(const float* l, int n, double beta, const uint32_t* w)' in text
  assert '#include "bsx_policy.h"' in text and '#include "bsx_gumbel.h"' in text
  code = re.sub(r'//.*', '', text)
  assert 'bsx_gumbel_score(l[0], beta, w[0])' in code and 'bsx_gumbel_score(l[a], beta, w[a])' in code and 'z > z_best' in code
  for word in ('bsx_log(', '0x1p-32', ' / ', 'fma'):                                              # no second statement of the score
    assert word not in code, word
  for word in ('-inf logit masks', 'NaN z_a never wins', 'NaN z_0 is never beaten'):               # the consequences, stated
    assert word in text, word
  assert '#include "../../bsuite_amd/csrc/bsx_tab_sample.h"' in open(SHIM).read()
  dev = open(os.path.join(CSRC, 'bsx_tab_sample_device.h')).read()
  assert '#include "bsx_tab_sample.h"' in dev and 'bsx_gumbel_select_n(l, A, p.beta, u.v)' in dev
  assert 'bsx_gumbel_draws(p.sample_seed, lane, step)' in dev
  # the pinned headers and kernels are as they were: nothing of this feature in them
  for f in ('bsx_gumbel.h', 'bsx_policy.h', 'bsx_gumbel_device.h', 'gumbel.hip', 'trajectory.hip', 'bsx_trajectory.h'):
    t = open(os.path.join(CSRC, f)).read()
    assert 'tab_sample' not in t and 'select_n' not in t and 'softmax_kernel' not in t, f
  stream_h = open(os.path.join(ROOT, 'include', 'bsx_stream.h')).read()
  assert re.search(r'#define BSX_STREAM_SAMPLE 3u\b', stream_h) and 'sample_policy' in stream_h


@pytest.mark.parametrize('n', [2, 3])
def test_random_cases_against_the_restatement_and_gumbel_select(shim, n):
  rng = np.random.RandomState(40 + n)
  n_cases = 5000
  logits = (rng.standard_normal((n_cases, n)) * rng.choice([1e-2, 1.0, 8.0], (n_cases, 1))).astype(np.float32)
  words, beta = _words(rng, n_cases, n), rng.choice(BETAS, n_cases)
  z, action = _select_n(shim, logits, words, beta)
  want_z = tu.np_scores(logits, words, beta)
  np.testing.assert_array_equal(_bits(z), _bits(want_z))
  want = tu.np_argmax(want_z)
  np.testing.assert_array_equal(action, want)
  np.testing.assert_array_equal(want, tu.np_select(logits, words, beta))
  assert sorted(set(action.tolist())) == list(range(n))
  assert (action != np.argmax(logits, axis=1)).mean() > 0.05                                        # it samples
  for b in BETAS:
    m = beta == b
    ta = observations.gumbel_select(torch.from_numpy(logits[m]), words[m], temperature=1.0 / b)
    assert ta.dtype is torch.int32
    np.testing.assert_array_equal(ta.numpy(), want[m])
    tb = observations.gumbel_select(torch.from_numpy(logits[m]), torch.from_numpy(words[m].astype(np.int64)), 1.0 / b)
    np.testing.assert_array_equal(tb.numpy(), want[m])
  if n == 3:                                                                                         # the physics families' rule
    np.testing.assert_array_equal(_select_3_of_the_physics_families(shim, logits, words, beta), action)
  doc = observations.gumbel_select.__doc__
  assert '[B, A]' in doc and 'sample_policy' in doc


def test_masked_nan_and_infinite_logits(shim):
  nan, inf = np.float32('nan'), np.float32('inf')
  same = (0x9E3779B9,) * 3                       # one word for every action: equal noise, so equal logits tie
  lo, hi = 0x00000010, 0xFFFFFFF0                # g(lo) = -3.0.., g(hi) = +19.4..
  cases3 = [  # (logits, words, want)
      ((1, 1, 1), same, 0), ((0, 1, 1), same, 1), ((0, 0, 1), same, 2), ((-0.0, 0.0, -0.0), same, 0),
      # -inf masks an action whatever its noise: the Gumbel variate is finite
      ((-inf, 0, 0), (hi, lo, lo), 1), ((0, -inf, 0), (lo, hi, lo), 0), ((0, 0, -inf), (lo, lo, hi), 0), ((-inf, -inf, 0), (hi, hi, lo), 2),
      ((-inf, 0, -inf), (hi, lo, hi), 1), ((-inf, -1e30, -inf), (hi, lo, hi), 1),
      # all -inf: nothing beats z_0
      ((-inf, -inf, -inf), (lo, hi, hi), 0), ((-inf, -inf, -inf), same, 0),
      # NaN in each position: it never wins, and in position 0 it is never beaten
      ((nan, 1, 2), same, 0), ((nan, inf, inf), (lo, hi, hi), 0), ((0, nan, 2), same, 2), ((0, nan, -2), same, 0), ((0, 1, nan), same, 1),
      ((0, nan, nan), (lo, hi, hi), 0), ((nan, nan, nan), same, 0), ((-inf, nan, 0), same, 2), ((-inf, nan, -inf), (lo, hi, hi), 0),
      # +inf always wins, the lowest of two
      ((-inf, 0, inf), (hi, hi, lo), 2), ((inf, inf, 0), (lo, hi, hi), 0), ((0, inf, inf), (hi, lo, hi), 1), ((inf, 0, 0), (lo, hi, hi), 0),
      # the noise decides between equal logits
      ((0, 0, 0), (lo, hi, lo), 1), ((0, 0, 0), (lo, lo, hi), 2), ((0, 0, 0), (hi, lo, lo), 0),
  ]
  cases2 = [
      ((1, 1), same, 0), ((0, 1), same, 1), ((1, 0), same, 0), ((-0.0, 0.0), same, 0),
      ((-inf, 0), (hi, lo), 1), ((0, -inf), (lo, hi), 0), ((-inf, -inf), (lo, hi), 0), ((-inf, -inf), same, 0),
      ((nan, 1), same, 0), ((nan, inf), (lo, hi), 0), ((0, nan), (hi, lo), 0), ((-inf, nan), (lo, hi), 0), ((nan, nan), same, 0),
      ((0, inf), (hi, lo), 1), ((inf, 0), (lo, hi), 0), ((inf, inf), (lo, hi), 0), ((-inf, inf), (hi, lo), 1),
      ((0, 0), (lo, hi), 1), ((0, 0), (hi, lo), 0),
  ]
  for n, cases in ((2, cases2), (3, cases3)):
    logits = np.array([c[0] for c in cases], np.float32)
    words = np.array([c[1][:n] for c in cases], np.uint32)
    for b in BETAS:
      z, action = _select_n(shim, logits, words, b)
      np.testing.assert_array_equal(_bits(z), _bits(tu.np_scores(logits, words, np.full(len(cases), b))))
      np.testing.assert_array_equal(action, tu.np_argmax(z))
      for k, c in enumerate(cases):
        assert action[k] == c[2], (n, b, k, c)
      np.testing.assert_array_equal(observations.gumbel_select(torch.from_numpy(logits), words, 1.0 / b).numpy(), action)
      if n == 3:
        np.testing.assert_array_equal(_select_3_of_the_physics_families(shim, logits, words, b), action)
  # a masked column is never drawn, at any word
  rng = np.random.RandomState(1)
  for n in (2, 3):
    logits = rng.standard_normal((4000, n)).astype(np.float32)
    logits[:, 0] = -np.inf
    _, action = _select_n(shim, logits, _words(rng, 4000, n), 1.0)
    assert action.min() >= 1 and action.max() == n - 1


def test_a_whole_lane_step_of_the_action_source(shim):
  """key -> clamp -> the row's logits -> block 0 of stream 3 -> the rule, as the kernel chains them: against the restatement
  with oracle/stream.py's words, for keys inside and outside the table."""
  rng = np.random.RandomState(9)
  for n, S in ((2, 16), (3, 250)):
    table = rng.standard_normal((S, n)).astype(np.float32)
    n_cases, lane0, seed, step = 3000, (1 << 32) - 17, (1 << 63) + 5, (1 << 34) + 3
    keys = rng.randint(0, S, n_cases).astype(np.int32)
    keys[:6] = (-1, -(1 << 31), S, S + 7, (1 << 31) - 1, 0)
    action = np.full(n_cases, -1, np.int32)
    shim.shim_table_actions(n_cases, n, S, _ptr(table), _ptr(keys), seed, lane0, step, 0.5, _ptr(action))
    words = stream.words(seed, np.uint64(lane0) + np.arange(n_cases, dtype=np.uint64), step, tu.STREAM_SAMPLE, n)
    want = tu.np_select(table[np.clip(keys, 0, S - 1)], words, 0.5)
    np.testing.assert_array_equal(action, want)


@pytest.mark.parametrize('A', [2, 3])
def test_action_frequencies_follow_the_softmax(A):
  """The frequency case of the GPU test (tests/tab_sample_util.py): constant rows (0, ln 3) / (0, ln 2, ln 4), 4096 lanes from
  lane 2^32 - 17 on, the live call indices of one fresh call of 11 steps: every action's frequency within 4 sigma of the
  softmax, sigma = sqrt(p (1 - p) / N), at the recorded sample seed."""
  assert (tu.FREQ_B, tu.FREQ_T, tu.FREQ_LANE0) == (4096, 11, (1 << 32) - 17)
  l = tu.freq_row(A)
  np.testing.assert_array_equal(l, np.log(np.array([1.0, 3.0] if A == 2 else [1.0, 2.0, 4.0])).astype(np.float32))
  p = np.array([1, 3], np.float64) / 4 if A == 2 else np.array([1, 2, 4], np.float64) / 7
  q = np.exp(l.astype(np.float64))
  np.testing.assert_allclose(q / q.sum(), p, rtol=1e-7)
  counts = tu.restated_counts(A)
  N = tu.FREQ_B * len(tu.FREQ_LIVE[A])
  assert counts.sum() == N and all(0 <= t < tu.FREQ_T for t in tu.FREQ_LIVE[A])
  sigma = np.sqrt(p * (1 - p) / N)
  freq = counts / N
  print('A', A, 'sample seed', tu.FREQ_SEED[A], 'counts', counts, 'in sigma', (freq - p) / sigma)
  assert (np.abs(freq - p) <= 4 * sigma).all(), (counts, p, (freq - p) / sigma)


def test_the_shim_runs_stand_alone_under_the_sanitizers(tmp_path):
  """bsx_tab_sample.h with its own main under AddressSanitizer and UBSan, on the CPU: a program of its own, nothing loaded
  into python."""
  exe = str(tmp_path / 'tab_sample_shim_main')
  cmd = GCC + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DTAB_SAMPLE_SHIM_MAIN', SHIM, '-o', exe, '-lm']
  if subprocess.run(cmd, capture_output=True).returncode != 0:
    pytest.skip('this gcc has no sanitizer runtime')
  out = subprocess.run([exe], capture_output=True, text=True)
  assert out.returncode == 0, out
  seen = [int(x) for x in out.stdout.split()]
  assert len(seen) == 3 and sum(seen) == 2 * 3 * 64 and seen[2] > 0, out


# ------------------------------------------------------------------------------------------ the Python entry points
def _envs():
  return [deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4, observation_mode='index'),
          catch.Catch(seed=0, batch=4, observation_mode='index')]


def _logits(env, P=None):
  try:
    S, A = env.policy_num_states, env.action_spec().num_values
  except ValueError:
    S, A = 4, 2
  return torch.zeros((S, A) if P is None else (P, S, A), dtype=torch.float32)


def _refused(env, name, exc=ValueError, match=None, **kw):
  """env.<name>(...) raises, its message names the caller (or the family), and nothing was allocated."""
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  logits = kw.pop('logits') if 'logits' in kw else _logits(raw)                                     # (None is one of the bad values)
  with pytest.raises(exc, match=match or name):
    getattr(env, name)(logits, kw.pop('num_steps', 4), **kw)
  assert not raw._allocated and not raw._policy_rollout_out and raw._policy_eval_out is None        # pylint: disable=protected-access


def test_signatures_docstrings_and_families():
  for name in CALLS:
    fn = getattr(base.Environment, name)
    p = inspect.signature(fn).parameters
    assert list(p) == ['self', 'logits', 'num_steps', 'policy_index', 'temperature', 'sample_seed']
    assert [p[k].kind for k in ('policy_index', 'temperature', 'sample_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
    assert p['policy_index'].default is None and p['temperature'].default == 1.0 and p['sample_seed'].default == 0
    assert list(p)[3:] == list(inspect.signature(base.Environment.sample_linear).parameters)[4:]
    for env in _envs():                                                                               # every refusal first: the last
      env._device = torch.device('cpu')                                                               # one of the call allocates nothing
      _refused(env, name, sample_seed=-1, match='sample_seed must be')
      # the order, two faults at a time: the environment, the logits, the population rule, the temperature, the seed
      idx = torch.zeros(4, dtype=torch.int32)
      _refused(env, name, logits=None, num_steps=0, match='num_steps')
      _refused(env, name, logits=None, policy_index=idx, match='logits must be')
      _refused(env, name, policy_index=idx, temperature=0.0, match='must be None')
      _refused(env, name, temperature=0.0, sample_seed=-1, match='temperature must be')
      env._logging = dict(steps=None)
      _refused(env, name, logits=None, num_steps=0, match='Logging')
  # the environment's part and the population rule are rollout_policy's: the same words
  for drawn, greedy in (('sample_policy', 'rollout_policy'), ('evaluate_sampled_policy', 'evaluate_policy')):
    for spoil, kw in ((lambda e: setattr(e, '_grouped_by', object()), {}), (lambda e: None, dict(num_steps=0)),
                      (lambda e: None, dict(policy_index=torch.zeros(4, dtype=torch.int32)))):
      said = []
      for call, table in ((drawn, _logits), (greedy, lambda e: torch.zeros(e.policy_num_states, dtype=torch.uint8))):
        env = _envs()[1]
        env._device = torch.device('cpu')
        spoil(env)
        args = dict(kw)
        with pytest.raises((ValueError, RuntimeError)) as info:
          getattr(env, call)(table(env), args.pop('num_steps', 4), **args)
        said.append(str(info.value).replace(call, ''))
        assert not env._allocated
      assert said[0] == said[1], (drawn, kw)
  doc = base.Environment.sample_policy.__doc__
  for word in ('ts[t] = step(a); actions[t] = a', 'gumbel_select', 'policy_key', 'stream 3', 'rollout(actions)', 'policy_index',
               'cached per T', 'temperature', 'sample_seed', '4-byte', '-inf', 'rollout_policy'):
    assert word in doc, word
  doc = base.Environment.evaluate_sampled_policy.__doc__
  for word in ('sample_policy', 'PolicyEvaluation', 'evaluate_policy', 'float64'):
    assert word in doc, word
  abi = lambda cls, name: cls._closed_loop_abi(object.__new__(cls), name)                             # pylint: disable=protected-access
  for fam, cls in (('deep_sea', deep_sea.DeepSea), ('catch', catch.Catch)):
    assert abi(cls, 'sample_policy') == SAMPLE[fam] and abi(cls, 'evaluate_sampled_policy') == SAMPLE_EVAL[fam]
    assert SAMPLE[fam] in _native.EXPORTED and SAMPLE_EVAL[fam] in _native.EXPORTED
  for name in CALLS:
    assert abi(base.Environment, name) is None and abi(cartpole.Cartpole, name) is None


@pytest.mark.parametrize('name', CALLS)
def test_views_families_and_modes_are_refused(name):
  _refused(catch.Catch(seed=0), name, match='batched view')
  _refused(deep_sea.DeepSea(size=8, mapping_seed=0, seed=0), name, match='batched view')
  for bsuite_id in ('bandit/0', 'cartpole/0', 'mountain_car/0', 'memory_len/0', 'umbrella_length/0', 'discounting_chain/0',
                    'cartpole_swingup/0'):
    _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), name, match='deep_sea and catch only')
  # non-index modes
  _refused(catch.Catch(seed=0, batch=4), name, match="observation_mode='index'")
  _refused(catch.Catch(seed=0, batch=4, observation_mode='delta'), name, match="observation_mode='index'")
  _refused(deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4), name, match="observation_mode='index'")
  for dt in (torch.uint8, 'float16', torch.bfloat16):
    _refused(catch.Catch(seed=0, batch=4, observation_dtype=dt), name, match="observation_mode='index'")
  _refused(catch.Catch(seed=0, batch=4, observation_mode='index', rng='mt19937'), name, match='philox')
  _refused(deep_sea.DeepSea(size=6, mapping_seed=0, seed=0, batch=4, observation_mode='index', rng='mt19937'), name, match='philox')
  for env in _envs():
    env._logging = dict(steps=None)           # what enable_logging() leaves behind (it allocates: not without a GPU)
    _refused(env, name, match='Logging')
  for env in _envs():
    env._grouped_by = object()                # what SweepBatch sets while its prepared groups hold the column pointers
    _refused(env, name, exc=RuntimeError, match='release_groups')
  # the messages carry the caller's name
  with pytest.raises(ValueError, match=name + r'\(\) needs the batched view'):
    getattr(catch.Catch(seed=0), name)(torch.zeros((250, 3)), 4)


def test_the_messages_of_the_two_existing_calls_did_not_change():
  with pytest.raises(ValueError, match=r'^rollout_policy\(\) needs the batched view \(batch=B\)$'):
    catch.Catch(seed=0).rollout_policy(torch.zeros(250, dtype=torch.uint8), 4)
  with pytest.raises(ValueError, match=r"^evaluate_policy\(\) looks its actions up by the index observation: build the environment with "
                                       r"observation_mode='index' \(this one is 'dense', torch.float32\)$"):
    catch.Catch(seed=0, batch=4).evaluate_policy(torch.zeros(250, dtype=torch.uint8), 4)
  env = catch.Catch(seed=0, batch=4, observation_mode='index')
  env._device = torch.device('cpu')
  ok = torch.zeros(250, dtype=torch.uint8)
  with pytest.raises(ValueError, match=r'^rollout_policy: num_steps must be an integer >= 1, got 0$'):
    env.rollout_policy(ok, 0)
  with pytest.raises(ValueError, match=r'^rollout_policy: epsilon must be a number in \[0, 1\], got 2$'):
    env.rollout_policy(ok, 4, epsilon=2)
  with pytest.raises(ValueError, match=r'^evaluate_policy: explore_seed must be an integer in \[0, 2\^64\), got -1$'):
    env.evaluate_policy(ok, 4, explore_seed=-1)
  with pytest.raises(ValueError, match=r'^rollout_policy: policy must be a contiguous uint8 tensor of shape \(250,\) or \(P, 250\) on cpu$'):
    env.rollout_policy(ok[:-1], 4)
  with pytest.raises(ValueError, match=r'^evaluate_policy: policy_index names the row of a population of tables; with one table it must be None$'):
    env.evaluate_policy(ok, 4, policy_index=torch.zeros(4, dtype=torch.int32))
  with pytest.raises(ValueError, match=r'^rollout_policy: a population of 2 tables needs policy_index, a contiguous int32 tensor of shape '
                                       r'\(4,\) on cpu$'):
    env.rollout_policy(torch.zeros((2, 250), dtype=torch.uint8), 4)
  with pytest.raises(ValueError, match=r'^Cartpole has no tabular policy rollout \(deep_sea and catch only\)$'):
    cartpole.Cartpole(seed=0, batch=4).rollout_policy(ok, 4)
  # the order of the refusals too: the scalars before the table
  with pytest.raises(ValueError, match='epsilon'):
    env.rollout_policy(None, 4, epsilon=2)
  assert env._check_rollout_policy(ok, 4, None, 0.0, 0) == 1                                         # pylint: disable=protected-access


@pytest.mark.parametrize('name', CALLS)
def test_the_wrappers_refuse_instead_of_delegating(name):
  for make in (lambda e: wrappers.RewardNoise(e, noise_scale=0.5, seed=1), lambda e: wrappers.RewardScale(e, reward_scale=2.0)):
    for raw in _envs():
      _refused(make(raw), name, match='not available through')
      _refused(raw, name, match='reward wrapper')                       # ... and the raw environment knows it is wrapped
  for bsuite_id in ('catch_noise/2', 'catch_scale/4', 'deep_sea_stochastic/3'):
    env = bsuite_amd.load_from_id(bsuite_id, batch=4, observation_mode='index')
    if hasattr(env, 'raw_env'):
      _refused(env, name, match='not available through')
  # every wrapper class carries its own method (attribute delegation would reach the raw environment's)
  for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    fn = getattr(cls, name)
    assert fn is not getattr(base.Environment, name) and any(name in vars(c) for c in cls.__mro__[:-1]), cls
    with pytest.raises(ValueError, match=name):
      fn(object.__new__(cls), torch.zeros((4, 2)), 4, temperature=2.0, sample_seed=1)
  image = wrappers.ImageObservation(catch.Catch(seed=0, batch=4), (84, 84, 1))
  _refused(image, name, match='not available through ImageObservation')


@pytest.mark.parametrize('name', CALLS)
def test_arguments_are_checked_before_any_gpu_use(name):
  for env in _envs():
    env._device = torch.device('cpu')       # the checks themselves, on host tensors: dtype, shape, contiguity
    S, A = env.policy_num_states, env.action_spec().num_values
    assert A == (2 if isinstance(env, deep_sea.DeepSea) else 3)
    ok, pop = _logits(env), _logits(env, 4)
    idx = torch.zeros(4, dtype=torch.int32)
    for n in (0, -1, 2.0, None, '4', True):
      _refused(env, name, logits=ok, num_steps=n, match=f'{name}: num_steps')
    for bad in (ok.to(torch.float64), ok.to(torch.float16), ok.to(torch.uint8), ok.numpy(), ok.tolist(), None,
                torch.zeros((S, A + 1)), torch.zeros((S, A - 1)), torch.zeros((S, 5 - A)),                 # the other family's A
                torch.zeros((S + 1, A)), torch.zeros((S - 1, A)), torch.zeros(S * A), torch.zeros((A, S)), torch.zeros((2, 2, S, A)),
                torch.zeros((0, S, A)), torch.zeros((S, 2 * A))[:, ::2], torch.zeros((2 * S, A))[::2], torch.zeros(())):
      _refused(env, name, logits=bad, match=f'{name}: logits must be')
    _refused(env, name, logits=ok, policy_index=idx, match='must be None')
    _refused(env, name, logits=ok.reshape(1, S, A), policy_index=idx, match='must be None')                # [1, S, A] is one table
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, name, logits=pop, policy_index=bad, match='policy_index')
    for t in (0.0, -1.0, -0.0, float('nan'), float('inf'), float('-inf'), 5e-324, 1e-310, '1.0', None, True, [1.0]):
      _refused(env, name, logits=ok, temperature=t, match=f'{name}: temperature')
    for seed in (-1, 1 << 64, 0.5, None, True, '3'):
      _refused(env, name, logits=ok, sample_seed=seed, match=f'{name}: sample_seed')
    for word in ('epsilon', 'explore_seed'):                               # there is no epsilon: the softmax explores
      with pytest.raises(TypeError, match=word):
        getattr(env, name)(ok, 4, **{word: 0})
    # the order: the table before the temperature
    _refused(env, name, logits=None, temperature=0.0, match='logits must be')
    # a view that starts one float into a buffer passes the checks (only 4-byte alignment is assumed)
    view = torch.zeros(S * A + 1)[1:].reshape(S, A)
    assert view.is_contiguous() and view.data_ptr() % 8 == 4
    P, beta = env._check_sample_policy(view, 4, None, 4.0, (1 << 64) - 1, name)      # pylint: disable=protected-access
    assert (P, beta) == (1, 0.25)
    assert env._check_sample_policy(pop, np.int64(7), idx, np.float32(0.5), np.int64(5), name) == (4, 2.0)   # pylint: disable=protected-access
    assert not env._allocated                                                                              # pylint: disable=protected-access
  # host logits for an environment on the GPU
  env = catch.Catch(seed=0, batch=4, observation_mode='index')
  _refused(env, name, logits=_logits(env), match='logits must be')


# ------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_export_agree_and_the_abi_stays_v12():
  header = open(HEADER).read()
  assert re.search(r'#define BSX_ABI_VERSION 12\b', header)
  assert _native.ABI_VERSION == 12 and _native.lib.bsx_abi_version() == 12
  plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  out = subprocess.check_output(['nm', '-D', '--defined-only', _native.SO_PATH], text=True)
  P = ctypes.c_void_p
  text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()

  def types_of(name):
    decl = re.search(r'int ' + name + r'\(([^;]*)\);', plain)
    assert decl, f'include/bsuite_amd.h does not declare {name}'
    return [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(decl.group(1).split()).split(',')]

  for fam in ('deep_sea', 'catch'):
    cfg = dict(deep_sea=_native.DeepSeaCfg, catch=_native.CatchCfg)[fam]
    for name, like, out_t, out_c in ((SAMPLE[fam], f'bsx_{fam}_policy_rollout', 'bsx_timestep_t', _native.TimeStepPtrs),
                                     (SAMPLE_EVAL[fam], f'bsx_{fam}_policy_evaluate', 'bsx_policy_eval_t', _native.PolicyEvalPtrs)):
      types = types_of(name)
      assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_policy_logits_t*', 'int32_t*', out_t, 'double*']
      assert [t.replace('bsx_policy_logits_t', 'bsx_policy_t') for t in types] == types_of(like)      # the signature of the greedy call
      assert name in _native.EXPORTED
      fn = getattr(_native.lib, name)
      assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.PolicyLogits), P, out_c, P]
      assert fn.restype is ctypes.c_int
      assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
      assert name in text, f'INTEGRATION.md does not describe {name}'
      assert 'extern "C" int ' + name + '(' in open(os.path.join(CSRC, fam + '.hip')).read()
  body = re.search(r'typedef struct \{([^}]*)\} bsx_policy_logits_t;', plain).group(1)
  fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
  assert fields == ['const float* logits', 'int32_t n_states, n_actions, n_policies', 'const int32_t* policy_index',
                    'double inv_temperature', 'uint64_t sample_seed', 'int32_t* actions_out']
  assert [f[0] for f in _native.PolicyLogits._fields_] == ['logits', 'n_states', 'n_actions', 'n_policies', 'policy_index',      # pylint: disable=protected-access
                                                           'inv_temperature', 'sample_seed', 'actions_out']
  # the layout, against the C compiler's
  src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bsuite_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
         'sizeof(bsx_policy_logits_t), offsetof(bsx_policy_logits_t, n_actions), offsetof(bsx_policy_logits_t, policy_index), '
         'offsetof(bsx_policy_logits_t, inv_temperature), offsetof(bsx_policy_logits_t, sample_seed), offsetof(bsx_policy_logits_t, actions_out)); return 0; }\n')
  import tempfile
  with tempfile.TemporaryDirectory() as d:
    open(os.path.join(d, 'l.c'), 'w').write(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'l.c'), '-o', os.path.join(d, 'l')])
    got = [int(x) for x in subprocess.check_output([os.path.join(d, 'l')], text=True).split()]
  L = _native.PolicyLogits
  assert got == [ctypes.sizeof(L), L.n_actions.offset, L.policy_index.offset, L.inv_temperature.offset, L.sample_seed.offset,
                 L.actions_out.offset] == [56, 12, 24, 32, 40, 48]
  note = header[header.index('fused sampled rollouts from a table of logits'):header.index('} bsx_policy_logits_t;')]
  for word in ('BSX_STREAM_SAMPLE', 'BSX_ERANGE', 'BSX_EALIGN', 'BSX_EINVAL', 'inv_temperature', '4-byte aligned', 'n_actions'):
    assert word in note, word


def _abi_case(fam):
  if fam == 'deep_sea':
    return _native.DeepSeaCfg(size=10, deterministic=1, move_cost=0.001, inv_size=0.1), 100, 2, _native.DeepSeaCfg(size=65)
  return _native.CatchCfg(10, 5), 250, 3, _native.CatchCfg(1, 5)


@pytest.mark.parametrize('kind', ['sample', 'sample_evaluate'])
@pytest.mark.parametrize('fam', ['deep_sea', 'catch'])
def test_argument_checks_of_the_entry_points(fam, kind):
  """Every refusal comes before any device work: garbage stands in for device pointers, none is dereferenced.  The codes and
  their order are those of bsx_<family>_policy_rollout / _policy_evaluate; a wrong n_actions is BSX_EINVAL where a wrong
  n_states is, a bad inv_temperature BSX_ERANGE where an epsilon outside [0, 1] is there, and logits off the 4-byte grid are
  BSX_EALIGN, after the pointers."""
  record = kind == 'sample'
  fn = getattr(_native.lib, (SAMPLE if record else SAMPLE_EVAL)[fam])
  cfg, S, A, bad_cfg = _abi_case(fam)
  junk = 0xDEAD0010                                                # never mapped: a dereference would fault (16-byte aligned)
  E = _native
  nan, inf = float('nan'), float('inf')

  def call(**kw):
    c = _native.Call(n_lanes=kw.pop('n_lanes', 4), n_steps=kw.pop('n_steps', 4), flags=kw.pop('flags', E.CALL_OBS_INDEX))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def pol(**kw):
    d = dict(logits=junk, n_states=S, n_actions=A, n_policies=1, policy_index=None, inv_temperature=1.0, sample_seed=0,
             actions_out=junk if record else None)
    d.update(kw)
    return _native.PolicyLogits(**d)

  def outs(*ptrs):
    if record:
      return _native.TimeStepPtrs(*(ptrs or (junk,) * 4))
    return _native.PolicyEvalPtrs(*(ptrs or (junk,) * 3))

  def run(c, q, state=junk, out=None, info=junk, cfg_=cfg):
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, state, outs() if out is None else out, info)

  # null structs
  assert run(call(), pol(), cfg_=None) == E.BSX_ENULL
  assert run(None, pol()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: the observation code, and everything the fused loop does not carry — before the scalars and the temperature
  for flags in (0, E.CALL_STATE_TAGGED, E.CALL_OBS_U8, E.CALL_OBS_INDEX | E.CALL_OBS_U8, E.CALL_OBS_INDEX | E.CALL_OBS_F16,
                E.CALL_OBS_INDEX | E.CALL_OBS_BF16):
    assert run(call(flags=flags), pol(n_states=-1)) == E.BSX_EMODE, flags
    assert run(call(flags=flags), pol(inv_temperature=nan)) == E.BSX_EMODE, flags
  lg = _native.Logging()
  assert run(call(logging=ctypes.pointer(lg)), pol(n_actions=7)) == E.BSX_EMODE
  for wrap in (E.WRAP_SCALE, E.WRAP_NOISE, E.WRAP_SCALE_NOISE, E.WRAP_NOISE_SCALE):
    c = call()
    c.wrap.kind = wrap
    assert run(c, pol()) == E.BSX_EMODE, wrap
  c = call()
  c.stream.mt_state, c.stream.mt_pos = junk, junk
  assert run(c, pol()) == E.BSX_EMODE
  for member in ('reward_f64', 'obs_paint', 'state_alt'):
    assert run(call(**{member: junk}), pol()) == E.BSX_EMODE, member
  assert run(call(force_reset=1), pol(inv_temperature=0.0)) == E.BSX_EMODE
  assert run(call(action_ring=4), pol()) == E.BSX_EMODE
  # BSX_EINVAL: the scalars, before the temperature
  for n in (0, -1):
    assert run(call(n_steps=n), pol()) == E.BSX_EINVAL
    assert run(call(n_steps=n), pol(inv_temperature=-1.0)) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), pol(inv_temperature=inf)) == E.BSX_EINVAL
  for s in (S - 1, S + 1, 0, -S):
    assert run(call(), pol(n_states=s)) == E.BSX_EINVAL, s
  for a in (A - 1, A + 1, 5 - A, 0, -A, 1 << 20):                    # the other family's width among them
    assert run(call(), pol(n_actions=a)) == E.BSX_EINVAL, a
    assert run(call(), pol(n_actions=a, inv_temperature=nan)) == E.BSX_EINVAL, a
    assert run(call(n_lanes=0), pol(n_actions=a)) == E.BSX_EINVAL, a
  for n in (0, -3):
    assert run(call(), pol(n_policies=n)) == E.BSX_EINVAL
    assert run(call(), pol(n_policies=n, inv_temperature=0.0)) == E.BSX_EINVAL
  # BSX_ERANGE: inv_temperature finite and > 0 — before an empty call returns and before any pointer is looked at
  for b in (0.0, -0.0, -1.0, nan, inf, -inf):
    assert run(call(), pol(inv_temperature=b)) == E.BSX_ERANGE, b
    assert run(call(n_lanes=0), pol(inv_temperature=b)) == E.BSX_ERANGE, b
    assert run(call(), pol(inv_temperature=b, logits=None), state=None) == E.BSX_ERANGE, b
  assert run(call(), pol(), cfg_=bad_cfg) == E.BSX_ERANGE
  assert run(call(flags=0), pol(), cfg_=bad_cfg) == E.BSX_ERANGE                             # (the cfg comes first)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at; the extreme temperatures are accepted
  for b in (1.0, 5e-324, 1.7976931348623157e308):
    assert run(call(n_lanes=0), pol(logits=None, inv_temperature=b, actions_out=None), state=None,
               out=outs(*((0,) * (4 if record else 3))), info=None) == 0, b
  assert run(call(n_lanes=0), pol(logits=junk + 2)) == 0                                      # (not even the alignment)
  # BSX_ENULL: every pointer — the other ones garbage
  assert run(call(), pol(logits=None)) == E.BSX_ENULL
  assert run(call(), pol(), state=None) == E.BSX_ENULL
  assert run(call(), pol(), info=None) == E.BSX_ENULL
  n_out = 4 if record else 3
  for k in range(n_out):
    ptrs = [junk] * n_out
    ptrs[k] = 0
    assert run(call(), pol(), out=outs(*ptrs)) == E.BSX_ENULL, k
  if record:
    assert run(call(), pol(actions_out=None)) == E.BSX_ENULL                                  # the action column
    assert run(call(), pol(), out=outs(junk, junk, junk, junk + 8)) == E.BSX_EALIGN           # the index rows: 16 bytes, as in the greedy call
  else:
    assert run(call(n_lanes=0), pol(actions_out=junk)) == 0                                   # (not looked at)
  assert run(call(), pol(n_policies=2)) == E.BSX_ENULL                                        # a population without policy_index
  # BSX_EALIGN: logits off the 4-byte grid — after the pointers; 4 bytes are enough
  for off in (1, 2, 3, 5, 6, 7):
    assert run(call(), pol(logits=junk + off)) == E.BSX_EALIGN, off
    assert run(call(), pol(logits=junk + off), state=None) == E.BSX_ENULL, off
  assert run(call(n_lanes=1 << 40), pol()) == E.BSX_EINVAL                                    # more workgroups than a grid holds
  assert run(call(action_ring=-2), pol()) == E.BSX_EINVAL


# ------------------------------------------------------------------------------------------ the source text
def test_the_kernel_bodies_use_the_headers():
  dev = open(os.path.join(CSRC, 'bsx_tab_sample_device.h')).read()

  def fn_text(name):
    t = dev[dev.index('void ' + name + '('):]
    return t[:t.index('\n}\n')]

  action = dev[dev.index('int bsx_tab_softmax_action('):]
  action = action[:action.index('\n}\n')]
  for call_ in ('bsx_policy_clamp(fn.policy_key(st), p.n_states)', 'bsx_gumbel_draws(p.sample_seed, lane, step)',
                'bsx_gumbel_select_n(l, A, p.beta, u.v)', '(bsx_tab_lds)s_tab + key * A', 'asm volatile("" : "+v"(l[c]))'):
    assert call_ in action, call_
  assert action.index('fn.policy_key(st)') < action.index('if (p.in_lds != 0)') < action.index('bsx_gumbel_draws(') < action.index('bsx_gumbel_select_n(')
  record, returns = fn_text('bsx_tab_softmax_record_body'), fn_text('bsx_tab_softmax_returns_body')
  for body in (record, returns):
    loop = body[body.index('for (int t = 0; t < n_steps; ++t) {'):]
    loop = loop[:loop.index('\n    }\n')]
    assert 'if (!resets) act = bsx_tab_softmax_action<A>(' in loop and 'Fam::resets(st)' in loop        # nothing looked up or drawn on a reset
    assert loop.count('bsx_tab_softmax_view(ka)') == 1 and '__syncthreads' not in loop and 'atomic' not in loop
    assert 'bsx_policy_clamp(p.policy_index[i], p.n_policies)' in dev
  loop = record[record.index('for (int t = 0;'):]
  for call_ in ('Fam::template advance<true>(', 'bsx_emit_at<0, 0, false, -1, BSX_OUT_SCALARS.rollout>(',
                'bsx_index_store<BSX_OUT_INDEX.rollout>(', 'bsx_st<BSX_OUT_SCALARS.rollout>(&kt.p.actions_out[oi]'):
    assert call_ in loop, call_
  loop = returns[returns.index('for (int t = 0;'):]
  loop = loop[:loop.index('\n    }\n')]
  for call_ in ('Fam::advance_deferred(', 'bsx_eval_accumulate(&e, type, reward)'):
    assert call_ in loop, call_
  for word in ('bsx_emit', 'bsx_st<', 'bsx_index_store', 'commit_deferred', '.state[i] ='):
    assert word not in loop, word
  assert 'Fam::commit_deferred(a1, i, pend)' in returns
  # no second statement of the rule outside the C99 headers
  for f in ('bsx_tab_sample_device.h', 'tab_sample.hip'):
    text = re.sub(r'//.*', '', open(os.path.join(CSRC, f)).read())
    for word in ('z_best', 'bsx_log(', '0x1p-32', 'bsx_gumbel_score(', 'bsx_gumbel_select('):
      assert word not in text, (f, word)
  hip = open(os.path.join(CSRC, 'tab_sample.hip')).read()
  assert hip.count('__global__') == 1
  assert '__global__ void __launch_bounds__(BSX_BLOCK) bsx_tab_softmax_kernel(const bsx_tab_softmax_args a)' in hip
  for inst in ('record_body<bsx_tab_softmax_deep_sea>', 'returns_body<bsx_tab_softmax_deep_sea>', 'record_body<bsx_tab_softmax_catch>',
               'returns_body<bsx_tab_softmax_catch>'):
    assert 'bsx_tab_softmax_' + inst in hip, inst
  assert 's_tab[BSX_TAB_SAMPLE_LDS_BYTES / 4]' in hip
  # what paid for the kernel: one tagged kernel for the lane advance of a single-family group, its body the shared one
  misc = open(os.path.join(CSRC, 'misc.hip')).read()
  assert '__global__ void __launch_bounds__(BSX_BLOCK) bsx_pair_advance_group_kernel(const bsx_pair_advance_group_args a)' in misc
  assert 'bsx_advance_body<deep_sea_fam>(' in misc and 'bsx_advance_body<catch_fam>(' in misc
  pair_dev = open(os.path.join(CSRC, 'bsx_pair_device.h')).read()
  assert not re.search(r'__global__[^;{]*bsx_advance_group_kernel', pair_dev)
  assert 'bsx_launch_pair_advance_group(HotFn::FAMILY, g->d_args, g->index1(), g->total_blocks, st)' in open(os.path.join(CSRC, 'bsx_pair_host.h')).read()


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = 'bsx_tab_softmax_kernel'
FOLDED = 'bsx_pair_advance_group_kernel'


@needs_llvm
def test_product_library_has_the_one_new_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  assert [n for n in ks if 'softmax' in n or 'tab_sample' in n] == [NEW]                      # ONE kernel for the four cases
  for word in ('index', 'policy', 'eval', 'gumbel', 'trajectory', 'linear', 'score', 'mlp', 'hot_cells', 'hot_stream_tiny', 'calib_', 'mnist_'):
    assert word not in NEW and word not in FOLDED, word
  # what paid for it: the lane advance of a single-family group is one kernel for deep_sea and catch
  assert sorted(n for n in ks if 'advance_group' in n) == [FOLDED]
  assert not any(n.startswith('bsx_advance_group_kernel') for n in ks)
  g = ks[FOLDED]
  assert g['private_segment_fixed_size'] == 0 and g['vgpr_spill_count'] == 0 and g['sgpr_spill_count'] == 0 and g['agpr_count'] == 0, g
  assert g['vgpr_count'] <= 64 and g['group_segment_fixed_size'] <= 1024, g
  # ... and its neighbours, the store streams of the same groups and the stand-alone advances, are as they were
  for n in ('bsx_hot_stream_group_kernel<deep_sea_hot, 4>', 'bsx_hot_stream_group_kernel<catch_hot, 2>',
            'bsx_advance_kernel<deep_sea_fam, true, -1>', 'bsx_advance_kernel<catch_fam, true, -1>', 'bsx_tab_eval_kernel',
            'bsx_policy_rollout_kernel<deep_sea_fam, deep_sea_hot>', 'bsx_policy_rollout_kernel<catch_fam, catch_hot>', 'bsx_gumbel_kernel'):
    assert n in ks, n
  k = ks[NEW]
  print(NEW, {f: k[f] for f in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'kernarg_segment_size')})
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k      # no spill, no scratch
  assert k['agpr_count'] == 0, k
  assert 12288 <= k['group_segment_fixed_size'] <= 16384, k                                   # the table, deep_sea's mapping, two counters


def _loops(text):
  """{header label: [instructions]} of the loops of a kernel: the compiler names the loop of every block in its block comment
  ('=>This Inner Loop Header: Depth=1', 'in Loop: Header=BB0_52 Depth=1'); plus the instructions outside every loop."""
  loops, outside, cur = {}, [], None
  for l in text:
    m = re.match(r'^\.(LBB\d+_\d+):\s*(;.*)?$', l)
    if m or l.startswith('; %bb.'):
      cur = None
      if 'Loop Header' in l and m:
        cur = m.group(1)[1:]                                       # LBB0_52 -> BB0_52
      else:
        h = re.search(r'Header=(BB\d+_\d+)', l)
        if h:
          cur = h.group(1)
      if cur is not None:
        loops.setdefault(cur, [])
      continue
    s = l.strip()
    if s and not s.startswith(';') and not s.startswith('.'):
      (loops[cur] if cur is not None else outside).append(s)
  return loops, outside


@needs_llvm
def test_the_loops_of_the_new_kernel():
  """The step loops are the loops that compute in float64 (the Gumbel scores): four, one per branch.  Two of them — the
  returns-only branches — hold no store and no barrier; the other two hold the per-step stores, non-temporal.  No flat access
  anywhere in the kernel; an LDS and a global look-up of the logits inside the step loops; no scratch, no spill reload in any
  loop."""
  _, text = ki.kernel_text(os.path.join(CSRC, 'tab_sample.hip'), NEW)
  loops, outside = _loops(text)
  everything = outside + [s for body in loops.values() for s in body]
  assert not any(s.startswith('flat_') or s.startswith('scratch_') for s in everything)
  steps = {h: body for h, body in loops.items() if any(re.match(r'v_\w+_f64', s) for s in body)}
  assert len(steps) == 4, sorted(steps)
  is_store = lambda s: re.match(r'(global|flat|scratch|buffer)_store|ds_write|(global|ds)_atomic|ds_add', s)
  returns = [h for h, body in steps.items() if not any(is_store(s) for s in body)]
  record = [h for h in steps if h not in returns]
  assert len(returns) == 2 and len(record) == 2, (returns, record)
  for h, body in steps.items():
    assert not any(s.startswith('s_barrier') for s in body), h
    # both look-ups of the logits, typed: LDS and global, two branches
    assert sum(s.startswith('ds_read') for s in body) >= 2, h
    assert sum(s.startswith('global_load_dword') for s in body) >= 1, h
  for h in record:
    stores = [s for s in steps[h] if s.startswith('global_store')]
    # reward, discount, step_type, the index row, the action: non-temporal.  What else a step stores is the family's own
    # read-modify-write of a float64 bsuite_info column inside its lane advance (deep_sea: :121-123, :140-143; catch: the fold
    # of 127 misses), as in bsx_policy_rollout_kernel: plain 8-byte stores.
    assert sum(s.endswith(' nt') for s in stores) >= 5, (h, stores)
    assert all(s.startswith('global_store_dwordx2 ') for s in stores if not s.endswith(' nt')), stores
    assert not any(re.match(r'ds_write|(global|ds)_atomic|ds_add', s) for s in steps[h]), h
  # what the returns-only branches store, they store after their loops: state word + three columns each
  assert sum(s.startswith('global_store') for s in outside) >= 8
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
