"""CPU: sample_mlp2 / evaluate_sampled_mlp2 (fused closed loops of cartpole, swing-up and mountain_car under a SOFTMAX policy
with two ReLU hidden layers; bsx_<family>_mlp2_sample, bsx_<family>_mlp2_sample_evaluate) without a GPU — the decision the
kernel compiles (bsx_gumbel_select over bsx_mlp2_logits, through gcc) against utils.observations.gumbel_select(mlp2_logits);
every refusal of the two Python entry points with the native entry points replaced by a trap; the C ABI's declarations,
bindings and error codes; and the built library: the one kernel with the drawn mode in it still inside every bound it had,
its loops, and no other kernel changed."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import _native
from bsuite_amd.environments import base, cartpole, catch, mountain_car
from bsuite_amd.utils import observations, wrappers
from tests.test_mlp2_host import _abi_case, _dim, _envs, _random, ki, kr, needs_llvm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bsuite_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
SHIM = os.path.join(ROOT, 'tests', 'csrc', 'mlp2_sample_shim.c')
CALLS = ('sample_mlp2', 'evaluate_sampled_mlp2')
SUFFIX = dict(sample_mlp2='mlp2_sample', evaluate_sampled_mlp2='mlp2_sample_evaluate')
ENTRY = {(fam, c): f'bsx_{fam}_{SUFFIX[c]}' for fam in ('cartpole', 'mountain_car') for c in CALLS}
DIMS = [3, 6, 8]
WIDTHS = [(1, 1), (33, 7), (7, 17), (64, 64)]
TEMPERATURES = [0.25, 1.0, 4.0]
_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------ the decision, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('mlp2_sample') / 'mlp2_sample_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC', SHIM, '-o', so])
  lib = ctypes.CDLL(so)
  P = ctypes.c_void_p
  lib.shim_mlp2_sample.restype = None
  lib.shim_mlp2_sample.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P, P, P, P, P, P, P]
  lib.shim_stream_sample.restype = ctypes.c_uint32
  return lib


def _shim_run(lib, w1, w2, w3, o, words, beta):
  """(action [n], logits [n, 3]) of n cases, each with its own triple, words and beta."""
  w1, w2, w3, o = (np.ascontiguousarray(x, np.float32) for x in (w1, w2, w3, o))
  words = np.ascontiguousarray(words, np.uint32)
  n, H1, D1 = w1.shape
  H2 = w2.shape[1]
  beta = np.ascontiguousarray(np.broadcast_to(beta, (n,)), np.float64)
  assert w2.shape == (n, H2, H1 + 1) and w3.shape == (n, 3, H2 + 1) and o.shape == (n, D1 - 1) and words.shape == (n, 3)
  action, logits = np.full(n, -1, np.int32), np.full((n, 3), 7.0, np.float32)
  lib.shim_mlp2_sample(n, D1 - 1, H1, H2, _ptr(w1), _ptr(w2), _ptr(w3), _ptr(o), _ptr(words), _ptr(beta), _ptr(action), _ptr(logits))
  return action, logits


def _bits(x):
  return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _torch_rule(w1, w2, w3, o, words, temperature):
  t = [torch.from_numpy(np.ascontiguousarray(x, np.float32)) for x in (w1, w2, w3, o)]
  logits = observations.mlp2_logits(*t)
  return observations.gumbel_select(logits, np.ascontiguousarray(words, np.uint32), temperature).numpy(), logits.numpy()


def _words(rng, n):
  w = rng.integers(0, 1 << 32, size=(n, 3), dtype=np.uint64).astype(np.uint32)
  w[0], w[1], w[2] = 0, 0xFFFFFFFF, (0, 0xFFFFFFFF, 0x80000000)          # the ends of the range of a word
  return w


def test_the_shim_compiles_the_kernels_headers(shim):
  assert shim.shim_stream_sample() == 3
  text = open(SHIM).read()
  assert '#include "../../bsuite_amd/csrc/bsx_mlp2.h"' in text and '#include "../../bsuite_amd/csrc/bsx_gumbel.h"' in text
  assert 'bsx_gumbel_select(' in text and 'bsx_mlp2_logits(' in text
  torso = open(os.path.join(CSRC, 'bsx_torso.h')).read()
  assert '#include "bsx_mlp2.h"' in torso and '#include "bsx_gumbel.h"' in torso
  for header in ('bsx_mlp2.h', 'bsx_gumbel.h'):                            # plain C: what gcc compiles is what the kernel compiles
    assert '__device__' not in open(os.path.join(CSRC, header)).read(), header


@pytest.mark.parametrize('temperature', TEMPERATURES)
@pytest.mark.parametrize('H1,H2', WIDTHS)
@pytest.mark.parametrize('D', DIMS)
def test_random_triples_against_the_torch_rule(shim, D, H1, H2, temperature):
  rng = np.random.default_rng(1000 * D + 10 * H1 + H2 + int(8 * temperature))
  n = 192
  w1, w2, w3, o = _random(rng, n, D, H1, H2)
  words = _words(rng, n)
  action, logits = _shim_run(shim, w1, w2, w3, o, words, 1.0 / temperature)
  want, want_logits = _torch_rule(w1, w2, w3, o, words, temperature)
  np.testing.assert_array_equal(_bits(logits), _bits(want_logits))
  np.testing.assert_array_equal(action, want)
  assert set(action.tolist()) == {0, 1, 2}
  # it samples: the draw is not the greedy action everywhere (the logits of a random triple lie close together)
  greedy = observations.mlp2_select(*[torch.from_numpy(x) for x in (w1, w2, w3, o)]).numpy()
  assert (action != greedy).mean() >= 0.05, (action != greedy).mean()
  # one shared triple: 2-D tensors in torch, the same triple in every case of the shim
  k = 7
  shared = [np.broadcast_to(x[k], x.shape) for x in (w1, w2, w3)]
  s_action, s_logits = _shim_run(shim, *shared, o, words, 1.0 / temperature)
  t = [torch.from_numpy(x[k].copy()) for x in (w1, w2, w3)]
  t_logits = observations.mlp2_logits(*t, torch.from_numpy(o))
  np.testing.assert_array_equal(_bits(t_logits.numpy()), _bits(s_logits))
  np.testing.assert_array_equal(observations.gumbel_select(t_logits, words, temperature).numpy(), s_action)


@pytest.mark.parametrize('temperature', TEMPERATURES)
@pytest.mark.parametrize('H1,H2', WIDTHS)
@pytest.mark.parametrize('D', DIMS)
def test_special_weights_and_logits(shim, D, H1, H2, temperature):
  """NaN, +inf, -inf and -0.0 weights, one place each — the places of tests/test_gpu_mlp2.py's _triple(special=True) — and
  logits of -inf (the action is masked: never drawn), NaN (never wins; at action 0 never beaten) and +inf."""
  rng = np.random.default_rng(7 * D + H1 + 100 * H2 + int(8 * temperature))
  reps = 16
  cases, tags = [], []

  def add(tag, edit):
    for _ in range(reps):
      w1, w2, w3, o = (x[0] for x in _random(rng, 1, D, H1, H2))
      edit(w1, w2, w3)
      cases.append((w1, w2, w3, o)); tags.append(tag)

  def setter(which, idx, v):
    def edit(w1, w2, w3):
      (w1, w2, w3)[which][idx] = v
    return edit
  nan, inf = float('nan'), float('inf')
  add('nan bias 1', setter(0, (-1, D), nan))
  add('nan bias 2', setter(1, (-1, H1), nan))
  add('inf weight 2', setter(1, (0, 0), inf))
  add('-inf bias 1', setter(0, (0, D), -inf))
  add('-inf weight 3', setter(2, (1, 0), -inf))
  add('-0.0 bias 3', setter(2, (0, H2), -0.0))
  add('-0.0 bias 2', setter(1, (0, H1), -0.0))
  for a in range(3):
    add(('-inf logit', a), setter(2, (a, H2), -inf))
    add(('nan logit', a), setter(2, (a, H2), nan))
    add(('+inf logit', a), setter(2, (a, H2), inf))
  stack = [np.stack([c[k] for c in cases]) for k in range(4)]
  words = _words(rng, len(cases))
  action, logits = _shim_run(shim, *stack, words, 1.0 / temperature)
  want, want_logits = _torch_rule(*stack, words, temperature)
  np.testing.assert_array_equal(_bits(logits), _bits(want_logits))
  np.testing.assert_array_equal(action, want)
  assert np.isnan(logits).any() and np.isposinf(logits).any() and np.isneginf(logits).any()
  for i, tag in enumerate(tags):
    if not isinstance(tag, tuple):
      continue
    kind, a = tag
    row = logits[i]
    if kind == '-inf logit':
      assert np.isneginf(row[a]) and action[i] != a, (tag, row, action[i])       # masked (the other two are finite)
    elif kind == 'nan logit':
      assert np.isnan(row[a]) and (action[i] == 0 if a == 0 else action[i] != a), (tag, row, action[i])
    else:
      assert np.isposinf(row[a]) and action[i] == a, (tag, row, action[i])


def test_the_shim_runs_stand_alone_under_the_sanitizers(tmp_path):
  san = ['gcc', '-O1', '-g', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all']
  probe = tmp_path / 'probe.c'
  probe.write_text('int main(void) { return 0; }\n')
  if subprocess.run(san + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode != 0:
    pytest.skip('this gcc has no sanitizer runtime')
  exe = str(tmp_path / 'mlp2_sample_shim_main')
  # (the sanitizers are there: a failure to compile the shim itself is a failure)
  subprocess.check_call(san + ['-DMLP2_SAMPLE_SHIM_MAIN', SHIM, '-o', exe])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0 and len(r.stdout.split()) == 3 and set(r.stdout.split()) <= {'0', '1', '2'}, (r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------ the Python entry points
@pytest.fixture
def trap(monkeypatch):
  """Every native entry point of the two calls replaced by a trap: a refusal that came too late would fall into it."""
  hits = []

  class Lib:
    def __getattr__(self, name):
      if name in ENTRY.values():
        hits.append(name)
        raise AssertionError(f'{name} was reached')
      return getattr(_native.lib, name)
  monkeypatch.setattr(base._native, 'lib', Lib())                          # pylint: disable=protected-access
  yield hits
  assert not hits


def _refused(env, name, exc=ValueError, match=None, **kw):
  """env.<name>(...) raises, its message names the caller, and nothing was allocated."""
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  H1, H2 = 5, 4
  obs = kw.pop('observation') if 'observation' in kw else torch.zeros((4, 3), dtype=torch.float32)
  pol = (kw.pop('w1') if 'w1' in kw else torch.zeros((H1, 4), dtype=torch.float32),
         kw.pop('w2') if 'w2' in kw else torch.zeros((H2, H1 + 1), dtype=torch.float32),
         kw.pop('w3') if 'w3' in kw else torch.zeros((3, H2 + 1), dtype=torch.float32))
  with pytest.raises(exc, match=match or name) as info:
    getattr(env, name)(*pol, obs, kw.pop('num_steps', 4), **kw)
  assert name in str(info.value)
  assert not raw._allocated and not raw._policy_rollout_out and raw._linear_eval_out is None      # pylint: disable=protected-access


def _native_arguments(env, name, *args, **kw):
  """What env.<name>(...) hands to the library — (entry point, arguments, T) — with the allocation and the launch replaced on
  this instance and its columns on the CPU."""
  seen = []
  env._device = torch.device('cpu')
  env._ensure_allocated = lambda: None
  env._call_desc = _native.Call()
  env._state = dict(state=torch.zeros((4, 4)), steps=torch.zeros(4, dtype=torch.int32))
  env._info = torch.zeros((1, 4), dtype=torch.float64)
  env._launch_steps = lambda fn, a, T, what: seen.append((fn.__name__, a, T, what))
  out = getattr(env, name)(*args, **kw)
  (entry, a, T, what), = seen
  assert what == name
  return entry, a, T, out


def test_signatures_docstrings_and_families():
  want = ['self', 'w1', 'w2', 'w3', 'observation', 'num_steps', 'policy_index', 'temperature', 'sample_seed']
  for name, sibling, greedy in (('sample_mlp2', 'sample_mlp', 'rollout_mlp2'), ('evaluate_sampled_mlp2', 'evaluate_sampled_mlp', 'evaluate_mlp2')):
    fn = getattr(base.Environment, name)
    p = inspect.signature(fn).parameters
    assert list(p) == want
    old = inspect.signature(getattr(base.Environment, sibling)).parameters
    assert [k for k in p if k != 'w3'] == list(old) and all(p[k] == old[k] for k in old)            # the sibling's, with w3
    assert [p[k].kind for k in ('policy_index', 'temperature', 'sample_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
    assert p['temperature'].default == 1.0 and p['sample_seed'].default == 0 and p['policy_index'].default is None
    for word in ('gumbel_select(mlp2_logits(w1[row], w2[row], w3[row], obs), words(sample_seed, lane, call index), temperature)',
                 'torch.cat([lin.weight, lin.bias[:, None]], 1)', 'torch.nn.Linear', 'policy_index', '1 <= H1, H2 <= 64', sibling,
                 'a = 0 where the lane resets on this call'):
      assert word in fn.__doc__, (name, word)
    abi = lambda cls: cls._closed_loop_abi(object.__new__(cls), name)      # pylint: disable=protected-access,cell-var-from-loop
    assert abi(cartpole.Cartpole) == abi(cartpole.CartpoleSwingup) == ENTRY['cartpole', name]
    assert abi(mountain_car.MountainCar) == ENTRY['mountain_car', name] and ENTRY['cartpole', name] in _native.EXPORTED
    assert abi(base.Environment) is None and abi(catch.Catch) is None and ENTRY['mountain_car', name] in _native.EXPORTED
    assert 'epsilon' not in inspect.signature(fn).parameters
    for env in _envs():
      # the refusals are the greedy call's, then the temperature and the seed — two faults at a time, the earlier one's message
      # — and the last of them allocates nothing
      D = _dim(env)
      env._device = torch.device('cpu')
      good = dict(w1=torch.zeros((5, D + 1)), w2=torch.zeros((4, 6)), w3=torch.zeros((3, 5)), observation=torch.zeros((4, D)))
      _refused(env, name, match='w3 must be', temperature=0.0, **dict(good, w3=None))
      _refused(env, name, match='temperature must be', temperature=0.0, sample_seed=-1, **good)
      _refused(env, name, match='sample_seed must be', sample_seed=-1, **good)
      # what reaches the library: the triple in one bsx_mlp2_t with epsilon 0.0 and the SAMPLE seed in its explore_seed field,
      # 1 / temperature after it, the two state columns, the outputs — the recording call's with the action column — and info
      entry, a, T, out = _native_arguments(env, name, *good.values(), 7, temperature=4.0, sample_seed=(1 << 64) - 3)
      pol = a[2]._obj                                                      # pylint: disable=protected-access
      assert entry == ENTRY['mountain_car' if D == 3 else 'cartpole', name] and T == 7 and isinstance(pol, _native.Mlp2)
      assert (pol.w1, pol.w2, pol.w3, pol.observation_in) == tuple(t.data_ptr() for t in good.values())
      assert (pol.hidden1, pol.hidden2, pol.n_policies, pol.policy_index, pol.epsilon, pol.explore_seed) == (5, 4, 1, None, 0.0, (1 << 64) - 3)
      assert a[3] == 0.25 and a[4:6] == tuple(t.data_ptr() for t in env._state.values()) and a[-1] == env._info.data_ptr()
      if name == 'sample_mlp2':                                            # the [T,B] buffers of the rollout_* calls, + the actions
        ts, actions = out
        assert len(a) == 9 and isinstance(a[6], _native.TimeStepPtrs) and a[6].reward == ts.reward.data_ptr() and a[7] == actions.data_ptr()
        assert env._policy_rollout_out[7][2] is ts and env._policy_rollout_out[7][3] is actions and env._linear_eval_out is None
      else:                                                                # evaluate_linear's result columns; no [T,B] buffer
        assert len(a) == 8 and isinstance(a[6], _native.LinearEvalPtrs) and out is env._linear_eval_out and not env._policy_rollout_out
        assert (a[6].episodes, a[6].return_sum, a[6].episode_return_sum, a[6].observation_out) == tuple(t.data_ptr() for t in out)
  for word in ('-inf logit masks', 'NaN score never wins', 'never reads its row'):
    assert word in base.Environment.sample_mlp2.__doc__, word
  assert 'invalid_action_count()' in base.Environment.evaluate_sampled_mlp2.__doc__


@pytest.mark.parametrize('name', CALLS)
def test_views_families_and_modes_are_refused(name, trap):
  for env in (cartpole.Cartpole(seed=0), cartpole.CartpoleSwingup(seed=0), mountain_car.MountainCar(seed=0)):
    _refused(env, name, match='batched view')
  for bsuite_id in ('bandit/0', 'deep_sea/0', 'catch/0', 'memory_len/0', 'umbrella_length/0', 'discounting_chain/0'):
    _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), name, match='mountain_car only')
  for cls in (cartpole.Cartpole, cartpole.CartpoleSwingup, mountain_car.MountainCar):
    _refused(cls(seed=0, batch=4, rng='mt19937'), name, match='philox')
  for env in _envs():
    env._logging = dict(steps=None)             # what enable_logging() leaves behind (it allocates: not without a GPU)
    _refused(env, name, match='Logging')
  for env in _envs():
    env._grouped_by = object()                  # what SweepBatch sets while its prepared groups hold the column pointers
    _refused(env, name, exc=RuntimeError, match='release_groups')


def test_a_slab_of_4_gib_is_refused_by_the_recording_call_alone(trap):
  for env in _envs():
    D = _dim(env)
    env._device = torch.device('cpu')
    env._batch = -(-(1 << 32) // (4 * D))                                  # the first batch whose [B, D] slab reaches 4 GiB
    with pytest.raises(ValueError, match='sample_mlp2: .* 4 GiB'):
      env._check_trajectory_slab('sample_mlp2')                            # pylint: disable=protected-access
    # the whole method: the slab is the last refusal, after the arguments' and the temperature's, before anything is allocated
    w1, w2, w3 = torch.zeros((5, D + 1)), torch.zeros((4, 6)), torch.zeros((3, 5))
    big = torch.zeros((1, D)).expand(env._batch, D)                        # (not contiguous: refused first, as an argument)
    with pytest.raises(ValueError, match='sample_mlp2: observation must be'):
      env.sample_mlp2(w1, w2, w3, big, 4)
    real = big
    env._check_fused_eval_rows = lambda what, observation, P, *a: P        # (a contiguous [B, D] tensor of 4 GiB is not made for this)
    with pytest.raises(ValueError, match='sample_mlp2: temperature'):
      env.sample_mlp2(w1, w2, w3, real, 4, temperature=0.0)                # the temperature before the slab
    with pytest.raises(ValueError, match='sample_mlp2: .* 4 GiB'):
      env.sample_mlp2(w1, w2, w3, real, 4)
    with pytest.raises(ValueError, match='evaluate_sampled_mlp2: temperature'):
      env.evaluate_sampled_mlp2(w1, w2, w3, real, 4, temperature=0.0)
    del env._check_fused_eval_rows
    env._batch -= 1
    env._check_trajectory_slab('sample_mlp2')                              # pylint: disable=protected-access
    assert not env._allocated                                              # pylint: disable=protected-access
  for env in _envs():                                                      # returns only: no slab is written, none is refused —
    D = _dim(env)                                                          # the call goes on to allocate (never on 'meta')
    env._device = torch.device('meta')
    env._batch = -(-(1 << 32) // (4 * D))
    w = [torch.zeros(shape, device='meta') for shape in ((5, D + 1), (4, 6), (3, 5), (env._batch, D))]
    with pytest.raises(RuntimeError, match='no HIP device'):
      env.evaluate_sampled_mlp2(*w, 4)
    with pytest.raises(ValueError, match='sample_mlp2: .* 4 GiB'):
      env.sample_mlp2(*w, 4)
    assert not env._allocated and env._linear_eval_out is None             # pylint: disable=protected-access


@pytest.mark.parametrize('name', CALLS)
def test_the_wrappers_refuse_instead_of_delegating(name, trap):
  for make in (lambda e: wrappers.RewardNoise(e, noise_scale=0.5, seed=1), lambda e: wrappers.RewardScale(e, reward_scale=2.0)):
    for raw in _envs():
      _refused(make(raw), name, match='not available through')
      _refused(raw, name, match='reward wrapper')                         # ... and the raw environment knows it is wrapped
  for bsuite_id in ('cartpole_noise/2', 'cartpole_scale/4', 'mountain_car_noise/3', 'mountain_car_scale/1'):
    env = bsuite_amd.load_from_id(bsuite_id, batch=4)
    assert hasattr(env, 'raw_env'), bsuite_id
    _refused(env, name, match='not available through')
  for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    fn = getattr(cls, name)
    assert fn is not getattr(base.Environment, name) and any(name in vars(c) for c in cls.__mro__[:-1]), cls
    with pytest.raises(ValueError, match=name):
      fn(object.__new__(cls), torch.zeros((5, 4)), torch.zeros((4, 6)), torch.zeros((3, 5)), torch.zeros((4, 3)), 4)
  image = wrappers.ImageObservation(mountain_car.MountainCar(seed=0, batch=4), (84, 84, 1))
  _refused(image, name, match='not available through ImageObservation')


@pytest.mark.parametrize('name', CALLS)
def test_arguments_are_checked_before_any_gpu_use(name, trap):
  sibling = dict(sample_mlp2='sample_mlp', evaluate_sampled_mlp2='evaluate_sampled_mlp')[name]
  for env in _envs():
    env._device = torch.device('cpu')           # the checks themselves, on host tensors: dtype, shape, contiguity
    D, H1, H2 = _dim(env), 5, 4
    w1, w2, w3 = torch.zeros((H1, D + 1)), torch.zeros((H2, H1 + 1)), torch.zeros((3, H2 + 1))
    p1, p2, p3 = torch.zeros((4, H1, D + 1)), torch.zeros((4, H2, H1 + 1)), torch.zeros((4, 3, H2 + 1))
    obs = torch.zeros((4, 1, D), dtype=torch.float32)
    idx = torch.zeros(4, dtype=torch.int32)
    ok, pop = dict(w1=w1, w2=w2, w3=w3), dict(w1=p1, w2=p2, w3=p3)
    # the temperature and the seed: sample_mlp's refusals in sample_mlp's words
    for t in (0.0, -1.0, -0.0, float('nan'), float('inf'), float('-inf'), 5e-324, 1e-310, '1.0', None, True, [1.0]):
      _refused(env, name, temperature=t, observation=obs, match=f'{name}: temperature', **ok)
      with pytest.raises(ValueError) as mine:
        getattr(env, name)(w1, w2, w3, obs, 4, temperature=t)
      with pytest.raises(ValueError) as theirs:
        getattr(env, sibling)(w1, torch.zeros((3, H1 + 1)), obs, 4, temperature=t)
      assert str(mine.value) == str(theirs.value).replace(sibling, name), t
    for seed in (-1, 1 << 64, 0.5, None, True, '3'):
      _refused(env, name, sample_seed=seed, observation=obs, match=f'{name}: sample_seed', **ok)
      with pytest.raises(ValueError) as mine:
        getattr(env, name)(w1, w2, w3, obs, 4, sample_seed=seed)
      with pytest.raises(ValueError) as theirs:
        getattr(env, sibling)(w1, torch.zeros((3, H1 + 1)), obs, 4, sample_seed=seed)
      assert str(mine.value) == str(theirs.value).replace(sibling, name), seed
    for word in ('epsilon', 'explore_seed'):                               # there is no epsilon: the softmax explores
      with pytest.raises(TypeError, match=word):
        getattr(env, name)(w1, w2, w3, obs, 4, **{word: 0})
    for n in (0, -1, 2.0, None, '4', True):
      _refused(env, name, num_steps=n, observation=obs, match=f'{name}: num_steps', **ok)
    for bad in (obs.to(torch.float64), obs.numpy(), torch.zeros((4, D + 1)), torch.zeros((3, 1, D)), torch.zeros(4 * D),
                torch.zeros((4, 2 * D))[:, ::2], None):
      _refused(env, name, observation=bad, match=f'{name}: observation must be', **ok)
    _refused(env, name, observation=torch.zeros((4, D)), policy_index=idx, match='must be None', **ok)      # policy_index with one triple
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, name, observation=obs, policy_index=bad, match='policy_index', **pop)
    # a wrong H, dtype, contiguity or rank in any of the three matrices: rollout_mlp2's refusals
    for bad in (w1.to(torch.float64), w1.numpy(), torch.zeros((H1, D)), torch.zeros((0, D + 1)), torch.zeros((65, D + 1)),
                torch.zeros((H1, 2 * (D + 1)))[:, ::2], torch.zeros((H1 * (D + 1),)), None):
      _refused(env, name, w1=bad, w2=w2, w3=w3, observation=obs, match=f'{name}: w1 must be')
    for bad in (w2.to(torch.float64), w2.numpy(), torch.zeros((H2, H1)), torch.zeros((H2, H1 + 2)), torch.zeros((0, H1 + 1)),
                torch.zeros((65, H1 + 1)), torch.zeros((H2, 2 * (H1 + 1)))[:, ::2], torch.zeros((1, H2, H1 + 1)), None):
      _refused(env, name, w1=w1, w2=bad, w3=w3, observation=obs, match=f'{name}: w2 must be')
    for bad in (w3.to(torch.float64), w3.numpy(), torch.zeros((3, H2)), torch.zeros((3, H2 + 2)), torch.zeros((2, H2 + 1)),
                torch.zeros((3, 2 * (H2 + 1)))[:, ::2], torch.zeros((1, 3, H2 + 1)), None):
      _refused(env, name, w1=w1, w2=w2, w3=bad, observation=obs, match=f'{name}: w3 must be')
    _refused(env, name, w1=p1, w2=w2, w3=p3, observation=obs, policy_index=idx, match=f'{name}: w2 must be')
    _refused(env, name, w1=p1, w2=p2, w3=torch.zeros((5, 3, H2 + 1)), observation=obs, policy_index=idx, match=f'{name}: w3 must be')
    # the matrices are looked at before the temperature
    _refused(env, name, w1=None, w2=w2, w3=w3, observation=obs, temperature=0.0, match=f'{name}: w1 must be')
    assert not env._allocated                                              # pylint: disable=protected-access
  # host tensors for an environment on the GPU: the device
  env = mountain_car.MountainCar(seed=0, batch=4)
  _refused(env, name, observation=torch.zeros((4, 1, 3)), match='w1 must be')


# ------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_export_agree_and_the_abi_stays_v12():
  header = open(HEADER).read()
  assert re.search(r'#define BSX_ABI_VERSION 12\b', header)
  assert _native.ABI_VERSION == 12 and _native.lib.bsx_abi_version() == 12
  plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  out = subprocess.check_output(['nm', '-D', '--defined-only', _native.SO_PATH], text=True)
  P = ctypes.c_void_p
  text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for (fam, name), entry in ENTRY.items():
    decl = re.search(r'int ' + entry + r'\(([^;]*)\);', plain)
    assert decl, f'include/bsuite_amd.h does not declare {entry}'
    types = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(decl.group(1).split()).split(',')]
    tail = ['bsx_linear_eval_t', 'double*'] if name == 'evaluate_sampled_mlp2' else ['bsx_timestep_t', 'int32_t*', 'double*']
    assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_mlp2_t*', 'double', 'float*', 'int32_t*'] + tail
    # ... which is the one-hidden-layer sampled call's list with the other struct
    old = re.search(r'int ' + entry.replace('mlp2', 'mlp') + r'\(([^;]*)\);', plain)
    old_types = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(old.group(1).split()).split(',')]
    assert [t.replace('bsx_mlp_t', 'bsx_mlp2_t') for t in old_types] == types
    assert entry in _native.EXPORTED
    fn = getattr(_native.lib, entry)
    cfg = dict(cartpole=_native.CartpoleCfg, mountain_car=_native.MountainCarCfg)[fam]
    outs = [_native.LinearEvalPtrs, P] if name == 'evaluate_sampled_mlp2' else [_native.TimeStepPtrs, P, P]
    assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.Mlp2), ctypes.c_double, P, P] + outs
    assert fn.restype is ctypes.c_int
    assert any(l.split()[-1] == entry and ' T ' in l for l in out.splitlines())
    assert 'extern "C" int ' + entry + '(' in open(os.path.join(CSRC, fam + '.hip')).read()
    assert entry in text, f'INTEGRATION.md does not describe {entry}'
  # the header documents the section; the struct is the greedy calls', untouched
  note = header[header.index('two hidden layers, sampled'):header.index('int bsx_cartpole_mlp2_sample(')]
  for word in ('BSX_STREAM_SAMPLE', 'SAMPLE SEED', 'csrc/bsx_gumbel.h', 'csrc/bsx_mlp2.h', 'BSX_ERANGE', 'inv_temperature is not a finite number > 0',
               'before an empty call returns', 'draws nothing', '4 GiB'):
    assert word in note, word
  assert ctypes.sizeof(_native.Mlp2) == 72 and ctypes.sizeof(_native.Mlp) == 56 and ctypes.sizeof(_native.Linear) == 48
  assert _native.MISSING == []


@pytest.mark.parametrize('name', CALLS)
@pytest.mark.parametrize('fam', ['cartpole', 'mountain_car'])
def test_argument_checks_of_the_entry_points(fam, name):
  """Every refusal comes before any device work: garbage stands in for device pointers, none is dereferenced.  The codes and
  their order are those of bsx_<family>_mlp2_rollout / _mlp2_evaluate; a non-zero epsilon and a bad inv_temperature are
  BSX_ERANGE where an epsilon outside [0, 1] is there: after the modes and the scalars (the widths included), before an empty
  call returns, before the pointers."""
  fn = getattr(_native.lib, ENTRY[fam, name])
  cfg, bad_cfg = _abi_case(fam)
  junk = 0xDEAD0010                                                # never mapped: a dereference would fault (16-byte aligned)
  E = _native
  D = 3 if fam == 'mountain_car' else 6
  record = name == 'sample_mlp2'
  nan, inf = float('nan'), float('inf')

  def call(**kw):
    c = _native.Call(n_lanes=kw.pop('n_lanes', 4), n_steps=kw.pop('n_steps', 4), flags=kw.pop('flags', 0))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def policy(**kw):
    d = dict(w1=junk, w2=junk, w3=junk, hidden1=5, hidden2=4, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0,
             observation_in=junk)
    d.update(kw)
    return _native.Mlp2(**d)

  def run(c, q, beta=1.0, state=junk, steps=junk, out=None, actions=junk, info=junk, cfg_=cfg):
    if record:
      out = (_native.TimeStepPtrs(junk, junk, junk, junk) if out is None else out, actions)
    else:
      out = (_native.LinearEvalPtrs(junk, junk, junk, junk) if out is None else out,)
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, beta, state, steps, *out, info)

  bad_betas = (0.0, -0.0, -1.0, nan, inf, -inf)
  # null structs
  assert run(call(), policy(), cfg_=None) == E.BSX_ENULL
  assert run(None, policy()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: before the scalars — and before a bad temperature
  for flags in (E.CALL_OBS_INDEX, E.CALL_OBS_U8, E.CALL_OBS_F16, E.CALL_OBS_BF16, E.CALL_OBS_INDEX | E.CALL_OBS_U8):
    assert run(call(flags=flags), policy(n_policies=-1, hidden1=0)) == E.BSX_EMODE, flags
    assert run(call(flags=flags), policy(), beta=nan) == E.BSX_EMODE, flags
  lg = _native.Logging()
  assert run(call(logging=ctypes.pointer(lg)), policy(hidden2=99)) == E.BSX_EMODE
  for wrap in (E.WRAP_SCALE, E.WRAP_NOISE, E.WRAP_SCALE_NOISE, E.WRAP_NOISE_SCALE):
    c = call()
    c.wrap.kind = wrap
    assert run(c, policy()) == E.BSX_EMODE, wrap
  c = call()
  c.stream.mt_state, c.stream.mt_pos = junk, junk
  assert run(c, policy()) == E.BSX_EMODE
  for member in ('reward_f64', 'obs_paint', 'state_alt'):
    assert run(call(**{member: junk}), policy()) == E.BSX_EMODE, member
  assert run(call(force_reset=1), policy(), beta=0.0) == E.BSX_EMODE
  assert run(call(action_ring=4), policy(epsilon=0.5)) == E.BSX_EMODE
  # BSX_EINVAL: the scalars, the widths among them, before the temperature and the epsilon
  for n in (0, -1):
    assert run(call(n_steps=n), policy()) == E.BSX_EINVAL
    assert run(call(n_steps=n), policy(), beta=-1.0) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), policy(), beta=inf) == E.BSX_EINVAL
  for which in ('hidden1', 'hidden2'):
    for h in (0, -1, 65, 1 << 20):
      assert run(call(), policy(**{which: h})) == E.BSX_EINVAL, (which, h)
      assert run(call(), policy(**{which: h}), beta=nan) == E.BSX_EINVAL, (which, h)
      assert run(call(), policy(**{which: h}, epsilon=0.5)) == E.BSX_EINVAL, (which, h)
      assert run(call(n_lanes=0), policy(**{which: h})) == E.BSX_EINVAL, (which, h)
    for h in (1, 64):
      assert run(call(n_lanes=0), policy(**{which: h})) == 0
  for n in (0, -3):
    assert run(call(), policy(n_policies=n)) == E.BSX_EINVAL
    assert run(call(), policy(n_policies=n, epsilon=0.5), beta=0.0) == E.BSX_EINVAL
  # BSX_ERANGE: epsilon must be 0.0 — also one that an epsilon-greedy call accepts — and inv_temperature finite and > 0
  for eps in (0.3, 1.0, 5e-324, -1e-9, 1.0000001, nan, inf):
    assert run(call(), policy(epsilon=eps)) == E.BSX_ERANGE, eps
  assert run(call(n_lanes=0), policy(epsilon=-0.0)) == 0                                    # (-0.0 == 0.0)
  none = {k: None for k in ('w1', 'w2', 'w3', 'observation_in')}
  for b in bad_betas:
    assert run(call(), policy(), beta=b) == E.BSX_ERANGE, b
    assert run(call(n_lanes=0), policy(), beta=b) == E.BSX_ERANGE, b                        # an empty call still checks its scalars
    assert run(call(), policy(**none), beta=b, state=None) == E.BSX_ERANGE, b               # ... before any pointer is looked at
  assert run(call(), policy(), cfg_=bad_cfg) == E.BSX_ERANGE
  assert run(call(flags=E.CALL_OBS_INDEX), policy(), cfg_=bad_cfg) == E.BSX_ERANGE          # (the cfg comes first)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at; the extreme temperatures are accepted
  empty = _native.TimeStepPtrs(0, 0, 0, 0) if record else _native.LinearEvalPtrs(0, 0, 0, 0)
  for b in (1.0, 5e-324, 1.7976931348623157e308):
    assert run(call(n_lanes=0), policy(**none), beta=b, state=None, steps=None, out=empty, actions=None, info=None) == 0, b
  assert run(call(n_lanes=0), policy(epsilon=0.3)) == E.BSX_ERANGE
  # BSX_ENULL: every pointer — the other ones garbage; w3 is one more required pointer
  for missing in none:
    assert run(call(), policy(**{missing: None})) == E.BSX_ENULL, missing
  for missing in ('state', 'steps', 'info'):
    assert run(call(), policy(), **{missing: None}) == E.BSX_ENULL, missing
  for k in range(4):                                                                        # every output pointer
    ptrs = [junk] * 4
    ptrs[k] = 0
    assert run(call(), policy(), out=(_native.TimeStepPtrs if record else _native.LinearEvalPtrs)(*ptrs)) == E.BSX_ENULL, k
  if record:
    assert run(call(), policy(), actions=None) == E.BSX_ENULL
  assert run(call(), policy(n_policies=2)) == E.BSX_ENULL                                   # a population without policy_index
  if fam == 'cartpole':
    no_table = _abi_case(fam)[0]
    no_table.time_frac = None
    assert run(call(), policy(), cfg_=no_table) == E.BSX_ENULL
  assert run(call(n_lanes=1 << 40), policy()) == E.BSX_EINVAL                               # more workgroups than a grid holds
  assert run(call(action_ring=-2), policy()) == E.BSX_EINVAL
  slab = -(-(1 << 32) // (4 * D))
  if record:
    # what only a call that writes [T,B] slabs refuses: a slab the 32-bit lane offsets cannot span
    assert run(call(n_lanes=slab), policy()) == E.BSX_EINVAL
    assert run(call(n_lanes=1 << 31), policy()) == E.BSX_EINVAL


# ------------------------------------------------------------------------------------------ the source text
def test_the_kernel_body_draws_through_the_headers():
  dev = open(os.path.join(CSRC, 'bsx_torso.h')).read()
  assert '#define BSX_TORSO_GREEDY 0' in dev and '#define BSX_TORSO_DRAWN 1' in dev
  args = dev[dev.index('struct bsx_torso_args {'):]
  args = args[:args.index('};')]
  assert 'int32_t mode;' in args and 'double beta;' in args
  body = dev[dev.index('void bsx_torso_body('):]
  body = body[:body.index('\n}\n')]
  loop = body[body.index('for (int t = 0; t < n_steps; ++t) {'):]
  loop = loop[:loop.index('\n    }\n')]
  for call_ in ('bsx_gumbel_draws(p.explore_seed, lane, step)', 'bsx_gumbel_select(l, kt.beta, u.v[0], u.v[1], u.v[2])', 'if (!resets)',
                'bsx_policy_draws(p.explore_seed, lane, step)', 'bsx_policy_select('):
    assert call_ in loop, call_
  # the decision comes after the walk and before the step; the logits are the walk's own
  assert loop.rindex('bsx_torso_action_of<D>(') < loop.index('bsx_gumbel_draws(') < loop.index('Env::template core<')
  walk = dev[dev.index('int32_t bsx_torso_action('):]
  walk = walk[:walk.index('\n}\n')]
  assert 'float* keep = nullptr)' in walk.split('\n')[0] and 'return bsx_mlp_argmax(l);' in walk
  assert 'if constexpr (KEEP)' in walk and 'keep[a] = l[a]' in walk      # the walk's own logits, copied out for the drawn mode alone
  assert 'bsx_torso_action_of<D, true>(tab, W, H1, H2, o, l)' in loop and 'bsx_torso_action_of<D>(tab, W, H1, H2, o)' in loop
  for word in ('bsx_log', 'double', 'gumbel'):
    assert word not in walk, word                                          # no float64 inside the walk
  # the mode is a compile-time parameter, trailing and defaulted: the greedy instantiations are spelled as they were
  assert 'template <class Fam, int V, bool SHARED, bool RECORD, bool DRAWN = false>' in dev and 'if constexpr (DRAWN)' in loop
  hip = open(os.path.join(CSRC, 'torso.hip')).read()
  for inst in ('true, true', 'false, true', 'true, false', 'false, false'):
    assert f'bsx_torso_body<Fam, V, {inst}>' in hip and f'bsx_torso_body<Fam, V, {inst}, true>' in hip, inst
  assert 'a.mode == BSX_TORSO_DRAWN' in hip and hip.count('__global__') == 1
  # bsx_log's constants stay on the scalar unit (BSX_K), as for bsx_gumbel_kernel
  stream_h = open(os.path.join(ROOT, 'include', 'bsx_stream.h')).read()
  assert '#define BSX_K(c) bsx_k_(c)' in stream_h
  # the entry points: the sampled check, then the greedy path's
  # (bsx_torso_entry, stated once for both families in bsx_torso.h; the family's file delegates to it, twice in the drawn mode)
  assert 'bsx_check_mlp2_sample_call(call, mlp2, inv_temperature,' in dev[dev.index('static inline int bsx_torso_entry('):]
  for fam in ('cartpole', 'mountain_car'):
    text = open(os.path.join(CSRC, fam + '.hip')).read()
    assert text.count(f'bsx_torso_entry<{fam}_host>(cfg, call, mlp2, BSX_TORSO_DRAWN, inv_temperature') == 2


# ------------------------------------------------------------------------------------------ the built library
NEW = 'bsx_torso_kernel'
BEFORE = os.path.join(ROOT, 'profiles', 'mlp2_sample', 'kernel_resources_parent.json')


@needs_llvm
def test_the_one_kernel_keeps_its_bounds_with_the_drawn_mode_in_it():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  assert [n for n in ks if 'torso' in n] == [NEW]
  k = ks[NEW]
  print('bsx_torso_kernel:', {f: k[f] for f in kr.FIELDS})
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
  assert k['agpr_count'] == 0, k
  assert k['group_segment_fixed_size'] <= 16 * 1024, k
  # three waves per SIMD, as before the mode: the float64 scores live where the 64 layer-2 accumulators are dead
  assert k['vgpr_count'] <= 168, k


@needs_llvm
def test_no_other_kernel_changed():
  """The metadata of every kernel of the library as it was before the drawn mode (recorded from the parent commit's build):
  only bsx_torso_kernel may differ — in its scalar registers and in its arguments (beta)."""
  from bsuite_amd import build
  before = json.load(open(BEFORE))
  fields = before['fields']
  now = {k['name']: [k[f] for f in fields] for k in kr.kernels(build.build())}
  assert set(now) == set(before['kernels'])
  changed = {n: dict(zip(fields, zip(before['kernels'][n], now[n]))) for n in now if now[n] != before['kernels'][n]}
  assert [n.split('(')[0] for n in changed] == [NEW], list(changed)
  diff = {f: v for f, v in next(iter(changed.values())).items() if v[0] != v[1]}
  assert set(diff) <= {'sgpr_count', 'kernarg_segment_size'}, diff
  assert diff['kernarg_segment_size'][1] - diff['kernarg_segment_size'][0] == 8      # double beta


@needs_llvm
def test_the_loops_of_the_kernel():
  """The compile-time mode doubles the bodies: 24 step loops (3 family variants x shared or not x record or not x greedy or
  drawn), each with the walk at its three widths (72 loops of depth 2) — and no loop anywhere else but the two wave
  reductions of bsx_pool_counts after each step loop.  Inside ANY loop: no barrier, no atomic, no LDS write, no scratch
  access, no flat or buffer access and no spill reload; the walks multiply and add packed, never fused; the drawn bodies keep
  their float64 logarithms out of the walk."""
  _, text = ki.kernel_text(os.path.join(CSRC, 'torso.hip'), NEW)
  in_loop, in_walk, inside, walk, steps, walks, others = False, False, [], [], 0, 0, 0
  for l in text:
    if re.match(r'^\.LBB\d+_\d+:', l) or l.startswith('; %bb.'):
      in_loop, in_walk = 'Loop' in l, 'Depth=2' in l
      steps += 'Loop Header' in l and 'Depth=1' in l and 'Inner' not in l
      others += 'Inner Loop Header' in l and 'Depth=1' in l
      walks += 'Loop Header' in l and 'Depth=2' in l
      continue
    if 'Loop Header' in l:                                                  # (a header comment on a line of its own)
      walks += 'Depth=2' in l
      in_walk = in_walk or 'Depth=2' in l
      continue
    s = l.strip()
    if in_loop and s and not s.startswith(';') and not s.startswith('.'):
      inside.append(s)
      if in_walk:
        walk.append(s)
  assert (steps, walks, others) == (24, 72, 48), (steps, walks, others)
  assert not any('Depth=3' in l for l in text)
  bad = [s for s in inside if re.match(r'flat_|scratch_|buffer_|(global|ds)_atomic|ds_write|ds_add|ds_\w*rtn|s_barrier', s)]
  assert not bad, bad[:8]
  assert not any(re.match(r'v_(pk_)?(fma|fmac|mad|mac)_f32', s) for s in walk)
  assert any(s.startswith('v_pk_mul_f32') for s in walk) and any(s.startswith('v_pk_add_f32') for s in walk)
  assert not any(re.match(r'v_\w+_f64', s) for s in walk), 'float64 inside the walk'
  stores = [s for s in inside if s.startswith('global_store')]
  assert len(stores) >= 12 * 5, len(stores)                                # twelve recording branches x five outputs
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
  assert not any('v_readlane' in s or 'v_writelane' in s for s in walk)
