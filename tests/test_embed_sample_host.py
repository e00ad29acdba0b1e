"""CPU: sample_embedding / evaluate_sampled_embedding (fused sampled closed loops of deep_sea and catch from a one-hidden-layer
network on the index row; bsx_<family>_embedding_sample, bsx_<family>_embedding_sample_evaluate) without a GPU — the composed
rule the kernel compiles (bsuite_amd/csrc/bsx_embed_sample.h, through gcc) against the numpy restatements of its two halves and
against utils.observations.embedding_logits / gumbel_select; ties, NaN logits, masked actions; the shim under the sanitizers as
a program of its own; the weight seeds of the GPU test on the C oracle; every refusal of the Python entry points, all before any
GPU use; the C ABI's declarations, bindings, exports, layout and argument checks; the source text; and the built library: still
ONE kernel with `embed` in its name, inside the kernel budget and the resource conditions, eight step loops of which the four
returns-only ones hold no store and no barrier."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import _native
from bsuite_amd.environments import base, cartpole, catch, deep_sea
from bsuite_amd.utils import observations, wrappers
from oracle import stream
from tests import embed_sample_util as su
from tests import embed_util as mu
from tests import tab_sample_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bsuite_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
SHIM = os.path.join(ROOT, 'tests', 'csrc', 'embed_sample_shim.c')
SAMPLE = dict(deep_sea='bsx_deep_sea_embedding_sample', catch='bsx_catch_embedding_sample')
EVALUATE = dict(deep_sea='bsx_deep_sea_embedding_sample_evaluate', catch='bsx_catch_embedding_sample_evaluate')
CALLS = ('sample_embedding', 'evaluate_sampled_embedding')
GCC = ['gcc', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off']
SHAPES = [(K, A, H) for (K, A) in ((1, 2), (2, 3)) for H in (1, 5, 64)]

_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------ bsx_embed_sample.h, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('embed_sample') / 'embed_sample_shim.so')
  subprocess.check_call(GCC + ['-O2', '-shared', '-fPIC', SHIM, '-o', so])
  lib = ctypes.CDLL(so)
  P, I64, I32, U64, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_double
  lib.shim_embed_sample.restype = None
  lib.shim_embed_sample.argtypes = [I64, I32, I32, I32, I32, P, P, P, P, P, P]
  lib.shim_embed_sample_action.restype = None
  lib.shim_embed_sample_action.argtypes = [I64, I32, I32, I32, I32, P, P, P, F64, U64, P, U64, P]
  return lib


def _run(lib, w1, w2, cells, words, beta):
  w1, w2, cells = np.ascontiguousarray(w1, np.float32), np.ascontiguousarray(w2, np.float32), np.ascontiguousarray(cells, np.int32)
  words = np.ascontiguousarray(words, np.uint32)
  n, K = cells.shape
  C, H, A = w1.shape[0] - 2, w1.shape[1], w2.shape[0]
  assert w2.shape == (A, H + 1) and words.shape == (n, A)
  beta = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, np.float64), (n,)))
  action = np.full(n, -1, np.int32)
  lib.shim_embed_sample(n, K, C, H, A, _ptr(w1), _ptr(w2), _ptr(cells), _ptr(words), _ptr(beta), _ptr(action))
  return action


def _agree(lib, w1, w2, cells, words, temperature):
  """The shim, the numpy restatement and the torch helpers on one pair at one temperature: the action; returns it and the logits."""
  beta = 1.0 / temperature
  action = _run(lib, w1, w2, cells, words, beta)
  want, logits, _ = su.np_sample(w1, w2, cells, words, beta)
  np.testing.assert_array_equal(action, want)
  t1, t2 = torch.from_numpy(np.ascontiguousarray(w1)), torch.from_numpy(np.ascontiguousarray(w2))
  tl = observations.embedding_logits(t1, t2, torch.from_numpy(np.ascontiguousarray(cells, np.int32)))
  ta = observations.gumbel_select(tl, np.ascontiguousarray(words, np.uint32), temperature)
  assert ta.dtype is torch.int32
  np.testing.assert_array_equal(ta.numpy(), action)
  return action, logits


def test_the_shim_compiles_the_kernels_header(shim):
  assert shim.shim_embed_sample_stream() == tu.STREAM_SAMPLE == 3
  text = open(os.path.join(CSRC, 'bsx_embed_sample.h')).read()
  for decl in ('BSX_HD int32_t bsx_embed_sample_select(', 'BSX_HD int32_t bsx_embed_sample_action(', '#include "bsx_embed.h"',
               '#include "bsx_tab_sample.h"'):
    assert decl in text, decl
  code = re.sub(r'//.*', '', text)
  # the composition alone: the two halves are called, not restated
  assert code.count('bsx_embed_logits(') == 1 and code.count('bsx_gumbel_select_n(') == 1 and code.count('bsx_gumbel_draws(') == 1
  assert 'fma' not in code and '__' not in code.replace('__cplusplus', '') and 'bsx_log' not in code and 'for (' not in code   # plain C99
  assert '#include "../../bsuite_amd/csrc/bsx_embed_sample.h"' in open(SHIM).read()
  assert '#include "bsx_embed_sample.h"' in open(os.path.join(CSRC, 'bsx_embed_device.h')).read()


@pytest.mark.parametrize('K,A,H', SHAPES)
def test_random_cases_against_the_restatements_and_the_helpers(shim, K, A, H):
  rng = np.random.RandomState(100 * K + 10 * A + H)
  C, n = 50 if K == 2 else 36, 3000
  w1, w2 = mu.pair(C, A, H, seed=H + A)
  cells = rng.randint(0, C, (n, K)).astype(np.int32)
  cells[:8, 0] = (-1, -2, -(1 << 31), C, C + 7, (1 << 31) - 1, 0, C - 1)       # "no cell", and cells outside [-1, C - 1]: clamped
  words = rng.randint(0, 1 << 32, (n, A), dtype=np.uint64).astype(np.uint32)
  words[:4] = [[0] * A, [0xFFFFFFFF] * A, [0] + [0xFFFFFFFF] * (A - 1), [0xFFFFFFFF] + [0] * (A - 1)]
  seen = set()
  for temperature in (1.0, 0.25, 4.0, 1e-3, 1e3):
    action, logits = _agree(shim, w1, w2, cells, words, temperature)
    seen |= set(action.tolist())
    if temperature == 1e-3:                                                     # cold: the draw is the greedy action where the logits differ enough
      gap = np.sort(logits, axis=1)
      sure = (gap[:, -1] - gap[:, -2]) * 1e3 > 60.0                             # |g_a - g_b| < 27 for every pair of words
      assert sure.sum() > n // 3
      np.testing.assert_array_equal(action[sure], mu.np_argmax(logits)[sure])
  assert seen == set(range(A))
  # a beta per case in one call, and the clamp: what is outside reads the nearest row
  beta = rng.choice([0.25, 1.0, 4.0], n)
  got = _run(shim, w1, w2, cells, words, beta)
  np.testing.assert_array_equal(got, su.np_sample(w1, w2, cells, words, beta)[0])
  np.testing.assert_array_equal(_run(shim, w1, w2, np.clip(cells, -1, C - 1), words, beta), got)
  # the words drawn in C: block 0 of stream 3 of (sample_seed, lane, step)
  lanes = np.uint64((1 << 32) - 17) + np.arange(n, dtype=np.uint64)
  for seed, step in ((0, 0), ((1 << 63) + 12345, 7), ((1 << 64) - 1, (1 << 40) + 3)):
    action = np.full(n, -1, np.int32)
    shim.shim_embed_sample_action(n, K, C, H, A, _ptr(w1), _ptr(w2), _ptr(cells), 0.5, seed, _ptr(lanes), step, _ptr(action))
    want = su.np_sample(w1, w2, cells, stream.words(seed, lanes, step, tu.STREAM_SAMPLE, A), 0.5)[0]
    np.testing.assert_array_equal(action, want)


def test_ties_nan_logits_and_masked_actions(shim):
  nan, inf = np.float32('nan'), np.float32('inf')
  rng = np.random.RandomState(5)
  for K, A in ((1, 2), (2, 3)):
    C, H, n = 6, 5, 7
    w1 = np.zeros((C + 2, H), np.float32)
    w2 = np.zeros((A, H + 1), np.float32)
    cells = np.array([[c] * K for c in range(-1, C)], np.int32)
    assert len(cells) == n
    same = np.full((n, A), 0x12345678, np.uint32)
    anyw = rng.randint(0, 1 << 32, (n, A), dtype=np.uint64).astype(np.uint32)
    # all logits equal and all words equal: every score is equal, the lowest index wins
    action, logits = _agree(shim, w1, w2, cells, same, 1.0)
    assert (action == 0).all() and (logits == 0).all()
    # ... the largest word alone decides between equal logits
    up = same.copy()
    up[:, A - 1] += 1
    assert (_agree(shim, w1, w2, cells, up, 1.0)[0] == A - 1).all()
    # a NaN logit never wins, whatever its word: l_1 = 0 + inf * 0
    w2[1, 2] = inf
    big = anyw.copy()
    big[:, 1] = 0xFFFFFFFF
    action, logits = _agree(shim, w1, w2, cells, big, 1.0)
    assert np.isnan(logits[:, 1]).all() and (action != 1).all()
    # a NaN l_0 is never beaten
    w2[:] = 0
    w2[0, 2] = inf
    w2[1, H] = 50.0
    action, logits = _agree(shim, w1, w2, cells, anyw, 1.0)
    assert np.isnan(logits[:, 0]).all() and (action == 0).all()
    # a -inf bias column masks its action at every temperature, for every word
    w2[:] = 0
    w2[0, H] = -inf
    low = anyw.copy()
    low[:, 1:] = 0                                                             # the smallest noise for the others
    low[:, 0] = 0xFFFFFFFF                                                     # the largest for the masked one
    for temperature in (0.25, 1.0, 4.0):
      action, logits = _agree(shim, w1, w2, cells, low, temperature)
      assert (logits[:, 0] == -inf).all() and (action != 0).all()
    w2[A - 1, H] = -inf
    action, _ = _agree(shim, w1, w2, cells, anyw, 4.0)
    if A == 3:
      assert (action == 1).all()
    # every bias -inf: nothing beats action 0
    w2[:, H] = -inf
    action, logits = _agree(shim, w1, w2, cells, anyw, 4.0)
    assert (logits == -inf).all() and (action == 0).all()
    # +inf logits tie at +inf: the lowest index among them
    w2[:] = 0
    w2[1:, H] = inf
    assert (_agree(shim, w1, w2, cells, anyw, 1.0)[0] == 1).all()


def test_the_shim_runs_stand_alone_under_the_sanitizers(tmp_path):
  """bsx_embed_sample.h with its own main under AddressSanitizer and UBSan, on the CPU: a program of its own, nothing loaded into
  python."""
  exe = str(tmp_path / 'embed_sample_shim_main')
  cmd = GCC + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DEMBED_SAMPLE_SHIM_MAIN', SHIM, '-o', exe, '-lm']
  if subprocess.run(cmd, capture_output=True).returncode != 0:
    pytest.skip('this gcc has no sanitizer runtime')
  out = subprocess.run([exe], capture_output=True, text=True)
  assert out.returncode == 0, out
  seen = [int(x) for x in out.stdout.split()]
  assert len(seen) == 3 and sum(seen) == 2 * 2 * 3 * 64 and all(s > 0 for s in seen), out


@pytest.mark.parametrize('name', [c[0] for c in su.CASES])
def test_the_weight_seeds_of_the_gpu_test_on_the_c_oracle(name):
  """The contract's SAMPLED loop on the C oracle, with the shared pair of each case of the GPU test, at its lanes, seed and
  defaults: a fresh call of 11 steps and 11 more take every action on live steps and see pre-activations of both signs — so a
  kernel that always answers 0 cannot pass there.  The recorded seed is the first that does."""
  _, fam, kwargs, H = next(c for c in su.CASES if c[0] == name)
  C, _, A = mu.geometry(fam, kwargs)
  assert su.CASES is mu.CASES and 1 <= H <= 64 and (mu.staged_bytes(C, H) > mu.LDS_BYTES) == name.endswith('_global')
  assert su.diverse(fam, kwargs, *mu.pair(C, A, H, su.PAIR_SEED[name]))
  assert su.first_good_seed(name) == su.PAIR_SEED[name]
  acts, pre = su.oracle_loop(fam, kwargs, *mu.pair(C, A, H, su.PAIR_SEED[name]))
  print(name, 'actions', np.bincount(acts, minlength=A), 'positive', int((pre > 0).sum()), 'negative', int((pre < 0).sum()))


# ------------------------------------------------------------------------------------------ the Python entry points
def _envs():
  return [deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4, observation_mode='index'),
          catch.Catch(seed=0, batch=4, observation_mode='index')]


def _weights(env, H=5, P=None):
  try:
    C, A = int(np.prod(env.board_shape)), env.action_spec().num_values
  except (ValueError, TypeError):
    C, A = 4, 2
  lead = () if P is None else (P,)
  return torch.zeros(lead + (C + 2, H)), torch.zeros(lead + (A, H + 1))


def _refused(env, name, exc=ValueError, match=None, **kw):
  """env.<name>(...) raises, its message names the caller (or the family), and nothing was allocated."""
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  w1, w2 = _weights(raw)
  w1, w2 = kw.pop('w1', w1), kw.pop('w2', w2)
  with pytest.raises(exc, match=match or name):
    getattr(env, name)(w1, w2, kw.pop('num_steps', 4), **kw)
  assert not raw._allocated and not raw._policy_rollout_out and raw._policy_eval_out is None        # pylint: disable=protected-access


def test_signatures_docstrings_and_families():
  for name in CALLS:
    fn = getattr(base.Environment, name)
    p = inspect.signature(fn).parameters
    assert list(p) == ['self', 'w1', 'w2', 'num_steps', 'policy_index', 'temperature', 'sample_seed']
    assert [p[k].kind for k in ('policy_index', 'temperature', 'sample_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
    assert p['policy_index'].default is None and p['temperature'].default == 1.0 and p['sample_seed'].default == 0
    for env in _envs():                                                                               # every refusal first: the last
      env._device = torch.device('cpu')                                                               # one of the call allocates nothing
      _refused(env, name, sample_seed=-1, match='sample_seed must be')
      # the order, two faults at a time: the environment, the matrices, the population rule (rollout_embedding's, in its
      # order), then the temperature and the seed, in sample_policy's words
      idx = torch.zeros(4, dtype=torch.int32)
      _refused(env, name, w1=None, num_steps=0, match='num_steps')
      _refused(env, name, w1=None, policy_index=idx, match='w1 and w2 must be')
      _refused(env, name, policy_index=idx, temperature=0.0, match='must be None')
      _refused(env, name, temperature=0.0, sample_seed=-1, match='temperature must be')
      env._logging = dict(steps=None)
      _refused(env, name, w1=None, num_steps=0, match='Logging')
  for tab, emb in (('sample_policy', 'sample_embedding'), ('evaluate_sampled_policy', 'evaluate_sampled_embedding')):
    env = _envs()[1]
    env._device = torch.device('cpu')
    said = []
    for call, args in ((tab, (torch.zeros((env.policy_num_states, 3)),)), (emb, _weights(env))):
      said.append(str(pytest.raises(ValueError, getattr(env, call), *args, 4, temperature=0.0).value).replace(call, ''))
    assert said[0] == said[1]                                                                         # one rule for the temperature
  doc = base.Environment.sample_embedding.__doc__
  for word in ('ts[t] = step(a); actions[t] = a', 'gumbel_select', 'embedding_logits', 'stream 3', 'rollout(actions)', 'policy_index',
               'cached per T', 'temperature', 'sample_seed', '4-byte', 'rollout_policy', 'rollout_embedding', 'C + 2', 'H + 1',
               '1 <= H <= 64', 'no epsilon', '-inf logit', 'softmax(logits / temperature)', '15 KiB'):
    assert word in doc, word
  doc = base.Environment.evaluate_sampled_embedding.__doc__
  for word in ('sample_embedding', 'PolicyEvaluation', 'evaluate_policy', 'float64'):
    assert word in doc, word
  abi = lambda cls, name: cls._closed_loop_abi(object.__new__(cls), name)                             # pylint: disable=protected-access
  for fam, cls in (('deep_sea', deep_sea.DeepSea), ('catch', catch.Catch)):
    assert abi(cls, 'sample_embedding') == SAMPLE[fam] and abi(cls, 'evaluate_sampled_embedding') == EVALUATE[fam]
    assert SAMPLE[fam] in _native.EXPORTED and EVALUATE[fam] in _native.EXPORTED
  for name in CALLS:
    assert abi(base.Environment, name) is None and abi(cartpole.Cartpole, name) is None


@pytest.mark.parametrize('name', CALLS)
def test_views_families_and_modes_are_refused(name):
  _refused(catch.Catch(seed=0), name, match='batched view')
  _refused(deep_sea.DeepSea(size=8, mapping_seed=0, seed=0), name, match='batched view')
  for bsuite_id in ('bandit/0', 'cartpole/0', 'mountain_car/0', 'memory_len/0', 'umbrella_length/0', 'discounting_chain/0',
                    'cartpole_swingup/0'):
    _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), name, match='deep_sea and catch only')
  _refused(catch.Catch(seed=0, batch=4), name, match="observation_mode='index'")
  _refused(catch.Catch(seed=0, batch=4, observation_mode='delta'), name, match="observation_mode='index'")
  _refused(deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4), name, match="observation_mode='index'")
  for dt in (torch.uint8, 'float16', torch.bfloat16):
    _refused(catch.Catch(seed=0, batch=4, observation_dtype=dt), name, match="observation_mode='index'")
  _refused(catch.Catch(seed=0, batch=4, observation_mode='index', rng='mt19937'), name, match='philox')
  for env in _envs():
    env._logging = dict(steps=None)           # what enable_logging() leaves behind (it allocates: not without a GPU)
    _refused(env, name, match='Logging')
  for env in _envs():
    env._grouped_by = object()                # what SweepBatch sets while its prepared groups hold the column pointers
    _refused(env, name, exc=RuntimeError, match='release_groups')
  with pytest.raises(ValueError, match=name + r'\(\) needs the batched view'):
    getattr(catch.Catch(seed=0), name)(torch.zeros((52, 3)), torch.zeros((3, 4)), 4)


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
  for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    fn = getattr(cls, name)
    assert fn is not getattr(base.Environment, name) and any(name in vars(c) for c in cls.__mro__[:-1]), cls
    with pytest.raises(ValueError, match=name):
      fn(object.__new__(cls), torch.zeros((6, 2)), torch.zeros((2, 3)), 4, temperature=0.5, sample_seed=1)
  image = wrappers.ImageObservation(catch.Catch(seed=0, batch=4), (84, 84, 1))
  _refused(image, name, match='not available through ImageObservation')


@pytest.mark.parametrize('name', CALLS)
def test_arguments_are_checked_before_any_gpu_use(name):
  for env in _envs():
    env._device = torch.device('cpu')       # the checks themselves, on host tensors: dtype, shape, contiguity
    C, A = int(np.prod(env.board_shape)), env.action_spec().num_values
    assert (C, A) == ((64, 2) if isinstance(env, deep_sea.DeepSea) else (50, 3))
    H = 5
    ok1, ok2 = _weights(env, H)
    pop1, pop2 = _weights(env, H, P=4)
    idx = torch.zeros(4, dtype=torch.int32)
    for n in (0, -1, 2.0, None, '4', True):
      _refused(env, name, num_steps=n, match=f'{name}: num_steps')
    msg = f'{name}: w1 and w2 must be'
    for bad in (ok1.to(torch.float64), ok1.to(torch.float16), ok1.numpy(), ok1.tolist(), None, torch.zeros((C + 1, H)), torch.zeros((C + 3, H)),
                torch.zeros((C + 2, H + 1)), torch.zeros((C + 2) * H), torch.zeros((H, C + 2)), torch.zeros((2, 2, C + 2, H)),
                torch.zeros((C + 2, 0)), torch.zeros((C + 2, 2 * H))[:, ::2], torch.zeros((2 * (C + 2), H))[::2], torch.zeros(()), pop1):
      _refused(env, name, w1=bad, match=msg)
    for bad in (ok2.to(torch.float64), ok2.numpy(), None, torch.zeros((A + 1, H + 1)), torch.zeros((A - 1, H + 1)), torch.zeros((5 - A, H + 1)),
                torch.zeros((A, H)), torch.zeros((A, H + 2)), torch.zeros((H + 1, A)), torch.zeros((A, 2 * (H + 1)))[:, ::2], pop2):
      _refused(env, name, w2=bad, match=msg)
    # H in [1, 64]
    _refused(env, name, w1=torch.zeros((C + 2, 65)), w2=torch.zeros((A, 66)), match=msg)
    _refused(env, name, w1=torch.zeros((0, C + 2, H)), w2=torch.zeros((0, A, H + 1)), match=msg)
    _refused(env, name, w1=pop1, w2=torch.zeros((3, A, H + 1)), match=msg)                                 # two populations of different sizes
    for h in (1, 64):
      assert env._check_sample_embedding(torch.zeros((C + 2, h)), torch.zeros((A, h + 1)), 4, None, 1.0, 0, name) == (1, h, 1.0)   # pylint: disable=protected-access
    assert '1 <= H <= 64' in str(pytest.raises(ValueError, getattr(env, name), None, None, 4).value)
    _refused(env, name, policy_index=idx, match='must be None')
    _refused(env, name, w1=ok1.reshape(1, C + 2, H), w2=ok2.reshape(1, A, H + 1), policy_index=idx, match='must be None')   # [1, ...] is one pair
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, name, w1=pop1, w2=pop2, policy_index=bad, match='policy_index')
    # the temperature and the seed: sample_policy's messages
    for t in (0.0, -1.0, float('nan'), float('inf'), -float('inf'), 1e-320, '1.0', None, True, [1.0]):
      _refused(env, name, temperature=t, match=rf'{name}: temperature must be a finite number > 0 with a finite 1 / temperature')
    for seed in (-1, 1 << 64, 0.5, None, True, '3'):
      _refused(env, name, sample_seed=seed, match=rf'{name}: sample_seed must be an integer in \[0, 2\^64\)')
    for word in ('epsilon', 'explore_seed'):                               # drawn: there is no epsilon
      with pytest.raises(TypeError, match=word):
        getattr(env, name)(ok1, ok2, 4, **{word: 0})
    # the order: the matrices before the population rule, the population rule before the temperature, the temperature before the seed
    _refused(env, name, w1=None, policy_index=idx, temperature=0.0, match=msg)
    _refused(env, name, policy_index=idx, temperature=0.0, match='must be None')
    _refused(env, name, temperature=0.0, sample_seed=-1, match='temperature')
    _refused(env, name, num_steps=0, w1=None, temperature=0.0, match='num_steps')
    # views that start one float into a buffer pass the checks (only 4-byte alignment is assumed)
    v1 = torch.zeros((C + 2) * H + 1)[1:].reshape(C + 2, H)
    v2 = torch.zeros(A * (H + 1) + 1)[1:].reshape(A, H + 1)
    assert v1.is_contiguous() and v1.data_ptr() % 8 == 4 and v2.data_ptr() % 8 == 4
    assert env._check_sample_embedding(v1, v2, 4, None, 0.25, (1 << 64) - 1, name) == (1, H, 4.0)     # pylint: disable=protected-access
    assert env._check_sample_embedding(pop1, pop2, np.int64(7), idx, np.float32(4.0), np.int64(5), name) == (4, H, 0.25)   # pylint: disable=protected-access
    assert not env._allocated                                                                              # pylint: disable=protected-access
  # host matrices for an environment on the GPU
  env = catch.Catch(seed=0, batch=4, observation_mode='index')
  _refused(env, name, match='w1 and w2 must be')


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
    for name, like, out_t, out_c in ((SAMPLE[fam], f'bsx_{fam}_policy_sample', 'bsx_timestep_t', _native.TimeStepPtrs),
                                     (EVALUATE[fam], f'bsx_{fam}_policy_sample_evaluate', 'bsx_policy_eval_t', _native.PolicyEvalPtrs)):
      types = types_of(name)
      assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_policy_embedding_sample_t*', 'int32_t*', out_t, 'double*']
      assert [t.replace('bsx_policy_embedding_sample_t', 'bsx_policy_logits_t') for t in types] == types_of(like)   # the signature of the tabular call
      assert name in _native.EXPORTED
      fn = getattr(_native.lib, name)
      assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.PolicyEmbeddingSample), P, out_c, P]
      assert fn.restype is ctypes.c_int
      assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
      assert name in text, f'INTEGRATION.md does not describe {name}'
      assert 'extern "C" int ' + name + '(' in open(os.path.join(CSRC, fam + '.hip')).read()
  body = re.search(r'typedef struct \{([^}]*)\} bsx_policy_embedding_sample_t;', plain).group(1)
  fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
  assert fields == ['const float* w1', 'const float* w2', 'int32_t n_cells, n_hidden, n_actions, n_policies', 'const int32_t* policy_index',
                    'double inv_temperature', 'uint64_t sample_seed', 'int32_t* actions_out']
  names = ['w1', 'w2', 'n_cells', 'n_hidden', 'n_actions', 'n_policies', 'policy_index', 'inv_temperature', 'sample_seed', 'actions_out']
  assert [f[0] for f in _native.PolicyEmbeddingSample._fields_] == names                                # pylint: disable=protected-access
  # the layout, against the C compiler's — and bsx_policy_embedding_t is where it was
  both = [('bsx_policy_embedding_sample_t', names),
          ('bsx_policy_embedding_t', [n.replace('inv_temperature', 'epsilon').replace('sample_seed', 'explore_seed') for n in names])]
  src = '#include <stdio.h>\n#include <stddef.h>\n#include "bsuite_amd.h"\nint main(void) {\n'
  for t, ns in both:
    src += ('  printf("%zu ' + '%zu ' * len(ns) + '\\n", sizeof(' + t + '), ' + ', '.join(f'offsetof({t}, {n})' for n in ns) + ');\n')
  src += '  return 0; }\n'
  with tempfile.TemporaryDirectory() as d:
    open(os.path.join(d, 'l.c'), 'w').write(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'l.c'), '-o', os.path.join(d, 'l')])
    got = [[int(x) for x in l.split()] for l in subprocess.check_output([os.path.join(d, 'l')], text=True).splitlines()]
  L = _native.PolicyEmbeddingSample
  layout = [64, 0, 8, 16, 20, 24, 28, 32, 40, 48, 56]
  assert got[0] == [ctypes.sizeof(L)] + [getattr(L, n).offset for n in names] == layout
  assert got[1] == layout and ctypes.sizeof(_native.PolicyEmbedding) == 64
  note = header[header.index('fused sampled closed loops from a hidden-layer policy on the index row'):header.index('} bsx_policy_embedding_sample_t;')]
  for word in ('BSX_STREAM_SAMPLE', 'BSX_ERANGE', 'BSX_EALIGN', 'inv_temperature', '4-byte aligned', 'bsx_embed_sample.h', 'v12, additive',
               'n_lanes == 0', 'graph-capturable', 'a -inf logit masks its action'):
    assert word in note, word


def _abi_case(fam):
  if fam == 'deep_sea':
    return _native.DeepSeaCfg(size=10, deterministic=1, move_cost=0.001, inv_size=0.1), 100, 2, _native.DeepSeaCfg(size=65)
  return _native.CatchCfg(10, 5), 50, 3, _native.CatchCfg(1, 5)


@pytest.mark.parametrize('kind', ['sample', 'evaluate'])
@pytest.mark.parametrize('fam', ['deep_sea', 'catch'])
def test_argument_checks_of_the_entry_points(fam, kind):
  """Every refusal comes before any device work: garbage stands in for device pointers, none is dereferenced.  The codes and
  their order are those of bsx_<family>_embedding_rollout / _embedding_evaluate; an inv_temperature that is not finite and > 0
  is BSX_ERANGE where an epsilon outside [0, 1] is there, and w1 or w2 off the 4-byte grid is BSX_EALIGN, last."""
  record = kind == 'sample'
  fn = getattr(_native.lib, (SAMPLE if record else EVALUATE)[fam])
  cfg, C, A, bad_cfg = _abi_case(fam)
  junk = 0xDEAD0010                                                # never mapped: a dereference would fault (16-byte aligned)
  E = _native
  nan, inf = float('nan'), float('inf')

  def call(**kw):
    c = _native.Call(n_lanes=kw.pop('n_lanes', 4), n_steps=kw.pop('n_steps', 4), flags=kw.pop('flags', E.CALL_OBS_INDEX))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def pol(**kw):
    d = dict(w1=junk, w2=junk + 64, n_cells=C, n_hidden=5, n_actions=A, n_policies=1, policy_index=None, inv_temperature=1.0,
             sample_seed=0, actions_out=junk if record else None)
    d.update(kw)
    return _native.PolicyEmbeddingSample(**d)

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
    assert run(call(flags=flags), pol(n_cells=-1)) == E.BSX_EMODE, flags
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
  for c_ in (C - 1, C + 1, C + 2, 0, -C):
    assert run(call(), pol(n_cells=c_)) == E.BSX_EINVAL, c_
  for a in (A - 1, A + 1, 5 - A, 0, -A, 1 << 20):                    # the other family's width among them
    assert run(call(), pol(n_actions=a)) == E.BSX_EINVAL, a
    assert run(call(), pol(n_actions=a, inv_temperature=nan)) == E.BSX_EINVAL, a
    assert run(call(n_lanes=0), pol(n_actions=a)) == E.BSX_EINVAL, a
  for h in (0, -1, 65, 1 << 20, -(1 << 31)):
    assert run(call(), pol(n_hidden=h)) == E.BSX_EINVAL, h
    assert run(call(), pol(n_hidden=h, inv_temperature=0.0)) == E.BSX_EINVAL, h
    assert run(call(n_lanes=0), pol(n_hidden=h)) == E.BSX_EINVAL, h
  for n in (0, -3):
    assert run(call(), pol(n_policies=n)) == E.BSX_EINVAL
    assert run(call(), pol(n_policies=n, inv_temperature=0.0)) == E.BSX_EINVAL
  # BSX_ERANGE: inv_temperature finite and > 0 — before an empty call returns and before any pointer is looked at
  for b in (0.0, -0.0, -0.1, -1.0, nan, inf, -inf):
    assert run(call(), pol(inv_temperature=b)) == E.BSX_ERANGE, b
    assert run(call(n_lanes=0), pol(inv_temperature=b)) == E.BSX_ERANGE, b
    assert run(call(), pol(inv_temperature=b, w1=None), state=None) == E.BSX_ERANGE, b
  assert run(call(), pol(), cfg_=bad_cfg) == E.BSX_ERANGE
  assert run(call(flags=0), pol(), cfg_=bad_cfg) == E.BSX_ERANGE                             # (the cfg comes first)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at; both ends of H, any acceptable inverse temperature
  for h, b in ((1, 5e-324), (64, 1.7976931348623157e308), (5, 2.0)):
    assert run(call(n_lanes=0), pol(w1=None, w2=None, n_hidden=h, inv_temperature=b, actions_out=None), state=None,
               out=outs(*((0,) * (4 if record else 3))), info=None) == 0, h
  assert run(call(n_lanes=0), pol(w1=junk + 2)) == 0                                          # (not even the alignment)
  # BSX_ENULL: every pointer — the other ones garbage
  assert run(call(), pol(w1=None)) == E.BSX_ENULL
  assert run(call(), pol(w2=None)) == E.BSX_ENULL
  assert run(call(), pol(), state=None) == E.BSX_ENULL
  assert run(call(), pol(), info=None) == E.BSX_ENULL
  n_out = 4 if record else 3
  for k in range(n_out):
    ptrs = [junk] * n_out
    ptrs[k] = 0
    assert run(call(), pol(), out=outs(*ptrs)) == E.BSX_ENULL, k
  if record:
    assert run(call(), pol(actions_out=None)) == E.BSX_ENULL                                  # the action column
    assert run(call(), pol(), out=outs(junk, junk, junk, junk + 8)) == E.BSX_EALIGN           # the index rows: 16 bytes, as in the tabular call
  else:
    assert run(call(n_lanes=0), pol(actions_out=junk)) == 0                                   # (not looked at)
  assert run(call(), pol(n_policies=2)) == E.BSX_ENULL                                        # a population without policy_index
  # BSX_EALIGN: w1 or w2 off the 4-byte grid — after the pointers; 4 bytes are enough
  for off in (1, 2, 3, 5, 6, 7):
    assert run(call(), pol(w1=junk + off)) == E.BSX_EALIGN, off
    assert run(call(), pol(w2=junk + 64 + off)) == E.BSX_EALIGN, off
    assert run(call(), pol(w1=junk + off), state=None) == E.BSX_ENULL, off
  assert run(call(n_lanes=1 << 40), pol()) == E.BSX_EINVAL                                    # more workgroups than a grid holds
  assert run(call(action_ring=-2), pol()) == E.BSX_EINVAL


# ------------------------------------------------------------------------------------------ the source text
def test_the_drawn_path_uses_the_headers_and_the_hidden_layer_is_stated_once():
  dev = open(os.path.join(CSRC, 'bsx_embed_device.h')).read()
  code = re.sub(r'//.*', '', dev)

  def fn_text(kind, name):
    t = dev[dev.index(kind + ' ' + name + '('):]
    return t[:t.index('\n}\n')]

  best = fn_text('int', 'bsx_embed_best')
  # the draw takes its logits from the walk the greedy action takes: after both look-ups, before the argmax
  assert best.index('} else {') < best.index('bsx_gumbel_draws(p.sample_seed, lane, step)') < best.index('bsx_gumbel_select_n(l, A, p.beta, u.v)') < best.index('bsx_embed_argmax(l, A)')
  assert 'if constexpr (__is_same(Source, bsx_embed_gumbel))' in best
  assert code.count('bsx_gumbel_draws(p.sample_seed, lane, step)') == 1 and code.count('bsx_gumbel_select_n(') == 1
  # the hidden-unit loops exist once each, with the padded stride and 16-byte LDS reads
  for once in ('for (int j = 0; j < H; j += 4) {', 'for (int j = 0; j < H; ++j) {', 'bsx_embed_preactivation(b[c], ek, K)',
               'bsx_embed_preactivation(gb[j], ek, K)', 'BSX_EMBED_STRIDE(H) >> 2', '(bsx_embed_lds4)s_net', 'int bsx_embed_best('):
    assert code.count(once) == 1, once
  assert code.count('bsx_embed_accumulate(') == 2 and code.count('void bsx_embed_record_body(') == 1 and code.count('void bsx_embed_returns_body(') == 1
  # the drawn action: the same function with the other source, no coin
  drawn = dev[dev.index('int bsx_embed_action(bsx_embed_gumbel,'):]
  drawn = drawn[:drawn.index('\n}\n')]
  assert 'bsx_embed_best<K, A, bsx_embed_gumbel>(fn, st, p, s_net, prow, lane, step)' in drawn
  assert 'epsilon' not in drawn and 'bsx_policy_select' not in drawn and 'bsx_policy_draws' not in drawn
  for body in ('bsx_embed_record_body', 'bsx_embed_returns_body'):
    t = fn_text('void', body)
    assert 'typedef typename bsx_embed_source_of<F>::type Source;' in t and 'bsx_embed_action<F::K, F::A>(Source(), ' in t
    assert t.count('bsx_embed_view(ka)') == 4                                # before the loop, per step, after the loop, the counters
  # no logarithm, no Philox and no second Gumbel rule outside the headers
  for f in ('bsx_embed_device.h', 'embed.hip', 'deep_sea.hip', 'catch.hip'):
    text = re.sub(r'//.*', '', open(os.path.join(CSRC, f)).read())
    for word in ('bsx_log(', 'bsx_gumbel_score', 'bsx_gumbel_noise', 'z_best', 'philox'):
      assert word not in text, (f, word)
  hip = open(os.path.join(CSRC, 'embed.hip')).read()
  assert hip.count('__global__') == 1 and hip.count('bsx_embed_view') == 0
  for inst in ('record_body<bsx_embed_drawn<bsx_embed_deep_sea>>', 'returns_body<bsx_embed_drawn<bsx_embed_deep_sea>>',
               'record_body<bsx_embed_drawn<bsx_embed_catch>>', 'returns_body<bsx_embed_drawn<bsx_embed_catch>>'):
    assert hip.count('bsx_embed_' + inst) == 1, inst
  assert 'if (a.drawn == 0) {' in hip
  # the entry points: the checks of the greedy calls on a stand-in, the temperature where the epsilon is
  assert 'bsx_check_embed_call(call, &em,' in dev and 'bsx_check_embed_eval_call(call, &em,' in dev
  assert '__builtin_isfinite(sm->inv_temperature) && sm->inv_temperature > 0.0' in dev


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position
from tests.test_tab_sample_host import _loops  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
KERNEL = 'bsx_embed_kernel'


@needs_llvm
def test_product_library_keeps_one_embed_kernel_inside_the_budget_and_the_resource_conditions():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  assert [n for n in ks if 'embed' in n] == [KERNEL]                                          # ONE kernel for the eight cases
  k = ks[KERNEL]
  print(KERNEL, {f: k[f] for f in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'kernarg_segment_size')})
  assert k['vgpr_count'] <= 80, k                                                             # 6 waves per SIMD, the greedy calls' occupancy
  assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0 and k['agpr_count'] == 0, k
  assert mu.LDS_BYTES <= k['group_segment_fixed_size'] <= 16384, k
  assert k['kernarg_segment_size'] <= 1024, k


@needs_llvm
def test_the_eight_step_loops_of_the_kernel():
  """The step loops are the outermost loops that compute in float64 (the reward sums, the lane advance, the Gumbel scores):
  eight, one per branch.  Four of them — the returns-only branches, greedy and drawn — hold no store and no barrier; the other
  four hold the per-step stores, non-temporal [T,B] outputs alone.  Four loops, two of each kind, hold the logarithms' divisions.
  No flat or scratch access anywhere in the kernel; no spill reload in any loop."""
  _, text = ki.kernel_text(os.path.join(CSRC, 'embed.hip'), KERNEL)
  loops, outside = _loops(text)
  everything = outside + [s for body in loops.values() for s in body]
  assert not any(s.startswith('flat_') or s.startswith('scratch_') for s in everything)
  is_store = lambda s: re.match(r'(global|flat|scratch|buffer)_store|ds_write|(global|ds)_atomic|ds_add', s)
  steps = {h: body for h, body in loops.items() if any(re.match(r'v_\w+_f64', s) for s in body)}
  print({h: len(b) for h, b in steps.items()})
  assert len(steps) >= 8, sorted(steps)
  assert not any(s.startswith('s_barrier') for body in steps.values() for s in body)
  returns = [h for h, body in steps.items() if not any(is_store(s) for s in body)]
  record = [h for h in steps if h not in returns]
  assert len(returns) >= 4 and len(record) >= 4, (returns, record)
  # the drawn loops: bsx_log divides ((m - 1) / (m + 1)), two logarithms per action — at least four float64 divisions (two
  # v_div_scale_f64 each) more than the family's greedy loop has in its lane advance (deep_sea none, catch three)
  divs = {h: sum(s.startswith('v_div_scale_f64') for s in body) for h, body in steps.items()}
  drawn = [h for h in steps if divs[h] >= 2 * 4 + min(divs.values())]
  assert min(divs.values()) == 0 and len(drawn) == 4, divs
  assert len([h for h in drawn if h in returns]) == 2 and len([h for h in drawn if h in record]) == 2, (drawn, returns)
  for h in record:
    stores = [s for s in steps[h] if s.startswith('global_store')]
    assert not any(re.match(r'ds_write|(global|ds)_atomic|ds_add', s) for s in steps[h]), h
    assert stores and all(s.endswith(' nt') or s.startswith('global_store_dwordx2 ') for s in stores), stores
  assert any(s.startswith('ds_read_b128') for s in everything) and any(s.startswith('global_load_dword ') for s in everything)
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
