"""CPU: rollout_embedding / evaluate_embedding (fused closed loops of deep_sea and catch from a one-hidden-layer network on the
index row; bsx_<family>_embedding_rollout, bsx_<family>_embedding_evaluate) without a GPU — the rule the kernel compiles
(bsuite_amd/csrc/bsx_embed.h, through gcc) against a numpy float32 restatement with one rounding per operation and against
utils.observations.embedding_logits / embedding_select; ties, NaN and infinite values, a -0.0 pre-activation, the same cell
twice, cell -1 and cells outside the board; the weight seeds of the GPU test on the C oracle; every refusal of the Python entry
points, all before any GPU use; the C ABI's declarations, bindings, exports and argument checks; the source text; and the built
library: ONE new kernel inside the kernel budget, paid for by the two single-family group kernels that became one, inside the
resource conditions, with no store and no barrier inside the loops of its returns-only branches."""
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
from tests import embed_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bsuite_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
SHIM = os.path.join(ROOT, 'tests', 'csrc', 'embed_shim.c')
ROLLOUT = dict(deep_sea='bsx_deep_sea_embedding_rollout', catch='bsx_catch_embedding_rollout')
EVALUATE = dict(deep_sea='bsx_deep_sea_embedding_evaluate', catch='bsx_catch_embedding_evaluate')
CALLS = ('rollout_embedding', 'evaluate_embedding')
GCC = ['gcc', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off']
SHAPES = [(K, A, H) for (K, A) in ((1, 2), (2, 3), (1, 3), (2, 2)) for H in (1, 5, 64)]

_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
_bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------ bsx_embed.h, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('embed') / 'embed_shim.so')
  subprocess.check_call(GCC + ['-O2', '-shared', '-fPIC', SHIM, '-o', so])
  lib = ctypes.CDLL(so)
  P, I64, I32, F32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
  lib.shim_embed.restype = None
  lib.shim_embed.argtypes = [I64, I32, I32, I32, I32, P, P, P, P, P]
  lib.shim_embed_row.restype, lib.shim_embed_row.argtypes = I32, [I32, I32]
  lib.shim_embed_preactivation.restype, lib.shim_embed_preactivation.argtypes = F32, [F32, P, I32]
  lib.shim_embed_argmax.restype, lib.shim_embed_argmax.argtypes = I32, [P, I32]
  lib.shim_embed_stride.restype, lib.shim_embed_stride.argtypes = I32, [I32]
  lib.shim_embed_staged_bytes.restype, lib.shim_embed_staged_bytes.argtypes = I64, [I32, I32]
  return lib


def _run(lib, w1, w2, cells, A):
  w1, w2, cells = np.ascontiguousarray(w1, np.float32), np.ascontiguousarray(w2, np.float32), np.ascontiguousarray(cells, np.int32)
  n, K = cells.shape
  C, H = w1.shape[0] - 2, w1.shape[1]
  assert w2.shape == (A, H + 1)
  logits, action = np.full((n, A), 7.0, np.float32), np.full(n, -1, np.int32)
  lib.shim_embed(n, K, C, H, A, _ptr(w1), _ptr(w2), _ptr(cells), _ptr(logits), _ptr(action))
  return logits, action


def _agree(lib, w1, w2, cells, A):
  """The shim, the numpy restatement and the torch helpers on one pair: the logits bit for bit, the action; returns both."""
  logits, action = _run(lib, w1, w2, cells, A)
  want, _ = mu.np_logits(w1, w2, cells)
  np.testing.assert_array_equal(_bits(logits), _bits(want))
  np.testing.assert_array_equal(action, mu.np_argmax(want))
  t1, t2, tc = torch.from_numpy(np.ascontiguousarray(w1)), torch.from_numpy(np.ascontiguousarray(w2)), torch.from_numpy(np.ascontiguousarray(cells, np.int32))
  tl = observations.embedding_logits(t1, t2, tc)
  assert tl.dtype is torch.float32 and tuple(tl.shape) == logits.shape
  np.testing.assert_array_equal(_bits(tl.numpy()), _bits(want))
  ta = observations.embedding_select(t1, t2, tc)
  assert ta.dtype is torch.int32
  np.testing.assert_array_equal(ta.numpy(), action)
  return logits, action


def test_the_shim_compiles_the_kernels_header(shim):
  assert shim.shim_embed_lds_bytes() == mu.LDS_BYTES == 15360 and shim.shim_embed_max_hidden() == mu.MAX_HIDDEN == _native.MLP_MAX_HIDDEN
  for H in range(1, 65):
    assert shim.shim_embed_stride(H) == mu.stride(H) and mu.stride(H) % 4 == 0 and mu.stride(H) >= H + 4 - 3
    assert (mu.stride(H) // 4) % 2 == 0 or mu.stride(H) % 64 != 0            # never a whole number of bank rows
    for C in (16, 36, 49, 50, 64, 100, 900):
      assert shim.shim_embed_staged_bytes(C, H) == mu.staged_bytes(C, H)
  # the budget: catch/0 with H = 64 fits, as does deep_sea size 7; size 8 is the smallest deep_sea that does not
  assert mu.staged_bytes(50, 64) == 52 * 68 * 4 + 65 * 16 == 15184 <= mu.LDS_BYTES
  assert mu.staged_bytes(49, 64) <= mu.LDS_BYTES < mu.staged_bytes(64, 64)
  assert all(mu.staged_bytes(900, H) > mu.LDS_BYTES for H in (16, 64))       # deep_sea/10: global memory
  text = open(os.path.join(CSRC, 'bsx_embed.h')).read()
  for decl in ('BSX_HD int32_t bsx_embed_row(int32_t cell, int32_t n_cells)', 'BSX_HD float bsx_embed_preactivation(float bias, const float* e, int K)',
               'BSX_HD void bsx_embed_accumulate(float* l, const float* w2j, float h, int A)', 'BSX_HD int32_t bsx_embed_argmax(const float* l, int A)',
               'BSX_HD int32_t bsx_embed_select(', 'BSX_HD void bsx_embed_logits('):
    assert decl in text, decl
  assert '#include "bsx_mlp.h"' in text and text.count('BSX_NO_CONTRACT') >= 3 and 'bsx_mlp_relu(' in text
  code = re.sub(r'//.*', '', text)
  assert 'fma' not in code and '__' not in code.replace('__cplusplus', '')   # plain C99
  assert '#include "../../bsuite_amd/csrc/bsx_embed.h"' in open(SHIM).read()
  # the pinned headers are as they were: nothing of this feature in them
  for f in ('bsx_mlp.h', 'bsx_policy.h', 'bsx_tab_sample.h', 'bsx_tab_sample_device.h', 'tab_sample.hip', 'mlp.hip'):
    assert 'embed' not in open(os.path.join(CSRC, f)).read(), f


def test_the_pieces(shim):
  C = 50
  for cell, want in ((-1, 0), (0, 1), (49, 50), (50, 50), (1 << 30, 50), (-2, 0), (-(1 << 31), 0), ((1 << 31) - 1, 50), (7, 8)):
    assert shim.shim_embed_row(cell, C) == want, cell
  e = np.array([1e8, -1e8], np.float32)
  # the order of the adds: (bias + e0) + e1
  assert shim.shim_embed_preactivation(1.0, _ptr(e), 2) == np.float32(np.float32(np.float32(1.0) + e[0]) + e[1]) == 0.0
  assert shim.shim_embed_preactivation(1.0, _ptr(e[::-1].copy()), 2) == 0.0 and shim.shim_embed_preactivation(1.0, _ptr(e), 1) == 1e8
  nan, inf = np.float32('nan'), np.float32('inf')
  for l, want in (((1, 1, 1), 0), ((0, 1, 1), 1), ((0, 0, 1), 2), ((-0.0, 0.0, -0.0), 0), ((nan, 1, 2), 0), ((0, nan, 2), 2),
                  ((0, 1, nan), 1), ((nan, nan, nan), 0), ((-inf, -inf, -inf), 0), ((0, inf, inf), 1), ((-inf, nan, 0), 2)):
    arr = np.array(l, np.float32)
    assert shim.shim_embed_argmax(_ptr(arr), 3) == want, l
    assert mu.np_argmax(arr[None])[0] == want
    if want < 2 and not (l[2] > l[want]):
      assert shim.shim_embed_argmax(_ptr(arr), 2) == want, l


@pytest.mark.parametrize('K,A,H', SHAPES)
def test_random_cases_against_the_restatement_and_the_helpers(shim, K, A, H):
  rng = np.random.RandomState(100 * K + 10 * A + H)
  C, n = 50 if K == 2 else 36, 3000
  w1, w2 = mu.pair(C, A, H, seed=H + A)
  cells = rng.randint(0, C, (n, K)).astype(np.int32)
  cells[:8, 0] = (-1, -2, -(1 << 31), C, C + 7, (1 << 31) - 1, 0, C - 1)       # "no cell", and cells outside [-1, C - 1]: clamped
  if K == 2:
    cells[8:16, 1] = cells[8:16, 0]                                            # the same cell twice: added twice
    cells[16:20, 1] = (-1, C, -5, 1 << 20)
  logits, action = _agree(shim, w1, w2, cells, A)
  assert len(np.unique(_bits(logits), axis=0)) > 4                               # the logits follow the cells (one hidden unit is 0 on half of them)
  _, s = mu.np_logits(w1, w2, cells)
  assert (s > 0).any() and (s < 0).any()
  # the clamp: what is outside reads the nearest row
  clamped = np.clip(cells, -1, C - 1)
  np.testing.assert_array_equal(_bits(_run(shim, w1, w2, clamped, A)[0]), _bits(logits))
  if K == 2:
    twice = mu.np_logits(w1, w2, cells[8:16])[1]
    want = (w1[C + 1] + w1[cells[8:16, 0] + 1]).astype(np.float32)
    want = (want + w1[cells[8:16, 0] + 1]).astype(np.float32)
    np.testing.assert_array_equal(_bits(twice), _bits(want))
  # one pair per lane
  p1, p2 = mu.pair(C, A, H, seed=9, P=64)
  tl = observations.embedding_logits(torch.from_numpy(p1), torch.from_numpy(p2), torch.from_numpy(cells[:64]))
  for b in range(0, 64, 7):
    np.testing.assert_array_equal(_bits(tl[b:b + 1].numpy()), _bits(_run(shim, p1[b], p2[b], cells[b:b + 1], A)[0]))
  # index_embedding stays usable on w1 as it is: its sum over the K rows, plus the bias row, is the pre-activation for K <= 2
  emb = observations.index_embedding(torch.from_numpy(clamped), torch.from_numpy(w1)).numpy()
  if K == 1:
    np.testing.assert_array_equal(_bits((w1[C + 1] + emb).astype(np.float32)), _bits(s))
  doc = observations.embedding_logits.__doc__ + observations.embedding_select.__doc__
  for word in ('[B, A]', 'rollout_embedding', 'index_embedding', 'clamped to [-1, C - 1]', 'never addcmul', 'lowest index wins'):
    assert word in doc, word
  src = inspect.getsource(observations.embedding_logits) + inspect.getsource(observations.embedding_select)
  assert 'addcmul' not in src.split('"""')[2] and 'matmul' not in src.split('"""')[2] and '@' not in src.split('"""')[2]


def test_ties_nan_infinities_and_signed_zeros(shim):
  nan, inf = np.float32('nan'), np.float32('inf')
  for K, A in ((1, 2), (2, 3)):
    C, H = 6, 5
    w1 = np.zeros((C + 2, H), np.float32)
    w2 = np.zeros((A, H + 1), np.float32)
    cells = np.array([[c] * K for c in range(-1, C)], np.int32)
    # all logits equal: the lowest index wins
    logits, action = _agree(shim, w1, w2, cells, A)
    assert (action == 0).all() and (logits == 0).all()
    # the last action strictly larger on cell 2 only
    w1[3, 0] = 1.0
    w2[A - 1, 0] = 1.0
    _, action = _agree(shim, w1, w2, cells, A)
    assert action[3] == A - 1 and (np.delete(action, 3) == 0).all()
    # a -0.0 pre-activation gives +0.0, a NaN pre-activation gives +0.0: the logits stay +0.0 + w2 * 0
    w1[:] = 0
    w1[C + 1, :] = -0.0
    w1[2, 1] = nan
    w2[:, :H] = 3.0
    logits, action = _agree(shim, w1, w2, cells, A)
    assert (action == 0).all() and (_bits(logits) == 0).all()
    # inf * 0: a NaN logit never wins, and a NaN l_0 is never beaten
    w2[:] = 0
    w2[1, 2] = inf                                                           # hidden unit 2 is 0 everywhere: l_1 = 0 + inf * 0 = NaN
    w2[A - 1, H] = -1.0
    logits, action = _agree(shim, w1, w2, cells, A)
    assert np.isnan(logits[:, 1]).all() and (action == 0).all()
    w2[:] = 0
    w2[0, 2] = inf                                                           # l_0 = NaN
    w2[1, H] = 5.0
    logits, action = _agree(shim, w1, w2, cells, A)
    assert np.isnan(logits[:, 0]).all() and (action == 0).all()
    # +inf pre-activation: relu keeps it; -inf gives 0
    w1[:] = 0
    w1[1, 0], w1[2, 0] = inf, -inf
    w2[:] = 0
    w2[1, 0] = 1.0
    logits, action = _agree(shim, w1, w2, cells, A)
    assert logits[1, 1] == inf and np.isnan(logits[1, 0]) and action[1] == 0              # (l_0 = 0 + 0 * inf: NaN, never beaten)
    assert (logits[2] == 0).all() and action[2] == 0
    w2[0, H] = -1.0
    w2[0, 0] = 1.0                                                           # l_0 = -1 + inf = inf too: the tie goes to 0
    logits, action = _agree(shim, w1, w2, cells, A)
    assert logits[1, 0] == inf and logits[1, 1] == inf and action[1] == 0 and action[2] == 1
    if K == 2:                                                                # inf + -inf across the two entries: NaN -> 0
      logits, action = _agree(shim, w1, w2, np.array([[0, 1], [1, 0]], np.int32), A)
      assert (logits[:, 1] == 0).all() and (logits[:, 0] == -1).all() and (action == 1).all()


def test_the_shim_runs_stand_alone_under_the_sanitizers(tmp_path):
  """bsx_embed.h with its own main under AddressSanitizer and UBSan, on the CPU: a program of its own, nothing loaded into
  python."""
  exe = str(tmp_path / 'embed_shim_main')
  cmd = GCC + ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DEMBED_SHIM_MAIN', SHIM, '-o', exe, '-lm']
  if subprocess.run(cmd, capture_output=True).returncode != 0:
    pytest.skip('this gcc has no sanitizer runtime')
  out = subprocess.run([exe], capture_output=True, text=True)
  assert out.returncode == 0, out
  seen = [int(x) for x in out.stdout.split()]
  assert len(seen) == 3 and sum(seen) == 2 * 3 * 64 and seen[2] > 0, out


@pytest.mark.parametrize('name', [c[0] for c in mu.CASES])
def test_the_weight_seeds_of_the_gpu_test_on_the_c_oracle(name):
  """The contract's greedy loop on the C oracle, with the shared pair of each case of the GPU test, at its lanes and seed: a
  fresh call of 11 steps and 11 more take every action on live steps and see pre-activations of both signs — so a kernel that
  always answers 0 cannot pass there.  The recorded seed is the first that does."""
  _, fam, kwargs, H = next(c for c in mu.CASES if c[0] == name)
  C, K, A = mu.geometry(fam, kwargs)
  assert 1 <= H <= 64 and (mu.staged_bytes(C, H) > mu.LDS_BYTES) == name.endswith('_global')
  assert mu.diverse(fam, kwargs, *mu.pair(C, A, H, mu.PAIR_SEED[name]))
  assert mu.first_good_seed(name) == mu.PAIR_SEED[name]
  acts, pre = mu.oracle_loop(fam, kwargs, *mu.pair(C, A, H, mu.PAIR_SEED[name]))
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
    assert list(p) == ['self', 'w1', 'w2', 'num_steps', 'policy_index', 'epsilon', 'explore_seed']
    assert [p[k].kind for k in ('policy_index', 'epsilon', 'explore_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
    assert p['policy_index'].default is None and p['epsilon'].default == 0.0 and p['explore_seed'].default == 0
    for env in _envs():                                                                               # every refusal first: the last
      env._device = torch.device('cpu')                                                               # one of the call allocates nothing
      _refused(env, name, explore_seed=-1, match='explore_seed must be')
      # the order, two faults at a time: the environment, the matrices, the population rule, epsilon, the seed
      idx = torch.zeros(4, dtype=torch.int32)
      _refused(env, name, w1=None, num_steps=0, match='num_steps')
      _refused(env, name, w1=None, policy_index=idx, match='w1 and w2 must be')
      _refused(env, name, policy_index=idx, epsilon=2.0, match='must be None')
      _refused(env, name, epsilon=2.0, explore_seed=-1, match='epsilon must be')
      env._logging = dict(steps=None)
      _refused(env, name, w1=None, num_steps=0, match='Logging')
  doc = base.Environment.rollout_embedding.__doc__
  for word in ('ts[t] = step(a); actions[t] = a', 'embedding_select', 'index_embedding', 'stream 2', 'rollout(actions)', 'policy_index',
               'cached per T', 'epsilon', 'explore_seed', '4-byte', 'rollout_policy', 'C + 2', 'H + 1', '1 <= H <= 64'):
    assert word in doc, word
  doc = base.Environment.evaluate_embedding.__doc__
  for word in ('rollout_embedding', 'PolicyEvaluation', 'evaluate_policy', 'float64'):
    assert word in doc, word
  abi = lambda cls, name: cls._closed_loop_abi(object.__new__(cls), name)                             # pylint: disable=protected-access
  for fam, cls in (('deep_sea', deep_sea.DeepSea), ('catch', catch.Catch)):
    assert abi(cls, 'rollout_embedding') == ROLLOUT[fam] and abi(cls, 'evaluate_embedding') == EVALUATE[fam]
    assert ROLLOUT[fam] in _native.EXPORTED and EVALUATE[fam] in _native.EXPORTED
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
      fn(object.__new__(cls), torch.zeros((6, 2)), torch.zeros((2, 3)), 4, epsilon=0.5, explore_seed=1)
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
      assert env._check_embedding(torch.zeros((C + 2, h)), torch.zeros((A, h + 1)), 4, None, 0.0, 0, name) == (1, h)   # pylint: disable=protected-access
    assert '1 <= H <= 64' in str(pytest.raises(ValueError, getattr(env, name), None, None, 4).value)
    _refused(env, name, policy_index=idx, match='must be None')
    _refused(env, name, w1=ok1.reshape(1, C + 2, H), w2=ok2.reshape(1, A, H + 1), policy_index=idx, match='must be None')   # [1, ...] is one pair
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, name, w1=pop1, w2=pop2, policy_index=bad, match='policy_index')
    for eps in (-0.1, 1.5, float('nan'), float('inf'), '0.1', None, True, [0.1]):
      _refused(env, name, epsilon=eps, match=rf'{name}: epsilon must be a number in \[0, 1\]')
    for seed in (-1, 1 << 64, 0.5, None, True, '3'):
      _refused(env, name, explore_seed=seed, match=rf'{name}: explore_seed must be an integer in \[0, 2\^64\)')
    for word in ('temperature', 'sample_seed'):                            # greedy: there is no temperature
      with pytest.raises(TypeError, match=word):
        getattr(env, name)(ok1, ok2, 4, **{word: 1})
    # the order: the matrices before the population rule, the population rule before epsilon and the seed
    _refused(env, name, w1=None, policy_index=idx, epsilon=2.0, match=msg)
    _refused(env, name, policy_index=idx, epsilon=2.0, match='must be None')
    _refused(env, name, epsilon=2.0, explore_seed=-1, match='epsilon')
    # views that start one float into a buffer pass the checks (only 4-byte alignment is assumed)
    v1 = torch.zeros((C + 2) * H + 1)[1:].reshape(C + 2, H)
    v2 = torch.zeros(A * (H + 1) + 1)[1:].reshape(A, H + 1)
    assert v1.is_contiguous() and v1.data_ptr() % 8 == 4 and v2.data_ptr() % 8 == 4
    assert env._check_embedding(v1, v2, 4, None, 1.0, (1 << 64) - 1, name) == (1, H)                  # pylint: disable=protected-access
    assert env._check_embedding(pop1, pop2, np.int64(7), idx, np.float32(0.5), np.int64(5), name) == (4, H)   # pylint: disable=protected-access
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
    for name, like, out_t, out_c in ((ROLLOUT[fam], f'bsx_{fam}_policy_rollout', 'bsx_timestep_t', _native.TimeStepPtrs),
                                     (EVALUATE[fam], f'bsx_{fam}_policy_evaluate', 'bsx_policy_eval_t', _native.PolicyEvalPtrs)):
      types = types_of(name)
      assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_policy_embedding_t*', 'int32_t*', out_t, 'double*']
      assert [t.replace('bsx_policy_embedding_t', 'bsx_policy_t') for t in types] == types_of(like)   # the signature of the tabular call
      assert name in _native.EXPORTED
      fn = getattr(_native.lib, name)
      assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.PolicyEmbedding), P, out_c, P]
      assert fn.restype is ctypes.c_int
      assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
      assert name in text, f'INTEGRATION.md does not describe {name}'
      assert 'extern "C" int ' + name + '(' in open(os.path.join(CSRC, fam + '.hip')).read()
  body = re.search(r'typedef struct \{([^}]*)\} bsx_policy_embedding_t;', plain).group(1)
  fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
  assert fields == ['const float* w1', 'const float* w2', 'int32_t n_cells, n_hidden, n_actions, n_policies', 'const int32_t* policy_index',
                    'double epsilon', 'uint64_t explore_seed', 'int32_t* actions_out']
  names = ['w1', 'w2', 'n_cells', 'n_hidden', 'n_actions', 'n_policies', 'policy_index', 'epsilon', 'explore_seed', 'actions_out']
  assert [f[0] for f in _native.PolicyEmbedding._fields_] == names                                      # pylint: disable=protected-access
  # the layout, against the C compiler's
  src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bsuite_amd.h"\nint main(void) { printf("%zu ' + '%zu ' * len(names) + '\\n", '
         'sizeof(bsx_policy_embedding_t), ' + ', '.join(f'offsetof(bsx_policy_embedding_t, {n})' for n in names) + '); return 0; }\n')
  with tempfile.TemporaryDirectory() as d:
    open(os.path.join(d, 'l.c'), 'w').write(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'l.c'), '-o', os.path.join(d, 'l')])
    got = [int(x) for x in subprocess.check_output([os.path.join(d, 'l')], text=True).split()]
  L = _native.PolicyEmbedding
  assert got == [ctypes.sizeof(L)] + [getattr(L, n).offset for n in names] == [64, 0, 8, 16, 20, 24, 28, 32, 40, 48, 56]
  note = header[header.index('fused closed loops from a hidden-layer policy on the index row'):header.index('} bsx_policy_embedding_t;')]
  for word in ('BSX_STREAM_POLICY', 'BSX_ERANGE', 'BSX_EALIGN', 'BSX_EINVAL', 'n_hidden outside [1, 64]', '4-byte aligned', 'n_actions',
               'clamped', 'v12, additive'):
    assert word in note, word


def _abi_case(fam):
  if fam == 'deep_sea':
    return _native.DeepSeaCfg(size=10, deterministic=1, move_cost=0.001, inv_size=0.1), 100, 2, _native.DeepSeaCfg(size=65)
  return _native.CatchCfg(10, 5), 50, 3, _native.CatchCfg(1, 5)


@pytest.mark.parametrize('kind', ['rollout', 'evaluate'])
@pytest.mark.parametrize('fam', ['deep_sea', 'catch'])
def test_argument_checks_of_the_entry_points(fam, kind):
  """Every refusal comes before any device work: garbage stands in for device pointers, none is dereferenced.  The codes and
  their order are those of bsx_<family>_policy_rollout / _policy_evaluate; a wrong n_cells or n_actions and an n_hidden outside
  [1, 64] are BSX_EINVAL where a wrong n_states is, an epsilon outside [0, 1] is BSX_ERANGE, and w1 or w2 off the 4-byte grid is
  BSX_EALIGN, after the pointers."""
  record = kind == 'rollout'
  fn = getattr(_native.lib, (ROLLOUT if record else EVALUATE)[fam])
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
    d = dict(w1=junk, w2=junk + 64, n_cells=C, n_hidden=5, n_actions=A, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0,
             actions_out=junk if record else None)
    d.update(kw)
    return _native.PolicyEmbedding(**d)

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
  # BSX_EMODE: the observation code, and everything the fused loop does not carry — before the scalars and epsilon
  for flags in (0, E.CALL_STATE_TAGGED, E.CALL_OBS_U8, E.CALL_OBS_INDEX | E.CALL_OBS_U8, E.CALL_OBS_INDEX | E.CALL_OBS_F16,
                E.CALL_OBS_INDEX | E.CALL_OBS_BF16):
    assert run(call(flags=flags), pol(n_cells=-1)) == E.BSX_EMODE, flags
    assert run(call(flags=flags), pol(epsilon=nan)) == E.BSX_EMODE, flags
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
  assert run(call(force_reset=1), pol(epsilon=2.0)) == E.BSX_EMODE
  assert run(call(action_ring=4), pol()) == E.BSX_EMODE
  # BSX_EINVAL: the scalars, before epsilon
  for n in (0, -1):
    assert run(call(n_steps=n), pol()) == E.BSX_EINVAL
    assert run(call(n_steps=n), pol(epsilon=-1.0)) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), pol(epsilon=inf)) == E.BSX_EINVAL
  for c_ in (C - 1, C + 1, C + 2, 0, -C):
    assert run(call(), pol(n_cells=c_)) == E.BSX_EINVAL, c_
  for a in (A - 1, A + 1, 5 - A, 0, -A, 1 << 20):                    # the other family's width among them
    assert run(call(), pol(n_actions=a)) == E.BSX_EINVAL, a
    assert run(call(), pol(n_actions=a, epsilon=nan)) == E.BSX_EINVAL, a
    assert run(call(n_lanes=0), pol(n_actions=a)) == E.BSX_EINVAL, a
  for h in (0, -1, 65, 1 << 20, -(1 << 31)):
    assert run(call(), pol(n_hidden=h)) == E.BSX_EINVAL, h
    assert run(call(), pol(n_hidden=h, epsilon=2.0)) == E.BSX_EINVAL, h
    assert run(call(n_lanes=0), pol(n_hidden=h)) == E.BSX_EINVAL, h
  for n in (0, -3):
    assert run(call(), pol(n_policies=n)) == E.BSX_EINVAL
    assert run(call(), pol(n_policies=n, epsilon=2.0)) == E.BSX_EINVAL
  # BSX_ERANGE: epsilon in [0, 1] — before an empty call returns and before any pointer is looked at
  for e in (-0.1, 1.5, nan, inf, -inf):
    assert run(call(), pol(epsilon=e)) == E.BSX_ERANGE, e
    assert run(call(n_lanes=0), pol(epsilon=e)) == E.BSX_ERANGE, e
    assert run(call(), pol(epsilon=e, w1=None), state=None) == E.BSX_ERANGE, e
  assert run(call(), pol(), cfg_=bad_cfg) == E.BSX_ERANGE
  assert run(call(flags=0), pol(), cfg_=bad_cfg) == E.BSX_ERANGE                             # (the cfg comes first)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at; both ends of H and of epsilon are accepted
  for h, e in ((1, 0.0), (64, 1.0)):
    assert run(call(n_lanes=0), pol(w1=None, w2=None, n_hidden=h, epsilon=e, actions_out=None), state=None,
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
def test_the_kernel_bodies_use_the_headers():
  dev = open(os.path.join(CSRC, 'bsx_embed_device.h')).read()

  def fn_text(kind, name):
    t = dev[dev.index(kind + ' ' + name + '('):]
    return t[:t.index('\n}\n')]

  best = fn_text('int', 'bsx_embed_best')
  for call_ in ('bsx_embed_row(cell[k], C)', 'bsx_embed_accumulate(l, w2j, bsx_mlp_relu(bsx_embed_preactivation(b[c], ek, K)), A)',
                'bsx_embed_accumulate(l, w2j, bsx_mlp_relu(bsx_embed_preactivation(gb[j], ek, K)), A)', 'bsx_embed_argmax(l, A)',
                '(bsx_embed_lds4)s_net', 'asm volatile("" : "+v"(l[a]))', 'float l[A];'):
    assert call_ in best, call_
  assert best.index('fn(st, cell[0], cell[1])') < best.index('if (p.in_lds != 0)') < best.index('} else {') < best.index('bsx_embed_argmax(')
  assert 'float h[' not in best and 'hidden[' not in best                                     # A accumulators, never H registers
  action = fn_text('int', 'bsx_embed_action')
  assert action.index('bsx_embed_best<K, A>(') < action.index('bsx_policy_draws(p.explore_seed, lane, step)') < action.index('bsx_policy_select(')
  assert 'if (p.epsilon > 0.0)' in action
  record, returns = fn_text('void', 'bsx_embed_record_body'), fn_text('void', 'bsx_embed_returns_body')
  for body in (record, returns):
    loop = body[body.index('for (int t = 0; t < n_steps; ++t) {'):]
    loop = loop[:loop.index('\n    }\n')]
    assert 'if (!resets) act = bsx_embed_action<F::K, F::A>(' in loop and 'Fam::resets(st)' in loop   # nothing computed or drawn on a reset
    assert loop.count('bsx_embed_view(ka)') == 1 and '__syncthreads' not in loop and 'atomic' not in loop
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
  assert 'bsx_embed_stand_in(' in dev and 'bsx_check_policy_call(call, &q,' in dev and 'bsx_check_policy_eval_call(call, &q,' in dev
  # no second statement of the rule outside bsx_embed.h
  for f in ('bsx_embed_device.h', 'embed.hip', 'deep_sea.hip', 'catch.hip'):
    text = re.sub(r'//.*', '', open(os.path.join(CSRC, f)).read())
    for word in ('l_best', '> 0.0f', 'l[a] +', 'l[a] = l[a]', '* h'):
      assert word not in text, (f, word)
  hip = open(os.path.join(CSRC, 'embed.hip')).read()
  assert hip.count('__global__') == 1
  assert '__global__ void __launch_bounds__(BSX_BLOCK) bsx_embed_kernel(const bsx_embed_args a)' in hip
  for inst in ('record_body<bsx_embed_deep_sea>', 'returns_body<bsx_embed_deep_sea>', 'record_body<bsx_embed_catch>', 'returns_body<bsx_embed_catch>'):
    assert 'bsx_embed_' + inst in hip, inst
  assert 's_net[BSX_EMBED_LDS_BYTES / 4]' in hip
  for f in ('linear.hip', 'mlp.hip', 'gumbel.hip', 'trajectory.hip', 'tab_sample.hip', 'drawn_returns.hip'):
    assert open(os.path.join(CSRC, f)).read().count('__global__') == 1, f
  # what paid for the kernel: one tagged kernel for the single-family groups of bandit and discounting_chain, its bodies the shared one
  sweep_hip = open(os.path.join(CSRC, 'sweep_mixed.hip')).read()
  assert '__global__ void __launch_bounds__(BSX_BLOCK) small_obs_duo_group_kernel(const small_obs_duo_group_args a)' in sweep_hip
  assert 'small_obs_group_body<bandit_env>(' in sweep_hip and 'small_obs_group_body<discounting_chain_env>(' in sweep_hip
  small = open(os.path.join(CSRC, 'small_obs.h')).read()
  assert 'if constexpr (small_obs_duo_group<Env>::value)' in small
  for f, env in (('bandit_env.h', 'bandit_env'), ('discounting_chain_env.h', 'discounting_chain_env')):
    assert f'struct small_obs_duo_group<{env}> {{ static constexpr bool value = true; }};' in open(os.path.join(CSRC, f)).read()


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position
from tests.test_tab_sample_host import _loops  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = 'bsx_embed_kernel'
FOLDED = 'small_obs_duo_group_kernel'


@needs_llvm
def test_product_library_has_the_one_new_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  assert [n for n in ks if 'embed' in n] == [NEW]                                             # ONE kernel for the four cases
  for word in ('index', 'policy', 'eval', 'gumbel', 'trajectory', 'linear', 'score', 'mlp', 'softmax', 'tab_sample', 'drawn_returns',
               'hot_cells', 'hot_stream_tiny', 'advance_group', 'advance_delta'):
    assert word not in NEW and word not in FOLDED, word
  assert not NEW.startswith(('calib_', 'mnist_')) and not FOLDED.startswith(('calib_', 'mnist_'))
  # what paid for it: the single-family groups of bandit and of discounting_chain are one kernel
  assert FOLDED in ks
  assert 'small_obs_group_kernel<bandit_env>' not in ks and 'small_obs_group_kernel<discounting_chain_env>' not in ks
  assert sorted(n for n in ks if n.startswith('small_obs_group_kernel<')) == sorted(
      f'small_obs_group_kernel<{e}>' for e in ('cartpole_env', 'memory_chain_env', 'mountain_car_env', 'umbrella_chain_env'))
  g = ks[FOLDED]
  assert g['private_segment_fixed_size'] == 0 and g['vgpr_spill_count'] == 0 and g['sgpr_spill_count'] == 0 and g['agpr_count'] == 0, g
  assert g['vgpr_count'] <= 128 and g['group_segment_fixed_size'] <= 1024, g
  for n in ('small_obs_mixed_group_kernel', 'sweep_phase0_kernel', 'bsx_tab_softmax_kernel', 'bsx_tab_eval_kernel', 'bsx_pair_advance_group_kernel',
            'bsx_policy_rollout_kernel<deep_sea_fam, deep_sea_hot>', 'bsx_policy_rollout_kernel<catch_fam, catch_hot>'):
    assert n in ks, n
  k = ks[NEW]
  print(NEW, {f: k[f] for f in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'kernarg_segment_size')})
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k      # no spill, no scratch
  assert k['agpr_count'] == 0 and k['vgpr_count'] <= 128, k
  assert mu.LDS_BYTES <= k['group_segment_fixed_size'] <= 16384, k                            # the pair, deep_sea's mapping, two counters


@needs_llvm
def test_the_loops_of_the_new_kernel():
  """The step loops are the loops that compute in float64 (the reward sums and the lane advance): four, one per branch.  Two of
  them — the returns-only branches — hold no store and no barrier; the other two hold the per-step stores, non-temporal.  No flat
  or scratch access anywhere in the kernel; an LDS and a global look-up of the matrices inside every step loop; no spill reload
  in any loop."""
  _, text = ki.kernel_text(os.path.join(CSRC, 'embed.hip'), NEW)
  loops, outside = _loops(text)
  everything = outside + [s for body in loops.values() for s in body]
  assert not any(s.startswith('flat_') or s.startswith('scratch_') for s in everything)
  assert any(s.startswith('ds_read_b128') for s in everything) and any(s.startswith('global_load_dword') for s in everything)
  is_store = lambda s: re.match(r'(global|flat|scratch|buffer)_store|ds_write|(global|ds)_atomic|ds_add', s)
  # a step loop is an outermost loop that holds the lane advance's float64 arithmetic, with the hidden-unit loops nested in it
  steps = {h: body for h, body in loops.items() if any(re.match(r'v_\w+_f64', s) for s in body)}
  print({h: len(b) for h, b in steps.items()})
  assert len(steps) >= 4, sorted(steps)
  assert not any(s.startswith('s_barrier') for body in steps.values() for s in body)
  returns = [h for h, body in steps.items() if not any(is_store(s) for s in body)]
  record = [h for h in steps if h not in returns]
  assert len(returns) >= 2 and len(record) >= 2, (returns, record)
  for h in record:
    stores = [s for s in steps[h] if s.startswith('global_store')]
    assert not any(re.match(r'ds_write|(global|ds)_atomic|ds_add', s) for s in steps[h]), h
    assert all(s.endswith(' nt') or s.startswith('global_store_dwordx2 ') for s in stores), stores
  assert sum(s.startswith('global_store') for s in outside) + sum(s.startswith('global_store') for h, b in loops.items() if h not in steps for s in b) >= 8
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
