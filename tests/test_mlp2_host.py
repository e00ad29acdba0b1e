"""CPU: evaluate_mlp2 / rollout_mlp2 (fused closed loops of cartpole, swing-up and mountain_car under a policy with two ReLU
hidden layers; bsx_<family>_mlp2_evaluate, bsx_<family>_mlp2_rollout) without a GPU — the rule the kernel compiles
(bsuite_amd/csrc/bsx_mlp2.h, through gcc) against a numpy float32 restatement with one rounding per operation and against
utils.observations.mlp2_select / mlp2_logits; every refusal of the two Python entry points with the native entry point
replaced by a trap; the C ABI's declarations, bindings, struct layout and error codes; and the built library: the kernel
budget, what paid for the new kernel, its resources and the instructions inside its loops."""
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
from bsuite_amd.environments import base, cartpole, catch, mountain_car
from bsuite_amd.utils import observations, wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bsuite_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
CALLS = ('evaluate', 'rollout')
ENTRY = {(fam, c): f'bsx_{fam}_mlp2_{c}' for fam in ('cartpole', 'mountain_car') for c in CALLS}
DIMS = [3, 6, 8]
WIDTHS = [(1, 1), (1, 64), (64, 1), (2, 3), (33, 7), (63, 64), (64, 64)]
_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------ bsx_mlp2_select, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('mlp2') / 'mlp2_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC',
                         os.path.join(ROOT, 'tests', 'csrc', 'mlp2_shim.c'), '-o', so])
  lib = ctypes.CDLL(so)
  P = ctypes.c_void_p
  lib.shim_mlp2.restype = None
  lib.shim_mlp2.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P, P, P, P, P, P]
  return lib


def _shim_run(lib, w1, w2, w3, o):
  """(best [n], logits [n, 3], s2 [n, H2]) of n cases, each with its own triple."""
  w1, w2, w3, o = (np.ascontiguousarray(x, np.float32) for x in (w1, w2, w3, o))
  n, H1, D1 = w1.shape
  H2 = w2.shape[1]
  assert w2.shape == (n, H2, H1 + 1) and w3.shape == (n, 3, H2 + 1) and o.shape == (n, D1 - 1)
  best, l, s2 = np.full(n, -1, np.int32), np.full((n, 3), 7.0, np.float32), np.full((n, H2), 7.0, np.float32)
  lib.shim_mlp2(n, D1 - 1, H1, H2, _ptr(w1), _ptr(w2), _ptr(w3), _ptr(o), _ptr(best), _ptr(l), _ptr(s2))
  return best, l, s2


def _restate(w1, w2, w3, o):
  """The rule in numpy float32, one rounding per operation, written from the issue's definition: (best, logits, s2)."""
  w1, w2, w3, o = (np.asarray(x, np.float32) for x in (w1, w2, w3, o))
  n, H1, D1 = w1.shape
  D, H2 = D1 - 1, w2.shape[1]
  with np.errstate(all='ignore'):
    s1 = w1[:, :, D].copy()
    for d in range(D):
      prod = (w1[:, :, d] * o[:, d:d + 1]).astype(np.float32)
      s1 = (s1 + prod).astype(np.float32)
    h1 = np.where(s1 > 0, s1, np.float32(0.0)).astype(np.float32)
    s2 = w2[:, :, H1].copy()
    for j in range(H1):
      prod = (w2[:, :, j] * h1[:, j:j + 1]).astype(np.float32)
      s2 = (s2 + prod).astype(np.float32)
    h2 = np.where(s2 > 0, s2, np.float32(0.0)).astype(np.float32)
    l = w3[:, :, H2].copy()
    for k in range(H2):
      prod = (w3[:, :, k] * h2[:, k:k + 1]).astype(np.float32)
      l = (l + prod).astype(np.float32)
    best, l_best = np.zeros(n, np.int32), l[:, 0].copy()
    for a in (1, 2):
      better = l[:, a] > l_best
      best, l_best = np.where(better, a, best).astype(np.int32), np.where(better, l[:, a], l_best)
  return best, l, s2


def _bits(x):
  return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _all_agree(shim, w1, w2, w3, o, what):
  """gcc's run of the header == numpy's restatement == the torch ops with per-lane matrices, bit for bit."""
  best, l, s2 = _shim_run(shim, w1, w2, w3, o)
  rb, rl, rs2 = _restate(w1, w2, w3, o)
  np.testing.assert_array_equal(_bits(s2), _bits(rs2), err_msg=f'{what}: s2')
  np.testing.assert_array_equal(_bits(l), _bits(rl), err_msg=f'{what}: logits')
  np.testing.assert_array_equal(best, rb, err_msg=f'{what}: best')
  t = [torch.from_numpy(np.ascontiguousarray(x, np.float32)) for x in (w1, w2, w3, o)]
  tl = observations.mlp2_logits(*t)
  tb, _, ts2 = observations.mlp2_select(*t, return_preactivations=True)
  assert torch.equal(tb, observations.mlp2_select(*t))
  assert tb.dtype is torch.int32 and tl.dtype is torch.float32
  np.testing.assert_array_equal(_bits(tl.numpy()), _bits(l), err_msg=f'{what}: torch logits')
  np.testing.assert_array_equal(_bits(ts2.numpy()), _bits(s2), err_msg=f'{what}: torch s2')
  np.testing.assert_array_equal(tb.numpy(), best, err_msg=f'{what}: torch best')
  return best, l, s2


def _random(rng, n, D, H1, H2, scale=1.0):
  return (rng.standard_normal((n, H1, D + 1)).astype(np.float32) * np.float32(scale),
          rng.standard_normal((n, H2, H1 + 1)).astype(np.float32) * np.float32(scale / np.sqrt(H1)),
          rng.standard_normal((n, 3, H2 + 1)).astype(np.float32) * np.float32(scale / np.sqrt(H2)),
          rng.standard_normal((n, D)).astype(np.float32))


def test_the_shim_compiles_the_kernels_header(shim):
  assert shim.shim_mlp2_triple_floats(8, 64, 64) == 64 * 9 + 64 * 65 + 3 * 65 == 4931
  text = open(os.path.join(CSRC, 'bsx_mlp2.h')).read()
  assert '#include "bsx_mlp.h"' in text and '__device__' not in text and 'hip' not in text.lower().replace('the hip kernel', '')
  for piece in ('bsx_mlp_hidden(', 'bsx_mlp_relu(', 'bsx_mlp_accumulate(', 'bsx_mlp_argmax('):      # built from bsx_mlp.h's pieces
    assert piece in text, piece
  assert 'l_best' not in text and '> 0.0f' not in text                     # no second statement of the ReLU or the argmax
  assert '#include "../../bsuite_amd/csrc/bsx_mlp2.h"' in open(os.path.join(ROOT, 'tests', 'csrc', 'mlp2_shim.c')).read()
  torso = open(os.path.join(CSRC, 'bsx_torso.h')).read()
  assert '#include "bsx_mlp2.h"' in torso and 'bsx_mlp2_accumulate(' in torso


@pytest.mark.parametrize('H1,H2', WIDTHS)
@pytest.mark.parametrize('D', DIMS)
def test_random_triples_per_lane_and_shared(shim, D, H1, H2):
  rng = np.random.default_rng(1000 * D + 10 * H1 + H2)
  n = 96
  w1, w2, w3, o = _random(rng, n, D, H1, H2)
  best, l, _ = _all_agree(shim, w1, w2, w3, o, (D, H1, H2, 'per lane'))
  if H1 > 1 and H2 > 1:
    assert set(best.tolist()) == {0, 1, 2}
  # one shared triple: 2-D tensors in torch, the same triple in every case of the shim
  k = 7
  shared = [np.broadcast_to(x[k], x.shape) for x in (w1, w2, w3)]
  sb, sl, _ = _all_agree(shim, *shared, o, (D, H1, H2, 'broadcast'))
  t = [torch.from_numpy(x[k].copy()) for x in (w1, w2, w3)]
  to = torch.from_numpy(o).reshape(n, 1, D)                                # [B, *obs_shape] is accepted as [B, D] is
  np.testing.assert_array_equal(_bits(observations.mlp2_logits(*t, to).numpy()), _bits(sl))
  np.testing.assert_array_equal(observations.mlp2_select(*t, to).numpy(), sb)
  assert (sb[k], _bits(sl[k]).tolist()) == (best[k], _bits(l[k]).tolist())


@pytest.mark.parametrize('H1,H2', WIDTHS)
@pytest.mark.parametrize('D', DIMS)
def test_special_pre_activations_in_either_layer_and_exact_ties(shim, D, H1, H2):
  """Pre-activations of +0.0, -0.0, NaN, +inf and -inf in layer 1 (through the bias of unit 0 under zero weights) and in layer
  2 (through the bias of unit 0, and through inf * 0), and logits that tie exactly."""
  rng = np.random.default_rng(7 * D + H1 + 100 * H2)
  specials = [0.0, -0.0, float('nan'), float('inf'), float('-inf')]
  cases, tags = [], []
  for layer in (1, 2):
    for v in specials:
      w1, w2, w3, o = (x[0] for x in _random(rng, 1, D, H1, H2))
      zero = np.float32(v) if v == 0 else np.float32(0.0)               # (-0.0 survives the sum only under products of -0.0)
      if layer == 1:
        w1[0, :D], w1[0, D], o = zero, v, np.abs(o)
      else:
        w2[0, :H1], w2[0, H1] = zero, v
      cases.append((w1, w2, w3, o)); tags.append((layer, v))
  # inf * 0: layer-1 unit 0 is off (a bias of -1 under zero weights) and meets an infinite weight in layer 2 -> a NaN s2,
  # h2 = 0; the same in layer 3: layer-2 unit 0 off under an infinite w3 -> a NaN logit
  w1, w2, w3, o = (x[0] for x in _random(rng, 1, D, H1, H2))
  w1[0, :D], w1[0, D], w2[0, 0] = 0.0, -1.0, float('inf')
  cases.append((w1, w2, w3, o)); tags.append('inf*0 in layer 2')
  w1, w2, w3, o = (x[0] for x in _random(rng, 1, D, H1, H2))
  w2[0, :H1], w2[0, H1], w3[1, 0] = 0.0, -1.0, float('inf')
  cases.append((w1, w2, w3, o)); tags.append('inf*0 in layer 3')
  # exact ties: equal rows of w3 (all three, then the last two above the first, then the first two above the last)
  for tie in ((0, 1, 2), (1, 2), (0, 1)):
    w1, w2, w3, o = (x[0] for x in _random(rng, 1, D, H1, H2))
    w3[:] = w3[0]
    if tie == (1, 2):
      w3[0, H2] -= 1.0
    elif tie == (0, 1):
      w3[2, H2] -= 1.0
    cases.append((w1, w2, w3, o)); tags.append(('tie', tie))
  stack = [np.stack([c[k] for c in cases]) for k in range(4)]
  best, l, s2 = _all_agree(shim, *stack, (D, H1, H2, 'special'))
  n_sp = len(specials)
  for i, v in enumerate(specials):                                        # layer 2: the pre-activation is the bias itself
    got = s2[n_sp + i, 0]
    assert (np.isnan(got) if np.isnan(v) else _bits(got) == _bits(np.float32(v))), (v, got)
  assert np.isnan(s2[2 * n_sp, 0])                                        # inf * 0
  assert np.isnan(l[2 * n_sp + 1, 1]) and best[2 * n_sp + 1] != 1         # a NaN logit never wins
  ties = best[2 * n_sp + 2:]
  assert ties.tolist() == [0, 1, 0], ties                                 # the lowest index wins a tie
  for row, tie in zip(l[2 * n_sp + 2:], ((0, 1, 2), (1, 2), (0, 1))):
    if not np.isnan(row).any():
      assert len({_bits(row[a]).item() for a in tie}) == 1


@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('H', [1, 5, 64])
def test_an_identity_second_layer_is_the_one_layer_rule(D, H):
  rng = np.random.default_rng(D + H)
  n = 64
  w1, _, w3, o = _random(rng, n, D, H, H)
  eye = np.concatenate([np.eye(H, dtype=np.float32), np.zeros((H, 1), np.float32)], 1)
  t1, t3, to = torch.from_numpy(w1), torch.from_numpy(w3), torch.from_numpy(o)
  two = observations.mlp2_logits(t1, torch.from_numpy(np.broadcast_to(eye, (n, H, H + 1)).copy()), t3, to)
  one = observations.mlp_logits(t1, t3, to)
  assert torch.equal(two.view(torch.int32), one.view(torch.int32))
  shared = observations.mlp2_logits(t1[3], torch.from_numpy(eye), t3[3], to)                        # 2-D matrices
  assert torch.equal(shared.view(torch.int32), observations.mlp_logits(t1[3], t3[3], to).view(torch.int32))
  assert torch.equal(observations.mlp2_select(t1, torch.from_numpy(eye).expand(n, -1, -1), t3, to), observations.mlp_select(t1, t3, to))


def test_the_shim_runs_stand_alone_under_the_sanitizers(tmp_path):
  san = ['gcc', '-O1', '-g', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all']
  probe = tmp_path / 'probe.c'
  probe.write_text('int main(void) { return 0; }\n')
  if subprocess.run(san + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode != 0:
    pytest.skip('this gcc has no sanitizer runtime')
  exe = str(tmp_path / 'mlp2_shim_main')
  # (the sanitizers are there: a failure to compile the shim itself is a failure)
  subprocess.check_call(san + ['-DMLP2_SHIM_MAIN', os.path.join(ROOT, 'tests', 'csrc', 'mlp2_shim.c'), '-o', exe])
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0 and r.stdout.strip() in ('0', '1', '2'), (r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------ the Python entry points
def _envs():
  return [cartpole.Cartpole(seed=0, batch=4), cartpole.CartpoleSwingup(seed=0, batch=4), mountain_car.MountainCar(seed=0, batch=4)]


def _dim(env):
  return int(np.prod(env.observation_spec().shape))


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


def _refused(env, call, exc=ValueError, match=None, **kw):
  """env.<call>_mlp2(...) raises, its message names the caller, and nothing was allocated."""
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  name = f'{call}_mlp2'
  H1, H2 = 5, 4
  obs = kw.pop('observation') if 'observation' in kw else torch.zeros((4, 3), dtype=torch.float32)
  pol = (kw.pop('w1') if 'w1' in kw else torch.zeros((H1, 4), dtype=torch.float32),
         kw.pop('w2') if 'w2' in kw else torch.zeros((H2, H1 + 1), dtype=torch.float32),
         kw.pop('w3') if 'w3' in kw else torch.zeros((3, H2 + 1), dtype=torch.float32))
  with pytest.raises(exc, match=match or name) as info:
    getattr(env, name)(*pol, obs, kw.pop('num_steps', 4), **kw)
  assert name in str(info.value)
  assert not raw._allocated and not raw._policy_rollout_out and raw._linear_eval_out is None      # pylint: disable=protected-access


def test_signatures_docstrings_and_families():
  want = ['self', 'w1', 'w2', 'w3', 'observation', 'num_steps', 'policy_index', 'epsilon', 'explore_seed']
  for call, sibling in (('evaluate', 'evaluate_mlp'), ('rollout', 'rollout_mlp')):
    fn = getattr(base.Environment, f'{call}_mlp2')
    p = inspect.signature(fn).parameters
    assert list(p) == want
    old = inspect.signature(getattr(base.Environment, sibling)).parameters
    assert [k for k in p if k != 'w3'] == list(old) and all(p[k] == old[k] for k in old)            # the sibling's, with w3
    assert [p[k].kind for k in ('policy_index', 'epsilon', 'explore_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
    for word in ('mlp2_select(w1[row], w2[row], w3[row], obs)', 'torch.cat([lin.weight, lin.bias[:, None]], 1)', 'torch.nn.Linear',
                 'policy_index', '1 <= H1, H2 <= 64', sibling):
      assert word in fn.__doc__, (call, word)
    abi = lambda cls: cls._closed_loop_abi(object.__new__(cls), f'{call}_mlp2')        # pylint: disable=protected-access,cell-var-from-loop
    assert abi(cartpole.Cartpole) == abi(cartpole.CartpoleSwingup) == ENTRY['cartpole', call]
    assert abi(mountain_car.MountainCar) == ENTRY['mountain_car', call] and ENTRY['cartpole', call] in _native.EXPORTED
    assert abi(base.Environment) is None and abi(catch.Catch) is None and ENTRY['mountain_car', call] in _native.EXPORTED
    for env in _envs():
      D = _dim(env)
      env._device = torch.device('cpu')
      good = dict(w1=torch.zeros((5, D + 1)), w2=torch.zeros((4, 6)), w3=torch.zeros((3, 5)), observation=torch.zeros((4, D)))
      # every refusal first: the last one of the arguments allocates nothing; and the order, two faults at a time
      _refused(env, call, match='must be None', policy_index=torch.zeros(4, dtype=torch.int32), **good)
      _refused(env, call, match='w3 must be', policy_index=torch.zeros(4, dtype=torch.int32), **dict(good, w3=None))
      _refused(env, call, match='observation must be', policy_index=torch.zeros(4, dtype=torch.int32), **dict(good, observation=None))
      # the refusals the three forms share are said in evaluate_mlp's words: the environment, the scalars, the rows, the population
      for kw in (dict(num_steps=0), dict(epsilon=2.0), dict(explore_seed=-1), dict(observation=None),
                 dict(policy_index=torch.zeros(4, dtype=torch.int32))):
        said = []
        for name, w in ((f'{call}_mlp2', (good['w1'], good['w2'], good['w3'])), (f'{call}_mlp', (good['w1'], torch.zeros((3, 6))))):
          args = {'observation': good['observation'], **kw}
          with pytest.raises(ValueError) as info:
            getattr(env, name)(*w, args.pop('observation'), args.pop('num_steps', 4), **args)
          said.append(str(info.value).replace(name, '').replace('triple', 'pair'))
        assert said[0] == said[1], kw
      # the slab comes after the arguments, for the recording call alone; the returns-only call goes on to allocate (never on 'meta')
      env._device = torch.device('meta')
      env._batch = -(-(1 << 32) // (4 * D))
      big = dict({k: torch.zeros(v.shape, device='meta') for k, v in good.items()}, observation=torch.zeros((env._batch, D), device='meta'))
      if call == 'rollout':
        _refused(env, call, match='must be None', policy_index=torch.zeros(env._batch, dtype=torch.int32, device='meta'), **big)
        _refused(env, call, match='4 GiB', **big)
      else:
        with pytest.raises(RuntimeError, match='no HIP device'):
          env.evaluate_mlp2(*big.values(), 4)
        assert not env._allocated and env._linear_eval_out is None and not env._policy_rollout_out
  assert list(inspect.signature(observations.mlp2_logits).parameters) == ['w1', 'w2', 'w3', 'obs']
  assert list(inspect.signature(observations.mlp2_select).parameters) == ['w1', 'w2', 'w3', 'obs', 'return_preactivations']
  assert 'torch.cat([lin.weight, lin.bias[:, None]], 1)' in observations.mlp2_logits.__doc__


@pytest.mark.parametrize('call', CALLS)
def test_views_families_and_modes_are_refused(call, trap):
  for env in (cartpole.Cartpole(seed=0), cartpole.CartpoleSwingup(seed=0), mountain_car.MountainCar(seed=0)):
    _refused(env, call, match='batched view')
  for bsuite_id in ('bandit/0', 'deep_sea/0', 'catch/0', 'memory_len/0', 'umbrella_length/0', 'discounting_chain/0'):
    _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), call, match='mountain_car only')
  for cls in (cartpole.Cartpole, cartpole.CartpoleSwingup, mountain_car.MountainCar):
    _refused(cls(seed=0, batch=4, rng='mt19937'), call, match='philox')
  for env in _envs():
    env._logging = dict(steps=None)             # what enable_logging() leaves behind (it allocates: not without a GPU)
    _refused(env, call, match='Logging')
  for env in _envs():
    env._grouped_by = object()                  # what SweepBatch sets while its prepared groups hold the column pointers
    _refused(env, call, exc=RuntimeError, match='release_groups')


def test_a_slab_of_4_gib_is_refused_by_the_recording_call_alone(trap):
  for env in _envs():
    D = _dim(env)
    env._device = torch.device('cpu')
    env._batch = 4
    ok = dict(w1=torch.zeros((5, D + 1)), observation=torch.zeros((4, D)))
    env._check_evaluate_mlp2(ok['w1'], torch.zeros((4, 6)), torch.zeros((3, 5)), ok['observation'], 4, None, 0.0, 0,
                             what='rollout_mlp2')                         # pylint: disable=protected-access
    env._batch = -(-(1 << 32) // (4 * D))                                  # the first batch whose [B, D] slab reaches 4 GiB
    with pytest.raises(ValueError, match='rollout_mlp2: .* 4 GiB'):
      env._check_trajectory_slab('rollout_mlp2')                           # pylint: disable=protected-access
    # the whole method: the slab is the last refusal, after the arguments', before anything is allocated
    big = torch.zeros((1, D)).expand(env._batch, D)                        # (not contiguous: refused first, as an argument)
    with pytest.raises(ValueError, match='rollout_mlp2: observation must be'):
      env.rollout_mlp2(ok['w1'], torch.zeros((4, 6)), torch.zeros((3, 5)), big, 4)
    meta = [torch.zeros(shape, device='meta') for shape in ((5, D + 1), (4, 6), (3, 5), (env._batch, D))]
    env._device = torch.device('meta')
    with pytest.raises(ValueError, match='rollout_mlp2: .* 4 GiB'):
      env.rollout_mlp2(*meta, 4)
    with pytest.raises(RuntimeError, match='no HIP device'):               # evaluate mode writes no slab: it goes on to allocate
      env.evaluate_mlp2(*meta, 4)                                          # (never on 'meta')
    env._device = torch.device('cpu')
    env._batch -= 1
    env._check_trajectory_slab('rollout_mlp2')                             # pylint: disable=protected-access
    assert not env._allocated                                              # pylint: disable=protected-access


@pytest.mark.parametrize('call', CALLS)
def test_the_wrappers_refuse_instead_of_delegating(call, trap):
  name = f'{call}_mlp2'
  for make in (lambda e: wrappers.RewardNoise(e, noise_scale=0.5, seed=1), lambda e: wrappers.RewardScale(e, reward_scale=2.0)):
    for raw in _envs():
      _refused(make(raw), call, match='not available through')
      _refused(raw, call, match='reward wrapper')                         # ... and the raw environment knows it is wrapped
  for bsuite_id in ('cartpole_noise/2', 'cartpole_scale/4', 'mountain_car_noise/3', 'mountain_car_scale/1'):
    env = bsuite_amd.load_from_id(bsuite_id, batch=4)
    assert hasattr(env, 'raw_env'), bsuite_id
    _refused(env, call, match='not available through')
  for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    fn = getattr(cls, name)
    assert fn is not getattr(base.Environment, name) and any(name in vars(c) for c in cls.__mro__[:-1]), cls
    with pytest.raises(ValueError, match=name):
      fn(object.__new__(cls), torch.zeros((5, 4)), torch.zeros((4, 6)), torch.zeros((3, 5)), torch.zeros((4, 3)), 4)
  image = wrappers.ImageObservation(mountain_car.MountainCar(seed=0, batch=4), (84, 84, 1))
  _refused(image, call, match='not available through ImageObservation')


@pytest.mark.parametrize('call', CALLS)
def test_arguments_are_checked_before_any_gpu_use(call, trap):
  name = f'{call}_mlp2'
  for env in _envs():
    env._device = torch.device('cpu')           # the checks themselves, on host tensors: dtype, shape, contiguity
    D, H1, H2 = _dim(env), 5, 4
    w1, w2, w3 = torch.zeros((H1, D + 1)), torch.zeros((H2, H1 + 1)), torch.zeros((3, H2 + 1))
    p1, p2, p3 = torch.zeros((4, H1, D + 1)), torch.zeros((4, H2, H1 + 1)), torch.zeros((4, 3, H2 + 1))
    obs = torch.zeros((4, 1, D), dtype=torch.float32)
    idx = torch.zeros(4, dtype=torch.int32)
    ok, pop = dict(w1=w1, w2=w2, w3=w3), dict(w1=p1, w2=p2, w3=p3)
    for eps in (-0.1, 1.5, float('nan'), float('inf'), '0.1', None, True):
      _refused(env, call, epsilon=eps, observation=obs, match=f'{name}: epsilon', **ok)
    for n in (0, -1, 2.0, None, '4', True):
      _refused(env, call, num_steps=n, observation=obs, match=f'{name}: num_steps', **ok)
    for seed in (-1, 1 << 64, 0.5, None):
      _refused(env, call, explore_seed=seed, observation=obs, match=f'{name}: explore_seed', **ok)
    for bad in (obs.to(torch.float64), obs.numpy(), torch.zeros((4, D + 1)), torch.zeros((3, 1, D)), torch.zeros(4 * D),
                torch.zeros((4, 2 * D))[:, ::2], None):
      _refused(env, call, observation=bad, match=f'{name}: observation must be', **ok)
    _refused(env, call, observation=torch.zeros((4, D)), policy_index=idx, match='must be None', **ok)      # policy_index with one triple
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, call, observation=obs, policy_index=bad, match='policy_index', **pop)
    # a wrong H, dtype, contiguity or rank in any of the three matrices
    for bad in (w1.to(torch.float64), w1.numpy(), torch.zeros((H1, D)), torch.zeros((0, D + 1)), torch.zeros((65, D + 1)),
                torch.zeros((H1, 2 * (D + 1)))[:, ::2], torch.zeros((H1 * (D + 1),)), None):
      _refused(env, call, w1=bad, w2=w2, w3=w3, observation=obs, match=f'{name}: w1 must be')
    for bad in (w2.to(torch.float64), w2.numpy(), torch.zeros((H2, H1)), torch.zeros((H2, H1 + 2)), torch.zeros((0, H1 + 1)),
                torch.zeros((65, H1 + 1)), torch.zeros((H2, 2 * (H1 + 1)))[:, ::2], torch.zeros((1, H2, H1 + 1)), None):
      _refused(env, call, w1=w1, w2=bad, w3=w3, observation=obs, match=f'{name}: w2 must be')
    for bad in (w3.to(torch.float64), w3.numpy(), torch.zeros((3, H2)), torch.zeros((3, H2 + 2)), torch.zeros((2, H2 + 1)),
                torch.zeros((3, 2 * (H2 + 1)))[:, ::2], torch.zeros((1, 3, H2 + 1)), None):
      _refused(env, call, w1=w1, w2=w2, w3=bad, observation=obs, match=f'{name}: w3 must be')
    # mixed 2-D and 3-D matrices, unequal P
    _refused(env, call, w1=p1, w2=w2, w3=p3, observation=obs, policy_index=idx, match=f'{name}: w2 must be')
    _refused(env, call, w1=p1, w2=p2, w3=w3, observation=obs, policy_index=idx, match=f'{name}: w3 must be')
    _refused(env, call, w1=w1, w2=p2, w3=w3, observation=obs, match=f'{name}: w2 must be')
    _refused(env, call, w1=p1, w2=torch.zeros((3, H2, H1 + 1)), w3=p3, observation=obs, policy_index=idx, match=f'{name}: w2 must be')
    _refused(env, call, w1=p1, w2=p2, w3=torch.zeros((5, 3, H2 + 1)), observation=obs, policy_index=idx, match=f'{name}: w3 must be')
    assert not env._allocated                                              # pylint: disable=protected-access
  # host tensors for an environment on the GPU: the device
  env = mountain_car.MountainCar(seed=0, batch=4)
  _refused(env, call, observation=torch.zeros((4, 1, 3)), match='w1 must be')


# ------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_export_and_layout_agree_and_the_abi_stays_v12(tmp_path):
  header = open(HEADER).read()
  assert re.search(r'#define BSX_ABI_VERSION 12\b', header)
  assert _native.ABI_VERSION == 12 and _native.lib.bsx_abi_version() == 12
  plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  out = subprocess.check_output(['nm', '-D', '--defined-only', _native.SO_PATH], text=True)
  P = ctypes.c_void_p
  text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for (fam, call), name in ENTRY.items():
    decl = re.search(r'int ' + name + r'\(([^;]*)\);', plain)
    assert decl, f'include/bsuite_amd.h does not declare {name}'
    types = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(decl.group(1).split()).split(',')]
    tail = ['bsx_linear_eval_t', 'double*'] if call == 'evaluate' else ['bsx_timestep_t', 'int32_t*', 'double*']
    assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_mlp2_t*', 'float*', 'int32_t*'] + tail
    assert name in _native.EXPORTED
    fn = getattr(_native.lib, name)
    cfg = dict(cartpole=_native.CartpoleCfg, mountain_car=_native.MountainCarCfg)[fam]
    outs = [_native.LinearEvalPtrs, P] if call == 'evaluate' else [_native.TimeStepPtrs, P, P]
    assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.Mlp2), P, P] + outs
    assert fn.restype is ctypes.c_int
    assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
    assert 'extern "C" int ' + name + '(' in open(os.path.join(CSRC, fam + '.hip')).read()
    assert name in text, f'INTEGRATION.md does not describe {name}'
  # the header states the definition
  note = header[header.index('two hidden layers: the greedy evaluation'):header.index('} bsx_mlp2_t;')]
  for word in ('s2_k = w2[k][H1]', 'j ascending', 'no FMA', 'torch.nn.Linear', 'hidden1 or hidden2 outside [1, 64]', 'BSX_ENULL also for w3',
               'csrc/bsx_mlp2.h'):
    assert word in note, word
  # the older structs are untouched, the new one is laid out as gcc lays it out
  assert ctypes.sizeof(_native.Linear) == 48 and ctypes.sizeof(_native.Mlp) == 56
  fields = [f[0] for f in _native.Mlp2._fields_]                           # pylint: disable=protected-access
  assert fields == ['w1', 'w2', 'w3', 'hidden1', 'hidden2', 'n_policies', 'policy_index', 'epsilon', 'explore_seed', 'observation_in']
  src = tmp_path / 'layout.c'
  src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bsuite_amd.h"\nint main(void) {\n  printf("%zu", sizeof(bsx_mlp2_t));\n'
                 + ''.join(f'  printf(" %zu", offsetof(bsx_mlp2_t, {f}));\n' for f in fields) + '  return 0;\n}\n')
  exe = str(tmp_path / 'layout')
  subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', exe])
  got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
  assert got == [ctypes.sizeof(_native.Mlp2)] + [getattr(_native.Mlp2, f).offset for f in fields], got
  assert got[0] == 72


def _abi_case(fam):
  if fam == 'mountain_car':
    return _native.MountainCarCfg(1000, 0), _native.MountainCarCfg(0, 0)
  good = dict(swingup=0, last_step=1001, height_threshold=0.8, x_threshold=3.0, theta_dot_threshold=1.0, x_reward_threshold=1.0,
              timescale=0.01, mass_cart=1.0, mass_pole=0.1, length=0.5, force_mag=10.0, gravity=9.8, move_cost=0.0, init_range=0.05,
              theta_offset=0.0, time_frac=0xDEAD0008)
  return _native.CartpoleCfg(**good), _native.CartpoleCfg(**dict(good, last_step=0))


@pytest.mark.parametrize('call_', CALLS)
@pytest.mark.parametrize('fam', ['cartpole', 'mountain_car'])
def test_argument_checks_of_the_entry_points(fam, call_):
  """Every refusal comes before any device work: garbage stands in for device pointers, none is dereferenced.  The codes and
  their order are those of bsx_<family>_mlp_evaluate / _mlp_rollout: null structs, the cfg, modes, scalars, pointers, the slab."""
  fn = getattr(_native.lib, ENTRY[fam, call_])
  cfg, bad_cfg = _abi_case(fam)
  junk = 0xDEAD0010                                                # never mapped: a dereference would fault (16-byte aligned)
  E = _native
  D = 3 if fam == 'mountain_car' else 6
  record = call_ == 'rollout'

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

  def run(c, q, state=junk, steps=junk, out=None, actions=junk, info=junk, cfg_=cfg):
    if record:
      out = (_native.TimeStepPtrs(junk, junk, junk, junk) if out is None else out, actions)
    else:
      out = (_native.LinearEvalPtrs(junk, junk, junk, junk) if out is None else out,)
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, state, steps, *out, info)

  # null structs
  assert run(call(), policy(), cfg_=None) == E.BSX_ENULL
  assert run(None, policy()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: before the scalars
  for flags in (E.CALL_OBS_INDEX, E.CALL_OBS_U8, E.CALL_OBS_F16, E.CALL_OBS_BF16, E.CALL_OBS_INDEX | E.CALL_OBS_U8):
    assert run(call(flags=flags), policy(n_policies=-1, hidden1=0)) == E.BSX_EMODE, flags
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
  assert run(call(force_reset=1), policy()) == E.BSX_EMODE
  assert run(call(action_ring=4), policy()) == E.BSX_EMODE
  # BSX_EINVAL / BSX_ERANGE: the scalars; hidden1 / hidden2 where bsx_mlp_t's hidden is
  for n in (0, -1):
    assert run(call(n_steps=n), policy()) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), policy()) == E.BSX_EINVAL
  for which in ('hidden1', 'hidden2'):
    for h in (0, -1, 65, 1 << 20):
      assert run(call(), policy(**{which: h})) == E.BSX_EINVAL, (which, h)
      assert run(call(), policy(**{which: h}, epsilon=2.0)) == E.BSX_EINVAL, (which, h)         # before epsilon
      assert run(call(n_lanes=0), policy(**{which: h})) == E.BSX_EINVAL, (which, h)
    for h in (1, 64):
      assert run(call(n_lanes=0), policy(**{which: h})) == 0
  for n in (0, -3):
    assert run(call(), policy(n_policies=n)) == E.BSX_EINVAL
  for eps in (-1e-9, 1.0000001, float('nan'), float('inf')):
    assert run(call(), policy(epsilon=eps)) == E.BSX_ERANGE, eps
  assert run(call(), policy(), cfg_=bad_cfg) == E.BSX_ERANGE
  assert run(call(flags=E.CALL_OBS_INDEX), policy(), cfg_=bad_cfg) == E.BSX_ERANGE              # (the cfg comes first)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at
  none = {k: None for k in ('w1', 'w2', 'w3', 'observation_in')}
  empty = _native.TimeStepPtrs(0, 0, 0, 0) if record else _native.LinearEvalPtrs(0, 0, 0, 0)
  assert run(call(n_lanes=0), policy(**none), state=None, steps=None, out=empty, actions=None, info=None) == 0
  assert run(call(n_lanes=0), policy(epsilon=2.0)) == E.BSX_ERANGE                              # ... but the scalars are
  # BSX_ENULL: every pointer — the other ones garbage; w3 is one more required pointer
  for missing in none:
    assert run(call(), policy(**{missing: None})) == E.BSX_ENULL, missing
  for missing in ('state', 'steps', 'info'):
    assert run(call(), policy(), **{missing: None}) == E.BSX_ENULL, missing
  for k in range(4):                                                                            # every output pointer
    ptrs = [junk] * 4
    ptrs[k] = 0
    assert run(call(), policy(), out=(_native.TimeStepPtrs if record else _native.LinearEvalPtrs)(*ptrs)) == E.BSX_ENULL, k
  if record:
    assert run(call(), policy(), actions=None) == E.BSX_ENULL
  assert run(call(), policy(n_policies=2)) == E.BSX_ENULL                                       # a population without policy_index
  if fam == 'cartpole':
    no_table = _abi_case(fam)[0]
    no_table.time_frac = None
    assert run(call(), policy(), cfg_=no_table) == E.BSX_ENULL
  assert run(call(n_lanes=1 << 40), policy()) == E.BSX_EINVAL                                   # more workgroups than a grid holds
  assert run(call(action_ring=-2), policy()) == E.BSX_EINVAL
  if record:
    # what only a call that writes [T,B] slabs refuses: a slab the 32-bit lane offsets cannot span
    assert run(call(n_lanes=-(-(1 << 32) // (4 * D))), policy()) == E.BSX_EINVAL
    assert run(call(n_lanes=1 << 31), policy()) == E.BSX_EINVAL


# ------------------------------------------------------------------------------------------ the source text
def test_the_kernel_body_uses_the_helpers():
  dev = open(os.path.join(CSRC, 'bsx_torso.h')).read()
  body = dev[dev.index('void bsx_torso_body('):]
  body = body[:body.index('\n}\n')]
  walk = dev[dev.index('int32_t bsx_torso_action('):]
  walk = walk[:walk.index('\n}\n')]
  for call_ in ('bsx_torso_action_of<D>(', 'bsx_policy_draws(p.explore_seed, lane, step)', 'bsx_policy_clamp(k0.p.policy_index[i], k0.p.n_policies)',
                'bsx_policy_select(', 'Env::reset_pending(rg)', 'bsx_pool_counts(', 'Env::template core<0, 0, true, false, false, V, true>(',
                'Env::template load_info<V>(', 'Env::template store_info<V>(', 'bsx_fresh(0u)', 'bsx_torso_view(ka)', 'bsx_eval_accumulate(&e, type, reward)',
                'bsx_emit_values<0, 0, false, 0>(', 'bsx_trajectory_store_row<D>(', 'small_rollout_nt_scalars<Env>::value',
                'bsx_st<BSX_OUT_SCALARS.rollout>(bsx_at_off(kt.actions_out'):
    assert call_ in body, call_
  for piece in ('bsx_mlp_hidden(', 'bsx_mlp2_accumulate(', 'bsx_mlp_relu(', 'bsx_mlp_accumulate(', 'bsx_mlp_argmax('):
    assert piece in walk, piece
  assert '#pragma unroll 1\n  for (int j = 0; j < H1; ++j)' in walk
  loop = body[body.index('for (int t = 0; t < n_steps; ++t) {'):]
  loop = loop[:loop.index('\n    }\n')]
  for word in ('__syncthreads', 'atomic', 's_w[', 'Env::store', 'store_info', 'observation_in', 'bsx_pool_counts'):
    assert word not in loop, word
  for word in ('__syncthreads', 'atomic', 'bsx_st<', 's_w['):
    assert word not in walk, word
  assert body.count('bsx_torso_view(ka)') == 4 and loop.count('bsx_torso_view(ka)') == 1
  for f in ('bsx_torso.h', 'torso.hip'):                                   # no second statement of the rules
    text = open(os.path.join(CSRC, f)).read()
    assert 'l_best' not in text and '> 0.0f' not in text, f
  hip = open(os.path.join(CSRC, 'torso.hip')).read()
  assert hip.count('__global__') == 1
  assert '__global__ void __launch_bounds__(BSX_BLOCK) bsx_torso_kernel(const bsx_torso_args a)' in hip
  assert 'extern __shared__' in hip                                        # the shared triple: dynamic LDS, sized by the launch
  for inst in ('<Fam, V, true, true>', '<Fam, V, false, true>', '<Fam, V, true, false>', '<Fam, V, false, false>'):
    assert 'bsx_torso_body' + inst in hip, inst
  assert open(os.path.join(CSRC, 'linear.hip')).read().count('__global__') == 1
  assert open(os.path.join(CSRC, 'mlp.hip')).read().count('__global__') == 1
  assert 'int32_t mode;' in dev and 'BSX_TORSO_GREEDY' in dev              # room for the drawn actions
  # what paid for the kernel: deep_sea's two wrapped lane advances are one kernel with a uniform switch over the two bodies
  host = open(os.path.join(CSRC, 'bsx_pair_host.h')).read()
  assert 'else if constexpr (Fam::ADVANCE_WITHOUT_MT)' in host
  assert 'ADVANCE_WITHOUT_MT = false' in open(os.path.join(CSRC, 'deep_sea_fam.h')).read()
  assert 'ADVANCE_WITHOUT_MT = true' in open(os.path.join(CSRC, 'catch_fam.h')).read()
  pair = open(os.path.join(CSRC, 'bsx_pair_device.h')).read()
  kern = pair[pair.index('bsx_advance_kernel(const typename Fam::args a) {'):]
  kern = kern[:kern.index('\n}\n')]
  assert 'if constexpr (!LEAN && MT == -1 && !Fam::ADVANCE_WITHOUT_MT)' in kern
  assert 'if (a.ctl.mt_state == nullptr) bsx_advance_body<Fam, false, 0>(' in kern and 'else bsx_advance_body<Fam, false, -1>(' in kern


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = 'bsx_torso_kernel'
FORBIDDEN = ('mlp', 'linear', 'score', 'eval', 'policy', 'index', 'embed', 'gumbel', 'softmax', 'tab_sample', 'trajectory',
             'drawn_returns', 'lambda_scan', 'hot_cells', 'advance_group', 'advance_delta')


@needs_llvm
def test_product_library_has_the_one_new_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  assert [n for n in ks if 'torso' in n] == [NEW]                        # ONE kernel for the twelve cases
  assert not any(w in NEW for w in FORBIDDEN)
  # what paid for it: deep_sea's wrapped lane advance without the MT19937 generators is no kernel of its own any more but
  # one of the two bodies of <deep_sea_fam, false, -1>, behind a uniform switch; catch keeps all three of its kernels
  assert 'bsx_advance_kernel<deep_sea_fam, false, 0>' not in ks
  assert 'bsx_advance_kernel<deep_sea_fam, false, -1>' in ks and 'bsx_advance_kernel<deep_sea_fam, true, -1>' in ks
  for mt in ('true, -1', 'false, -1', 'false, 0'):
    assert f'bsx_advance_kernel<catch_fam, {mt}>' in ks, mt
  folded = ks['bsx_advance_kernel<deep_sea_fam, false, -1>']
  assert folded['vgpr_count'] <= 64 and folded['vgpr_spill_count'] == 0 and folded['sgpr_spill_count'] == 0, folded   # full occupancy
  assert folded['private_segment_fixed_size'] == 0, folded
  k = ks[NEW]
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
  assert k['agpr_count'] == 0, k
  assert k['group_segment_fixed_size'] <= 16 * 1024, k                     # static; the shared triple is dynamic, <= 19,984 bytes
  # 64 layer-2 accumulators beside the closed loop's registers.  gfx950 allocates vector registers in granules of 8 out of
  # 512 per SIMD lane: 168 is the last count at which three waves fit a SIMD (3 * 168 = 504); 169 would leave two.
  assert k['vgpr_count'] <= 168, k


@needs_llvm
def test_nothing_that_waits_inside_the_loops_of_the_new_kernel():
  """Inside ANY loop of the kernel (the compiler marks a loop's blocks in its block comments): no barrier, no atomic, no LDS
  write, no scratch access and no spill reload; the shared branches read LDS there, 16 bytes at a time, and the recording
  branches store."""
  _, text = ki.kernel_text(os.path.join(CSRC, 'torso.hip'), NEW)
  in_loop, in_walk, inside, walk, outer, inner = False, False, [], [], 0, 0
  for l in text:
    if re.match(r'^\.LBB\d+_\d+:', l) or l.startswith('; %bb.'):
      in_loop, in_walk = 'Loop' in l, 'Depth=2' in l
      outer += 'Loop Header' in l and 'Depth=1' in l
      continue
    if 'Loop Header' in l:                                                  # (a header comment on a line of its own)
      inner += 'Depth=2' in l
      in_walk = in_walk or 'Depth=2' in l
      continue
    s = l.strip()
    if in_loop and s and not s.startswith(';') and not s.startswith('.'):
      inside.append(s)
      if in_walk:
        walk.append(s)
  assert outer >= 12 and inner >= 12 * 3, (outer, inner)                   # twelve step loops, three widths of the walk in each
  bad = [s for s in inside if re.match(r'flat_|scratch_|buffer_|(global|ds)_atomic|ds_write|ds_add|ds_\w*rtn|s_barrier', s)]
  assert not bad, bad[:8]
  # the walk over the hidden units (the loops of depth 2): the shared triple is read 16 bytes at a time, and no multiply is
  # fused with its add (the physics' own polynomials, outside the walk, are written with fma)
  assert sum(s.startswith('ds_read_b128') for s in walk) >= 6 * 3 * 4, 'the shared triple is read 16 bytes at a time inside the walk'
  assert not any(re.match(r'v_(pk_)?(fma|fmac|mad|mac)_f32', s) for s in walk)
  assert any(s.startswith('v_pk_mul_f32') for s in walk) and any(s.startswith('v_pk_add_f32') for s in walk)
  stores = [s for s in inside if s.startswith('global_store')]
  assert len(stores) >= 6 * 5, len(stores)                                 # six recording branches x five outputs
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
  assert not any('v_readlane' in s or 'v_writelane' in s for s in walk)
