"""CPU: evaluate_mlp (fused hidden-layer policy evaluation of cartpole, swing-up and mountain_car; bsx_<family>_mlp_evaluate)
without a GPU — the rule the kernel compiles (bsx_mlp_select and its pieces in bsuite_amd/csrc/bsx_mlp.h, through gcc)
against a numpy float32 restatement with one rounding per operation and against utils.observations.mlp_select; every refusal
of the Python entry point, all before any GPU use; the C ABI's declaration / binding / export and argument checks; and the
kernel budget: ONE new kernel, paid for by the two one-float-per-thread board writers that became one, inside the resource
conditions, with no store, no LDS write, no atomic, no barrier and no spill reload inside any of its loops."""
import ctypes
import fractions
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
ENTRY = dict(cartpole='bsx_cartpole_mlp_evaluate', mountain_car='bsx_mountain_car_mlp_evaluate')
DIMS = [3, 6, 8]
HIDDEN = [1, 5, 64]


# ------------------------------------------------------------------------------------------ bsx_mlp_select, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('mlp') / 'mlp_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC',
                         os.path.join(ROOT, 'tests', 'csrc', 'mlp_shim.c'), '-o', so])
  lib = ctypes.CDLL(so)
  P = ctypes.c_void_p
  lib.shim_mlp_select.restype = None
  lib.shim_mlp_select.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, P, P, P, P]
  lib.shim_mlp_hidden.restype = None
  lib.shim_mlp_hidden.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, P, P, P, P]
  lib.shim_mlp_relu.restype = None
  lib.shim_mlp_relu.argtypes = [ctypes.c_int64, P, P]
  return lib


_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _shim_run(lib, w1, w2, o):
  """(best [n], s [n, H], h [n, H]) of n cases, each with its own pair."""
  w1, w2, o = (np.ascontiguousarray(x, np.float32) for x in (w1, w2, o))
  n, H, D1 = w1.shape
  assert w2.shape == (n, 3, H + 1) and o.shape == (n, D1 - 1)
  best = np.full(n, -1, np.int32)
  s, h = np.full((n, H), 7.0, np.float32), np.full((n, H), 7.0, np.float32)
  lib.shim_mlp_select(n, D1 - 1, H, _ptr(w1), _ptr(w2), _ptr(o), _ptr(best))
  lib.shim_mlp_hidden(n, D1 - 1, H, _ptr(w1), _ptr(o), _ptr(s), _ptr(h))
  return best, s, h


def _round_f32(x):
  """A rational rounded to the nearest float32, ties to even (values well inside the normal range)."""
  if x == 0:
    return np.float32(0.0)
  f = np.float32(float(x))                          # float(Fraction) is correctly rounded to f64; f32 of that can double-round
  cands = sorted({float(np.nextafter(f, np.float32(-np.inf))), float(f), float(np.nextafter(f, np.float32(np.inf)))})
  err = [abs(fractions.Fraction(c) - x) for c in cands]
  winners = [c for c, e in zip(cands, err) if e == min(err)]
  if len(winners) > 1:                              # a tie: the even mantissa
    winners = [c for c in winners if (np.float32(c).view(np.uint32) & 1) == 0]
  return np.float32(winners[0])


def _madd(acc, w, x, fused):
  """acc + w * x in float32: two roundings, or — `fused` — one (exact rationals; non-finite operands take the plain path)."""
  if fused and np.isfinite(acc) and np.isfinite(w) and np.isfinite(x):
    return _round_f32(fractions.Fraction(float(w)) * fractions.Fraction(float(x)) + fractions.Fraction(float(acc)))
  prod = np.float32(w) * np.float32(x)
  return np.float32(np.float32(acc) + prod)


def _numpy_mlp(w1, w2, o, fused=False):
  """The rule in np.float32 scalars for ONE case: (best, s [H], h [H], logits [3])."""
  H, D = w1.shape[0], w1.shape[1] - 1
  s, h = np.zeros(H, np.float32), np.zeros(H, np.float32)
  with np.errstate(all='ignore'):
    l = [np.float32(w2[a, H]) for a in range(3)]
    for j in range(H):
      acc = np.float32(w1[j, D])
      for d in range(D):
        acc = _madd(acc, w1[j, d], o[d], fused)
      s[j] = acc
      h[j] = acc if acc > np.float32(0.0) else np.float32(0.0)
      for a in range(3):
        l[a] = _madd(l[a], w2[a, j], h[j], fused)
    best = 0
    for a in (1, 2):
      if l[a] > l[best]:
        best = a
  return best, s, h, np.array(l, np.float32)


def _numpy_run(w1, w2, o, fused=False):
  r = [_numpy_mlp(w1[c], w2[c], o[c], fused) for c in range(w1.shape[0])]
  return np.array([x[0] for x in r], np.int32), np.stack([x[1] for x in r]), np.stack([x[2] for x in r])


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _torch_run(w1, w2, o):
  best, s = observations.mlp_select(torch.from_numpy(w1), torch.from_numpy(w2), torch.from_numpy(o), return_preactivations=True)
  assert best.dtype is torch.int32 and s.dtype is torch.float32
  return best.numpy(), s.numpy()


def test_the_shim_compiles_the_kernels_header(shim):
  assert shim.shim_mlp_max_hidden() == 64 == _native.MLP_MAX_HIDDEN
  assert shim.shim_mlp_pair_floats(8, 64) == 771
  dev = open(os.path.join(CSRC, 'bsx_mlp_returns.h')).read()
  assert '#include "bsx_mlp.h"' in dev
  m = re.search(r'#define BSX_MLP_LDS_FLOATS (\d+)', dev)
  assert 771 <= int(m.group(1)) and int(m.group(1)) * 4 + 8 <= 4096
  text = open(os.path.join(CSRC, 'bsx_mlp.h')).read()
  assert 'BSX_HD int32_t bsx_mlp_select(' in text and 'BSX_NO_CONTRACT' in text
  assert 'fma' not in text.lower().replace('no fma', '')
  assert '#include "../../bsuite_amd/csrc/bsx_mlp.h"' in open(os.path.join(ROOT, 'tests', 'csrc', 'mlp_shim.c')).read()


@pytest.mark.parametrize('H', HIDDEN)
@pytest.mark.parametrize('D', DIMS)
def test_random_weights_and_observations(shim, D, H):
  rng = np.random.RandomState(100 * D + H)
  n = 400
  w1 = (rng.standard_normal((n, H, D + 1)) * rng.choice([1e-3, 1.0, 50.0], (n, 1, 1))).astype(np.float32)
  w2 = (rng.standard_normal((n, 3, H + 1)) * rng.choice([1e-2, 1.0, 20.0], (n, 1, 1))).astype(np.float32)
  w2[:, :, H] *= np.float32(0.1)                              # small biases: the hidden layer decides
  o = (rng.standard_normal((n, D)) * rng.choice([0.1, 1.0, 7.0], (n, 1))).astype(np.float32)
  best, s, h = _shim_run(shim, w1, w2, o)
  want, ws, wh = _numpy_run(w1, w2, o)
  np.testing.assert_array_equal(_bits(s), _bits(ws))
  np.testing.assert_array_equal(_bits(h), _bits(wh))
  np.testing.assert_array_equal(best, want)
  # not a constant policy and not a linear one: all three actions, both ReLU branches
  assert sorted(set(best.tolist())) == [0, 1, 2]
  assert (s > 0).any() and (s < 0).any() and (h[s < 0] == 0).all() and (h[s > 0] > 0).all()
  # ... and utils.observations.mlp_select is the same rule: one pair per lane, and a shared pair
  tb, ts = _torch_run(w1, w2, o)
  np.testing.assert_array_equal(tb, want)
  np.testing.assert_array_equal(_bits(ts), _bits(ws))
  one = observations.mlp_select(torch.from_numpy(w1[7]), torch.from_numpy(w2[7]), torch.from_numpy(o).reshape(n, 1, D))
  m = 64
  shared = _numpy_run(np.broadcast_to(w1[7], w1[:m].shape), np.broadcast_to(w2[7], w2[:m].shape), o[:m])[0]
  np.testing.assert_array_equal(one.numpy()[:m], shared)
  everywhere = _shim_run(shim, np.broadcast_to(w1[7], w1.shape), np.broadcast_to(w2[7], w2.shape), o)[0]
  np.testing.assert_array_equal(one.numpy(), everywhere)


def test_relu_of_nan_infinities_and_signed_zero(shim):
  nan, inf = np.float32('nan'), np.float32('inf')
  s = np.array([nan, -nan, inf, -inf, 0.0, -0.0, 1e-45, -1e-45, 3.0, -3.0], np.float32)
  h = np.full_like(s, 7.0)
  shim.shim_mlp_relu(len(s), _ptr(s), _ptr(h))
  want = np.array([0.0, 0.0, inf, 0.0, 0.0, 0.0, 1e-45, 0.0, 3.0, 0.0], np.float32)
  np.testing.assert_array_equal(_bits(h), _bits(want))          # bit for bit: every zero is +0.0


@pytest.mark.parametrize('H', HIDDEN)
@pytest.mark.parametrize('D', DIMS)
def test_ties_nan_infinities_and_denormals(shim, D, H):
  nan, inf = np.float32('nan'), np.float32('inf')
  rng = np.random.RandomState(7 * D + H)
  o = rng.standard_normal(D).astype(np.float32)
  cases, expect = [], []

  def add(w1, w2, want, row=None):
    cases.append((w1, w2, o if row is None else row))
    expect.append(want)

  z1, z2 = np.zeros((H, D + 1), np.float32), np.zeros((3, H + 1), np.float32)
  # ties of two and three logits through the biases alone (every h is 0): the lowest index wins
  for bias, want in (((1, 1, 1), 0), ((0, 1, 1), 1), ((1, 0, 1), 0), ((0, 0, 1), 2), ((2, 1, 2), 0), ((-0.0, 0.0, -0.0), 0)):
    w2 = z2.copy(); w2[:, H] = bias
    add(z1, w2, want)
  # ... and through the hidden layer: unit H-1 is h = 2 exactly, equal columns of w2 give equal logits
  on = z1.copy(); on[H - 1, D] = 2.0
  for col, want in (((3, 3, 3), 0), ((1, 3, 3), 1), ((3, 1, 3), 0), ((1, 1, 3), 2), ((-1, -1, -2), 0)):
    w2 = z2.copy(); w2[:, H - 1] = col
    add(on, w2, want)
  # NaN never wins; a NaN l_0 is never beaten
  for bias, want in (((nan, 1, 2), 0), ((0, nan, 2), 2), ((0, 1, nan), 1), ((0, nan, nan), 0), ((nan, nan, nan), 0),
                     ((-inf, -inf, -inf), 0), ((-inf, 0, inf), 2), ((inf, inf, 0), 0), ((0, inf, inf), 1), ((0, -inf, nan), 0)):
    w2 = z2.copy(); w2[:, H] = bias
    add(z1, w2, want)
  # pre-activations NaN, -inf, -0.0 (h = +0.0: the unit is off, action 0 by the tie) and +inf (h = inf: action 2)
  pay = z2.copy(); pay[2, 0] = 1.0; pay[1, 0] = -1.0; pay[0, 0] = -2.0      # (a zero weight on h = inf would be a NaN)
  for b, want in ((nan, 0), (-inf, 0), (-0.0, 0), (inf, 2)):
    w1 = z1.copy(); w1[0, D] = b
    add(w1, pay, want)
  w1 = z1.copy(); w1[0, 0] = inf                                        # inf * 0 in layer 1: s = NaN, the unit is off
  row = o.copy(); row[0] = 0.0
  add(w1, pay, 0, row)
  w1 = z1.copy(); w1[0, 0] = 3e38; w1[0, D] = -inf                      # +inf (overflow) + -inf: NaN again
  row = o.copy(); row[0] = 3e38
  add(w1, pay, 0, row)
  # inf * 0 in layer 2: an off unit under an infinite weight makes a NaN logit, which never wins — and spoils l_0 for good
  w2 = z2.copy(); w2[1, 0] = inf; w2[2, H] = -5.0
  add(z1, w2, 0)
  w2 = z2.copy(); w2[0, 0] = inf; w2[2, H] = 5.0
  add(z1, w2, 0)
  # a denormal product: h = 2^-100 times w2 = 2^-40 is 2^-140, not flushed to zero — it beats l_0 = 0
  w1 = z1.copy(); w1[0, D] = np.float32(2.0 ** -100)
  w2 = z2.copy(); w2[1, 0] = np.float32(2.0 ** -40)
  add(w1, w2, 1)
  w1 = z1.copy(); w1[0, 0] = np.float32(2.0 ** -100)                    # ... and one in layer 1: s = 2^-140 > 0
  row = o.copy(); row[0] = np.float32(2.0 ** -40)
  w2 = z2.copy(); w2[2, 0] = np.float32(2.0 ** 100)
  add(w1, w2, 2, row)
  W1, W2, O = (np.stack([c[k] for c in cases]).astype(np.float32) for k in range(3))
  best, s, h = _shim_run(shim, W1, W2, O)
  ref, rs, rh = _numpy_run(W1, W2, O)
  np.testing.assert_array_equal(best, ref)
  np.testing.assert_array_equal(_bits(h), _bits(rh))
  assert not (np.signbit(h) & (h == 0)).any()                            # no -0.0 activation anywhere
  for k, want in enumerate(expect):
    assert best[k] == want, (k, W1[k], W2[k])
  tb, _ = _torch_run(W1, W2, O)
  np.testing.assert_array_equal(tb, ref)


@pytest.mark.parametrize('H', HIDDEN)
@pytest.mark.parametrize('D', DIMS)
def test_fma_contraction_would_flip_the_action(shim, D, H):
  """w * o = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a tie in float32 and rounds to 1 + 2^-11; added to -(1 + 2^-11) it leaves
  exactly 0.  A fused multiply-add keeps the 2^-24.  Layer 1: the pre-activation is 0 (the unit is off) or 2^-24 (on), and a
  large w2 makes that the action.  Layer 2: l_1 is 0 (a tie with l_0: action 0) or 2^-24 (action 1)."""
  x = np.float32(1.0) + np.float32(2.0 ** -12)
  y = -(np.float32(1.0) + np.float32(2.0 ** -11))
  for j in sorted({0, H - 1}):
    for d in range(D):                                                    # layer 1, the product in every position of the row
      w1, w2, o = np.zeros((1, H, D + 1), np.float32), np.zeros((1, 3, H + 1), np.float32), np.zeros((1, D), np.float32)
      w1[0, j, d], o[0, d], w1[0, j, D] = x, x, y
      w2[0, 1, j] = np.float32(2.0 ** 30)
      a, s, _, _ = _numpy_mlp(w1[0], w2[0], o[0])
      b, sf, _, lf = _numpy_mlp(w1[0], w2[0], o[0], fused=True)
      assert s[j] == 0.0 and sf[j] == np.float32(2.0 ** -24) and lf[1] == 64.0
      assert (a, b) == (0, 1)                                             # the two roundings differ
      assert _shim_run(shim, w1, w2, o)[0].tolist() == [0]
      assert _torch_run(w1, w2, o)[0].tolist() == [0]
    # layer 2: unit j is h = x exactly (s = x + 0 * o), w2[1][j] = x, the bias of action 1 is y
    w1, w2, o = np.zeros((1, H, D + 1), np.float32), np.zeros((1, 3, H + 1), np.float32), np.ones((1, D), np.float32)
    w1[0, j, D], w2[0, 1, j], w2[0, 1, H] = x, x, y
    a, _, h, l = _numpy_mlp(w1[0], w2[0], o[0])
    b, _, _, lf = _numpy_mlp(w1[0], w2[0], o[0], fused=True)
    assert h[j] == x and l[1] == 0.0 and lf[1] == np.float32(2.0 ** -24)
    assert (a, b) == (0, 1)
    assert _shim_run(shim, w1, w2, o)[0].tolist() == [0]
    assert _torch_run(w1, w2, o)[0].tolist() == [0]


def test_the_shim_runs_stand_alone_under_the_sanitizers(tmp_path):
  """bsx_mlp.h with its own main under AddressSanitizer and UBSan, on the CPU (nothing loaded into python)."""
  exe = str(tmp_path / 'mlp_shim_main')
  cmd = ['gcc', '-O1', '-g', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-DMLP_SHIM_MAIN', os.path.join(ROOT, 'tests', 'csrc', 'mlp_shim.c'), '-o', exe]
  if subprocess.run(cmd, capture_output=True).returncode != 0:
    pytest.skip('this gcc has no sanitizer runtime')
  out = subprocess.run([exe], capture_output=True, text=True)
  assert out.returncode == 0 and out.stdout.strip() in ('0', '1', '2'), out


# ------------------------------------------------------------------------------------------ the Python entry point
def _envs():
  return [cartpole.Cartpole(seed=0, batch=4), cartpole.CartpoleSwingup(seed=0, batch=4), mountain_car.MountainCar(seed=0, batch=4)]


def _dim(env):
  return int(np.prod(env.observation_spec().shape))


def _pair(env, H=5, P=None):
  D, lead = _dim(env), (() if P is None else (P,))
  return torch.zeros(lead + (H, D + 1), dtype=torch.float32), torch.zeros(lead + (3, H + 1), dtype=torch.float32)


def _refused(env, exc=ValueError, match='evaluate_mlp', **kw):
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  w1 = kw.pop('w1') if 'w1' in kw else torch.zeros((5, 4), dtype=torch.float32)       # (None is one of the bad values)
  w2 = kw.pop('w2') if 'w2' in kw else torch.zeros((3, 6), dtype=torch.float32)
  obs = kw.pop('observation') if 'observation' in kw else torch.zeros((4, 3), dtype=torch.float32)
  with pytest.raises(exc, match=match) as info:
    env.evaluate_mlp(w1, w2, obs, kw.pop('num_steps', 4), **kw)
  assert 'evaluate_mlp' in str(info.value)                               # every message names the caller
  assert not raw._allocated                                              # pylint: disable=protected-access
  assert raw._linear_eval_out is None                                    # pylint: disable=protected-access


def test_signature_result_type_and_families():
  p = inspect.signature(base.Environment.evaluate_mlp).parameters
  assert list(p) == ['self', 'w1', 'w2', 'observation', 'num_steps', 'policy_index', 'epsilon', 'explore_seed']
  assert [p[k].kind for k in ('policy_index', 'epsilon', 'explore_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
  assert p['policy_index'].default is None and p['epsilon'].default == 0.0 and p['explore_seed'].default == 0
  assert all(p[k].default is inspect.Parameter.empty for k in ('w1', 'w2', 'observation', 'num_steps'))
  abi = lambda cls: cls._closed_loop_abi(object.__new__(cls), 'evaluate_mlp')                               # pylint: disable=protected-access
  assert abi(cartpole.Cartpole) == abi(cartpole.CartpoleSwingup) == ENTRY['cartpole'] and abi(mountain_car.MountainCar) == ENTRY['mountain_car']
  assert abi(base.Environment) is None and abi(catch.Catch) is None and set(ENTRY.values()) <= set(_native.EXPORTED)
  assert base.LinearEvaluation._fields == ('episodes', 'return_sum', 'episode_return_sum', 'observation')
  doc = base.Environment.evaluate_mlp.__doc__
  assert 'mlp_select' in doc and 'LinearEvaluation' in doc and 'policy_index' in doc
  # the two calls share their common refusals: the same words for the environment, num_steps, epsilon and the seed
  def spoil(what):
    env = mountain_car.MountainCar(seed=0, batch=4, rng='mt19937' if what == 'rng' else 'philox')
    env._device = torch.device('cpu')                                                                       # pylint: disable=protected-access
    if what == 'logging':
      env._logging = dict(steps=None)                                                                       # pylint: disable=protected-access
    if what == 'grouped':
      env._grouped_by = object()                                                                            # pylint: disable=protected-access
    if what == 'wrapped':
      wrappers.RewardScale(env, reward_scale=2.0)
    return env, dict(dict(num_steps=dict(num_steps=0), epsilon=dict(epsilon=2.0), seed=dict(explore_seed=-1)).get(what, {}))
  for what in ('rng', 'logging', 'grouped', 'wrapped', 'num_steps', 'epsilon', 'seed'):
    said = []
    for call, weights in (('evaluate_linear', (torch.zeros((3, 4)),)), ('evaluate_mlp', (torch.zeros((5, 4)), torch.zeros((3, 6))))):
      env, kw = spoil(what)
      with pytest.raises((ValueError, RuntimeError)) as info:
        getattr(env, call)(*weights, torch.zeros((4, 3)), kw.pop('num_steps', 4), **kw)
      said.append(str(info.value).replace(call, ''))
      assert not env._allocated and env._linear_eval_out is None                                            # pylint: disable=protected-access
    assert said[0] == said[1], what


def test_views_families_and_modes_are_refused():
  for env in (cartpole.Cartpole(seed=0), cartpole.CartpoleSwingup(seed=0), mountain_car.MountainCar(seed=0)):
    _refused(env, match='batched view')
  for bsuite_id in ('bandit/0', 'deep_sea/0', 'catch/0', 'memory_len/0', 'umbrella_length/0', 'discounting_chain/0'):
    _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), match='mountain_car only')
  _refused(catch.Catch(seed=0, batch=4, observation_mode='index'), match='mountain_car only')
  for cls in (cartpole.Cartpole, cartpole.CartpoleSwingup, mountain_car.MountainCar):
    _refused(cls(seed=0, batch=4, rng='mt19937'), match='philox')
  for env in _envs():
    env._logging = dict(steps=None)           # what enable_logging() leaves behind (it allocates: not without a GPU)
    _refused(env, match='Logging')
  for env in _envs():
    env._grouped_by = object()                # what SweepBatch sets while its prepared groups hold the column pointers
    _refused(env, exc=RuntimeError, match='release_groups')


def test_the_wrappers_refuse_instead_of_delegating():
  for make in (lambda e: wrappers.RewardNoise(e, noise_scale=0.5, seed=1), lambda e: wrappers.RewardScale(e, reward_scale=2.0)):
    for raw in _envs():
      _refused(make(raw), match='not available through')
      _refused(raw, match='reward wrapper')                       # ... and the raw environment knows it is wrapped
  for bsuite_id in ('cartpole_noise/2', 'cartpole_scale/4', 'mountain_car_noise/3', 'mountain_car_scale/1'):
    env = bsuite_amd.load_from_id(bsuite_id, batch=4)
    assert hasattr(env, 'raw_env'), bsuite_id
    _refused(env, match='not available through')
  # every wrapper class carries its own method (attribute delegation would reach the raw environment's)
  for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    fn = getattr(cls, 'evaluate_mlp')
    assert fn is not base.Environment.evaluate_mlp and any('evaluate_mlp' in vars(c) for c in cls.__mro__[:-1]), cls
    with pytest.raises(ValueError, match='evaluate_mlp'):
      fn(object.__new__(cls), torch.zeros((5, 4)), torch.zeros((3, 6)), torch.zeros((4, 3)), 4)
  image = wrappers.ImageObservation(mountain_car.MountainCar(seed=0, batch=4), (84, 84, 1))
  _refused(image, match='not available through ImageObservation')


def test_arguments_are_checked_before_any_gpu_use():
  for env in _envs():
    env._device = torch.device('cpu')       # the checks themselves, on host tensors: dtype, shape, contiguity
    D, H = _dim(env), 5
    (w1, w2), (p1, p2) = _pair(env), _pair(env, P=4)
    obs = torch.zeros((4, 1, D), dtype=torch.float32)
    idx = torch.zeros(4, dtype=torch.int32)
    ok = dict(w1=w1, w2=w2, observation=obs)
    for eps in (-0.1, 1.5, float('nan'), float('inf'), '0.1', None, True):
      _refused(env, epsilon=eps, match='evaluate_mlp: epsilon', **ok)
    for n in (0, -1, 2.0, None, '4', True):
      _refused(env, num_steps=n, match='evaluate_mlp: num_steps', **ok)
    for seed in (-1, 1 << 64, 0.5, None):
      _refused(env, explore_seed=seed, match='evaluate_mlp: explore_seed', **ok)
    for bad in (w1.to(torch.float64), w1.to(torch.float16), w1.numpy(), w1.tolist(), torch.zeros((H, D)), torch.zeros((H, D + 2)),
                torch.zeros((0, D + 1)), torch.zeros((65, D + 1)), torch.zeros(H * (D + 1)), torch.zeros((2, 2, H, D + 1)),
                torch.zeros((0, H, D + 1)), torch.zeros((H, 2 * (D + 1)))[:, ::2], torch.zeros((D + 1, H)).t(), None):
      _refused(env, w1=bad, w2=w2, observation=obs, match='evaluate_mlp: w1 must be')
    for bad in (w2.to(torch.float64), w2.numpy(), torch.zeros((3, H)), torch.zeros((3, H + 2)), torch.zeros((2, H + 1)),
                torch.zeros((1, 3, H + 1)), torch.zeros(3 * (H + 1)), torch.zeros((3, 2 * (H + 1)))[:, ::2], torch.zeros((H + 1, 3)).t(), None):
      _refused(env, w1=w1, w2=bad, observation=obs, match='evaluate_mlp: w2 must be')
    # a population: the same P and the same H in both
    for bad in (w2, torch.zeros((3, 3, H + 1)), torch.zeros((4, 3, H + 2)), torch.zeros((4, 3, H))):
      _refused(env, w1=p1, w2=bad, observation=obs, policy_index=idx, match='evaluate_mlp: w2 must be')
    for bad in (obs.to(torch.float64), obs.numpy(), torch.zeros((4, D + 1)), torch.zeros((3, 1, D)), torch.zeros((4, D, 1)),
                torch.zeros(4 * D), torch.zeros((4, 2 * D))[:, ::2], torch.zeros((D, 4)).t(), None):
      _refused(env, w1=w1, w2=w2, observation=bad, match='evaluate_mlp: observation must be')
    _refused(env, w1=w1, w2=w2, observation=torch.zeros((4, D)), policy_index=idx, match='must be None')   # ([B, D] is a legal shape)
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, w1=p1, w2=p2, observation=obs, policy_index=bad, match='policy_index')
    # the widest and the narrowest legal pair pass the checks (and nothing was allocated by them)
    for h in (1, 64):
      a, b = _pair(env, H=h)
      assert env._check_evaluate_mlp(a, b, obs, 4, None, 0.0, 0) == (1, h)          # pylint: disable=protected-access
    assert env._check_evaluate_mlp(p1, p2, obs, 4, idx, 0.5, 7) == (4, H)           # pylint: disable=protected-access
    assert not env._allocated                                                       # pylint: disable=protected-access
  # host tensors for an environment on the GPU
  env = mountain_car.MountainCar(seed=0, batch=4)
  a, b = _pair(env)
  _refused(env, w1=a, w2=b, observation=torch.zeros((4, 1, 3)), match='w1 must be')


# ------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_export_agree_and_the_abi_stays_v12():
  header = open(HEADER).read()
  assert re.search(r'#define BSX_ABI_VERSION 12\b', header)
  assert _native.ABI_VERSION == 12 and _native.lib.bsx_abi_version() == 12
  plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  out = subprocess.check_output(['nm', '-D', '--defined-only', _native.SO_PATH], text=True)
  P = ctypes.c_void_p
  for fam, name in ENTRY.items():
    decl = re.search(r'int ' + name + r'\(([^;]*)\);', plain)
    assert decl, f'include/bsuite_amd.h does not declare {name}'
    types = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(decl.group(1).split()).split(',')]
    assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_mlp_t*', 'float*', 'int32_t*', 'bsx_linear_eval_t', 'double*']
    assert name in _native.EXPORTED
    fn = getattr(_native.lib, name)
    cfg = dict(cartpole=_native.CartpoleCfg, mountain_car=_native.MountainCarCfg)[fam]
    assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.Mlp), P, P,
                           _native.LinearEvalPtrs, P] and fn.restype is ctypes.c_int
    assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
  body = re.search(r'typedef struct \{([^}]*)\} bsx_mlp_t;', plain).group(1)
  fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
  assert fields == ['const float* w1', 'const float* w2', 'int32_t hidden, n_policies', 'const int32_t* policy_index', 'double epsilon',
                    'uint64_t explore_seed', 'const float* observation_in']
  M = _native.Mlp
  names = [f[0] for f in M._fields_]                                                 # pylint: disable=protected-access
  assert names == ['w1', 'w2', 'hidden', 'n_policies', 'policy_index', 'epsilon', 'explore_seed', 'observation_in']
  assert [getattr(M, n).offset for n in names] == [0, 8, 16, 20, 24, 32, 40, 48] and ctypes.sizeof(M) == 56
  assert ctypes.sizeof(_native.LinearEvalPtrs) == 32 and ctypes.sizeof(_native.Linear) == 48       # the output struct is reused as it is
  assert re.search(r'#define BSX_MLP_MAX_HIDDEN 64\b', open(os.path.join(CSRC, 'bsx_mlp.h')).read())
  text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for name in list(ENTRY.values()) + ['bsx_mlp_t']:
    assert name in text, f'INTEGRATION.md does not describe {name}'


def _abi_case(fam):
  if fam == 'mountain_car':
    return _native.MountainCarCfg(1000, 0), _native.MountainCarCfg(0, 0)
  good = dict(swingup=0, last_step=1001, height_threshold=0.8, x_threshold=3.0, theta_dot_threshold=1.0, x_reward_threshold=1.0,
              timescale=0.01, mass_cart=1.0, mass_pole=0.1, length=0.5, force_mag=10.0, gravity=9.8, move_cost=0.0, init_range=0.05,
              theta_offset=0.0, time_frac=0xDEAD0008)
  return _native.CartpoleCfg(**good), _native.CartpoleCfg(**dict(good, last_step=0))


@pytest.mark.parametrize('fam', ['cartpole', 'mountain_car'])
def test_argument_checks_of_the_entry_points(fam):
  """Every refusal comes before any device work: host buffers (and garbage) stand in for device pointers, none is
  dereferenced.  The codes and their order are those of bsx_<family>_linear_evaluate: modes, scalars, pointers."""
  fn = getattr(_native.lib, ENTRY[fam])
  cfg, bad_cfg = _abi_case(fam)
  buf = (ctypes.c_uint8 * 64)()
  p = ctypes.addressof(buf)
  p -= p % 16
  junk = 0xDEAD0008                                                # never mapped: a dereference would fault
  E = _native

  def call(**kw):
    c = _native.Call(n_lanes=kw.pop('n_lanes', 4), n_steps=kw.pop('n_steps', 4), flags=kw.pop('flags', 0))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def mlp(**kw):
    d = dict(w1=p, w2=p, hidden=5, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, observation_in=p)
    d.update(kw)
    return _native.Mlp(**d)

  def run(c, q, state=p, steps=p, out=None, info=p, cfg_=cfg):
    out = _native.LinearEvalPtrs(p, p, p, p) if out is None else out
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, state, steps, out, info)

  # null structs
  assert run(call(), mlp(), cfg_=None) == E.BSX_ENULL
  assert run(None, mlp()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: before the scalars (a bad hidden and a bad n_policies are not looked at yet)
  for flags in (E.CALL_OBS_INDEX, E.CALL_OBS_U8, E.CALL_OBS_F16, E.CALL_OBS_BF16, E.CALL_OBS_INDEX | E.CALL_OBS_U8):
    assert run(call(flags=flags), mlp(n_policies=-1, hidden=0)) == E.BSX_EMODE, flags
  lg = _native.Logging()
  assert run(call(logging=ctypes.pointer(lg)), mlp(hidden=99)) == E.BSX_EMODE
  for kind in (E.WRAP_SCALE, E.WRAP_NOISE, E.WRAP_SCALE_NOISE, E.WRAP_NOISE_SCALE):
    c = call()
    c.wrap.kind = kind
    assert run(c, mlp()) == E.BSX_EMODE, kind
  c = call()
  c.stream.mt_state, c.stream.mt_pos = junk, junk
  assert run(c, mlp()) == E.BSX_EMODE
  for member in ('reward_f64', 'obs_paint', 'state_alt'):
    assert run(call(**{member: junk}), mlp()) == E.BSX_EMODE, member
  assert run(call(force_reset=1), mlp()) == E.BSX_EMODE
  assert run(call(action_ring=4), mlp()) == E.BSX_EMODE
  # BSX_EINVAL / BSX_ERANGE: the scalars — with garbage in every pointer
  wild = dict(state=junk, steps=junk, out=_native.LinearEvalPtrs(junk, junk, junk, junk), info=junk)
  wmlp = lambda **kw: mlp(w1=junk, w2=junk, observation_in=junk, **kw)
  for n in (0, -1):
    assert run(call(n_steps=n), wmlp(), **wild) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), wmlp(), **wild) == E.BSX_EINVAL
  for n in (0, -3):
    assert run(call(), wmlp(n_policies=n), **wild) == E.BSX_EINVAL
  for h in (0, -1, 65, 1 << 20):
    assert run(call(), wmlp(hidden=h), **wild) == E.BSX_EINVAL, h
    assert run(call(), wmlp(hidden=h, epsilon=2.0), **wild) == E.BSX_EINVAL, h      # where n_policies < 1 is: before epsilon
    assert run(call(n_lanes=0), wmlp(hidden=h), **wild) == E.BSX_EINVAL, h
  for h in (1, 64):
    assert run(call(n_lanes=0), wmlp(hidden=h), **wild) == 0
  for eps in (-1e-9, 1.0000001, float('nan'), float('inf')):
    assert run(call(), wmlp(epsilon=eps), **wild) == E.BSX_ERANGE, eps
  assert run(call(), wmlp(), cfg_=bad_cfg, **wild) == E.BSX_ERANGE
  assert run(call(flags=E.CALL_OBS_INDEX), wmlp(), cfg_=bad_cfg, **wild) == E.BSX_ERANGE      # (the cfg comes first)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at
  none = mlp(w1=None, w2=None, observation_in=None)
  assert run(call(n_lanes=0), none, state=None, steps=None, out=_native.LinearEvalPtrs(0, 0, 0, 0), info=None) == 0
  assert run(call(n_lanes=0), wmlp(), **wild) == 0
  assert run(call(n_lanes=0), mlp(epsilon=2.0)) == E.BSX_ERANGE                      # ... but the scalars are
  # BSX_ENULL: every pointer — the other ones garbage
  for missing in ('w1', 'w2', 'observation_in'):
    assert run(call(), mlp(**dict(dict(w1=junk, w2=junk, observation_in=junk), **{missing: None})), **wild) == E.BSX_ENULL, missing
  for missing in ('state', 'steps', 'info'):
    assert run(call(), wmlp(), **dict(wild, **{missing: None})) == E.BSX_ENULL, missing
  for k in range(4):
    ptrs = [junk] * 4
    ptrs[k] = 0
    assert run(call(), wmlp(), **dict(wild, out=_native.LinearEvalPtrs(*ptrs))) == E.BSX_ENULL, k
  assert run(call(), wmlp(n_policies=2), **wild) == E.BSX_ENULL                      # a population without policy_index
  if fam == 'cartpole':
    no_table = _abi_case(fam)[0]
    no_table.time_frac = None
    assert run(call(), wmlp(), cfg_=no_table, **wild) == E.BSX_ENULL
  assert run(call(n_lanes=1 << 40), wmlp(), **wild) == E.BSX_EINVAL                  # more workgroups than a grid holds
  assert run(call(action_ring=-2), wmlp(), **wild) == E.BSX_EINVAL


# ------------------------------------------------------------------------------------------ the source text
def test_the_kernel_body_uses_the_headers():
  dev = open(os.path.join(CSRC, 'bsx_mlp_returns.h')).read()
  body = dev[dev.index('void bsx_mlp_returns_body('):]
  body = body[:body.index('\n}\n')]
  for call_ in ('bsx_mlp_hidden(w1j, o, D)', 'bsx_mlp_accumulate(l, w2j, ', 'bsx_mlp_argmax(l)', 'bsx_policy_draws(p.explore_seed, lane, step)',
                'bsx_policy_clamp(k0.p.policy_index[i], k0.p.n_policies)', 'bsx_policy_select(', 'Env::reset_pending(rg)',
                'bsx_eval_accumulate(&e, type, reward)', 'bsx_pool_counts(', 'Env::template core<0, 0, true, false, false, V, true>(',
                'Env::template load_info<V>(', 'Env::template store_info<V>(', 'bsx_fresh(0u)', 'bsx_mlp_view(ka)'):
    assert call_ in body, call_
  loop = body[body.index('for (int t = 0; t < n_steps; ++t) {'):]
  loop = loop[:loop.index('\n    }\n')]
  assert 'bsx_eval_accumulate' in loop and 'core<' in loop and loop.count('bsx_mlp_hidden(') == 2 and 'bsx_mlp_argmax' in loop
  for word in ('bsx_emit', 'bsx_st<', 'small_obs_store_row', 'Env::store', 'store_info', 'out.', '__syncthreads', 'atomic', 's_w['):
    assert word not in loop, word
  rule = open(os.path.join(CSRC, 'bsx_mlp.h')).read()
  select = rule[rule.index('BSX_HD int32_t bsx_mlp_select('):]
  for piece in ('bsx_mlp_hidden(', 'bsx_mlp_accumulate(', 'bsx_mlp_argmax('):      # bsx_mlp_select is made of the kernel's pieces
    assert piece in select, piece
  hip = open(os.path.join(CSRC, 'mlp.hip')).read()
  for inst in ('<bsx_mlp_mountain_car, 0, true>', '<bsx_mlp_mountain_car, 0, false>', '<bsx_mlp_cartpole, 0, true>',
               '<bsx_mlp_cartpole, 0, false>', '<bsx_mlp_cartpole, 1, true>', '<bsx_mlp_cartpole, 1, false>'):
    assert 'bsx_mlp_returns_body' + inst in hip, inst
  assert hip.count('__global__') == 1 and open(os.path.join(CSRC, 'linear.hip')).read().count('__global__') == 1
  for f, entry in (('cartpole.hip', ENTRY['cartpole']), ('mountain_car.hip', ENTRY['mountain_car'])):
    assert 'extern "C" int ' + entry + '(' in open(os.path.join(CSRC, f)).read()
  # the merged board writer: one kernel in misc.hip, a uniform switch over a tagged struct; the template it replaces is gone
  misc = open(os.path.join(CSRC, 'misc.hip')).read()
  assert '__global__ void __launch_bounds__(BSX_BLOCK) bsx_hot_cells_kernel(const bsx_hot_cells_args a)' in misc
  assert 'bsx_launch_hot_cells(' in open(os.path.join(CSRC, 'bsx_pair_host.h')).read()
  assert '__global__' not in open(os.path.join(CSRC, 'bsx_pair_device.h')).read().split('bsx_hot_cells_body')[1].split('Narrow observation stream')[0]


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = 'bsx_mlp_returns_kernel'


@needs_llvm
def test_product_library_has_the_one_new_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  assert [n for n in ks if 'mlp' in n] == [NEW]                          # ONE kernel for the six cases
  assert not any(w in NEW for w in ('linear', 'score', 'eval', 'policy', 'index'))
  # what paid for it: the two one-float-per-thread board writers are one kernel
  hot = sorted(n for n in ks if 'hot_cells' in n or 'hot_stream_tiny' in n)
  assert hot == ['bsx_hot_cells_kernel'], hot
  k = ks[NEW]
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
  assert k['agpr_count'] == 0, k
  assert k['vgpr_count'] <= 128, k
  assert k['group_segment_fixed_size'] <= 4096, k


@needs_llvm
def test_no_store_no_barrier_and_no_spill_reload_inside_any_loop_of_the_new_kernel():
  """Inside ANY loop of the kernel — the six step loops and the hidden-unit loop nested in each; the compiler marks the blocks
  of a loop in its block comments — there is no global / flat / buffer store, no LDS write, no atomic, no barrier and no spill
  reload.  The shared pair is read from LDS inside three of them."""
  _, text = ki.kernel_text(os.path.join(CSRC, 'mlp.hip'), NEW)
  in_loop, inside, headers = False, [], 0
  for l in text:
    if re.match(r'^\.LBB\d+_\d+:', l) or l.startswith('; %bb.'):
      in_loop = 'Loop' in l
      headers += 'Loop Header' in l and 'Depth=1' in l
      continue
    s = l.strip()
    if in_loop and s and not s.startswith(';') and not s.startswith('.'):
      inside.append(s)
  assert headers >= 6, headers
  assert sum(s.startswith('ds_read') for s in inside) >= 3, 'the shared pair is read inside the loops'
  bad = [s for s in inside if re.match(r'(global|flat|scratch|buffer)_store|(global|flat|buffer|ds)_atomic|ds_write|ds_add|ds_\w*rtn|s_barrier', s)]
  assert not bad, bad
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
