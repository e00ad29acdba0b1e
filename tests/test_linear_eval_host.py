"""CPU: evaluate_linear (fused linear-policy evaluation of cartpole, swing-up and mountain_car; bsx_<family>_linear_evaluate)
without a GPU — the C ABI's declaration / binding / export and argument checks; every refusal of the Python entry point,
all before any GPU use; the selection rule the kernel compiles (bsx_linear_select in bsuite_amd/csrc/bsx_linear.h, through
gcc) against a numpy float32 restatement with one rounding per operation; and the kernel budget: ONE new kernel for the
three cases, paid for by the non-temporal calibration fill that became a mode of calib_copy_n_kernel, inside the resource
conditions, with no store, no barrier and no spill reload inside any of its loops."""
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
from bsuite_amd.environments import base, cartpole, catch, deep_sea, mountain_car
from bsuite_amd.utils import observations, wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
ENTRY = dict(cartpole='bsx_cartpole_linear_evaluate', mountain_car='bsx_mountain_car_linear_evaluate')
DIMS = dict(mountain_car=3, cartpole=6, swingup=8)


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
    assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_linear_t*', 'float*', 'int32_t*', 'bsx_linear_eval_t', 'double*']
    assert name in _native.EXPORTED
    fn = getattr(_native.lib, name)
    cfg = dict(cartpole=_native.CartpoleCfg, mountain_car=_native.MountainCarCfg)[fam]
    assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.Linear), P, P,
                           _native.LinearEvalPtrs, P] and fn.restype is ctypes.c_int
    assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
  fields = lambda t: [' '.join(f.split()) for f in re.search(r'typedef struct \{([^}]*)\} ' + t + ';', plain).group(1).split(';') if f.strip()]
  assert fields('bsx_linear_t') == ['const float* weights', 'int32_t n_policies', 'const int32_t* policy_index', 'double epsilon',
                                    'uint64_t explore_seed', 'const float* observation_in']
  assert fields('bsx_linear_eval_t') == ['int32_t* episodes', 'double* return_sum', 'double* episode_return_sum', 'float* observation_out']
  L, E = _native.Linear, _native.LinearEvalPtrs
  assert [f[0] for f in L._fields_] == ['weights', 'n_policies', 'policy_index', 'epsilon', 'explore_seed', 'observation_in']    # pylint: disable=protected-access
  assert [getattr(L, f[0]).offset for f in L._fields_] == [0, 8, 16, 24, 32, 40] and ctypes.sizeof(L) == 48                       # pylint: disable=protected-access
  assert [f[0] for f in E._fields_] == ['episodes', 'return_sum', 'episode_return_sum', 'observation_out']                        # pylint: disable=protected-access
  assert ctypes.sizeof(E) == 32
  # the tabular entry points and their result struct are as they were
  assert ctypes.sizeof(_native.PolicyEvalPtrs) == 24 and base.PolicyEvaluation._fields == ('episodes', 'return_sum', 'episode_return_sum')
  text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for name in ENTRY.values():
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
  dereferenced.  The codes and their order are those of bsx_<family>_policy_evaluate."""
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

  def lin(**kw):
    d = dict(weights=p, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, observation_in=p)
    d.update(kw)
    return _native.Linear(**d)

  def run(c, q, state=p, steps=p, out=None, info=p, cfg_=cfg):
    out = _native.LinearEvalPtrs(p, p, p, p) if out is None else out
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, state, steps, out, info)

  # null structs
  assert run(call(), lin(), cfg_=None) == E.BSX_ENULL
  assert run(None, lin()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: an observation code or index observations, and everything the fused loop does not carry — before the scalars
  for flags in (E.CALL_OBS_INDEX, E.CALL_OBS_U8, E.CALL_OBS_F16, E.CALL_OBS_BF16, E.CALL_OBS_INDEX | E.CALL_OBS_U8):
    assert run(call(flags=flags), lin(n_policies=-1)) == E.BSX_EMODE, flags
  lg = _native.Logging()
  assert run(call(logging=ctypes.pointer(lg)), lin()) == E.BSX_EMODE
  for kind in (E.WRAP_SCALE, E.WRAP_NOISE, E.WRAP_SCALE_NOISE, E.WRAP_NOISE_SCALE):
    c = call()
    c.wrap.kind = kind
    assert run(c, lin()) == E.BSX_EMODE, kind
  c = call()
  c.stream.mt_state, c.stream.mt_pos = junk, junk
  assert run(c, lin()) == E.BSX_EMODE
  for member in ('reward_f64', 'obs_paint', 'state_alt'):
    assert run(call(**{member: junk}), lin()) == E.BSX_EMODE, member
  assert run(call(force_reset=1), lin()) == E.BSX_EMODE
  assert run(call(action_ring=4), lin()) == E.BSX_EMODE
  # BSX_EINVAL / BSX_ERANGE: the scalars — with garbage in every pointer
  wild = dict(state=junk, steps=junk, out=_native.LinearEvalPtrs(junk, junk, junk, junk), info=junk)
  wlin = lambda **kw: lin(weights=junk, observation_in=junk, **kw)
  for n in (0, -1):
    assert run(call(n_steps=n), wlin(), **wild) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), wlin(), **wild) == E.BSX_EINVAL
  for n in (0, -3):
    assert run(call(), wlin(n_policies=n), **wild) == E.BSX_EINVAL
  for eps in (-1e-9, 1.0000001, float('nan'), float('inf')):
    assert run(call(), wlin(epsilon=eps), **wild) == E.BSX_ERANGE, eps
  assert run(call(), wlin(), cfg_=bad_cfg, **wild) == E.BSX_ERANGE
  assert run(call(flags=E.CALL_OBS_INDEX), wlin(), cfg_=bad_cfg, **wild) == E.BSX_ERANGE      # (the cfg comes first, as in policy_evaluate)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at
  assert run(call(n_lanes=0), lin(weights=None, observation_in=None), state=None, steps=None, out=_native.LinearEvalPtrs(0, 0, 0, 0), info=None) == 0
  assert run(call(n_lanes=0), wlin(), **wild) == 0
  assert run(call(n_lanes=0), lin(epsilon=2.0)) == E.BSX_ERANGE                      # ... but the scalars are
  # BSX_ENULL: every pointer — the other ones garbage
  assert run(call(), lin(weights=None, observation_in=junk), **wild) == E.BSX_ENULL
  assert run(call(), lin(weights=junk, observation_in=None), **wild) == E.BSX_ENULL
  for missing in ('state', 'steps', 'info'):
    assert run(call(), wlin(), **dict(wild, **{missing: None})) == E.BSX_ENULL, missing
  for k in range(4):
    ptrs = [junk] * 4
    ptrs[k] = 0
    assert run(call(), wlin(), **dict(wild, out=_native.LinearEvalPtrs(*ptrs))) == E.BSX_ENULL, k
  assert run(call(), wlin(n_policies=2), **wild) == E.BSX_ENULL                      # a population without policy_index
  if fam == 'cartpole':
    no_table = _abi_case(fam)[0]
    no_table.time_frac = None
    assert run(call(), wlin(), cfg_=no_table, **wild) == E.BSX_ENULL
  assert run(call(n_lanes=1 << 40), wlin(), **wild) == E.BSX_EINVAL                  # more workgroups than a grid holds
  assert run(call(action_ring=-2), wlin(), **wild) == E.BSX_EINVAL


def test_the_calibration_fill_keeps_its_codes():
  """bsx_calib_fill(nontemporal != 0) is served by a mode of calib_copy_n_kernel now: the entry point's checks are the same
  for both values of the flag (what it writes: tests/test_gpu_linear_eval.py)."""
  buf = (ctypes.c_uint8 * 64)()
  p = ctypes.addressof(buf)
  p -= p % 16
  for nt in (0, 1):
    assert _native.lib.bsx_calib_fill(None, 16, nt, None) == _native.BSX_ENULL
    assert _native.lib.bsx_calib_fill(p, -16, nt, None) == _native.BSX_EINVAL
    assert _native.lib.bsx_calib_fill(p, 24, nt, None) == _native.BSX_EINVAL
    assert _native.lib.bsx_calib_fill(p + 4, 16, nt, None) == _native.BSX_EALIGN
    assert _native.lib.bsx_calib_fill(p, 0, nt, None) == 0
    assert _native.lib.bsx_calib_fill(p, (0x7FFFFFFF * 256 + 1) * 16, nt, None) == _native.BSX_EINVAL


# ------------------------------------------------------------------------------------------ the Python entry point
def _envs():
  return [cartpole.Cartpole(seed=0, batch=4), cartpole.CartpoleSwingup(seed=0, batch=4), mountain_car.MountainCar(seed=0, batch=4)]


def _dim(env):
  return int(np.prod(env.observation_spec().shape))


def _weights(env, P=None):
  D = _dim(env)
  return torch.zeros((3, D + 1) if P is None else (P, 3, D + 1), dtype=torch.float32)


def _refused(env, exc=ValueError, match='evaluate_linear', **kw):
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  weights, obs = kw.pop('weights', None), kw.pop('observation', None)
  if weights is None:
    weights = torch.zeros((3, 4), dtype=torch.float32)
  if obs is None:
    obs = torch.zeros((4, 3), dtype=torch.float32)
  with pytest.raises(exc, match=match) as info:
    env.evaluate_linear(weights, obs, kw.pop('num_steps', 4), **kw)
  assert 'evaluate_linear' in str(info.value)                          # every message names the caller
  assert not raw._allocated                                            # pylint: disable=protected-access
  assert raw._linear_eval_out is None                                  # pylint: disable=protected-access


def test_signature_and_result_type():
  p = inspect.signature(base.Environment.evaluate_linear).parameters
  assert list(p) == ['self', 'weights', 'observation', 'num_steps', 'policy_index', 'epsilon', 'explore_seed']
  assert [p[k].kind for k in ('policy_index', 'epsilon', 'explore_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
  assert p['policy_index'].default is None and p['epsilon'].default == 0.0 and p['explore_seed'].default == 0
  assert all(p[k].default is inspect.Parameter.empty for k in ('weights', 'observation', 'num_steps'))     # the observation is required
  assert base.LinearEvaluation._fields == ('episodes', 'return_sum', 'episode_return_sum', 'observation')
  assert base.PolicyEvaluation._fields == ('episodes', 'return_sum', 'episode_return_sum')
  abi = lambda cls: cls._closed_loop_abi(object.__new__(cls), 'evaluate_linear')                                 # pylint: disable=protected-access
  assert abi(cartpole.Cartpole) == abi(cartpole.CartpoleSwingup) == ENTRY['cartpole'] and abi(mountain_car.MountainCar) == ENTRY['mountain_car']
  assert abi(base.Environment) is None and abi(catch.Catch) is None and set(ENTRY.values()) <= set(_native.EXPORTED)
  assert [_dim(e) for e in _envs()] == [DIMS['cartpole'], DIMS['swingup'], DIMS['mountain_car']]
  doc = base.Environment.evaluate_linear.__doc__
  assert 'linear_select' in doc and 'never reads its row' in doc


def test_the_scalar_view_is_refused():
  for env in (cartpole.Cartpole(seed=0), cartpole.CartpoleSwingup(seed=0), mountain_car.MountainCar(seed=0)):
    _refused(env, match='batched view')


@pytest.mark.parametrize('bsuite_id', ['bandit/0', 'deep_sea/0', 'catch/0', 'memory_len/0', 'umbrella_length/0', 'discounting_chain/0'])
def test_other_families_are_refused(bsuite_id):
  _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), match='mountain_car only')
  _refused(catch.Catch(seed=0, batch=4, observation_mode='index'), match='mountain_car only')


def test_mnist_is_refused():
  from bsuite_amd.environments import mnist
  from tests import golden_util as gu
  images, labels = gu.mnist_dataset()
  _refused(mnist.MNISTBandit(images=images, labels=labels, seed=0, batch=4), match='mountain_car only')


def test_the_tabular_calls_keep_refusing_these_families():
  for env in _envs():
    for fn in (env.evaluate_policy, env.rollout_policy):
      with pytest.raises(ValueError, match='deep_sea and catch only'):
        fn(torch.zeros(4, dtype=torch.uint8), 4)


def test_mt19937_is_refused():
  for cls in (cartpole.Cartpole, cartpole.CartpoleSwingup, mountain_car.MountainCar):
    _refused(cls(seed=0, batch=4, rng='mt19937'), match='philox')


def test_an_environment_with_logging_enabled_is_refused():
  for env in _envs():
    env._logging = dict(steps=None)           # what enable_logging() leaves behind (it allocates: not without a GPU)
    _refused(env, match='Logging')


def test_a_segment_of_prepared_sweep_groups_is_refused():
  for env in _envs():
    env._grouped_by = object()                # what SweepBatch sets while its prepared groups hold the column pointers
    _refused(env, exc=RuntimeError, match='release_groups')


def test_the_wrappers_refuse_instead_of_delegating():
  for make in (lambda e: wrappers.RewardNoise(e, noise_scale=0.5, seed=1), lambda e: wrappers.RewardScale(e, reward_scale=2.0)):
    for raw in _envs():
      env = make(raw)
      _refused(env, match='not available through')
      _refused(raw, match='reward wrapper')                       # ... and the raw environment knows it is wrapped
  for bsuite_id in ('cartpole_noise/2', 'cartpole_scale/4', 'mountain_car_noise/3', 'mountain_car_scale/1'):
    env = bsuite_amd.load_from_id(bsuite_id, batch=4)
    assert hasattr(env, 'raw_env'), bsuite_id
    _refused(env, match='not available through')
  # every wrapper class carries its own method (attribute delegation would reach the raw environment's)
  for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    fn = getattr(cls, 'evaluate_linear')
    assert fn is not base.Environment.evaluate_linear and any('evaluate_linear' in vars(c) for c in cls.__mro__[:-1]), cls
    with pytest.raises(ValueError, match='evaluate_linear'):
      fn(object.__new__(cls), torch.zeros((3, 4)), torch.zeros((4, 3)), 4)
  image = wrappers.ImageObservation(mountain_car.MountainCar(seed=0, batch=4), (84, 84, 1))
  _refused(image, match='not available through ImageObservation')


def test_arguments_are_checked_before_any_gpu_use():
  for env in _envs():
    env._device = torch.device('cpu')       # the checks themselves, on host tensors: dtype, shape, contiguity
    D = _dim(env)
    ok, pop = _weights(env), _weights(env, 4)
    obs = torch.zeros((4, 1, D), dtype=torch.float32)
    idx = torch.zeros(4, dtype=torch.int32)
    for eps in (-0.1, 1.5, float('nan'), float('inf'), '0.1', None, True):
      _refused(env, weights=ok, observation=obs, epsilon=eps, match='evaluate_linear: epsilon')
    for n in (0, -1, 2.0, None, '4', True):
      _refused(env, weights=ok, observation=obs, num_steps=n, match='evaluate_linear: num_steps')
    for seed in (-1, 1 << 64, 0.5, None):
      _refused(env, weights=ok, observation=obs, explore_seed=seed, match='evaluate_linear: explore_seed')
    for bad in (ok.to(torch.float64), ok.to(torch.float16), ok.numpy(), ok.tolist(), torch.zeros((3, D)), torch.zeros((3, D + 2)),
                torch.zeros((2, D + 1)), torch.zeros((4, D + 1)), torch.zeros(3 * (D + 1)), torch.zeros((2, 2, 3, D + 1)),
                torch.zeros((0, 3, D + 1)), torch.zeros((3, 2 * (D + 1)))[:, ::2], torch.zeros((D + 1, 3)).t(), None):
      with pytest.raises(ValueError, match='evaluate_linear: weights must be'):
        env.evaluate_linear(bad, obs, 4)
      assert not env._allocated and env._linear_eval_out is None      # pylint: disable=protected-access
    for bad in (obs.to(torch.float64), obs.numpy(), torch.zeros((4, D + 1)), torch.zeros((3, 1, D)), torch.zeros((4, D, 1)),
                torch.zeros(4 * D), torch.zeros((4, 2 * D))[:, ::2], torch.zeros((D, 4)).t(), None):
      with pytest.raises(ValueError, match='evaluate_linear: observation must be'):
        env.evaluate_linear(ok, bad, 4)
      assert not env._allocated and env._linear_eval_out is None      # pylint: disable=protected-access
    _refused(env, weights=ok, observation=torch.zeros((4, D)), policy_index=idx, match='must be None')     # ([B, D] is a legal shape)
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, weights=pop, observation=obs, policy_index=bad, match='policy_index')
  # host tensors for an environment on the GPU
  env = mountain_car.MountainCar(seed=0, batch=4)
  _refused(env, weights=_weights(env), observation=torch.zeros((4, 1, 3)), match='weights must be')


# ------------------------------------------------------------------------------------------ bsx_linear_select, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('lin') / 'linear_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC',
                         os.path.join(ROOT, 'tests', 'csrc', 'linear_shim.c'), '-o', so])
  lib = ctypes.CDLL(so)
  lib.shim_linear_select.restype = None
  lib.shim_linear_select.argtypes = [ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 3
  return lib


def _shim_run(lib, w, o):
  w, o = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(o, np.float32)
  n, A, D1 = w.shape
  assert A == 3 and o.shape == (n, D1 - 1)
  best = np.full(n, -1, np.int32)
  ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  lib.shim_linear_select(n, D1 - 1, ptr(w), ptr(o), ptr(best))
  return best


def _logits(w, o, fused=False):
  """The rule in numpy: np.float32 scalars, one rounding per operation — or, `fused`, each multiply-add rounded once (exact in
  float64: a product of two float32 has 48 significant bits, and the sum is rounded to float32 directly... which float64
  cannot do in general, so the fused form is taken with exact rationals)."""
  import fractions  # pylint: disable=import-outside-toplevel
  A, D = w.shape[0], w.shape[1] - 1
  out = np.zeros(A, np.float32)
  with np.errstate(all='ignore'):
    for a in range(A):
      l = np.float32(w[a, D])
      for d in range(D):
        if fused and np.isfinite(l) and np.isfinite(w[a, d]) and np.isfinite(o[d]):
          exact = fractions.Fraction(float(w[a, d])) * fractions.Fraction(float(o[d])) + fractions.Fraction(float(l))
          l = _round_f32(exact)
        else:
          prod = np.float32(w[a, d]) * np.float32(o[d])
          l = np.float32(l + prod)
      out[a] = l
  return out


def _round_f32(x):
  """A rational rounded to the nearest float32, ties to even (values well inside the normal range)."""
  import fractions  # pylint: disable=import-outside-toplevel
  if x == 0:
    return np.float32(0.0)
  f = np.float32(float(x))                          # float(Fraction) is correctly rounded to f64; f32 of that can double-round
  lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
  cands = sorted({float(lo), float(f), float(hi)})
  err = [abs(fractions.Fraction(c) - x) for c in cands]
  best = min(err)
  winners = [c for c, e in zip(cands, err) if e == best]
  if len(winners) > 1:                              # a tie: the even mantissa
    winners = [c for c in winners if (np.float32(c).view(np.uint32) & 1) == 0]
  return np.float32(winners[0])


def _argmax(l):
  best = 0
  for a in range(1, len(l)):
    if l[a] > l[best]:
      best = a
  return best


def _numpy_select(w, o, fused=False):
  return np.array([_argmax(_logits(w[c], o[c], fused)) for c in range(w.shape[0])], np.int32)


def test_the_shim_compiles_the_kernels_header(shim):
  assert shim.shim_linear_actions() == 3 and shim.shim_linear_max_obs() == 8
  dev = open(os.path.join(ROOT, 'bsuite_amd', 'csrc', 'bsx_linear_score.h')).read()
  assert '#include "bsx_linear.h"' in dev
  text = open(os.path.join(ROOT, 'bsuite_amd', 'csrc', 'bsx_linear.h')).read()
  assert 'BSX_HD int32_t bsx_linear_select(' in text and 'BSX_NO_CONTRACT' in text and 'fma' not in text.lower().replace('no fma', '')


@pytest.mark.parametrize('D', [3, 6, 8])
def test_random_weights_and_observations(shim, D):
  rng = np.random.RandomState(D)
  n = 2000
  w = (rng.standard_normal((n, 3, D + 1)) * rng.choice([1e-3, 1.0, 50.0], (n, 1, 1))).astype(np.float32)
  o = (rng.standard_normal((n, D)) * rng.choice([0.1, 1.0, 7.0], (n, 1))).astype(np.float32)
  got, want = _shim_run(shim, w, o), _numpy_select(w, o)
  np.testing.assert_array_equal(got, want)
  assert sorted(set(got.tolist())) == [0, 1, 2]
  # ... and utils.observations.linear_select is the same rule: shared matrix and one matrix per lane
  t = observations.linear_select(torch.from_numpy(w), torch.from_numpy(o).reshape(n, 1, D))
  assert t.dtype is torch.int32
  np.testing.assert_array_equal(t.numpy(), want)
  one = observations.linear_select(torch.from_numpy(w[7]), torch.from_numpy(o))
  np.testing.assert_array_equal(one.numpy(), _numpy_select(np.broadcast_to(w[7], w.shape), o))


@pytest.mark.parametrize('D', [3, 6, 8])
def test_ties_nan_and_infinities(shim, D):
  rng = np.random.RandomState(100 + D)
  base_w = rng.standard_normal((3, D + 1)).astype(np.float32)
  o = rng.standard_normal(D).astype(np.float32)
  cases, want = [], []

  def add(w, expect):
    cases.append(w)
    want.append(expect)

  # exact ties: equal rows give equal logits — the lowest index wins
  for rows, expect in (((0, 0, 0), 0), ((0, 0, 1), None), ((1, 0, 0), None), ((0, 1, 0), None), ((1, 1, 0), None)):
    w = base_w[list(rows)]
    add(w, expect)
  hi = base_w.copy()
  hi[:, :D] = 0.0
  for bias, expect in (((1, 1, 1), 0), ((0, 1, 1), 1), ((1, 0, 1), 0), ((0, 0, 1), 2), ((2, 1, 2), 0), ((-0.0, 0.0, -0.0), 0)):
    w = hi.copy()
    w[:, D] = bias
    add(w, expect)
  # NaN never wins; a NaN l_0 is never beaten (l > NaN is false)
  nan, inf = np.float32('nan'), np.float32('inf')
  for bias, expect in (((nan, 1, 2), 0), ((0, nan, 2), 2), ((0, 1, nan), 1), ((0, nan, nan), 0), ((nan, nan, nan), 0), ((1, nan, 0), 0),
                       ((-inf, -inf, -inf), 0), ((-inf, 0, inf), 2), ((inf, inf, 0), 0), ((0, inf, inf), 1), ((-inf, nan, -inf), 0),
                       ((inf, nan, inf), 0), ((0, -inf, nan), 0)):
    w = hi.copy()
    w[:, D] = bias
    add(w, expect)
  # infinities and NaN made by the arithmetic itself: inf * 0 and inf - inf are NaN, overflow is inf
  zero = np.zeros_like(hi)
  w = zero.copy(); w[1, 0] = inf; add(w, None)
  w = zero.copy(); w[2, 0] = 3e38; w[2, 1] = 3e38; add(w, None)
  w = zero.copy(); w[1, 0] = 3e38; w[1, D] = -inf; add(w, None)
  W = np.stack(cases).astype(np.float32)
  O = np.broadcast_to(o, (len(cases), D)).copy()
  O[-3, 0] = 0.0                      # inf * 0
  O[-2, :2] = 3e38                    # overflow to +inf
  O[-1, 0] = 3e38                     # +inf + -inf
  got, ref = _shim_run(shim, W, O), _numpy_select(W, O)
  np.testing.assert_array_equal(got, ref)
  for k, expect in enumerate(want):
    if expect is not None:
      assert got[k] == expect, (k, W[k, :, D])
  assert got[-3] == 0 and got[-2] == 2 and got[-1] == 0
  t = observations.linear_select(torch.from_numpy(W), torch.from_numpy(O))
  np.testing.assert_array_equal(t.numpy(), ref)


@pytest.mark.parametrize('D', [3, 6, 8])
def test_fma_contraction_would_flip_the_argmax(shim, D):
  """w * o = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a tie in float32 and rounds to 1 + 2^-11; the bias -(1 + 2^-11) then leaves
  exactly 0, which does not beat l_0 = 0.  A fused multiply-add keeps the 2^-24: l_1 > l_0 and the argmax is 1."""
  x = np.float32(1.0) + np.float32(2.0 ** -12)
  for d in range(D):                                   # the product in every position of the row
    w = np.zeros((1, 3, D + 1), np.float32)
    o = np.zeros((1, D), np.float32)
    w[0, 1, d], o[0, d] = x, x
    w[0, 1, D] = -(np.float32(1.0) + np.float32(2.0 ** -11))
    unfused, fused = _logits(w[0], o[0]), _logits(w[0], o[0], fused=True)
    assert unfused[1] == 0.0 and fused[1] == np.float32(2.0 ** -24) and unfused[0] == fused[0] == 0.0
    assert _numpy_select(w, o).tolist() == [0] and _numpy_select(w, o, fused=True).tolist() == [1]       # the two differ
    assert _shim_run(shim, w, o).tolist() == [0]
    assert observations.linear_select(torch.from_numpy(w[0]), torch.from_numpy(o)).tolist() == [0]
  # ... and one where the unfused result is the one that moves away from a tie: fused 1 wins over 2, unfused they tie -> 1 as well,
  # but against a slightly larger l_2 only the fused sum wins
  w = np.zeros((1, 3, D + 1), np.float32)
  o = np.zeros((1, D), np.float32)
  w[0, 1, D - 1], o[0, D - 1] = x, x
  w[0, 2, D] = np.float32(1.0) + np.float32(2.0 ** -11)
  w[0, 0, D] = -1.0
  assert _numpy_select(w, o).tolist() == [1] == _shim_run(shim, w, o).tolist()     # a tie of 1 and 2: the lower index
  w[0, 2, D] = np.nextafter(w[0, 2, D], np.float32(2.0))                            # l_2 one ulp above the rounded product
  assert _numpy_select(w, o).tolist() == [2] == _shim_run(shim, w, o).tolist()
  assert _numpy_select(w, o, fused=True).tolist() == [2]


def test_the_kernel_body_uses_the_headers():
  csrc = os.path.join(ROOT, 'bsuite_amd', 'csrc')
  dev = open(os.path.join(csrc, 'bsx_linear_score.h')).read()
  body = dev[dev.index('void bsx_linear_score_body('):]
  body = body[:body.index('\n}\n')]
  for call_ in ('bsx_linear_select(w, o, D)', 'bsx_policy_draws(p.explore_seed, lane, step)', 'bsx_policy_clamp(', 'bsx_policy_select(',
                'Env::reset_pending(rg)', 'bsx_eval_accumulate(&e, type, reward)', 'bsx_pool_counts(',
                'Env::template core<0, 0, true, false, false, V, true>(', 'Env::template load_info<V>(', 'Env::template store_info<V>('):
    assert call_ in body, call_
  loop = body[body.index('for (int t = 0; t < n_steps; ++t) {'):]
  loop = loop[:loop.index('\n    }\n')]
  assert 'bsx_eval_accumulate' in loop and 'core<' in loop and 'bsx_linear_select' in loop
  for word in ('bsx_emit', 'bsx_st<', 'small_obs_store_row', 'Env::store', 'store_info', 'out.', '__syncthreads', 'atomic'):
    assert word not in loop, word
  hip = open(os.path.join(csrc, 'linear.hip')).read()
  for inst in ('<bsx_linear_mountain_car, 0, true>', '<bsx_linear_mountain_car, 0, false>', '<bsx_linear_cartpole, 0, true>',
               '<bsx_linear_cartpole, 0, false>', '<bsx_linear_cartpole, 1, true>', '<bsx_linear_cartpole, 1, false>'):
    assert 'bsx_linear_score_body' + inst in hip, inst
  assert hip.count('__global__') == 1
  for f, entry in (('cartpole.hip', ENTRY['cartpole']), ('mountain_car.hip', ENTRY['mountain_car'])):
    assert 'extern "C" int ' + entry + '(' in open(os.path.join(csrc, f)).read()


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = 'bsx_linear_score_kernel'


@needs_llvm
def test_product_library_has_the_one_new_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  new = [n for n in ks if 'linear' in n or 'score' in n]
  assert new == [NEW], new                                              # ONE kernel for the three cases
  assert 'eval' not in NEW and 'policy' not in NEW and 'index' not in NEW
  assert sorted(n for n in ks if 'eval' in n) == ['bsx_tab_eval_kernel']
  assert sorted(n for n in ks if 'policy' in n) == ['bsx_policy_rollout_kernel<catch_fam, catch_hot>',
                                                    'bsx_policy_rollout_kernel<deep_sea_fam, deep_sea_hot>']
  # what paid for it: the non-temporal fill is a mode of calib_copy_n_kernel; the fill the benchmark measures against is as it was
  calib = sorted(n for n in ks if n.startswith('calib_'))
  assert calib == ['calib_copy_kernel<2>', 'calib_copy_n_kernel', 'calib_fill_kernel<false>'], calib
  k = ks[NEW]
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
  assert k['agpr_count'] == 0, k
  assert k['vgpr_count'] <= 128, k
  assert k['group_segment_fixed_size'] <= 1024, k                       # the shared matrix and two counters: no table, no pool


@needs_llvm
def test_no_store_no_barrier_and_no_spill_reload_inside_any_loop_of_the_new_kernel():
  """The six step loops (three cases, shared matrix or one per lane) keep everything in registers: inside ANY loop of the
  kernel — the compiler marks the blocks of a loop in its block comments — there is no global / flat / buffer / scratch
  store, no LDS write, no barrier (resets are not pooled) and no spill reload.  The shared matrix is read from LDS inside
  three of them, so the loops looked at are the step loops."""
  _, text = ki.kernel_text(os.path.join(ROOT, 'bsuite_amd', 'csrc', 'linear.hip'), NEW)
  in_loop, inside, outside, headers = False, [], [], 0
  for l in text:
    if re.match(r'^\.LBB\d+_\d+:', l) or l.startswith('; %bb.'):
      in_loop = 'Loop' in l
      headers += 'Loop Header' in l and 'Depth=1' in l
      continue
    s = l.strip()
    if s and not s.startswith(';') and not s.startswith('.'):
      (inside if in_loop else outside).append(s)
  assert headers >= 6, headers
  assert sum(s.startswith('ds_read') for s in inside) >= 3 * 2, 'the shared matrix is read inside the loops'
  bad = [s for s in inside if re.match(r'(global|flat|scratch|buffer)_store|(global|flat|buffer)_atomic|ds_write|ds_add|s_barrier', s)]
  assert not bad, bad
  assert not any(s.startswith('flat_') or s.startswith('scratch_') for s in inside + outside)
  assert sum(s.startswith('global_store') for s in outside) >= 6 * 5     # state, steps, info, three columns, the row: per loop
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
  assert not any(re.search(r'v_(readlane|writelane)_b32 \w+, \w+, \d+', s) for s in inside + outside)     # no spill to lanes anywhere
