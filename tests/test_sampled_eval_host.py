"""CPU: evaluate_sampled_linear / evaluate_sampled_mlp (fused softmax-policy evaluation of cartpole, swing-up and mountain_car;
bsx_<family>_linear_sample_evaluate, bsx_<family>_mlp_sample_evaluate) without a GPU — the C ABI's declarations, bindings,
exports and argument checks; every refusal of the Python entry points, all before any GPU use; the source text of the new
body (every rule through the existing headers); and the built library: ONE new kernel inside the kernel budget, paid for by
the two delta-mode lane advances of deep_sea and catch that became one kernel, inside the resource conditions, with no
store and nothing that waits inside its loops.  (The rule itself — logits, draws, Gumbel-max — is tests/test_sample_host.py's:
the new kernel calls the same header.)"""
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
from bsuite_amd.utils import wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bsuite_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
KINDS = ('linear', 'mlp')
ENTRY = {(fam, kind): f'bsx_{fam}_{kind}_sample_evaluate' for fam in ('cartpole', 'mountain_car') for kind in KINDS}
RESERVED = ('linear', 'score', 'eval', 'policy', 'index', 'mlp', 'trajectory', 'gumbel', 'softmax', 'tab_sample', 'hot_cells',
            'hot_stream_tiny')


# ------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_export_agree_and_the_abi_stays_v12():
  header = open(HEADER).read()
  assert re.search(r'#define BSX_ABI_VERSION 12\b', header)
  assert _native.ABI_VERSION == 12 and _native.lib.bsx_abi_version() == 12
  plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  out = subprocess.check_output(['nm', '-D', '--defined-only', _native.SO_PATH], text=True)
  P = ctypes.c_void_p
  text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  table = open(os.path.join(ROOT, 'include', 'bsx_stream.h')).read()
  assert 'bsx_<family>_linear_sample_evaluate / bsx_<family>_mlp_sample_evaluate' in table
  for (fam, kind), name in ENTRY.items():
    decl = re.search(r'int ' + name + r'\(([^;]*)\);', plain)
    assert decl, f'include/bsuite_amd.h does not declare {name}'
    types = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(decl.group(1).split()).split(',')]
    assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', f'const bsx_{kind}_t*', 'double', 'float*', 'int32_t*',
                     'bsx_linear_eval_t', 'double*']
    # the matching *_evaluate with one double after the policy struct
    ev = re.search(r'int ' + name.replace('_sample_evaluate', '_evaluate') + r'\(([^;]*)\);', plain)
    etypes = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(ev.group(1).split()).split(',')]
    assert types[:3] + types[4:] == etypes
    assert name in _native.EXPORTED
    fn = getattr(_native.lib, name)
    cfg = dict(cartpole=_native.CartpoleCfg, mountain_car=_native.MountainCarCfg)[fam]
    policy = dict(linear=_native.Linear, mlp=_native.Mlp)[kind]
    assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(policy), ctypes.c_double, P, P,
                           _native.LinearEvalPtrs, P]
    assert fn.restype is ctypes.c_int
    assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
    assert name in text, f'INTEGRATION.md does not describe {name}'
    assert 'extern "C" int ' + name + '(' in open(os.path.join(CSRC, fam + '.hip')).read()
  # no new struct and no new field: the policies and the result are the existing ones
  assert ctypes.sizeof(_native.Linear) == 48 and ctypes.sizeof(_native.Mlp) == 56 and ctypes.sizeof(_native.LinearEvalPtrs) == 32
  note = header[header.index('fused sampled evaluation'):header.index('int bsx_cartpole_linear_sample_evaluate(')]
  for word in ('SAMPLE SEED', 'BSX_ERANGE', 'inv_temperature', 'epsilon is not 0.0', 'observation_out', 'no 4 GiB refusal',
               'n_lanes == 0'):
    assert word in note, word


def _abi_case(fam):
  if fam == 'mountain_car':
    return _native.MountainCarCfg(1000, 0), _native.MountainCarCfg(0, 0)
  good = dict(swingup=0, last_step=1001, height_threshold=0.8, x_threshold=3.0, theta_dot_threshold=1.0, x_reward_threshold=1.0,
              timescale=0.01, mass_cart=1.0, mass_pole=0.1, length=0.5, force_mag=10.0, gravity=9.8, move_cost=0.0, init_range=0.05,
              theta_offset=0.0, time_frac=0xDEAD0008)
  return _native.CartpoleCfg(**good), _native.CartpoleCfg(**dict(good, last_step=0))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam', ['cartpole', 'mountain_car'])
def test_argument_checks_of_the_entry_points(fam, kind):
  """Every refusal comes before any device work: garbage stands in for device pointers, none is dereferenced, and every call
  here is refused or empty — none reaches a launch.  The codes and their order are those of bsx_<family>_<kind>_evaluate; a
  non-zero epsilon and a bad inv_temperature are BSX_ERANGE where an epsilon outside [0, 1] is there: after the modes and the
  scalars, before an empty call returns, before the pointers."""
  fn = getattr(_native.lib, ENTRY[fam, kind])
  cfg, bad_cfg = _abi_case(fam)
  junk = 0xDEAD0010                                                # never mapped: a dereference would fault (16-byte aligned)
  E = _native
  D = 3 if fam == 'mountain_car' else 6
  nan, inf = float('nan'), float('inf')

  def call(**kw):
    c = _native.Call(n_lanes=kw.pop('n_lanes', 4), n_steps=kw.pop('n_steps', 4), flags=kw.pop('flags', 0))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def policy(**kw):
    if kind == 'linear':
      kw.pop('hidden', None)
      d = dict(weights=junk, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, observation_in=junk)
      d.update(kw)
      return _native.Linear(**d)
    d = dict(w1=junk, w2=junk, hidden=5, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, observation_in=junk)
    d.update(kw)
    return _native.Mlp(**d)

  def run(c, q, beta=1.0, state=junk, steps=junk, out=None, info=junk, cfg_=cfg):
    out = _native.LinearEvalPtrs(junk, junk, junk, junk) if out is None else out
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, beta, state, steps, out, info)

  bad_betas = (0.0, -0.0, -1.0, nan, inf, -inf)
  # null structs
  assert run(call(), policy(), cfg_=None) == E.BSX_ENULL
  assert run(None, policy()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: before the scalars — and before a bad temperature
  for flags in (E.CALL_OBS_INDEX, E.CALL_OBS_U8, E.CALL_OBS_F16, E.CALL_OBS_BF16, E.CALL_OBS_INDEX | E.CALL_OBS_U8):
    assert run(call(flags=flags), policy(n_policies=-1, hidden=0)) == E.BSX_EMODE, flags
    assert run(call(flags=flags), policy(), beta=nan) == E.BSX_EMODE, flags
  lg = _native.Logging()
  assert run(call(logging=ctypes.pointer(lg)), policy(hidden=99)) == E.BSX_EMODE
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
  # BSX_EINVAL: the scalars, before the temperature
  for n in (0, -1):
    assert run(call(n_steps=n), policy()) == E.BSX_EINVAL
    assert run(call(n_steps=n), policy(), beta=-1.0) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), policy(), beta=inf) == E.BSX_EINVAL
  if kind == 'mlp':
    for h in (0, -1, 65, 1 << 20):
      assert run(call(), policy(hidden=h)) == E.BSX_EINVAL, h
      assert run(call(), policy(hidden=h), beta=nan) == E.BSX_EINVAL, h               # where n_policies < 1 is: before the temperature
      assert run(call(n_lanes=0), policy(hidden=h)) == E.BSX_EINVAL, h
    for h in (1, 64):
      assert run(call(n_lanes=0), policy(hidden=h)) == 0
  for n in (0, -3):
    assert run(call(), policy(n_policies=n)) == E.BSX_EINVAL
    assert run(call(), policy(n_policies=n, epsilon=0.5), beta=0.0) == E.BSX_EINVAL
  # BSX_ERANGE: epsilon must be 0.0 — also one that an epsilon-greedy call accepts — and inv_temperature finite and > 0
  for eps in (0.3, 1.0, 5e-324, -1e-9, 1.0000001, nan, inf):
    assert run(call(), policy(epsilon=eps)) == E.BSX_ERANGE, eps
  assert run(call(n_lanes=0), policy(epsilon=-0.0)) == 0                                    # (-0.0 == 0.0)
  none = {k: None for k in (('weights',) if kind == 'linear' else ('w1', 'w2')) + ('observation_in',)}
  for b in bad_betas:
    assert run(call(), policy(), beta=b) == E.BSX_ERANGE, b
    assert run(call(n_lanes=0), policy(), beta=b) == E.BSX_ERANGE, b                        # an empty call still checks its scalars
    assert run(call(), policy(**none), beta=b, state=None) == E.BSX_ERANGE, b               # ... before any pointer is looked at
  assert run(call(), policy(), cfg_=bad_cfg) == E.BSX_ERANGE
  assert run(call(flags=E.CALL_OBS_INDEX), policy(), cfg_=bad_cfg) == E.BSX_ERANGE          # (the cfg comes first)
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at; the extreme temperatures are accepted
  for b in (1.0, 5e-324, 1.7976931348623157e308):
    assert run(call(n_lanes=0), policy(**none), beta=b, state=None, steps=None, out=_native.LinearEvalPtrs(0, 0, 0, 0),
               info=None) == 0, b
  assert run(call(n_lanes=0), policy(epsilon=0.3)) == E.BSX_ERANGE
  # BSX_ENULL: every pointer — the other ones garbage
  for missing in none:
    assert run(call(), policy(**{missing: None})) == E.BSX_ENULL, missing
  for missing in ('state', 'steps', 'info'):
    assert run(call(), policy(), **{missing: None}) == E.BSX_ENULL, missing
  for k in range(4):                                                                        # every pointer of the result
    ptrs = [junk] * 4
    ptrs[k] = 0
    assert run(call(), policy(), out=_native.LinearEvalPtrs(*ptrs)) == E.BSX_ENULL, k
  assert run(call(), policy(n_policies=2)) == E.BSX_ENULL                                   # a population without policy_index
  if fam == 'cartpole':
    no_table = _abi_case(fam)[0]
    no_table.time_frac = None
    assert run(call(), policy(), cfg_=no_table) == E.BSX_ENULL
  assert run(call(n_lanes=1 << 40), policy()) == E.BSX_EINVAL                               # more workgroups than a grid holds
  assert run(call(action_ring=-2), policy()) == E.BSX_EINVAL
  # No slab is written, so a [B, D] slab of 4 GiB or more is not refused for its size: such a call goes through the checks of
  # the evaluation and stops where that one stops (a call that passed them all would be launched: none here does).  The
  # recording call's slab refusal (BSX_EINVAL) would hide none of these, so the entry points are also read: they do not name it.
  slab = -(-(1 << 32) // (4 * D))
  for lanes in (slab, 1 << 31):
    assert run(call(n_lanes=lanes), policy(), info=None) == E.BSX_ENULL, lanes
    assert run(call(n_lanes=lanes), policy(), out=_native.LinearEvalPtrs(junk, junk, junk, 0)) == E.BSX_ENULL, lanes
  # (the body of both families' entry points, stated once beside the kind's checks; the family's file delegates to it)
  dev = open(os.path.join(CSRC, 'bsx_drawn_returns.h')).read()
  body = dev[dev.index('static inline int bsx_drawn_returns_entry('):]
  body = body[:body.index('\n}\n')]
  assert 'bsx_check_drawn_returns_call(' in body and 'slab' not in body and 'bsx_check_trajectory' not in body
  hip = open(os.path.join(CSRC, fam + '.hip')).read()
  assert hip.count(f'return bsx_drawn_returns_entry<{fam}_host>(cfg, call, ') == 2 and 'slab' not in hip
  assert 'bsx_check_trajectory' not in dev and '<< 32' not in dev


# ------------------------------------------------------------------------------------------ the Python entry points
def _envs():
  return [cartpole.Cartpole(seed=0, batch=4), cartpole.CartpoleSwingup(seed=0, batch=4), mountain_car.MountainCar(seed=0, batch=4)]


def _dim(env):
  return int(np.prod(env.observation_spec().shape))


def _refused(env, kind, exc=ValueError, match=None, **kw):
  """env.evaluate_sampled_<kind>(...) raises, its message names the caller, and nothing was allocated."""
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  name = f'evaluate_sampled_{kind}'
  obs = kw.pop('observation') if 'observation' in kw else torch.zeros((4, 3), dtype=torch.float32)
  if kind == 'linear':
    pol = (kw.pop('weights') if 'weights' in kw else torch.zeros((3, 4), dtype=torch.float32),)      # (None is one of the bad values)
  else:
    pol = (kw.pop('w1') if 'w1' in kw else torch.zeros((5, 4), dtype=torch.float32),
           kw.pop('w2') if 'w2' in kw else torch.zeros((3, 6), dtype=torch.float32))
  with pytest.raises(exc, match=match or name) as info:
    getattr(env, name)(*pol, obs, kw.pop('num_steps', 4), **kw)
  assert name in str(info.value)
  assert not raw._allocated and raw._linear_eval_out is None               # pylint: disable=protected-access


def test_signatures_docstrings_and_families():
  want = dict(linear=['self', 'weights', 'observation', 'num_steps', 'policy_index', 'temperature', 'sample_seed'],
              mlp=['self', 'w1', 'w2', 'observation', 'num_steps', 'policy_index', 'temperature', 'sample_seed'])
  for kind in KINDS:
    fn = getattr(base.Environment, f'evaluate_sampled_{kind}')
    p = inspect.signature(fn).parameters
    assert list(p) == want[kind]
    assert [p[k].kind for k in ('policy_index', 'temperature', 'sample_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
    assert p['policy_index'].default is None and p['temperature'].default == 1.0 and p['sample_seed'].default == 0
    assert 'epsilon' not in p and 'explore_seed' not in p
    assert list(p) == list(inspect.signature(getattr(base.Environment, f'sample_{kind}')).parameters)       # sample_*'s arguments
    doc = ' '.join(fn.__doc__.split())
    for word in (f'sample_{kind}', 'LinearEvaluation', 'evaluate_linear', 'no TimeStep is written', 'ts = step(a); obs = ts.observation', f'{kind}_logits', 'gumbel_select', 'policy_index', 'temperature',
                 'sample_seed', 'overwritten by the next call', 'bit for bit'):
      assert word in doc, (kind, word)
    abi = lambda cls: cls._closed_loop_abi(object.__new__(cls), f'evaluate_sampled_{kind}')   # pylint: disable=protected-access,cell-var-from-loop
    assert abi(cartpole.Cartpole) == abi(cartpole.CartpoleSwingup) == ENTRY['cartpole', kind]
    assert abi(mountain_car.MountainCar) == ENTRY['mountain_car', kind] and ENTRY['cartpole', kind] in _native.EXPORTED
    assert abi(base.Environment) is None and abi(catch.Catch) is None and ENTRY['mountain_car', kind] in _native.EXPORTED
    # the refusals are sample_*'s, in its order — two faults at a time, the earlier one's message — without the slab, all
    # before the allocation
    for env in _envs():
      D, first = _dim(env), 'weights' if kind == 'linear' else 'w1'
      shapes = dict(weights=(3, D + 1)) if kind == 'linear' else dict(w1=(5, D + 1), w2=(3, 6))
      env._device = torch.device('cpu')
      good = dict({k: torch.zeros(v) for k, v in shapes.items()}, observation=torch.zeros((4, D)))
      _refused(env, kind, match=f'{first} must be', temperature=0.0, **dict(good, **{first: None}))
      _refused(env, kind, match='temperature must be', temperature=0.0, sample_seed=-1, **good)
      env._device = torch.device('meta')                                   # tensors without storage: a slab of 4 GiB passes the
      env._batch = -(-(1 << 32) // (4 * D))                                # arguments' checks
      big = dict({k: torch.zeros(v, device='meta') for k, v in shapes.items()}, observation=torch.zeros((env._batch, D), device='meta'))
      _refused(env, kind, match='sample_seed must be', sample_seed=-1, **big)
      with pytest.raises(RuntimeError, match='no HIP device'):             # no slab is written, none is refused: the call goes on
        getattr(env, f'evaluate_sampled_{kind}')(*list(big.values())[:-1], big['observation'], 4)     # to allocate (never on 'meta')
      assert not env._allocated and env._linear_eval_out is None and not env._policy_rollout_out


def test_views_families_and_modes_are_refused():
  for kind in KINDS:
    for env in (cartpole.Cartpole(seed=0), cartpole.CartpoleSwingup(seed=0), mountain_car.MountainCar(seed=0)):
      _refused(env, kind, match='batched view')
    for bsuite_id in ('bandit/0', 'deep_sea/0', 'catch/0', 'memory_len/0', 'umbrella_length/0', 'discounting_chain/0'):
      _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), kind, match='mountain_car only')
    _refused(catch.Catch(seed=0, batch=4, observation_mode='index'), kind, match='mountain_car only')
    for cls in (cartpole.Cartpole, cartpole.CartpoleSwingup, mountain_car.MountainCar):
      _refused(cls(seed=0, batch=4, rng='mt19937'), kind, match='philox')
    for env in _envs():
      env._logging = dict(steps=None)           # what enable_logging() leaves behind (it allocates: not without a GPU)
      _refused(env, kind, match='Logging')
    for env in _envs():
      env._grouped_by = object()                # what SweepBatch sets while its prepared groups hold the column pointers
      _refused(env, kind, exc=RuntimeError, match='release_groups')


def test_the_wrappers_refuse_instead_of_delegating():
  for kind in KINDS:
    name = f'evaluate_sampled_{kind}'
    for make in (lambda e: wrappers.RewardNoise(e, noise_scale=0.5, seed=1), lambda e: wrappers.RewardScale(e, reward_scale=2.0)):
      for raw in _envs():
        _refused(make(raw), kind, match='not available through')
        _refused(raw, kind, match='reward wrapper')                       # ... and the raw environment knows it is wrapped
    for bsuite_id in ('cartpole_noise/2', 'cartpole_scale/4', 'mountain_car_noise/3', 'mountain_car_scale/1'):
      env = bsuite_amd.load_from_id(bsuite_id, batch=4)
      assert hasattr(env, 'raw_env'), bsuite_id
      _refused(env, kind, match='not available through')
    # every wrapper class carries its own method (attribute delegation would reach the raw environment's)
    for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
      fn = getattr(cls, name)
      assert fn is not getattr(base.Environment, name) and any(name in vars(c) for c in cls.__mro__[:-1]), cls
      args = (torch.zeros((3, 4)),) if kind == 'linear' else (torch.zeros((5, 4)), torch.zeros((3, 6)))
      with pytest.raises(ValueError, match=name):
        fn(object.__new__(cls), *args, torch.zeros((4, 3)), 4, temperature=2.0, sample_seed=1)
    image = wrappers.ImageObservation(mountain_car.MountainCar(seed=0, batch=4), (84, 84, 1))
    _refused(image, kind, match='not available through ImageObservation')


def test_arguments_are_checked_before_any_gpu_use():
  for env in _envs():
    env._device = torch.device('cpu')       # the checks themselves, on host tensors: dtype, shape, contiguity
    D, H = _dim(env), 5
    w, pw = torch.zeros((3, D + 1)), torch.zeros((4, 3, D + 1))
    w1, w2, p1, p2 = torch.zeros((H, D + 1)), torch.zeros((3, H + 1)), torch.zeros((4, H, D + 1)), torch.zeros((4, 3, H + 1))
    obs = torch.zeros((4, 1, D), dtype=torch.float32)
    idx = torch.zeros(4, dtype=torch.int32)
    for kind, ok, pop in (('linear', dict(weights=w), dict(weights=pw)), ('mlp', dict(w1=w1, w2=w2), dict(w1=p1, w2=p2))):
      name = f'evaluate_sampled_{kind}'
      for t in (0.0, -1.0, -0.0, float('nan'), float('inf'), float('-inf'), 5e-324, 1e-310, '1.0', None, True, [1.0]):
        _refused(env, kind, temperature=t, observation=obs, match=f'{name}: temperature', **ok)
      for n in (0, -1, 2.0, None, '4', True):
        _refused(env, kind, num_steps=n, observation=obs, match=f'{name}: num_steps', **ok)
      for seed in (-1, 1 << 64, 0.5, None, True, '3'):
        _refused(env, kind, sample_seed=seed, observation=obs, match=f'{name}: sample_seed', **ok)
      for word in ('epsilon', 'explore_seed'):                             # there is no epsilon: the softmax explores
        with pytest.raises(TypeError, match=word):
          getattr(env, name)(*ok.values(), obs, 4, **{word: 0})
      for bad in (obs.to(torch.float64), obs.numpy(), torch.zeros((4, D + 1)), torch.zeros((3, 1, D)), torch.zeros(4 * D),
                  torch.zeros((4, 2 * D))[:, ::2], None):
        _refused(env, kind, observation=bad, match=f'{name}: observation must be', **ok)
      _refused(env, kind, observation=torch.zeros((4, D)), policy_index=idx, match='must be None', **ok)
      for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)[::2]):
        _refused(env, kind, observation=obs, policy_index=bad, match='policy_index', **pop)
    for bad in (w.to(torch.float64), w.numpy(), torch.zeros((3, D)), torch.zeros((2, D + 1)), torch.zeros((0, 3, D + 1)),
                torch.zeros((3, 2 * (D + 1)))[:, ::2], None):
      _refused(env, 'linear', weights=bad, observation=obs, match='evaluate_sampled_linear: weights must be')
    for bad in (w1.to(torch.float64), torch.zeros((H, D)), torch.zeros((0, D + 1)), torch.zeros((65, D + 1)), None):
      _refused(env, 'mlp', w1=bad, w2=w2, observation=obs, match='evaluate_sampled_mlp: w1 must be')
    for bad in (w2.to(torch.float64), torch.zeros((3, H)), torch.zeros((2, H + 1)), torch.zeros((1, 3, H + 1)), None):
      _refused(env, 'mlp', w1=w1, w2=bad, observation=obs, match='evaluate_sampled_mlp: w2 must be')
    assert not env._allocated                                                       # pylint: disable=protected-access
  # host tensors for an environment on the GPU
  env = mountain_car.MountainCar(seed=0, batch=4)
  _refused(env, 'linear', weights=torch.zeros((3, 4)), observation=torch.zeros((4, 1, 3)), match='weights must be')
  _refused(env, 'mlp', observation=torch.zeros((4, 1, 3)), match='w1 must be')


# ------------------------------------------------------------------------------------------ the source text
def test_the_kernel_body_uses_the_headers():
  dev = open(os.path.join(CSRC, 'bsx_drawn_returns.h')).read()
  body = dev[dev.index('void bsx_drawn_returns_body('):]
  body = body[:body.index('\n}\n')]
  for call_ in ('bsx_linear_logits(w, o, D, l)', 'bsx_gumbel_hidden_logits<D>(', 'bsx_gumbel_draws(p.explore_seed, lane, step)',
                'bsx_gumbel_select(l, kt.beta, u.v[0], u.v[1], u.v[2])', 'bsx_policy_clamp(k0.p.policy_index[i], k0.p.n_policies)',
                'Env::reset_pending(rg)', 'bsx_pool_counts(', 'Env::template core<0, 0, true, false, false, V, true>(',
                'Env::template load_info<V>(', 'Env::template store_info<V>(', 'bsx_fresh(0u)', 'bsx_drawn_returns_view(ka)',
                'bsx_eval_accumulate(&e, type, reward)', 'small_obs_store_row<false>(k1.out.observation_out + i * D, o, D)',
                'k1.out.episodes[i] = e.n', 'k1.out.return_sum[i] = e.total', 'k1.out.episode_return_sum[i] = e.done',
                'n_last = (uint32_t)e.n', 'n_first = n_last + pending_in - (Env::reset_pending(rg) ? 1u : 0u)'):
    assert call_ in body, call_
  loop = body[body.index('for (int t = 0; t < n_steps; ++t) {'):]
  loop = loop[:loop.index('\n    }\n')]
  assert 'core<' in loop and 'bsx_gumbel_select(' in loop and loop.count('bsx_gumbel_hidden_logits<D>(') == 2
  assert 'bsx_eval_accumulate(' in loop
  assert 'if (!resets) {' in loop and loop.index('if (!resets) {') < loop.index('bsx_gumbel_draws(')       # nothing drawn on a reset
  for word in ('__syncthreads', 'atomic', 's_w[', 'Env::store', 'store_info', 'observation_in', 'bsx_pool_counts', 'epsilon', 'bsx_st<',
               'small_obs_store_row', 'bsx_at_off', '.out.'):
    assert word not in loop, word
  # three views: before the loop, per step, after the loop (+ the pooled counts)
  assert body.count('bsx_drawn_returns_view(ka)') == 4 and loop.count('bsx_drawn_returns_view(ka)') == 1
  # no second statement of any rule: no comparison of logits or scores, no logarithm, no ReLU, no hidden-layer walk of its own
  assert '#include "bsx_gumbel_device.h"' in dev and 'void bsx_gumbel_hidden_logits(' not in dev
  for f in ('bsx_drawn_returns.h', 'drawn_returns.hip'):
    text = open(os.path.join(CSRC, f)).read()
    for word in ('bsx_log(', '0x1p-32', 'z_best', 'l_best'):
      assert word not in text, (f, word)
    code = re.sub(r'//.*', '', text)
    for word in ('> 0.0f', 'bsx_mlp_argmax', 'bsx_linear_select', 'bsx_mlp_hidden(', 'bsx_mlp_accumulate(', 'bsx_philox'):
      assert word not in code, (f, word)
  hip = open(os.path.join(CSRC, 'drawn_returns.hip')).read()
  assert hip.count('__global__') == 1
  assert '__global__ void __launch_bounds__(BSX_BLOCK) bsx_drawn_returns_kernel(const bsx_drawn_returns_args a)' in hip
  for inst in ('<Fam, V, true, true>', '<Fam, V, false, true>', '<Fam, V, true, false>', '<Fam, V, false, false>'):
    assert 'bsx_drawn_returns_body' + inst in hip, inst
  for inst in ('<bsx_drawn_returns_mountain_car, 0>', '<bsx_drawn_returns_cartpole, 1>', '<bsx_drawn_returns_cartpole, 0>'):
    assert 'bsx_drawn_returns_switch' + inst in hip, inst
  assert re.search(r'struct bsx_drawn_returns_args \{\s*int32_t family;[^\n]*\n\s*int32_t n_steps;\s*bsx_trajectory_policy p;\s*'
                   r'double beta;[^\n]*\n\s*bsx_linear_eval_t out;\s*union \{\s*cartpole_env::args cartpole;\s*'
                   r'mountain_car_env::args mountain_car;\s*\} fam;', dev)
  # the neighbours keep one kernel each
  for f in ('gumbel.hip', 'linear.hip', 'mlp.hip', 'trajectory.hip', 'tab_sample.hip'):
    assert open(os.path.join(CSRC, f)).read().count('__global__') == 1, f
  # what paid for the kernel: one tagged kernel for the delta-mode lane advance of deep_sea and catch, its body the shared one
  misc = open(os.path.join(CSRC, 'misc.hip')).read()
  assert '__global__ void __launch_bounds__(BSX_BLOCK) bsx_pair_advance_delta_kernel(const bsx_pair_advance_delta_args a)' in misc
  assert 'bsx_advance_delta_body<deep_sea_fam, deep_sea_hot>(' in misc and 'bsx_advance_delta_body<catch_fam, catch_hot>(' in misc
  pair_dev = open(os.path.join(CSRC, 'bsx_pair_device.h')).read()
  assert not re.search(r'__global__[^;{]*bsx_advance_delta', pair_dev) and 'void bsx_advance_delta_body(' in pair_dev
  assert 'bsx_launch_pair_advance_delta(HotFn::FAMILY, &a, &fn, paint, cells, blocks, st)' in open(os.path.join(CSRC, 'bsx_pair_host.h')).read()


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = 'bsx_drawn_returns_kernel'
FOLDED = 'bsx_pair_advance_delta_kernel'


@needs_llvm
def test_product_library_has_the_one_new_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  assert [n for n in ks if 'drawn_returns' in n] == [NEW]                # ONE kernel for the twelve cases
  assert not any(w in NEW for w in RESERVED) and not NEW.startswith(('calib_', 'mnist_'))
  # what paid for it: the delta-mode lane advance is one kernel for deep_sea and catch
  assert sorted(n for n in ks if 'advance_delta' in n) == [FOLDED]
  assert not any(n.startswith('bsx_advance_delta_kernel') for n in ks)
  assert not any(w in FOLDED for w in RESERVED)
  g = ks[FOLDED]
  print(FOLDED, {k: g[k] for k in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')})
  assert g['private_segment_fixed_size'] == 0 and g['vgpr_spill_count'] == 0 and g['sgpr_spill_count'] == 0, g
  assert g['agpr_count'] == 0 and g['vgpr_count'] <= 64 and g['group_segment_fixed_size'] <= 1024, g
  k = ks[NEW]
  print(NEW, {f: k[f] for f in ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size')})
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
  assert k['agpr_count'] == 0, k
  assert k['vgpr_count'] <= 128, k
  assert k['group_segment_fixed_size'] <= 4096, k
  # the neighbours it was modelled on are untouched
  for name in ('bsx_gumbel_kernel', 'bsx_trajectory_kernel', 'bsx_linear_score_kernel', 'bsx_mlp_returns_kernel', 'bsx_tab_softmax_kernel'):
    assert name in ks, name


@needs_llvm
def test_no_store_inside_the_loops_of_the_new_kernel_and_nothing_that_waits():
  """Inside ANY loop of the kernel (the compiler marks a loop's blocks in its block comments): no global store, no flat,
  scratch or buffer access, no barrier, no LDS write, no atomic, no spill reload.  The shared policy is read from LDS inside
  the loops, and the float64 Gumbel scores are computed there."""
  _, text = ki.kernel_text(os.path.join(CSRC, 'drawn_returns.hip'), NEW)
  in_loop, inside, headers = False, [], 0
  for l in text:
    if re.match(r'^\.LBB\d+_\d+:', l) or l.startswith('; %bb.'):
      in_loop = 'Loop' in l
      headers += 'Loop Header' in l and 'Depth=1' in l
      continue
    s = l.strip()
    if in_loop and s and not s.startswith(';') and not s.startswith('.'):
      inside.append(s)
  assert headers >= 12, headers
  assert not [s for s in inside if s.startswith('global_store')]
  assert sum(s.startswith('ds_read') for s in inside) >= 6, 'the shared policy is read inside the loops'
  assert any('f64' in s for s in inside), 'the Gumbel scores are computed inside the loops'
  bad = [s for s in inside if re.match(r'flat_|scratch_|buffer_|(global|ds)_atomic|ds_write|ds_add|ds_\w*rtn|s_barrier', s)]
  assert not bad, bad
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
  # the stores exist, after the loops: the state, the info, the sums and the row
  assert any(l.strip().startswith('global_store') for l in text)
