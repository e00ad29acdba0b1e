"""CPU: rollout_policy (fused closed-loop rollouts from a tabular policy; bsx_<family>_policy_rollout) without a GPU — every
refusal of the Python entry point, all before any GPU use; policy_num_states and utils.observations.policy_key; the C ABI's
declaration / binding / export and argument checks; the key arithmetic and the selection rule the kernels compile
(bsuite_amd/csrc/bsx_policy.h, through gcc) against trajectories of the unmodified reference
(tests/golden/.tools/policy_rollout, tools/make_policy_rollout_golden.py); and the kernel budget: both policy kernels are
in the product library at 8 waves per SIMD, the two table instantiations that could never launch are gone, and the
library still holds at most 186 kernels."""
import ctypes
import glob
import json
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
from bsuite_amd.environments import base, catch, deep_sea
from bsuite_amd.utils import observations, wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, 'tests', 'golden', '.tools', 'policy_rollout')


def _fixtures():
  out = []
  for p in sorted(glob.glob(os.path.join(FIXTURES, '*.npz'))):
    with np.load(p) as z:
      g = {k: z[k] for k in z.files}
    g['meta'] = json.loads(str(g['meta']))
    out.append(g)
  return out


def test_there_are_fixtures_of_every_case():
  names = sorted(g['meta']['name'] for g in _fixtures())
  assert names == ['catch_6x7_eps', 'catch_greedy', 'catch_population', 'deep_sea_greedy', 'deep_sea_optimal',
                   'deep_sea_population', 'deep_sea_stochastic_eps']


# ------------------------------------------------------------------------------------------ the Python entry point
def _table(env, P=None, device='cpu'):
  S = env.policy_num_states
  return torch.zeros(S if P is None else (P, S), dtype=torch.uint8, device=device)


def _refused(env, exc=ValueError, match=None, **kw):
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  policy = kw.pop('policy', None)
  if policy is None:
    try:
      policy = _table(raw)
    except ValueError:
      policy = torch.zeros(4, dtype=torch.uint8)
  with pytest.raises(exc, match=match):
    env.rollout_policy(policy, kw.pop('num_steps', 4), **kw)
  assert not raw._allocated                                            # pylint: disable=protected-access


def test_policy_num_states():
  assert deep_sea.DeepSea(size=12, mapping_seed=1, seed=0, batch=4, observation_mode='index').policy_num_states == 144
  assert deep_sea.DeepSea(size=64, mapping_seed=1, seed=0, batch=4).policy_num_states == 4096
  assert catch.Catch(seed=0, batch=4, observation_mode='index').policy_num_states == 250
  assert catch.Catch(rows=6, columns=7, seed=0, batch=4).policy_num_states == 294
  assert bsuite_amd.load_from_id('deep_sea/10', batch=4, observation_mode='index').policy_num_states == 900
  with pytest.raises(ValueError):
    bsuite_amd.load_from_id('bandit/0', batch=4).policy_num_states     # pylint: disable=expression-not-assigned


def test_the_scalar_view_is_refused():
  _refused(catch.Catch(seed=0), match='batched view')
  _refused(deep_sea.DeepSea(size=8, mapping_seed=0, seed=0), match='batched view')


def test_dense_delta_and_narrow_environments_are_refused():
  _refused(catch.Catch(seed=0, batch=4), match="observation_mode='index'")
  _refused(catch.Catch(seed=0, batch=4, observation_mode='delta'), match="observation_mode='index'")
  _refused(deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4), match="observation_mode='index'")
  for dt in (torch.uint8, 'float16', torch.bfloat16):
    _refused(catch.Catch(seed=0, batch=4, observation_dtype=dt), match="observation_mode='index'")
    _refused(deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4, observation_dtype=dt), match="observation_mode='index'")


@pytest.mark.parametrize('bsuite_id', ['bandit/0', 'cartpole/0', 'mountain_car/0', 'memory_len/0', 'umbrella_length/0',
                                       'discounting_chain/0', 'cartpole_swingup/0'])
def test_other_families_are_refused(bsuite_id):
  _refused(bsuite_amd.load_from_id(bsuite_id, batch=4), match='deep_sea and catch only')


def test_mnist_is_refused():
  from bsuite_amd.environments import mnist
  from tests import golden_util as gu
  images, labels = gu.mnist_dataset()
  _refused(mnist.MNISTBandit(images=images, labels=labels, seed=0, batch=4), match='deep_sea and catch only')


def test_mt19937_is_refused():
  _refused(catch.Catch(seed=0, batch=4, observation_mode='index', rng='mt19937'), match='philox')
  _refused(deep_sea.DeepSea(size=6, mapping_seed=0, seed=0, batch=4, observation_mode='index', rng='mt19937'), match='philox')


def test_an_environment_with_logging_enabled_is_refused():
  env = catch.Catch(seed=0, batch=4, observation_mode='index')
  env._logging = dict(steps=None)           # what enable_logging() leaves behind (it allocates: not without a GPU)
  _refused(env, match='Logging')


def test_a_segment_of_prepared_sweep_groups_is_refused():
  env = catch.Catch(seed=0, batch=4, observation_mode='index')
  env._grouped_by = object()                # what SweepBatch sets while its prepared groups hold the column pointers
  _refused(env, exc=RuntimeError, match='release_groups')


def test_the_wrappers_refuse_instead_of_delegating():
  for make in (lambda e: wrappers.RewardNoise(e, noise_scale=0.5, seed=1), lambda e: wrappers.RewardScale(e, reward_scale=2.0)):
    for raw in (catch.Catch(seed=0, batch=4, observation_mode='index'),
                deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4, observation_mode='index')):
      env = make(raw)
      _refused(env, match='rollout_policy')
      _refused(raw, match='reward wrapper')                       # ... and the raw environment knows it is wrapped
  for bsuite_id in ('catch_noise/2', 'catch_scale/4', 'deep_sea_stochastic/3'):
    env = bsuite_amd.load_from_id(bsuite_id, batch=4, observation_mode='index')
    if hasattr(env, 'raw_env'):
      _refused(env, match='rollout_policy')
  # every wrapper class carries its own method (attribute delegation would reach the raw environment's)
  for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    fn = getattr(cls, 'rollout_policy')
    assert fn is not base.Environment.rollout_policy and any('rollout_policy' in vars(c) for c in cls.__mro__[:-1]), cls
    with pytest.raises(ValueError, match='rollout_policy'):
      fn(object.__new__(cls), torch.zeros(4, dtype=torch.uint8), 4)
  image = wrappers.ImageObservation(catch.Catch(seed=0, batch=4), (84, 84, 1))
  _refused(image, match='rollout_policy')


def test_arguments_are_checked_before_any_gpu_use():
  for env in (catch.Catch(seed=0, batch=4, observation_mode='index'),
              deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4, observation_mode='index')):
    env._device = torch.device('cpu')       # the checks themselves, on host tensors: dtype, shape, contiguity
    S = env.policy_num_states
    ok, pop = _table(env), _table(env, 4)
    idx = torch.zeros(4, dtype=torch.int32)
    assert env._check_rollout_policy(ok, 4, None, 0.0, 0) == 1
    assert env._check_rollout_policy(ok.reshape(1, S), 1, None, 1.0, (1 << 64) - 1) == 1
    assert env._check_rollout_policy(pop, np.int64(7), idx, np.float32(0.5), np.uint64(5)) == 4
    for eps in (-0.1, 1.5, float('nan'), float('inf'), '0.1', None, True):
      _refused(env, policy=ok, epsilon=eps, match='epsilon')
    for n in (0, -1, 2.0, None, '4', True):
      _refused(env, policy=ok, num_steps=n, match='num_steps')
    for seed in (-1, 1 << 64, 0.5, None):
      _refused(env, policy=ok, explore_seed=seed, match='explore_seed')
    for bad in (ok.to(torch.int32), ok.to(torch.int8), ok.numpy(), ok.tolist(), torch.zeros(S + 1, dtype=torch.uint8),
                torch.zeros(S - 1, dtype=torch.uint8), torch.zeros((2, 2, S), dtype=torch.uint8), torch.zeros((0, S), dtype=torch.uint8),
                torch.zeros(2 * S, dtype=torch.uint8)[::2], torch.zeros((), dtype=torch.uint8)):
      _refused(env, policy=bad, match='policy must be')
    _refused(env, policy=ok, policy_index=idx, match='must be None')
    _refused(env, policy=ok.reshape(1, S), policy_index=idx, match='must be None')
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, policy=pop, policy_index=bad, match='policy_index')
  # a host table for an environment on the GPU
  env = catch.Catch(seed=0, batch=4, observation_mode='index')
  _refused(env, policy=_table(env), match='policy must be')


def test_signature():
  import inspect
  p = inspect.signature(base.Environment.rollout_policy).parameters
  assert list(p) == ['self', 'policy', 'num_steps', 'policy_index', 'epsilon', 'explore_seed']
  assert [p[k].kind for k in ('policy_index', 'epsilon', 'explore_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
  assert p['policy_index'].default is None and p['epsilon'].default == 0.0 and p['explore_seed'].default == 0


# ------------------------------------------------------------------------------------------ policy_key
def _key_np(rows_, shape):
  rows_ = np.asarray(rows_, np.int64)
  if rows_.shape[-1] == 1:
    return rows_[..., 0]
  return rows_[..., 0] * shape[1] + (rows_[..., 1] - (shape[0] - 1) * shape[1])


def test_policy_key_against_numpy_on_every_fixture():
  for g in _fixtures():
    shape = tuple(g['meta']['board_shape'])
    got = observations.policy_key(torch.from_numpy(g['index']), shape)
    assert got.dtype is torch.int64 and tuple(got.shape) == g['index'].shape[:2]
    np.testing.assert_array_equal(got.numpy(), _key_np(g['index'], shape))
    # the key the reference's agent used on call t is the key of the observation call t - 1 returned
    live = g['resets'][1:] == 0
    np.testing.assert_array_equal(got.numpy()[:-1][live], g['keys'][1:][live])
    if g['meta']['family'] == 'deep_sea':
      assert (got.numpy()[g['step_type'] == 2] == -1).all()                 # the terminal row: never looked up
    assert got.numpy().max() < g['meta']['n_states']
  with pytest.raises(ValueError):
    observations.policy_key(torch.zeros((4, 3), dtype=torch.int32), (3, 3))


def test_policy_key_covers_the_table_exactly():
  for shape in ((10, 5), (6, 7), (2, 1)):
    r, c = shape
    rows_ = np.array([[by * c + bx, (r - 1) * c + px] for by in range(r) for bx in range(c) for px in range(c)], np.int32)
    keys = observations.policy_key(torch.from_numpy(rows_), shape).numpy()
    np.testing.assert_array_equal(keys, np.arange(r * c * c))
  keys = observations.policy_key(torch.arange(-1, 64, dtype=torch.int32).reshape(-1, 1), (8, 8)).numpy()
  np.testing.assert_array_equal(keys, np.arange(-1, 64))


# ------------------------------------------------------------------------------------------ the C ABI
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
ENTRY = dict(deep_sea='bsx_deep_sea_policy_rollout', catch='bsx_catch_policy_rollout')


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
    assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_policy_t*', 'int32_t*', 'bsx_timestep_t', 'double*']
    assert name in _native.EXPORTED
    fn = getattr(_native.lib, name)
    cfg = dict(deep_sea=_native.DeepSeaCfg, catch=_native.CatchCfg)[fam]
    assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.Policy), P,
                           _native.TimeStepPtrs, P] and fn.restype is ctypes.c_int
    assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
  # bsx_policy_t as the header lays it out
  body = re.search(r'typedef struct \{([^}]*)\} bsx_policy_t;', plain).group(1)
  fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
  assert fields == ['const uint8_t* table', 'int32_t n_states, n_policies', 'const int32_t* policy_index', 'double epsilon',
                    'uint64_t explore_seed', 'int32_t* actions_out']
  assert [f[0] for f in _native.Policy._fields_] == ['table', 'n_states', 'n_policies', 'policy_index', 'epsilon',    # pylint: disable=protected-access
                                                     'explore_seed', 'actions_out']
  assert ctypes.sizeof(_native.Policy) == 48
  assert re.search(r'#define BSX_STREAM_POLICY 2u\b', open(os.path.join(ROOT, 'include', 'bsx_stream.h')).read())


def _abi_case(fam):
  if fam == 'deep_sea':
    return _native.DeepSeaCfg(size=10, deterministic=1, move_cost=0.001, inv_size=0.1), 100
  return _native.CatchCfg(10, 5), 250


@pytest.mark.parametrize('fam', ['deep_sea', 'catch'])
def test_argument_checks_of_the_entry_points(fam):
  """Every refusal comes before any device work: host buffers stand in for device pointers, none is dereferenced."""
  fn = getattr(_native.lib, ENTRY[fam])
  cfg, S = _abi_case(fam)
  buf = (ctypes.c_uint8 * 64)()
  p = ctypes.addressof(buf)                                      # (ctypes arrays are 16-byte aligned or better on glibc)
  p -= p % 16
  E = _native

  def call(**kw):
    c = _native.Call(n_lanes=kw.pop('n_lanes', 4), n_steps=kw.pop('n_steps', 4), flags=kw.pop('flags', E.CALL_OBS_INDEX))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def pol(**kw):
    d = dict(table=p, n_states=S, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, actions_out=p)
    d.update(kw)
    return _native.Policy(**d)

  def run(c, q, state=p, out=None, info=p, cfg_=cfg):
    out = _native.TimeStepPtrs(p, p, p, p) if out is None else out
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, state, out, info)

  # null structs
  assert run(call(), pol(), cfg_=None) == E.BSX_ENULL
  assert run(None, pol()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: the observation code, and everything the fused rollout does not carry — checked before the scalars
  for flags in (0, E.CALL_STATE_TAGGED, E.CALL_OBS_U8, E.CALL_OBS_INDEX | E.CALL_OBS_U8, E.CALL_OBS_INDEX | E.CALL_OBS_F16,
                E.CALL_OBS_INDEX | E.CALL_OBS_BF16):
    assert run(call(flags=flags), pol(n_states=-1)) == E.BSX_EMODE, flags
  lg = _native.Logging()
  assert run(call(logging=ctypes.pointer(lg)), pol()) == E.BSX_EMODE
  for kind in (E.WRAP_SCALE, E.WRAP_NOISE, E.WRAP_SCALE_NOISE, E.WRAP_NOISE_SCALE):
    c = call()
    c.wrap.kind = kind
    assert run(c, pol()) == E.BSX_EMODE, kind
  c = call()
  c.stream.mt_state, c.stream.mt_pos = p, p
  assert run(c, pol()) == E.BSX_EMODE
  for member in ('reward_f64', 'obs_paint', 'state_alt'):
    assert run(call(**{member: p}), pol()) == E.BSX_EMODE, member
  assert run(call(force_reset=1), pol()) == E.BSX_EMODE
  assert run(call(action_ring=4), pol()) == E.BSX_EMODE
  # BSX_EINVAL / BSX_ERANGE: the scalars
  for n in (0, -1):
    assert run(call(n_steps=n), pol()) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), pol()) == E.BSX_EINVAL
  for s in (S - 1, S + 1, 0, -S):
    assert run(call(), pol(n_states=s)) == E.BSX_EINVAL, s
  for n in (0, -3):
    assert run(call(), pol(n_policies=n)) == E.BSX_EINVAL
  for eps in (-1e-9, 1.0000001, float('nan'), float('inf')):
    assert run(call(), pol(epsilon=eps)) == E.BSX_ERANGE, eps
  bad_cfg = _native.DeepSeaCfg(size=65) if fam == 'deep_sea' else _native.CatchCfg(1, 5)
  assert run(call(), pol(), cfg_=bad_cfg) == E.BSX_ERANGE
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at
  assert run(call(n_lanes=0), pol(table=None, actions_out=None), state=None, out=_native.TimeStepPtrs(0, 0, 0, 0), info=None) == 0
  assert run(call(n_lanes=0), pol(epsilon=2.0)) == E.BSX_ERANGE                      # ... but the scalars are
  # BSX_ENULL: every pointer
  assert run(call(), pol(table=None)) == E.BSX_ENULL
  assert run(call(), pol(actions_out=None)) == E.BSX_ENULL
  assert run(call(), pol(), state=None) == E.BSX_ENULL
  assert run(call(), pol(), info=None) == E.BSX_ENULL
  for k in range(4):
    ptrs = [p] * 4
    ptrs[k] = 0
    assert run(call(), pol(), out=_native.TimeStepPtrs(*ptrs)) == E.BSX_ENULL, k
  assert run(call(), pol(n_policies=2)) == E.BSX_ENULL                               # a population without policy_index
  assert run(call(), pol(), out=_native.TimeStepPtrs(p, p, p, p + 4)) == E.BSX_EALIGN
  assert run(call(n_lanes=1 << 40), pol()) == E.BSX_EINVAL                           # more workgroups than a grid holds


# ------------------------------------------------------------------------------------------ bsx_policy.h, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('pol') / 'policy_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC',
                         os.path.join(ROOT, 'tests', 'csrc', 'policy_shim.c'), '-o', so])
  lib = ctypes.CDLL(so)
  P = ctypes.c_void_p
  lib.shim_select.restype = ctypes.c_int32
  lib.shim_select.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                              ctypes.c_uint32]
  lib.shim_draws.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, P]
  lib.shim_actions.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, P, P, P, ctypes.c_int32, ctypes.c_int32,
                               P, ctypes.c_double, ctypes.c_uint64, P, ctypes.c_uint64, ctypes.c_uint32, P, P]
  lib.shim_stream_id.restype = ctypes.c_uint32
  return lib


def _ptr(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def test_constants_and_table_sizes(shim):
  assert shim.shim_stream_id() == 2
  assert shim.shim_lds_bytes() == 4096
  for n in (1, 8, 30, 64):
    assert shim.shim_states_deep_sea(n) == n * n
  assert shim.shim_states_deep_sea(64) <= shim.shim_lds_bytes()          # every deep_sea table is staged in LDS
  for r, c in ((10, 5), (6, 7), (2, 1), (64, 64)):
    assert shim.shim_states_catch(r, c) == r * c * c
  assert [shim.shim_clamp(v, 4) for v in (-5, -1, 0, 3, 4, 1 << 30)] == [0, 0, 0, 3, 3, 3]
  assert shim.shim_key_deep_sea(-1) == -1 and shim.shim_key_deep_sea(17) == 17
  assert shim.shim_key_catch(3 * 5 + 2, 9 * 5 + 4, 10, 5) == (3 * 5 + 2) * 5 + 4


def test_exploration_draws_are_block_0_of_stream_2(shim):
  from oracle import stream as S
  out = np.zeros(4, np.uint32)
  for seed, lane, step in ((0, 0, 0), (77, 5, 3), ((1 << 40) + 11, (1 << 33) + 5, (1 << 34) + 77), ((1 << 64) - 1, (1 << 64) - 1, (1 << 48) - 1)):
    shim.shim_draws(seed, lane, step, _ptr(out))
    np.testing.assert_array_equal(out, S.words(seed, [lane], step, 2, 4)[0])
    assert not np.array_equal(out, S.words(seed, [lane], step, 0, 4)[0])


def test_selection_rule_by_hand(shim):
  top = 0xFFFFFFFF
  assert shim.shim_select(7, 1, 1.0, 0, 0, top, 3) == 0                 # a lane that resets: action 0, whatever else
  assert shim.shim_select(7, 0, 0.0, 0, 0, top, 3) == 7                 # epsilon == 0: the entry as it is, out of range or not
  assert shim.shim_select(255, 0, 0.0, 0, 0, 0, 2) == 255
  assert shim.shim_select(1, 0, 1.0, top, top, top, 3) == 2             # U = 1 - 2^-53 < 1: epsilon == 1 always explores
  assert shim.shim_select(1, 0, 1.0, top, top, 0, 3) == 0
  assert shim.shim_select(1, 0, 0.5, 1 << 31, 0, top, 3) == 1           # U = 0.5 exactly: not < epsilon
  assert shim.shim_select(1, 0, 0.5, (1 << 31) - 32, 0, 1 << 31, 3) == 1 == (3 * (1 << 31)) >> 32     # U just below: RandInt
  assert shim.shim_select(0, 0, 0.5, (1 << 31) - 32, top, top, 2) == 1


def test_key_and_selection_reproduce_the_reference_on_every_fixture(shim):
  """For every (t, lane): from the index row the reference returned on call t - 1, the table and the replayed draws,
  bsx_policy.h gives the key and the action of the reference's agent on call t."""
  from oracle import stream as S
  n_checked = 0
  for g in _fixtures():
    m = g['meta']
    T, B = g['actions'].shape
    K = g['index'].shape[2]
    rows_, cols = m['board_shape']
    lanes = np.ascontiguousarray(g['lanes'], np.uint64)
    table = np.ascontiguousarray(g['table'], np.uint8)
    pidx = np.ascontiguousarray(g['policy_index'], np.int32)
    for t in range(T):
      prev = np.ascontiguousarray(g['index'][t - 1] if t else np.full((B, K), -1), np.int32)
      resets = np.ascontiguousarray(g['resets'][t], np.uint8)
      keys, acts = np.zeros(B, np.int32), np.zeros(B, np.int32)
      shim.shim_actions(K, rows_, cols, B, _ptr(prev), _ptr(resets), _ptr(table), m['n_states'], m['n_policies'],
                        _ptr(pidx) if m['n_policies'] > 1 else None, m['epsilon'], m['explore_seed'], _ptr(lanes), m['step0'] + t,
                        m['num_actions'], _ptr(keys), _ptr(acts))
      live = resets == 0
      np.testing.assert_array_equal(keys[live], g['keys'][t][live], err_msg=f'{m["name"]} t={t}')
      np.testing.assert_array_equal(acts, g['actions'][t], err_msg=f'{m["name"]} t={t}')
      # ... and the selection alone, fed the oracle's own words (oracle/stream.py shares no code with the header)
      if m['epsilon'] > 0:
        w = S.words(m['explore_seed'], lanes, m['step0'] + t, 2, 4)
        for l in range(B):
          entry = int(table[pidx[l], max(int(g['keys'][t, l]), 0)])
          a = shim.shim_select(entry, int(resets[l]), m['epsilon'], int(w[l, 0]), int(w[l, 1]), int(w[l, 2]), m['num_actions'])
          assert a == g['actions'][t, l], (m['name'], t, l)
          u = ((int(w[l, 0]) >> 5) * (1 << 26) + (int(w[l, 1]) >> 6)) * 2.0 ** -53
          assert bool(g['explored'][t, l]) == (bool(live[l]) and u < m['epsilon'])
      n_checked += B
  assert n_checked > 10000


def test_the_kernels_use_the_header(shim):
  """The device code calls the functions the shim has just checked, and tests the reset bits the step kernels test."""
  del shim
  csrc = os.path.join(ROOT, 'bsuite_amd', 'csrc')
  dev = open(os.path.join(csrc, 'bsx_pair_device.h')).read()
  body = dev[dev.index('bsx_policy_rollout_kernel('):]
  body = body[:body.index('\n}\n')]
  for call_ in ('fn.policy_key(st)', 'bsx_policy_clamp(', 'bsx_policy_draws(p.explore_seed, lane, step)', 'bsx_policy_select(', 'Fam::resets(st)'):
    assert call_ in body, call_
  ds, ct = open(os.path.join(csrc, 'deep_sea_fam.h')).read(), open(os.path.join(csrc, 'catch_fam.h')).read()
  assert 'return bsx_policy_key_deep_sea(a);' in ds and 'return (st & DS_RESET_BIT) != 0;' in ds
  assert 'return bsx_policy_key_catch(a, b, rows, cols);' in ct and 'return (st & CATCH_RESET_BIT) != 0;' in ct


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = ['bsx_policy_rollout_kernel<deep_sea_fam, deep_sea_hot>', 'bsx_policy_rollout_kernel<catch_fam, catch_hot>']
RETIRED = ['small_obs_lean_rollout_kernel<bandit_env, false, 0, true>',
           'small_obs_lean_rollout_kernel<discounting_chain_env, false, 0, true>']


@needs_llvm
def test_product_library_has_both_policy_kernels_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  for name in RETIRED:
    assert name not in ks, f'{name} can never launch (its family has no table)'
    assert name.replace('true>', 'false>') in ks
  assert sorted(n for n in ks if 'policy' in n) == sorted(NEW)
  for name in NEW:
    k = ks[name]
    assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
    assert k['agpr_count'] == 0, (name, k)
    assert k['vgpr_count'] <= 64, (name, k)                                          # 8 waves per SIMD, both families
    assert 4096 <= k['group_segment_fixed_size'] <= 16 << 10, (name, k)              # the table, the family's own, two counters


@needs_llvm
@pytest.mark.parametrize('src,fam,width', [('deep_sea.hip', 'deep_sea_fam, deep_sea_hot', 'dword'), ('catch.hip', 'catch_fam, catch_hot', 'dwordx2')])
def test_outputs_of_the_policy_kernels_are_non_temporal(src, fam, width):
  """A rollout's outputs have no reader inside the call: every column, the action column included, is
  stored non-temporal; nothing is write-through; no barrier and no spill reload inside the step loop."""
  _, text = ki.kernel_text(os.path.join(ROOT, 'bsuite_amd', 'csrc', src), f'bsx_policy_rollout_kernel<{fam}>')
  stores = [l.strip() for l in text if re.match(r'\s*global_store_', l)]
  nt = [s for s in stores if re.search(r'\bnt\b', s)]
  assert any(s.startswith(f'global_store_{width} ') for s in nt), stores           # the index row
  n_dword = sum(s.startswith('global_store_dword ') for s in nt)
  assert n_dword >= (4 if width == 'dword' else 3), stores                         # reward, discount, actions (+ deep_sea's row)
  assert any(s.startswith('global_store_byte ') for s in nt), stores               # step_type
  assert not any(s.endswith('sc1') for s in stores), stores
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
  assert sum(bool(re.match(r'\s*s_barrier', l)) for l in text) <= 2                # staging + the final flush: none per step
  assert any(re.match(r'\s*ds_read_u8', l) for l in text), 'the shared table is read from LDS'
