"""CPU: evaluate_policy (fused tabular rollouts that write only returns; bsx_<family>_policy_evaluate) without a GPU — the
C ABI's declaration / binding / export and argument checks; every refusal of the Python entry point, all before any GPU
use; the accumulation rule the kernel compiles (bsx_eval_accumulate in bsuite_amd/csrc/bsx_policy.h, through gcc) against
a numpy restatement of the contract over the reference's trajectories (tests/golden/.tools/policy_rollout); and the
kernel budget: ONE new kernel for both families, paid for by the two calibration-copy instantiations that are now one,
inside the register / LDS targets, with no store and no barrier inside any of its loops."""
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
from bsuite_amd.utils import wrappers
from tests import policy_eval_util as pe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')
ENTRY = dict(deep_sea='bsx_deep_sea_policy_evaluate', catch='bsx_catch_policy_evaluate')


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
    assert types == [f'const bsx_{fam}_t*', 'const bsx_call_t*', 'const bsx_policy_t*', 'int32_t*', 'bsx_policy_eval_t', 'double*']
    assert name in _native.EXPORTED
    fn = getattr(_native.lib, name)
    cfg = dict(deep_sea=_native.DeepSeaCfg, catch=_native.CatchCfg)[fam]
    assert fn.argtypes == [ctypes.POINTER(cfg), ctypes.POINTER(_native.Call), ctypes.POINTER(_native.Policy), P,
                           _native.PolicyEvalPtrs, P] and fn.restype is ctypes.c_int
    assert any(l.split()[-1] == name and ' T ' in l for l in out.splitlines())
  body = re.search(r'typedef struct \{([^}]*)\} bsx_policy_eval_t;', plain).group(1)
  fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
  assert fields == ['int32_t* episodes', 'double* return_sum', 'double* episode_return_sum']
  assert [f[0] for f in _native.PolicyEvalPtrs._fields_] == ['episodes', 'return_sum', 'episode_return_sum']    # pylint: disable=protected-access
  assert ctypes.sizeof(_native.PolicyEvalPtrs) == 24


def _abi_case(fam):
  if fam == 'deep_sea':
    return _native.DeepSeaCfg(size=10, deterministic=1, move_cost=0.001, inv_size=0.1), 100
  return _native.CatchCfg(10, 5), 250


@pytest.mark.parametrize('fam', ['deep_sea', 'catch'])
def test_argument_checks_of_the_entry_points(fam):
  """Every refusal comes before any device work: host buffers (and garbage) stand in for device pointers, none is
  dereferenced.  The codes and their order are those of bsx_<family>_policy_rollout."""
  fn = getattr(_native.lib, ENTRY[fam])
  cfg, S = _abi_case(fam)
  buf = (ctypes.c_uint8 * 64)()
  p = ctypes.addressof(buf)
  p -= p % 16
  junk = 0xDEAD0008                                                # never mapped: a dereference would fault
  E = _native

  def call(**kw):
    c = _native.Call(n_lanes=kw.pop('n_lanes', 4), n_steps=kw.pop('n_steps', 4), flags=kw.pop('flags', E.CALL_OBS_INDEX))
    for k, v in kw.items():
      setattr(c, k, v)
    return c

  def pol(**kw):
    d = dict(table=p, n_states=S, n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, actions_out=None)
    d.update(kw)
    return _native.Policy(**d)

  def run(c, q, state=p, out=None, info=p, cfg_=cfg):
    out = _native.PolicyEvalPtrs(p, p, p) if out is None else out
    return fn(ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(c) if c is not None else None,
              ctypes.byref(q) if q is not None else None, state, out, info)

  # null structs
  assert run(call(), pol(), cfg_=None) == E.BSX_ENULL
  assert run(None, pol()) == E.BSX_ENULL
  assert run(call(), None) == E.BSX_ENULL
  # BSX_EMODE: the observation code, and everything the fused loop does not carry — checked before the scalars
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
  c.stream.mt_state, c.stream.mt_pos = junk, junk
  assert run(c, pol()) == E.BSX_EMODE
  for member in ('reward_f64', 'obs_paint', 'state_alt'):
    assert run(call(**{member: junk}), pol()) == E.BSX_EMODE, member
  assert run(call(force_reset=1), pol()) == E.BSX_EMODE
  assert run(call(action_ring=4), pol()) == E.BSX_EMODE
  # BSX_EINVAL / BSX_ERANGE: the scalars — with garbage in every pointer
  wild = dict(state=junk, out=_native.PolicyEvalPtrs(junk, junk, junk), info=junk)
  for n in (0, -1):
    assert run(call(n_steps=n), pol(table=junk), **wild) == E.BSX_EINVAL
  assert run(call(n_lanes=-1), pol(table=junk), **wild) == E.BSX_EINVAL
  for s in (S - 1, S + 1, 0, -S):
    assert run(call(), pol(n_states=s, table=junk), **wild) == E.BSX_EINVAL, s
  for n in (0, -3):
    assert run(call(), pol(n_policies=n, table=junk), **wild) == E.BSX_EINVAL
  for eps in (-1e-9, 1.0000001, float('nan'), float('inf')):
    assert run(call(), pol(epsilon=eps, table=junk), **wild) == E.BSX_ERANGE, eps
  bad_cfg = _native.DeepSeaCfg(size=65) if fam == 'deep_sea' else _native.CatchCfg(1, 5)
  assert run(call(), pol(table=junk), cfg_=bad_cfg, **wild) == E.BSX_ERANGE
  # n_lanes == 0: nothing to do, nothing launched, no pointer looked at
  assert run(call(n_lanes=0), pol(table=None), state=None, out=_native.PolicyEvalPtrs(0, 0, 0), info=None) == 0
  assert run(call(n_lanes=0), pol(table=junk), **wild) == 0
  assert run(call(n_lanes=0), pol(epsilon=2.0)) == E.BSX_ERANGE                      # ... but the scalars are
  # BSX_ENULL: every pointer — the other ones garbage
  assert run(call(), pol(table=None), **wild) == E.BSX_ENULL
  assert run(call(), pol(table=junk), state=None, out=wild['out'], info=junk) == E.BSX_ENULL
  assert run(call(), pol(table=junk), state=junk, out=wild['out'], info=None) == E.BSX_ENULL
  for k in range(3):
    ptrs = [junk] * 3
    ptrs[k] = 0
    assert run(call(), pol(table=junk), state=junk, out=_native.PolicyEvalPtrs(*ptrs), info=junk) == E.BSX_ENULL, k
  assert run(call(), pol(n_policies=2, table=junk), **wild) == E.BSX_ENULL            # a population without policy_index
  assert run(call(n_lanes=1 << 40), pol(table=junk), **wild) == E.BSX_EINVAL          # more workgroups than a grid holds
  assert run(call(action_ring=-2), pol(table=junk), **wild) == E.BSX_EINVAL


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
    env.evaluate_policy(policy, kw.pop('num_steps', 4), **kw)
  assert not raw._allocated                                            # pylint: disable=protected-access
  assert raw._policy_eval_out is None                                  # pylint: disable=protected-access


def test_signature_and_result_type():
  p = inspect.signature(base.Environment.evaluate_policy).parameters
  assert list(p) == list(inspect.signature(base.Environment.rollout_policy).parameters)
  assert [p[k].kind for k in ('policy_index', 'epsilon', 'explore_seed')] == [inspect.Parameter.KEYWORD_ONLY] * 3
  assert p['policy_index'].default is None and p['epsilon'].default == 0.0 and p['explore_seed'].default == 0
  assert base.PolicyEvaluation._fields == ('episodes', 'return_sum', 'episode_return_sum')
  abi = lambda cls: cls._closed_loop_abi(object.__new__(cls), 'evaluate_policy')                                      # pylint: disable=protected-access
  assert abi(catch.Catch) == ENTRY['catch'] and abi(deep_sea.DeepSea) == ENTRY['deep_sea']
  assert abi(base.Environment) is None and abi(cartpole.Cartpole) is None and set(ENTRY.values()) <= set(_native.EXPORTED)
  doc = base.Environment.evaluate_policy.__doc__
  assert 'already running' in doc and 'index_add_' in doc              # the partial first episode; reducing by policy


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
      _refused(env, match='evaluate_policy')
      _refused(raw, match='reward wrapper')                       # ... and the raw environment knows it is wrapped
  for bsuite_id in ('catch_noise/2', 'catch_scale/4', 'deep_sea_stochastic/3'):
    env = bsuite_amd.load_from_id(bsuite_id, batch=4, observation_mode='index')
    if hasattr(env, 'raw_env'):
      _refused(env, match='evaluate_policy')
  # every wrapper class carries its own method (attribute delegation would reach the raw environment's)
  for cls in (wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    fn = getattr(cls, 'evaluate_policy')
    assert fn is not base.Environment.evaluate_policy and any('evaluate_policy' in vars(c) for c in cls.__mro__[:-1]), cls
    with pytest.raises(ValueError, match='evaluate_policy'):
      fn(object.__new__(cls), torch.zeros(4, dtype=torch.uint8), 4)
  image = wrappers.ImageObservation(catch.Catch(seed=0, batch=4), (84, 84, 1))
  _refused(image, match='evaluate_policy')


def test_arguments_are_checked_before_any_gpu_use():
  for env in (catch.Catch(seed=0, batch=4, observation_mode='index'),
              deep_sea.DeepSea(size=8, mapping_seed=0, seed=0, batch=4, observation_mode='index')):
    env._device = torch.device('cpu')       # the checks themselves, on host tensors: dtype, shape, contiguity
    S = env.policy_num_states
    ok, pop = _table(env), _table(env, 4)
    idx = torch.zeros(4, dtype=torch.int32)
    for eps in (-0.1, 1.5, float('nan'), float('inf'), '0.1', None, True):
      _refused(env, policy=ok, epsilon=eps, match='evaluate_policy: epsilon')
    for n in (0, -1, 2.0, None, '4', True):
      _refused(env, policy=ok, num_steps=n, match='evaluate_policy: num_steps')
    for seed in (-1, 1 << 64, 0.5, None):
      _refused(env, policy=ok, explore_seed=seed, match='evaluate_policy: explore_seed')
    for bad in (ok.to(torch.int32), ok.to(torch.int8), ok.numpy(), ok.tolist(), torch.zeros(S + 1, dtype=torch.uint8),
                torch.zeros(S - 1, dtype=torch.uint8), torch.zeros((2, 2, S), dtype=torch.uint8), torch.zeros((0, S), dtype=torch.uint8),
                torch.zeros(2 * S, dtype=torch.uint8)[::2], torch.zeros((), dtype=torch.uint8)):
      _refused(env, policy=bad, match='evaluate_policy: policy must be')
    _refused(env, policy=ok, policy_index=idx, match='must be None')
    for bad in (None, idx.to(torch.int64), idx.numpy(), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
      _refused(env, policy=pop, policy_index=bad, match='policy_index')
  # a host table for an environment on the GPU
  env = catch.Catch(seed=0, batch=4, observation_mode='index')
  _refused(env, policy=_table(env), match='policy must be')
  # ... and rollout_policy's own messages still name rollout_policy
  with pytest.raises(ValueError, match=r'rollout_policy\(\) needs the batched view'):
    catch.Catch(seed=0).rollout_policy(torch.zeros(250, dtype=torch.uint8), 4)


# ------------------------------------------------------------------------------------------ bsx_eval_accumulate, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('pev') / 'policy_eval_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC',
                         os.path.join(ROOT, 'tests', 'csrc', 'policy_eval_shim.c'), '-o', so])
  lib = ctypes.CDLL(so)
  lib.shim_evaluate.restype = None
  lib.shim_evaluate.argtypes = [ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 5
  return lib


def _shim_run(lib, step_type, reward):
  T, B = step_type.shape
  st = np.ascontiguousarray(step_type, np.int8)
  r = np.ascontiguousarray(reward, np.float64)
  n, total, done = np.full(B, -1, np.int32), np.full(B, np.nan), np.full(B, np.nan)
  ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  lib.shim_evaluate(T, B, ptr(st), ptr(r), ptr(n), ptr(total), ptr(done))
  return n, total, done


def test_there_are_fixtures_of_every_case():
  assert pe.FIXTURES == ['catch_6x7_eps', 'catch_greedy', 'catch_population', 'deep_sea_greedy', 'deep_sea_optimal',
                         'deep_sea_population', 'deep_sea_stochastic_eps']


def test_the_rule_by_hand(shim):
  st = np.array([[0], [1], [2], [0], [1], [1]], np.int8)
  r = np.array([[np.nan], [0.25], [1.0], [7.0], [-0.5], [0.125]])      # (the value on a FIRST step is not looked at)
  n, total, done = _shim_run(shim, st, r)
  assert n.tolist() == [1] and total.tolist() == [0.875] and done.tolist() == [1.25]
  # an episode already running when the call starts gives only its in-call rewards
  n, total, done = _shim_run(shim, st[2:], r[2:])
  assert n.tolist() == [1] and total.tolist() == [0.625] and done.tolist() == [1.0]
  n, total, done = _shim_run(shim, st[4:], r[4:])
  assert n.tolist() == [0] and total.tolist() == [-0.375] and done.tolist() == [0.0]


@pytest.mark.parametrize('name', pe.FIXTURES)
def test_the_rule_reproduces_the_contract_on_every_fixture(shim, name):
  meta, g = pe.load(name)
  st, reward = g['step_type'], g['reward']
  assert reward.dtype == np.float64
  T = st.shape[0]
  checked = 0
  for cuts in ((T,), (T // 3, T - T // 3)):
    t0 = 0
    for n_steps in cuts:
      sl = slice(t0, t0 + n_steps)
      got = _shim_run(shim, st[sl], np.nan_to_num(reward[sl]))
      want = pe.host_loop(st[sl], reward[sl])
      np.testing.assert_array_equal(got[0], want[0], err_msg=f'{name} {cuts} episodes')
      np.testing.assert_array_equal(got[0], (st[sl] == 2).sum(axis=0))
      np.testing.assert_array_equal(pe.bits(got[1]), pe.bits(want[1]), err_msg=f'{name} {cuts} return_sum')
      np.testing.assert_array_equal(pe.bits(got[2]), pe.bits(want[2]), err_msg=f'{name} {cuts} episode_return_sum')
      checked += int(got[0].sum())
      t0 += n_steps
  assert checked > 0                                                    # episodes did end inside the fixture
  # the two contracts a caller could mean: for deep_sea the f64 sum is not the sum of the float32 rewards, in any lane
  whole = pe.host_loop(st, reward)
  f32 = pe.host_loop(st, np.nan_to_num(reward).astype(np.float32))
  if meta['family'] == 'deep_sea':
    assert (whole[1] != f32[1]).all(), name
  else:
    np.testing.assert_array_equal(pe.bits(whole[1]), pe.bits(f32[1]))   # catch pays -1 / 0 / +1: exact either way


def test_the_kernel_body_uses_the_header():
  csrc = os.path.join(ROOT, 'bsuite_amd', 'csrc')
  dev = open(os.path.join(csrc, 'bsx_pair_device.h')).read()
  assert dev.index('bsx_tab_eval_body(') > dev.index('bsx_policy_rollout_kernel(')      # a sibling placed after it
  body = dev[dev.index('bsx_tab_eval_body('):]
  body = body[:body.index('\n}\n')]
  for call_ in ('fn.policy_key(st)', 'bsx_policy_clamp(', 'bsx_policy_draws(p.explore_seed, lane, step)', 'bsx_policy_select(',
                'Fam::resets(st)', 'bsx_eval_accumulate(&e, type, reward)', 'bsx_pool_counts('):
    assert call_ in body, call_
  assert 'bsx_emit' not in body and 'bsx_st<' not in body and 'bsx_index_store' not in body
  misc = open(os.path.join(csrc, 'misc.hip')).read()
  assert 'bsx_tab_eval_body<deep_sea_fam, deep_sea_hot>' in misc and 'bsx_tab_eval_body<catch_fam, catch_hot>' in misc


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
NEW = 'bsx_tab_eval_kernel'


@needs_llvm
def test_product_library_has_the_one_new_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  new = [n for n in ks if 'eval' in n]
  assert new == [NEW], new                                              # ONE kernel for both families
  assert 'policy' not in NEW and 'index' not in NEW
  assert sorted(n for n in ks if 'policy' in n) == ['bsx_policy_rollout_kernel<catch_fam, catch_hot>',
                                                    'bsx_policy_rollout_kernel<deep_sea_fam, deep_sea_hot>']
  # what paid for it: writes_per_read 1 and 3 of bsx_calib_copy are one kernel now; 2 — the benchmark's — is as it was
  copies = sorted(n for n in ks if n.startswith('calib_copy'))
  assert copies == ['calib_copy_kernel<2>', 'calib_copy_n_kernel'], copies
  k = ks[NEW]
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
  assert k['agpr_count'] == 0, k
  assert k['vgpr_count'] <= 64, k                                       # 8 waves per SIMD
  assert 4096 <= k['group_segment_fixed_size'] <= 16 << 10, k           # the table, deep_sea's mapping, two counters


@needs_llvm
def test_no_store_and_no_barrier_inside_any_loop_of_the_new_kernel():
  """The step loops (one per family) keep everything in registers: inside ANY loop of the kernel — the compiler marks the
  blocks of a loop in its block comments — there is no global / flat / scratch store and no barrier; the table lookup of
  each family is there (ds_read_u8 and global_load_ubyte), so the loops looked at are the step loops."""
  _, text = ki.kernel_text(os.path.join(ROOT, 'bsuite_amd', 'csrc', 'misc.hip'), NEW)
  in_loop, inside, outside = False, [], []
  for l in text:
    if re.match(r'^\.LBB\d+_\d+:', l) or l.startswith('; %bb.'):
      in_loop = 'Loop' in l
      continue
    s = l.strip()
    if s and not s.startswith(';') and not s.startswith('.'):
      (inside if in_loop else outside).append(s)
  assert sum(s.startswith('ds_read_u8') for s in inside) >= 2 and sum(s.startswith('global_load_ubyte') for s in inside) >= 2, \
      'both families look the table up inside a loop'
  bad = [s for s in inside if re.match(r'(global|flat|scratch|buffer)_store|s_barrier', s)]
  assert not bad, bad
  assert not any(s.startswith('flat_') for s in inside + outside)       # the lookups are typed: LDS or global, never flat
  assert sum(s.startswith('global_store') for s in outside) >= 8        # state word + three columns, per family
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
