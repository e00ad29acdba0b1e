"""CPU: observation_mode='index' of deep_sea and catch — construction, specs and properties through the wrappers, every
refusal before any GPU use, the C ABI's flag bit, width query and BSX_EMODE cases, the torch helpers against numpy, and
the new kernels' budgets and store policies in the built library."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

import bsuite_amd
from bsuite_amd import _native
from bsuite_amd.environments import catch, deep_sea
from bsuite_amd.utils import observations, wrappers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'bsuite_amd.h')

IDS = [('deep_sea/10', 1, (30, 30)), ('deep_sea_stochastic/3', 1, None), ('catch/0', 2, (10, 5)), ('catch_noise/2', 2, (10, 5)),
       ('catch_scale/4', 2, (10, 5))]


def _check(env, K, board_shape):
  cells = board_shape[0] * board_shape[1]
  assert env.observation_mode == 'index' and env.observation_dtype is torch.int32
  assert tuple(env.board_shape) == tuple(board_shape)
  spec = env.observation_spec()
  assert type(spec).__name__ == 'BoundedArray' and spec.shape == (K,) and spec.dtype == np.int32
  assert spec.minimum == -1 and spec.maximum == cells - 1


def test_construction_through_the_classes():
  _check(deep_sea.DeepSea(size=12, mapping_seed=1, seed=0, batch=8, observation_mode='index'), 1, (12, 12))
  _check(catch.Catch(rows=7, columns=3, seed=0, batch=8, observation_mode='index'), 2, (7, 3))
  _check(catch.Catch(seed=0, batch=1, observation_mode='index', observation_dtype='float32'), 2, (10, 5))


@pytest.mark.parametrize('bsuite_id,K,board_shape', IDS)
def test_load_from_id_passes_the_mode_through_the_wrappers(bsuite_id, K, board_shape):
  dense = bsuite_amd.load_from_id(bsuite_id, batch=16)
  assert dense.observation_mode == 'dense' and dense.observation_dtype is torch.float32
  shape = tuple(dense.observation_spec().shape)
  assert board_shape is None or shape == board_shape
  assert tuple(dense.board_shape) == shape
  env = bsuite_amd.load_from_id(bsuite_id, batch=16, observation_mode='index')
  _check(env, K, shape)
  _check(getattr(env, 'raw_env', env), K, shape)
  # ... and through `load`, engine keywords given either way
  name = bsuite_id.split('/')[0]
  kwargs = bsuite_amd.sweep.SETTINGS[bsuite_id]
  _check(bsuite_amd.load(name, kwargs, batch=4, observation_mode='index'), K, shape)


def test_dense_and_delta_behave_as_before():
  ds = deep_sea.DeepSea(size=12, mapping_seed=1, seed=0, batch=8)
  assert ds.observation_mode == 'dense' and ds.board_shape == (12, 12)
  spec = ds.observation_spec()
  assert type(spec).__name__ == 'Array' and spec.shape == (12, 12) and spec.dtype == np.float32
  ct = catch.Catch(rows=7, columns=3, seed=0, batch=8, observation_mode='delta')
  assert ct.observation_mode == 'delta' and ct.board_shape == (7, 3) and ct.observation_dtype is torch.float32
  spec = ct.observation_spec()
  assert type(spec).__name__ == 'BoundedArray' and spec.shape == (7, 3) and spec.minimum == 0 and spec.maximum == 1
  u8 = catch.Catch(seed=0, batch=8, observation_dtype=torch.uint8)
  assert u8.observation_mode == 'dense' and u8.observation_dtype is torch.uint8 and u8.observation_spec().dtype == np.uint8
  assert deep_sea.DeepSea(size=4, mapping_seed=1, seed=0).observation_mode == 'dense'      # the scalar view
  assert bsuite_amd.load_from_id('bandit/0', batch=4).observation_mode == 'dense'
  for bad in ('sparse', 'Index', '', None):
    with pytest.raises(ValueError):
      catch.Catch(seed=0, batch=4, observation_mode=bad)


@pytest.mark.parametrize('bsuite_id', ['bandit/0', 'cartpole/0', 'mountain_car/0', 'memory_len/0', 'umbrella_length/0',
                                       'discounting_chain/0', 'cartpole_swingup/0'])
def test_other_families_are_refused(bsuite_id):
  with pytest.raises(ValueError):
    bsuite_amd.load_from_id(bsuite_id, batch=4, observation_mode='index')


def test_mnist_is_refused():
  from bsuite_amd.environments import mnist
  from tests import golden_util as gu
  images, labels = gu.mnist_dataset()
  with pytest.raises(ValueError):
    mnist.MNISTBandit(images=images, labels=labels, seed=0, batch=4, observation_mode='index')


def test_scalar_view_narrow_dtypes_and_sweep_batch_are_refused():
  with pytest.raises(ValueError):
    deep_sea.DeepSea(size=10, mapping_seed=0, seed=0, observation_mode='index')                  # batch=None
  with pytest.raises(ValueError):
    bsuite_amd.load_from_id('catch/0', observation_mode='index')
  for dt in (torch.uint8, 'float16', torch.bfloat16):
    with pytest.raises(ValueError):
      catch.Catch(seed=0, batch=4, observation_mode='index', observation_dtype=dt)
  with pytest.raises(ValueError):
    deep_sea.DeepSea(size=10, mapping_seed=0, seed=0, batch=4, observation_mode='index', obs_allocator=lambda shape: None)
  from bsuite_amd.sweep_batch import SweepBatch
  with pytest.raises(ValueError):
    SweepBatch(['catch/0', 'deep_sea/0'], total_lanes=256, env_kwargs={'catch': dict(observation_mode='index')})


def test_group_set_is_refused_before_anything_is_allocated():
  env = catch.Catch(seed=0, batch=4, observation_mode='index', device_step_counter=True)
  with pytest.raises(ValueError):
    env._group_set(None, 0, torch.zeros(4, dtype=torch.int32))         # pylint: disable=protected-access
  assert not env._allocated                                            # pylint: disable=protected-access


def test_image_observation_and_to_image_refuse_index_observations():
  env = catch.Catch(seed=0, batch=4, observation_mode='index')
  for dt in (None, torch.float32, torch.uint8):
    with pytest.raises(TypeError):
      wrappers.ImageObservation(env, (84, 84, 1), dtype=dt)
    noisy = wrappers.RewardNoise(catch.Catch(seed=0, batch=4, observation_mode='index'), noise_scale=0.1, seed=0)
    with pytest.raises(TypeError):
      wrappers.ImageObservation(noisy, (84, 84, 1), dtype=dt)
  with pytest.raises(TypeError):
    wrappers.to_image((84, 84, 1), torch.zeros((4, 2), dtype=torch.int32))
  wrappers.ImageObservation(catch.Catch(seed=0, batch=4), (84, 84, 1))       # dense: as before


# ----------------------------------------------------------------------------------------------- the C ABI
def _define(name):
  m = re.search(r'#define\s+' + name + r'\s+(.+?)\s*(?:/\*.*)?$', open(HEADER).read(), flags=re.M)
  return eval(m.group(1), {}, {'BSX_CALL_OBS_SHIFT': 1})      # pylint: disable=eval-used  (integer shifts)


def test_native_constants_match_the_header():
  assert _native.CALL_OBS_INDEX == _define('BSX_CALL_OBS_INDEX') == 1 << 3
  assert _native.CALL_OBS_INDEX & _define('BSX_CALL_OBS_MASK') == 0
  assert _native.CALL_OBS_INDEX & _define('BSX_CALL_STATE_TAGGED') == 0
  assert _native.CALL_OBS_INDEX & _native.CALL_OBS_MASK == 0 and _native.CALL_OBS_INDEX & _native.CALL_STATE_TAGGED == 0
  assert _native.lib.bsx_abi_version() == 12 == _define('BSX_ABI_VERSION')
  assert 'bsx_observation_index_width' in _native.EXPORTED
  assert re.search(r'int\s+bsx_observation_index_width\s*\(\s*int32_t', open(HEADER).read())


def test_observation_index_width_query():
  lib = _native.lib
  for name, fam in _native.FAMILY_IDS.items():
    assert lib.bsx_observation_index_width(fam) == dict(deep_sea=1, catch=2).get(name, 0), name
  assert lib.bsx_observation_index_width(-1) == 0 and lib.bsx_observation_index_width(99) == 0
  assert lib.bsx_observation_dtypes(_native.FAMILY_IDS['deep_sea']) == 0xF       # unchanged
  assert deep_sea.DeepSea._index_width == 1 and catch.Catch._index_width == 2    # pylint: disable=protected-access


def test_flags_on_the_call_descriptor_are_set_from_the_mode():
  assert catch.Catch(seed=0, batch=4, observation_mode='index')._obs_flags == _native.CALL_OBS_INDEX   # pylint: disable=protected-access
  assert catch.Catch(seed=0, batch=4)._obs_flags == 0                                                    # pylint: disable=protected-access


def test_abi_rejects_the_index_bit_before_device_work():
  """Null device pointers throughout: every one of these calls returns BSX_EMODE before touching them."""
  lib = _native.lib
  out = _native.TimeStepPtrs(0, 0, 0, 0)
  ds = _native.DeepSeaCfg(size=10, deterministic=1, move_cost=0.001, inv_size=0.1)
  ct = _native.CatchCfg(10, 5)
  call = _native.Call(n_lanes=4, flags=_native.CALL_OBS_INDEX)
  # other families
  bandit_cfg = _native.BanditCfg(num_actions=3)
  assert lib.bsx_bandit_step(ctypes.byref(bandit_cfg), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_EMODE
  mc = _native.MountainCarCfg(max_steps=100)
  assert lib.bsx_mountain_car_step(ctypes.byref(mc), ctypes.byref(call), 0, 0, 0, out, 0) == _native.BSX_EMODE
  cp = _native.CartpoleCfg()
  assert lib.bsx_cartpole_step(ctypes.byref(cp), ctypes.byref(call), 0, 0, 0, out, 0) == _native.BSX_EMODE
  mem = _native.MemoryChainCfg(3, 1)
  assert lib.bsx_memory_chain_step(ctypes.byref(mem), ctypes.byref(call), 0, 0, 0, out, 0) == _native.BSX_EMODE
  umb = _native.UmbrellaChainCfg(3, 2)
  assert lib.bsx_umbrella_chain_step(ctypes.byref(umb), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_EMODE
  dc = _native.DiscountingChainCfg(0)
  assert lib.bsx_discounting_chain_step(ctypes.byref(dc), ctypes.byref(call), 0, 0, out) == _native.BSX_EMODE
  mn = _native.MnistCfg(num_data=1, num_pixels=1)
  assert lib.bsx_mnist_step(ctypes.byref(mn), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_EMODE
  # a non-zero element code in the same call
  for code in (_native.CALL_OBS_U8, _native.CALL_OBS_F16, _native.CALL_OBS_BF16):
    call.flags = _native.CALL_OBS_INDEX | code
    assert lib.bsx_deep_sea_step(ctypes.byref(ds), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_EMODE
    assert lib.bsx_catch_step(ctypes.byref(ct), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_EMODE
  call.flags = _native.CALL_OBS_INDEX
  # delta mode (obs_paint)
  call.obs_paint = 16
  assert lib.bsx_deep_sea_step(ctypes.byref(ds), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_EMODE
  assert lib.bsx_catch_step(ctypes.byref(ct), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_EMODE
  call.obs_paint = None
  # groups (a host-side handle: bsx_group_create allocates nothing on the device before commit)
  for fam, setter, cfg in (('deep_sea', lib.bsx_group_set_deep_sea, ds), ('catch', lib.bsx_group_set_catch, ct)):
    for group_family in (_native.FAMILY_IDS[fam], _native.FAMILY_IDS['pair_mixed'], _native.FAMILY_IDS['sweep_mixed']):
      g = ctypes.c_void_p()
      assert lib.bsx_group_create(group_family, 1, ctypes.byref(g)) == 0
      try:
        assert setter(g, 0, ctypes.byref(cfg), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_EMODE
      finally:
        lib.bsx_group_destroy(g)
  for fam, setter, cfg, args in (('bandit', lib.bsx_group_set_bandit, bandit_cfg, (0, 0, out, 0)),
                                 ('mnist', lib.bsx_group_set_mnist, mn, (0, 0, out, 0))):
    g = ctypes.c_void_p()
    assert lib.bsx_group_create(_native.FAMILY_IDS[fam], 1, ctypes.byref(g)) == 0
    try:
      assert setter(g, 0, ctypes.byref(cfg), ctypes.byref(call), *args) == _native.BSX_EMODE
    finally:
      lib.bsx_group_destroy(g)
  # ... while the same deep_sea / catch call gets past the mode checks (to the null-pointer check), with and without
  # the bit, alone or beside BSX_CALL_STATE_TAGGED
  for flags in (0, _native.CALL_OBS_INDEX, _native.CALL_OBS_INDEX | _native.CALL_STATE_TAGGED):
    call.flags = flags
    assert lib.bsx_deep_sea_step(ctypes.byref(ds), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_ENULL
    assert lib.bsx_catch_step(ctypes.byref(ct), ctypes.byref(call), 0, 0, out, 0) == _native.BSX_ENULL


# ----------------------------------------------------------------------------------------------- the torch helpers
def _dense_np(index, shape):
  cells = shape[0] * shape[1]
  out = np.zeros(index.shape[:-1] + (cells,), np.float32)
  for pos in np.ndindex(*index.shape[:-1]):
    for c in index[pos]:
      if c >= 0:
        out[pos + (c,)] = 1.0
  return out.reshape(index.shape[:-1] + shape)


@pytest.mark.parametrize('lead', [(), (5,), (3, 4)])
def test_index_to_dense_against_numpy(lead):
  rng = np.random.default_rng(0)
  for K, shape in ((1, (6, 6)), (2, (7, 3)), (2, (2, 1)), (1, (1, 1))):
    cells = shape[0] * shape[1]
    idx = rng.integers(-1, cells, size=lead + (K,)).astype(np.int32)
    if K == 2 and lead:
      idx[..., 0, 1] = idx[..., 0, 0]                       # coinciding catch cells: ONE 1
      idx[..., -1, :] = -1
    want = _dense_np(idx, shape)
    got = observations.index_to_dense(torch.from_numpy(idx), shape)
    assert got.dtype is torch.float32 and tuple(got.shape) == lead + shape
    np.testing.assert_array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    for dt in (torch.uint8, torch.float16, torch.float64):
      np.testing.assert_array_equal(observations.index_to_dense(torch.from_numpy(idx), shape, dtype=dt).to(torch.float32).numpy(), want)
    out = torch.full(lead + shape, 7.0)
    assert observations.index_to_dense(torch.from_numpy(idx), shape, out=out) is out
    np.testing.assert_array_equal(out.numpy(), want)
  with pytest.raises(ValueError):
    observations.index_to_dense(torch.zeros((4, 1), dtype=torch.int32), (3, 3), out=torch.zeros((4, 9)))


def test_index_embedding_against_numpy():
  rng = np.random.default_rng(1)
  cells, D = 21, 5
  W = rng.standard_normal((cells, D)).astype(np.float32)
  table = torch.from_numpy(np.concatenate([np.zeros((1, D), np.float32), W]))
  for lead in ((), (9,), (2, 9)):
    for K in (1, 2):
      idx = rng.integers(-1, cells, size=lead + (K,)).astype(np.int32)
      if lead:
        idx[..., 0, :] = -1
        idx[..., 1, :] = 3                                    # coinciding cells: the row counts twice in the gather
      want = np.zeros(lead + (D,), np.float32)
      for k in range(K):
        want = want + np.where(idx[..., k:k + 1] >= 0, W[np.maximum(idx[..., k], 0)], np.float32(0))
      got = observations.index_embedding(torch.from_numpy(idx), table)
      assert tuple(got.shape) == lead + (D,)
      np.testing.assert_array_equal(got.numpy(), want)
      # one-hot rows without a shared cell: the gather IS board @ W
      distinct = idx.copy()
      if K == 2:
        distinct[..., 1] = np.where(distinct[..., 1] == distinct[..., 0], -1, distinct[..., 1])
      board = _dense_np(distinct, (3, 7)).reshape(lead + (cells,))
      np.testing.assert_array_equal(observations.index_embedding(torch.from_numpy(distinct), table).numpy(),
                                    (torch.from_numpy(board) @ torch.from_numpy(W)).numpy())


# ----------------------------------------------------------------------------------------------- the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_isa as ki  # noqa: E402  pylint: disable=wrong-import-position
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
LEAN = ['bsx_index_step_kernel<deep_sea_fam, deep_sea_hot>', 'bsx_index_step_kernel<catch_fam, catch_hot>',
        'bsx_index_rollout_kernel<deep_sea_fam, deep_sea_hot>', 'bsx_index_rollout_kernel<catch_fam, catch_hot>']


@needs_llvm
def test_index_kernels_exist_within_their_budgets():
  from bsuite_amd import build
  all_k = kr.kernels(build.build())
  assert len(all_k) < 190, len(all_k)
  ks = {k['name'].split('(')[0]: k for k in all_k}
  new = [n for n in ks if 'index' in n]
  assert sorted(new) == sorted(LEAN + ['bsx_index_decode_kernel']), new           # at most 5 new kernels: these
  for name in new:
    k = ks[name]
    assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (name, k)
    assert k['group_segment_fixed_size'] <= 16 << 10, (name, k)
    assert k['vgpr_count'] <= 64 and k['agpr_count'] == 0, (name, k)                  # 8 waves per SIMD


def _stores(src, kernel):
  _, text = ki.kernel_text(os.path.join(ROOT, 'bsuite_amd', 'csrc', src), kernel)
  return [l.strip() for l in text if re.match(r'\s*global_store_', l)], text


@needs_llvm
@pytest.mark.parametrize('src,fam,width', [('deep_sea.hip', 'deep_sea_fam, deep_sea_hot', 'dword'), ('catch.hip', 'catch_fam, catch_hot', 'dwordx2')])
def test_store_policies_of_the_lean_kernels(src, fam, width):
  """An eager step's outputs are write-through (sc1, never nt), a fused rollout's non-temporal."""
  stores, text = _stores(src, f'bsx_index_step_kernel<{fam}>')
  out = [s for s in stores if s.endswith('sc1')]
  assert any(s.startswith(f'global_store_{width} ') for s in out), stores         # the index row
  assert sum(s.startswith('global_store_dword ') for s in out) >= 2 and any(s.startswith('global_store_byte ') for s in out), stores
  assert not any(re.search(r'\bnt\b', s) for s in stores), stores
  for j, l in enumerate(text):                                                     # every sc1 store brings its s_nop
    if re.match(r'\s*global_store_\w+ .* sc1', l):
      assert text[j + 1].strip().startswith('s_nop'), text[j:j + 2]
  stores, text = _stores(src, f'bsx_index_rollout_kernel<{fam}>')
  out = [s for s in stores if re.search(r'\bnt\b', s)]
  assert any(s.startswith(f'global_store_{width} ') for s in out), stores
  assert sum(s.startswith('global_store_dword ') for s in out) >= 2 and any(s.startswith('global_store_byte ') for s in out), stores
  assert not any(s.endswith('sc1') for s in stores), stores
  assert ki.loop_spill_reloads(text, min_depth=1) == 0
  assert sum(bool(re.match(r'\s*s_barrier', l)) for l in text) <= 2               # staging + the final flush: none per step


@needs_llvm
def test_decode_kernel_has_both_policies_and_no_lds():
  stores, _ = _stores('misc.hip', 'bsx_index_decode_kernel')
  assert any(s.endswith('sc1') for s in stores) and any(re.search(r'\bnt\b', s) for s in stores), stores
  from bsuite_amd import build
  k = [k for k in kr.kernels(build.build()) if k['name'].startswith('bsx_index_decode_kernel')]
  assert len(k) == 1 and k[0]['group_segment_fixed_size'] == 0 and k[0]['vgpr_count'] <= 32
