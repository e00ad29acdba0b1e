"""CPU: per-lane reset (step(actions, reset_mask=), mark_reset(), bsx_lane_reset_mark) without a GPU — the refusals of the
Python entry points (all before any GPU use), the C ABI's declaration / binding / export and argument checks, the word
arithmetic the marking kernel compiles (bsuite_amd/csrc/bsx_lane_reset.h, through gcc) against hand-derived words of
every family, and the kernel budget: the marking kernel is in the product library with full occupancy, the product
library holds at most 186 kernels and none of the tuning-only row-stream instantiations, the tuning build keeps them."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bsuite_amd', 'csrc')
FAM = dict(deep_sea=0, catch=1, bandit=2, memory_chain=3, umbrella_chain=4, discounting_chain=5, cartpole=6,
           mountain_car=7, mnist=8)


# ------------------------------------------------------------------------------------------ the Python entry points
def _envs():
  from bsuite_amd.environments import cartpole, catch
  from bsuite_amd.utils import wrappers
  yield catch.Catch(batch=4, seed=0)
  yield cartpole.Cartpole(batch=4, seed=0)
  yield wrappers.RewardNoise(catch.Catch(batch=4, seed=0), noise_scale=0.5, seed=1)
  yield wrappers.RewardScale(catch.Catch(batch=4, seed=0), reward_scale=2.0)


def _not_allocated(env):
  raw = env.raw_env if hasattr(env, 'raw_env') else env
  return not raw._allocated


@pytest.mark.parametrize('bad', [
    [1, 0, 0, 1],                                       # not a tensor
    np.zeros(4, bool),
    torch.zeros(4, dtype=torch.bool),                   # a host tensor: not on the environment's device
    torch.zeros(4, dtype=torch.uint8),
], ids=['list', 'numpy', 'host_bool', 'host_uint8'])
def test_masks_that_are_not_device_tensors_are_refused_before_any_gpu_use(bad):
  for env in _envs():
    a = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match='reset_mask'):
      env.step(a, reset_mask=bad)
    with pytest.raises(ValueError, match='reset_mask'):
      env.mark_reset(bad)
    assert _not_allocated(env)


def test_mask_dtype_shape_and_layout_are_checked():
  from bsuite_amd.environments import catch
  env = catch.Catch(batch=4, seed=0)
  env._device = torch.device('cpu')        # the checks themselves, on host tensors: dtype, shape, contiguity
  ok = torch.zeros(4, dtype=torch.bool)
  env._check_reset_mask(ok)
  env._check_reset_mask(ok.to(torch.uint8))
  for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int8), torch.zeros(4, dtype=torch.float32),
              torch.zeros(5, dtype=torch.bool), torch.zeros((4, 1), dtype=torch.bool), torch.zeros((), dtype=torch.bool),
              torch.zeros(8, dtype=torch.bool)[::2]):
    with pytest.raises(ValueError, match='reset_mask'):
      env._check_reset_mask(bad)
  assert not env._allocated


def test_the_scalar_view_is_refused():
  from bsuite_amd.environments import catch
  env = catch.Catch(seed=0)
  with pytest.raises(ValueError, match='batched view'):
    env.step(0, reset_mask=torch.zeros(1, dtype=torch.bool))
  with pytest.raises(ValueError, match='batched view'):
    env.mark_reset(torch.zeros(1, dtype=torch.bool))
  assert not env._allocated


def test_a_segment_of_prepared_sweep_groups_is_refused():
  from bsuite_amd.environments import catch
  env = catch.Catch(batch=4, seed=0)
  env._grouped_by = object()               # what SweepBatch sets while its prepared groups hold the column pointers
  with pytest.raises(RuntimeError, match='release_groups'):
    env.mark_reset(torch.zeros(4, dtype=torch.bool))
  with pytest.raises(RuntimeError, match='release_groups'):
    env.step(torch.zeros(4, dtype=torch.int32), reset_mask=torch.zeros(4, dtype=torch.bool))
  assert not env._allocated


def test_step_signature_keeps_the_plain_call():
  import inspect
  from bsuite_amd.environments import base
  from bsuite_amd.utils import wrappers
  for cls in (base.Environment, wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging, wrappers.ImageObservation):
    p = inspect.signature(cls.step).parameters
    assert list(p)[:3] == ['self', 'action', 'reset_mask'] and p['reset_mask'].default is None, cls
  for cls in (base.Environment, wrappers.RewardNoise, wrappers.RewardScale, wrappers.Logging):
    assert callable(getattr(cls, 'mark_reset')), cls


# ------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_export_agree_and_the_abi_stays_v12():
  from bsuite_amd import _native
  header = open(os.path.join(ROOT, 'include', 'bsuite_amd.h')).read()
  assert re.search(r'#define BSX_ABI_VERSION 12\b', header)
  assert _native.ABI_VERSION == 12 and _native.lib.bsx_abi_version() == 12
  decl = re.search(r'int bsx_lane_reset_mark\(([^;]*)\);', re.sub(r'/\*.*?\*/', '', header, flags=re.S))
  assert decl, 'include/bsuite_amd.h does not declare bsx_lane_reset_mark'
  types = [re.sub(r'\s*\w+$', '', a.strip()) for a in ' '.join(decl.group(1).split()).split(',')]
  assert types == ['int32_t', 'int32_t', 'int64_t', 'const uint8_t*', 'int32_t*', 'double*', 'int32_t', 'void*']
  assert 'bsx_lane_reset_mark' in _native.EXPORTED
  P = ctypes.c_void_p
  fn = _native.lib.bsx_lane_reset_mark
  assert fn.argtypes == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, P, P, P, ctypes.c_int32, P] and fn.restype is ctypes.c_int
  out = subprocess.check_output(['nm', '-D', '--defined-only', _native.SO_PATH], text=True)
  assert any(l.split()[-1] == 'bsx_lane_reset_mark' and ' T ' in l for l in out.splitlines())


def test_argument_checks_of_bsx_lane_reset_mark():
  """Every refusal comes before any device work: host buffers stand in for device pointers, none is dereferenced."""
  from bsuite_amd import _native
  fn = _native.lib.bsx_lane_reset_mark
  buf = (ctypes.c_uint8 * 64)()
  p = ctypes.addressof(buf)
  for fam in (-1, 9, 10, 11, 12, 1 << 20):              # outside deep_sea .. mnist (the group families included)
    assert fn(fam, 0, 4, p, p, p, 0, None) == _native.BSX_EINVAL, fam
  for fam in FAM.values():
    assert fn(fam, 0, -1, p, p, p, 0, None) == _native.BSX_EINVAL
    assert fn(fam, 0, 0, None, None, None, 1, None) == 0             # nothing to do, nothing launched
    assert fn(fam, 0, 4, None, p, p, 0, None) == _native.BSX_ENULL   # mask
    assert fn(fam, 0, 4, p, None, p, 0, None) == _native.BSX_ENULL   # state
  # info is needed exactly where the family folds: classic cartpole / mountain_car with per-episode columns
  assert fn(FAM['cartpole'], 0, 4, p, p, None, 1, None) == _native.BSX_ENULL
  assert fn(FAM['mountain_car'], 0, 4, p, p, None, 1, None) == _native.BSX_ENULL
  assert fn(FAM['cartpole'], 0, 1 << 40, p, p, p, 1, None) == _native.BSX_EINVAL     # more workgroups than a grid holds


# ------------------------------------------------------------------------------------------ the word arithmetic, through gcc
@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('lr') / 'lane_reset_shim.so')
  subprocess.check_call(['gcc', '-O2', '-std=gnu99', '-Wall', '-Werror', '-shared', '-fPIC',
                         os.path.join(ROOT, 'tests', 'csrc', 'lane_reset_shim.c'), '-o', so])
  lib = ctypes.CDLL(so)
  lib.shim_reset_word.restype = ctypes.c_int32
  lib.shim_reset_word.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_double)]
  lib.shim_reset_bit.restype = ctypes.c_int32
  return lib


def _i32(x):
  return int(np.array(x & 0xFFFFFFFF, np.uint32).view(np.int32))


def _word(shim, word, family, variant=0, folded=1):
  d = ctypes.c_double(123.0)
  w = shim.shim_reset_word(_i32(word), FAM[family], variant, folded, ctypes.byref(d))
  return w & 0xFFFFFFFF, d.value


# (family, variant, folded, word, word after the mark, info delta) — derived by hand from the layouts in include/bsuite_amd.h
WORDS = [
    # deep_sea: row | col<<8 | bad<<16 | reset<<17 | tag<<18: row 3, col 2, bad, tag 1 -> the tag stays
    ('deep_sea', 0, 1, 0x00050203, 0x00070203, 0.0),
    ('deep_sea', 0, 1, 0x00010203, 0x00030203, 0.0),              # tag 0 stays 0
    ('deep_sea', 0, 1, 0x00060808, 0x00060808, 0.0),              # after LAST: untouched
    # catch: ball_x | ball_y<<8 | paddle<<16 | reset<<24 | pending<<25: 5 pending misses stay
    ('catch', 0, 1, 0x0A020304, 0x0B020304, 0.0),
    ('catch', 0, 1, 0xFE020904, 0xFF020904, 0.0),                 # 127 pending: the sign bit is data
    ('catch', 0, 0, 0x00020304, 0x01020304, 0.0),
    ('catch', 0, 1, 0x0B020304, 0x0B020304, 0.0),
    # bandit: the word itself is the flag
    ('bandit', 0, 1, 0, 1, 0.0), ('bandit', 0, 1, 1, 1, 0.0), ('bandit', 0, 1, 7, 7, 0.0),
    # memory_chain: t | query<<20 | reset<<28
    ('memory_chain', 0, 1, 0x00300004, 0x10300004, 0.0), ('memory_chain', 0, 1, 0x10300004, 0x10300004, 0.0),
    # umbrella_chain: t | need<<20 | has<<21 | reset<<22
    ('umbrella_chain', 0, 1, 0x00300005, 0x00700005, 0.0), ('umbrella_chain', 0, 1, 0x00500005, 0x00500005, 0.0),
    # discounting_chain: t | (context + 6)<<8 | reset<<12
    ('discounting_chain', 0, 1, 0x0907, 0x1907, 0.0), ('discounting_chain', 0, 1, 0x1564, 0x1564, 0.0),
    # cartpole `steps`: k | reset<<30.  Classic, per-episode columns: the 17 rewards of +1 the episode has paid are folded
    ('cartpole', 0, 1, 17, (1 << 30) | 17, 17.0),
    ('cartpole', 0, 0, 17, (1 << 30) | 17, 0.0),                  # under Logging the columns are per step: nothing pending
    ('cartpole', 1, 1, 17, (1 << 30) | 17, 0.0),                  # swing-up accumulates per step
    ('cartpole', 0, 1, 0, 1 << 30, 0.0),                          # FIRST was the previous TimeStep: k = 0
    ('cartpole', 0, 1, (1 << 30) | 9, (1 << 30) | 9, 0.0),        # after LAST: that episode is folded already
    ('cartpole', 0, 1, 1000, (1 << 30) | 1000, 1000.0),
    # mountain_car `steps`: every step pays -1
    ('mountain_car', 0, 1, 12, (1 << 30) | 12, -12.0),
    ('mountain_car', 0, 0, 12, (1 << 30) | 12, 0.0),
    ('mountain_car', 0, 1, (1 << 30) | 12, (1 << 30) | 12, 0.0),
    ('mountain_car', 0, 1, 0, 1 << 30, 0.0),
    # mnist: index | label<<24 | reset<<28 | show<<29
    ('mnist', 0, 1, 0x2500004D, 0x3500004D, 0.0), ('mnist', 0, 1, 0x1500004D, 0x1500004D, 0.0),
]


@pytest.mark.parametrize('family,variant,folded,word,want,delta', WORDS)
def test_marked_words_against_hand_derived_values(shim, family, variant, folded, word, want, delta):
  got, d = _word(shim, word, family, variant, folded)
  assert got == want, f'{family}: {word:#010x} -> {got:#010x}, expected {want:#010x}'
  assert d == delta
  again, d2 = _word(shim, got, family, variant, folded)          # marking twice is marking once
  assert again == got and d2 == 0.0


def test_reset_bits_are_the_kernels_own(shim):
  """The bit positions in bsx_lane_reset.h against the *_RESET_BIT macros the step kernels test."""
  text = ''.join(open(os.path.join(CSRC, f)).read() for f in ('deep_sea_fam.h', 'catch_fam.h', 'mnist_fam.h', 'small_obs.h', 'bandit_env.h',
                           'memory_chain_env.h', 'umbrella_chain_env.h', 'discounting_chain_env.h', 'cartpole_env.h',
                           'mountain_car_env.h'))
  macros = {m: 1 << int(s) for m, s in re.findall(r'#define (\w+_RESET_BIT) \(1 << (\d+)\)', text)}
  want = dict(deep_sea='DS', catch='CATCH', memory_chain='MC', umbrella_chain='UC', discounting_chain='DC', cartpole='CP',
              mountain_car='CP', mnist='MN')
  assert sorted(macros) == sorted({v + '_RESET_BIT' for v in want.values()})
  for fam, prefix in want.items():
    assert shim.shim_reset_bit(FAM[fam]) == macros[prefix + '_RESET_BIT'], fam
  assert shim.shim_reset_bit(FAM['bandit']) == 0
  for fam in (-1, 9, 10, 11):
    assert shim.shim_reset_bit(fam) == -1
    d = ctypes.c_double(1.0)
    assert shim.shim_reset_word(0x1234, fam, 0, 1, ctypes.byref(d)) == 0x1234 and d.value == 0.0


def test_marking_touches_masked_running_lanes_only(shim):
  """The kernel's loop over its columns: unmasked lanes and lanes that reset anyway are not written; a second mark of the
  same lanes writes nothing and folds nothing."""
  rng = np.random.RandomState(5)
  n = 4096
  for fam, sign in (('cartpole', 1.0), ('mountain_car', -1.0)):
    k = rng.randint(0, 500, size=n).astype(np.int32)
    reset = rng.rand(n) < 0.3
    state = (k | (reset.astype(np.int32) << 30)).astype(np.int32)
    info = rng.randint(-50, 50, size=n).astype(np.float64)
    mask = (rng.rand(n) < 0.5).astype(np.uint8) * rng.randint(1, 256, size=n).astype(np.uint8)   # any non-zero byte marks
    s2, i2 = state.copy(), info.copy()
    written = np.zeros(n, np.int32)
    args = lambda: (FAM[fam], 0, ctypes.c_int64(n), mask.ctypes.data_as(ctypes.c_void_p), s2.ctypes.data_as(ctypes.c_void_p),
                    i2.ctypes.data_as(ctypes.c_void_p), 1, written.ctypes.data_as(ctypes.c_void_p))
    shim.shim_mark(*args())
    hit = (mask != 0) & ~reset
    np.testing.assert_array_equal(written != 0, hit)
    np.testing.assert_array_equal(s2, np.where(hit, state | (1 << 30), state))
    np.testing.assert_array_equal(i2, np.where(hit, info + sign * k, info))
    s3, i3 = s2.copy(), i2.copy()
    shim.shim_mark(*args())
    assert not written.any()
    np.testing.assert_array_equal(s2, s3)
    np.testing.assert_array_equal(i2, i3)


# ------------------------------------------------------------------------------------------ the kernel budget
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_resources as kr  # noqa: E402

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')
RETIRED = [f'bsx_row_stream_kernel<{rows}, {k}>' for rows in ('memory_rows', 'umbrella_rows') for k in (1, 4)]


@needs_llvm
def test_product_library_has_the_marking_kernel_inside_the_kernel_budget():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) <= 186, len(ks)
  for name in RETIRED:
    assert name not in ks, f'{name} is launched by the tuning build only'
  for rows in ('memory_rows', 'umbrella_rows'):
    assert f'bsx_row_stream_kernel<{rows}, 2>' in ks
  k = ks['bsx_lane_reset_kernel']
  assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
  assert k['agpr_count'] == 0 and k['vgpr_count'] <= 64 and k['group_segment_fixed_size'] == 0, k      # 8 waves per SIMD


@needs_llvm
def test_tuning_library_keeps_every_row_stream_instantiation():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0] for k in kr.kernels(build.build(tuning=True))}
  for name in RETIRED:
    assert name in ks, name
  assert 'bsx_lane_reset_kernel' in ks
