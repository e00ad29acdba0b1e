"""CPU: lambda_returns / td_lambda / trajectory_targets (bsuite_amd/utils/returns.py) and the host side of bsx_lambda_returns.
Every refusal is raised before any device work; the entry point's status codes in their documented order, with fake pointers;
bsx_returns_t's layout against the ctypes mirror; the CPU torch path equals the numpy restatement (tests/returns_util.py) bit
for bit over the grid the GPU test runs; the two properties the definition promises (episode returns with the FIRST rule,
rlax's td_lambda where no FIRST row interrupts an episode); the kernel budget and the new kernels' resources."""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

from bsuite_amd import _native
from bsuite_amd.utils import returns as R
from tests import returns_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(x):
  return None if x is None else torch.from_numpy(np.array(x))


def _case(T=3, B=5):
  inp = ru.make_inputs(T, B)
  return {k: _t(v) for k, v in inp.items()}


# ------------------------------------------------------------------------------------------ refusals
def _refusals():
  c = _case()
  r, d, v, s, b = c['reward'], c['discount'], c['values'], c['step_type'], c['bootstrap']
  wide = torch.zeros((3, 10))
  yield 'reward not a tensor', lambda: R.lambda_returns(r.numpy(), d)
  yield 'reward float64', lambda: R.lambda_returns(r.double(), d)
  yield 'reward rank 1', lambda: R.lambda_returns(r[0], d[0])
  yield 'reward rank 3', lambda: R.lambda_returns(r[None], d[None])
  yield 'reward not contiguous', lambda: R.lambda_returns(wide[:, ::2], d)
  yield 'T = 0', lambda: R.lambda_returns(r[:0], d[:0])
  yield 'discount dtype', lambda: R.lambda_returns(r, d.double())
  yield 'discount shape', lambda: R.lambda_returns(r, d[:2])
  yield 'discount not contiguous', lambda: R.lambda_returns(r, wide[:, ::2])
  yield 'discount on another device', lambda: R.lambda_returns(r, d.to('meta'))
  yield 'values dtype', lambda: R.lambda_returns(r, d, v.double())
  yield 'values [T,B]', lambda: R.lambda_returns(r, d, v[:3])
  yield 'values not contiguous', lambda: R.lambda_returns(r, d, torch.zeros((4, 10))[:, ::2])
  yield 'values on another device', lambda: R.lambda_returns(r, d, v.to('meta'))
  yield 'step_type dtype', lambda: R.lambda_returns(r, d, step_type=s.to(torch.int32))
  yield 'step_type shape', lambda: R.lambda_returns(r, d, step_type=s[:2])
  yield 'step_type on another device', lambda: R.lambda_returns(r, d, step_type=s.to('meta'))
  yield 'bootstrap dtype', lambda: R.lambda_returns(r, d, bootstrap=b.double())
  yield 'bootstrap shape', lambda: R.lambda_returns(r, d, bootstrap=b[None])
  yield 'bootstrap on another device', lambda: R.lambda_returns(r, d, bootstrap=b.to('meta'))
  yield 'bootstrap with values', lambda: R.lambda_returns(r, d, v, bootstrap=b)
  yield 'bootstrap with values (targets)', lambda: R.trajectory_targets(types.SimpleNamespace(reward=r, discount=d, step_type=s), v, bootstrap=b)
  for name in ('gamma', 'lambda_'):
    for bad in (True, False, float('nan'), 'x', None, -1e-9, 1.0000001, float('inf'), 1j, np.float64('nan')):
      yield f'{name} = {bad!r}', lambda name=name, bad=bad: R.lambda_returns(r, d, **{name: bad})
    yield f'{name} = 2 (td_lambda)', lambda name=name: R.td_lambda(r, d, v, **{name: 2})
  yield 'td_lambda without values', lambda: R.td_lambda(r, d, None)
  yield 'out shape', lambda: R.lambda_returns(r, d, out=torch.empty((3, 4)))
  yield 'out dtype', lambda: R.lambda_returns(r, d, out=torch.empty((3, 5), dtype=torch.float64))
  yield 'out not contiguous', lambda: R.lambda_returns(r, d, out=wide[:, ::2])
  yield 'out on another device', lambda: R.lambda_returns(r, d, out=torch.empty((3, 5), device='meta'))
  yield 'out is reward', lambda: R.lambda_returns(r, d, out=r)
  yield 'out is discount', lambda: R.lambda_returns(r, d, out=d)
  yield 'out inside values', lambda: R.lambda_returns(r, d, v, out=v[1:])
  yield 'out shares storage with bootstrap', lambda: R.lambda_returns(torch.zeros((1, 5)), torch.zeros((1, 5)), bootstrap=b, out=b.view(1, 5))


REFUSALS = list(_refusals())


@pytest.mark.parametrize('what,call', REFUSALS, ids=[w for w, _ in REFUSALS])
def test_refusals_are_value_errors_before_any_native_call(what, call, monkeypatch):
  def never(*a):
    raise AssertionError('the native entry point was called')
  monkeypatch.setattr(R._native.lib, 'bsx_lambda_returns', never, raising=False)
  with pytest.raises(ValueError):
    call()


def test_an_empty_batch_returns_empty_tensors():
  r = torch.empty((4, 0))
  out = R.lambda_returns(r, r.clone())
  assert out.shape == (4, 0) and out.dtype == torch.float32
  td = R.td_lambda(r, r.clone(), torch.empty((5, 0)))
  assert td.td_errors.shape == (4, 0) and td.returns.shape == (4, 0)
  tt = R.trajectory_targets(types.SimpleNamespace(reward=r, discount=r.clone(), step_type=torch.empty((4, 0), dtype=torch.int8)))
  assert tt.td_errors is None and tt.returns.shape == (4, 0)


# ------------------------------------------------------------------------------------------ the C ABI
def test_status_codes_in_their_documented_order_without_touching_the_gpu():
  f = _native.lib.bsx_lambda_returns
  EINVAL, ENULL, ERANGE, EMODE = -1, -2, -4, -5

  def args(**kw):
    base = dict(n_lanes=4, n_steps=3, reward=16, discount=16, step_type=16, values=None, bootstrap=None, gamma=0.5, lambda_=0.5,
                returns=16, td_errors=None)
    base.update(kw)
    return ctypes.byref(_native.Returns(**base))

  assert f(None, None) == ENULL
  # the scalars come before everything else ...
  for kw in (dict(n_steps=0), dict(n_steps=-1), dict(n_lanes=-1), dict(n_lanes=(1 << 40) + 1)):
    assert f(args(gamma=2.0, values=16, bootstrap=16, reward=None, **kw), None) == EINVAL, kw
  # ... then the range of gamma and lambda, NaN included ...
  for kw in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float('nan')), dict(lambda_=-1e-300), dict(lambda_=1.0000001),
             dict(lambda_=float('nan')), dict(gamma=float('inf'))):
    assert f(args(values=16, bootstrap=16, reward=None, n_lanes=0, **kw), None) == ERANGE, kw
  # ... then the combinations ...
  assert f(args(values=16, bootstrap=16, reward=None, n_lanes=0), None) == EMODE
  assert f(args(td_errors=16, reward=None, n_lanes=0), None) == EMODE
  # ... then the empty batch, which looks at no pointer ...
  assert f(args(n_lanes=0, reward=None, discount=None, returns=None), None) == 0
  # ... then the pointers ...
  assert f(args(reward=None), None) == ENULL
  assert f(args(discount=None), None) == ENULL
  assert f(args(returns=None), None) == ENULL
  assert f(args(returns=None, td_errors=None, values=16), None) == ENULL
  # ... and last what cannot be launched: more lanes than one grid of 256-thread workgroups holds
  assert f(args(n_lanes=1 << 40), None) == EINVAL
  assert f(args(n_lanes=(1 << 39) + 1, values=16, td_errors=16), None) == EINVAL
  assert f(args(n_lanes=1 << 38, n_steps=(1 << 31) - 1), None) == EINVAL         # the last byte offset would not fit 64 bits
  assert b'range' in _native.lib.bsx_strerror(ERANGE)


def test_struct_layout_matches_the_header():
  fields = [n for n, _ in _native.Returns._fields_]
  c_names = [('lambda' if n == 'lambda_' else n) for n in fields]
  prints = ' '.join(f'printf("%zu ", offsetof(bsx_returns_t, {n}));' for n in c_names)
  src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bsuite_amd.h"\n'
         'int main(void) { printf("%zu ", sizeof(bsx_returns_t)); ' + prints + ' return 0; }\n')
  with tempfile.TemporaryDirectory() as d:
    c, exe = os.path.join(d, 'l.c'), os.path.join(d, 'l')
    with open(c, 'w') as fh:
      fh.write(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
  want = [ctypes.sizeof(_native.Returns)] + [getattr(_native.Returns, n).offset for n in fields]
  assert got == want
  assert got[0] == 88


def test_the_documents_name_the_entry_point():
  for doc, name in (('INTEGRATION.md', 'bsx_lambda_returns'), ('DESIGN.md', 'bsx_lambda_returns'), ('README.md', 'lambda_returns')):
    assert name in open(os.path.join(ROOT, doc)).read(), doc
  assert 'bsx_lambda_returns' in _native.EXPORTED
  header = open(os.path.join(ROOT, 'include', 'bsuite_amd.h')).read()
  assert 'int bsx_lambda_returns(const bsx_returns_t* r, void* hip_stream);' in header
  assert '#define BSX_ABI_VERSION 12' in header


# ------------------------------------------------------------------------------------------ the CPU path
@pytest.mark.parametrize('T', ru.TS)
@pytest.mark.parametrize('B', ru.BS)
def test_cpu_path_equals_the_numpy_restatement_bit_for_bit(B, T):
  inp = ru.make_inputs(T, B)
  r, d = _t(inp['reward']), _t(inp['discount'])
  for gamma, lam in ru.GAMMA_LAMBDA:
    for mode, td in ru.MODES:
      for with_steps in (False, True):
        kw = ru.select(inp, mode, with_steps)
        want, want_td = ru.lambda_returns_ref(inp['reward'], inp['discount'], gamma=gamma, lambda_=lam, want_td=td, **kw)
        tk = {k: _t(v) for k, v in kw.items()}
        if td:
          got = R.td_lambda(r, d, tk['values'], gamma=gamma, lambda_=lam, step_type=tk['step_type'])
          assert np.array_equal(ru.bits(got.td_errors.numpy()), ru.bits(want_td)), (gamma, lam, mode, with_steps)
          got = got.returns
        else:
          got = R.lambda_returns(r, d, tk['values'], gamma=gamma, lambda_=lam, step_type=tk['step_type'], bootstrap=tk['bootstrap'])
        assert got.dtype == torch.float32 and tuple(got.shape) == (T, B)
        assert np.array_equal(ru.bits(got.numpy()), ru.bits(want)), (gamma, lam, mode, with_steps)


def test_cpu_path_keeps_the_sign_of_zero_and_writes_into_out():
  inp = ru.make_inputs(7, 65, neg_zero=True)
  r, d, s = _t(inp['reward']), _t(inp['discount']), _t(inp['step_type'])
  # gamma = 0: g = reward + 0 * mix, and -0.0 + 0 * mix is -0.0 under a negative mix and +0.0 otherwise
  want, _ = ru.lambda_returns_ref(inp['reward'], inp['discount'], step_type=inp['step_type'], gamma=0.0, lambda_=1.0)
  assert (ru.bits(want) == 0x80000000).any() and (ru.bits(want)[inp['reward'] == 0] == 0).any()     # both zeros are expected
  out = torch.full((7, 65), 9.0)
  got = R.lambda_returns(r, d, gamma=0.0, step_type=s, out=out)
  assert got is out
  assert np.array_equal(ru.bits(out.numpy()), ru.bits(want))


def test_monte_carlo_returns_are_the_remaining_reward_of_the_episode():
  """gamma = lambda = 1, no values, step types given: returns[t] is the reward still to come in the lane's episode, and 0 on
  FIRST rows — also where a FIRST follows a MID (the rows in front of it do not look into the new episode)."""
  for T, B in ((33, 257), (7, 64), (1, 65)):
    inp = ru.make_inputs(T, B, seed=3, small_rewards=True)
    st = inp['step_type']
    if T > 1:
      assert ((st[1:] == ru.FIRST) & (st[:-1] == ru.MID)).any() and ((st[1:] == ru.FIRST) & (st[:-1] == ru.LAST)).any()
    ts = types.SimpleNamespace(reward=_t(inp['reward']), discount=_t(inp['discount']), step_type=_t(st))
    got = R.trajectory_targets(ts)
    assert got.td_errors is None
    want = ru.remaining_episode_reward(inp['reward'], st)
    assert np.array_equal(got.returns.numpy().astype(np.float64), want)
    assert (got.returns.numpy()[st == ru.FIRST] == 0).all()


def test_td_errors_are_rlax_td_lambda_where_no_first_row_interrupts():
  """With values and no FIRST inside the window, td_errors is rlax.td_lambda(v_tm1, r_t, discount_t * gamma, v_t, lambda_):
  lambda_returns(r_t, discount_t, v_t, lambda_) - v_tm1 with
  returns[t] = r_t[t] + discount_t[t] * ((1 - lambda_) * v_t[t] + lambda_ * returns[t+1]), returns[T] = v_t[T-1]."""
  T, B = 33, 257
  inp = ru.make_inputs(T, B, seed=5)
  st = np.where(inp['step_type'] == ru.FIRST, ru.MID, inp['step_type']).astype(np.int8)
  st[0, ::2] = ru.FIRST                                                      # a FIRST at row 0 interrupts nothing
  reward = np.where(st == ru.FIRST, np.float32(0), inp['reward']).astype(np.float32)
  gamma, lam = 0.99, 0.9
  v = inp['values'].astype(np.float64)
  v_tm1, v_t = v[:-1], v[1:]
  discount_t = inp['discount'].astype(np.float64) * gamma
  ret = np.empty((T, B))
  g = v_t[-1]
  for t in reversed(range(T)):
    g = reward[t] + discount_t[t] * ((1 - lam) * v_t[t] + lam * g)
    ret[t] = g
  want = ret - v_tm1
  got = R.td_lambda(_t(reward), _t(inp['discount']), _t(inp['values']), gamma=gamma, lambda_=lam, step_type=_t(st))
  live = st != ru.FIRST
  np.testing.assert_allclose(got.td_errors.numpy()[live], want[live], rtol=0, atol=1e-5)
  np.testing.assert_allclose(got.returns.numpy()[live], ret[live], rtol=0, atol=1e-5)
  assert (got.td_errors.numpy()[~live] == 0).all()                           # exactly 0 on rows that are no transition
  # ... and without step types the same numbers on the live rows (a FIRST at row 0 has nothing above it to cut)
  plain = R.td_lambda(_t(reward), _t(inp['discount']), _t(inp['values']), gamma=gamma, lambda_=lam)
  assert np.array_equal(plain.td_errors.numpy()[live], got.td_errors.numpy()[live])


# ------------------------------------------------------------------------------------------ the built library
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_resources as kr  # noqa: E402  pylint: disable=wrong-import-position

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(kr.LLVM, 'clang-offload-bundler')) or shutil.which('c++filt') is None,
                                reason='needs the ROCm LLVM tools')


@needs_llvm
def test_two_new_kernels_inside_the_kernel_budget_without_lds_or_scratch():
  from bsuite_amd import build
  ks = {k['name'].split('(')[0]: k for k in kr.kernels(build.build())}
  assert len(ks) < 190, len(ks)
  assert len(ks) <= 186, len(ks)                                              # what the earlier features' tests hold the library to
  new = sorted(n for n in ks if 'lambda_scan' in n)
  assert len(new) == 2 and all(n.startswith('bsx_lambda_scan_kernel<') for n in new), new     # values absent / present
  for n in new:
    k = ks[n]
    print(n, {f: k[f] for f in ('vgpr_count', 'sgpr_count', 'kernarg_segment_size')})
    assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0, k
    assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['agpr_count'] == 0, k
    assert k['vgpr_count'] <= 64 and k['max_flat_workgroup_size'] == 256, k     # 8 waves per SIMD
  # what paid for them: cartpole's two-lanes-per-thread eager step, whose size gate is 0 (never), is in the tuning build alone
  assert not any(n.startswith('small_obs_eager2_kernel<cartpole_env') for n in ks)
  tuning = {k['name'].split('(')[0] for k in kr.kernels(build.build(tuning=True))}
  assert 'small_obs_eager2_kernel<cartpole_env, 0, 2>' in tuning and 'small_obs_eager2_kernel<cartpole_env, 1, 2>' in tuning
