"""GPU: per-lane reset — env.step(actions, reset_mask=m) / env.mark_reset(m).

The pin is the fixtures under tests/golden/.tools/lane_reset (tools/make_lane_reset_golden.py): B instances of the
unmodified reference, each called with reset() or step(a) as its own mask element says.  Integer / grid families and both
wrappers bit-exact, cartpole / swing-up / mountain_car teacher-forced at |a-b| <= 1e-6*max(1,|b|).

Beside them a composition check at sizes no fixture can hold: a masked call must equal the whole-batch reset() on its masked
lanes and the plain step() on the others (TimeStep, state, info, counters) — the engine's own whole-batch paths, which the
existing suite pins to the reference; it shows the marking composes with every launch path (deep_sea's single-launch step,
catch's fused tiles, the pair path, two lanes per thread), it is not a second source of expected values."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from bsuite_amd.utils import observations, wrappers
from tests import engine_util as eu
from tests import golden_util as gu

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]      # every test under its own time limit

FIXTURES = os.path.join(gu.GOLDEN_DIR, '.tools', 'lane_reset')
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FIXTURES, '*.npz')))


def _load(name):
  with np.load(os.path.join(FIXTURES, name + '.npz')) as z:
    g = {k: z[k] for k in z.files if k != 'meta'}
    meta = json.loads(str(z['meta']))
  return meta, g


def _mask(m, t=0):
  """bool and uint8 masks alternate; a uint8 mask marks with any non-zero byte."""
  m = torch.from_numpy(np.ascontiguousarray(m)).cuda()
  return (m != 0) if t % 2 == 0 else (m != 0).to(torch.uint8) * (3 + t % 200)


def _build(meta, g, **engine_kwargs):
  fam, B = meta['family'], g['mask'].shape[1]
  kwargs = dict(meta['kwargs'])
  if fam == 'mnist':
    kwargs['images'], kwargs['labels'] = gu.mnist_dataset()
  wrap = tuple(meta['wrap']) if meta['wrap'] else None
  if meta['rng'] == 'mt19937':
    import warnings
    seeds = [int(x) for x in g['lanes']]
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      env = eu.CTORS[fam](**kwargs, seed=seeds, batch=B, rng='mt19937', num_buffers=1, **engine_kwargs)
    if wrap:
      env = eu.apply_wrap(env, wrap, seeds)
  else:
    lanes = [int(x) for x in g['lanes']]
    assert lanes == list(range(lanes[0], lanes[0] + B))
    env = eu.make_env(fam, kwargs, batch=B, lane_offset=lanes[0], seed=meta['seed'], wrap=wrap, **engine_kwargs)
    eu.raw(env)._step_index = meta['step0']
  logged = None
  if meta.get('log'):
    env = logged = wrappers.Logging(env, None, log_by_step=meta['log'] == 'by_step', max_rows=g['log_rows'].shape[1] + 3)
  return env, logged


def _run_fixture(name, obs_of=None, **engine_kwargs):
  """Steps the engine through a fixture with the fixture's masks; `obs_of`: engine observation -> the dense f32 boards."""
  meta, g = _load(name)
  fam = meta['family']
  phys = fam in gu.PHYSICS
  env, logged = _build(meta, g, **engine_kwargs)
  raw = eu.raw(env)
  T, B = g['mask'].shape
  for t in range(T):
    if phys and t > 0:            # teacher-forced: the f32 state := the reference's f64 state after the previous call
      p = g['phys'][t - 1]
      st = (np.stack([p[:, 0], p[:, 1]]) if fam == 'mountain_car' else p[:, :4].T).astype(np.float32)
      raw._state['state'].copy_(torch.from_numpy(np.ascontiguousarray(st)).cuda())
    ts = env.step(torch.from_numpy(g['actions'][t]).cuda(), reset_mask=_mask(g['mask'][t], t))
    if obs_of is not None:
      ts = ts._replace(observation=obs_of(raw, ts.observation))
    st_, r, d, o = eu.to_np(ts)
    gst = g['step_type'][t]
    np.testing.assert_array_equal(st_, gst, err_msg=f'{name} step_type t={t}')
    first = gst == 0
    assert (st_[g['mask'][t] != 0] == 0).all()
    assert (r[first] == 0).all() and (d[first] == 1).all(), f'{name} t={t}: FIRST lanes carry reward 0, discount 1'
    np.testing.assert_array_equal(d[~first], g['discount'][t][~first].astype(np.float32), err_msg=f'{name} discount t={t}')
    if phys:
      eu.assert_within_tol(o, g['obs'][t], err_msg=f'{name} obs t={t}')
      eu.assert_within_tol(r[~first], g['reward'][t][~first], err_msg=f'{name} reward t={t}')
    else:
      np.testing.assert_array_equal(eu.f32_bits(r[~first]), eu.f32_bits(g['reward'][t][~first].astype(np.float32)),
                                    err_msg=f'{name} reward t={t}')
      np.testing.assert_array_equal(eu.f32_bits(o), eu.f32_bits(g['obs'][t]), err_msg=f'{name} obs t={t}')
    info = env.bsuite_info()
    for j, k in enumerate(meta['info_keys']):
      got = info[k].cpu().numpy()
      if phys:
        np.testing.assert_allclose(got, g['info'][t, :, j], rtol=1e-9, atol=1e-9, err_msg=f'{name} {k} t={t}')
      else:
        np.testing.assert_array_equal(got, g['info'][t, :, j], err_msg=f'{name} {k} t={t}')
  if logged is not None:          # the rows the unmodified reference Logging wrapper wrote, per lane
    cols = [meta['log_columns'].index(c) for c in raw.logging_columns() if not c.startswith('_')]
    keep = [j for j, c in enumerate(raw.logging_columns()) if not c.startswith('_')]
    n_rows = logged.num_rows().cpu().numpy()
    np.testing.assert_array_equal(n_rows, g['log_n_rows'], err_msg=f'{name} n_rows')
    rows = logged._lg['rows'].cpu().numpy()
    for l in range(B):
      want, got = g['log_rows'][l, :n_rows[l]][:, cols], rows[l, :n_rows[l]][:, keep]
      if phys:
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9, err_msg=f'{name} lane {l}')
      else:
        np.testing.assert_array_equal(got, want, err_msg=f'{name} lane {l}')
  assert int(raw.invalid_action_count().item()) == 0
  return raw


def test_every_case_has_a_fixture():
  assert len(NAMES) == 16, NAMES


@pytest.mark.parametrize('name', NAMES)
def test_masked_steps_reproduce_the_reference_lane_by_lane(name):
  _run_fixture(name)


@pytest.mark.parametrize('name', ['deep_sea', 'catch', 'bandit', 'cartpole', 'mountain_car'])
def test_fixture_with_the_call_index_on_the_device(name):
  raw = _run_fixture(name, device_step_counter=True)
  meta, g = _load(name)
  assert raw.device_step_index() == meta['step0'] + g['mask'].shape[0]     # marking consumed no call index


def _index_dense(raw, obs):
  return observations.index_to_dense(obs, raw.board_shape)


@pytest.mark.parametrize('name', ['deep_sea', 'deep_sea_stochastic', 'catch'])
@pytest.mark.parametrize('mode', ['delta', 'index', 'uint8', 'bfloat16'])
def test_fixture_in_every_observation_mode_and_narrow_dtype(name, mode):
  if mode == 'delta':
    _run_fixture(name, observation_mode='delta')
  elif mode == 'index':
    _run_fixture(name, obs_of=_index_dense, observation_mode='index')
  else:
    _run_fixture(name, obs_of=lambda raw, o: o.to(torch.float32), observation_dtype=mode)


# ---------------------------------------------------------------------------------------------- composition at large sizes
SIZES = (1, 1000, 4099, 1 << 18, 1 << 20, (1 << 20) + 257)
FAMILIES = {
    # name: (family, kwargs, number of actions, largest batch)
    'deep_sea_n30': ('deep_sea', dict(size=30, mapping_seed=42), 2, 1 << 18),        # the single-launch step (<= 1 GiB of boards)
    'deep_sea_n10': ('deep_sea', dict(size=10, mapping_seed=42), 2, None),           # fused tiles / the pair path
    'deep_sea_n12_stochastic': ('deep_sea', dict(size=12, deterministic=False, mapping_seed=42), 2, None),
    'catch': ('catch', dict(), 3, None),
    'bandit': ('bandit', dict(mapping_seed=3), 11, None),
    'memory_len': ('memory_chain', dict(memory_length=3, num_bits=1), 2, None),
    'memory_size': ('memory_chain', dict(memory_length=2, num_bits=12), 2, None),
    'umbrella': ('umbrella_chain', dict(chain_length=4, n_distractor=20), 2, None),
    'discounting_chain': ('discounting_chain', dict(mapping_seed=1), 5, None),
    'cartpole': ('cartpole', dict(), 3, None),
    'cartpole_swingup': ('cartpole_swingup', dict(max_time=0.05), 3, None),
    'mountain_car': ('mountain_car', dict(max_steps=6), 3, None),
    'mnist': ('mnist', dict(), 10, 1 << 18),
}
CALLS = 14
CHECK_AT = (1, 2, 4, 5, 7, 8, 11, 13)     # episodes of 1 .. 10 steps: running lanes, lanes after LAST and (call 1) after FIRST


def _same(a, b, what):
  a, b = a.cpu().numpy(), b.cpu().numpy()
  np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)


def _rows(m, x, y):
  """TimeStep fields ([B, ...]: the lane is the first dimension): x on masked lanes, y on the others."""
  return torch.where(m.view((-1,) + (1,) * (x.dim() - 1)), x, y)


def _cols(m, x, y):
  """State / info columns ([B] or [K, B]: the lane is the last dimension): x on masked lanes, y on the others."""
  return torch.where(m, x, y)


# (deep_sea N = 30 and mnist stop at 2^18 lanes: the single-launch step ends there, and larger batches of these boards
#  cross no other launch path)
@pytest.mark.parametrize('case,B', [(c, b) for c in sorted(FAMILIES) for b in SIZES if FAMILIES[c][3] is None or b <= FAMILIES[c][3]])
def test_masked_call_is_reset_on_masked_lanes_and_step_on_the_others(case, B):
  fam, kwargs, na, _ = FAMILIES[case]
  kwargs = dict(kwargs)
  if fam == 'mnist':
    kwargs['images'], kwargs['labels'] = gu.mnist_dataset()
  mk = lambda: eu.make_env(fam, kwargs, batch=B, lane_offset=11, seed=5)
  env, rst, stp = mk(), mk(), mk()
  gen = torch.Generator(device='cuda').manual_seed(B + len(case))
  density = (0.0, 1.0 / 64, 0.5, 1.0)
  for t in range(CALLS):
    a = torch.randint(0, na, (B,), generator=gen, device='cuda', dtype=torch.int32)
    m = torch.rand(B, generator=gen, device='cuda') < density[t % 4]
    if t not in CHECK_AT:
      env.step(a, reset_mask=m)
      continue
    d = env.state_dict()
    rst.load_state_dict(d)
    stp.load_state_dict(d)
    c0 = env.episode_counters().clone()
    x, y = rst.reset(), stp.step(a)
    ts = env.step(a, reset_mask=m if t % 2 else m.to(torch.uint8))
    for f in ('step_type', 'reward', 'discount', 'observation'):
      _same(getattr(ts, f), _rows(m, getattr(x, f), getattr(y, f)), f'{case} B={B} t={t} {f}')
    assert bool((ts.step_type[m] == 0).all())
    dx, dy, de = rst.state_dict(), stp.state_dict(), env.state_dict()
    for k in env._state:
      _same(de[k], _cols(m, dx[k], dy[k]), f'{case} B={B} t={t} state column {k}')
    _same(de['__info'], _cols(m, dx['__info'], dy['__info']), f'{case} B={B} t={t} info columns')
    assert de['__step_index'] == dx['__step_index'] == dy['__step_index'] == t + 1
    ix, iy, ie = rst.bsuite_info(), stp.bsuite_info(), env.bsuite_info()
    for k in ie:
      _same(ie[k], _cols(m, ix[k], iy[k]), f'{case} B={B} t={t} bsuite_info {k}')
    want = c0 + torch.stack([(ts.step_type == 2).sum(), (ts.step_type == 0).sum()])
    assert torch.equal(env.episode_counters(), want), f'{case} B={B} t={t} counters'
  assert int(env.invalid_action_count().item()) == 0


# ---------------------------------------------------------------------------------------------- the C oracle, lane by lane
# tests/test_lane_reset_oracle.py holds the oracle with per-lane reset flags to the reference's fixtures; here it gives the
# expected values at sizes the fixtures cannot hold (the integer / grid families: bit-exact).
# (deep_sea N = 30 at 4099 lanes only: a gigabyte of boards per call is the host comparison's time, not the device's)
@pytest.mark.parametrize('case,B', [(c, b) for c in ('deep_sea_n30', 'deep_sea_n10', 'deep_sea_n12_stochastic', 'catch', 'bandit',
                                                     'memory_len', 'memory_size', 'umbrella', 'discounting_chain')
                                    for b in (4099, 1 << 18) if not (c == 'deep_sea_n30' and b > 4099)])
def test_masked_steps_against_the_c_oracle_driven_lane_by_lane(case, B):
  from oracle import coracle
  fam, kwargs, na, _ = FAMILIES[case]
  seed, lane0, T = 21, 1000003, 26
  env = eu.make_env(fam, kwargs, batch=B, lane_offset=lane0, seed=seed)
  orc = coracle.OracleEnv(fam, dict(kwargs), np.arange(lane0, lane0 + B, dtype=np.uint64), seed=seed)
  rng = np.random.default_rng(B)
  for t in range(T):
    a = rng.integers(0, na, size=B).astype(np.int32)
    m = rng.random(B) < (0.0, 1.0 / 16, 0.5, 1.0 / 64, 1.0)[t % 5]
    ts = env.step(torch.from_numpy(a).cuda(), reset_mask=torch.from_numpy(m).cuda())
    orc.reset_next[m] = 1            # base.py:59-62: step() of an instance whose flag is set IS its reset()
    st, r, d, o = orc.call(a, t)
    gst, gr, gd, go = eu.to_np(ts)
    np.testing.assert_array_equal(gst, st, err_msg=f'{case} B={B} t={t} step_type')
    live = st != 0
    np.testing.assert_array_equal(eu.f32_bits(gr[live]), eu.f32_bits(r[live].astype(np.float32)), err_msg=f'{case} B={B} t={t} reward')
    np.testing.assert_array_equal(gd[live], d[live].astype(np.float32), err_msg=f'{case} B={B} t={t} discount')
    np.testing.assert_array_equal(eu.f32_bits(go), eu.f32_bits(o), err_msg=f'{case} B={B} t={t} observation')
  info = env.bsuite_info()
  for k, v in orc.bsuite_info().items():
    np.testing.assert_array_equal(info[k].cpu().numpy(), v, err_msg=f'{case} B={B} {k}')


# ---------------------------------------------------------------------------------------------- the rest of the contract
ALL = [(k,) + v[:3] for k, v in sorted(FAMILIES.items())]


@pytest.mark.parametrize('case,fam,kwargs,na', ALL)
def test_all_zero_mask_is_the_plain_step_bit_for_bit(case, fam, kwargs, na):
  B, T = 1000, 24
  kwargs = dict(kwargs)
  if fam == 'mnist':
    kwargs['images'], kwargs['labels'] = gu.mnist_dataset()
  plain = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=3)
  masked = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=3)
  zero = torch.zeros(B, dtype=torch.bool, device='cuda')
  gen = torch.Generator(device='cuda').manual_seed(1)
  for t in range(T):
    a = torch.randint(0, na, (B,), generator=gen, device='cuda', dtype=torch.int32)
    x, y = plain.step(a), masked.step(a, reset_mask=zero if t % 2 else zero.to(torch.uint8))
    if t % 3 == 0:
      masked.mark_reset(zero)
    for f in ('step_type', 'reward', 'discount', 'observation'):
      _same(getattr(y, f), getattr(x, f), f'{case} t={t} {f}')
  dx, dy = plain.state_dict(), masked.state_dict()
  assert sorted(dx) == sorted(dy)
  for k in dx:
    if torch.is_tensor(dx[k]):
      _same(dy[k], dx[k], f'{case} {k}')
    else:
      assert dx[k] == dy[k], k
  assert plain.step_index == masked.step_index == T


@pytest.mark.parametrize('case', ['deep_sea_n10', 'deep_sea_n30', 'catch', 'bandit', 'memory_len', 'discounting_chain', 'cartpole',
                                  'cartpole_swingup', 'mountain_car', 'mnist'])
def test_mark_reset_before_a_rollout_is_a_masked_first_step(case):
  fam, kwargs, na, _ = FAMILIES[case]
  B, T = 4099, 6
  kwargs = dict(kwargs)
  if fam == 'mnist':
    kwargs['images'], kwargs['labels'] = gu.mnist_dataset()
  rolled = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=8)
  stepped = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=8)
  gen = torch.Generator(device='cuda').manual_seed(2)
  for _ in range(4):
    a = torch.randint(0, na, (B,), generator=gen, device='cuda', dtype=torch.int32)
    rolled.step(a), stepped.step(a)
  acts = torch.randint(0, na, (T, B), generator=gen, device='cuda', dtype=torch.int32)
  m = torch.rand(B, generator=gen, device='cuda') < 0.3
  rolled.mark_reset(m)
  out = rolled.rollout(acts)
  assert bool((out.step_type[0][m] == 0).all())
  for t in range(T):      # (compared call by call: the stepped environment has ONE output buffer, its TimeSteps alias)
    ref = stepped.step(acts[0], reset_mask=m) if t == 0 else stepped.step(acts[t])
    for f in ('step_type', 'reward', 'discount', 'observation'):
      _same(getattr(out, f)[t], getattr(ref, f), f'{case} t={t} {f}')
  dx, dy = rolled.state_dict(), stepped.state_dict()
  for k in dx:
    if torch.is_tensor(dx[k]) and k != '__counters':      # (a rollout kernel spreads its counts over other shards: sums below)
      _same(dx[k], dy[k], f'{case} {k}')
  assert dx['__step_index'] == dy['__step_index']
  assert torch.equal(rolled.episode_counters(), stepped.episode_counters())
  for k, v in rolled.bsuite_info().items():
    _same(v, stepped.bsuite_info()[k], f'{case} bsuite_info {k}')


def test_invalid_action_count_ignores_masked_lanes():
  from bsuite_amd.environments import bandit, catch, discounting_chain
  B = 1000
  m = torch.arange(B, device='cuda') % 3 == 0
  bad = torch.full((B,), 99, dtype=torch.int32, device='cuda')
  ok = torch.zeros(B, dtype=torch.int32, device='cuda')
  for env in (catch.Catch(batch=B, seed=1), bandit.SimpleBandit(mapping_seed=1, batch=B, seed=1),
              discounting_chain.DiscountingChain(mapping_seed=1, batch=B, seed=1)):
    env.step(ok)                             # FIRST everywhere: the next call of every lane looks at its action
    assert int(env.invalid_action_count().item()) == 0
    ts = env.step(bad, reset_mask=m)
    assert bool((ts.step_type[m] == 0).all()) and bool((ts.step_type[~m] != 0).all())
    assert int(env.invalid_action_count().item()) == int((~m).sum().item()), type(env).__name__


@pytest.mark.parametrize('case', ['catch', 'cartpole', 'mountain_car', 'deep_sea_n10'])
def test_marking_twice_is_marking_once(case):
  fam, kwargs, na, _ = FAMILIES[case]
  B = 4099
  once = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=4)
  twice = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=4)
  gen = torch.Generator(device='cuda').manual_seed(3)
  for _ in range(5):
    a = torch.randint(0, na, (B,), generator=gen, device='cuda', dtype=torch.int32)
    once.step(a), twice.step(a)
  m = torch.rand(B, generator=gen, device='cuda') < 0.5
  once.mark_reset(m)
  twice.mark_reset(m)
  twice.mark_reset(m.to(torch.uint8))
  for k, v in once.bsuite_info().items():      # between the mark and the call: nothing is lost, nothing counted twice
    _same(twice.bsuite_info()[k], v, f'{case} bsuite_info {k} after the marks')
  x, y = once.step(a), twice.step(a, reset_mask=m)
  for f in ('step_type', 'reward', 'discount', 'observation'):
    _same(getattr(y, f), getattr(x, f), f'{case} {f}')
  dx, dy = once.state_dict(), twice.state_dict()
  for k in dx:
    if torch.is_tensor(dx[k]):
      _same(dy[k], dx[k], f'{case} {k}')
  for k, v in once.bsuite_info().items():
    _same(twice.bsuite_info()[k], v, f'{case} bsuite_info {k}')


def test_bsuite_info_is_unchanged_by_a_mark():
  """cartpole / mountain_car / catch report running episodes through their state word: a mark moves the pending part into
  the column (or leaves it in the word, catch) and the reported value stays what it was."""
  for case in ('cartpole', 'mountain_car', 'catch'):
    fam, kwargs, na, _ = FAMILIES[case]
    B = 4099
    env = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=6)
    gen = torch.Generator(device='cuda').manual_seed(4)
    for _ in range(40 if case == 'catch' else 5):
      env.step(torch.randint(0, na, (B,), generator=gen, device='cuda', dtype=torch.int32))
    before = {k: v.clone() for k, v in env.bsuite_info().items()}
    assert any(bool((v != 0).any()) for v in before.values())
    env.mark_reset(torch.rand(B, generator=gen, device='cuda') < 0.5)
    for k, v in env.bsuite_info().items():
      _same(v, before[k], f'{case} {k}')


@pytest.mark.parametrize('case', ['catch', 'cartpole', 'deep_sea_n30'])
def test_state_dict_taken_after_a_mark_resets_the_same_lanes_elsewhere(case):
  fam, kwargs, na, _ = FAMILIES[case]
  B = 4099
  src = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=4)
  dst = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=4)
  gen = torch.Generator(device='cuda').manual_seed(5)
  for _ in range(5):
    a = torch.randint(0, na, (B,), generator=gen, device='cuda', dtype=torch.int32)
    src.step(a)
  m = torch.rand(B, generator=gen, device='cuda') < 0.25
  src.mark_reset(m)
  dst.load_state_dict(src.state_dict())
  x, y = src.step(a), dst.step(a)
  assert bool((y.step_type[m] == 0).all()) and bool((y.step_type[~m] != 0).any())
  for f in ('step_type', 'reward', 'discount', 'observation'):
    _same(getattr(y, f), getattr(x, f), f'{case} {f}')
  for k, v in src.bsuite_info().items():
    _same(dst.bsuite_info()[k], v, f'{case} bsuite_info {k}')


@pytest.mark.parametrize('case', ['catch', 'cartpole'])
def test_graph_capture_replays_a_masked_step_with_a_static_mask_buffer(case):
  fam, kwargs, na, _ = FAMILIES[case]
  B, reps = 4099, 6
  eager = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=13)
  graphed = eu.make_env(fam, kwargs, batch=B, lane_offset=0, seed=13, device_step_counter=True)
  gen = torch.Generator(device='cuda').manual_seed(6)
  a = torch.randint(0, na, (B,), generator=gen, device='cuda', dtype=torch.int32)
  mask = torch.zeros(B, dtype=torch.bool, device='cuda')
  graphed.step(a, reset_mask=mask)                                # allocate + call 0 outside capture
  eager.step(a, reset_mask=mask)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.stream(side):
    with torch.cuda.graph(g, stream=side):
      out = graphed.step(a, reset_mask=mask)
  torch.cuda.current_stream().wait_stream(side)
  for rep in range(reps):
    a.copy_(torch.randint(0, na, (B,), generator=gen, device='cuda', dtype=torch.int32))
    mask.copy_(torch.rand(B, generator=gen, device='cuda') < (0.0, 1.0 / 64, 0.5, 1.0, 0.25, 0.0)[rep])
    g.replay()
    ref = eager.step(a, reset_mask=mask)
    torch.cuda.synchronize()
    assert bool((out.step_type[mask] == 0).all())
    for f in ('step_type', 'reward', 'discount', 'observation'):
      _same(getattr(out, f), getattr(ref, f), f'{case} rep={rep} {f}')
  assert graphed.device_step_index() == 1 + reps == eager.step_index
  for k, v in eager.bsuite_info().items():
    _same(graphed.bsuite_info()[k], v, f'{case} bsuite_info {k}')


def test_wrappers_forward_both_entry_points():
  from bsuite_amd.environments import catch
  B = 1000
  plain = catch.Catch(batch=B, seed=2)
  noisy = wrappers.RewardScale(wrappers.RewardNoise(catch.Catch(batch=B, seed=2), noise_scale=0.5, seed=7), reward_scale=2.0)
  logged = wrappers.Logging(wrappers.RewardNoise(catch.Catch(batch=B, seed=2), noise_scale=0.5, seed=7), None)
  gen = torch.Generator(device='cuda').manual_seed(7)
  for t in range(30):
    a = torch.randint(0, 3, (B,), generator=gen, device='cuda', dtype=torch.int32)
    m = torch.rand(B, generator=gen, device='cuda') < 0.1
    if t % 2:
      x, y, z = plain.step(a, reset_mask=m), noisy.step(a, reset_mask=m), logged.step(a, reset_mask=m)
    else:
      for e in (plain, noisy, logged):
        e.mark_reset(m)
      x, y, z = plain.step(a), noisy.step(a), logged.step(a)
    for w in (y, z):
      _same(w.step_type, x.step_type, f't={t} step_type')
      _same(w.observation, x.observation, f't={t} observation')
    assert bool((x.step_type[m] == 0).all())
  # Logging: FIRST TimeSteps are not counted as steps; episodes are the LAST TimeSteps
  c = logged.counters()
  assert int(c['episode'].sum().item()) == int(plain.episode_counters()[0].item())
