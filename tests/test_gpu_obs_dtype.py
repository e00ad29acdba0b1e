"""GPU: narrow observation dtypes (uint8 / float16 / bfloat16) of deep_sea and catch.  Every narrow board, widened to
float32, is bit-equal to the float32 engine's board and to the C oracle's; the scalar TimeStep fields and bsuite_info
are unchanged — at one lane, thousands of lanes, 2^20 lanes and ragged sizes whose byte length is not a multiple of
16, through rollouts, wrappers, MT19937-exact draws, state_dict round trips and HIP-graph replays."""
import numpy as np
import pytest
import torch

from bsuite_amd.utils import wrappers
from oracle import coracle
from tests import engine_util as eu
from tests.test_gpu_oracle_batch import CASES

pytestmark = pytest.mark.gpu

NARROW = (torch.uint8, torch.float16, torch.bfloat16)
BOARD_CASES = [c for c in CASES if c[0] in ('deep_sea', 'catch')]


def _episode_len(family, kwargs):
  return kwargs.get('size', 10) if family == 'deep_sea' else kwargs.get('rows', 10) - 1


def _assert_same(ts, ref, dtype, what):
  assert ts.observation.dtype is dtype and ts.observation.shape == ref.observation.shape, what
  assert torch.equal(ts.observation.float(), ref.observation), what
  assert torch.equal(ts.step_type, ref.step_type), what
  assert torch.equal(ts.reward, ref.reward), what
  assert torch.equal(ts.discount, ref.discount), what


def _assert_same_info(env, ref):
  for k, v in ref.bsuite_info().items():
    assert torch.equal(env.bsuite_info()[k], v), k
  assert torch.equal(eu.raw(env).episode_counters(), eu.raw(ref).episode_counters())


@pytest.mark.parametrize('family,kwargs,wrap', BOARD_CASES)
@pytest.mark.parametrize('batch,lane_offset', [(1, 0), (1000, 0), (4099, (1 << 32) - 17)])
def test_narrow_equals_float32_engine(family, kwargs, wrap, batch, lane_offset):
  if family == 'catch' and kwargs.get('rows') == 64 and batch > 1000:
    pytest.skip('big board at big batch adds nothing')
  seed = 1234
  mk = lambda dt: eu.make_env(family, kwargs, batch=batch, lane_offset=lane_offset, seed=seed, wrap=wrap,
                              observation_dtype=dt)
  ref, envs = mk(torch.float32), {dt: mk(dt) for dt in NARROW}
  L = _episode_len(family, kwargs)
  T = 2 * L + 20                          # explicit resets mid-episode, then at least two whole episodes
  resets = (5, 6) if L > 6 else (2, 3)
  rng = np.random.default_rng(batch)
  for t in range(T):
    a = torch.from_numpy(rng.integers(0, 3 if family == 'catch' else 2, size=batch).astype(np.int32)).cuda()
    want = ref.reset() if t in resets else ref.step(a)
    for dt, env in envs.items():
      got = env.reset() if t in resets else env.step(a)
      _assert_same(got, want, dt, (dt, t))
  for env in envs.values():
    _assert_same_info(env, ref)


@pytest.mark.parametrize('family,kwargs', [('deep_sea', dict(size=30, mapping_seed=42)), ('catch', dict(rows=10, columns=5))])
@pytest.mark.parametrize('dtype', NARROW)
def test_narrow_boards_equal_the_oracle(family, kwargs, dtype):
  B, seed = 1000, 77
  env = eu.make_env(family, kwargs, batch=B, lane_offset=0, seed=seed, observation_dtype=dtype)
  orc = coracle.OracleEnv(family, kwargs, np.arange(B, dtype=np.uint64), seed=seed)
  rng = np.random.default_rng(3)
  for t in range(70):
    a = rng.integers(0, orc.num_actions, size=B).astype(np.int32)
    force = t == 9
    ts = env.reset() if force else env.step(torch.from_numpy(a).cuda())
    st, r, _, o = orc.call(a, t, force_reset=force)
    assert ts.observation.dtype is dtype
    np.testing.assert_array_equal(ts.observation.float().cpu().numpy(), o, err_msg=f't={t}')
    np.testing.assert_array_equal(ts.step_type.cpu().numpy(), st)
    live = st != 0
    np.testing.assert_array_equal(ts.reward.cpu().numpy()[live], r[live].astype(np.float32))
  for k, v in orc.bsuite_info().items():
    np.testing.assert_array_equal(env.bsuite_info()[k].cpu().numpy(), v, err_msg=k)


def _acts(T, B, n, seed):
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  return torch.randint(n, (T, B), generator=g, device='cuda', dtype=torch.int32)


# deep_sea/10 (30 x 30) and catch/0 (10 x 5) at 2^20 lanes, and ragged lane counts: (2^20 + 257) * cells * E is not a
# multiple of 16 for any E
@pytest.mark.parametrize('family,kwargs,batch', [
    ('deep_sea', dict(size=30, mapping_seed=42), 1 << 20), ('deep_sea', dict(size=30, mapping_seed=42), (1 << 20) + 257),
    ('catch', dict(), 1 << 20), ('catch', dict(), (1 << 20) + 257), ('catch', dict(), (1 << 21) + 257)])
def test_full_size_and_ragged(family, kwargs, batch):
  seed = 5
  mk = lambda dt: eu.make_env(family, kwargs, batch=batch, lane_offset=0, seed=seed, observation_dtype=dt)
  ref, envs = mk(torch.float32), {dt: mk(dt) for dt in NARROW}
  L = _episode_len(family, kwargs)
  acts = _acts(L + 3, batch, 3 if family == 'catch' else 2, 1)
  for t in range(L + 3):
    want = ref.step(acts[t])
    for dt, env in envs.items():
      _assert_same(env.step(acts[t]), want, dt, (dt, t))
  for env in envs.values():
    _assert_same_info(env, ref)


@pytest.mark.parametrize('family,kwargs', [('deep_sea', dict(size=30, mapping_seed=42)), ('deep_sea', dict(size=3, mapping_seed=1)),
                                           ('catch', dict()), ('catch', dict(rows=2, columns=1)),
                                           ('catch', dict(rows=7, columns=3))])
@pytest.mark.parametrize('batch', [1003, 4099, 65537])
@pytest.mark.parametrize('dtype', NARROW)
def test_rollout_equals_steps(family, kwargs, batch, dtype):
  """rollout(T) == T step() calls; at these lane counts slice t starts at a byte offset that is not 16-byte aligned."""
  seed = 21
  mk = lambda: eu.make_env(family, kwargs, batch=batch, lane_offset=11, seed=seed, observation_dtype=dtype)
  roll, step = mk(), mk()
  n = 3 if family == 'catch' else 2
  for T, k in ((1, 0), (7, 1), (32, 2)):
    acts = _acts(T, batch, n, k)
    got = roll.rollout(acts)
    assert got.observation.dtype is dtype and got.observation.shape == (T, batch) + tuple(roll.observation_spec().shape)
    for t in range(T):
      want = step.step(acts[t])
      assert torch.equal(got.observation[t], want.observation), (T, t)
      assert torch.equal(got.step_type[t], want.step_type) and torch.equal(got.reward[t], want.reward), (T, t)
      assert torch.equal(got.discount[t], want.discount), (T, t)
  _assert_same_info(roll, step)


@pytest.mark.parametrize('dtype', NARROW)
def test_logging_and_reward_noise_on_a_narrow_env(dtype):
  B, seed = 2051, 9
  mk = lambda dt: wrappers.Logging(eu.make_env('catch', {}, batch=B, lane_offset=3, seed=seed, wrap=('noise', 0.3),
                                               observation_dtype=dt), None)
  ref, log = mk(torch.float32), mk(dtype)
  assert log.observation_dtype is dtype
  acts = _acts(150, B, 3, 4)
  for t in range(150):
    _assert_same(log.step(acts[t]), ref.step(acts[t]), dtype, t)
  for k, v in ref.counters().items():
    assert torch.equal(log.counters()[k], v), k
  assert torch.equal(log.num_rows(), ref.num_rows())
  assert torch.equal(log._lg['rows'], ref._lg['rows'])           # pylint: disable=protected-access
  assert log.all_rows() == ref.all_rows()                         # what the CSV logger writes


@pytest.mark.parametrize('family,kwargs', [('deep_sea', dict(size=8, deterministic=False, mapping_seed=3)), ('catch', dict())])
@pytest.mark.parametrize('dtype', NARROW)
def test_mt19937_draws(family, kwargs, dtype):
  B = 64
  mk = lambda dt: eu.make_env(family, kwargs, batch=B, lane_offset=0, seed=17, rng='mt19937', observation_dtype=dt)
  ref, env = mk(torch.float32), mk(dtype)
  acts = _acts(40, B, 2, 6)
  for t in range(40):
    _assert_same(env.step(acts[t]), ref.step(acts[t]), dtype, t)
  _assert_same_info(env, ref)


@pytest.mark.parametrize('family,kwargs', [('deep_sea', dict(size=30, mapping_seed=42)), ('catch', dict())])
@pytest.mark.parametrize('dtype', NARROW)
def test_graph_capture_replays_equal_eager_float32(family, kwargs, dtype):
  B, T, reps, seed = 4099, 4, 6, 13
  acts = _acts(T, B, 2, 8)
  eager = eu.make_env(family, kwargs, batch=B, lane_offset=0, seed=seed)
  graphed = eu.make_env(family, kwargs, batch=B, lane_offset=0, seed=seed, observation_dtype=dtype,
                        device_step_counter=True)
  graphed.step(acts[0])                                    # allocate + call 0 outside capture
  eager.step(acts[0])
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.stream(side):
    with torch.cuda.graph(g, stream=side):
      outs = [graphed.step(acts[t]) for t in range(T)]
  torch.cuda.current_stream().wait_stream(side)
  for _ in range(reps):
    g.replay()
    refs = [eager.step(acts[t]) for t in range(T)]
    torch.cuda.synchronize()
    _assert_same(outs[-1], refs[-1], dtype, 'replay')
  assert graphed.device_step_index() == 1 + T * reps == eager.step_index
  _assert_same_info(graphed, eager)


@pytest.mark.parametrize('dtype', NARROW)
def test_state_dict_round_trip(dtype):
  B = 1000
  mk = lambda: eu.make_env('deep_sea', dict(size=12, mapping_seed=2), batch=B, lane_offset=0, seed=3, observation_dtype=dtype)
  a, b = mk(), mk()
  acts = _acts(40, B, 2, 9)
  for t in range(17):
    a.step(acts[t])
  b.load_state_dict(a.state_dict())
  for t in range(17, 40):
    x, y = a.step(acts[t]), b.step(acts[t])
    assert torch.equal(x.observation, y.observation) and torch.equal(x.reward, y.reward), t


@pytest.mark.parametrize('num_buffers', [1, 2, 3])
@pytest.mark.parametrize('dtype', NARROW)
def test_buffers_have_the_requested_dtype(dtype, num_buffers):
  B = 257
  for family, kwargs, shape in (('deep_sea', dict(size=9, mapping_seed=0), (9, 9)), ('catch', dict(rows=6, columns=4), (6, 4))):
    env = eu.make_env(family, kwargs, batch=B, lane_offset=0, seed=1, num_buffers=num_buffers, observation_dtype=dtype)
    seen = []
    for t in range(2 * num_buffers):
      ts = env.reset() if t == 0 else env.step(torch.zeros(B, dtype=torch.int32, device='cuda'))
      o = ts.observation
      assert o.dtype is dtype and o.shape == (B,) + shape and o.is_contiguous() and o.is_cuda
      assert set(torch.unique(o.float()).tolist()) <= {0.0, 1.0}
      seen.append(o.data_ptr())
    assert len(set(seen)) == num_buffers
