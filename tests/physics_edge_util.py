"""The edge-state grid of the physics families (cartpole, swing-up, mountain_car) and its reference side, for
tests/test_physics_edges_host.py (CPU) and tests/test_gpu_physics_edges.py (GPU).

Natural trajectories never reach several branches of csrc/cartpole_env.h / csrc/mountain_car_env.h: the second sine /
cosine evaluation behind |dt*theta_dot| > 0.5, the `floor` fallback of the angle wrap, the wrap at 0 and at 2*pi, a
time-out on the step that also crosses a threshold, the wall, the clips.  The grid is a deterministic product of
(state, step count, action) values chosen to sit on both sides of every one of them.  Every state value is exactly
representable in float32, so the float64 reference (oracle/coracle.OracleEnv, its numpy state written in place) and
the device start from the same numbers; the engine side is loaded through the public state_dict() / load_state_dict().
"""
import numpy as np

from oracle import coracle
from tests import engine_util as eu

RESET_BIT = 1 << 30
BLOCK = 256                      # lanes per workgroup (csrc/bsx_device.h)
STEP0 = 5                        # the call index the grids are loaded at: resets inside a T = 3 run draw at 6 and 7
SEED = 23
LANE_OFFSET = (1 << 32) - 300    # the global lane ids cross 2^32 inside the second workgroup
TWO_PI = 2.0 * np.pi

# (family, constructor arguments): the defaults stage the time table in LDS (TAB); the long ones (> 16 KiB) read it from
# device memory
CASES = [('cartpole', {}), ('cartpole_swingup', {}), ('mountain_car', {}),
         ('cartpole', dict(max_time=50.)), ('cartpole_swingup', dict(max_time=50.)), ('mountain_car', dict(max_steps=5000))]
CASE_IDS = [f + ('_' + '_'.join(f'{k}{v}' for k, v in kw.items()) if kw else '') for f, kw in CASES]
# the segments of the grouped test: the sweep ids whose settings (but for the seed) are these.  cartpole/0 and mountain_car/0
# are the default-argument cases; swing-up's sweep has no id with the default thresholds (its first is upright from
# cos(theta) > 0 on), so that segment brings a grid of its own, held to the same conditions by tests/test_physics_edges_host.py
GROUPED_IDS = {'cartpole/0': ('cartpole', {}), 'cartpole_swingup/0': ('cartpole_swingup', dict(height_threshold=0.0, x_reward_threshold=1.0)),
               'mountain_car/0': ('mountain_car', {})}
GROUPED_CASES = [c for c in GROUPED_IDS.values() if c not in CASES]

CARTPOLE_PREDICATES = ('adv_small', 'adv_large', 'wrap_up', 'wrap_down', 'wrap_floor', 'theta_in_at_f32_2pi', 'timeout',
                       'timeout_and_threshold', 'x_in', 'x_out')
SWINGUP_PREDICATES = CARTPOLE_PREDICATES + ('up_true', 'up_false', 'flag6_pos', 'flag6_neg', 'flag7_pos', 'flag7_neg')
MOUNTAIN_CAR_PREDICATES = ('wall', 'vel_clip_lo', 'vel_clip_hi', 'pos_clip_hi', 'goal', 'mc_timeout')
PREDICATES = dict(cartpole=CARTPOLE_PREDICATES, cartpole_swingup=SWINGUP_PREDICATES, mountain_car=MOUNTAIN_CAR_PREDICATES)
MIN_LANES = 64                   # every predicate on at least one full wave
MAX_WAIVED = 0.01                # of the grid: what the tie rules may waive, so that they cannot hide a failure
WALL_TOL = 1e-6                  # the wall rule's window around -1.2 (f64 pre-clip position + velocity)
# rows of the grid that the rng='mt19937' environment is loaded with (2.5 KB of generator state per lane, seeded on the
# host lane by lane): every MT_STRIDE-th row; the stride is coprime to every factor of the products
MT_STRIDE = 17


def mt_rows(g):
  """The rows of the grid that the rng='mt19937' environment runs: all of a small grid, else every MT_STRIDE-th."""
  return np.arange(0, g['lanes'], 1 if g['lanes'] <= 8192 else MT_STRIDE)


def f32_exact(values):
  """float64 array of the float32 roundings of `values`."""
  return np.asarray(values, np.float64).astype(np.float32).astype(np.float64)


def _pm(values):
  return [s * v for v in values for s in (1.0, -1.0)]


def time_sums(timescale, max_time):
  """The reference's f64 running sum `time_elapsed += timescale` (cartpole.py:63): sums[k] after k steps, up to the
  first one above max_time; last_step = len(sums) - 1 (as environments/cartpole._time_table replays it)."""
  sums, t = [0.0], 0.0
  while not t > max_time:
    t = t + timescale
    sums.append(t)
  return np.asarray(sums, np.float64)


def _product(*axes):
  return [m.reshape(-1) for m in np.meshgrid(*axes, indexing='ij')]


def _padded(columns, n_sets, seed):
  """Product rows + seeded random rows from the same sets, up to a lane count of m * BLOCK + 1: the last workgroup and
  its last wave are ragged."""
  n = len(columns[0])
  total = -(-n // BLOCK) * BLOCK + 1
  rng = np.random.default_rng(seed)
  return [np.concatenate([c, rng.choice(s, size=total - n)]) for c, s in zip(columns, n_sets)], n


def cartpole_grid(family, kwargs):
  cfg = eu.cartpole_cfg(family, kwargs)
  sums = time_sums(kwargs.get('timescale', 0.01), kwargs.get('max_time', 10.))
  last_step = len(sums) - 1
  two_pi32 = np.float32(TWO_PI)                                    # 6.2831855f: NOT below the f64 2*pi
  ac = np.arccos(cfg['height_threshold'])
  theta = f32_exact([0.0, 1e-6, np.pi / 2, np.pi - 1e-3, np.pi + 1e-3, 3 * np.pi / 2, np.nextafter(two_pi32, np.float32(0)),
                     two_pi32, -0.05, ac - 1e-4, ac + 1e-4, TWO_PI - ac - 1e-4, TWO_PI - ac + 1e-4])
  theta_dot = f32_exact([0.0] + _pm([1e-3, 0.999, 1.001, 10., 49.9, 50.1, 100., 599., 627., 629., 650., 700.]))
  x = f32_exact([0.0] + _pm([0.999, 1.001, 2.98, 3.02]))
  x_dot = f32_exact([0.0, 3.0, -3.0])
  k = np.asarray([0, 1, last_step - 2, last_step - 1], np.int64)
  action = np.asarray([0, 1, 2], np.int64)
  sets = (theta, theta_dot, x, x_dot, k, action)
  (theta, theta_dot, x, x_dot, k, action), n = _padded(_product(*sets), sets, seed=101)
  assert (np.abs(theta_dot) <= 700.0).all()
  return dict(family=family, kwargs=dict(kwargs), cfg=cfg, n_product=n, lanes=len(k), last_step=last_step, sums=sums,
              timescale=kwargs.get('timescale', 0.01), state=np.stack([x, x_dot, theta, theta_dot], axis=1),
              k=k.astype(np.int32), action=action.astype(np.int32))


def mountain_car_grid(kwargs):
  max_steps = kwargs.get('max_steps', 1000)
  # -1.2 (f64) is not a float32: the device holds f32(-1.2), which lies 4.8e-8 BELOW the reference's wall, and the
  # reference is given the same number; its float32 neighbour towards 0 is the closest state inside the wall
  wall32 = np.float32(-1.2)
  position = f32_exact([wall32, np.nextafter(wall32, np.float32(0)), -1.19, -1.15, -1.13, -np.pi / 6, -0.5, 0.0, 0.43, 0.44,
                        0.4999, 0.5, 0.55, 0.6])
  velocity = f32_exact([0.0] + _pm([1e-4, 0.03, 0.0685, 0.07]))
  t = np.asarray([0, 1, max_steps - 2, max_steps - 1], np.int64)
  action = np.asarray([0, 1, 2], np.int64)
  sets = (position, velocity, t, action)
  (position, velocity, t, action), n = _padded(_product(*sets), sets, seed=202)
  return dict(family='mountain_car', kwargs=dict(kwargs), cfg={}, n_product=n, lanes=len(t), max_steps=max_steps,
              state=np.stack([position, velocity], axis=1), k=t.astype(np.int32), action=action.astype(np.int32))


_GRIDS = {}


def grid(family, kwargs):
  """The (cached, read-only) grid of a case."""
  key = (family, tuple(sorted(kwargs.items())))
  if key not in _GRIDS:
    g = mountain_car_grid(kwargs) if family == 'mountain_car' else cartpole_grid(family, kwargs)
    for v in g.values():
      if isinstance(v, np.ndarray):
        v.setflags(write=False)
    _GRIDS[key] = g
  return _GRIDS[key]


def running_info(g, per_step):
  """f64 [n_columns, B]: the engine's info columns for a running episode of k steps.  per_step: the accounting of
  swing-up and of every family under Logging (the reference's: raw_return and _episode_return grow with every step);
  else the lean one of classic cartpole and mountain_car, which fold an episode into the columns when it ends and add
  the running one on the host (csrc/cartpole_env.h, Cartpole._pending_info): all zero.  The history of a loaded lane is
  ours to choose: classic cartpole earned 1 per step, mountain_car -1, swing-up 0.25 (exact in binary)."""
  fam, k = g['family'], g['k'].astype(np.float64)
  if fam == 'mountain_car':
    return (-k if per_step else np.zeros_like(k))[None]
  info = np.zeros((4, len(k)), np.float64)
  if fam == 'cartpole_swingup':
    info[0] = info[2] = 0.25 * k
  elif per_step:
    info[0] = info[2] = k
  return info


def make_oracle(g, rows=None):
  """The reference at the grid's states (rows: an index array — only those lanes, which keep their global ids)."""
  fam = g['family']
  rows = np.arange(g['lanes']) if rows is None else np.asarray(rows)
  orc = coracle.OracleEnv(fam, g['kwargs'], np.uint64(LANE_OFFSET) + rows.astype(np.uint64), seed=SEED)
  k = g['k'][rows]
  if fam == 'mountain_car':
    orc.s['position'][:] = g['state'][rows, 0]
    orc.s['velocity'][:] = g['state'][rows, 1]
    orc.s['timestep'][:] = k
    orc.info['raw_return'][:] = -k.astype(np.float64)
  else:
    orc.s['state'][:, :4] = g['state'][rows]
    orc.s['state'][:, 4] = g['sums'][k]
    earned = (0.25 if fam == 'cartpole_swingup' else 1.0) * k.astype(np.float64)
    orc.info['raw_return'][:] = earned
    orc._episode_return[:] = earned          # pylint: disable=protected-access
  orc.reset_next[:] = 0
  return orc


def oracle_step(g, rows=None, reset_mask=None):
  """One step of the reference from the grid: (orc, (step_type, reward, discount, obs) copies).  reset_mask: bool [B], the
  lanes that are called with reset() instead of step()."""
  orc = make_oracle(g, rows)
  if reset_mask is not None:
    orc.reset_next[np.asarray(reset_mask)] = 1
  a = g['action'] if rows is None else g['action'][np.asarray(rows)]
  return orc, tuple(v.copy() for v in orc.call(a, STEP0))


def load(env, g, rows=None, step0=STEP0):
  """Loads the grid into an engine environment (possibly wrapped) through state_dict() / load_state_dict().  step0 = None
  keeps the environment's own call index."""
  import torch          # pylint: disable=import-outside-toplevel
  r = eu.raw(env)
  rows = slice(None) if rows is None else np.asarray(rows)
  d = r.state_dict()
  dev, shape = d['state'].device, tuple(d['state'].shape)
  d['state'] = torch.from_numpy(np.ascontiguousarray(g['state'][rows].T.astype(np.float32))).to(dev)
  d['steps'] = torch.from_numpy(np.array(g['k'][rows], np.int32)).to(dev)          # RESET_BIT clear: running episodes
  per_step = g['family'] == 'cartpole_swingup' or '__logging_steps' in d
  d['__info'] = torch.from_numpy(np.ascontiguousarray(running_info(g, per_step)[:, rows])).to(dev)
  if step0 is not None:
    d['__step_index'] = step0
  assert tuple(d['state'].shape) == shape and d['steps'].dtype == torch.int32
  r.load_state_dict(d)


# ------------------------------------------------------------------------------------------------ branch predicates
def predicates(g, orc, want):
  """{name: bool [B]}: which branch each row takes, in float64 from the input state and the reference's output."""
  st, _, _, obs = want
  obs = obs.reshape(len(st), -1)
  k = g['k'].astype(np.int64)
  if g['family'] == 'mountain_car':
    pos, vel = g['state'][:, 0], g['state'][:, 1]
    v1 = vel + (g['action'] - 1.0) * 0.001 + np.cos(3.0 * pos) * -0.0025
    p1 = pos + np.clip(v1, -0.07, 0.07)
    return dict(wall=orc.s['position'] == -1.2, vel_clip_lo=v1 < -0.07, vel_clip_hi=v1 > 0.07, pos_clip_hi=p1 > 0.6,
                goal=orc.s['position'] >= 0.5, mc_timeout=k + 1 >= g['max_steps'], _pre_clip_position=p1)
  cfg, dt = g['cfg'], g['timescale']
  theta, theta_dot = g['state'][:, 2], g['state'][:, 3]
  raw = theta + dt * theta_dot
  x1, th1, thd1 = orc.s['state'][:, 0], orc.s['state'][:, 2], orc.s['state'][:, 3]
  timeout = k + 1 >= g['last_step']
  cos_ok = np.cos(th1) > cfg['height_threshold']
  p = dict(adv_small=np.abs(dt * theta_dot) <= 0.5, adv_large=np.abs(dt * theta_dot) > 0.5,
           wrap_up=(raw < 0.0) & (raw >= -TWO_PI), wrap_down=(raw >= TWO_PI) & (raw < 2 * TWO_PI),
           wrap_floor=(raw >= 2 * TWO_PI) | (raw < -TWO_PI), theta_in_at_f32_2pi=theta >= TWO_PI, timeout=timeout)
  if g['family'] == 'cartpole':
    p.update(x_in=np.abs(x1) < cfg['x_threshold'], x_out=~(np.abs(x1) < cfg['x_threshold']))
    p['timeout_and_threshold'] = timeout & ~(cos_ok & p['x_in'])
  else:
    p.update(x_out=np.abs(x1) > cfg['x_threshold'], x_in=~(np.abs(x1) > cfg['x_threshold']))
    p['timeout_and_threshold'] = timeout & p['x_out']
    up = cos_ok & (np.abs(thd1) < cfg['theta_dot_threshold']) & (np.abs(x1) < cfg['x_reward_threshold'])
    p.update(up_true=up, up_false=~up, flag6_pos=obs[:, 6] == 1.0, flag6_neg=obs[:, 6] == -1.0,
             flag7_pos=obs[:, 7] == 1.0, flag7_neg=obs[:, 7] == -1.0)
  return p


def segment_rows(g, n, seed):
  """int64 [n]: the rows of the grid a grouped segment of n lanes is loaded with (the cartpole grids are larger than a
  segment): a wave of every branch predicate, then seeded random rows."""
  orc, want = oracle_step(g)
  pred = predicates(g, orc, want)
  picked = np.concatenate([np.flatnonzero(pred[name])[:MIN_LANES] for name in PREDICATES[g['family']]])
  assert len(picked) < n
  fill = np.random.default_rng(seed).integers(0, g['lanes'], size=n - len(picked))
  return np.concatenate([picked, fill])


def threshold_ties(g, orc):
  """engine_util.physics_ties on the reference's state after the step."""
  return eu.physics_ties(g['family'], g['cfg'], **eu.oracle_physics_state(orc, g['family']))


def wall_ties(g, rows=None):
  """mountain_car's wall is a discontinuity like the thresholds: position == -1.2 zeroes a negative velocity
  (mountain_car.py:84-85).  A lane whose f64 pre-clip position + velocity lies within WALL_TOL of -1.2 may land on it on
  one side and beside it on the other: it may show the reference's velocity or max(velocity, 0); its position must meet
  the bound all the same.  For these tests only (engine_util.physics_ties is what every other test uses)."""
  if g['family'] != 'mountain_car':
    return np.zeros(g['lanes'] if rows is None else len(rows), bool)
  pos, vel, a = (c if rows is None else c[np.asarray(rows)] for c in (g['state'][:, 0], g['state'][:, 1], g['action']))
  v1 = np.clip(vel + (a - 1.0) * 0.001 + np.cos(3.0 * pos) * -0.0025, -0.07, 0.07)
  return np.abs(pos + v1 - -1.2) <= WALL_TOL


def apply_wall_rule(g, got_obs, want_obs, rows=None):
  """(want', used): `want_obs` with, on wall-tie lanes whose observed velocity is not within the bound of the reference's,
  the reference's velocity replaced by max(velocity, 0); `used` marks those lanes (they count as waived)."""
  tie = wall_ties(g, rows)
  want = np.array(want_obs, np.float32).reshape(len(tie), -1)
  got = np.asarray(got_obs).reshape(len(tie), -1)
  alt = np.maximum(want[:, 1], np.float32(0.0))
  used = tie & ~eu.within_tol(got[:, 1], want[:, 1])[0] & (alt != want[:, 1])
  want[used, 1] = alt[used]
  return want.reshape(np.shape(want_obs)), used


def theta_dot_band(g, rows=None):
  """int [B]: 0 = |theta_dot| <= 50 (and every mountain_car row): the project's contract; 1 = (50, 100], 2 = (100, 600],
  3 = (600, 700]: input states no natural trajectory reaches."""
  n = g['lanes'] if rows is None else len(rows)
  if g['family'] == 'mountain_car':
    return np.zeros(n, np.int64)
  thd = np.abs(g['state'][:, 3] if rows is None else g['state'][np.asarray(rows), 3])
  return np.digitize(thd, [50.0, 100.0, 600.0], right=True)


BAND_NAMES = ('|theta_dot| <= 50', '50 < |theta_dot| <= 100', '100 < |theta_dot| <= 600', '600 < |theta_dot| <= 700')
