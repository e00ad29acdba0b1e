"""Writes tests/golden/.tools/policy_rollout/<case>.npz: B instances of the UNMODIFIED reference, each run in the closed
loop of bsuite/baselines/experiment.py:43-57 by a tabular agent — what `env.rollout_policy(table, T, ...)` must reproduce
lane by lane (tests/test_gpu_policy_rollout.py).  The reference runs on the CPU through oracle.replay's draw replay
(instance i replays lane lane0 + i of the engine's stream).

Per call t and instance: it RESETS when it is fresh or its previous TimeStep was LAST (base.py:59-62, catch.py:80-81) and is
then called with action 0, which the reference ignores.  Otherwise the KEY is derived from the reference's own board —
the hot cells of the observation it returned last: deep_sea `row * N + col` of the one hot cell; catch
`ball_cell * columns + paddle_x`, the ball the hot cell above the bottom row, the paddle the one in it — and the action is
`table[policy_index[instance], key]` of a seeded random uint8 table.  With epsilon > 0 the instance first draws from
oracle/stream.py's `LaneStream(explore_seed, lane, stream_id=2)` at the call's index: U(); if U < epsilon the action is
RandInt(num_actions) instead.  The environment's own draws stay on stream 0.

`check()` asserts what keeps a test on a fixture from passing vacuously: B <= 64, T <= 300, at least 4 LAST steps, every
action of the action_spec taken, for the epsilon cases at least 10 % of the non-reset steps explore and at least 10 %
exploit and some explored action differs from the table's, for the population cases every table is used and two tables
disagree on a key that is looked up, and for the optimal deep_sea table every finished episode reaches the treasure
(total_bad_episodes == 0 and a positive return).

The fixtures live in a dot-directory: tests/test_golden_regen.py requires every other file under tests/golden to be written
by oracle/make_golden.py, and tests/golden_util.py reads every top-level *.npz as an environment fixture.
tests/test_policy_rollout_golden_regen.py regenerates them and compares array for array.  Needs the reference (found the
way oracle/make_golden.py finds it).

  python tools/make_policy_rollout_golden.py            # rewrites the fixtures
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

OUT_DIR = os.path.join(ROOT, 'tests', 'golden', '.tools', 'policy_rollout')

BIG_LANE = (1 << 33) + 5        # counter word 1 of the draw stream
BIG_STEP = (1 << 34) + 77       # the step[47:32] counter bits
STREAM_POLICY = 2               # BSX_STREAM_POLICY (include/bsx_stream.h)


def cases():
  """name -> dict(family, kwargs, B, T, ...).  Appended last = new seed: a case's draws are seeded by its position."""
  c = []

  def add(name, family, kwargs, B, T, **k):
    c.append(dict(name=name, family=family, kwargs=kwargs, B=B, T=T, case_seed=9000 + len(c), **k))
  add('deep_sea_greedy', 'deep_sea', dict(size=8, mapping_seed=42), 16, 60)
  add('deep_sea_stochastic_eps', 'deep_sea', dict(size=6, deterministic=False, mapping_seed=42), 16, 80,
      epsilon=0.25, explore_seed=(1 << 40) + 11, step0=BIG_STEP)
  add('catch_greedy', 'catch', dict(), 32, 100, lane0=BIG_LANE)
  add('catch_6x7_eps', 'catch', dict(rows=6, columns=7), 16, 80, epsilon=0.5, explore_seed=77)
  add('deep_sea_population', 'deep_sea', dict(size=8, mapping_seed=3), 32, 60, P=4)
  add('catch_population', 'catch', dict(), 32, 100, P=4)
  add('deep_sea_optimal', 'deep_sea', dict(size=8, mapping_seed=42), 16, 60, table='optimal')
  return c


def keys_of(family, obs):
  """The policy key of one dense board of the reference (see the module docstring); -1 for deep_sea's all-zero board."""
  rows, columns = obs.shape
  hot = np.flatnonzero(obs.reshape(-1))
  if family == 'deep_sea':
    assert len(hot) <= 1
    return int(hot[0]) if len(hot) else -1
  ball = [h for h in hot if h < (rows - 1) * columns]
  paddle = [h for h in hot if h >= (rows - 1) * columns]
  assert len(ball) == 1 and len(paddle) == 1, 'a board the key is taken from has the ball above the bottom row'
  return int(ball[0]) * columns + (int(paddle[0]) - (rows - 1) * columns)


def index_rows_of(family, raw, obs):
  """The index observation (hot-cell numbers, include/bsuite_amd.h BSX_CALL_OBS_INDEX) of the reference's state."""
  rows, columns = obs.shape
  if family == 'deep_sea':
    hot = np.flatnonzero(obs.reshape(-1))
    return [int(hot[0]) if len(hot) else -1]
  ball = int(raw._ball_y) * columns + int(raw._ball_x)  # pylint: disable=protected-access
  paddle = (rows - 1) * columns + int(raw._paddle_x)  # pylint: disable=protected-access
  assert set(np.flatnonzero(obs.reshape(-1))) == {ball, paddle}
  return [ball, paddle]


def run(bs, family, kwargs, B, T, case_seed, lane0=3, step0=0, seed=42, epsilon=0.0, explore_seed=0, P=1, table='random',
        name=None):
  from oracle import make_golden as mg  # pylint: disable=import-outside-toplevel
  from oracle import replay  # pylint: disable=import-outside-toplevel
  from oracle import stream as S  # pylint: disable=import-outside-toplevel
  lanes = [lane0 + i for i in range(B)]
  envs, rngs = [], []
  for lane in lanes:
    env = mg._make_env(bs, family, kwargs, None)  # pylint: disable=protected-access
    rngs.append(replay.attach_replay(env, seed, lane))
    envs.append(env)
  explore = [S.LaneStream(explore_seed, lane, STREAM_POLICY) for lane in lanes]
  num_actions = int(envs[0].action_spec().num_values)
  board_shape = tuple(envs[0].observation_spec().shape)
  rows, columns = board_shape
  n_states = rows * columns if family == 'deep_sea' else rows * columns * columns
  K = 1 if family == 'deep_sea' else 2
  info_keys = sorted(envs[0].bsuite_info().keys())
  rs = np.random.RandomState(case_seed)
  if table == 'optimal':          # 'right' is the action the cell's mapping names (deep_sea.py:118)
    tab = np.asarray(mg._raw(envs[0])._action_mapping).reshape(1, -1).astype(np.uint8)  # pylint: disable=protected-access
  else:
    tab = rs.randint(num_actions, size=(P, n_states)).astype(np.uint8)
  assert tab.shape == (P, n_states)
  policy_index = rs.randint(P, size=B).astype(np.int32) if P > 1 else np.zeros(B, np.int32)

  actions = np.zeros((T, B), np.int32)
  keys = np.full((T, B), -1, np.int32)
  resets = np.zeros((T, B), np.uint8)
  explored = np.zeros((T, B), np.uint8)
  step_type = np.zeros((T, B), np.int8)
  reward = np.full((T, B), np.nan, np.float64)
  discount = np.full((T, B), np.nan, np.float64)
  obs = np.zeros((T, B) + board_shape, np.float32)
  index = np.zeros((T, B, K), np.int32)
  info = np.zeros((T, B, len(info_keys)), np.float64)
  for t in range(T):
    for l, env in enumerate(envs):
      fresh = t == 0 or step_type[t - 1, l] == 2
      a = 0
      if fresh:
        resets[t, l] = 1
      else:
        keys[t, l] = keys_of(family, obs[t - 1, l])
        a = int(tab[policy_index[l], keys[t, l]])
        if epsilon > 0:
          explore[l].begin_step(step0 + t)
          if explore[l].uniform01() < epsilon:
            a = int(explore[l].randint(num_actions))
            explored[t, l] = 1
      actions[t, l] = a
      for r in rngs[l]:
        r.begin_step(step0 + t)
      ts = env.step(a)
      step_type[t, l] = int(ts.step_type)
      assert (int(ts.step_type) == 0) == fresh
      if ts.reward is not None:
        reward[t, l] = float(ts.reward)
        discount[t, l] = float(ts.discount)
      o = np.asarray(ts.observation)
      assert o.dtype == np.float32 and o.shape == board_shape, (o.dtype, o.shape)
      obs[t, l] = o
      index[t, l] = index_rows_of(family, mg._raw(env), o)  # pylint: disable=protected-access
      bi = env.bsuite_info()
      info[t, l] = [float(bi[k]) for k in info_keys]

  meta = dict(name=name, family=family, kwargs=kwargs, seed=seed, step0=step0, epsilon=epsilon, explore_seed=explore_seed,
              n_policies=P, n_states=n_states, table=table, info_keys=info_keys, num_actions=num_actions,
              board_shape=list(board_shape))
  out = dict(lanes=np.array(lanes, np.uint64), table=tab, policy_index=policy_index, actions=actions, keys=keys,
             resets=resets, explored=explored, step_type=step_type, reward=reward, discount=discount, obs=obs, index=index,
             info=info)
  check(meta, out)
  out['meta'] = np.array(json.dumps(meta, sort_keys=True))
  return out


def check(meta, g):
  """What keeps a test on this fixture from passing vacuously (see the module docstring)."""
  name = meta['name']
  T, B = g['actions'].shape
  assert B <= 64 and T <= 300, f'{name}: B = {B}, T = {T}'
  live = g['resets'] == 0
  n_last = int((g['step_type'] == 2).sum())
  assert n_last >= 4, f'{name}: {n_last} LAST steps'
  assert (g['step_type'][~live] == 0).all() and (g['step_type'][live] != 0).all(), f'{name}: resets are the FIRST steps'
  assert (g['actions'][~live] == 0).all() and (g['keys'][~live] == -1).all(), f'{name}: a reset step takes action 0'
  assert (g['keys'][live] >= 0).all() and (g['keys'][live] < meta['n_states']).all(), f'{name}: a key outside the table'
  taken = set(np.unique(g['actions'][live]).tolist())
  assert taken == set(range(meta['num_actions'])), f'{name}: actions taken {sorted(taken)}'
  rows_of = np.broadcast_to(g['policy_index'][None, :], (T, B))
  from_table = g['table'][rows_of[live], g['keys'][live]].astype(np.int32)
  ex = g['explored'][live] != 0
  assert (g['actions'][live][~ex] == from_table[~ex]).all(), f'{name}: an exploiting step that is not the table entry'
  stats = dict(last=n_last, live=int(live.sum()), explored=int(ex.sum()))
  if meta['epsilon'] > 0:
    n = int(live.sum())
    assert 10 * int(ex.sum()) >= n and 10 * int((~ex).sum()) >= n, f'{name}: {int(ex.sum())} of {n} steps explore'
    assert (g['actions'][live][ex] != from_table[ex]).any(), f'{name}: no explored action differs from the table'
  else:
    assert not ex.any(), f'{name}: exploration without epsilon'
  if meta['n_policies'] > 1:
    P = meta['n_policies']
    assert set(np.unique(g['policy_index']).tolist()) == set(range(P)), f'{name}: not every table is used'
    k = g['keys'][live]
    assert (g['table'][:, k].min(axis=0) != g['table'][:, k].max(axis=0)).any(), f'{name}: the tables agree on every key used'
  else:
    assert (g['policy_index'] == 0).all()
  if meta['table'] == 'optimal':
    bad = g['info'][-1, :, meta['info_keys'].index('total_bad_episodes')]
    assert (bad == 0).all(), f'{name}: total_bad_episodes {bad}'
    last = g['step_type'] == 2
    assert (g['reward'][last] > 0.9).all(), f'{name}: a finished episode that did not reach the treasure'
  return stats


def make():
  """{case name: {array name: array}} of every case."""
  from oracle import replay  # pylint: disable=import-outside-toplevel
  bs = replay.import_reference()
  out = {}
  for c in cases():
    c = dict(c)
    out[c['name']] = run(bs, c.pop('family'), c.pop('kwargs'), c.pop('B'), c.pop('T'), c.pop('case_seed'), **c)
  return out


if __name__ == '__main__':
  os.makedirs(OUT_DIR, exist_ok=True)
  for case_name, arrays in make().items():
    path = os.path.join(OUT_DIR, case_name + '.npz')
    np.savez_compressed(path, **arrays)
    m = json.loads(str(arrays['meta']))
    s = check(m, arrays)
    print(f'{case_name:26s} T={arrays["actions"].shape[0]:4d} B={arrays["actions"].shape[1]:3d} last={s["last"]:4d} '
          f'live={s["live"]:5d} explored={s["explored"]:4d} {os.path.getsize(path) / 1024:7.1f} KiB')
