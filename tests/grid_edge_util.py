"""The edge-state grid of the grid families (catch, deep_sea) and its reference side, for tests/test_grid_edges_host.py
(CPU) and tests/test_gpu_grid_edges.py (GPU).

The lane advance of the two families (csrc/catch_fam.h, csrc/deep_sea_fam.h) is compiled into some twenty kernels, four
of them in the deferred form (advance_deferred + commit_deferred).  Trajectories from a fresh reset never reach several of
its branches through most of them: catch's fold of 127 pending misses into the total_regret column (bits 25..31 of the
state word, the sign bit among them), deep_sea's paying bottom-right cell and its bad-episode bit at a chosen diagonal
cell.  The grid is a deterministic product of state fields and actions on both sides of every one of them, padded with
seeded random rows of the same product to m * 256 + 1 lanes (or + 2, + 4: the `aligned` cases below).  The reference side is oracle/coracle.OracleEnv with its numpy
state written in place; the engine side is loaded through the public state_dict() / load_state_dict().

The products are the plain ones: every field value within the range the advance writes (pending <= 126, col <= row, reset
words shaped as a LAST step leaves them), not only the combinations a trajectory from reset() visits.
"""
import numpy as np

from oracle import coracle

BLOCK = 256                      # lanes per workgroup (csrc/bsx_device.h)
STEP0 = 5                        # the call index the grids are loaded at: resets inside a T = 3 run draw at 6 and 7
SEED = 23
LANE_OFFSET = (1 << 32) - 300    # the global lane ids cross 2^32 inside the second workgroup
MIN_LANES = 64                   # every predicate on at least one full wave
MIN_BLOCKS = 8                   # small products are padded to at least this many workgroups (+ 1 lane)
MT_STRIDE = 17                   # the rows the rng='mt19937' environment is loaded with: every 17th

CATCH_RESET_BIT, CATCH_PENDING_SHIFT, CATCH_PENDING_MAX = 1 << 24, 25, 127
DS_RESET_BIT = 1 << 17
PENDING = (0, 1, 63, 64, 125, 126)           # from 64 up bit 31 of the word is set; at 126 a miss folds
COLUMN = (0.0, 254.0 * 3)                    # the total_regret column itself
DS_HISTORY = (3.0, 5.0)                      # total_bad_episodes, denoised_return of every loaded deep_sea lane
CORNER_REPEATS = 40                          # deep_sea: the two last-row corner cells, this many times more
RESET_REPEATS = 8                            # deep_sea: each reset word (column, bad bit, action), this many times

# (family, constructor arguments, aligned).  catch 10x5: fused tiles; 13x10: 130 cells, over the 128-cell fuse limit (advance
# + stream pair, pipelined rollout); 2x5: an episode every two calls; 64x64: the three position fields at the top of their
# range.  deep_sea 4; 6 stochastic; 12: 144 cells, the pair path; 30: the single-launch step; 7 with the identity mapping.
# The fused tile step, the fused rollout and the pipelined rollout need lanes * cells to be a multiple of 4 (16-byte store
# stream: csrc/bsx_pair_host.h); otherwise a call is lane advance + store stream per step, with 4-byte stores on the slices of
# a rollout that start off a 16-byte boundary.  With m * 256 + 1 lanes the boards of 50, 130, 10 and 49 cells are on the
# 4-byte side, so each of them is a second case, `aligned`: m * 256 + 2 (+ 4 for 49 cells) lanes, still a ragged last wave.
CASES = [('catch', dict(rows=10, columns=5), False), ('catch', dict(rows=10, columns=5), True),
         ('catch', dict(rows=13, columns=10), False), ('catch', dict(rows=13, columns=10), True),
         ('catch', dict(rows=2, columns=5), False), ('catch', dict(rows=2, columns=5), True),
         ('catch', dict(rows=64, columns=64), False),
         ('deep_sea', dict(size=4, mapping_seed=42), False), ('deep_sea', dict(size=6, deterministic=False, mapping_seed=1), False),
         ('deep_sea', dict(size=12, mapping_seed=3), False), ('deep_sea', dict(size=30, mapping_seed=42), False),
         ('deep_sea', dict(size=7, randomize_actions=False, unscaled_move_cost=0.05), False),
         ('deep_sea', dict(size=7, randomize_actions=False, unscaled_move_cost=0.05), True)]
# the segments of the grouped test (a SweepBatch of catch/0 and deep_sea/0): the settings of those two ids
GROUPED_CASES = [('catch', dict(rows=10, columns=5), False), ('deep_sea', dict(size=10, mapping_seed=42), False)]


def case_id(family, kwargs, aligned=False):
  tail = '_aligned' if aligned else ''
  if family == 'catch':
    return f'catch_{kwargs["rows"]}x{kwargs["columns"]}' + tail
  return f'deep_sea_{kwargs["size"]}' + ('_stochastic' if not kwargs.get('deterministic', True) else '') + (
      '_identity' if not kwargs.get('randomize_actions', True) else '') + tail


CASE_IDS = [case_id(*c) for c in CASES]


def cells_of(family, kwargs):
  return kwargs['rows'] * kwargs['columns'] if family == 'catch' else kwargs['size'] ** 2


CATCH_PREDICATES = ('lands_catch', 'lands_miss', 'fold', 'sign_bit_in', 'sign_bit_out', 'clamp_left', 'clamp_right', 'resets')
DEEP_SEA_PREDICATES = ('corner_right_pays', 'corner_left_last_row', 'sets_bad', 'ends_bad', 'ends_good', 'clamp_left', 'resets')


def predicate_names(family, kwargs):
  if family == 'catch':
    return CATCH_PREDICATES
  return DEEP_SEA_PREDICATES + (() if kwargs.get('deterministic', True) else ('noise_drawn',))


def _product(*axes):
  return [m.reshape(-1) for m in np.meshgrid(*axes, indexing='ij')]


def _padded(columns, seed, cells, aligned):
  """The rows + seeded random rows drawn from the product, up to a lane count of m * BLOCK + e with m >= MIN_BLOCKS: the last
  workgroup and its last wave are ragged.  e = 1, or — `aligned` — the smallest e >= 1 with lanes * cells a multiple of 4."""
  n = len(columns[0])
  total = max(-(-n // BLOCK), MIN_BLOCKS) * BLOCK + 1
  while aligned and (total * cells) % 4:
    total += 1
  pick = np.random.default_rng(seed).integers(0, n, size=total - n)
  return [np.concatenate([c, c[pick]]) for c in columns], n


def _edge_values(n):
  return np.arange(n) if n <= 5 else np.asarray(sorted({0, 1, n // 2, n - 2, n - 1}))


def catch_grid(kwargs, aligned=False):
  rows, cols = kwargs['rows'], kwargs['columns']
  xs = _edge_values(cols)
  ys = np.asarray(sorted({max(0, y) for y in (0, rows - 3, rows - 2)}))       # at rows - 2 the ball lands on this call
  pend, column, action = np.asarray(PENDING), np.asarray(COLUMN), np.asarray([0, 1, 2])
  bx, px, by, pe, co, ac = _product(xs, xs, ys, pend, column, action)
  reset = np.zeros(len(bx), np.int64)
  # reset rows: the word a LAST step leaves (ball in the paddle's row, reset bit set), with each pending value
  rbx, rpx, rpe, rco = _product(xs, xs, pend, column)
  cols_ = [np.concatenate(p) for p in ((bx, rbx), (px, rpx), (by, np.full(len(rbx), rows - 1)), (pe, rpe), (co, rco),
                                       (ac, np.arange(len(rbx)) % 3), (reset, np.ones(len(rbx), np.int64)))]
  (bx, px, by, pe, co, ac, reset), n = _padded(cols_, 303, rows * cols, aligned)
  word = (bx | (by << 8) | (px << 16) | (reset * CATCH_RESET_BIT) | (pe << CATCH_PENDING_SHIFT)).astype(np.uint32).view(np.int32)
  return dict(family='catch', kwargs=dict(kwargs), n_product=n, lanes=len(bx), rows=rows, columns=cols, ball_x=bx, paddle_x=px,
              ball_y=by, pending=pe, column=co.astype(np.float64), reset=reset.astype(bool), action=ac.astype(np.int32), state=word,
              info=co.astype(np.float64)[None].copy())


def deep_sea_grid(kwargs, aligned=False):
  N = kwargs['size']
  cells = np.asarray([(r, c) for r in range(N) for c in range(r + 1)])        # the triangle col <= row < N
  cell, bad, ac = _product(np.arange(len(cells)), np.asarray([0, 1]), np.asarray([0, 1]))
  row, col = cells[cell, 0], cells[cell, 1]
  # the two last-row corners are 2 of N (N + 1) / 2 cells: repeated, so that a full wave of lanes stands on each
  crow, ccol, cbad, cac, _ = _product(np.asarray([N - 1]), np.asarray([0, N - 1]), np.asarray([0, 1]), np.asarray([0, 1]),
                                      np.arange(CORNER_REPEATS))
  # reset rows: the word a LAST step leaves (row = N), with the bad bit both ways
  rcol, rbad, rac, _ = _product(np.arange(N), np.asarray([0, 1]), np.asarray([0, 1]), np.arange(RESET_REPEATS))
  reset = np.concatenate([np.zeros(len(row) + len(crow), np.int64), np.ones(len(rcol), np.int64)])
  cols_ = [np.concatenate(p) for p in ((row, crow, np.full(len(rcol), N)), (col, ccol, rcol), (bad, cbad, rbad), (ac, cac, rac))]
  (row, col, bad, ac, reset), n = _padded(cols_ + [reset], 404, N * N, aligned)
  word = (row | (col << 8) | (bad << 16) | (reset * DS_RESET_BIT)).astype(np.int32)
  info = np.repeat(np.asarray(DS_HISTORY, np.float64)[:, None], len(row), axis=1)
  mapping = coracle.deep_sea_mapping(N, kwargs.get('mapping_seed'), kwargs.get('randomize_actions', True))
  return dict(family='deep_sea', kwargs=dict(kwargs), n_product=n, lanes=len(row), size=N, row=row, col=col, bad=bad,
              reset=reset.astype(bool), action=ac.astype(np.int32), state=word, info=info, mapping=mapping,
              move_cost=float(kwargs.get('unscaled_move_cost', 0.01)) / N, deterministic=bool(kwargs.get('deterministic', True)))


_GRIDS = {}


def grid(family, kwargs, aligned=False):
  """The (cached, read-only) grid of a case."""
  key = (family, tuple(sorted(kwargs.items())), aligned)
  if key not in _GRIDS:
    g = catch_grid(kwargs, aligned) if family == 'catch' else deep_sea_grid(kwargs, aligned)
    g['aligned'], g['cells'] = aligned, cells_of(family, kwargs)
    for v in g.values():
      if isinstance(v, np.ndarray):
        v.setflags(write=False)
    _GRIDS[key] = g
  return _GRIDS[key]


def mt_rows(g):
  return np.arange(0, g['lanes'], MT_STRIDE)


def draw_rows(g):
  """bool [B]: the rows whose first step consumes a draw that shows in the result — catch's reset draws the ball's column; a
  stochastic deep_sea draws on every step right and on the two last-row corners.  Runs on another lane id or another generator
  (tiled batches, rng='mt19937') are comparable with the grid's own on the other rows only."""
  if g['family'] == 'catch':
    return g['reset'].copy()
  if g['deterministic']:
    return np.zeros(g['lanes'], bool)
  N, running = g['size'], ~g['reset']
  row = np.minimum(g['row'], N - 1)
  right = g['action'] == g['mapping'][row, g['col']]
  return running & (right | ((g['row'] == N - 1) & ((g['col'] == 0) | (g['col'] == N - 1))))


def catch_words(ball_x, ball_y, paddle_x, pending, reset=0):
  """The packed catch state word (csrc/catch_fam.h) as int32."""
  w = np.asarray(ball_x, np.int64) | (np.asarray(ball_y, np.int64) << 8) | (np.asarray(paddle_x, np.int64) << 16)
  w = w | (np.asarray(reset, np.int64) * CATCH_RESET_BIT) | (np.asarray(pending, np.int64) << CATCH_PENDING_SHIFT)
  return w.astype(np.uint32).view(np.int32)


def pending_of(words):
  """The pending-miss field of catch state words (int32 array, or a torch tensor's numpy view)."""
  return (np.asarray(words).view(np.uint32) >> CATCH_PENDING_SHIFT).astype(np.int64)


def make_oracle(g, rows=None, lane_ids=None):
  """The reference at the grid's states (rows: an index array — those rows of the grid on lanes LANE_OFFSET + rows, or on
  `lane_ids` if given)."""
  rows = np.arange(g['lanes']) if rows is None else np.asarray(rows)
  ids = np.uint64(LANE_OFFSET) + rows.astype(np.uint64) if lane_ids is None else np.asarray(lane_ids, np.uint64)
  orc = coracle.OracleEnv(g['family'], g['kwargs'], ids, seed=SEED)
  if g['family'] == 'catch':
    for k in ('ball_x', 'ball_y', 'paddle_x'):
      orc.s[k][:] = g[k][rows]
    orc.info['total_regret'][:] = g['column'][rows] + 2.0 * g['pending'][rows]
  else:
    for k in ('row', 'col', 'bad'):
      orc.s[k][:] = g[k][rows]
    orc.info['total_bad_episodes'][:] = g['info'][0, rows]
    orc.info['denoised_return'][:] = g['info'][1, rows]
  orc.reset_next[:] = g['reset'][rows]
  return orc


def oracle_step(g, rows=None, lane_ids=None):
  """One step of the reference from the grid: (orc, (step_type, reward, discount, obs) copies)."""
  orc = make_oracle(g, rows, lane_ids)
  a = g['action'] if rows is None else g['action'][np.asarray(rows)]
  return orc, tuple(v.copy() for v in orc.call(a, STEP0))


def oracle_run(g, actions, rows=None, step0=STEP0):
  """The reference from the grid through actions [T, B]: (orc, step_type [T, B], float64 reward [T, B])."""
  orc = make_oracle(g, rows)
  st, r = [], []
  for t, a in enumerate(np.asarray(actions)):
    s, rew, _, _ = orc.call(a, step0 + t)
    st.append(s.copy())
    r.append(rew.copy())
  return orc, np.stack(st), np.stack(r)


def load(env, g, rows=None, step0=STEP0, fold_pending=False):
  """Loads the grid into an engine environment (possibly wrapped) through state_dict() / load_state_dict().  step0 = None
  keeps the environment's own call index.  fold_pending (catch): pending loaded as 0, its misses moved into the column —
  the form an environment under Logging holds."""
  import torch          # pylint: disable=import-outside-toplevel
  from tests import engine_util as eu          # pylint: disable=import-outside-toplevel
  r = eu.raw(env)
  rows = np.arange(g['lanes']) if rows is None else np.asarray(rows)
  d = r.state_dict()
  dev, shape, ishape = d['state'].device, tuple(d['state'].shape), tuple(d['__info'].shape)
  state, info = g['state'][rows], g['info'][:, rows]
  if fold_pending:
    assert g['family'] == 'catch'
    info = info + 2.0 * g['pending'][rows]
    state = catch_words(g['ball_x'][rows], g['ball_y'][rows], g['paddle_x'][rows], 0, g['reset'][rows])
  d['state'] = torch.from_numpy(np.ascontiguousarray(state)).to(dev)
  d['__info'] = torch.from_numpy(np.ascontiguousarray(info)).to(dev)
  if step0 is not None:
    d['__step_index'] = step0
  assert tuple(d['state'].shape) == shape and d['state'].dtype == torch.int32 and tuple(d['__info'].shape) == ishape
  r.load_state_dict(d)


def catch_expected(g, want):
  """(column, pending) int64-exact float64 / int64 [B] after the step, from the grid and the reference's TimeStep: a miss at
  pending 126 adds 254 to the column and clears pending, any other miss adds 1 to pending, everything else keeps both."""
  st, reward = want[0], want[1]
  miss = (st == 2) & (reward == -1.0)
  fold = miss & (g['pending'] == CATCH_PENDING_MAX - 1)
  return g['column'] + 254.0 * fold, np.where(fold, 0, g['pending'] + (miss & ~fold))


# ------------------------------------------------------------------------------------------------ branch predicates
def predicates(g, orc, want):
  """{name: bool [B]}: which branch each row takes, from the input state and the reference's output."""
  st, reward = want[0], want[1]
  running = ~g['reset']
  if g['family'] == 'catch':
    lands = running & (g['ball_y'] + 1 == g['rows'] - 1)
    assert ((st == 2) == lands).all() and ((st == 0) == g['reset']).all()
    _, pending_out = catch_expected(g, want)
    return dict(lands_catch=lands & (reward == 1.0), lands_miss=lands & (reward == -1.0),
                fold=lands & (reward == -1.0) & (g['pending'] == CATCH_PENDING_MAX - 1),
                sign_bit_in=g['pending'] >= 64, sign_bit_out=pending_out >= 64,
                clamp_left=running & (g['paddle_x'] == 0) & (g['action'] == 0),
                clamp_right=running & (g['paddle_x'] == g['columns'] - 1) & (g['action'] == 2), resets=g['reset'].copy())
  N = g['size']
  row, col = np.minimum(g['row'], N - 1), g['col']
  right = running & (g['action'] == g['mapping'][row, col])
  left = running & ~right
  last = running & (g['row'] == N - 1)
  assert ((st == 2) == last).all() and ((st == 0) == g['reset']).all()
  p = dict(corner_right_pays=right & (col == N - 1), corner_left_last_row=last & (col == 0),
           sets_bad=left & (g['row'] == col) & (g['bad'] == 0), ends_bad=last & (orc.s['bad'] == 1),
           ends_good=last & (orc.s['bad'] == 0), clamp_left=left & (col == 0), resets=g['reset'].copy())
  if not g['deterministic']:
    p['noise_drawn'] = last & ((col == 0) | (col == N - 1))
  return p


# ------------------------------------------------------------------------------------------- several folds in one call
# catch 2x5, 513 lanes from LANE_OFFSET, seed SEED, every lane loaded running with 120 pending misses; always-left for 600
# calls: an episode every two calls, a catch only when the ball falls in column 1.
# 513 lanes x 10 cells is not a multiple of 4 (a rollout is then lane advance + store stream per step); 514 lanes is, and
# its rollout is ONE fused launch with the fold inside the loop.
FOLDS = dict(kwargs=dict(rows=2, columns=5), lanes=513, pending=120, calls=600)
FOLD_LANES = (513, 514)


def folds_grid(B=FOLDS['lanes']):
  bx = (np.arange(B) % 5).astype(np.int64)
  by, px, pe = np.zeros(B, np.int64), np.full(B, 5 // 2, np.int64), np.full(B, FOLDS['pending'], np.int64)
  return dict(family='catch', kwargs=dict(FOLDS['kwargs']), n_product=B, lanes=B, rows=2, columns=5, ball_x=bx, paddle_x=px,
              ball_y=by, pending=pe, column=np.zeros(B), reset=np.zeros(B, bool), action=np.zeros(B, np.int32),
              state=catch_words(bx, by, px, pe), info=np.zeros((1, B)), aligned=(B * 10) % 4 == 0, cells=10)
