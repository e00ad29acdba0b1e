"""Test-owned restatement of the lambda-return definition (include/bsuite_amd.h, bsx_lambda_returns) in numpy: a float64 loop
over t, vectorised over lanes, every multiply and add a separate numpy operation — plus the input generator and the grid the CPU
and the GPU tests share."""
import functools

import numpy as np

FIRST, MID, LAST = 0, 1, 2

BS = (1, 63, 64, 65, 257, 1000, 1023)
TS = (1, 2, 3, 7, 33)                       # below the kernel's ring of rows, not a multiple of it, several turns of it
GAMMA_LAMBDA = ((1.0, 1.0), (0.99, 0.9), (0.5, 0.0), (0.0, 1.0))
# (value mode, td requested): td_errors need values
MODES = (('none', False), ('bootstrap', False), ('values', False), ('values', True))


def lambda_returns_ref(reward, discount, values=None, step_type=None, bootstrap=None, gamma=1.0, lambda_=1.0, want_td=False):
  """(returns float32 [T,B], td_errors float32 [T,B] or None) of the definition."""
  T, B = reward.shape
  gamma, lambda_ = np.float64(gamma), np.float64(lambda_)
  one_minus = np.float64(1.0) - lambda_
  zero = np.zeros(B, np.float64)
  vals = values.astype(np.float64) if values is not None else None
  carry = vals[T] if vals is not None else (bootstrap.astype(np.float64) if bootstrap is not None else zero)
  returns = np.empty((T, B), np.float32)
  td = np.empty((T, B), np.float32) if want_td else None
  for t in range(T - 1, -1, -1):
    v = vals[t] if vals is not None else zero
    v_next = vals[t + 1] if vals is not None else zero
    dg = gamma * discount[t].astype(np.float64)
    a = one_minus * v_next
    b = lambda_ * carry
    mix = a + b
    c = dg * mix
    g = reward[t].astype(np.float64) + c
    if step_type is not None:
      g = np.where(step_type[t] == FIRST, v, g)
    carry = g
    returns[t] = g.astype(np.float32)
    if want_td:
      td[t] = (g - v).astype(np.float32)
  return returns, td


def make_step_types(T, B, rng, p_end=0.2, p_restart=0.08):
  """int8 [T,B] with this library's episode structure: a FIRST row after every LAST (auto-reset), a FIRST at row 0 in about
  half the lanes (a window that starts with a reset), and now and then a FIRST after a MID or a FIRST (a lane restarted by
  mark_reset, a window stitched from two calls)."""
  st = np.empty((T, B), np.int8)
  prev = np.where(rng.random(B) < 0.5, LAST, MID)             # what row -1 was: LAST -> row 0 is a FIRST
  for t in range(T):
    u = rng.random(B)
    cur = np.where(u < p_end, LAST, np.where(u < p_end + p_restart, FIRST, MID))
    cur = np.where(prev == LAST, FIRST, cur)
    st[t] = cur
    prev = cur
  return st


@functools.lru_cache(maxsize=None)
def make_inputs(T, B, seed=0, neg_zero=False, small_rewards=False):
  """dict of read-only arrays: reward, discount float32 [T,B], step_type int8 [T,B], values float32 [T+1,B], bootstrap float32
  [B].  Rewards are 0 on FIRST rows and the discount 0 on LAST rows, 1 elsewhere.  neg_zero: a third of the rewards are -0.0
  (FIRST rows too).  small_rewards: rewards from {-1, -0.5, 0, 0.5, 1, 2}, whose float64 sums are exact in any order."""
  rng = np.random.default_rng([seed, T, B])
  st = make_step_types(T, B, rng)
  if small_rewards:
    reward = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0, 2.0], np.float32), size=(T, B))
  else:
    reward = rng.standard_normal((T, B)).astype(np.float32)
  reward = np.where(st == FIRST, np.float32(0.0), reward).astype(np.float32)
  if neg_zero:
    reward = np.where(rng.random((T, B)) < 1 / 3, np.float32(-0.0), reward).astype(np.float32)
  discount = np.where(st == LAST, np.float32(0.0), np.float32(1.0)).astype(np.float32)
  out = dict(reward=reward, discount=discount, step_type=st,
             values=rng.standard_normal((T + 1, B)).astype(np.float32), bootstrap=rng.standard_normal(B).astype(np.float32))
  for a in out.values():
    a.setflags(write=False)
  return out


def select(inp, mode, with_steps):
  """The keyword arguments of one grid case: (values, step_type, bootstrap)."""
  return dict(values=inp['values'] if mode == 'values' else None, step_type=inp['step_type'] if with_steps else None,
              bootstrap=inp['bootstrap'] if mode == 'bootstrap' else None)


def remaining_episode_reward(reward, step_type):
  """float64 [T,B]: the reward still to come in the lane's episode from row t on, row t included — up to its LAST row, the row
  in front of the next FIRST, or the end of the window — and 0 on FIRST rows.  Written forwards, per lane, on purpose."""
  T, B = reward.shape
  out = np.zeros((T, B), np.float64)
  for i in range(B):
    t = 0
    while t < T:
      if step_type[t, i] == FIRST:
        t += 1
        continue
      end = t                                                  # last row of this stretch of transitions
      while step_type[end, i] != LAST and end + 1 < T and step_type[end + 1, i] != FIRST:
        end += 1
      for k in range(t, end + 1):
        out[k, i] = np.sum(reward[k:end + 1, i].astype(np.float64))
      t = end + 1
  return out


def bits(x):
  """uint32 view of a float32 array: equality of bits, so that -0.0 != +0.0 and NaNs compare."""
  return np.ascontiguousarray(x, np.float32).view(np.uint32)
