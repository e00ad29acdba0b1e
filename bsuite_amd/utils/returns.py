"""Returns of a recorded trajectory: `lambda_returns`, `td_lambda` and `trajectory_targets` turn the `[T,B]` TimeStep of a
recording call (`rollout_*`, `sample_*`) into the targets a policy-gradient or actor-critic learner builds its loss from — the
last step of `bsuite/baselines/jax/actor_critic/agent.py:60-66` (`rlax.td_lambda`) on this library's layout.

The definition (include/bsuite_amd.h, `bsx_lambda_returns`).  All inputs `[T,B]`, T >= 1; `values` is `[T+1,B]` with `values[0]`
the value of the observation the trajectory started from and `values[t+1]` the value of `ts.observation[t]` (rlax's
`v_tm1 = values[:-1]`, `v_t = values[1:]`).  Each lane i on its own, in float64, every multiply and add rounded on its own,
`one_minus = 1.0 - lambda_` computed once on the host:

    vals(t) = values[t][i] if values is given else +0.0
    carry   = values[T][i] if values is given else (bootstrap[i] if bootstrap is given else +0.0)
    for t = T-1 .. 0:
      if step_type is given and step_type[t][i] == FIRST:
        g = vals(t)                           # the row is no transition: its td error is exactly 0 ...
      else:
        dg  = gamma * discount[t][i]
        mix = one_minus * vals(t+1) + lambda_ * carry
        g   = reward[t][i] + dg * mix
      carry = g                               # ... and the row before it bootstraps from the value of its own last
                                              #     observation only (truncation), never from the new episode
      returns[t][i]   = float32(g)
      td_errors[t][i] = float32(g - vals(t))  # td_lambda only

A LAST row has discount 0, which cuts the recursion by itself; the FIRST rule adds what the discount cannot express: a lane
restarted by `mark_reset`, or a window stitched from two calls, has a FIRST with no LAST in front of it.  With `lambda_ = 1` and
no values this is the discounted Monte-Carlo return; with values it is `rlax.lambda_returns`, and `td_errors` is `rlax.td_lambda`
on the rows that are transitions.  "No values" is the arithmetic above with +0.0, additions included.

Device tensors go to one kernel launch on the current torch stream (csrc/returns.hip).  CPU tensors take `torch_scan`, the same
definition in separate float64 torch operations — no native call, the same numbers bit for bit.
"""
import ctypes
import math
import numbers
from typing import NamedTuple, Optional

import torch

from bsuite_amd import _native

FIRST = _native.FIRST


class TDLambda(NamedTuple):
  td_errors: Optional[torch.Tensor]     # float32 [T,B]; None from trajectory_targets without values
  returns: torch.Tensor                 # float32 [T,B]


def _unit(name, x):
  if isinstance(x, bool) or not isinstance(x, numbers.Real):
    raise ValueError(f'{name} must be a number in [0, 1], got {x!r}')
  x = float(x)
  if math.isnan(x) or not 0.0 <= x <= 1.0:
    raise ValueError(f'{name} must be a number in [0, 1], got {x!r}')
  return x


def _column(name, x, dtype, shape, device):
  if not isinstance(x, torch.Tensor):
    raise ValueError(f'{name} must be a torch tensor, got {type(x).__name__}')
  if x.dtype != dtype:
    raise ValueError(f'{name} must be {dtype}, got {x.dtype}')
  if shape is not None and tuple(x.shape) != shape:
    raise ValueError(f'{name} must have shape {shape}, got {tuple(x.shape)}')
  if device is not None and x.device != device:
    raise ValueError(f'{name} is on {x.device}, reward on {device}: all tensors must be on one device')
  if not x.is_contiguous():
    raise ValueError(f'{name} must be contiguous')
  return x


def _check(what, reward, discount, values, step_type, bootstrap, gamma, lambda_, out):
  """Every refusal, before any device work.  Returns (T, B, gamma, lambda_)."""
  gamma, lambda_ = _unit(f'{what}: gamma', gamma), _unit(f'{what}: lambda_', lambda_)
  _column(f'{what}: reward', reward, torch.float32, None, None)
  if reward.dim() != 2:
    raise ValueError(f'{what}: reward must be [T, B], got {tuple(reward.shape)}')
  T, B = int(reward.shape[0]), int(reward.shape[1])
  if T < 1:
    raise ValueError(f'{what}: a trajectory has T >= 1 rows, got T = {T}')
  dev = reward.device
  _column(f'{what}: discount', discount, torch.float32, (T, B), dev)
  if values is not None and bootstrap is not None:
    raise ValueError(f'{what}: bootstrap is the value behind the last row when there are no values; values[T] is that value already')
  if values is not None:
    _column(f'{what}: values', values, torch.float32, (T + 1, B), dev)
  if step_type is not None:
    _column(f'{what}: step_type', step_type, torch.int8, (T, B), dev)
  if bootstrap is not None:
    _column(f'{what}: bootstrap', bootstrap, torch.float32, (B,), dev)
  if out is not None:
    _column(f'{what}: out', out, torch.float32, (T, B), dev)
    if B > 0:
      mine = out.untyped_storage().data_ptr()
      for name, x in (('reward', reward), ('discount', discount), ('values', values), ('step_type', step_type), ('bootstrap', bootstrap)):
        if x is not None and x.untyped_storage().data_ptr() == mine:
          raise ValueError(f'{what}: out shares its storage with {name}')
  return T, B, gamma, lambda_


def torch_scan(reward, discount, values=None, *, gamma=1.0, lambda_=1.0, step_type=None, bootstrap=None, want_td=False, out=None):
  """The definition in torch, one row at a time: `(returns, td_errors or None)`.  Separate float64 operations, so every multiply
  and add is rounded on its own on any device.  It is the CPU path of this module, the loop the kernel replaces (on device
  tensors: some twelve small launches per row) and what tools/bench_returns.py measures the kernel against.  No checks."""
  T, B = int(reward.shape[0]), int(reward.shape[1])
  one_minus = 1.0 - lambda_
  zero = torch.zeros((B,), dtype=torch.float64, device=reward.device)
  vals = values.to(torch.float64) if values is not None else None
  carry = vals[T] if vals is not None else (bootstrap.to(torch.float64) if bootstrap is not None else zero)
  returns = out if out is not None else torch.empty((T, B), dtype=torch.float32, device=reward.device)
  td = torch.empty((T, B), dtype=torch.float32, device=reward.device) if want_td else None
  for t in range(T - 1, -1, -1):
    v = vals[t] if vals is not None else zero
    v_next = vals[t + 1] if vals is not None else zero
    dg = gamma * discount[t].to(torch.float64)
    mix = one_minus * v_next + lambda_ * carry
    g = reward[t].to(torch.float64) + dg * mix
    if step_type is not None:
      g = torch.where(step_type[t] == FIRST, v, g)
    carry = g
    returns[t] = g.to(torch.float32)
    if want_td:
      td[t] = (g - v).to(torch.float32)
  return returns, td


def _run(what, reward, discount, values, step_type, bootstrap, gamma, lambda_, want_td, out):
  T, B, gamma, lambda_ = _check(what, reward, discount, values, step_type, bootstrap, gamma, lambda_, out)
  dev = reward.device
  if B == 0:
    empty = lambda: torch.empty((T, 0), dtype=torch.float32, device=dev)
    return (out if out is not None else empty()), (empty() if want_td else None)
  if dev.type != 'cuda':
    return torch_scan(reward, discount, values, gamma=gamma, lambda_=lambda_, step_type=step_type, bootstrap=bootstrap,
                      want_td=want_td, out=out)
  returns = out if out is not None else torch.empty((T, B), dtype=torch.float32, device=dev)
  td = torch.empty((T, B), dtype=torch.float32, device=dev) if want_td else None
  ptr = lambda x: None if x is None else x.data_ptr()
  r = _native.Returns(n_lanes=B, n_steps=T, reward=ptr(reward), discount=ptr(discount), step_type=ptr(step_type),
                      values=ptr(values), bootstrap=ptr(bootstrap), gamma=gamma, lambda_=lambda_,
                      returns=ptr(returns), td_errors=ptr(td))
  with torch.cuda.device(dev):
    rc = _native.lib.bsx_lambda_returns(ctypes.byref(r), torch.cuda.current_stream(dev).cuda_stream)
  _native.check(rc, what)
  return returns, td


def lambda_returns(reward, discount, values=None, *, gamma=1.0, lambda_=1.0, step_type=None, bootstrap=None, out=None):
  """`returns` float32 `[T,B]` of the module's definition.  reward, discount: float32 `[T,B]`; values: float32 `[T+1,B]` or
  None; step_type: int8 `[T,B]` or None (no FIRST rule); bootstrap: float32 `[B]`, the value behind the last row, only without
  values; out: a float32 `[T,B]` tensor to write into, sharing storage with no input.  All contiguous and on one device.
  ValueError for anything else, and for gamma or lambda_ outside [0, 1], before any device work."""
  return _run('lambda_returns', reward, discount, values, step_type, bootstrap, gamma, lambda_, False, out)[0]


def td_lambda(reward, discount, values, *, gamma=1.0, lambda_=1.0, step_type=None):
  """`TDLambda(td_errors, returns)`, both float32 `[T,B]`, from one launch: `lambda_returns` and `returns - values[:-1]` computed
  in float64 before the rounding — 0 exactly on FIRST rows.  `values` (float32 `[T+1,B]`) is required."""
  if values is None:
    raise ValueError('td_lambda: values is required (lambda_returns computes returns without a critic)')
  returns, td = _run('td_lambda', reward, discount, values, step_type, None, gamma, lambda_, True, None)
  return TDLambda(td, returns)


def trajectory_targets(ts, values=None, *, gamma=1.0, lambda_=1.0, bootstrap=None):
  """The targets of the `[T,B]` TimeStep `ts` a recording call returned: `td_lambda(ts.reward, ts.discount, values, ...,
  step_type=ts.step_type)` with values, else `TDLambda(None, lambda_returns(ts.reward, ts.discount, ..., step_type=ts.step_type,
  bootstrap=bootstrap))`."""
  if values is not None:
    if bootstrap is not None:
      raise ValueError('trajectory_targets: bootstrap is the value behind the last row when there are no values; values[T] is that value already')
    return td_lambda(ts.reward, ts.discount, values, gamma=gamma, lambda_=lambda_, step_type=ts.step_type)
  return TDLambda(None, lambda_returns(ts.reward, ts.discount, gamma=gamma, lambda_=lambda_, step_type=ts.step_type, bootstrap=bootstrap))
