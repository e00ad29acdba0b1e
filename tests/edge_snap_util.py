"""What the GPU edge-grid tests (tests/test_gpu_physics_edges.py, tests/test_gpu_grid_edges.py,
tests/test_gpu_chain_edges.py) share: snapshots of a TimeStep and of what an environment holds after a call, as bit patterns
on the device, and their exact comparison with the lanes that differ named in the failure."""
import torch

from tests import engine_util as eu

TS_FIELDS = ('step_type', 'reward', 'discount', 'observation')


def bits(t):
  """A floating-point tensor as the integers of its bit patterns (any other tensor as it is)."""
  if not t.is_floating_point():
    return t
  return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def snap_ts(ts):
  return {f: bits(getattr(ts, f)).clone() for f in TS_FIELDS}


def snap_after(env):
  r = eu.raw(env)
  return dict(state={k: bits(v).clone() for k, v in r._state.items()},          # pylint: disable=protected-access
              info={k: bits(v).clone() for k, v in r.bsuite_info().items()},
              raw_info=bits(r._info).clone(),                                   # pylint: disable=protected-access
              counters=r.episode_counters().clone(), step_index=r.step_index)


def stack(snaps, T):
  return {f: torch.stack([s[f] for s in snaps[:T]]) for f in snaps[0]}


def assert_ts(got, want, what, fields=TS_FIELDS, rows=None):
  stacked = want['step_type'].dim() == 2                                        # [T, B, ...] of a rollout, else [B, ...]
  for f in fields:
    w = want[f] if rows is None else want[f][rows]
    if not torch.equal(got[f], w):
      d = (got[f] != w).movedim(1, 0) if stacked else got[f] != w
      bad = d.reshape(d.shape[0], -1).any(dim=1).nonzero().flatten()
      raise AssertionError(f'{what}: {f} differs from the eager step on {len(bad)} lanes, first {bad[:8].tolist()}')


def assert_after(got, want, what, info=True, rows=None, state_mask=None, raw_info=False):
  """rows: `got` holds those lanes of `want` (the counters are then the caller's to check).  state_mask: the bits of the state
  words that are compared.  raw_info: the info columns themselves as well as bsuite_info()."""
  for k, w in want['state'].items():
    w, s = (w if rows is None else w[..., rows]), got['state'][k]
    if state_mask is not None:
      w, s = w & state_mask, s & state_mask
    if not torch.equal(s, w):
      bad = (s != w).reshape(-1, w.shape[-1]).any(dim=0).nonzero().flatten()
      raise AssertionError(f'{what}: state column {k!r} differs from the eager step on {len(bad)} lanes, first {bad[:8].tolist()}')
  if info:
    for k, w in want['info'].items():
      w = w if rows is None else w[rows]
      if not torch.equal(got['info'][k], w):
        bad = (got['info'][k] != w).nonzero().flatten()
        raise AssertionError(f'{what}: bsuite_info {k!r} differs from the eager step on {len(bad)} lanes, first {bad[:8].tolist()}')
  if raw_info:
    w = want['raw_info'] if rows is None else want['raw_info'][:, rows]
    assert torch.equal(got['raw_info'], w), (what, 'the info columns themselves')
  if rows is None:
    assert torch.equal(got['counters'], want['counters']), (what, 'episode_counters', got['counters'].tolist(), want['counters'].tolist())
  assert got['step_index'] == want['step_index'], (what, 'call index')
