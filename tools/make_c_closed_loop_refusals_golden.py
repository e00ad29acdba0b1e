"""Writes tests/golden/.tools/c_closed_loop_refusals.json: the code each of the forty fused closed-loop C entry points
(bsx_<cartpole|mountain_car>_<linear|mlp|mlp2>_<verb> and bsx_<deep_sea|catch>_<policy|embedding>_<verb>, verb = rollout,
evaluate, sample, sample_evaluate) returns for a catalogue of bad arguments, called through ctypes (`_native.lib`) with
garbage standing in for device pointers.  A case is one fault or two faults of different classes ('a+b'); the two-fault
cases pin the ORDER of the refusals: the code recorded is the earlier fault's.

NO case reaches a launch: every one is refused (a negative BSX_E* code) or empty (n_lanes == 0, code 0).  `record()`
asserts that of each case, and `main()` refuses to run where a GPU is visible.

It is a characterisation fixture: recorded once, at the commit the fixture names (`parent`), before the entry points were
given one host-side prologue, and asserted exactly by tests/test_c_closed_loop_refusals_host.py.  Regenerating it from
changed code to make that test pass defeats it.

  python tools/make_c_closed_loop_refusals_golden.py <parent commit hash>      # rewrites the fixture
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from bsuite_amd import _native                                                        # pylint: disable=wrong-import-position

OUT = os.path.join(ROOT, 'tests', 'golden', '.tools', 'c_closed_loop_refusals.json')
E = _native
CODES = {0: 'OK', E.BSX_EINVAL: 'EINVAL', E.BSX_ENULL: 'ENULL', E.BSX_EALIGN: 'EALIGN', E.BSX_ERANGE: 'ERANGE', E.BSX_EMODE: 'EMODE'}
JUNK = 0xDEAD0010                               # never mapped: a dereference would fault (16-byte aligned)
PHYSICS, GRID = ('cartpole', 'mountain_car'), ('deep_sea', 'catch')
VERBS = ('rollout', 'evaluate', 'sample', 'sample_evaluate')
ENTRIES = tuple(f'bsx_{fam}_{kind}_{verb}' for fams, kinds in ((PHYSICS, ('linear', 'mlp', 'mlp2')), (GRID, ('policy', 'embedding')))
                for fam in fams for kind in kinds for verb in VERBS)
NAN, INF = float('nan'), float('inf')
BAD_BETAS = (0.0, -0.0, -1.0, NAN, INF, -INF)
CELLS = dict(deep_sea=(64, 64, 2), catch=(250, 50, 3))        # (table length, cells, actions) of the good cfg below


def parts(entry):
  fam = next(f for f in PHYSICS + GRID if entry.startswith(f'bsx_{f}_'))
  kind, verb = entry[len(f'bsx_{fam}_'):].split('_', 1)
  return fam, kind, verb


def records(verb):
  return verb in ('rollout', 'sample')


def drawn(verb):
  return verb.startswith('sample')


def good(entry):
  """Valid arguments of `entry`, by name, every pointer garbage: with n_lanes > 0 and no fault they would launch."""
  fam, kind, verb = parts(entry)
  a = dict(call=E.Call(n_lanes=4, n_steps=4, flags=E.CALL_OBS_INDEX if fam in GRID else 0), state=JUNK, info=JUNK)
  if fam == 'cartpole':
    a['cfg'] = E.CartpoleCfg(swingup=0, last_step=1001, height_threshold=0.8, x_threshold=3.0, theta_dot_threshold=1.0,
                             x_reward_threshold=1.0, timescale=0.01, mass_cart=1.0, mass_pole=0.1, length=0.5, force_mag=10.0,
                             gravity=9.8, move_cost=0.0, init_range=0.05, theta_offset=0.0, time_frac=0xDEAD0008)
  elif fam == 'mountain_car':
    a['cfg'] = E.MountainCarCfg(1000, 0)
  elif fam == 'deep_sea':
    a['cfg'] = E.DeepSeaCfg(size=8, deterministic=1, move_cost=0.001, inv_size=0.125)
  else:
    a['cfg'] = E.CatchCfg(10, 5)
  if fam in PHYSICS:
    common = dict(n_policies=1, policy_index=None, epsilon=0.0, explore_seed=0, observation_in=JUNK)
    a['policy'] = (E.Linear(weights=JUNK, **common) if kind == 'linear' else
                   E.Mlp(w1=JUNK, w2=JUNK, hidden=5, **common) if kind == 'mlp' else
                   E.Mlp2(w1=JUNK, w2=JUNK, w3=JUNK, hidden1=5, hidden2=4, **common))
    a['steps'] = JUNK
    if drawn(verb):
      a['beta'] = 1.0
    if records(verb):
      a['out'], a['actions'] = E.TimeStepPtrs(JUNK, JUNK, JUNK, JUNK), JUNK
    else:
      a['out'] = E.LinearEvalPtrs(JUNK, JUNK, JUNK, JUNK)
  else:
    S, C, A = CELLS[fam]
    tail = (dict(inv_temperature=1.0, sample_seed=0) if drawn(verb) else dict(epsilon=0.0, explore_seed=0))
    tail.update(n_policies=1, policy_index=None, actions_out=JUNK)
    if kind == 'policy':
      a['policy'] = E.PolicyLogits(logits=JUNK, n_states=S, n_actions=A, **tail) if drawn(verb) else E.Policy(table=JUNK, n_states=S, **tail)
    else:
      a['policy'] = (E.PolicyEmbeddingSample if drawn(verb) else E.PolicyEmbedding)(w1=JUNK, w2=JUNK, n_cells=C, n_hidden=5, n_actions=A, **tail)
    a['out'] = E.TimeStepPtrs(JUNK, JUNK, JUNK, JUNK) if records(verb) else E.PolicyEvalPtrs(JUNK, JUNK, JUNK)
  return a


def run(entry, a):
  fam, _, verb = parts(entry)
  ref = lambda s: ctypes.byref(s) if s is not None else None
  args = [ref(a['cfg']), ref(a['call']), ref(a['policy'])]
  if fam in PHYSICS:
    args += ([a['beta']] if drawn(verb) else []) + [a['state'], a['steps'], a['out']] + ([a['actions']] if records(verb) else [])
  else:
    args += [a['state'], a['out']]
  return getattr(E.lib, entry)(*args, a['info'])


def _set(path, value):
  """A fault: sets `path` ('call.wrap.kind', 'state', 'policy.w1', ...) of the arguments to `value`."""
  def apply(a):
    names = path.split('.')
    if len(names) == 1:
      a[path] = value
      return
    obj = a[names[0]]
    for n in names[1:-1]:
      obj = getattr(obj, n)
    setattr(obj, names[-1], value)
  return apply


def _both(*fs):
  def apply(a):
    for f in fs:
      f(a)
  return apply


def _logging(a):
  a['_keep'] = E.Logging()
  a['call'].logging = ctypes.pointer(a['_keep'])


def faults(entry):
  """[(class, id, fields touched, apply, representative)]: the single faults of `entry`, in the documented order of their
  classes.  `representative` faults are the ones paired across classes."""
  fam, kind, verb = parts(entry)
  physics, rec, drw = fam in PHYSICS, records(verb), drawn(verb)
  out = []

  def add(cls, fid, path, value, rep=False):
    out.append((cls, fid, {path}, _set(path, value), rep))

  for s in ('cfg', 'call', 'policy'):
    add('null', f'{s}=NULL', s, None, rep=s == 'cfg')
  # the cfg
  if fam == 'cartpole':
    add('cfg', 'last_step=0', 'cfg.last_step', 0, rep=True)
    add('cfg', 'last_step=2^30', 'cfg.last_step', 1 << 30)
    add('cfg', 'x_threshold=0', 'cfg.x_threshold', 0.0)
    out.append(('cfg', 'derive:theta_offset,init_range>32', {'cfg.theta_offset', 'cfg.init_range'},
                _both(_set('cfg.theta_offset', 31.0), _set('cfg.init_range', 2.0)), True))
  elif fam == 'mountain_car':
    add('cfg', 'max_steps=0', 'cfg.max_steps', 0, rep=True)
    add('cfg', 'max_steps=2^30', 'cfg.max_steps', 1 << 30)
  elif fam == 'deep_sea':
    add('cfg', 'size=0', 'cfg.size', 0)
    add('cfg', 'size=65', 'cfg.size', 65, rep=True)
  else:
    add('cfg', 'rows=1', 'cfg.rows', 1, rep=True)
    add('cfg', 'rows=65', 'cfg.rows', 65)
    add('cfg', 'columns=0', 'cfg.columns', 0)
    add('cfg', 'columns=65', 'cfg.columns', 65)
  # the modes
  flags = dict(INDEX=E.CALL_OBS_INDEX, U8=E.CALL_OBS_U8, F16=E.CALL_OBS_F16, BF16=E.CALL_OBS_BF16,
               INDEX_U8=E.CALL_OBS_INDEX | E.CALL_OBS_U8, F32=0)
  for k, v in flags.items():
    if v != (0 if physics else E.CALL_OBS_INDEX):
      add('mode', f'flags={k}', 'call.flags', v, rep=k == 'U8')
  out.append(('mode', 'logging', {'call.logging'}, _logging, False))
  for k in ('SCALE', 'NOISE', 'SCALE_NOISE', 'NOISE_SCALE'):
    add('mode', f'wrap={k}', 'call.wrap.kind', getattr(E, f'WRAP_{k}'))
  out.append(('mode', 'mt_state,mt_pos', {'call.stream.mt_state', 'call.stream.mt_pos'},
              _both(_set('call.stream.mt_state', JUNK), _set('call.stream.mt_pos', JUNK)), False))
  add('mode', 'mt_pos', 'call.stream.mt_pos', JUNK)
  for member in ('reward_f64', 'obs_paint', 'state_alt'):
    add('mode', member, f'call.{member}', JUNK)
  add('mode', 'force_reset', 'call.force_reset', 1)
  add('mode', 'action_ring=4', 'call.action_ring', 4, rep=True)
  # the scalars
  for n in (0, -1):
    add('scalar', f'n_steps={n}', 'call.n_steps', n, rep=n == 0)
  add('scalar', 'n_lanes=-1', 'call.n_lanes', -1)
  add('scalar', 'n_lanes=2^40+1', 'call.n_lanes', (1 << 40) + 1)
  for n in (0, -3):
    add('scalar', f'n_policies={n}', 'policy.n_policies', n, rep=n == 0)
  widths = dict(mlp=('hidden',), mlp2=('hidden1', 'hidden2'), embedding=('n_hidden',)).get(kind, ())
  for w in widths:
    for h in (0, -1, 65, 1 << 20):
      add('scalar', f'{w}={h}', f'policy.{w}', h, rep=h == 65)
  if not physics:
    S, C, A = CELLS[fam]
    if kind == 'policy':
      for n in (S - 1, S + 1, 0):
        add('scalar', f'n_states={n}', 'policy.n_states', n, rep=n == S + 1)
      if drw:
        for n in (A - 1, A + 1):
          add('scalar', f'n_actions={n}', 'policy.n_actions', n)
    else:
      for n in (C - 1, C + 1):
        add('scalar', f'n_cells={n}', 'policy.n_cells', n, rep=n == C + 1)
      for n in (A - 1, A + 1):
        add('scalar', f'n_actions={n}', 'policy.n_actions', n)
  # epsilon / the inverse temperature
  beta = 'beta' if physics else 'policy.inv_temperature'
  if drw:
    for b in BAD_BETAS:
      add('range', f'inv_temperature={b!r}', beta, b, rep=b in (0.0, INF) and str(b) != '-0.0')
    if physics:
      for eps in (0.3, 1.0, NAN):
        add('range', f'epsilon={eps!r}', 'policy.epsilon', eps)
  else:
    for eps in (-0.1, 1.5, NAN, INF):
      add('range', f'epsilon={eps!r}', 'policy.epsilon', eps, rep=eps == 1.5)
  # an empty call
  add('empty', 'n_lanes=0', 'call.n_lanes', 0, rep=True)
  # the pointers
  ptrs = dict(linear=('weights',), mlp=('w1', 'w2'), mlp2=('w1', 'w2', 'w3'), embedding=('w1', 'w2'),
              policy=('logits',) if drw else ('table',))[kind]
  for p in ptrs + (('observation_in',) if physics else ()):
    add('pointer', f'{p}=NULL', f'policy.{p}', None, rep=p in ('w2', 'w3'))
  if not physics and rec:                       # (an evaluation does not look at actions_out)
    add('pointer', 'actions_out=NULL', 'policy.actions_out', None)
  for p in ('state', 'info') + (('steps',) if physics else ()) + (('actions',) if physics and rec else ()):
    add('pointer', f'{p}=NULL', p, None, rep=p == 'state')
  out_fields = ('reward', 'discount', 'step_type', 'observation') if rec else \
               ('episodes', 'return_sum', 'episode_return_sum') + (('observation_out',) if physics else ())
  for p in out_fields:
    add('pointer', f'out.{p}=NULL', f'out.{p}', None)
  add('pointer', 'population without policy_index', 'policy.n_policies', 2, rep=True)
  if fam == 'cartpole':
    add('pointer', 'time_frac=NULL', 'cfg.time_frac', None, rep=True)
  # alignment
  if not physics:
    if rec:
      add('align', 'out.observation+4', 'out.observation', JUNK + 4, rep=True)
    for p in (('w1', 'w2') if kind == 'embedding' else ('logits',) if drw else ()):
      add('align', f'{p}+2', f'policy.{p}', JUNK + 2, rep=p in ('w1', 'logits'))
    if rec:                                     # what only the family's make() refuses, after the kind's checks
      add('late', 'mt_gauss', 'call.stream.mt_gauss', JUNK, rep=True)
  # what comes last
  add('late', 'action_ring=-2', 'call.action_ring', -2, rep=True)
  add('last', 'n_lanes=2^40', 'call.n_lanes', 1 << 40, rep=True)
  if physics:
    D = 3 if fam == 'mountain_car' else 6
    # the first batch whose [B, D] slab reaches 4 GiB: refused by a recording call, and by it alone — so the other calls
    # get it only next to a fault of their own
    for fid, n in (('slab', -(-(1 << 32) // (4 * D))), ('slab:n_lanes=2^31', 1 << 31)):
      out.append(('slab', fid, {'call.n_lanes'}, _set('call.n_lanes', n), rec and fid == 'slab'))
      if not rec:
        out[-1] = ('slab-unrefused', fid, {'call.n_lanes'}, _set('call.n_lanes', n), fid == 'slab')
  return out


def _clash(t1, t2):
  """Two faults write the same argument, or one removes the struct the other writes into."""
  return any(p == q or p.startswith(q + '.') or q.startswith(p + '.') for p in t1 for q in t2)


def cases(entry):
  """(case id, [apply, ...]) of `entry`: every single fault, then every pair of representative faults of two classes."""
  fs = faults(entry)
  for cls, fid, _, apply, _ in fs:
    if cls != 'slab-unrefused':
      yield fid, [apply]
  reps = [f for f in fs if f[4]]
  for (c1, i1, t1, f1, _), (c2, i2, t2, f2, _) in itertools.combinations(reps, 2):
    if c1 != c2 and not _clash(t1, t2):
      yield f'{i1}+{i2}', [f1, f2]


def record(entries=ENTRIES):
  """{'<entry>/<case id>': code name}.  Asserts of every case that it is refused or empty."""
  got = {}
  for entry in entries:
    for cid, applies in cases(entry):
      a = good(entry)
      for f in applies:
        f(a)
      rc = run(entry, a)
      n_lanes = a['call'].n_lanes if a['call'] is not None else None
      assert rc in CODES and (rc != 0 or n_lanes == 0), f'{entry}/{cid}: code {rc} — the case was not refused before the launch'
      key = f'{entry}/{cid}'
      assert key not in got, key
      got[key] = CODES[rc]
  return got


def pack(got, parent):
  """The fixture's layout: `outcomes` the distinct code names; `cases`: case id -> per entry of `entries`, the index of its
  outcome, -1 where the entry has no such case."""
  outcomes, rows = [], {}
  for key, code in got.items():
    entry, cid = key.split('/', 1)
    if code not in outcomes:
      outcomes.append(code)
    rows.setdefault(cid, [-1] * len(ENTRIES))[ENTRIES.index(entry)] = outcomes.index(code)
  z = dict(parent=parent, entries=list(ENTRIES), outcomes=outcomes, cases=rows)
  assert unpack(z) == got
  return z


def unpack(z):
  return {f'{entry}/{cid}': z['outcomes'][k] for cid, row in z['cases'].items() for entry, k in zip(z['entries'], row) if k >= 0}


def load():
  """({'<entry>/<case id>': code name}, parent commit) of the committed fixture."""
  with open(OUT) as f:
    z = json.load(f)
  return unpack(z), z['parent']


def main():
  import torch                                  # pylint: disable=import-outside-toplevel
  if torch.cuda.is_available():
    raise SystemExit('record this fixture on a machine without a GPU: a case that is not refused would launch')
  if len(sys.argv) != 2:
    raise SystemExit(__doc__)
  z = pack(record(), sys.argv[1])
  os.makedirs(os.path.dirname(OUT), exist_ok=True)
  with open(OUT, 'w') as f:                      # one case per line
    f.write('{"parent": %s,\n"entries": %s,\n"outcomes": %s,\n"cases": {\n%s\n}}\n' % (
        json.dumps(z['parent']), json.dumps(z['entries']), json.dumps(z['outcomes']),
        ',\n'.join(f'{json.dumps(cid)}: {json.dumps(row, separators=(",", ":"))}' for cid, row in z['cases'].items())))
  print(f'{len(unpack(z))} cases, {len(z["cases"])} rows -> {OUT} ({os.path.getsize(OUT)} bytes)')


if __name__ == '__main__':
  main()
