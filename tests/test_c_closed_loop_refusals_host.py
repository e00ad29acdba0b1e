"""CPU: the forty fused closed-loop C entry points (bsx_<family>_<kind>_<rollout|evaluate|sample|sample_evaluate>) return
exactly the codes, in exactly the order, that they returned before they were given one host-side prologue.

tests/golden/.tools/c_closed_loop_refusals.json (tools/make_c_closed_loop_refusals_golden.py) is a characterisation
fixture: recorded at the commit it names, from the entry points as they were written out family by family, and never
regenerated from changed code (that would defeat it).  Every case is refused or empty, so nothing here reaches a launch;
the cases named 'a+b' carry two faults of different classes and pin the order: the recorded code is the earlier fault's.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_c_closed_loop_refusals_golden as refusals     # pylint: disable=wrong-import-position
sys.path.pop(0)


def test_every_entry_point_returns_the_recorded_code():
  want, parent = refusals.load()
  assert len(parent) == 40 and len(refusals.ENTRIES) == 40
  assert len(want) > 6000 and {key.split('/')[0] for key in want} == set(refusals.ENTRIES)
  got = refusals.record()                                    # (asserts of every case that it is refused or empty)
  assert set(got) == set(want)
  wrong = {key: (got[key], want[key]) for key in want if got[key] != want[key]}
  assert not wrong, (len(wrong), list(wrong.items())[:8])


def test_the_catalogue_reaches_every_code_and_the_last_refusal_of_each_entry_point():
  """The fixture itself: per entry point every code it can return before launching, the two-fault cases, and its last
  refusal before the launch — the grid bound, and for a recording physics call the 4 GiB slab behind every pointer."""
  want, _ = refusals.load()
  for entry in refusals.ENTRIES:
    own = {key[len(entry) + 1:]: code for key, code in want.items() if key.startswith(entry + '/')}
    fam, kind, verb = refusals.parts(entry)
    # (BSX_EALIGN: the grid calls' boards, logits and matrices — bsx_<family>_policy_evaluate has none of them: it reads a
    # table of bytes and writes no board)
    aligns = fam in refusals.GRID and (refusals.records(verb) or refusals.drawn(verb) or kind == 'embedding')
    codes = {'ENULL', 'EMODE', 'EINVAL', 'ERANGE', 'OK'} | ({'EALIGN'} if aligns else set())
    assert set(own.values()) == codes, entry
    assert sum(1 for cid in own if '+' in cid) >= 50, entry
    assert own['n_lanes=0'] == 'OK' and all('n_lanes=0' in cid.split('+') for cid, code in own.items() if code == 'OK'), entry
    assert own['n_lanes=2^40'] == 'EINVAL' and own['action_ring=-2'] == 'EINVAL', entry
    assert own['state=NULL+n_lanes=2^40'] == 'ENULL', entry                             # (the grid bound comes last)
    recording_physics = fam in refusals.PHYSICS and refusals.records(verb)
    assert ('slab' in own) == recording_physics, entry
    if recording_physics:
      assert own['slab'] == own['slab:n_lanes=2^31'] == 'EINVAL' and own['state=NULL+slab'] == 'ENULL', entry
    elif fam in refusals.PHYSICS:
      assert own['state=NULL+slab'] == 'ENULL' and own['cfg=NULL+slab'] == 'ENULL', entry
    if fam == 'cartpole':
      assert own['derive:theta_offset,init_range>32'] == 'ERANGE' and own['time_frac=NULL'] == 'ENULL', entry
      assert own['derive:theta_offset,init_range>32+flags=U8'] == 'ERANGE', entry      # (the cfg's range before the kind's check)
    if refusals.drawn(verb):
      for b in refusals.BAD_BETAS:
        assert own[f'inv_temperature={b!r}'] == 'ERANGE', (entry, b)
      assert own['inv_temperature=inf+n_lanes=0'] == 'ERANGE', entry                    # an empty call still checks its scalars
