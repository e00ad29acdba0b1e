"""Index observations against the float32 and uint8 boards, one process: deep_sea/10 and catch/0 at 2^20 lanes, eager
step() and rollout(T), one JSON line per (workload, variant, mode).  The uint8 row is the yardstick (the fastest
observation a board user can ask for), the float32 row the control against profiles/obs_dtype/.

  python tools/bench_obs_index.py [--lanes 1048576] [--steps 200] [--T 32] [--reps 3] [--out FILE]

Lanes carry the steady FIRST / MID / LAST mix (bench.stagger_phases) and the bench's synthetic actions.  Eager rows
alternate the three variants inside each repetition (all three environments are resident); rollout rows build one
environment at a time (T = 32 output slices of float32 deep_sea boards are 121 GB), in the order float32, uint8, index
and back.  Per row: every repetition's ms per step on HIP events (`ms_event_reps`, in the order measured) and their
median, the wall clock around a synchronize, env-steps/s, the algorithmic bytes per step (13 + observation + state:
E * obs_numel for a board, 4 * K for an index row) and their share of the 8 TB/s HBM peak.  The last line per
(workload, mode) says whether the index variant was faster than uint8 in EVERY repetition, and by how much.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

VARIANTS = ('float32', 'uint8', 'index')
INDEX_K = dict(deep_sea=1, catch=2)
WORKLOADS = ('deep_sea', 'catch')


def _make(bsuite_amd, torch, workload, variant, lanes, dev):
  bsuite_id, _, _, _, _, period = bench.WORKLOADS[workload]
  kw = dict(observation_mode='index') if variant == 'index' else dict(observation_dtype=variant)
  env = bsuite_amd.load_from_id(bsuite_id, batch=lanes, device=dev, seed=42, num_buffers=2, **kw)
  actions = bench.synthetic_actions(torch, env.action_spec().num_values, 64, 0, lanes, dev)
  bench.stagger_phases(env, actions, period)
  return env, actions


def _time(torch, run, steps):
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  ev0.record()
  run(steps)
  ev1.record()
  torch.cuda.synchronize()
  return ev0.elapsed_time(ev1) / steps, (time.perf_counter() - t0) * 1e3 / steps


def _bytes_per_step(workload, variant):
  _, _, _, obs_numel, state_bytes, _ = bench.WORKLOADS[workload]
  obs = 4 * INDEX_K[workload] if variant == 'index' else (4 if variant == 'float32' else 1) * obs_numel
  return 13 + obs + state_bytes


def _row(workload, variant, mode, lanes, T, samples):
  ev = statistics.median(s[0] for s in samples)
  wall = statistics.median(s[1] for s in samples)
  bps = _bytes_per_step(workload, variant)
  return bench.sig(dict(workload=workload, bsuite_id=bench.WORKLOADS[workload][0], variant=variant, mode=mode, lanes=lanes,
                        T=T if mode == 'rollout' else None, ms_per_step_event=ev, ms_per_step_wall=wall,
                        ms_event_reps=[s[0] for s in samples],
                        env_steps_per_s=lanes / (wall * 1e-3), algorithmic_bytes_per_step=bps,
                        frac_8tbs=bps * lanes / (ev * 1e-3) / 1e9 / bench.HBM_PEAK_GBPS, reps=len(samples)))


def _verdict(workload, mode, samples):
  ratios = [u[0] / i[0] for u, i in zip(samples['uint8'], samples['index'])]
  return bench.sig(dict(workload=workload, mode=mode, index_faster_than_uint8_in_every_rep=all(r > 1.0 for r in ratios),
                        uint8_over_index_reps=ratios))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--modes', default='eager,rollout')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_obs_index.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  out = open(a.out, 'a') if a.out else None

  def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  for w in a.workloads.split(','):
    if 'eager' in a.modes:
      envs = {v: _make(bsuite_amd, torch, w, v, a.lanes, dev) for v in VARIANTS}
      runs = {}
      for v, (env, acts) in envs.items():
        runs[v] = (lambda env, acts: lambda n: [env.step(acts[t % acts.shape[0]]) for t in range(n)])(env, acts)
        runs[v](32)                                                # warm-up
      samples = {v: [] for v in VARIANTS}
      for rep in range(a.reps):
        for v in (VARIANTS if rep % 2 == 0 else VARIANTS[::-1]):
          samples[v].append(_time(torch, runs[v], a.steps))
      for v in VARIANTS:
        emit(_row(w, v, 'eager', a.lanes, None, samples[v]))
      emit(_verdict(w, 'eager', samples))
      del envs, runs
      torch.cuda.empty_cache()
    if 'rollout' in a.modes:
      samples = {v: [] for v in VARIANTS}
      chunks = max(1, a.steps // a.T)
      for rep in range(a.reps):
        for v in (VARIANTS if rep % 2 == 0 else VARIANTS[::-1]):
          env, acts = _make(bsuite_amd, torch, w, v, a.lanes, dev)
          roll = acts[:a.T].contiguous()
          run = lambda n, env=env, roll=roll: [env.rollout(roll) for _ in range(n // a.T)]
          run(2 * a.T)                                             # warm-up (allocates the [T, B, ...] outputs)
          samples[v].append(_time(torch, run, chunks * a.T))
          del env, acts, roll, run
          torch.cuda.empty_cache()
      for v in VARIANTS:
        emit(_row(w, v, 'rollout', a.lanes, a.T, samples[v]))
      emit(_verdict(w, 'rollout', samples))
  if out:
    out.close()


if __name__ == '__main__':
  main()
