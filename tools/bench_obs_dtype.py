"""Narrow observation dtypes against float32, one process: deep_sea/10 and catch/0 at 2^20 lanes, eager step() and
rollout(T), one JSON line per (workload, dtype, mode).  The float32 row of each pair is the control.

  python tools/bench_obs_dtype.py [--lanes 1048576] [--steps 200] [--T 32] [--reps 3] [--out FILE]

Lanes carry the steady FIRST / MID / LAST mix (bench.stagger_phases) and the bench's synthetic actions.  Eager rows
alternate the four dtypes inside each repetition (all four environments are resident); rollout rows build one
environment at a time (T = 32 output slices of float32 deep_sea boards are 121 GB), in the order f32, u8, f16, bf16 and
back.  Per row: the median over repetitions of ms per step on HIP events and on the wall clock around a synchronize,
env-steps/s, the algorithmic bytes per step (13 + E * obs_numel + 8: bench.algorithmic_bytes_per_step with the
element size E in place of 4) and their share of the 8 TB/s HBM peak.
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

DTYPES = ('float32', 'uint8', 'float16', 'bfloat16')
ELEM = dict(float32=4, uint8=1, float16=2, bfloat16=2)
WORKLOADS = ('deep_sea', 'catch')


def _make(bsuite_amd, torch, workload, dtype, lanes, dev):
  bsuite_id, _, _, _, _, period = bench.WORKLOADS[workload]
  env = bsuite_amd.load_from_id(bsuite_id, batch=lanes, device=dev, seed=42, num_buffers=2, observation_dtype=dtype)
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


def _row(workload, dtype, mode, lanes, T, samples):
  _, _, _, obs_numel, state_bytes, _ = bench.WORKLOADS[workload]
  ev = statistics.median(s[0] for s in samples)
  wall = statistics.median(s[1] for s in samples)
  bps = 13 + ELEM[dtype] * obs_numel + state_bytes
  return bench.sig(dict(workload=workload, bsuite_id=bench.WORKLOADS[workload][0], dtype=dtype, mode=mode, lanes=lanes,
                        T=T if mode == 'rollout' else None, ms_per_step_event=ev, ms_per_step_wall=wall,
                        ms_event_min_max=[min(s[0] for s in samples), max(s[0] for s in samples)],
                        env_steps_per_s=lanes / (wall * 1e-3), algorithmic_bytes_per_step=bps,
                        frac_8tbs=bps * lanes / (ev * 1e-3) / 1e9 / bench.HBM_PEAK_GBPS, reps=len(samples)))


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
    raise SystemExit('bench_obs_dtype.py measures on the GPU; none is visible')
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
      envs = {d: _make(bsuite_amd, torch, w, d, a.lanes, dev) for d in DTYPES}
      runs = {}
      for d, (env, acts) in envs.items():
        runs[d] = (lambda env, acts: lambda n: [env.step(acts[t % acts.shape[0]]) for t in range(n)])(env, acts)
        runs[d](32)                                                # warm-up
      samples = {d: [] for d in DTYPES}
      for rep in range(a.reps):
        for d in (DTYPES if rep % 2 == 0 else DTYPES[::-1]):
          samples[d].append(_time(torch, runs[d], a.steps))
      for d in DTYPES:
        emit(_row(w, d, 'eager', a.lanes, None, samples[d]))
      del envs, runs
      torch.cuda.empty_cache()
    if 'rollout' in a.modes:
      samples = {d: [] for d in DTYPES}
      chunks = max(1, a.steps // a.T)
      for rep in range(a.reps):
        for d in (DTYPES if rep % 2 == 0 else DTYPES[::-1]):
          env, acts = _make(bsuite_amd, torch, w, d, a.lanes, dev)
          roll = acts[:a.T].contiguous()
          run = lambda n, env=env, roll=roll: [env.rollout(roll) for _ in range(n // a.T)]
          run(2 * a.T)                                             # warm-up (allocates the [T, B, ...] outputs)
          samples[d].append(_time(torch, run, chunks * a.T))
          del env, acts, roll, run
          torch.cuda.empty_cache()
      for d in DTYPES:
        emit(_row(w, d, 'rollout', a.lanes, a.T, samples[d]))
  if out:
    out.close()


if __name__ == '__main__':
  main()
