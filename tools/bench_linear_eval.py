"""evaluate_linear against the eager loop it replaces (step + utils.observations.linear_select), one process: cartpole,
cartpole_swingup and mountain_car at 2^20 lanes, one JSON line per (workload, matrices, exploration, variant).

  python tools/bench_linear_eval.py [--lanes 1048576] [--steps 512] [--eager-steps 64] [--T 32,256] [--reps 3] [--out FILE]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_linear_eval.py --T 32 --variants fused --reps 1
  python tools/bench_linear_eval.py --summarize-trace DIR --T 32      # the kernel: dispatches, us per launch and per step

Variants, alternated inside each repetition (each has its own resident environment, warmed up past its first resets):
  eager       obs -> linear_select(weights, obs) [-> where(rand < epsilon, randint, a)] -> step(a), step by step;
  fused_T     evaluate_linear(weights, obs, T[, epsilon]) with the returned observation passed back in.
Matrices: `shared` (one [3, D+1] matrix) or `per_lane` (a population of B, policy_index = the lane).  The weights make
all three actions occur (a signed feature of the row decides), so episodes end at the rate a non-trivial agent sees.
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median, and
env-steps/s from it; the last line per case gives eager / fused per repetition.
"""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

WORKLOADS = dict(cartpole='cartpole/0', cartpole_swingup='cartpole_swingup/0', mountain_car='mountain_car/0')
KERNEL = 'bsx_linear_score_kernel'


def _time(torch, run, steps):
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  ev0.record()
  run(steps)
  ev1.record()
  torch.cuda.synchronize()
  return ev0.elapsed_time(ev1) * 1e3 / steps


def make_weights(torch, workload, D, P, dev, seed=0):
  """[P, 3, D+1]: l_0 = -k s, l_1 = a bias, l_2 = +k s with s a signed feature of the row (cartpole: sin(theta) and
  theta_dot, mountain_car: position + 0.5 and velocity), plus small random terms; k differs from row to row."""
  g = torch.Generator(device=dev).manual_seed(seed)
  w = torch.randn((P, 3, D + 1), generator=g, device=dev) * 0.05
  k = 20.0 * (1.0 + 0.5 * torch.rand((P,), generator=g, device=dev))
  if workload == 'mountain_car':
    w[:, 0, 0] -= k; w[:, 2, 0] += k
    w[:, 0, D] -= 0.5 * k; w[:, 2, D] += 0.5 * k
    w[:, 0, 1] -= 200.0; w[:, 2, 1] += 200.0
  else:
    w[:, 0, 2] -= k; w[:, 2, 2] += k
    w[:, 0, 4] -= 0.3 * k; w[:, 2, 4] += 0.3 * k
  w[:, 1, D] += 0.4
  return w.contiguous()


def summarize_trace(directory, T):
  """One JSON line for the kernel of a rocprofv3 kernel trace: its dispatches, us per launch and per step (launch / T)."""
  per = collections.defaultdict(list)
  for f in glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True):
    for r in csv.DictReader(open(f)):
      if KERNEL in r['Kernel_Name']:
        per[r['Kernel_Name'].split('(')[0].replace('void ', '')].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
  for k, v in sorted(per.items()):
    print(json.dumps(bench.sig(dict(kernel=k, dispatches=len(v), us_per_launch_median=statistics.median(v), us_per_launch_min=min(v),
                                    us_per_launch_max=max(v), us_per_step_median=statistics.median(v) / T))))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--steps', type=int, default=512)
  ap.add_argument('--eager-steps', type=int, default=64)
  ap.add_argument('--T', default='32,256')
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--epsilon', type=float, default=0.1)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--matrices', default='shared,per_lane')
  ap.add_argument('--variants', default='eager,fused')
  ap.add_argument('--summarize-trace', default=None, metavar='DIR')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  Ts = [int(t) for t in a.T.split(',')]
  if a.summarize_trace:
    return summarize_trace(a.summarize_trace, Ts[0])
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_linear_eval.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  out = open(a.out, 'a') if a.out else None
  kinds = a.variants.split(',')

  def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  B = a.lanes
  for w in a.workloads.split(','):
    for matrices in a.matrices.split(','):
      for eps in (0.0, a.epsilon):
        runs, steps_of = {}, {}
        lanes = torch.arange(B, device=dev, dtype=torch.int32)

        def fresh():
          env = bsuite_amd.load_from_id(WORKLOADS[w], batch=B, device=dev, seed=42)
          D = env.observation_spec().shape[-1]
          P = 1 if matrices == 'shared' else B
          weights = make_weights(torch, w, D, P, dev)
          return env, (weights[0].contiguous() if P == 1 else weights), (None if P == 1 else lanes)

        if 'eager' in kinds:
          env, weights, _ = fresh()
          state = dict(obs=env.reset().observation)
          g = torch.Generator(device=dev).manual_seed(1)

          def eager(n, env=env, weights=weights, state=state, g=g, eps=eps):
            obs = state['obs']
            for _ in range(n):
              act = observations.linear_select(weights, obs)
              if eps > 0.0:
                explore = torch.rand(B, generator=g, device=dev) < eps
                act = torch.where(explore, torch.randint(3, (B,), generator=g, device=dev, dtype=torch.int32), act)
              obs = env.step(act).observation
            state['obs'] = obs

          runs['eager'], steps_of['eager'] = eager, a.eager_steps
          eager(8)
        if 'fused' in kinds:
          for T in Ts:
            env, weights, pidx = fresh()
            state = dict(obs=env.reset().observation.clone())

            def fused(n, env=env, weights=weights, pidx=pidx, state=state, T=T, eps=eps):
              obs = state['obs']
              for _ in range(n // T):
                obs = env.evaluate_linear(weights, obs, T, policy_index=pidx, epsilon=eps, explore_seed=7).observation
              state['obs'] = obs

            runs[f'fused_{T}'], steps_of[f'fused_{T}'] = fused, max(1, a.steps // T) * T
            fused(2 * T)                                               # warm-up (allocates the outputs)
        order = tuple(runs)
        samples = {v: [] for v in order}
        for rep in range(a.reps):
          for v in (order if rep % 2 == 0 else order[::-1]):
            samples[v].append(_time(torch, runs[v], steps_of[v]))
        for v in order:
          us = statistics.median(samples[v])
          emit(bench.sig(dict(workload=w, bsuite_id=WORKLOADS[w], matrices=matrices, epsilon=eps, variant=v, lanes=B, steps=steps_of[v],
                              us_per_step_event=us, us_event_reps=samples[v], env_steps_per_s=B / (us * 1e-6), reps=a.reps)))
        if 'eager' in runs:
          for v in order:
            if v != 'eager':
              emit(bench.sig(dict(workload=w, matrices=matrices, epsilon=eps, variant=v,
                                  eager_over_fused_reps=[e / f for e, f in zip(samples['eager'], samples[v])])))
        del runs
        torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
