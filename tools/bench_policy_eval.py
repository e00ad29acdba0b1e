"""evaluate_policy against rollout_policy of the same T, one process: deep_sea/10 and catch/0 at 2^20 lanes in index mode,
a seeded random uint8 table, one JSON line per (workload, T, variant).

  python tools/bench_policy_eval.py [--lanes 1048576] [--steps 512] [--T 32,256] [--reps 3] [--variants a,b] [--out FILE]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_policy_eval.py --T 32 --variants eval_greedy,rollout_greedy
  python tools/bench_policy_eval.py --summarize-trace DIR --T 32      # per kernel: dispatches, us per launch and per step

Variants, alternated inside each repetition (each has its own resident environment):
  rollout_greedy / rollout_eps   rollout_policy(table, T[, epsilon]) — writes every TimeStep of every lane;
  eval_greedy / eval_eps         evaluate_policy(table, T[, epsilon]) — the same closed loop, three numbers per lane.
Lanes carry the steady FIRST / MID / LAST mix (bench.stagger_phases).  Per row: every repetition's us per step on HIP
events (`us_event_reps`, in the order measured), their median, and env-steps/s from it.  The last line per (workload, T)
says whether evaluate_policy was faster than rollout_policy in EVERY repetition, greedy and exploring, and gives the
ratio per repetition.  (Both eval variants launch the same kernel: trace them in separate runs, --variants.)
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

VARIANTS = ('rollout_greedy', 'eval_greedy', 'rollout_eps', 'eval_eps')
WORKLOADS = ('deep_sea', 'catch')


def _time(torch, run, steps):
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  ev0.record()
  run(steps)
  ev1.record()
  torch.cuda.synchronize()
  return ev0.elapsed_time(ev1) * 1e3 / steps


def summarize_trace(directory, T):
  """One JSON line per closed-loop kernel of a rocprofv3 kernel trace: its dispatches, us per launch and per step (launch / T)."""
  per = collections.defaultdict(list)
  for f in glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True):
    for r in csv.DictReader(open(f)):
      if 'policy_rollout_kernel' in r['Kernel_Name'] or 'tab_eval_kernel' in r['Kernel_Name']:
        per[r['Kernel_Name'].split('(')[0].replace('void ', '')].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
  for k, v in sorted(per.items()):
    print(json.dumps(bench.sig(dict(kernel=k, dispatches=len(v), us_per_launch_median=statistics.median(v), us_per_launch_min=min(v),
                                    us_per_launch_max=max(v), us_per_step_median=statistics.median(v) / T))))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--steps', type=int, default=512)
  ap.add_argument('--T', default='32,256')
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--epsilon', type=float, default=0.1)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--variants', default=','.join(VARIANTS))
  ap.add_argument('--summarize-trace', default=None, metavar='DIR')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  Ts = [int(t) for t in a.T.split(',')]
  if a.summarize_trace:
    return summarize_trace(a.summarize_trace, Ts[0])
  variants = tuple(v for v in VARIANTS if v in a.variants.split(','))
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_policy_eval.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  out = open(a.out, 'a') if a.out else None

  def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  for w in a.workloads.split(','):
    bsuite_id, _, _, _, _, period = bench.WORKLOADS[w]
    for T in Ts:
      steps = max(1, a.steps // T) * T
      runs = {}
      for v in variants:
        env = bsuite_amd.load_from_id(bsuite_id, batch=a.lanes, device=dev, seed=42, num_buffers=2, observation_mode='index')
        n_act = env.action_spec().num_values
        bench.stagger_phases(env, bench.synthetic_actions(torch, n_act, 64, 0, a.lanes, dev), period)
        g = torch.Generator(device=dev).manual_seed(0)
        table = torch.randint(n_act, (env.policy_num_states,), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
        eps = a.epsilon if v.endswith('_eps') else 0.0
        fn = env.evaluate_policy if v.startswith('eval') else env.rollout_policy
        runs[v] = lambda n, fn=fn, t=table, eps=eps, T=T: [fn(t, T, epsilon=eps, explore_seed=7) for _ in range(n // T)]
        runs[v](2 * T)                                               # warm-up (allocates the outputs)
      samples = {v: [] for v in variants}
      for rep in range(a.reps):
        for v in (variants if rep % 2 == 0 else variants[::-1]):
          samples[v].append(_time(torch, runs[v], steps))
      for v in variants:
        us = statistics.median(samples[v])
        emit(bench.sig(dict(workload=w, bsuite_id=bsuite_id, variant=v, lanes=a.lanes, T=T, steps=steps, us_per_step_event=us,
                            us_event_reps=samples[v], env_steps_per_s=a.lanes / (us * 1e-6), reps=a.reps,
                            epsilon=a.epsilon if v.endswith('_eps') else 0.0)))
      if variants == VARIANTS:
        ratio = lambda k: [r / e for e, r in zip(samples['eval_' + k], samples['rollout_' + k])]      # noqa: E731
        emit(bench.sig(dict(workload=w, T=T,
                            eval_faster_than_rollout_in_every_rep=all(x > 1.0 for x in ratio('greedy') + ratio('eps')),
                            rollout_over_eval_greedy_reps=ratio('greedy'), rollout_over_eval_eps_reps=ratio('eps'))))
      del runs
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
