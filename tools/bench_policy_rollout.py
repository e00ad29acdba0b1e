"""rollout_policy against the open-loop rollout and the eager closed loop, one process: deep_sea/10 and catch/0 at 2^20
lanes in index mode, a seeded random uint8 table, one JSON line per (workload, variant).

  python tools/bench_policy_rollout.py [--lanes 1048576] [--steps 256] [--T 32] [--reps 3] [--variants a,b] [--out FILE]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_policy_rollout.py --variants open_loop,fused_greedy
  python tools/bench_policy_rollout.py --summarize-trace DIR [--T 32]      # per kernel: dispatches, us per launch and per step

Variants, alternated inside each repetition (all four environments are resident: index mode is 25-29 bytes per lane-step):
  open_loop      rollout(T) with pre-generated actions [T,B] — bsx_index_rollout_kernel, the yardstick the fused closed
                 loop is held against (it only exists when the actions do not depend on the observations);
  eager_loop     the closed loop in torch: step(table[policy_key(observation)]) — one launch per step plus the gather;
  fused_greedy   rollout_policy(table, T);
  fused_eps      rollout_policy(table, T, epsilon=0.1).
Lanes carry the steady FIRST / MID / LAST mix (bench.stagger_phases).  Per row: every repetition's us per step on HIP
events (`us_event_reps`, in the order measured), their median, and env-steps/s from it.  The last line per workload says
whether fused_greedy beat eager_loop in EVERY repetition and gives fused_greedy / open_loop per repetition.
(fused_greedy and fused_eps launch the same kernel: trace them in separate runs, --variants.)
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

VARIANTS = ('open_loop', 'eager_loop', 'fused_greedy', 'fused_eps')
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
  """One JSON line per rollout kernel of a rocprofv3 kernel trace: its dispatches, us per launch and per step (launch / T)."""
  per = collections.defaultdict(list)
  for f in glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True):
    for r in csv.DictReader(open(f)):
      if 'rollout_kernel' in r['Kernel_Name']:
        per[r['Kernel_Name'].split('(')[0].replace('void ', '')].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
  for k, v in sorted(per.items()):
    print(json.dumps(bench.sig(dict(kernel=k, dispatches=len(v), us_per_launch_median=statistics.median(v), us_per_launch_min=min(v),
                                    us_per_launch_max=max(v), us_per_step_median=statistics.median(v) / T))))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--epsilon', type=float, default=0.1)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--variants', default=','.join(VARIANTS))
  ap.add_argument('--summarize-trace', default=None, metavar='DIR')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  if a.summarize_trace:
    return summarize_trace(a.summarize_trace, a.T)
  variants = tuple(v for v in VARIANTS if v in a.variants.split(','))
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_policy_rollout.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  out = open(a.out, 'a') if a.out else None

  def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  steps = max(1, a.steps // a.T) * a.T
  for w in a.workloads.split(','):
    bsuite_id, _, _, _, _, period = bench.WORKLOADS[w]
    runs = {}
    for v in variants:
      env = bsuite_amd.load_from_id(bsuite_id, batch=a.lanes, device=dev, seed=42, num_buffers=2, observation_mode='index')
      n_act = env.action_spec().num_values
      actions = bench.synthetic_actions(torch, n_act, 64, 0, a.lanes, dev)
      bench.stagger_phases(env, actions, period)
      g = torch.Generator(device=dev).manual_seed(0)
      table = torch.randint(n_act, (env.policy_num_states,), generator=g, device=dev, dtype=torch.int32)
      table_u8 = table.to(torch.uint8)
      if v == 'open_loop':
        roll = actions[:a.T].contiguous()
        runs[v] = lambda n, env=env, roll=roll: [env.rollout(roll) for _ in range(n // a.T)]
      elif v == 'eager_loop':
        def run(n, env=env, table=table, shape=env.board_shape, acts=actions):
          ts = env.step(acts[0])
          for _ in range(n - 1):
            ts = env.step(table[observations.policy_key(ts.observation, shape).clamp_(min=0)])
        runs[v] = run
      else:
        eps = a.epsilon if v == 'fused_eps' else 0.0
        runs[v] = lambda n, env=env, t=table_u8, eps=eps: [env.rollout_policy(t, a.T, epsilon=eps, explore_seed=7) for _ in range(n // a.T)]
      runs[v](2 * a.T)                                               # warm-up (allocates the [T, B, ...] outputs)
    samples = {v: [] for v in variants}
    for rep in range(a.reps):
      for v in (variants if rep % 2 == 0 else variants[::-1]):
        samples[v].append(_time(torch, runs[v], steps))
    for v in variants:
      us = statistics.median(samples[v])
      emit(bench.sig(dict(workload=w, bsuite_id=bsuite_id, variant=v, lanes=a.lanes, T=a.T, steps=steps, us_per_step_event=us,
                          us_event_reps=samples[v], env_steps_per_s=a.lanes / (us * 1e-6), reps=a.reps,
                          epsilon=a.epsilon if v == 'fused_eps' else 0.0)))
    if variants == VARIANTS:
      emit(bench.sig(dict(workload=w, fused_faster_than_eager_in_every_rep=all(c < b for c, b in zip(samples['fused_greedy'], samples['eager_loop'])),
                          eager_over_fused_reps=[b / c for c, b in zip(samples['fused_greedy'], samples['eager_loop'])],
                          fused_over_open_loop_reps=[c / o for c, o in zip(samples['fused_greedy'], samples['open_loop'])],
                          fused_eps_over_open_loop_reps=[c / o for c, o in zip(samples['fused_eps'], samples['open_loop'])])))
    del runs
    torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
