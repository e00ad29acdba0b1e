"""rollout_linear / rollout_mlp against what a trajectory cost before them and against their two neighbours — one process:
cartpole, cartpole_swingup and mountain_car at 2^20 lanes, T = 32, one JSON line per (workload, policy, exploration, variant).

  python tools/bench_trajectory.py [--lanes 1048576] [--T 32] [--steps 256] [--eager-steps 32] [--reps 3] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_trajectory.py --variants fused --reps 1
  python tools/bench_trajectory.py --summarize-trace DIR           # the kernel: dispatches, us per launch and per step

Policies: `linear` (one matrix), `mlp16` (one H = 16 pair), `pop16` (a population of --population H = 16 pairs, policy_index =
lane * P // B: the lanes of a wave name one pair); each greedy and with --epsilon.
Variants, alternated inside each repetition (each has its own resident environment, warmed up past its first resets):
  eager       (a) obs -> select(obs) [-> where(rand < epsilon, randint, a)] -> step(a), step by step: how a trajectory was
              recorded under such a policy before this call (the TimeSteps are what step() returns);
  open_loop   (b) rollout(actions) with a [T,B] action tensor made beforehand: the trajectory without the decision;
  evaluate    (c) evaluate_linear / evaluate_mlp with the same arguments: the decision without the trajectory;
  fused       (d) rollout_linear / rollout_mlp, the last observation passed back in.
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median and env-steps/s;
then per case eager / fused, fused / open_loop and fused / evaluate per repetition.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import bench_linear_eval as ble  # noqa: E402
import bench_mlp_eval as bme  # noqa: E402

WORKLOADS = ble.WORKLOADS
KERNEL = 'bsx_trajectory_kernel'
HIDDEN = 16


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--eager-steps', type=int, default=32)
  ap.add_argument('--population', type=int, default=1024)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--epsilon', type=float, default=0.1)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--policies', default='linear,mlp16,pop16')
  ap.add_argument('--variants', default='eager,open_loop,evaluate,fused')
  ap.add_argument('--summarize-trace', default=None, metavar='DIR')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  T = a.T
  if a.summarize_trace:
    ble.KERNEL = KERNEL
    return ble.summarize_trace(a.summarize_trace, T)
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_trajectory.py measures on the GPU; none is visible')
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
  n_fused = max(1, a.steps // T) * T
  for w in a.workloads.split(','):
    for policy in a.policies.split(','):
      P = a.population if policy == 'pop16' else 1
      pidx = (torch.arange(B, device=dev, dtype=torch.int64) * P // B).to(torch.int32) if P > 1 else None
      for eps in (0.0, a.epsilon):
        runs, steps_of = {}, {}

        def fresh():
          env = bsuite_amd.load_from_id(WORKLOADS[w], batch=B, device=dev, seed=42)
          D = env.observation_spec().shape[-1]
          if policy == 'linear':
            pol = (ble.make_weights(torch, w, D, 1, dev)[0].contiguous(),)
          else:
            w1, w2 = bme.make_pairs(torch, w, D, HIDDEN, P, dev)
            pol = (w1[0].contiguous(), w2[0].contiguous()) if P == 1 else (w1, w2)
          return env, pol

        kw = dict(policy_index=pidx, epsilon=eps, explore_seed=7)
        if 'eager' in kinds:
          env, pol = fresh()
          # (a lane's own pair, gathered once: the eager loop is not charged for the gather)
          own = pol if P == 1 else tuple(t[pidx.long()] for t in pol)
          select = observations.linear_select if policy == 'linear' else observations.mlp_select
          state = dict(obs=env.reset().observation)
          g = torch.Generator(device=dev).manual_seed(1)

          def eager(n, env=env, own=own, select=select, state=state, g=g, eps=eps):
            obs = state['obs']
            for _ in range(n):
              act = select(*own, obs)
              if eps > 0.0:
                explore = torch.rand(B, generator=g, device=dev) < eps
                act = torch.where(explore, torch.randint(3, (B,), generator=g, device=dev, dtype=torch.int32), act)
              obs = env.step(act).observation
            state['obs'] = obs

          runs['eager'], steps_of['eager'] = eager, a.eager_steps
          eager(4)
        if 'open_loop' in kinds:
          env, _ = fresh()
          acts = torch.randint(3, (T, B), generator=torch.Generator(device=dev).manual_seed(2), device=dev, dtype=torch.int32)

          def open_loop(n, env=env, acts=acts):
            for _ in range(n // T):
              env.rollout(acts)

          runs['open_loop'], steps_of['open_loop'] = open_loop, n_fused
          open_loop(2 * T)
        for name in ('evaluate', 'fused'):
          if name not in kinds:
            continue
          env, pol = fresh()
          method = ('evaluate_' if name == 'evaluate' else 'rollout_') + ('linear' if policy == 'linear' else 'mlp')
          state = dict(obs=env.reset().observation.clone())

          def closed(n, call=getattr(env, method), pol=pol, state=state, name=name, kw=kw):
            obs = state['obs']
            for _ in range(n // T):
              r = call(*pol, obs, T, **kw)
              obs = r.observation if name == 'evaluate' else r[0].observation[-1]
            state['obs'] = obs

          runs[name], steps_of[name] = closed, n_fused
          closed(2 * T)                                                    # warm-up (allocates the outputs)
        order = tuple(runs)
        samples = {v: [] for v in order}
        for rep in range(a.reps):
          for v in (order if rep % 2 == 0 else order[::-1]):
            samples[v].append(ble._time(torch, runs[v], steps_of[v]))       # pylint: disable=protected-access
        case = dict(workload=w, policy=policy, epsilon=eps, T=T)
        for v in order:
          us = statistics.median(samples[v])
          emit(bench.sig(dict(case, bsuite_id=WORKLOADS[w], population=P, variant=v, lanes=B, steps=steps_of[v], us_per_step_event=us,
                              us_event_reps=samples[v], env_steps_per_s=B / (us * 1e-6), reps=a.reps)))
        if 'fused' in runs:
          for other, key in (('eager', 'eager_over_fused_reps'), ('open_loop', 'fused_over_open_loop_reps'),
                             ('evaluate', 'fused_over_evaluate_reps')):
            if other in runs:
              ratio = [(o / f if other == 'eager' else f / o) for o, f in zip(samples[other], samples['fused'])]
              emit(bench.sig(dict(case, variant='fused', **{key: ratio})))
        del runs
        torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
