"""evaluate_mlp against the eager loop it replaces (step + utils.observations.mlp_select) and against evaluate_linear, the floor a
hidden layer is added to — one process: cartpole, cartpole_swingup and mountain_car at 2^20 lanes, one JSON line per
(workload, hidden width, weights, exploration, variant).

  python tools/bench_mlp_eval.py [--lanes 1048576] [--steps 512] [--eager-steps 32] [--T 32,256] [--hidden 16,64] [--reps 3] [--out FILE]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_mlp_eval.py --T 32 --variants fused --reps 1
  python tools/bench_mlp_eval.py --summarize-trace DIR --T 32      # the kernel: dispatches, us per launch and per step

Variants, alternated inside each repetition (each has its own resident environment, warmed up past its first resets):
  eager       obs -> mlp_select(w1, w2, obs) [-> where(rand < epsilon, randint, a)] -> step(a), step by step;
  fused_T     evaluate_mlp(w1, w2, obs, T[, epsilon]) with the returned observation passed back in;
  linear_T    evaluate_linear(weights, obs, T[, epsilon]) on the same workload with the same layout of policy_index.
Weights: `shared` (one pair), `grouped` (a population of --population pairs, policy_index = lane * P // B: the lanes of a wave
name one pair) or `shuffled` (the same population, policy_index permuted: a wave names up to 64 pairs).  The pairs make all
three actions occur and switch hidden units on and off (a signed feature of the row decides).
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median, and
env-steps/s from it; the last lines per case give eager / fused and fused / linear per repetition.
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

WORKLOADS = ble.WORKLOADS
KERNEL = 'bsx_mlp_returns_kernel'


def make_pairs(torch, workload, D, H, P, dev, seed=0):
  """w1 [P, H, D+1], w2 [P, 3, H+1]: unit j sees +k s (j even) or -k s (j odd) of a signed feature s of the row (cartpole:
  sin(theta) and theta_dot, mountain_car: position + 0.5 and velocity); l_0 = 0.3, l_1 = the mean of the units, l_2 = twice
  that - 1; plus small random terms; k differs from pair to pair."""
  g = torch.Generator(device=dev).manual_seed(seed)
  w1 = torch.randn((P, H, D + 1), generator=g, device=dev) * 0.02
  w2 = torch.randn((P, 3, H + 1), generator=g, device=dev) * 0.02
  k = 20.0 * (1.0 + 0.5 * torch.rand((P, 1), generator=g, device=dev))
  sign = torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(H)], device=dev).unsqueeze(0)
  if workload == 'mountain_car':
    w1[:, :, 0] += k * sign; w1[:, :, D] += 0.5 * k * sign; w1[:, :, 1] += 10.0 * k * sign
  else:
    w1[:, :, 2] += k * sign; w1[:, :, 4] += 0.3 * k * sign
  share = torch.tensor([1.0 / len(range(j % 2, H, 2)) for j in range(H)], device=dev).unsqueeze(0)
  w2[:, 0, H] += 0.3
  w2[:, 1, :H] += share
  w2[:, 2, :H] += 2.0 * share
  w2[:, 2, H] -= 1.0
  return w1.contiguous(), w2.contiguous()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--steps', type=int, default=512)
  ap.add_argument('--eager-steps', type=int, default=32)
  ap.add_argument('--T', default='32,256')
  ap.add_argument('--hidden', default='16,64')
  ap.add_argument('--population', type=int, default=1024)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--epsilon', type=float, default=0.1)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--weights', default='shared,grouped,shuffled')
  ap.add_argument('--variants', default='eager,fused,linear')
  ap.add_argument('--summarize-trace', default=None, metavar='DIR')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  Ts = [int(t) for t in a.T.split(',')]
  if a.summarize_trace:
    ble.KERNEL = KERNEL
    return ble.summarize_trace(a.summarize_trace, Ts[0])
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_mlp_eval.py measures on the GPU; none is visible')
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
    for H in (int(h) for h in a.hidden.split(',')):
      for layout in a.weights.split(','):
        P = 1 if layout == 'shared' else a.population
        pidx = None
        if P > 1:
          pidx = (torch.arange(B, device=dev, dtype=torch.int64) * P // B).to(torch.int32)
          if layout == 'shuffled':
            pidx = pidx[torch.randperm(B, generator=torch.Generator(device=dev).manual_seed(5), device=dev)].contiguous()
        for eps in (0.0, a.epsilon):
          runs, steps_of = {}, {}

          def fresh():
            env = bsuite_amd.load_from_id(WORKLOADS[w], batch=B, device=dev, seed=42)
            return env, env.observation_spec().shape[-1]

          if 'eager' in kinds:
            env, D = fresh()
            w1, w2 = make_pairs(torch, w, D, H, P, dev)
            # (a lane's own pair, gathered once: the eager loop is not charged for the gather)
            e1, e2 = (w1[0], w2[0]) if P == 1 else (w1[pidx.long()], w2[pidx.long()])
            state = dict(obs=env.reset().observation)
            g = torch.Generator(device=dev).manual_seed(1)

            def eager(n, env=env, e1=e1, e2=e2, state=state, g=g, eps=eps):
              obs = state['obs']
              for _ in range(n):
                act = observations.mlp_select(e1, e2, obs)
                if eps > 0.0:
                  explore = torch.rand(B, generator=g, device=dev) < eps
                  act = torch.where(explore, torch.randint(3, (B,), generator=g, device=dev, dtype=torch.int32), act)
                obs = env.step(act).observation
              state['obs'] = obs

            runs['eager'], steps_of['eager'] = eager, a.eager_steps
            eager(4)
          for T in Ts:
            if 'fused' in kinds:
              env, D = fresh()
              w1, w2 = make_pairs(torch, w, D, H, P, dev)
              if P == 1:
                w1, w2 = w1[0].contiguous(), w2[0].contiguous()
              state = dict(obs=env.reset().observation.clone())

              def fused(n, env=env, w1=w1, w2=w2, state=state, T=T, eps=eps):
                obs = state['obs']
                for _ in range(n // T):
                  obs = env.evaluate_mlp(w1, w2, obs, T, policy_index=pidx, epsilon=eps, explore_seed=7).observation
                state['obs'] = obs

              runs[f'fused_{T}'], steps_of[f'fused_{T}'] = fused, max(1, a.steps // T) * T
              fused(2 * T)                                               # warm-up (allocates the outputs)
            if 'linear' in kinds:
              env, D = fresh()
              lw = ble.make_weights(torch, w, D, P, dev)
              if P == 1:
                lw = lw[0].contiguous()
              state = dict(obs=env.reset().observation.clone())

              def linear(n, env=env, lw=lw, state=state, T=T, eps=eps):
                obs = state['obs']
                for _ in range(n // T):
                  obs = env.evaluate_linear(lw, obs, T, policy_index=pidx, epsilon=eps, explore_seed=7).observation
                state['obs'] = obs

              runs[f'linear_{T}'], steps_of[f'linear_{T}'] = linear, max(1, a.steps // T) * T
              linear(2 * T)
          order = tuple(runs)
          samples = {v: [] for v in order}
          for rep in range(a.reps):
            for v in (order if rep % 2 == 0 else order[::-1]):
              samples[v].append(ble._time(torch, runs[v], steps_of[v]))     # pylint: disable=protected-access
          case = dict(workload=w, hidden=H, weights=layout, epsilon=eps)
          for v in order:
            us = statistics.median(samples[v])
            emit(bench.sig(dict(case, bsuite_id=WORKLOADS[w], population=P, variant=v, lanes=B, steps=steps_of[v], us_per_step_event=us,
                                us_event_reps=samples[v], env_steps_per_s=B / (us * 1e-6), reps=a.reps)))
          for v in order:
            if v.startswith('fused') and 'eager' in runs:
              emit(bench.sig(dict(case, variant=v, eager_over_fused_reps=[e / f for e, f in zip(samples['eager'], samples[v])])))
            if v.startswith('fused') and v.replace('fused', 'linear') in runs:
              emit(bench.sig(dict(case, variant=v, fused_over_linear_reps=[f / l for f, l in
                                                                           zip(samples[v], samples[v.replace('fused', 'linear')])])))
          del runs
          torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
