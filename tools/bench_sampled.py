"""sample_linear / sample_mlp against the eager loop they replace and against the greedy recording call — one process:
cartpole, cartpole_swingup and mountain_car at 2^20 lanes, T = 32, one JSON line per (workload, policy, variant).

  python tools/bench_sampled.py [--lanes 1048576] [--T 32] [--steps 256] [--eager-steps 32] [--reps 3] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_sampled.py --variants fused --reps 1
  python tools/bench_sampled.py --summarize-trace DIR           # the kernel: dispatches, us per launch and per step

Policies: `linear` (one matrix), `mlp16` (one H = 16 pair), `pop16` (a population of --population H = 16 pairs, policy_index =
lane * P // B: the lanes of a wave name one pair); temperature --temperature.
Variants, alternated inside each repetition (each has its own resident environment, warmed up past its first resets):
  eager    obs -> logits(obs) -> gumbel_select(logits, words, temperature) -> step(a), step by step: how a softmax agent's
           trajectory was recorded before this call.  The words are torch.randint on the device, not the counter stream (a
           restatement of Philox in torch would only make the loop slower): the loop is charged for one [B, 3] draw per step;
  greedy   rollout_linear / rollout_mlp with the same policy, epsilon = 0: the recording call without the sampling;
  fused    sample_linear / sample_mlp, the last observation passed back in.
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median and env-steps/s;
then per case eager / fused and fused / greedy per repetition.
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
KERNEL = 'bsx_gumbel_kernel'
HIDDEN = 16


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--eager-steps', type=int, default=32)
  ap.add_argument('--population', type=int, default=1024)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--temperature', type=float, default=1.0)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--policies', default='linear,mlp16,pop16')
  ap.add_argument('--variants', default='eager,greedy,fused')
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
    raise SystemExit('bench_sampled.py measures on the GPU; none is visible')
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

      if 'eager' in kinds:
        env, pol = fresh()
        # (a lane's own pair, gathered once: the eager loop is not charged for the gather)
        own = pol if P == 1 else tuple(t[pidx.long()] for t in pol)
        logits_of = observations.linear_logits if policy == 'linear' else observations.mlp_logits
        state = dict(obs=env.reset().observation)
        g = torch.Generator(device=dev).manual_seed(1)

        def eager(n, env=env, own=own, logits_of=logits_of, state=state, g=g):
          obs = state['obs']
          for _ in range(n):
            words = torch.randint(1 << 32, (B, 3), generator=g, device=dev, dtype=torch.int64)
            obs = env.step(observations.gumbel_select(logits_of(*own, obs), words, a.temperature)).observation
          state['obs'] = obs

        runs['eager'], steps_of['eager'] = eager, a.eager_steps
        eager(4)
      for name in ('greedy', 'fused'):
        if name not in kinds:
          continue
        env, pol = fresh()
        method = ('rollout_' if name == 'greedy' else 'sample_') + ('linear' if policy == 'linear' else 'mlp')
        kw = dict(policy_index=pidx)
        kw.update(dict(epsilon=0.0) if name == 'greedy' else dict(temperature=a.temperature, sample_seed=7))
        state = dict(obs=env.reset().observation.clone())

        def closed(n, call=getattr(env, method), pol=pol, state=state, kw=kw):
          obs = state['obs']
          for _ in range(n // T):
            obs = call(*pol, obs, T, **kw)[0].observation[-1]
          state['obs'] = obs

        runs[name], steps_of[name] = closed, n_fused
        closed(2 * T)                                                      # warm-up (allocates the outputs)
      order = tuple(runs)
      samples = {v: [] for v in order}
      for rep in range(a.reps):
        for v in (order if rep % 2 == 0 else order[::-1]):
          samples[v].append(ble._time(torch, runs[v], steps_of[v]))         # pylint: disable=protected-access
      case = dict(workload=w, policy=policy, temperature=a.temperature, T=T)
      for v in order:
        us = statistics.median(samples[v])
        emit(bench.sig(dict(case, bsuite_id=WORKLOADS[w], population=P, variant=v, lanes=B, steps=steps_of[v], us_per_step_event=us,
                            us_event_reps=samples[v], env_steps_per_s=B / (us * 1e-6), reps=a.reps)))
      if 'fused' in runs:
        for other, key in (('eager', 'eager_over_fused_reps'), ('greedy', 'fused_over_greedy_reps')):
          if other in runs:
            ratio = [(o / f if other == 'eager' else f / o) for o, f in zip(samples[other], samples['fused'])]
            emit(bench.sig(dict(case, variant='fused', **{key: ratio})))
      del runs
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
