"""evaluate_sampled_linear / evaluate_sampled_mlp against the recording call they spare and against the greedy evaluation — one
process: cartpole, cartpole_swingup and mountain_car at 2^20 lanes, T = 32, one JSON line per (workload, policy, variant).

  python tools/bench_sampled_eval.py [--lanes 1048576] [--T 32] [--steps 256] [--reps 3] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_sampled_eval.py --variants fused --reps 1
  python tools/bench_sampled_eval.py --summarize-trace DIR      # the kernel: dispatches, us per launch and per step

The timing method is tools/bench_sampled.py's.  Policies: `linear` (one matrix), `mlp16` (one H = 16 pair), `pop16` (a
population of --population H = 16 pairs, policy_index = lane * P // B: the lanes of a wave name one pair); temperature
--temperature.  Variants, alternated inside each repetition (each has its own resident environment, warmed up past its first
resets):
  recorded  sample_linear / sample_mlp, the last observation passed back in: what a caller who wants only the returns of a
            softmax policy had to launch before this call (the host-side reduction of its [T,B] slabs is not charged);
  greedy    evaluate_linear / evaluate_mlp with the same policy, epsilon = 0: the returns-only call without the sampling;
  fused     evaluate_sampled_linear / evaluate_sampled_mlp with the arguments of `recorded`.
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median and env-steps/s;
then per case fused / recorded in env-steps/s per repetition (the bar: >= 0.95 at every shape) and fused / greedy in us.
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
KERNEL = 'bsx_drawn_returns_kernel'
HIDDEN = 16
METHOD = dict(recorded='sample_', greedy='evaluate_', fused='evaluate_sampled_')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--population', type=int, default=1024)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--temperature', type=float, default=1.0)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--policies', default='linear,mlp16,pop16')
  ap.add_argument('--variants', default='recorded,greedy,fused')
  ap.add_argument('--summarize-trace', default=None, metavar='DIR')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  T = a.T
  if a.summarize_trace:
    ble.KERNEL = KERNEL
    return ble.summarize_trace(a.summarize_trace, T)
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_sampled_eval.py measures on the GPU; none is visible')
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
      runs = {}

      def fresh():
        env = bsuite_amd.load_from_id(WORKLOADS[w], batch=B, device=dev, seed=42)
        D = env.observation_spec().shape[-1]
        if policy == 'linear':
          pol = (ble.make_weights(torch, w, D, 1, dev)[0].contiguous(),)
        else:
          w1, w2 = bme.make_pairs(torch, w, D, HIDDEN, P, dev)
          pol = (w1[0].contiguous(), w2[0].contiguous()) if P == 1 else (w1, w2)
        return env, pol

      for name in ('recorded', 'greedy', 'fused'):
        if name not in kinds:
          continue
        env, pol = fresh()
        method = METHOD[name] + ('linear' if policy == 'linear' else 'mlp')
        kw = dict(policy_index=pidx)
        kw.update(dict(epsilon=0.0) if name == 'greedy' else dict(temperature=a.temperature, sample_seed=7))
        state = dict(obs=env.reset().observation.clone())
        # the next call's input: the last slab of a recording call, the result's row of a returns-only call
        last = (lambda r: r[0].observation[-1]) if name == 'recorded' else (lambda r: r.observation)

        def closed(n, call=getattr(env, method), pol=pol, state=state, kw=kw, last=last):
          obs = state['obs']
          for _ in range(n // T):
            obs = last(call(*pol, obs, T, **kw))
          state['obs'] = obs

        runs[name] = closed
        closed(2 * T)                                                      # warm-up (allocates the outputs)
      order = tuple(runs)
      samples = {v: [] for v in order}
      for rep in range(a.reps):
        for v in (order if rep % 2 == 0 else order[::-1]):
          samples[v].append(ble._time(torch, runs[v], n_fused))             # pylint: disable=protected-access
      case = dict(workload=w, policy=policy, temperature=a.temperature, T=T)
      for v in order:
        us = statistics.median(samples[v])
        emit(bench.sig(dict(case, bsuite_id=WORKLOADS[w], population=P, variant=v, lanes=B, steps=n_fused, us_per_step_event=us,
                            us_event_reps=samples[v], env_steps_per_s=B / (us * 1e-6), reps=a.reps)))
      if 'fused' in runs:
        if 'recorded' in runs:   # env-steps/s of the new call over the recording call's: us(recorded) / us(fused)
          ratio = [r / f for r, f in zip(samples['recorded'], samples['fused'])]
          emit(bench.sig(dict(case, variant='fused', fused_over_recorded_steps_per_s_reps=ratio,
                              fused_over_recorded_steps_per_s=statistics.median(samples['recorded']) / statistics.median(samples['fused']))))
        if 'greedy' in runs:     # what the float64 Gumbel scores cost: us(fused) / us(greedy)
          emit(bench.sig(dict(case, variant='fused', fused_over_greedy_us_reps=[f / g for f, g in zip(samples['fused'], samples['greedy'])])))
      del runs
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
