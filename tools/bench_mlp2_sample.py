"""sample_mlp2 / evaluate_sampled_mlp2 against the only way the policy ran before them, and against the greedy calls of the
same shapes — one process: cartpole, cartpole_swingup and mountain_car at 2^20 lanes, T = 32, one JSON line per (workload,
policy, variant).  In the manner of tools/bench_mlp2.py (whose shapes and triples these are) and tools/bench_sampled.py.

  python tools/bench_mlp2_sample.py [--lanes 1048576] [--T 32] [--steps 256] [--eager-steps 32] [--reps 3] [--out FILE]

Policies: `s64` (one shared 64 x 64 triple), `s16` (one shared 16 x 16 triple), `pop16` (a population of --population
16 x 16 triples, policy_index = lane * P // B: the lanes of a wave name one triple); temperature --temperature.
Variants, alternated inside each repetition (each has its own resident environment, warmed up past its first resets):
  eager            obs -> mlp2_logits(obs) -> gumbel_select(logits, words, temperature) -> step(a), step by step: how this
                   policy ran before these calls (the yardstick; it runs none of the new code).  The words are torch.randint
                   on the device, not the counter stream (a restatement of Philox in torch would only make the loop slower):
                   the loop is charged for one [B, 3] draw per step;
  sample           sample_mlp2, the last observation passed back in;
  sample_evaluate  evaluate_sampled_mlp2 with the same arguments;
  greedy           rollout_mlp2 with the same triple, epsilon = 0: the recording call without the draw;
  greedy_evaluate  evaluate_mlp2 with the same triple, epsilon = 0.
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median, env-steps/s,
and for the fused calls the fraction of the fp32 vector rate that 2 H1 H2 + 2 H1 (D + 1) + 6 H2 operations per lane-step imply
(--peak-tflops, default 157.3: 256 CUs x 128 lanes x 2 ops x 2.4 GHz; the float64 scores of the draw are not counted); then
eager / this and this / greedy per repetition."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_mlp2 import HIDDEN, _sig, _time, make_triples  # noqa: E402  pylint: disable=wrong-import-position

GREEDY_OF = dict(sample='greedy', sample_evaluate='greedy_evaluate')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--eager-steps', type=int, default=32)
  ap.add_argument('--population', type=int, default=1024)
  ap.add_argument('--temperature', type=float, default=1.0)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--workloads', default='cartpole,cartpole_swingup,mountain_car')
  ap.add_argument('--policies', default='s64,s16,pop16')
  ap.add_argument('--variants', default='eager,sample,sample_evaluate,greedy,greedy_evaluate')
  ap.add_argument('--peak-tflops', type=float, default=157.3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  out = open(a.out, 'a') if a.out else None

  def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  sys.path.insert(0, ROOT)
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_mlp2_sample.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  kinds = a.variants.split(',')
  B, T = a.lanes, a.T
  n_fused = max(1, a.steps // T) * T
  for w in a.workloads.split(','):
    for policy in a.policies.split(','):
      H1, H2 = HIDDEN[policy]
      P = a.population if policy == 'pop16' else 1
      pidx = (torch.arange(B, device=dev, dtype=torch.int64) * P // B).to(torch.int32) if P > 1 else None
      runs, steps_of = {}, {}

      def fresh():
        env = bsuite_amd.load_from_id(w + '/0', batch=B, device=dev, seed=42)
        return env, env.observation_spec().shape[-1]

      env, D = fresh()
      triples = make_triples(torch, D, H1, H2, P, dev)
      pol = tuple(t[0].contiguous() for t in triples) if P == 1 else triples
      if 'eager' in kinds:
        own = pol if P == 1 else tuple(t[pidx.long()] for t in pol)      # (gathered once: the loop is not charged for it)
        state = dict(obs=env.reset().observation)
        g = torch.Generator(device=dev).manual_seed(1)

        def eager(n, env=env, own=own, state=state, g=g):
          obs = state['obs']
          for _ in range(n):
            words = torch.randint(1 << 32, (B, 3), generator=g, device=dev, dtype=torch.int64)
            obs = env.step(observations.gumbel_select(observations.mlp2_logits(*own, obs), words, a.temperature)).observation
          state['obs'] = obs

        runs['eager'], steps_of['eager'] = eager, a.eager_steps
        eager(4)
      drawn = dict(policy_index=pidx, temperature=a.temperature, sample_seed=7)
      for name, method, kw in (('sample', 'sample_mlp2', drawn), ('sample_evaluate', 'evaluate_sampled_mlp2', drawn),
                               ('greedy', 'rollout_mlp2', dict(policy_index=pidx)),
                               ('greedy_evaluate', 'evaluate_mlp2', dict(policy_index=pidx))):
        if name not in kinds:
          continue
        env, D = fresh()
        state = dict(obs=env.reset().observation.clone())

        def closed(n, call=getattr(env, method), state=state, rec=name in ('sample', 'greedy'), kw=kw):
          obs = state['obs']
          for _ in range(n // T):
            r = call(*pol, obs, T, **kw)
            obs = r[0].observation[-1] if rec else r.observation
          state['obs'] = obs

        runs[name], steps_of[name] = closed, n_fused
        closed(2 * T)                                                      # warm-up (allocates the outputs)
      order = tuple(runs)
      samples = {v: [] for v in order}
      for rep in range(a.reps):
        for v in (order if rep % 2 == 0 else order[::-1]):
          samples[v].append(_time(torch, runs[v], steps_of[v]))
      case = dict(workload=w, policy=policy, hidden=[H1, H2], population=P, T=T, lanes=B, temperature=a.temperature)
      ops = 2 * H1 * H2 + 2 * H1 * (D + 1) + 6 * H2
      for v in order:
        us = statistics.median(samples[v])
        row = dict(case, variant=v, steps=steps_of[v], us_per_step_event=us, us_event_reps=samples[v], env_steps_per_s=B / (us * 1e-6))
        if v != 'eager':
          row['policy_ops_per_lane_step'] = ops
          row['fraction_of_fp32_vector_rate'] = ops * B / (us * 1e-6) / (a.peak_tflops * 1e12)
        emit(_sig(row))
      for v in ('sample', 'sample_evaluate'):
        if v not in runs:
          continue
        ratios = dict(case, variant=v)
        if 'eager' in runs:
          ratios['eager_over_this_reps'] = [e / f for e, f in zip(samples['eager'], samples[v])]
        if GREEDY_OF[v] in runs:
          ratios['this_over_greedy_reps'] = [f / q for f, q in zip(samples[v], samples[GREEDY_OF[v]])]
        emit(_sig(ratios))
      del runs
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
