"""sample_embedding / evaluate_sampled_embedding against the eager loop they replace, against the greedy calls of the same kernel
and against the tabular drawn call — one process: deep_sea/10 (N = 30: the pair is read from global memory) and catch/0 (the pair
staged in LDS) at 2^20 lanes, T = 32, H in {16, 64} (the four shapes of tools/bench_embed.py), one JSON line per (workload, H,
variant).

  python tools/bench_embed_sample.py [--lanes 1048576] [--T 32] [--steps 256] [--eager-steps 32] [--reps 3] [--hidden 16,64] [--out FILE]

Variants, alternated inside each repetition (each has its own resident environment in observation_mode='index', warmed up
past its first resets):
  eager          obs -> embedding_logits(w1, w2, obs) -> gumbel_select(logits, words, temperature) -> step(a), step by step: the
                 loop of the contract, which is how a softmax network policy drove these families before this call.  The words
                 are torch.randint on the device, not the counter stream (a restatement of Philox in torch would only make the
                 loop slower): the loop is charged for one [B, A] draw per step;
  greedy         rollout_embedding, epsilon = 0: the recording call without the sampling;
  fused          sample_embedding;
  greedy_returns evaluate_embedding;
  fused_returns  evaluate_sampled_embedding;
  table          sample_policy with a table of logits: the drawn recording call without the network.
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median and env-steps/s;
then per (workload, H) eager / fused, eager / fused_returns, fused / greedy, fused_returns / greedy_returns, fused / table and
the env-steps/s of fused_returns over those of fused (= fused / fused_returns in time) per repetition.
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
from bench_embed import LDS_BYTES, WORKLOADS, staged_bytes  # noqa: E402

KERNEL = 'bsx_embed_kernel'


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--eager-steps', type=int, default=32)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--hidden', default='16,64')
  ap.add_argument('--temperature', type=float, default=1.0)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--variants', default='eager,greedy,fused,greedy_returns,fused_returns,table')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  T = a.T
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_embed_sample.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  out = open(a.out, 'a') if a.out else None
  kinds = a.variants.split(',')

  def emit(r):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  def make_env(w):
    return bsuite_amd.load_from_id(w, batch=B, device=dev, seed=42, observation_mode='index')

  B = a.lanes
  n_fused = max(1, a.steps // T) * T
  drawn = dict(temperature=a.temperature, sample_seed=7)
  for w in a.workloads.split(','):
    probe = bsuite_amd.load_from_id(w, batch=4, device=dev, seed=42, observation_mode='index')
    S, A, shape = probe.policy_num_states, probe.action_spec().num_values, probe.board_shape
    C = int(shape[0]) * int(shape[1])
    del probe
    for H in (int(h) for h in a.hidden.split(',')):
      runs, steps_of = {}, {}
      g = torch.Generator(device=dev).manual_seed(H)
      w1 = torch.randn((C + 2, H), generator=g, device=dev, dtype=torch.float32)
      w2 = torch.randn((A, H + 1), generator=g, device=dev, dtype=torch.float32)
      logits = torch.randn((S, A), generator=g, device=dev, dtype=torch.float32)

      if 'eager' in kinds:
        env = make_env(w)
        state = dict(obs=env.reset().observation)
        gw = torch.Generator(device=dev).manual_seed(1)

        def eager(n, env=env, state=state, gw=gw, w1=w1, w2=w2):
          obs = state['obs']
          for _ in range(n):
            words = torch.randint(1 << 32, (B, A), generator=gw, device=dev, dtype=torch.int64)
            l = observations.embedding_logits(w1, w2, obs)
            obs = env.step(observations.gumbel_select(l, words, a.temperature)).observation
          state['obs'] = obs

        runs['eager'], steps_of['eager'] = eager, a.eager_steps
        eager(4)
      for name, method, args, kw in (('greedy', 'rollout_embedding', (w1, w2), {}),
                                     ('fused', 'sample_embedding', (w1, w2), drawn),
                                     ('greedy_returns', 'evaluate_embedding', (w1, w2), {}),
                                     ('fused_returns', 'evaluate_sampled_embedding', (w1, w2), drawn),
                                     ('table', 'sample_policy', (logits,), drawn)):
        if name not in kinds:
          continue
        env = make_env(w)

        def closed(n, call=getattr(env, method), args=args, kw=kw):
          for _ in range(n // T):
            call(*args, T, **kw)

        runs[name], steps_of[name] = closed, n_fused
        closed(2 * T)                                                        # warm-up (allocates the outputs)
      order = tuple(runs)
      samples = {v: [] for v in order}
      for rep in range(a.reps):
        for v in (order if rep % 2 == 0 else order[::-1]):
          samples[v].append(ble._time(torch, runs[v], steps_of[v]))           # pylint: disable=protected-access
      case = dict(workload=w, n_cells=C, n_actions=A, hidden=H, pair='lds' if staged_bytes(C, H) <= LDS_BYTES else 'global',
                  temperature=a.temperature, T=T)
      for v in order:
        us = statistics.median(samples[v])
        emit(bench.sig(dict(case, variant=v, lanes=B, steps=steps_of[v], us_per_step_event=us, us_event_reps=samples[v],
                            env_steps_per_s=B / (us * 1e-6), reps=a.reps)))
      for num, den, key in (('eager', 'fused', 'eager_over_fused_reps'), ('eager', 'fused_returns', 'eager_over_fused_returns_reps'),
                            ('fused', 'greedy', 'fused_over_greedy_reps'),
                            ('fused_returns', 'greedy_returns', 'fused_returns_over_greedy_returns_reps'),
                            ('fused', 'table', 'fused_over_table_reps'),
                            ('fused', 'fused_returns', 'returns_steps_per_s_over_fused_steps_per_s_reps')):
        if num in runs and den in runs:
          emit(bench.sig(dict(case, variant='ratio', **{key: [x / y for x, y in zip(samples[num], samples[den])]})))
      del runs
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
