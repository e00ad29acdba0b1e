"""sample_policy / evaluate_sampled_policy against the eager loop they replace and against the greedy tabular calls — one
process: deep_sea/10 and catch/0 (the shared table of logits staged in LDS) and deep_sea N = 50 (the table read from global
memory) at 2^20 lanes, T = 32, one JSON line per (workload, variant).

  python tools/bench_tab_sample.py [--lanes 1048576] [--T 32] [--steps 256] [--eager-steps 32] [--reps 3] [--out FILE]

Variants, alternated inside each repetition (each has its own resident environment in observation_mode='index', warmed up
past its first resets):
  eager          obs -> logits[policy_key(obs)] -> gumbel_select(logits, words, temperature) -> step(a), step by step: how a
                 tabular softmax agent's trajectory was recorded before this call.  The words are torch.randint on the device,
                 not the counter stream (a restatement of Philox in torch would only make the loop slower): the loop is charged
                 for one [B, A] draw per step;
  greedy         rollout_policy with the table argmax(logits), epsilon = 0: the recording call without the sampling;
  fused          sample_policy;
  greedy_returns evaluate_policy with the same uint8 table;
  fused_returns  evaluate_sampled_policy.
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median and env-steps/s;
then per workload eager / fused, fused / greedy and fused_returns / greedy_returns per repetition.
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

WORKLOADS = ('deep_sea/10', 'catch/0', 'deep_sea_n50')
KERNEL = 'bsx_tab_softmax_kernel'
LDS_BYTES = 12288


def make_env(w, B, dev):
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.environments import deep_sea  # pylint: disable=import-outside-toplevel
  if w == 'deep_sea_n50':
    return deep_sea.DeepSea(size=50, mapping_seed=42, seed=42, batch=B, device=dev, observation_mode='index')
  return bsuite_amd.load_from_id(w, batch=B, device=dev, seed=42, observation_mode='index')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--eager-steps', type=int, default=32)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--temperature', type=float, default=1.0)
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--variants', default='eager,greedy,fused,greedy_returns,fused_returns')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  T = a.T
  import torch  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_tab_sample.py measures on the GPU; none is visible')
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
    runs, steps_of = {}, {}
    probe = make_env(w, 4, dev)
    S, A, shape = probe.policy_num_states, probe.action_spec().num_values, probe.board_shape
    del probe
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn((S, A), generator=g, device=dev, dtype=torch.float32)
    table = torch.argmax(logits, dim=1).to(torch.uint8)
    in_lds = S * A * 4 <= LDS_BYTES

    if 'eager' in kinds:
      env = make_env(w, B, dev)
      state = dict(obs=env.reset().observation)
      gw = torch.Generator(device=dev).manual_seed(1)

      def eager(n, env=env, state=state, gw=gw):
        obs = state['obs']
        for _ in range(n):
          words = torch.randint(1 << 32, (B, A), generator=gw, device=dev, dtype=torch.int64)
          key = observations.policy_key(obs, shape).clamp(0, S - 1)
          obs = env.step(observations.gumbel_select(logits[key], words, a.temperature)).observation
        state['obs'] = obs

      runs['eager'], steps_of['eager'] = eager, a.eager_steps
      eager(4)
    for name, method, arg, kw in (('greedy', 'rollout_policy', table, dict(epsilon=0.0)),
                                  ('fused', 'sample_policy', logits, dict(temperature=a.temperature, sample_seed=7)),
                                  ('greedy_returns', 'evaluate_policy', table, dict(epsilon=0.0)),
                                  ('fused_returns', 'evaluate_sampled_policy', logits, dict(temperature=a.temperature, sample_seed=7))):
      if name not in kinds:
        continue
      env = make_env(w, B, dev)

      def closed(n, call=getattr(env, method), arg=arg, kw=kw):
        for _ in range(n // T):
          call(arg, T, **kw)

      runs[name], steps_of[name] = closed, n_fused
      closed(2 * T)                                                        # warm-up (allocates the outputs)
    order = tuple(runs)
    samples = {v: [] for v in order}
    for rep in range(a.reps):
      for v in (order if rep % 2 == 0 else order[::-1]):
        samples[v].append(ble._time(torch, runs[v], steps_of[v]))           # pylint: disable=protected-access
    case = dict(workload=w, n_states=S, n_actions=A, table='lds' if in_lds else 'global', temperature=a.temperature, T=T)
    for v in order:
      us = statistics.median(samples[v])
      emit(bench.sig(dict(case, variant=v, lanes=B, steps=steps_of[v], us_per_step_event=us, us_event_reps=samples[v],
                          env_steps_per_s=B / (us * 1e-6), reps=a.reps)))
    for num, den, key in (('eager', 'fused', 'eager_over_fused_reps'), ('fused', 'greedy', 'fused_over_greedy_reps'),
                          ('fused_returns', 'greedy_returns', 'fused_returns_over_greedy_returns_reps')):
      if num in runs and den in runs:
        emit(bench.sig(dict(case, variant='ratio', **{key: [x / y for x, y in zip(samples[num], samples[den])]})))
    del runs
    torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
