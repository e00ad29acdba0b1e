"""rollout_embedding / evaluate_embedding against the eager closed loop they replace and against the greedy tabular calls — one
process: deep_sea/10 (N = 30: the pair is read from global memory) and catch/0 (the pair staged in LDS) at 2^20 lanes, T = 32,
H in {16, 64}, one JSON line per (workload, H, variant).

  python tools/bench_embed.py [--lanes 1048576] [--T 32] [--steps 256] [--eager-steps 32] [--reps 3] [--hidden 16,64] [--out FILE]

Variants, alternated inside each repetition (each has its own resident environment in observation_mode='index', warmed up
past its first resets):
  eager          obs -> relu(index_embedding(obs, w1) + bias) @ w2.T + bias -> argmax -> step(a), step by step, as
                 examples/closed_loop_policy.py does with index_embedding and a matrix product: how a network policy drove
                 these families before this call (a fast torch policy, not the bit-exact helper);
  table          rollout_policy with a uint8 table, epsilon = 0: the recording loop without the network (the floor);
  fused          rollout_embedding, one shared pair;
  fused_pop      rollout_embedding with a population of two pairs and policy_index = 0 everywhere: the same weights looked up
                 through the population's path, which is always global memory (LDS against global at equal H, for catch);
  table_returns  evaluate_policy with the same uint8 table;
  fused_returns  evaluate_embedding.
Per row: every repetition's us per step on HIP events (`us_event_reps`, in the order measured), their median and env-steps/s;
then per (workload, H) eager / fused, fused / table, fused_pop / fused and fused_returns / table_returns per repetition.
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

WORKLOADS = ('deep_sea/10', 'catch/0')
KERNEL = 'bsx_embed_kernel'
LDS_BYTES = 15360


def staged_bytes(C, H, pad=4):
  return 4 * ((C + 2) * (((H + 3) & ~3) + pad) + 4 * (H + 1))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--lanes', type=int, default=1 << 20)
  ap.add_argument('--T', type=int, default=32)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--eager-steps', type=int, default=32)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--hidden', default='16,64')
  ap.add_argument('--workloads', default=','.join(WORKLOADS))
  ap.add_argument('--variants', default='eager,table,fused,fused_pop,table_returns,fused_returns')
  ap.add_argument('--label', default=None, help='copied into every row (which build of the library was measured)')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  T = a.T
  import torch  # pylint: disable=import-outside-toplevel
  import bsuite_amd  # pylint: disable=import-outside-toplevel
  from bsuite_amd.utils import observations  # pylint: disable=import-outside-toplevel
  if not torch.cuda.is_available():
    raise SystemExit('bench_embed.py measures on the GPU; none is visible')
  dev = torch.device('cuda:0')
  out = open(a.out, 'a') if a.out else None
  kinds = a.variants.split(',')

  def emit(r):
    if a.label:
      r = dict(r, label=a.label)
    line = json.dumps(r)
    print(line, flush=True)
    if out:
      out.write(line + '\n')
      out.flush()

  def make_env(w):
    return bsuite_amd.load_from_id(w, batch=B, device=dev, seed=42, observation_mode='index')

  B = a.lanes
  n_fused = max(1, a.steps // T) * T
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
      table = torch.randint(A, (S,), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
      pop1, pop2 = torch.stack([w1, w1]).contiguous(), torch.stack([w2, w2]).contiguous()
      zeros = torch.zeros(B, dtype=torch.int32, device=dev)

      if 'eager' in kinds:
        env = make_env(w)
        state = dict(obs=env.reset().observation)
        emb, bias = w1[:C + 1].contiguous(), w1[C + 1].contiguous()
        out_w, out_b = w2[:, :H].t().contiguous(), w2[:, H].contiguous()

        def eager(n, env=env, state=state, emb=emb, bias=bias, out_w=out_w, out_b=out_b):
          obs = state['obs']
          for _ in range(n):
            h = torch.relu(observations.index_embedding(obs, emb) + bias)
            obs = env.step(torch.addmm(out_b, h, out_w).argmax(dim=1).to(torch.int32)).observation
          state['obs'] = obs

        runs['eager'], steps_of['eager'] = eager, a.eager_steps
        eager(4)
      for name, method, args, kw in (('table', 'rollout_policy', (table,), {}),
                                     ('fused', 'rollout_embedding', (w1, w2), {}),
                                     ('fused_pop', 'rollout_embedding', (pop1, pop2), dict(policy_index=zeros)),
                                     ('table_returns', 'evaluate_policy', (table,), {}),
                                     ('fused_returns', 'evaluate_embedding', (w1, w2), {})):
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
      case = dict(workload=w, n_cells=C, n_actions=A, hidden=H, pair='lds' if staged_bytes(C, H) <= LDS_BYTES else 'global', T=T)
      for v in order:
        us = statistics.median(samples[v])
        emit(bench.sig(dict(case, variant=v, lanes=B, steps=steps_of[v], us_per_step_event=us, us_event_reps=samples[v],
                            env_steps_per_s=B / (us * 1e-6), reps=a.reps)))
      for num, den, key in (('eager', 'fused', 'eager_over_fused_reps'), ('eager', 'fused_returns', 'eager_over_fused_returns_reps'),
                            ('fused', 'table', 'fused_over_table_reps'), ('fused_pop', 'fused', 'fused_pop_over_fused_reps'),
                            ('fused_returns', 'table_returns', 'fused_returns_over_table_returns_reps')):
        if num in runs and den in runs:
          emit(bench.sig(dict(case, variant='ratio', **{key: [x / y for x, y in zip(samples[num], samples[den])]})))
      del runs
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == '__main__':
  main()
