"""Closed loop on the device: a batched environment stepped by a (random-weight) linear policy that
reads the observation tensor the engine just wrote — no host round trip anywhere in the loop.

    python examples/closed_loop_policy.py [bsuite_id] [lanes] [steps] [--observation-dtype float32|uint8|float16|bfloat16]
                                          [--observation-mode dense|index] [--fused-table [--evaluate]]

With a narrow --observation-dtype (deep_sea, catch) the engine writes the boards as bytes or 16-bit floats, and the policy
converts each board once, as it reads it: to float32 from uint8, not at all from float16 / bfloat16, whose weights and
matrix product stay in that type.

With --observation-mode index (deep_sea, catch) the engine writes the numbers of the board's hot cells instead of the
board, and the same linear policy is a row gather: `board @ W` of a one-hot board is `W[cell]` (summed over the ball's and
the paddle's cell for catch; a cell they share counts once, as on the board) — the same float32 logits as the dense run
for the same weights, without the board ever being written or read.

With --fused-table (deep_sea, catch; implies --observation-mode index) the same greedy policy is tabulated once — entry k
of a uint8 table is the argmax of the logits of the observation with key k (`observations.policy_key`) — and the whole
loop runs inside the engine: `env.rollout_policy(table, T)` is ONE launch for T closed-loop steps, and gives the same
trajectories (the same bsuite_info sums) as the eager index run.  With --evaluate on top the calls are
`env.evaluate_policy(table, T)`: the same steps, but no TimeStep is written — three numbers per lane come back (episodes
ended, sum of rewards, sum of the returns of the episodes that ended), and the mean episode return is printed from them.

This is the batched counterpart of the reference run loop (bsuite/baselines/experiment.py:43-57):
`timestep = env.step(agent.select_action(timestep))`, with 2^20 environments per call.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
import bsuite_amd  # noqa: E402
from bsuite_amd.utils import observations  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('bsuite_id', nargs='?', default='deep_sea/10')
  ap.add_argument('lanes', nargs='?', type=int, default=1 << 20)
  ap.add_argument('steps', nargs='?', type=int, default=200)
  ap.add_argument('--observation-dtype', default='float32', choices=('float32', 'uint8', 'float16', 'bfloat16'))
  ap.add_argument('--observation-mode', default='dense', choices=('dense', 'index'))
  ap.add_argument('--fused-table', action='store_true', help='tabulate the greedy policy and run the loop inside the engine (rollout_policy)')
  ap.add_argument('--evaluate', action='store_true', help='with --fused-table: evaluate_policy instead of rollout_policy (returns only)')
  a = ap.parse_args()
  if a.evaluate and not a.fused_table:
    ap.error('--evaluate needs --fused-table')
  if a.fused_table:
    a.observation_mode = 'index'
  bsuite_id, lanes, steps = a.bsuite_id, a.lanes, a.steps
  index = a.observation_mode == 'index'
  env = bsuite_amd.load_from_id(bsuite_id, batch=lanes, seed=0, observation_dtype=a.observation_dtype,
                                observation_mode=a.observation_mode)
  n_obs = int(torch.tensor(env.board_shape if index else env.observation_spec().shape).prod())
  n_act = env.action_spec().num_values
  compute = torch.float32 if index or not env.observation_dtype.is_floating_point else env.observation_dtype
  g = torch.Generator(device='cuda').manual_seed(0)
  weights = torch.randn((n_obs, n_act), device='cuda', generator=g).to(compute)
  table = torch.cat([torch.zeros((1, n_act), device='cuda', dtype=compute), weights]) if index else None   # row 0: "no cell"

  def logits_of(timestep):                        # a linear read-out of the observation
    if index:
      cells = timestep.observation                                     # int32 [lanes, K]
      if cells.shape[1] == 2:                                          # catch: a cell ball and paddle share is ONE 1 on the board
        cells = torch.where((cells[:, 1:] == cells[:, :1]).expand(-1, 2) & torch.tensor([False, True], device=cells.device),
                            torch.full_like(cells, -1), cells)
      return observations.index_embedding(cells, table)
    board = timestep.observation.reshape(lanes, n_obs).to(compute)      # the one conversion (none for a float board)
    return board @ weights

  def policy(timestep):                           # greedy
    return logits_of(timestep).argmax(dim=1).to(torch.int32)

  def greedy_table():                             # entry k: the action `policy` takes on the observation with key k
    rows, columns = env.board_shape
    k = torch.arange(env.policy_num_states, device='cuda')
    if env.observation_spec().shape[0] == 1:      # deep_sea: the key is the cell
      cells = k[:, None].to(torch.int32)
    else:                                         # catch: key = ball_cell * columns + paddle_x
      cells = torch.stack([k // columns, (rows - 1) * columns + k % columns], dim=1).to(torch.int32)
    return policy(ts._replace(observation=cells)).to(torch.uint8)

  ts = env.reset()
  if a.fused_table:
    fused = greedy_table()
    run = env.evaluate_policy if a.evaluate else env.rollout_policy
    run(fused, 20)
    torch.cuda.synchronize()
    episodes = torch.zeros(lanes, dtype=torch.int64, device=fused.device)
    returns = torch.zeros(lanes, dtype=torch.float64, device=fused.device)
    t0 = time.perf_counter()
    for n in [32] * (steps // 32) + ([steps % 32] if steps % 32 else []):
      ev = run(fused, n)
      if a.evaluate:                              # (the three columns are overwritten by the next call)
        episodes += ev.episodes
        returns += ev.return_sum                  # (episode_return_sum counts only a call's own rewards of an episode the
                                                  # calls cut in two; over many calls the sum of all rewards loses nothing)
  else:
    for _ in range(20):
      ts = env.step(policy(ts))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
      ts = env.step(policy(ts))
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  info = {k: float(v.sum()) for k, v in env.bsuite_info().items()}
  if a.evaluate:
    print(json.dumps(dict(episodes=int(episodes.sum()), mean_episode_return=float(returns.sum() / episodes.sum().clamp(min=1)))))
  print(json.dumps(dict(bsuite_id=bsuite_id, observation_dtype=a.observation_dtype, observation_mode=a.observation_mode, fused_table=a.fused_table, lanes=lanes, steps=steps, ms_per_step=round(dt / steps * 1e3, 4),
                        env_steps_per_s=round(lanes * steps / dt), episodes_finished=int(env.episode_counters()[0]),
                        bsuite_info_sums=info)))


if __name__ == '__main__':
  main()
