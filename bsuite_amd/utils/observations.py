"""Helpers for index observations (observation_mode='index' of deep_sea and catch: dense boards, table keys, and hidden-layer
policies on the index row, `env.rollout_embedding`, `env.evaluate_embedding`) and for linear and hidden-layer policies on
the float observations of the physics families (`env.evaluate_linear`, `env.evaluate_mlp`, `env.sample_linear`, `env.sample_mlp`).

An index observation names the hot cells of a one-hot board: int32 `[..., K]`, each entry a flat cell number of the
dense board (`env.board_shape`) or -1 for "no cell" (deep_sea's all-zero terminal board).  Pure torch: they work on
any device and on any leading dimensions (`[B, K]` from step(), `[T, B, K]` from rollout()).
"""
from typing import Optional, Sequence

import numpy as np
import torch


def index_to_dense(index: torch.Tensor, board_shape: Sequence[int], dtype: torch.dtype = torch.float32,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
  """The dense boards `[..., *board_shape]` an index observation `[..., K]` stands for: zeros with a one at every entry
  >= 0 (entries that name the same cell give one 1, as in the dense observation).  `out`, if given, is overwritten."""
  board_shape = tuple(int(s) for s in board_shape)
  cells = 1
  for s in board_shape:
    cells *= s
  lead = tuple(index.shape[:-1])
  if out is None:
    out = torch.zeros(lead + board_shape, dtype=dtype, device=index.device)
  else:
    if tuple(out.shape) != lead + board_shape or not out.is_contiguous() or out.device != index.device:
      raise ValueError(f'index_to_dense: `out` must be a contiguous tensor of shape {lead + board_shape} on {index.device}')
    out.zero_()
  idx = index.reshape(-1, index.shape[-1]).to(torch.int64)
  flat = out.view(-1, cells)
  # -1 entries go to a scratch column behind the board, which is dropped: no data-dependent control flow, no host sync
  padded = torch.zeros((flat.shape[0], cells + 1), dtype=out.dtype, device=out.device)
  padded.scatter_(1, torch.where(idx >= 0, idx, torch.full_like(idx, cells)), 1)
  flat.copy_(padded[:, :cells])
  return out


def policy_key(index_rows: torch.Tensor, board_shape: Sequence[int]) -> torch.Tensor:
  """The key `[...]` (int64) of an index observation `[..., K]` in a tabular policy (`env.rollout_policy`): the entry of
  the table a lane with that observation takes its action from.

    deep_sea (K = 1)  the observation itself, `row * N + col`; -1 on the terminal observation, which is never looked up
                      (the lane resets on the call that follows it);
    catch    (K = 2)  `ball_cell * columns + paddle_x` with `paddle_x = paddle_cell - (rows - 1) * columns`.

  A table has `env.policy_num_states` entries: N * N, or rows * columns * columns."""
  rows, columns = (int(s) for s in board_shape)
  k = int(index_rows.shape[-1])
  idx = index_rows.to(torch.int64)
  if k == 1:
    return idx[..., 0]
  if k == 2:
    return idx[..., 0] * columns + (idx[..., 1] - (rows - 1) * columns)
  raise ValueError(f'policy_key: index observations have one (deep_sea) or two (catch) entries, got {k}')


def index_embedding(index: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
  """`sum_k table[index[..., k] + 1]`: the gather form of `board.reshape(..., cells) @ W` for a one-hot board, with
  `table` = `[cells + 1, D]` whose row 0 is zero (the row -1 selects) and whose row c + 1 is `W[c]`.  For catch the two
  rows of ball and paddle are summed, also when they name the same cell — there the dense board holds ONE 1, so the
  two forms differ on the step where the paddle catches the ball; use index_to_dense where that matters."""
  return table[index.to(torch.int64) + 1].sum(dim=-2)


def embedding_logits(w1: torch.Tensor, w2: torch.Tensor, index_rows: torch.Tensor, return_preactivations: bool = False):
  """The logits `[B, A]` (float32) of a policy with one ReLU hidden layer on index observations `[B, K]`, exactly as
  `env.rollout_embedding` / `env.evaluate_embedding` compute them inside their kernel (csrc/bsx_embed.h).  `w1` is float32
  `[C + 2, H]` — row c + 1 the embedding of cell c, row 0 the row a -1 entry selects (`index_embedding`'s layout), row C + 1
  the hidden bias — and `w2` `[A, H + 1]`, the bias in the last column (one pair), or `[B, C + 2, H]` and `[B, A, H + 1]` (lane
  b's own pair, e.g. `population[policy_index.clamp(0, P - 1).long()]`).

    l_a = w2[a][H]
    for j = 0..H-1: s = w1[C+1][j]; for k = 0..K-1: s = s + w1[cell_k + 1][j]    float32, every multiply and every add rounded
                    h = s if s > 0 else +0.0                                      on its own: separate torch ops, never addcmul
                    l_a = l_a + w2[a][j] * h                                      or matmul; a NaN s gives h = 0

  cell_k is entry k of the row in order (catch: ball, then paddle; the same cell twice is added twice, as index_embedding
  does), clamped to [-1, C - 1].  With `return_preactivations` the result is `(logits, s)`, `s` float32 `[B, H]`."""
  B, K = int(index_rows.shape[0]), int(index_rows.shape[1])
  a1 = w1 if w1.dim() == 3 else w1.unsqueeze(0).expand(B, -1, -1)
  a2 = w2 if w2.dim() == 3 else w2.unsqueeze(0).expand(B, -1, -1)
  C, H = int(a1.shape[1]) - 2, int(a1.shape[2])
  rows = index_rows.to(torch.int64).clamp(-1, C - 1) + 1                                    # [B, K]
  s = a1[:, C + 1, :].clone()                                                               # [B, H]: all hidden units at once
  for k in range(K):
    e = torch.gather(a1, 1, rows[:, k].reshape(B, 1, 1).expand(B, 1, H))[:, 0, :]
    s = s + e
  h = torch.where(s > 0, s, torch.zeros_like(s))
  logits = a2[:, :, H].clone()
  for j in range(H):
    prod = a2[:, :, j] * h[:, j:j + 1]
    logits = logits + prod
  return (logits, s) if return_preactivations else logits


def embedding_select(w1: torch.Tensor, w2: torch.Tensor, index_rows: torch.Tensor) -> torch.Tensor:
  """The greedy action `[B]` (int32) of `embedding_logits(w1, w2, index_rows)`, exactly as `env.rollout_embedding` selects it
  inside its kernel (csrc/bsx_embed.h):

    best = 0; for a = 1..A-1: if l_a > l_best: best = a                the lowest index wins a tie, a NaN never wins"""
  logits = embedding_logits(w1, w2, index_rows)
  best = torch.zeros(logits.shape[0], dtype=torch.int32, device=logits.device)
  l_best = logits[:, 0]
  for a in range(1, int(logits.shape[1])):
    better = logits[:, a] > l_best
    best = torch.where(better, torch.full_like(best, a), best)
    l_best = torch.where(better, logits[:, a], l_best)
  return best


def linear_select(weights: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
  """The greedy action `[B]` (int32) of a linear policy on float observations, exactly as `env.evaluate_linear` selects it
  inside its kernel (csrc/bsx_linear.h).  `weights` is float32 `[A, D+1]` (one matrix) or `[B, A, D+1]` (lane b's own
  matrix, e.g. `population[policy_index.clamp(0, P - 1).long()]`), column D the bias; `obs` is float32 `[B, *obs_shape]`
  with D elements per lane.

    l_a = w[a][D]; for d = 0..D-1: l_a = l_a + w[a][d] * obs[d]        float32, every multiply and every add rounded on its
                                                                       own: separate torch ops, never addcmul or matmul
    best = 0; for a = 1..A-1: if l_a > l_best: best = a                the lowest index wins a tie, a NaN never wins"""
  o = obs.reshape(obs.shape[0], -1)
  D = int(o.shape[1])
  w = weights if weights.dim() == 3 else weights.unsqueeze(0).expand(o.shape[0], -1, -1)
  logits = w[:, :, D].clone()
  for d in range(D):
    prod = w[:, :, d] * o[:, d:d + 1]
    logits = logits + prod
  best = torch.zeros(o.shape[0], dtype=torch.int32, device=o.device)
  l_best = logits[:, 0]
  for a in range(1, int(w.shape[1])):
    better = logits[:, a] > l_best
    best = torch.where(better, torch.full_like(best, a), best)
    l_best = torch.where(better, logits[:, a], l_best)
  return best


def mlp_select(w1: torch.Tensor, w2: torch.Tensor, obs: torch.Tensor, return_preactivations: bool = False):
  """The greedy action `[B]` (int32) of a policy with one ReLU hidden layer on float observations, exactly as
  `env.evaluate_mlp` selects it inside its kernel (csrc/bsx_mlp.h).  `w1` is float32 `[H, D+1]` and `w2` `[3, H+1]` (one
  pair), or `[B, H, D+1]` and `[B, 3, H+1]` (lane b's own pair, e.g. `population[policy_index.clamp(0, P - 1).long()]`), the
  bias in the last column of each; `obs` is float32 `[B, *obs_shape]` with D elements per lane.

    l_a = w2[a][H]
    for j = 0..H-1: s = w1[j][D]; for d = 0..D-1: s = s + w1[j][d] * obs[d]      float32, every multiply and every add rounded
                    h = s if s > 0 else +0.0                                      on its own: separate torch ops, never addcmul
                    l_a = l_a + w2[a][j] * h                                      or matmul; a NaN s gives h = 0
    best = 0; for a = 1, 2: if l_a > l_best: best = a                             the lowest index wins a tie, a NaN never wins

  With `return_preactivations` the result is `(best, s)`, `s` float32 `[B, H]`."""
  o = obs.reshape(obs.shape[0], -1)
  B, D = int(o.shape[0]), int(o.shape[1])
  a1 = w1 if w1.dim() == 3 else w1.unsqueeze(0).expand(B, -1, -1)
  a2 = w2 if w2.dim() == 3 else w2.unsqueeze(0).expand(B, -1, -1)
  H = int(a1.shape[1])
  s = a1[:, :, D].clone()                                    # [B, H]: all hidden units at once, each in its own d order
  for d in range(D):
    prod = a1[:, :, d] * o[:, d:d + 1]
    s = s + prod
  h = torch.where(s > 0, s, torch.zeros_like(s))
  logits = a2[:, :, H].clone()
  for j in range(H):
    prod = a2[:, :, j] * h[:, j:j + 1]
    logits = logits + prod
  best = torch.zeros(B, dtype=torch.int32, device=o.device)
  l_best = logits[:, 0]
  for a in range(1, int(a2.shape[1])):
    better = logits[:, a] > l_best
    best = torch.where(better, torch.full_like(best, a), best)
    l_best = torch.where(better, logits[:, a], l_best)
  return (best, s) if return_preactivations else best


def linear_logits(weights: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
  """The logits `[B, A]` (float32) of a linear policy on float observations, exactly as `env.sample_linear` computes them
  inside its kernel (bsx_linear_logits, csrc/bsx_gumbel.h) — the accumulations of `linear_select`, without its argmax:

    l_a = w[a][D]; for d = 0..D-1: l_a = l_a + w[a][d] * obs[d]        float32, every multiply and every add rounded on its
                                                                       own: separate torch ops, never addcmul or matmul

  `weights` is float32 `[A, D+1]` or `[B, A, D+1]` (lane b's own matrix), `obs` float32 `[B, *obs_shape]`.  What a learner
  recomputes log-probabilities from: the action of step t was drawn from
  `softmax(linear_logits(w, ts.observation[t - 1]) / temperature)`."""
  o = obs.reshape(obs.shape[0], -1)
  D = int(o.shape[1])
  w = weights if weights.dim() == 3 else weights.unsqueeze(0).expand(o.shape[0], -1, -1)
  logits = w[:, :, D].clone()
  for d in range(D):
    prod = w[:, :, d] * o[:, d:d + 1]
    logits = logits + prod
  return logits


def mlp_logits(w1: torch.Tensor, w2: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
  """The logits `[B, 3]` (float32) of a policy with one ReLU hidden layer, exactly as `env.sample_mlp` computes them inside its
  kernel (csrc/bsx_mlp.h's pieces) — the accumulations of `mlp_select`, without its argmax:

    l_a = w2[a][H]
    for j = 0..H-1: s = w1[j][D]; for d = 0..D-1: s = s + w1[j][d] * obs[d]      float32, every multiply and every add rounded
                    h = s if s > 0 else +0.0                                      on its own: separate torch ops, never addcmul
                    l_a = l_a + w2[a][j] * h                                      or matmul; a NaN s gives h = 0

  `w1` is float32 `[H, D+1]` and `w2` `[3, H+1]`, or `[B, H, D+1]` and `[B, 3, H+1]` (lane b's own pair)."""
  o = obs.reshape(obs.shape[0], -1)
  B, D = int(o.shape[0]), int(o.shape[1])
  a1 = w1 if w1.dim() == 3 else w1.unsqueeze(0).expand(B, -1, -1)
  a2 = w2 if w2.dim() == 3 else w2.unsqueeze(0).expand(B, -1, -1)
  H = int(a1.shape[1])
  s = a1[:, :, D].clone()
  for d in range(D):
    prod = a1[:, :, d] * o[:, d:d + 1]
    s = s + prod
  h = torch.where(s > 0, s, torch.zeros_like(s))
  logits = a2[:, :, H].clone()
  for j in range(H):
    prod = a2[:, :, j] * h[:, j:j + 1]
    logits = logits + prod
  return logits


def _mlp2_forward(w1, w2, w3, obs):
  """(logits [B, 3], s1 [B, H1], s2 [B, H2]) of the two-hidden-layer rule: `mlp2_logits` has the definition."""
  o = obs.reshape(obs.shape[0], -1)
  B, D = int(o.shape[0]), int(o.shape[1])
  a1, a2, a3 = (w if w.dim() == 3 else w.unsqueeze(0).expand(B, -1, -1) for w in (w1, w2, w3))
  H1, H2 = int(a1.shape[1]), int(a2.shape[1])
  s1 = a1[:, :, D].clone()                                   # [B, H1]: all units of a layer at once, each in its own order
  for d in range(D):
    prod = a1[:, :, d] * o[:, d:d + 1]
    s1 = s1 + prod
  h1 = torch.where(s1 > 0, s1, torch.zeros_like(s1))
  s2 = a2[:, :, H1].clone()                                  # [B, H2]
  for j in range(H1):
    prod = a2[:, :, j] * h1[:, j:j + 1]
    s2 = s2 + prod
  h2 = torch.where(s2 > 0, s2, torch.zeros_like(s2))
  logits = a3[:, :, H2].clone()
  for k in range(H2):
    prod = a3[:, :, k] * h2[:, k:k + 1]
    logits = logits + prod
  return logits, s1, s2


def mlp2_logits(w1: torch.Tensor, w2: torch.Tensor, w3: torch.Tensor, obs: torch.Tensor) -> torch.Tensor:
  """The logits `[B, 3]` (float32) of a policy with two ReLU hidden layers, exactly as `env.evaluate_mlp2` / `env.rollout_mlp2`
  compute them inside their kernel (csrc/bsx_mlp2.h):

    h1_j = s if s > 0 else +0.0, s = w1[j][D]; for d = 0..D-1: s = s + w1[j][d] * obs[d]          float32, every multiply and
    s2_k = w2[k][H1]; for j = 0..H1-1: s2_k = s2_k + w2[k][j] * h1_j                               every add rounded on its own:
    h2_k = s2_k if s2_k > 0 else +0.0                                                              separate torch ops, never
    l_a  = w3[a][H2]; for k = 0..H2-1: l_a = l_a + w3[a][k] * h2_k                                 addcmul or matmul

  `w1` is float32 `[H1, D+1]`, `w2` `[H2, H1+1]` and `w3` `[3, H2+1]` (one triple), or `[B, H1, D+1]`, `[B, H2, H1+1]` and
  `[B, 3, H2+1]` (lane b's own triple, e.g. `population[policy_index.clamp(0, P - 1).long()]`), the bias in the last column of
  each: `torch.cat([lin.weight, lin.bias[:, None]], 1)` of a `torch.nn.Linear`.  A NaN pre-activation gives an activation of
  0; `inf * 0` gives a NaN."""
  return _mlp2_forward(w1, w2, w3, obs)[0]


def mlp2_select(w1: torch.Tensor, w2: torch.Tensor, w3: torch.Tensor, obs: torch.Tensor, return_preactivations: bool = False):
  """The greedy action `[B]` (int32) of a policy with two ReLU hidden layers on float observations, exactly as
  `env.evaluate_mlp2` / `env.rollout_mlp2` select it inside their kernel (csrc/bsx_mlp2.h): the argmax of `mlp2_logits` (which
  has the shapes and the rule) — the lowest index wins a tie, a NaN never wins.  With `return_preactivations` the result is
  `(best, s1 [B, H1], s2 [B, H2])`."""
  logits, s1, s2 = _mlp2_forward(w1, w2, w3, obs)
  best = torch.zeros(logits.shape[0], dtype=torch.int32, device=logits.device)
  l_best = logits[:, 0]
  for a in range(1, int(logits.shape[1])):
    better = logits[:, a] > l_best
    best = torch.where(better, torch.full_like(best, a), best)
    l_best = torch.where(better, logits[:, a], l_best)
  return (best, s1, s2) if return_preactivations else best


def _stream_log(x: torch.Tensor) -> torch.Tensor:
  """bsx_log (include/bsx_stream.h) on a float64 tensor of positive normal numbers, operation for operation: the exponent
  and the mantissa from the bits, m in [~0.707, 1.414], s = (m - 1) / (m + 1), the odd series of 2 atanh(s) to s^25 by
  Horner's rule with every multiply and every add a torch op of its own.  Never torch.log: its last bits differ."""
  u = x.contiguous().view(torch.int64)
  e = ((u >> 52) & 0x7FF) - 1023
  m = ((u & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000).view(torch.float64)
  big = m > 1.4142135623730951
  m = torch.where(big, m * 0.5, m)
  e = torch.where(big, e + 1, e)
  s = (m - 1.0) / (m + 1.0)
  s2 = s * s
  p = torch.full_like(s, 1.0 / 25.0)
  for d in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
    p = p * s2
    p = p + 1.0 / d
  p = p * s2
  p = p + 1.0
  lm = (2.0 * s) * p
  return e.to(torch.float64) * 0.6931471805599453 + lm


def gumbel_select(logits: torch.Tensor, words, temperature: float = 1.0) -> torch.Tensor:
  """The action `[B]` (int32) that `env.sample_linear` / `env.sample_mlp` (A = 3) and `env.sample_policy` /
  `env.evaluate_sampled_policy` (A = 2 for deep_sea, 3 for catch) draw from float32 `logits` `[B, A]` and the lane's A 32-bit
  words `[B, A]` (a uint32 numpy array such as oracle.stream.words(sample_seed, lanes, call index, 3, A), or an integer tensor
  with values in [0, 2^32)), exactly as the kernels do (bsx_gumbel_select, csrc/bsx_gumbel.h; bsx_gumbel_select_n,
  csrc/bsx_tab_sample.h) — Gumbel-max in float64, every operation a torch op of its own:

    beta = 1 / temperature                                   Python float64
    u_a = (word_a + 0.5) * 2^-32                             exact, in (0, 1)
    g_a = -log(-log(u_a))                                    the engine's bit-reproducible log, never torch.log
    z_a = float64(l_a) * beta + g_a                          a multiply, then an add
    best = 0; for a = 1 .. A-1: if z_a > z_best: best = a    the lowest index wins a tie, a NaN never wins

  so that P(a) = softmax(logits / temperature)[a] over the words."""
  beta = 1.0 / float(temperature)
  if not torch.is_tensor(words):
    words = torch.from_numpy(np.ascontiguousarray(np.asarray(words).astype(np.int64)))
  w = (words.to(torch.int64) & 0xFFFFFFFF).to(logits.device)
  u = (w.to(torch.float64) + 0.5) * 2.0 ** -32
  g = -_stream_log(-_stream_log(u))
  z = logits.to(torch.float64) * beta
  z = z + g
  best = torch.zeros(z.shape[0], dtype=torch.int32, device=z.device)
  z_best = z[:, 0]
  for a in range(1, int(z.shape[1])):
    better = z[:, a] > z_best
    best = torch.where(better, torch.full_like(best, a), best)
    z_best = torch.where(better, z[:, a], z_best)
  return best
