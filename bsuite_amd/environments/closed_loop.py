"""The fused closed-loop calls of the batched environments: T steps in ONE launch with the actions chosen on the device.

Twenty entry points, four verbs — rollout_ (greedy / epsilon-greedy, records the trajectory), evaluate_ (the same steps,
returns only), sample_ (actions drawn from a softmax, records) and evaluate_sampled_ (drawn, returns only) — times five
policy forms: `policy` and `embedding` on the index observation of the grids (deep_sea, catch), `linear`, `mlp` and `mlp2`
on the float rows of the physics families (cartpole, swing-up, mountain_car).  `ClosedLoop` is the mixin that gives them to
base.Environment; this module is the one place that knows how such a call is checked, named, given outputs and launched:

* the entry point of call <verb>_<kind> is bsx_<family>_<kind>_<rollout|evaluate|sample|sample_evaluate> for a family that
  lists <kind> in `_closed_loop_kinds` (`_closed_loop_abi`), and the refusal of a family without the call reads the same rule;
* every refusal comes before anything is allocated or any native symbol is fetched: the environment's (`_check_closed_loop_env`),
  then the call's own weights, population and scalars (the `_check_*` of each form), then — recording physics calls alone —
  the 4 GiB slab;
* a recording call writes the [T,B] outputs and the action tensor cached per T in `_policy_rollout_out` and returns
  `(timestep, actions)` (`_record`); a returns-only call writes the family's one cached set of result columns —
  `_policy_eval_out` on the grids, `_linear_eval_out` with the final observation rows on the physics families — and returns
  it (`_evaluate`);
* the grids and the physics families differ in the argument list (`_launch_closed_loop`) and the result columns
  (`_evaluation_out`), nowhere else.

Each public method is its check, its ctypes struct and one of the two helpers; the T-step launch itself is
base.Environment._launch_steps.
"""
import collections
import ctypes
import functools
import math

import numpy as np
import torch

from bsuite_amd import _native

# What evaluate_policy() returns: three device tensors [B] (int32, float64, float64).
PolicyEvaluation = collections.namedtuple('PolicyEvaluation', ['episodes', 'return_sum', 'episode_return_sum'])
# What evaluate_linear() returns: the same three columns and the observation of the call's last step, float32 [B, *obs_shape].
LinearEvaluation = collections.namedtuple('LinearEvaluation', ['episodes', 'return_sum', 'episode_return_sum', 'observation'])

# the verb of a public call's name -> the verb of its entry point
_ABI_VERBS = {'rollout': 'rollout', 'evaluate': 'evaluate', 'sample': 'sample', 'evaluate_sampled': 'sample_evaluate'}
# the public calls of the forms that read the index observation (the grids'); every other form reads float rows
_GRID_CALLS = frozenset(f'{verb}_{kind}' for verb in _ABI_VERBS for kind in ('policy', 'embedding'))


@functools.lru_cache(maxsize=None)
def _entry_point(family, kinds, what):
  """bsx_<family>_<kind>_<verb> for the public call `what` (<verb>_<kind>) of a family with the forms `kinds`, else None.
  (Cached: the calls resolve their name on every launch, and a launch of the small families is a few microseconds.)"""
  verb, kind = what.rsplit('_', 1)
  return f'bsx_{family}_{kind}_{_ABI_VERBS[verb]}' if kind in kinds else None


class ClosedLoop:
  """The fused closed-loop calls of base.Environment (a mixin: it uses the environment's columns, call descriptor and
  `_launch_steps`)."""

  _closed_loop_kinds = ()   # subclass: the policy forms the family has entry points for (deep_sea, catch: 'policy', 'embedding';
                            # cartpole, swing-up, mountain_car: 'linear', 'mlp', 'mlp2')

  def _closed_loop_abi(self, what):
    """The C-ABI entry point of the public call `what` (<verb>_<kind>), or None where the family lacks the form."""
    return _entry_point(self._abi_name, self._closed_loop_kinds, what)

  @property
  def policy_num_states(self) -> int:
    """Entries of one table of `rollout_policy` (deep_sea: N * N, catch: rows * columns * columns)."""
    raise ValueError(f'{type(self).__name__} has no tabular policy rollout (deep_sea and catch only)')

  # ----------------------------------------------------------------------------------------
  # the refusals every call shares: all of them before any GPU use, nothing allocated
  def _check_closed_loop_env(self, what, num_steps):
    """The environment's part of the refusals of the fused call `what`: the family, the view, the modes (the index
    observation for the grids' calls) and num_steps."""
    name, grid = type(self).__name__, what in _GRID_CALLS
    if self._closed_loop_abi(what) is None:
      if grid:
        raise ValueError(f'{name} has no tabular policy rollout (deep_sea and catch only)')
      raise ValueError(f'{name} has no {what}() (cartpole, cartpole_swingup and mountain_car only)')
    if self._scalar:
      raise ValueError(f'{what}() needs the batched view (batch=B)')
    if grid and not self._index:
      raise ValueError(f"{what}() looks its actions up by the index observation: build the environment with "
                       f"observation_mode='index' (this one is {self.observation_mode!r}, {self._obs_dtype})")
    if self._rng_mode != 'philox':
      raise ValueError(f"{what}() needs the counter-based draw stream (rng='philox')")
    if self._logging is not None:
      raise ValueError(f'{what}() is not available with Logging enabled')
    if self._wrap[0] != _native.WRAP_NONE:
      raise ValueError(f'{what}() is not available under a reward wrapper')
    if self._grouped_by is not None:
      raise RuntimeError(f'{what}() on a segment of prepared sweep groups: SweepBatch.release_groups() first')
    if isinstance(num_steps, bool) or not isinstance(num_steps, (int, np.integer)) or num_steps < 1:
      raise ValueError(f'{what}: num_steps must be an integer >= 1, got {num_steps!r}')

  @staticmethod
  def _check_epsilon(what, epsilon, explore_seed):
    """What the greedy calls refuse of their scalars: epsilon and the seed of its coin."""
    if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float, np.integer, np.floating)) or not 0.0 <= float(epsilon) <= 1.0:
      raise ValueError(f'{what}: epsilon must be a number in [0, 1], got {epsilon!r}')
    if isinstance(explore_seed, bool) or not isinstance(explore_seed, (int, np.integer)) or not 0 <= int(explore_seed) < (1 << 64):
      raise ValueError(f'{what}: explore_seed must be an integer in [0, 2^64), got {explore_seed!r}')

  @staticmethod
  def _check_sample(what, temperature, sample_seed):
    """What only the sampling calls refuse (before any GPU use): the temperature and the seed.  Returns beta = 1 / temperature,
    computed here in float64: the kernel multiplies by it and never divides."""
    ok = not isinstance(temperature, bool) and isinstance(temperature, (int, float, np.integer, np.floating))
    t = float(temperature) if ok else float('nan')
    ok = ok and math.isfinite(t) and t > 0.0
    beta = 1.0 / t if ok else float('nan')
    if not ok or not math.isfinite(beta):
      raise ValueError(f'{what}: temperature must be a finite number > 0 with a finite 1 / temperature, got {temperature!r} '
                       '(there is no greedy limit: that is rollout_linear / rollout_mlp)')
    if isinstance(sample_seed, bool) or not isinstance(sample_seed, (int, np.integer)) or not 0 <= int(sample_seed) < (1 << 64):
      raise ValueError(f'{what}: sample_seed must be an integer in [0, 2^64), got {sample_seed!r}')
    return beta

  def _check_population(self, what, P, policy_index, noun='tables', one='table'):
    """The rule every form shares: `policy_index` names each lane's member of a population of P `noun`."""
    if P == 1:
      if policy_index is not None:
        raise ValueError(f'{what}: policy_index names the row of a population of {noun}; with one {one} it must be None')
    elif (not torch.is_tensor(policy_index) or policy_index.dtype != torch.int32 or policy_index.device != self._device
          or tuple(policy_index.shape) != (self._batch,) or not policy_index.is_contiguous()):
      raise ValueError(f'{what}: a population of {P} {noun} needs policy_index, a contiguous int32 tensor of shape '
                       f'({self._batch},) on {self._device}')

  def _check_trajectory_slab(self, what):
    """What only the recording physics calls refuse: a [B, D] slab the kernel's 32-bit lane offsets cannot span."""
    D = int(np.prod(self._obs_shape))
    if self._batch * D * 4 >= 1 << 32:
      raise ValueError(f'{what}: a step of {self._batch} lanes x {D} floats is 4 GiB or more; split the lanes over several '
                       'environments (lane_offset)')

  # ----------------------------------------------------------------------------------------
  # outputs and the launch
  _evaluation_ptrs = None   # the struct of pointers the library writes the result columns through: _evaluation_out

  def _evaluation_out(self, grid):
    """The result columns of the returns-only calls — one set per environment, shared by all of the family's calls: a
    PolicyEvaluation on the grids, a LinearEvaluation (with the final observation rows) on the physics families — and the
    struct of pointers the library writes them through."""
    ev = self._policy_eval_out if grid else self._linear_eval_out
    if ev is None:
      cols = (torch.empty(self._batch, dtype=torch.int32, device=self._device),
              torch.empty(self._batch, dtype=torch.float64, device=self._device),
              torch.empty(self._batch, dtype=torch.float64, device=self._device))
      if grid:
        ev = self._policy_eval_out = PolicyEvaluation(*cols)
      else:
        ev = self._linear_eval_out = LinearEvaluation(
            *cols, observation=torch.empty((self._batch,) + self._obs_shape, dtype=torch.float32, device=self._device))
      self._evaluation_ptrs = (_native.PolicyEvalPtrs if grid else _native.LinearEvalPtrs)(*[t.data_ptr() for t in ev])
    return ev, self._evaluation_ptrs

  _closed_loop_fixed = None   # the arguments that are the same in every launch: _launch_closed_loop

  def _launch_closed_loop(self, what, policy, beta, T, out, actions):
    """Calls the entry point of `what`: configuration, call descriptor, policy struct, [beta,] the state columns, the outputs,
    [the action tensor,] info.  The grids carry the action tensor — and the beta of a drawn call — inside the policy struct;
    the physics families pass beta after the struct and the action tensor as an argument of its own after the outputs."""
    fixed = self._closed_loop_fixed
    if fixed is None:          # (once allocated, the state and info columns never move: load_state_dict copies in place)
      fixed = self._closed_loop_fixed = ((ctypes.byref(self._cfg), ctypes.byref(self._call_desc)),
                                         tuple(t.data_ptr() for t in self._state.values()), self._info.data_ptr())
    head, state, info = fixed
    if what in _GRID_CALLS:
      if actions is not None:
        policy.actions_out = actions.data_ptr()
      args = head + (ctypes.byref(policy),) + state + (out, info)
    elif beta is None:
      args = head + (ctypes.byref(policy),) + state + ((out, info) if actions is None else (out, actions.data_ptr(), info))
    else:
      args = head + (ctypes.byref(policy), beta) + state + ((out, info) if actions is None else (out, actions.data_ptr(), info))
    self._launch_steps(getattr(_native.lib, self._closed_loop_abi(what)), args, T, what)

  def _record(self, what, policy, num_steps, beta=None):
    """The recording calls, once their arguments are checked: the [T,B] outputs and the action tensor — one set per T, shared
    by all the recording calls of the family, _new_outputs((T, B), ...) + the action tensor — and the launch.  Returns
    `(timestep, actions)`."""
    if what not in _GRID_CALLS:
      self._check_trajectory_slab(what)
    self._ensure_allocated()
    T = int(num_steps)
    if T not in self._policy_rollout_out:
      actions = torch.empty((T, self._batch), dtype=torch.int32, device=self._device)
      self._policy_rollout_out[T] = self._new_outputs((T, self._batch), dict(device=self._device)) + (actions,)
    _, ptrs, timestep, actions = self._policy_rollout_out[T]
    self._launch_closed_loop(what, policy, beta, T, ptrs, actions)
    return timestep, actions

  def _evaluate(self, what, policy, num_steps, beta=None):
    """The returns-only calls, once their arguments are checked: the cached result columns and the launch.  Returns the
    evaluation tuple."""
    self._ensure_allocated()
    ev, out = self._evaluation_out(what in _GRID_CALLS)
    self._launch_closed_loop(what, policy, beta, int(num_steps), out, None)
    return ev

  # ----------------------------------------------------------------------------------------
  # the grids: a table of actions or of logits
  def _check_rollout_policy(self, policy, num_steps, policy_index, epsilon, explore_seed, what='rollout_policy'):
    """The refusals of rollout_policy() and evaluate_policy() (`what`): all of them before any GPU use, nothing allocated.
    The environment's part, epsilon and its seed, then the table of actions' own."""
    self._check_closed_loop_env(what, num_steps)
    self._check_epsilon(what, epsilon, explore_seed)
    S = self.policy_num_states
    if (not torch.is_tensor(policy) or policy.dtype != torch.uint8 or policy.device != self._device or policy.dim() not in (1, 2)
        or int(policy.shape[-1]) != S or policy.numel() == 0 or not policy.is_contiguous()):
      raise ValueError(f'{what}: policy must be a contiguous uint8 tensor of shape ({S},) or (P, {S}) on {self._device}')
    P = 1 if policy.dim() == 1 else int(policy.shape[0])
    self._check_population(what, P, policy_index)
    return P

  def _check_sample_policy(self, logits, num_steps, policy_index, temperature, sample_seed, what):
    """The refusals of sample_policy() and evaluate_sampled_policy() (`what`), all before any GPU use: the environment's part,
    the table of logits, then the temperature and the seed (_check_sample).  Returns (P, beta)."""
    self._check_closed_loop_env(what, num_steps)
    S, A = self.policy_num_states, int(self._num_actions)
    if (not torch.is_tensor(logits) or logits.dtype != torch.float32 or logits.device != self._device or logits.dim() not in (2, 3)
        or tuple(logits.shape[-2:]) != (S, A) or logits.numel() == 0 or not logits.is_contiguous()):
      raise ValueError(f'{what}: logits must be a contiguous float32 tensor of shape ({S}, {A}) or (P, {S}, {A}) on {self._device}')
    P = 1 if logits.dim() == 2 else int(logits.shape[0])
    self._check_population(what, P, policy_index)
    return P, self._check_sample(what, temperature, sample_seed)

  def _policy_table(self, policy, P, policy_index, epsilon, explore_seed):
    return _native.Policy(policy.data_ptr(), self.policy_num_states, P,
                          policy_index.data_ptr() if policy_index is not None else None, float(epsilon), int(explore_seed), None)

  def _policy_logits(self, logits, P, policy_index, beta, sample_seed):
    return _native.PolicyLogits(logits.data_ptr(), self.policy_num_states, int(self._num_actions), P,
                                policy_index.data_ptr() if policy_index is not None else None, beta, int(sample_seed), None)

  def rollout_policy(self, policy, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """A closed-loop rollout of `num_steps` steps in ONE launch, the actions looked up in a table by the lane's own
    observation (DeepSea and Catch, batched view, observation_mode='index', counter-based draws, no wrapper).

    policy: uint8 device tensor [S] (one table for all lanes) or [P, S] (a population; `policy_index`, int32 [B], names
    each lane's row and is clamped to [0, P-1]); S = `policy_num_states`; entry k is the action taken when the lane's
    observation has key k (utils.observations.policy_key).  Returns `(ts, actions)`: `ts` as rollout() returns it
    ([T,B] step_type / reward / discount, [T,B,K] int32 observation) and `actions` int32 [T,B], the actions taken.  The
    result equals, bit for bit,

        for t in range(T): a = 0 where the lane resets on this call, else policy[row, key(observation before the call)]
                           step(a)

    — a lane resets when it is fresh, after LAST, or marked by mark_reset(); actions[t] is 0 there.  A table entry outside
    the action_spec behaves as the same value passed to step().  With epsilon > 0 a lane that does not reset draws U()
    and, if U < epsilon, takes RandInt(num_actions) instead: stream 2 of (explore_seed, global lane id, call index)
    (include/bsx_stream.h); the environment's own draws are untouched.  State, info, counters and the call index are
    left as T step() calls leave them; calls interleave freely with step / rollout / mark_reset / reset.  Output buffers
    are cached per T and overwritten by the next call of the same T."""
    P = self._check_rollout_policy(policy, num_steps, policy_index, epsilon, explore_seed)
    return self._record('rollout_policy', self._policy_table(policy, P, policy_index, epsilon, explore_seed), num_steps)

  def evaluate_policy(self, policy, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """`rollout_policy` with the same arguments, returns only: the lanes take the same `num_steps` steps in ONE launch — same
    actions, draws, keys and clamps — and state, bsuite_info(), episode_counters(), invalid_action_count() and the call
    index are left bit for bit where rollout_policy leaves them, but no TimeStep is written.  Returns a `PolicyEvaluation`
    of three device tensors [B], per lane over the steps of this call in order, in float64:

        acc = done = total = 0.0; n = 0
        for t in range(T):                      # type_t, r_t: step type and reward of step t
          if type_t != FIRST: acc += r_t; total += r_t
          if type_t == LAST:  done += acc; acc = 0.0; n += 1
        episodes = n (int32); return_sum = total; episode_return_sum = done

    r_t is the float64 reward of the step BEFORE the rounding to float32 that a TimeStep's reward gets: return_sum is what
    the reference's run loop sums from `timestep.reward` as Python floats (for deep_sea it differs from the sum of
    rollout_policy's float32 rewards).  The mean episode return of a lane is episode_return_sum / episodes.  An episode
    that is already running when the call starts contributes only the rewards of this call to episode_return_sum; after
    mark_reset() of all lanes, reset() or on a fresh environment there is none.  Nothing is reduced over lanes on the
    device (float64 atomics have no fixed order): to score a population, reduce on the lanes grouped by policy, e.g.
    `torch.zeros(P, dtype=torch.float64, device=...).index_add_(0, policy_index.long(), ev.episode_return_sum)`.  The three
    buffers are cached per environment and overwritten by the next call.  Calls interleave freely with step / rollout /
    rollout_policy / mark_reset / reset."""
    P = self._check_rollout_policy(policy, num_steps, policy_index, epsilon, explore_seed, what='evaluate_policy')
    return self._evaluate('evaluate_policy', self._policy_table(policy, P, policy_index, epsilon, explore_seed), num_steps)

  def sample_policy(self, logits, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`rollout_policy` for a learner whose tabular policy is a softmax (REINFORCE, actor-critic, softmax population search):
    a closed-loop rollout of `num_steps` steps in ONE launch, the actions DRAWN from softmax(logits[row, key] / temperature)
    (DeepSea and Catch, batched view, observation_mode='index', counter-based draws, no wrapper).

    logits: a contiguous float32 device tensor [S, A] (one table for all lanes) or [P, S, A] (a population; `policy_index`,
    int32 [B], names each lane's row and is clamped to [0, P-1]; with one table it must be None); S = `policy_num_states`,
    A = action_spec().num_values (deep_sea 2, catch 3).  Only 4-byte alignment is assumed: a view that starts one float into
    a buffer is fine.  Returns `(ts, actions)` as rollout_policy does — `ts` with step_type int8 / reward / discount float32
    [T,B] and the int32 index observation [T,B,K], `actions` int32 [T,B] — and equals, bit for bit in everything it returns
    and everything it leaves behind,

        for t in range(T): a = 0 where the lane resets on this call, else
                               gumbel_select(logits[row, key(observation before the call)], words(sample_seed, lane, call index),
                                             temperature)
                           ts[t] = step(a); actions[t] = a

    key is utils.observations.policy_key (clamped into the table like rollout_policy's), gumbel_select is
    utils.observations': Gumbel-max in float64 over the A logits — u_a = (word_a + 0.5) * 2^-32, g_a = -log(-log(u_a)) with the
    engine's bit-reproducible logarithm, z_a = l_a * (1 / temperature) + g_a, the largest z wins, the lowest index wins a
    tie, a NaN never wins and a -inf logit masks its action — which draws action a with probability
    softmax(logits / temperature)[a].  The words are words 0..A-1 of block 0 of stream 3 of (sample_seed, global lane id, call
    index); nothing is drawn on a step that resets, and the environment's own stream 0 is untouched, so `rollout(actions)` on
    a twin reproduces `ts`.  temperature: a finite number > 0 whose inverse is finite; there is no epsilon and no greedy
    limit (that is rollout_policy).  Log-probabilities are not outputs: a learner gathers `logits[row, key]` itself.  A shared
    table of at most 12 KiB (every catch up to rows * columns^2 = 1024, deep_sea up to N = 39) is kept on chip; a larger one
    and every population is read from device memory.  State, bsuite_info(), episode_counters(), invalid_action_count() and the
    call index are left as T step() calls leave them; calls interleave freely with step / rollout / rollout_policy /
    evaluate_policy / mark_reset / reset.  Output buffers are cached per T, shared with rollout_policy(), and overwritten by
    the next call of the same T."""
    what = 'sample_policy'
    P, beta = self._check_sample_policy(logits, num_steps, policy_index, temperature, sample_seed, what)
    return self._record(what, self._policy_logits(logits, P, policy_index, beta, sample_seed), num_steps)

  def evaluate_sampled_policy(self, logits, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`sample_policy` with the same arguments, returns only: the lanes take the same `num_steps` steps with the same draws in
    ONE launch, and state, bsuite_info(), episode_counters(), invalid_action_count() and the call index are left bit for bit
    where sample_policy leaves them, but no TimeStep is written.  Returns the cached `PolicyEvaluation` of evaluate_policy —
    episodes int32, return_sum and episode_return_sum float64, [B] each — with the same definitions: the float64 reward of
    the step before its rounding to float32, summed in step order (evaluate_policy has the loop).  The refusals are
    sample_policy's.  The three buffers are shared with evaluate_policy() and overwritten by the next call of either."""
    what = 'evaluate_sampled_policy'
    P, beta = self._check_sample_policy(logits, num_steps, policy_index, temperature, sample_seed, what)
    return self._evaluate(what, self._policy_logits(logits, P, policy_index, beta, sample_seed), num_steps)

  # ----------------------------------------------------------------------------------------
  # the grids: a pair of matrices whose first layer is a row gather on the index observation
  def _check_embedding(self, w1, w2, num_steps, policy_index, epsilon, explore_seed, what):
    """The refusals of rollout_embedding() and evaluate_embedding() (`what`), all before any GPU use, nothing allocated: the
    environment's part (_check_closed_loop_env), the pair of matrices, the population rule, then epsilon and the seed as
    _check_rollout_policy refuses them.  Returns (P, H)."""
    self._check_closed_loop_env(what, num_steps)
    C, A = int(np.prod(self._board_shape)), int(self._num_actions)
    ok = lambda w: torch.is_tensor(w) and w.dtype == torch.float32 and w.device == self._device and w.numel() > 0 and w.is_contiguous()
    H = int(w1.shape[-1]) if ok(w1) and w1.dim() in (2, 3) else 0
    if (not ok(w1) or not ok(w2) or w1.dim() not in (2, 3) or w2.dim() != w1.dim() or not 1 <= H <= _native.MLP_MAX_HIDDEN
        or tuple(w1.shape[-2:]) != (C + 2, H) or tuple(w2.shape[-2:]) != (A, H + 1) or w1.shape[:-2] != w2.shape[:-2]):
      raise ValueError(f'{what}: w1 and w2 must be contiguous float32 tensors of shapes ({C + 2}, H) and ({A}, H + 1), or '
                       f'(P, {C + 2}, H) and (P, {A}, H + 1), with 1 <= H <= {_native.MLP_MAX_HIDDEN}, on {self._device}')
    P = 1 if w1.dim() == 2 else int(w1.shape[0])
    self._check_population(what, P, policy_index)
    self._check_epsilon(what, epsilon, explore_seed)
    return P, H

  def _policy_embedding(self, w1, w2, P, H, policy_index, epsilon, explore_seed):
    return _native.PolicyEmbedding(w1.data_ptr(), w2.data_ptr(), int(np.prod(self._board_shape)), H, int(self._num_actions), P,
                                   policy_index.data_ptr() if policy_index is not None else None, float(epsilon),
                                   int(explore_seed), None)

  def rollout_embedding(self, w1, w2, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """`rollout_policy` for an agent whose policy is a small network on the one-hot board (a DQN actor, an ES / CEM population of
    networks): a closed-loop rollout of `num_steps` steps in ONE launch, the actions the greedy — with `epsilon`, epsilon-greedy
    — choice of a network with one ReLU hidden layer whose first layer is a row gather on the lane's own index observation
    (DeepSea and Catch, batched view, observation_mode='index', counter-based draws, no wrapper).

    With C the cells of `board_shape`, K the entries of an index row (deep_sea 1, catch 2), A = action_spec().num_values
    (deep_sea 2, catch 3) and H hidden units, 1 <= H <= 64: `w1` is a contiguous float32 device tensor [C + 2, H] — row c + 1 the
    embedding of cell c, row 0 the row a -1 entry selects (utils.observations.index_embedding's layout, so
    `index_embedding(obs, w1)` stays usable as it is), row C + 1 the hidden bias — and `w2` float32 [A, H + 1], the bias in the
    last column (evaluate_mlp's `w2`).  A population is [P, C + 2, H] and [P, A, H + 1] with `policy_index`, int32 [B], naming
    each lane's pair (clamped to [0, P-1]; with one pair it must be None).  Only 4-byte alignment is assumed: a view that
    starts one float into a buffer is fine.  Returns `(ts, actions)` as rollout_policy does and equals, bit for bit in
    everything it returns and everything it leaves behind,

        for t in range(T): a = 0 where the lane resets on this call, else select(observation before the call)
                           ts[t] = step(a); actions[t] = a

    select is utils.observations.embedding_select followed by rollout_policy's epsilon coin — float32, every add and every
    multiply rounded on its own (csrc/bsx_embed.h):

        l_a = w2[a][H]
        for j in range(H): s = w1[C+1][j]; for k in range(K): s = s + w1[cell_k + 1][j]
                           h = s if s > 0 else +0.0;  l_a = l_a + w2[a][j] * h
        best = 0; for a in 1..A-1: if l_a > l_best: best = a          the lowest index wins a tie, a NaN never wins

    cell_k is entry k of the index row in order (catch: ball, then paddle; the same cell twice is added twice), clamped to
    [-1, C-1].  With epsilon > 0 a lane that does not reset draws U() and, if U < epsilon, takes RandInt(A) instead: stream 2 of
    (explore_seed, global lane id, call index), word for word rollout_policy's rule; nothing is computed or drawn on a step
    that resets, and the environment's own stream 0 is untouched, so `rollout(actions)` on a twin reproduces `ts`.  A shared
    pair whose on-chip copy fits 15 KiB (catch/0 up to H = 64, deep_sea N = 10 up to H = 32) is kept on chip; a larger one and
    every population is read from device memory.  State, bsuite_info(), episode_counters(), invalid_action_count() and the call
    index are left as T step() calls leave them; calls interleave freely with step / rollout / rollout_policy /
    evaluate_policy / sample_policy / mark_reset / reset.  Output buffers are cached per T, shared with rollout_policy(), and
    overwritten by the next call of the same T."""
    what = 'rollout_embedding'
    P, H = self._check_embedding(w1, w2, num_steps, policy_index, epsilon, explore_seed, what)
    return self._record(what, self._policy_embedding(w1, w2, P, H, policy_index, epsilon, explore_seed), num_steps)

  def evaluate_embedding(self, w1, w2, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """`rollout_embedding` with the same arguments, returns only: the lanes take the same `num_steps` steps with the same draws
    in ONE launch, and state, bsuite_info(), episode_counters(), invalid_action_count() and the call index are left bit for bit
    where rollout_embedding leaves them, but no TimeStep is written.  Returns the cached `PolicyEvaluation` of evaluate_policy
    — episodes int32, return_sum and episode_return_sum float64, [B] each — with the same definitions: the float64 reward of
    the step before its rounding to float32, summed in step order (evaluate_policy has the loop).  The refusals are
    rollout_embedding's.  The three buffers are shared with evaluate_policy() and overwritten by the next call of either."""
    what = 'evaluate_embedding'
    P, H = self._check_embedding(w1, w2, num_steps, policy_index, epsilon, explore_seed, what)
    return self._evaluate(what, self._policy_embedding(w1, w2, P, H, policy_index, epsilon, explore_seed), num_steps)

  def _check_sample_embedding(self, w1, w2, num_steps, policy_index, temperature, sample_seed, what):
    """The refusals of sample_embedding() and evaluate_sampled_embedding() (`what`), all before any GPU use, nothing allocated:
    _check_embedding's — the environment's part (_check_closed_loop_env), the pair of matrices, the population rule — without
    an epsilon, then the temperature and the seed as _check_sample_policy refuses them (_check_sample).  Returns (P, H, beta)."""
    P, H = self._check_embedding(w1, w2, num_steps, policy_index, 0.0, 0, what)
    return P, H, self._check_sample(what, temperature, sample_seed)

  def _policy_embedding_sample(self, w1, w2, P, H, policy_index, beta, sample_seed):
    return _native.PolicyEmbeddingSample(w1.data_ptr(), w2.data_ptr(), int(np.prod(self._board_shape)), H, int(self._num_actions), P,
                                         policy_index.data_ptr() if policy_index is not None else None, beta, int(sample_seed),
                                         None)

  def sample_embedding(self, w1, w2, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`rollout_embedding` for a learner that needs actions DRAWN from its network (REINFORCE, actor-critic, PPO on deep_sea or
    catch): a closed-loop rollout of `num_steps` steps in ONE launch, the actions drawn from softmax(logits / temperature) of
    a network with one ReLU hidden layer whose first layer is a row gather on the lane's own index observation (DeepSea and
    Catch, batched view, observation_mode='index', counter-based draws, no wrapper).

    `w1`, `w2` and `policy_index` are rollout_embedding's: with C the cells of `board_shape`, A = action_spec().num_values and
    H hidden units, 1 <= H <= 64, contiguous float32 device tensors [C + 2, H] and [A, H + 1], or a population [P, C + 2, H]
    and [P, A, H + 1] with `policy_index`, int32 [B], naming each lane's pair (clamped to [0, P-1]; with one pair it must be
    None).  Only 4-byte alignment is assumed.  Returns `(ts, actions)` as rollout_policy does and equals, bit for bit in
    everything it returns and everything it leaves behind,

        for t in range(T): a = 0 where the lane resets on this call, else
                               gumbel_select(embedding_logits(w1, w2, observation before the call),
                                             words(sample_seed, lane, call index), temperature)
                           ts[t] = step(a); actions[t] = a

    embedding_logits and gumbel_select are utils.observations': the float32 logits of rollout_embedding (every add and every
    multiply rounded on its own, cells clamped to [-1, C-1]; csrc/bsx_embed.h), then Gumbel-max in float64 over the A logits —
    u_a = (word_a + 0.5) * 2^-32, g_a = -log(-log(u_a)) with the engine's bit-reproducible logarithm,
    z_a = l_a * (1 / temperature) + g_a, the largest z wins, the lowest index wins a tie, a NaN never wins and a -inf logit
    masks its action — which draws action a with probability softmax(logits / temperature)[a].  The words are words 0..A-1 of
    block 0 of stream 3 of (sample_seed, global lane id, call index); nothing is computed or drawn on a step that resets, and
    the environment's own stream 0 is untouched, so `rollout(actions)` on a twin reproduces `ts`.  temperature: a finite
    number > 0 whose inverse is finite; there is no epsilon and no greedy limit (that is rollout_embedding).
    Log-probabilities are not outputs: a learner computes `embedding_logits` of the returned observations itself.  The 15 KiB
    on-chip rule for a shared pair is rollout_embedding's.  State, bsuite_info(), episode_counters(), invalid_action_count()
    and the call index are left as T step() calls leave them; calls interleave freely with step / rollout / rollout_policy /
    sample_policy / rollout_embedding / evaluate_embedding / mark_reset / reset.  Output buffers are cached per T, shared with
    rollout_policy(), and overwritten by the next call of the same T."""
    what = 'sample_embedding'
    P, H, beta = self._check_sample_embedding(w1, w2, num_steps, policy_index, temperature, sample_seed, what)
    return self._record(what, self._policy_embedding_sample(w1, w2, P, H, policy_index, beta, sample_seed), num_steps)

  def evaluate_sampled_embedding(self, w1, w2, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`sample_embedding` with the same arguments, returns only: the lanes take the same `num_steps` steps with the same draws
    in ONE launch, and state, bsuite_info(), episode_counters(), invalid_action_count() and the call index are left bit for bit
    where sample_embedding leaves them, but no TimeStep is written.  Returns the cached `PolicyEvaluation` of evaluate_policy
    — episodes int32, return_sum and episode_return_sum float64, [B] each — with the same definitions: the float64 reward of
    the step before its rounding to float32, summed in step order (evaluate_policy has the loop).  The refusals are
    sample_embedding's.  The three buffers are shared with evaluate_policy() and overwritten by the next call of either."""
    what = 'evaluate_sampled_embedding'
    P, H, beta = self._check_sample_embedding(w1, w2, num_steps, policy_index, temperature, sample_seed, what)
    return self._evaluate(what, self._policy_embedding_sample(w1, w2, P, H, policy_index, beta, sample_seed), num_steps)

  # ----------------------------------------------------------------------------------------
  # the physics families: one, two or three weight matrices on the float observation rows
  def _is_eval_weight(self, w, dims, tail):
    """A contiguous, non-empty float32 tensor on the environment's device with `dims` dimensions, the last two `tail`."""
    return (torch.is_tensor(w) and w.dtype == torch.float32 and w.device == self._device and w.dim() in dims
            and tuple(w.shape[-2:]) == tail and w.numel() != 0 and w.is_contiguous())

  def _check_fused_eval_rows(self, what, observation, P, policy_index, noun, one):
    """What the physics calls refuse after their weights: the observation rows, then the population rule.  Returns P."""
    D = int(np.prod(self._obs_shape))
    if (not torch.is_tensor(observation) or observation.dtype != torch.float32 or observation.device != self._device
        or tuple(observation.shape) not in ((self._batch,) + self._obs_shape, (self._batch, D)) or not observation.is_contiguous()):
      raise ValueError(f'{what}: observation must be a contiguous float32 tensor of shape {(self._batch,) + self._obs_shape} or '
                       f'({self._batch}, {D}) on {self._device}: the observation of the last TimeStep')
    self._check_population(what, P, policy_index, noun, one)
    return P

  def _check_evaluate_linear(self, weights, observation, num_steps, policy_index, epsilon, explore_seed, what='evaluate_linear'):
    """The refusals of evaluate_linear() and rollout_linear() (`what`): all of them before any GPU use, nothing allocated."""
    self._check_closed_loop_env(what, num_steps)
    self._check_epsilon(what, epsilon, explore_seed)
    A, D = self._num_actions, int(np.prod(self._obs_shape))
    if not self._is_eval_weight(weights, (2, 3), (A, D + 1)):
      raise ValueError(f'{what}: weights must be a contiguous float32 tensor of shape ({A}, {D + 1}) or (P, {A}, {D + 1}) on '
                       f'{self._device} (column {D} is the bias)')
    P = 1 if weights.dim() == 2 else int(weights.shape[0])
    return self._check_fused_eval_rows(what, observation, P, policy_index, 'weight matrices', 'matrix')

  def _linear_struct(self, weights, P, policy_index, epsilon, explore_seed, observation):
    return _native.Linear(weights.data_ptr(), P, policy_index.data_ptr() if policy_index is not None else None, float(epsilon),
                          int(explore_seed), observation.data_ptr())

  def evaluate_linear(self, weights, observation, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """The closed loop of a linear agent in ONE launch, returns only (Cartpole, CartpoleSwingup and MountainCar, batched
    view, counter-based draws, no wrapper).  The call equals, bit for bit in everything it leaves behind and returns,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else select(weights[row], obs)
                           ts = step(a); obs = ts.observation

    weights: float32 device tensor [A, D+1] (one matrix for all lanes) or [P, A, D+1] (a population; `policy_index`, int32
    [B], names each lane's matrix and is clamped to [0, P-1]); A = 3 actions, D the observation length (mountain_car 3,
    cartpole 6, swing-up 8), column D the bias.  select is utils.observations.linear_select: l_a = w[a][D], then
    l_a = l_a + w[a][d] * obs[d] for d = 0..D-1 in float32 with every multiply and add rounded on its own; the largest
    logit wins, the lowest index wins a tie, a NaN never wins.  With epsilon > 0 a lane that does not reset draws U() and,
    if U < epsilon, takes RandInt(3) instead: stream 2 of (explore_seed, global lane id, call index), as in rollout_policy.
    observation: float32 device tensor [B, *obs_shape] or [B, D], the observation of the last TimeStep — from reset(),
    step(), rollout(...).observation[-1] or a previous result's `.observation` (it is an argument because cartpole's observed
    sine / cosine are carried from step to step, not recomputed from the stored angle).  A lane that resets on the first
    step — fresh, after LAST, marked by mark_reset() — never reads its row.  Returns `LinearEvaluation(episodes int32 [B],
    return_sum f64 [B], episode_return_sum f64 [B], observation f32 [B, *obs_shape])`: the three columns as
    evaluate_policy() defines them, from the float64 reward of each step, and the observation of step T-1, written once
    after the loop.  The buffers are cached per environment and overwritten by the next call; passing `.observation` back
    in is legal.  State, bsuite_info(), episode_counters() and the call index are left as T step() calls with the same
    actions leave them; calls interleave freely with step / rollout / mark_reset / reset."""
    P = self._check_evaluate_linear(weights, observation, num_steps, policy_index, epsilon, explore_seed)
    lin = self._linear_struct(weights, P, policy_index, epsilon, explore_seed, observation)
    return self._evaluate('evaluate_linear', lin, num_steps)

  def _check_evaluate_mlp(self, w1, w2, observation, num_steps, policy_index, epsilon, explore_seed, what='evaluate_mlp'):
    """The refusals of evaluate_mlp() and rollout_mlp() (`what`): all of them before any GPU use, nothing allocated.  Returns
    (P, H)."""
    self._check_closed_loop_env(what, num_steps)
    self._check_epsilon(what, epsilon, explore_seed)
    A, D, Hmax = self._num_actions, int(np.prod(self._obs_shape)), _native.MLP_MAX_HIDDEN
    H = int(w1.shape[-2]) if torch.is_tensor(w1) and w1.dim() in (2, 3) else 0
    if not 1 <= H <= Hmax or not self._is_eval_weight(w1, (2, 3), (H, D + 1)):
      raise ValueError(f'{what}: w1 must be a contiguous float32 tensor of shape (H, {D + 1}) or (P, H, {D + 1}) on {self._device} '
                       f'with 1 <= H <= {Hmax} hidden units (column {D} is the bias)')
    if not self._is_eval_weight(w2, (w1.dim(),), (A, H + 1)) or (w1.dim() == 3 and int(w2.shape[0]) != int(w1.shape[0])):
      lead = '' if w1.dim() == 2 else f'{int(w1.shape[0])}, '
      raise ValueError(f'{what}: w2 must be a contiguous float32 tensor of shape ({lead}{A}, {H + 1}) on {self._device}, the '
                       f'same population and hidden width as w1 (column {H} is the bias)')
    P = 1 if w1.dim() == 2 else int(w1.shape[0])
    return self._check_fused_eval_rows(what, observation, P, policy_index, 'weight pairs', 'pair'), H

  def _mlp_struct(self, w1, w2, H, P, policy_index, epsilon, explore_seed, observation):
    return _native.Mlp(w1.data_ptr(), w2.data_ptr(), H, P, policy_index.data_ptr() if policy_index is not None else None,
                       float(epsilon), int(explore_seed), observation.data_ptr())

  def evaluate_mlp(self, w1, w2, observation, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """`evaluate_linear` for an agent with one ReLU hidden layer: the same ONE launch, the same contract, result type and
    refusals, with another greedy action.  The call equals, bit for bit in everything it leaves behind and returns,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else mlp_select(w1[row], w2[row], obs)
                           ts = step(a); obs = ts.observation

    w1: float32 device tensor [H, D+1] (one pair for all lanes) or [P, H, D+1]; w2: [3, H+1] or [P, 3, H+1] — the same P and
    the same H, 1 <= H <= 64, the bias in the last column of each.  With a population, `policy_index` (int32 [B], clamped to
    [0, P-1]) names each lane's pair; with 2-D weights it must be None.  mlp_select is utils.observations.mlp_select:
    l_a = w2[a][H]; for every hidden unit j: s = w1[j][D], then s = s + w1[j][d] * obs[d] for d = 0..D-1, h = s if s > 0 else
    +0.0 (a NaN pre-activation gives 0), l_a = l_a + w2[a][j] * h — float32, every multiply and add rounded on its own; the
    largest logit wins, the lowest index wins a tie, a NaN never wins.  epsilon, explore_seed, `observation` and the returned
    `LinearEvaluation` are evaluate_linear's; the result buffers are the ones evaluate_linear uses, so `.observation` of either
    call may be passed into either.  A shared pair is kept on chip.  A population is read from device memory by every lane on
    every step: group the lanes by policy (policy_index non-decreasing) — the lanes of a wave then share their loads; a
    shuffled policy_index is legal and slower.  State, bsuite_info(), episode_counters() and the call index are left as T
    step() calls with the same actions leave them; calls interleave freely with step / rollout / evaluate_linear /
    mark_reset / reset."""
    P, H = self._check_evaluate_mlp(w1, w2, observation, num_steps, policy_index, epsilon, explore_seed)
    mlp = self._mlp_struct(w1, w2, H, P, policy_index, epsilon, explore_seed, observation)
    return self._evaluate('evaluate_mlp', mlp, num_steps)

  def rollout_linear(self, weights, observation, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """`evaluate_linear` with the same arguments, recorded: the closed loop of a linear agent in ONE launch that writes the
    trajectory (Cartpole, CartpoleSwingup and MountainCar, batched view, counter-based draws, no wrapper).  Returns
    `(ts, actions)`: `ts` as rollout() returns it — step_type int8 [T,B], reward / discount float32 [T,B], observation
    float32 [T,B,*obs_shape] — and `actions` int32 [T,B], the action taken at every step, epsilon draws included, 0 where
    the lane resets.  The call equals, bit for bit in everything it returns and everything it leaves behind,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else linear_select(weights[row], obs)
                           ts[t] = step(a); actions[t] = a; obs = ts[t].observation

    so `rollout(actions)` on a twin reproduces `ts`, and a twin's evaluate_linear() with the same arguments ends in the same
    state with `.observation == ts.observation[-1]` and `.episodes == (ts.step_type == LAST).sum(0)`.  weights, observation,
    policy_index, epsilon and explore_seed are evaluate_linear's: the same shapes and population form, the same stream 2 of
    (explore_seed, global lane id, call index), nothing drawn with epsilon == 0 or on a step that resets, and a lane that
    resets on the first step never reads its row of `observation`.  Logits and log-probabilities are not outputs: a learner
    recomputes them from `ts.observation` and `actions` (utils.observations.linear_select has the rule).  State,
    bsuite_info(), episode_counters() and the call index are left as T step() calls leave them; calls interleave freely with
    step / rollout / evaluate_linear / evaluate_mlp / rollout_mlp / mark_reset / reset.  Output buffers are cached per T,
    shared with rollout_mlp(), and overwritten by the next call of the same T."""
    what = 'rollout_linear'
    P = self._check_evaluate_linear(weights, observation, num_steps, policy_index, epsilon, explore_seed, what=what)
    return self._record(what, self._linear_struct(weights, P, policy_index, epsilon, explore_seed, observation), num_steps)

  def rollout_mlp(self, w1, w2, observation, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """`rollout_linear` for an agent with one ReLU hidden layer — `evaluate_mlp` with the same arguments, recorded: the same
    ONE launch, the same `(ts, actions)`, contract and refusals, with another greedy action.  The call equals, bit for bit in
    everything it returns and everything it leaves behind,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else mlp_select(w1[row], w2[row], obs)
                           ts[t] = step(a); actions[t] = a; obs = ts[t].observation

    w1: float32 device tensor [H, D+1] or [P, H, D+1]; w2: [3, H+1] or [P, 3, H+1], 1 <= H <= 64; `policy_index`, epsilon,
    explore_seed and `observation` as in evaluate_mlp (utils.observations.mlp_select has the rule).  A shared pair is kept on
    chip; a population is read from device memory by every lane on every step: group the lanes by policy.  `rollout(actions)`
    on a twin reproduces `ts`; a twin's evaluate_mlp() with the same arguments ends in the same state.  Output buffers are
    cached per T, shared with rollout_linear(), and overwritten by the next call of the same T."""
    what = 'rollout_mlp'
    P, H = self._check_evaluate_mlp(w1, w2, observation, num_steps, policy_index, epsilon, explore_seed, what=what)
    return self._record(what, self._mlp_struct(w1, w2, H, P, policy_index, epsilon, explore_seed, observation), num_steps)

  def _check_evaluate_mlp2(self, w1, w2, w3, observation, num_steps, policy_index, epsilon, explore_seed, what='evaluate_mlp2'):
    """The refusals of evaluate_mlp2() and rollout_mlp2() (`what`): all of them before any GPU use, nothing allocated.  Returns
    (P, H1, H2)."""
    self._check_closed_loop_env(what, num_steps)
    self._check_epsilon(what, epsilon, explore_seed)
    A, D, Hmax = self._num_actions, int(np.prod(self._obs_shape)), _native.MLP_MAX_HIDDEN
    H1 = int(w1.shape[-2]) if torch.is_tensor(w1) and w1.dim() in (2, 3) else 0
    if not 1 <= H1 <= Hmax or not self._is_eval_weight(w1, (2, 3), (H1, D + 1)):
      raise ValueError(f'{what}: w1 must be a contiguous float32 tensor of shape (H1, {D + 1}) or (P, H1, {D + 1}) on {self._device} '
                       f'with 1 <= H1 <= {Hmax} hidden units (column {D} is the bias)')
    lead = '' if w1.dim() == 2 else f'{int(w1.shape[0])}, '
    same_p = lambda w: w1.dim() == 2 or int(w.shape[0]) == int(w1.shape[0])   # pylint: disable=unnecessary-lambda-assignment
    H2 = int(w2.shape[-2]) if torch.is_tensor(w2) and w2.dim() == w1.dim() else 0
    if not 1 <= H2 <= Hmax or not self._is_eval_weight(w2, (w1.dim(),), (H2, H1 + 1)) or not same_p(w2):
      raise ValueError(f'{what}: w2 must be a contiguous float32 tensor of shape ({lead}H2, {H1 + 1}) on {self._device} with '
                       f'1 <= H2 <= {Hmax} hidden units, the same population as w1 and its hidden width (column {H1} is the bias)')
    if not self._is_eval_weight(w3, (w1.dim(),), (A, H2 + 1)) or not same_p(w3):
      raise ValueError(f'{what}: w3 must be a contiguous float32 tensor of shape ({lead}{A}, {H2 + 1}) on {self._device}, the '
                       f'same population as w1 and the hidden width of w2 (column {H2} is the bias)')
    P = 1 if w1.dim() == 2 else int(w1.shape[0])
    return self._check_fused_eval_rows(what, observation, P, policy_index, 'weight triples', 'triple'), H1, H2

  def _mlp2_struct(self, w1, w2, w3, H1, H2, P, policy_index, epsilon, explore_seed, observation):
    return _native.Mlp2(w1.data_ptr(), w2.data_ptr(), w3.data_ptr(), H1, H2, P,
                        policy_index.data_ptr() if policy_index is not None else None, float(epsilon), int(explore_seed),
                        observation.data_ptr())

  def evaluate_mlp2(self, w1, w2, w3, observation, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """`evaluate_mlp` for an agent with TWO ReLU hidden layers — the shape of the reference agents' networks
    (`MLP([64, 64])` plus a head): the same ONE launch, the same contract, result type and refusals, with another greedy
    action.  The call equals, bit for bit in everything it leaves behind and returns,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else mlp2_select(w1[row], w2[row], w3[row], obs)
                           ts = step(a); obs = ts.observation

    w1: float32 device tensor [H1, D+1] (one triple for all lanes) or [P, H1, D+1]; w2: [H2, H1+1] or [P, H2, H1+1]; w3:
    [3, H2+1] or [P, 3, H2+1] — the same P, 1 <= H1, H2 <= 64, the bias in the last column of each: the layout is
    `torch.cat([lin.weight, lin.bias[:, None]], 1)` of a `torch.nn.Linear`.  With a population, `policy_index` (int32 [B],
    clamped to [0, P-1]) names each lane's triple; with 2-D weights it must be None.  mlp2_select is
    utils.observations.mlp2_select: h1_j = relu(w1[j][D] + sum_d w1[j][d] * obs[d]), s2_k = w2[k][H1] + sum_j w2[k][j] * h1_j
    (j ascending), h2_k = relu(s2_k), l_a = w3[a][H2] + sum_k w3[a][k] * h2_k — float32, every multiply and add rounded on its
    own, relu(s) = s if s > 0 else +0.0 (a NaN pre-activation gives 0); the largest logit wins, the lowest index wins a tie,
    a NaN never wins.  epsilon, explore_seed, `observation` and the returned `LinearEvaluation` are evaluate_linear's; the
    result buffers are the ones evaluate_linear / evaluate_mlp use, so `.observation` of any of them may be passed into any.
    A shared triple is kept on chip.  A population is read from device memory by every lane on every step: group the lanes
    by policy (policy_index non-decreasing) — the lanes of a wave then share their loads; a shuffled policy_index is legal
    and slower.  State, bsuite_info(), episode_counters() and the call index are left as T step() calls with the same
    actions leave them; calls interleave freely with step / rollout / evaluate_* / rollout_* / mark_reset / reset."""
    P, H1, H2 = self._check_evaluate_mlp2(w1, w2, w3, observation, num_steps, policy_index, epsilon, explore_seed)
    mlp2 = self._mlp2_struct(w1, w2, w3, H1, H2, P, policy_index, epsilon, explore_seed, observation)
    return self._evaluate('evaluate_mlp2', mlp2, num_steps)

  def rollout_mlp2(self, w1, w2, w3, observation, num_steps, *, policy_index=None, epsilon=0.0, explore_seed=0):
    """`rollout_mlp` for an agent with TWO ReLU hidden layers — `evaluate_mlp2` with the same arguments, recorded: the same
    ONE launch, the same `(ts, actions)`, contract and refusals as rollout_mlp, with another greedy action.  The call equals,
    bit for bit in everything it returns and everything it leaves behind,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else mlp2_select(w1[row], w2[row], w3[row], obs)
                           ts[t] = step(a); actions[t] = a; obs = ts[t].observation

    w1: float32 device tensor [H1, D+1] or [P, H1, D+1]; w2: [H2, H1+1] or [P, H2, H1+1]; w3: [3, H2+1] or [P, 3, H2+1],
    1 <= H1, H2 <= 64, each `torch.cat([lin.weight, lin.bias[:, None]], 1)` of a `torch.nn.Linear`; `policy_index`, epsilon,
    explore_seed and `observation` as in evaluate_mlp2 (utils.observations.mlp2_select has the rule).  A shared triple is kept
    on chip; a population is read from device memory by every lane on every step: group the lanes by policy.
    `rollout(actions)` on a twin reproduces `ts`; a twin's evaluate_mlp2() with the same arguments ends in the same state
    with `.observation == ts.observation[-1]` and `.episodes == (ts.step_type == LAST).sum(0)`.  Output buffers are cached
    per T, shared with rollout_linear() and rollout_mlp(), and overwritten by the next call of the same T."""
    what = 'rollout_mlp2'
    P, H1, H2 = self._check_evaluate_mlp2(w1, w2, w3, observation, num_steps, policy_index, epsilon, explore_seed, what=what)
    mlp2 = self._mlp2_struct(w1, w2, w3, H1, H2, P, policy_index, epsilon, explore_seed, observation)
    return self._record(what, mlp2, num_steps)

  def sample_linear(self, weights, observation, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`rollout_linear` for a learner that needs actions DRAWN from its policy (REINFORCE, actor-critic, PPO): the closed loop
    of a linear softmax agent in ONE launch that writes the trajectory (Cartpole, CartpoleSwingup and MountainCar, batched
    view, counter-based draws, no wrapper).  Returns `(ts, actions)` as rollout_linear does: `ts` with step_type int8 [T,B],
    reward / discount float32 [T,B], observation float32 [T,B,*obs_shape], and `actions` int32 [T,B], the action drawn at
    every step, 0 where the lane resets.  The call equals, bit for bit in everything it returns and everything it leaves
    behind,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else
                               gumbel_select(linear_logits(weights[row], obs), words(sample_seed, lane, call index), temperature)
                           ts[t] = step(a); actions[t] = a; obs = ts[t].observation

    so `rollout(actions)` on a twin reproduces `ts`.  linear_logits and gumbel_select are utils.observations': the float32
    logits of linear_select, then Gumbel-max in float64 — u_a = (word_a + 0.5) * 2^-32, g_a = -log(-log(u_a)) with the
    engine's bit-reproducible logarithm, z_a = l_a * (1 / temperature) + g_a, the largest z wins, the lowest index wins a
    tie, a NaN never wins — which draws action a with probability softmax(logits / temperature)[a].  The words are words
    0..2 of stream 3 of (sample_seed, global lane id, call index): an epsilon-greedy call with the same seed shares none, and
    nothing is drawn on a step that resets.  temperature: a finite number > 0 whose inverse is finite; there is no epsilon
    (the softmax explores) and no greedy limit (rollout_linear).  weights, observation and policy_index are rollout_linear's:
    the same shapes and population form, policy_index clamped to [0, P-1], and a lane that resets on the first step never
    reads its row of `observation`.  Logits and log-probabilities are not outputs: a learner recomputes them from
    `ts.observation` and `actions` with linear_logits.  State, bsuite_info(), episode_counters() and the call index are left
    as T step() calls leave them; calls interleave freely with step / rollout / rollout_linear / rollout_mlp / evaluate_* /
    mark_reset / reset.  Output buffers are cached per T, shared with rollout_linear(), rollout_mlp() and sample_mlp(), and
    overwritten by the next call of the same T."""
    what = 'sample_linear'
    P = self._check_evaluate_linear(weights, observation, num_steps, policy_index, 0.0, 0, what=what)
    beta = self._check_sample(what, temperature, sample_seed)
    return self._record(what, self._linear_struct(weights, P, policy_index, 0.0, sample_seed, observation), num_steps, beta)

  def sample_mlp(self, w1, w2, observation, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`sample_linear` for an agent with one ReLU hidden layer — `rollout_mlp` with actions drawn from the softmax of its
    logits: the same ONE launch, the same `(ts, actions)`, contract and refusals.  The call equals, bit for bit in everything
    it returns and everything it leaves behind,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else
                               gumbel_select(mlp_logits(w1[row], w2[row], obs), words(sample_seed, lane, call index), temperature)
                           ts[t] = step(a); actions[t] = a; obs = ts[t].observation

    w1: float32 device tensor [H, D+1] or [P, H, D+1]; w2: [3, H+1] or [P, 3, H+1], 1 <= H <= 64; `policy_index` and
    `observation` as in rollout_mlp; temperature and sample_seed as in sample_linear (utils.observations.mlp_logits and
    gumbel_select have the rule).  A shared pair is kept on chip; a population is read from device memory by every lane on
    every step: group the lanes by policy.  `rollout(actions)` on a twin reproduces `ts`.  Output buffers are cached per T,
    shared with sample_linear() and the rollout_* calls, and overwritten by the next call of the same T."""
    what = 'sample_mlp'
    P, H = self._check_evaluate_mlp(w1, w2, observation, num_steps, policy_index, 0.0, 0, what=what)
    beta = self._check_sample(what, temperature, sample_seed)
    return self._record(what, self._mlp_struct(w1, w2, H, P, policy_index, 0.0, sample_seed, observation), num_steps, beta)

  def evaluate_sampled_linear(self, weights, observation, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`sample_linear` with the same arguments, returns only: the lanes take the same `num_steps` steps with the same draws in
    ONE launch (Cartpole, CartpoleSwingup and MountainCar, batched view, counter-based draws, no wrapper).  The call equals,
    bit for bit in everything it leaves behind and returns,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else
                               gumbel_select(linear_logits(weights[row], obs), words(sample_seed, lane, call index), temperature)
                           ts = step(a); obs = ts.observation

    State, bsuite_info(), episode_counters() and the call index are left bit for bit where sample_linear leaves them, but no
    TimeStep is written.  Returns the cached `LinearEvaluation` of evaluate_linear — episodes int32 [B], return_sum and
    episode_return_sum float64 [B], observation float32 [B, *obs_shape] — with the same definitions: the sums as
    evaluate_policy() defines them, from the float64 reward of each step in step order, and `.observation` the row of step
    T-1, written once after the loop.  The buffers are shared with evaluate_linear(), evaluate_mlp() and
    evaluate_sampled_mlp() and overwritten by the next call of any of the four; passing `.observation` back in is legal.
    weights, observation, policy_index, temperature and sample_seed are sample_linear's: the same shapes and population
    form, words 0..2 of stream 3 of (sample_seed, global lane id, call index), nothing drawn on a step that resets, no
    epsilon and no greedy limit (evaluate_linear).  The refusals are sample_linear's, all before any GPU use, without the
    4 GiB slab (no slab is written).  Calls interleave freely with step / rollout / sample_* / rollout_* / evaluate_* /
    mark_reset / reset."""
    what = 'evaluate_sampled_linear'
    P = self._check_evaluate_linear(weights, observation, num_steps, policy_index, 0.0, 0, what=what)
    beta = self._check_sample(what, temperature, sample_seed)
    return self._evaluate(what, self._linear_struct(weights, P, policy_index, 0.0, sample_seed, observation), num_steps, beta)

  def evaluate_sampled_mlp(self, w1, w2, observation, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`evaluate_sampled_linear` for an agent with one ReLU hidden layer — `sample_mlp` with the same arguments, returns only:
    the same ONE launch, the same steps and draws, the same `LinearEvaluation`, contract and refusals.  The call equals, bit
    for bit in everything it leaves behind and returns,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else
                               gumbel_select(mlp_logits(w1[row], w2[row], obs), words(sample_seed, lane, call index), temperature)
                           ts = step(a); obs = ts.observation

    w1: float32 device tensor [H, D+1] or [P, H, D+1]; w2: [3, H+1] or [P, 3, H+1], 1 <= H <= 64; `policy_index` and
    `observation` as in sample_mlp; temperature and sample_seed as in sample_linear.  A shared pair is kept on chip; a
    population is read from device memory by every lane on every step: group the lanes by policy.  State, bsuite_info(),
    episode_counters() and the call index are left where sample_mlp leaves them; no TimeStep is written.  The result buffers
    are the ones evaluate_linear() uses, overwritten by the next call of evaluate_linear / evaluate_mlp /
    evaluate_sampled_linear / evaluate_sampled_mlp."""
    what = 'evaluate_sampled_mlp'
    P, H = self._check_evaluate_mlp(w1, w2, observation, num_steps, policy_index, 0.0, 0, what=what)
    beta = self._check_sample(what, temperature, sample_seed)
    return self._evaluate(what, self._mlp_struct(w1, w2, H, P, policy_index, 0.0, sample_seed, observation), num_steps, beta)

  def sample_mlp2(self, w1, w2, w3, observation, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`sample_mlp` for an agent with TWO ReLU hidden layers — `rollout_mlp2` with actions drawn from the softmax of its
    logits: the same ONE launch, the same `(ts, actions)`, contract and refusals.  The call equals, bit for bit in everything
    it returns and everything it leaves behind,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else
                               gumbel_select(mlp2_logits(w1[row], w2[row], w3[row], obs), words(sample_seed, lane, call index), temperature)
                           ts[t] = step(a); actions[t] = a; obs = ts[t].observation

    w1: float32 device tensor [H1, D+1] or [P, H1, D+1]; w2: [H2, H1+1] or [P, H2, H1+1]; w3: [3, H2+1] or [P, 3, H2+1],
    1 <= H1, H2 <= 64, each `torch.cat([lin.weight, lin.bias[:, None]], 1)` of a `torch.nn.Linear`; `policy_index` (clamped
    to [0, P-1]) and `observation` as in rollout_mlp2; temperature and sample_seed as in sample_linear
    (utils.observations.mlp2_logits and gumbel_select have the rule): a finite temperature > 0 whose inverse is finite, no
    epsilon and no greedy limit (rollout_mlp2).  The words are words 0..2 of stream 3 of (sample_seed, global lane id, call
    index); nothing is drawn on a step that resets, and a lane that resets on the first step never reads its row of
    `observation`.  A -inf logit masks its action; a NaN score never wins, and a NaN score of action 0 is never beaten.  A
    shared triple is kept on chip; a population is read from device memory by every lane on every step: group the lanes by
    policy.  `rollout(actions)` on a twin reproduces `ts`.  State, bsuite_info(), episode_counters() and the call index are
    left as T step() calls leave them.  Output buffers are cached per T, shared with the other sample_* and the rollout_*
    calls, and overwritten by the next call of the same T."""
    what = 'sample_mlp2'
    P, H1, H2 = self._check_evaluate_mlp2(w1, w2, w3, observation, num_steps, policy_index, 0.0, 0, what=what)
    beta = self._check_sample(what, temperature, sample_seed)
    mlp2 = self._mlp2_struct(w1, w2, w3, H1, H2, P, policy_index, 0.0, sample_seed, observation)
    return self._record(what, mlp2, num_steps, beta)

  def evaluate_sampled_mlp2(self, w1, w2, w3, observation, num_steps, *, policy_index=None, temperature=1.0, sample_seed=0):
    """`evaluate_sampled_mlp` for an agent with TWO ReLU hidden layers — `sample_mlp2` with the same arguments, returns only:
    the same ONE launch, the same steps and draws, the same `LinearEvaluation`, contract and refusals.  The call equals, bit
    for bit in everything it leaves behind and returns,

        obs = observation
        for t in range(T): a = 0 where the lane resets on this call, else
                               gumbel_select(mlp2_logits(w1[row], w2[row], w3[row], obs), words(sample_seed, lane, call index), temperature)
                           ts = step(a); obs = ts.observation

    w1: float32 device tensor [H1, D+1] or [P, H1, D+1]; w2: [H2, H1+1] or [P, H2, H1+1]; w3: [3, H2+1] or [P, 3, H2+1],
    1 <= H1, H2 <= 64, each `torch.cat([lin.weight, lin.bias[:, None]], 1)` of a `torch.nn.Linear`; `policy_index` and
    `observation` as in sample_mlp2; temperature and sample_seed as in sample_linear.  A shared triple is kept on chip; a
    population is read from device memory by every lane on every step: group the lanes by policy.  State, bsuite_info(),
    episode_counters(), invalid_action_count() and the call index are left bit for bit where sample_mlp2 leaves them; no
    TimeStep is written, and there is no 4 GiB slab refusal (no slab is written).  The result buffers are the ones
    evaluate_linear() uses, overwritten by the next call of any evaluate_* / evaluate_sampled_* call on this family."""
    what = 'evaluate_sampled_mlp2'
    P, H1, H2 = self._check_evaluate_mlp2(w1, w2, w3, observation, num_steps, policy_index, 0.0, 0, what=what)
    beta = self._check_sample(what, temperature, sample_seed)
    mlp2 = self._mlp2_struct(w1, w2, w3, H1, H2, P, policy_index, 0.0, sample_seed, observation)
    return self._evaluate(what, mlp2, num_steps, beta)

