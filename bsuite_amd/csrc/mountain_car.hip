// mountain_car.hip — C-ABI entry points of mountain_car (bsuite/environments/mountain_car.py:62-90; auto-reset of bsuite/environments/base.py:54-65).
// Device code: mountain_car_env.h on the skeleton of small_obs.h.  One translation unit per small-observation family: the families' kernels are independent
// template instantiations, and compiling them side by side is what keeps a clean build() under a minute (round 6; as ONE
// file they were a 56 s single-threaded compile, the long pole of every build).
#include "small_obs.h"
#include "bsx_linear_score.h"
#include "bsx_mlp_returns.h"
#include "bsx_trajectory.h"
#include "bsx_torso.h"
#include "bsx_gumbel_device.h"
#include "bsx_drawn_returns.h"
#include "mountain_car_env.h"

static int mountain_car_make(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info, mountain_car_env::args* a) {
  if (cfg == nullptr) return BSX_ENULL;
  int rc = bsx_check_call(call, action, out);
  if (rc != 0) return rc;
  if (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) return BSX_ERANGE;
  if (call->n_lanes > 0 && (state == nullptr || steps == nullptr || info == nullptr)) return BSX_ENULL;
  a->ctl = bsx_make_ctl(call); a->action = action; a->state = state; a->steps = steps; a->out = out;
  a->info = info; a->obs_numel = 3; a->max_steps = cfg->max_steps;
  return 0;
}

extern "C" int bsx_mountain_car_step(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info) {
  mountain_car_env::args a;
  int rc = mountain_car_make(cfg, call, action, state, steps, out, info, &a);
  if (rc != 0) return rc;
  if (call->n_lanes == 0) return 0;
  return launch_small_obs<mountain_car_env>(a, bsx_n_steps(call), call->hip_stream);
}

extern "C" int bsx_mountain_car_linear_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear,
                                                 float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  if (cfg == nullptr || call == nullptr || linear == nullptr) return BSX_ENULL;
  int rc = (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) ? BSX_ERANGE : 0;
  if (rc == 0) rc = bsx_check_linear_call(call, linear, state, steps, out, info, cfg);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_linear_score_args e;
  mountain_car_env::args* a = &e.fam.mountain_car;
  a->ctl = bsx_make_ctl(call); a->action = nullptr; a->state = state; a->steps = steps; a->out = bsx_timestep_t{};   // (no action column, no TimeStep)
  a->info = info; a->obs_numel = 3; a->max_steps = cfg->max_steps;
  return bsx_linear_score_call(e, BSX_FAM_MOUNTAIN_CAR, call, linear, out);
}

extern "C" int bsx_mountain_car_mlp_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                              float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  if (cfg == nullptr || call == nullptr || mlp == nullptr) return BSX_ENULL;
  int rc = (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) ? BSX_ERANGE : 0;
  if (rc == 0) rc = bsx_check_mlp_call(call, mlp, state, steps, out, info, cfg);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_mlp_returns_args e;
  mountain_car_env::args* a = &e.fam.mountain_car;
  a->ctl = bsx_make_ctl(call); a->action = nullptr; a->state = state; a->steps = steps; a->out = bsx_timestep_t{};   // (no action column, no TimeStep)
  a->info = info; a->obs_numel = 3; a->max_steps = cfg->max_steps;
  return bsx_mlp_returns_call(e, BSX_FAM_MOUNTAIN_CAR, call, mlp, out);
}

// rollout_linear / rollout_mlp: the two evaluations' closed loop, writing the [T,B] TimeSteps and the actions taken.
template <class Policy>
static int mountain_car_trajectory(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const Policy* policy, float* state,
                                   int32_t* steps, const bsx_timestep_t& out, int32_t* actions_out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) ? BSX_ERANGE : 0;
  if (rc == 0) rc = bsx_check_trajectory_call(call, policy, state, steps, out, actions_out, info, cfg, 3);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_trajectory_args e;
  mountain_car_env::args* a = &e.fam.mountain_car;
  a->ctl = bsx_make_ctl(call); a->action = nullptr; a->state = state; a->steps = steps; a->out = bsx_timestep_t{};   // (the kernel reads e.out)
  a->info = info; a->obs_numel = 3; a->max_steps = cfg->max_steps;
  return bsx_trajectory_call(e, BSX_FAM_MOUNTAIN_CAR, call, policy, out, actions_out);
}

extern "C" int bsx_mountain_car_linear_rollout(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear,
                                                float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return mountain_car_trajectory(cfg, call, linear, state, steps, out, actions_out, info);
}

extern "C" int bsx_mountain_car_mlp_rollout(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                             float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return mountain_car_trajectory(cfg, call, mlp, state, steps, out, actions_out, info);
}

// evaluate_mlp2 / rollout_mlp2 (BSX_TORSO_GREEDY) and evaluate_sampled_mlp2 / sample_mlp2 (BSX_TORSO_DRAWN): the closed loop
// under a policy with two ReLU hidden layers, returns only or recorded.
static int mountain_car_torso(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2, int32_t mode,
                              double inv_temperature, float* state, int32_t* steps, bool record, const bsx_linear_eval_t& ev,
                              const bsx_timestep_t& out, int32_t* actions_out, double* info) {
  if (cfg == nullptr || call == nullptr || mlp2 == nullptr) return BSX_ENULL;
  int rc = (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) ? BSX_ERANGE : 0;
  const bool present = record ? bsx_trajectory_outputs_present(out, actions_out) : bsx_linear_eval_present(ev);
  if (rc == 0)
    rc = mode == BSX_TORSO_DRAWN ? bsx_check_mlp2_sample_call(call, mlp2, inv_temperature, state, steps, present, info, cfg)
                                 : bsx_check_mlp2_call(call, mlp2, state, steps, present, info, cfg);
  if (record) rc = bsx_check_trajectory_slab(rc, call, 3);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_torso_args e;
  mountain_car_env::args* a = &e.fam.mountain_car;
  a->ctl = bsx_make_ctl(call); a->action = nullptr; a->state = state; a->steps = steps; a->out = bsx_timestep_t{};   // (the kernel reads e.out)
  a->info = info; a->obs_numel = 3; a->max_steps = cfg->max_steps;
  return bsx_torso_call(e, BSX_FAM_MOUNTAIN_CAR, call, mlp2, mode, inv_temperature, record, ev, out, actions_out);
}

extern "C" int bsx_mountain_car_mlp2_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2,
                                               float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return mountain_car_torso(cfg, call, mlp2, BSX_TORSO_GREEDY, 0.0, state, steps, false, out, bsx_timestep_t{}, nullptr, info);
}

extern "C" int bsx_mountain_car_mlp2_rollout(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2,
                                              float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return mountain_car_torso(cfg, call, mlp2, BSX_TORSO_GREEDY, 0.0, state, steps, true, bsx_linear_eval_t{}, out, actions_out, info);
}

extern "C" int bsx_mountain_car_mlp2_sample(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2,
                                             double inv_temperature, float* state, int32_t* steps, bsx_timestep_t out,
                                             int32_t* actions_out, double* info) {
  return mountain_car_torso(cfg, call, mlp2, BSX_TORSO_DRAWN, inv_temperature, state, steps, true, bsx_linear_eval_t{}, out, actions_out,
                            info);
}

extern "C" int bsx_mountain_car_mlp2_sample_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2,
                                                      double inv_temperature, float* state, int32_t* steps, bsx_linear_eval_t out,
                                                      double* info) {
  return mountain_car_torso(cfg, call, mlp2, BSX_TORSO_DRAWN, inv_temperature, state, steps, false, out, bsx_timestep_t{}, nullptr,
                            info);
}

// sample_linear / sample_mlp: the recording closed loop with actions drawn from softmax(logits * inv_temperature).
template <class Policy>
static int mountain_car_sample(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const Policy* policy, double inv_temperature,
                               float* state, int32_t* steps, const bsx_timestep_t& out, int32_t* actions_out, double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) ? BSX_ERANGE : 0;
  if (rc == 0) rc = bsx_check_gumbel_call(call, policy, inv_temperature, state, steps, out, actions_out, info, cfg, 3);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_gumbel_args e;
  mountain_car_env::args* a = &e.t.fam.mountain_car;
  a->ctl = bsx_make_ctl(call); a->action = nullptr; a->state = state; a->steps = steps; a->out = bsx_timestep_t{};   // (the kernel reads e.t.out)
  a->info = info; a->obs_numel = 3; a->max_steps = cfg->max_steps;
  return bsx_gumbel_call(e, BSX_FAM_MOUNTAIN_CAR, call, policy, inv_temperature, out, actions_out);
}

extern "C" int bsx_mountain_car_linear_sample(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear,
                                               double inv_temperature, float* state, int32_t* steps, bsx_timestep_t out,
                                               int32_t* actions_out, double* info) {
  return mountain_car_sample(cfg, call, linear, inv_temperature, state, steps, out, actions_out, info);
}

extern "C" int bsx_mountain_car_mlp_sample(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                            double inv_temperature, float* state, int32_t* steps, bsx_timestep_t out,
                                            int32_t* actions_out, double* info) {
  return mountain_car_sample(cfg, call, mlp, inv_temperature, state, steps, out, actions_out, info);
}

// evaluate_sampled_linear / evaluate_sampled_mlp: the sampled closed loop, writing only what the evaluation writes.
template <class Policy>
static int mountain_car_sample_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const Policy* policy,
                                        double inv_temperature, float* state, int32_t* steps, const bsx_linear_eval_t& out,
                                        double* info) {
  if (cfg == nullptr || call == nullptr || policy == nullptr) return BSX_ENULL;
  int rc = (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) ? BSX_ERANGE : 0;
  if (rc == 0) rc = bsx_check_drawn_returns_call(call, policy, inv_temperature, state, steps, out, info, cfg);
  if (rc != 0 || call->n_lanes == 0) return rc;
  bsx_drawn_returns_args e;
  mountain_car_env::args* a = &e.fam.mountain_car;
  a->ctl = bsx_make_ctl(call); a->action = nullptr; a->state = state; a->steps = steps; a->out = bsx_timestep_t{};   // (no action column, no TimeStep)
  a->info = info; a->obs_numel = 3; a->max_steps = cfg->max_steps;
  return bsx_drawn_returns_call(e, BSX_FAM_MOUNTAIN_CAR, call, policy, inv_temperature, out);
}

extern "C" int bsx_mountain_car_linear_sample_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call,
                                                        const bsx_linear_t* linear, double inv_temperature, float* state,
                                                        int32_t* steps, bsx_linear_eval_t out, double* info) {
  return mountain_car_sample_evaluate(cfg, call, linear, inv_temperature, state, steps, out, info);
}

extern "C" int bsx_mountain_car_mlp_sample_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                                     double inv_temperature, float* state, int32_t* steps, bsx_linear_eval_t out,
                                                     double* info) {
  return mountain_car_sample_evaluate(cfg, call, mlp, inv_temperature, state, steps, out, info);
}

extern "C" int bsx_group_set_mountain_car(bsx_group_t* g, int32_t index, const bsx_mountain_car_t* cfg, const bsx_call_t* call,
                                     const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info) {
  if (g == nullptr) return BSX_ENULL;
  mountain_car_env::args a;
  int rc = mountain_car_make(cfg, call, action, state, steps, out, info, &a);
  if (rc != 0) return rc;
  return small_obs_group_put<mountain_car_env>(g, BSX_FAM_MOUNTAIN_CAR, index, call, a);
}
