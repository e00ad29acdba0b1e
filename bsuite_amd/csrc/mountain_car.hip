// mountain_car.hip — C-ABI entry points of mountain_car (bsuite/environments/mountain_car.py:62-90; auto-reset of bsuite/environments/base.py:54-65).
// Device code: mountain_car_env.h on the skeleton of small_obs.h.  One translation unit per small-observation family: the families' kernels are independent
// template instantiations, and compiling them side by side is what keeps a clean build() under a minute (round 6; as ONE
// file they were a 56 s single-threaded compile, the long pole of every build).
// Host code: the family's host trait (mountain_car_host), make() for step and the groups, and the extern "C" definitions — the twelve
// fused closed-loop ones are one-statement delegations ("Host glue of the closed-loop calls").
#include "small_obs.h"
#include "bsx_linear_score.h"
#include "bsx_mlp_returns.h"
#include "bsx_trajectory.h"
#include "bsx_torso.h"
#include "bsx_gumbel_device.h"
#include "bsx_drawn_returns.h"
#include "mountain_car_env.h"

// What differs between the physics families on the host: the trait of bsx_physics_closed_loop (bsx_host.h).
namespace {                                 // (internal linkage: the library exports its C ABI and nothing else)
struct mountain_car_host {
  typedef bsx_mountain_car_t cfg_t;
  typedef mountain_car_env env;
  static constexpr int32_t code = BSX_FAM_MOUNTAIN_CAR;
  static int range(const cfg_t* cfg, env::args*) { return (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) ? BSX_ERANGE : 0; }
  static int obs_numel(const cfg_t*) { return 3; }
  static const void* extra(const cfg_t* cfg) { return cfg; }              // (nothing but the cfg itself)
  static void fill(const cfg_t* cfg, const bsx_call_t* call, const int32_t* action, float* state, int32_t* steps,
                   const bsx_timestep_t& out, double* info, env::args* a) {
    a->ctl = bsx_make_ctl(call); a->action = action; a->state = state; a->steps = steps; a->out = out;
    a->info = info; a->obs_numel = 3; a->max_steps = cfg->max_steps;
  }
  template <class Union>
  static env::args* of(Union& fam) { return &fam.mountain_car; }
};
}  // namespace

static int mountain_car_make(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info, mountain_car_env::args* a) {
  if (cfg == nullptr) return BSX_ENULL;
  int rc = bsx_check_call(call, action, out);
  if (rc != 0) return rc;
  if (cfg->max_steps < 1 || cfg->max_steps >= (1 << 30)) return BSX_ERANGE;
  if (call->n_lanes > 0 && (state == nullptr || steps == nullptr || info == nullptr)) return BSX_ENULL;
  mountain_car_host::fill(cfg, call, action, state, steps, out, info, a);
  return 0;
}

extern "C" int bsx_mountain_car_step(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info) {
  mountain_car_env::args a;
  int rc = mountain_car_make(cfg, call, action, state, steps, out, info, &a);
  if (rc != 0) return rc;
  if (call->n_lanes == 0) return 0;
  return launch_small_obs<mountain_car_env>(a, bsx_n_steps(call), call->hip_stream);
}

// The twelve fused closed-loop entry points: each body is stated once for both families, beside its kind's checks
// (bsx_<kind>_entry in bsx_linear_score.h ... bsx_drawn_returns.h), over the one prologue of bsx_host.h.
extern "C" int bsx_mountain_car_linear_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear,
                                                float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_linear_score_entry<mountain_car_host>(cfg, call, linear, state, steps, out, info);
}

extern "C" int bsx_mountain_car_mlp_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                             float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_mlp_returns_entry<mountain_car_host>(cfg, call, mlp, state, steps, out, info);
}

// rollout_linear / rollout_mlp: the two evaluations' closed loop, writing the [T,B] TimeSteps and the actions taken.
extern "C" int bsx_mountain_car_linear_rollout(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear,
                                               float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_trajectory_entry<mountain_car_host>(cfg, call, linear, state, steps, out, actions_out, info);
}

extern "C" int bsx_mountain_car_mlp_rollout(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                            float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_trajectory_entry<mountain_car_host>(cfg, call, mlp, state, steps, out, actions_out, info);
}

// evaluate_mlp2 / rollout_mlp2 (BSX_TORSO_GREEDY) and evaluate_sampled_mlp2 / sample_mlp2 (BSX_TORSO_DRAWN): the closed loop
// under a policy with two ReLU hidden layers, returns only or recorded.
extern "C" int bsx_mountain_car_mlp2_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2,
                                              float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_torso_entry<mountain_car_host>(cfg, call, mlp2, BSX_TORSO_GREEDY, 0.0, state, steps,
                                            false, out, bsx_timestep_t{}, nullptr, info);
}

extern "C" int bsx_mountain_car_mlp2_rollout(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2,
                                             float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_torso_entry<mountain_car_host>(cfg, call, mlp2, BSX_TORSO_GREEDY, 0.0, state, steps,
                                            true, bsx_linear_eval_t{}, out, actions_out, info);
}

extern "C" int bsx_mountain_car_mlp2_sample(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2, double inv_temperature,
                                            float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_torso_entry<mountain_car_host>(cfg, call, mlp2, BSX_TORSO_DRAWN, inv_temperature, state, steps,
                                            true, bsx_linear_eval_t{}, out, actions_out, info);
}

extern "C" int bsx_mountain_car_mlp2_sample_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2, double inv_temperature,
                                                     float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_torso_entry<mountain_car_host>(cfg, call, mlp2, BSX_TORSO_DRAWN, inv_temperature, state, steps,
                                            false, out, bsx_timestep_t{}, nullptr, info);
}

// sample_linear / sample_mlp: the recording closed loop with actions drawn from softmax(logits * inv_temperature).
extern "C" int bsx_mountain_car_linear_sample(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear, double inv_temperature,
                                              float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_gumbel_entry<mountain_car_host>(cfg, call, linear, inv_temperature, state, steps, out, actions_out, info);
}

extern "C" int bsx_mountain_car_mlp_sample(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp, double inv_temperature,
                                           float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_gumbel_entry<mountain_car_host>(cfg, call, mlp, inv_temperature, state, steps, out, actions_out, info);
}

// evaluate_sampled_linear / evaluate_sampled_mlp: the sampled closed loop, writing only what the evaluation writes.
extern "C" int bsx_mountain_car_linear_sample_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear, double inv_temperature,
                                                       float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_drawn_returns_entry<mountain_car_host>(cfg, call, linear, inv_temperature, state, steps, out, info);
}

extern "C" int bsx_mountain_car_mlp_sample_evaluate(const bsx_mountain_car_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp, double inv_temperature,
                                                    float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_drawn_returns_entry<mountain_car_host>(cfg, call, mlp, inv_temperature, state, steps, out, info);
}

extern "C" int bsx_group_set_mountain_car(bsx_group_t* g, int32_t index, const bsx_mountain_car_t* cfg, const bsx_call_t* call,
                                     const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info) {
  if (g == nullptr) return BSX_ENULL;
  mountain_car_env::args a;
  int rc = mountain_car_make(cfg, call, action, state, steps, out, info, &a);
  if (rc != 0) return rc;
  return small_obs_group_put<mountain_car_env>(g, BSX_FAM_MOUNTAIN_CAR, index, call, a);
}
