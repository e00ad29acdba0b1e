// cartpole.hip — C-ABI entry points of cartpole / swingup (bsuite/environments/cartpole.py:37-177, bsuite/experiments/cartpole_swingup/cartpole_swingup.py:81-150; auto-reset of bsuite/environments/base.py:54-65).
// Device code: cartpole_env.h on the skeleton of small_obs.h.  One translation unit per small-observation family: the families' kernels are independent
// template instantiations, and compiling them side by side is what keeps a clean build() under a minute (round 6; as ONE
// file they were a 56 s single-threaded compile, the long pole of every build).
// Host code: the family's host trait (cartpole_host), make() for step and the groups, and the extern "C" definitions — the twelve
// fused closed-loop ones are one-statement delegations ("Host glue of the closed-loop calls").
#include "small_obs.h"
#include "bsx_linear_score.h"
#include "bsx_mlp_returns.h"
#include "bsx_trajectory.h"
#include "bsx_torso.h"
#include "bsx_gumbel_device.h"
#include "bsx_drawn_returns.h"
#include "cartpole_env.h"

// The parameters derived from a cfg on the host in f64, rounded once; BSX_ERANGE for a cfg outside the family's range.
static int cartpole_derive(const bsx_cartpole_t* cfg, cartpole_env::args* a) {
  const double m_total = (double)cfg->mass_cart + (double)cfg->mass_pole;
  const double pole_ml = (double)cfg->mass_pole * (double)cfg->length;
  if (!(m_total > 0.0) || !(cfg->x_threshold > 0.0f) || !(cfg->length > 0.0f)) return BSX_ERANGE;
  // the kernel's sine/cosine is specified for |angle| <= BSX_SINCOS_MAX_ARG; angles live in [0, 2*pi) after
  // the first step, so only the reset value theta_offset + U(-init_range, init_range) needs the bound
  if (!(fabs(cfg->theta_offset) + fabs(cfg->init_range) <= 32.0)) return BSX_ERANGE;
  a->inv_m_total = (float)(1.0 / m_total);
  a->pole_ml = (float)pole_ml;
  a->pole_ml_over_mt = (float)(pole_ml / m_total);
  a->den_a = (float)((double)cfg->length * 4.0 / 3.0);                       // l * 4/3
  a->den_b = (float)((double)cfg->length * (double)cfg->mass_pole / m_total);  // l * m_p / m_t
  a->inv_x_threshold = (float)(1.0 / (double)cfg->x_threshold);
  return 0;
}

// What differs between the physics families on the host: the trait of bsx_physics_closed_loop (bsx_host.h).
namespace {                                 // (internal linkage: the library exports its C ABI and nothing else)
struct cartpole_host {
  typedef bsx_cartpole_t cfg_t;
  typedef cartpole_env env;
  static constexpr int32_t code = BSX_FAM_CARTPOLE;
  static int range(const cfg_t* cfg, env::args* a) {
    return (cfg->last_step < 1 || cfg->last_step >= (1 << 30)) ? BSX_ERANGE : cartpole_derive(cfg, a);
  }
  static int obs_numel(const cfg_t* cfg) { return cfg->swingup ? 8 : 6; }
  static const void* extra(const cfg_t* cfg) { return cfg->time_frac; }
  static void fill(const cfg_t* cfg, const bsx_call_t* call, const int32_t* action, float* state, int32_t* steps,
                   const bsx_timestep_t& out, double* info, env::args* a) {
    a->ctl = bsx_make_ctl(call); a->action = action; a->state = state; a->steps = steps; a->out = out;
    a->info = info; a->obs_numel = obs_numel(cfg); a->cfg = *cfg;
  }
  template <class Union>
  static env::args* of(Union& fam) { return &fam.cartpole; }
};
}  // namespace

static int cartpole_make(const bsx_cartpole_t* cfg, const bsx_call_t* call, const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info, cartpole_env::args* a) {
  if (cfg == nullptr) return BSX_ENULL;
  int rc = bsx_check_call(call, action, out);
  if (rc != 0) return rc;
  if (cfg->last_step < 1 || cfg->last_step >= (1 << 30)) return BSX_ERANGE;
  if (call->n_lanes > 0 && (state == nullptr || steps == nullptr || info == nullptr || cfg->time_frac == nullptr))
    return BSX_ENULL;
  cartpole_host::fill(cfg, call, action, state, steps, out, info, a);
  return cartpole_derive(cfg, a);
}

extern "C" int bsx_cartpole_step(const bsx_cartpole_t* cfg, const bsx_call_t* call, const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info) {
  cartpole_env::args a;
  int rc = cartpole_make(cfg, call, action, state, steps, out, info, &a);
  if (rc != 0) return rc;
  if (call->n_lanes == 0) return 0;
  return launch_small_obs<cartpole_env>(a, bsx_n_steps(call), call->hip_stream);
}

// The twelve fused closed-loop entry points: each body is stated once for both families, beside its kind's checks
// (bsx_<kind>_entry in bsx_linear_score.h ... bsx_drawn_returns.h), over the one prologue of bsx_host.h.
extern "C" int bsx_cartpole_linear_evaluate(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear,
                                            float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_linear_score_entry<cartpole_host>(cfg, call, linear, state, steps, out, info);
}

extern "C" int bsx_cartpole_mlp_evaluate(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                         float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_mlp_returns_entry<cartpole_host>(cfg, call, mlp, state, steps, out, info);
}

// rollout_linear / rollout_mlp: the two evaluations' closed loop, writing the [T,B] TimeSteps and the actions taken.
extern "C" int bsx_cartpole_linear_rollout(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear,
                                           float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_trajectory_entry<cartpole_host>(cfg, call, linear, state, steps, out, actions_out, info);
}

extern "C" int bsx_cartpole_mlp_rollout(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp,
                                        float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_trajectory_entry<cartpole_host>(cfg, call, mlp, state, steps, out, actions_out, info);
}

// evaluate_mlp2 / rollout_mlp2 (BSX_TORSO_GREEDY) and evaluate_sampled_mlp2 / sample_mlp2 (BSX_TORSO_DRAWN): the closed loop
// under a policy with two ReLU hidden layers, returns only or recorded.
extern "C" int bsx_cartpole_mlp2_evaluate(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2,
                                          float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_torso_entry<cartpole_host>(cfg, call, mlp2, BSX_TORSO_GREEDY, 0.0, state, steps, false, out, bsx_timestep_t{}, nullptr, info);
}

extern "C" int bsx_cartpole_mlp2_rollout(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2,
                                         float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_torso_entry<cartpole_host>(cfg, call, mlp2, BSX_TORSO_GREEDY, 0.0, state, steps,
                                        true, bsx_linear_eval_t{}, out, actions_out, info);
}

extern "C" int bsx_cartpole_mlp2_sample(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2, double inv_temperature,
                                        float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_torso_entry<cartpole_host>(cfg, call, mlp2, BSX_TORSO_DRAWN, inv_temperature, state, steps,
                                        true, bsx_linear_eval_t{}, out, actions_out, info);
}

extern "C" int bsx_cartpole_mlp2_sample_evaluate(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_mlp2_t* mlp2, double inv_temperature,
                                                 float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_torso_entry<cartpole_host>(cfg, call, mlp2, BSX_TORSO_DRAWN, inv_temperature, state, steps,
                                        false, out, bsx_timestep_t{}, nullptr, info);
}

// sample_linear / sample_mlp: the recording closed loop with actions drawn from softmax(logits * inv_temperature).
extern "C" int bsx_cartpole_linear_sample(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear, double inv_temperature,
                                          float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_gumbel_entry<cartpole_host>(cfg, call, linear, inv_temperature, state, steps, out, actions_out, info);
}

extern "C" int bsx_cartpole_mlp_sample(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp, double inv_temperature,
                                       float* state, int32_t* steps, bsx_timestep_t out, int32_t* actions_out, double* info) {
  return bsx_gumbel_entry<cartpole_host>(cfg, call, mlp, inv_temperature, state, steps, out, actions_out, info);
}

// evaluate_sampled_linear / evaluate_sampled_mlp: the sampled closed loop, writing only what the evaluation writes.
extern "C" int bsx_cartpole_linear_sample_evaluate(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_linear_t* linear, double inv_temperature,
                                                   float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_drawn_returns_entry<cartpole_host>(cfg, call, linear, inv_temperature, state, steps, out, info);
}

extern "C" int bsx_cartpole_mlp_sample_evaluate(const bsx_cartpole_t* cfg, const bsx_call_t* call, const bsx_mlp_t* mlp, double inv_temperature,
                                                float* state, int32_t* steps, bsx_linear_eval_t out, double* info) {
  return bsx_drawn_returns_entry<cartpole_host>(cfg, call, mlp, inv_temperature, state, steps, out, info);
}

extern "C" int bsx_group_set_cartpole(bsx_group_t* g, int32_t index, const bsx_cartpole_t* cfg, const bsx_call_t* call,
                                     const int32_t* action, float* state, int32_t* steps, bsx_timestep_t out, double* info) {
  if (g == nullptr) return BSX_ENULL;
  cartpole_env::args a;
  int rc = cartpole_make(cfg, call, action, state, steps, out, info, &a);
  if (rc != 0) return rc;
  return small_obs_group_put<cartpole_env>(g, BSX_FAM_CARTPOLE, index, call, a);
}
