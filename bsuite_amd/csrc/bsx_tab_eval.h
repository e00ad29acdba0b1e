// bsx_tab_eval.h — bsx_<family>_policy_evaluate (evaluate_policy): the arguments of the ONE kernel that serves deep_sea and
// catch (bsx_tab_eval_kernel, misc.hip; its body is bsx_tab_eval_body, bsx_pair_device.h) and its launcher.  The family is
// a uniform switch per launch, so the arguments are a tagged struct: `family` says which member of `fam` is set.
#ifndef BSX_TAB_EVAL_H_
#define BSX_TAB_EVAL_H_

#include "bsx_pair_host.h"
#include "catch_fam.h"
#include "deep_sea_fam.h"

struct bsx_tab_eval_args {
  int32_t family;                // BSX_FAM_DEEP_SEA or BSX_FAM_CATCH
  int32_t n_steps;
  bsx_policy_args p;             // (actions_out is not used)
  bsx_policy_eval_t out;
  union {
    deep_sea_fam::args deep_sea;
    catch_fam::args catch_;
  } fam;
};

// Launches bsx_tab_eval_kernel over a.fam's lanes (the caller has checked that the grid fits).
int bsx_launch_tab_eval(const bsx_tab_eval_args& a, hipStream_t st);

// What the two entry points share once the family's args are in place.
static inline int bsx_tab_eval_call(bsx_tab_eval_args& a, int32_t family, const bsx_call_t* call, const bsx_policy_t* pol,
                                    uint32_t num_actions, const bsx_policy_eval_t& out) {
  a.family = family;
  a.n_steps = call->n_steps;
  a.p = bsx_make_policy_args(pol, num_actions);
  a.p.actions_out = nullptr;
  a.out = out;
  return bsx_launch_tab_eval(a, (hipStream_t)call->hip_stream);
}

// bsx_<family>_policy_evaluate (Fam: the family's host trait, bsx_host.h).
template <class Fam>
static inline int bsx_tab_eval_entry(const typename Fam::cfg_t* cfg, const bsx_call_t* call, const bsx_policy_t* policy, int32_t* state,
                                     const bsx_policy_eval_t& out, double* info) {
  bsx_tab_eval_args e;
  return bsx_grid_closed_loop<Fam>(
      cfg, call, policy, state, nullptr, info, Fam::of(e.fam),
      [&] { return bsx_check_policy_eval_call(call, policy, Fam::states(cfg), state, out, info); },
      [&] { return bsx_tab_eval_call(e, Fam::code, call, policy, Fam::actions, out); });
}

#endif  // BSX_TAB_EVAL_H_
