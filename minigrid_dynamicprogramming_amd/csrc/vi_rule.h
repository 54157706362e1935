// vi_rule.h -- the global stopping rule that closes every solve and evaluation, stated once.
//
// Pure host C++17 (nothing from HIP, as vi_plan.h).  Every grid has run its own rule and been taken to
// the common sweep K; with exact arithmetic dV(K) < tol then holds.  Where rounding broke that,
// rule_sweeps takes all grids on a sweep at a time; rule_report is the one place (horizon, dV, tol)
// becomes `converged`.  The callers (vi_host_serve.h: solve_close; vi_host_eval.h: eval_run) differ in
// the step only.  tests/test_vi_rule_cpu.py checks both on the CPU (tools/vi_rule_check.cpp).
#pragma once

#include <cstdint>

namespace mgdp {

// From the common sweep *k with *dv = dV(*k): step(k + 1, dv) takes every grid to sweep k + 1 and
// stores its dV (0 = done, else the error code, which ends the loop at once with *k the last sweep
// completed).  `<`, not `<=`; a NaN dV keeps sweeping to the cap.
template <typename Step>
int rule_sweeps(double tol, int32_t max_sweeps, int32_t *k, double *dv, Step &&step) {
    while (!(*dv < tol) && *k < max_sweeps) {  // contraction broken by rounding: global rule
        if (int rc = step(*k + 1, dv)) return rc;
        ++*k;
    }
    return 0;
}

// `converged` of a solve that ended at sweep k with dV(k) = dv, also written to the out-parameters
// (each may be null).  A finite horizon is exact after its H sweeps, whatever dV is.
inline int32_t rule_report(int horizon, double tol, int32_t k, double dv, int32_t *sweeps_out, double *dv_out,
                           int32_t *converged_out) {
    const int32_t converged = horizon > 0 ? 1 : dv < tol;
    if (sweeps_out) *sweeps_out = k;
    if (dv_out) *dv_out = dv;
    if (converged_out) *converged_out = converged;
    return converged;
}

}  // namespace mgdp
