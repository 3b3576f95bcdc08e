// pu_newton.h -- the safeguarded Newton-Raphson rule that optimises a length (an edge, a
// quartet's central length, a query's pendant length) as a resumable state machine:
// newton_start() names the first abscissa to evaluate, newton_step() takes lnL and its two
// derivatives there and names the next one, until `done`.  One definition serves every driver:
// the host loop over k_edge launches (pu_edge.cpp), the combiner of the persistent k_edge_newton
// launch (pu_edge.hip), the three arrangements that advance per k_quartet launch (pu_nni.hip),
// the loop inside k_place_newton (pu_place.hip) and the five-length rounds inside k_lmap_opt
// (pu_lmap.hip).  No contraction into fused multiply-adds: the
// arithmetic is that of tests/newton_reference.py, operation for operation.
#pragma once

#include <math.h>

#include <hip/hip_runtime.h>

namespace pu {

// lengths stay within these bounds, the start included
constexpr double kMinLen = 1e-8;
constexpr double kMaxLen = 100.0;

// a plain aggregate: it also lives in __shared__ memory
struct NewtonState {
    double t, lnl, d1, d2;  // the accepted point
    double tn;              // the abscissa to evaluate next; == t once done
    int it;                 // accepted steps
    int h;                  // halvings of the current step
    int evals;
    int started, done;
};

// (a NaN gives kMinLen: it takes a NaN d1 beside a finite lnL, which no kernel produces)
__host__ __device__ inline double newton_clamp(double x) { return fmin(fmax(x, kMinLen), kMaxLen); }

__host__ __device__ inline double newton_start(NewtonState &s, double t0) {
    s.t = s.tn = newton_clamp(t0);
    s.it = s.h = s.evals = 0;
    s.started = s.done = 0;
    return s.tn;
}

// the step from the accepted point: -d1 / d2 where the point is concave, else expansion
// (d1 > 0) or halving; ends at max_iter accepted steps, on a non-finite lnL and on no move
__host__ __device__ inline void newton_plan(NewtonState &s, int max_iter) {
#pragma clang fp contract(off)
    if (s.it >= max_iter || !isfinite(s.lnl)) {
        s.done = 1;
        return;
    }
    const double step = s.d2 < 0.0 ? -s.d1 / s.d2 : (s.d1 > 0.0 ? s.t + 0.1 : -0.5 * s.t);
    s.tn = newton_clamp(s.t + step);
    s.h = 0;
    if (s.tn == s.t) s.done = 1;
}

// lnl, d1, d2: the evaluation at the abscissa the last call named
__host__ __device__ inline double newton_step(NewtonState &s, double lnl, double d1, double d2,
                                              double tol, int max_iter) {
#pragma clang fp contract(off)
    ++s.evals;
    if (!s.started) {  // the start
        s.started = 1;
        s.lnl = lnl;
        s.d1 = d1;
        s.d2 = d2;
        newton_plan(s, max_iter);
    } else if (lnl >= s.lnl - 1e-13 * fabs(s.lnl)) {  // accepted
        const double dt = fabs(s.tn - s.t);
        s.t = s.tn;
        s.lnl = lnl;
        s.d1 = d1;
        s.d2 = d2;
        ++s.it;
        if (dt <= tol * (1.0 + s.t))
            s.done = 1;
        else
            newton_plan(s, max_iter);
    } else if (++s.h < 30) {  // a step that lowers the lnL is halved
        s.tn = 0.5 * (s.t + s.tn);
    } else {
        s.done = 1;  // no ascent along this direction: t is (numerically) optimal
    }
    if (s.done) s.tn = s.t;
    return s.tn;
}

}  // namespace pu
