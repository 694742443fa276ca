// cg_small.hpp — commons-math3 3.4.1 NonLinearConjugateGradientOptimizer(FLETCHER_REEVES, SimpleValueChecker(tol, tol))
// with its default LineSearch (BracketFinder(100, 500) + BrentOptimizer(1e-15, MIN_VALUE,
// SimpleUnivariateValueChecker(1e-8, 1e-8))) as one series' resumable state machine, for the small models whose fits
// run it with another objective than ARIMA's CSS: EWMA.fitModel (EWMA.scala:45-69; K = 1, GoalType.MINIMIZE) and
// GARCH.fitModel (GARCH.scala:33-53; K = 3, no GoalType: commons then maximises). The restatement followed is
// oracle/arima_oracle.c (cg_optimize, line_search) and SURVEY.md Appendix A; tests/smallfit_ref.py is the same in Python.
//
// Portable C++ (host and device): k_model_fit (arima_models.hip) keeps one SmallCG per lane in registers, and
// tests/sim/smallfit_sim.cpp runs the same code on the CPU.
//
// The machine posts one point at a time (x()); the caller answers with the objective AND the gradient at that point
// (one joint pass over the series) and calls advance(). Unlike cg_lane.hpp there is no speculation and no shortcut
// that assumes an objective: every evaluation the reference makes is a pass, with one exception that is independent
// of the objective -- F(point) at the top of a CG iteration is asked at the very array the preceding gradient was
// asked at, so the value the joint pass returned with that gradient is used (counted as the reference counts it).
//
// The goal is a template parameter and MINIMIZE is implemented as commons implements it (`isMinim ? a < b : a > b`, the
// negated gradient), not by negating the objective: BracketFinder's `denom = |val| < EPS_MIN ? 2 EPS_MIN : val` does
// not mirror under negation.
//
// Counting (oracle/arima_oracle.c:437-462): computeObjectiveValue checks MaxEval before it evaluates; BracketFinder's
// own 500-evaluation Incrementor is checked first; gradient calls are not evaluations; MaxIter is checked at the top
// of every iteration. `iter % K == 0` restarts the direction (at K = 1, every iteration).
#pragma once

#include <stdint.h>

#include "../../include/sparkts_arima.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define STS_SM_HD __host__ __device__ __forceinline__
#else
#define STS_SM_HD inline
#endif

namespace sts {
namespace small {

constexpr int kSmMaxEval = 10000;     // new MaxEval(10000)
constexpr int kSmMaxIter = 10000;     // new MaxIter(10000)
constexpr int kSmBracketMax = 500;    // BracketFinder() = BracketFinder(100, 500)

STS_SM_HD double sm_abs(double x) { return __builtin_fabs(x); }

// Precision.equals(x, y, 1)
STS_SM_HD bool sm_prec_equals(double x, double y) {
    const long long xi = __builtin_bit_cast(long long, x), yi = __builtin_bit_cast(long long, y);
    bool eq;
    if (((xi ^ yi) & (long long)0x8000000000000000ull) == 0) {
        const long long dd = xi - yi;
        eq = (dd < 0 ? -dd : dd) <= 1;
    } else {
        const long long NEG0 = (long long)0x8000000000000000ull;
        long long dplus, dminus;
        if (xi < yi) { dplus = yi; dminus = xi - NEG0; } else { dplus = xi; dminus = yi - NEG0; }
        eq = (dplus > 1) ? false : (dminus <= (1 - dplus));
    }
    return eq && !__builtin_isnan(x) && !__builtin_isnan(y);
}

// Simple(Univariate)ValueChecker.converged: |p - c| <= max(|p|, |c|) * rel || |p - c| <= abs (FastMath.max: NaN wins)
STS_SM_HD bool sm_converged(double p, double c, double rel, double abs_) {
    const double diff = sm_abs(p - c);
    const double ap = sm_abs(p), ac = sm_abs(c);
    double size;
    if (ap > ac) size = ap;
    else if (ap < ac) size = ac;
    else if (ap != ac) size = __builtin_nan("");
    else size = ap;
    return (diff <= size * rel) || (diff <= abs_);
}

template <int K, bool MINIM>
struct SmallCG {
    enum : int { W_G0 = 0, W_BR_A, W_BR_B, W_BR_C, W_BR_W1, W_BR_W3, W_BR_SHIFT, W_BRENT_FX, W_BRENT_FU, W_G, DONE };

    double tol;                       // the CG value checker's relative and absolute threshold
    double point[K], dir[K], xq[K];   // xq: the posted point
    double delta, cur_obj, fpt;       // fpt: the objective at `point` (from the gradient's pass)
    double xA, xB, xC, fA, fB, fC, bw, fW;                 // BracketFinder
    double a, b, x, v, w, d, e, fx, fv, fw, u;            // BrentOptimizer
    double prev_x, prev_f, cur_x, cur_f, best_x, best_f;  // Brent's previous / current / best pairs
    int32_t n_eval, n_grad, n_iter, bcount, status, pc;
    bool have_cur, have_prev;

    STS_SM_HD static bool better(double p, double q) { return MINIM ? p < q : p > q; }      // isMinim ? p < q : p > q
    STS_SM_HD static bool keeps(double p, double q) { return MINIM ? p <= q : p >= q; }     // best(a, b, isMinim) keeps a

    STS_SM_HD bool done() const { return pc == DONE; }
    STS_SM_HD const double *xreq() const { return xq; }

    // optimizer.optimize(..., new InitialGuess(init)): posts the first gradient
    STS_SM_HD void start(const double *init, double tol_) {
        tol = tol_;
        n_eval = n_grad = n_iter = bcount = 0;
        status = ARIMA_ST_OK;
        have_cur = have_prev = false;
        delta = cur_obj = fpt = 0.0;
        xA = xB = xC = fA = fB = fC = bw = fW = 0.0;
        a = b = x = v = w = d = e = fx = fv = fw = u = 0.0;
        prev_x = prev_f = cur_x = cur_f = best_x = best_f = 0.0;
        for (int i = 0; i < K; ++i) { point[i] = init[i]; xq[i] = init[i]; dir[i] = 0.0; }
        pc = W_G0;
    }

    // the result: parameters and objective (NaN unless the fit returned normally)
    STS_SM_HD void result(double *coef, double *obj) const {
        for (int i = 0; i < K; ++i) coef[i] = status == ARIMA_ST_OK ? point[i] : __builtin_nan("");
        *obj = status == ARIMA_ST_OK ? cur_obj : __builtin_nan("");
    }

    STS_SM_HD void fail(int st) { status = st; pc = DONE; }

    // computeObjectiveValue at startPoint + alpha * direction (LineSearch's univariate function)
    STS_SM_HD bool ls_eval(double alpha, int next) {
        if (n_eval + 1 > kSmMaxEval) { fail(ARIMA_ST_MAX_EVAL); return false; }
        ++n_eval;
        for (int i = 0; i < K; ++i) xq[i] = point[i] + alpha * dir[i];
        pc = next;
        return true;
    }
    // BracketFinder.eval: its own Incrementor first
    STS_SM_HD bool br_eval(double alpha, int next) {
        if (bcount + 1 > kSmBracketMax) { fail(ARIMA_ST_BRACKET_MAX_EVAL); return false; }
        ++bcount;
        return ls_eval(alpha, next);
    }

    // The caller's answer to the posted point: objective f and gradient g (K entries). Runs the machine to its next
    // posted point or to the end.
    STS_SM_HD void advance(double f, const double *g) {
        constexpr double GOLD = 1.618034, EPS_MIN = 1e-21, GROW = 100.0;
        enum : int { L_NONE = 0, L_TOP, L_BR_LOOP, L_BR_SHIFT, L_BR_END, L_BRENT_LOOP, L_LS_DONE };
        int go = L_NONE;
        double step = 0.0;
        switch (pc) {
        case W_G0: {
            ++n_grad;
            delta = 0.0;
            for (int i = 0; i < K; ++i) {
                const double r = MINIM ? -g[i] : g[i];
                dir[i] = r;                            // steepestDescent = r (identity preconditioner); direction = clone
                delta = delta + r * dir[i];
            }
            fpt = f;
            go = L_TOP;
            break;
        }
        case W_BR_A:
            fA = f;
            if (!br_eval(xB, W_BR_B)) return;
            return;
        case W_BR_B:
            fB = f;
            if (better(fA, fB)) {
                double t = xA; xA = xB; xB = t;
                t = fA; fA = fB; fB = t;
            }
            xC = xB + GOLD * (xB - xA);
            br_eval(xC, W_BR_C);
            return;
        case W_BR_C:
            fC = f;
            go = L_BR_LOOP;
            break;
        case W_BR_W1:
            fW = f;
            if (better(fW, fC)) { xA = xB; xB = bw; fA = fB; fB = fW; go = L_BR_END; break; }
            if (MINIM ? fW > fB : fW < fB) { xC = bw; fC = fW; go = L_BR_END; break; }
            bw = xC + GOLD * (xC - xB);
            br_eval(bw, W_BR_SHIFT);
            return;
        case W_BR_W3:
            fW = f;
            if (better(fW, fC)) {
                xB = xC; xC = bw; bw = xC + GOLD * (xC - xB); fB = fC; fC = fW;
                br_eval(bw, W_BR_SHIFT);
                return;
            }
            go = L_BR_SHIFT;
            break;
        case W_BR_SHIFT:
            fW = f;
            go = L_BR_SHIFT;
            break;
        case W_BRENT_FX:
            fx = MINIM ? f : -f;
            fv = fx; fw = fx;
            have_prev = false;
            prev_x = 0.0; prev_f = 0.0;
            cur_x = x; cur_f = f;
            best_x = x; best_f = f;
            go = L_BRENT_LOOP;
            break;
        case W_BRENT_FU: {
            const double fu = MINIM ? f : -f;
            prev_x = cur_x; prev_f = cur_f; have_prev = true;
            cur_x = u; cur_f = f;
            {
                double bx2, bf2;
                if (keeps(prev_f, cur_f)) { bx2 = prev_x; bf2 = prev_f; } else { bx2 = cur_x; bf2 = cur_f; }
                if (!keeps(best_f, bf2)) { best_x = bx2; best_f = bf2; }
            }
            if (sm_converged(prev_f, cur_f, 1e-8, 1e-8)) { step = best_x; go = L_LS_DONE; break; }
            if (fu <= fx) {
                if (u < x) b = x; else a = x;
                v = w; fv = fw; w = x; fw = fx; x = u; fx = fu;
            } else {
                if (u < x) a = u; else b = u;
                if (fu <= fw || sm_prec_equals(w, x)) { v = w; fv = fw; w = u; fw = fu; }
                else if (fu <= fv || sm_prec_equals(v, x) || sm_prec_equals(v, w)) { v = u; fv = fu; }
            }
            go = L_BRENT_LOOP;
            break;
        }
        case W_G: {
            ++n_grad;
            const double delta_old = delta;
            delta = 0.0;
            double r[K];
            for (int i = 0; i < K; ++i) {
                r[i] = MINIM ? -g[i] : g[i];
                delta = delta + r[i] * r[i];
            }
            const double beta = delta / delta_old;
            if (n_iter % K == 0 || beta < 0) {
                for (int i = 0; i < K; ++i) dir[i] = r[i];
            } else {
                for (int i = 0; i < K; ++i) dir[i] = r[i] + beta * dir[i];
            }
            fpt = f;
            go = L_TOP;
            break;
        }
        default:
            return;
        }

        for (;;) {
            switch (go) {
            case L_TOP: {
                if (n_iter + 1 > kSmMaxIter) { fail(ARIMA_ST_MAX_ITER); return; }
                ++n_iter;
                if (n_eval + 1 > kSmMaxEval) { fail(ARIMA_ST_MAX_EVAL); return; }
                ++n_eval;
                const double objective = fpt;
                const bool conv = have_cur && sm_converged(cur_obj, objective, tol, tol);
                cur_obj = objective;
                have_cur = true;
                if (conv) { pc = DONE; return; }
                // LineSearch.search: BracketFinder.search(f, goal, 0, 1e-8)
                bcount = 0;
                xA = 0.0; xB = 1e-8;
                br_eval(xA, W_BR_A);
                return;
            }
            case L_BR_SHIFT:
                xA = xB; fA = fB; xB = xC; fB = fC; xC = bw; fC = fW;
                go = L_BR_LOOP;
                break;
            case L_BR_LOOP: {
                if (!better(fC, fB)) { go = L_BR_END; break; }
                const double tmp1 = (xB - xA) * (fB - fC);
                const double tmp2 = (xB - xC) * (fB - fA);
                const double val = tmp2 - tmp1;
                const double denom = sm_abs(val) < EPS_MIN ? 2 * EPS_MIN : val;
                bw = xB - ((xB - xC) * tmp2 - (xB - xA) * tmp1) / (2 * denom);
                const double wLim = xB + GROW * (xC - xB);
                if ((bw - xC) * (xB - bw) > 0) {
                    br_eval(bw, W_BR_W1);
                } else if ((bw - wLim) * (wLim - xC) >= 0) {
                    bw = wLim;
                    br_eval(bw, W_BR_SHIFT);
                } else if ((bw - wLim) * (xC - bw) > 0) {
                    br_eval(bw, W_BR_W3);
                } else {
                    bw = xC + GOLD * (xC - xB);
                    br_eval(bw, W_BR_SHIFT);
                }
                return;
            }
            case L_BR_END: {
                double lo = xA, hi = xC;
                const double mid = xB;
                if (lo > hi) { const double t = lo; lo = hi; hi = t; }
                // new SearchInterval(lo, hi, mid)
                if (lo >= hi) { fail(ARIMA_ST_BAD_INTERVAL); return; }
                if (mid < lo || mid > hi) { fail(ARIMA_ST_BAD_INTERVAL); return; }
                // BrentOptimizer.doOptimize
                if (lo < hi) { a = lo; b = hi; } else { a = hi; b = lo; }
                x = mid; v = x; w = x; d = 0.0; e = 0.0;
                ls_eval(x, W_BRENT_FX);
                return;
            }
            case L_BRENT_LOOP: {
                const double GS = 0.5 * (3 - __builtin_sqrt(5.0));
                const double m = 0.5 * (a + b);
                const double tol1 = 1e-15 * sm_abs(x) + 4.9e-324;
                const double tol2 = 2 * tol1;
                const bool stop = sm_abs(x - m) <= tol2 - 0.5 * (b - a);
                if (stop) {
                    if (have_prev) {
                        double bx2, bf2;
                        if (keeps(prev_f, cur_f)) { bx2 = prev_x; bf2 = prev_f; } else { bx2 = cur_x; bf2 = cur_f; }
                        if (!keeps(best_f, bf2)) { best_x = bx2; best_f = bf2; }
                    } else {
                        if (!keeps(best_f, cur_f)) { best_x = cur_x; best_f = cur_f; }
                    }
                    step = best_x;
                    go = L_LS_DONE;
                    break;
                }
                double p = 0, q = 0, r = 0;
                if (sm_abs(e) > tol1) {
                    r = (x - w) * (fx - fv);
                    q = (x - v) * (fx - fw);
                    p = (x - v) * q - (x - w) * r;
                    q = 2 * (q - r);
                    if (q > 0) p = -p; else q = -q;
                    r = e;
                    e = d;
                    if (p > q * (a - x) && p < q * (b - x) && sm_abs(p) < sm_abs(0.5 * q * r)) {
                        d = p / q;
                        u = x + d;
                        if (u - a < tol2 || b - u < tol2) d = (x <= m) ? tol1 : -tol1;
                    } else {
                        e = (x < m) ? b - x : a - x;
                        d = GS * e;
                    }
                } else {
                    e = (x < m) ? b - x : a - x;
                    d = GS * e;
                }
                if (sm_abs(d) < tol1) u = (d >= 0) ? x + tol1 : x - tol1;
                else u = x + d;
                ls_eval(u, W_BRENT_FU);
                return;
            }
            case L_LS_DONE:
                // point += step * searchDirection; r = computeObjectiveGradient(point)
                for (int i = 0; i < K; ++i) {
                    point[i] = point[i] + step * dir[i];
                    xq[i] = point[i];
                }
                pc = W_G;
                return;
            default:
                return;
            }
        }
    }
};

}  // namespace small
}  // namespace sts
