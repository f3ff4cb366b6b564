// rk_driver.h — what the C-level Runge-Kutta drivers (ode_driver.hip, gat_driver.hip) share: the error-propagation macros,
// the coefficient tables of every method and the term lists built from them - each list is built by ONE function over a
// Tableau, whichever method a driver runs.  Private to csrc/; everything here has internal linkage, so the header adds
// nothing to the library's exports.
#pragma once
#include "common.h"

#define GODE_TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)
#define GODE_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return (int)e__; } while (0)

namespace {

// Launch-bound graphs close an adjoint stage's parameter derivative with ONE reduction launch (rk.hip:
// reduce_segments_kernel); above this many rows the separate launches are kept: the weight-gradient reduction has a
// 16-byte form that matters there.  The same bound as graph_odenet_amd/gat_ode.py: MERGED_FINISH_MAX_ROWS.
constexpr int64_t kMergedFinishMaxRows = 1 << 16;

// step size, stage times and h*coefficient products are formed in double and rounded once, exactly as the
// Python driver (solver.py) does, so both drivers feed identical fp32 coefficients to the kernels
// rk4, 3/8 rule
const double C38[4] = {0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0};
const double A38[4][3] = {{0.0, 0.0, 0.0}, {1.0 / 3.0, 0.0, 0.0}, {-1.0 / 3.0, 1.0, 0.0}, {1.0, -1.0, 1.0}};
const double B38[4] = {1.0 / 8.0, 3.0 / 8.0, 3.0 / 8.0, 1.0 / 8.0};
// explicit Euler; the explicit midpoint rule (b_1 = 0: the closing combination never reads k_1)
const double CEU[1] = {0.0};
const double AEU[1][1] = {{0.0}};
const double BEU[1] = {1.0};
const double CMID[2] = {0.0, 0.5};
const double AMID[2][1] = {{0.0}, {0.5}};
const double BMID[2] = {0.0, 1.0};
// Dormand-Prince 5(4)
const double DPC[7] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
const double DPA[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84},
};
const double DPB[7] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0};
const double DPE[7] = {35.0 / 384 - 1951.0 / 21600, 0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720,
                       -2187.0 / 6784 - -12231.0 / 42400, 11.0 / 84 - 649.0 / 6300, -1.0 / 60.0};

inline gode_lincomb_t one_term(const float* p) { gode_lincomb_t lc; lc.n = 1; lc.coef[0] = 1.f; lc.ptr[0] = p; return lc; }
inline gode_lincomb_t negated(gode_lincomb_t lc) { for (int j = 0; j < lc.n; ++j) lc.coef[j] = -lc.coef[j]; return lc; }

// A Butcher matrix as the sweeps read it: a[q * lda + s] = A[q][s] of a method with `stages` stages
// (b, c: the weights and abscissae)
struct Tableau { const double* a; int lda; int stages; const double* b; const double* c; };
const Tableau TAB38 = {&A38[0][0], 3, 4, B38, C38};
const Tableau TABDP = {&DPA[0][0], 6, 7, DPB, DPC};
const Tableau TABEU = {&AEU[0][0], 1, 1, BEU, CEU};
const Tableau TABMID = {&AMID[0][0], 1, 2, BMID, CMID};
// the fixed-grid methods by their GODE_RK_* code; nullptr outside the list
inline const Tableau* fixed_tableau(int method) {
    return method == GODE_RK_RK4_38 ? &TAB38 : method == GODE_RK_EULER ? &TABEU : method == GODE_RK_MIDPOINT ? &TABMID : nullptr;
}
// explicit_adams: 4th-order Adams-Bashforth, y_{i+1} = y_i + h sum_j ADAMS_B[j] f_{i-j}, after kAdamsStart 3/8-rule steps
constexpr int kAdamsStart = 3;
const double ADAMS_B[4] = {55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0};
// terms of  y + h * sum_{j=1..3} ADAMS_B[j] * fh[j - 1]  (fh: f_{i-1}, f_{i-2}, f_{i-3}): what the launch that evaluates f_i
// adds h ADAMS_B[0] f_i to
inline gode_lincomb_t adams_pre(const float* y, const float* const* fh, double h) {
    gode_lincomb_t lc = one_term(y);
    for (int j = 1; j < 4; ++j) { lc.coef[lc.n] = (float)(h * ADAMS_B[j]); lc.ptr[lc.n] = fh[j - 1]; ++lc.n; }
    return lc;
}
// the weight f_i (the evaluation that opens step i of n) ends up with over the multistep steps that read it:
// h * sum of ADAMS_B[m - i] over m = max(i, 3) .. min(i + 3, n - 1)  (solver.multistep_weight, the same sum in double)
inline double adams_weight(int i, int n, double h) {
    double s = 0.0;
    const int lo = i > kAdamsStart ? i : kAdamsStart, hi = i + 3 < n - 1 ? i + 3 : n - 1;
    for (int m = lo; m <= hi; ++m) s += ADAMS_B[m - i];
    return h * s;
}
// Bogacki-Shampine 3(2) and Heun-Euler 2(1), both in FSAL form as Dormand-Prince is (the last row of a is b); Heun-Euler's
// third stage f(t + h, y1) is what makes it so.  e = b - b*
const double BSC[4] = {0.0, 1.0 / 2, 3.0 / 4, 1.0};
const double BSA[4][3] = {{0, 0, 0}, {1.0 / 2, 0, 0}, {0, 3.0 / 4, 0}, {2.0 / 9, 1.0 / 3, 4.0 / 9}};
const double BSB[4] = {2.0 / 9, 1.0 / 3, 4.0 / 9, 0};
const double BSE[4] = {2.0 / 9 - 7.0 / 24, 1.0 / 3 - 1.0 / 4, 4.0 / 9 - 1.0 / 3, -1.0 / 8};
const double HEC[3] = {0.0, 1.0, 1.0};
const double HEA[3][2] = {{0, 0}, {1.0, 0}, {1.0 / 2, 1.0 / 2}};
const double HEB[3] = {1.0 / 2, 1.0 / 2, 0};
const double HEE[3] = {-1.0 / 2, 1.0 / 2, 0};
const Tableau TABBS = {&BSA[0][0], 3, 4, BSB, BSC};
const Tableau TABHE = {&HEA[0][0], 2, 3, HEB, HEC};
// the adaptive methods by their GODE_RKA_* code: tableau, error weights e, order p; nullptr outside the list
struct AdaptiveMethod { Tableau tab; const double* e; int order; };
const AdaptiveMethod ADAPTIVE[3] = {{TABDP, DPE, 5}, {TABBS, BSE, 3}, {TABHE, HEE, 2}};
inline const AdaptiveMethod* adaptive_method(int method) {
    return method >= GODE_RKA_DOPRI5 && method <= GODE_RKA_ADAPTIVE_HEUN ? &ADAPTIVE[method] : nullptr;
}
// The close of an adaptive step as gode_rk_close_err_multi_f32 takes it: sol = y + h sum_j b_j k_j over the stages whose b
// or e is non-zero (a stage with b = 0 enters with the coefficient 0, which changes no bit of the sum), ecoef = h e_j over
// the same terms (0 for y); every array `off` elements in
inline gode_lincomb_t close_terms(const AdaptiveMethod& am, const float* y, float* const* k, double h, float* ecoef,
                                  int64_t off = 0) {
    gode_lincomb_t lc = one_term(y + off);
    for (int j = 0; j < GODE_MAX_TERMS; ++j) ecoef[j] = 0.f;
    for (int j = 0; j < am.tab.stages; ++j)
        if (am.tab.b[j] != 0.0 || am.e[j] != 0.0) {
            lc.coef[lc.n] = (float)(h * am.tab.b[j]); ecoef[lc.n] = (float)(h * am.e[j]); lc.ptr[lc.n] = k[j] + off; ++lc.n;
        }
    return lc;
}
// terms of  y + h * sum_{j<s} A[s][j] * k[j]  of a tableau (zero coefficients dropped)
inline gode_lincomb_t tab_stage_terms(const Tableau& tab, const float* y, float* const* k, int s, double h) {
    gode_lincomb_t lc = one_term(y);
    for (int j = 0; j < s; ++j) {
        const double a = tab.a[s * tab.lda + j];
        if (a != 0.0) { lc.coef[lc.n] = (float)(h * a); lc.ptr[lc.n] = k[j]; ++lc.n; }
    }
    return lc;
}
// terms of  y + h * sum_{j<stages-1} b_j * k[j]: what the launch that produces the last stage adds h b_last f to
inline gode_lincomb_t tab_combine_terms(const Tableau& tab, const float* y, float* const* k, double h) {
    gode_lincomb_t lc = one_term(y);
    for (int j = 0; j + 1 < tab.stages; ++j)
        if (tab.b[j] != 0.0) { lc.coef[lc.n] = (float)(h * tab.b[j]); lc.ptr[lc.n] = k[j]; ++lc.n; }
    return lc;
}

// kbar_s of a backprop sweep: w abar + h sum_{q > s} A[q][s] Ybar_q  (w = h b_s in a plain step; a zero w, a zero
// A[q][s] and a stage q with dead[q] set - its cotangent was identically zero, so it has no Ybar_q - add no term:
// the result may have none)
inline gode_lincomb_t stage_cotangent(const Tableau& tab, const float* abar, float w, float* const* ybar, int s, double h,
                                      const bool* dead = nullptr) {
    gode_lincomb_t lc;
    lc.n = 0;
    if (w != 0.f) { lc.coef[0] = w; lc.ptr[0] = abar; lc.n = 1; }
    for (int q = s + 1; q < tab.stages; ++q) {
        const double a = tab.a[q * tab.lda + s];
        if (a != 0.0 && !(dead && dead[q])) { lc.coef[lc.n] = (float)(h * a); lc.ptr[lc.n] = ybar[q]; ++lc.n; }
    }
    return lc;
}
// w abar + sum_{from <= q < stages} Ybar_q: what a sweep adds up to the cotangent of the step's start state
inline gode_lincomb_t sweep_pre(const Tableau& tab, const float* abar, float w, float* const* ybar, int from,
                                const bool* dead = nullptr) {
    gode_lincomb_t lc = one_term(abar);
    lc.coef[0] = w;
    for (int q = from; q < tab.stages; ++q)
        if (!(dead && dead[q])) { lc.coef[lc.n] = 1.f; lc.ptr[lc.n] = ybar[q]; ++lc.n; }
    return lc;
}
// terms of  y + h * sum_{j<count} coef[j] * k[j], every array `off` elements in  (zero coefficients dropped)
inline gode_lincomb_t dp_terms(const float* y, float* const* k, const double* coef, int count, double h, bool with_y,
                               int64_t off = 0) {
    gode_lincomb_t lc;
    lc.n = 0;
    if (with_y) { lc.coef[0] = 1.f; lc.ptr[0] = y + off; lc.n = 1; }
    for (int j = 0; j < count; ++j)
        if (coef[j] != 0.0) { lc.coef[lc.n] = (float)(h * coef[j]); lc.ptr[lc.n] = k[j] + off; ++lc.n; }
    return lc;
}

}  // namespace
