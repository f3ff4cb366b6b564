// dense_pc.h - launchers of the producer / consumer dense kernels (gemm_pc.hip), called from the dispatch in gemm.hip.
// d = 128 only; cg = channels per GroupNorm group (forward: 0, 1, 2, 4; VJP: 0, 4); operands 16-byte aligned (checked
// by the caller).  Return 0, a hipError_t, or GODE_E_UNSUPPORTED when no kernel is instantiated for the arguments.
#pragma once
#include "common.h"

int gode_pc_fwd_launch(const LinComb& lc, int64_t n_rows, float eps, const float* gamma, const float* beta,
                       const float* W, int has_time, float t, float* S, float* xout, const float* aux_coef, float* aux,
                       int cg, hipStream_t s);   // aux (nullable): second combination of the terms, 4 terms only
// diagonal-only rows in the forward product (gemm_pc.hip, DIAG): diag[i] = a_ii of such a row, 0 elsewhere; skip[i] != 0:
// the S row is not stored; K[i, :] = relu(a_ii S[i, :] + bias) for the rows with diag[i] != 0.  All four non-null.
// alpha: the last-stage form only (gode_pc_fwd_diag_aux_launch).
struct FwdDiag { const float* diag; const float* skip; const float* bias; float* K; float alpha; };
int gode_pc_fwd_diag_launch(const LinComb& lc, int64_t n_rows, float eps, const float* gamma, const float* beta,
                            const float* W, int has_time, float t, float* S, const FwdDiag& dg, int cg, hipStream_t s);   // 1-3 terms, cg 0 / 4
// AUX and DIAG: 4 terms, cg 0 / 4; dg.K is the array of the second combination P (coefficients aux_coef) and receives
// fmaf(dg.alpha, relu(a_ii S[i, :] + bias), P[i, :]) on the rows with diag[i] != 0, P on the others
int gode_pc_fwd_diag_aux_launch(const LinComb& lc, int64_t n_rows, float eps, const float* gamma, const float* beta,
                                const float* W, int has_time, float t, float* S, const float* aux_coef, const FwdDiag& dg,
                                int cg, hipStream_t s);
int gode_pc_bwd_launch(const LinComb& lc, int64_t n_rows, float eps, const float* gamma, const float* W, int has_time,
                       const float* dS, float out_scale, const LinComb& pre, float* dx, float* dgamma_part,
                       float* dbeta_part, int64_t n_part, int cg, hipStream_t s);
// VJP and weight gradient in one pass (round 4): dW_part holds gode_pc_bwd_wgrad_parts(n_rows) partials of (128 + has_time) x 128
int64_t gode_pc_bwd_wgrad_parts(int64_t n_rows);
int gode_pc_bwd_wgrad_launch(const LinComb& lc, int64_t n_rows, float eps, const float* gamma, const float* beta, const float* W,
                             int has_time, const float* dS, float out_scale, const LinComb& pre, float* dx,
                             float* dgamma_part, float* dbeta_part, int64_t n_part, float* dW_part, int cg, hipStream_t s);
// The forward rk4 (3/8 rule) solve of rows that are isolated in A and A^T, in one launch (gemm_pc.hip:
// gcn_local_tail_rk4_kernel): row i of y_out = st.n_steps steps of x' = relu(a_ii[i] [t | GN(x)] W + bias) from row i of
// y_in, with the bits the dense DIAG launches of ode_driver.hip give that row.  coef[s]: the s + 1 coefficients of
// tab_stage_terms(TAB38, .., s, h); acoef: those of tab_combine_terms(TAB38, ..); alpha = h b_3; ts[i][s]: the stage times, rounded from double by the host.
// W has its time row; cg 0 / 4; y_out may be y_in.
#define GODE_LOCAL_TAIL_MAX_STEPS 16
struct LocalTailSteps { float coef[4][4]; float acoef[4]; float alpha; int n_steps; float ts[GODE_LOCAL_TAIL_MAX_STEPS][4]; };
int gode_pc_local_tail_launch(const float* y_in, float* y_out, int64_t n_rows, const float* a_ii, float eps,
                              const float* gamma, const float* beta, const float* W, const float* bias,
                              const LocalTailSteps& st, int cg, int blocks, hipStream_t s);
// One stage of the adjoint solve's forward recompute on n_rows isolated rows (gemm_pc.hip: gcn_adjoint_tail_kernel): Gf and
// the one-entry records of Sp(g) with the cotangent epilogue in one launch, with the bits that pair gives those rows.
// Every pointer names the FIRST ROW OF THE TAIL (the terms of yin and cot as well).  yin and cot have the same 1-4 terms
// count; cot's coefficients are negated already (ep.cot).  k: the stage's derivative - or, last, y_new = fmaf(alpha, k,
// fmaf(1, P, 0)) with P = sum pcoef[j] yin.ptr[j]; dS = fmaf(at_ii, g, 0) of the relu-masked g; x_out (nullable): the
// combined input; last: cot_out = sum c3[j] cot.ptr[j], unmasked.  colpart: gode_pc_adjoint_tail_colsum_rows(n_rows)
// rows of 128 floats, row q = g[8 q] + g[8 q + 1] + .. + g[8 q + 7] of the unscaled g, added in that order (what a block of
// the d = 128 SpMM leaves for 8 consecutive one-entry records).  The S and dZ rows of the tail are not stored.
struct AdjTail {
    const float* a_ii; const float* at_ii; const float* bias;
    float* k; float* dS; float* x_out; float* cot_out; float* colpart;
    float pcoef[4], c3[4], alpha;
};
int64_t gode_pc_adjoint_tail_blocks(int64_t n_rows, int terms);   // the grid
int64_t gode_pc_adjoint_tail_colsum_rows(int64_t n_rows);
int gode_pc_adjoint_tail_launch(const LinComb& yin, const LinComb& cot, int64_t n_rows, float eps, const float* gamma,
                                const float* beta, const float* W, float t, const AdjTail& at, bool last, int cg, hipStream_t s);
