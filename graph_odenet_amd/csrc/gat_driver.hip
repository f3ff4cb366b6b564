// gat_driver.hip — one adaptive step of the GAT ODE function per C-ABI call, and backprop through its solves.
//
// f(t, x) = relu(EdgeAttention([t | GroupNorm(x)]))  (reference: GAT/models.py:172-179 -> GAT/layers.py:95-122).
// The layer's message activation is f->act (GODE_GAT_ACT_*; zeroed: relu): eval_forward and stage_vjp hand it to the
// aggregation of csrc/edge.hip as gode_gat_act_t{f->act, f->act_param, 1}; check_common refuses a bad one before any launch.
// The adaptive controller (step-size choice, accept / reject, interpolation) stays with the caller, as for the GCN
// function in ode_driver.hip; this file only sequences the launches of six stage evaluations, the solution combine
// and the error-ratio sums, so that an adaptive step on a citation-size graph is one call instead of ~200.
// The launch sequence of one evaluation is graph_odenet_amd/gat_ode.py (GatOdeField / GatOdeAdjointField), which
// branches on the head count where this file does.
// After the dopri5 steps: backprop through the solve on launch-bound graphs, whose stage reverse is the adjoint stage's
// (stage_vjp).  Each of its launch sequences is ONE body over a tableau of rk_driver.h:
//   forward_save   gode_gat_ode_rk4_forward_save (TAB38), gode_gat_ode_fixed_forward_save (the tableau of the GODE_RK_* code)
//   backprop       gode_gat_ode_rk4_backprop, gode_gat_ode_fixed_backprop
//   step_backprop  gode_gat_ode_dopri5_step_backprop (ADAPTIVE[GODE_RKA_DOPRI5]), gode_gat_ode_adaptive_step_backprop
// An entry point names its tableau and calls the body, which validates (a code outside the list: a null tableau, refused where
// the method's entry point always refused it).  At the end of the file the forward and the adjoint step for any adaptive
// method (gode_gat_ode_adaptive_step_*: bosh3, adaptive_heun, dopri5 from its tableau); they close a step with another launch
// than the dopri5 steps at the top, so those stay apart.
#include "rk_driver.h"
#include "options.h"
#include <cmath>

namespace {

inline int64_t n_heads(const gode_gat_odefunc_t* f) { return f->heads > 1 ? f->heads : 1; }

// projections as the edge kernels see them: with H heads the n x (H*o) matrices ARE the (n*H) x o matrices of the
// virtual nodes (row stride o), and A2 (n x 2H) is (n*H) x 2
gode_gat_proj_t proj_of(const gode_gat_odefunc_t* f, const gode_gat_workspace_t* w) {
    const int64_t o = f->d / n_heads(f);
    gode_gat_proj_t p;
    p.ps = w->Ps; p.ld_s = o; p.pt = w->Pt; p.ld_t = o; p.as = w->A2; p.at = w->A2 + 1; p.ld_a = 2;
    return p;
}

// Pt[row, :] += bf  (heads: the per-head message biases ride the target-side projection)
__global__ __launch_bounds__(256) void add_row_bias_kernel(float* __restrict__ P, const float* __restrict__ b, int64_t n, int d) {
    const int64_t total = n * d;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) P[i] += b[i % d];
}
// dst[h] = src[2h + 1]  (logit-bias gradients out of the column sums of dA2)
__global__ void odd_entries_kernel(float* __restrict__ dst, const float* __restrict__ src, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[2 * i + 1];
}

inline bool small_dense(const gode_gat_odefunc_t* f) {
    return gode_opt_small_fused() && gode_gat_small_supported(f->n, f->d, f->groups, n_heads(f));
}

// the same condition as gat_ode.GatOdeField.raw_logits (the Python and the C driver issue the same launches)
inline bool raw_logits(const gode_gat_odefunc_t* f) {
    return f->n * n_heads(f) <= 65536 && f->n_edges > 8192 && small_dense(f);
}

// Ps, Pt, A2 of the stage input; a multi-term input is combined once (x_out) and read back as one array afterwards
int project(const gode_gat_odefunc_t* f, const gode_gat_workspace_t* w, gode_lincomb_t* yin, float t, void* stream) {
    const int64_t n = f->n, d = f->d;
    float* xo = yin->n > 1 ? w->X : nullptr;
    const int64_t Hh = n_heads(f);
    if (small_dense(f)) {                       // launch-bound graphs: the three products (and the bias add) as one launch
        GODE_TRY(gode_gat_project_small_f32(yin, n, d, f->groups, f->eps_gn, f->gamma, f->beta, f->Wsrc, f->Wtgt, f->Wlog, Hh,
                                            Hh > 1 ? f->bf : nullptr, t, w->Ps, w->Pt, w->A2, xo, f->Wpacked, stream));
        if (xo) { yin->n = 1; yin->coef[0] = 1.f; yin->ptr[0] = xo; }
        return 0;
    }
    GODE_TRY(gode_gn_time_gemm_pair_f32(yin, n, d, f->groups, f->eps_gn, f->gamma, f->beta, f->Wsrc, f->Wtgt, 1, t, w->Ps, w->Pt,
                                        xo, stream));
    if (xo) { yin->n = 1; yin->coef[0] = 1.f; yin->ptr[0] = xo; }
    const int64_t H = n_heads(f);
    GODE_TRY(gode_gn_time_gemm_f32(yin, n, d, f->groups, f->eps_gn, f->gamma, f->beta, f->Wlog, 2 * H, 1, t, w->A2, stream));
    if (H > 1) {
        int64_t blocks = (n * d + 255) / 256; if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(add_row_bias_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w->Pt, f->bf, n, (int)d);
        GODE_LAUNCH_CHECK();
    }
    return 0;
}

int eval_forward(const gode_gat_odefunc_t* f, const gode_gat_workspace_t* w, gode_lincomb_t* yin, float t, float* ky,
                 void* stream) {
    GODE_TRY(project(f, w, yin, t, stream));
    const gode_gat_proj_t pr = proj_of(f, w);
    const int64_t H = n_heads(f);
    const gode_gat_act_t mode = {f->act, f->act_param, 1};     // message activation inside, the function's relu outside
    if (H > 1) {   // logits shifted by their head's maximum (so the aggregation runs with amax = 0), biases in Pt
        if (raw_logits(f)) {     // launch-bound graphs: no launch that shifts the logits (csrc/edge.hip, HeadMax)
            GODE_TRY(gode_gat_logits_heads_raw_f32(&pr, f->bw, f->src, f->tgt, f->n_edges, H, w->a, w->heads_scratch, stream));
            return gode_gat_agg_heads_f32_fwd(&f->mt, f->src, f->tgt, &pr, f->d / H, w->zeros, w->a, w->heads_scratch, f->n_edges, H,
                                              f->eps, ky, w->wgt, w->den, &mode, stream);
        }
        GODE_TRY(gode_gat_logits_heads_f32(&pr, f->bw, f->src, f->tgt, f->n_edges, H, w->a, nullptr, w->heads_scratch, stream));
        return gode_gat_agg_f32_fwd(&f->mt, f->src, f->tgt, &pr, f->d / H, w->zeros, w->a, w->zeros, f->eps, ky, w->wgt, w->den,
                                    &mode, stream);
    }
    GODE_TRY(gode_gat_logits_f32(&pr, f->bw, f->src, f->tgt, f->n_edges, w->a, w->amax, (float*)w->logits_scratch, stream));
    return gode_gat_agg_f32_fwd(&f->mt, f->src, f->tgt, &pr, f->d, f->bf, w->a, w->amax, f->eps, ky, w->wgt, w->den, &mode, stream);
}

// The reverse of one evaluation k = f(t, sum yin) with cotangent cot_scale * (sum cot), shared by the adjoint step (cot = a,
// scale -1) and the backprop sweeps (cot = kbar_s, scale +1): f evaluated again at the stage input (ky, which masks the
// cotangent: the relu), the aggregation's VJP, the path through the maxima, the incidence sums into dPs / dPt / dA2 and -
// with `part`, on launch-bound graphs - the dense VJP into ka (+ pre) and into the partial slot `part`.  yin names the
// combined input on return.  part == NULL: the caller issues the dense half itself.
int stage_vjp(const gode_gat_odefunc_t* f, const gode_gat_workspace_t* w, gode_lincomb_t* yin, const gode_lincomb_t& cot,
              float cot_scale, float t, float* ky, float* ka, const gode_lincomb_t* pre, float* part, void* stream) {
    const int64_t H = n_heads(f);
    const int64_t n = f->n, d = f->d, o = d / H, nv = n * H;
    GODE_TRY(eval_forward(f, w, yin, t, ky, stream));                  // yin now names the combined input
    const gode_gat_proj_t pr = proj_of(f, w);
    int32_t did = 0;
    const gode_gat_act_t mode = {f->act, f->act_param, 1};
    GODE_TRY(gode_gat_agg_f32_bwd(&f->mt, f->src, f->tgt, &pr, o, H > 1 ? w->zeros : f->bf, w->wgt, w->den, ky, nullptr, &cot,
                                  cot_scale, w->dz, w->da, w->dPt, o, w->dA2 + 1, 2, &did, &mode, stream));
    if (f->n_edges > 0) {
        if (H > 1 && raw_logits(f) && !did && part)     // first half; the dense VJP launch below closes the step
            GODE_TRY(gode_gat_maxpath_heads_part_f32(w->a, w->da, f->n_edges, H, f->tgt, w->heads_scratch, stream));
        else if (H > 1 && raw_logits(f))
            GODE_TRY(gode_gat_maxpath_heads_raw_f32(w->a, w->da, f->n_edges, H, f->tgt, did ? w->dA2 + 1 : nullptr, 2,
                                                    w->heads_scratch, stream));
        else if (H > 1)
            GODE_TRY(gode_gat_maxpath_heads_f32(w->a, w->da, f->n_edges, H, f->tgt, did ? w->dA2 + 1 : nullptr, 2,
                                                w->heads_scratch, stream));
        else
            GODE_TRY(gode_gat_maxpath_f32(w->a, w->amax, w->da, f->n_edges, did ? f->tgt : nullptr, did ? w->dA2 + 1 : nullptr, 2,
                                          w->maxpath_scratch, stream));
    }
    if (did) {
        GODE_TRY(gode_spmm_csr_f32(f->ms_inc.rowptr, f->ms_inc.col, nullptr, f->ms_inc.items, f->ms_inc.n_items,
                                   f->ms_inc.long_rows, f->ms_inc.n_long, f->ms_inc.partial, w->dz, o, w->dPs, o, nv, o,
                                   nullptr, stream));
        GODE_TRY(gode_spmm_csr_f32(f->ms_inc.rowptr, f->ms_inc.col, nullptr, f->ms_inc.items, f->ms_inc.n_items,
                                   f->ms_inc.long_rows, f->ms_inc.n_long, f->ms_inc.partial, w->da, 1, w->dA2, 2, nv, 1,
                                   nullptr, stream));
    } else {
        GODE_TRY(gode_gat_scatter_f32(f->ms_inc.rowptr, f->ms_inc.col, f->mt_inc.rowptr, f->mt_inc.col, w->dz, w->da, o, nv,
                                      w->dPs, o, w->dPt, o, w->dA2, w->dA2 + 1, 2, stream));
    }
    if (!part) return 0;
    // k_a and all parameter-gradient partials in one launch; a closing launch reads the partials
    return gode_gat_dense_vjp_small_f32(yin, n, d, f->groups, f->eps_gn, f->gamma, f->beta, f->Wsrc, f->Wtgt, f->Wlog, H,
                                        w->dPs, w->dPt, w->dA2, 1.f, pre, ka, part,
                                        (H > 1 && raw_logits(f) && !did && f->n_edges > 0) ? w->heads_scratch : nullptr, f->src, f->tgt,
                                        f->n_edges, f->Wpacked, stream);
}

// theta-k layout: [Wsrc ((d+1)*d) | Wtgt ((d+1)*d) | Wlog ((d+1)*2H) | bf (d) | bw (H) | gamma (d) | beta (d)]   (H = 1: one head)
// An adjoint stage: the stage VJP with cotangent -a, then the parameter derivative closed from what it left.  `slot`
// (one-launch route only): the stage's partials go there instead of w->small_part and the caller closes them, with those
// of the step's other stages, in one gode_gat_small_finish_multi_f32.
int eval_adjoint(const gode_gat_odefunc_t* f, const gode_gat_workspace_t* w, gode_lincomb_t yin, const gode_lincomb_t& ain,
                 float t, float* ky, float* ka, float* kat, float* kth, void* stream, float* slot = nullptr) {
    const int64_t H = n_heads(f);
    const int64_t n = f->n, d = f->d, nW = (d + 1) * d, nL = (d + 1) * 2 * H;
    float* part = (w->small_part && small_dense(f)) ? (slot ? slot : w->small_part) : nullptr;
    GODE_TRY(stage_vjp(f, w, &yin, ain, -1.f, t, ky, ka, nullptr, part, stream));
    if (part && slot) return 0;
    if (part) return gode_gat_small_finish_f32(part, n, d, H, t, kth, kat, stream);      // one more launch to close
    float* g_src = kth; float* g_tgt = kth + nW; float* g_log = kth + 2 * nW;
    float* g_bf = g_log + nL; float* g_bw = g_bf + d; float* g_gamma = g_bw + H; float* g_beta = g_gamma + d;
    const int64_t nb = gode_gemm_bwd_parts(n);
    const bool affine = f->groups > 0;
    const float* Wj[3] = {f->Wsrc, f->Wtgt, f->Wlog};
    const float* dPj[3] = {w->dPs, w->dPt, w->dA2};
    const int64_t dout[3] = {d, d, 2 * H};
    // launch-bound graphs: ONE reduction launch closes the stage (the same launch sequence as gat_ode.py)
    const bool merged = n <= kMergedFinishMaxRows && affine && w->colsum_scratch2 != nullptr;
    int64_t n_a = 0, n_b = 0;
    if (merged) {
        GODE_TRY(gode_colsum_parts_f32(w->dPt, n, d, (float*)w->colsum_scratch, &n_a, stream));
        GODE_TRY(gode_colsum_parts_f32(w->dA2, n, 2 * H, (float*)w->colsum_scratch2, &n_b, stream));
    } else {
        // bias gradients from the per-target node sums (every edge has exactly one target)
        GODE_TRY(gode_colsum_f32(g_bf, w->dPt, n, d, 1.f, 0, (float*)w->colsum_scratch, stream));
        GODE_TRY(gode_colsum_f32(w->pair, w->dA2, n, 2 * H, 1.f, 0, (float*)w->colsum_scratch, stream));
        hipLaunchKernelGGL(odd_entries_kernel, dim3((unsigned)((H + 63) / 64)), dim3(64), 0, (hipStream_t)stream, g_bw, (const float*)w->pair, (int)H);
        GODE_LAUNCH_CHECK();
    }
    gode_lincomb_t acc; acc.n = 1; acc.coef[0] = 1.f; acc.ptr[0] = ka;
    for (int j = 0; j < 3; ++j)
        GODE_TRY(gode_gn_time_gemm_bwd_f32(&yin, n, d, f->groups, f->eps_gn, f->gamma, Wj[j], dout[j], 1, dPj[j], 1.f,
                                           j ? &acc : nullptr, ka, affine ? w->gp + j * nb * d : nullptr,
                                           affine ? w->bp + j * nb * d : nullptr, stream));
    if (affine && !merged) GODE_TRY(gode_reduce_parts2_f32(g_gamma, w->gp, g_beta, w->bp, 3 * nb, d, 1.f, 0, stream));
    else if (!affine) GODE_TRY(gode_zero_f32(g_gamma, 2 * d, stream));
    float* gW[3] = {g_src, g_tgt, g_log};
    const int64_t lenW[3] = {nW, nW, nL};
    const int64_t npw = gode_wgrad_parts(n);
    for (int j = 0; j < 3; ++j)
        GODE_TRY(gode_wgrad_f32(&yin, n, d, f->groups, f->eps_gn, f->gamma, f->beta, dPj[j], dout[j], 1, w->wp[j], stream));
    if (merged) {
        gode_reduce_seg_t sg[7] = {};
        sg[0] = {g_src, w->wp[0], npw, nW, 0, 1, nW, f->Wsrc, d};                              // row 0 of each block: its time row
        sg[1] = {g_tgt, w->wp[1], npw, nW, 0, 1, nW, f->Wtgt, d};
        sg[2] = {g_log, w->wp[2], npw, nL, 0, 1, nL, f->Wlog, 2 * H};
        sg[3] = {g_bf, (const float*)w->colsum_scratch, n_a, d, 0, 1, d, nullptr, 0};
        sg[4] = {g_bw, (const float*)w->colsum_scratch2, n_b, 2 * H, 1, 2, H, nullptr, 0};      // odd columns of the n x 2H sums
        sg[5] = {g_gamma, w->gp, 3 * nb, d, 0, 1, d, nullptr, 0};
        sg[6] = {g_beta, w->bp, 3 * nb, d, 0, 1, d, nullptr, 0};
        return gode_reduce_segments_f32(sg, 7, t, kat, stream);
    }
    GODE_TRY(gode_reduce_parts2_f32(gW[0], w->wp[0], gW[1], w->wp[1], npw, lenW[0], 1.f, 0, stream));
    GODE_TRY(gode_reduce_parts_f32(gW[2], w->wp[2], npw, lenW[2], 1.f, 0, stream));
    // a_t' = -a^T df/dt over the three time rows; each row 0 *= t
    return gode_time_row_fixup3_f32(gW[0], Wj[0], dout[0], gW[1], Wj[1], dout[1], gW[2], Wj[2], dout[2], t, kat, stream);
}

int check_common(const gode_gat_odefunc_t* f, const gode_gat_workspace_t* w, bool adjoint) {
    if (!f || !w) return GODE_E_NULLPTR;
    if (f->act < GODE_GAT_ACT_RELU || f->act > GODE_GAT_ACT_SIGMOID) return GODE_E_SHAPE;
    if ((f->act == GODE_GAT_ACT_LEAKY_RELU || f->act == GODE_GAT_ACT_ELU) && !std::isfinite(f->act_param)) return GODE_E_SHAPE;
    if (f->n <= 0 || f->d <= 0 || f->n_edges < 0 || f->heads < 0) return GODE_E_SHAPE;
    if (f->heads > 1) {
        if (f->d % f->heads || f->heads > 64) return GODE_E_SHAPE;
        if (!w->zeros || !w->heads_scratch) return GODE_E_NULLPTR;
    }
    if (!f->Wsrc || !f->Wtgt || !f->Wlog || !f->bf || !f->bw || !f->mt.rowptr) return GODE_E_NULLPTR;
    if (!w->X || !w->Ps || !w->Pt || !w->A2 || !w->amax || !w->den || !w->logits_scratch) return GODE_E_NULLPTR;
    if (f->n_edges > 0 && (!f->src || !f->tgt || !w->a || !w->wgt)) return GODE_E_NULLPTR;
    if (adjoint) {
        if (!w->dPs || !w->dPt || !w->dA2 || !w->pair || !w->colsum_scratch || !w->maxpath_scratch || !w->wp[0] || !w->wp[1] ||
            !w->wp[2] || !f->ms_inc.rowptr || !f->mt_inc.rowptr) return GODE_E_NULLPTR;
        if (f->n_edges > 0 && (!w->dz || !w->da)) return GODE_E_NULLPTR;
        if (f->groups > 0 && (!w->gp || !w->bp)) return GODE_E_NULLPTR;
    }
    return 0;
}

// the backprop sweeps run on the one-launch route only
int check_sweep(const gode_gat_odefunc_t* f, const gode_gat_workspace_t* w) {
    int rc = check_common(f, w, true); if (rc) return rc;
    if (!small_dense(f) || !w->small_part) return GODE_E_UNSUPPORTED;
    return 0;
}
int check_steps(int32_t n_steps, int32_t step_begin, int32_t step_end) {
    if (n_steps <= 0 || step_begin < 0 || step_end > n_steps || step_begin >= step_end) return GODE_E_SHAPE;
    return 0;
}
// floats of one stage's slot of parameter partials
inline int64_t part_slot(const gode_gat_odefunc_t* f) {
    return gode_gat_small_parts(f->n, f->d) * gode_gat_small_part_len(f->d, n_heads(f));
}

}  // namespace

extern "C" int64_t gode_gat_ode_theta_len(int64_t d) { return 2 * (d + 1) * d + (d + 1) * 2 + d + 1 + 2 * d; }
extern "C" int64_t gode_gat_ode_theta_len_heads(int64_t d, int64_t heads) {
    if (heads < 1) heads = 1;
    return 2 * (d + 1) * d + (d + 1) * 2 * heads + d + heads + 2 * d;
}

extern "C" int gode_gat_ode_dopri5_step_forward(const gode_gat_odefunc_t* f, const float* y, float* const* k, float* y1,
                                                const gode_gat_workspace_t* w, double t, double h, float rtol, float atol,
                                                double* sums, void* err_scratch, void* stream)
{
    int rc = check_common(f, w, false); if (rc) return rc;
    if (!y || !k || !y1 || !sums || !err_scratch) return GODE_E_NULLPTR;
    for (int s = 0; s < 7; ++s) if (!k[s]) return GODE_E_NULLPTR;
    const int64_t nd = f->n * f->d;
    for (int s = 1; s < 7; ++s) {
        gode_lincomb_t yin = tab_stage_terms(TABDP, y, k, s, h);
        GODE_TRY(eval_forward(f, w, &yin, (float)(t + DPC[s] * h), k[s], stream));
    }
    gode_lincomb_t sol = dp_terms(y, k, DPB, 7, h, true);
    GODE_TRY(gode_lincomb_f32(y1, &sol, nd, stream));
    gode_lincomb_t err = dp_terms(nullptr, k, DPE, 7, h, false);
    return gode_rk_errnorm_f32(sums, y, y1, &err, rtol, atol, nd, err_scratch, stream);
}

extern "C" int gode_gat_ode_dopri5_step_adjoint(const gode_gat_odefunc_t* f, const float* y, const float* a,
                                                const float* a_t, const float* theta, float* const* ky, float* const* ka,
                                                float* const* kat, float* const* kth, float* y1, float* a1, float* a_t1,
                                                float* theta1, const gode_gat_workspace_t* w, double t, double h,
                                                float rtol, float atol, double* sums /* 4 */, void* err_scratch,
                                                void* stream)
{
    int rc = check_common(f, w, true); if (rc) return rc;
    if (!y || !a || !a_t || !theta || !ky || !ka || !kat || !kth || !y1 || !a1 || !a_t1 || !theta1 || !sums || !err_scratch)
        return GODE_E_NULLPTR;
    for (int s = 0; s < 7; ++s) if (!ky[s] || !ka[s] || !kat[s] || !kth[s]) return GODE_E_NULLPTR;
    const int64_t nd = f->n * f->d, P = gode_gat_ode_theta_len_heads(f->d, n_heads(f));
    for (int s = 1; s < 7; ++s) {
        gode_lincomb_t yin = tab_stage_terms(TABDP, y, ky, s, h);
        gode_lincomb_t ain = tab_stage_terms(TABDP, a, ka, s, h);
        GODE_TRY(eval_adjoint(f, w, yin, ain, (float)(t + DPC[s] * h), ky[s], ka[s], kat[s], kth[s], stream));
    }
    struct Part { const float* y0; float* const* k; float* y1; int64_t len; };
    const Part parts[4] = {{y, ky, y1, nd}, {a, ka, a1, nd}, {a_t, kat, a_t1, 1}, {theta, kth, theta1, P}};
    // the four solution combines in one launch, the four error sums in one pair (same numbers as the single forms)
    float* outs[4]; gode_lincomb_t sols[4], errs[4]; int64_t lens[4]; const float* e0[4]; const float* e1[4];
    for (int c = 0; c < 4; ++c) {
        outs[c] = parts[c].y1; lens[c] = parts[c].len; e0[c] = parts[c].y0; e1[c] = parts[c].y1;
        sols[c] = dp_terms(parts[c].y0, parts[c].k, DPB, 7, h, true);
        errs[c] = dp_terms(nullptr, parts[c].k, DPE, 7, h, false);
    }
    GODE_TRY(gode_lincomb_multi_f32(outs, sols, lens, 4, stream));
    return gode_rk_errnorm_multi_f32(sums, e0, e1, errs, lens, 4, rtol, atol, err_scratch, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Backprop through the solve on launch-bound graphs (odeint._OdeintBackprop; the GCN forms are in ode_driver.hip and
// the algebra is stated there).  The reverse of a stage is stage_vjp with cotangent scale +1: the stage is evaluated
// again (k_scratch) rather than its saved k_s read, because the aggregation's VJP wants the edge weights and sums the
// evaluation leaves in the workspace.  Every swept stage writes its parameter partials into a slot of its own and ONE
// gode_gat_small_close_stages_f32 launch per step adds them to theta.
// ---------------------------------------------------------------------------------------------------------------
namespace {

// Steps step_begin .. step_end - 1 of a fixed-grid solve into records of (S + 1) n x d floats, [ y_n | k_1 .. k_S ]
// (tabp == NULL, here and below: a code outside GODE_RK_*, refused after the null checks)
int forward_save(const Tableau* tabp, const gode_gat_odefunc_t* f, const float* y0, float* y_end, float* save,
                 const gode_gat_workspace_t* ws, float t0, float t1, int32_t n_steps, int32_t step_begin, int32_t step_end,
                 void* stream)
{
    if (!f || !ws || !y0 || !y_end || !save) return GODE_E_NULLPTR;
    if (!tabp) return GODE_E_SHAPE;
    int rc = check_steps(n_steps, step_begin, step_end); if (rc) return rc;
    rc = check_sweep(f, ws); if (rc) return rc;
    const Tableau& tab = *tabp;
    const int S = tab.stages;
    const int64_t nd = f->n * f->d;
    const double h = ((double)t1 - (double)t0) / n_steps;
    if (y0 != save) {                                            // record 0 starts with a copy of y0
        const gode_lincomb_t c = one_term(y0);
        GODE_TRY(gode_lincomb_f32(save, &c, nd, stream));
    }
    for (int i = step_begin; i < step_end; ++i) {
        float* rec = save + (int64_t)(i - step_begin) * (S + 1) * nd;
        float* k[4] = {};
        for (int s = 0; s < S; ++s) k[s] = rec + (int64_t)(s + 1) * nd;
        float* ynext = (i + 1 < step_end) ? rec + (int64_t)(S + 1) * nd : y_end;      // the next record's y_n, or the result
        const double t = (double)t0 + i * h;
        for (int s = 0; s < S; ++s) {
            gode_lincomb_t yin = tab_stage_terms(tab, rec, k, s, h);
            GODE_TRY(eval_forward(f, ws, &yin, (float)(t + tab.c[s] * h), k[s], stream));
        }
        gode_lincomb_t sol = one_term(rec);
        for (int s = 0; s < S; ++s)
            if (tab.b[s] != 0.0) { sol.coef[sol.n] = (float)(h * tab.b[s]); sol.ptr[sol.n] = k[s]; ++sol.n; }
        GODE_TRY(gode_lincomb_f32(ynext, &sol, nd, stream));
    }
    return 0;
}

// The reverse sweep over those records: S slots of `parts`, one closing launch per swept step
int backprop(const Tableau* tabp, const gode_gat_odefunc_t* f, const float* save, float* a, float* theta, float* const* ybar,
             float* k_scratch, float* parts, const gode_gat_workspace_t* ws, float t0, float t1, int32_t n_steps,
             int32_t step_begin, int32_t step_end, void* stream)
{
    if (!f || !ws || !save || !a || !theta || !ybar || !k_scratch || !parts) return GODE_E_NULLPTR;
    if (!tabp) return GODE_E_SHAPE;
    const Tableau& tab = *tabp;
    const int S = tab.stages;
    for (int s = 0; s < S; ++s) if (!ybar[s]) return GODE_E_NULLPTR;
    int rc = check_steps(n_steps, step_begin, step_end); if (rc) return rc;
    for (int s = 0; s < S; ++s) {
        if (ybar[s] == a || ybar[s] == k_scratch) return GODE_E_SHAPE;
        for (int r = s + 1; r < S; ++r) if (ybar[s] == ybar[r]) return GODE_E_SHAPE;
    }
    if (k_scratch == a) return GODE_E_SHAPE;
    rc = check_sweep(f, ws); if (rc) return rc;
    const int64_t n = f->n, d = f->d, nd = n * d, H = n_heads(f), slot = part_slot(f);
    const double h = ((double)t1 - (double)t0) / n_steps;
    for (int i = step_end - 1; i >= step_begin; --i) {
        float* y = (float*)save + (int64_t)(i - step_begin) * (S + 1) * nd;     // read only
        float* k[4] = {};
        for (int s = 0; s < S; ++s) k[s] = y + (int64_t)(s + 1) * nd;
        const double t = (double)t0 + i * h;
        float ts[4];
        // every stage of these methods has a cotangent: b_S is non-zero and each earlier stage feeds a later one
        for (int s = S - 1; s >= 0; --s) {
            ts[s] = (float)(t + tab.c[s] * h);
            const gode_lincomb_t cot = stage_cotangent(tab, a, (float)(h * tab.b[s]), ybar, s, h);
            gode_lincomb_t yin = tab_stage_terms(tab, y, k, s, h);
            GODE_TRY(stage_vjp(f, ws, &yin, cot, 1.f, ts[s], k_scratch, ybar[s], nullptr, parts + s * slot, stream));
        }
        GODE_TRY(gode_gat_small_close_stages_f32(parts, n, d, H, S, ts, theta, stream));
        const gode_lincomb_t sum = sweep_pre(tab, a, 1.f, ybar, 0);      // a + Ybar_1 + .. + Ybar_S
        GODE_TRY(gode_lincomb_f32(a, &sum, nd, stream));
    }
    return 0;
}

// The reverse sweep over one accepted step of an adaptive method (am == NULL: a code outside GODE_RKA_*; the entries of k /
// ybar are looked at after that: their count is the method's).  kbar_last arrives on k_S.
int step_backprop(const AdaptiveMethod* am, const gode_gat_odefunc_t* f, const float* y, float* const* k, const float* g,
                  const float* kbar_last, double wy, const double* wk, double t, double h, int32_t first, float* const* ybar,
                  float* ybar_n, float* kbar1, float* theta, float* k_scratch, float* parts, const gode_gat_workspace_t* ws,
                  void* stream)
{
    if (!f || !ws || !y || !k || !g || !wk || !ybar || !ybar_n || !theta || !k_scratch || !parts) return GODE_E_NULLPTR;
    if (!first && !kbar1) return GODE_E_NULLPTR;
    if (!am) return GODE_E_SHAPE;
    const Tableau& tab = am->tab;
    const int S = tab.stages;
    for (int s = 0; s < S; ++s) if (!k[s]) return GODE_E_NULLPTR;
    for (int s = first ? 0 : 1; s < S; ++s) if (!ybar[s]) return GODE_E_NULLPTR;
    if (ybar_n == g || ybar_n == kbar_last || ybar_n == k_scratch || k_scratch == g || k_scratch == kbar_last) return GODE_E_SHAPE;
    if (!first && (kbar1 == g || kbar1 == kbar_last || kbar1 == ybar_n || kbar1 == k_scratch)) return GODE_E_SHAPE;
    for (int s = first ? 0 : 1; s < S; ++s) {
        if (ybar[s] == g || ybar[s] == kbar_last || ybar[s] == ybar_n || (!first && ybar[s] == kbar1) || ybar[s] == k_scratch)
            return GODE_E_SHAPE;
        for (int r = s + 1; r < S; ++r) if (ybar[s] == ybar[r]) return GODE_E_SHAPE;
    }
    int rc = check_sweep(f, ws); if (rc) return rc;
    const int64_t n = f->n, d = f->d, nd = n * d, H = n_heads(f), slot = part_slot(f);
    const int last = first ? 0 : 1;                // the last stage the sweep pushes through f
    bool dead[7] = {};
    float ts[7];
    int live = 0;
    auto cotangent = [&](int s) {
        gode_lincomb_t c = stage_cotangent(tab, g, (float)wk[s], ybar, s, h, dead);
        if (s == S - 1 && kbar_last) { c.coef[c.n] = 1.f; c.ptr[c.n] = kbar_last; ++c.n; }
        return c;
    };
    for (int s = S - 1; s >= last; --s) {
        const gode_lincomb_t cot = cotangent(s);
        if (cot.n == 0) { dead[s] = true; continue; }
        ts[live] = (float)(t + tab.c[s] * h);
        gode_lincomb_t yin = tab_stage_terms(tab, y, k, s, h);
        GODE_TRY(stage_vjp(f, ws, &yin, cot, 1.f, ts[live], k_scratch, ybar[s], nullptr, parts + live * slot, stream));
        ++live;
    }
    // ybar_n = wy g + sum Ybar_s, and (not first) kbar_1 for the step before: one launch
    float* outs[2] = {ybar_n, kbar1};
    gode_lincomb_t lcs[2] = {sweep_pre(tab, g, (float)wy, ybar, last, dead), first ? gode_lincomb_t() : cotangent(0)};
    int64_t lens[2] = {nd, nd};
    int count = first ? 1 : 2;
    if (count == 2 && lcs[1].n == 0) { GODE_TRY(gode_zero_f32(kbar1, nd, stream)); count = 1; }
    GODE_TRY(gode_lincomb_multi_f32(outs, lcs, lens, count, stream));
    if (live == 0) return 0;
    return gode_gat_small_close_stages_f32(parts, n, d, H, live, ts, theta, stream);
}

}  // namespace

// The entry points: the rk4 pair under the 3/8 rule's tableau, the fixed pair under that of its GODE_RK_* code, the dopri5
// sweep under ADAPTIVE[GODE_RKA_DOPRI5] (the adaptive one is below, with the other adaptive steps).
extern "C" int gode_gat_ode_rk4_forward_save(const gode_gat_odefunc_t* f, const float* y0, float* y_end, float* save,
                                             const gode_gat_workspace_t* ws, float t0, float t1, int32_t n_steps,
                                             int32_t step_begin, int32_t step_end, void* stream)
{
    return forward_save(&TAB38, f, y0, y_end, save, ws, t0, t1, n_steps, step_begin, step_end, stream);
}

extern "C" int gode_gat_ode_fixed_forward_save(int32_t method, const gode_gat_odefunc_t* f, const float* y0, float* y_end,
                                               float* save, const gode_gat_workspace_t* ws, float t0, float t1,
                                               int32_t n_steps, int32_t step_begin, int32_t step_end, void* stream)
{
    return forward_save(fixed_tableau(method), f, y0, y_end, save, ws, t0, t1, n_steps, step_begin, step_end, stream);
}

extern "C" int gode_gat_ode_rk4_backprop(const gode_gat_odefunc_t* f, const float* save, float* a, float* theta,
                                         float* const* ybar, float* k_scratch, float* parts, const gode_gat_workspace_t* ws,
                                         float t0, float t1, int32_t n_steps, int32_t step_begin, int32_t step_end,
                                         void* stream)
{
    return backprop(&TAB38, f, save, a, theta, ybar, k_scratch, parts, ws, t0, t1, n_steps, step_begin, step_end, stream);
}

extern "C" int gode_gat_ode_fixed_backprop(int32_t method, const gode_gat_odefunc_t* f, const float* save, float* a,
                                           float* theta, float* const* ybar, float* k_scratch, float* parts,
                                           const gode_gat_workspace_t* ws, float t0, float t1, int32_t n_steps,
                                           int32_t step_begin, int32_t step_end, void* stream)
{
    return backprop(fixed_tableau(method), f, save, a, theta, ybar, k_scratch, parts, ws, t0, t1, n_steps, step_begin, step_end,
                    stream);
}

extern "C" int gode_gat_ode_dopri5_step_backprop(const gode_gat_odefunc_t* f, const float* y, float* const* k, const float* g,
                                                 const float* kbar7, double wy, const double* wk, double t, double h,
                                                 int32_t first, float* const* ybar, float* ybar_n, float* kbar1, float* theta,
                                                 float* k_scratch, float* parts, const gode_gat_workspace_t* ws, void* stream)
{
    return step_backprop(&ADAPTIVE[GODE_RKA_DOPRI5], f, y, k, g, kbar7, wy, wk, t, h, first, ybar, ybar_n, kbar1, theta, k_scratch,
                         parts, ws, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// The adaptive step drivers by method (GODE_RKA_*): the dopri5 steps at the top driven by a tableau and its error weights
// (rk_driver.h: AdaptiveMethod), on the same routes and under every message activation; the sweep is step_backprop.  The forward and the
// adjoint step close with the fused launch of rk.hip (gode_rk_close_err_multi_f32): the solution and the error sums from
// one pass over the stages.  On the one-launch route the adjoint step, given `parts`, leaves each stage's partials in a
// slot of their own and closes the S - 1 stages with ONE gode_gat_small_finish_multi_f32: nothing inside the step reads
// kth[s] / kat[s] before the close.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int gode_gat_ode_adaptive_step_forward(int32_t method, const gode_gat_odefunc_t* f, const float* y,
                                                  float* const* k, float* y1, const gode_gat_workspace_t* w, double t,
                                                  double h, float rtol, float atol, double* sums, void* err_scratch,
                                                  void* stream)
{
    if (!f || !w || !y || !k || !y1 || !sums || !err_scratch) return GODE_E_NULLPTR;
    const AdaptiveMethod* am = adaptive_method(method);
    if (!am) return GODE_E_SHAPE;
    int rc = check_common(f, w, false); if (rc) return rc;
    const Tableau& tab = am->tab;
    const int S = tab.stages;
    for (int s = 0; s < S; ++s) if (!k[s]) return GODE_E_NULLPTR;
    const int64_t nd = f->n * f->d;
    for (int s = 1; s < S; ++s) {
        gode_lincomb_t yin = tab_stage_terms(tab, y, k, s, h);
        GODE_TRY(eval_forward(f, w, &yin, (float)(t + tab.c[s] * h), k[s], stream));
    }
    float ec[GODE_MAX_TERMS];
    const gode_lincomb_t sol = close_terms(*am, y, k, h, ec);
    const float* ecp = ec;
    return gode_rk_close_err_multi_f32(&y1, &sol, &ecp, &nd, 1, rtol, atol, sums, err_scratch, stream);
}

extern "C" int gode_gat_ode_adaptive_step_adjoint(int32_t method, const gode_gat_odefunc_t* f, const float* y, const float* a,
                                                  const float* a_t, const float* theta, float* const* ky, float* const* ka,
                                                  float* const* kat, float* const* kth, float* y1, float* a1, float* a_t1,
                                                  float* theta1, const gode_gat_workspace_t* w, float* parts, double t,
                                                  double h, float rtol, float atol, double* sums /* 4 */, void* err_scratch,
                                                  void* stream)
{
    if (!f || !w || !y || !a || !a_t || !theta || !ky || !ka || !kat || !kth || !y1 || !a1 || !a_t1 || !theta1 || !sums ||
        !err_scratch) return GODE_E_NULLPTR;
    const AdaptiveMethod* am = adaptive_method(method);
    if (!am) return GODE_E_SHAPE;
    int rc = check_common(f, w, true); if (rc) return rc;
    const Tableau& tab = am->tab;
    const int S = tab.stages;
    for (int s = 0; s < S; ++s) if (!ky[s] || !ka[s] || !kat[s] || !kth[s]) return GODE_E_NULLPTR;
    const int64_t nd = f->n * f->d, H = n_heads(f), P = gode_gat_ode_theta_len_heads(f->d, H);
    const bool multi = parts && w->small_part && small_dense(f);      // the stages' closing launches as one
    const int64_t slot = multi ? part_slot(f) : 0;
    float tsv[7];
    for (int s = 1; s < S; ++s) {
        gode_lincomb_t yin = tab_stage_terms(tab, y, ky, s, h);
        gode_lincomb_t ain = tab_stage_terms(tab, a, ka, s, h);
        tsv[s - 1] = (float)(t + tab.c[s] * h);
        GODE_TRY(eval_adjoint(f, w, yin, ain, tsv[s - 1], ky[s], ka[s], kat[s], kth[s], stream,
                              multi ? parts + (s - 1) * slot : nullptr));
    }
    if (multi) GODE_TRY(gode_gat_small_finish_multi_f32(parts, f->n, f->d, H, S - 1, kth + 1, kat + 1, tsv, stream));
    // one close for the four outputs and the four error groups y, a, a_t, theta, each group the decomposition the separate
    // error norm gives it
    float ec[4][GODE_MAX_TERMS];
    const gode_lincomb_t sols[4] = {close_terms(*am, y, ky, h, ec[0]), close_terms(*am, a, ka, h, ec[1]),
                                    close_terms(*am, a_t, kat, h, ec[2]), close_terms(*am, theta, kth, h, ec[3])};
    float* outs[4] = {y1, a1, a_t1, theta1};
    const float* ecs[4] = {ec[0], ec[1], ec[2], ec[3]};
    const int64_t lens[4] = {nd, nd, 1, P};
    return gode_rk_close_err_multi_f32(outs, sols, ecs, lens, 4, rtol, atol, sums, err_scratch, stream);
}

extern "C" int gode_gat_ode_adaptive_step_backprop(int32_t method, const gode_gat_odefunc_t* f, const float* y,
                                                   float* const* k, const float* g, const float* kbar_last, double wy,
                                                   const double* wk, double t, double h, int32_t first, float* const* ybar,
                                                   float* ybar_n, float* kbar1, float* theta, float* k_scratch, float* parts,
                                                   const gode_gat_workspace_t* ws, void* stream)
{
    return step_backprop(adaptive_method(method), f, y, k, g, kbar_last, wy, wk, t, h, first, ybar, ybar_n, kbar1, theta,
                         k_scratch, parts, ws, stream);
}
