// ode_driver.hip — whole fixed-grid integrations of the GCN ODE function as ONE C-ABI call.
//
// The reference drives its ODE function from Python (torchdiffeq, call site GCN/models.py:192).  On
// citation-graph sizes (Cora: 2708 x 16 state) every kernel runs for a few microseconds, so the
// integration is bound by the host's per-launch cost; these entry points issue the complete launch
// sequence of a forward solve, an adjoint solve or a backprop sweep from C with no allocation and no
// synchronisation, which also makes the call capturable into a HIP graph by the caller.
// Launch sequence per stage = graph_odenet_amd/gcn_ode.py (GcnOdeField / GcnOdeAdjointField).
//
// Every launch sequence is stated once, over a tableau (tables and term lists: rk_driver.h); no method has a copy of its own:
//   feval_large         Gf then Sp of one evaluation on the large route (optionally closing a step, optionally keeping k_S)
//   fixed_forward_step  one step of a fixed-grid forward solve, fused or large route
//   forward_solve / forward_save   fixed_forward_step per step, swapping buffers / into records
//   adjoint_small_step / fixed_adjoint_small   a step / the solve of the fused launch-bound schedule of a fixed-grid adjoint solve
//   close_bias / close_weight / close_affine    the reductions that close a stage's parameter derivative, large route
//   stage_finish_merged the same as ONE launch, launch-bound sizes
//   sweep_stage         one stage of a reverse sweep on the multi-launch routes
//   backprop            the reverse sweep over forward_save's records: the fused sweep, or sweep_stage per stage
//   step_backprop       the reverse sweep over one accepted step of an adaptive method
//   sweep_pre           the terms a backprop step's last launch adds up to abar_n
// and the entry points name a tableau and call them.  A body validates, in the order its entry points always did; it takes
// the tableau by pointer, NULL being a method code outside the list, refused where the by-method entry point refused it:
//   gode_gcn_ode_rk4_forward, _rk4_forward_save, _rk4_backprop     forward_solve, forward_save, backprop under TAB38
//   gode_gcn_ode_fixed_forward, _fixed_forward_save, _fixed_backprop   the same under fixed_tableau(method)
//   gode_gcn_ode_rk4_adjoint     fixed_adjoint_small under TAB38, or the two-chain loop: Gf (one lambda), Sp, SpT, dense VJP,
//                                close_* (the 3/8 rule's alone); gode_gcn_ode_fixed_adjoint: fixed_adjoint_small, rk4 to the former
//   gode_gcn_ode_dopri5_step_backprop, gode_gcn_ode_adaptive_step_backprop   step_backprop under ADAPTIVE[..]
//   gode_gcn_ode_dopri5_step_forward / _adjoint   dp_eval_forward (feval_large) / dp_eval_adjoint (close_*) per stage; the
//                                adaptive_step_forward / _adjoint run the same stages and close the step with ONE fused launch
//                                where these use two, so the two pairs stay apart
//   gode_gcn_ode_adams_*         fixed_forward_step / adjoint_small_step under TAB38 for the start-up steps
#include <map>
#include <mutex>
#include <utility>
#include "rk_driver.h"
#include "dense_pc.h"
#include "options.h"

namespace {

int spmm(const gode_graph_t& g, const float* X, float* Y, int64_t d, const gode_spmm_epilogue_t* ep, void* s) {
    return gode_spmm_csr_f32(g.rowptr, g.col, g.val, g.items, g.n_items, g.long_rows, g.n_long, g.partial,
                             X, d, Y, d, g.n_rows, d, ep, s);
}
// relu(. + b): the epilogue of every Sp
gode_spmm_epilogue_t relu_bias_epilogue(const gode_gcn_odefunc_t* f) {
    gode_spmm_epilogue_t ep = {};
    ep.bias = f->b; ep.relu = 1; ep.alpha = 1.f;
    return ep;
}

// theta-k layout: [ W ((d+1)*d) | b (d) | gamma (d) | beta (d) | a_t (1) ]
// after the weight-gradient reduction row 0 of W holds colsum(dS):  a_t' = row0 . W[0,:],  row0 *= t
__global__ void theta_fixup_kernel(float* ktheta, const float* W, float t, int d, int64_t off_at) {
    __shared__ float sm[4];
    float s = 0.f;
    for (int c = threadIdx.x; c < d; c += blockDim.x) s += ktheta[c] * W[c];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) ktheta[off_at] = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += blockDim.x) ktheta[c] *= t;
}

// Closing a stage's parameter derivative kt on the large route, slot by slot (the schedules place the three on different
// streams, with launches and event waits between them).
// b: column sums of `src` - dZ itself (n rows), or the per-block column sums an earlier launch of the stage left
int close_bias(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, float* kt, const float* src, int64_t rows,
               void* stream) {
    return gode_colsum_f32(kt + (f->d + 1) * f->d, src, rows, f->d, 1.f, 0, ws->colsum_scratch, stream);
}
// W from the `parts` block partials in ws->wpart, then the time-row bookkeeping (a_t; row 0 *= ts)
int close_weight(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, float* kt, int64_t parts, float ts,
                 void* stream) {
    const int64_t d = f->d;
    GODE_TRY(gode_reduce_parts_f32(kt, ws->wpart, parts, (d + 1) * d, 1.f, 0, stream));
    hipLaunchKernelGGL(theta_fixup_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, kt, f->W, ts, (int)d,
                       gode_gcn_ode_theta_len(d) - 1);
    GODE_LAUNCH_CHECK();
    return 0;
}
// gamma, beta from the dense VJP's block partials (zeros without GroupNorm)
int close_affine(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, float* kt, void* stream) {
    const int64_t d = f->d;
    float* kg = kt + (d + 1) * d + d;
    if (f->groups <= 0) return gode_zero_f32(kg, 2 * d, stream);
    return gode_reduce_parts2_f32(kg, ws->gpart, kg + d, ws->bpart, gode_gemm_bwd_parts(f->n), d, 1.f, 0, stream);
}

// Launch-bound graphs: the four reduction launches that close an adjoint stage (weight-gradient partials, time-row
// bookkeeping, bias column sums, GroupNorm affine partials) as ONE launch (rk.hip: reduce_segments_kernel), up to
// kMergedFinishMaxRows rows.
// kt = [W | b | gamma | beta | a_t] from ws->wpart, colsum partials of dZ, ws->gpart / ws->bpart
int stage_finish_merged(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, float* kt, float ts, void* stream) {
    const int64_t n = f->n, d = f->d, nW = (d + 1) * d, P = gode_gcn_ode_theta_len(d);
    int64_t cparts = 0;
    GODE_TRY(gode_colsum_parts_f32(ws->dZ, n, d, (float*)ws->colsum_scratch, &cparts, stream));
    const int64_t gp = gode_gemm_bwd_parts(n);
    gode_reduce_seg_t sg[4] = {};
    sg[0] = {kt, ws->wpart, gode_wgrad_parts(n), nW, 0, 1, nW, f->W, d};                       // dW; row 0 is the time row
    sg[1] = {kt + nW, (const float*)ws->colsum_scratch, cparts, d, 0, 1, d, nullptr, 0};           // bias: colsum(dZ)
    sg[2] = {kt + nW + d, ws->gpart, gp, d, 0, 1, d, nullptr, 0};
    sg[3] = {kt + nW + 2 * d, ws->bpart, gp, d, 0, 1, d, nullptr, 0};
    GODE_TRY(gode_reduce_segments_f32(sg, f->groups > 0 ? 4 : 2, ts, kt + (P - 1), stream));
    if (f->groups <= 0) GODE_TRY(gode_zero_f32(kt + nW + d, 2 * d, stream));
    return 0;
}

// Launch-bound graphs: ONE launch per f-eval and one per VJP (csrc/small.hip) instead of 2 + 8
bool fused_small(const gode_gcn_odefunc_t* f) {
    return gode_opt_small_fused() && gode_gcn_small_supported(f->n, f->d, f->groups);
}

// Closing combination of a step formed ONCE (option rk_close_once; large route: no fused launch, > 65 536 rows, d = 128).
// The last stage's input  y + h (k0 - k1 + k2)  and the closing combination  P = y + h/8 k0 + 3h/8 k1 + 3h/8 k2  are
// combinations of the same four arrays in the same order, so the launch that loads them for the one also stores the
// other (dense product: aux output; SpMM: third output) and the closing launch reads {1.0, P} - one array instead of
// four.  P is formed with the multiply-add chain every kernel forms a combination with (lc_load4_n), and a one-term
// {1.0, P} reproduces P exactly, so every result keeps its bits.
bool close_once_route(const gode_gcn_odefunc_t* f) {
    return gode_opt_rk_close_once() && !fused_small(f) && f->n > kMergedFinishMaxRows && f->d == 128;
}

// Gf of a last stage (input terms xin) that also leaves P (terms pre) in `p_out`.  *formed = false (and the plain launch
// issued) where the kernel the options select cannot: the caller then closes the step from the four terms as before.
// diag_taken (forward solve, no x_out; the ODE function carries A's core list): the launch may also close the
// diagonal-only rows, p_out[i] = P[i] + alpha relu(a_ii S[i] + b), and says in *diag_taken whether it did.
int gf_last_stage(const gode_gcn_odefunc_t* f, const gode_lincomb_t& xin, const gode_lincomb_t& pre, float t, float* S,
                  float* x_out, float* p_out, bool* formed, void* stream, float alpha = 0.f, int32_t* diag_taken = nullptr) {
    *formed = false;
    bool distinct = p_out != S && p_out != x_out;
    for (int j = 0; j < xin.n; ++j) distinct = distinct && p_out != xin.ptr[j];
    if (distinct && xin.n == pre.n) {       // same arrays in the same order (every A38[3][j] is non-zero)
        const int rc = (diag_taken && !x_out)
            ? gode_gn_time_gemm_diag_aux_f32(&xin, f->n, f->d, f->groups, f->eps, f->gamma, f->beta, f->W, f->d, 1, t, S,
                                             pre.coef, p_out, alpha, f->a_diag, f->at_diag, f->b, diag_taken, stream)
            : gode_gn_time_gemm_xout_aux_f32(&xin, f->n, f->d, f->groups, f->eps, f->gamma, f->beta, f->W, f->d, 1, t, S,
                                             x_out, pre.coef, p_out, stream);
        if (rc != GODE_E_UNSUPPORTED) { *formed = rc == 0; return rc; }
    }
    return gode_gn_time_gemm_xout_f32(&xin, f->n, f->d, f->groups, f->eps, f->gamma, f->beta, f->W, f->d, 1, t, S, x_out, stream);
}

// How an evaluation closes a step:  out = sum pre + alpha * f(t, x);  once: the closing-combination-once route
struct StepClose { gode_lincomb_t pre; float alpha; bool once; };

// Gf then Sp of one evaluation on the large route: out = f(t, sum xin) through S, or the closed step (`close`).  On the
// once route Gf leaves the closing combination in `out`, which Sp then reads and overwrites.  k_save: Sp also stores the
// plain derivative there (the k_4 a backprop record keeps).
// diag_ok (plain evaluations, and the closed step on the once route without k_save under option diag_last): the ODE
// function carries A's core list and the caller runs the forward rk4 solve - Gf also stores `out` of the diagonal-only
// rows and Sp runs without them, where Gf reports that it did (per launch: the fp32-MFMA forward kernel, option fwd_pc
// 0, has no such form)
int feval_large(const gode_gcn_odefunc_t* f, const gode_lincomb_t& xin, float t, float* S, float* out,
                const StepClose* close, float* k_save, void* stream, bool diag_ok = false) {
    const int64_t d = f->d;
    bool p_formed = false;
    if (diag_ok && !close && !k_save) {
        int32_t taken = 0;
        GODE_TRY(gode_gn_time_gemm_diag_f32(&xin, f->n, d, f->groups, f->eps, f->gamma, f->beta, f->W, d, 1, t, S, f->a_diag,
                                            f->at_diag, f->b, out, &taken, stream));
        gode_spmm_epilogue_t ep = relu_bias_epilogue(f);
        if (!taken) return spmm(f->A, S, out, d, &ep, stream);
        ep.n_items_full = f->A.n_items;                         // same kernels, same name in the profile
        const gode_graph_t& g = f->A;
        return gode_spmm_csr_f32(g.rowptr, g.col, g.val, f->a_core_items, f->a_n_core, g.long_rows, g.n_long, g.partial,
                                 S, d, out, d, g.n_rows, d, &ep, stream);
    }
    int32_t last_taken = 0;
    if (close && close->once) {
        const bool diag_last = diag_ok && !k_save && gode_opt_diag_last();
        GODE_TRY(gf_last_stage(f, xin, close->pre, t, S, nullptr, out, &p_formed, stream, close->alpha,
                               diag_last ? &last_taken : nullptr));
    } else {
        GODE_TRY(gode_gn_time_gemm_f32(&xin, f->n, d, f->groups, f->eps, f->gamma, f->beta, f->W, d, 1, t, S, stream));
    }
    gode_spmm_epilogue_t ep = relu_bias_epilogue(f);
    if (close) { ep.pre = p_formed ? one_term(out) : close->pre; ep.alpha = close->alpha; }
    const gode_graph_t& g = f->A;
    if (last_taken) {                                           // `out` holds y_new on the diagonal-only rows, P elsewhere
        ep.n_items_full = g.n_items;
        return gode_spmm_csr_f32(g.rowptr, g.col, g.val, f->a_core_items, f->a_n_core, g.long_rows, g.n_long, g.partial,
                                 S, d, out, d, g.n_rows, d, &ep, stream);
    }
    if (!k_save) return spmm(f->A, S, out, d, &ep, stream);
    return gode_spmm_csr_save_f32(g.rowptr, g.col, g.val, g.items, g.n_items, g.long_rows, g.n_long, g.partial,
                                  S, d, out, d, g.n_rows, d, &ep, k_save, stream);
}

// the closing-combination-once launch needs the last stage's input and the closing combination to name the same arrays in
// the same order, and saves something only where they are several (the 3/8 rule).  The midpoint rule's differ and explicit
// Euler's is y alone: both close from their terms - one array, as the once route reads.
bool same_arrays(const gode_lincomb_t& x, const gode_lincomb_t& p) {
    if (x.n != p.n || x.n < 2) return false;
    for (int j = 0; j < x.n; ++j) if (x.ptr[j] != p.ptr[j]) return false;
    return true;
}

// One step of the forward solve from y at time t: k_1..k_{S-1} into k[0..S-2], y_{n+1} into ynext (which may be k[S-1]: the
// folded last stage never materialises k_S) - or, keep_last, k_S into k[S-1] as well (ynext is then another array).
int fixed_forward_step(const Tableau& tab, const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, const float* y,
                       float* const* k, float* ynext, bool keep_last, double t, double h, bool fused, bool close_once,
                       void* stream, bool diag_ok = false) {
    const int S = tab.stages;
    for (int s = 0; s < S; ++s) {
        const gode_lincomb_t xin = tab_stage_terms(tab, y, k, s, h);
        const float ts = (float)(t + tab.c[s] * h);
        if (s + 1 < S) {
            if (fused) GODE_TRY(gode_gcn_feval_small_f32(f, &xin, ts, 1.f, nullptr, nullptr, nullptr, k[s], stream));
            else GODE_TRY(feval_large(f, xin, ts, ws->S, k[s], nullptr, nullptr, stream, diag_ok));
            continue;
        }
        StepClose close = {tab_combine_terms(tab, y, k, h), (float)(h * tab.b[s]), close_once};
        close.once = close_once && same_arrays(xin, close.pre);
        float* klast = keep_last ? k[s] : nullptr;
        if (!fused) GODE_TRY(feval_large(f, xin, ts, ws->S, ynext, &close, klast, stream, diag_ok));
        else if (keep_last) GODE_TRY(gode_gcn_feval_small_save_f32(f, &xin, ts, close.alpha, &close.pre, ynext, klast, stream));
        else GODE_TRY(gode_gcn_feval_small_f32(f, &xin, ts, close.alpha, &close.pre, nullptr, nullptr, ynext, stream));
    }
    return 0;
}

// diagonal-only rows of A (option diag_rows; large route at d = 128): stages before the last, and on the closing-combination-
// once route the last stage as well (option diag_last): the producer waves of its dense launch hand the closing combination
// to the consumer waves through LDS, and the consumer is the only writer of a diagonal-only row of y_new.
bool diag_rows_route(const gode_gcn_odefunc_t* f, bool fused) {
    return gode_opt_diag_rows() && !fused && f->n > kMergedFinishMaxRows && f->d == 128 && f->a_core_items && f->a_diag &&
           f->at_diag && f->A.items && f->a_n_core > 0 && f->a_n_core <= f->A.n_items;
}

// Side stream + events for the two-chain schedule of the adjoint solve (and the tail launch of the forward solve:
// tail_in / tail_out): one set per (device, caller stream), created
// on first use and kept for the life of the process, so that two caller streams (or two threads, each on its own
// stream) never share a side stream or an event.  The map is the only mutable state here and is mutex-guarded.
struct Overlap {
    hipStream_t side = nullptr;
    hipEvent_t sp = nullptr, gf = nullptr, spt = nullptr, wg = nullptr, tail_in = nullptr, tail_out = nullptr;
    bool ok = false;
};
Overlap* overlap_ctx(hipStream_t caller) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, Overlap*> ctxs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto key = std::make_pair(dev, caller);
    auto it = ctxs.find(key);
    if (it != ctxs.end()) return it->second;
    Overlap* c = new Overlap();
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) == hipSuccess) {
        bool ok = true;
        for (hipEvent_t* ev : {&c->sp, &c->gf, &c->spt, &c->wg, &c->tail_in, &c->tail_out})
            ok = ok && hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess;
        c->ok = ok;
    }
    ctxs[key] = c;
    return c;
}

// Isolated rows at the end of the state (option local_tail; gode_gcn_odefunc_t: n_tail).  Such a row's ODE is local to
// the row, so one launch integrates rows [n - n_tail, n) over the whole solve (gemm_pc.hip: gcn_local_tail_rk4_kernel,
// the statements of the DIAG launches on the same numbers: same bits) and every dense launch of the solve runs on the
// rows before them.  The SpMM launches never held those rows (A's core list).  Only where EVERY dense launch of the
// solve takes its DIAG form - otherwise another kernel's arithmetic would have made those rows.
// -> channels per GroupNorm group of the tail kernel (0 / 4), or -1: no tail launch.
int local_tail_cg(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, const float* y, bool diag_ok, bool close_once) {
    if (!gode_opt_local_tail() || !diag_ok || !close_once || !gode_opt_diag_last() || gode_opt_fwd_pc() != 3) return -1;
    if (f->n_tail <= 0 || f->n_tail >= f->n || f->n - f->n_tail <= kMergedFinishMaxRows) return -1;
    const int cg = f->groups == 0 ? 0 : (f->groups > 0 && f->d % f->groups == 0 && f->d / f->groups == 4) ? 4 : -1;
    uintptr_t bits = (uintptr_t)y | (uintptr_t)ws->S | (uintptr_t)f->W | (uintptr_t)f->b | (uintptr_t)f->gamma | (uintptr_t)f->beta;
    for (int j = 0; j < 4; ++j) bits |= (uintptr_t)ws->ky[j];
    return (bits & 15) || !f->W || !f->b ? -1 : cg;
}

// The launches of the tail solve on stream s: n_steps steps from y's tail rows into those of `res` (y itself is fine: a
// block reads its tile before it writes it).  A launch covers GODE_LOCAL_TAIL_MAX_STEPS steps; further ones go on in `res`.
int local_tail_solve(const gode_gcn_odefunc_t* f, const float* y, float* res, float t0, double h, int32_t n_steps, int cg,
                     int blocks, hipStream_t s) {
    const int64_t off = (f->n - f->n_tail) * f->d;
    float* const kdummy[4] = {nullptr, nullptr, nullptr, nullptr};
    LocalTailSteps st = {};
    for (int q = 0; q < 4; ++q) {
        const gode_lincomb_t lc = tab_stage_terms(TAB38, nullptr, kdummy, q, h);
        if (lc.n != q + 1) return GODE_E_UNSUPPORTED;
        for (int j = 0; j <= q; ++j) st.coef[q][j] = lc.coef[j];
    }
    const gode_lincomb_t pre = tab_combine_terms(TAB38, nullptr, kdummy, h);
    for (int j = 0; j < 4; ++j) st.acoef[j] = pre.coef[j];
    st.alpha = (float)(h * B38[3]);
    const float* src = y + off;
    for (int i0 = 0; i0 < n_steps; i0 += GODE_LOCAL_TAIL_MAX_STEPS) {
        st.n_steps = n_steps - i0 < GODE_LOCAL_TAIL_MAX_STEPS ? n_steps - i0 : GODE_LOCAL_TAIL_MAX_STEPS;
        for (int i = 0; i < st.n_steps; ++i)
            for (int q = 0; q < 4; ++q) st.ts[i][q] = (float)(((double)t0 + (i0 + i) * h) + C38[q] * h);   // fixed_forward_step's
        GODE_TRY(gode_pc_local_tail_launch(src, res + off, f->n_tail, f->a_diag + (f->n - f->n_tail), f->eps, f->gamma, f->beta,
                                           f->W, f->b, st, cg, blocks, s));
        src = res + off;
    }
    return 0;
}

// The forward solve of a fixed-grid method (tabp == NULL, here and in the bodies below: a code outside GODE_RK_*, refused
// after the null checks): fixed_forward_step per step, the solution and k[S-1] swapping.
int forward_solve(const Tableau* tabp, const gode_gcn_odefunc_t* f, float* y, float** result, const gode_rk4_workspace_t* ws,
                  float t0, float t1, int32_t n_steps, void* stream)
{
    if (!f || !y || !ws || !result) return GODE_E_NULLPTR;
    if (!tabp) return GODE_E_SHAPE;
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    const Tableau& tab = *tabp;
    const int S = tab.stages, L = S - 1;
    if (!ws->S) return GODE_E_NULLPTR;
    for (int s = 0; s < S; ++s) if (!ws->ky[s]) return GODE_E_NULLPTR;
    const double h = ((double)t1 - (double)t0) / n_steps;
    float* cur = y;
    float* k[4] = {ws->ky[0], ws->ky[1], ws->ky[2], ws->ky[3]};
    const bool fused = fused_small(f);
    const bool close_once = close_once_route(f);
    const bool diag_ok = diag_rows_route(f, fused);
    // isolated tail rows (option local_tail; the 3/8 rule only: the tail kernel integrates its step): one launch of their own
    // writes them into the buffer *result will name (the buffers swap once per step); the steps below then run their dense
    // launches on the rows before the tail.  Outside a capture and with option overlap the launch goes to the side stream,
    // beside the solve's HBM-bound SpMM launches: it waits for what the caller's stream held at entry, and the caller's
    // stream joins it before the return.
    // (the pointer test is sound inside this file: TAB38 has one copy per translation unit, and fixed_tableau() of this one returns it)
    const int tail_cg = tabp == &TAB38 ? local_tail_cg(f, ws, y, diag_ok, close_once) : -1;
    gode_gcn_odefunc_t fcore;
    Overlap* ov = nullptr;
    if (tail_cg >= 0) {
        hipStream_t hs = (hipStream_t)stream;
        float* res = (n_steps & 1) ? ws->ky[3] : y;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (gode_opt_overlap() && hipStreamIsCapturing(hs, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
            ov = overlap_ctx(hs);
            if (ov && !ov->ok) ov = nullptr;
        }
        if (ov) {
            GODE_HIP(hipEventRecord(ov->tail_in, hs));
            GODE_HIP(hipStreamWaitEvent(ov->side, ov->tail_in, 0));
        }
        // grid (measured at 2^20 x 128, 45 % of the rows in the tail): beside the solve 128 blocks - the
        // dense launches want whole CUs, and a chip-filling tail launch makes them queue behind it; alone on the caller's
        // stream the full chip, two blocks per CU (128 blocks there take twice as long as the launches they replace save)
        const int blocks = gode_opt_local_tail_blocks() > 0 ? gode_opt_local_tail_blocks() : ov ? 128 : 512;
        const int rc = local_tail_solve(f, y, res, t0, h, n_steps, tail_cg, blocks, ov ? ov->side : hs);
        if (ov) {                                      // joined on every path: the side stream never outlives the call
            (void)hipEventRecord(ov->tail_out, ov->side);
            if (rc) (void)hipStreamWaitEvent(hs, ov->tail_out, 0);
        }
        if (rc) return rc;
        fcore = *f;
        fcore.n = f->n - f->n_tail;                     // Gf of every stage; the SpMM launches take their rows from f->A
        f = &fcore;
    }
    int rc = 0;
    for (int i = 0; i < n_steps && !rc; ++i) {
        rc = fixed_forward_step(tab, f, ws, cur, k, k[L], false, (double)t0 + i * h, h, fused, close_once, stream, diag_ok);
        float* tmp = cur; cur = k[L]; k[L] = tmp;      // k[L] holds the new solution
    }
    if (ov) GODE_HIP(hipStreamWaitEvent((hipStream_t)stream, ov->tail_out, 0));
    if (rc) return rc;
    *result = cur;
    return 0;
}

// One step of the adjoint solve on launch-bound graphs, fused launches, from (y, a) at time t: two launches per stage - f-eval
// (+ masked cotangent dZ), VJP (+ block partials) - and one more, which adds h * sum_s b_s ktheta_s to theta straight from
// the stages' block partials (w0_extra: added to the first stage's weight h b_1 - explicit_adams' start-up steps); a single
// stream.  The new y and a are left in ky[S-1] and ka[S-1].  Any tableau of up to 4 stages.
int adjoint_small_step(const Tableau& tab, const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, const float* y,
                       float* const* ky, const float* a, float* const* ka, float* theta, double t, double h, double w0_extra,
                       void* stream) {
    const int S = tab.stages, L = S - 1;
    const int64_t slot = gode_gcn_small_parts(f->n) * gode_gcn_small_part_len(f->d);
    const float hbl = (float)(h * tab.b[L]);
    float stage_t[4], wb[4];
    const gode_lincomb_t ypre = tab_combine_terms(tab, y, ky, h), apre = tab_combine_terms(tab, a, ka, h);
    for (int s = 0; s < S; ++s) {
        stage_t[s] = (float)(t + tab.c[s] * h);
        wb[s] = (float)(h * tab.b[s] + (s == 0 ? w0_extra : 0.0));
        const gode_lincomb_t yin = tab_stage_terms(tab, y, ky, s, h);
        const gode_lincomb_t cot = negated(tab_stage_terms(tab, a, ka, s, h));          // cotangent of the VJP is -a
        GODE_TRY(gode_gcn_feval_small_f32(f, &yin, stage_t[s], s == L ? hbl : 1.f, s == L ? &ypre : nullptr,
                                          &cot, ws->dZ, ky[s], stream));
        GODE_TRY(gode_gcn_vjp_small_f32(f, &yin, ws->dZ, s == L ? hbl : 1.f, s == L ? &apre : nullptr,
                                        ka[s], ws->small_part + s * slot, stream));
    }
    // every weight rounded to zero (an empty or denormal-sized interval): the launch below refuses such a step, and theta stays
    bool any = false;
    for (int s = 0; s < S; ++s) any = any || wb[s] != 0.f;
    if (!any) return 0;
    return gode_gcn_small_finish_step_f32(f, ws->small_part, S, theta, wb, stage_t, stream);
}

// The whole solve: adjoint_small_step per step, the solutions and ky[S-1] / ka[S-1] swapping
int fixed_adjoint_small(const Tableau& tab, const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, float* y, float* a,
                        float* theta, float** y_result, float** a_result, float t0, double h, int32_t n_steps, void* stream) {
    const int L = tab.stages - 1;
    float* ycur = y; float* acur = a;
    float* ky[4] = {ws->ky[0], ws->ky[1], ws->ky[2], ws->ky[3]};
    float* ka[4] = {ws->ka[0], ws->ka[1], ws->ka[2], ws->ka[3]};
    for (int i = 0; i < n_steps; ++i) {
        GODE_TRY(adjoint_small_step(tab, f, ws, ycur, ky, acur, ka, theta, (double)t0 + i * h, h, 0.0, stream));
        float* tmp = ycur; ycur = ky[L]; ky[L] = tmp;
        tmp = acur; acur = ka[L]; ka[L] = tmp;
    }
    *y_result = ycur;
    *a_result = acur;
    return 0;
}

}  // namespace

extern "C" int64_t gode_gcn_ode_theta_len(int64_t d) { return (d + 1) * d + 3 * d + 1; }

extern "C" int gode_gcn_ode_rk4_forward(const gode_gcn_odefunc_t* f, float* y, float** result,
                                        const gode_rk4_workspace_t* ws, float t0, float t1, int32_t n_steps,
                                        void* stream)
{
    return forward_solve(&TAB38, f, y, result, ws, t0, t1, n_steps, stream);
}

// Adjoint solve.  Per stage the launches form two chains:
//   F (forward recompute):  Gf(s) = [t|GN(y_s)]W  ->  Sp(s) = relu(A . + b) (+ masked cotangent dZ)
//   B (vector-Jacobian)  :  SpT(s) = A^T dZ  ->  Gb(s) (k_a)  |  Wg(s) (dW partials)  |  colsum(dZ), reductions
// Gf(s+1) needs only k_y(s).  The SpMM launches (HBM-bound) run alone; the three MFMA-bound launches that follow
// SpT(s) run side by side: Gb(s) on the caller's stream, Wg(s) then Gf(s+1) on a side stream - each of them alone
// keeps the matrix pipe ~50 % busy (S is double-buffered when ws->S2 is given; events order every buffer reuse).
extern "C" int gode_gcn_ode_rk4_adjoint(const gode_gcn_odefunc_t* f, float* y, float* a, float* theta,
                                        float** y_result, float** a_result,
                                        const gode_rk4_workspace_t* ws, float t0, float t1, int32_t n_steps,
                                        void* stream)
{
    if (!f || !y || !a || !theta || !ws || !y_result || !a_result) return GODE_E_NULLPTR;
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    for (int s = 0; s < 4; ++s) if (!ws->ky[s] || !ws->ka[s] || !ws->ktheta[s]) return GODE_E_NULLPTR;
    if (!ws->S || !ws->dZ || !ws->dS || !ws->wpart || !ws->colsum_scratch) return GODE_E_NULLPTR;
    if (f->groups > 0 && (!ws->gpart || !ws->bpart)) return GODE_E_NULLPTR;
    const int64_t n = f->n, d = f->d;
    const double h = ((double)t1 - (double)t0) / n_steps;   // negative: the adjoint runs from t0 (later) to t1 (earlier)
    if (fused_small(f) && ws->small_part != nullptr)
        return fixed_adjoint_small(TAB38, f, ws, y, a, theta, y_result, a_result, t0, h, n_steps, stream);
    hipStream_t hs = (hipStream_t)stream;
    // the side stream exists only for callers that ask for the two-chain schedule (never created inside a capture:
    // odeint turns the option off around its HIP-graph captures)
    // launch-bound sizes gain nothing from the second stream and close every stage with one merged reduction launch
    const bool small = f->n <= kMergedFinishMaxRows;
    Overlap* ov = (!small && ws->S2 != nullptr && gode_opt_overlap()) ? overlap_ctx(hs) : nullptr;
    const bool two = ov != nullptr && ov->ok;
    void* side = two ? (void*)ov->side : stream;
    float* Sbuf[2] = {ws->S, two ? ws->S2 : ws->S};
    float* ycur = y; float* acur = a;
    float* ky[4] = {ws->ky[0], ws->ky[1], ws->ky[2], ws->ky[3]};
    float* ka[4] = {ws->ka[0], ws->ka[1], ws->ka[2], ws->ka[3]};
    const int64_t wparts = gode_wgrad_parts(n);
    const int total = 4 * n_steps;
    // d = 128 on large graphs: Gb(s) and Wg(s) as ONE pass over x and dS (gemm_pc.hip: gn_gemm_bwd_wgrad_pc_kernel)
    const bool bw = !small && gode_bwd_wgrad_supported(n, d, d, f->groups) && gode_bwd_wgrad_parts(n) <= wparts;
    // colsum(dZ), the bias gradient of a stage: from the per-block column sums Sp(g) leaves in ws->y2_colsum (1/8 of
    // dZ's bytes) when the workspace has them and the graph runs on the kernels that form them
    const int64_t y2rows = (bw && ws->y2_colsum && gode_opt_y2_colsum())
        ? gode_spmm_y2_colsum_rows(f->A.items ? f->A.n_items : f->A.n_rows, f->A.items ? f->A.n_long : 0, d) : 0;

    // Stage inputs with 3 or 4 terms (stages 2 and 3 of the 3/8 rule) are written out by their Gf launch so that
    // Gb and Wg read ONE n x d array instead of the term list (measured at C5: Gb 0.78 -> 0.42 ms, Wg 0.56 -> 0.43 ms
    // for +0.10 ms in Gf).  X[g&1]: Gf(g+2) is ordered after Gb(g) and Wg(g) by the spt event / side-stream order.
    const bool mat = ws->X[0] != nullptr && ws->X[1] != nullptr;
    auto x_out_of = [&](int g) -> float* { return (mat && (g % 4) >= 2) ? ws->X[g & 1] : nullptr; };
    auto stage_time = [&](int g) { return (float)((double)t0 + (g / 4) * h + C38[g % 4] * h); };

    // the closing combinations of a step formed once (bw branch): P_y by Gf of the last stage into ky[3], P_a by Sp(3) into
    // ka[3]; Sp(3) and the stage-3 dense launch read and overwrite them in place, row by row (the SpMM's lane group and
    // its finishing launch load the pre-terms of the row they then store; the consumer lane of the dense launch loads
    // pre[row, c0..c0+3] and stores dx[row, c0..c0+3]).  ky[3] / ka[3] hold the state two steps back: their last readers
    // are launches of the previous step on the caller's stream, ahead of these in stream order.
    const bool close_once = bw && close_once_route(f);
    bool py_formed = false;
    // Isolated rows (option diag_rows; one-pass branch only): (A^T dZ)[i] = a_ii dZ[i] needs no gather and nobody gathers
    // dZ[i], so Sp(g) stores a_ii dZ[i] straight into dS and SpT(g) runs on A^T's list without those rows.  The bias
    // gradient must come from Sp(g)'s per-block column sums: those rows of dZ itself are not written.
    const bool at_core = bw && y2rows > 0 && gode_opt_diag_rows() && f->at_core_items && f->at_diag && f->AT.items &&
                         f->at_n_core > 0 && f->at_n_core <= f->AT.n_items;
    // Isolated tail rows (option adjoint_tail; with at_core): rows [n - n_tail, n) gather nothing, so what Gf(g) and Sp(g)
    // make of them - k_y (or the closed step), a_ii dZ[i] into dS, x_out, the closing combination of the cotangent - is
    // row-local work on a number Gf(g) held in registers.  Gf(g) runs on the rows before the tail, one dense launch of
    // their own (gemm_pc.hip: gcn_adjoint_tail_kernel, the statements of the pair on the same numbers: same bits)
    // recomputes the stage on the tail, and Sp(g) runs on A's record list without the tail's records (launched with the
    // whole list's count: the same kernels).  The S and dZ rows of the tail are never stored.  The tail's records are the
    // last of A's list, in row order (gode_gcn_odefunc_t: a_head_items), and the launch starts on a block boundary of that
    // list - the up to 7 tail rows whose records fill the head's last block of 8 stay with Gf and Sp(g) - and leaves, per 8
    // rows, the column-sum row Sp(g)'s block would have left in ws->y2_colsum: close_bias reduces the same rows holding the
    // same numbers, so the bias gradient keeps its bits, like everything else.  A last stage goes this way only on the
    // closing-combination-once route (its P is formed inside the launch); otherwise it keeps the full list.
    const int tail_cg = f->groups == 0 ? 0 : (f->groups > 0 && d % f->groups == 0 && d / f->groups == 4) ? 4 : -1;
    const int64_t kRec = 8;                                                   // records per block of the d = 128 SpMM
    const int64_t head_items = f->a_head_items ? (f->a_n_head + kRec - 1) / kRec * kRec : 0;
    const int64_t n_tail = f->A.n_items - head_items;                         // rows of the tail launch
    const int64_t n_head = n - n_tail;
    const int64_t head_rows = head_items / kRec;
    bool a_tail = at_core && gode_opt_adjoint_tail() && gode_opt_fwd_pc() == 3 && d == 128 && tail_cg >= 0 && f->n_tail > 0 &&
                  f->a_head_items && f->a_head_items == f->A.items && f->a_diag && f->W && f->b && f->a_n_head > 0 &&
                  f->a_n_head == f->A.n_items - f->n_tail && n_tail > 0 && n_head > kMergedFinishMaxRows &&
                  head_items > 65536 && head_rows + gode_pc_adjoint_tail_colsum_rows(n_tail) <= y2rows;
    if (a_tail) {
        uintptr_t bits = (uintptr_t)y | (uintptr_t)a | (uintptr_t)ws->dS | (uintptr_t)ws->y2_colsum | (uintptr_t)f->W |
                         (uintptr_t)f->b | (uintptr_t)f->gamma | (uintptr_t)f->beta | (uintptr_t)ws->X[0] | (uintptr_t)ws->X[1];
        for (int j = 0; j < 4; ++j) bits |= (uintptr_t)ws->ky[j] | (uintptr_t)ws->ka[j];
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        a_tail = !(bits & 15) && hipStreamIsCapturing(hs, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
    }
    int full_g = -1;            // a last stage whose Gf could not form P (below): that stage keeps the full list
    auto tail_stage = [&](int g) { return a_tail && (g % 4 != 3 || close_once) && g != full_g; };
    gode_gcn_odefunc_t fhead = *f;
    fhead.n = n_head;
    // Gf(g) from the y-chain as it stands (stage g's step must be the current one: Sp of a last stage swaps the chain)
    auto gf = [&](int g, void* st) -> int {
        const gode_lincomb_t yin = tab_stage_terms(TAB38, ycur, ky, g % 4, h);
        const bool tl = tail_stage(g);
        if (g % 4 == 3 && close_once) {
            GODE_TRY(gf_last_stage(tl ? &fhead : f, yin, tab_combine_terms(TAB38, ycur, ky, h), stage_time(g), Sbuf[g & 1], x_out_of(g), ky[3],
                                   &py_formed, st));
            if (tl && !py_formed) {         // the tail launch forms P itself, so Sp(3) would have to read {1.0, P}: the kernel
                full_g = g;                 // the options select cannot form it - this stage goes the parent's way, on every row
                return gode_gn_time_gemm_xout_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->beta, f->W, d, 1, stage_time(g),
                                                  Sbuf[g & 1], x_out_of(g), st);
            }
            return 0;
        }
        return gode_gn_time_gemm_xout_f32(&yin, tl ? n_head : n, d, f->groups, f->eps, f->gamma, f->beta, f->W, d, 1, stage_time(g),
                                          Sbuf[g & 1], x_out_of(g), st);
    };
    // the tail launch of stage g, from both chains as they stand, on the caller's stream: issued once the side chain of
    // stage g - 1 is joined (it reads ws->y2_colsum), behind the dense launch of stage g - 1 (the last reader of dS and the
    // writer of ka[(g - 1) % 4]) and ahead of Sp(g)
    auto gf_tail = [&](int g) -> int {
        if (!tail_stage(g)) return 0;
        const int s = g % 4;
        const int64_t off = n_head * d;
        gode_lincomb_t yin = tab_stage_terms(TAB38, ycur, ky, s, h), cot = negated(tab_stage_terms(TAB38, acur, ka, s, h));
        if (yin.n != cot.n || yin.n != s + 1) return GODE_E_UNSUPPORTED;
        for (int j = 0; j < yin.n; ++j) { yin.ptr[j] += off; cot.ptr[j] += off; }
        AdjTail at = {};
        at.a_ii = f->a_diag + n_head; at.at_ii = f->at_diag + n_head; at.bias = f->b;
        at.k = ky[s] + off; at.dS = ws->dS + off; at.x_out = x_out_of(g) ? x_out_of(g) + off : nullptr;
        at.colpart = ws->y2_colsum + head_rows * d;
        if (s == 3) {
            const gode_lincomb_t ypre = tab_combine_terms(TAB38, ycur, ky, h), apre = tab_combine_terms(TAB38, acur, ka, h);
            if (ypre.n != 4 || apre.n != 4) return GODE_E_UNSUPPORTED;
            for (int j = 0; j < 4; ++j) { at.pcoef[j] = ypre.coef[j]; at.c3[j] = apre.coef[j]; }
            at.alpha = (float)(h * B38[3]);
            at.cot_out = ka[3] + off;
        }
        return gode_pc_adjoint_tail_launch(make_lincomb(&yin), make_lincomb(&cot), n_tail, f->eps, f->gamma, f->beta, f->W,
                                           stage_time(g), at, s == 3, tail_cg, hs);
    };
    GODE_TRY(gf(0, stream));
    GODE_TRY(gf_tail(0));
    bool wg_pending = false;
    for (int g = 0; g < total; ++g) {
        const int s = g % 4;
        const float ts = stage_time(g);
        // terms of THIS stage (used by Gb / Wg below)
        const gode_lincomb_t yin = x_out_of(g) ? one_term(x_out_of(g)) : tab_stage_terms(TAB38, ycur, ky, s, h);
        const gode_lincomb_t ain = tab_stage_terms(TAB38, acur, ka, s, h);
        gode_spmm_epilogue_t ep = relu_bias_epilogue(f);
        ep.cot = negated(ain);                                // cotangent of the VJP is -a
        ep.Y2 = ws->dZ;
        if (y2rows > 0) ep.Y2_colsum = ws->y2_colsum;
        gode_lincomb_t apre; apre.n = 0;
        if (s == 3) {
            ep.pre = py_formed ? one_term(ky[3]) : tab_combine_terms(TAB38, ycur, ky, h);
            ep.alpha = (float)(h * B38[3]);
            apre = tab_combine_terms(TAB38, acur, ka, h);
            if (close_once && ain.n == apre.n) {              // the cotangent terms are a, ka0, ka1, ka2 in this order
                ep.cot_out = ka[3];
                for (int j = 0; j < apre.n; ++j) ep.cot_out_coef[j] = apre.coef[j];
                apre = one_term(ka[3]);
            }
            py_formed = false;
        }
        if (at_core) {
            // Sp(g) writes rows of dS.  Its last reader is the one-pass dense launch of stage g - 1, which this branch
            // issues on the caller's stream ahead of Sp(g); the side stream's launches of this branch (column sums and
            // the reductions of the partials) never read dS.  The other branch reads dS on the side stream (Wg) while
            // Sp runs, which is why it keeps the full list.
            ep.Y2_scale = f->at_diag;
            ep.Y2_scaled = ws->dS;
        }
        if (two && g > 0) GODE_HIP(hipStreamWaitEvent(hs, ov->gf, 0));          // S of this stage was produced on the side stream
        const bool tl = tail_stage(g);
        if (tl) {                                                               // Sp(g) without the tail's records
            ep.n_items_full = f->A.n_items;                                     // same kernels, same name in the profile
            GODE_TRY(gode_spmm_csr_f32(f->A.rowptr, f->A.col, f->A.val, f->A.items, head_items, f->A.long_rows, f->A.n_long,
                                       f->A.partial, Sbuf[g & 1], d, ky[s], d, f->A.n_rows, d, &ep, stream));
        } else
        GODE_TRY(spmm(f->A, Sbuf[g & 1], ky[s], d, &ep, stream));               // Sp(g): k_y (or new y) and dZ
        if (s == 3) { float* tmp = ycur; ycur = ky[3]; ky[3] = tmp; }           // the y-chain as Gf(g+1) will see it
        if (two && wg_pending) GODE_HIP(hipStreamWaitEvent(hs, ov->wg, 0));     // previous Wg still reads dS
        if (at_core) {                                                          // SpT(g) without the rows Sp(g) has stored
            gode_spmm_epilogue_t pt = {};
            pt.alpha = 1.f;
            pt.n_items_full = f->AT.n_items;                                    // same kernels, same name in the profile
            GODE_TRY(gode_spmm_csr_f32(f->AT.rowptr, f->AT.col, f->AT.val, f->at_core_items, f->at_n_core, f->AT.long_rows,
                                       f->AT.n_long, f->AT.partial, ws->dZ, d, ws->dS, d, f->AT.n_rows, d, &pt, stream));
        } else
        GODE_TRY(spmm(f->AT, ws->dZ, ws->dS, d, nullptr, stream));              // SpT(g): alone on the chip
        if (two) {
            GODE_HIP(hipEventRecord(ov->spt, hs));
            GODE_HIP(hipStreamWaitEvent(ov->side, ov->spt, 0));
        }
        float* kt = ws->ktheta[s];
        const float out_scale = s == 3 ? (float)(h * B38[3]) : 1.f;
        float* gpart = f->groups > 0 ? ws->gpart : nullptr;
        float* bpart = f->groups > 0 ? ws->bpart : nullptr;
        if (bw) {
            // Gb(g) + Wg(g) in one launch on the caller's stream, then Gf(g+1) behind it (a 138 KB-LDS block and a
            // forward block do not share a CU anyway); the small reductions of the stage run on the side stream beside
            // them: colsum(dZ) as soon as SpT(g) is done, the partial sums once the dense launch is
            if (two) GODE_HIP(hipStreamWaitEvent(ov->side, ov->spt, 0));
            GODE_TRY(close_bias(f, ws, kt, y2rows > 0 ? ws->y2_colsum : ws->dZ, y2rows > 0 ? y2rows : n, side));
            GODE_TRY(gode_gn_time_gemm_bwd_wgrad_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->beta, f->W, d, 1, ws->dS,
                                                     out_scale, s == 3 ? &apre : nullptr, ka[s], gpart, bpart, ws->wpart, stream));
            if (two) {
                GODE_HIP(hipEventRecord(ov->sp, hs));
                GODE_HIP(hipStreamWaitEvent(ov->side, ov->sp, 0));
            }
            GODE_TRY(close_weight(f, ws, kt, gode_bwd_wgrad_parts(n), ts, side));
            GODE_TRY(close_affine(f, ws, kt, side));
            if (two) { GODE_HIP(hipEventRecord(ov->wg, ov->side)); wg_pending = true; }
            if (g + 1 < total) {                                                    // Gf(g+1), same stream as Sp(g+1)
                GODE_TRY(gf(g + 1, stream));
                if (two) GODE_HIP(hipEventRecord(ov->gf, hs));      // the wait at the top of the next stage finds it done
            }
            // the side chain still reads dZ and the partial buffers, which Sp(g+1) and the next dense launch overwrite
            if (two) { GODE_HIP(hipStreamWaitEvent(hs, ov->wg, 0)); wg_pending = false; }
        } else {
            // side stream, beside Gb(g) on the main stream: Wg(g), then the dense part of the NEXT stage
            GODE_TRY(gode_wgrad_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->beta, ws->dS, d, 1, ws->wpart, side));   // Wg(g)
            if (!small) GODE_TRY(close_weight(f, ws, kt, wparts, ts, side));
            if (two) { GODE_HIP(hipEventRecord(ov->wg, ov->side)); wg_pending = true; }
            if (g + 1 < total) {                                                    // Gf(g+1)
                GODE_TRY(gf(g + 1, side));
                if (two) GODE_HIP(hipEventRecord(ov->gf, ov->side));
            }
            GODE_TRY(gode_gn_time_gemm_bwd_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->W, d, 1, ws->dS, out_scale,
                                               s == 3 ? &apre : nullptr, ka[s], gpart, bpart, stream));               // Gb(g)
            if (small) {                                                            // launch-bound: one finishing launch per stage
                GODE_TRY(stage_finish_merged(f, ws, kt, ts, stream));
            } else {
                GODE_TRY(close_bias(f, ws, kt, ws->dZ, n, stream));
                GODE_TRY(close_affine(f, ws, kt, stream));
            }
        }
        if (s == 3) {
            // theta <- theta + h * sum b_s ktheta_s   (packed small components, one launch)
            if (two) { GODE_HIP(hipStreamWaitEvent(hs, ov->wg, 0)); wg_pending = false; }
            gode_lincomb_t tc = one_term(theta);
            tc.n = 5;
            for (int q = 0; q < 4; ++q) { tc.coef[1 + q] = (float)(h * B38[q]); tc.ptr[1 + q] = ws->ktheta[q]; }
            GODE_TRY(gode_lincomb_f32(theta, &tc, gode_gcn_ode_theta_len(d), stream));
            float* tmp = acur; acur = ka[3]; ka[3] = tmp;
        }
        if (g + 1 < total) GODE_TRY(gf_tail(g + 1));      // both chains are stage g + 1's now, and the side chain is joined
    }
    if (two) {                      // join: nothing of this call is left running on the side stream
        GODE_HIP(hipEventRecord(ov->gf, ov->side));
        GODE_HIP(hipStreamWaitEvent(hs, ov->gf, 0));
    }
    *y_result = ycur;
    *a_result = acur;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// One Dormand-Prince 5(4) step of the same ODE function per C-ABI call (adaptive solves on launch-bound sizes).
// The controller stays with the caller: it passes the FSAL stage in k[0], gets the 5th-order solution in y1 (and a1 /
// theta1), the remaining stages in k[1..6] and the squared error-ratio sums of the tensors torchdiffeq's norm treats
// separately as fp64 device scalars, reads those (its one synchronisation per step) and decides.
// ---------------------------------------------------------------------------------------------------------------
namespace {

// next / x_next (fused launch-bound path only): the stage's launch also writes the next stage's combined input
int dp_eval_forward(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, const gode_lincomb_t* yin, float t,
                    float* k_out, const gode_lincomb_t* next, float* x_next, void* stream) {
    if (fused_small(f)) return gode_gcn_feval_small_next_f32(f, yin, t, 1.f, nullptr, nullptr, nullptr, k_out, next, x_next, stream);
    return feval_large(f, *yin, t, ws->S, k_out, nullptr, nullptr, stream);
}

// One evaluation of the augmented adjoint field: k_y = f(t, y), k_a = -a^T df/dy, k_theta = [-a^T df/dW | .. b | .. gamma |
// .. beta | -a^T df/dt]  (the launch sequence of GcnOdeAdjointField._stage, single stream).
// part_slot >= 0 (fused path): the stage's block partials go to that slot of ws->small_part and the caller closes all
// stages of the step in one launch (gode_gcn_small_finish_multi_f32); -1: the stage is closed here
int dp_eval_adjoint(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, gode_lincomb_t yin,
                    const gode_lincomb_t& ain, float t, float* ky, float* ka, float* kth, const gode_lincomb_t* next,
                    float* x_next, int part_slot, void* stream) {
    const int64_t n = f->n, d = f->d;
    if (fused_small(f) && ws->small_part) {
        const gode_lincomb_t cot = negated(ain);
        GODE_TRY(gode_gcn_feval_small_next_f32(f, &yin, t, 1.f, nullptr, &cot, ws->dZ, ky, next, x_next, stream));
        float* part = ws->small_part + (part_slot > 0 ? part_slot : 0) * gode_gcn_small_parts(n) * gode_gcn_small_part_len(d);
        GODE_TRY(gode_gcn_vjp_small_f32(f, &yin, ws->dZ, 1.f, nullptr, ka, part, stream));
        if (part_slot >= 0) return 0;
        return gode_gcn_small_finish_f32(f, part, kth, t, stream);
    }
    float* xo = (yin.n >= 3 && ws->X[0]) ? ws->X[0] : nullptr;
    GODE_TRY(gode_gn_time_gemm_xout_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->beta, f->W, d, 1, t, ws->S, xo, stream));
    if (xo) yin = one_term(xo);
    gode_spmm_epilogue_t ep = relu_bias_epilogue(f);
    ep.cot = negated(ain);
    ep.Y2 = ws->dZ;
    GODE_TRY(spmm(f->A, ws->S, ky, d, &ep, stream));
    GODE_TRY(spmm(f->AT, ws->dZ, ws->dS, d, nullptr, stream));
    GODE_TRY(gode_gn_time_gemm_bwd_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->W, d, 1, ws->dS, 1.f, nullptr, ka,
                                       f->groups > 0 ? ws->gpart : nullptr, f->groups > 0 ? ws->bpart : nullptr, stream));
    GODE_TRY(gode_wgrad_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->beta, ws->dS, d, 1, ws->wpart, stream));
    if (n <= kMergedFinishMaxRows) return stage_finish_merged(f, ws, kth, t, stream);
    GODE_TRY(close_weight(f, ws, kth, gode_wgrad_parts(n), t, stream));
    GODE_TRY(close_bias(f, ws, kth, ws->dZ, n, stream));
    return close_affine(f, ws, kth, stream);
}

}  // namespace

extern "C" int gode_gcn_ode_dopri5_step_forward(const gode_gcn_odefunc_t* f, const float* y, float* const* k, float* y1,
                                                const gode_rk4_workspace_t* ws, double t, double h, float rtol,
                                                float atol, double* sums, void* err_scratch, void* stream)
{
    if (!f || !y || !k || !y1 || !ws || !sums || !err_scratch) return GODE_E_NULLPTR;
    if (f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    for (int s = 0; s < 7; ++s) if (!k[s]) return GODE_E_NULLPTR;
    if (!ws->S) return GODE_E_NULLPTR;
    const int64_t nd = f->n * f->d;
    // launch-bound graphs: from the second stage on a stage reads its combined input from X[s & 1], written row by row by
    // the stage before it (same multiply-adds in the same order as combining the terms on the fly: bit-identical)
    const bool chain = fused_small(f) && ws->X[0] && ws->X[1];
    for (int s = 1; s < 7; ++s) {
        gode_lincomb_t yin = tab_stage_terms(TABDP, y, k, s, h);
        if (chain && s >= 2) yin = one_term(ws->X[s & 1]);
        gode_lincomb_t nxt; nxt.n = 0;
        if (chain && s < 6) nxt = tab_stage_terms(TABDP, y, k, s + 1, h);
        GODE_TRY(dp_eval_forward(f, ws, &yin, (float)(t + DPC[s] * h), k[s], nxt.n > 0 ? &nxt : nullptr,
                                 nxt.n > 0 ? ws->X[(s + 1) & 1] : nullptr, stream));
    }
    gode_lincomb_t sol = dp_terms(y, k, DPB, 7, h, true);
    GODE_TRY(gode_lincomb_f32(y1, &sol, nd, stream));
    gode_lincomb_t err = dp_terms(nullptr, k, DPE, 7, h, false);
    return gode_rk_errnorm_f32(sums, y, y1, &err, rtol, atol, nd, err_scratch, stream);
}

extern "C" int gode_gcn_ode_dopri5_step_adjoint(const gode_gcn_odefunc_t* f, const float* y, const float* a,
                                                const float* theta, float* const* ky, float* const* ka,
                                                float* const* kth, float* y1, float* a1, float* theta1,
                                                const gode_rk4_workspace_t* ws, double t, double h, float rtol,
                                                float atol, double* sums /* 4 */, void* err_scratch, void* stream)
{
    if (!f || !y || !a || !theta || !ky || !ka || !kth || !y1 || !a1 || !theta1 || !ws || !sums || !err_scratch)
        return GODE_E_NULLPTR;
    if (f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    for (int s = 0; s < 7; ++s) if (!ky[s] || !ka[s] || !kth[s]) return GODE_E_NULLPTR;
    if (!ws->S || !ws->dZ || !ws->dS || !ws->wpart || !ws->colsum_scratch) return GODE_E_NULLPTR;
    if (f->groups > 0 && (!ws->gpart || !ws->bpart)) return GODE_E_NULLPTR;
    const int64_t nd = f->n * f->d, P = gode_gcn_ode_theta_len(f->d);
    const bool fused = fused_small(f) && ws->small_part;
    const bool chain = fused && ws->X[0] && ws->X[1];                                   // as in the forward step
    for (int s = 1; s < 7; ++s) {
        gode_lincomb_t yin = tab_stage_terms(TABDP, y, ky, s, h);
        if (chain && s >= 2) yin = one_term(ws->X[s & 1]);
        gode_lincomb_t ain = tab_stage_terms(TABDP, a, ka, s, h);
        gode_lincomb_t nxt; nxt.n = 0;
        if (chain && s < 6) nxt = tab_stage_terms(TABDP, y, ky, s + 1, h);
        GODE_TRY(dp_eval_adjoint(f, ws, yin, ain, (float)(t + DPC[s] * h), ky[s], ka[s], kth[s], nxt.n > 0 ? &nxt : nullptr,
                                 nxt.n > 0 ? ws->X[(s + 1) & 1] : nullptr, fused ? s - 1 : -1, stream));
    }
    if (fused) {      // the six stages' small components in one launch: nothing inside the step reads them
        float* kout[6]; float tsv[6];
        for (int s = 1; s < 7; ++s) { kout[s - 1] = kth[s]; tsv[s - 1] = (float)(t + DPC[s] * h); }
        GODE_TRY(gode_gcn_small_finish_multi_f32(f, ws->small_part, 6, kout, tsv, stream));
    }
    gode_lincomb_t sy = dp_terms(y, ky, DPB, 7, h, true), sa = dp_terms(a, ka, DPB, 7, h, true),
                   st = dp_terms(theta, kth, DPB, 7, h, true);
    {   // the three solution combines in one launch, the four error sums in one pair (same numbers as the single forms)
        float* outs[3] = {y1, a1, theta1};
        const gode_lincomb_t sols[3] = {sy, sa, st};
        const int64_t lens[3] = {nd, nd, P};
        GODE_TRY(gode_lincomb_multi_f32(outs, sols, lens, 3, stream));
    }
    // a_t is the last entry of the packed vector, the flattened parameters the P-1 before it
    const gode_lincomb_t errs[4] = {dp_terms(nullptr, ky, DPE, 7, h, false), dp_terms(nullptr, ka, DPE, 7, h, false),
                                    dp_terms(nullptr, kth, DPE, 7, h, false, P - 1), dp_terms(nullptr, kth, DPE, 7, h, false)};
    const float* e0[4] = {y, a, theta + (P - 1), theta};
    const float* e1[4] = {y1, a1, theta1 + (P - 1), theta1};
    const int64_t ens[4] = {nd, nd, 1, P - 1};
    return gode_rk_errnorm_multi_f32(sums, e0, e1, errs, ens, 4, rtol, atol, err_scratch, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Backprop through a fixed-grid solve (odeint._OdeintBackprop): a forward solve that keeps every step's y_n and
// k_1..k_S (forward_save), and ONE call for the whole reverse sweep over them (backprop).  Record r of `save` (step
// step_begin + r) is [ y_n | k_1 | .. | k_S ], S + 1 n x d arrays (rk4: five).  Per step, with cotangent abar = dL/dy_{n+1},
// kbar_s = h b_s abar + h sum_{q > s} A[q][s] Ybar_q; under the 3/8 rule:
//   kbar_4 = h/8 abar,  kbar_3 = 3h/8 abar + h Ybar_4,  kbar_2 = 3h/8 abar + h Ybar_3 - h Ybar_4,
//   kbar_1 = h/8 abar + h/3 Ybar_2 - h/3 Ybar_3 + h Ybar_4;   Ybar_s = J_s^T kbar_s,  theta += (df/dtheta)_s^T kbar_s,
//   abar_n = abar + sum_s Ybar_s
// where J_s is the Jacobian of f at the stage input Y_s = y_n + h sum_j A38[s][j] k_j; f = relu(z), so the VJP's mask
// [z_s > 0] is [k_s > 0] of the saved derivative  (kbar_s: rk_driver.h, stage_cotangent).
// ---------------------------------------------------------------------------------------------------------------
namespace {

// Which launches a reverse sweep's stage takes where the fused launch does not apply
struct SweepRoute {
    bool small;             // launch-bound: one merged finishing launch per stage
    bool bw;                // large graphs at d = 128: dense VJP and weight-gradient partials from one pass
    int64_t wparts, cparts; // weight-gradient partial rows; column-sum rows of the masked cotangent (0: none)
    float* cot_colpart;
    float* gpart; float* bpart;
};
SweepRoute sweep_route(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, float* cot_colpart) {
    SweepRoute r;
    r.small = f->n <= kMergedFinishMaxRows;
    r.wparts = gode_wgrad_parts(f->n);
    r.bw = !r.small && gode_bwd_wgrad_supported(f->n, f->d, f->d, f->groups) && gode_bwd_wgrad_parts(f->n) <= r.wparts;
    r.cparts = (!r.small && cot_colpart) ? gode_masked_cot_parts(f->n, f->d) : 0;
    r.cot_colpart = cot_colpart;
    r.gpart = f->groups > 0 ? ws->gpart : nullptr;
    r.bpart = f->groups > 0 ? ws->bpart : nullptr;
    return r;
}

// One stage of a reverse sweep, multi-launch routes: masked cotangent kbar * [k > 0], SpT, the dense VJP at the stage
// input yin into ybar (pre, nullable: added to it), the weight gradient, and the stage's parameter part closed into kt
int sweep_stage(const gode_gcn_odefunc_t* f, const gode_rk4_workspace_t* ws, const SweepRoute& r, const gode_lincomb_t& cot,
                const float* k, const gode_lincomb_t& yin, const gode_lincomb_t* pre, float* ybar, float* kt, float ts,
                void* stream) {
    const int64_t n = f->n, d = f->d;
    GODE_TRY(gode_masked_cot_f32(&cot, k, ws->dZ, n, d, r.cparts > 0 ? r.cot_colpart : nullptr, stream));
    GODE_TRY(spmm(f->AT, ws->dZ, ws->dS, d, nullptr, stream));                 // dS = A^T dZ
    if (r.bw) {
        GODE_TRY(gode_gn_time_gemm_bwd_wgrad_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->beta, f->W, d, 1, ws->dS,
                                                 1.f, pre, ybar, r.gpart, r.bpart, ws->wpart, stream));
    } else {
        GODE_TRY(gode_gn_time_gemm_bwd_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->W, d, 1, ws->dS, 1.f,
                                           pre, ybar, r.gpart, r.bpart, stream));
        GODE_TRY(gode_wgrad_f32(&yin, n, d, f->groups, f->eps, f->gamma, f->beta, ws->dS, d, 1, ws->wpart, stream));
        if (r.small) return stage_finish_merged(f, ws, kt, ts, stream);
    }
    GODE_TRY(close_weight(f, ws, kt, r.bw ? gode_bwd_wgrad_parts(n) : r.wparts, ts, stream));
    GODE_TRY(close_bias(f, ws, kt, r.cparts > 0 ? r.cot_colpart : ws->dZ, r.cparts > 0 ? r.cparts : n, stream));
    return close_affine(f, ws, kt, stream);
}

// theta += sum of `count` closed stage parts   (weights 1: h is already inside kbar)
int add_stage_parts(float* theta, float* const* kt, int count, int64_t len, void* stream) {
    gode_lincomb_t tc = one_term(theta);
    for (int q = 0; q < count; ++q) { tc.coef[tc.n] = 1.f; tc.ptr[tc.n] = kt[q]; ++tc.n; }
    return gode_lincomb_f32(theta, &tc, len, stream);
}

// Steps step_begin .. step_end - 1 of forward_solve's launches into records (the folded last stage also stores k_S)
int forward_save(const Tableau* tabp, const gode_gcn_odefunc_t* f, const float* y0, float* y_end, float* save,
                 const gode_rk4_workspace_t* ws, float t0, float t1, int32_t n_steps, int32_t step_begin, int32_t step_end,
                 void* stream)
{
    if (!f || !y0 || !y_end || !save || !ws) return GODE_E_NULLPTR;
    if (!tabp) return GODE_E_SHAPE;
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    if (step_begin < 0 || step_end > n_steps || step_begin >= step_end) return GODE_E_SHAPE;
    if (!ws->S) return GODE_E_NULLPTR;
    const int S = tabp->stages;
    const int64_t nd = f->n * f->d;
    const double h = ((double)t1 - (double)t0) / n_steps;
    const bool fused = fused_small(f);
    const bool close_once = close_once_route(f);
    if (y0 != save) {                                            // record 0 starts with a copy of y0
        const gode_lincomb_t c = one_term(y0);
        GODE_TRY(gode_lincomb_f32(save, &c, nd, stream));
    }
    for (int i = step_begin; i < step_end; ++i) {
        float* rec = save + (int64_t)(i - step_begin) * (S + 1) * nd;
        float* k[4] = {};
        for (int s = 0; s < S; ++s) k[s] = rec + (int64_t)(s + 1) * nd;
        float* ynext = (i + 1 < step_end) ? rec + (int64_t)(S + 1) * nd : y_end;      // the next record's y_n, or the result
        GODE_TRY(fixed_forward_step(*tabp, f, ws, rec, k, ynext, true, (double)t0 + i * h, h, fused, close_once, stream));
    }
    return 0;
}

// The reverse sweep over those records
int backprop(const Tableau* tabp, const gode_gcn_odefunc_t* f, const float* save, float* a, float* theta, float** a_result,
             const gode_rk4_workspace_t* ws, float* cot_colpart, float t0, float t1, int32_t n_steps, int32_t step_begin,
             int32_t step_end, void* stream)
{
    if (!f || !save || !a || !theta || !a_result || !ws) return GODE_E_NULLPTR;
    if (!tabp) return GODE_E_SHAPE;
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    if (step_begin < 0 || step_end > n_steps || step_begin >= step_end) return GODE_E_SHAPE;
    const Tableau& tab = *tabp;
    const int S = tab.stages, L = S - 1;
    for (int s = 0; s < S; ++s) if (!ws->ka[s] || !ws->ktheta[s]) return GODE_E_NULLPTR;
    if (!ws->dZ || !ws->dS || !ws->wpart || !ws->colsum_scratch) return GODE_E_NULLPTR;
    if (f->groups > 0 && (!ws->gpart || !ws->bpart)) return GODE_E_NULLPTR;
    const int64_t n = f->n, d = f->d, nd = n * d;
    const double h = ((double)t1 - (double)t0) / n_steps;
    float* acur = a;
    float* yb[4] = {ws->ka[0], ws->ka[1], ws->ka[2], ws->ka[3]};   // yb[1..S-1]: Ybar_2..S; yb[0] receives abar_n
    auto record = [&](int i) { return save + (int64_t)(i - step_begin) * (S + 1) * nd; };
    // kbar_S = h b_S abar: b_S is non-zero in every method of the list, so the sweep of a step always opens with one term
    const float hbl = (float)(h * tab.b[L]);
    const bool fused = fused_small(f) && ws->small_part != nullptr;
    if (fused) {
        // launch-bound graphs: ONE launch per stage - the VJP of stage s (csrc/small.hip) also forms the masked cotangent
        // of the stage after it in the sweep (s - 1, or stage S of the previous step); one launch per step closes theta
        const int64_t slot = gode_gcn_small_parts(n) * gode_gcn_small_part_len(d);
        float* dz[2] = {ws->dZ, ws->dS};
        int cur = 0;
        {
            const float* r = record(step_end - 1);
            const gode_lincomb_t cl = stage_cotangent(tab, acur, hbl, yb, L, h);
            GODE_TRY(gode_masked_cot_f32(&cl, r + (int64_t)S * nd, dz[0], n, d, nullptr, stream));
        }
        for (int i = step_end - 1; i >= step_begin; --i) {
            const float* y = record(i);
            float* k[4] = {};
            for (int s = 0; s < S; ++s) k[s] = (float*)y + (int64_t)(s + 1) * nd;
            const double t = (double)t0 + i * h;
            const gode_lincomb_t pre = sweep_pre(tab, acur, 1.f, yb, 1);
            float stage_t[4], w1[4];
            for (int s = L; s >= 0; --s) {
                stage_t[s] = (float)(t + tab.c[s] * h);
                w1[s] = 1.f;                                           // h is already inside kbar
                const gode_lincomb_t yin = tab_stage_terms(tab, y, k, s, h);
                gode_lincomb_t nxt; nxt.n = 0;
                const float* knext = nullptr;
                if (s > 0) {
                    nxt = stage_cotangent(tab, acur, (float)(h * tab.b[s - 1]), yb, s - 1, h);   // names yb[s]: this launch's rows
                    knext = k[s - 1];
                } else if (i > step_begin) {
                    nxt = one_term(yb[0]); nxt.coef[0] = hbl;                                  // kbar_S of step i - 1
                    knext = record(i - 1) + (int64_t)S * nd;
                }
                float* part = ws->small_part + s * slot;
                if (knext && nxt.n > 0) {
                    GODE_TRY(gode_gcn_vjp_small_next_f32(f, &yin, dz[cur], 1.f, s == 0 ? &pre : nullptr, yb[s], part,
                                                         &nxt, knext, dz[cur ^ 1], stream));
                    cur ^= 1;
                } else {
                    GODE_TRY(gode_gcn_vjp_small_f32(f, &yin, dz[cur], 1.f, s == 0 ? &pre : nullptr, yb[s], part, stream));
                }
            }
            GODE_TRY(gode_gcn_small_finish_step_f32(f, ws->small_part, S, theta, w1, stage_t, stream));
            float* tmp = acur; acur = yb[0]; yb[0] = tmp;
        }
        *a_result = acur;
        return 0;
    }
    const SweepRoute route = sweep_route(f, ws, cot_colpart);
    for (int i = step_end - 1; i >= step_begin; --i) {
        const float* y = record(i);
        float* k[4] = {};
        for (int s = 0; s < S; ++s) k[s] = (float*)y + (int64_t)(s + 1) * nd;
        const double t = (double)t0 + i * h;
        const gode_lincomb_t pre = sweep_pre(tab, acur, 1.f, yb, 1);
        for (int s = L; s >= 0; --s) {
            const gode_lincomb_t cot = stage_cotangent(tab, acur, (float)(h * tab.b[s]), yb, s, h);
            GODE_TRY(sweep_stage(f, ws, route, cot, k[s], tab_stage_terms(tab, y, k, s, h), s == 0 ? &pre : nullptr, yb[s],
                                 ws->ktheta[s], (float)(t + tab.c[s] * h), stream));
        }
        GODE_TRY(add_stage_parts(theta, ws->ktheta, S, gode_gcn_ode_theta_len(d), stream));
        float* tmp = acur; acur = yb[0]; yb[0] = tmp;
    }
    *a_result = acur;
    return 0;
}

}  // namespace

extern "C" int gode_gcn_ode_rk4_forward_save(const gode_gcn_odefunc_t* f, const float* y0, float* y_end, float* save,
                                             const gode_rk4_workspace_t* ws, float t0, float t1, int32_t n_steps,
                                             int32_t step_begin, int32_t step_end, void* stream)
{
    return forward_save(&TAB38, f, y0, y_end, save, ws, t0, t1, n_steps, step_begin, step_end, stream);
}

extern "C" int gode_gcn_ode_rk4_backprop(const gode_gcn_odefunc_t* f, const float* save, float* a, float* theta,
                                         float** a_result, const gode_rk4_workspace_t* ws, float* cot_colpart,
                                         float t0, float t1, int32_t n_steps, int32_t step_begin, int32_t step_end,
                                         void* stream)
{
    return backprop(&TAB38, f, save, a, theta, a_result, ws, cot_colpart, t0, t1, n_steps, step_begin, step_end, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Backprop through an adaptive solve (odeint._OdeintBackpropDopri5): the reverse sweep over ONE accepted step per
// call - the controller's record (which steps were accepted, their sizes, the interpolation that ends an interval) stays
// with the caller, as the controller itself does.  One body (step_backprop) over an AdaptiveMethod: the dopri5 entry point
// runs it under ADAPTIVE[GODE_RKA_DOPRI5], the adaptive one under the method of its code.  The step went from y_n at t_n
// with step h through the saved stage derivatives k_1..k_S (FSAL: k_1 = f(t_n, y_n) is the step before's k_S, or the
// interval's opening evaluation); with one cotangent array g and host weights wy, wk[1..S] (stages numbered from 1 in this
// comment, from 0 in the code; A: the method's Butcher matrix):
//   kbar_s = wk[s] g + h sum_{q > s} A[q][s] Ybar_q  (+ kbar_last when s = S),
//   Ybar_s = J_s^T kbar_s,  theta += (df/dtheta)_s^T kbar_s   for s = S..2 (and s = 1 when `first`),
//   ybar_n = wy g + sum_s Ybar_s
// kbar_1 leaves the call as the kbar_last of the step before, unless `first`: then it is pushed through f at (t_n, y_n) here.
// An ordinary step has g = ybar_{n+1}, wy = 1, wk[s] = h b_s; the interpolated last step of an interval folds the
// interpolation's coefficients into wy and wk.  A stage whose cotangent has no term is skipped.
// The launches of a stage are the rk4 sweep's (sweep_stage; fused: masked cotangent + one VJP launch); the stages'
// parameter parts are added to theta by one launch per step.
// ---------------------------------------------------------------------------------------------------------------
namespace {

// am == NULL: a code outside GODE_RKA_*, refused after the null checks
int step_backprop(const AdaptiveMethod* am, const gode_gcn_odefunc_t* f, const float* y, float* const* k, const float* g,
                  const float* kbar_last, double wy, const double* wk, double t, double h, int32_t first, float* const* ybar,
                  float* ybar_n, float* kbar1, float* theta, float* const* ktheta, const gode_rk4_workspace_t* ws,
                  float* cot_colpart, void* stream)
{
    if (!f || !y || !k || !g || !wk || !ybar || !ybar_n || !theta || !ktheta || !ws) return GODE_E_NULLPTR;
    if (!am) return GODE_E_SHAPE;
    const Tableau& tab = am->tab;
    const int S = tab.stages;
    if (f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    if (!first && !kbar1) return GODE_E_NULLPTR;
    for (int s = 0; s < S; ++s) if (!k[s] || !ktheta[s]) return GODE_E_NULLPTR;
    for (int s = 1; s < S; ++s) if (!ybar[s]) return GODE_E_NULLPTR;
    if (first && !ybar[0]) return GODE_E_NULLPTR;
    if (ybar_n == g || ybar_n == kbar_last || (kbar1 && (kbar1 == g || kbar1 == kbar_last || kbar1 == ybar_n))) return GODE_E_SHAPE;
    for (int s = 0; s < S; ++s)
        if (ybar[s] && (ybar[s] == g || ybar[s] == kbar_last || ybar[s] == ybar_n || ybar[s] == kbar1)) return GODE_E_SHAPE;
    if (!ws->dZ || !ws->dS || !ws->wpart || !ws->colsum_scratch) return GODE_E_NULLPTR;
    if (f->groups > 0 && (!ws->gpart || !ws->bpart)) return GODE_E_NULLPTR;
    const int64_t n = f->n, d = f->d, nd = n * d, P = gode_gcn_ode_theta_len(d);
    const bool fused = fused_small(f) && ws->small_part != nullptr;
    const SweepRoute route = sweep_route(f, ws, cot_colpart);
    const int64_t slot = fused ? gode_gcn_small_parts(n) * gode_gcn_small_part_len(d) : 0;
    const int last = first ? 0 : 1;                // the last stage the sweep pushes through f
    bool dead[7] = {};
    float* kt[7]; float kt_time[7];
    int live = 0;
    auto cotangent = [&](int s) {
        gode_lincomb_t c = stage_cotangent(tab, g, (float)wk[s], ybar, s, h, dead);
        if (s == S - 1 && kbar_last) { c.coef[c.n] = 1.f; c.ptr[c.n] = kbar_last; ++c.n; }
        return c;
    };
    for (int s = S - 1; s >= last; --s) {
        const gode_lincomb_t cot = cotangent(s);
        if (cot.n == 0) { dead[s] = true; continue; }
        const float ts = (float)(t + tab.c[s] * h);
        const gode_lincomb_t yin = tab_stage_terms(tab, y, k, s, h);
        // `first`: the launch that forms Ybar_1 adds the rest of ybar_n to it (every later stage is settled by then)
        const bool closes = first && s == 0;
        const gode_lincomb_t pre = sweep_pre(tab, g, (float)wy, ybar, 1, dead);
        float* out = closes ? ybar_n : ybar[s];
        if (fused) {
            GODE_TRY(gode_masked_cot_f32(&cot, k[s], ws->dZ, n, d, nullptr, stream));
            GODE_TRY(gode_gcn_vjp_small_f32(f, &yin, ws->dZ, 1.f, closes ? &pre : nullptr, out, ws->small_part + live * slot, stream));
        } else {
            GODE_TRY(sweep_stage(f, ws, route, cot, k[s], yin, closes ? &pre : nullptr, out, ktheta[live], ts, stream));
        }
        kt[live] = ktheta[live]; kt_time[live] = ts;
        ++live;
    }
    if (!first || dead[0]) {
        // ybar_n = wy g + sum Ybar_s, and (not first) kbar_1 for the step before: one launch
        float* outs[2] = {ybar_n, kbar1};
        gode_lincomb_t lcs[2] = {sweep_pre(tab, g, (float)wy, ybar, 1, dead), cotangent(0)};
        int64_t lens[2] = {nd, nd};
        int count = first ? 1 : 2;
        if (count == 2 && lcs[1].n == 0) { GODE_TRY(gode_zero_f32(kbar1, nd, stream)); count = 1; }
        GODE_TRY(gode_lincomb_multi_f32(outs, lcs, lens, count, stream));
    }
    if (live == 0) return 0;
    if (fused) GODE_TRY(gode_gcn_small_finish_multi_f32(f, ws->small_part, live, kt, kt_time, stream));
    return add_stage_parts(theta, kt, live, P, stream);
}

}  // namespace

extern "C" int gode_gcn_ode_dopri5_step_backprop(const gode_gcn_odefunc_t* f, const float* y, float* const* k,
                                                 const float* g, const float* kbar7, double wy, const double* wk,
                                                 double t, double h, int32_t first, float* const* ybar, float* ybar_n,
                                                 float* kbar1, float* theta, float* const* ktheta,
                                                 const gode_rk4_workspace_t* ws, float* cot_colpart, void* stream)
{
    return step_backprop(&ADAPTIVE[GODE_RKA_DOPRI5], f, y, k, g, kbar7, wy, wk, t, h, first, ybar, ybar_n, kbar1, theta, ktheta, ws,
                         cot_colpart, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// The adaptive step drivers by method (GODE_RKA_*): the dopri5 step functions above driven by a tableau and its error
// weights (rk_driver.h: AdaptiveMethod), on the same routes.  The forward and the adjoint step close with the fused
// launch of rk.hip (gode_rk_close_err_multi_f32): the solution and the error sums from one pass over the stages; the sweep
// is step_backprop, the body the dopri5 sweep runs.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int gode_rka_stages(int32_t method)
{
    const AdaptiveMethod* am = adaptive_method(method);
    return am ? am->tab.stages : GODE_E_SHAPE;
}

extern "C" int gode_rka_order(int32_t method)
{
    const AdaptiveMethod* am = adaptive_method(method);
    return am ? am->order : GODE_E_SHAPE;
}

extern "C" int gode_rka_tableau(int32_t method, double* c, double* a, double* b, double* e)
{
    const AdaptiveMethod* am = adaptive_method(method);
    if (!am) return GODE_E_SHAPE;
    const Tableau& tab = am->tab;
    const int S = tab.stages;
    for (int s = 0; s < S; ++s) {
        if (c) c[s] = tab.c[s];
        if (b) b[s] = tab.b[s];
        if (e) e[s] = am->e[s];
        if (a) for (int j = 0; j < S; ++j) a[s * S + j] = j < s ? tab.a[s * tab.lda + j] : 0.0;
    }
    return 0;
}

extern "C" int gode_gcn_ode_adaptive_step_forward(int32_t method, const gode_gcn_odefunc_t* f, const float* y,
                                                  float* const* k, float* y1, const gode_rk4_workspace_t* ws, double t,
                                                  double h, float rtol, float atol, double* sums, void* err_scratch,
                                                  void* stream)
{
    if (!f || !y || !k || !y1 || !ws || !sums || !err_scratch) return GODE_E_NULLPTR;
    const AdaptiveMethod* am = adaptive_method(method);
    if (!am) return GODE_E_SHAPE;
    const Tableau& tab = am->tab;
    const int S = tab.stages;
    if (f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    for (int s = 0; s < S; ++s) if (!k[s]) return GODE_E_NULLPTR;
    if (!ws->S) return GODE_E_NULLPTR;
    const int64_t nd = f->n * f->d;
    const bool chain = fused_small(f) && ws->X[0] && ws->X[1];                         // as in the dopri5 step
    for (int s = 1; s < S; ++s) {
        gode_lincomb_t yin = tab_stage_terms(tab, y, k, s, h);
        if (chain && s >= 2) yin = one_term(ws->X[s & 1]);
        gode_lincomb_t nxt; nxt.n = 0;
        if (chain && s < S - 1) nxt = tab_stage_terms(tab, y, k, s + 1, h);
        GODE_TRY(dp_eval_forward(f, ws, &yin, (float)(t + tab.c[s] * h), k[s], nxt.n > 0 ? &nxt : nullptr,
                                 nxt.n > 0 ? ws->X[(s + 1) & 1] : nullptr, stream));
    }
    float ec[GODE_MAX_TERMS];
    const gode_lincomb_t sol = close_terms(*am, y, k, h, ec);
    const float* ecp = ec;
    return gode_rk_close_err_multi_f32(&y1, &sol, &ecp, &nd, 1, rtol, atol, sums, err_scratch, stream);
}

extern "C" int gode_gcn_ode_adaptive_step_adjoint(int32_t method, const gode_gcn_odefunc_t* f, const float* y,
                                                  const float* a, const float* theta, float* const* ky, float* const* ka,
                                                  float* const* kth, float* y1, float* a1, float* theta1,
                                                  const gode_rk4_workspace_t* ws, double t, double h, float rtol,
                                                  float atol, double* sums /* 4 */, void* err_scratch, void* stream)
{
    if (!f || !y || !a || !theta || !ky || !ka || !kth || !y1 || !a1 || !theta1 || !ws || !sums || !err_scratch)
        return GODE_E_NULLPTR;
    const AdaptiveMethod* am = adaptive_method(method);
    if (!am) return GODE_E_SHAPE;
    const Tableau& tab = am->tab;
    const int S = tab.stages;
    if (f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    for (int s = 0; s < S; ++s) if (!ky[s] || !ka[s] || !kth[s]) return GODE_E_NULLPTR;
    if (!ws->S || !ws->dZ || !ws->dS || !ws->wpart || !ws->colsum_scratch) return GODE_E_NULLPTR;
    if (f->groups > 0 && (!ws->gpart || !ws->bpart)) return GODE_E_NULLPTR;
    const int64_t nd = f->n * f->d, P = gode_gcn_ode_theta_len(f->d);
    const bool fused = fused_small(f) && ws->small_part;
    const bool chain = fused && ws->X[0] && ws->X[1];
    for (int s = 1; s < S; ++s) {
        gode_lincomb_t yin = tab_stage_terms(tab, y, ky, s, h);
        if (chain && s >= 2) yin = one_term(ws->X[s & 1]);
        const gode_lincomb_t ain = tab_stage_terms(tab, a, ka, s, h);
        gode_lincomb_t nxt; nxt.n = 0;
        if (chain && s < S - 1) nxt = tab_stage_terms(tab, y, ky, s + 1, h);
        GODE_TRY(dp_eval_adjoint(f, ws, yin, ain, (float)(t + tab.c[s] * h), ky[s], ka[s], kth[s], nxt.n > 0 ? &nxt : nullptr,
                                 nxt.n > 0 ? ws->X[(s + 1) & 1] : nullptr, fused ? s - 1 : -1, stream));
    }
    if (fused) {      // the S - 1 stages' small components in one launch: nothing inside the step reads them
        float* kout[6]; float tsv[6];
        for (int s = 1; s < S; ++s) { kout[s - 1] = kth[s]; tsv[s - 1] = (float)(t + tab.c[s] * h); }
        GODE_TRY(gode_gcn_small_finish_multi_f32(f, ws->small_part, S - 1, kout, tsv, stream));
    }
    // one close for the three outputs and the four error groups: y, a, a_t (the last entry of the packed vector) and the
    // flattened parameters (the P - 1 before it), each group the decomposition the separate error norm gives it
    float ec[4][GODE_MAX_TERMS];
    const gode_lincomb_t sols[4] = {close_terms(*am, y, ky, h, ec[0]), close_terms(*am, a, ka, h, ec[1]),
                                    close_terms(*am, theta, kth, h, ec[2], P - 1), close_terms(*am, theta, kth, h, ec[3])};
    float* outs[4] = {y1, a1, theta1 + (P - 1), theta1};
    const float* ecs[4] = {ec[0], ec[1], ec[2], ec[3]};
    const int64_t lens[4] = {nd, nd, 1, P - 1};
    return gode_rk_close_err_multi_f32(outs, sols, ecs, lens, 4, rtol, atol, sums, err_scratch, stream);
}

extern "C" int gode_gcn_ode_adaptive_step_backprop(int32_t method, const gode_gcn_odefunc_t* f, const float* y,
                                                   float* const* k, const float* g, const float* kbar_last, double wy,
                                                   const double* wk, double t, double h, int32_t first,
                                                   float* const* ybar, float* ybar_n, float* kbar1, float* theta,
                                                   float* const* ktheta, const gode_rk4_workspace_t* ws,
                                                   float* cot_colpart, void* stream)
{
    return step_backprop(adaptive_method(method), f, y, k, g, kbar_last, wy, wk, t, h, first, ybar, ybar_n, kbar1, theta, ktheta,
                         ws, cot_colpart, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// The fixed-grid drivers by method (GODE_RK_*): the bodies the rk4 entry points run, under the tableau of the code
// (rk_driver.h: fixed_tableau).  The last stage of a step is the closing one.
// ---------------------------------------------------------------------------------------------------------------
extern "C" int gode_rk_stages(int32_t method)
{
    const Tableau* tab = fixed_tableau(method);
    return tab ? tab->stages : GODE_E_SHAPE;
}

extern "C" int gode_rk_tableau(int32_t method, double* c, double* a, double* b)
{
    const Tableau* tab = fixed_tableau(method);
    if (!tab) return GODE_E_SHAPE;
    const int S = tab->stages;
    for (int s = 0; s < S; ++s) {
        if (c) c[s] = tab->c[s];
        if (b) b[s] = tab->b[s];
        if (a) for (int j = 0; j < S; ++j) a[s * S + j] = j < s ? tab->a[s * tab->lda + j] : 0.0;
    }
    return 0;
}

extern "C" int gode_gcn_ode_fixed_forward(int32_t method, const gode_gcn_odefunc_t* f, float* y, float** result,
                                          const gode_rk4_workspace_t* ws, float t0, float t1, int32_t n_steps, void* stream)
{
    return forward_solve(fixed_tableau(method), f, y, result, ws, t0, t1, n_steps, stream);
}

// (the rk4 adjoint has routes of its own - the two-chain schedule of large graphs - so that code goes to its entry point)
extern "C" int gode_gcn_ode_fixed_adjoint(int32_t method, const gode_gcn_odefunc_t* f, float* y, float* a, float* theta,
                                          float** y_result, float** a_result, const gode_rk4_workspace_t* ws,
                                          float t0, float t1, int32_t n_steps, void* stream)
{
    if (!f || !y || !a || !theta || !ws || !y_result || !a_result) return GODE_E_NULLPTR;
    const Tableau* tab = fixed_tableau(method);
    if (!tab) return GODE_E_SHAPE;
    if (method == GODE_RK_RK4_38) return gode_gcn_ode_rk4_adjoint(f, y, a, theta, y_result, a_result, ws, t0, t1, n_steps, stream);
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    if (!(fused_small(f) && ws->small_part != nullptr)) return GODE_E_UNSUPPORTED;      // the launch-bound route only
    for (int s = 0; s < tab->stages; ++s) if (!ws->ky[s] || !ws->ka[s]) return GODE_E_NULLPTR;
    if (!ws->dZ) return GODE_E_NULLPTR;
    const double h = ((double)t1 - (double)t0) / n_steps;
    return fixed_adjoint_small(*tab, f, ws, y, a, theta, y_result, a_result, t0, h, n_steps, stream);
}

extern "C" int gode_gcn_ode_fixed_forward_save(int32_t method, const gode_gcn_odefunc_t* f, const float* y0, float* y_end,
                                               float* save, const gode_rk4_workspace_t* ws, float t0, float t1,
                                               int32_t n_steps, int32_t step_begin, int32_t step_end, void* stream)
{
    return forward_save(fixed_tableau(method), f, y0, y_end, save, ws, t0, t1, n_steps, step_begin, step_end, stream);
}

extern "C" int gode_gcn_ode_fixed_backprop(int32_t method, const gode_gcn_odefunc_t* f, const float* save, float* a,
                                           float* theta, float** a_result, const gode_rk4_workspace_t* ws,
                                           float* cot_colpart, float t0, float t1, int32_t n_steps, int32_t step_begin,
                                           int32_t step_end, void* stream)
{
    return backprop(fixed_tableau(method), f, save, a, theta, a_result, ws, cot_colpart, t0, t1, n_steps, step_begin, step_end,
                    stream);
}

// ---------------------------------------------------------------------------------------------------------------
// explicit_adams (4th-order Adams-Bashforth on the fixed grid): kAdamsStart 3/8-rule steps - fixed_forward_step /
// adjoint_small_step under TAB38, whose k_1 = f_i is kept - then ONE evaluation per step.  A multistep step is explicit
// Euler's closing stage with more pre terms: the launch that evaluates f_i on y_i stores f_i (the save form) and
// y_{i+1} = (y_i + h sum_{j>=1} beta_j f_{i-j}) + h beta_0 f_i.  At most kAdamsStart steps: the rk4 entry point itself.
// Arrays: y, the four ws->ky (ka) and two more per chain from `extra` take turns as the solution, the history and the stage
// buffers; nothing is allocated.
// ---------------------------------------------------------------------------------------------------------------
namespace {

// The arrays of one chain (y or a) of a multistep solve: the solution, the rk4 stage buffers and the history take turns
struct AdamsChain {
    float* cur; float* k[4]; float* spare[2];
    const float* fh[4];                                  // f_{i-1}, f_{i-2}, f_{i-3} (and the one that falls out)
    float* free_[4]; int n_free = 0;
    AdamsChain(float* y, float* const* ky, float* e0, float* e1) : cur(y), k{ky[0], ky[1], ky[2], ky[3]}, spare{e0, e1}, fh{} {}
    // after start-up step i (k[3] holds the new solution, k[0] = f_i): f_i joins the history, the chain moves on
    void close_start(int i) {
        fh[2] = fh[1]; fh[1] = fh[0]; fh[0] = k[0];
        float* tmp = cur; cur = k[3]; k[3] = tmp;
        if (i < 2) k[0] = spare[i];
        else { free_[0] = k[1]; free_[1] = k[2]; free_[2] = k[3]; n_free = 3; }
    }
    float* take() { return free_[--n_free]; }
    // after a multistep step that wrote y_{i+1} into ynext and f_i into fnew
    void close_multi(float* ynext, float* fnew) {
        if (fh[2]) free_[n_free++] = (float*)fh[2];      // f_{i-3}: no later step reads it
        free_[n_free++] = cur;
        fh[2] = fh[1]; fh[1] = fh[0]; fh[0] = fnew;
        cur = ynext;
    }
};

}  // namespace

extern "C" int gode_gcn_ode_adams_forward(const gode_gcn_odefunc_t* f, float* y, float** result,
                                          const gode_rk4_workspace_t* ws, float* const* extra, float t0, float t1,
                                          int32_t n_steps, void* stream)
{
    if (!f || !y || !ws || !result || !extra) return GODE_E_NULLPTR;
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    if (n_steps <= kAdamsStart) return gode_gcn_ode_rk4_forward(f, y, result, ws, t0, t1, n_steps, stream);
    if (!ws->S || !ws->ky[0] || !ws->ky[1] || !ws->ky[2] || !ws->ky[3] || !extra[0] || !extra[1]) return GODE_E_NULLPTR;
    const double h = ((double)t1 - (double)t0) / n_steps;
    const bool fused = fused_small(f);
    const bool close_once = close_once_route(f);
    const bool diag_ok = diag_rows_route(f, fused);
    // (option local_tail is rk4's alone: the tail rows take the launches of the other rows here)
    AdamsChain c(y, ws->ky, extra[0], extra[1]);
    for (int i = 0; i < kAdamsStart; ++i) {
        GODE_TRY(fixed_forward_step(TAB38, f, ws, c.cur, c.k, c.k[3], false, (double)t0 + i * h, h, fused, close_once, stream, diag_ok));
        c.close_start(i);
    }
    const float hb0 = (float)(h * ADAMS_B[0]);
    for (int i = kAdamsStart; i < n_steps; ++i) {
        const float ts = (float)((double)t0 + i * h);
        float* ynext = c.take(); float* fnew = c.take();
        const gode_lincomb_t xin = one_term(c.cur);
        const StepClose close = {adams_pre(c.cur, c.fh, h), hb0, false};
        if (fused) GODE_TRY(gode_gcn_feval_small_save_f32(f, &xin, ts, hb0, &close.pre, ynext, fnew, stream));
        else GODE_TRY(feval_large(f, xin, ts, ws->S, ynext, &close, fnew, stream));
        c.close_multi(ynext, fnew);
    }
    *result = c.cur;
    return 0;
}

// The adjoint solve on the launch-bound route: adjoint_small_step for the start-up (k_1 of y and of a kept), then
// two launches and the closing reduction per step - the forward recompute leaves f_i, the masked cotangent and y_{i+1}, the
// VJP leaves a's derivative for the history and a_{i+1}.  The parameter and a_t components are pure quadratures (no stage
// input reads them): every evaluation's partials are added ONCE, with the weight the evaluation ends up with (adams_weight;
// a start-up step's k_1 gets it on top of h b_1), so theta holds its value at t1 only when the call returns.
extern "C" int gode_gcn_ode_adams_adjoint(const gode_gcn_odefunc_t* f, float* y, float* a, float* theta,
                                          float** y_result, float** a_result, const gode_rk4_workspace_t* ws,
                                          float* const* extra, float t0, float t1, int32_t n_steps, void* stream)
{
    if (!f || !y || !a || !theta || !ws || !y_result || !a_result || !extra) return GODE_E_NULLPTR;
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    if (!(fused_small(f) && ws->small_part != nullptr)) return GODE_E_UNSUPPORTED;      // the launch-bound route only
    if (n_steps <= kAdamsStart) return gode_gcn_ode_rk4_adjoint(f, y, a, theta, y_result, a_result, ws, t0, t1, n_steps, stream);
    for (int s = 0; s < 4; ++s) if (!ws->ky[s] || !ws->ka[s] || !extra[s]) return GODE_E_NULLPTR;
    if (!ws->dZ) return GODE_E_NULLPTR;
    const double h = ((double)t1 - (double)t0) / n_steps;   // negative: the adjoint runs from t0 (later) to t1 (earlier)
    AdamsChain cy(y, ws->ky, extra[0], extra[1]), ca(a, ws->ka, extra[2], extra[3]);
    for (int i = 0; i < kAdamsStart; ++i) {
        GODE_TRY(adjoint_small_step(TAB38, f, ws, cy.cur, cy.k, ca.cur, ca.k, theta, (double)t0 + i * h, h,
                                    adams_weight(i, n_steps, h), stream));
        cy.close_start(i);
        ca.close_start(i);
    }
    const float hb0 = (float)(h * ADAMS_B[0]);
    for (int i = kAdamsStart; i < n_steps; ++i) {
        const float ts = (float)((double)t0 + i * h);
        float* ynext = cy.take(); float* fnew = cy.take();
        float* anext = ca.take(); float* ganew = ca.take();
        const gode_lincomb_t yin = one_term(cy.cur);
        const gode_lincomb_t ypre = adams_pre(cy.cur, cy.fh, h), apre = adams_pre(ca.cur, ca.fh, h);
        const gode_lincomb_t cot = negated(one_term(ca.cur));
        GODE_TRY(gode_gcn_feval_small_save_cot_f32(f, &yin, ts, hb0, &ypre, &cot, ws->dZ, ynext, fnew, stream));
        GODE_TRY(gode_gcn_vjp_small_raw_f32(f, &yin, ws->dZ, hb0, &apre, anext, ws->small_part, ganew, stream));
        const float w = (float)adams_weight(i, n_steps, h);
        GODE_TRY(gode_gcn_small_finish_step_f32(f, ws->small_part, 1, theta, &w, &ts, stream));
        cy.close_multi(ynext, fnew);
        ca.close_multi(anext, ganew);
    }
    *y_result = cy.cur;
    *a_result = ca.cur;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Backprop through an explicit_adams solve.  Records are compact: a start-up step keeps [ y_i | k_1..k_4 ] (5 n d floats,
// the rk4 record), a multistep step [ y_i | f_i ] (2 n d); in both f_i sits right behind y_i.  With ybar_{m+1} the
// cotangent of y_{m+1}, f_i receives  fbar_i = sum_j h beta_j ybar_{i+j+1}  over the multistep steps m = i + j >= 3 that read
// it (j <= 3, m <= n - 1): at most the four latest cotangents are pending.  A multistep step is then ONE stage,
//   ybar_i = ybar_{i+1} + J_i^T fbar_i,   theta += (df/dtheta)_i^T fbar_i,   the mask [f_i > 0] from the record;
// a start-up step is the rk4 sweep's step with fbar_i added to kbar_1 (4 + at most 3 terms).
// ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t gode_adams_record_offset(int32_t step, int64_t nd)
{
    if (step < 0 || nd < 0) return GODE_E_SHAPE;
    const int64_t start = step < kAdamsStart ? step : kAdamsStart;
    return (5 * start + 2 * (int64_t)(step - start)) * nd;
}

extern "C" int gode_gcn_ode_adams_forward_save(const gode_gcn_odefunc_t* f, const float* y0, float* y_end, float* save,
                                               const float* const* hist, const gode_rk4_workspace_t* ws, float t0, float t1,
                                               int32_t n_steps, int32_t step_begin, int32_t step_end, void* stream)
{
    if (!f || !y0 || !y_end || !save || !ws) return GODE_E_NULLPTR;
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    if (step_begin < 0 || step_end > n_steps || step_begin >= step_end) return GODE_E_SHAPE;
    if (n_steps <= kAdamsStart)
        return gode_gcn_ode_rk4_forward_save(f, y0, y_end, save, ws, t0, t1, n_steps, step_begin, step_end, stream);
    if (!ws->S) return GODE_E_NULLPTR;
    if (step_begin > 0 && step_end > kAdamsStart) {               // f of up to three steps before step_begin
        if (!hist) return GODE_E_NULLPTR;
        for (int j = 0; j < kAdamsStart && j < step_begin; ++j) if (!hist[j]) return GODE_E_NULLPTR;
    }
    const int64_t nd = f->n * f->d;
    const double h = ((double)t1 - (double)t0) / n_steps;
    const bool fused = fused_small(f);
    const bool close_once = close_once_route(f);
    auto record = [&](int i) { return save + (gode_adams_record_offset(i, nd) - gode_adams_record_offset(step_begin, nd)); };
    auto f_of = [&](int j) -> const float* { return j >= step_begin ? record(j) + nd : hist[step_begin - 1 - j]; };
    if (y0 != save) {                                            // record 0 starts with a copy of y0
        const gode_lincomb_t c = one_term(y0);
        GODE_TRY(gode_lincomb_f32(save, &c, nd, stream));
    }
    const float hb0 = (float)(h * ADAMS_B[0]);
    for (int i = step_begin; i < step_end; ++i) {
        float* rec = record(i);
        float* ynext = (i + 1 < step_end) ? record(i + 1) : y_end;       // the next record's y_i, or the result
        if (i < kAdamsStart) {
            float* k[4] = {rec + nd, rec + 2 * nd, rec + 3 * nd, rec + 4 * nd};
            GODE_TRY(fixed_forward_step(TAB38, f, ws, rec, k, ynext, true, (double)t0 + i * h, h, fused, close_once, stream));
            continue;
        }
        const float* fh[3] = {f_of(i - 1), f_of(i - 2), f_of(i - 3)};
        const float ts = (float)((double)t0 + i * h);
        const gode_lincomb_t xin = one_term(rec);
        const StepClose close = {adams_pre(rec, fh, h), hb0, false};
        if (fused) GODE_TRY(gode_gcn_feval_small_save_f32(f, &xin, ts, hb0, &close.pre, ynext, rec + nd, stream));
        else GODE_TRY(feval_large(f, xin, ts, ws->S, ynext, &close, rec + nd, stream));
    }
    return 0;
}

namespace {

// The pending cotangents of the sweep: P[j] = ybar_{i+1+j}, j < count <= 4, in a ring of five arrays
struct AdamsPending {
    float* P[4]; int count;
    float* free_[5]; int n_free;
    float* take() { return free_[--n_free]; }
    void push(float* ybar_i) {
        if (count == 4) free_[n_free++] = P[3]; else ++count;
        P[3] = P[2]; P[2] = P[1]; P[1] = P[0]; P[0] = ybar_i;
    }
};
// lc + fbar_i: the terms h beta_j ybar_{i+j+1} of the multistep steps i + j (>= 3, <= n - 1) that read f_i
gode_lincomb_t adams_fbar(gode_lincomb_t lc, const AdamsPending& p, int i, int n, double h) {
    for (int j = i < kAdamsStart ? kAdamsStart - i : 0; j <= 3 && i + j <= n - 1; ++j) {
        lc.coef[lc.n] = (float)(h * ADAMS_B[j]); lc.ptr[lc.n] = p.P[j]; ++lc.n;
    }
    return lc;
}

}  // namespace

// save: the records of steps 0 .. n_steps - 1 (gode_adams_record_offset) - or, with `rerun` given (5 n d floats), the
// start-up steps' y_0, y_1, y_2 alone (3 n d floats) followed by the multistep records: each start-up step is then re-run
// into `rerun` (fixed_forward_step, the forward's launches) just before its sweep.  work: four n x d arrays; with `a` they
// hold the pending cotangents, and *a_result names the one that holds dL/dy_0.
extern "C" int gode_gcn_ode_adams_backprop(const gode_gcn_odefunc_t* f, const float* save, float* rerun, float* a, float* theta,
                                           float** a_result, const gode_rk4_workspace_t* ws, float* cot_colpart,
                                           float* const* work, float t0, float t1, int32_t n_steps, void* stream)
{
    if (!f || !save || !a || !theta || !a_result || !ws || !work) return GODE_E_NULLPTR;
    if (n_steps <= 0 || f->n <= 0 || f->d <= 0) return GODE_E_SHAPE;
    if (n_steps <= kAdamsStart) {
        if (rerun) return GODE_E_SHAPE;                           // the rk4 sweep's own re-run mode is its caller's
        return gode_gcn_ode_rk4_backprop(f, save, a, theta, a_result, ws, cot_colpart, t0, t1, n_steps, 0, n_steps, stream);
    }
    for (int s = 0; s < 4; ++s) if (!ws->ka[s] || !ws->ktheta[s] || !work[s]) return GODE_E_NULLPTR;
    if (!ws->dZ || !ws->dS || !ws->wpart || !ws->colsum_scratch) return GODE_E_NULLPTR;
    if (f->groups > 0 && (!ws->gpart || !ws->bpart)) return GODE_E_NULLPTR;
    if (rerun && !ws->S) return GODE_E_NULLPTR;
    const int64_t n = f->n, d = f->d, nd = n * d, P = gode_gcn_ode_theta_len(d);
    const double h = ((double)t1 - (double)t0) / n_steps;
    const bool fused = fused_small(f) && ws->small_part != nullptr;
    const bool close_once = close_once_route(f);
    const int64_t slot = fused ? gode_gcn_small_parts(n) * gode_gcn_small_part_len(d) : 0;
    const SweepRoute route = sweep_route(f, ws, cot_colpart);
    const int64_t multi0 = rerun ? (int64_t)kAdamsStart * nd : gode_adams_record_offset(kAdamsStart, nd);
    auto multi = [&](int i) { return save + multi0 + (int64_t)(i - kAdamsStart) * 2 * nd; };
    AdamsPending pend = {{a, nullptr, nullptr, nullptr}, 1, {work[0], work[1], work[2], work[3], nullptr}, 4};
    float* dz[2] = {ws->dZ, ws->dS};
    int cur = 0;
    const float one = 1.f;
    gode_lincomb_t none; none.n = 0;
    if (fused) {                                                 // the masked cotangent of the last step opens the chain
        const gode_lincomb_t c = adams_fbar(none, pend, n_steps - 1, n_steps, h);
        GODE_TRY(gode_masked_cot_f32(&c, multi(n_steps - 1) + nd, dz[0], n, d, nullptr, stream));
    }
    for (int i = n_steps - 1; i >= kAdamsStart; --i) {
        const float* rec = multi(i);
        const float ts = (float)((double)t0 + i * h);
        const gode_lincomb_t yin = one_term(rec), pre = one_term(pend.P[0]);
        float* out = pend.take();
        if (!fused) {
            const gode_lincomb_t cot = adams_fbar(none, pend, i, n_steps, h);
            GODE_TRY(sweep_stage(f, ws, route, cot, rec + nd, yin, &pre, out, ws->ktheta[0], ts, stream));
            GODE_TRY(add_stage_parts(theta, ws->ktheta, 1, P, stream));
            pend.push(out);
            continue;
        }
        if (i > kAdamsStart) {                                   // ... and every VJP launch forms the next step's
            AdamsPending nxt = pend;
            nxt.push(out);                                       // names `out`: this launch's rows
            const gode_lincomb_t cn = adams_fbar(none, nxt, i - 1, n_steps, h);
            GODE_TRY(gode_gcn_vjp_small_next_f32(f, &yin, dz[cur], 1.f, &pre, out, ws->small_part, &cn, multi(i - 1) + nd,
                                                 dz[cur ^ 1], stream));
            cur ^= 1;
        } else {
            GODE_TRY(gode_gcn_vjp_small_f32(f, &yin, dz[cur], 1.f, &pre, out, ws->small_part, stream));
        }
        GODE_TRY(gode_gcn_small_finish_step_f32(f, ws->small_part, 1, theta, &one, &ts, stream));
        pend.push(out);
    }
    float* yb[4] = {nullptr, ws->ka[1], ws->ka[2], ws->ka[3]};   // yb[1..3]: Ybar_2..4 of a start-up step; yb[0]: ybar_i
    for (int i = kAdamsStart - 1; i >= 0; --i) {
        const double t = (double)t0 + i * h;
        const float* y = rerun ? save + (int64_t)i * nd : save + gode_adams_record_offset(i, nd);
        float* k[4];
        if (rerun) {
            for (int s = 0; s < 4; ++s) k[s] = rerun + (int64_t)(s + 1) * nd;
            GODE_TRY(fixed_forward_step(TAB38, f, ws, y, k, rerun, true, t, h, fused_small(f), close_once, stream));
        } else {
            for (int s = 0; s < 4; ++s) k[s] = (float*)y + (int64_t)(s + 1) * nd;
        }
        const float* abar = pend.P[0];
        yb[0] = pend.take();
        const gode_lincomb_t pre = sweep_pre(TAB38, abar, 1.f, yb, 1);
        // kbar_s of the rk4 sweep; kbar_1 also carries fbar_i
        auto kbar = [&](int s) {
            const gode_lincomb_t c = stage_cotangent(TAB38, abar, (float)(h * B38[s]), yb, s, h);
            return s == 0 ? adams_fbar(c, pend, i, n_steps, h) : c;
        };
        if (fused) {
            const gode_lincomb_t c4 = kbar(3);
            GODE_TRY(gode_masked_cot_f32(&c4, k[3], dz[cur], n, d, nullptr, stream));
            float stage_t[4];
            for (int s = 3; s >= 0; --s) {
                stage_t[s] = (float)(t + C38[s] * h);
                const gode_lincomb_t yin = tab_stage_terms(TAB38, y, k, s, h);
                float* part = ws->small_part + s * slot;
                if (s > 0) {
                    const gode_lincomb_t nxt = kbar(s - 1);                      // names yb[s]: this launch's rows
                    GODE_TRY(gode_gcn_vjp_small_next_f32(f, &yin, dz[cur], 1.f, nullptr, yb[s], part, &nxt, k[s - 1],
                                                         dz[cur ^ 1], stream));
                    cur ^= 1;
                } else {
                    GODE_TRY(gode_gcn_vjp_small_f32(f, &yin, dz[cur], 1.f, &pre, yb[0], part, stream));
                }
            }
            const float w1[4] = {1.f, 1.f, 1.f, 1.f};               // h is already inside kbar
            GODE_TRY(gode_gcn_small_finish4_f32(f, ws->small_part, theta, w1, stage_t, stream));
        } else {
            for (int s = 3; s >= 0; --s)
                GODE_TRY(sweep_stage(f, ws, route, kbar(s), k[s], tab_stage_terms(TAB38, y, k, s, h), s == 0 ? &pre : nullptr, yb[s],
                                     ws->ktheta[s], (float)(t + C38[s] * h), stream));
            GODE_TRY(add_stage_parts(theta, ws->ktheta, 4, P, stream));
        }
        pend.push(yb[0]);
    }
    *a_result = pend.P[0];
    return 0;
}
