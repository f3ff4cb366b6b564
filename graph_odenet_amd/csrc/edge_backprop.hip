// edge_backprop.hip — the reverse sweep of a backprop solve over the edge-conditioned ODE function (qc_ode.py),
//     S = [t | GN(Y)] W,   k = relu(Etgt . bmm(A, S[Esrc]) + b),
// on launch-bound batches.  k of every stage is on record, so the sweep re-evaluates nothing, and everything after the
// edge gather is local to a row, so a stage needs no reduction of its own.  Two entry points:
//   gode_edge_ode_stage_bwd_f32   one launch per stage, a block per atom u: the masked cotangent dM[u], dS[u] through the
//                                 source incidence, the GroupNorm / time / GEMM VJP of the row into Ybar[u], the row's dgamma
//                                 and dbeta shares, and (on request) S[u] for the edge-matrix outer sum
//   gode_edge_ode_step_close_f32  one launch per RK step: the parameter gradients of up to 8 stages added into the packed
//                                 buffer [W | b | gamma | beta] (the weight partials are gode_wgrad_f32's, one launch a stage)
// Deterministic: every sum runs in a fixed order, no float atomics.
#include "common.h"
#include "dense_common.h"
#include "prof.h"

namespace {

constexpr int kRound = 16;               // edges of a source whose cotangent rows are staged together (edge_ode_vjp_kernel)
constexpr int kCloseCols = 16;           // step-close: columns of a column-sum block; 256 / kCloseCols row lanes

struct StageBwdOut { float* dM; float* dS; float* ybar; float* dgamma_rows; float* dbeta_rows; float* S; };

// block u.  Phase 1 is edge_ode_vjp_kernel's by-source form: the cotangent rows an edge needs are formed from the terms
// (never read back from dM: other blocks write it); column j of A_e is read by thread j, the h rows split over 256 / hp
// thread groups whose partial sums meet in LDS in a fixed order.  Phase 2 works on the row alone: GroupNorm statistics of
// Y[u], S[u] with the rows of W split over the same thread groups, dy = W[1:] dS[u] with a wave per row of W (the lanes
// read the row contiguously and meet in a butterfly, the same value in every lane), and ATen's GroupNorm backward.
__global__ __launch_bounds__(256) void edge_ode_stage_bwd_kernel(const int* __restrict__ ms_rowptr, const int* __restrict__ ms_eid,
                                                                 const int* __restrict__ erow, const float* __restrict__ eval,
                                                                 const float* __restrict__ A, LinComb cot, float cot_scale,
                                                                 const float* __restrict__ k, LinComb yin, float t,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ W, int h, int groups, float eps,
                                                                 StageBwdOut o) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int es[kRound], rs[kRound];
    __shared__ float vs[kRound];
    float* dm = smem;                          // [kRound][h]
    float* red = dm + kRound * h;              // [256 / hp][hp]
    float* xs = red + 256;                     // [h] the row of the stage input
    float* xn = xs + h;                        // [h] its GroupNorm
    float* ds = xn + h;                        // [h] dS[u]
    float* dy = ds + h;                        // [h] cotangent of GN(Y)[u]
    float* st = dy + h;                        // [groups][4] mean, rstd, sum dh x, sum dh
    const int u = blockIdx.x, tid = threadIdx.x, hh = h * h, ti = tid < h ? tid : h - 1;
    const int64_t ridx = (int64_t)u * h + ti;
    {
        const float x = lc_load1(yin, ridx), g = masked_cot(cot, cot_scale, k, ridx);
        if (tid < h) { xs[tid] = x; o.dM[ridx] = g; }
    }
    const int kb = ms_rowptr[u], ke = ms_rowptr[u + 1];
    const int hp = h > 1 ? 1 << (32 - __clz(h - 1)) : 1;       // h rounded up to a power of two
    const int G = 256 / hp, j = tid & (hp - 1), grp = tid / hp, jj = j < h ? j : h - 1;
    const int rpg = (h + G - 1) / G, i0 = min(h, grp * rpg), i1 = min(h, i0 + rpg);
    float acc = 0.f;
    for (int base = kb; base < ke; base += kRound) {
        const int cnt = min(kRound, ke - base);
        __syncthreads();
        if (tid < cnt) {
            const int q = base + tid, e = ms_eid ? ms_eid[q] : q;
            es[tid] = e; rs[tid] = erow[e]; vs[tid] = eval ? eval[e] : 1.f;
        }
        __syncthreads();
        for (int idx = tid; idx < cnt * h; idx += 256) {
            const int q = idx / h, c = idx - q * h, row = rs[q];
            const float g = masked_cot(cot, cot_scale, k, (int64_t)(row >= 0 ? row : 0) * h + c);
            dm[idx] = row >= 0 ? vs[q] * g : 0.f;
        }
        __syncthreads();
        for (int q = 0; q < cnt; ++q) {
            const float* Aj = A + (int64_t)es[q] * hh + jj;
            const float* dq = dm + q * h;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            int i = i0;
            for (; i + 8 <= i1; i += 8) {                        // eight rows per trip, their loads requested together
                float a[8];
#pragma unroll
                for (int v = 0; v < 8; ++v) a[v] = Aj[(int64_t)(i + v) * h];
                s0 = fmaf(a[0], dq[i], s0); s1 = fmaf(a[1], dq[i + 1], s1); s2 = fmaf(a[2], dq[i + 2], s2); s3 = fmaf(a[3], dq[i + 3], s3);
                s0 = fmaf(a[4], dq[i + 4], s0); s1 = fmaf(a[5], dq[i + 5], s1); s2 = fmaf(a[6], dq[i + 6], s2); s3 = fmaf(a[7], dq[i + 7], s3);
            }
            for (; i < i1; ++i) s0 = fmaf(Aj[(int64_t)i * h], dq[i], s0);
            acc += (s0 + s1) + (s2 + s3);
        }
    }
    red[grp * hp + j] = acc;
    __syncthreads();                                             // red, and xs of the prologue
    if (tid < h) {
        float s = 0.f;
        for (int g = 0; g < G; ++g) s += red[g * hp + tid];
        ds[tid] = s;
        o.dS[(int64_t)u * h + tid] = s;
    }
    const int cg = h / groups;
    if (tid < groups) {                                          // the statistics of stage_rows_gn (gemm.hip)
        const float* p = xs + tid * cg;
        float m = 0.f;
        for (int c = 0; c < cg; ++c) m += p[c];
        m /= cg;
        float v = 0.f;
        for (int c = 0; c < cg; ++c) v += (p[c] - m) * (p[c] - m);
        v /= cg;
        st[tid * 4] = m; st[tid * 4 + 1] = 1.0f / sqrtf(v + eps);
    }
    __syncthreads();
    {
        const int gi = ti / cg;
        const float v = gn_apply1(xs[ti], st[gi * 4], st[gi * 4 + 1], gamma[ti], beta[ti]);
        if (tid < h) xn[tid] = v;
    }
    __syncthreads();
    if (o.S) {                                                   // S[u] = t W[0] + GN(Y[u]) W[1:], uniform branch
        float s0 = 0.f, s1 = 0.f;
        int i = i0;
        for (; i + 2 <= i1; i += 2) {
            s0 = fmaf(xn[i], W[(int64_t)(i + 1) * h + jj], s0);
            s1 = fmaf(xn[i + 1], W[(int64_t)(i + 2) * h + jj], s1);
        }
        for (; i < i1; ++i) s0 = fmaf(xn[i], W[(int64_t)(i + 1) * h + jj], s0);
        red[grp * hp + j] = s0 + s1;
        __syncthreads();
        const float w0 = W[ti];
        if (tid < h) {
            float s = t * w0;
            for (int g = 0; g < G; ++g) s += red[g * hp + tid];
            o.S[(int64_t)u * h + tid] = s;
        }
    }
    {
        const int wave = tid >> 6, lane = tid & 63, l1 = lane + 64 < h ? lane + 64 : h - 1, l0 = lane < h ? lane : h - 1;
        const float d0 = lane < h ? ds[l0] : 0.f, d1 = lane + 64 < h ? ds[l1] : 0.f;
        for (int i = wave; i < h; i += 8) {                      // two rows per trip, their loads requested together
            const int i2 = i + 4 < h ? i + 4 : i;                // past the end: the same row again (no load under a branch)
            const float* wa = W + (int64_t)(i + 1) * h;
            const float* wb = W + (int64_t)(i2 + 1) * h;
            const float a0 = wa[l0], a1 = wa[l1], b0 = wb[l0], b1 = wb[l1];
            const float va = wave_sum(fmaf(a0, d0, a1 * d1)), vb = wave_sum(fmaf(b0, d0, b1 * d1));
            if (lane == 0) { dy[i] = va; dy[i2] = vb; }
        }
    }
    __syncthreads();
    if (tid < groups) {                                          // ds, db of ATen's GroupNorm backward
        float dsum = 0.f, bsum = 0.f;
        for (int c = 0; c < cg; ++c) {
            const int cc = tid * cg + c;
            const float dh = dy[cc] * gamma[cc];
            dsum += dh * xs[cc]; bsum += dh;
        }
        st[tid * 4 + 2] = dsum; st[tid * 4 + 3] = bsum;
    }
    __syncthreads();
    {
        const int gi = ti / cg;
        const float gm = gamma[ti];
        if (tid < h) {
            const float m = st[gi * 4], rstd = st[gi * 4 + 1], dsum = st[gi * 4 + 2], bsum = st[gi * 4 + 3];
            const float sc = 1.0f / cg;
            const float c2 = (bsum * m - dsum) * rstd * rstd * rstd * sc;
            const float c3 = -c2 * m - bsum * rstd * sc;
            const int64_t idx = (int64_t)u * h + tid;
            o.ybar[idx] = rstd * gm * dy[tid] + c2 * xs[tid] + c3;
            o.dgamma_rows[idx] = dy[tid] * (xs[tid] - m) * rstd;
            o.dbeta_rows[idx] = dy[tid];
        }
    }
}

struct StepClose {
    int n;
    float ts[GODE_MAX_TERMS];
    const float* wpart[GODE_MAX_TERMS]; const float* dM[GODE_MAX_TERMS];
    const float* dgamma_rows[GODE_MAX_TERMS]; const float* dbeta_rows[GODE_MAX_TERMS];
};

// blocks [0, w_blocks): 256 entries of W each, theta[W][j] += sum_s scale_s(j) sum_p wpart_s[p][j], scale_s = t_s on the
// time row (j < h), else 1.  The blocks after them: kCloseCols columns of b, gamma or beta, the rows of the stages'
// dM / dgamma / dbeta arrays split over 16 row lanes that meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void edge_ode_step_close_kernel(StepClose g, int n_wparts, int n_rows, int h, int w_blocks,
                                                                  float* __restrict__ theta) {
    __shared__ float sm[256 / kCloseCols][kCloseCols + 1];
    const int tid = threadIdx.x, wlen = (h + 1) * h;
    if ((int)blockIdx.x < w_blocks) {
        const int j = blockIdx.x * 256 + tid, jc = j < wlen ? j : wlen - 1;
        float v = 0.f;
        for (int s = 0; s < g.n; ++s) {
            const float* part = g.wpart[s] + jc;
            float a = 0.f;
            for (int p = 0; p < n_wparts; ++p) a += part[(int64_t)p * wlen];
            v = fmaf(jc < h ? g.ts[s] : 1.f, a, v);
        }
        const float old = theta[jc];
        if (j < wlen) theta[j] = old + v;
        return;
    }
    const int b = blockIdx.x - w_blocks, cb = (h + kCloseCols - 1) / kCloseCols, seg = b / cb;
    const int col = (b - seg * cb) * kCloseCols + (tid & (kCloseCols - 1)), cc = col < h ? col : h - 1, rl = tid / kCloseCols;
    float a = 0.f;
    for (int s = 0; s < g.n; ++s) {
        const float* src = (seg == 0 ? g.dM[s] : seg == 1 ? g.dgamma_rows[s] : g.dbeta_rows[s]) + cc;
        float as = 0.f;
        for (int r = rl; r < n_rows; r += 256 / kCloseCols) as += src[(int64_t)r * h];
        a += as;
    }
    sm[rl][tid & (kCloseCols - 1)] = a;
    __syncthreads();
    if (rl == 0 && col < h) {
        float s = 0.f;
        for (int q = 0; q < 256 / kCloseCols; ++q) s += sm[q][tid];
        theta[wlen + seg * h + col] += s;
    }
}

}  // namespace

extern "C" int gode_edge_ode_stage_bwd_supported(int64_t n_rows, int64_t h, int32_t groups) {
    if (n_rows < 1 || n_rows > INT32_MAX || h < 1 || !gode_edge_ode_supported(h) || groups < 1 || h % groups) return 0;
    const int64_t cg = h / groups;
    return cg >= 1 && cg <= 3 ? 1 : 0;
}

extern "C" int gode_edge_ode_stage_bwd_f32(const int32_t* ms_rowptr, const int32_t* ms_eid, const int32_t* edge_row,
                                           const float* edge_val, const float* A, const gode_lincomb_t* cot, float cot_scale,
                                           const float* k, const gode_lincomb_t* yin, float t, const float* gamma,
                                           const float* beta, const float* W, int32_t groups, float eps, int64_t h,
                                           int64_t n_rows, int64_t n_edges, float* dM, float* dS, float* ybar,
                                           float* dgamma_rows, float* dbeta_rows, float* S, void* stream) {
    if (n_rows < 0 || n_edges < 0 || h <= 0 || groups < 0) return GODE_E_SHAPE;
    if (!gode_edge_ode_supported(h) || n_rows > INT32_MAX || n_edges > INT32_MAX) return GODE_E_RANGE;
    int rc = check_lincomb(cot, true); if (rc) return rc;
    rc = check_lincomb(yin, true); if (rc) return rc;
    if (n_rows == 0) return 0;
    if (!ms_rowptr || !k || !gamma || !beta || !W || !dM || !dS || !ybar || !dgamma_rows || !dbeta_rows) return GODE_E_NULLPTR;
    if (n_edges > 0 && (!edge_row || !A)) return GODE_E_NULLPTR;
    if (groups > 0 && h % groups) return GODE_E_SHAPE;
    if (!gode_edge_ode_stage_bwd_supported(n_rows, h, groups)) return GODE_E_UNSUPPORTED;
    // a block forms the cotangent rows of OTHER atoms from the terms while their blocks write the outputs
    float* const outs[6] = {dM, dS, ybar, dgamma_rows, dbeta_rows, S};
    for (int a = 0; a < 6; ++a) {
        if (!outs[a]) continue;
        if (outs[a] == k) return GODE_E_SHAPE;
        for (int j = 0; j < cot->n; ++j) if (cot->ptr[j] == outs[a]) return GODE_E_SHAPE;
        for (int j = 0; j < yin->n; ++j) if (yin->ptr[j] == outs[a]) return GODE_E_SHAPE;
        for (int b = a + 1; b < 6; ++b) if (outs[a] == outs[b]) return GODE_E_SHAPE;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)(kRound * h + 256 + 4 * h + 4 * groups) * sizeof(float);
    StageBwdOut o{dM, dS, ybar, dgamma_rows, dbeta_rows, S};
    const int slot = gode_prof_begin(s, h, n_rows, (int64_t)cot->n + yin->n, GODE_PROF_EDGE_STAGE_BWD);
    hipLaunchKernelGGL(edge_ode_stage_bwd_kernel, dim3((unsigned)n_rows), dim3(256), lds, s, ms_rowptr, ms_eid, edge_row, edge_val,
                       A, make_lincomb(cot), cot_scale, k, make_lincomb(yin), t, gamma, beta, W, (int)h, (int)groups, eps, o);
    gode_prof_end(s, slot);
    GODE_LAUNCH_CHECK();
    return 0;
}

extern "C" int gode_edge_ode_step_close_f32(int32_t n_stages, const float* const* wpart, const float* const* dM,
                                            const float* const* dgamma_rows, const float* const* dbeta_rows, const float* ts,
                                            int64_t n_wparts, int64_t n_rows, int64_t h, float* theta, void* stream) {
    if (n_rows < 0 || n_wparts < 0 || h <= 0) return GODE_E_SHAPE;
    if (n_stages < 1 || n_stages > GODE_MAX_TERMS || !gode_edge_ode_supported(h) || n_rows > INT32_MAX || n_wparts > INT32_MAX)
        return GODE_E_RANGE;
    if (!wpart || !dM || !dgamma_rows || !dbeta_rows || !ts || !theta) return GODE_E_NULLPTR;
    StepClose g;
    g.n = n_stages;
    for (int q = 0; q < GODE_MAX_TERMS; ++q) {
        const bool on = q < n_stages;
        if (on && (!dM[q] || !dgamma_rows[q] || !dbeta_rows[q] || (n_wparts > 0 && !wpart[q]))) return GODE_E_NULLPTR;
        g.ts[q] = on ? ts[q] : 0.f; g.wpart[q] = on ? wpart[q] : nullptr; g.dM[q] = on ? dM[q] : nullptr;
        g.dgamma_rows[q] = on ? dgamma_rows[q] : nullptr; g.dbeta_rows[q] = on ? dbeta_rows[q] : nullptr;
    }
    hipStream_t s = (hipStream_t)stream;
    const int w_blocks = (int)(((h + 1) * h + 255) / 256);
    const int blocks = w_blocks + 3 * (int)((h + kCloseCols - 1) / kCloseCols);
    const int slot = gode_prof_begin(s, h, n_rows, (int64_t)n_stages, GODE_PROF_EDGE_STEP_CLOSE);
    hipLaunchKernelGGL(edge_ode_step_close_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g, (int)n_wparts, (int)n_rows, (int)h,
                       w_blocks, theta);
    gode_prof_end(s, slot);
    GODE_LAUNCH_CHECK();
    return 0;
}
