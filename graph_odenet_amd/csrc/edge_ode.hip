// edge_ode.hip — the edge-conditioned ODE function of the QM9 models,
//     S = [t | GN(X)] W  (gemm.hip),   f = relu(Etgt . bmm(A, S[Esrc]) + b),
// and its vector-Jacobian product (qc_ode.py).  Four entry points:
//   gode_edge_ode_feval_f32      message + per-target sum + bias + relu (+ the RK solution combine) in one launch; the
//                                E x h message array is never written
//   gode_edge_ode_feval_save_f32 the same launch, also storing f itself (the stage derivative a folded last rk4 stage
//                                never materialises: backprop through the solve needs it as the relu mask)
//   gode_edge_ode_vjp_f32        masked stage cotangent dM formed from its RK terms inside the kernel; dS through the source
//                                incidence (launch-bound batches) or dxe per edge (large batches); no dA
//   gode_edge_outer_sum_acc_f32  dA (+)= sum_s w_s (val dM_s[tgt]) (x) S_s[src]: the four stages of a fixed-grid step in
//                                one pass, RK weights applied, accumulated into the adjoint component
// Deterministic: every sum runs in a fixed order, no float atomics.
#include "common.h"
#include "prof.h"

constexpr int kEdgeOdeMaxH = 112;        // the padded h x (h + 1) LDS tile + index triples stay under 64 KB
constexpr int kVjpRound = 16;            // edges of a source whose cotangent rows are staged together

// block per target atom v.  The index triples (edge id, value, source atom) of up to 256 of its edges are fetched
// together; the matrix of edge q + 1 is requested (into registers) before the products of edge q start, so an edge
// costs one load round trip, overlapped with the previous edge's arithmetic.  Thread i owns output element i and reads
// row i of the LDS tile at stride h + 1 (conflict-free).
// SAVE: relu(z) is also stored to ksave, before the pre / alpha combine.
template <int PF, bool SAVE>
__global__ __launch_bounds__(256) void edge_ode_feval_kernel(const int* __restrict__ rowptr, const int* __restrict__ eid,
                                                             const float* __restrict__ val, const int* __restrict__ src,
                                                             const float* __restrict__ A, const float* __restrict__ S,
                                                             int h, const float* __restrict__ bias, LinComb pre, float alpha,
                                                             float* __restrict__ out, float* __restrict__ ksave) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int es[256], ss[256];
    __shared__ float vs[256];
    float* xs = smem;                    // [h]
    float* tile = smem + h;              // [h][h + 1]
    const int v = blockIdx.x, tid = threadIdx.x, hh = h * h, ti = tid < h ? tid : h - 1;
    const int rb = rowptr[v], ne = rowptr[v + 1] - rb;
    float acc = 0.f;
    for (int base = 0; base < ne; base += 256) {
        const int cnt = min(256, ne - base);
        __syncthreads();
        if (tid < cnt) {
            const int k = rb + base + tid, e = eid ? eid[k] : k;
            es[tid] = e; vs[tid] = val ? val[k] : 1.f; ss[tid] = src[e];
        }
        __syncthreads();
        float pa[PF], xa;
        auto issue = [&](int q) {
            const float* Ae = A + (int64_t)es[q] * hh;
#pragma unroll
            for (int u = 0; u < PF; ++u) { const int p = tid + 256 * u; pa[u] = Ae[p < hh ? p : hh - 1]; }
            xa = S[(int64_t)ss[q] * h + ti];
        };
        issue(0);
        for (int q = 0; q < cnt; ++q) {
            __syncthreads();                                     // the previous edge's tile is done with
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int p = tid + 256 * u;
                if (p < hh) { const int i = p / h; tile[i * (h + 1) + (p - i * h)] = pa[u]; }
            }
            if (tid < h) xs[tid] = xa;
            __syncthreads();
            issue(q + 1 < cnt ? q + 1 : q);                      // past the end: the same edge again (no load under a branch)
            const float* row = tile + ti * (h + 1);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            int j = 0;
            for (; j + 4 <= h; j += 4) {
                s0 = fmaf(row[j], xs[j], s0); s1 = fmaf(row[j + 1], xs[j + 1], s1);
                s2 = fmaf(row[j + 2], xs[j + 2], s2); s3 = fmaf(row[j + 3], xs[j + 3], s3);
            }
            for (; j < h; ++j) s0 = fmaf(row[j], xs[j], s0);
            acc = fmaf(vs[q], (s0 + s1) + (s2 + s3), acc);
        }
    }
    if (tid < h) {
        const int64_t idx = (int64_t)v * h + tid;
        const float r = fmaxf(acc + bias[tid], 0.f);
        if (SAVE) ksave[idx] = r;
        out[idx] = pre.n > 0 ? fmaf(alpha, r, lc_load1(pre, idx)) : alpha * r;
    }
}

// One block per unit of work:
//   by source (ms_rowptr given): block u writes dM[u] and dS[u] = sum over the edges leaving u of A_e^T (val_e dM[tgt_e]);
//   by edge   (ms_rowptr NULL):  blocks 0 .. n_rows - 1 write dM rows, block n_rows + e writes dxe[e] = A_e^T (val_e dM[tgt_e]).
// The cotangent rows an edge needs are formed from the RK terms (never read back from dM: other blocks write it).
// Column j of A_e is read by thread j (consecutive addresses across the wave); the h rows are split over 256 / hp thread
// groups whose partial sums meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void edge_ode_vjp_kernel(const int* __restrict__ ms_rowptr, const int* __restrict__ ms_eid,
                                                           const int* __restrict__ erow, const float* __restrict__ eval,
                                                           const float* __restrict__ A, LinComb cot, float cot_scale,
                                                           const float* __restrict__ fout, int h, int hp, int n_rows,
                                                           float* __restrict__ dM, float* __restrict__ dS,
                                                           float* __restrict__ dxe) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int es[kVjpRound], rs[kVjpRound];
    __shared__ float vs[kVjpRound];
    float* dm = smem;                          // [kVjpRound][h]
    float* red = smem + kVjpRound * h;         // [256 / hp][hp]
    const int b = blockIdx.x, tid = threadIdx.x, hh = h * h;
    int kb = 0, ke = 0, node = -1;
    float* orow = nullptr;
    if (ms_rowptr) { node = b; kb = ms_rowptr[b]; ke = ms_rowptr[b + 1]; orow = dS + (int64_t)b * h; }
    else if (b < n_rows) node = b;
    else { kb = b - n_rows; ke = kb + 1; orow = dxe + (int64_t)kb * h; }
    if (node >= 0 && tid < h) {
        const int64_t idx = (int64_t)node * h + tid;
        dM[idx] = masked_cot(cot, cot_scale, fout, idx);
    }
    if (!orow) return;
    const int G = 256 / hp, j = tid & (hp - 1), grp = tid / hp, jj = j < h ? j : h - 1;
    const int rpg = (h + G - 1) / G, i0 = min(h, grp * rpg), i1 = min(h, i0 + rpg);
    float acc = 0.f;
    for (int base = kb; base < ke; base += kVjpRound) {
        const int cnt = min(kVjpRound, ke - base);
        __syncthreads();
        if (tid < cnt) {
            const int k = base + tid, e = (ms_rowptr && ms_eid) ? ms_eid[k] : k;
            es[tid] = e; rs[tid] = erow[e]; vs[tid] = eval ? eval[e] : 1.f;
        }
        __syncthreads();
        for (int idx = tid; idx < cnt * h; idx += 256) {
            const int q = idx / h, c = idx - q * h, row = rs[q];
            const float g = masked_cot(cot, cot_scale, fout, (int64_t)(row >= 0 ? row : 0) * h + c);
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
                for (int u = 0; u < 8; ++u) a[u] = Aj[(int64_t)(i + u) * h];
                s0 = fmaf(a[0], dq[i], s0); s1 = fmaf(a[1], dq[i + 1], s1); s2 = fmaf(a[2], dq[i + 2], s2); s3 = fmaf(a[3], dq[i + 3], s3);
                s0 = fmaf(a[4], dq[i + 4], s0); s1 = fmaf(a[5], dq[i + 5], s1); s2 = fmaf(a[6], dq[i + 6], s2); s3 = fmaf(a[7], dq[i + 7], s3);
            }
            for (; i < i1; ++i) s0 = fmaf(Aj[(int64_t)i * h], dq[i], s0);
            acc += (s0 + s1) + (s2 + s3);
        }
    }
    red[grp * hp + j] = acc;
    __syncthreads();
    if (tid < h) {
        float s = 0.f;
        for (int g = 0; g < G; ++g) s += red[g * hp + tid];
        orow[tid] = s;
    }
}

// block per edge e: dA_e (+)= sum_s w_s (val_e dM_s[tgt_e]) (x) S_s[src_e]
struct OuterTermsW { int n; float w[GODE_MAX_TERMS]; const float* dM[GODE_MAX_TERMS]; const float* X[GODE_MAX_TERMS]; };
__global__ __launch_bounds__(256) void edge_outer_sum_acc_kernel(const int* __restrict__ erow, const float* __restrict__ eval,
                                                                 const int* __restrict__ src, OuterTermsW tm, int h,
                                                                 int accumulate, float* __restrict__ dA) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                    // [n][h]
    float* dm = smem + tm.n * h;         // [n][h], RK weight and edge value folded in
    const int e = blockIdx.x;
    const int row = erow[e], sc = src[e];
    const float vv = eval ? eval[e] : 1.f;
    for (int idx = threadIdx.x; idx < tm.n * h; idx += 256) {
        const int t = idx / h, j = idx - t * h;
        xs[idx] = tm.X[t][(int64_t)sc * h + j];
        const float g = tm.dM[t][(int64_t)(row >= 0 ? row : 0) * h + j];
        dm[idx] = row >= 0 ? tm.w[t] * vv * g : 0.f;
    }
    __syncthreads();
    const int64_t base = (int64_t)e * h * h;
    for (int idx = threadIdx.x; idx < h * h; idx += 256) {
        const int i = idx / h, j = idx - i * h;
        const float old = dA[base + idx];                        // requested before the products; dropped when overwriting
        float v = 0.f;
        for (int t = 0; t < tm.n; ++t) v = fmaf(dm[t * h + i], xs[t * h + j], v);
        dA[base + idx] = accumulate ? old + v : v;
    }
}

extern "C" int gode_edge_ode_supported(int64_t h) { return h >= 1 && h <= kEdgeOdeMaxH ? 1 : 0; }

namespace {
int feval_launch(const int32_t* rowptr, const int32_t* eid, const float* val, const int32_t* src, const float* A,
                 const float* S, int64_t h, int64_t n_rows, const float* bias, const gode_lincomb_t* pre, float alpha,
                 float* out, float* ksave, bool save, void* stream) {
    if (n_rows < 0 || h <= 0) return GODE_E_SHAPE;
    if (h > kEdgeOdeMaxH || n_rows > INT32_MAX) return GODE_E_RANGE;
    int rc = check_lincomb(pre, false); if (rc) return rc;
    if (n_rows == 0) return 0;
    if (!rowptr || !src || !A || !S || !bias || !out || (save && !ksave)) return GODE_E_NULLPTR;
    if (save) {
        if (ksave == out) return GODE_E_SHAPE;
        for (int j = 0; pre && j < pre->n; ++j) if (pre->ptr[j] == ksave) return GODE_E_SHAPE;
    }
    hipStream_t s = (hipStream_t)stream;
    LinComb lp = make_lincomb(pre);
    const size_t lds = (size_t)(h + h * (h + 1)) * sizeof(float);
#define GODE_EF2(PFV, SV) { if (lds > 48 * 1024) { rc = gode_set_lds_once((const void*)edge_ode_feval_kernel<PFV, SV>, lds); if (rc) return rc; } \
        const int slot = gode_prof_begin(s, h, n_rows, (int64_t)lp.n, GODE_PROF_EDGE_FEVAL);                                \
        hipLaunchKernelGGL((edge_ode_feval_kernel<PFV, SV>), dim3((unsigned)n_rows), dim3(256), lds, s, rowptr, eid, val, src, A, S, \
                           (int)h, bias, lp, alpha, out, ksave);                                                             \
        gode_prof_end(s, slot); }
#define GODE_EF(PFV) { if (save) GODE_EF2(PFV, true) else GODE_EF2(PFV, false) }
    if (h <= 32) GODE_EF(4) else if (h <= 64) GODE_EF(16) else GODE_EF(49)
#undef GODE_EF
#undef GODE_EF2
    GODE_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int gode_edge_ode_feval_f32(const int32_t* rowptr, const int32_t* eid, const float* val, const int32_t* src,
                                       const float* A, const float* S, int64_t h, int64_t n_rows, const float* bias,
                                       const gode_lincomb_t* pre, float alpha, float* out, void* stream) {
    return feval_launch(rowptr, eid, val, src, A, S, h, n_rows, bias, pre, alpha, out, nullptr, false, stream);
}

extern "C" int gode_edge_ode_feval_save_f32(const int32_t* rowptr, const int32_t* eid, const float* val, const int32_t* src,
                                            const float* A, const float* S, int64_t h, int64_t n_rows, const float* bias,
                                            const gode_lincomb_t* pre, float alpha, float* out, float* k, void* stream) {
    return feval_launch(rowptr, eid, val, src, A, S, h, n_rows, bias, pre, alpha, out, k, true, stream);
}

extern "C" int gode_edge_ode_vjp_f32(const int32_t* ms_rowptr, const int32_t* ms_eid, const int32_t* edge_row,
                                     const float* edge_val, const float* A, const gode_lincomb_t* cot, float cot_scale,
                                     const float* fout, int64_t h, int64_t n_rows, int64_t n_edges, float* dM, float* dS,
                                     float* dxe, void* stream) {
    if (n_rows < 0 || n_edges < 0 || h <= 0) return GODE_E_SHAPE;
    if (h > kEdgeOdeMaxH || n_rows + n_edges > INT32_MAX) return GODE_E_RANGE;
    int rc = check_lincomb(cot, true); if (rc) return rc;
    if (n_rows == 0) return 0;
    if (!fout || !dM || (ms_rowptr ? !dS : (n_edges > 0 && !dxe))) return GODE_E_NULLPTR;
    if (n_edges > 0 && (!edge_row || !A)) return GODE_E_NULLPTR;
    hipStream_t s = (hipStream_t)stream;
    int hp = 1; while (hp < h) hp <<= 1;
    const int64_t blocks = ms_rowptr ? n_rows : n_rows + n_edges;
    const size_t lds = (size_t)(kVjpRound * h + 256) * sizeof(float);
    const int slot = gode_prof_begin(s, h, blocks, (int64_t)cot->n, GODE_PROF_EDGE_VJP);
    hipLaunchKernelGGL(edge_ode_vjp_kernel, dim3((unsigned)blocks), dim3(256), lds, s, ms_rowptr, ms_eid, edge_row, edge_val, A,
                       make_lincomb(cot), cot_scale, fout, (int)h, hp, (int)n_rows, dM, dS, dxe);
    gode_prof_end(s, slot);
    GODE_LAUNCH_CHECK();
    return 0;
}

extern "C" int gode_edge_outer_sum_acc_f32(const int32_t* edge_row, const float* edge_val, const int32_t* src, int32_t n_terms,
                                           const float* const* dM, const float* const* X, const float* w, int64_t h,
                                           int64_t n_edges, int accumulate, float* dA, void* stream) {
    if (n_edges < 0 || h <= 0) return GODE_E_SHAPE;
    if (n_terms < 1 || n_terms > GODE_MAX_TERMS) return GODE_E_RANGE;
    if (n_edges == 0) return 0;
    if (!edge_row || !src || !dM || !X || !w || !dA) return GODE_E_NULLPTR;
    if (n_edges > INT32_MAX || h > 1024) return GODE_E_RANGE;
    OuterTermsW tm;
    tm.n = n_terms;
    for (int t = 0; t < GODE_MAX_TERMS; ++t) {
        tm.dM[t] = t < n_terms ? dM[t] : nullptr; tm.X[t] = t < n_terms ? X[t] : nullptr; tm.w[t] = t < n_terms ? w[t] : 0.f;
        if (t < n_terms && (!dM[t] || !X[t])) return GODE_E_NULLPTR;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)2 * n_terms * h * sizeof(float);
    if (lds > 48 * 1024) { const int rc = gode_set_lds_once((const void*)edge_outer_sum_acc_kernel, lds); if (rc) return rc; }
    const int slot = gode_prof_begin(s, h, n_edges, (int64_t)n_terms, accumulate ? GODE_PROF_EDGE_OUTER_STEP : GODE_PROF_EDGE_OUTER_STAGE);
    hipLaunchKernelGGL(edge_outer_sum_acc_kernel, dim3((unsigned)n_edges), dim3(256), lds, s, edge_row, edge_val, src, tm, (int)h,
                       accumulate ? 1 : 0, dA);
    gode_prof_end(s, slot);
    GODE_LAUNCH_CHECK();
    return 0;
}
