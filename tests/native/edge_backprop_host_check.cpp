// Stand-alone host check of the entry points of csrc/edge_backprop.hip and gode_edge_ode_feval_save_f32: argument
// validation and marshalling only (every call returns before it reaches a launch), built with the address and
// undefined-behaviour sanitizers and run on the CPU by tests/test_edge_backprop_host_sanitizer.py.
// What the two sources use of the rest of the library is stubbed here; no validation path reaches a stub.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "graphode.h"

int gode_prof_begin(hipStream_t, int64_t, int64_t, int64_t, int) { std::abort(); }
void gode_prof_end(hipStream_t, int) { std::abort(); }
int gode_set_lds_once(const void*, size_t) { std::abort(); }

static int failures = 0;
#define EXPECT(call, code) do { const int rc__ = (call); if (rc__ != (code)) { ++failures; \
    std::printf("line %d: %s returned %d, expected %d\n", __LINE__, #call, rc__, (int)(code)); } } while (0)

static gode_lincomb_t terms(std::vector<std::vector<float>>& pool, int n) {
    gode_lincomb_t lc;
    lc.n = n;
    for (int j = 0; j < GODE_MAX_TERMS; ++j) { lc.coef[j] = 0.f; lc.ptr[j] = nullptr; }
    for (int j = 0; j < n && j < GODE_MAX_TERMS; ++j) { pool.emplace_back(4); lc.coef[j] = 1.f; lc.ptr[j] = pool.back().data(); }
    return lc;
}

int main() {
    std::vector<std::vector<float>> pool;
    pool.reserve(256);
    std::vector<float> f[12];
    for (auto& v : f) v.resize(4);
    std::vector<int32_t> rp(4), er(4), src(4);
    gode_lincomb_t cot = terms(pool, 3), yin = terms(pool, 7), many = terms(pool, 8);
    many.n = 9;
    float *k = f[0].data(), *ga = f[1].data(), *be = f[2].data(), *W = f[3].data(), *A = f[4].data();
    float *dM = f[5].data(), *dS = f[6].data(), *yb = f[7].data(), *gr = f[8].data(), *br = f[9].data(), *S = f[10].data();
#define STAGE(COT, YIN, K, GROUPS, H, N, DM, DS, YB, GR, BR, SS) \
    gode_edge_ode_stage_bwd_f32(rp.data(), nullptr, er.data(), nullptr, A, COT, 0.5f, K, YIN, 0.25f, ga, be, W, GROUPS, 1e-5f, H, N, \
                                30, DM, DS, YB, GR, BR, SS, nullptr)
    EXPECT(STAGE(&cot, &yin, k, 32, 0, 11, dM, dS, yb, gr, br, S), GODE_E_SHAPE);
    EXPECT(STAGE(&cot, &yin, k, 32, 96, -1, dM, dS, yb, gr, br, S), GODE_E_SHAPE);
    EXPECT(STAGE(&cot, &yin, k, 113, 113, 11, dM, dS, yb, gr, br, S), GODE_E_RANGE);
    EXPECT(STAGE(&many, &yin, k, 32, 96, 11, dM, dS, yb, gr, br, S), GODE_E_RANGE);
    EXPECT(STAGE(&cot, &many, k, 32, 96, 11, dM, dS, yb, gr, br, S), GODE_E_RANGE);
    EXPECT(STAGE(nullptr, &yin, k, 32, 96, 11, dM, dS, yb, gr, br, S), GODE_E_NULLPTR);
    EXPECT(STAGE(&cot, &yin, nullptr, 32, 96, 11, dM, dS, yb, gr, br, S), GODE_E_NULLPTR);
    EXPECT(STAGE(&cot, &yin, k, 32, 96, 11, dM, dS, nullptr, gr, br, S), GODE_E_NULLPTR);
    EXPECT(STAGE(&cot, &yin, k, 36, 96, 11, dM, dS, yb, gr, br, S), GODE_E_SHAPE);
    EXPECT(STAGE(&cot, &yin, k, 16, 64, 11, dM, dS, yb, gr, br, S), GODE_E_UNSUPPORTED);
    EXPECT(STAGE(&cot, &yin, k, 32, 96, 0, dM, dS, yb, gr, br, S), 0);
    {   // every output against every term of both combinations and against k
        float* outs[6] = {dM, dS, yb, gr, br, S};
        for (int q = 0; q < 6; ++q) {
            gode_lincomb_t c2 = cot; c2.ptr[2] = outs[q];
            EXPECT(STAGE(&c2, &yin, k, 32, 96, 11, dM, dS, yb, gr, br, S), GODE_E_SHAPE);
            gode_lincomb_t y2 = yin; y2.ptr[6] = outs[q];
            EXPECT(STAGE(&cot, &y2, k, 32, 96, 11, dM, dS, yb, gr, br, S), GODE_E_SHAPE);
            EXPECT(STAGE(&cot, &yin, outs[q], 32, 96, 11, dM, dS, yb, gr, br, S), GODE_E_SHAPE);
        }
        EXPECT(STAGE(&cot, &yin, k, 32, 96, 11, dM, dM, yb, gr, br, S), GODE_E_SHAPE);
        EXPECT(STAGE(&cot, &yin, k, 32, 96, 11, dM, dS, yb, gr, br, br), GODE_E_SHAPE);
    }
    EXPECT(gode_edge_ode_stage_bwd_supported(330, 96, 32), 1);
    EXPECT(gode_edge_ode_stage_bwd_supported(330, 64, 32), 1);
    EXPECT(gode_edge_ode_stage_bwd_supported(11, 7, 7), 1);
    EXPECT(gode_edge_ode_stage_bwd_supported(330, 113, 113), 0);
    EXPECT(gode_edge_ode_stage_bwd_supported(330, 64, 16), 0);

    const float* p8[9]; const float* holes[8]; float ts[9] = {0};
    for (int q = 0; q < 9; ++q) p8[q] = f[q % 4].data();
    for (int q = 0; q < 8; ++q) holes[q] = q == 5 ? nullptr : f[0].data();
    EXPECT(gode_edge_ode_step_close_f32(9, p8, p8, p8, p8, ts, 11, 330, 96, f[11].data(), nullptr), GODE_E_RANGE);
    EXPECT(gode_edge_ode_step_close_f32(0, p8, p8, p8, p8, ts, 11, 330, 96, f[11].data(), nullptr), GODE_E_RANGE);
    EXPECT(gode_edge_ode_step_close_f32(4, p8, p8, p8, p8, ts, 11, 330, 0, f[11].data(), nullptr), GODE_E_SHAPE);
    EXPECT(gode_edge_ode_step_close_f32(4, p8, p8, p8, p8, ts, 11, 330, 113, f[11].data(), nullptr), GODE_E_RANGE);
    EXPECT(gode_edge_ode_step_close_f32(4, p8, p8, p8, p8, ts, 11, 330, 96, nullptr, nullptr), GODE_E_NULLPTR);
    EXPECT(gode_edge_ode_step_close_f32(4, nullptr, p8, p8, p8, ts, 11, 330, 96, f[11].data(), nullptr), GODE_E_NULLPTR);
    EXPECT(gode_edge_ode_step_close_f32(8, p8, holes, p8, p8, ts, 11, 330, 96, f[11].data(), nullptr), GODE_E_NULLPTR);
    EXPECT(gode_edge_ode_step_close_f32(5, p8, holes, p8, p8, ts, 11, 330, 96, nullptr, nullptr), GODE_E_NULLPTR);

    gode_lincomb_t pre = terms(pool, 4);
#define FEVAL(H, N, PRE, OUT, KK) gode_edge_ode_feval_save_f32(rp.data(), nullptr, nullptr, src.data(), A, S, H, N, be, PRE, 0.5f, OUT, KK, nullptr)
    EXPECT(FEVAL(0, 11, &pre, dM, k), GODE_E_SHAPE);
    EXPECT(FEVAL(113, 11, &pre, dM, k), GODE_E_RANGE);
    EXPECT(FEVAL(96, 11, &many, dM, k), GODE_E_RANGE);
    EXPECT(FEVAL(96, 11, &pre, dM, nullptr), GODE_E_NULLPTR);
    EXPECT(FEVAL(96, 11, &pre, dM, dM), GODE_E_SHAPE);
    { gode_lincomb_t p2 = pre; p2.ptr[3] = k; EXPECT(FEVAL(96, 11, &p2, dM, k), GODE_E_SHAPE); }
    EXPECT(FEVAL(96, 0, nullptr, dM, k), 0);
    std::printf(failures ? "FAILED: %d\n" : "host check ok\n", failures);
    return failures ? 1 : 0;
}
