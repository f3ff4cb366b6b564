// backprop.hip — the masked cotangent of a backward sweep through a saved rk4 solve (gfx950).
//
// Backprop through odeint (odeint._OdeintBackprop) needs, per RK stage s, dZ_s = kbar_s * [z_s > 0] where the stage
// cotangent kbar_s is a linear combination of dL/dy_{n+1} and the VJPs of the later stages of the step, and the mask of
// f = relu(z) is exactly [k_s > 0] of the saved stage derivative.  The bias gradient of the stage is colsum(dZ_s): the
// kernel leaves one column-sum row per block (the caller reduces gridDim.x rows with gode_colsum_f32 instead of reading
// the n x d array again).
//
// Pure streaming: every thread handles 16 bytes of a row per pass (d / 4 lanes per row, 256 / (d / 4) rows per pass of a
// block, kMcPasses passes), so a pass of a block reads and writes 4 KB contiguous per term.  No data is reused across
// blocks, so the grid needs no XCD-aware ordering.  Bound: HBM, (terms + 2) * n * d * 4 bytes.
#include "common.h"

namespace {

constexpr int kMcPasses = 16;

template <int T>
__global__ __launch_bounds__(256) void masked_cot_kernel(LinComb cot, const float* __restrict__ k, float* __restrict__ dZ,
                                                         int64_t n_rows, float* __restrict__ colpart)
{
    constexpr int R = 256 / T, D = 4 * T;
    const int lane = threadIdx.x % T, r = threadIdx.x / T;
    const int64_t row0 = (int64_t)blockIdx.x * (R * kMcPasses) + r;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int p = 0; p < kMcPasses; ++p) {
        const int64_t row = row0 + (int64_t)p * R;
        if (row < n_rows) {
            const int64_t o = row * D + 4 * lane;
            float4 g = lc_load4(cot, o);
            const float4 kk = *reinterpret_cast<const float4*>(k + o);
            g.x = kk.x > 0.f ? g.x : 0.f; g.y = kk.y > 0.f ? g.y : 0.f;
            g.z = kk.z > 0.f ? g.z : 0.f; g.w = kk.w > 0.f ? g.w : 0.f;
            *reinterpret_cast<float4*>(dZ + o) = g;
            acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
        }
    }
    if (!colpart) return;                                    // uniform over the grid
    __shared__ float4 cs[256];
    cs[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < T) {                                   // rows of the block added in a fixed order: deterministic
        float4 t = cs[threadIdx.x];
#pragma unroll
        for (int q = 1; q < R; ++q) {
            const float4 a = cs[q * T + threadIdx.x];
            t.x += a.x; t.y += a.y; t.z += a.z; t.w += a.w;
        }
        *reinterpret_cast<float4*>(colpart + (int64_t)blockIdx.x * D + 4 * threadIdx.x) = t;
    }
}

// any width / alignment: one element per thread, no column sums
__global__ __launch_bounds__(256) void masked_cot_generic_kernel(LinComb cot, const float* __restrict__ k,
                                                                 float* __restrict__ dZ, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = lc_load1(cot, i);
    dZ[i] = k[i] > 0.f ? g : 0.f;
}

int64_t lanes_per_row(int64_t d) {
    if (d <= 0 || d % 4) return 0;
    const int64_t t = d / 4;
    return (t <= 64 && !(t & (t - 1))) ? t : 0;
}

}  // namespace

extern "C" int64_t gode_masked_cot_parts(int64_t n_rows, int64_t d)
{
    const int64_t t = lanes_per_row(d);
    if (n_rows <= 0 || t == 0) return 0;
    const int64_t rows = (256 / t) * kMcPasses;
    return (n_rows + rows - 1) / rows;
}

extern "C" int gode_masked_cot_f32(const gode_lincomb_t* cot, const float* k, float* dZ, int64_t n_rows, int64_t d,
                                   float* colpart, void* stream)
{
    if (n_rows < 0 || d <= 0) return GODE_E_SHAPE;
    if (!cot || !k || !dZ) return GODE_E_NULLPTR;
    int rc = check_lincomb(cot, true); if (rc) return rc;
    if (n_rows == 0) return 0;
    if (n_rows * d >= ((int64_t)1 << 38)) return GODE_E_RANGE;
    for (int j = 0; j < cot->n; ++j) if (cot->ptr[j] == dZ) return GODE_E_SHAPE;      // rows are read and written by one thread
    const LinComb lc = make_lincomb(cot);
    const int64_t t = lanes_per_row(d);
    const bool al = lincomb_aligned16(cot) && !((((uintptr_t)k) | ((uintptr_t)dZ) | ((uintptr_t)colpart)) & 15);
    if (t > 0 && al) {
        const int64_t blocks = gode_masked_cot_parts(n_rows, d);
        if (blocks > INT32_MAX) return GODE_E_RANGE;
        switch (t) {
#define GODE_MC(T) case T: hipLaunchKernelGGL(masked_cot_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, \
                                              lc, k, dZ, n_rows, colpart); break;
            GODE_MC(1) GODE_MC(2) GODE_MC(4) GODE_MC(8) GODE_MC(16) GODE_MC(32) GODE_MC(64)
#undef GODE_MC
            default: return GODE_E_UNSUPPORTED;
        }
        GODE_LAUNCH_CHECK();
        return 0;
    }
    if (colpart) return GODE_E_UNSUPPORTED;                 // column-sum rows only on the 16-byte kernel
    const int64_t n = n_rows * d;
    hipLaunchKernelGGL(masked_cot_generic_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       lc, k, dZ, n);
    GODE_LAUNCH_CHECK();
    return 0;
}
