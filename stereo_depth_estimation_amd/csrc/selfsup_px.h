// The per-pixel arithmetic the two label-free loss stages share (selfsup.hip: sd_selfsup_loss; selfsup_ssim.hip:
// sd_selfsup_loss_ssim), so that there is one statement of each: the normaliser launch, the warp, the Charbonnier error
// and its slope, and a smoothness pair. INTEGRATION.md "sd_selfsup_loss" is the normative text. Every function states
// its contraction setting in its own body: float32, every operation rounded on its own.
#pragma once
#include <math.h>

#include "common.h"
#include "stage_util.h"

namespace {

constexpr int SS_ROW = row_walk::ROW;
constexpr int SS_HEAD = 8;  // doubles ahead of the partial rows in `work`: [0] the normaliser N
constexpr int SS_CNT_THREADS = 256;

// One smoothness pair (p, q): its term and s; false (and both 0) when a disparity is not finite.
__device__ __forceinline__ bool ss_pair(float dp, float dq, float lp0, float lp1, float lp2, float lq0, float lq1,
                                        float lq2, float gamma, float eps_s2, float& term, float& s) {
#pragma clang fp contract(off)
    term = 0.f, s = 0.f;
    if (!(finite_f(dp) && finite_f(dq))) return false;
    const float t = dq - dp;
    const float g = __fdiv_rn((fabsf(lq0 - lp0) + fabsf(lq1 - lp1)) + fabsf(lq2 - lp2), 3.0f);
    const float w = expf(-(gamma * g));
    const float r = __fsqrt_rn(t * t + eps_s2);
    term = w * r;
    s = __fdiv_rn(w * t, r);
    return true;
}

// The warp of pixel x with disparity d: r_c and b_c - a_c per channel from the right frame's row (rrow = R_0's row, the
// channels `plane` floats apart). The only data-dependent loads of either stage.
__device__ __forceinline__ void ss_warp(const float* __restrict__ rrow, size_t plane, unsigned x, unsigned W, float d,
                                        float (&r)[3], float (&dba)[3]) {
#pragma clang fp contract(off)
    const float xr = (float)x - d;
    const int xf = (int)floorf(xr);
    const unsigned x0 = (unsigned)min(max(xf, 0), (int)W - 1), x1 = min(x0 + 1u, W - 1u);
    const float f = xr - (float)x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* rp = rrow + c * plane;
        const float ra = rp[x0], rb = rp[x1];
        dba[c] = rb - ra;
        r[c] = ra + f * dba[c];
    }
}

// The Charbonnier error e of a warped pixel and its slope de/dd.
__device__ __forceinline__ void ss_charbonnier(float l0, float l1, float l2, const float (&r)[3], const float (&dba)[3],
                                               float eps2, float& e, float& de) {
#pragma clang fp contract(off)
    const float l[3] = {l0, l1, l2};
    float phi[3], q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = l[c] - r[c];
        phi[c] = __fsqrt_rn(t * t + eps2);
        q[c] = __fdiv_rn(t, phi[c]) * dba[c];
    }
    e = __fdiv_rn((phi[0] + phi[1]) + phi[2], 3.0f);
    de = __fdiv_rn((q[0] + q[1]) + q[2], 3.0f);
}

// N = max(1, sum_i (rows[i][0] - rows[i][1] - rows[i][2] - rows[i][6])) over the check stage's rows: exact integers in
// fp64 below 2^53, so the strided chains and the tree give the sum in index order. count = that sum as int32
// (saturated), 0 when nothing is counted.
__global__ __launch_bounds__(SS_CNT_THREADS) void k_selfsup_count(const double* __restrict__ check_rows, int n,
                                                                  double* __restrict__ nrm, int* __restrict__ count) {
    double t = 0.0;
    for (int i = threadIdx.x; i < n; i += SS_CNT_THREADS) {
        const double* r = check_rows + (size_t)i * SS_ROW;
        t += ((r[0] - r[1]) - r[2]) - r[6];
    }
    double z = 0.0;
    block_sum2<SS_CNT_THREADS>(t, z);
    if (threadIdx.x == 0) {
        nrm[0] = t < 1.0 ? 1.0 : t;
        count[0] = t < 1.0 ? 0 : (t > 2147483647.0 ? 2147483647 : (int)t);
    }
}

}  // namespace
