// Exact order statistics of the members of a float map, on the device: one three-level radix select, shared by the live
// loop's auto range (live.hip, sd_live_select_n) and the preview montages' percentiles (preview.hip,
// sd_quantile_select_n). Each caller states its rule set as a struct R:
//   static bool     member(float)    which values count
//   static unsigned key(float)       order-preserving key of a member, 22 + LAST_BITS bits wide
//   static float    value(unsigned)  its inverse
//   static constexpr int LAST_BITS   width of the last level (the first two are 11 bits each)
//   static float    lerp(float a, float b, double pos)   the quantile from the two order statistics around pos
// Level 1 histograms the top 11 key bits of every member; a one-block scan finds, for each of the four wanted ranks
// (floor((n - 1) q) and the one after it, for q_lo and q_hi), the bin that holds it and the rank within the bin;
// level 2 histograms the next 11 bits of the members in those bins, level 3 the last LAST_BITS. Targets that share a
// prefix share a histogram. Histograms are built in LDS per block and added to the global ones (non-zero bins only);
// counts are 32-bit. The last scan writes the result row sel[8] = {n (as uint32), the four order statistics, the two
// quantiles, unused} and zeroes the map's work buffer again. Integer atomics only: a map's result does not depend on
// what else is in the launch. blockIdx.y (histograms) / blockIdx.x (scans) is the map; a map whose bit is set in `hold`
// is left alone.
#pragma once
#include <math.h>

#include "common.h"

namespace {

// work buffer of one map, in 32-bit words; state: n, prefix[4], rank[4]
template <typename R> struct SelectLayout {
    static constexpr int H1 = 0, H2 = 2048, H3 = H2 + 4 * 2048, STATE = H3 + 4 * (1 << R::LAST_BITS);
    static constexpr int WORDS = STATE + 16;
};
template <typename R, int LEVEL> struct SelectLevel {
    static constexpr int BITS = LEVEL == 3 ? R::LAST_BITS : 11, BINS = 1 << BITS, NH = LEVEL == 1 ? 1 : 4;
    using Lay = SelectLayout<R>;
    static constexpr int BASE = LEVEL == 1 ? Lay::H1 : LEVEL == 2 ? Lay::H2 : Lay::H3;
};

// grid (blocks, m): values [m][P], work [m][WORDS]
template <typename R, int LEVEL>
__global__ __launch_bounds__(256) void k_select_hist(const float* __restrict__ values, int P,
                                                     unsigned* __restrict__ work_all, unsigned long long hold) {
    using Lv = SelectLevel<R, LEVEL>;
    constexpr int BINS = Lv::BINS, NH = Lv::NH, LAST = R::LAST_BITS, STATE = SelectLayout<R>::STATE;
    if ((hold >> blockIdx.y) & 1ull) return;
    const float* __restrict__ v = values + (size_t)blockIdx.y * P;
    unsigned* __restrict__ work = work_all + (size_t)blockIdx.y * SelectLayout<R>::WORDS;
    __shared__ unsigned h[NH * BINS];
    for (int i = threadIdx.x; i < NH * BINS; i += 256) h[i] = 0u;
    unsigned pf[4] = {0u, 0u, 0u, 0u};
    bool own[4] = {true, false, false, false};
    if (LEVEL > 1) {
        if (work[STATE] == 0u) return;  // no member (uniform over the map's blocks)
#pragma unroll
        for (int j = 0; j < 4; ++j) pf[j] = work[STATE + 1 + j];
#pragma unroll
        for (int j = 1; j < 4; ++j) own[j] = pf[j] != pf[j - 1];
    }
    __syncthreads();
    // P < 2^31 and select_launch's grid is 256 blocks at most: the 32-bit unsigned index cannot wrap
    const unsigned stride = gridDim.x * 256u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)P; i += stride) {
        const float x = v[i];
        if (!R::member(x)) continue;
        const unsigned key = R::key(x);
        if (LEVEL == 1) {
            atomicAdd(&h[key >> (11 + LAST)], 1u);
        } else {
            const unsigned hi = LEVEL == 2 ? key >> (11 + LAST) : key >> LAST;
            const unsigned lo = LEVEL == 2 ? (key >> LAST) & 2047u : key & ((1u << LAST) - 1u);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (own[j] && hi == pf[j]) atomicAdd(&h[j * BINS + lo], 1u);
        }
    }
    __syncthreads();
    unsigned* g = work + Lv::BASE;
    for (int i = threadIdx.x; i < NH * BINS; i += 256)
        if (h[i]) atomicAdd(g + i, h[i]);
}

// The scan of one map: its work buffer and its sel[8]. A function of its own with __restrict__ parameters, not the
// kernel's body: the compiler then knows that `work` and `sel` do not overlap and keeps the loads of the four
// histograms in flight together (measured: 1.3 us of 15.5 us in the level-3 scan without it).
template <typename R, int LEVEL>
__device__ __forceinline__ void select_scan_body(unsigned* __restrict__ work, float* __restrict__ sel, double q_lo,
                                                 double q_hi) {
#pragma clang fp contract(off)  // (n - 1) * q is one fp64 multiply
    using Lv = SelectLevel<R, LEVEL>;
    constexpr int BINS = Lv::BINS, PER = BINS / 256, BITS = Lv::BITS, WORDS = SelectLayout<R>::WORDS;
    unsigned* st = work + SelectLayout<R>::STATE;
    __shared__ unsigned part[4][256];
    __shared__ unsigned s_pf[4], s_rk[4], s_out[4], s_n;
    const int t = threadIdx.x;
    if (t < 4) {
        s_pf[t] = LEVEL == 1 ? 0u : st[1 + t];
        s_rk[t] = LEVEL == 1 ? 0u : st[5 + t];
    }
    if (t == 0) s_n = LEVEL == 1 ? 0u : st[0];
    __syncthreads();
    const unsigned* hist[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int src = j;
        if (LEVEL > 1)
            while (src > 0 && s_pf[src] == s_pf[src - 1]) --src;
        hist[j] = LEVEL == 1 ? work + Lv::BASE : work + Lv::BASE + src * BINS;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned sum = 0u;
        for (int i = 0; i < PER; ++i) sum += hist[j][t * PER + i];
        part[j][t] = sum;
    }
    __syncthreads();
    if (LEVEL == 1 && t == 0) {
        unsigned n = 0u;
        for (int c = 0; c < 256; ++c) n += part[0][c];
        s_n = n;
        if (n > 0u) {
            const unsigned klo = (unsigned)floor((double)(n - 1u) * q_lo);
            const unsigned khi = (unsigned)floor((double)(n - 1u) * q_hi);
            s_rk[0] = min(klo, n - 1u);
            s_rk[1] = min(klo + 1u, n - 1u);
            s_rk[2] = min(khi, n - 1u);
            s_rk[3] = min(khi + 1u, n - 1u);
        }
    }
    __syncthreads();
    const unsigned n = s_n;
    if (t < 4 && n > 0u) {
        const unsigned r = s_rk[t];
        unsigned cum = 0u;
        int c = 0;
        while (c < 255 && cum + part[t][c] <= r) cum += part[t][c++];
        int b = c * PER;
        while (b < c * PER + PER - 1 && cum + hist[t][b] <= r) cum += hist[t][b++];
        s_out[t] = (s_pf[t] << BITS) | (unsigned)b;
        st[1 + t] = s_out[t];
        st[5 + t] = r - cum;
    }
    if (t == 0) st[0] = n;
    if (LEVEL == 3) {
        __syncthreads();  // the histograms were read: zero the whole work buffer for the next call
        for (int i = t; i < WORDS; i += 256) work[i] = 0u;
        if (t == 0) {
            reinterpret_cast<unsigned*>(sel)[0] = n;
            if (n == 0u) {
                for (int j = 1; j < 7; ++j) sel[j] = NAN;
            } else {
                const float a0 = R::value(s_out[0]), a1 = R::value(s_out[1]);
                const float b0 = R::value(s_out[2]), b1 = R::value(s_out[3]);
                sel[1] = a0;
                sel[2] = a1;
                sel[3] = b0;
                sel[4] = b1;
                sel[5] = R::lerp(a0, a1, (double)(n - 1u) * q_lo);
                sel[6] = R::lerp(b0, b1, (double)(n - 1u) * q_hi);
            }
        }
    }
}
// one block per map: work [m][WORDS], sel [m][8]
template <typename R, int LEVEL>
__global__ __launch_bounds__(256) void k_select_scan(unsigned* __restrict__ work, float* __restrict__ sel, double q_lo,
                                                     double q_hi, unsigned long long hold) {
    if ((hold >> blockIdx.x) & 1ull) return;
    select_scan_body<R, LEVEL>(work + (size_t)blockIdx.x * SelectLayout<R>::WORDS, sel + (size_t)blockIdx.x * 8, q_lo,
                               q_hi);
}

// the six launches over m maps of P > 0 values each (the callers check their sizes)
template <typename R>
void select_launch(int m, const float* values, int P, double q_lo, double q_hi, unsigned* work, float* sel,
                   unsigned long long hold, hipStream_t st) {
    const dim3 g(cdiv(P, 1024) < 256 ? cdiv(P, 1024) : 256, m), g1(m), b(256);
    hipLaunchKernelGGL((k_select_hist<R, 1>), g, b, 0, st, values, P, work, hold);
    hipLaunchKernelGGL((k_select_scan<R, 1>), g1, b, 0, st, work, sel, q_lo, q_hi, hold);
    hipLaunchKernelGGL((k_select_hist<R, 2>), g, b, 0, st, values, P, work, hold);
    hipLaunchKernelGGL((k_select_scan<R, 2>), g1, b, 0, st, work, sel, q_lo, q_hi, hold);
    hipLaunchKernelGGL((k_select_hist<R, 3>), g, b, 0, st, values, P, work, hold);
    hipLaunchKernelGGL((k_select_scan<R, 3>), g1, b, 0, st, work, sel, q_lo, q_hi, hold);
}

}  // namespace
