// Per-epoch preview montages of the training CLI (the reference's eval_utils.py:42-73, save_preview_montage):
// for each sample, left | right | gray(target) | gray(pred) as uint8 RGB, each map normalised to its own
// 5th-95th percentile.
//   quantile select : np.percentile(values, q) of the FINITE values of a map (zeros and negatives are members), exact,
//                     on the device: a three-level radix select over full 32-bit keys
//   compose         : the four panels of n samples in one launch
// The select is the scheme of live.hip's sd_live_select (11 + 11 + 9 bits over the 31-bit patterns of finite positive
// floats, fixed 2 % / 98 %) restated for this rule: every finite value, 32-bit keys through the monotone map (negative:
// all bits flipped, else the sign bit set), 11 + 11 + 10 bits, and the two quantiles as arguments. live.hip is untouched.
// No allocation, no synchronisation; integer atomics only, so a map's result does not depend on what else is in the
// batch.
#include <limits.h>
#include <math.h>

#include "common.h"

// every rounding below is the one written: a * b + c stays two roundings
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }  // false for NaN

// order-preserving key of a float: -x < -0.0 < +0.0 < x as unsigned integers
__device__ __forceinline__ unsigned key_of(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float value_of(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

// ------------------------------------------------------------------ exact order statistics
// Level 1 histograms the top 11 key bits of every finite value; a one-block scan finds, for each of the four wanted
// ranks, the bin that holds it and the rank within the bin; level 2 histograms the next 11 bits of the values in those
// bins, level 3 the last 10. Targets that share a prefix share a histogram. Histograms are built in LDS per block and
// added to the global ones (non-zero bins only); counts are 32-bit. The last scan writes the result row and zeroes the
// map's work buffer again.
constexpr int QS_H1 = 0, QS_H2 = 2048, QS_H3 = QS_H2 + 4 * 2048, QS_STATE = QS_H3 + 4 * 1024;
constexpr int QS_WORDS = QS_STATE + 16;  // state: n, prefix[4], rank[4]

template <int LEVEL> struct QsLevel {
    static constexpr int BINS = LEVEL == 3 ? 1024 : 2048, BITS = LEVEL == 3 ? 10 : 11, NH = LEVEL == 1 ? 1 : 4;
    static constexpr int BASE = LEVEL == 1 ? QS_H1 : LEVEL == 2 ? QS_H2 : QS_H3;
};

// grid (blocks, m): work [m][QS_WORDS]
template <int LEVEL>
__global__ __launch_bounds__(256) void k_qs_hist(const float* __restrict__ values, int P, unsigned* __restrict__ work_all) {
    using Lv = QsLevel<LEVEL>;
    constexpr int BINS = Lv::BINS, NH = Lv::NH;
    const float* __restrict__ v = values + (size_t)blockIdx.y * P;
    unsigned* __restrict__ work = work_all + (size_t)blockIdx.y * QS_WORDS;
    __shared__ unsigned h[NH * BINS];
    for (int i = threadIdx.x; i < NH * BINS; i += 256) h[i] = 0u;
    unsigned pf[4] = {0u, 0u, 0u, 0u};
    bool own[4] = {true, false, false, false};
    if (LEVEL > 1) {
        if (work[QS_STATE] == 0u) return;  // no finite value (uniform over the map's blocks)
#pragma unroll
        for (int j = 0; j < 4; ++j) pf[j] = work[QS_STATE + 1 + j];
#pragma unroll
        for (int j = 1; j < 4; ++j) own[j] = pf[j] != pf[j - 1];
    }
    __syncthreads();
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += stride) {
        const float x = v[i];
        if (!finite_f(x)) continue;
        const unsigned key = key_of(x);
        if (LEVEL == 1) {
            atomicAdd(&h[key >> 21], 1u);
        } else {
            const unsigned hi = LEVEL == 2 ? key >> 21 : key >> 10;
            const unsigned lo = LEVEL == 2 ? (key >> 10) & 2047u : key & 1023u;
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

// the percentile from the two order statistics around (n - 1) * q: v[k] + (v[k + 1] - v[k]) * g in fp64, rounded to
// float32 once
__device__ __forceinline__ float lerp_q(float a, float b, double pos) {
    const double g = pos - floor(pos);
    const double d = (double)b - (double)a;
    const double t = d * g;
    return (float)((double)a + t);
}

// one block per map: sel [m][8]
template <int LEVEL>
__global__ __launch_bounds__(256) void k_qs_scan(unsigned* __restrict__ work_all, float* __restrict__ sel_all, double q_lo,
                                                 double q_hi) {
    using Lv = QsLevel<LEVEL>;
    constexpr int BINS = Lv::BINS, PER = BINS / 256, BITS = Lv::BITS;
    unsigned* __restrict__ work = work_all + (size_t)blockIdx.x * QS_WORDS;
    float* __restrict__ sel = sel_all + (size_t)blockIdx.x * 8;
    unsigned* st = work + QS_STATE;
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
        hist[j] = work + Lv::BASE + (LEVEL == 1 ? 0 : src * BINS);
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
            const unsigned klo = (unsigned)floor((double)(n - 1u) * q_lo), khi = (unsigned)floor((double)(n - 1u) * q_hi);
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
        for (int i = t; i < QS_WORDS; i += 256) work[i] = 0u;
        if (t == 0) {
            reinterpret_cast<unsigned*>(sel)[0] = n;
            if (n == 0u) {
                for (int j = 1; j < 7; ++j) sel[j] = NAN;
            } else {
                const float a0 = value_of(s_out[0]), a1 = value_of(s_out[1]);
                const float b0 = value_of(s_out[2]), b1 = value_of(s_out[3]);
                sel[1] = a0;
                sel[2] = a1;
                sel[3] = b0;
                sel[4] = b1;
                sel[5] = lerp_q(a0, a1, (double)(n - 1u) * q_lo);
                sel[6] = lerp_q(b0, b1, (double)(n - 1u) * q_hi);
            }
        }
    }
}

// ------------------------------------------------------------------ montage
// colour code of an input value: trunc(clip(float32(x * 255), 0, 255)); NaN -> 0 (fmaxf returns the other operand)
__device__ __forceinline__ uint8_t colour_of(float x) {
    const float v = fminf(fmaxf(x * 255.f, 0.f), 255.f);
    return (uint8_t)(int)v;
}
// gray code of a map value (_normalize_map): trunc(float32(clip((m - vmin) / scale, 0, 1) * 255)); NaN -> 0
__device__ __forceinline__ uint8_t gray_of(float m, float vmin, float scale) {
    const float d = m - vmin;
    const float x = fminf(fmaxf(d / scale, 0.f), 1.f);
    return (uint8_t)(int)(x * 255.f);
}

template <int V> __device__ __forceinline__ void ld_f(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}
// V RGB pixels (3 V bytes): three 4-B stores for V = 4
template <int V> __device__ __forceinline__ void st_rgb(uint8_t* p, const uint8_t (&c)[3 * V]) {
    if constexpr (V == 4) {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = (uint32_t)c[4 * k] | (uint32_t)c[4 * k + 1] << 8 | (uint32_t)c[4 * k + 2] << 16 |
                   (uint32_t)c[4 * k + 3] << 24;
    } else {
        p[0] = c[0];
        p[1] = c[1];
        p[2] = c[2];
    }
}

// grid (blocks, n). One work item = V consecutive pixels of one panel row: item -> (y, panel, x). V = 4 needs W % 4 == 0
// and aligned pointers (then every plane row, sample slice and 12-B output group keeps the alignment).
template <int V>
__global__ __launch_bounds__(256) void k_preview_compose(const float* __restrict__ input, const float* __restrict__ target,
                                                         const float* __restrict__ pred, int H, int W,
                                                         const float* __restrict__ sel_t, const float* __restrict__ sel_p,
                                                         uint8_t* __restrict__ montage) {
    const size_t P = (size_t)H * W;
    const int smp = blockIdx.y;
    const float* __restrict__ inp = input + (size_t)smp * 6 * P;
    const float* __restrict__ maps[2] = {target + (size_t)smp * P, pred + (size_t)smp * P};
    const float* __restrict__ sels[2] = {sel_t + (size_t)smp * 8, sel_p + (size_t)smp * 8};
    uint8_t* __restrict__ out = montage + (size_t)smp * P * 12;
    float vmin[2], scale[2];
    bool any[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        any[j] = reinterpret_cast<const unsigned*>(sels[j])[0] != 0u;
        vmin[j] = any[j] ? sels[j][5] : 0.f;
        scale[j] = any[j] ? (float)fmax((double)sels[j][6] - (double)sels[j][5], 1e-6) : 1.f;
    }
    const int WV = W / V;
    const long long items = (long long)H * 4 * WV, stride = (long long)gridDim.x * 256;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += stride) {
        const int y = (int)(it / (4 * WV));
        const int r = (int)(it - (long long)y * 4 * WV);
        const int panel = r / WV, x = (r - panel * WV) * V;
        const size_t px = (size_t)y * W + x;
        uint8_t c[3 * V];
        if (panel < 2) {
            float ch[3][V];
#pragma unroll
            for (int k = 0; k < 3; ++k) ld_f<V>(inp + (size_t)(panel * 3 + k) * P + px, ch[k]);
#pragma unroll
            for (int i = 0; i < V; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) c[3 * i + k] = colour_of(ch[k][i]);
        } else {
            const int j = panel - 2;
            float m[V];
            ld_f<V>(maps[j] + px, m);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const uint8_t g = any[j] ? gray_of(m[i], vmin[j], scale[j]) : (uint8_t)0;
                c[3 * i] = c[3 * i + 1] = c[3 * i + 2] = g;
            }
        }
        st_rgb<V>(out + ((size_t)y * 4 * W + (size_t)panel * W + x) * 3, c);
    }
}

// ------------------------------------------------------------------ host side
bool aligned(const void* p, unsigned a) { return ((uintptr_t)p % a) == 0; }
bool maps_ok(int m) { return m >= 1 && m <= 64; }
int grid_for(long long work) {
    long long g = (work + 255) / 256;
    if (g > 2048) g = 2048;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" long long sd_quantile_select_ws_bytes(int m) { return maps_ok(m) ? (long long)m * QS_WORDS * 4 : -1; }

extern "C" int sd_quantile_select_n(int m, const float* values, int count, double q_lo, double q_hi, unsigned* work,
                                    float* sel, sd_stream s) {
    const char* fn = "sd_quantile_select_n";
    SD_REQUIRE(maps_ok(m), "%s: m = %d maps (1..64)", fn, m);
    SD_REQUIRE(values && work && sel, "%s: null pointer (values, work, sel)", fn);
    SD_REQUIRE(count > 0, "%s: count %d", fn, count);
    SD_REQUIRE(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0, "%s: quantiles %g, %g (0 <= q_lo <= q_hi <= 1)", fn, q_lo, q_hi);
    const int blocks = cdiv(count, 1024) < 256 ? cdiv(count, 1024) : 256;
    const dim3 g(blocks, m), g1(m), b(256);
    hipStream_t st = to_stream(s);
    hipLaunchKernelGGL(k_qs_hist<1>, g, b, 0, st, values, count, work);
    hipLaunchKernelGGL(k_qs_scan<1>, g1, b, 0, st, work, sel, q_lo, q_hi);
    hipLaunchKernelGGL(k_qs_hist<2>, g, b, 0, st, values, count, work);
    hipLaunchKernelGGL(k_qs_scan<2>, g1, b, 0, st, work, sel, q_lo, q_hi);
    hipLaunchKernelGGL(k_qs_hist<3>, g, b, 0, st, values, count, work);
    hipLaunchKernelGGL(k_qs_scan<3>, g1, b, 0, st, work, sel, q_lo, q_hi);
    return sd_check_launch(fn);
}

extern "C" int sd_preview_compose_n(int n, const float* input, const float* target, const float* pred, int H, int W,
                                    const float* sel_t, const float* sel_p, uint8_t* montage, sd_stream s) {
    const char* fn = "sd_preview_compose_n";
    SD_REQUIRE(maps_ok(n), "%s: n = %d samples (1..64)", fn, n);
    SD_REQUIRE(input && target && pred, "%s: null pointer (input, target, pred)", fn);
    SD_REQUIRE(sel_t && sel_p && montage, "%s: null pointer (sel_t, sel_p, montage)", fn);
    SD_REQUIRE(H > 0 && W > 0 && (long long)H * W <= INT_MAX / 16, "%s: bad sizes %dx%d", fn, H, W);
    const bool vec = W % 4 == 0 && aligned(input, 16) && aligned(target, 16) && aligned(pred, 16) && aligned(montage, 4);
    const long long items = (long long)H * 4 * (W / (vec ? 4 : 1));
    hipLaunchKernelGGL(vec ? k_preview_compose<4> : k_preview_compose<1>, dim3(grid_for(items), n), dim3(256), 0,
                       to_stream(s), input, target, pred, H, W, sel_t, sel_p, montage);
    return sd_check_launch(fn);
}
