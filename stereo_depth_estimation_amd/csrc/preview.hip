// Per-epoch preview montages of the training CLI (the reference's eval_utils.py:42-73, save_preview_montage):
// for each sample, left | right | gray(target) | gray(pred) as uint8 RGB, each map normalised to its own
// 5th-95th percentile.
//   quantile select : np.percentile(values, q) of the FINITE values of a map (zeros and negatives are members), exact,
//                     on the device: a three-level radix select over full 32-bit keys
//   compose         : the four panels of n samples in one launch
// The select is radix_select.h's, which sd_live_select shares (there: finite positive values, their 31-bit patterns as
// keys, 11 + 11 + 9 bits, 2 % / 98 %, numpy's _lerp). This rule set: every finite value, 32-bit keys through the monotone
// map (negative: all bits flipped, else the sign bit set), 11 + 11 + 10 bits, the two quantiles as arguments, a + d g.
// No allocation, no synchronisation; integer atomics only, so a map's result does not depend on what else is in the
// batch.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "radix_select.h"
#include "stage_util.h"

// every rounding below is the one written: a * b + c stays two roundings
#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------ exact order statistics
// radix_select.h's three-level select under this rule set: every finite value counts; 32-bit keys through the monotone
// map, 11 + 11 + 10 bits.
struct PreviewSelect {
    static constexpr int LAST_BITS = 10;
    __device__ __forceinline__ static bool member(float v) { return finite_f(v); }
    // order-preserving key of a float: -x < -0.0 < +0.0 < x as unsigned integers
    __device__ __forceinline__ static unsigned key(float x) {
        const unsigned b = __float_as_uint(x);
        return (b & 0x80000000u) ? ~b : b | 0x80000000u;
    }
    __device__ __forceinline__ static float value(unsigned key) {
        return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
    }
    // the percentile from the two order statistics around (n - 1) * q: v[k] + (v[k + 1] - v[k]) * g in fp64, rounded
    // to float32 once
    __device__ __forceinline__ static float lerp(float a, float b, double pos) {
        const double g = pos - floor(pos);
        const double d = (double)b - (double)a;
        const double t = d * g;
        return (float)((double)a + t);
    }
};

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
        uint32_t c[V];  // r | g << 8 | b << 16
        if (panel < 2) {
            float ch[3][V];
#pragma unroll
            for (int k = 0; k < 3; ++k) ld_f<V>(inp + (size_t)(panel * 3 + k) * P + px, ch[k]);
#pragma unroll
            for (int i = 0; i < V; ++i)
                c[i] = (uint32_t)colour_of(ch[0][i]) | (uint32_t)colour_of(ch[1][i]) << 8 |
                       (uint32_t)colour_of(ch[2][i]) << 16;
        } else {
            const int j = panel - 2;
            float m[V];
            ld_f<V>(maps[j] + px, m);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const uint32_t g = any[j] ? gray_of(m[i], vmin[j], scale[j]) : 0u;
                c[i] = g | g << 8 | g << 16;
            }
        }
        st_rgb<V>(out + ((size_t)y * 4 * W + (size_t)panel * W + x) * 3, c);
    }
}

// ------------------------------------------------------------------ host side
bool maps_ok(int m) { return m >= 1 && m <= 64; }

}  // namespace

extern "C" long long sd_quantile_select_ws_bytes(int m) {
    return maps_ok(m) ? (long long)m * SelectLayout<PreviewSelect>::WORDS * 4 : -1;
}

extern "C" int sd_quantile_select_n(int m, const float* values, int count, double q_lo, double q_hi, unsigned* work,
                                    float* sel, sd_stream s) {
    const char* fn = "sd_quantile_select_n";
    SD_REQUIRE(maps_ok(m), "%s: m = %d maps (1..64)", fn, m);
    SD_REQUIRE(values && work && sel, "%s: null pointer (values, work, sel)", fn);
    SD_REQUIRE(count > 0, "%s: count %d", fn, count);
    SD_REQUIRE(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0, "%s: quantiles %g, %g (0 <= q_lo <= q_hi <= 1)", fn, q_lo, q_hi);
    select_launch<PreviewSelect>(m, values, count, q_lo, q_hi, work, sel, 0, to_stream(s));
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
    hipLaunchKernelGGL(vec ? k_preview_compose<4> : k_preview_compose<1>, dim3(grid_for(items, 2048), n), dim3(256), 0,
                       to_stream(s), input, target, pred, H, W, sel_t, sel_p, montage);
    return sd_check_launch(fn);
}
