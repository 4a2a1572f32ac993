// On-device frame path of the live depth loop (the reference's live_camera/depth_live_dl.py around model(x)):
// raw uint8 BGR camera frames in, display-ready uint8 images and three scalars out.
//   front end : cv2.remap + cvtColor + cv2.resize + /255 + cat + upload + the engine's input pack (:476-493,225-229,516-520)
//   post      : EMA, disparity_to_depth, confidence_from_logvar, colour codes, depth_contour_mask (:531-540,371-381,254-275,232-251)
//   select    : np.percentile(values, 2 / 98) of the auto range (:242-244), exact, without a host round trip
//   centre    : the centre-window medians (:542-595)
//   compose   : applyColorMap + cv2.resize back to the view + the contour overlay (:568-574,601-617)
// Byte and fp32 streaming kernels, grid-stride (as data.hip): one pixel per thread in the gathering kernels (the front
// end stores a 16/32-B NHWC vector), four elements per thread with 16-B float and 4-B byte accesses in the plane kernels
// when counts and pointers allow, else one. No allocation, no synchronisation.
// Every stage is one kernel over n camera pairs, the stream in blockIdx.y, behind one host function; the entry points
// sd_live_*_n pass their arguments through and the single-stream sd_live_* are their n = 1 case (at the end).
//
// Arithmetic: fp32 from the bytes on, every rounding explicit (fmaf, or mul_rn / add_rn / ... under fp contract(off)),
// so that no contraction choice of the compiler can differ between instantiations: the packed input is bit-identical
// to sd_pack_input of the NCHW output, and the post stage reproduces numpy's float32 arithmetic (Python-float scalars
// cast to float32 first, NEP 50).
// OpenCV's intermediate uint8 rounding and its fixed-point coefficient tables are NOT reproduced.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "radix_select.h"
#include "stage_util.h"

// No contraction anywhere in this file: a * b + c stays two roundings unless written fmaf. HIP's __fmul_rn / __fadd_rn
// are plain operators that the compiler may still fuse after inlining (it did, in one instantiation of the post kernel
// and not in another), so the single-rounding operations are spelled out here, under the pragma.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

int live_grid(long long work) { return grid_for(work, 16384); }

// the values of a map that count: the auto range and the centre medians
struct LivePositive {
    __device__ __forceinline__ static bool test(float v) { return finite_f(v) && v > 0.f; }
};

// V consecutive elements per thread in the plane-streaming kernels (post, contours, auto-range codes): V = 4 when the
// element count is a multiple of 4 and the pointers are aligned (16-B float and 4-B byte-plane accesses), else V = 1.
// The gathering kernels (front end, rectified view, compose) stay one pixel per thread: four pixels per thread with
// 12-B BGR stores measured slower (rectify 4.7 -> 7.2 us, compose 6.1 -> 7.2 us at 640x480: a quarter of the threads,
// each with four times the dependent gather latency). ld_f and st_u8 are stage_util.h's.
template <int V> __device__ __forceinline__ void st_f(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

// ------------------------------------------------------------------ front end
// Remapped pixel (y, x) of one BGR frame, values in [0, 255]. map1 int16 [Hc][Wc][2] = integer x, y; map2 uint16
// [Hc][Wc], low 10 bits = fy5 << 5 | fx5 (fractions in 1/32 px): OpenCV's CV_16SC2 fixed-point maps. Bilinear, a tap
// outside the frame contributes 0. Weights are multiples of 1/32 and taps are bytes: every product and sum below is
// exact in fp32. map1 == NULL: the frame itself.
__device__ __forceinline__ void remap_px(const uint8_t* __restrict__ img, int Hc, int Wc, const short* __restrict__ map1,
                                         const unsigned short* __restrict__ map2, int y, int x, float (&v)[3]) {
    const size_t p = (size_t)y * Wc + x;
    if (!map1) {
        const uint8_t* q = img + p * 3;
        v[0] = (float)q[0];
        v[1] = (float)q[1];
        v[2] = (float)q[2];
        return;
    }
    const int ix = map1[2 * p], iy = map1[2 * p + 1];
    const unsigned f = map2[p];
    const float fx = (float)(f & 31u) * (1.f / 32.f), fy = (float)((f >> 5) & 31u) * (1.f / 32.f);
    float t[2][2][3];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int yy = iy + dy, xx = ix + dx;
            const bool in = (unsigned)yy < (unsigned)Hc && (unsigned)xx < (unsigned)Wc;
            const uint8_t* q = img + ((size_t)(in ? yy : 0) * Wc + (in ? xx : 0)) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) t[dy][dx][c] = in ? (float)q[c] : 0.f;
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = fmaf(fx, sub_rn(t[0][1][c], t[0][0][c]), t[0][0][c]);
        const float bot = fmaf(fx, sub_rn(t[1][1][c], t[1][0][c]), t[1][0][c]);
        v[c] = fmaf(fy, sub_rn(bot, top), top);
    }
}

// Model-resolution pixel (y, x) of one frame: bilinear resize (half-pixel centres, edge replicate: src_index) taken over
// the REMAPPED image (up to 16 source taps per channel), / 255, in RGB order. The one place this value is computed.
__device__ __forceinline__ void live_px(const uint8_t* __restrict__ img, int Hc, int Wc, const short* __restrict__ map1,
                                        const unsigned short* __restrict__ map2, int H, int W, int y, int x,
                                        float (&rgb)[3]) {
    int y0, y1, x0, x1;
    float ly, lx;
    src_index(y, H, Hc, y0, y1, ly);
    src_index(x, W, Wc, x0, x1, lx);
    float a[3], b[3], c[3], d[3];
    remap_px(img, Hc, Wc, map1, map2, y0, x0, a);
    remap_px(img, Hc, Wc, map1, map2, y0, x1, b);
    remap_px(img, Hc, Wc, map1, map2, y1, x0, c);
    remap_px(img, Hc, Wc, map1, map2, y1, x1, d);
    const float wx = sub_rn(1.f, lx), wy = sub_rn(1.f, ly);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float top = fmaf(b[ch], lx, mul_rn(a[ch], wx));
        const float bot = fmaf(d[ch], lx, mul_rn(c[ch], wx));
        rgb[2 - ch] = div_rn(fmaf(bot, ly, mul_rn(top, wy)), 255.f);
    }
}

// one model pixel per thread: 8-channel NHWC vector store [L_R, L_G, L_B, R_R, R_G, R_B, 0, 0], optional NCHW planes,
// optional max over the frame into amax[slot] with amax[clear] zeroed by the launch's one `clearer` block (the protocol
// of k_pack_input_amax, misc.hip). Each stage below is written once, as the body that its kernel runs per stream.
template <typename T>
__device__ __forceinline__ void live_frontend_body(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                                                   int Hc, int Wc, const short* __restrict__ m1l,
                                                   const unsigned short* __restrict__ m2l, const short* __restrict__ m1r,
                                                   const unsigned short* __restrict__ m2r, int H, int W,
                                                   T* __restrict__ xin, float* __restrict__ nchw, unsigned* amax, int slot,
                                                   int clear, bool clearer) {
    const int P = H * W;
    float m = 0.f;
    for (int px = blockIdx.x * 256 + threadIdx.x; px < P; px += gridDim.x * 256) {
        const int y = px / W, x = px - y * W;
        float l[3], r[3];
        live_px(left, Hc, Wc, m1l, m2l, H, W, y, x, l);
        live_px(right, Hc, Wc, m1r, m2r, H, W, y, x, r);
        const float v[8] = {l[0], l[1], l[2], r[0], r[1], r[2], 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 6; ++i) m = fmaxf(m, fabsf(v[i]));
        store8(xin + (size_t)px * 8, v);
        if (nchw) {
#pragma unroll
            for (int i = 0; i < 6; ++i) nchw[(size_t)i * P + px] = v[i];
        }
    }
    if (amax) {  // uniform over the grid
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        __shared__ float wm[4];
        if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned mb = __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3])));
            if (mb > __hip_atomic_load(amax + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax + slot, mb);
        }
        if (clearer && threadIdx.x == 64 && clear >= 0) amax[clear] = 0u;
    }
}

// The kernels: blockIdx.y is the stream, every buffer is [n] of one stream's layout, and each block runs the body on
// its stream's slices (blockIdx.x / gridDim.x keep their meaning inside the body). A stream whose bit is set in `hold`
// returns before it reads or writes anything. Optional (NULL) buffers stay NULL.
template <typename T> __device__ __forceinline__ T* at(T* p, size_t off) { return p ? p + off : nullptr; }
__device__ __forceinline__ bool bit(unsigned long long mask, unsigned i) { return (mask >> i) & 1ull; }

// maps: map_stride pixels between the streams' map sets (0: one set for all)
template <typename T>
__global__ __launch_bounds__(256) void k_live_frontend(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                                                       int Hc, int Wc, const short* __restrict__ m1l,
                                                       const unsigned short* __restrict__ m2l,
                                                       const short* __restrict__ m1r,
                                                       const unsigned short* __restrict__ m2r, size_t map_stride, int H,
                                                       int W, T* __restrict__ xin, float* __restrict__ nchw,
                                                       unsigned* amax, int slot, int clear) {
    const size_t i = blockIdx.y, F = (size_t)Hc * Wc * 3, P = (size_t)H * W, mo = i * map_stride;
    live_frontend_body<T>(left + i * F, right + i * F, Hc, Wc, at(m1l, 2 * mo), at(m2l, mo), at(m1r, 2 * mo), at(m2r, mo),
                          H, W, xin + i * P * 8, at(nchw, i * 6 * P), amax, slot, clear,
                          blockIdx.x == 0 && blockIdx.y == 0);
}

// the rectified view as the display shows it: remapped BGR bytes, round half to even (the value is a multiple of 1/1024)
__device__ __forceinline__ void live_rectify_body(const uint8_t* __restrict__ img, int Hc, int Wc,
                                                  const short* __restrict__ map1,
                                                  const unsigned short* __restrict__ map2, uint8_t* __restrict__ view) {
    const int P = Hc * Wc;
    for (int px = blockIdx.x * 256 + threadIdx.x; px < P; px += gridDim.x * 256) {
        const int y = px / Wc, x = px - y * Wc;
        float v[3];
        remap_px(img, Hc, Wc, map1, map2, y, x, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) view[(size_t)px * 3 + c] = (uint8_t)min(max(__float2int_rn(v[c]), 0), 255);
    }
}
__global__ __launch_bounds__(256) void k_live_rectify(const uint8_t* __restrict__ img, int Hc, int Wc,
                                                      const short* __restrict__ map1,
                                                      const unsigned short* __restrict__ map2, size_t map_stride,
                                                      uint8_t* __restrict__ view) {
    const size_t i = blockIdx.y, F = (size_t)Hc * Wc * 3, mo = i * map_stride;
    live_rectify_body(img + i * F, Hc, Wc, map1 + 2 * mo, map2 + mo, view + i * F);
}

// ------------------------------------------------------------------ post stage
// colorize_scalar_map's uint8 code: trunc(clip((v - lo) / scale, 0, 1) * 255) for finite v > 0, else 0
__device__ __forceinline__ uint8_t code_of(float v, float lo, float scale) {
    if (!(finite_f(v) && v > 0.f)) return 0;
    const float t = fminf(fmaxf(div_rn(sub_rn(v, lo), scale), 0.f), 1.f);
    return (uint8_t)(int)mul_rn(t, 255.f);
}

template <int V>
__device__ __forceinline__ void live_post_body(const float* __restrict__ pred, const float* __restrict__ logvar, int P,
                                               float* __restrict__ state, int copy, float a, float b, int depth_on,
                                               float fb, float* __restrict__ depth, float* __restrict__ conf,
                                               uint8_t* __restrict__ dcode, float dlo, float dscale,
                                               uint8_t* __restrict__ ccode, float clo, float cscale) {
    for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < P; i += gridDim.x * 256 * V) {
        float s[V];
        ld_f<V>(pred + i, s);
        if (!copy) {
            float o[V];
            ld_f<V>(state + i, o);
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] = add_rn(mul_rn(a, s[k]), mul_rn(b, o[k]));
        }
        st_f<V>(state + i, s);
        if (depth_on) {
            float d[V];
            uint8_t c[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                d[k] = (finite_f(s[k]) && s[k] > 1e-6f) ? div_rn(fb, s[k]) : NAN;
                c[k] = code_of(d[k], dlo, dscale);
            }
            st_f<V>(depth + i, d);
            if (dcode) st_u8<V>(dcode + i, c);
        }
        if (logvar) {
            float l[V];
            uint8_t c[V];
            ld_f<V>(logvar + i, l);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                l[k] = expf(mul_rn(-0.5f, l[k]));
                c[k] = code_of(l[k], clo, cscale);
            }
            st_f<V>(conf + i, l);
            if (ccode) st_u8<V>(ccode + i, c);
        }
    }
}
// copy: bit i = stream i takes its prediction as is; focal_baseline: fbs[i] per stream, or fb for all when fbs is NULL
template <int V>
__global__ __launch_bounds__(256) void k_live_post(const float* __restrict__ pred, const float* __restrict__ logvar, int P,
                                                   float* __restrict__ state, unsigned long long copy,
                                                   unsigned long long hold, float a, float b, int depth_on,
                                                   const float* __restrict__ fbs, float fb, float* __restrict__ depth,
                                                   float* __restrict__ conf, uint8_t* __restrict__ dcode, float dlo,
                                                   float dscale, uint8_t* __restrict__ ccode, float clo, float cscale) {
    const unsigned i = blockIdx.y;
    if (bit(hold, i)) return;
    const size_t o = (size_t)i * P;
    live_post_body<V>(pred + o, at(logvar, o), P, state + o, (int)bit(copy, i), a, b, depth_on, fbs ? fbs[i] : fb,
                      at(depth, o), at(conf, o), at(dcode, o), dlo, dscale, at(ccode, o), clo, cscale);
}

// depth_contour_mask: 255 where the right or the lower neighbour is valid too and lies in another depth bin
__device__ __forceinline__ int contour_bin(float d, float dmin, float dmax, float step) {
    if (!(finite_f(d) && d > dmin && d <= dmax)) return -1;
    return (int)floorf(div_rn(sub_rn(fminf(fmaxf(d, dmin), dmax), dmin), step));
}
// V = 4 needs W % 4 == 0: the four pixels of a thread then lie in one row
template <int V>
__device__ __forceinline__ void live_edges_body(const float* __restrict__ depth, int H, int W, float dmin, float dmax,
                                                float step, uint8_t* __restrict__ edge) {
    const int P = H * W;
    for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < P; i += gridDim.x * 256 * V) {
        const int y = i / W, x = i - y * W;
        float d[V], dn[V];
        ld_f<V>(depth + i, d);
        const bool below = y + 1 < H;
        if (below) ld_f<V>(depth + i + W, dn);
        int b[V + 1];
#pragma unroll
        for (int k = 0; k < V; ++k) b[k] = contour_bin(d[k], dmin, dmax, step);
        b[V] = x + V < W ? contour_bin(depth[i + V], dmin, dmax, step) : -1;
        uint8_t e[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            bool on = b[k] >= 0 && b[k + 1] >= 0 && b[k + 1] != b[k];
            if (below && b[k] >= 0) {
                const int q = contour_bin(dn[k], dmin, dmax, step);
                on |= q >= 0 && q != b[k];
            }
            e[k] = on ? 255 : 0;
        }
        st_u8<V>(edge + i, e);
    }
}
template <int V>
__global__ __launch_bounds__(256) void k_live_edges(const float* __restrict__ depth, int H, int W, float dmin, float dmax,
                                                    float step, uint8_t* __restrict__ edge, unsigned long long hold) {
    if (bit(hold, blockIdx.y)) return;
    const size_t o = (size_t)blockIdx.y * H * W;
    live_edges_body<V>(depth + o, H, W, dmin, dmax, step, edge + o);
}

// ------------------------------------------------------------------ exact order statistics (auto range)
// radix_select.h's three-level select under this rule set: the finite, > 0 values count; they order like their bit
// patterns (< 0x7f800000, 31 bits), so the key is the pattern itself, 11 + 11 + 9 bits; the quantiles are 2 % and 98 %.
struct LiveSelect {
    static constexpr int LAST_BITS = 9;
    __device__ __forceinline__ static bool member(float v) { return LivePositive::test(v); }
    __device__ __forceinline__ static unsigned key(float v) { return __float_as_uint(v); }
    __device__ __forceinline__ static float value(unsigned key) { return __uint_as_float(key); }
    // numpy's `linear` percentile of the sorted valid values from the two order statistics around (n - 1) * q, in fp64
    // (lib/_function_base_impl.py: _lerp), rounded to float32 once
    __device__ __forceinline__ static float lerp(float a, float b, double vi) {
        const double g = vi - floor(vi), d = (double)b - (double)a;
        return (float)(g >= 0.5 ? (double)b - d * (1.0 - g) : (double)a + d * g);
    }
};
constexpr double LIVE_Q_LO = 0.02, LIVE_Q_HI = 0.98;

// the auto-range codes: lo, hi and n from sd_live_select's result, on the device; scale = max(hi - lo, 1e-6) in fp64
template <int V>
__device__ __forceinline__ void live_code_auto_body(const float* __restrict__ v, int P, const float* __restrict__ sel,
                                                    uint8_t* __restrict__ code) {
    const unsigned n = reinterpret_cast<const unsigned*>(sel)[0];
    const float lo = sel[5];
    const float scale = (float)fmax((double)sel[6] - (double)sel[5], 1e-6);
    for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < P; i += gridDim.x * 256 * V) {
        float x[V];
        uint8_t c[V];
        ld_f<V>(v + i, x);
#pragma unroll
        for (int k = 0; k < V; ++k) c[k] = n ? code_of(x[k], lo, scale) : 0;
        st_u8<V>(code + i, c);
    }
}
template <int V>
__global__ __launch_bounds__(256) void k_live_code_auto(const float* __restrict__ v, int P, const float* __restrict__ sel,
                                                        uint8_t* __restrict__ code, unsigned long long hold) {
    if (bit(hold, blockIdx.y)) return;
    const size_t o = (size_t)blockIdx.y * P;
    live_code_auto_body<V>(v + o, P, sel + (size_t)blockIdx.y * 8, code + o);
}

// ------------------------------------------------------------------ centre-window medians
// block (b, i): stage_util.h's center_median of the finite, > 0 values of stream i's map b (bounds as
// depth_live_dl.py:542-548); a map that is not given: NaN. grid (3, n): out [n][3]
__global__ __launch_bounds__(256) void k_live_center(const float* m0, const float* m1, const float* m2, int H, int W,
                                                     int window, float* __restrict__ out, unsigned long long hold) {
    if (bit(hold, blockIdx.y)) return;
    const float* src = blockIdx.x == 0 ? m0 : blockIdx.x == 1 ? m1 : m2;
    const float m = src ? center_median<LivePositive>(src + (size_t)blockIdx.y * H * W, H, W, window) : NAN;
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * 3 + blockIdx.x] = m;
}

// ------------------------------------------------------------------ compose
// One view pixel per thread. Each colour image: the [256][3] BGR LUT applied to the model-resolution codes, resized
// bilinearly to the view (half-pixel centres, edge replicate, round half to even), i.e. cv2.resize(applyColorMap(code)).
// The contour mask is nearest-resized (sx = min(dx * Ws / Wd, Ws - 1)) and painted (0, 255, 0) onto the left view.
__device__ __forceinline__ void lut_bilerp(const uint8_t* __restrict__ code, const uint8_t* lut, int W, int y0, int y1,
                                           int x0, int x1, float ly, float lx, uint8_t* out) {
    const uint8_t* a = lut + 3 * code[(size_t)y0 * W + x0];
    const uint8_t* b = lut + 3 * code[(size_t)y0 * W + x1];
    const uint8_t* c = lut + 3 * code[(size_t)y1 * W + x0];
    const uint8_t* d = lut + 3 * code[(size_t)y1 * W + x1];
    const float wx = sub_rn(1.f, lx), wy = sub_rn(1.f, ly);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float top = fmaf((float)b[ch], lx, mul_rn((float)a[ch], wx));
        const float bot = fmaf((float)d[ch], lx, mul_rn((float)c[ch], wx));
        out[ch] = (uint8_t)min(max(__float2int_rn(fmaf(bot, ly, mul_rn(top, wy))), 0), 255);
    }
}

__device__ __forceinline__ void live_compose_body(const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ lut_a,
                                                  uint8_t* __restrict__ vis_a, const uint8_t* __restrict__ code_b,
                                                  const uint8_t* __restrict__ lut_b, uint8_t* __restrict__ vis_b,
                                                  const uint8_t* __restrict__ edge, const uint8_t* __restrict__ view,
                                                  uint8_t* __restrict__ left_view, int H, int W, int Hc, int Wc) {
    __shared__ uint8_t lut[2][768];
    for (int i = threadIdx.x; i < 768; i += 256) {
        lut[0][i] = code_a ? lut_a[i] : 0;
        lut[1][i] = code_b ? lut_b[i] : 0;
    }
    __syncthreads();
    const int P = Hc * Wc;
    for (int px = blockIdx.x * 256 + threadIdx.x; px < P; px += gridDim.x * 256) {
        const int dy = px / Wc, dx = px - dy * Wc;
        if (code_a || code_b) {
            int y0, y1, x0, x1;
            float ly, lx;
            src_index(dy, Hc, H, y0, y1, ly);
            src_index(dx, Wc, W, x0, x1, lx);
            if (code_a) lut_bilerp(code_a, lut[0], W, y0, y1, x0, x1, ly, lx, vis_a + (size_t)px * 3);
            if (code_b) lut_bilerp(code_b, lut[1], W, y0, y1, x0, x1, ly, lx, vis_b + (size_t)px * 3);
        }
        if (left_view) {
            bool on = false;
            if (edge) {
                const int sy = min((int)((long long)dy * H / Hc), H - 1), sx = min((int)((long long)dx * W / Wc), W - 1);
                on = edge[(size_t)sy * W + sx] != 0;
            }
            const uint8_t* q = view + (size_t)px * 3;
            uint8_t* o = left_view + (size_t)px * 3;
            o[0] = on ? 0 : q[0];
            o[1] = on ? 255 : q[1];
            o[2] = on ? 0 : q[2];
        }
    }
}
// the colour tables are shared by the streams
__global__ __launch_bounds__(256) void k_live_compose(const uint8_t* __restrict__ code_a, const uint8_t* __restrict__ lut_a,
                                                      uint8_t* __restrict__ vis_a, const uint8_t* __restrict__ code_b,
                                                      const uint8_t* __restrict__ lut_b, uint8_t* __restrict__ vis_b,
                                                      const uint8_t* __restrict__ edge, const uint8_t* __restrict__ view,
                                                      uint8_t* __restrict__ left_view, int H, int W, int Hc, int Wc,
                                                      unsigned long long hold) {
    if (bit(hold, blockIdx.y)) return;
    const size_t m = (size_t)blockIdx.y * H * W, f = (size_t)blockIdx.y * Hc * Wc * 3;
    live_compose_body(at(code_a, m), lut_a, at(vis_a, f), at(code_b, m), lut_b, at(vis_b, f), at(edge, m), at(view, f),
                      at(left_view, f), H, W, Hc, Wc);
}

// ------------------------------------------------------------------ host side
// One function per stage with all of its checks, the vector-path decision and its launches; fn is the calling entry
// point's name, for the messages. The vector paths are taken only when every stream's slice is aligned: the element
// count per stream a multiple of 4 (so that the slices of streams 1..n-1 start on the 16-B / 4-B boundary the base
// pointer has) and the base pointers aligned.
bool live_dims_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= INT_MAX / 16; }
bool streams_ok(int n) { return n >= 1 && n <= 64; }
bool mask_ok(unsigned long long mask, int n) { return n >= 64 || (mask >> n) == 0ull; }

#define LIVE_N_REQUIRE(fn, n) SD_REQUIRE(streams_ok(n), "%s: n = %d streams (1..64)", fn, n)
#define LIVE_MASK_REQUIRE(fn, name, mask, n) \
    SD_REQUIRE(mask_ok(mask, n), "%s: " name " 0x%llx has a bit at or above n = %d", fn, (unsigned long long)(mask), n)
#define LIVE_STRIDE_REQUIRE(fn, map_stride, Hc, Wc)                      \
    SD_REQUIRE(map_stride == 0 || map_stride == (long long)(Hc) * (Wc), \
               "%s: map_stride %lld (0: shared maps, Hc * Wc: one set per stream)", fn, map_stride)

int live_frontend(const char* fn, int n, int dtype, const uint8_t* left, const uint8_t* right, int Hc, int Wc,
                  const int16_t* map1_l, const uint16_t* map2_l, const int16_t* map1_r, const uint16_t* map2_r,
                  long long map_stride, int H, int W, void* xin, float* nchw, unsigned* amax, int slot, int clear,
                  sd_stream s) {
    LIVE_N_REQUIRE(fn, n);
    SD_REQUIRE(left && right && xin, "%s: null pointer (left, right, xin)", fn);
    SD_REQUIRE(live_dims_ok(Hc, Wc) && live_dims_ok(H, W), "%s: bad sizes %dx%d -> %dx%d", fn, Hc, Wc, H, W);
    SD_REQUIRE(!map1_l == !map2_l && !map1_r == !map2_r, "%s: map1 and map2 go together", fn);
    LIVE_STRIDE_REQUIRE(fn, map_stride, Hc, Wc);
    SD_REQUIRE(dtype == SD_F32 || dtype == SD_BF16, "%s: dtype %d", fn, dtype);
    SD_REQUIRE((uintptr_t)xin % 16 == 0, "%s: xin must be 16-B aligned", fn);
    SD_REQUIRE(!amax || (slot >= 0 && clear != slot), "%s: amax slot %d clear %d", fn, slot, clear);
    const dim3 g(live_grid((long long)H * W), n);
    if (dtype == SD_BF16)
        hipLaunchKernelGGL(k_live_frontend<__bf16>, g, dim3(256), 0, to_stream(s), left, right, Hc, Wc, map1_l, map2_l,
                           map1_r, map2_r, (size_t)map_stride, H, W, (__bf16*)xin, nchw, amax, slot, clear);
    else
        hipLaunchKernelGGL(k_live_frontend<float>, g, dim3(256), 0, to_stream(s), left, right, Hc, Wc, map1_l, map2_l,
                           map1_r, map2_r, (size_t)map_stride, H, W, (float*)xin, nchw, amax, slot, clear);
    return sd_check_launch(fn);
}

int live_rectify(const char* fn, int n, const uint8_t* frames, int Hc, int Wc, const int16_t* map1, const uint16_t* map2,
                 long long map_stride, uint8_t* views, sd_stream s) {
    LIVE_N_REQUIRE(fn, n);
    SD_REQUIRE(frames && views, "%s: null pointer (frames, views)", fn);
    SD_REQUIRE(map1 && map2, "%s: null pointer (map1 and map2 go together, both needed)", fn);
    SD_REQUIRE(live_dims_ok(Hc, Wc), "%s: bad sizes %dx%d", fn, Hc, Wc);
    LIVE_STRIDE_REQUIRE(fn, map_stride, Hc, Wc);
    hipLaunchKernelGGL(k_live_rectify, dim3(live_grid((long long)Hc * Wc), n), dim3(256), 0, to_stream(s), frames, Hc, Wc,
                       map1, map2, (size_t)map_stride, views);
    return sd_check_launch(fn);
}

// focal_baseline: the device array fbs [n] when fb_array (sd_live_post_n), else the scalar fb for every stream
int live_post(const char* fn, int n, const float* disp, const float* logvar, int H, int W, float* state,
              unsigned long long copy_mask, unsigned long long hold_mask, float alpha, float one_minus_alpha, int depth_on,
              bool fb_array, const float* fbs, float fb, float* depth, float* conf, uint8_t* depth_code, float depth_lo,
              float depth_scale, uint8_t* conf_code, float conf_lo, float conf_scale, sd_stream s) {
    LIVE_N_REQUIRE(fn, n);
    SD_REQUIRE(disp && state, "%s: null pointer (disp, state)", fn);
    SD_REQUIRE(live_dims_ok(H, W), "%s: bad sizes %dx%d", fn, H, W);
    LIVE_MASK_REQUIRE(fn, "copy_mask", copy_mask, n);
    LIVE_MASK_REQUIRE(fn, "hold_mask", hold_mask, n);
    SD_REQUIRE(!depth_on || (depth && (fbs || !fb_array)),
               "%s: depth enabled without a depth buffer or focal_baseline", fn);
    SD_REQUIRE(!logvar || conf, "%s: logvar without a confidence buffer", fn);
    SD_REQUIRE((!depth_code || depth_scale > 0.f) && (!conf_code || conf_scale > 0.f), "%s: code scale <= 0", fn);
    const int P = H * W;
    const bool vec = P % 4 == 0 && aligned(disp, 16) && aligned(logvar, 16) && aligned(state, 16) && aligned(depth, 16) &&
                     aligned(conf, 16) && aligned(depth_code, 4) && aligned(conf_code, 4);
    hipLaunchKernelGGL(vec ? k_live_post<4> : k_live_post<1>, dim3(live_grid(vec ? P / 4 : P), n), dim3(256), 0,
                       to_stream(s), disp, logvar, P, state, copy_mask, hold_mask, alpha, one_minus_alpha, depth_on,
                       depth_on && fb_array ? fbs : nullptr, fb, depth, conf, depth_code, depth_lo, depth_scale, conf_code,
                       conf_lo, conf_scale);
    return sd_check_launch(fn);
}

int live_contours(const char* fn, int n, const float* depth, int H, int W, float min_depth, float max_depth, float step,
                  uint8_t* edge, unsigned long long hold_mask, sd_stream s) {
    LIVE_N_REQUIRE(fn, n);
    SD_REQUIRE(depth && edge, "%s: null pointer (depth, edge)", fn);
    SD_REQUIRE(live_dims_ok(H, W), "%s: bad sizes %dx%d", fn, H, W);
    LIVE_MASK_REQUIRE(fn, "hold_mask", hold_mask, n);
    SD_REQUIRE(step > 0.f && max_depth > min_depth, "%s: bad range", fn);
    // W % 4 == 0 makes H * W a multiple of 4 too: every stream's slice keeps the base pointers' alignment
    const bool vec = W % 4 == 0 && aligned(depth, 16) && aligned(edge, 4);
    hipLaunchKernelGGL(vec ? k_live_edges<4> : k_live_edges<1>, dim3(live_grid((long long)H * W / (vec ? 4 : 1)), n),
                       dim3(256), 0, to_stream(s), depth, H, W, min_depth, max_depth, step, edge, hold_mask);
    return sd_check_launch(fn);
}

int live_select(const char* fn, int n, const float* values, int H, int W, unsigned* work, float* sel, uint8_t* code,
                unsigned long long hold_mask, sd_stream s) {
    LIVE_N_REQUIRE(fn, n);
    SD_REQUIRE(values && work && sel, "%s: null pointer (values, work, sel)", fn);
    SD_REQUIRE(live_dims_ok(H, W), "%s: bad sizes %dx%d", fn, H, W);
    LIVE_MASK_REQUIRE(fn, "hold_mask", hold_mask, n);
    const int P = H * W;
    hipStream_t st = to_stream(s);
    select_launch<LiveSelect>(n, values, P, LIVE_Q_LO, LIVE_Q_HI, work, sel, hold_mask, st);
    if (code) {
        const bool vec = P % 4 == 0 && aligned(values, 16) && aligned(code, 4);
        hipLaunchKernelGGL(vec ? k_live_code_auto<4> : k_live_code_auto<1>, dim3(live_grid(vec ? P / 4 : P), n), dim3(256),
                           0, st, values, P, sel, code, hold_mask);
    }
    return sd_check_launch(fn);
}

int live_center(const char* fn, int n, const float* disp, const float* depth, const float* conf, int H, int W, int window,
                float* out3, unsigned long long hold_mask, sd_stream s) {
    LIVE_N_REQUIRE(fn, n);
    SD_REQUIRE(disp && out3, "%s: null pointer (disp, out3)", fn);
    SD_REQUIRE(live_dims_ok(H, W), "%s: bad sizes %dx%d", fn, H, W);
    LIVE_MASK_REQUIRE(fn, "hold_mask", hold_mask, n);
    SD_REQUIRE(window >= 0 && window <= 63, "%s: window %d (max 63)", fn, window);
    hipLaunchKernelGGL(k_live_center, dim3(3, n), dim3(256), 0, to_stream(s), disp, depth, conf, H, W, window, out3,
                       hold_mask);
    return sd_check_launch(fn);
}

int live_compose(const char* fn, int n, const uint8_t* code_a, const uint8_t* lut_a, uint8_t* vis_a, const uint8_t* code_b,
                 const uint8_t* lut_b, uint8_t* vis_b, const uint8_t* edge, const uint8_t* view, uint8_t* left_view, int H,
                 int W, int Hc, int Wc, unsigned long long hold_mask, sd_stream s) {
    LIVE_N_REQUIRE(fn, n);
    SD_REQUIRE(code_a || code_b || left_view, "%s: nothing to do", fn);
    SD_REQUIRE(!code_a || (lut_a && vis_a), "%s: null pointer (image a: lut_a, vis_a)", fn);
    SD_REQUIRE(!code_b || (lut_b && vis_b), "%s: null pointer (image b: lut_b, vis_b)", fn);
    SD_REQUIRE(!left_view || view, "%s: null pointer (view)", fn);
    SD_REQUIRE(!edge || left_view, "%s: contour mask without a left view to paint", fn);
    SD_REQUIRE(live_dims_ok(H, W) && live_dims_ok(Hc, Wc), "%s: bad sizes %dx%d -> %dx%d", fn, H, W, Hc, Wc);
    LIVE_MASK_REQUIRE(fn, "hold_mask", hold_mask, n);
    hipLaunchKernelGGL(k_live_compose, dim3(live_grid((long long)Hc * Wc), n), dim3(256), 0, to_stream(s), code_a, lut_a,
                       vis_a, code_b, lut_b, vis_b, edge, view, left_view, H, W, Hc, Wc, hold_mask);
    return sd_check_launch(fn);
}

}  // namespace

// ------------------------------------------------------------------ entry points
// sd_live_X_n hands its arguments to live_X; sd_live_X is the same call for one stream: n = 1, no stream held, shared
// maps (map_stride 0), `copy` as bit 0 of the copy mask, focal_baseline by value.
extern "C" int sd_live_frontend_n(int n, int dtype, const uint8_t* left, const uint8_t* right, int Hc, int Wc,
                                  const int16_t* map1_l, const uint16_t* map2_l, const int16_t* map1_r,
                                  const uint16_t* map2_r, long long map_stride, int H, int W, void* xin, float* nchw,
                                  unsigned* amax, int slot, int clear, sd_stream s) {
    return live_frontend("sd_live_frontend_n", n, dtype, left, right, Hc, Wc, map1_l, map2_l, map1_r, map2_r, map_stride, H,
                         W, xin, nchw, amax, slot, clear, s);
}
extern "C" int sd_live_frontend(int dtype, const uint8_t* left, const uint8_t* right, int Hc, int Wc,
                                const int16_t* map1_l, const uint16_t* map2_l, const int16_t* map1_r,
                                const uint16_t* map2_r, int H, int W, void* xin, float* nchw, unsigned* amax, int slot,
                                int clear, sd_stream s) {
    return live_frontend("sd_live_frontend", 1, dtype, left, right, Hc, Wc, map1_l, map2_l, map1_r, map2_r, 0, H, W, xin,
                         nchw, amax, slot, clear, s);
}

extern "C" int sd_live_rectify_n(int n, const uint8_t* frames, int Hc, int Wc, const int16_t* map1, const uint16_t* map2,
                                 long long map_stride, uint8_t* views, sd_stream s) {
    return live_rectify("sd_live_rectify_n", n, frames, Hc, Wc, map1, map2, map_stride, views, s);
}
extern "C" int sd_live_rectify(const uint8_t* frame, int Hc, int Wc, const int16_t* map1, const uint16_t* map2,
                               uint8_t* view, sd_stream s) {
    return live_rectify("sd_live_rectify", 1, frame, Hc, Wc, map1, map2, 0, view, s);
}

extern "C" int sd_live_post_n(int n, const float* disp, const float* logvar, int H, int W, float* state,
                              unsigned long long copy_mask, unsigned long long hold_mask, float alpha,
                              float one_minus_alpha, int depth_on, const float* focal_baseline, float* depth, float* conf,
                              uint8_t* depth_code, float depth_lo, float depth_scale, uint8_t* conf_code, float conf_lo,
                              float conf_scale, sd_stream s) {
    return live_post("sd_live_post_n", n, disp, logvar, H, W, state, copy_mask, hold_mask, alpha, one_minus_alpha, depth_on,
                     true, focal_baseline, 0.f, depth, conf, depth_code, depth_lo, depth_scale, conf_code, conf_lo,
                     conf_scale, s);
}
extern "C" int sd_live_post(const float* disp, const float* logvar, int H, int W, float* state, int copy, float alpha,
                            float one_minus_alpha, int depth_on, float focal_baseline, float* depth, float* conf,
                            uint8_t* depth_code, float depth_lo, float depth_scale, uint8_t* conf_code, float conf_lo,
                            float conf_scale, sd_stream s) {
    return live_post("sd_live_post", 1, disp, logvar, H, W, state, copy ? 1 : 0, 0, alpha, one_minus_alpha, depth_on, false,
                     nullptr, focal_baseline, depth, conf, depth_code, depth_lo, depth_scale, conf_code, conf_lo,
                     conf_scale, s);
}

extern "C" int sd_live_contours_n(int n, const float* depth, int H, int W, float min_depth, float max_depth, float step,
                                  uint8_t* edge, unsigned long long hold_mask, sd_stream s) {
    return live_contours("sd_live_contours_n", n, depth, H, W, min_depth, max_depth, step, edge, hold_mask, s);
}
extern "C" int sd_live_contours(const float* depth, int H, int W, float min_depth, float max_depth, float step,
                                uint8_t* edge, sd_stream s) {
    return live_contours("sd_live_contours", 1, depth, H, W, min_depth, max_depth, step, edge, 0, s);
}

extern "C" long long sd_live_select_n_ws_bytes(int n) {
    return streams_ok(n) ? (long long)n * SelectLayout<LiveSelect>::WORDS * 4 : -1;
}
extern "C" long long sd_live_select_ws_bytes(void) { return sd_live_select_n_ws_bytes(1); }

extern "C" int sd_live_select_n(int n, const float* values, int H, int W, unsigned* work, float* sel, uint8_t* code,
                                unsigned long long hold_mask, sd_stream s) {
    return live_select("sd_live_select_n", n, values, H, W, work, sel, code, hold_mask, s);
}
extern "C" int sd_live_select(const float* values, int H, int W, unsigned* work, float* sel, uint8_t* code,
                              sd_stream s) {
    return live_select("sd_live_select", 1, values, H, W, work, sel, code, 0, s);
}

extern "C" int sd_live_center_n(int n, const float* disp, const float* depth, const float* conf, int H, int W, int window,
                                float* out3, unsigned long long hold_mask, sd_stream s) {
    return live_center("sd_live_center_n", n, disp, depth, conf, H, W, window, out3, hold_mask, s);
}
extern "C" int sd_live_center(const float* disp, const float* depth, const float* conf, int H, int W, int window,
                              float* out3, sd_stream s) {
    return live_center("sd_live_center", 1, disp, depth, conf, H, W, window, out3, 0, s);
}

extern "C" int sd_live_compose_n(int n, const uint8_t* code_a, const uint8_t* lut_a, uint8_t* vis_a, const uint8_t* code_b,
                                 const uint8_t* lut_b, uint8_t* vis_b, const uint8_t* edge, const uint8_t* view,
                                 uint8_t* left_view, int H, int W, int Hc, int Wc, unsigned long long hold_mask,
                                 sd_stream s) {
    return live_compose("sd_live_compose_n", n, code_a, lut_a, vis_a, code_b, lut_b, vis_b, edge, view, left_view, H, W, Hc,
                        Wc, hold_mask, s);
}
extern "C" int sd_live_compose(const uint8_t* code_a, const uint8_t* lut_a, uint8_t* vis_a, const uint8_t* code_b,
                               const uint8_t* lut_b, uint8_t* vis_b, const uint8_t* edge, const uint8_t* view,
                               uint8_t* left_view, int H, int W, int Hc, int Wc, sd_stream s) {
    return live_compose("sd_live_compose", 1, code_a, lut_a, vis_a, code_b, lut_b, vis_b, edge, view, left_view, H, W, Hc,
                        Wc, 0, s);
}
