// Building blocks shared by the device stages (live, preview, predict, check, selfsup, sgm): the fixed-order reductions
// behind their `rows`, the centre-window median, and the small pixel load / store helpers. Every function that does
// floating-point arithmetic states its contraction setting in its own body, so its result does not depend on the
// including file.
#pragma once
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

// ------------------------------------------------------------------ pixel helpers
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }  // false for NaN

// V consecutive elements per thread in the plane-streaming kernels: V = 4 when the element count is a multiple of 4 and
// the pointers are aligned (16-B float and 4-B byte accesses), else V = 1.
template <int V> __device__ __forceinline__ void ld_f(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}
__device__ __forceinline__ uint32_t pack4(uint8_t a, uint8_t b, uint8_t c, uint8_t d) {
    return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16 | (uint32_t)d << 24;
}
template <int V> __device__ __forceinline__ void st_u8(uint8_t* p, const uint8_t (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<uint32_t*>(p) = pack4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}
// V RGB pixels, each r | g << 8 | b << 16 (memory order R, G, B): three 4-B stores for V = 4 (dst 4-B aligned), three
// bytes for V = 1
__device__ __forceinline__ void st_rgb1(uint8_t* dst, uint32_t v) {
    dst[0] = (uint8_t)v, dst[1] = (uint8_t)(v >> 8), dst[2] = (uint8_t)(v >> 16);
}
template <int V> __device__ __forceinline__ void st_rgb(uint8_t* dst, const uint32_t (&v)[V]) {
    if constexpr (V == 4) {
        uint32_t* w = reinterpret_cast<uint32_t*>(dst);
        w[0] = v[0] | v[1] << 24;       // r0 g0 b0 r1
        w[1] = v[1] >> 8 | v[2] << 16;  // g1 b1 r2 g2
        w[2] = v[2] >> 16 | v[3] << 8;  // b2 r3 g3 b3
    } else {
        st_rgb1(dst, v[0]);
    }
}

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p % a) == 0; }  // NULL counts as aligned

// blocks of 256 threads for `work` items of a grid-stride kernel, `cap` at most
int grid_for(long long work, int cap) {
    long long g = (work + 255) / 256;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

// ------------------------------------------------------------------ the sums behind `rows`
// The row walk of the check and selfsup stages: a block owns whole rows and walks them in steps of STEP pixels, four
// consecutive pixels per thread; each block leaves one partial row of ROW doubles, and a second launch adds a sample's
// partial rows.
namespace row_walk {
constexpr int THREADS = 256;  // four waves
constexpr int PX = 4;         // consecutive pixels per thread
constexpr int STEP = THREADS * PX;  // pixels per step of the row walk (check.SCAN_PIXELS, selfsup.STEP_PIXELS)
constexpr int MAX_BLOCKS = 1024;    // partial rows per sample at most
constexpr int SMALL_ROWS = 16;      // rows a block owns at most because W is small
constexpr int ROW = 8;
constexpr int SUM_THREADS = 512;  // of the launch that adds the partial rows: 64 partial rows x 8 columns a step

bool sizes_ok(int n, int H, int W) { return n >= 1 && n <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31); }
// rows per block: STEP / W of them when W is small (16 at most), more when H exceeds what MAX_BLOCKS blocks cover. A
// function of (H, W) alone, as is the number of blocks (= partial rows per sample).
int rows_per_block(int H, int W) {
    int r = STEP / W;
    r = r < 1 ? 1 : (r > SMALL_ROWS ? SMALL_ROWS : r);
    const int need = (H + MAX_BLOCKS - 1) / MAX_BLOCKS;
    return r > need ? r : need;
}
int blocks(int H, int W) {
    const int r = rows_per_block(H, W);
    return (H + r - 1) / r;
}
}  // namespace row_walk

// The block's partial row from every thread's K sums: each wave by a shuffle tree, then the NT / 64 waves in index
// order (counts are exact as doubles); columns K .. 7 are stored as 0. One fixed order. Every thread of the block
// calls it.
template <int NT, int K>
__device__ __forceinline__ void block_partial_row(const double (&v)[K], double* __restrict__ partial_row) {
#pragma clang fp contract(off)
    static_assert(NT % 64 == 0 && K <= row_walk::ROW, "whole waves, a row of 8 at most");
    __shared__ double red[NT / 64][row_walk::ROW];
    double t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        t[k] = v[k];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) t[k] += __shfl_down(t[k], s);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = t[k];
    }
    __syncthreads();
    if (threadIdx.x < row_walk::ROW) {
        const int k = threadIdx.x;
        double sum = 0.0;
        if (k < K) {
            sum = red[0][k];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) sum += red[w][k];
        }
        partial_row[k] = sum;
    }
}

// rows[b][k] = the sum of the sample's partial rows; one block per sample, thread = (partial row j of THREADS / ROW,
// column k of ROW). Thread (j, k) adds column k of the partial rows j, j + 64, ... in that order (independent loads:
// with a thousand partial rows a single chain of them was most of the check stage's time at n = 1), a wave adds its
// eight j by shuffles and the eight waves are added in order: one fixed order for a given number of partial rows.
template <int ROW, int THREADS>
__global__ __launch_bounds__(THREADS) void k_rows_sum(const double* __restrict__ partial, int nblk,
                                                      double* __restrict__ rows) {
#pragma clang fp contract(off)
    static_assert(ROW == 8 && THREADS % 64 == 0, "a wave holds eight partial rows of eight columns");
    const int b = blockIdx.x, k = threadIdx.x & (ROW - 1), j = threadIdx.x >> 3;
    const double* p = partial + (size_t)b * nblk * ROW;
    double t = 0.0;
    for (int i = j; i < nblk; i += THREADS / ROW) t += p[(size_t)i * ROW + k];
#pragma unroll
    for (int s = 32; s >= ROW; s >>= 1) t += __shfl_down(t, s);
    __shared__ double red[THREADS / 64][ROW];
    if ((threadIdx.x & 63) < ROW) red[threadIdx.x >> 6][k] = t;
    __syncthreads();
    if (threadIdx.x < ROW) {
        double sum = red[0][k];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) sum += red[w][k];
        rows[(size_t)b * ROW + k] = sum;
    }
}

// ------------------------------------------------------------------ centre-window median
// The median of the members of the [H][W] map's centre window (half = max(1, window / 2) around (H / 2, W / 2), clipped
// to the map; window <= 63), in thread 0 of a block of 256: a bitonic sort of the window in LDS (<= 63 x 63 values,
// non-members and the padding to a power of two as +inf). Even count: the fp32 mean of the two middle values (numpy's
// median); no member: NaN. Member::test(float) says which values count. Every thread of the block calls it.
template <typename Member>
__device__ __forceinline__ float center_median(const float* __restrict__ src, int H, int W, int window) {
#pragma clang fp contract(off)
    __shared__ float buf[4096];
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    const int cx = W / 2, cy = H / 2, half = max(1, window / 2);
    const int y0 = max(0, cy - half), y1 = min(H, cy + half + 1), x0 = max(0, cx - half), x1 = min(W, cx + half + 1);
    const int ww = x1 - x0, total = (y1 - y0) * ww;
    int n2 = 64;
    while (n2 < total) n2 <<= 1;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n2; i += 256) {
        float x = INFINITY;
        if (i < total) {
            const int r = i / ww;
            x = src[(size_t)(y0 + r) * W + x0 + (i - r * ww)];
            if (Member::test(x)) ++mine;
            else x = INFINITY;
        }
        buf[i] = x;
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const float a = buf[i], b = buf[l];
                    if ((a > b) == ((i & k) == 0)) {
                        buf[i] = b;
                        buf[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    const int m = s_cnt;
    return m == 0 ? NAN : (m & 1) ? buf[m / 2] : (buf[m / 2 - 1] + buf[m / 2]) / 2.f;
}

}  // namespace
