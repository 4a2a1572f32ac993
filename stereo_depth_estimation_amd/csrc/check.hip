// Label-free check of a disparity map (stereo_depth_estimation_amd/check.py): the visibility class of every pixel and,
// with the two rectified frames, the photometric residual after warping the right frame onto the left. Stated in
// INTEGRATION.md ("sd_stereo_check") and pinned bit for bit to the NumPy restatement tests/check_ref.py. Per pixel, all
// in float32 with every operation rounded on its own:
//   value       disp finite and > 0 (the cloud stage's rule); xr = float32(x) - disp, the column in the right image
//   out of view a value with xr < 0
//   occluded    a value in view with m(x) + occ_tol <= xr, m(x) = the minimum of xr over the values right of x in the
//               row (+inf when there is none): a nearer pixel further right lands on or left of it
//   residual    (frames given; a value in view and not occluded) x0 = floor(xr), f = xr - x0, x1 = min(x0 + 1, W - 1),
//               r_c = a + f (b - a) per channel from right[y][x0], right[y][x1], e = (|L0 - r0| + |L1 - r1|) + |L2 - r2|
//   class       0 visible, 1 no value, 2 out of view, 3 occluded, 4 mismatch (would be 0, but e > photo_thr)
// One block owns whole rows and walks each right to left in steps of CHECK_SCAN pixels, four consecutive pixels per
// thread. The suffix minimum of a step: the thread's own pixels in registers, the lanes to its right by a wave64 shuffle
// scan, the waves to its right through LDS, the steps to its right in a register (block-uniform carry). The same thread
// then gathers from `right` and writes the outputs, so the row is read once and no block waits for another. The minimum
// is exact in any order; the sums of `rows` have one fixed order: a thread adds its pixels in the order it meets them
// (rows ascending, steps right to left, the four pixels left to right), a block adds its threads by a shuffle tree and
// its four waves in order into one partial row in `work`, and a second launch adds a sample's partial rows (64 strided
// chains, a shuffle tree, eight waves in order). No atomics; the grid is a function of (n, H, W) alone, and both store
// paths give a thread the same pixels.
// No allocation, no synchronisation: the entry point is graph-capturable. Workspace is the caller's.
#include <float.h>
#include <math.h>

#include "common.h"
#include "stage_util.h"

// the restatement rounds every operation on its own: nothing here may fuse (r_c = a + f (b - a) is two roundings)
#pragma clang fp contract(off)

namespace {

// the row walk's shape, the sizes it accepts and the blocks it takes are stage_util.h's row_walk
constexpr int CHECK_THREADS = row_walk::THREADS, CHECK_PX = row_walk::PX, CHECK_ROW = row_walk::ROW;
constexpr int CHECK_SCAN = row_walk::STEP;  // pixels per step of the row walk (check.SCAN_PIXELS)

struct CheckArgs {
    const float* disp;
    const uint8_t* left;
    const uint8_t* right;
    uint8_t* cls;
    float* resid;
    float* disp_vis;
    uint8_t* vis_rgb;
    double* partial;
    int H, W, rows_per;
    float occ_tol, photo_thr;
};

// VEC: W % 4 == 0, so a thread's four pixels are all inside the row or all outside, and every pointer is aligned:
// 16-B loads of disp, word loads of left, word and 16-B stores. Otherwise scalar loads and stores, any width and
// alignment; the same pixels per thread, so the same bytes and the same sums. blockIdx.y = sample.
template <bool VEC>
__global__ __launch_bounds__(CHECK_THREADS) void k_stereo_check(CheckArgs a) {
    const unsigned sid = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned W = (unsigned)a.W;
    const int nsteps = (int)((W + CHECK_SCAN - 1) / CHECK_SCAN);
    const bool frames = a.left != nullptr;
    __shared__ float wmin[2][CHECK_THREADS / 64];  // the waves' minima of a step; two sets, so one barrier per step
    unsigned it = 0;                               // steps taken so far: selects the set
    unsigned n_val = 0, n_oov = 0, n_occ = 0, n_cnt = 0, n_mis = 0;
    double se = 0.0, se2 = 0.0;
    const int y_begin = (int)blockIdx.x * a.rows_per, y_end = min(a.H, y_begin + a.rows_per);
    for (int y = y_begin; y < y_end; ++y) {
        const size_t row = ((size_t)sid * a.H + y) * W;  // first pixel of the row
        float carry = INFINITY;                          // min xr over the steps to the right: block-uniform
        for (int k = nsteps - 1; k >= 0; --k, ++it) {
            const unsigned xb = (unsigned)k * CHECK_SCAN + CHECK_PX * tid;  // < W + CHECK_SCAN < 2^32
            const int cnt = xb >= W ? 0 : (VEC ? CHECK_PX : (int)min((unsigned)CHECK_PX, W - xb));
            float d[CHECK_PX] = {0.f, 0.f, 0.f, 0.f};
            if (VEC) {
                if (cnt) {
                    const float4 q = *reinterpret_cast<const float4*>(a.disp + row + xb);
                    d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
                }
            } else {
#pragma unroll
                for (int p = 0; p < CHECK_PX; ++p)
                    if (p < cnt) d[p] = a.disp[row + xb + p];
            }
            bool has[CHECK_PX];
            float xr[CHECK_PX];
#pragma unroll
            for (int p = 0; p < CHECK_PX; ++p) {
                has[p] = p < cnt && d[p] > 0.f && d[p] <= FLT_MAX;  // false for NaN, +-inf, <= 0
                xr[p] = has[p] ? (float)(xb + p) - d[p] : INFINITY;
            }
            // 1. registers: suf[p] = min of the thread's pixels right of p
            float suf[CHECK_PX];
            suf[3] = INFINITY;
            suf[2] = xr[3];
            suf[1] = fminf(xr[2], suf[2]);
            suf[0] = fminf(xr[1], suf[1]);
            // 2. lanes: inclusive suffix minimum over the lanes at and right of this one
            float v = fminf(xr[0], suf[0]);
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float u = __shfl_down(v, o);
                if (lane + o < 64) v = fminf(v, u);
            }
            float ex = __shfl_down(v, 1);  // the lanes strictly right
            if (lane == 63) ex = INFINITY;
            // 3. waves: through LDS
            float* wm = wmin[it & 1];
            if (lane == 0) wm[wave] = v;
            __syncthreads();
            for (unsigned w = wave + 1; w < CHECK_THREADS / 64; ++w) ex = fminf(ex, wm[w]);
            // 4. steps: the carry
            ex = fminf(ex, carry);
            carry = fminf(carry, fminf(fminf(wm[0], wm[1]), fminf(wm[2], wm[3])));

            if (cnt == 0) continue;  // no barrier follows in this step
            uint32_t lw[3] = {0u, 0u, 0u};
            if (VEC && frames) {
                const uint32_t* lp = reinterpret_cast<const uint32_t*>(a.left + (row + xb) * 3);
                lw[0] = lp[0], lw[1] = lp[1], lw[2] = lp[2];
            }
            uint32_t cl[CHECK_PX] = {1u, 1u, 1u, 1u}, col[CHECK_PX] = {0u, 0u, 0u, 0u};
            float rs[CHECK_PX] = {NAN, NAN, NAN, NAN}, dv[CHECK_PX] = {NAN, NAN, NAN, NAN};
#pragma unroll
            for (int p = 0; p < CHECK_PX; ++p) {
                if (!has[p]) continue;
                ++n_val;
                if (xr[p] < 0.f) {
                    cl[p] = 2u, col[p] = 0xff0000u, ++n_oov;  // (0, 0, 255)
                    continue;
                }
                const float m = fminf(ex, suf[p]);
                if (m + a.occ_tol <= xr[p]) {
                    cl[p] = 3u, col[p] = 0x0000ffu, ++n_occ;  // (255, 0, 0)
                    continue;
                }
                cl[p] = 0u;
                if (frames) {
                    // 0 <= xr <= x, so x0 is inside the row; the clamp acts only where float32(x) is not x (W > 2^24)
                    const unsigned x0 = min((unsigned)xr[p], W - 1u), x1 = min(x0 + 1u, W - 1u);
                    const float f = xr[p] - (float)x0;
                    const uint8_t* r0 = a.right + (row + x0) * 3;
                    const uint8_t* r1 = a.right + (row + x1) * 3;
                    float ad[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float ra = (float)r0[c], rb = (float)r1[c];
                        const float r = ra + f * (rb - ra);
                        const int bi = 3 * p + c;
                        const float l = VEC ? (float)((lw[bi >> 2] >> (8 * (bi & 3))) & 0xffu)
                                            : (float)a.left[(row + xb + p) * 3 + c];
                        ad[c] = fabsf(l - r);
                    }
                    const float e = (ad[0] + ad[1]) + ad[2];
                    rs[p] = e;
                    const double e64 = (double)e;
                    ++n_cnt;
                    se += e64;
                    se2 += e64 * e64;
                    if (e > a.photo_thr) {
                        cl[p] = 4u, col[p] = 0x00ffffu, ++n_mis;  // (255, 255, 0)
                    } else {
                        const uint32_t g = (uint32_t)min(255, (int)__fdiv_rn(e, 3.0f));
                        col[p] = g | g << 8 | g << 16;
                    }
                }
                if (cl[p] == 0u) dv[p] = d[p];
            }
            if (VEC) {
                if (a.cls) *reinterpret_cast<uint32_t*>(a.cls + row + xb) = cl[0] | cl[1] << 8 | cl[2] << 16 | cl[3] << 24;
                if (a.resid) *reinterpret_cast<float4*>(a.resid + row + xb) = make_float4(rs[0], rs[1], rs[2], rs[3]);
                if (a.disp_vis)
                    *reinterpret_cast<float4*>(a.disp_vis + row + xb) = make_float4(dv[0], dv[1], dv[2], dv[3]);
                if (a.vis_rgb) st_rgb<4>(a.vis_rgb + (row + xb) * 3, col);
            } else {
#pragma unroll
                for (int p = 0; p < CHECK_PX; ++p) {
                    if (p >= cnt) continue;
                    const size_t i = row + xb + p;
                    if (a.cls) a.cls[i] = (uint8_t)cl[p];
                    if (a.resid) a.resid[i] = rs[p];
                    if (a.disp_vis) a.disp_vis[i] = dv[p];
                    if (a.vis_rgb) st_rgb1(a.vis_rgb + i * 3, col[p]);
                }
            }
        }
    }
    if (a.partial == nullptr) return;  // uniform over the grid
    const double v[7] = {(double)n_val, (double)n_oov, (double)n_occ, (double)n_cnt, se, se2, (double)n_mis};
    block_partial_row<CHECK_THREADS>(v, a.partial + ((size_t)sid * gridDim.x + blockIdx.x) * CHECK_ROW);
}

}  // namespace

extern "C" long long sd_stereo_check_ws_bytes(int n, int H, int W) {
    if (!row_walk::sizes_ok(n, H, W)) return -1;
    return (long long)n * row_walk::blocks(H, W) * CHECK_ROW * (long long)sizeof(double);
}

extern "C" int sd_stereo_check(int n, const float* disp, const uint8_t* left, const uint8_t* right, int H, int W,
                               float occ_tol, float photo_thr, uint8_t* cls, float* resid, float* disp_vis,
                               uint8_t* vis_rgb, double* rows, void* work, sd_stream s) {
    SD_REQUIRE(n >= 1 && n <= 65535, "sd_stereo_check: n = %d samples (1..65535)", n);
    SD_REQUIRE(disp, "sd_stereo_check: null disp");
    SD_REQUIRE(row_walk::sizes_ok(n, H, W), "sd_stereo_check: bad sizes H x W = %d x %d (positive, H * W < 2^31)", H, W);
    SD_REQUIRE((left == nullptr) == (right == nullptr), "sd_stereo_check: left and right: both or neither");
    SD_REQUIRE(resid == nullptr || left != nullptr, "sd_stereo_check: resid needs frames");
    SD_REQUIRE(vis_rgb == nullptr || left != nullptr, "sd_stereo_check: vis_rgb needs frames");
    SD_REQUIRE(cls || resid || disp_vis || vis_rgb || rows, "sd_stereo_check: no output requested");
    SD_REQUIRE(occ_tol >= 0.f && occ_tol <= FLT_MAX, "sd_stereo_check: occ_tol %g (finite and >= 0)", (double)occ_tol);
    SD_REQUIRE(photo_thr == photo_thr, "sd_stereo_check: photo_thr is NaN (+inf for no mismatch class)");
    SD_REQUIRE(rows == nullptr || (work != nullptr && (uintptr_t)work % 8 == 0 && (uintptr_t)rows % 8 == 0),
               "sd_stereo_check: rows need an 8-B aligned work buffer of sd_stereo_check_ws_bytes");
    CheckArgs a;
    a.disp = disp;
    a.left = left;
    a.right = right;
    a.cls = cls;
    a.resid = resid;
    a.disp_vis = disp_vis;
    a.vis_rgb = vis_rgb;
    a.partial = rows ? static_cast<double*>(work) : nullptr;
    a.H = H;
    a.W = W;
    a.rows_per = row_walk::rows_per_block(H, W);
    a.occ_tol = occ_tol;
    a.photo_thr = photo_thr;
    const int nblk = row_walk::blocks(H, W);
    const bool vec = W % 4 == 0 && (uintptr_t)disp % 16 == 0 && (uintptr_t)left % 4 == 0 && (uintptr_t)cls % 4 == 0 &&
                     (uintptr_t)resid % 16 == 0 && (uintptr_t)disp_vis % 16 == 0 && (uintptr_t)vis_rgb % 4 == 0;
    hipStream_t st = to_stream(s);
    const dim3 grid(nblk, n), block(CHECK_THREADS);
    if (vec)
        hipLaunchKernelGGL(k_stereo_check<true>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_stereo_check<false>, grid, block, 0, st, a);
    if (rows)
        hipLaunchKernelGGL((k_rows_sum<CHECK_ROW, row_walk::SUM_THREADS>), dim3(n), dim3(row_walk::SUM_THREADS), 0, st,
                           a.partial, nblk, rows);
    return sd_check_launch("sd_stereo_check");
}
