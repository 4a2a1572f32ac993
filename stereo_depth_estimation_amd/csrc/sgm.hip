// Semi-global matcher of the classical live loop (the reference's live_camera/depth_live.py:158-178: cvtColor,
// cv2.StereoSGBM.compute in 3-way mode, reprojectImageTo3D, nanmedian, normalize), on the device. The algorithm is
// stated in INTEGRATION.md ("The semi-global matcher"); everything up to the int16 disparity is integer arithmetic and
// is pinned bit for bit to the NumPy restatement tests/sgm_ref.py, not to OpenCV's bytes.
//   gray / prefilter : byte streaming kernels
//   cost             : Birchfield-Tomasi pixel cost, bs x bs block sum as a row pass and a column pass -> uint16
//                      C[y][x][d] (d fastest). With the census cost ("The census cost") the
//                      prefilter gives way to a descriptor kernel and the row pass takes the Hamming distance of two
//                      uint64 descriptors as its pixel cost; the column pass and all that follows are shared
//   aggregate        : three scan-line recurrences with d across the 64 lanes of a wave (d = lane + 64 k, k < D / 64
//                      rounded up): top->down writes S, left->right adds to S, right->left keeps its L in registers,
//                      forms the total and does the winner, the right-view disparity and the left-right check in flight.
//                      The 4-, 5- and 8-path modes add bottom->up and the diagonals between the first two, one launch
//                      of k_sgm_walk each (S += L); tests/sgm_modes_ref.py restates them
//   speckle          : union-find over the 4-neighbour graph (atomicMin on parent links), count at the roots, invalidate
//   post             : disparity, fp64 reprojection, min/max on the device, display codes; the centre nanmedian
// Several stereo rigs of one size go through the same launches (sd_sgm_compute_n / _speckle_n / _post_n / _center_n):
// the stream is a grid dimension of these kernels, and the single-stream entry points are their n = 1 case.
// No allocation, no synchronisation: every entry point is graph-capturable. Workspace is the caller's.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "stage_util.h"

// fp64 reprojection and display codes reproduce numpy's separately rounded operations
#pragma clang fp contract(off)

namespace {

constexpr int SGM_INF = 1 << 28;  // "+infinity" of the d +- 1 neighbours outside [0, D) and of the idle lanes
constexpr int SGM_SEG = 32;       // columns per sliding-window segment of the cost kernel
constexpr int SGM_MAX_W = 4096;   // the winner kernel keeps 14 bytes per column (+ 1) in LDS, and x in 12 bits of a key

int sgm_grid(long long work) {
    long long g = (work + 255) / 256;
    if (g > 16384) g = 16384;
    return (int)(g < 1 ? 1 : g);
}
long long align256(long long v) { return (v + 255) / 256 * 256; }
bool sgm_dims_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= INT_MAX / 16; }

struct SgmParams {
    int minD, D, bs, P1, P2, max_diff, uniq, speckle_window, speckle_range, cap;
    int npaths = 3;  // paths summed into S: 3 (3-way), 4 (hh4), 5 (sgbm), 8 (hh)
    int nbits = 0;   // census cost: the descriptor's bits (the pixel cost is 0..nbits); 0: Birchfield-Tomasi
};
// the census windows (rows x columns) and their descriptor bits wh * ww - 1; 0 for any other window
int sgm_census_bits(int wh, int ww) {
    const bool ok = (wh == 3 && ww == 3) || (wh == 5 && ww == 5) || (wh == 7 && ww == 7) || (wh == 7 && ww == 9);
    return ok ? wh * ww - 1 : 0;
}
// the paths of a mode (SD_SGM_MODE_*, cv2's constants), 0 for anything else
int sgm_mode_paths(int mode) {
    switch (mode) {
    case SD_SGM_MODE_3WAY: return 3;
    case SD_SGM_MODE_HH4: return 4;
    case SD_SGM_MODE_SGBM: return 5;
    case SD_SGM_MODE_HH: return 8;
    default: return 0;
    }
}
const char* sgm_params_error(const SgmParams& p) {
    if (p.minD < 0) return "min_disparity must be >= 0";
    if (p.D % 16 != 0 || p.D < 16 || p.D > 256) return "num_disparities must be a multiple of 16 in [16, 256]";
    if (p.bs % 2 == 0 || p.bs < 3 || p.bs > 11) return "block_size must be odd in [3, 11]";
    if (p.cap < 1 || p.cap > 63) return "pre_filter_cap must be in [1, 63]";
    if (p.P1 < 0 || p.P2 < p.P1) return "0 <= P1 <= P2 required";
    if (p.nbits) {  // census: a pixel cost is at most nbits
        if (p.nbits != 8 && p.nbits != 24 && p.nbits != 48 && p.nbits != 62) return "nbits must be 8, 24, 48 or 62";
        if ((long long)p.npaths * ((long long)p.bs * p.bs * p.nbits + p.P2) > 65535)
            return p.npaths == 3   ? "3 * (bs^2 * nbits + P2) exceeds 65535"
                   : p.npaths == 4 ? "4 * (bs^2 * nbits + P2) exceeds 65535 (4 paths)"
                   : p.npaths == 5 ? "5 * (bs^2 * nbits + P2) exceeds 65535 (5 paths)"
                                   : "8 * (bs^2 * nbits + P2) exceeds 65535 (8 paths)";
    } else if ((long long)p.npaths * ((long long)p.bs * p.bs * (2 * p.cap + 63) + p.P2) > 65535)
        return p.npaths == 3   ? "3 * (bs^2 * (2 * cap + 63) + P2) exceeds 65535"
               : p.npaths == 4 ? "4 * (bs^2 * (2 * cap + 63) + P2) exceeds 65535 (4 paths)"
               : p.npaths == 5 ? "5 * (bs^2 * (2 * cap + 63) + P2) exceeds 65535 (5 paths)"
                               : "8 * (bs^2 * (2 * cap + 63) + P2) exceeds 65535 (8 paths)";
    if (p.uniq < 0 || p.uniq > 100) return "uniqueness_ratio must be in [0, 100]";
    if (p.speckle_window < 0 || p.speckle_range < 0 || p.speckle_range > 1024) return "bad speckle parameters";
    return nullptr;
}

// Several streams (stereo rigs) in one launch: the stream is a grid dimension (y, or z where y is taken) and every
// buffer is n slices of the single-stream layout. A kernel folds stream * (elements per slice) into its base pointers
// once, before any loop, from a wave-uniform index: the scan loops keep their instruction count. The fold sits behind
// a branch that stream 0, and so every block of a single-stream launch, skips: the 64-bit scalar multiplies are not
// free in the streaming kernels, where every wave of a CU runs its few instructions at once on one scalar unit.
__device__ __forceinline__ unsigned stream_index(unsigned block) {
    return (unsigned)__builtin_amdgcn_readfirstlane((int)block);
}
// first statement of `if (stream_index(..))`: an empty side effect, so that the body stays behind a branch
__device__ __forceinline__ void stream_branch() { asm volatile(""); }
template <class P> __device__ __forceinline__ void seek_stream(P& p, unsigned sid, long long stride) {  // P: a pointer
    p += (size_t)sid * (size_t)stride;
}
// the scan kernels (one long-lived wave per scan line) fold it without the branch: their prologue is a rounding error
// of their run time, and their main loops compile to what they were
__device__ __forceinline__ size_t stream_off(unsigned block, long long stride) {
    return (size_t)stream_index(block) * (size_t)stride;
}

// ------------------------------------------------------------------ stages 1, 2
__global__ __launch_bounds__(256) void k_sgm_gray(const uint8_t* __restrict__ bgr, int P, uint8_t* __restrict__ g) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
        const uint8_t* q = bgr + (size_t)i * 3;
        g[i] = (uint8_t)((1868 * q[0] + 9617 * q[1] + 4899 * q[2] + 8192) >> 14);
    }
}

__global__ __launch_bounds__(256) void k_sgm_prefilter(const uint8_t* __restrict__ a, int H, int W, int cap,
                                                       uint8_t* __restrict__ out, long long a_stride,
                                                       long long out_stride) {
    const int P = H * W;
    if (const unsigned sid = stream_index(blockIdx.y)) {
        stream_branch();
        seek_stream(a, sid, a_stride), seek_stream(out, sid, out_stride);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
        const int y = i / W, x = i - y * W;
        const int xm = max(x - 1, 0), xp = min(x + 1, W - 1);
        const uint8_t* r0 = a + (size_t)max(y - 1, 0) * W;
        const uint8_t* r1 = a + (size_t)y * W;
        const uint8_t* r2 = a + (size_t)min(y + 1, H - 1) * W;
        const int s = 2 * ((int)r1[xp] - (int)r1[xm]) + ((int)r0[xp] - (int)r0[xm]) + ((int)r2[xp] - (int)r2[xm]);
        out[i] = (uint8_t)(min(max(s, -cap), cap) + cap);
    }
}

// ------------------------------------------------------------------ stage 2c (census cost)
// The census descriptor of every pixel of a gray plane ("The census cost", step 2c): bit k is set where
// the k-th window position, row-major without the centre, holds a value strictly below the centre's; positions outside
// the image take the nearest pixel of the same image. Block: a tile of 64 columns x 16 rows, staged with its halo in
// LDS (clamped to the image there, so the descriptor loop has no bounds). A wave walks a row: its 64 lanes read 64
// adjacent bytes of one LDS row, 16 or 17 dwords in as many banks, the four lanes of a dword one broadcast. Each
// thread builds the descriptors of four rows (ty, ty + 4, ...) from LDS alone and stores 8 bytes per pixel.
constexpr int CENSUS_TW = 64, CENSUS_TH = 16;
template <int WH, int WW>
__global__ __launch_bounds__(256) void k_sgm_census(const uint8_t* __restrict__ g, int H, int W,
                                                    unsigned long long* __restrict__ desc, long long img_stride,
                                                    long long desc_stride) {
    constexpr int RY = WH / 2, RX = WW / 2, LH = CENSUS_TH + 2 * RY, LW = CENSUS_TW + 2 * RX;
    __shared__ unsigned char tile[LH][LW];
    if (const unsigned sid = stream_index(blockIdx.z)) {
        stream_branch();
        seek_stream(g, sid, img_stride), seek_stream(desc, sid, desc_stride);
    }
    const int x0 = blockIdx.x * CENSUS_TW, y0 = blockIdx.y * CENSUS_TH;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = min(max(y0 + ly - RY, 0), H - 1), gx = min(max(x0 + lx - RX, 0), W - 1);
        tile[ly][lx] = g[(size_t)gy * W + gx];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, x = x0 + lane;
    if (x >= W) return;
#pragma unroll
    for (int j = 0; j < CENSUS_TH / 4; ++j) {
        const int ly = (threadIdx.x >> 6) + 4 * j, y = y0 + ly;
        if (y >= H) break;
        const unsigned c = tile[ly + RY][lane + RX];
        unsigned lo = 0, hi = 0;  // bits 0..31 and 32..63: the shifts are compile-time constants
#pragma unroll
        for (int dy = 0; dy < WH; ++dy)
#pragma unroll
            for (int dx = 0; dx < WW; ++dx) {
                if (dy == RY && dx == RX) continue;
                const int k = dy * WW + dx - (dy * WW + dx > RY * WW + RX ? 1 : 0);
                const unsigned below = tile[ly + dy][lane + dx] < c ? 1u : 0u;
                if (k < 32)
                    lo |= below << k;
                else
                    hi |= below << (k - 32);
            }
        desc[(size_t)y * W + x] = (unsigned long long)hi << 32 | lo;
    }
}

// ------------------------------------------------------------------ stages 3, 4
__device__ __forceinline__ void bt_terms(const uint8_t* __restrict__ row, int x, int W, int& u, int& u0, int& u1) {
    u = row[x];
    const int l = row[max(x - 1, 0)], r = row[min(x + 1, W - 1)];
    const int ul = (u + l) >> 1, ur = (u + r) >> 1;
    u0 = min(u, min(ul, ur));
    u1 = max(u, max(ul, ur));
}
__device__ __forceinline__ int bt_plane(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int W, int x, int xr) {
    int u, u0, u1, v, v0, v1;
    bt_terms(a, x, W, u, u0, u1);
    bt_terms(b, xr, W, v, v0, v1);
    return min(max(0, max(u - v1, v0 - u)), max(0, max(v - u1, u0 - v)));
}
// The block sum is separable: one kernel sums the pixel costs over the bs columns of the window, row by row, into a
// scratch volume; a second sums bs rows of that. Each evaluates or loads what enters the window and what leaves it,
// not the window.
//
// Rows: block (segment group, row y), 256 threads = 256 / D segments of SGM_SEG columns x D disparities. A thread
// slides the bs-wide window of its (segment, d) along x: the pixel costs inside the window live in a ring in LDS
// (private to the thread: no barrier), their sum in a register. Lanes run along d: 2-byte stores, 128 B per wave.
//
// The pixel cost is the kernel's template parameter: the planes it reads, as kernel arguments, and value(cx, xr), the
// cost of left column cx against right column xr of the block's row. Both costs are at most 255, the ring's bytes.
// A cost reads the gray planes, a second kind of plane of its own ("side" planes), or both: seek() moves its pointers to
// stream sid given the distance between the streams' gray planes and between their side planes, each in elements of
// the plane. The host takes the second distance from cost_side_stride() below, per cost type, never from the caller.
struct CostBT {  // step 3: Birchfield-Tomasi of the prefiltered planes + that of the gray planes >> 2
    const uint8_t *__restrict__ gl, *__restrict__ gr, *__restrict__ pl, *__restrict__ pr;
    __device__ __forceinline__ void seek(unsigned sid, long long img_stride, long long side_stride) {  // side: pl, pr
        seek_stream(gl, sid, img_stride), seek_stream(gr, sid, img_stride);
        seek_stream(pl, sid, side_stride), seek_stream(pr, sid, side_stride);
    }
    __device__ __forceinline__ void row(size_t o) { gl += o, gr += o, pl += o, pr += o; }
    __device__ __forceinline__ int value(int W, int cx, int xr) const {
        return bt_plane(pl, pr, W, cx, xr) + (bt_plane(gl, gr, W, cx, xr) >> 2);
    }
};
// step 3c: the Hamming distance of the two census descriptors. cx is uniform over the d lanes of a segment (one
// address, broadcast); xr = cx - d - minD runs contiguously along d: 8 bytes per lane, whole cache lines per wave.
struct CostCensus {
    const unsigned long long *__restrict__ cl, *__restrict__ cr;
    __device__ __forceinline__ void seek(unsigned sid, long long, long long side_stride) {  // side: cl, cr; no gray
        seek_stream(cl, sid, side_stride), seek_stream(cr, sid, side_stride);
    }
    __device__ __forceinline__ void row(size_t o) { cl += o, cr += o; }
    __device__ __forceinline__ int value(int, int cx, int xr) const { return __popcll(cl[cx] ^ cr[xr]); }
};
template <class Cost>
__global__ __launch_bounds__(256) void k_sgm_cost_rows(Cost cost, int W, int minD, int D, int bs,
                                                       uint16_t* __restrict__ Hs, long long img_stride,
                                                       long long side_stride, long long vol_stride) {
    __shared__ unsigned char ring[11][256];
    const int tid = threadIdx.x, spb = 256 / D, seg = tid / D, d = tid - seg * D;
    if (seg >= spb) return;
    const int maxD = minD + D, y = blockIdx.y, r = bs / 2;
    const int xs = maxD + (blockIdx.x * spb + seg) * SGM_SEG;
    if (xs >= W) return;
    const int xe = min(xs + SGM_SEG, W);
    if (const unsigned sid = stream_index(blockIdx.z)) {
        stream_branch();
        cost.seek(sid, img_stride, side_stride), seek_stream(Hs, sid, vol_stride);
    }
    const size_t o = (size_t)y * W;
    cost.row(o);
    int sum = 0, last_cx = -1, last_val = 0, slot = 0;
    for (int pos = xs - r; pos <= xs + r; ++pos) {
        const int cx = min(max(pos, maxD), W - 1), xr = cx - d - minD;
        if (cx != last_cx) last_val = cost.value(W, cx, xr);
        last_cx = cx;
        ring[slot][tid] = (unsigned char)last_val;
        sum += last_val;
        slot = slot + 1 == bs ? 0 : slot + 1;
    }
    uint16_t* out = Hs + o * D + d;
    out[(size_t)xs * D] = (uint16_t)sum;
    for (int x = xs + 1; x < xe; ++x) {  // slot: the column that leaves (x - r - 1), replaced by the one that enters
        const int cx = min(x + r, W - 1), xr = cx - d - minD;
        if (cx != last_cx) last_val = cost.value(W, cx, xr);
        last_cx = cx;
        sum += last_val - (int)ring[slot][tid];
        ring[slot][tid] = (unsigned char)last_val;
        slot = slot + 1 == bs ? 0 : slot + 1;
        out[(size_t)x * D] = (uint16_t)sum;
    }
}

// Columns: a thread owns four adjacent d of one x (8-byte accesses; D is a multiple of 16, so the (W - maxD) * D
// values of a row are contiguous and 32-byte aligned) over SGM_YSEG rows, and slides the bs-high window down: add the
// row that enters, subtract the one that leaves (re-read: it was loaded bs rows ago and is still in L2).
constexpr int SGM_YSEG = 32;
__device__ __forceinline__ void ld4(const uint16_t* p, int (&v)[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = t.x & 0xffff, v[1] = t.x >> 16, v[2] = t.y & 0xffff, v[3] = t.y >> 16;
}
__global__ __launch_bounds__(256) void k_sgm_cost_cols(const uint16_t* __restrict__ Hs, int H, int W, int maxD, int D,
                                                       int bs, uint16_t* __restrict__ C, long long vol_stride) {
    const long long n = (long long)(W - maxD) * D, e = 4ll * (blockIdx.x * 256 + threadIdx.x);
    if (e >= n) return;
    if (const unsigned sid = stream_index(blockIdx.z)) {
        stream_branch();
        seek_stream(Hs, sid, vol_stride), seek_stream(C, sid, vol_stride);
    }
    const size_t pitch = (size_t)W * D, base = (size_t)maxD * D + e;
    const int r = bs / 2, ys = blockIdx.y * SGM_YSEG, ye = min(ys + SGM_YSEG, H);
    int sum[4] = {0, 0, 0, 0}, v[4], w[4];
    for (int dy = -r; dy <= r; ++dy) {
        ld4(Hs + (size_t)min(max(ys + dy, 0), H - 1) * pitch + base, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[k] += v[k];
    }
    for (int y = ys;;) {
        *reinterpret_cast<uint2*>(C + (size_t)y * pitch + base) =
            make_uint2((unsigned)sum[0] | (unsigned)sum[1] << 16, (unsigned)sum[2] | (unsigned)sum[3] << 16);
        if (++y >= ye) break;
        ld4(Hs + (size_t)min(y + r, H - 1) * pitch + base, v);
        ld4(Hs + (size_t)max(y - r - 1, 0) * pitch + base, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[k] += v[k] - w[k];
    }
}

// ------------------------------------------------------------------ stage 5
// A pixel's D values across one wave: lane holds d = lane + 64 k, k < NK; idle slots (d >= D) hold SGM_INF.
// Cross-lane traffic is DPP (register to register), not LDS permutes: the recurrence is one dependent chain per scan
// line, so the latency of the minimum and of the d +- 1 neighbours is the step time. All 64 lanes are always active.
template <int CTRL> __device__ __forceinline__ int dpp_mov(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E;            // quad_perm [1,0,3,2], [2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;  // lane i <- 7 - i within 8, i <- 15 - i within 16
constexpr int DPP_WAVE_ROL1 = 0x134, DPP_WAVE_ROR1 = 0x13C; // lane i <- i + 1 (63 <- 0), lane i <- i - 1 (0 <- 63)
__device__ __forceinline__ int wave_min(int m) {
    m = min(m, dpp_mov<DPP_XOR1>(m));
    m = min(m, dpp_mov<DPP_XOR2>(m));
    m = min(m, dpp_mov<DPP_HALF_MIRROR>(m));
    m = min(m, dpp_mov<DPP_MIRROR>(m));  // every lane: the minimum of its row of 16
    return min(min(__builtin_amdgcn_readlane(m, 0), __builtin_amdgcn_readlane(m, 16)),
               min(__builtin_amdgcn_readlane(m, 32), __builtin_amdgcn_readlane(m, 48)));
}
// FULL: D == 64 NK, no idle slots (the app's 128), so no predicate anywhere. Otherwise idle slots load a valid
// address (d clamped) and are overwritten with SGM_INF.
template <int NK, bool FULL>
__device__ __forceinline__ void ld_vol(const uint16_t* __restrict__ p, int lane, int D, int (&v)[NK]) {
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = (int)p[FULL ? lane + 64 * k : min(lane + 64 * k, D - 1)];
}
template <int NK, bool FULL>
__device__ __forceinline__ void st_vol(uint16_t* __restrict__ p, int lane, int D, const int (&v)[NK]) {
#pragma unroll
    for (int k = 0; k < NK; ++k)
        if (FULL || lane + 64 * k < D) p[lane + 64 * k] = (uint16_t)v[k];
}
// L = 0 before the first pixel of a path makes the general step give L = C there: m = 0 and min(0, P1, P1, P2) = 0
// (P1, P2 >= 0). So a path has no special first step.
template <int NK, bool FULL> __device__ __forceinline__ void path_init(int (&L)[NK], int lane, int D) {
#pragma unroll
    for (int k = 0; k < NK; ++k) L[k] = (FULL || lane + 64 * k < D) ? 0 : SGM_INF;
}
// L(p, d) = C(p, d) + min(L(q, d), L(q, d - 1) + P1, L(q, d + 1) + P1, m(q) + P2) - m(q), L in place
template <int NK, bool FULL>
__device__ __forceinline__ void path_step(int (&L)[NK], const int (&c)[NK], int lane, int D, int P1, int P2) {
    int m = L[0];
#pragma unroll
    for (int k = 1; k < NK; ++k) m = min(m, L[k]);
    m = wave_min(m);
    int tm[NK], tp[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        tm[k] = dpp_mov<DPP_WAVE_ROR1>(L[k]);  // lane - 1 (lane 0: lane 63)
        tp[k] = dpp_mov<DPP_WAVE_ROL1>(L[k]);  // lane + 1 (lane 63: lane 0)
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int dn = lane == 0 ? (k > 0 ? tm[k > 0 ? k - 1 : 0] : SGM_INF) : tm[k];
        const int up = lane == 63 ? (k < NK - 1 ? tp[k < NK - 1 ? k + 1 : k] : SGM_INF) : tp[k];
        const int v = c[k] + min(min(L[k], dn + P1), min(up + P1, m + P2)) - m;
        L[k] = (FULL || lane + 64 * k < D) ? v : SGM_INF;
    }
}

// The loads of a scan line do not depend on its chain: they run SGM_PF steps ahead in a ring of registers, so a
// step waits for the recurrence, not for memory. The main loop is SGM_PF whole steps of straight-line code (ring slot
// j reloaded, unconditionally, with step t + SGM_PF clamped to the last one, so that s_waitcnt can count exactly);
// the last n % SGM_PF steps find their data in the ring.
constexpr int SGM_PF = 8;

// top -> down: one wave per column x >= maxD, four adjacent columns per block; S = L
template <int NK, bool FULL>
__global__ __launch_bounds__(256) void k_sgm_down(const uint16_t* __restrict__ C, int H, int W, int maxD, int D, int P1,
                                                  int P2, uint16_t* __restrict__ S, long long vol_stride) {
    const int lane = threadIdx.x & 63, x = maxD + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= W) return;
    const size_t pitch = (size_t)W * D, so = stream_off(blockIdx.y, vol_stride);
    const uint16_t* c = C + so + (size_t)x * D;
    uint16_t* s = S + so + (size_t)x * D;
    int L[NK], ring[SGM_PF][NK];
    path_init<NK, FULL>(L, lane, D);
#pragma unroll
    for (int j = 0; j < SGM_PF; ++j) ld_vol<NK, FULL>(c + (size_t)min(j, H - 1) * pitch, lane, D, ring[j]);
    int y = 0;
    for (; y + SGM_PF <= H; y += SGM_PF) {
#pragma unroll
        for (int j = 0; j < SGM_PF; ++j) {
            int cc[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) cc[k] = ring[j][k];
            ld_vol<NK, FULL>(c + (size_t)min(y + j + SGM_PF, H - 1) * pitch, lane, D, ring[j]);
            path_step<NK, FULL>(L, cc, lane, D, P1, P2);
            st_vol<NK, FULL>(s + (size_t)(y + j) * pitch, lane, D, L);
        }
    }
#pragma unroll
    for (int j = 0; j < SGM_PF; ++j)
        if (y + j < H) {
            path_step<NK, FULL>(L, ring[j], lane, D, P1, P2);
            st_vol<NK, FULL>(s + (size_t)(y + j) * pitch, lane, D, L);
        }
}

// left -> right: one wave per row; S += L
template <int NK, bool FULL>
__global__ __launch_bounds__(64) void k_sgm_right(const uint16_t* __restrict__ C, int W, int maxD, int D, int P1, int P2,
                                                  uint16_t* __restrict__ S, long long vol_stride) {
    const int lane = threadIdx.x, n = W - maxD;
    const size_t row = stream_off(blockIdx.y, vol_stride) + ((size_t)blockIdx.x * W + maxD) * D;
    const uint16_t* c = C + row;
    uint16_t* s = S + row;
    int L[NK], rc[SGM_PF][NK], rs[SGM_PF][NK];
    path_init<NK, FULL>(L, lane, D);
#pragma unroll
    for (int j = 0; j < SGM_PF; ++j) {
        ld_vol<NK, FULL>(c + (size_t)min(j, n - 1) * D, lane, D, rc[j]);
        ld_vol<NK, FULL>(s + (size_t)min(j, n - 1) * D, lane, D, rs[j]);
    }
    int t = 0;
    for (; t + SGM_PF <= n; t += SGM_PF) {
#pragma unroll
        for (int j = 0; j < SGM_PF; ++j) {
            int cc[NK], sc[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                cc[k] = rc[j][k];
                sc[k] = rs[j][k];
            }
            // the S of step t + SGM_PF is read before any store to it: stores reach step t + j only
            ld_vol<NK, FULL>(c + (size_t)min(t + j + SGM_PF, n - 1) * D, lane, D, rc[j]);
            ld_vol<NK, FULL>(s + (size_t)min(t + j + SGM_PF, n - 1) * D, lane, D, rs[j]);
            path_step<NK, FULL>(L, cc, lane, D, P1, P2);
#pragma unroll
            for (int k = 0; k < NK; ++k) sc[k] += L[k];
            st_vol<NK, FULL>(s + (size_t)(t + j) * D, lane, D, sc);
        }
    }
#pragma unroll
    for (int j = 0; j < SGM_PF; ++j)
        if (t + j < n) {
            int sc[NK];
            path_step<NK, FULL>(L, rc[j], lane, D, P1, P2);
#pragma unroll
            for (int k = 0; k < NK; ++k) sc[k] = rs[j][k] + L[k];
            st_vol<NK, FULL>(s + (size_t)(t + j) * D, lane, D, sc);
        }
}

// The further paths of the 4-, 5- and 8-path modes, and any single path of sd_sgm_aggregate_dir: one wave per scan
// line, walking (y, x) += (dy, dx) with x taken modulo n = W - maxD. Vertical family (dy = +-1): wave c starts in column
// c of the first (last) row and takes T = H steps, so at every step the n waves cover the n columns of one row once, a
// diagonal that leaves the image on one side re-enters on the other as a new path (L back to the path-start state),
// and no wave ever needs another's L. Left -> right (dy = 0, dx = 1): wave r walks row r, T = n. Each pixel is visited
// once per launch, by one wave, so S = L or S += L is a plain store and the S of step t + SGM_PF can be read ahead.
// One wave alone on its SIMD issues an instruction every four cycles, scalar ones included, so the walk is kept to a
// few scalar instructions per step: a cursor is a 64-bit element offset that advances by one of two precomputed
// increments (a plain move, or one that wraps in x) and the column it is in. The ring's cursor stops on the last step,
// as the clamped reloads of the other passes do.
struct SgmWalk {  // wave-uniform constants of a launch
    long long inc, inc_wrap;
    int dx, wrap_at, wrap_to;
};
struct SgmCursor {
    long long off;
    int x;
};
__device__ __forceinline__ void walk_advance(SgmCursor& c, const SgmWalk& w, bool go) {
    const int nx = c.x + w.dx;
    const bool wrap = nx == w.wrap_at;
    const long long inc = wrap ? w.inc_wrap : w.inc;
    c.off += go ? inc : 0;
    c.x = go ? (wrap ? w.wrap_to : nx) : c.x;
}
template <int NK, bool FULL, bool ACC>
__global__ __launch_bounds__(256) void k_sgm_walk(const uint16_t* __restrict__ C, int H, int W, int maxD, int D, int P1,
                                                  int P2, int dy, int dx, int lines, int T, uint16_t* __restrict__ S,
                                                  long long vol_stride) {
    const int lane = threadIdx.x & 63;
    const int line = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (line >= lines) return;
    const int n = W - maxD;
    const long long pitch = (long long)W * D;
    const size_t so = stream_off(blockIdx.y, vol_stride) + (size_t)maxD * D;
    const uint16_t* c = C + so;
    uint16_t* s = S + so;
    SgmWalk w;
    w.dx = dx;
    w.inc = dy * pitch + dx * D;
    w.inc_wrap = w.inc - dx * (long long)n * D;
    w.wrap_at = dx > 0 ? n : -1;  // dx == 0: never reached
    w.wrap_to = dx > 0 ? 0 : n - 1;
    const int y0 = dy == 0 ? line : (dy > 0 ? 0 : H - 1), x0 = dy == 0 ? 0 : line;
    const SgmCursor first = {y0 * pitch + (long long)x0 * D, x0};
    const int xstart = dx > 0 ? 0 : (dx < 0 ? n - 1 : -1);  // the column in which a path that moves along x starts
    int L[NK], L0[NK], rc[SGM_PF][NK], rs[ACC ? SGM_PF : 1][NK];
    path_init<NK, FULL>(L0, lane, D);
#pragma unroll
    for (int k = 0; k < NK; ++k) L[k] = L0[k];
    // the cursor runs SGM_PF steps ahead, with the loads; a step finds its own offset and column where its loads were
    // issued from, in a ring of scalars (static slots of the unrolled loop: registers)
    SgmCursor ld = first;
    long long roff[SGM_PF];
    int rx[SGM_PF];
#pragma unroll
    for (int j = 0; j < SGM_PF; ++j) {
        ld_vol<NK, FULL>(c + ld.off, lane, D, rc[j]);
        if (ACC) ld_vol<NK, FULL>(s + ld.off, lane, D, rs[j]);
        roff[j] = ld.off, rx[j] = ld.x;
        walk_advance(ld, w, j + 1 < T);
    }
    int t = 0;
    for (; t + SGM_PF <= T; t += SGM_PF) {
#pragma unroll
        for (int j = 0; j < SGM_PF; ++j) {
            int cc[NK], sc[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                cc[k] = rc[j][k];
                sc[k] = ACC ? rs[ACC ? j : 0][k] : 0;
            }
            const long long off = roff[j];
            const bool start = rx[j] == xstart;
            ld_vol<NK, FULL>(c + ld.off, lane, D, rc[j]);
            if (ACC) ld_vol<NK, FULL>(s + ld.off, lane, D, rs[ACC ? j : 0]);
            roff[j] = ld.off, rx[j] = ld.x;
            walk_advance(ld, w, t + j + SGM_PF + 1 < T);
#pragma unroll
            for (int k = 0; k < NK; ++k) L[k] = start ? L0[k] : L[k];
            path_step<NK, FULL>(L, cc, lane, D, P1, P2);
#pragma unroll
            for (int k = 0; k < NK; ++k) sc[k] += L[k];
            st_vol<NK, FULL>(s + off, lane, D, sc);
        }
    }
#pragma unroll
    for (int j = 0; j < SGM_PF; ++j)
        if (t + j < T) {
            int sc[NK];
            const bool start = rx[j] == xstart;
#pragma unroll
            for (int k = 0; k < NK; ++k) L[k] = start ? L0[k] : L[k];
            path_step<NK, FULL>(L, rc[j], lane, D, P1, P2);
#pragma unroll
            for (int k = 0; k < NK; ++k) sc[k] = (ACC ? rs[ACC ? j : 0][k] : 0) + L[k];
            st_vol<NK, FULL>(s + roff[j], lane, D, sc);
        }
}

// ------------------------------------------------------------------ stages 5 (third path), 6, 7
// right -> left: one wave (= one workgroup) per row, x descending. The total S = S + L stays in registers. In the scan
// loop only what needs the whole wave happens per pixel: the minimum, its lowest d, the uniqueness test and the two
// neighbours of the minimum; lane 0 leaves them in LDS. After the scan the row is finished 64 pixels at a time:
//   - the sub-pixel value;
//   - the right view. "x descending, replace when strictly lower" picks, for each right pixel x2, the candidate of
//     the lowest minS and among equals the largest x: an LDS atomicMin over the key minS << 12 | (4095 - x), from
//     which x (and so disp2 = x - x2) is read back. No key: disp2 = minD - 1;
//   - after a barrier, the left-right check.
constexpr int SGM_KEY_NONE = 0x7fffffff;
// what the scan loop leaves per pixel, in LDS ([W + 1] each: slot W takes the loop's first, empty, call)
struct SgmRow {
    unsigned short *mn, *sm, *sp;
    short* best;  // -1: failed the uniqueness test
};
// The winner of one pixel from its total costs `st` (idle slots hold SGM_INF): the minimum, its lowest d, the
// uniqueness verdict and the minimum's two neighbours. Everything is wave-uniform; lane 0 stores.
template <int NK>
__device__ __forceinline__ void winner_px(const int (&st)[NK], int x, int lane, int D, int uniq, const SgmRow& r) {
    int mn = st[0];
#pragma unroll
    for (int k = 1; k < NK; ++k) mn = min(mn, st[k]);
    mn = wave_min(mn);
    int best = -1;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const unsigned long long hit = __ballot(st[k] == mn);
        if (best < 0 && hit) best = 64 * k + __ffsll((long long)hit) - 1;
    }
    best = __builtin_amdgcn_readfirstlane(best);
    bool far_low = false;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int d = lane + 64 * k;
        far_low |= d < D && abs(d - best) > 1 && st[k] * (100 - uniq) < mn * 100;
    }
    const bool bad = __any(far_low);
    const int dm = max(best - 1, 0), dp = min(best + 1, D - 1);
    int sm = 0, sp = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int a = __builtin_amdgcn_readlane(st[k], dm & 63), b = __builtin_amdgcn_readlane(st[k], dp & 63);
        if ((dm >> 6) == k) sm = a;
        if ((dp >> 6) == k) sp = b;
    }
    if (lane == 0) {
        r.mn[x] = (unsigned short)mn;
        r.sm[x] = (unsigned short)sm;
        r.sp[x] = (unsigned short)sp;
        r.best[x] = (short)(bad ? -1 : best);
    }
}

template <int NK, bool FULL, bool TOTAL>
__global__ __launch_bounds__(64) void k_sgm_left(const uint16_t* __restrict__ C, const uint16_t* __restrict__ S, int W,
                                                 int minD, int D, int P1, int P2, int uniq, int max_diff,
                                                 uint16_t* __restrict__ S_total, int16_t* __restrict__ q_raw,
                                                 int16_t* __restrict__ q_out, long long vol_stride,
                                                 long long img_stride) {
    extern __shared__ int sgm_lds[];
    int* key2 = sgm_lds;  // [W + 1]
    SgmRow row_lds;
    row_lds.mn = reinterpret_cast<unsigned short*>(sgm_lds + W + 1);
    row_lds.sm = row_lds.mn + W + 1;
    row_lds.sp = row_lds.sm + W + 1;
    row_lds.best = reinterpret_cast<short*>(row_lds.sp + W + 1);
    short* qrow = row_lds.best + W + 1;
    const unsigned short *r_mn = row_lds.mn, *r_sm = row_lds.sm, *r_sp = row_lds.sp;
    const short* r_best = row_lds.best;
    const int lane = threadIdx.x, maxD = minD + D, y = blockIdx.x, n = W - maxD;
    const int invalid = 16 * (minD - 1);
    for (int x = lane; x < W; x += 64) key2[x] = SGM_KEY_NONE;
    if (n > 0) {
        // scan step t is pixel x = W - 1 - t. The winner of pixel t - 1 is taken inside the step of pixel t: two
        // independent instruction streams in one basic block. The first call works on zeros and stores to slot W.
        const size_t row = stream_off(blockIdx.y, vol_stride) + ((size_t)y * W + (W - 1)) * D;  // step 0, this stream
        const uint16_t* c = C + row;
        const uint16_t* s = S + row;
        int L[NK], prev[NK], rc[SGM_PF][NK], rs[SGM_PF][NK];
        path_init<NK, FULL>(L, lane, D);
#pragma unroll
        for (int k = 0; k < NK; ++k) prev[k] = L[k];
#pragma unroll
        for (int j = 0; j < SGM_PF; ++j) {
            ld_vol<NK, FULL>(c - (size_t)min(j, n - 1) * D, lane, D, rc[j]);
            ld_vol<NK, FULL>(s - (size_t)min(j, n - 1) * D, lane, D, rs[j]);
        }
        int t = 0;
        for (; t + SGM_PF <= n; t += SGM_PF) {
#pragma unroll
            for (int j = 0; j < SGM_PF; ++j) {
                int cc[NK], st[NK];
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    cc[k] = rc[j][k];
                    st[k] = rs[j][k];
                }
                ld_vol<NK, FULL>(c - (size_t)min(t + j + SGM_PF, n - 1) * D, lane, D, rc[j]);
                ld_vol<NK, FULL>(s - (size_t)min(t + j + SGM_PF, n - 1) * D, lane, D, rs[j]);
                path_step<NK, FULL>(L, cc, lane, D, P1, P2);
                winner_px<NK>(prev, W - (t + j), lane, D, uniq, row_lds);
#pragma unroll
                for (int k = 0; k < NK; ++k) prev[k] = (FULL || lane + 64 * k < D) ? st[k] + L[k] : SGM_INF;
                if (TOTAL) st_vol<NK, FULL>(S_total + row - (size_t)(t + j) * D, lane, D, prev);
            }
        }
#pragma unroll
        for (int j = 0; j < SGM_PF; ++j)
            if (t + j < n) {
                path_step<NK, FULL>(L, rc[j], lane, D, P1, P2);
                winner_px<NK>(prev, W - (t + j), lane, D, uniq, row_lds);
#pragma unroll
                for (int k = 0; k < NK; ++k) prev[k] = (FULL || lane + 64 * k < D) ? rs[j][k] + L[k] : SGM_INF;
                if (TOTAL) st_vol<NK, FULL>(S_total + row - (size_t)(t + j) * D, lane, D, prev);
            }
        winner_px<NK>(prev, maxD, lane, D, uniq, row_lds);
    }
    __syncthreads();
    {  // the disparity maps are not touched by the scan: their stream offset is folded in here, after it
        const size_t qo = stream_off(blockIdx.y, img_stride);
        q_out += qo;
        if (q_raw) q_raw += qo;
    }
    for (int x = lane; x < W; x += 64) {
        int q = invalid;
        if (x >= maxD && r_best[x] >= 0) {
            const int best = r_best[x], mn = r_mn[x], sm = r_sm[x], sp = r_sp[x];
            atomicMin(key2 + (x - best - minD), (mn << 12) | (4095 - x));
            q = 16 * best;
            if (best > 0 && best < D - 1) {
                const int den = max(sm + sp - 2 * mn, 1);
                q += ((sm - sp) * 16 + den) / (2 * den);
            }
            q += 16 * minD;
        }
        qrow[x] = (short)q;
    }
    __syncthreads();
    for (int x = lane; x < W; x += 64) {
        int q = qrow[x];
        if (q_raw) q_raw[(size_t)y * W + x] = (int16_t)q;
        if (q != invalid && max_diff >= 0) {
            bool fail[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int dv = (q + 15 * i) >> 4, xx = x - dv;
                fail[i] = false;
                if (xx >= 0 && xx < W) {
                    const int key = key2[xx];
                    // disp2[xx] = (the winning candidate's x) - xx >= minD when there is one
                    fail[i] = key != SGM_KEY_NONE && abs((4095 - (key & 4095)) - xx - dv) > max_diff;
                }
            }
            if (fail[0] && fail[1]) q = invalid;
        }
        q_out[(size_t)y * W + x] = (int16_t)q;
    }
}

// ------------------------------------------------------------------ stage 8
// Union-find over the pixels: parent[i] <= i always (links only ever decrease, by atomicMin), so every walk follows
// strictly decreasing indices and ends at a root on its own; no loop waits for another thread.
__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int uf_find(const int* parent, int i) {
    for (;;) {
        const int n = uf_load(parent + i);
        if (n >= i) return i;
        i = n;
    }
}
// the same walk, shortening the path behind it (a node is re-pointed at its grandparent: still an ancestor, lower)
__device__ __forceinline__ int uf_find_halve(int* parent, int i) {
    for (;;) {
        const int n = uf_load(parent + i);
        if (n >= i) return i;
        const int g = uf_load(parent + n);
        if (g < n) atomicMin(parent + i, g);
        i = n;
    }
}
// a + b strictly decreases in every iteration that does not finish
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
    for (;;) {
        a = uf_find_halve(parent, a);
        b = uf_find_halve(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);  // a > b
        if (old == a) return;
        a = old;
    }
}
__device__ __forceinline__ bool sp_joined(int a, int b, int invalid, int lim) {
    return a != invalid && b != invalid && abs(a - b) <= lim;
}
// One wave per 64 pixels of a row: every pixel starts linked to the first pixel of its horizontal run inside the
// segment (the highest run start at or below the lane, from one ballot), so most horizontal unions never happen.
__global__ __launch_bounds__(256) void k_speckle_init(const int16_t* __restrict__ q, int H, int W, int invalid, int lim,
                                                      int* __restrict__ parent, int* __restrict__ count,
                                                      long long img_stride, long long work_stride) {
    const int lane = threadIdx.x & 63, nseg = (W + 63) / 64, total = H * nseg;
    if (const unsigned sid = stream_index(blockIdx.y)) {
        stream_branch();
        seek_stream(q, sid, img_stride), seek_stream(parent, sid, work_stride), seek_stream(count, sid, work_stride);
    }
    for (int w = blockIdx.x * 4 + (threadIdx.x >> 6); w < total; w += gridDim.x * 4) {
        const int y = w / nseg, x = (w - y * nseg) * 64 + lane;
        const bool in = x < W;
        const int i = y * W + x;
        const int v = in ? (int)q[i] : invalid;
        const int left = __shfl_up(v, 1);
        const bool conn = lane > 0 && sp_joined(v, left, invalid, lim);
        const unsigned long long starts = __ballot(!conn);  // bit 0 is always set
        const unsigned long long below = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
        const int start = 63 - __clzll((long long)(starts & below));
        if (in) {
            parent[i] = i - (lane - start);
            count[i] = 0;
        }
    }
}
// The remaining edges: horizontal ones across a segment boundary, and vertical ones, except where the edge one
// column to the left joins the same two runs (its own union, or by induction the one further left, covers it).
__global__ __launch_bounds__(256) void k_speckle_link(const int16_t* __restrict__ q, int H, int W, int invalid, int lim,
                                                      int* parent, long long img_stride, long long work_stride) {
    const int P = H * W;
    if (const unsigned sid = stream_index(blockIdx.y)) {
        stream_branch();
        seek_stream(q, sid, img_stride), seek_stream(parent, sid, work_stride);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
        const int v = q[i];
        if (v == invalid) continue;
        const int y = i / W, x = i - y * W;
        const int l = x > 0 ? (int)q[i - 1] : invalid;
        if ((x & 63) == 0 && sp_joined(v, l, invalid, lim)) uf_union(parent, i, i - 1);
        if (y + 1 < H) {
            const int n = q[i + W];
            if (sp_joined(v, n, invalid, lim)) {
                const int ln = x > 0 ? (int)q[i + W - 1] : invalid;
                const bool covered = sp_joined(v, l, invalid, lim) && sp_joined(n, ln, invalid, lim) && sp_joined(l, ln, invalid, lim);
                if (!covered) uf_union(parent, i, i + W);
            }
        }
    }
}
// after the links are final: the root of every valid pixel (stored back: a plain shortening of its own path) and the
// component sizes at the roots, one atomicAdd per distinct root of a wave
__global__ __launch_bounds__(256) void k_speckle_count(const int16_t* __restrict__ q, int P, int invalid, int* parent,
                                                       int* count, long long img_stride, long long work_stride) {
    const int lane = threadIdx.x & 63;
    if (const unsigned sid = stream_index(blockIdx.y)) {
        stream_branch();
        seek_stream(q, sid, img_stride), seek_stream(parent, sid, work_stride), seek_stream(count, sid, work_stride);
    }
    for (int i0 = blockIdx.x * 256 + (threadIdx.x & ~63); i0 < P; i0 += gridDim.x * 256) {
        const int i = i0 + lane;
        bool todo = i < P && q[i] != invalid;
        int r = -1;
        if (todo) {
            r = uf_find(parent, i);
            if (r != i) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (;;) {  // at most 64 rounds: each retires the lanes of one root
            const unsigned long long open = __ballot(todo);
            if (!open) break;
            const int src = __ffsll((long long)open) - 1;
            const int r0 = __shfl(r, src);
            const unsigned long long same = __ballot(todo && r == r0);
            if (lane == src) atomicAdd(count + r0, __popcll(same));
            if (r == r0) todo = false;
        }
    }
}
__global__ __launch_bounds__(256) void k_speckle_apply(int16_t* __restrict__ q, int P, int invalid, int window,
                                                       const int* __restrict__ parent, const int* __restrict__ count,
                                                       long long img_stride, long long work_stride) {
    if (const unsigned sid = stream_index(blockIdx.y)) {
        stream_branch();
        seek_stream(q, sid, img_stride), seek_stream(parent, sid, work_stride), seek_stream(count, sid, work_stride);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
        if (q[i] == invalid) continue;
        if (count[uf_find(parent, i)] <= window) q[i] = (int16_t)invalid;
    }
}

// ------------------------------------------------------------------ stage 9
struct SgmQ {
    double q2[4], q3[4];  // rows 2 and 3 of the 4 x 4 reprojection matrix
};
__global__ void k_sgm_mm_init(unsigned* mm) {  // one block per stream
    if (threadIdx.x == 0) {
        mm[2 * blockIdx.x] = 0xffffffffu;
        mm[2 * blockIdx.x + 1] = 0u;
    }
}
// disp = q / 16 (NaN where <= 0), z in fp64 from nan_to_num(disp), and the min / max of nan_to_num(disp): its values
// are >= 0, so they order like their bit patterns. QDEV: the rows come from Qdev, f64 [n][16] on the device, one matrix
// per stream; else from Q, by value (the single-stream entry point: they stay in scalar registers). mm: [n][2]
template <bool QDEV>
__global__ __launch_bounds__(256) void k_sgm_post(const int16_t* __restrict__ q, int H, int W, SgmQ Q,
                                                  const double* __restrict__ Qdev, float* __restrict__ disp,
                                                  float* __restrict__ z, unsigned* mm) {
    const int P = H * W;
    if (const unsigned sid = stream_index(blockIdx.y)) {
        stream_branch();
        seek_stream(q, sid, P), seek_stream(disp, sid, P), seek_stream(z, sid, P), seek_stream(mm, sid, 2);
        if (QDEV) seek_stream(Qdev, sid, 16);
    }
    if (QDEV) {
#pragma unroll
        for (int i = 0; i < 4; ++i) Q.q2[i] = Qdev[8 + i], Q.q3[i] = Qdev[12 + i];
    }
    unsigned lo = 0xffffffffu, hi = 0u;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
        const int y = i / W, x = i - y * W;
        const int v = q[i];
        const bool ok = v > 0;
        const float d0 = ok ? (float)v / 16.f : 0.f;
        disp[i] = ok ? d0 : NAN;
        const double xd = (double)x, yd = (double)y, dd = (double)d0;
        const double num = ((Q.q2[0] * xd + Q.q2[1] * yd) + Q.q2[2] * dd) + Q.q2[3];
        const double den = ((Q.q3[0] * xd + Q.q3[1] * yd) + Q.q3[2] * dd) + Q.q3[3];
        z[i] = ok ? (float)(num / den) : NAN;
        const unsigned b = __float_as_uint(d0);
        lo = min(lo, b);
        hi = max(hi, b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
    }
    __shared__ unsigned wlo[4], whi[4];
    if ((threadIdx.x & 63) == 0) {
        wlo[threadIdx.x >> 6] = lo;
        whi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one pair of atomics per block, and only where it would change the value
        lo = min(min(wlo[0], wlo[1]), min(wlo[2], wlo[3]));
        hi = max(max(whi[0], whi[1]), max(whi[2], whi[3]));
        if (lo < __hip_atomic_load(mm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(mm, lo);
        if (hi > __hip_atomic_load(mm + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(mm + 1, hi);
    }
}
// cv2.normalize(NORM_MINMAX, 0, 255) + astype(uint8) as stated: trunc(float32(v * scale + shift)), fp64 scale / shift
__global__ __launch_bounds__(256) void k_sgm_code(const float* __restrict__ disp, int P, const unsigned* __restrict__ mm,
                                                  uint8_t* __restrict__ code) {
    if (const unsigned sid = stream_index(blockIdx.y)) {
        stream_branch();
        seek_stream(disp, sid, P), seek_stream(code, sid, P), seek_stream(mm, sid, 2);
    }
    const double lo = (double)__uint_as_float(mm[0]), hi = (double)__uint_as_float(mm[1]);
    const double scale = hi != lo ? 255.0 / (hi - lo) : 0.0;
    const double shift = -lo * scale;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
        const float v = disp[i];
        const double d0 = v == v ? (double)v : 0.0;
        code[i] = (uint8_t)(int)truncf((float)(d0 * scale + shift));
    }
}

// np.nanmedian of the centre window: stage_util.h's center_median over every non-NaN value, infinities and negatives
// included (sd_live_center keeps only finite, > 0 values).
struct NotNaN {
    __device__ __forceinline__ static bool test(float v) { return v == v; }
};
__global__ __launch_bounds__(256) void k_sgm_center(const float* __restrict__ src, int H, int W, int window,
                                                    float* __restrict__ out) {  // one block per stream
    if (const unsigned sid = stream_index(blockIdx.x)) {
        stream_branch();
        seek_stream(src, sid, (long long)H * W), out += sid;
    }
    const float m = center_median<NotNaN>(src, H, W, window);
    if (threadIdx.x == 0) out[0] = m;
}

// ------------------------------------------------------------------ launches
// The streams of a launch and the distances between their slices: img in elements of an image plane (gray, q), pre in
// bytes between the prefiltered planes, vol in uint16 elements between the volumes, spk in int32 elements between the
// speckle planes. A single-stream entry point passes SGM_ONE; a slice of the batched workspace is the single-stream
// workspace, so pre, vol and spk are all its size there.
struct SgmBatch {
    int n;
    long long img, pre, vol, spk;
    long long dsc = 0;  // census cost: uint64 elements between the streams' descriptor planes
};
constexpr SgmBatch SGM_ONE = {1, 0, 0, 0, 0};

// the distance between the streams' side planes of a cost, in the elements Cost::seek counts in: bytes between the
// prefiltered planes, uint64 between the descriptor planes
long long cost_side_stride(const SgmBatch& nb, const CostBT&) { return nb.pre; }
long long cost_side_stride(const SgmBatch& nb, const CostCensus&) { return nb.dsc; }
template <class Cost>
int launch_cost(const SgmBatch& nb, const Cost& cost, int H, int W, const SgmParams& p, uint16_t* C,
                uint16_t* tmp, hipStream_t st, const char* what) {
    const int maxD = p.minD + p.D;
    if (W <= maxD) return SD_OK;
    const int nseg = cdiv(W - maxD, SGM_SEG), spb = 256 / p.D;
    // grid y is the row (cost_rows) or the row segment (cost_cols): the stream goes in z
    hipLaunchKernelGGL(k_sgm_cost_rows<Cost>, dim3(cdiv(nseg, spb), H, nb.n), dim3(256), 0, st, cost, W, p.minD, p.D,
                       p.bs, tmp, nb.img, cost_side_stride(nb, cost), nb.vol);
    hipLaunchKernelGGL(k_sgm_cost_cols, dim3(cdiv((long long)(W - maxD) * p.D, 1024), cdiv(H, SGM_YSEG), nb.n), dim3(256),
                       0, st, tmp, H, W, maxD, p.D, p.bs, C, nb.vol);
    return sd_check_launch(what);
}

// the descriptors of n planes g [n][H][W] (img_stride apart) into desc (desc_stride apart), one launch
int launch_census(int n, const uint8_t* g, int H, int W, int wh, int ww, unsigned long long* desc, long long img_stride,
                  long long desc_stride, hipStream_t st) {
    const dim3 grid(cdiv(W, CENSUS_TW), cdiv(H, CENSUS_TH), n), b(256);
#define SGM_CENSUS(WH, WW) \
    hipLaunchKernelGGL((k_sgm_census<WH, WW>), grid, b, 0, st, g, H, W, desc, img_stride, desc_stride)
    if (wh == 3)
        SGM_CENSUS(3, 3);
    else if (wh == 5)
        SGM_CENSUS(5, 5);
    else if (ww == 7)
        SGM_CENSUS(7, 7);
    else
        SGM_CENSUS(7, 9);
#undef SGM_CENSUS
    return sd_check_launch("sd_sgm_census");
}

template <int NK, bool FULL>
void launch_path(const SgmBatch& nb, int pass, const uint16_t* C, int H, int W, const SgmParams& p, uint16_t* S,
                 hipStream_t st) {
    const int maxD = p.minD + p.D;
    if (pass == 0)
        hipLaunchKernelGGL((k_sgm_down<NK, FULL>), dim3(cdiv(W - maxD, 4), nb.n), dim3(256), 0, st, C, H, W, maxD, p.D,
                           p.P1, p.P2, S, nb.vol);
    else
        hipLaunchKernelGGL((k_sgm_right<NK, FULL>), dim3(H, nb.n), dim3(64), 0, st, C, W, maxD, p.D, p.P1, p.P2, S,
                           nb.vol);
}
int launch_aggregate(const SgmBatch& nb, int pass, const uint16_t* C, int H, int W, const SgmParams& p, uint16_t* S,
                     hipStream_t st) {
    if (W <= p.minD + p.D) return SD_OK;
    const bool full = p.D % 64 == 0;
#define SGM_PATH(NK)                                                \
    (full ? launch_path<NK, true>(nb, pass, C, H, W, p, S, st)     \
          : launch_path<NK, false>(nb, pass, C, H, W, p, S, st))
    switch ((p.D + 63) / 64) {
    case 1: SGM_PATH(1); break;
    case 2: SGM_PATH(2); break;
    case 3: SGM_PATH(3); break;
    default: SGM_PATH(4); break;
    }
#undef SGM_PATH
    return sd_check_launch("sd_sgm_aggregate");
}

template <int NK, bool FULL>
void launch_walk(const SgmBatch& nb, const uint16_t* C, int H, int W, const SgmParams& p, int dy, int dx, bool acc,
                 uint16_t* S, hipStream_t st) {
    const int maxD = p.minD + p.D, n = W - maxD;
    const int lines = dy == 0 ? H : n, T = dy == 0 ? n : H;
    if (acc)
        hipLaunchKernelGGL((k_sgm_walk<NK, FULL, true>), dim3(cdiv(lines, 4), nb.n), dim3(256), 0, st, C, H, W, maxD, p.D,
                           p.P1, p.P2, dy, dx, lines, T, S, nb.vol);
    else
        hipLaunchKernelGGL((k_sgm_walk<NK, FULL, false>), dim3(cdiv(lines, 4), nb.n), dim3(256), 0, st, C, H, W, maxD, p.D,
                           p.P1, p.P2, dy, dx, lines, T, S, nb.vol);
}
// one path (dy, dx) other than right -> left: S = L (acc false) or S += L. Top -> down writing S and left -> right
// adding to it are the 3-way mode's own kernels.
int launch_dir(const SgmBatch& nb, const uint16_t* C, int H, int W, const SgmParams& p, int dy, int dx, bool acc,
               uint16_t* S, hipStream_t st) {
    if (W <= p.minD + p.D) return SD_OK;
    if (dy == 1 && dx == 0 && !acc) return launch_aggregate(nb, 0, C, H, W, p, S, st);
    if (dy == 0 && dx == 1 && acc) return launch_aggregate(nb, 1, C, H, W, p, S, st);
    const bool full = p.D % 64 == 0;
#define SGM_WALK(NK)                                                          \
    (full ? launch_walk<NK, true>(nb, C, H, W, p, dy, dx, acc, S, st)        \
          : launch_walk<NK, false>(nb, C, H, W, p, dy, dx, acc, S, st))
    switch ((p.D + 63) / 64) {
    case 1: SGM_WALK(1); break;
    case 2: SGM_WALK(2); break;
    case 3: SGM_WALK(3); break;
    default: SGM_WALK(4); break;
    }
#undef SGM_WALK
    return sd_check_launch("sd_sgm_aggregate_dir");
}

template <int NK, bool FULL>
void launch_left(const SgmBatch& nb, const uint16_t* C, const uint16_t* S, int H, int W, const SgmParams& p,
                 uint16_t* S_total, int16_t* q_raw, int16_t* q, hipStream_t st) {
    const size_t lds = (size_t)(W + 1) * 14;
    if (S_total)
        hipLaunchKernelGGL((k_sgm_left<NK, FULL, true>), dim3(H, nb.n), dim3(64), lds, st, C, S, W, p.minD, p.D, p.P1,
                           p.P2, p.uniq, p.max_diff, S_total, q_raw, q, nb.vol, nb.img);
    else
        hipLaunchKernelGGL((k_sgm_left<NK, FULL, false>), dim3(H, nb.n), dim3(64), lds, st, C, S, W, p.minD, p.D, p.P1,
                           p.P2, p.uniq, p.max_diff, S_total, q_raw, q, nb.vol, nb.img);
}
int launch_winner(const SgmBatch& nb, const uint16_t* C, const uint16_t* S, int H, int W, const SgmParams& p,
                  uint16_t* S_total, int16_t* q_raw, int16_t* q, hipStream_t st) {
    const bool full = p.D % 64 == 0;
#define SGM_LEFT(NK)                                                             \
    (full ? launch_left<NK, true>(nb, C, S, H, W, p, S_total, q_raw, q, st)     \
          : launch_left<NK, false>(nb, C, S, H, W, p, S_total, q_raw, q, st))
    switch ((p.D + 63) / 64) {
    case 1: SGM_LEFT(1); break;
    case 2: SGM_LEFT(2); break;
    case 3: SGM_LEFT(3); break;
    default: SGM_LEFT(4); break;
    }
#undef SGM_LEFT
    return sd_check_launch("sd_sgm_winner");
}

// Every stream's pixels index its own parent / count planes from 0 (nb.img, nb.spk apart): a link can only name a
// pixel of the same stream, so no component crosses a stream boundary.
int launch_speckle(const SgmBatch& nb, int16_t* q, int H, int W, int invalid, int window, int range, void* work,
                   hipStream_t st) {
    if (window <= 0) return SD_OK;
    const int P = H * W;
    int* parent = static_cast<int*>(work);
    int* count = reinterpret_cast<int*>(static_cast<char*>(work) + align256(4ll * P));
    const dim3 g(sgm_grid(P), nb.n), b(256);
    hipLaunchKernelGGL(k_speckle_init, dim3(sgm_grid(64ll * H * ((W + 63) / 64)), nb.n), b, 0, st, q, H, W, invalid,
                       16 * range, parent, count, nb.img, nb.spk);
    hipLaunchKernelGGL(k_speckle_link, g, b, 0, st, q, H, W, invalid, 16 * range, parent, nb.img, nb.spk);
    hipLaunchKernelGGL(k_speckle_count, g, b, 0, st, q, P, invalid, parent, count, nb.img, nb.spk);
    hipLaunchKernelGGL(k_speckle_apply, g, b, 0, st, q, P, invalid, window, parent, count, nb.img, nb.spk);
    return sd_check_launch("sd_sgm_speckle");
}
bool sgm_streams_ok(int n) { return n >= 1 && n <= 64; }
#define SGM_N_REQUIRE(fn, n) SD_REQUIRE(sgm_streams_ok(n), "%s: n = %d streams (1..64)", fn, n)

#define SGM_PARAMS_OK(what, p)                                     \
    do {                                                           \
        const char* e_ = sgm_params_error(p);                      \
        SD_REQUIRE(!e_, what ": %s", e_);                          \
    } while (0)

}  // namespace

extern "C" long long sd_sgm_speckle_ws_bytes(int H, int W) { return 2 * align256(4ll * H * W); }

extern "C" long long sd_sgm_ws_bytes(int H, int W, int D) {
    const long long P = (long long)H * W;
    return 2 * align256(2 * P * D) + 2 * align256(P) + sd_sgm_speckle_ws_bytes(H, W);
}

extern "C" int sd_sgm_gray(const uint8_t* bgr, int H, int W, uint8_t* gray, sd_stream s) {
    SD_REQUIRE(bgr && gray, "sd_sgm_gray: null pointer");
    SD_REQUIRE(sgm_dims_ok(H, W), "sd_sgm_gray: bad sizes %dx%d", H, W);
    hipLaunchKernelGGL(k_sgm_gray, dim3(sgm_grid((long long)H * W)), dim3(256), 0, to_stream(s), bgr, H * W, gray);
    return sd_check_launch("sd_sgm_gray");
}

extern "C" int sd_sgm_prefilter(const uint8_t* gray, int H, int W, int cap, uint8_t* out, sd_stream s) {
    SD_REQUIRE(gray && out, "sd_sgm_prefilter: null pointer");
    SD_REQUIRE(sgm_dims_ok(H, W), "sd_sgm_prefilter: bad sizes %dx%d", H, W);
    SD_REQUIRE(cap >= 1 && cap <= 63, "sd_sgm_prefilter: cap %d (1..63)", cap);
    hipLaunchKernelGGL(k_sgm_prefilter, dim3(sgm_grid((long long)H * W)), dim3(256), 0, to_stream(s), gray, H, W, cap, out,
                       0ll, 0ll);
    return sd_check_launch("sd_sgm_prefilter");
}

extern "C" int sd_sgm_cost(const uint8_t* gray_l, const uint8_t* gray_r, const uint8_t* pre_l, const uint8_t* pre_r, int H,
                           int W, int min_disparity, int num_disparities, int block_size, uint16_t* C, uint16_t* tmp,
                           sd_stream s) {
    SD_REQUIRE(gray_l && gray_r && pre_l && pre_r && C && tmp && C != tmp, "sd_sgm_cost: null pointer");
    SD_REQUIRE((uintptr_t)C % 8 == 0 && (uintptr_t)tmp % 8 == 0, "sd_sgm_cost: volumes must be 8-B aligned");
    SD_REQUIRE(sgm_dims_ok(H, W) && H <= 65535, "sd_sgm_cost: bad sizes %dx%d", H, W);
    const SgmParams p = {min_disparity, num_disparities, block_size, 0, 0, 1, 0, 0, 0, 31};
    SGM_PARAMS_OK("sd_sgm_cost", p);
    return launch_cost(SGM_ONE, CostBT{gray_l, gray_r, pre_l, pre_r}, H, W, p, C, tmp, to_stream(s), "sd_sgm_cost");
}

extern "C" int sd_sgm_census_n(int n, const uint8_t* gray, int H, int W, int win_h, int win_w, uint64_t* desc,
                               sd_stream s) {
    SGM_N_REQUIRE("sd_sgm_census_n", n);
    SD_REQUIRE(gray && desc, "sd_sgm_census_n: null pointer");
    SD_REQUIRE((uintptr_t)desc % 8 == 0, "sd_sgm_census_n: desc must be 8-B aligned");
    SD_REQUIRE(sgm_dims_ok(H, W) && H <= 65535, "sd_sgm_census_n: bad sizes %dx%d", H, W);
    SD_REQUIRE(sgm_census_bits(win_h, win_w), "sd_sgm_census_n: window %dx%d (3x3, 5x5, 7x7 or 7x9, rows x columns)",
               win_h, win_w);
    const long long P = (long long)H * W;
    return launch_census(n, gray, H, W, win_h, win_w, reinterpret_cast<unsigned long long*>(desc), P, P, to_stream(s));
}

extern "C" int sd_sgm_cost_census(const uint64_t* desc_l, const uint64_t* desc_r, int H, int W, int min_disparity,
                                  int num_disparities, int block_size, int nbits, uint16_t* C, uint16_t* tmp,
                                  sd_stream s) {
    SD_REQUIRE(desc_l && desc_r && C && tmp && C != tmp, "sd_sgm_cost_census: null pointer");
    SD_REQUIRE((uintptr_t)desc_l % 8 == 0 && (uintptr_t)desc_r % 8 == 0, "sd_sgm_cost_census: desc must be 8-B aligned");
    SD_REQUIRE((uintptr_t)C % 8 == 0 && (uintptr_t)tmp % 8 == 0, "sd_sgm_cost_census: volumes must be 8-B aligned");
    SD_REQUIRE(sgm_dims_ok(H, W) && H <= 65535, "sd_sgm_cost_census: bad sizes %dx%d", H, W);
    SD_REQUIRE(nbits == 8 || nbits == 24 || nbits == 48 || nbits == 62, "sd_sgm_cost_census: nbits %d (8, 24, 48, 62)",
               nbits);
    SgmParams p = {min_disparity, num_disparities, block_size, 0, 0, 1, 0, 0, 0, 31};
    p.nbits = nbits;
    SGM_PARAMS_OK("sd_sgm_cost_census", p);
    const CostCensus cost = {reinterpret_cast<const unsigned long long*>(desc_l),
                             reinterpret_cast<const unsigned long long*>(desc_r)};
    return launch_cost(SGM_ONE, cost, H, W, p, C, tmp, to_stream(s), "sd_sgm_cost_census");
}

extern "C" int sd_sgm_aggregate(const uint16_t* C, int H, int W, int min_disparity, int num_disparities, int P1, int P2,
                                int pass, uint16_t* S, sd_stream s) {
    SD_REQUIRE(C && S, "sd_sgm_aggregate: null pointer");
    SD_REQUIRE(sgm_dims_ok(H, W), "sd_sgm_aggregate: bad sizes %dx%d", H, W);
    SD_REQUIRE(pass == 0 || pass == 1, "sd_sgm_aggregate: pass %d (0 top-down, 1 left-right)", pass);
    const SgmParams p = {min_disparity, num_disparities, 3, P1, P2, 1, 0, 0, 0, 1};
    SGM_PARAMS_OK("sd_sgm_aggregate", p);
    return launch_aggregate(SGM_ONE, pass, C, H, W, p, S, to_stream(s));
}

extern "C" int sd_sgm_aggregate_dir(const uint16_t* C, int H, int W, int min_disparity, int num_disparities, int P1,
                                    int P2, int dy, int dx, int accumulate, uint16_t* S, sd_stream s) {
    SD_REQUIRE(C && S, "sd_sgm_aggregate_dir: null pointer");
    SD_REQUIRE(sgm_dims_ok(H, W), "sd_sgm_aggregate_dir: bad sizes %dx%d", H, W);
    SD_REQUIRE(!(dy == 0 && dx == -1),
               "sd_sgm_aggregate_dir: the right -> left path (0, -1) runs inside sd_sgm_winner, on top of the other paths' S");
    SD_REQUIRE(((dy == 1 || dy == -1) && dx >= -1 && dx <= 1) || (dy == 0 && dx == 1),
               "sd_sgm_aggregate_dir: direction (%d, %d): dy = +-1 with dx in {-1, 0, 1}, or (0, 1)", dy, dx);
    SD_REQUIRE(accumulate == 0 || accumulate == 1, "sd_sgm_aggregate_dir: accumulate %d (0: S = L, 1: S += L)", accumulate);
    const SgmParams p = {min_disparity, num_disparities, 3, P1, P2, 1, 0, 0, 0, 1};
    SGM_PARAMS_OK("sd_sgm_aggregate_dir", p);
    return launch_dir(SGM_ONE, C, H, W, p, dy, dx, accumulate != 0, S, to_stream(s));
}

extern "C" int sd_sgm_winner(const uint16_t* C, const uint16_t* S, int H, int W, int min_disparity, int num_disparities,
                             int P1, int P2, int uniqueness_ratio, int disp12_max_diff, uint16_t* S_total,
                             int16_t* q_raw, int16_t* q, sd_stream s) {
    SD_REQUIRE(C && S && q, "sd_sgm_winner: null pointer");
    SD_REQUIRE(sgm_dims_ok(H, W) && W <= SGM_MAX_W, "sd_sgm_winner: bad sizes %dx%d (W <= %d)", H, W, SGM_MAX_W);
    const SgmParams p = {min_disparity, num_disparities, 3, P1, P2, disp12_max_diff, uniqueness_ratio, 0, 0, 1};
    SGM_PARAMS_OK("sd_sgm_winner", p);
    return launch_winner(SGM_ONE, C, S, H, W, p, S_total, q_raw, q, to_stream(s));
}

namespace {
// sd_sgm_speckle (n = 1) and sd_sgm_speckle_n: q is [n][H][W], work n slices of sd_sgm_speckle_ws_bytes
int sgm_speckle(const char* fn, int n, int16_t* q, int H, int W, int invalid_value, int window, int range, void* work,
                sd_stream s) {
    SGM_N_REQUIRE(fn, n);
    SD_REQUIRE(q && (work || window <= 0), "%s: null pointer (q, work)", fn);
    SD_REQUIRE(sgm_dims_ok(H, W), "%s: bad sizes %dx%d", fn, H, W);
    SD_REQUIRE(window >= 0 && range >= 0 && range <= 1024, "%s: window %d range %d", fn, window, range);
    SD_REQUIRE((uintptr_t)work % 4 == 0, "%s: work must be 4-B aligned", fn);
    const SgmBatch nb = {n, (long long)H * W, 0, 0, sd_sgm_speckle_ws_bytes(H, W) / 4};
    return launch_speckle(nb, q, H, W, invalid_value, window, range, work, to_stream(s));
}
}  // namespace

extern "C" int sd_sgm_speckle(int16_t* q, int H, int W, int invalid_value, int window, int range, void* work,
                              sd_stream s) {
    return sgm_speckle("sd_sgm_speckle", 1, q, H, W, invalid_value, window, range, work, s);
}
extern "C" int sd_sgm_speckle_n(int n, int16_t* q, int H, int W, int invalid_value, int window, int range, void* work,
                                sd_stream s) {
    return sgm_speckle("sd_sgm_speckle_n", n, q, H, W, invalid_value, window, range, work, s);
}

namespace {
// the vertical-family paths a mode adds to the 3-way mode's three, as (dy, dx)
const int SGM_EXTRA_PATHS[5][2] = {{1, 1}, {1, -1}, {-1, 0}, {-1, 1}, {-1, -1}};
// One stream's workspace: sd_sgm_ws_bytes, and for the census cost two uint64 descriptor planes behind it, so that the
// Birchfield-Tomasi layout is a prefix of the census one. A multiple of 256.
long long sgm_ws_slice(int H, int W, int D, int cost) {
    return sd_sgm_ws_bytes(H, W, D) + (cost == SD_SGM_COST_CENSUS ? 2 * align256(8ll * H * W) : 0);
}
// The whole matcher for n streams: gray_l, gray_r [n][H][W], q [n][H][W], work n slices of sd_sgm_ws_bytes. One launch
// sequence whatever n is; the single-stream entry points are n = 1. p.nbits != 0 is the census cost of window
// (wh, ww): work is then n slices of sgm_ws_slice(.., SD_SGM_COST_CENSUS), the Birchfield-Tomasi slice followed by the
// two descriptor planes, and the prefiltered planes stay unwritten.
int sgm_compute(const char* what, int n, const uint8_t* gray_l, const uint8_t* gray_r, int H, int W, const SgmParams& p,
                int mode, int wh, int ww, void* work, int16_t* q, sd_stream s) {
    SGM_N_REQUIRE(what, n);
    SD_REQUIRE(gray_l && gray_r && work && q, "%s: null pointer (gray_l, gray_r, work, q)", what);
    SD_REQUIRE(sgm_dims_ok(H, W) && H <= 65535 && W <= SGM_MAX_W, "%s: bad sizes %dx%d (W <= %d)", what, H, W, SGM_MAX_W);
    SD_REQUIRE((uintptr_t)work % 256 == 0, "%s: work must be 256-B aligned", what);
    const char* e = sgm_params_error(p);
    SD_REQUIRE(!e, "%s: %s", what, e);
    const bool census = p.nbits != 0;
    const long long P = (long long)H * W, vol = align256(2 * P * p.D);
    const long long slice = sgm_ws_slice(H, W, p.D, census ? SD_SGM_COST_CENSUS : SD_SGM_COST_BT);
    const SgmBatch nb = {n, P, slice, slice / 2, slice / 4, slice / 8};
    char* w = static_cast<char*>(work);
    uint16_t* C = reinterpret_cast<uint16_t*>(w);
    uint16_t* S = reinterpret_cast<uint16_t*>(w + vol);
    uint8_t* pl = reinterpret_cast<uint8_t*>(w + 2 * vol);
    uint8_t* pr = pl + align256(P);
    void* sw = pr + align256(P);
    hipStream_t st = to_stream(s);
    int rc;
    if (census) {
        unsigned long long* cl = reinterpret_cast<unsigned long long*>(w + sd_sgm_ws_bytes(H, W, p.D));
        unsigned long long* cr = cl + align256(8 * P) / 8;
        rc = launch_census(n, gray_l, H, W, wh, ww, cl, nb.img, nb.dsc, st);
        if (rc == SD_OK) rc = launch_census(n, gray_r, H, W, wh, ww, cr, nb.img, nb.dsc, st);
        if (rc == SD_OK) rc = launch_cost(nb, CostCensus{cl, cr}, H, W, p, C, S, st, "sd_sgm_cost_census");
    } else {
        const dim3 g(sgm_grid(P), n), b(256);
        hipLaunchKernelGGL(k_sgm_prefilter, g, b, 0, st, gray_l, H, W, p.cap, pl, nb.img, nb.pre);
        hipLaunchKernelGGL(k_sgm_prefilter, g, b, 0, st, gray_r, H, W, p.cap, pr, nb.img, nb.pre);
        // S is free until the first path writes it
        rc = launch_cost(nb, CostBT{gray_l, gray_r, pl, pr}, H, W, p, C, S, st, "sd_sgm_cost");
    }
    if (rc == SD_OK) rc = launch_aggregate(nb, 0, C, H, W, p, S, st);
    // successive launches, each S += L: sgbm takes the two downward diagonals, hh4 bottom -> up, hh all five
    const int first = mode == SD_SGM_MODE_HH4 ? 2 : 0;
    const int last = mode == SD_SGM_MODE_HH4 ? 3 : mode == SD_SGM_MODE_SGBM ? 2 : mode == SD_SGM_MODE_HH ? 5 : 0;
    for (int i = first; i < last && rc == SD_OK; ++i)
        rc = launch_dir(nb, C, H, W, p, SGM_EXTRA_PATHS[i][0], SGM_EXTRA_PATHS[i][1], true, S, st);
    if (rc == SD_OK) rc = launch_aggregate(nb, 1, C, H, W, p, S, st);
    if (rc == SD_OK) rc = launch_winner(nb, C, S, H, W, p, nullptr, nullptr, q, st);
    if (rc == SD_OK) rc = launch_speckle(nb, q, H, W, 16 * (p.minD - 1), p.speckle_window, p.speckle_range, sw, st);
    return rc;
}
}  // namespace

extern "C" long long sd_sgm_ws_bytes_n(int n, int H, int W, int D) {
    return sgm_streams_ok(n) ? n * sd_sgm_ws_bytes(H, W, D) : -1;
}

extern "C" int sd_sgm_compute_n(int n, const uint8_t* gray_l, const uint8_t* gray_r, int H, int W, int min_disparity,
                                int num_disparities, int block_size, int P1, int P2, int disp12_max_diff,
                                int uniqueness_ratio, int speckle_window, int speckle_range, int pre_filter_cap, int mode,
                                void* work, int16_t* q, sd_stream s) {
    SGM_N_REQUIRE("sd_sgm_compute_n", n);
    const int npaths = sgm_mode_paths(mode);
    SD_REQUIRE(npaths, "sd_sgm_compute_n: mode %d (SD_SGM_MODE_SGBM 0, _HH 1, _3WAY 2, _HH4 3)", mode);
    const SgmParams p = {min_disparity, num_disparities, block_size, P1, P2, disp12_max_diff, uniqueness_ratio,
                         speckle_window, speckle_range, pre_filter_cap, npaths};
    return sgm_compute("sd_sgm_compute_n", n, gray_l, gray_r, H, W, p, mode, 0, 0, work, q, s);
}

extern "C" long long sd_sgm_ws_bytes_cost_n(int n, int H, int W, int D, int cost) {
    const bool ok = sgm_streams_ok(n) && (cost == SD_SGM_COST_BT || cost == SD_SGM_COST_CENSUS);
    return ok ? n * sgm_ws_slice(H, W, D, cost) : -1;
}

extern "C" int sd_sgm_compute_cost_n(int n, const uint8_t* gray_l, const uint8_t* gray_r, int H, int W,
                                     int min_disparity, int num_disparities, int block_size, int P1, int P2,
                                     int disp12_max_diff, int uniqueness_ratio, int speckle_window, int speckle_range,
                                     int pre_filter_cap, int mode, int cost, int win_h, int win_w, void* work,
                                     int16_t* q, sd_stream s) {
    SGM_N_REQUIRE("sd_sgm_compute_cost_n", n);
    const int npaths = sgm_mode_paths(mode);
    SD_REQUIRE(npaths, "sd_sgm_compute_cost_n: mode %d (SD_SGM_MODE_SGBM 0, _HH 1, _3WAY 2, _HH4 3)", mode);
    SD_REQUIRE(cost == SD_SGM_COST_BT || cost == SD_SGM_COST_CENSUS,
               "sd_sgm_compute_cost_n: cost %d (SD_SGM_COST_BT 0, SD_SGM_COST_CENSUS 1)", cost);
    SgmParams p = {min_disparity, num_disparities, block_size, P1, P2, disp12_max_diff, uniqueness_ratio,
                   speckle_window, speckle_range, pre_filter_cap, npaths};
    if (cost == SD_SGM_COST_CENSUS) {
        p.nbits = sgm_census_bits(win_h, win_w);
        SD_REQUIRE(p.nbits, "sd_sgm_compute_cost_n: window %dx%d (3x3, 5x5, 7x7 or 7x9, rows x columns)", win_h, win_w);
    }
    return sgm_compute("sd_sgm_compute_cost_n", n, gray_l, gray_r, H, W, p, mode, win_h, win_w, work, q, s);
}

extern "C" int sd_sgm_compute(const uint8_t* gray_l, const uint8_t* gray_r, int H, int W, int min_disparity,
                              int num_disparities, int block_size, int P1, int P2, int disp12_max_diff,
                              int uniqueness_ratio, int speckle_window, int speckle_range, int pre_filter_cap, void* work,
                              int16_t* q, sd_stream s) {
    const SgmParams p = {min_disparity, num_disparities, block_size, P1, P2, disp12_max_diff, uniqueness_ratio,
                         speckle_window, speckle_range, pre_filter_cap};
    return sgm_compute("sd_sgm_compute", 1, gray_l, gray_r, H, W, p, SD_SGM_MODE_3WAY, 0, 0, work, q, s);
}

extern "C" int sd_sgm_compute_mode(const uint8_t* gray_l, const uint8_t* gray_r, int H, int W, int min_disparity,
                                   int num_disparities, int block_size, int P1, int P2, int disp12_max_diff,
                                   int uniqueness_ratio, int speckle_window, int speckle_range, int pre_filter_cap,
                                   int mode, void* work, int16_t* q, sd_stream s) {
    const int npaths = sgm_mode_paths(mode);
    SD_REQUIRE(npaths, "sd_sgm_compute_mode: mode %d (SD_SGM_MODE_SGBM 0, _HH 1, _3WAY 2, _HH4 3)", mode);
    const SgmParams p = {min_disparity, num_disparities, block_size, P1, P2, disp12_max_diff, uniqueness_ratio,
                         speckle_window, speckle_range, pre_filter_cap, npaths};
    return sgm_compute("sd_sgm_compute_mode", 1, gray_l, gray_r, H, W, p, mode, 0, 0, work, q, s);
}

namespace {
// sd_sgm_post (Q on the host, by value) and sd_sgm_post_n (Qdev: f64 [n][16] on the device); minmax is [n][2]
int sgm_post(const char* fn, int n, const int16_t* q, int H, int W, const double* Qhost, const double* Qdev, float* disp,
             float* z, uint8_t* code, unsigned* minmax, sd_stream s) {
    SGM_N_REQUIRE(fn, n);
    SD_REQUIRE(q && (Qhost || Qdev) && disp && z && code && minmax, "%s: null pointer (q, Q, disp, z, code, minmax)", fn);
    SD_REQUIRE(sgm_dims_ok(H, W), "%s: bad sizes %dx%d", fn, H, W);
    SgmQ m = {};
    for (int i = 0; Qhost && i < 4; ++i) {
        m.q2[i] = Qhost[8 + i];
        m.q3[i] = Qhost[12 + i];
    }
    hipStream_t st = to_stream(s);
    const dim3 g(sgm_grid((long long)H * W), n), b(256);
    hipLaunchKernelGGL(k_sgm_mm_init, dim3(n), dim3(64), 0, st, minmax);
    hipLaunchKernelGGL(Qdev ? k_sgm_post<true> : k_sgm_post<false>, g, b, 0, st, q, H, W, m, Qdev, disp, z, minmax);
    hipLaunchKernelGGL(k_sgm_code, g, b, 0, st, disp, H * W, minmax, code);
    return sd_check_launch(fn);
}
int sgm_center(const char* fn, int n, const float* z, int H, int W, int window, float* out, sd_stream s) {
    SGM_N_REQUIRE(fn, n);
    SD_REQUIRE(z && out, "%s: null pointer (z, out)", fn);
    SD_REQUIRE(sgm_dims_ok(H, W), "%s: bad sizes %dx%d", fn, H, W);
    SD_REQUIRE(window >= 0 && window <= 63, "%s: window %d (max 63)", fn, window);
    hipLaunchKernelGGL(k_sgm_center, dim3(n), dim3(256), 0, to_stream(s), z, H, W, window, out);
    return sd_check_launch(fn);
}
}  // namespace

extern "C" int sd_sgm_post(const int16_t* q, int H, int W, const double* Q, float* disp, float* z, uint8_t* code,
                           unsigned* minmax, sd_stream s) {
    return sgm_post("sd_sgm_post", 1, q, H, W, Q, nullptr, disp, z, code, minmax, s);
}
extern "C" int sd_sgm_post_n(int n, const int16_t* q, int H, int W, const double* Qdev, float* disp, float* z,
                             uint8_t* code, unsigned* minmax, sd_stream s) {
    return sgm_post("sd_sgm_post_n", n, q, H, W, nullptr, Qdev, disp, z, code, minmax, s);
}

extern "C" int sd_sgm_center(const float* z, int H, int W, int window, float* out, sd_stream s) {
    return sgm_center("sd_sgm_center", 1, z, H, W, window, out, s);
}
extern "C" int sd_sgm_center_n(int n, const float* z, int H, int W, int window, float* out, sd_stream s) {
    return sgm_center("sd_sgm_center_n", n, z, H, W, window, out, s);
}
