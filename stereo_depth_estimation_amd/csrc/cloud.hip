// Coloured point clouds from disparity maps (cv2.reprojectImageTo3D of the reference's live_camera/depth_live.py:164,
// all three coordinates instead of [:, :, 2] only), on the device. Stated in INTEGRATION.md ("sd_cloud_build_n") and
// pinned bit for bit to the NumPy restatement tests/cloud_ref.py.
//   value  : a pixel whose disparity is finite and > 0; R_r = ((Q[r][0] x + Q[r][1] y) + Q[r][2] d) + Q[r][3] in fp64,
//            every operation rounded on its own; X, Y, Z = float32(R_0 / R_3), float32(R_1 / R_3), float32(R_2 / R_3)
//   kept   : a value whose X, Y, Z are finite and whose Z lies in [z_min, z_max] (float32 comparisons)
//   xyz    : the organised cloud, NaN where not kept
//   points : the kept pixels of the stride lattice, packed in ascending (y, x) order as 16-byte records
// The packing is a stream compaction in three plain launches, the stream being grid dimension y of each:
//   count   one block per tile of CLOUD_TILE pixels (linear pixel index, so ascending (y, x)): the number it packs
//   scan    one block per stream: the exclusive prefix sum of its tile counts, CLOUD_SCAN of them per step, and the total
//   scatter the count pass again (the same device function, so the same decisions), each record stored at tile offset +
//           offset of the wave within the block (LDS) + rank of the lane within the wave (ballot / mbcnt)
// No block waits for another block and no atomics take part, so the order is the pixel order on every run. Nothing
// is kept between the passes but the tile counts: the scatter pass recomputes the points (three fp64 divisions a pixel)
// rather than read back a mask, which keeps the workspace at 4 bytes per 1024 pixels.
// No allocation, no synchronisation: the entry point is graph-capturable. Workspace is the caller's.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"

// the fp64 reprojection reproduces numpy's separately rounded operations (as sgm.hip's k_sgm_post)
#pragma clang fp contract(off)

namespace {

constexpr int CLOUD_THREADS = 256;  // four waves
constexpr int CLOUD_ROUNDS = 4;     // pixels per thread: a wave owns 256 consecutive pixels, 64 per round
constexpr int CLOUD_TILE = CLOUD_THREADS * CLOUD_ROUNDS;
constexpr int CLOUD_SCAN = 256;     // tile counts per step of the scan kernel (one per thread)

long long cloud_align256(long long v) { return (v + 255) / 256 * 256; }
bool cloud_dims_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W < (1ll << 31); }
long long cloud_tiles(int H, int W) { return ((long long)H * W + CLOUD_TILE - 1) / CLOUD_TILE; }
// u32 words between the tile counts of two streams
long long cloud_pitch(int H, int W) { return cloud_align256(4 * cloud_tiles(H, W)) / 4; }

struct CloudArgs {
    const float* disp;
    const uint8_t* color;
    const double* Qdev;
    float* xyz;
    uint4* points;
    unsigned* work;
    long long cap;
    long long pitch;
    unsigned P;
    int W, stride, bgr;
    FastDiv fw, fs;
    float z_min, z_max;
};

struct CloudPoint {
    float x, y, z;
    bool keep;
};

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= FLT_MAX; }  // false for NaN

// the value of pixel (x, y) with disparity dv, and whether it is kept
__device__ __forceinline__ CloudPoint cloud_point(float dv, int x, int y, const double (&Q)[16], float z_min,
                                                  float z_max) {
    const bool has = dv > 0.f && dv <= FLT_MAX;
    const double xd = (double)x, yd = (double)y, dd = has ? (double)dv : 1.0;
    double R[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) R[r] = ((Q[4 * r] * xd + Q[4 * r + 1] * yd) + Q[4 * r + 2] * dd) + Q[4 * r + 3];
    CloudPoint p;
    p.x = (float)(R[0] / R[3]);
    p.y = (float)(R[1] / R[3]);
    p.z = (float)(R[2] / R[3]);
    p.keep = has && finite32(p.x) && finite32(p.y) && finite32(p.z) && z_min <= p.z && p.z <= z_max;
    return p;
}

// SCATTER false: the tile's count into work. SCATTER true: xyz (if asked for) and the tile's records, from the tile
// offsets the scan left in work.
template <bool SCATTER>
__global__ __launch_bounds__(CLOUD_THREADS) void k_cloud_tile(CloudArgs a) {
    const unsigned sid = blockIdx.y, tile = blockIdx.x;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t img = (size_t)sid * a.P;
    double Q[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) Q[i] = a.Qdev[(size_t)sid * 16 + i];
    // P < 2^31 and tile * CLOUD_TILE < P, so the index of a thread's last pixel fits 32 unsigned bits
    const unsigned first = tile * CLOUD_TILE + wave * (64 * CLOUD_ROUNDS) + lane;
    CloudPoint pt[CLOUD_ROUNDS];
    unsigned rank[CLOUD_ROUNDS];
    bool pack[CLOUD_ROUNDS];
    unsigned wcount = 0;  // packed by this wave so far: wave-uniform
#pragma unroll
    for (int r = 0; r < CLOUD_ROUNDS; ++r) {
        const unsigned i = first + 64 * r;
        pack[r] = false;
        pt[r] = CloudPoint{NAN, NAN, NAN, false};
        if (i < a.P) {
            const unsigned y = fdiv(i, a.fw), x = i - y * (unsigned)a.W;
            const bool lattice = a.points && x == fdiv(x, a.fs) * (unsigned)a.stride && y == fdiv(y, a.fs) * (unsigned)a.stride;
            if (lattice || (SCATTER && a.xyz)) pt[r] = cloud_point(a.disp[img + i], (int)x, (int)y, Q, a.z_min, a.z_max);
            if (SCATTER && a.xyz) {
                float* o = a.xyz + (img + i) * 3;
                o[0] = pt[r].keep ? pt[r].x : NAN;
                o[1] = pt[r].keep ? pt[r].y : NAN;
                o[2] = pt[r].keep ? pt[r].z : NAN;
            }
            pack[r] = lattice && pt[r].keep;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(pack[r]);
        rank[r] = wcount + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        wcount += (unsigned)__builtin_popcountll(m);
    }
    if (!a.points) return;  // xyz alone: one launch, nothing to pack (uniform over the grid)
    __shared__ unsigned wtot[CLOUD_THREADS / 64];
    if (lane == 0) wtot[wave] = wcount;
    __syncthreads();
    unsigned* slot = a.work + (size_t)sid * (size_t)a.pitch + tile;
    if (!SCATTER) {
        if (threadIdx.x == 0) *slot = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
        return;
    }
    unsigned off = *slot;
    for (unsigned w = 0; w < wave; ++w) off += wtot[w];
    uint4* out = a.points + (size_t)sid * (size_t)a.cap;
#pragma unroll
    for (int r = 0; r < CLOUD_ROUNDS; ++r) {
        const unsigned long long pos = (unsigned long long)off + rank[r];
        if (!pack[r] || pos >= (unsigned long long)a.cap) continue;
        unsigned rgba = 0xffffffffu;
        if (a.color) {
            const uint8_t* c = a.color + (img + (first + 64 * r)) * 3;
            const unsigned c0 = c[0], c1 = c[1], c2 = c[2];
            rgba = a.bgr ? (c2 | c1 << 8 | c0 << 16 | 0xff000000u) : (c0 | c1 << 8 | c2 << 16 | 0xff000000u);
        }
        out[pos] = make_uint4(__float_as_uint(pt[r].x), __float_as_uint(pt[r].y), __float_as_uint(pt[r].z), rgba);
    }
}

// one block per stream: work[0 .. tiles) from counts to their exclusive prefix sums, count[stream] = the total
__global__ __launch_bounds__(CLOUD_SCAN) void k_cloud_scan(unsigned* __restrict__ work, int tiles, long long pitch,
                                                           unsigned* __restrict__ count) {
    unsigned* w = work + (size_t)blockIdx.x * (size_t)pitch;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __shared__ unsigned wsum[CLOUD_SCAN / 64];
    unsigned carry = 0;  // the sum of all earlier steps: block-uniform
    for (int t0 = 0; t0 < tiles; t0 += CLOUD_SCAN) {
        const int t = t0 + (int)threadIdx.x;
        const unsigned c = t < tiles ? w[t] : 0u;
        unsigned v = c;  // inclusive scan within the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = (unsigned)__shfl_up((int)v, o);
            if ((int)lane >= o) v += u;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        unsigned pre = carry;
        for (unsigned k = 0; k < wave; ++k) pre += wsum[k];
        carry += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (t < tiles) w[t] = pre + (v - c);
        __syncthreads();  // wsum is rewritten by the next step
    }
    if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

}  // namespace

extern "C" long long sd_cloud_ws_bytes(int n, int H, int W, int stride) {
    if (n < 1 || n > 64 || !cloud_dims_ok(H, W) || stride < 1 || stride > 64) return -1;
    return n * 4 * cloud_pitch(H, W);
}

extern "C" int sd_cloud_build_n(int n, const float* disp, const uint8_t* color, int color_bgr, int H, int W,
                                const double* Qdev, float z_min, float z_max, int stride, float* xyz, void* points,
                                long long cap, unsigned* count, void* work, sd_stream s) {
    SD_REQUIRE(n >= 1 && n <= 64, "sd_cloud_build_n: n = %d streams (1..64)", n);
    SD_REQUIRE(disp, "sd_cloud_build_n: null disp");
    SD_REQUIRE(Qdev, "sd_cloud_build_n: null Qdev");
    SD_REQUIRE(color_bgr == 0 || color_bgr == 1, "sd_cloud_build_n: color_bgr %d (0 or 1)", color_bgr);
    SD_REQUIRE(cloud_dims_ok(H, W), "sd_cloud_build_n: bad sizes H x W = %d x %d (positive, H * W < 2^31)", H, W);
    SD_REQUIRE(z_min == z_min && z_max == z_max, "sd_cloud_build_n: z_min / z_max is NaN");
    SD_REQUIRE(z_min <= z_max, "sd_cloud_build_n: z_min %g > z_max %g", (double)z_min, (double)z_max);
    SD_REQUIRE(stride >= 1 && stride <= 64, "sd_cloud_build_n: stride %d (1..64)", stride);
    SD_REQUIRE(xyz || points, "sd_cloud_build_n: no output (xyz and points are both null)");
    if (points) {
        SD_REQUIRE((uintptr_t)points % 16 == 0, "sd_cloud_build_n: points must be 16-B aligned");
        SD_REQUIRE(count, "sd_cloud_build_n: points need count");
        SD_REQUIRE(cap >= 1, "sd_cloud_build_n: cap %lld (>= 1 with points)", cap);
        SD_REQUIRE(work && (uintptr_t)work % 4 == 0, "sd_cloud_build_n: points need a 4-B aligned work buffer");
    }
    CloudArgs a;
    a.disp = disp;
    a.color = color;
    a.Qdev = Qdev;
    a.xyz = xyz;
    a.points = static_cast<uint4*>(points);
    a.work = static_cast<unsigned*>(work);
    a.cap = cap;
    a.pitch = cloud_pitch(H, W);
    a.P = (unsigned)((long long)H * W);
    a.W = W;
    a.stride = stride;
    a.bgr = color_bgr;
    a.fw = make_fdiv((uint32_t)W);
    a.fs = make_fdiv((uint32_t)stride);
    a.z_min = z_min;
    a.z_max = z_max;
    const int tiles = (int)cloud_tiles(H, W);
    hipStream_t st = to_stream(s);
    const dim3 g(tiles, n), b(CLOUD_THREADS);
    if (points) {
        hipLaunchKernelGGL(k_cloud_tile<false>, g, b, 0, st, a);
        hipLaunchKernelGGL(k_cloud_scan, dim3(n), dim3(CLOUD_SCAN), 0, st, a.work, tiles, a.pitch, count);
    }
    hipLaunchKernelGGL(k_cloud_tile<true>, g, b, 0, st, a);
    return sd_check_launch("sd_cloud_build_n");
}
