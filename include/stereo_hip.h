/*
 * stereo_hip.h — C ABI of libstereo_hip.so, the MI355X (gfx950) kernel library
 * behind the stereo-disparity U-Net training path.
 *
 * The reference (sdfgeoff/stereo_depth_estimation) has no FFI: its boundary is the
 * PyTorch module / train-step API.  Every entry point below replaces
 * one ATen op family that the reference dispatches on that path; the reference
 * call site it replaces is cited per function.  Host-side mirror of the reference
 * interface: stereo_depth_estimation_amd/{model,engine,train}.py (Python, ctypes).
 *
 * Conventions
 *  - Plain C: raw device pointers, sizes, and a hipStream_t passed as an opaque
 *    pointer (sd_stream).  No torch types.  The caller (PyTorch) owns every buffer.
 *  - Every call is stream-ordered on the given stream, never synchronizes the device,
 *    never allocates or frees device memory (safe inside hipGraph capture).
 *  - Return 0 on success, SD_EINVAL for a rejected argument (checked on the host
 *    before any launch), SD_EHIP for a HIP launch error; sd_last_error() returns a
 *    thread-local message for the last failure.
 *  - Activations are NHWC, element type `dtype` (SD_F32 = fp32 parity mode, SD_BF16 =
 *    bf16 storage with fp32 accumulation).  Channel counts are multiples of 8.
 *  - Per-channel BN affines, statistics, parameters, gradients, optimizer state: fp32.
 */
#ifndef STEREO_HIP_H
#define STEREO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sd_stream; /* hipStream_t */

enum { SD_OK = 0, SD_EINVAL = 1, SD_EHIP = 2 };
enum { SD_F32 = 0, SD_BF16 = 1 };
/* gather transforms: identity, max(scale*x + shift, 0), scale*x + shift (fp8 quantisation of a signed source) */
enum { SD_IDENT = 0, SD_BNRELU = 1, SD_AFFINE = 2 };
/* conv-GEMM epilogues */
enum { SD_EPI_STORE = 0, SD_EPI_STATS = 1, SD_EPI_SPLIT = 2, SD_EPI_PIXSHUF = 3, SD_EPI_SPLIT_STATS = 4 };
/* weight-gradient layouts */
enum { SD_W_CONV3 = 0, SD_W_CONVT = 1, SD_W_ROWSUM = 2 };
/* heads modes */
enum { SD_HEADS_INFER = 0, SD_HEADS_LOSS = 1, SD_HEADS_GRADS = 2 };

/*
 * Operand source of an implicit GEMM (the im2col gather).  Up to two NHWC sources
 * concatenated along channels (model.py:89-95 torch.cat([up, skip], 1)); each with an
 * optional fused BN+ReLU transform y -> max(scale[c]*y + shift[c], 0) (model.py:37-41),
 * an optional 2x2 max pool after the transform (model.py:59,83-86), and a tap pattern:
 *   taps = 1  : 1x1 (pixel (h,w) of the GEMM grid)
 *   taps = 9  : 3x3, pad 1 (pixel (h+kh-1, w+kw-1)), K index = tap*Ctot + c
 *   taps = 4  : 2x2 sub-pixel gather from a 2x-resolution source (2h+a, 2w+b)
 * H, W are the source's stored spatial dims.  Ctot = chans[0] + chans[1].
 */
typedef struct sd_src {
    const void* ptr[2];
    const float* scale[2];
    const float* shift[2];
    int chans[2];
    int xform[2];
    int H, W;
    int taps;
    int pool;
} sd_src;

int sd_version(void);
/* Diagnostics: device buffer for the per-wave cycle counters of timing builds (-DWG_EXP=1024; no effect
   otherwise). Not a reference interface. */
int sd_debug_buffer(void* dev_ptr);
/* Diagnostics: effective shader clock under MFMA load (bench.py "clock"). blocks x 256 threads of back-to-back bf16
   MFMAs; out[4 * block + {0,1,2,3}] = s_memtime start/end, s_memrealtime (100 MHz) start/end; sink: >= 256 floats
   (never written in practice). Not a reference interface. */
int sd_clock_probe(int blocks, int iters, unsigned long long* out, float* sink, sd_stream s);
const char* sd_last_error(void);
int sd_device_init(int device);

/* ---- packing (weights are fp32 PyTorch layout in, dtype MFMA-ready layout out) ---- */
/* reference input [B,6,H,W] f32 (train.py:320) -> NHWC dtype with cpad channels (zero pad). */
int sd_pack_input(int dtype, const float* x_nchw, int batch, int cin, int H, int W, int cpad, void* out, sd_stream s);
/* The same pack, also writing max |x| over the batch as float bits into amax[slot] (atomicMax into a zeroed word) and
 * zeroing amax[clear] for a later call (clear < 0: none): the fp8 live loop's input-range check (a frame brighter than
 * the calibration frame of the static e4m3 scales triggers a recalibration), read back asynchronously. */
int sd_pack_input_amax(int dtype, const float* x_nchw, int batch, int cin, int H, int W, int cpad, void* out,
                       unsigned* amax, int slot, int clear, sd_stream s);
/* Conv2d(k3,p1,no bias) weight [co][ci][3][3] (model.py:36,39) -> fwd [co][kpad] (k = tap*ci_pad + ci)
 * or, dgrad != 0, the flipped/transposed [ci][kpad] (k = tap*co + o, W[o][ci][8-tap]). */
int sd_pack_conv3_w(int dtype, const float* w, int co, int ci, int ci_pad, int dgrad, int kpad, void* out, sd_stream s);
/* ConvTranspose2d(k2,s2) weight [ci][co][2][2] (model.py:67-73) -> fwd [(t,o)][kpad=ci]
 * or, dgrad != 0, [ci][kpad] (k = t*co + o). */
int sd_pack_convT_w(int dtype, const float* w, int ci, int co, int dgrad, int kpad, void* out, sd_stream s);
/* Every pack of a step in ONE launch (the per-tensor forms above, up to 64 jobs): job j writes
 * out + out_off (elements of dtype) exactly as the per-tensor call of its kind would.
 * The weights it reads are the reference's Conv2d/ConvTranspose2d parameters (model.py:36,39,67-73). */
enum { SD_PACK_CONV3_FWD = 0, SD_PACK_CONV3_DGRAD = 1, SD_PACK_CONVT_FWD = 2, SD_PACK_CONVT_DGRAD = 3,
       /* bf16 hi/lo pairs of the fp32 weights (w = hi + lo to ~2^-17 relative; sd_conv3x3_wsplit and the doubled-K
        * ConvTranspose forward): conv3 fwd [co][kpad], k = tap*2*ci_pad + {ci: hi | ci_pad + ci: lo};
        * convT fwd [(t,o)][kpad], k = {i: hi | ci + i: lo} */
       SD_PACK_CONV3_FWD_SPLIT = 4, SD_PACK_CONVT_FWD_SPLIT = 5 };
typedef struct sd_pack_job {
    const float* w; /* fp32 PyTorch layout: conv3 [co][ci][3][3], convT [ci][co][2][2] */
    int kind;
    int co, ci, ci_pad; /* ci_pad: conv3 fwd only */
    int kpad;
    int64_t out_off;
} sd_pack_job;
int sd_pack_weights(int dtype, const sd_pack_job* jobs, int njobs, void* out, sd_stream s);

/* ---- implicit-GEMM convolution (replaces mkldnn_convolution / convolution_backward dgrad,
 *      model.py:36,39,67-77) ----
 * out[m, n] = sum_k A[m,k] * Wp[n,k], m = (b,h,w) over batch x H x W, n < N, k < K.
 * epi SD_EPI_STORE  : out0 NHWC [M][N]
 *     SD_EPI_STATS  : as STORE + stats[rows][N] float2 (sum, sumsq) per M-block (BN batch stats)
 *     SD_EPI_SPLIT  : n < n_split -> out0 [M][n_split], else out1 [M][N-n_split]  (cat backward)
 *     SD_EPI_PIXSHUF: n = t*C + o -> out0 [b][2h+t/2][2w+t%2][o] + bias[o]  (ConvTranspose2d)
 *     SD_EPI_SPLIT_STATS: SPLIT + stats rows over all N columns (bf16, 3x3 halo shapes only): the dgrad of a
 *                    decoder conv0 also yields the column sums of d(up), the ConvTranspose2d bias gradient
 *                    (sd_stat_rows_sum) */
int sd_conv_gemm(int dtype, const sd_src* a, int batch, int H, int W, const void* wpack, int N, int kpad, int epi,
                 void* out0, void* out1, int n_split, const float* bias, float* stats, sd_stream s);
/* number of float2 stat rows sd_conv_gemm(SD_EPI_STATS) writes for this shape */
int sd_conv_gemm_stat_rows(int dtype, int batch, int H, int W, int N);
/* name of the kernel instance sd_conv_gemm / sd_wgrad_gemm launches for a shape (as rocprofv3 shows it) */
const char* sd_conv_gemm_kernel_name(int dtype, const sd_src* a, int batch, int H, int W, int N, int epi);
const char* sd_wgrad_kernel_name(int dtype, const sd_src* a, const sd_src* b, int M, int N);

/* sd_conv_gemm(SD_EPI_STORE) of a dgrad whose output `out` is the upstream gradient da of a BatchNorm layer with raw
 * output y (model.py:37,40): the same launch also writes that layer's BatchNorm-backward partial sums (what
 * sd_bn_bwd_reduce computes from da and y in a pass of its own), sd_conv_gemm_bnsum_rows() rows of float2[N],
 * for sd_bn_bwd_finalize. bf16 3x3 halo shapes and the ConvTranspose2d dgrad (4-tap sub-pixel source, model.py:67-73)
 * where the LDS-resident-weight kernel takes it: sd_conv_gemm_bnsum_ok. */
int sd_conv_gemm_bnsum(int dtype, const sd_src* a, int batch, int H, int W, const void* wpack, int N, int kpad,
                       void* out, const void* y, const float* scale, const float* shift, const float* mean,
                       const float* invstd, float* partials, sd_stream s);
int sd_conv_gemm_bnsum_ok(int dtype, const sd_src* a, int N);

/* The bf16 3x3 convolution (model.py:36,39) of the halo kernel with two precision options for the eval forwards:
 *  flags & SD_CONV_WSPLIT: the fp32 weights as bf16 hi/lo pairs (sd_pack_weights kind SD_PACK_CONV3_FWD_SPLIT): each
 *      chunk of input channels meets the hi then the lo halves, so the weights carry fp32 precision into the MFMA
 *      while the activations stay bf16 (twice the MFMA work). The weights' bf16 rounding is a systematic change of
 *      the function that shifted the EPE of trained checkpoints by 2e-3..1e-2 px (tools/precision_study.py).
 *  out_scale / out_shift (both or neither; STORE only): the stored value is bf16(acc*out_scale[n] + out_shift[n]),
 *      the layer's eval-mode BatchNorm applied before the rounding (model.py:37,40), so consumers apply only the ReLU
 *      (pass scale 1, shift 0) and bf16 keeps its relative precision on the normalised activation.
 * epi: SD_EPI_STORE or SD_EPI_STATS (stats as sd_conv_gemm). bf16 3x3 halo shapes only (N = 32 or N % 64 == 0,
 * unpooled source): sd_conv3x3_ex_ok. */
enum { SD_CONV_WSPLIT = 1 };
int sd_conv3x3_ex(const sd_src* a, int batch, int H, int W, const void* wpack, int N, int kpad, int epi, int flags,
                  const float* out_scale, const float* out_shift, void* out, float* stats, sd_stream s);
int sd_conv3x3_ex_ok(const sd_src* a, int N);
const char* sd_conv3x3_ex_kernel_name(const sd_src* a, int H, int W, int N, int epi, int flags, int out_affine);
/* The same with a split-K workspace: a STORE launch whose items would leave most CUs idle (the batch-1 forwards of the
 * deep layers) runs in groups of blocks over slices of the input-channel chunks (and of the hi/lo passes), and a
 * second launch adds their fp32 partial sums, applies the output affine and stores bf16. ws (16-B aligned) must hold
 * sd_conv3x3_ex_ws_bytes(...) bytes (0: no split for the shape); a NULL or smaller ws runs unsplit. Results equal
 * sd_conv3x3_ex's up to the fp32 summation order. */
long long sd_conv3x3_ex_ws_bytes(const sd_src* a, int batch, int H, int W, int N, int epi, int flags);
int sd_conv3x3_ex_ws(const sd_src* a, int batch, int H, int W, const void* wpack, int N, int kpad, int epi, int flags,
                     const float* out_scale, const float* out_shift, void* out, float* stats, void* ws,
                     long long ws_bytes, sd_stream s);
int sd_conv_gemm_bnsum_rows(const sd_src* a, int batch, int H, int W, int N);
const char* sd_conv_gemm_bnsum_kernel_name(const sd_src* a, int H, int W, int N);

/* ---- weight gradient (replaces convolution_backward wgrad, model.py:36,39,67-73) ----
 * slab[z][m][n] = sum over the z-th pixel range of A(p, m) * B(p, n), p over batch x H x W. */
int sd_wgrad_splits(int dtype, int batch, int H, int W, int M, int N);
int sd_wgrad_gemm(int dtype, const sd_src* a, const sd_src* b, int batch, int H, int W, int M, int N, float* slab,
                  int splits, sd_stream s);
/* The BatchNorm2d backward apply (sd_bn_bwd_apply, model.py:37,40) fused into the bf16 3x3 weight gradient
 * (convolution_backward wgrad, model.py:36,39): the kernel stages A = dy formed from the raw pair
 * (da, y) as sd_bn_bwd_apply defines it, dy = coef0*(dz - coef1 - xhat*coef2), dz = da*[scale*y+shift > 0],
 * xhat = (y-mean)*invstd, and also writes that dy to a->ptr[0] ([pixels][M], for the dgrad). Same b/slab/splits
 * contract as sd_wgrad_gemm (a: the plain 1x1 [pixels][M] source, used as the dy destination). The kernel
 * takes coef0 = scale (both are gamma*invstd as sd_bn_fwd_finalize / sd_bn_eval_coeffs and
 * sd_bn_bwd_finalize write them) and reads coef1, coef2 from coef. a->ptr[0] may be NULL: dy is not written
 * (a layer without a dgrad); the shapes with x channels not a multiple of 32 (M = 32 only) require that.
 * sd_wgrad_bnbwd_ok: 0 when the shape has no fused kernel (then apply + sd_wgrad_gemm), else the number of
 * x-channel blocks that each form the same dy tile (1: dy is formed once; more: the transform is repeated per
 * block, which costs more than the separate apply pass at the model's deep layers). */
int sd_wgrad_bnbwd_ok(int dtype, const sd_src* a, const sd_src* b, int M, int N);
int sd_wgrad_gemm_bnbwd(int dtype, const sd_src* a, const sd_src* b, int batch, int H, int W, int M, int N,
                        const void* da, const void* y, const float* scale, const float* shift, const float* mean,
                        const float* invstd, const float* coef, float* slab, int splits, sd_stream s);
const char* sd_wgrad_bnbwd_kernel_name(const sd_src* a, const sd_src* b, int M, int N);
/* sum the slabs and write the PyTorch-layout fp32 gradient:
 *   SD_W_CONV3: M = co, N = 9*ci_pad -> dw[co][ci_real][3][3]
 *   SD_W_CONVT: M = ci, N = 4*co     -> dw[ci][co][2][2] */
int sd_wgrad_reduce(const float* slab, int splits, int M, int N, int layout, int ci_real, float* dw, sd_stream s);
/* up to 48 of those reduces in ONE launch, each bit-identical to its sd_wgrad_reduce call (the slabs must be
 * distinct buffers: the engine defers a step's reduces into one launch per gradient-ready group).
 * layout SD_W_ROWSUM: dw[c] = sum over r < splits of ((const float2*)slab)[r * N + c].x for c < ci_real (M = 1),
 * bit-identical to sd_stat_rows_sum(slab, splits, N, ci_real, dw): the ConvTranspose2d bias gradients joined to the
 * batch instead of a launch each */
typedef struct sd_wred_job {
    const float* slab;
    int splits, M, N, layout, ci_real;
    float* dw;
} sd_wred_job;
int sd_wgrad_reduce_batch(const sd_wred_job* jobs, int njobs, sd_stream s);

/* ---- host data path: the reference's sample cache (dataset.py:86-105 load_cached_sample; cache.py:50-112) ----
 * Reads n np.savez cache files (stored zip of left.npy / right.npy uint8 [H][W][3], disparity.npy f16 [H][W]) with
 * `threads` host threads into left/right [n][H][W][3] and disparity [n][H][W] (f16 bits). Returns 0, or 1 + the index
 * of the first file that is missing, compressed, or of another dtype/shape (message in err), or -1 for bad args. */
int sd_read_cache_batch(const char* const* paths, int n, int H, int W, uint8_t* left, uint8_t* right,
                        uint16_t* disparity, int threads, char* err, int errlen);

/* Writes n cache files in that format from host buffers left/right [n][H][W][3], disp_f16 [n][H][W] with at most
 * min(threads, 16) host threads: a zip of left.npy, right.npy, disparity.npy (version-1.0 .npy headers, C order), members
 * stored (compress == 0, np.savez) or raw-deflated (np.savez_compressed). Each file is written under a temporary name
 * in its own directory (which must exist) and renamed over the target, so a target is either absent, its earlier self
 * or complete. Returns 0, or 1 + the index of the first path that failed (path and reason in err; its temporary file
 * removed, an earlier file at the target untouched; the other files are still written), or -1 for bad args. */
int sd_write_cache_batch(const char* const* paths, int n, int H, int W, const uint8_t* left, const uint8_t* right,
                         const uint16_t* disp_f16, int compress, int threads, char* err, int errlen);

/* PNG frames of the un-cached source (reference dataset.py:23-30,184-212: PIL open + convert("RGB")): 8-bit RGB or
 * RGBA, not interlaced. sd_png_size reads the IHDR; sd_read_png_batch decodes n frames of H x W with `threads` host
 * threads into out [n][H][W][3]. Returns as sd_read_cache_batch (other PNG kinds: an error, for a PIL fallback). */
int sd_png_size(const char* path, int* height, int* width);
int sd_read_png_batch(const char* const* paths, int n, int H, int W, uint8_t* out, int threads, char* err, int errlen);

/* ---- BatchNorm2d train/eval (model.py:37,40; native_batch_norm / _backward) ---- */
int sd_bn_fwd_finalize(const float* stats, int rows, int C, double count, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                       float eps, float* mean, float* invstd, float* scale, float* shift, sd_stream s);
int sd_bn_eval_coeffs(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
                      int C, float eps, float* mean, float* invstd, float* scale, float* shift, sd_stream s);
/* rows of float2 partials sd_bn_bwd_reduce / sd_chan_sum write */
int sd_chan_reduce_rows(int64_t pixels, int C);
/* partial (sum dz, sum dz*xhat), dz = da * [scale*y+shift > 0], xhat = (y-mean)*invstd */
int sd_bn_bwd_reduce(int dtype, const void* da, const void* y, const float* scale, const float* shift,
                     const float* mean, const float* invstd, int64_t pixels, int C, float* partials, sd_stream s);
/* -> dgamma, dbeta (fp32, into the flat grad buffer) and coef[C][3] = {gamma*invstd, sum dz/N, sum dz*xhat/N};
 * batch_stats = 0 (forward used running stats, eval mode): coef = {gamma*invstd, 0, 0}. */
int sd_bn_bwd_finalize(const float* partials, int rows, int C, double count, const float* gamma,
                       const float* invstd, int batch_stats, float* dgamma, float* dbeta, float* coef, sd_stream s);
/* SyncBatchNorm (SURVEY §8e "--sync-bn"; torch.nn.SyncBatchNorm semantics, replacing the per-rank reductions of
 * model.py:37,40 under DDP). Each rank reduces its float2 partial rows (the producer's STATS rows, or the
 * BatchNorm-backward partials) to fp64 sums[2C + 1]: per channel (sum, sumsq), then this rank's pixel count; the
 * host all-reduces the whole vector (SUM) across ranks, so the count that arrives is the global one whatever each
 * rank's batch size; the finalizes below read it from sums[2C]. The backward writes dgamma/dbeta from local_sums
 * (the gradient all-reduce adds the ranks' shares) and coef from global_sums. */
int sd_bn_rows_sum64(const float* rows, int nrows, int C, double pixels, double* sums, sd_stream s);
int sd_bn_fwd_finalize64(const double* sums, int C, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                         float eps, float* mean, float* invstd, float* scale, float* shift, sd_stream s);
int sd_bn_bwd_finalize64(const double* local_sums, const double* global_sums, int C, const float* gamma,
                         const float* invstd, int batch_stats, float* dgamma, float* dbeta, float* coef, sd_stream s);
/* dy = coef0 * (dz - coef1 - xhat*coef2) */
int sd_bn_bwd_apply(int dtype, const void* da, const void* y, const float* scale, const float* shift,
                    const float* mean, const float* invstd, const float* coef, int64_t pixels, int C, void* dy,
                    sd_stream s);
/* MaxPool2d(2) backward (first max in row-major window order, as ATen CPU) + skip-gradient add:
 * da[b,h,w,c] = dskip[b,h,w,c] + (argmax ? dpool[b,h/2,w/2,c] : 0); dskip may be NULL.
 * partials != NULL: also the BatchNorm-backward partial sums of this layer (what sd_bn_bwd_reduce
 * computes from da and y, here from registers), sd_pool_bwd_rows() rows of float2[C], for
 * sd_bn_bwd_finalize; needs mean/invstd and C/8 dividing 256. */
int sd_pool_bwd_add(int dtype, const void* y, const float* scale, const float* shift, const void* dskip,
                    const void* dpool, int batch, int H, int W, int C, void* da, const float* mean,
                    const float* invstd, float* partials, sd_stream s);
int sd_pool_bwd_rows(int batch, int H, int W, int C);
/* bf16: materialise MaxPool2d(2)(relu(scale*y + shift)) [b][H/2][W/2][C] (model.py:59,83-86) so the
 * next conv's gather is a plain read (the fp32 parity path pools inside the gather instead) */
int sd_bnrelu_pool(int dtype, const void* y, const float* scale, const float* shift, int batch, int H, int W, int C,
                   void* out, sd_stream s);
/* column sums over pixels (ConvTranspose2d bias grad): partials then out[C] = sum (fp32) */
int sd_chan_sum(int dtype, const void* x, int64_t pixels, int C, float* partials, float* out, sd_stream s);
/* out[c] = sum over rows of stats[r][c].sum (float2 rows of ld columns, c < C; fp64 accumulation): the column
 * sums of an SD_EPI_SPLIT_STATS (or STATS) launch, e.g. the ConvTranspose2d bias gradient (model.py:67-73) */
int sd_stat_rows_sum(const float* stats, int rows, int ld, int C, float* out, sd_stream s);

/* ---- heads + loss (model.py:76-77,98,103; train.py:329-356) ----
 * act = max(scale*y + shift, 0) [pixels][C] (dec1 output), head weights wd/wl [C], biases bd/bl [1].
 * INFER : disp = softplus(act.wd + bd), logvar = clamp(act.wl + bl, -6, 3)
 * LOSS  : + masked heteroscedastic NLL with n = *count valid pixels (mask & isfinite(target)):
 *         da[pixels][C] (dtype) = d loss / d act; partials for head grads and metric sums
 * GRADS : da from given dense gdisp/glogvar (autograd path) */
/* valid pixels of a batch (train.py:329-330: valid_mask & isfinite(target)) into count[0..ncount-1] (1-4 counters, all
 * set to the same value: this rank's count and the loss normaliser that DDP all-reduces, without a copy launch).
 * clear == NULL: count is zeroed first (a memset); else count must already be zero and the kernel zeroes
 * clear[0..ncount-1] for the caller's next call (double-buffered counters: one launch per batch). */
int sd_count_valid(const float* target, const uint8_t* mask, int64_t pixels, int* count, int ncount, int* clear,
                   sd_stream s);
/* the train step's prologue in ONE launch (train.py:320-330 before the forward): sd_pack_weights(dtype, jobs, njobs,
 * wpack), sd_pack_input(dtype, x, batch, cin, H, W, cpad, xout) and sd_count_valid(target, mask, pixels, count, ncount,
 * clear) with a non-NULL clear, a 4-B aligned mask and 16-B aligned targets; the same results as the three calls */
int sd_step_prologue(int dtype, const sd_pack_job* jobs, int njobs, void* wpack, const float* x, int batch, int cin,
                     int H, int W, int cpad, void* xout, const float* target, const uint8_t* mask, int64_t pixels,
                     int* count, int ncount, int* clear, sd_stream s);
int sd_heads_rows(int64_t pixels);
int sd_heads(int dtype, int mode, const void* y, const float* scale, const float* shift, int64_t pixels, int C,
             const float* wd, const float* bd, const float* wl, const float* bl, float* disp, float* logvar,
             const float* target, const uint8_t* mask, const int* count, const float* gdisp, const float* glogvar,
             void* da, float* partials, sd_stream s);
/* sd_heads (LOSS / GRADS) that also writes the BatchNorm-backward partial sums of the dec1 layer it
 * reads (replaces sd_bn_bwd_reduce over da and y, model.py:40-41 backward): bnpart[sd_heads_rows][C]
 * float2 = (sum dz, sum dz*xhat), dz = da (as stored) where y*scale+shift > 0, xhat = (y-mean)*invstd */
int sd_heads_bnsum(int dtype, int mode, const void* y, const float* scale, const float* shift, int64_t pixels, int C,
                   const float* wd, const float* bd, const float* wl, const float* bl, float* disp, float* logvar,
                   const float* target, const uint8_t* mask, const int* count, const float* gdisp,
                   const float* glogvar, void* da, float* partials, const float* mean, const float* invstd,
                   float* bnpart, sd_stream s);
/* reduce heads partials: head grads into dwd[C], dbd[1], dwl[C], dbl[1] (skipped if NULL) and
 * metric sums (sum nll, sum |d|, sum d^2, sum exp(lv/2), n) added into metrics[5] (fp64). */
int sd_heads_finalize(const float* partials, int rows, int C, float* dwd, float* dbd, float* dwl, float* dbl,
                      double* metrics, const int* count, sd_stream s);

/* ---- fp8 (OCP e4m3) inference forward of the 3x3 convolutions (eval-mode model.py:36-41 as the live app
 *      runs it, depth_live_dl.py:516-529) ----
 * Activations stay bf16 NHWC. Each source of `a` carries its folded quantisation affine in scale/shift:
 * q = e4m3(clamp(xform(x*scale + shift), +-448)), xform = ReLU for SD_BNRELU, none for SD_AFFINE
 * (sd_fp8_qparams computes them). Weights: sd_pack_conv3_w_fp8, e4m3 [co][kpad] (k = tap*ctap + c,
 * ctap = ctot rounded up to 16) with one fp32 scale per output channel.
 * out[m][n] (bf16) = act_scale[0] * wscale[n] * sum_k q[m][k] * wq[n][k]   (v_mfma_scale_f32_32x32x64_f8f6f4)
 * minmax: sd_conv3x3_fp8_rows() rows of float2[N] = (min, max) of the stored outputs, per block. */
int sd_pack_conv3_w_fp8(const float* w, int co, int ci, int ci_pad, int kpad, void* out, float* scale, sd_stream s);
int sd_conv3x3_fp8(const sd_src* a, int batch, int H, int W, const void* wq, const float* wscale,
                   const float* act_scale, int N, int kpad, void* out, float* minmax, sd_stream s);
int sd_conv3x3_fp8_rows(int batch, int H, int W, int N);
const char* sd_conv3x3_fp8_kernel_name(int N);
/* per-channel (min, max) rows of a bf16 NHWC tensor [pixels][C] (sources no fp8 conv produced: the packed
 * input, ConvTranspose outputs): sd_chan_minmax_rows() rows of float2[C] */
int sd_chan_minmax_rows(int64_t pixels, int C);
int sd_chan_minmax(const void* x, int64_t pixels, int C, float* rows, sd_stream s);
/* Dynamic activation scale of one conv input (1 or 2 concatenated sources): amax over the sources of
 * xform(scale*x + shift) from their (min, max) rows (identity affine when scale == NULL),
 * act_scale[0] = s_a = amax / 448, and per source the folded affine for the fp8 gather:
 * qscale = scale / s_a, qshift = shift / s_a (or 1/s_a, 0 when scale == NULL or ident: the consumer
 * reads the already-transformed tensor, e.g. the materialised MaxPool of relu(bn(y))). */
typedef struct sd_qsrc {
    const float* rows; /* [nrows][C] float2 (min, max) */
    int nrows;
    int C;
    const float* scale; /* per-channel affine before the quantisation, NULL = identity */
    const float* shift;
    int relu;
    int ident;
    float* qscale; /* out [C] */
    float* qshift; /* out [C] */
} sd_qsrc;
int sd_fp8_qparams(const sd_qsrc* src, int nsrc, float* act_scale, sd_stream s);
/* The same conv with STATIC scales (the engine's forwards after its calibration forward, while the model state is
 * unchanged): act_scale and the sources' folded affines are the ones sd_fp8_qparams left; no min/max rows are
 * written. Same operands and result contract as sd_conv3x3_fp8 otherwise (N = 32 or a multiple of 64, <= 512 input
 * channels; a concatenation's first source a multiple of 16 channels). */
int sd_conv3x3_q8(const sd_src* a, int batch, int H, int W, const void* wq, const float* wscale,
                  const float* act_scale, int N, int kpad, void* out, sd_stream s);
const char* sd_conv3x3_q8_kernel_name(int batch, int H, int W, int N, int c0, int c1);

/* ---- fused backward of a full-resolution 32 -> 32 conv + BatchNorm + ReLU layer (model.py:36-41: enc1.1, dec1.1)
 * One pass over the layer: dy = BatchNorm-backward(da, y) (scale, shift, mean, invstd: this layer's forward
 * coefficients, coef: its [C][3] backward coefficients from sd_bn_bwd_finalize), never stored; the weight gradient as
 * split-K slabs slab[splits][32][288] (k = tap*32 + ci, reduced by sd_wgrad_reduce with SD_W_CONV3); dx = the dgrad
 * (wd: sd_pack_conv3_w dgrad layout, kpad >= 288) into dx, which is da of the previous BatchNorm layer, whose raw
 * output yp and coefficients (pscale, pshift: x = relu(pscale*yp + pshift); pmean, pinvstd) it takes; and that
 * layer's BatchNorm-backward sums (sum dz, sum dz*xhat) as partials[splits][32] float2, for sd_bn_bwd_finalize.
 * Replaces sd_wgrad_gemm_bnbwd + sd_conv_gemm_bnsum for these layers. splits = sd_conv3x3_bwd_fused_splits(...). */
int sd_conv3x3_bwd_fused_ok(int C, int Cx, int H, int W);
int sd_conv3x3_bwd_fused_splits(int batch, int H, int W);
int sd_conv3x3_bwd_fused(const void* da, const void* y, const float* scale, const float* shift, const float* mean,
                         const float* invstd, const float* coef, const void* yp, const float* pscale,
                         const float* pshift, const float* pmean, const float* pinvstd, const void* wd, int kpad,
                         int batch, int H, int W, void* dx, float* slab, float* partials, sd_stream s);
/* The same for the full-resolution decoder conv0 (model.py:89-95, dec1.0: cat(u, relu(sscale*xs + sshift)), 32 + 32
 * -> 32 channels): dy from (da, y) as above; the weight gradient as slab[splits][32][576] (k = tap*64 + ci, ci < 32 the
 * u half; sd_wgrad_reduce with SD_W_CONV3, ci_real 64); the 64-channel dgrad (wd: [64][kpad], kpad >= 288) stored
 * split, du = its first 32 channels (d(u), the ConvTranspose2d output gradient), dskip the other 32; and the column
 * sums of du (the ConvTranspose2d bias gradient) as partials[splits][32] float2 (sum, 0) for sd_stat_rows_sum(ld 32).
 * Replaces sd_wgrad_gemm_bnbwd (two 32-channel x blocks) + the SD_EPI_SPLIT_STATS dgrad. */
int sd_conv3x3_bwd_fused_dec_ok(int C, int Cu, int Cs, int H, int W);
int sd_conv3x3_bwd_fused_dec(const void* da, const void* y, const float* scale, const float* shift, const float* mean,
                             const float* invstd, const float* coef, const void* xu, const void* xs,
                             const float* sscale, const float* sshift, const void* wd, int kpad, int batch, int H,
                             int W, void* du, void* dskip, float* slab, float* partials, sd_stream s);

/* ---- AdamW (train.py:343,578; torch 2.10 single-tensor AdamW, decoupled weight decay) ----
 * One flat fp32 parameter/gradient/state buffer (all tensors share lr/betas/eps/wd).
 * The step is skipped (and *step not advanced) when *count == 0 (train.py:331-332). One launch: scratch[0] is the
 * kernel's block counter (zero before the first call; every call leaves it zero). */
int sd_adamw(float* p, const float* g, float* m, float* v, int64_t n, double lr, double weight_decay, double beta1,
             double beta2, double eps, int* step, const int* count, float* scratch /* 4 floats */, sd_stream s);

/* ---- data path (dataset.py:184-212): bilinear resize, align_corners=False, no antialias ----
 * in [planes][Hi][Wi] f32 -> out [planes][Ho][Wo] f32, times `mul` (disparity width scaling). */
int sd_resize_bilinear(const float* in, int planes, int Hi, int Wi, float* out, int Ho, int Wo, float mul, sd_stream s);

/* ---- on-device sample preparation (replaces FoundationStereoDataset.__getitem__'s tensor work,
 * dataset.py:184-212,305-311, which the reference runs in DataLoader workers) ----
 * Raw samples, uint8 HWC at the source resolution as PIL decodes them (RGB order):
 *   left, right [B][Hs][Ws][3]; disparity RGB24 [B][Hs][Ws][3] (depth_uint8_decoding, dataset.py:23-30)
 * -> input  [B][6][Ho][Wo] f32: left RGB/255 then right, bilinear (align_corners=False), dataset.py:184-193
 *    target [B][1][Ho][Wo] f32: (R*255*255 + G*255 + B)/1000, bilinear, times Wo/Ws, dataset.py:195-212
 *    valid  [B][1][Ho][Wo] u8 : target > 0, dataset.py:306
 * Optional asymmetric colour augmentation (dataset.py:248-270) is applied afterwards by sd_augment_rgb. */
int sd_stereo_preprocess(const uint8_t* left, const uint8_t* right, const uint8_t* disp_rgb, int batch, int Hs,
                         int Ws, int Ho, int Wo, float* input, float* target, uint8_t* valid, sd_stream s);
/* Cached samples (load_cached_sample, dataset.py:86-105): left/right uint8 [B][Ho][Wo][3] and disparity
 * f16 [B][Ho][Wo] already at the training resolution -> the same three outputs. */
int sd_stereo_from_cache(const uint8_t* left, const uint8_t* right, const uint16_t* disp_f16, int batch, int Ho,
                         int Wo, float* input, float* target, uint8_t* valid, sd_stream s);
/* The cache builder's kernel (reference cache.py:50-112 + save_cached_sample, dataset.py:110-128): the inputs of
 * sd_stereo_preprocess -> the cache's own layout, out_left/out_right uint8 [B][Ho][Wo][3] and out_disp_f16 f16 bits
 * [B][Ho][Wo], i.e. the buffers sd_read_cache_batch fills and sd_stereo_from_cache consumes. Per pixel the fp32 values
 * are those of sd_stereo_preprocess (the same device code); colour = (uint8) clip(x * 255, 0, 255) truncated,
 * disparity = float16(target), round to nearest even (subnormals kept, overflow to inf). Four pixels per thread with
 * word stores when Wo % 4 == 0, out_left/out_right are 4-B and out_disp_f16 is 8-B aligned; a per-pixel form otherwise.
 * Allocates nothing, does not synchronise. */
int sd_stereo_to_cache(const uint8_t* left, const uint8_t* right, const uint8_t* disp_rgb, int batch, int Hs, int Ws,
                       int Ho, int Wo, uint8_t* out_left, uint8_t* out_right, uint16_t* out_disp_f16, sd_stream s);
/* Asymmetric colour augmentation (FoundationStereoDataset._augment_rgb, dataset.py:248-270, torchvision 0.25
 * functional ops), in place on input [B][6][H][W] f32 = 2B RGB images (left, right of each pair).
 * params [2B][7] f32 per image: brightness, contrast, saturation factors, hue shift, gamma, blur sigma
 * (0 = no blur), noise std. blur_ksize odd in [3, 31]. Noise: counter-based N(0,1) keyed by `seed`.
 * work: 8-B aligned scratch of B*6*H*W + 128*B floats (the images, then 64 fp64 contrast partial sums per pair). */
int sd_augment_rgb(float* input, int batch, int H, int W, const float* params, int blur_ksize, uint64_t seed,
                   float* work, sd_stream s);

/* ---- on-device frame path of the live loop (live_camera/depth_live_dl.py around model(x)) ----
 * Frames are BGR uint8 [Hc][Wc][3] as cv2 captures them; the model runs at [H][W]; B = 1. All buffers are the
 * caller's, nothing allocates or synchronises (graph-capturable).
 *
 * Front end (depth_live_dl.py:476-493 cv2.remap, :225-229 cvtColor / resize / /255, :516-520 cat + upload) and the
 * engine's input pack in one pass. Per side, optional rectification maps in OpenCV's CV_16SC2 fixed-point format (as
 * RectificationData holds them): map1 int16 [Hc][Wc][2] = integer x, y; map2 uint16 [Hc][Wc], low 10 bits =
 * fy5 << 5 | fx5, fractions in 1/32 px (NULL, NULL: no rectification). Remap: bilinear, a tap outside the frame
 * contributes 0. Resize: bilinear on half-pixel centres with edge replicate, taken over the remapped image (<= 16 source
 * taps per value). fp32 throughout, / 255 last. OpenCV's uint8 intermediate and fixed-point tables are not reproduced.
 *   xin  : NHWC dtype (SD_F32 / SD_BF16), 8 channels [L_R, L_G, L_B, R_R, R_G, R_B, 0, 0]: the engine's input,
 *          bit-identical to sd_pack_input(dtype, nchw, 1, 6, H, W, 8, xin)
 *   nchw : optional f32 [6][H][W], the reference's model_input
 *   amax : optional; as sd_pack_input_amax (atomicMax of max|x| into amax[slot], amax[clear] zeroed, clear < 0: none) */
int sd_live_frontend(int dtype, const uint8_t* left, const uint8_t* right, int Hc, int Wc, const int16_t* map1_l,
                     const uint16_t* map2_l, const int16_t* map1_r, const uint16_t* map2_r, int H, int W, void* xin,
                     float* nchw, unsigned* amax, int slot, int clear, sd_stream s);
/* The rectified view for display (:489): the remap alone, rounded half to even -> uint8 BGR [Hc][Wc][3]. */
int sd_live_rectify(const uint8_t* frame, int Hc, int Wc, const int16_t* map1, const uint16_t* map2, uint8_t* view,
                    sd_stream s);
/* Post stage on the heads' f32 [H][W] maps, numpy float32 arithmetic (scalars are the caller's float32 casts):
 *   EMA (:531-540)       state = copy ? disp : alpha * disp + one_minus_alpha * state   (copy: first frame or alpha 0)
 *   depth (:371-377)     depth = focal_baseline / state where state is finite and > 1e-6, else NaN   (depth_on)
 *   confidence (:380-381) conf = exp(-0.5 * logvar)                                                   (logvar != NULL)
 *   codes (:237-250, fixed range) code = trunc(clip((v - lo) / scale, 0, 1) * 255) for finite v > 0, else 0; u8 [H][W],
 *                        depth_code of depth, conf_code of conf (each optional) */
int sd_live_post(const float* disp, const float* logvar, int H, int W, float* state, int copy, float alpha,
                 float one_minus_alpha, int depth_on, float focal_baseline, float* depth, float* conf,
                 uint8_t* depth_code, float depth_lo, float depth_scale, uint8_t* conf_code, float conf_lo,
                 float conf_scale, sd_stream s);
/* depth_contour_mask (:254-275): edge u8 [H][W] = 255 where the pixel and its right or lower neighbour are both valid
 * (finite, > min_depth, <= max_depth) and floor((clip(depth) - min_depth) / step) differs, else 0. */
int sd_live_contours(const float* depth, int H, int W, float min_depth, float max_depth, float step, uint8_t* edge,
                     sd_stream s);
/* The auto range of colorize_scalar_map (:242-244, np.percentile(values, 2 / 98)), exact, on the device: a radix
 * select over the finite, > 0 values. sel (7 words): [0] the count n as uint32; [1..4] the order statistics at
 * floor((n-1)*0.02), the next index, floor((n-1)*0.98), the next index (clamped to n-1); [5] lo, [6] hi = float32 of the
 * fp64 linear interpolation. n == 0: NaN. code (optional, u8 [H][W]): the codes of `values` in that range, all 0 when
 * n == 0. work: sd_live_select_ws_bytes() bytes, zero before the first call; every call leaves it zero. */
long long sd_live_select_ws_bytes(void);
int sd_live_select(const float* values, int H, int W, unsigned* work, float* sel, uint8_t* code, sd_stream s);
/* The centre read-out (:542-595): out3 = medians of the finite, > 0 values of the centre window (half = max(1,
 * window / 2) around (H/2, W/2), clipped) of disp, depth, conf (NULL map or empty window: NaN; even count: the float32
 * mean of the two middle values). window <= 63. */
int sd_live_center(const float* disp, const float* depth, const float* conf, int H, int W, int window, float* out3,
                   sd_stream s);
/* Display images at the view size (:568-574 contour overlay, :601-617 applyColorMap + cv2.resize INTER_LINEAR): vis_x
 * u8 BGR [Hc][Wc][3] = bilinear resize (half-pixel centres, edge replicate, round half to even) of lut_x[code_x], lut
 * u8 [256][3] BGR, code u8 [H][W]; left_view = view with (0, 255, 0) where the nearest-resized edge mask
 * (sx = min(dx * W / Wc, W - 1)) is set. Each of image a, image b and the left view is optional (NULL). */
int sd_live_compose(const uint8_t* code_a, const uint8_t* lut_a, uint8_t* vis_a, const uint8_t* code_b,
                    const uint8_t* lut_b, uint8_t* vis_b, const uint8_t* edge, const uint8_t* view, uint8_t* left_view,
                    int H, int W, int Hc, int Wc, sd_stream s);

/* ---- the same frame path for n camera pairs per launch (1 <= n <= 64) ----
 * One entry point per stage above. Every buffer is stream-major: [n] of the single-stream layout, stream i's slice at
 * i * (the single-stream element count); the colour tables, the scalars of the colour ranges and the EMA weights are
 * shared. Each entry point issues as many launches as its single-stream form issues for one stream (the stream is a
 * grid dimension), and stream i's outputs are bit-identical to the single-stream entry point run on stream i's slices.
 * The 16-B / 4-B vector paths are taken only when every slice is aligned for them (the per-stream element count a
 * multiple of 4 and the base pointers aligned), so H * W or Hc * Wc * 3 need not be a multiple of anything.
 * Masks are passed by value, bit i for stream i; a bit at or above n is an error.
 *   hold_mask : stream i had no new frame: the entry point reads and writes nothing of stream i (its state, maps,
 *               codes, images, sel row, centre row and select workspace stay as they are)
 *   copy_mask : (post) stream i's EMA state takes the prediction as is (first frame, reset, or alpha 0)
 * The front end and the rectified view take no mask: they run over whatever the frame slots hold.
 * Arguments are checked before any launch; no allocation, no synchronisation, graph-capturable.
 *
 * Front end. left, right: u8 [n][Hc][Wc][3]. Maps: NULL, or map1 int16 [m][Hc][Wc][2] / map2 uint16 [m][Hc][Wc] with
 * map_stride = 0 (m = 1: one set shared by all streams) or Hc * Wc (m = n: one set per stream), the same for both
 * sides. xin: [n][H][W][8] (the engine's batch-n input, = sd_pack_input(dtype, nchw, n, 6, H, W, 8, xin)); nchw:
 * optional f32 [n][6][H][W]. amax: as sd_live_frontend, the maximum taken over all streams, amax[clear] zeroed once. */
int sd_live_frontend_n(int n, int dtype, const uint8_t* left, const uint8_t* right, int Hc, int Wc,
                       const int16_t* map1_l, const uint16_t* map2_l, const int16_t* map1_r, const uint16_t* map2_r,
                       long long map_stride, int H, int W, void* xin, float* nchw, unsigned* amax, int slot, int clear,
                       sd_stream s);
/* Rectified views: frames, views u8 [n][Hc][Wc][3]; maps and map_stride as above (both maps required). */
int sd_live_rectify_n(int n, const uint8_t* frames, int Hc, int Wc, const int16_t* map1, const uint16_t* map2,
                      long long map_stride, uint8_t* views, sd_stream s);
/* Post stage: disp, logvar, state, depth, conf f32 [n][H][W]; depth_code, conf_code u8 [n][H][W]; focal_baseline: a
 * DEVICE array of n float32 (read when depth_on; depth is on for all streams or for none). Optional buffers as in
 * sd_live_post. */
int sd_live_post_n(int n, const float* disp, const float* logvar, int H, int W, float* state,
                   unsigned long long copy_mask, unsigned long long hold_mask, float alpha, float one_minus_alpha,
                   int depth_on, const float* focal_baseline, float* depth, float* conf, uint8_t* depth_code,
                   float depth_lo, float depth_scale, uint8_t* conf_code, float conf_lo, float conf_scale, sd_stream s);
/* Contours: depth f32 [n][H][W] -> edge u8 [n][H][W]. */
int sd_live_contours_n(int n, const float* depth, int H, int W, float min_depth, float max_depth, float step,
                       uint8_t* edge, unsigned long long hold_mask, sd_stream s);
/* Auto range per stream: values f32 [n][H][W], sel f32 [n][8] (row i: the 7 words of sd_live_select for stream i; a
 * stream without a finite positive value gets NaN and all-zero codes), code optional u8 [n][H][W]. work:
 * sd_live_select_n_ws_bytes(n) bytes (n single-stream workspaces; -1 for n outside 1..64), zero before the first call;
 * every call leaves every stream's part zero. Seven launches (six without code), as sd_live_select. */
long long sd_live_select_n_ws_bytes(int n);
int sd_live_select_n(int n, const float* values, int H, int W, unsigned* work, float* sel, uint8_t* code,
                     unsigned long long hold_mask, sd_stream s);
/* Centre medians: disp, depth, conf f32 [n][H][W] (depth, conf optional) -> out3 f32 [n][3]. One launch. */
int sd_live_center_n(int n, const float* disp, const float* depth, const float* conf, int H, int W, int window,
                     float* out3, unsigned long long hold_mask, sd_stream s);
/* Display images: code_x, edge u8 [n][H][W]; vis_x, view, left_view u8 [n][Hc][Wc][3]; lut_x u8 [256][3], shared. */
int sd_live_compose_n(int n, const uint8_t* code_a, const uint8_t* lut_a, uint8_t* vis_a, const uint8_t* code_b,
                      const uint8_t* lut_b, uint8_t* vis_b, const uint8_t* edge, const uint8_t* view, uint8_t* left_view,
                      int H, int W, int Hc, int Wc, unsigned long long hold_mask, sd_stream s);

/* ---- semi-global matcher of the classical live loop (live_camera/depth_live.py:67-83 build_matcher, :158-178) ----
 * The algorithm is stated in INTEGRATION.md ("The semi-global matcher"): OpenCV's StereoSGBM step by step with three
 * paths, integer arithmetic up to the int16 disparity (16 * d, invalid = 16 * (min_disparity - 1)), pinned to the NumPy
 * restatement in tests/sgm_ref.py bit for bit; equality with cv2's bytes is not claimed. Images are uint8 [H][W], B = 1;
 * volumes are uint16 [H][W][D], d fastest, defined for x >= min_disparity + D. Parameters: min_disparity >= 0,
 * D = num_disparities a multiple of 16 in [16, 256], block_size odd in [3, 11], 0 <= P1 <= P2 and
 * 3 * (block_size^2 * (2 * pre_filter_cap + 63) + P2) <= 65535 (every sum fits uint16; the modes with more paths put
 * their path count in place of the 3: sd_sgm_compute_mode), else SD_EINVAL. All buffers
 * are the caller's, nothing allocates or synchronises (graph-capturable). */
/* cvtColor(BGR2GRAY) (:158-159): gray = (1868 B + 9617 G + 4899 R + 8192) >> 14 of a BGR uint8 [H][W][3] view. */
int sd_sgm_gray(const uint8_t* bgr, int H, int W, uint8_t* gray, sd_stream s);
/* The x-Sobel prefilter inside StereoSGBM.compute (:161): clip(2 (a[y][x+1] - a[y][x-1]) + (a[y-1][x+1] - a[y-1][x-1])
 * + (a[y+1][x+1] - a[y+1][x-1]), -cap, cap) + cap, edge replicate. */
int sd_sgm_prefilter(const uint8_t* gray, int H, int W, int cap, uint8_t* out, sd_stream s);
/* Pixel cost (Birchfield-Tomasi of the prefiltered planes + that of the gray planes >> 2) summed over the
 * block_size^2 window (x clamped to [maxD, W - 1], y to [0, H - 1]) -> C. tmp: a second volume of C's size (the row
 * sums of the separable block sum; S serves before the first path writes it). Both 8-B aligned. */
int sd_sgm_cost(const uint8_t* gray_l, const uint8_t* gray_r, const uint8_t* pre_l, const uint8_t* pre_r, int H, int W,
                int min_disparity, int num_disparities, int block_size, uint16_t* C, uint16_t* tmp, sd_stream s);
/* One aggregation path L(p, d) = C + min(L(q, d), L(q, d -+ 1) + P1, min L(q) + P2) - min L(q):
 * pass 0 top -> down, S = L; pass 1 left -> right, S += L. */
int sd_sgm_aggregate(const uint16_t* C, int H, int W, int min_disparity, int num_disparities, int P1, int P2, int pass,
                     uint16_t* S, sd_stream s);
/* The right -> left path on top of S (passes 0 and 1), then per pixel, x descending: the winner (lowest d of the
 * minimum), the uniqueness test, the right-view disparity, the sub-pixel value; then the left-right check
 * (disp12_max_diff < 0: none). q int16 [H][W]; optional S_total (the three-path sum, uint16 volume) and q_raw (the
 * values before the left-right check). W <= 4096. */
int sd_sgm_winner(const uint16_t* C, const uint16_t* S, int H, int W, int min_disparity, int num_disparities, int P1,
                  int P2, int uniqueness_ratio, int disp12_max_diff, uint16_t* S_total, int16_t* q_raw, int16_t* q,
                  sd_stream s);
/* Speckle filter in place: connected components (4-neighbour edges between valid pixels that differ by <=
 * 16 * range) of <= window pixels become invalid_value; window 0: nothing. work: sd_sgm_speckle_ws_bytes(H, W). */
long long sd_sgm_speckle_ws_bytes(int H, int W);
int sd_sgm_speckle(int16_t* q, int H, int W, int invalid_value, int window, int range, void* work, sd_stream s);
/* matcher.compute (:161): prefilter, cost, the three paths, winner, left-right check, speckle filter.
 * work: sd_sgm_ws_bytes(H, W, D) = 2 * a(2 H W D) + 2 * a(H W) + sd_sgm_speckle_ws_bytes, a = round up to 256;
 * 256-B aligned. */
long long sd_sgm_ws_bytes(int H, int W, int D);
int sd_sgm_compute(const uint8_t* gray_l, const uint8_t* gray_r, int H, int W, int min_disparity, int num_disparities,
                   int block_size, int P1, int P2, int disp12_max_diff, int uniqueness_ratio, int speckle_window,
                   int speckle_range, int pre_filter_cap, void* work, int16_t* q, sd_stream s);
/* The aggregation modes (cv2.StereoSGBM's constants) and their paths (dy, dx), the predecessor of (y, x) being
 * (y - dy, x - dx) and a path starting where that lies outside [0, H) x [maxD, W):
 *   SD_SGM_MODE_3WAY (1,0) (0,1) (0,-1); _HH4 adds (-1,0); _SGBM adds (1,1) (1,-1); _HH is all eight.
 * The uint16 bound is npaths * (block_size^2 * (2 * pre_filter_cap + 63) + P2) <= 65535 with 3 / 4 / 5 / 8 paths. */
#define SD_SGM_MODE_SGBM 0
#define SD_SGM_MODE_HH 1
#define SD_SGM_MODE_3WAY 2
#define SD_SGM_MODE_HH4 3
/* One aggregation path along (dy, dx): dy = +-1 with dx in {-1, 0, 1}, or (0, 1). accumulate 0: S = L, 1: S += L.
 * Nothing is written for x < maxD; W <= maxD is a successful no-op. (0, -1) is refused: that path runs inside
 * sd_sgm_winner, on top of the S of all the others. */
int sd_sgm_aggregate_dir(const uint16_t* C, int H, int W, int min_disparity, int num_disparities, int P1, int P2, int dy,
                         int dx, int accumulate, uint16_t* S, sd_stream s);
/* sd_sgm_compute with the paths of `mode`; SD_SGM_MODE_3WAY issues exactly sd_sgm_compute's launches. The further
 * paths are successive launches that add into S, so the workspace is sd_sgm_ws_bytes for every mode. */
int sd_sgm_compute_mode(const uint8_t* gray_l, const uint8_t* gray_r, int H, int W, int min_disparity,
                        int num_disparities, int block_size, int P1, int P2, int disp12_max_diff, int uniqueness_ratio,
                        int speckle_window, int speckle_range, int pre_filter_cap, int mode, void* work, int16_t* q,
                        sd_stream s);
/* The display stage (:161-177): disp = q / 16 as f32, NaN where <= 0; z = row 2 / row 3 of Q (host, 16 doubles, row
 * major) applied to (x, y, nan_to_num(disp), 1) in fp64, cast to f32, NaN where disp is (reprojectImageTo3D's z);
 * code = trunc(float32(nan_to_num(disp) * scale + shift)), scale = 255 / (max - min) (0 when equal), shift = -min *
 * scale in fp64 (cv2.normalize NORM_MINMAX + astype(uint8)); the min / max is found on the device (minmax: 2 words). */
int sd_sgm_post(const int16_t* q, int H, int W, const double* Q, float* disp, float* z, uint8_t* code,
                unsigned* minmax, sd_stream s);
/* np.nanmedian of z's centre window (:168-172; half = max(1, window / 2) around (H/2, W/2), clipped): every non-NaN
 * value counts (sd_live_center keeps only finite, > 0 values); none: NaN. window <= 63. */
int sd_sgm_center(const float* z, int H, int W, int window, float* out, sd_stream s);

/* ---- several stereo rigs (n streams, 1 <= n <= 64) through one matcher step ----
 * The stream is a grid dimension of the kernels above: every entry point below issues the launches its single-stream
 * form issues for one stream, each covering all n streams, and stream i's bytes are identical to the single-stream
 * entry point run on stream i's slices. All streams share one size and one matcher configuration. Buffers are
 * stream-major: gray_l, gray_r u8 [n][H][W]; q int16 [n][H][W]; disp, z f32 [n][H][W]; code u8 [n][H][W] (H * W
 * need not be a multiple of anything). Workspaces are n slices of the single-stream layout. Arguments are checked
 * before any launch (n first); no allocation, no synchronisation, graph-capturable.
 * Gray has no batched entry: a u8 [n][H][W][3] buffer is sd_sgm_gray on n * H rows (sd_sgm_gray(bgr, n * H, W, gray, s)).
 * Rectification and the colour image are sd_live_rectify_n (shared or per-stream maps through map_stride) and
 * sd_live_compose_n (hold_mask 0). */
/* n * sd_sgm_ws_bytes(H, W, D), slice i at i * sd_sgm_ws_bytes (a multiple of 256); negative for n outside 1..64.
 * 640 x 480, D = 128: n * 160 MB. Host only. */
long long sd_sgm_ws_bytes_n(int n, int H, int W, int D);
/* sd_sgm_compute_mode for n streams; work: sd_sgm_ws_bytes_n, 256-B aligned. SD_SGM_MODE_3WAY with n = 1 issues exactly
 * sd_sgm_compute's launches. */
int sd_sgm_compute_n(int n, const uint8_t* gray_l, const uint8_t* gray_r, int H, int W, int min_disparity,
                     int num_disparities, int block_size, int P1, int P2, int disp12_max_diff, int uniqueness_ratio,
                     int speckle_window, int speckle_range, int pre_filter_cap, int mode, void* work, int16_t* q,
                     sd_stream s);
/* sd_sgm_speckle on q [n][H][W]: components never join across a stream boundary (parent links are indices local to
 * the stream). work: n slices of sd_sgm_speckle_ws_bytes(H, W). */
int sd_sgm_speckle_n(int n, int16_t* q, int H, int W, int invalid_value, int window, int range, void* work,
                     sd_stream s);
/* sd_sgm_post per stream. Qdev: a DEVICE array f64 [n][16], one row-major 4 x 4 matrix per stream; minmax: u32 [n][2],
 * each stream's display range is its own. */
int sd_sgm_post_n(int n, const int16_t* q, int H, int W, const double* Qdev, float* disp, float* z, uint8_t* code,
                  unsigned* minmax, sd_stream s);
/* sd_sgm_center per stream: z f32 [n][H][W] -> out f32 [n], one block per stream. */
int sd_sgm_center_n(int n, const float* z, int H, int W, int window, float* out, sd_stream s);

/* ---- the census / Hamming pixel cost of the matcher ("The census cost": steps 2c and 3c) ----
 * In place of the prefilter and the Birchfield-Tomasi cost: a descriptor per pixel of each gray plane that depends only
 * on the order of the intensities inside that image, and the Hamming distance of two descriptors as the pixel cost.
 * Everything from the block sum on is the matcher's as above. Windows (rows x columns): 3x3, 5x5, 7x7, 7x9;
 * nbits = rows * columns - 1 = 8, 24, 48, 62. The uint16 bound is npaths * (block_size^2 * nbits + P2) <= 65535, else
 * SD_EINVAL; pre_filter_cap is checked as before and otherwise unused. Pinned bit for bit to tests/sgm_census_ref.py. */
#define SD_SGM_COST_BT 0
#define SD_SGM_COST_CENSUS 1
/* gray u8 [n][H][W] -> desc u64 [n][H][W] (8-B aligned). Bit k of a descriptor: the k-th position of the win_h x win_w
 * window around the pixel, row-major (dy outer from -win_h/2, dx inner from -win_w/2) with the centre skipped, holds a
 * value strictly below the centre's; positions outside [0, H) x [0, W) of the pixel's own image take the nearest pixel
 * of it (never another stream's). Bits >= nbits are zero. Any other window: SD_EINVAL. */
int sd_sgm_census_n(int n, const uint8_t* gray, int H, int W, int win_h, int win_w, uint64_t* desc, sd_stream s);
/* sd_sgm_cost with the pixel cost popcount(desc_l[y][x] ^ desc_r[y][x - d - min_disparity]) (0..nbits) in place of
 * Birchfield-Tomasi; C, tmp and the block sum as there. nbits: 8, 24, 48 or 62. */
int sd_sgm_cost_census(const uint64_t* desc_l, const uint64_t* desc_r, int H, int W, int min_disparity,
                       int num_disparities, int block_size, int nbits, uint16_t* C, uint16_t* tmp, sd_stream s);
/* The workspace of sd_sgm_compute_cost_n. SD_SGM_COST_BT: sd_sgm_ws_bytes_n. SD_SGM_COST_CENSUS: every stream's slice is
 * sd_sgm_ws_bytes followed by two descriptor planes of a(8 H W) bytes, so the Birchfield-Tomasi layout is a prefix of
 * it (the prefiltered planes stay unwritten). Negative for n outside 1..64 or an unknown cost. Host only. */
long long sd_sgm_ws_bytes_cost_n(int n, int H, int W, int D, int cost);
/* sd_sgm_compute_n with a choice of pixel cost. SD_SGM_COST_BT ignores the window and issues exactly
 * sd_sgm_compute_n's launches on its workspace; SD_SGM_COST_CENSUS runs sd_sgm_census_n on both sides and
 * sd_sgm_cost_census in place of the two prefilter launches and sd_sgm_cost. work: sd_sgm_ws_bytes_cost_n, 256-B
 * aligned. */
int sd_sgm_compute_cost_n(int n, const uint8_t* gray_l, const uint8_t* gray_r, int H, int W, int min_disparity,
                          int num_disparities, int block_size, int P1, int P2, int disp12_max_diff,
                          int uniqueness_ratio, int speckle_window, int speckle_range, int pre_filter_cap, int mode,
                          int cost, int win_h, int win_w, void* work, int16_t* q, sd_stream s);

/* ---- per-epoch preview montages of the training CLI (eval_utils.py:42-73: _normalize_map, save_preview_montage) ----
 * One sample: left | right | gray(target) | gray(pred) along the width, uint8 RGB; each map normalised to the 5th-95th
 * percentile of its own finite values. Two steps: the percentiles (an exact select, on the device), then the bytes.
 * Arguments are checked before any launch; no allocation, no synchronisation, graph-capturable; map / sample i of a
 * batch is byte-identical to a call on it alone. */
/* np.percentile(v, 100 q) (`linear`) of the FINITE values v of each map, exact: a radix select over full 32-bit keys
 * (negative: all bits flipped, else the sign bit set), so zeros, -0.0 and negative values are members and order as
 * numbers (sd_live_select keeps finite values > 0 only, at fixed 2 % / 98 %). values f32 [m][count], 1 <= m <= 64,
 * 0 <= q_lo <= q_hi <= 1. sel f32 [m][8], row i as sd_live_select_n's: [0] the count n of finite values as uint32;
 * [1..4] the order statistics at k = floor((n-1) q_lo), min(k+1, n-1), floor((n-1) q_hi) and its successor; [5] lo,
 * [6] hi = float32(v[k] + (v[k+1] - v[k]) * ((n-1) q - k)) evaluated in fp64. n == 0: NaN in [1..6]. Histogram counts
 * are 32-bit. work: sd_quantile_select_ws_bytes(m) bytes (-1 for m outside 1..64), zero before the first call; every
 * call leaves it zero. Six launches. */
long long sd_quantile_select_ws_bytes(int m);
int sd_quantile_select_n(int m, const float* values, int count, double q_lo, double q_hi, unsigned* work, float* sel,
                         sd_stream s);
/* The montages (:55-73) of n samples (1..64) in one launch: input f32 [n][6][H][W] (planes 0-2 left RGB, 3-5 right RGB),
 * target, pred f32 [n][H][W], sel_t, sel_p f32 [n][8] (rows of sd_quantile_select_n for target and pred; q 0.05 / 0.95
 * for the reference's images) -> montage u8 [n][H][4W][3]; H * W need not be a multiple of anything.
 *   colour  c = trunc(clip(float32(x * 255), 0, 255)), NaN -> 0
 *   map     vmin = lo, scale = float32(max(fp64(hi) - fp64(lo), 1e-6)); gray = trunc(float32(clip((m - vmin) / scale,
 *           0, 1) * 255)) in float32, on all three channels; NaN -> 0, +inf -> 255, -inf -> 0; n == 0: all 0 */
int sd_preview_compose_n(int n, const float* input, const float* target, const float* pred, int H, int W,
                         const float* sel_t, const float* sel_p, uint8_t* montage, sd_stream s);

/* ---- predict and evaluate from files (stereo_depth_estimation_amd/predict.py; no counterpart in the reference) ----
 * Output stage: the heads' f32 maps disp, logvar [B][H][W] at the model resolution -> images at the frames' own size
 * [Hs][Ws] in the dataset's RGB24 disparity encoding, and the rows of the stereo metrics against the native ground truth.
 * One entry point, two launches at most; allocates nothing, does not synchronise, graph-capturable; arguments are
 * checked before any launch. Per output pixel:
 *   d       = sd_resize_bilinear(disp, B, H, W -> Hs, Ws, mul), mul = float32(Ws / float(W)) (F.interpolate bilinear,
 *             align_corners=False, and the reference's width scaling, dataset.py:195-212), bit for bit that entry
 *             point's value (one shared device function); disp_up f32 [B][Hs][Ws] receives d
 *   code(v) = 0 when v is not finite, else c = rint(clip(v * 1000, 0, 16646655)), ties to even as np.round, the product
 *             exact (formed in fp64) and rounded once; bytes R = min(c / 65025, 255), rem = c - 65025 R,
 *             G = min(rem / 255, 255), B = rem - 255 G. For c < 16646400 that is R = c / 65025, G = (c / 255) % 255,
 *             B = c % 255, with G and B below 255; the 256 codes above saturate the digits up to (255, 255, 255). The
 *             inverse of depth_uint8_decoding (dataset.py:23-30): decode(code(x)) == x for every float32 x = c / 1000.
 *             Code 0 is the dataset's "no value" (valid = target > 0).
 *   disp_rgb  u8 [B][Hs][Ws][3] = code(d)
 *   sigma_rgb u8 [B][Hs][Ws][3] = code(expf(0.5f * lv) * mul), lv = the same resize of logvar with mul = 1 (needs logvar)
 *   metrics   f64 [B][8] (needs gt_rgb u8 [B][Hs][Ws][3] and work): gt = (R * 65025 + G * 255 + B) / 1000.f as
 *             sd_stereo_preprocess decodes it; a pixel counts when gt > 0 and d is finite; e = |d - gt| in float32;
 *             row = [n, sum e, sum e^2 (each square exact in fp64), #(e > 1), #(e > 2), #(e > 3),
 *             #(e > 3 && e > 0.05f * gt) (D1), 0]. A sample without a counted pixel gets zeros. The sums have one fixed
 *             order (per-block partial rows in work, added in index order by the second launch; no atomics): two runs on
 *             the same inputs, and the two store paths, give the same 64 bits.
 * Each of disp_rgb, sigma_rgb, disp_up and metrics is optional (NULL), one at least is required. Four pixels per thread
 * with word stores when Ws % 4 == 0, disp_rgb / sigma_rgb are 4-B and disp_up is 16-B aligned; byte and float stores
 * otherwise; the same bytes either way. work: sd_disp_export_ws_bytes(batch, Hs, Ws) bytes, 8-B aligned, needs no
 * clearing (-1 for sizes outside batch 1..65535, Hs * Ws < 2^31 - 3). */
long long sd_disp_export_ws_bytes(int batch, int Hs, int Ws);
int sd_disp_export(const float* disp, const float* logvar, int batch, int H, int W, const uint8_t* gt_rgb, int Hs,
                   int Ws, uint8_t* disp_rgb, uint8_t* sigma_rgb, float* disp_up, double* metrics, void* work,
                   sd_stream s);
/* Uncertainty evaluation (stereo_depth_estimation_amd/uncert.py; no counterpart in the reference): how well the
 * log-variance head ranks and sizes the errors of the disparity head, against the native ground truth, without a sort.
 * The contract is sd_disp_export's: allocates nothing, does not synchronise, graph-capturable (a memset node and two
 * launches), every argument checked before any launch. All arithmetic float32, nothing fused, unless it says otherwise.
 * Per output pixel of sample b at the frame's own size [Hs][Ws]:
 *   d, lv, gt  exactly sd_disp_export's: d = the resize of disp with mul = float32(Ws / float(W)), lv = the resize of
 *              logvar with mul = 1, gt = the decoded RGB24 ground truth
 *   counted    gt > 0 and d finite and lv finite
 *   e  = |d - gt|;  q = min(rint(e * 4096), 2^30) as an integer (the product is exact, ties to even). Every error sum of
 *              the curves is a sum of q: integers, so no summation order exists.
 *   u  = the uncertainty bin: t = (lv + 32.f) * 64.f; 0 if t < 0, 4095 if t >= 4095, else (int)floorf(t): 1/64 steps of
 *              log-variance over [-32, 32), the ends saturate
 *   o  = the oracle bin: clip((bits(e) >> 15) - (119 << 8), 0, 4095): 256 bins per octave over e in [2^-8, 2^8) px
 *   e_m = e / mul (model pixels);  nll_px = e_m * expf(-lv) + lv (train.py:339 of the reference)
 *   covered at z in {0.5, 1, 2, 3}: e_m <= z * expf(lv) (Laplace with b = exp(logvar): nominal share 1 - exp(-z))
 * Per sample, from the histograms cnt_u, sum_u and cnt_o, sum_o [4096] (uint32 counts, uint64 sums of q), n = sum cnt:
 *   for k = 0 .. steps - 1: keep m_k = n - floor(n k / steps) pixels (64-bit integers); j = the bin with
 *   C_{<j} < m_k <= C_{<=j}, cumulating upwards from bin 0;
 *   curve_k = ((double)S_{<j} + (double)(m_k - C_{<j}) * (double)sum_j / (double)cnt_j) / (double)m_k / 4096.0, the
 *   operations in that order in fp64 (S_{<j} = the integer sum of sum_i over i < j): the pixels of the bin the cut falls
 *   into share the cut, each entering with the bin's mean error. unc_k from the u histogram, orc_k from the o histogram.
 *   AUSE = (sum_k ((unc_k - orc_k) / unc_0)) / steps, AURG = (sum_k (1 - unc_k / unc_0)) / steps, each term formed and
 *   added in index order in fp64; both 0 when unc_0 == 0.
 * rows f64 [B][16 + 2 steps]: [0] n, [1] sum q as a double (the integer rounded once), [2] sum nll_px accumulated in fp64
 * (one fixed order: a thread's pixels in index order, block_partial_row, the partial rows in index order), [3..6] the
 * coverage counts at z = 0.5, 1, 2, 3, [7] AUSE, [8] AURG, [9] counted pixels in u bin 0 or 4095, [10] the same for o,
 * [11..15] 0, then unc[steps], then orc[steps]. A sample without a counted pixel gets a row of zeros. Integer atomics
 * only: a sample's row depends neither on launch order nor on the rest of the batch, and two runs give the same 64 bits.
 * steps in 1..256; rows and work 8-B aligned; work: sd_uncert_eval_ws_bytes(batch, Hs, Ws, steps) bytes, needs no clearing
 * by the caller (the entry point clears the histograms itself with a memset node ahead of the first launch); -1 for
 * steps outside 1..256 or sizes outside sd_disp_export's (batch 1..65535, Hs * Ws < 2^31 - 3). */
long long sd_uncert_eval_ws_bytes(int batch, int Hs, int Ws, int steps);
int sd_uncert_eval(const float* disp, const float* logvar, int batch, int H, int W, const uint8_t* gt_rgb, int Hs,
                   int Ws, int steps, double* rows, void* work, sd_stream s);
/* Host only: n images rgb u8 [n][H][W][3] -> PNG files (8-bit RGB, not interlaced, filter type 0 on every row, one zlib
 * stream at `level` 0..9 in one IDAT chunk), by at most min(threads, 16) threads. File handling as
 * sd_write_cache_batch: each file is written under <name>.tmp.<pid>.<serial> beside its target and renamed over it; a
 * failed file is removed and an earlier file at the target keeps its bytes; the other files are still written.
 * Returns 0, or 1 + the lowest failing index with the path and reason in err, or -1 for bad arguments. */
int sd_write_png_batch(const char* const* paths, int n, int H, int W, const uint8_t* rgb, int level, int threads,
                       char* err, int errlen);

/* ---- coloured point clouds (stereo_depth_estimation_amd/cloud.py; cv2.reprojectImageTo3D of depth_live.py:164 with
 * all three coordinates, masked and packed) ----
 * n streams (1..64) of one size H x W, stream-major: disp f32 [n][H][W]; color u8 [n][H][W][3] or NULL, BGR when
 * color_bgr is 1, RGB when 0; Qdev a DEVICE array f64 [n][16], one row-major 4 x 4 matrix per stream, as sd_sgm_post_n
 * takes it; z_min <= z_max as float32, +-inf for no bound, NaN refused; stride 1..64.
 *   value  a pixel whose disp is finite and > 0. d = (double)disp, R_r = ((Q[r][0] x + Q[r][1] y) + Q[r][2] d) + Q[r][3]
 *          in fp64, every operation rounded on its own; X, Y, Z = float32(R_0 / R_3), float32(R_1 / R_3),
 *          float32(R_2 / R_3). Z is bit-equal to sd_sgm_post's z on the same disparity.
 *   kept   a value whose X, Y and Z are finite as float32 and z_min <= Z <= z_max (compared in float32)
 *   xyz    f32 [n][H][W][3] or NULL: the organised cloud, the point of a kept pixel and three NaNs elsewhere; stride
 *          and cap do not apply to it
 *   points [n][cap] records of 16 bytes, 16-B aligned, or NULL: float32 x, y, z; uint8 red, green, blue, alpha = 255
 *          (little-endian; white without color). Stream i holds its kept pixels with x % stride == 0 && y % stride == 0
 *          in ascending (y, x) order (NumPy's boolean-mask order). count u32 [n]: their number, whether or not it
 *          exceeds cap; only the first min(count[i], cap) records are written, and no other byte of points is touched.
 * The same inputs give the same bytes on every run, and stream i's bytes do not depend on n or on its neighbours: the
 * order comes from a prefix sum (count per 1024-pixel tile, scan of the tile counts per stream, scatter), never from
 * atomics, and no block waits for another. Three launches with points, one with xyz alone, whatever n is. One of xyz /
 * points at least; points need count, cap >= 1 and work: sd_cloud_ws_bytes(n, H, W, stride) bytes, 4-B aligned, needs no
 * clearing (-1 for n outside 1..64, non-positive sizes, H * W >= 2^31, stride outside 1..64; host only). Arguments are
 * checked before any launch; no allocation, no synchronisation, graph-capturable. */
long long sd_cloud_ws_bytes(int n, int H, int W, int stride);
int sd_cloud_build_n(int n, const float* disp, const uint8_t* color, int color_bgr, int H, int W, const double* Qdev,
                     float z_min, float z_max, int stride, float* xyz, void* points, long long cap, unsigned* count,
                     void* work, sd_stream s);
/* Host only: n clouds -> binary little-endian PLY files. points: [n][cap] records as sd_cloud_build_n writes them (in
 * host memory), counts u32 [n]. File i is the header
 *   ply / format binary_little_endian 1.0 / element vertex N / property float x / property float y / property float z /
 *   property uchar red / property uchar green / property uchar blue / property uchar alpha / end_header
 * (one line each, '\n' ends), N = min(counts[i], cap), followed by the first N records of slice i verbatim; N = 0 is a
 * valid file. At most min(threads, 16) threads; file handling and return codes as sd_write_png_batch. */
int sd_write_ply_batch(const char* const* paths, int n, const void* points, long long cap, const unsigned* counts,
                       int threads, char* err, int errlen);

/* ---- label-free check of a disparity map: visibility classes and photometric residual
 * (stereo_depth_estimation_amd/check.py; INTEGRATION.md "sd_stereo_check" is the normative text) ----
 * n samples (1..65535) of one size H x W, H * W < 2^31: disp f32 [n][H][W], the left view's disparity in pixels of these
 * frames; left, right u8 [n][H][W][3], rectified frames of that size in any colour order (the same in both), both given
 * or both NULL; occ_tol finite and >= 0; photo_thr +inf for no mismatch class, NaN refused. All in float32, every
 * operation rounded on its own:
 *   value       disp finite and > 0 (sd_cloud_build_n's rule); xr = float32(x) - disp
 *   out of view a value with xr < 0
 *   occluded    a value in view with m(x) + occ_tol <= xr, m(x) = min xr(x') over the values x' > x of the row (those out
 *               of view included), +inf when there is none
 *   residual    frames given, a value in view and not occluded: x0 = floor(xr) (at most W - 1), f = xr - float32(x0),
 *               x1 = min(x0 + 1, W - 1), r_c = a + f (b - a) with a = right[y][x0][c], b = right[y][x1][c],
 *               e = (|L_0 - r_0| + |L_1 - r_1|) + |L_2 - r_2|, L_c = left[y][x][c]; e in [0, 765]
 *   class       0 visible, 1 no value, 2 out of view, 3 occluded, 4 mismatch (would be 0; frames given and e > photo_thr)
 * Outputs, each optional, one at least; resid and vis_rgb need frames:
 *   cls      u8  [n][H][W]
 *   resid    f32 [n][H][W]    e for classes 0 and 4, NaN elsewhere
 *   disp_vis f32 [n][H][W]    disp for class 0, NaN elsewhere: what sd_cloud_build_n takes in place of the raw map
 *   vis_rgb  u8  [n][H][W][3] class 0 gray min(255, (int)(e / 3.0f)), 1 black, 2 (0, 0, 255), 3 (255, 0, 0),
 *                             4 (255, 255, 0)
 *   rows     f64 [n][8]       [0] values, [1] out of view, [2] occluded, [3] class 0 + class 4 (0 without frames, as are
 *                             [4..6]), [4] sum e over those, [5] sum e^2 (each square exact in fp64), [6] class 4, [7] 0
 * One fixed summation order, a function of (n, H, W) alone, no atomics: two runs give the same 64 bits, every subset of
 * outputs the same bytes for the outputs it has, and sample i's bytes do not depend on n or on its neighbours. At most
 * two plain launches whatever n is (the stage; the addition of the partial rows when rows is asked for), the sample a
 * grid dimension; one block owns whole rows and walks each right to left in steps of 1024 pixels, so no block waits for
 * another. Four pixels per thread with word stores when W % 4 == 0 and disp, resid, disp_vis are 16-B and left, cls,
 * vis_rgb 4-B aligned; scalar loads and stores otherwise; the same bytes either way. work:
 * sd_stereo_check_ws_bytes(n, H, W) bytes, 8-B aligned, needs no clearing (-1 for n outside 1..65535, non-positive
 * sizes, H * W >= 2^31; host only). Arguments are checked before any launch; no allocation, no synchronisation,
 * graph-capturable. */
long long sd_stereo_check_ws_bytes(int n, int H, int W);
int sd_stereo_check(int n, const float* disp, const uint8_t* left, const uint8_t* right, int H, int W, float occ_tol,
                    float photo_thr, uint8_t* cls, float* resid, float* disp_vis, uint8_t* vis_rgb, double* rows,
                    void* work, sd_stream s);

/* ---- label-free adaptation loss: photometric reconstruction + edge-aware smoothness and their gradient
 * (stereo_depth_estimation_amd/selfsup.py; INTEGRATION.md "sd_selfsup_loss" is the normative text) ----
 * n samples (1..65535) of one size H x W, H * W < 2^31, no divisibility asked: disp f32 [n][H][W], the heads' output;
 * logvar f32 [n][H][W] or NULL; input f32 [n][6][H][W] planar, the model's input batch (left RGB / 255, then right);
 * cls u8 [n][H][W] and check_rows f64 [n][8] from one sd_stereo_check call on this disp (geometry only is enough), both
 * required. w_photo, w_smooth, gamma finite and >= 0; eps, eps_s finite and > 0. All in float32, every operation
 * rounded on its own (division and square root correctly rounded):
 *   counted     cls == 0; N = max(1, sum_i (check_rows[i][0] - [i][1] - [i][2] - [i][6])), exact in fp64;
 *               *count = that sum as int32 (0 when nothing is counted, saturated at 2^31 - 1)
 *   warp        xr = float32(x) - disp, x0 = clamp(floor(xr), 0, W - 1), f = xr - float32(x0), x1 = min(x0 + 1, W - 1),
 *               a = R_c[y][x0], b = R_c[y][x1], r_c = a + f (b - a)
 *   photometric t_c = L_c - r_c, phi_c = sqrt(t_c t_c + eps eps), e = ((phi_0 + phi_1) + phi_2) / 3,
 *               de/dd = (((t_0 / phi_0)(b_0 - a_0) + (t_1 / phi_1)(b_1 - a_1)) + (t_2 / phi_2)(b_2 - a_2)) / 3;
 *               l = e without logvar, else v = exp(-lv): l = e v + lv, dl/dd = v de/dd, dl/dlv = 1 - e v
 *   smoothness  every pair (p, q), q right of or below p, with both disparities finite: t = d_q - d_p,
 *               g = ((|L_0q - L_0p| + |L_1q - L_1p|) + |L_2q - L_2p|) / 3, w = exp(-(gamma g)),
 *               r = sqrt(t t + eps_s eps_s), term w r, s = (w t) / r;
 *               g_s(x, y) = (sx(x - 1) - sx(x)) + (sy(y - 1) - sy(y)), a missing or omitted pair gives 0
 * Outputs:
 *   gdisp   f32 [n][H][W]  (w_photo / float32(N)) [cls == 0] dl/dd + (w_smooth / float32(n H W)) g_s, every pixel
 *                          written; 0 where disp is not finite
 *   glogvar f32 [n][H][W]  optional, only with logvar: (w_photo / float32(N)) [cls == 0] dl/dlv, 0 elsewhere
 *   rows    f64 [n][8]     [0] counted pixels, [1] sum l, [2] sum e, [3] sum of the smoothness terms, [4] smoothness
 *                          pairs, [5] sum |gdisp|, [6..7] 0
 * One fixed summation order, a function of (n, H, W) alone, no atomics: two runs give the same bits and sample i's bytes
 * do not depend on n or on its neighbours (N excepted, which is the batch's). Three plain launches whatever n is (N, the
 * pass, the addition of the partial rows), the sample a grid dimension. Four pixels per thread with 16-B loads and
 * stores when W % 4 == 0 and disp, logvar, input, gdisp, glogvar are 16-B and cls 4-B aligned; scalar ones otherwise;
 * the same bytes either way. work: sd_selfsup_ws_bytes(n, H, W) bytes, 8-B aligned, needs no clearing (-1 for n outside
 * 1..65535, non-positive sizes, H * W >= 2^31; host only). Arguments are checked before any launch; no allocation, no
 * synchronisation, graph-capturable. */
long long sd_selfsup_ws_bytes(int n, int H, int W);
int sd_selfsup_loss(int n, const float* disp, const float* logvar, const float* input, const uint8_t* cls,
                    const double* check_rows, int H, int W, float w_photo, float w_smooth, float eps, float eps_s,
                    float gamma, float* gdisp, float* glogvar, double* rows, int* count, void* work, sd_stream s);

/* ---- the same loss with an SSIM term in the photometric error (SelfSupLoss(ssim=alpha); INTEGRATION.md
 * "sd_selfsup_loss_ssim" is the normative text) ----
 * sd_selfsup_loss's arguments, checks, alignment rules, count, N and M, with one more float32 parameter after gamma:
 * alpha in [0, 1] (NaN and values outside are refused). The smoothness term, e and de/dd are sd_selfsup_loss's. With
 * win(p) the pixels of p's sample at most one row and one column away, inside the image and with cls == 0 (k of them,
 * every window sum started at 0 and taken in ascending (y, x) order), C1 = 0.01f 0.01f, C2 = 0.03f 0.03f, per channel:
 *   muL = (sum L) / k, mur = (sum r) / k, sL = (sum (L - muL)^2) / k, sr = (sum (r - mur)^2) / k,
 *   sLr = (sum (L - muL)(r - mur)) / k, A1 = 2 (muL mur) + C1, A2 = 2 sLr + C2, B1 = (muL muL + mur mur) + C1,
 *   B2 = (sL + sr) + C2, S_c = (A1 A2) / (B1 B2)
 *   s = (((1 - S_0) + (1 - S_1)) + (1 - S_2)) / 6, e' = (1 - alpha) e + alpha s; l and dl/dlv as before with e' for e
 *   P = 2 ((muL A2) / (B1 B2) - (S mur) / B1), Qv = -(S / B2), T = (2 A1) / (B1 B2),
 *   h_c(p, q) = ((P + (2 Qv)(r(q) - mur(p))) + T (L(q) - muL(p))) / k(p), u(p) = exp(-lv(p)) or 1,
 *   g_ssim(q) = (((dba_0 sum_p u h_0) + dba_1 sum_p u h_1) + dba_2 sum_p u h_2) / 6 over p in win(q), dba_c = b_c - a_c
 *   gdisp = (w_photo / float32(N)) [cls == 0] ((1 - alpha)(u de/dd) + alpha g_ssim) + (w_smooth / float32(M)) g_s
 * rows [n][8]: as sd_selfsup_loss ([1] sum l with e', [2] sum e unchanged in meaning), [6] sum s, [7] 0.
 * Three plain launches whatever n is; the pass is tiled (a block of 256 threads owns 32 x 16 pixels and stages them with
 * a halo of two into LDS: the gradient is a gather, no atomics). One fixed summation order, a function of (n, H, W)
 * alone; the vector and the scalar path give the same bytes. work: sd_selfsup_ssim_ws_bytes(n, H, W) bytes (64 of
 * header, 64 per tile; -1 for sizes out of range; host only), 8-B aligned, needs no clearing. */
long long sd_selfsup_ssim_ws_bytes(int n, int H, int W);
int sd_selfsup_loss_ssim(int n, const float* disp, const float* logvar, const float* input, const uint8_t* cls,
                         const double* check_rows, int H, int W, float w_photo, float w_smooth, float eps, float eps_s,
                         float gamma, float alpha, float* gdisp, float* glogvar, double* rows, int* count, void* work,
                         sd_stream s);

/* ---- proxy-label adaptation: the matcher's labels as a sparse target of the heads, alone or on top of the label-free
 * loss (stereo_depth_estimation_amd/proxy.py; INTEGRATION.md "sd_proxy_gray" and "sd_proxy_loss" are the normative
 * text) ----
 * sd_proxy_gray: the model's input batch back to the gray images of the matcher. n samples (1..65535) of one size,
 * H * W < 2^31: input f32 [n][6][H][W] planar (left RGB / 255, then right), gray_l and gray_r u8 [n][H][W]. Per channel
 * value x: b = (int) rintf(min(max(x 255, 0), 255)) in float32 (ties to even; a NaN gives 0), then the matcher's step 1
 * on the bytes with channel 0 as R: g = (4899 R + 9617 G + 1868 B + 8192) >> 14. An input that is float32(b / 255) gives
 * b back. One launch, the sample a grid dimension; 16-B loads and 4-B stores when W % 4 == 0, input is 16-B and the
 * outputs are 4-B aligned, scalar accesses otherwise, the same bytes either way. */
int sd_proxy_gray(int n, const float* input, int H, int W, uint8_t* gray_l, uint8_t* gray_r, sd_stream s);

/* sd_proxy_loss: n samples (1..65535) of one size, H * W < 2^31: disp f32 [n][H][W], the heads' output; logvar f32
 * [n][H][W] or NULL; proxy_q4 i16 [n][H][W], 16 * disparity as the matcher writes it, required; w_proxy finite and
 * >= 0; accumulate 0 or 1. All in float32, every operation rounded on its own:
 *   labelled    q4 > 0 and disp finite (the matcher's invalid value and a disparity of 0 are no label)
 *   Np          max(1, labelled pixels of the batch), counted exactly; *count = that number as int32 (accumulate = 1:
 *               plus what *count held), saturated at 2^31 - 1
 *   per pixel   t = float32(q4) / 16, a = |disp - t|, sgn = 1, -1 or 0 (disp == t); l = a, dl/dd = sgn without
 *               logvar, else v = exp(-lv): l = a v + lv, dl/dd = sgn v, dl/dlv = 1 - a v
 *   g_d         (w_proxy / float32(Np)) dl/dd, g_lv = (w_proxy / float32(Np)) dl/dlv
 * Outputs:
 *   gdisp   f32 [n][H][W]  accumulate = 0: g_d, 0 where the pixel is not labelled, every pixel written; accumulate = 1:
 *                          gdisp + g_d at a labelled pixel, an unlabelled pixel is not written
 *   glogvar f32 [n][H][W]  optional, only with logvar: the same with g_lv
 *   rows    f64 [n][8]     [0] labelled pixels, [1] sum l, [2] sum a, [3] sum a^2 (each square exact in fp64),
 *                          [4] sum |g_d|, [5] pixels with q4 > 0 and a non-finite disp, [6..7] 0
 * The loss g_d and g_lv are the gradient of is w_proxy * sum_i rows[i][1] / Np. One fixed summation order, a function of
 * (n, H, W) alone, no atomics: two runs give the same bits, and sample i's bytes depend on its neighbours only through
 * Np. Four plain launches whatever n is (the blocks' counts, Np, the pass, the addition of the partial rows), the sample
 * a grid dimension. Four pixels per thread with 16-B and 8-B accesses when W % 4 == 0, disp, logvar, gdisp, glogvar are
 * 16-B and proxy_q4 is 8-B aligned; scalar ones otherwise; the same bytes either way. work: sd_proxy_ws_bytes(n, H, W)
 * bytes (64 of header, 64 per block), 8-B aligned, needs no clearing (-1 for n outside 1..65535, non-positive sizes,
 * H * W >= 2^31; host only). Arguments are checked before any launch; no allocation, no synchronisation,
 * graph-capturable. */
long long sd_proxy_ws_bytes(int n, int H, int W);
int sd_proxy_loss(int n, const float* disp, const float* logvar, const int16_t* proxy_q4, int H, int W, float w_proxy,
                  int accumulate, float* gdisp, float* glogvar, double* rows, int* count, void* work, sd_stream s);

#ifdef __cplusplus
}
#endif
#endif /* STEREO_HIP_H */
