// hm_image.hip - the image metrics of the reference's evaluation (evaluation/eval.py: PSNR over the object mask and
// SSIM per rendered view; contract: include/hashmod.h).  Images are fp32 [B, H, W, C], channels interleaved; every
// difference, product, sum and quotient is fp64 on the fp32 values.  Both means are two-stage reductions in a fixed
// order - per-workgroup partials, then one workgroup per image over its partials in index order - without atomics,
// so two calls give the same bits.
//
//   hm_image_sqerr  sqerr_partial  per kSqPixels pixels of one image: sum of (x - y)^2 over the set pixels' channels,
//                                  and the number of set pixels
//                   sqerr_final    one workgroup per image: the partials in order -> out[b] = {sum, n}
//   hm_image_ssim   ssim_tile      one workgroup per kTH x kTW tile of window positions of one image, all channels:
//                                  stage the patch, horizontal then vertical pass of the five moments through LDS,
//                                  the SSIM formula, the optional map, the tile's sum
//                   ssim_final     one workgroup per image: the tile sums in order / (positions * C)
//
// ssim_tile.  The tile's window positions need the (kTH + win - 1) x (kTW + win - 1) pixel patch of both images.  Its
// rows are contiguous runs of (pixels * C) floats in memory and are loaded as such, consecutive lanes on consecutive
// floats; they are written to LDS one plane per channel, so that the horizontal pass of a channel reads consecutive
// floats (horizontal neighbours are C floats apart in memory: read in place, C = 4 would put the 16 columns of a row on
// 16 of the 64 banks).  Per channel: thread (r, col) forms the five horizontal sums of patch row r at column col
// (every patch row, kTW columns) into hb; after a barrier thread (row, col) forms the five vertical sums of hb - the
// 64 lanes of a wave read 64 consecutive doubles per tap, conflict-free - and evaluates
//     s = ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2)).
// x*x, y*y and x*y go through the same sums, so for y == x the five moments pair up bit for bit and s == 1 exactly.
// A tile on the image's lower or right edge computes only the positions that exist; LDS it did not fill is not read.
//
// LDS of ssim_tile, in bytes: 8 * (5 * PH * kTW + 32 + kThreads) + 4 * 2 * C * PH * PW with PH = kTH + win - 1 and
// PW = kTW + win - 1.  win = 11, C = 3: 35,168 (four workgroups per CU).  The largest case, win = 31 and C = 4
// (PH = PW = 46): 29,440 + 256 + 2,048 + 67,712 = 99,456 of the CU's 163,840, one workgroup per CU.  The launcher
// computes the figure and refuses what exceeds the CU.
#include <math.h>

#include "hm_block_dev.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTH = 16, kTW = 16;            // window positions per tile; kTH * kTW == kThreads (one each, vertical pass)
constexpr int kMaxWin = 31;
constexpr int kSqPer = 4;                    // pixels per thread of sqerr_partial
constexpr int kSqPixels = kThreads * kSqPer; // pixels per workgroup
constexpr int64_t kLdsPerCu = 160 * 1024;
static_assert(kTH * kTW == kThreads, "the vertical pass gives every thread one window position");

__global__ __launch_bounds__(kThreads) void sqerr_partial_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                 const uint8_t *__restrict__ mask, int64_t pixels, int C,
                                                                 int64_t blocks, double *__restrict__ partial) {
    __shared__ double red[2][kThreads];
    const int64_t b = blockIdx.x / blocks, blk = blockIdx.x % blocks;
    double sum = 0.0, cnt = 0.0;
#pragma unroll
    for (int j = 0; j < kSqPer; ++j) {
        const int64_t p = blk * kSqPixels + j * kThreads + threadIdx.x;
        if (p < pixels && (!mask || mask[b * pixels + p] != 0)) {
            const int64_t at = (b * pixels + p) * C;
            for (int c = 0; c < C; ++c) {
                const double d = (double)x[at + c] - (double)y[at + c];
                sum += d * d;
            }
            cnt += 1.0;
        }
    }
    red[0][threadIdx.x] = sum;
    red[1][threadIdx.x] = cnt;
    hm_block_tree_sum(red);
    if (threadIdx.x < 2) partial[(int64_t)blockIdx.x * 2 + threadIdx.x] = red[threadIdx.x][0];
}

// rows [n_img][per][K] of partials -> red[k][0] = image blockIdx.x's sum of column k, the partials taken in index order
// by thread (t, t + kThreads, ...) and the threads by the fixed tree
template <int K>
__device__ __forceinline__ void image_sum(const double *__restrict__ partial, int64_t per, double (&red)[K][kThreads]) {
    const double *p = partial + (int64_t)blockIdx.x * per * K;
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int64_t i = threadIdx.x; i < per; i += kThreads) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += p[i * K + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = s[k];
    hm_block_tree_sum(red);
}

__global__ __launch_bounds__(kThreads) void sqerr_final_kernel(const double *__restrict__ partial, int64_t blocks,
                                                               double *__restrict__ out) {
    __shared__ double red[2][kThreads];
    image_sum(partial, blocks, red);
    if (threadIdx.x < 2) out[(int64_t)blockIdx.x * 2 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(kThreads) void ssim_final_kernel(const double *__restrict__ partial, int64_t tiles,
                                                              double count, double *__restrict__ out) {
    __shared__ double red[1][kThreads];
    image_sum(partial, tiles, red);
    if (threadIdx.x == 0) out[blockIdx.x] = red[0][0] / count;
}

struct SsimLds {
    int ph, pw;                 // patch extents kTH + win - 1, kTW + win - 1
    int64_t hb, wt, red, px, py, bytes;   // byte offsets of the parts
};

__host__ __device__ inline SsimLds ssim_lds(int C, int win) {
    SsimLds l;
    l.ph = kTH + win - 1;
    l.pw = kTW + win - 1;
    l.hb = 0;
    l.wt = l.hb + (int64_t)sizeof(double) * 5 * l.ph * kTW;
    l.red = l.wt + (int64_t)sizeof(double) * (kMaxWin + 1);
    l.px = l.red + (int64_t)sizeof(double) * kThreads;
    l.py = l.px + (int64_t)sizeof(float) * C * l.ph * l.pw;
    l.bytes = l.py + (int64_t)sizeof(float) * C * l.ph * l.pw;
    return l;
}

__global__ __launch_bounds__(kThreads) void ssim_tile_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                             int64_t H, int64_t W, int C, int win,
                                                             const double *__restrict__ weights, double c1, double c2,
                                                             int64_t tiles_x, int64_t tiles_y, double *__restrict__ map,
                                                             double *__restrict__ partial) {
    extern __shared__ __align__(16) unsigned char lds[];
    const SsimLds at = ssim_lds(C, win);
    double *hb = reinterpret_cast<double *>(lds + at.hb);        // [5][ph][kTW]
    double *wt = reinterpret_cast<double *>(lds + at.wt);        // [win]
    double(&red)[1][kThreads] = *reinterpret_cast<double(*)[1][kThreads]>(lds + at.red);
    float *px = reinterpret_cast<float *>(lds + at.px);          // [C][ph][pw]
    float *py = reinterpret_cast<float *>(lds + at.py);
    const int tid = threadIdx.x, ph = at.ph, pw = at.pw;
    const int64_t tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
    const int64_t OH = H - win + 1, OW = W - win + 1, oy0 = ty * kTH, ox0 = tx * kTW;
    const int vh = (int)min((int64_t)kTH, OH - oy0), vw = (int)min((int64_t)kTW, OW - ox0);   // positions that exist
    const int rows = vh + win - 1, run = (vw + win - 1) * C;     // patch rows inside the image, floats of each

    if (tid < win) wt[tid] = weights[tid];
    for (int i = tid; i < rows * run; i += kThreads) {
        const int r = i / run, s = i - r * run, p = s / C, c = s - p * C;
        const int64_t g = ((b * H + oy0 + r) * W + ox0) * C + s;
        px[(c * ph + r) * pw + p] = x[g];
        py[(c * ph + r) * pw + p] = y[g];
    }
    __syncthreads();

    const int row = tid / kTW, col = tid % kTW;
    const bool live = row < vh && col < vw;
    const int plane = ph * kTW;
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
        for (int i = tid; i < rows * kTW; i += kThreads) {
            const int r = i / kTW, q = i % kTW;
            if (q >= vw) continue;
            const float *rx = px + (c * ph + r) * pw + q, *ry = py + (c * ph + r) * pw + q;
            double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
            for (int k = 0; k < win; ++k) {
                const double w = wt[k], a = rx[k], d = ry[k];
                mx += w * a;
                my += w * d;
                exx += w * (a * a);
                eyy += w * (d * d);
                exy += w * (a * d);
            }
            hb[i] = mx;
            hb[plane + i] = my;
            hb[2 * plane + i] = exx;
            hb[3 * plane + i] = eyy;
            hb[4 * plane + i] = exy;
        }
        __syncthreads();
        if (live) {
            const double *h = hb + row * kTW + col;
            double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
            for (int k = 0; k < win; ++k) {
                const double w = wt[k];
                mx += w * h[k * kTW];
                my += w * h[plane + k * kTW];
                exx += w * h[2 * plane + k * kTW];
                eyy += w * h[3 * plane + k * kTW];
                exy += w * h[4 * plane + k * kTW];
            }
            const double mxy = mx * my, mxx = mx * mx, myy = my * my;
            const double sxy = exy - mxy, sx2 = exx - mxx, sy2 = eyy - myy;
            const double s = ((2.0 * mxy + c1) * (2.0 * sxy + c2)) / ((mxx + myy + c1) * (sx2 + sy2 + c2));
            if (map) map[((b * OH + oy0 + row) * OW + ox0 + col) * C + c] = s;
            acc += s;
        }
        __syncthreads();   // hb is rewritten for the next channel
    }
    red[0][tid] = acc;
    hm_block_tree_sum(red);
    if (tid == 0) partial[blockIdx.x] = red[0][0];
}

// extents in [1, 2^31) with B*H*W*C < 2^62
int image_check_shape(const std::string &w, int64_t B, int64_t H, int64_t W, int64_t C) {
    const int64_t lim = (int64_t)1 << 31;
    HM_CHECK_ARG(B >= 1 && B < lim && H >= 1 && H < lim && W >= 1 && W < lim, w + ": B, H and W must be in [1, 2^31)");
    HM_CHECK_ARG(C >= 1 && C <= 4, w + ": C must be in [1, 4]");
    const int64_t big = ((int64_t)1 << 62) - 1;
    HM_CHECK_ARG(H <= big / C / W && B <= big / (H * W * C), w + ": B*H*W*C must be below 2^62");
    return HM_OK;
}

int image_check_win(const std::string &w, int64_t H, int64_t W, int64_t win) {
    HM_CHECK_ARG(win >= 3 && win <= kMaxWin && (win & 1) == 1, w + ": win must be odd and in [3, 31]");
    HM_CHECK_ARG(H >= win && W >= win, w + ": the image is smaller than the window");
    return HM_OK;
}

int64_t sq_blocks(int64_t H, int64_t W) { return (H * W + kSqPixels - 1) / kSqPixels; }
int64_t ssim_tiles_y(int64_t H, int64_t win) { return (H - win + 1 + kTH - 1) / kTH; }
int64_t ssim_tiles_x(int64_t W, int64_t win) { return (W - win + 1 + kTW - 1) / kTW; }

}  // namespace

extern "C" int64_t hm_image_sqerr_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    if (int rc = image_check_shape("hm_image_sqerr_workspace_bytes", B, H, W, 1)) return rc;
    const int64_t blocks = sq_blocks(H, W);
    if (blocks > (((int64_t)1 << 31) - 1) / B)
        return hm_fail(HM_ERR_INVALID, "hm_image_sqerr_workspace_bytes: more than 2^31 workgroups");
    return (int64_t)sizeof(double) * 2 * B * blocks;
}

extern "C" int hm_image_sqerr(const float *x, const float *y, const uint8_t *mask, int64_t B, int64_t H, int64_t W,
                              int64_t C, double *partial_ws, double *out, void *stream) {
    if (int rc = image_check_shape("hm_image_sqerr", B, H, W, C)) return rc;
    HM_CHECK_ARG(x && y && partial_ws && out, "hm_image_sqerr: NULL pointer");
    const int64_t blocks = sq_blocks(H, W);
    HM_CHECK_ARG(blocks <= (((int64_t)1 << 31) - 1) / B, "hm_image_sqerr: more than 2^31 workgroups");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(sqerr_partial_kernel, dim3((unsigned)(B * blocks)), dim3(kThreads), 0, st, x, y, mask, H * W,
                       (int)C, blocks, partial_ws);
    hipLaunchKernelGGL(sqerr_final_kernel, dim3((unsigned)B), dim3(kThreads), 0, st,
                       static_cast<const double *>(partial_ws), blocks, out);
    HM_CHECK_LAUNCH("hm_image_sqerr");
    return HM_OK;
}

extern "C" int64_t hm_image_ssim_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t win) {
    if (int rc = image_check_shape("hm_image_ssim_workspace_bytes", B, H, W, 1)) return rc;
    if (int rc = image_check_win("hm_image_ssim_workspace_bytes", H, W, win)) return rc;
    const int64_t tiles = ssim_tiles_y(H, win) * ssim_tiles_x(W, win);
    if (tiles > (((int64_t)1 << 31) - 1) / B)
        return hm_fail(HM_ERR_INVALID, "hm_image_ssim_workspace_bytes: more than 2^31 workgroups");
    return (int64_t)sizeof(double) * B * tiles;
}

extern "C" int hm_image_ssim(const float *x, const float *y, int64_t B, int64_t H, int64_t W, int64_t C, int64_t win,
                             const double *weights, double c1, double c2, double *map, double *partial_ws, double *out,
                             void *stream) {
    if (int rc = image_check_shape("hm_image_ssim", B, H, W, C)) return rc;
    if (int rc = image_check_win("hm_image_ssim", H, W, win)) return rc;
    HM_CHECK_ARG(std::isfinite(c1) && std::isfinite(c2) && c1 > 0.0 && c2 > 0.0,
                 "hm_image_ssim: c1 and c2 must be finite and positive");
    HM_CHECK_ARG(x && y && weights && partial_ws && out, "hm_image_ssim: NULL pointer");
    const int64_t tiles_y = ssim_tiles_y(H, win), tiles_x = ssim_tiles_x(W, win), tiles = tiles_x * tiles_y;
    HM_CHECK_ARG(tiles <= (((int64_t)1 << 31) - 1) / B, "hm_image_ssim: more than 2^31 workgroups");
    const SsimLds at = ssim_lds((int)C, (int)win);
    HM_CHECK_ARG(at.bytes <= kLdsPerCu, "hm_image_ssim: a tile of this window and channel count needs " +
                                            std::to_string(at.bytes) + " bytes of LDS, the CU has " +
                                            std::to_string(kLdsPerCu));
    if (int rc = hm_allow_dynamic_lds<ssim_tile_kernel>((int)kLdsPerCu)) return rc;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(B * tiles)), dim3(kThreads), (size_t)at.bytes, st, x, y, H, W,
                       (int)C, (int)win, weights, c1, c2, tiles_x, tiles_y, map, partial_ws);
    hipLaunchKernelGGL(ssim_final_kernel, dim3((unsigned)B), dim3(kThreads), 0, st,
                       static_cast<const double *>(partial_ws), tiles,
                       (double)(H - win + 1) * (double)(W - win + 1) * (double)C, out);
    HM_CHECK_LAUNCH("hm_image_ssim");
    return HM_OK;
}
