// evaluate.hip -- libmmlf_eval_hip.so (gfx950): the multimodal evaluation of include/mmlf_eval_hip.h.
// Three per-pixel kernels, one thread per pixel, lanes along x.  Nothing here is shared with libmmlf_hip.so: this file
// includes none of its headers, so the training library's source hash does not see it.
// Built with -ffp-contract=off: every float64 expression below is the sequence of IEEE operations that is written, and
// mmlf_amd/multimodal.py restates the same sequence on CPU tensors.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mmlf_eval_hip.h"

static thread_local char g_eval_err[512];

static int eval_fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_eval_err, sizeof(g_eval_err), fmt, ap);
    va_end(ap);
    return 1;
}

#define EVAL_CHECK_ARG(cond, ...)                   \
    do {                                            \
        if (!(cond)) return eval_fail(__VA_ARGS__); \
    } while (0)

static int eval_launch_status(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return eval_fail("%s: launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

// pixels of every image of the batch must be countable in an int64 and blocks in an int
static bool eval_shape_ok(int B, int H, int W, long long planes)
{
    if (B <= 0 || H <= 0 || W <= 0 || planes <= 0) return false;
    const long long hw = (long long)H * W;
    return hw <= (1ll << 40) / B / planes;      // (B * planes * H * W <= 2^40 elements)
}

extern "C" const char *mmlf_eval_last_error(void) { return g_eval_err; }
extern "C" int mmlf_eval_abi_version(void) { return MMLF_EVAL_ABI_VERSION; }

// ---------------------------------------------------------------- (a) ground-truth modes

constexpr int GT_THREADS = 128;
constexpr int GT_MAXN = 49;      // offsets with dy^2 + dx^2 <= MMLF_EVAL_MAX_RADIUS^2

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// r2max = floor(radius^2): dy^2 + dx^2 is an integer, so `<= radius^2` and `<= r2max` are one test
__global__ __launch_bounds__(GT_THREADS) void gt_modes_kernel(const float *__restrict__ gt, double *__restrict__ modes,
                                                               int32_t *__restrict__ edges, long long npix, int H, int W,
                                                               int rint_, int r2max, double threshold)
{
    // the neighbourhood of one pixel is a column of this tile (a per-thread array indexed by the sort would live in scratch):
    // element k of thread t at [k * GT_THREADS + t], conflict-free; a thread touches its own column only, so no barrier
    __shared__ float tile[GT_MAXN * GT_THREADS];
    const long long p = (long long)blockIdx.x * GT_THREADS + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p % W);
    const long long row = p / W;
    const int y = (int)(row % H);
    const float *img = gt + (row / H) * ((long long)H * W);

    // Sobel on the 3 x 3 clamped neighbourhood (`reflect` of reach 1 is the clamp), float32
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[r][c] = img[(long long)clampi(y + r - 1, H - 1) * W + clampi(x + c - 1, W - 1)];
    const float dy0 = g[2][0] - g[0][0], dy1 = g[2][1] - g[0][1], dy2 = g[2][2] - g[0][2];
    const float dx0 = g[0][2] - g[0][0], dx1 = g[1][2] - g[1][0], dx2 = g[2][2] - g[2][0];
    const float sy = (dy0 + dy2) + 2.0f * dy1;
    const float sx = (dx0 + dx2) + 2.0f * dx1;
    const float der = __fsqrt_rn(sy * sy + sx * sx);
    const bool edge = (double)der > threshold;
    edges[p] = edge ? 1 : 0;
    const double own = (double)g[1][1];
    if (!edge) {
        modes[2 * p] = own;
        modes[2 * p + 1] = own;
        return;
    }
    float *col = tile + threadIdx.x;
    int n = 0;
    for (int dy = -rint_; dy <= rint_; ++dy)
        for (int dx = -rint_; dx <= rint_; ++dx) {
            if (dy * dy + dx * dx > r2max) continue;
            const float v = img[(long long)clampi(y + dy, H - 1) * W + clampi(x + dx, W - 1)];
            int i = n;                                   // insertion sort, ascending
            while (i > 0 && col[(i - 1) * GT_THREADS] > v) {
                col[i * GT_THREADS] = col[(i - 1) * GT_THREADS];
                --i;
            }
            col[i * GT_THREADS] = v;
            ++n;
        }
    if (col[0] == col[(n - 1) * GT_THREADS]) {           // all equal (n == 1 included)
        modes[2 * p] = (double)col[0];
        modes[2 * p + 1] = (double)col[0];
        return;
    }
    double s = 0.0, q = 0.0;
    for (int i = 0; i < n; ++i) {
        const double v = (double)col[i * GT_THREADS];
        s += v;
        q += v * v;
    }
    double slo = 0.0, qlo = 0.0, best = 0.0, m0 = 0.0, m1 = 0.0;
    for (int k = 1; k < n; ++k) {
        const double v = (double)col[(k - 1) * GT_THREADS];
        slo += v;
        qlo += v * v;
        const double shi = s - slo, qhi = q - qlo;
        const double cost = (qlo - slo * slo / (double)k) + (qhi - shi * shi / (double)(n - k));
        if (k == 1 || cost < best) {
            best = cost;
            m0 = slo / (double)k;
            m1 = shi / (double)(n - k);
        }
    }
    modes[2 * p] = m0 <= m1 ? m0 : m1;
    modes[2 * p + 1] = m0 <= m1 ? m1 : m0;
}

extern "C" int mmlf_eval_gt_modes(const float *gt, double *modes, int32_t *edges, int B, int H, int W, double radius,
                                  double edge_threshold, void *stream)
{
    EVAL_CHECK_ARG(gt && modes && edges, "mmlf_eval_gt_modes: null pointer");
    EVAL_CHECK_ARG(eval_shape_ok(B, H, W, 2), "mmlf_eval_gt_modes: bad shape B=%d H=%d W=%d", B, H, W);
    EVAL_CHECK_ARG(radius > 0.0 && radius <= (double)MMLF_EVAL_MAX_RADIUS,
                   "mmlf_eval_gt_modes: radius %g is outside (0, %d]", radius, MMLF_EVAL_MAX_RADIUS);
    EVAL_CHECK_ARG(edge_threshold == edge_threshold, "mmlf_eval_gt_modes: edge_threshold is NaN");
    const long long npix = (long long)B * H * W;
    const long long blocks = (npix + GT_THREADS - 1) / GT_THREADS;
    EVAL_CHECK_ARG(blocks <= 0x7fffffffll, "mmlf_eval_gt_modes: %lld pixels are too many for one launch", npix);
    gt_modes_kernel<<<dim3((unsigned)blocks), dim3(GT_THREADS), 0, (hipStream_t)stream>>>(
        gt, modes, edges, npix, H, W, (int)ceil(radius), (int)floor(radius * radius), edge_threshold);
    return eval_launch_status("mmlf_eval_gt_modes");
}

// ---------------------------------------------------------------- (b) modes of a posterior

constexpr int PM_THREADS = 256;
constexpr int PM_RADIUS = 8;                 // int(4 sigma + 0.5) of sigma = 2
constexpr int PM_TAPS = 2 * PM_RADIUS + 1;
struct Taps { double w[PM_RADIUS + 1]; };    // w[|k|]: the filter is symmetric, exp() of one argument on both sides

// scipy's `reflect`: d c b a | a b c d | d c b a, period 2S (S below the radius reflects more than once)
__device__ __forceinline__ int reflect(int i, int S)
{
    const int period = 2 * S;
    int m = i % period;
    if (m < 0) m += period;
    return m < S ? m : period - 1 - m;
}

__global__ __launch_bounds__(PM_THREADS) void posterior_modes_kernel(
    const float *__restrict__ post, int32_t *__restrict__ n_modes, double *__restrict__ mode_disp,
    int32_t *__restrict__ mode_cnt, float *__restrict__ mode_prop, long long npix, long long HW, int S, double disp_min,
    double disp_max, double outlier, Taps taps)
{
    const long long p = (long long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (p >= npix) return;
    const long long b = p / HW;
    const float *col = post + b * S * HW + (p - b * HW);      // bin r of this pixel at col[r * HW]

    // the 17 bins around bin i, boundary applied: moved by one bin per step with unrolled copies, so it stays in registers
    float win[PM_TAPS];
#pragma unroll
    for (int t = 0; t < PM_TAPS; ++t) win[t] = col[reflect(t - PM_RADIUS, S) * HW];

    // raw modes: the two strongest strict interior maxima, the lower bin on equal heights; the arg-max bin for none
    int cnt = 0, b1 = 0, b2 = 0, abin = 0;
    float h1 = 0.f, h2 = 0.f, amax = 0.f;
    // smoothed: the top two maxima in (height, bin) order, and the smallest minimum between them
    int nmax = 0, has2 = 0, since_has = 0, between_has = 0;
    float t1 = 0.f, t2 = 0.f, since = 0.f, between = 0.f, s1 = 0.f, s2 = 0.f;

    for (int i = 0; i < S; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < PM_TAPS; ++t) acc += taps.w[t < PM_RADIUS ? PM_RADIUS - t : t - PM_RADIUS] * (double)win[t];
        const float s = (float)acc;

        const float c = win[PM_RADIUS];
        if (i == 0 || c > amax) {
            amax = c;
            abin = i;
        }
        if (i >= 1 && i <= S - 2 && c > win[PM_RADIUS - 1] && c > win[PM_RADIUS + 1]) {
            ++cnt;
            if (cnt == 1 || c > h1) {
                h2 = h1; b2 = b1;
                h1 = c; b1 = i;
            } else if (cnt == 2 || c > h2) {
                h2 = c; b2 = i;
            }
        }
        if (i >= 2) {                                        // bin i - 1 of the smoothed values has both neighbours now
            if (s2 < s1 && s < s1) {
                ++nmax;
                if (nmax == 1 || s1 >= t1) {                 // the new maximum leads; the old leader is second
                    has2 = nmax > 1;
                    t2 = t1;
                    t1 = s1;
                    between = since; between_has = since_has;
                    since_has = 0;
                } else if (!has2 || s1 >= t2) {              // second behind the leader: the minima since the leader lie between
                    has2 = 1;
                    t2 = s1;
                    between = since; between_has = since_has;
                }
            } else if (s2 > s1 && s > s1) {
                if (!since_has || s1 < since) since = s1;
                since_has = 1;
            }
        }
        s2 = s1;
        s1 = s;
#pragma unroll
        for (int t = 0; t < PM_TAPS - 1; ++t) win[t] = win[t + 1];
        win[PM_TAPS - 1] = i + 1 < S ? col[reflect(i + 1 + PM_RADIUS, S) * HW] : 0.f;
    }

    if (n_modes) n_modes[p] = cnt < 2 ? cnt : 2;
    if (mode_disp) {
        int lo, hi;
        if (cnt == 0) lo = hi = abin;
        else if (cnt == 1) lo = hi = b1;
        else { lo = b1 < b2 ? b1 : b2; hi = b1 < b2 ? b2 : b1; }
        const double den = (double)(S > 1 ? S - 1 : 1), range = disp_max - disp_min;
        mode_disp[2 * p] = (double)lo / den * range + disp_min;
        mode_disp[2 * p + 1] = (double)hi / den * range + disp_min;
    }
    const bool two = has2 && (double)t2 > outlier * (double)t1;
    if (mode_cnt) mode_cnt[p] = two ? 1 : 0;
    if (mode_prop) mode_prop[p] = two && between_has ? (float)((double)t2 / (double)between) : 0.f;
}

extern "C" int mmlf_eval_posterior_modes(const float *posterior, int32_t *n_modes, double *mode_disp, int32_t *mode_cnt,
                                         float *mode_prop, int B, int S, int H, int W, double disp_min, double disp_max,
                                         double sigma, double outlier, void *stream)
{
    EVAL_CHECK_ARG(posterior, "mmlf_eval_posterior_modes: null posterior");
    EVAL_CHECK_ARG(S >= 1 && S <= (1 << 20) && eval_shape_ok(B, H, W, S),
                   "mmlf_eval_posterior_modes: bad shape B=%d S=%d H=%d W=%d", B, S, H, W);
    EVAL_CHECK_ARG(sigma > 0.0 && (int)(4.0 * sigma + 0.5) == PM_RADIUS,
                   "mmlf_eval_posterior_modes: sigma %g gives a filter radius other than %d", sigma, PM_RADIUS);
    EVAL_CHECK_ARG(outlier == outlier && disp_min == disp_min && disp_max == disp_max,
                   "mmlf_eval_posterior_modes: NaN argument");
    Taps taps;
    double sum = 0.0;
    double w[PM_TAPS];
    for (int k = -PM_RADIUS; k <= PM_RADIUS; ++k) {
        w[k + PM_RADIUS] = exp(-0.5 / (sigma * sigma) * (double)(k * k));
        sum += w[k + PM_RADIUS];
    }
    for (int k = 0; k <= PM_RADIUS; ++k) taps.w[k] = w[k + PM_RADIUS] / sum;
    const long long HW = (long long)H * W, npix = (long long)B * HW;
    const long long blocks = (npix + PM_THREADS - 1) / PM_THREADS;
    EVAL_CHECK_ARG(blocks <= 0x7fffffffll, "mmlf_eval_posterior_modes: %lld pixels are too many for one launch", npix);
    posterior_modes_kernel<<<dim3((unsigned)blocks), dim3(PM_THREADS), 0, (hipStream_t)stream>>>(
        posterior, n_modes, mode_disp, mode_cnt, mode_prop, npix, HW, S, disp_min, disp_max, outlier, taps);
    return eval_launch_status("mmlf_eval_posterior_modes");
}

// ---------------------------------------------------------------- (c) two-mode error sums

constexpr int TM_THREADS = 256;
constexpr int TM_FIELDS = 6;
constexpr int TM_MAX_BLOCKS = MMLF_EVAL_PARTIALS / TM_FIELDS;

// the six sums of one workgroup, in a fixed order: a tree over LDS, thread 0 holds the result
__device__ __forceinline__ void block_sums(double (&v)[TM_FIELDS], double *__restrict__ dst)
{
    __shared__ double sh[TM_FIELDS][TM_THREADS];
#pragma unroll
    for (int f = 0; f < TM_FIELDS; ++f) sh[f][threadIdx.x] = v[f];
    __syncthreads();
    for (int o = TM_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int f = 0; f < TM_FIELDS; ++f) sh[f][threadIdx.x] += sh[f][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int f = 0; f < TM_FIELDS; ++f) dst[f] = sh[f][0];
    }
}

__global__ __launch_bounds__(TM_THREADS) void two_mode_partial_kernel(
    const double *__restrict__ mode_disp, const int32_t *__restrict__ n_modes, const double *__restrict__ gt_modes,
    const float *__restrict__ gt, const float *__restrict__ pred, long long npix, int H, int W, int margin, int lb,
    double *__restrict__ partials)
{
    double v[TM_FIELDS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const long long stride = (long long)gridDim.x * TM_THREADS;
    for (long long p = (long long)blockIdx.x * TM_THREADS + threadIdx.x; p < npix; p += stride) {
        const int x = (int)(p % W), y = (int)((p / W) % H);
        if (x < margin || x >= W - margin || y < margin || y >= H - margin) continue;
        const double m0 = gt_modes[2 * p], m1 = gt_modes[2 * p + 1];
        if (m0 == m1) continue;
        const double d0 = mode_disp[2 * p], d1 = mode_disp[2 * p + 1], g = (double)gt[p];
        double mse, bad;
        if (lb) {
            const double e0 = g - d0, e1 = g - d1;
            mse = fmin(e0 * e0, e1 * e1);
            bad = fmin(fabs(e0) > 0.07 ? 1.0 : 0.0, fabs(e1) > 0.07 ? 1.0 : 0.0);
        } else {
            const double e0 = d0 - m0, e1 = d1 - m1;
            mse = (e0 * e0 + e1 * e1) * 0.5;
            bad = ((fabs(e0) > 0.07 ? 1.0 : 0.0) + (fabs(e1) > 0.07 ? 1.0 : 0.0)) * 0.5;
        }
        const double eu = g - (double)pred[p];
        v[0] += 1.0;
        v[1] += mse;
        v[2] += bad;
        v[3] += eu * eu;
        v[4] += fabs(eu) > 0.07 ? 1.0 : 0.0;
        v[5] += n_modes[p] < 2 ? 1.0 : 0.0;
    }
    block_sums(v, partials + (long long)blockIdx.x * TM_FIELDS);
}

__global__ __launch_bounds__(TM_THREADS) void two_mode_final_kernel(const double *__restrict__ partials, int nblocks,
                                                                     double *__restrict__ out)
{
    double v[TM_FIELDS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int blk = threadIdx.x; blk < nblocks; blk += TM_THREADS) {
#pragma unroll
        for (int f = 0; f < TM_FIELDS; ++f) v[f] += partials[(long long)blk * TM_FIELDS + f];
    }
    block_sums(v, out);
}

extern "C" int mmlf_eval_two_mode_error(const double *mode_disp, const int32_t *n_modes, const double *gt_modes,
                                        const float *gt, const float *pred, int B, int H, int W, int margin, int lb,
                                        double *partials, double *out, void *stream)
{
    EVAL_CHECK_ARG(mode_disp && n_modes && gt_modes && gt && pred && partials && out,
                   "mmlf_eval_two_mode_error: null pointer");
    EVAL_CHECK_ARG(eval_shape_ok(B, H, W, 2), "mmlf_eval_two_mode_error: bad shape B=%d H=%d W=%d", B, H, W);
    EVAL_CHECK_ARG(margin >= 0, "mmlf_eval_two_mode_error: margin %d is negative", margin);
    EVAL_CHECK_ARG(lb == 0 || lb == 1, "mmlf_eval_two_mode_error: lb is %d, not 0 or 1", lb);
    const long long npix = (long long)B * H * W;
    long long blocks = (npix + TM_THREADS - 1) / TM_THREADS;
    if (blocks > TM_MAX_BLOCKS) blocks = TM_MAX_BLOCKS;
    two_mode_partial_kernel<<<dim3((unsigned)blocks), dim3(TM_THREADS), 0, (hipStream_t)stream>>>(
        mode_disp, n_modes, gt_modes, gt, pred, npix, H, W, margin, lb, partials);
    if (eval_launch_status("mmlf_eval_two_mode_error")) return 1;
    two_mode_final_kernel<<<dim3(1), dim3(TM_THREADS), 0, (hipStream_t)stream>>>(partials, (int)blocks, out);
    return eval_launch_status("mmlf_eval_two_mode_error (second stage)");
}
