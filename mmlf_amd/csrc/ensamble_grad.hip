// ensamble_grad.hip -- libmmlf_ese_hip.so (gfx950): the backward pass of the Ensamble, include/mmlf_ese_hip.h.
// Two kernels: the adjoint of the fusion (mmlf_ensamble_reduce) and the adjoint of the shear into the trunk's grid layout
// (mmlf_shift_pack), summed over the members.  Nothing here is shared with libmmlf_hip.so or libmmlf_eval_hip.so: this file
// includes none of their headers, so neither library's source hash sees it.
// Built with -ffp-contract=off: every float32 expression below is the sequence of IEEE operations that is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mmlf_ese_hip.h"

static thread_local char g_ese_err[512];

static int ese_fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_ese_err, sizeof(g_ese_err), fmt, ap);
    va_end(ap);
    return 1;
}

#define ESE_CHECK_ARG(cond, ...)                   \
    do {                                           \
        if (!(cond)) return ese_fail(__VA_ARGS__); \
    } while (0)

static int ese_launch_status(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ese_fail("%s: launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

// every element of `planes` images of the batch must be countable well inside an int64
static bool ese_shape_ok(int B, int H, int W, long long planes)
{
    if (B <= 0 || H <= 0 || W <= 0 || planes <= 0) return false;
    const long long hw = (long long)H * W;
    return hw <= (1ll << 40) / B / planes;      // (B * planes * H * W <= 2^40 elements)
}

extern "C" const char *mmlf_ese_last_error(void) { return g_ese_err; }
extern "C" int mmlf_ese_abi_version(void) { return MMLF_ESE_ABI_VERSION; }

// ---------------------------------------------------------------- (a) backward of the fusion

constexpr int RB_THREADS = 64;

// One thread per (pixel, member j), lanes along the pixels: S x S exponentials per pixel (1.3e9 for a 70-member 512 x 512
// scene) are the work, so the members are spread over the grid -- a thread per pixel alone is 4 waves per SIMD at that size
// and a fraction of one for a chunk of a scene.  Every load is one plane read with consecutive addresses across the wave.
// The member is the FAST block coordinate: the S workgroups of one piece of 64 pixels are dispatched together, so the S
// planes of g_posterior and (for the arg-min) of logvars that all of them read are fetched once and served from L2 to the
// rest, not S times from memory.  A thread sums its S terms over k ascending, whatever the geometry.
__global__ __launch_bounds__(RB_THREADS) void reduce_bwd_kernel(
    const float *__restrict__ means, const float *__restrict__ logvars, const float *__restrict__ grid,
    const float *__restrict__ g_mean, const float *__restrict__ g_logvar, const float *__restrict__ g_post,
    float *__restrict__ g_means, float *__restrict__ g_logvars, int S, long long HW, long long total /* B*HW */,
    long long pix_blocks)
{
    const long long blk = blockIdx.x;
    const long long pb = blk / S;
    const int j = (int)(blk - pb * S);
    const long long idx = pb * RB_THREADS + threadIdx.x;
    if (idx >= total) return;
    const long long b = idx / HW;
    const long long p = idx - b * HW;
    const float m = means[(size_t)j * total + idx];
    const float lv = logvars[(size_t)j * total + idx];
    float gm = 0.f, glv = 0.f;
    if (g_post) {
        const float bj = expf(lv);
        const float half_inv = __fdiv_rn(1.0f, __fmul_rn(2.0f, bj));       // the forward's 1 / (2 b)
        const float *gp = g_post + (size_t)b * S * HW + p;
        for (int k = 0; k < S; ++k) {
            const float d = __fsub_rn(grid[k], m);
            const float a = __fdiv_rn(fabsf(d), bj);
            const float gl = __fmul_rn(gp[(size_t)k * HW], __fmul_rn(half_inv, expf(-a)));      // g_posterior_k L_kj
            const float sgn = d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.0f);
            gm = __fadd_rn(gm, __fdiv_rn(__fmul_rn(gl, sgn), bj));
            glv = __fadd_rn(glv, __fmul_rn(gl, __fsub_rn(a, 1.0f)));
        }
        gm = __fdiv_rn(gm, (float)S);
        glv = __fdiv_rn(glv, (float)S);
    }
    if (g_mean || g_logvar) {
        // the forward's arg-min, comparison for comparison (ensamble_reduce_kernel)
        float best = INFINITY;
        int bi = 0;
        for (int i = 0; i < S; ++i) {
            const float v = logvars[(size_t)i * total + idx];
            if (v < best) { best = v; bi = i; }
        }
        if (bi == j) {
            if (g_mean) gm = __fadd_rn(gm, g_mean[idx]);
            if (g_logvar) glv = __fadd_rn(glv, g_logvar[idx]);
        }
    }
    g_means[(size_t)j * total + idx] = gm;
    g_logvars[(size_t)j * total + idx] = glv;
}

extern "C" int mmlf_ese_reduce_bwd(const float *means, const float *logvars, const float *grid, const float *g_mean,
                                   const float *g_logvar, const float *g_posterior, float *g_means, float *g_logvars, int S,
                                   int B, int H, int W, void *stream)
{
    ESE_CHECK_ARG(means && logvars && grid && g_means && g_logvars, "mmlf_ese_reduce_bwd: null pointer");
    ESE_CHECK_ARG(S >= 1 && S <= (1 << 20), "mmlf_ese_reduce_bwd: S=%d members (1 .. 2^20)", S);
    ESE_CHECK_ARG(ese_shape_ok(B, H, W, S), "mmlf_ese_reduce_bwd: bad shape B=%d S=%d H=%d W=%d", B, S, H, W);
    const long long HW = (long long)H * W, total = (long long)B * HW;
    const long long pix_blocks = (total + RB_THREADS - 1) / RB_THREADS;
    ESE_CHECK_ARG(pix_blocks <= 0x7fffffffll / S, "mmlf_ese_reduce_bwd: shape B=%d S=%d H=%d W=%d is too large for one launch",
                  B, S, H, W);
    reduce_bwd_kernel<<<dim3((unsigned)(pix_blocks * S)), dim3(RB_THREADS), 0, (hipStream_t)stream>>>(
        means, logvars, grid, g_mean, g_logvar, g_posterior, g_means, g_logvars, S, HW, total, pix_blocks);
    return ese_launch_status("mmlf_ese_reduce_bwd");
}

// ---------------------------------------------------------------- (b) adjoint of the shear, summed over the members

constexpr int US_THREADS = 256;
constexpr int US_XT = 64;                    // output positions of one workgroup
constexpr int US_PITCH = US_XT | 1;          // odd pitch of the transpose tile: conflict-free both ways
constexpr int GRID_PAD = 2;                  // the trunk's grid: pitch W + 2, H + 2 rows, extent (H, W) at (1, 1)

struct UnshiftTab { int s0, s1; float w0, w1; };

// Source index of the ADJOINT of a roll by +s with Python-slice clamping: the forward reads src[roll_src(x, s, n)] =
// src[(x - s) mod n] into x, so position x of the source collects the gradient at (x + s) mod n; |s| >= n is the identity in
// both.  No integer division: |s| < n, so x + s lies in (-n, 2n).
__device__ __forceinline__ int unroll_src(int x, int s, int n)
{
    if (s >= n || -s >= n) return x;
    int a = x + s;
    a += a < 0 ? n : 0;
    a -= a >= n ? n : 0;
    return a;
}

// One workgroup per (output row y, piece of US_XT positions).  The gradient arrives position-major (channels of a position
// side by side), the stack's gradient leaves plane-major: the gather runs with the VIEWS across the lanes -- a lane reads
// the three colours of its view, 12 consecutive bytes, neighbouring lanes neighbouring views of the same or the next
// position -- and keeps its three sums in registers over the member loop; the sums cross to x-across-the-lanes through an
// LDS tile, as pack_nchw_kernel's transpose does, and are added to `out` in whole row pieces.  The members' shift table
// sits in LDS ahead of the loop (n views entries).
template <int KIND>
__global__ __launch_bounds__(US_THREADS) void unshift_sum_kernel(const float *__restrict__ g, int cs,
                                                                 const int32_t *__restrict__ tab_s,
                                                                 const float *__restrict__ tab_w, int n, int views, int H,
                                                                 int W, float *__restrict__ out, int x_pieces)
{
    extern __shared__ float4 ese_lds[];                                     // (float4: a 16-byte aligned base)
    UnshiftTab *tab = reinterpret_cast<UnshiftTab *>(ese_lds);              // [n][views]
    float *tile = reinterpret_cast<float *>(tab + (size_t)n * views);       // [3 views][US_PITCH]
    const int P = W + GRID_PAD, R = H + GRID_PAD;
    const int y = blockIdx.x / x_pieces;
    const int x0 = (blockIdx.x - y * x_pieces) * US_XT;
    const int nx = min(US_XT, W - x0);
    for (int k = threadIdx.x; k < n * views; k += US_THREADS) {
        UnshiftTab t;
        t.s0 = tab_s[2 * k]; t.s1 = tab_s[2 * k + 1];
        t.w0 = tab_w[2 * k]; t.w1 = tab_w[2 * k + 1];
        tab[k] = t;
    }
    __syncthreads();
    const size_t member = (size_t)R * P * cs;
    for (int item = threadIdx.x; item < nx * views; item += US_THREADS) {
        const int xl = item / views, view = item - xl * views;             // view fastest
        const int x = x0 + xl;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        const float *gv = g + 3 * view;
        for (int s = 0; s < n; ++s, gv += member) {
            const UnshiftTab t = tab[s * views + view];
            auto at = [&](int yy, int xx) { return gv + ((size_t)(yy + 1) * P + (xx + 1)) * cs; };
            auto lerp = [&](float a, float b) { return __fadd_rn(__fmul_rn(a, t.w0), __fmul_rn(b, t.w1)); };
            float v0, v1, v2;
            if (KIND == 0 || KIND == 1) {
                const float *p0 = KIND == 0 ? at(y, unroll_src(x, t.s0, W)) : at(unroll_src(y, t.s0, H), x);
                const float *p1 = KIND == 0 ? at(y, unroll_src(x, t.s1, W)) : at(unroll_src(y, t.s1, H), x);
                v0 = lerp(p0[0], p1[0]);
                v1 = lerp(p0[1], p1[1]);
                v2 = lerp(p0[2], p1[2]);
            } else {
                const int sg = KIND == 2 ? -1 : 1;
                const int ya = unroll_src(y, sg * t.s0, H), yb = unroll_src(y, sg * t.s1, H);
                const int xa = unroll_src(x, t.s0, W), xb = unroll_src(x, t.s1, W);
                const float *paa = at(ya, xa), *pab = at(ya, xb), *pba = at(yb, xa), *pbb = at(yb, xb);
                v0 = lerp(lerp(paa[0], pab[0]), lerp(pba[0], pbb[0]));
                v1 = lerp(lerp(paa[1], pab[1]), lerp(pba[1], pbb[1]));
                v2 = lerp(lerp(paa[2], pab[2]), lerp(pba[2], pbb[2]));
            }
            a0 = __fadd_rn(a0, v0);
            a1 = __fadd_rn(a1, v1);
            a2 = __fadd_rn(a2, v2);
        }
        tile[(3 * view) * US_PITCH + xl] = a0;
        tile[(3 * view + 1) * US_PITCH + xl] = a1;
        tile[(3 * view + 2) * US_PITCH + xl] = a2;
    }
    __syncthreads();
    const int C = 3 * views;
    for (int e = threadIdx.x; e < C * nx; e += US_THREADS) {
        const int c = e / nx, xl = e - c * nx;                              // x fastest: whole row pieces of a plane
        float *o = out + ((size_t)c * H + y) * W + x0 + xl;
        *o = __fadd_rn(*o, tile[c * US_PITCH + xl]);
    }
}

extern "C" int mmlf_ese_unshift_sum(const float *g, int cs, int kind, const int32_t *tab_s, const float *tab_w, int n,
                                    int views, int H, int W, float *out, void *stream)
{
    ESE_CHECK_ARG(g && tab_s && tab_w && out, "mmlf_ese_unshift_sum: null pointer");
    ESE_CHECK_ARG(kind >= 0 && kind <= 3, "mmlf_ese_unshift_sum: kind=%d (0 .. 3)", kind);
    ESE_CHECK_ARG(views >= 1 && views <= MMLF_ESE_MAX_TAB && cs >= 4 && cs % 4 == 0 && cs <= (1 << 16) && 3 * views <= cs,
                  "mmlf_ese_unshift_sum: views=%d cs=%d (cs a multiple of 4 that holds 3 views channels)", views, cs);
    ESE_CHECK_ARG(n >= 1 && n <= MMLF_ESE_MAX_TAB / views, "mmlf_ese_unshift_sum: n=%d members of %d views (n views <= %d)",
                  n, views, MMLF_ESE_MAX_TAB);
    ESE_CHECK_ARG(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) &&
                      (long long)(H + GRID_PAD) * (W + GRID_PAD) <= (1ll << 40) / cs / n,
                  "mmlf_ese_unshift_sum: bad shape n=%d H=%d W=%d cs=%d", n, H, W, cs);
    const int x_pieces = (W + US_XT - 1) / US_XT;
    const long long blocks = (long long)H * x_pieces;
    ESE_CHECK_ARG(blocks <= 0x7fffffffll, "mmlf_ese_unshift_sum: shape H=%d W=%d is too large for one launch", H, W);
    const size_t lds = (size_t)n * views * sizeof(UnshiftTab) + (size_t)3 * views * US_PITCH * sizeof(float);
    ESE_CHECK_ARG(lds <= 64 * 1024, "mmlf_ese_unshift_sum: views=%d does not fit the transpose tile", views);
    const dim3 gr((unsigned)blocks), bl(US_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch (kind) {
    case 0: unshift_sum_kernel<0><<<gr, bl, lds, st>>>(g, cs, tab_s, tab_w, n, views, H, W, out, x_pieces); break;
    case 1: unshift_sum_kernel<1><<<gr, bl, lds, st>>>(g, cs, tab_s, tab_w, n, views, H, W, out, x_pieces); break;
    case 2: unshift_sum_kernel<2><<<gr, bl, lds, st>>>(g, cs, tab_s, tab_w, n, views, H, W, out, x_pieces); break;
    default: unshift_sum_kernel<3><<<gr, bl, lds, st>>>(g, cs, tab_s, tab_w, n, views, H, W, out, x_pieces); break;
    }
    return ese_launch_status("mmlf_ese_unshift_sum");
}
