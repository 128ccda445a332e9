// patch_chain.hip -- libmmlf_data_hip.so (gfx950): the composable training patch chain, include/mmlf_data_hip.h.
// Two gather kernels behind one entry point (view stacks; centre view, ground truth, MPI planes and mask) and one pass for
// Contrast and Noise.  Nothing here is shared with libmmlf_hip.so, libmmlf_eval_hip.so or libmmlf_ese_hip.so: this file
// includes none of their headers, so no other library's source hash sees it.  The per-pixel arithmetic of the gather is
// mmlf_patch_gather's (elementwise.hip), restated in the same operation order; what is new is that every frame coordinate
// goes through the per-sample index tables ymap / xmap (Zoom, DownSampling) and that the shear wraps the SCALED frame.
// Built with -ffp-contract=off: every float32 / float64 expression below is the sequence of IEEE operations that is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mmlf_data_hip.h"

static thread_local char g_data_err[512];

static int data_fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_data_err, sizeof(g_data_err), fmt, ap);
    va_end(ap);
    return 1;
}

#define DATA_CHECK_ARG(cond, ...)                   \
    do {                                            \
        if (!(cond)) return data_fail(__VA_ARGS__); \
    } while (0)

static int data_launch_status(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return data_fail("%s: launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

extern "C" const char *mmlf_data_last_error(void) { return g_data_err; }
extern "C" int mmlf_data_abi_version(void) { return MMLF_DATA_ABI_VERSION; }

// ---------------------------------------------------------------- the gather

constexpr int DATA_IP = 8;
constexpr int DATA_FP = 4;
constexpr int ROW_THREADS = 128;

struct ChainSample {
    int scene, hs, ws, y0, x0, rot, flags;
    float gscale, disp, bright;
};

__device__ __forceinline__ ChainSample chain_sample(const int32_t *ip, const float *fp, int b)
{
    ChainSample p;
    p.scene = ip[b * DATA_IP + 0]; p.hs = ip[b * DATA_IP + 1]; p.ws = ip[b * DATA_IP + 2];
    p.y0 = ip[b * DATA_IP + 3]; p.x0 = ip[b * DATA_IP + 4]; p.rot = ip[b * DATA_IP + 5];
    p.flags = ip[b * DATA_IP + 6];
    p.gscale = fp[b * DATA_FP + 0]; p.disp = fp[b * DATA_FP + 1]; p.bright = fp[b * DATA_FP + 2];
    return p;
}

struct ShearTab { int s0, s1; float w0, w1; };

__device__ __forceinline__ int wrapi(int a, int n) { a %= n; return a < 0 ? a + n : a; }
// source index of a roll by +s with Python-slice clamping (|s| >= n -> identity)
__device__ __forceinline__ int roll_src(int x, int s, int n) { return (s >= n || -s >= n) ? x : wrapi(x - s, n); }

// patch coordinates before `rot` applications of out[y][x] = in[x][ps-1-y] (flip(transpose(.)), hci4d.py:1058-1061)
__device__ __forceinline__ void unrotate(int rot, int ps, int &y, int &x)
{
    for (int k = 0; k < rot; ++k) {
        const int t = y;
        y = x;
        x = ps - 1 - t;
    }
}

// RedistColor: float64 matrix entry x float32 image, rounded to float32 after every step (numpy >= 2)
__device__ __forceinline__ void redist_color(const double *m, float &c0, float &c1, float &c2)
{
    const double s0 = c0, s1 = c1, s2 = c2;
    float o[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float a = (float)__dmul_rn(m[3 * r], s0);
        a = (float)__dadd_rn((double)a, __dmul_rn(m[3 * r + 1], s1));
        a = (float)__dadd_rn((double)a, __dmul_rn(m[3 * r + 2], s2));
        o[r] = a;
    }
    c0 = o[0]; c1 = o[1]; c2 = o[2];
}

// grid: (B * 4 stacks * V views * ps rows); threads over x.  out: (4, B, V, 3, ps, ps)
__global__ __launch_bounds__(ROW_THREADS) void chain_stacks_kernel(
    const float *__restrict__ stacks, const int32_t *__restrict__ ip, const float *__restrict__ fp,
    const int32_t *__restrict__ ymap, int map_h, const int32_t *__restrict__ xmap, int map_w,
    const int32_t *__restrict__ tab_s, const float *__restrict__ tab_w, const double *__restrict__ mat,
    const int32_t *__restrict__ rot_src, float *__restrict__ out, double *__restrict__ mean_sum, int B, int V,
    int Hf, int Wf, int ps)
{
    int r = blockIdx.x;
    const int y = r % ps; r /= ps;
    const int n = r % V; r /= V;
    const int so = r % 4;
    const int b = r / 4;
    const ChainSample p = chain_sample(ip, fp, b);
    const int src = rot_src[(p.rot * 4 + so) * V + n];
    const int ss = src / V, sn = src % V;                 // stack and view the pixel comes from
    const int Hd = p.hs, Wd = p.ws;                       // the scaled frame the shear wraps
    ShearTab t;
    t.s0 = tab_s[2 * (b * V + sn)]; t.s1 = tab_s[2 * (b * V + sn) + 1];
    t.w0 = tab_w[2 * (b * V + sn)]; t.w1 = tab_w[2 * (b * V + sn) + 1];
    const bool do_shift = p.flags & MMLF_DATA_SHEAR;
    const bool do_roll = p.flags & MMLF_DATA_ROLL;
    const size_t plane = (size_t)Hf * Wf;
    const float *base = stacks + (((size_t)p.scene * 4 + ss) * V + sn) * 3 * plane;
    const int32_t *ym = ymap + (size_t)b * map_h, *xm = xmap + (size_t)b * map_w;
    auto lerp = [&](float a, float c) { return __fadd_rn(__fmul_rn(a, t.w0), __fmul_rn(c, t.w1)); };
    double local = 0.0;
    for (int x = threadIdx.x; x < ps; x += blockDim.x) {
        int yy = y, xx = x;
        unrotate(p.rot, ps, yy, xx);
        const int Y = p.y0 + yy, X = p.x0 + xx;           // scaled-frame coordinates
        float c[3];
        if (do_roll) {                                    // IntegerShift: one tap, no arithmetic (hci4d.py:860-882)
            const int sg = ss == 2 ? -1 : 1;              // the I stack's second axis rolls the other way (:877-879)
            const int xr = ss == 1 ? X : roll_src(X, t.s0, Wd);
            const int yr = ss == 0 ? Y : roll_src(Y, sg * t.s0, Hd);
            const int ry = ym[yr], rx = xm[xr];
            const size_t o = (size_t)ry * Wf + rx;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = (ry | rx) < 0 ? 0.f : base[ch * plane + o];
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float *pl = base + ch * plane;
                auto at = [&](int yd, int xd) {           // a negative entry: Zoom's constant, zero (mmlf_data_hip.h)
                    const int ry = ym[yd], rx = xm[xd];
                    return (ry | rx) < 0 ? 0.f : pl[(size_t)ry * Wf + rx];
                };
                if (!do_shift) { c[ch] = at(Y, X); continue; }
                const int x0 = roll_src(X, t.s0, Wd), x1 = roll_src(X, t.s1, Wd);
                if (ss == 0) { c[ch] = lerp(at(Y, x0), at(Y, x1)); continue; }
                const int sg = ss == 2 ? -1 : 1;          // the I stack's vertical pass rolls by -s (:971-975)
                const int ya = roll_src(Y, sg * t.s0, Hd), yb = roll_src(Y, sg * t.s1, Hd);
                if (ss == 1) { c[ch] = lerp(at(ya, X), at(yb, X)); continue; }
                c[ch] = lerp(lerp(at(ya, x0), at(ya, x1)), lerp(at(yb, x0), at(yb, x1)));
            }
        }
        if (p.flags & MMLF_DATA_COLOR) redist_color(mat + 9 * b, c[0], c[1], c[2]);
        if (p.flags & MMLF_DATA_BRIGHT) {
            c[0] = __fmul_rn(c[0], p.bright); c[1] = __fmul_rn(c[1], p.bright); c[2] = __fmul_rn(c[2], p.bright);
        }
        float *o = out + ((((size_t)so * B + b) * V + n) * 3 * ps + y) * ps + x;
        o[0] = c[0]; o[(size_t)ps * ps] = c[1]; o[(size_t)2 * ps * ps] = c[2];
        local += (double)c[0] + (double)c[1] + (double)c[2];
    }
    if (so == 0 && mean_sum) {                            // Contrast's mean is over data[0] (:742)
        __shared__ double red[ROW_THREADS];
        red[threadIdx.x] = local;
        __syncthreads();
        for (int k = ROW_THREADS / 2; k > 0; k >>= 1) {
            if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
            __syncthreads();
        }
        if (threadIdx.x == 0) atomicAdd(mean_sum + b, red[0]);
    }
}

// ground-truth corrections in the reference's order: the scale's (Zoom: times, DownSampling: divided by), then the shear's
__device__ __forceinline__ float correct_disparity(float g, const ChainSample &p)
{
    if (p.flags & MMLF_DATA_GT_MUL) g = __fmul_rn(g, p.gscale);
    if (p.flags & MMLF_DATA_GT_DIV) g = __fdiv_rn(g, p.gscale);
    if (p.flags & (MMLF_DATA_SHEAR | MMLF_DATA_ROLL)) g = __fsub_rn(g, p.disp);
    return g;
}

// centre view, ground truth, MPI planes and mask.  grid: (B * (1 + 1 + 5P + 1) planes * ps rows)
__global__ __launch_bounds__(ROW_THREADS) void chain_planes_kernel(
    const float *__restrict__ center, const float *__restrict__ gt, const float *__restrict__ mpi,
    const int32_t *__restrict__ mask, const int32_t *__restrict__ ip, const float *__restrict__ fp,
    const int32_t *__restrict__ ymap, int map_h, const int32_t *__restrict__ xmap, int map_w,
    const double *__restrict__ mat, float *__restrict__ o_center, float *__restrict__ o_gt,
    float *__restrict__ o_mpi, int32_t *__restrict__ o_mask, int B, int P, int Hf, int Wf, int ps)
{
    const int nplanes = 1 + 1 + 5 * P + 1;                // centre (3 channels at once), gt, mpi, mask
    int r = blockIdx.x;
    const int y = r % ps; r /= ps;
    const int k = r % nplanes;
    const int b = r / nplanes;
    const ChainSample p = chain_sample(ip, fp, b);
    const size_t plane = (size_t)Hf * Wf;
    const int32_t *ym = ymap + (size_t)b * map_h, *xm = xmap + (size_t)b * map_w;
    for (int x = threadIdx.x; x < ps; x += blockDim.x) {
        int yy = y, xx = x;
        if (k != nplanes - 1) unrotate(p.rot, ps, yy, xx);            // the mask is not rotated (:1056)
        const int ry = ym[p.y0 + yy], rx = xm[p.x0 + xx];
        const bool fill = (ry | rx) < 0;                               // Zoom's constant: zero in every plane
        const size_t src = fill ? 0 : (size_t)ry * Wf + rx;
        const size_t dst = (size_t)y * ps + x;
        if (k == 0) {                                                  // centre: the shear touches the stacks only
            const float *pc = center + (size_t)p.scene * 3 * plane;
            float c0 = pc[src], c1 = pc[plane + src], c2 = pc[2 * plane + src];
            if (fill) c0 = c1 = c2 = 0.f;
            if (p.flags & MMLF_DATA_COLOR) redist_color(mat + 9 * b, c0, c1, c2);
            if (p.flags & MMLF_DATA_BRIGHT) {
                c0 = __fmul_rn(c0, p.bright); c1 = __fmul_rn(c1, p.bright); c2 = __fmul_rn(c2, p.bright);
            }
            float *o = o_center + (size_t)b * 3 * ps * ps + dst;
            o[0] = c0; o[(size_t)ps * ps] = c1; o[(size_t)2 * ps * ps] = c2;
        } else if (k == 1) {
            o_gt[(size_t)b * ps * ps + dst] = correct_disparity(fill ? 0.f : gt[(size_t)p.scene * plane + src], p);
        } else if (k == nplanes - 1) {
            o_mask[(size_t)b * ps * ps + dst] = fill ? 0 : mask[(size_t)p.scene * plane + src];
        } else {                                                       // mpi[:, 4] carries the same corrections
            const int q = k - 2;
            float v = fill ? 0.f : mpi[((size_t)p.scene * 5 * P + q) * plane + src];
            if (q % 5 == 4) v = correct_disparity(v, p);
            o_mpi[((size_t)b * 5 * P + q) * ps * ps + dst] = v;
        }
    }
}

extern "C" int mmlf_data_gather(const float *stacks, const float *center, const float *gt, const float *mpi,
                                const int32_t *mask, int S, int V, int P, int Hf, int Wf, const int32_t *iparam,
                                const float *fparam, const int32_t *ymap, int map_h, const int32_t *xmap, int map_w,
                                const int32_t *tab_s, const float *tab_w, const double *mat, const int32_t *rot_src,
                                float *o_stacks, float *o_center, float *o_gt, float *o_mpi, int32_t *o_mask,
                                double *mean_sum, int B, int ps, void *stream)
{
    DATA_CHECK_ARG(stacks && center && gt && mask && iparam && fparam && ymap && xmap && tab_s && tab_w && mat && rot_src,
                   "mmlf_data_gather: null input");
    DATA_CHECK_ARG(o_stacks && o_center && o_gt && o_mask, "mmlf_data_gather: null output");
    DATA_CHECK_ARG(S > 0 && V > 0 && P >= 0 && Hf > 0 && Wf > 0 && B > 0 && ps > 0,
                   "mmlf_data_gather: bad shape S=%d V=%d P=%d frame %dx%d B=%d ps=%d", S, V, P, Hf, Wf, B, ps);
    DATA_CHECK_ARG(map_h >= ps && map_w >= ps, "mmlf_data_gather: index tables of %d x %d entries for a %d-px patch",
                   map_h, map_w, ps);
    DATA_CHECK_ARG(P == 0 || (mpi && o_mpi), "mmlf_data_gather: P=%d but no mpi buffers", P);
    DATA_CHECK_ARG((long long)B * 4 * V * ps < (1ll << 31) && (long long)B * (3 + 5ll * P) * ps < (1ll << 31),
                   "mmlf_data_gather: grid too large");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(chain_stacks_kernel, dim3((unsigned)(B * 4 * V * ps)), dim3(ROW_THREADS), 0, st, stacks, iparam,
                       fparam, ymap, map_h, xmap, map_w, tab_s, tab_w, mat, rot_src, o_stacks, mean_sum, B, V, Hf, Wf, ps);
    hipLaunchKernelGGL(chain_planes_kernel, dim3((unsigned)(B * (3 + 5 * P) * ps)), dim3(ROW_THREADS), 0, st, center, gt,
                       mpi, mask, iparam, fparam, ymap, map_h, xmap, map_w, mat, o_center, o_gt, o_mpi, o_mask, B, P, Hf,
                       Wf, ps);
    return data_launch_status("mmlf_data_gather");
}

// ---------------------------------------------------------------- Contrast + Noise

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1; c[3] = (uint32_t)p0;
        c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// Box-Muller on two words: u1 in (0, 1] and u2 in [0, 1) with 24 bits each (every value exact in float32)
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float &z0, float &z1)
{
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(b >> 8) * 0x1p-24f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    z0 = rad * cs;
    z1 = rad * sn;
}

constexpr int FIN_THREADS = 256;

// One thread per group of 4 consecutive elements of [o_stacks | o_center] (n_st = 4 B per_stack is a multiple of 4, so a
// group never straddles the two buffers); the group index is the generator's counter, whatever the launch geometry.
__global__ __launch_bounds__(FIN_THREADS) void chain_finish_kernel(
    float *__restrict__ stacks, float *__restrict__ center, const double *__restrict__ mean_sum,
    const float *__restrict__ alpha, int noise, float stdev, uint32_t k0, uint32_t k1, uint32_t call_lo, uint32_t call_hi,
    int B, long long per_stack /* V*3*ps*ps */, long long per_center /* 3*ps*ps */, long long n_st, long long total)
{
    const long long groups = (total + 3) / 4;
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        const long long e0 = 4 * g;
        const bool in_st = e0 < n_st;
        float *base = in_st ? stacks + e0 : center + (e0 - n_st);
        const int cnt = (int)(total - e0 < 4 ? total - e0 : 4);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (cnt == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(base);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int j = 0; j < cnt; ++j) v[j] = base[j];
        }
        if (alpha) {
            for (int j = 0; j < cnt; ++j) {
                const long long e = e0 + j;
                const int b = in_st ? (int)((e / per_stack) % B) : (int)((e - n_st) / per_center);
                const float a = alpha[2 * b];                           // float32(alpha), float32(1 - alpha)
                const float mean = (float)(mean_sum[b] / (double)per_stack);
                const float off = __fmul_rn(mean, alpha[2 * b + 1]);
                v[j] = __fadd_rn(__fmul_rn(v[j], a), off);
            }
        }
        if (noise) {
            uint32_t c[4] = {(uint32_t)g, (uint32_t)((uint64_t)g >> 32), call_lo, call_hi};
            philox4x32_10(c, k0, k1);
            float z[4];
            box_muller(c[0], c[1], z[0], z[1]);
            box_muller(c[2], c[3], z[2], z[3]);
            for (int j = 0; j < cnt; ++j)                               // float32 += float64 (hci4d.py:815-816)
                v[j] = (float)__dadd_rn((double)v[j], __dmul_rn((double)stdev, (double)z[j]));
        }
        if (cnt == 4) {
            *reinterpret_cast<float4 *>(base) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int j = 0; j < cnt; ++j) base[j] = v[j];
        }
    }
}

extern "C" int mmlf_data_finish(float *o_stacks, float *o_center, const double *mean_sum, const float *alpha, int noise,
                                float stdev, int64_t seed, int64_t call, int B, int V, int ps, void *stream)
{
    DATA_CHECK_ARG(o_stacks && o_center, "mmlf_data_finish: null output");
    DATA_CHECK_ARG(B > 0 && V > 0 && ps > 0, "mmlf_data_finish: bad shape B=%d V=%d ps=%d", B, V, ps);
    DATA_CHECK_ARG(!alpha || mean_sum, "mmlf_data_finish: Contrast without the sums of the horizontal stack");
    DATA_CHECK_ARG(alpha || noise, "mmlf_data_finish: neither Contrast nor Noise");
    DATA_CHECK_ARG(!noise || (stdev >= 0.f && stdev == stdev), "mmlf_data_finish: bad noise stdev %g", (double)stdev);
    DATA_CHECK_ARG(((uintptr_t)o_stacks & 15) == 0 && ((uintptr_t)o_center & 15) == 0,
                   "mmlf_data_finish: outputs must be 16-byte aligned");
    const long long per_center = 3ll * ps * ps, per_stack = per_center * V;
    DATA_CHECK_ARG(per_stack <= (1ll << 40) / B / 4, "mmlf_data_finish: batch too large");
    const long long n_st = 4ll * B * per_stack, total = n_st + (long long)B * per_center;
    const long long groups = (total + 3) / 4;
    long long blocks = (groups + FIN_THREADS - 1) / FIN_THREADS;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(chain_finish_kernel, dim3((unsigned)blocks), dim3(FIN_THREADS), 0, (hipStream_t)stream, o_stacks,
                       o_center, mean_sum, alpha, noise, stdev, (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32),
                       (uint32_t)(uint64_t)call, (uint32_t)((uint64_t)call >> 32), B, per_stack, per_center, n_st, total);
    return data_launch_status("mmlf_data_finish");
}
