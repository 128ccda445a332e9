// scene.hip -- libmmlf_scene_hip.so (gfx950): a cached training scene from decoded view images, include/mmlf_scene_hip.h.
// Two kernels: the texture mask of hci4d.create_mask_texture (each pixel's window walked out of an LDS tile) and the pass
// from HWC images to the four CHW float view stacks.  Nothing here is shared with the four other libraries: this file
// includes none of their headers, so no other library's source hash sees it.
// Built with -ffp-contract=off: every float32 expression below is the sequence of IEEE operations that is written.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mmlf_scene_hip.h"

static thread_local char g_scene_err[512];

static int scene_fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_scene_err, sizeof(g_scene_err), fmt, ap);
    va_end(ap);
    return 1;
}

#define SCENE_CHECK_ARG(cond, ...)                   \
    do {                                             \
        if (!(cond)) return scene_fail(__VA_ARGS__); \
    } while (0)

static int scene_launch_status(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return scene_fail("%s: launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

extern "C" const char *mmlf_scene_last_error(void) { return g_scene_err; }
extern "C" int mmlf_scene_abi_version(void) { return MMLF_SCENE_ABI_VERSION; }

// ---------------------------------------------------------------- the texture mask
//
// One workgroup of 256 lanes per 32 x 32 output tile.  The tile and its halo of R = wsize / 2 pixels, all three channels,
// are staged in LDS as [channel][TEX_T + 2R rows][TEX_T + 2R columns] float32, zero outside the frame (unfold's padding).
// A lane owns column tx = lane % 32 and the four rows 4 * (lane / 32) .. + 3 of the tile.  The 32 lanes of a half-wave
// read 32 consecutive floats of one LDS row (ds_read_b32 banks a half-wave at a time: consecutive dwords, no conflict,
// whatever the row stride), and the two halves of a wave read rows that belong to different lanes' pixels.  Four
// vertically adjacent pixels share wsize - 1 .. wsize - 3 of their window rows, so every value read from LDS feeds up to
// four |x - c| terms: wsize + 3 row walks per channel instead of 4 * wsize.
constexpr int TEX_T = 32;              // tile edge, pixels
constexpr int TEX_PPL = 4;             // pixels per lane (vertically adjacent)
constexpr int TEX_THREADS = TEX_T * TEX_T / TEX_PPL;

__global__ __launch_bounds__(TEX_THREADS) void scene_texture_kernel(
    const float *__restrict__ center, int wsize, float threshold, float denom, const int32_t *__restrict__ mask_in,
    int32_t *__restrict__ mask_out, float *__restrict__ mae_out, int H, int W)
{
    extern __shared__ float tile[];
    const int R = wsize >> 1;
    const int LW = TEX_T + 2 * R, LH = TEX_T + 2 * R;
    const int b = blockIdx.z, ty0 = blockIdx.y * TEX_T, tx0 = blockIdx.x * TEX_T;
    const size_t plane = (size_t)H * W;
    const float *src = center + (size_t)b * 3 * plane;
    const int tid = threadIdx.x;

    // stage: every halo load is range-checked and reads as zero outside the frame
    const int per_ch = LH * LW;
    for (int i = tid; i < 3 * per_ch; i += TEX_THREADS) {
        const int ch = i / per_ch, rem = i - ch * per_ch;
        const int ly = rem / LW, lx = rem - ly * LW;
        const int gy = ty0 - R + ly, gx = tx0 - R + lx;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = src[ch * plane + (size_t)gy * W + gx];
        tile[i] = v;
    }
    __syncthreads();

    const int tx = tid & (TEX_T - 1), py = (tid / TEX_T) * TEX_PPL;
    float acc[TEX_PPL];
#pragma unroll
    for (int k = 0; k < TEX_PPL; ++k) acc[k] = 0.f;
    for (int ch = 0; ch < 3; ++ch) {
        const float *base = tile + ch * per_ch;
        float c[TEX_PPL];
#pragma unroll
        for (int k = 0; k < TEX_PPL; ++k) c[k] = base[(py + k + R) * LW + tx + R];
        // window row r of the lane's first pixel is tile row py + r; pixel k uses rows k .. k + wsize - 1
        for (int r = 0; r < wsize + TEX_PPL - 1; ++r) {
            const float *row = base + (py + r) * LW + tx;
            if (r >= TEX_PPL - 1 && r < wsize) {               // a row all four windows hold
                for (int dx = 0; dx < wsize; ++dx) {
                    const float v = row[dx];
#pragma unroll
                    for (int k = 0; k < TEX_PPL; ++k) acc[k] = __fadd_rn(acc[k], fabsf(__fsub_rn(v, c[k])));
                }
            } else {
                bool use[TEX_PPL];
#pragma unroll
                for (int k = 0; k < TEX_PPL; ++k) use[k] = r >= k && r - k < wsize;
                for (int dx = 0; dx < wsize; ++dx) {
                    const float v = row[dx];
#pragma unroll
                    for (int k = 0; k < TEX_PPL; ++k)
                        if (use[k]) acc[k] = __fadd_rn(acc[k], fabsf(__fsub_rn(v, c[k])));
                }
            }
        }
    }

    const int gx = tx0 + tx;
    if (gx >= W) return;
#pragma unroll
    for (int k = 0; k < TEX_PPL; ++k) {
        const int gy = ty0 + py + k;
        if (gy >= H) break;
        const size_t o = (size_t)b * plane + (size_t)gy * W + gx;
        const float mae = __fdiv_rn(acc[k], denom);            // sum, then one division: the reference's mean
        if (mae_out) mae_out[o] = mae;
        if (mask_out) {
            int m = (mae >= threshold) ? 1 : 0;                // a NaN compares false
            if (gy < R || gy >= H - R || gx < R || gx >= W - R) m = 0;
            if (mask_in) m *= mask_in[o];
            mask_out[o] = m;
        }
    }
}

extern "C" int mmlf_scene_texture(const float *center, int wsize, double threshold, const int32_t *mask_in,
                                  int32_t *mask_out, float *mae_out, int B, int H, int W, void *stream)
{
    SCENE_CHECK_ARG(center, "mmlf_scene_texture: null center");
    SCENE_CHECK_ARG(mask_out || mae_out, "mmlf_scene_texture: neither mask_out nor mae_out");
    SCENE_CHECK_ARG(wsize >= 1 && wsize <= MMLF_SCENE_MAX_WSIZE, "mmlf_scene_texture: wsize %d not in [1, %d]", wsize,
                    MMLF_SCENE_MAX_WSIZE);
    SCENE_CHECK_ARG(wsize % 2 == 1, "mmlf_scene_texture: even wsize %d (the window has no centre pixel)", wsize);
    SCENE_CHECK_ARG(B > 0 && H > 0 && W > 0, "mmlf_scene_texture: bad shape B=%d H=%d W=%d", B, H, W);
    SCENE_CHECK_ARG((long long)B * H * W <= INT_MAX / 3, "mmlf_scene_texture: 3*B*H*W = 3*%d*%d*%d exceeds 2^31 - 1", B,
                    H, W);
    const int tiles_x = (W + TEX_T - 1) / TEX_T, tiles_y = (H + TEX_T - 1) / TEX_T;
    SCENE_CHECK_ARG(B <= 65535 && tiles_y <= 65535, "mmlf_scene_texture: B=%d or H=%d too large for one launch", B, H);
    const int R = wsize / 2;
    const size_t lds = (size_t)3 * (TEX_T + 2 * R) * (TEX_T + 2 * R) * sizeof(float);       // 35 KB at 23, 106 KB at 63
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(scene_texture_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return scene_fail("mmlf_scene_texture: %zu bytes of LDS for wsize %d refused: %s", lds, wsize,
                              hipGetErrorString(e));
    }
    hipLaunchKernelGGL(scene_texture_kernel, dim3(tiles_x, tiles_y, B), dim3(TEX_THREADS), lds, (hipStream_t)stream,
                       center, wsize, (float)threshold, (float)(3 * wsize * wsize), mask_in, mask_out, mae_out, H, W);
    return scene_launch_status("mmlf_scene_texture");
}

// ---------------------------------------------------------------- the view stacks
//
// One workgroup per (slot, image row): 256 pixels of the HWC row at a time go through LDS, read as consecutive elements
// (single bytes for a uint8 grid: W * 3 is in general no multiple of 4, so nothing wider is aligned) and written as three
// runs of consecutive floats, one per channel plane.  The stride-3 LDS read is conflict-free (3 is odd).
constexpr int PACK_PX = 256;

__global__ __launch_bounds__(PACK_PX) void scene_pack_kernel(
    const uint8_t *__restrict__ grid_u8, const float *__restrict__ grid_f32, const float *__restrict__ lut,
    const int32_t *__restrict__ sel, int center_slot, int N, int H, int W, float *__restrict__ stacks,
    float *__restrict__ center)
{
    __shared__ float row[PACK_PX * 3];
    const int slot = blockIdx.x / H, y = blockIdx.x - slot * H;
    const int img = sel[slot];
    if (img < 0 || img >= N) return;                           // (the whole workgroup: no barrier is left behind)
    const size_t plane = (size_t)H * W;
    const size_t in0 = ((size_t)img * H + y) * W * 3;
    const int tid = threadIdx.x;
    for (int x0 = 0; x0 < W; x0 += PACK_PX) {
        const int px = min(PACK_PX, W - x0);
        for (int i = tid; i < px * 3; i += PACK_PX) {
            const size_t e = in0 + (size_t)x0 * 3 + i;
            row[i] = grid_u8 ? lut[grid_u8[e]] : grid_f32[e];
        }
        __syncthreads();
        if (tid < px) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float v = row[tid * 3 + ch];
                const size_t o = ch * plane + (size_t)y * W + x0 + tid;
                stacks[(size_t)slot * 3 * plane + o] = v;
                if (slot == center_slot) center[o] = v;
            }
        }
        __syncthreads();
    }
}

extern "C" int mmlf_scene_pack_views(const uint8_t *grid_u8, const float *grid_f32, const float *lut, const int32_t *sel,
                                     int center_slot, int N, int V, int H, int W, float *stacks, float *center,
                                     void *stream)
{
    SCENE_CHECK_ARG((grid_u8 != nullptr) != (grid_f32 != nullptr), "mmlf_scene_pack_views: exactly one of grid_u8 and grid_f32");
    SCENE_CHECK_ARG(!grid_u8 || lut, "mmlf_scene_pack_views: a uint8 grid needs the 256-entry table");
    SCENE_CHECK_ARG(sel && stacks && center, "mmlf_scene_pack_views: null sel, stacks or center");
    SCENE_CHECK_ARG(N > 0 && V > 0 && H > 0 && W > 0, "mmlf_scene_pack_views: bad shape N=%d V=%d H=%d W=%d", N, V, H, W);
    SCENE_CHECK_ARG(V <= INT_MAX / 4 && center_slot >= 0 && center_slot < 4 * V,
                    "mmlf_scene_pack_views: center_slot %d not in [0, 4*%d)", center_slot, V);
    SCENE_CHECK_ARG((long long)N * H * W <= INT_MAX / 3, "mmlf_scene_pack_views: N*H*W*3 = %d*%d*%d*3 exceeds 2^31 - 1", N,
                    H, W);
    SCENE_CHECK_ARG(4ll * V * H * W <= INT_MAX / 3, "mmlf_scene_pack_views: 4*V*3*H*W = 4*%d*3*%d*%d exceeds 2^31 - 1", V,
                    H, W);
    hipLaunchKernelGGL(scene_pack_kernel, dim3((unsigned)(4 * V * H)), dim3(PACK_PX), 0, (hipStream_t)stream, grid_u8,
                       grid_f32, lut, sel, center_slot, N, H, W, stacks, center);
    return scene_launch_status("mmlf_scene_pack_views");
}
