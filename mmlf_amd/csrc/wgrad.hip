// wgrad.hip -- weight + bias gradient of the k=2 and k=3 convolutions on the padded NHWC grid (exact-f32 MFMA:
// wgrad_f32_taps<KS, NT>, the one body behind wgrad4tap_kernel and wgrad9tap_kernel; for k=2 also the split-arithmetic
// kernels wgrad4tap_x6w / x6n), the thin (1-2 output channel) weight gradient, their C ABI entry points.
// gfx950 only.  Arithmetic replaced: the weight / bias gradient of nn.Conv2d(k=2, pad 1|0), reference
// mmlf/model/feed_forward.py:123,125 under autograd (mmlf/train/cli.py:257).
#include "conv_device.h"
#include "wgrad_map.h"
#include "row_walk.h"

#ifdef MMLF_BOUNDS_DEBUG
int mmlf_oob_counts_wgrad(unsigned long long *host8, int reset)
{
    if (hipMemcpyFromSymbol(host8, HIP_SYMBOL(g_mmlf_oob), sizeof(unsigned long long) * 8) != hipSuccess) return 1;
    if (reset) {
        const unsigned long long z[8] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_mmlf_oob), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif

// ---------------------------------------------------------------------------------------------
// weight-gradient kernel: dW[t][ci][co] = sum_q in[q + off_t][ci] * g[q + g_shift][co]
// ---------------------------------------------------------------------------------------------
struct WgradArgs {
    const float *in;
    const float *g;
    float *part;          // [nsplit][4][CIP][NP]
    long long NQpad;
    int cs_in, cin, cs_g, g_shift, P, nsplit, nslice, chunks_per_split, nchunks;
    int items;            // blocks of the one-shot launch, wgrad_grid_blocks(nslice, nsplit): what the persistent wide kernel walks
    int g_cols;           // channels of a row of g from the pointer on: cs_g, less the offset of a column block (wgrad_impl)
    const float *in_amax, *g_amax;   // f16 split: amax arrays of in and g (common.h)
    const float *chunk_scales;       // f16 split: [nchunks][2] power-of-two operand scales (wgrad_chunk_scales_kernel)
    long long in_bytes, g_bytes, part_floats;   // what the buffers hold by the ABI's contract: the wide kernel's staging loads are
                                                // range-checked against in_bytes / g_bytes (buffer descriptors); the rest is read by
                                                // the MMLF_BOUNDS_DEBUG build only
};

// block -> (slice, split) item, the wide launch's splits and its grid: wgrad_map.h (shared with tools/wgrad_items.hip)
#define WG_KQ 32  // positions per chunk

// Exact-f32 weight + bias gradient of both filter sizes: one body on KS = 2 (wgrad4tap_kernel) or 3 (wgrad9tap_kernel),
//   gw[co][ci][tap] (+)= sum_q in[q + dy*P + dx][ci] * g[q + g_shift][co],  gb[co] (+)= sum_q g[q + g_shift][co].
// MFMA rows = ci (A operand), cols = co (B operand), K = positions.  The first channel past Cin
// is staged as 1.0 so that row Cin of tap 0 accumulates the bias gradient for free.
//  KS = 2: 256 threads = 4 waves, wave = tap (dy, dx); block = (32-channel ci slice, position split), both tap rows staged.
//  KS = 3: one tap ROW per workgroup: 192 threads = 3 waves, wave = dx; block = (32-channel ci slice, dy, position
//          split), so that nine accumulator sets of up to 9 x 16 registers never share a workgroup.  The gradient tile is
//          staged once per (slice, dy) block; the three dy blocks of a slice read it from L2.
// Partial sums: [nsplit][KS*KS][CIP][NP].
template <int KS>
struct WgradF32Shape {
    static constexpr int WAVES = KS == 2 ? 4 : 3;
    static constexpr int SEGS = KS == 2 ? 2 : 1;       // tap rows staged per workgroup
    static constexpr int BPS = KS / SEGS;              // workgroups per ci slice: one per group of SEGS tap rows
    static constexpr int ROWS = WG_KQ + KS - 1;        // positions of one tap row: the chunk's and the dx behind them
    static constexpr int A_FL = SEGS * ROWS * 32;      // floats
    static constexpr size_t lds_bytes(int nt) { return (A_FL + WG_KQ * nt * 32) * sizeof(float); }
};

template <int KS, int NT>
__device__ __forceinline__ void wgrad_f32_taps(const WgradArgs &a)
{
    using S = WgradF32Shape<KS>;
    constexpr int TAPS = KS * KS, THREADS = 64 * S::WAVES, SEGS = S::SEGS, BPS = S::BPS, ROWS = S::ROWS, A_FL = S::A_FL;
    constexpr int NP = NT * 32;
    constexpr int A_F4 = A_FL / 4;
    constexpr int NA = (A_F4 + THREADS - 1) / THREADS;
    constexpr int G_F4 = WG_KQ * NP / 4;
    constexpr int NG = (G_F4 + THREADS - 1) / THREADS;
    static_assert(KS == 3 || G_F4 % THREADS == 0, "2x2: the gradient tile is a whole number of staging rounds (no guard)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *As = reinterpret_cast<float *>(smem);
    float *Gs = As + A_FL;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int i = lane & 31, kh = lane >> 5;
    int sd, split;
    if (!wgrad_block_map(blockIdx.x, a.nslice, a.nsplit, sd, split)) return;
    const int slice = sd / BPS, dy = sd - BPS * slice;
    const int ci0 = slice * 32;
    int c_begin = split * a.chunks_per_split;
    int c_end = c_begin + a.chunks_per_split;
    if (c_end > a.nchunks) c_end = a.nchunks;

    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    float4 ra[NA], rg[NG];
    auto gload = [&](int c) {
        const long long Qc = (long long)c * WG_KQ + (long long)dy * a.P;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int idx = tid + THREADS * j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < A_F4) {
                const int row = idx >> 3, f = idx & 7;
                const int seg = SEGS > 1 && row >= ROWS, pix = row - ROWS * seg;
                const int ch = ci0 + 4 * f;
                if (ch < a.cs_in)
                    v = *reinterpret_cast<const float4 *>(a.in + (size_t)(Qc + seg * a.P + pix) * a.cs_in + ch);
            }
            ra[j] = v;
        }
        const long long Qg = (long long)c * WG_KQ + a.g_shift;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int idx = tid + THREADS * j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (KS == 2 || idx < G_F4) {
                const int row = idx / (NP / 4), f = idx - row * (NP / 4);
                if (4 * f < a.g_cols) v = *reinterpret_cast<const float4 *>(a.g + (size_t)(Qg + row) * a.cs_g + 4 * f);
            }
            rg[j] = v;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int idx = tid + THREADS * j;
            if (idx < A_F4) {
                float4 v = ra[j];          // ones row (bias gradient) patched at store time
                const int ch = ci0 + 4 * (idx & 7);
                if (ch == a.cin) v.x = 1.f;
                if (ch + 1 == a.cin) v.y = 1.f;
                if (ch + 2 == a.cin) v.z = 1.f;
                if (ch + 3 == a.cin) v.w = 1.f;
                reinterpret_cast<float4 *>(As)[idx] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int idx = tid + THREADS * j;
            if (KS == 2 || idx < G_F4) reinterpret_cast<float4 *>(Gs)[idx] = rg[j];
        }
    };

    const int seg = KS == 2 ? wv >> 1 : 0, dx = KS == 2 ? wv & 1 : wv;   // this wave's tap: row dy + seg, column dx
    if (c_begin < c_end) {
        gload(c_begin);
        for (int c = c_begin; c < c_end; ++c) {
            lstore();
            __syncthreads();
            if (c + 1 < c_end) gload(c + 1);
            const float *ap = As + (seg * ROWS + dx + kh) * 32 + i;
            const float *gp = Gs + kh * NP + i;
#pragma unroll
            for (int s = 0; s < WG_KQ / 2; ++s) {
                const float av = ap[2 * s * 32];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float bv = gp[2 * s * NP + 32 * nt];
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[nt], 0, 0, 0);
                }
            }
            __syncthreads();
        }
    }
    const int CIP = a.nslice / BPS * 32;
    float *pp = a.part + ((size_t)(split * TAPS + KS * (dy + seg) + dx) * CIP + ci0) * NP;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
            pp[(size_t)row * NP + 32 * nt + i] = acc[nt][r];
        }
}

template <int NT>
__global__ __launch_bounds__(256, 2) void wgrad4tap_kernel(WgradArgs a)
{
    wgrad_f32_taps<2, NT>(a);
}

template <int NT>
__global__ __launch_bounds__(192, 2) void wgrad9tap_kernel(WgradArgs a)
{
    wgrad_f32_taps<3, NT>(a);
}

// ---------------------------------------------------------------------------------------------
// weight-gradient kernels, split-bf16 arithmetic (same decomposition as wgrad4tap_kernel).
// K = positions: the bf16 MFMA wants 8 consecutive positions per lane for a fixed channel, i.e. the
// transposed image of the NHWC tiles.  The tiles are split into three bf16 planes while they are staged
// (registers -> LDS, row-major [position][channel] like global memory) and the fragments are fetched
// with ds_read_b64_tr_b16, gfx950's transposing LDS read.
// ---------------------------------------------------------------------------------------------
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;

__device__ __forceinline__ bf16x8 tr_frag(const char *lds_row0, int row_stride_bytes)
{
    // two transposed 4-row reads = k 0..3 and 4..7 of this lane's column
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(lds_row0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(lds_row0 + 4 * row_stride_bytes));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ void split_store4(float4 v, char *p0, int plane_stride_bytes)
{
    unsigned h0, m0, l0, h1, m1, l1;
    split3_pair(v.x, v.y, h0, m0, l0);
    split3_pair(v.z, v.w, h1, m1, l1);
    *reinterpret_cast<uint2 *>(p0) = make_uint2(h0, h1);
    *reinterpret_cast<uint2 *>(p0 + plane_stride_bytes) = make_uint2(m0, m1);
    *reinterpret_cast<uint2 *>(p0 + 2 * plane_stride_bytes) = make_uint2(l0, l1);
}

// plane-count generic pieces of the weight-gradient kernels: PL = 3 bf16 planes / six cross terms, or
// PL = 2 f16 planes of the scaled operands / three cross terms (see split2_pair_f16)
template <int PL>
__device__ __forceinline__ void split_store4_pl(float4 v, float scale, char *p0, int plane_stride_bytes)
{
    if constexpr (PL == 3) {
        split_store4(v, p0, plane_stride_bytes);
    } else {
        unsigned h0, l0, h1, l1;
        split2_pair_f16<true>(v.x, v.y, scale, h0, l0);
        split2_pair_f16<true>(v.z, v.w, scale, h1, l1);
        *reinterpret_cast<uint2 *>(p0) = make_uint2(h0, h1);
        *reinterpret_cast<uint2 *>(p0 + plane_stride_bytes) = make_uint2(l0, l1);
    }
}
template <int PL>
__device__ __forceinline__ f32x4 mfma16_pl(bf16x8 x, bf16x8 y, f32x4 c)
{
    if constexpr (PL == 3) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, x), __builtin_bit_cast(f16x8, y), c, 0, 0, 0);
}
// cross terms (activation plane, gradient plane), small ones first
template <int PL> __device__ __forceinline__ constexpr int term_a(int t)
{
    return PL == 3 ? (t == 0 ? 2 : t == 1 ? 0 : t <= 3 ? 1 : 0) : (t == 0 ? 1 : 0);
}
template <int PL> __device__ __forceinline__ constexpr int term_b(int t)
{
    return PL == 3 ? (t == 0 ? 0 : t == 1 ? 2 : t == 2 ? 1 : t == 3 ? 0 : t == 4 ? 1 : 0) : (t == 1 ? 1 : 0);
}
// f16 split of the weight gradient.  The sum runs over all positions, so every chunk of 32 positions must carry
// the SAME product of operand scales -- but the split between the two operands is free per chunk:
//   in * (sA * 2^x)  and  g * (sG * 2^-x),   sA, sG = the tensors' global scales (max |.| -> [2^14, 2^15)),
// with x chosen per chunk by wgrad_chunk_scales_kernel from the maxima of the grid rows the chunk reads: if the
// chunk's activations sit u binades below their tensor's maximum and its gradients v binades below theirs,
// x = (u - v) / 2 gives each operand (u + v) / 2 binades of headroom loss instead of u resp. v, so a chunk keeps
// all 22 bits of both operands as long as its products are within 2^-36 of the largest products of the launch
// (smaller ones are below float32's accumulation error of the sum anyway).  The ones row that yields the bias
// gradient is staged as 1 / sA, i.e. 2^x after scaling: exact in f16 for -24 <= x <= 15, which bounds x.
struct WgradScales { float inv_sa, inv_sg; };
template <int PL> __device__ __forceinline__ WgradScales wgrad_scales(const WgradArgs &a)
{
    WgradScales s = {1.f, 1.f};
    if constexpr (PL == 2) {
        // left behind the per-chunk scales by wgrad_chunk_scales_kernel (the tensors' maxima live in 64 shards)
        s.inv_sa = a.chunk_scales[2 * (size_t)a.nchunks];
        s.inv_sg = a.chunk_scales[2 * (size_t)a.nchunks + 1];
    }
    return s;
}
// operand scales of chunk c (PL == 3: no scaling)
// (Round 5 tried issuing the LOAD of a chunk's scales a whole chunk before their first use -- read at the top of a chunk and used by
// its first staging piece, the wave waits there for a memory round trip -- and the wide kernel got SLOWER: 8.44 against 7.98 ms on
// one box, profiles/r05_kbench_wgrad_zeropad.log; the narrow one did not move.  Left as it was.)
template <int PL> __device__ __forceinline__ void wgrad_chunk_scale(const WgradArgs &a, int c, float &sa, float &sg)
{
    if constexpr (PL == 2) {
        const float2 v = *reinterpret_cast<const float2 *>(a.chunk_scales + 2 * (size_t)c);
        sa = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v.x)));
        sg = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v.y)));
    } else {
        sa = 1.f; sg = 1.f;
    }
}
struct ChunkScaleArgs {
    const float *in_amax, *g_amax;
    float *out;                      // [nchunks][2], then 1 / sA, 1 / sG of the two tensors
    long long NQ;
    int nchunks, P, g_shift, nrows;
    Magic divP;
};
__device__ __forceinline__ int pow2_exponent(float p) { return (int)(__float_as_uint(p) >> 23) - 127; }
__global__ __launch_bounds__(256) void wgrad_chunk_scales_kernel(ChunkScaleArgs a)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    const float sA = pow2_scale_for(mmlf_amax_tensor_max(a.in_amax)), sG = pow2_scale_for(mmlf_amax_tensor_max(a.g_amax));
    if (c == 0) {                                   // the tensors' scales (inverted) for the weight-gradient kernel
        a.out[2 * (size_t)a.nchunks] = 1.f / sA;
        a.out[2 * (size_t)a.nchunks + 1] = 1.f / sG;
    }
    if (c >= a.nchunks) return;
    const long long q0 = (long long)c * WG_KQ;
    int x = 0;
    if (q0 < a.NQ) {
        // activations: the chunk stages in[q0 .. q0 + 32 + P] (its positions' four taps); gradients: g[q + g_shift].
        // EVERY staged element must stay inside the f16 range, also those that only meet zero gradients (an
        // overflow would put inf * 0 into the sum), so all rows the staging touches count.
        const long long ql = q0 + WG_KQ - 1;
        const unsigned r0 = fastdiv((unsigned)q0, a.divP);
        unsigned r1 = fastdiv((unsigned)(ql + a.P + 1), a.divP);
        if (r1 >= (unsigned)a.nrows) r1 = a.nrows - 1;
        float ma = 0.f, mg = 0.f;
        for (unsigned r = r0; r <= r1; ++r) ma = fmaxf(ma, a.in_amax[MMLF_AMAX_HEAD + r]);
        const unsigned g0 = fastdiv((unsigned)(q0 + a.g_shift), a.divP);
        unsigned g1 = fastdiv((unsigned)(ql + a.g_shift), a.divP);
        if (g1 >= (unsigned)a.nrows) g1 = a.nrows - 1;
        for (unsigned r = g0; r <= g1; ++r) mg = fmaxf(mg, a.g_amax[MMLF_AMAX_HEAD + r]);
        // headroom (binades) of the chunk's operands under the global scales; an all-zero operand takes any scale
        const int u = ma > 0.f ? pow2_exponent(pow2_scale_for(ma)) - pow2_exponent(sA) : 60;
        const int v = mg > 0.f ? pow2_exponent(pow2_scale_for(mg)) - pow2_exponent(sG) : 60;
        const int uu = u < 0 ? 0 : u, vv = v < 0 ? 0 : v;        // (row maxima never exceed the tensor's)
        x = (uu - vv) >> 1;                                        // floor
        x = x > 15 ? 15 : (x < -24 ? -24 : x);
    }
    a.out[2 * (size_t)c] = sA * exp2f((float)x);
    a.out[2 * (size_t)c + 1] = sG * exp2f((float)-x);
}

// ---------------------------------------------------------------------------------------------
// weight gradient on v_mfma_f32_16x16x32_bf16 (K = the chunk's 32 positions).  A workgroup owns a slice
// of 16*MB input channels (MFMA rows, the ones row included) x 16*NB output channels and a split of the
// positions; wave t = tap t accumulates MB x NB tiles.
//  <5,5>: the 70-channel stream layers in ONE slice, 80 x 80 (three 32-row slices x 96 columns would
//         be 1.85x the useful MFMA work), gradient tile staged and split once per chunk;
//  <2,18>: 32-channel slices x 288 columns for the 280-wide layers.
// LDS rows are padded to an odd multiple of 32 B: the 8 position rows one half-wave touches in a
// transposed read then start on 8 distinct multiples of 8 banks (conflict-free).  Lane group q4 takes
// positions {4q4..4q4+3, 16+4q4..}: the same k permutation for both operands, which a dot product
// does not see.
// ---------------------------------------------------------------------------------------------
template <int MB, int NB, int PL>
__global__ __launch_bounds__(256, 2) void wgrad4tap_x6n_kernel(WgradArgs a)
{
    constexpr int ROWA = 32 * (MB | 1), ROWG = 32 * (NB | 1);   // bytes per position row
    constexpr int A_PLANE = 34 * ROWA;                          // per (seg, plane)
    constexpr int A_BYTES = 2 * PL * A_PLANE;
    constexpr int NTERM = PL == 3 ? 6 : 3;
    const WgradScales sc = wgrad_scales<PL>(a);
    constexpr int G_PLANE = WG_KQ * ROWG;
    constexpr int FA = 4 * MB, FG = 4 * NB;                     // float4 per staged row
    constexpr int NA = (66 * FA + 255) / 256, NG = (WG_KQ * FG + 255) / 256;
    constexpr bool HOLD_G = NB <= 5;    // few columns: keep all gradient fragments, stream the activations
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *As = smem;
    char *Gs = smem + A_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63, t = tid >> 6;
    const int r16 = lane & 15, q4 = lane >> 4;
    int slice, split;
    if (!wgrad_block_map(blockIdx.x, a.nslice, a.nsplit, slice, split)) return;
    const int ci0 = slice * 16 * MB;
    int c_begin = split * a.chunks_per_split;
    int c_end = c_begin + a.chunks_per_split;
    if (c_end > a.nchunks) c_end = a.nchunks;

    f32x4 acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mb][nb][r] = 0.f;

    // Staging items and channels past the tile are CLAMPED (round 5) -- surplus threads load and store the last
    // item again, padding channels are copies of the tensor's last four -- instead of predicated and zero-filled: no divergent
    // branch per piece; the padding only feeds accumulator rows / columns the reduction never reads (as in the wide kernel).
    float4 ra[NA], rg[NG];
#define WN_GLOAD(c)                                                                                         \
    do {                                                                                                    \
        const long long Qc = (long long)(c) * WG_KQ;                                                        \
        _Pragma("unroll") for (int j = 0; j < NA; ++j) {                                                    \
            const int idx = min(tid + 256 * j, 66 * FA - 1);                                                \
            const int row = idx / FA, f = idx - row * FA;                                                   \
            const int seg = row >= 33, pix = row - 33 * seg;                                                \
            const int ch = min(ci0 + 4 * f, a.cs_in - 4);                                                   \
            MMLF_OOB(OOB_WG_IN, ((Qc + seg * a.P + pix) * a.cs_in + ch + 4) * 4ll > a.in_bytes);            \
            ra[j] = *reinterpret_cast<const float4 *>(a.in + (size_t)(Qc + seg * a.P + pix) * a.cs_in + ch); \
        }                                                                                                   \
        _Pragma("unroll") for (int j = 0; j < NG; ++j) {                                                    \
            const int idx = min(tid + 256 * j, WG_KQ * FG - 1);                                             \
            const int row = idx / FG, f = idx - row * FG;                                                   \
            const int gc = min(4 * f, a.g_cols - 4);                                                        \
            MMLF_OOB(OOB_WG_G, ((Qc + a.g_shift + row) * a.cs_g + gc + 4) * 4ll > a.g_bytes);               \
            rg[j] = *reinterpret_cast<const float4 *>(a.g + (size_t)(Qc + a.g_shift + row) * a.cs_g + gc);  \
        }                                                                                                   \
    } while (0)
#define WN_LSTORE()                                                                                         \
    do {                                                                                                    \
        _Pragma("unroll") for (int j = 0; j < NA; ++j) {                                                    \
            const int idx = min(tid + 256 * j, 66 * FA - 1);                                                \
            const int row = idx / FA, f = idx - row * FA;                                                   \
            const int seg = row >= 33, pix = row - 33 * seg;                                                \
            float4 v = ra[j];         /* ones row (bias gradient): patched here, not at load time, */       \
            const int ch = ci0 + 4 * f; /* so that the global loads issue back to back               */     \
            if (ch == a.cin) v.x = sc.inv_sa;   /* = 1 after scaling */                                     \
            if (ch + 1 == a.cin) v.y = sc.inv_sa;                                                           \
            if (ch + 2 == a.cin) v.z = sc.inv_sa;                                                           \
            if (ch + 3 == a.cin) v.w = sc.inv_sa;                                                           \
            split_store4_pl<PL>(v, st_sa, As + seg * PL * A_PLANE + pix * ROWA + 8 * f, A_PLANE);           \
        }                                                                                                   \
        _Pragma("unroll") for (int j = 0; j < NG; ++j) {                                                    \
            const int idx = min(tid + 256 * j, WG_KQ * FG - 1);                                             \
            const int row = idx / FG, f = idx - row * FG;                                                   \
            split_store4_pl<PL>(rg[j], st_sg, Gs + row * ROWG + 8 * f, G_PLANE);                            \
        }                                                                                                   \
    } while (0)
    // transposed-read geometry: lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3
    const int tq = (lane & 15) >> 2, tp = lane & 3;
    const char *a_lane = As + (t >> 1) * PL * A_PLANE + ((t & 1) + 4 * q4 + tq) * ROWA + 8 * tp;
    const char *g_lane = Gs + (4 * q4 + tq) * ROWG + 8 * tp;

    float st_sa = 1.f, st_sg = 1.f;          // operand scales of the chunk being staged
    if (c_begin < c_end) {
        WN_GLOAD(c_begin);
        for (int c = c_begin; c < c_end; ++c) {
            wgrad_chunk_scale<PL>(a, c, st_sa, st_sg);
            WN_LSTORE();
            __syncthreads();
            if (c + 1 < c_end) WN_GLOAD(c + 1);
            if constexpr (HOLD_G) {
                bf16x8 gf[NB][PL];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int pl = 0; pl < PL; ++pl) gf[nb][pl] = tr_frag(g_lane + pl * G_PLANE + 32 * nb, 4 * ROWG);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    bf16x8 af[PL];
#pragma unroll
                    for (int pl = 0; pl < PL; ++pl) af[pl] = tr_frag(a_lane + pl * A_PLANE + 32 * mb, 4 * ROWA);
#pragma unroll
                    for (int term = 0; term < NTERM; ++term)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[mb][nb] = mfma16_pl<PL>(af[term_a<PL>(term)], gf[nb][term_b<PL>(term)], acc[mb][nb]);
                }
            } else {
                bf16x8 af[MB][PL];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int pl = 0; pl < PL; ++pl) af[mb][pl] = tr_frag(a_lane + pl * A_PLANE + 32 * mb, 4 * ROWA);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    bf16x8 gf[PL];
#pragma unroll
                    for (int pl = 0; pl < PL; ++pl) gf[pl] = tr_frag(g_lane + pl * G_PLANE + 32 * nb, 4 * ROWG);
#pragma unroll
                    for (int term = 0; term < NTERM; ++term)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb)
                            acc[mb][nb] = mfma16_pl<PL>(af[mb][term_a<PL>(term)], gf[term_b<PL>(term)], acc[mb][nb]);
                }
            }
            __syncthreads();
        }
    }
#undef WN_GLOAD
#undef WN_LSTORE
    constexpr int NP = 16 * NB;
    const int CIP = a.nslice * 16 * MB;
    float *pp = a.part + ((size_t)(split * 4 + t) * CIP + ci0) * NP;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mb + 4 * q4 + r;      // the ones row (bias gradient) carries no input scale
                const float un = (ci0 + row == a.cin ? 1.f : sc.inv_sa) * sc.inv_sg;
                MMLF_OOB(OOB_WG_PART, (long long)(pp - a.part) + (long long)row * NP + 16 * nb + r16 >= a.part_floats);
                pp[(size_t)row * NP + 16 * nb + r16] = acc[mb][nb][r] * un;
            }
}

// ---------------------------------------------------------------------------------------------
// wide-layer weight gradient (128 < Cout <= 288, and the first 288 columns of a wider layer): 512 threads = 8 waves, wave w = (tap w&3, column half w>>2).
// A workgroup owns a slice of 16*MB input channels x all 288 columns and a split of the positions; the
// LDS image is DOUBLE-buffered: while chunk c is multiplied, the registers holding chunk c+1 (loaded
// from global memory one iteration earlier) are split and stored into the other buffer between the
// MFMAs, and chunk c+2's loads are issued.  One barrier per chunk, no phase in which the matrix
// cores wait for staging.  155.9 KB of LDS: one workgroup per CU.
// ---------------------------------------------------------------------------------------------
template <int MB, int NBH, int PL>
__global__ __launch_bounds__(512, 2) void wgrad4tap_x6w_kernel(WgradArgs a)
{
    constexpr int NB = 2 * NBH;
    const WgradScales sc = wgrad_scales<PL>(a);
    constexpr int ROWA = 32 * (MB | 1), ROWG = 32 * (NB | 1);
    constexpr int A_PLANE = 34 * ROWA;
    constexpr int A_BYTES = 2 * PL * A_PLANE;
    constexpr int G_PLANE = WG_KQ * ROWG;
    constexpr int BUF_BYTES = A_BYTES + PL * G_PLANE;
    constexpr int FA = 4 * MB, FG = 4 * NB;
    constexpr int NA = (66 * FA + 511) / 512, NG = (WG_KQ * FG + 511) / 512;
    static_assert(2 * BUF_BYTES <= 160 * 1024, "LDS");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = w & 3, h = w >> 2;
    const int q4 = lane >> 4;

    float4 ra[NA], rg[NG];
    // Input channels past cs_in and gradient columns past cs_g (the slices' and the 288 columns' padding) are staged as COPIES of
    // the tensor's last four channels (the clamped load) instead of zeros: they only feed accumulator rows / columns that
    // wgrad_reduce_kernel never reads (ci > Cin, co >= Cout), the copies are in-range values (no f16 overflow), and the ones row
    // (ci == Cin) is patched in WW_STORE_A either way.  Four selects per staging piece less (round 5; the zero-filling form:
    // profiles/r05_kbench_wgrad_zeropad.log).

    // staging items are clamped to the last one instead of predicated: surplus threads load and store that
    // item again (same value), which keeps the loop free of branches.  Also of SCALAR ones: round 5 let the waves whose
    // items of a piece are all surplus (3 of 8 on the second activation piece, 4 of 8 on the fifth gradient piece at <3, 9>)
    // skip the piece -- less work, no 64 lanes storing to one LDS address -- and the launch took 8.53 ms instead of 8.17
    // (profiles/r05_kbench_wgrad_surplus.log): a branch per column block ends the basic block the MFMAs and the staging
    // instructions are interleaved in.  Nor do the surplus lanes' stores to ONE address cost anything: giving every such lane
    // an LDS slot of its own measured 8.04 ms against 8.02 (profiles/r05_kbench_wgrad_surplus.log) -- equal addresses merge.
    // Per-lane parts of every staging address, formed ONCE: the byte offset of a piece's item from its chunk's first position
    // (32 bits: the load is `global_load_dwordx4 v, v_offset, s[base]`, no vector arithmetic per load) and its byte offset
    // inside an LDS buffer.  Round 5: with the addresses recomputed from 64-bit terms in the loop and the padding channels
    // zero-filled by selects, a chunk had 136 vector instructions per wave next to its 81 MFMAs; the vector-issue port is what
    // this kernel runs out of (each one removed is ~0.01 ms per launch: profiles/r05_kbench_wgrad_zeropad.log).
    // (of these, the gradient's and the LDS offsets belong to the lane alone and are formed once per workgroup; the activation
    // offsets carry the item's input-channel slice and are formed once per item, below)
    unsigned ga_off[NA], gg_off[NG];
    int la_off[NA], lg_off[NG], a_ch[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int idx = min(tid + 512 * j, 66 * FA - 1);
        const int row = idx / FA, f = idx - row * FA;
        const int seg = row >= 33, pix = row - 33 * seg;
        la_off[j] = seg * PL * A_PLANE + pix * ROWA + 8 * f;
    }
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int idx = min(tid + 512 * j, WG_KQ * FG - 1);
        const int row = idx / FG, f = idx - row * FG;
        gg_off[j] = (unsigned)((a.g_shift + row) * a.cs_g + min(4 * f, a.g_cols - 4)) * 4u;
        lg_off[j] = A_BYTES + row * ROWG + 8 * f;
    }
    const char *const in_b = reinterpret_cast<const char *>(a.in), *const g_b = reinterpret_cast<const char *>(a.g);
#define WW_GLOAD_A(j, c)                                                                                    \
    do {                                                                                                    \
        const long long cb_ = (long long)(c) * WG_KQ * a.cs_in * 4;      /* wave-uniform */                   \
        MMLF_OOB(OOB_WG_IN, cb_ + ga_off[j] + 16 > a.in_bytes);                                             \
        /* buffer load on a per-chunk descriptor: base and what is left of the tensor in scalar registers, the lane's */ \
        /* 32-bit offset as is -- no vector address arithmetic, and the address unit range-checks the access          */ \
        const __amdgpu_buffer_rsrc_t rs_ = __builtin_amdgcn_make_buffer_rsrc(                               \
            const_cast<char *>(in_b + cb_), 0, mmlf_records_left(a.in_bytes, cb_), MMLF_BUF_FLAGS);         \
        ra[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs_, ga_off[j], 0, 0));    \
    } while (0)
#define WW_GLOAD_G(j, c)                                                                                    \
    do {                                                                                                    \
        const long long cb_ = (long long)(c) * WG_KQ * a.cs_g * 4;                                          \
        MMLF_OOB(OOB_WG_G, cb_ + gg_off[j] + 16 > a.g_bytes);                                               \
        const __amdgpu_buffer_rsrc_t rs_ = __builtin_amdgcn_make_buffer_rsrc(                               \
            const_cast<char *>(g_b + cb_), 0, mmlf_records_left(a.g_bytes, cb_), MMLF_BUF_FLAGS);           \
        rg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs_, gg_off[j], 0, 0));    \
    } while (0)
#define WW_GLOAD(c)                                                                                         \
    do {                                                                                                    \
        _Pragma("unroll") for (int j = 0; j < NA; ++j) WW_GLOAD_A(j, c);                                    \
        _Pragma("unroll") for (int j = 0; j < NG; ++j) WW_GLOAD_G(j, c);                                    \
    } while (0)
#define WW_STORE_A(j, dst)                                                                                  \
    do {                                                                                                    \
        float4 v = ra[j];                 /* ones row -> bias gradient */                                   \
        const int ch = a_ch[j];                                                                             \
        v.x = ch == a.cin ? sc.inv_sa : v.x;   /* = 1 after scaling */                                      \
        v.y = ch + 1 == a.cin ? sc.inv_sa : v.y;                                                            \
        v.z = ch + 2 == a.cin ? sc.inv_sa : v.z;                                                            \
        v.w = ch + 3 == a.cin ? sc.inv_sa : v.w;                                                            \
        split_store4_pl<PL>(v, st_sa, (dst) + la_off[j], A_PLANE);                                          \
    } while (0)
#define WW_STORE_G(j, dst) split_store4_pl<PL>(rg[j], st_sg, (dst) + lg_off[j], G_PLANE)

    const int tq = (lane & 15) >> 2, tp = lane & 3;
    int a_off = (t >> 1) * PL * A_PLANE + ((t & 1) + 4 * q4 + tq) * ROWA + 8 * tp;
    int g_off = A_BYTES + (4 * q4 + tq) * ROWG + 8 * tp + 32 * NBH * h;

    // PERSISTENT over the (slice, split) items of the launch: workgroup blockIdx.x runs the blocks b = blockIdx.x,
    // + gridDim.x, ... of the one-shot launch, each exactly as that block ran it -- accumulators zeroed per item, its own
    // partial sums written in its own epilogue -- so the partial sums and the gradient are the one-shot launch's bit for bit.
    // With gridDim.x = items (MMLF_WGRAD_PERSIST=0, and every launch of no more items than CUs) it IS the one-shot launch.
    // b is wave-uniform: the loop state lives in scalar registers.  (The item's body keeps the indentation it had as the
    // whole kernel.)
    for (int b = blockIdx.x; b < a.items; b += gridDim.x) {
    int slice, split;
    if (!wgrad_block_map(b, a.nslice, a.nsplit, slice, split)) continue;      // (workgroup-uniform)
    const int ci0 = slice * 16 * MB;
    const int c_begin = split * a.chunks_per_split;
    int c_end = c_begin + a.chunks_per_split;
    if (c_end > a.nchunks) c_end = a.nchunks;

    f32x4 acc[MB][NBH];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mb][nb][r] = 0.f;
    // (the thread index and the lane's staging / fragment offsets are made opaque per item, here and at the epilogue: what
    // depends on the lane alone would otherwise be hoisted out of the item loop and held in registers across the chunk loop
    // -- 254 of them instead of 226, past the 232 the BatchNorm pairing leaves this kernel; EXPERIMENTS section 8, constraint (i))
#pragma unroll
    for (int j = 0; j < NA; ++j) asm volatile("" : "+v"(la_off[j]));
#pragma unroll
    for (int j = 0; j < NG; ++j) asm volatile("" : "+v"(lg_off[j]), "+v"(gg_off[j]));
    asm volatile("" : "+v"(a_off), "+v"(g_off));
    int tid_i;               // = tid, rebuilt from the lane count and the scalar wave index: tid itself need not stay live
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(tid_i));
    tid_i += 64 * w;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int idx = min(tid_i + 512 * j, 66 * FA - 1);
        const int row = idx / FA, f = idx - row * FA;
        const int seg = row >= 33, pix = row - 33 * seg;
        a_ch[j] = ci0 + 4 * f;
        ga_off[j] = (unsigned)((seg * a.P + pix) * a.cs_in + min(ci0 + 4 * f, a.cs_in - 4)) * 4u;
    }

    float st_sa = 1.f, st_sg = 1.f;          // operand scales of the chunk being staged
    if (c_begin < c_end) {
        WW_GLOAD(c_begin);
        __syncthreads();        // the previous item's last chunk may still be being read from the buffers staged into next
        wgrad_chunk_scale<PL>(a, c_begin, st_sa, st_sg);
#pragma unroll
        for (int j = 0; j < NA; ++j) WW_STORE_A(j, smem);
#pragma unroll
        for (int j = 0; j < NG; ++j) WW_STORE_G(j, smem);
        if (c_begin + 1 < c_end) WW_GLOAD(c_begin + 1);
        __syncthreads();
        int buf = 0;
        // EARLY (as in the conv kernel): the chunk's barrier stands two column blocks before its end -- every staging
        // store of the chunk is out by then (one piece per column block, NA + NG <= NBH - 2) and every fragment read
        // requested -- and behind it the wave asks for the NEXT chunk's first gradient fragments (the rotating slots run
        // on, NBH % 3 == 0) and its first two activation row blocks, which arrive under the last 2 x 3 x MB MFMAs.
        constexpr bool EARLY = PL == 2 && NBH % 3 == 0 && NA + NG <= NBH - 2 && MB >= 2;
        bf16x8 af[MB][PL], gfr[3][PL], afp[2][PL];
        if constexpr (EARLY) {
            const char *cur0 = smem;
#pragma unroll
            for (int g0 = 0; g0 < 2; ++g0)
#pragma unroll
                for (int pl = 0; pl < PL; ++pl) gfr[g0][pl] = tr_frag(cur0 + g_off + pl * G_PLANE + 32 * g0, 4 * ROWG);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int pl = 0; pl < PL; ++pl) af[mb][pl] = tr_frag(cur0 + a_off + pl * A_PLANE + 32 * mb, 4 * ROWA);
        }
        // One chunk: gradient fragments are read two column blocks ahead (three register sets); with STAGE the
        // registers holding chunk c+1 are split and stored into the other buffer, one piece per column
        // block, branch-free so that the stores interleave with the MFMAs -- and the register a piece leaves is
        // loaded with the same piece of chunk c+2 right away: a whole chunk between a global load and its use
        // (loaded in bulk at the end of the chunk, every load was waited for at the next chunk's first column blocks).
#define WW_TERM(gf, pa, pb)                                                                                  \
    _Pragma("unroll") for (int mb = 0; mb < MB; ++mb)                                                        \
        acc[mb][nb] = mfma16_pl<PL>(af[mb][pa], gf[pb], acc[mb][nb])
#define WW_CHUNK(STAGE, RELOAD)                                                                              \
    do {                                                                                                     \
        const char *cur = smem + buf * BUF_BYTES;                                                            \
        char *nxt = smem + (buf ^ 1) * BUF_BYTES;                                                            \
        if (!EARLY) {                                                                                        \
            _Pragma("unroll") for (int g0 = 0; g0 < 2; ++g0)                                                 \
                _Pragma("unroll") for (int pl = 0; pl < PL; ++pl)                                             \
                    gfr[g0][pl] = tr_frag(cur + g_off + pl * G_PLANE + 32 * g0, 4 * ROWG);                   \
        }                                                                                                    \
        _Pragma("unroll") for (int mb = EARLY ? 2 : 0; mb < MB; ++mb)                                        \
            _Pragma("unroll") for (int pl = 0; pl < PL; ++pl)                                                 \
                af[mb][pl] = tr_frag(cur + a_off + pl * A_PLANE + 32 * mb, 4 * ROWA);                        \
        _Pragma("unroll") for (int nb = 0; nb < NBH; ++nb) {                                                 \
            if (EARLY && (STAGE) && nb == NBH - 2) {                                                         \
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   /* my staging stores and fragment reads */ \
                __syncthreads();                                                                             \
                _Pragma("unroll") for (int mb = 0; mb < 2; ++mb)                                             \
                    _Pragma("unroll") for (int pl = 0; pl < PL; ++pl)                                         \
                        afp[mb][pl] = tr_frag(nxt + a_off + pl * A_PLANE + 32 * mb, 4 * ROWA);               \
            }                                                                                                \
            if (nb + 2 < NBH) {                                                                              \
                _Pragma("unroll") for (int pl = 0; pl < PL; ++pl)                                             \
                    gfr[(nb + 2) % 3][pl] = tr_frag(cur + g_off + pl * G_PLANE + 32 * (nb + 2), 4 * ROWG);   \
            } else if (EARLY && (STAGE)) {                                                                   \
                _Pragma("unroll") for (int pl = 0; pl < PL; ++pl)                                             \
                    gfr[(nb + 2) % 3][pl] = tr_frag(nxt + g_off + pl * G_PLANE + 32 * (nb + 2 - NBH), 4 * ROWG); \
            }                                                                                                \
            if (STAGE) {                                                                                     \
                if (nb < NA) {                                                                               \
                    WW_STORE_A(nb < NA ? nb : 0, nxt);                                                       \
                    if (RELOAD) WW_GLOAD_A(nb < NA ? nb : 0, c + 2);                                         \
                } else if (nb - NA < NG) {                                                                   \
                    WW_STORE_G(nb - NA < NG ? nb - NA : 0, nxt);                                             \
                    if (RELOAD) WW_GLOAD_G(nb - NA < NG ? nb - NA : 0, c + 2);                               \
                }                                                                                            \
            }                                                                                                \
            _Pragma("unroll") for (int term = 0; term < (PL == 3 ? 6 : 3); ++term)                           \
                WW_TERM(gfr[nb % 3], term_a<PL>(term), term_b<PL>(term));                                    \
        }                                                                                                    \
        if (EARLY && (STAGE)) {                                                                              \
            _Pragma("unroll") for (int mb = 0; mb < 2; ++mb)                                                 \
                _Pragma("unroll") for (int pl = 0; pl < PL; ++pl) af[mb][pl] = afp[mb][pl];                   \
        }                                                                                                    \
    } while (0)
        static_assert(NA + NG <= NBH, "one staging piece per column block");
        for (int c = c_begin; c + 1 < c_end; ++c) {
            wgrad_chunk_scale<PL>(a, c + 1, st_sa, st_sg);
            // (the scalar branch around each of the seven reloads stays: with unconditional loads -- the split's last chunk loaded
            // once more, never staged -- the chunk is one basic block and the compiler's own order of it is 1.7 % SLOWER, 8.17
            // against 8.04 ms, profiles/r05_kbench_wgrad_zeropad.log; the branches are what pins the interleaving written here)
            const bool reload = c + 2 < c_end;
            WW_CHUNK(true, reload);
            if constexpr (!EARLY) __syncthreads();
            buf ^= 1;
        }
        {
            const int c = c_end - 1;
            (void)c;
            WW_CHUNK(false, false);          // last chunk: nothing left to stage
        }
    }
    // (an item whose split holds no chunks writes its zero partial sums like any other: the reduction reads every split)
    constexpr int NP = 16 * NB;
    const int CIP = a.nslice * 16 * MB;
    float *pp = a.part + ((size_t)(split * 4 + t) * CIP + ci0) * NP + 16 * NBH * h;
    int tid_e;               // = lane, as above
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(tid_e));
    const int r16e = tid_e & 15, q4e = (tid_e & 63) >> 4;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mb + 4 * q4e + r;     // the ones row (bias gradient) carries no input scale
                const float un = (ci0 + row == a.cin ? 1.f : sc.inv_sa) * sc.inv_sg;
                MMLF_OOB(OOB_WG_PART, (long long)(pp - a.part) + (long long)row * NP + 16 * nb + r16e >= a.part_floats);
                pp[(size_t)row * NP + 16 * nb + r16e] = acc[mb][nb][r] * un;
            }
    }
#undef WW_CHUNK
#undef WW_TERM
#undef WW_GLOAD
#undef WW_GLOAD_A
#undef WW_GLOAD_G
#undef WW_STORE_A
#undef WW_STORE_G
}

// sum the position splits and scatter to the OIHW master gradient (+ bias gradient).  One thread per output element:
// at 64 patches per GPU this launch is latency-bound and wants every CU full of waves -- a float4-per-thread form with a
// quarter of the threads ran 2.5x longer (130 vs 50 us at 280 -> 280, measured in the step).
// NTAP = 4 (2x2 filters, partials [nsplit][4][CIP][NP]) or 9 (3x3 filters, wgrad9tap_kernel's [nsplit][9][CIP][NP]).
template <int NTAP>
__global__ void wgrad_reduce_kernel(const float *__restrict__ part, float *__restrict__ gw, float *__restrict__ gb,
                                     int Cin, int Cout, int CIP, int NP, int nsplit, int variant, int accumulate)
{
    const int total = NTAP * (Cin + 1) * Cout;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int co = idx % Cout;
    int r = idx / Cout;
    const int ci = r % (Cin + 1);
    const int t = r / (Cin + 1);
    if (ci == Cin && (t != 0 || gb == nullptr)) return;
    const float *pp = part + ((size_t)t * CIP + ci) * NP + co;
    const size_t stride = (size_t)NTAP * CIP * NP;
    constexpr int U = 16;
    double acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.0;
    int sp = 0;
    for (; sp + U <= nsplit; sp += U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = pp[(size_t)(sp + u) * stride];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] += v[u];
    }
    for (; sp < nsplit; ++sp) acc[0] += pp[(size_t)sp * stride];
#pragma unroll
    for (int h = U / 2; h > 0; h >>= 1)
#pragma unroll
        for (int u = 0; u < h; ++u) acc[u] += acc[u + h];
    const double s = acc[0];
    if (ci == Cin) {
        gb[co] = accumulate ? gb[co] + (float)s : (float)s;
    } else {
        const size_t o = ((size_t)co * Cin + ci) * NTAP + master_tap<(NTAP == 4 ? 2 : 3)>(t, variant);
        gw[o] = accumulate ? gw[o] + (float)s : (float)s;
    }
}

// the same for MANY partials of few elements (the thin weight gradient: 4096 wave-private partials of 4 x 281 x 2 sums):
// one WAVE per output element, lanes stride over the partials, fixed-order butterfly at the end (one thread per element
// walked 4096 partials 9 KB apart by itself: 1.95 ms per step for 2 248 sums)
__global__ __launch_bounds__(256) void wgrad_reduce_wave_kernel(const float *__restrict__ part, float *__restrict__ gw,
                                                                float *__restrict__ gb, int Cin, int Cout, int CIP, int NP,
                                                                int nsplit, int variant, int accumulate)
{
    const int total = 4 * (Cin + 1) * Cout;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (idx >= total) return;
    const int co = idx % Cout;
    int r = idx / Cout;
    const int ci = r % (Cin + 1);
    const int t = r / (Cin + 1);
    if (ci == Cin && (t != 0 || gb == nullptr)) return;
    const float *pp = part + ((size_t)t * CIP + ci) * NP + co;
    const size_t stride = (size_t)4 * CIP * NP;
    double acc = 0.0;
    for (int sp = lane; sp < nsplit; sp += 64) acc += pp[(size_t)sp * stride];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane) return;
    if (ci == Cin) {
        gb[co] = accumulate ? gb[co] + (float)acc : (float)acc;
    } else {
        const size_t o = ((size_t)co * Cin + ci) * 4 + master_tap<2>(t, variant);
        gw[o] = accumulate ? gw[o] + (float)acc : (float)acc;
    }
}

// ---------------------------------------------------------------------------------------------
// The bias gradient WITHOUT a weight gradient (gw == NULL at an entry point: the layer's filter is frozen, its bias trains):
// gb[c] (+)= sum_q g[q + g_shift][c] over the padded grid.  g is zero outside its extent (the entry points' contract), so no
// mask is read: one pass over g and nothing else, 4 NQ cs_g bytes, HBM-bound.  A row kernel (row_walk.h): a block takes
// grid rows blockIdx.x, + gridDim.x, ...; a thread keeps ONE group of four channels (reduce_walk) and meets positions
// pl, pl + ppi, ... < P of each row with a 16-byte non-temporal load, so every read is at the float index
//     ((row * P + x + g_shift) * cs_g + 4 * cg + k,   row < B * R,  x < P,  4 * cg + k < cs_g  (4 cvn <= cs_g: cs_g % 4 == 0)
// below (NQ + g_shift) * cs_g, inside what mmlf_audit_wgrad_h2 / mmlf_audit_wgrad3x3 report for g.  Sums in float64; a
// block's go to partial[blockIdx.x][C] in the entry point's workspace, and bias_grad_finish_kernel adds the blocks in a
// fixed order and rounds once.  No atomics: two launches give the same bits.
// ---------------------------------------------------------------------------------------------
constexpr int BIAS_GRAD_MAX_C = 512, BIAS_GRAD_MAX_BLOCKS = 1024;

__device__ __forceinline__ void bias_grad_load(const float *p, float *o, bool is_aligned)
{
    if (is_aligned) {                                   // streamed once: non-temporal, as bn_rows_kernel reads
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(p));
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = __builtin_nontemporal_load(p + k);
    }
}

__global__ __launch_bounds__(256) void bias_grad_rows_kernel(const float *__restrict__ g, int cs_g, int C, int g_shift, int P,
                                                             int nrows, double *__restrict__ partial)
{
    int cvn, ppi;                               // channel groups that hold real channels, positions per iteration
    reduce_walk(C, 4, cvn, ppi);
    const int tid = threadIdx.x;
    const int pl = tid / cvn, cg = tid - pl * cvn;
    const bool active = pl < ppi;
    double s[4] = {0, 0, 0, 0};
    // every access of the launch is 16-byte aligned (cs_g % 4 == 0), or none is promised to be
    const bool aligned = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
        const float *rp = g + ((size_t)row * P + g_shift) * cs_g + 4 * cg;
        // two positions per iteration, both loads issued before either sum (the order of the sums stays x, x + ppi, ...)
        for (int x = pl; active && x < P; x += 2 * ppi) {
            float a[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            bias_grad_load(rp + (size_t)x * cs_g, a, aligned);
            if (x + ppi < P) bias_grad_load(rp + (size_t)(x + ppi) * cs_g, b, aligned);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += a[e];
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += b[e];
        }
    }
    __shared__ double red[ROW_THREADS][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) red[tid][e] = s[e];
    __syncthreads();
    if (tid < cvn) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double acc = 0;
            for (int p = 0; p < ppi; ++p) acc += red[p * cvn + tid][e];
            const int c = 4 * tid + e;
            if (c < C) partial[(size_t)blockIdx.x * C + c] = acc;
        }
    }
}

// second stage: one wave per channel, lanes stride over the blocks' partial sums, a fixed-order shuffle tree, then ONE rounding
// -- with the old value joined in float64 before it where the launch accumulates
__global__ __launch_bounds__(64) void bias_grad_finish_kernel(const double *__restrict__ partial, int nblocks, int C,
                                                              float *__restrict__ gb, int accumulate)
{
    const int c = blockIdx.x;
    double acc = 0;
    for (int blk = threadIdx.x; blk < nblocks; blk += 64) acc += partial[(size_t)blk * C + c];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x != 0) return;
    gb[c] = (float)(accumulate ? acc + (double)gb[c] : acc);
}

// The host side of every weight-gradient entry point called with gw == NULL (the entry point has validated its own
// arguments).  ws_floats: the partial-sum floats that entry point's workspace query promises; the block count follows from it.
static int bias_grad_only(const char *who, const float *g, int cs_g, int C, int g_shift, float *gb, int accumulate,
                          float *workspace, int64_t ws_floats, const Grid &gr, hipStream_t st)
{
    MMLF_CHECK_ARG(C >= 1 && C <= BIAS_GRAD_MAX_C && C <= cs_g && cs_g % 4 == 0, "%s: bias gradient alone: C=%d cs_g=%d", who, C, cs_g);
    MMLF_CHECK_ARG(gr.NQ + 2 * gr.P + 64 < (1ll << 31), "%s: batch x image too large", who);
    // float64 partials in a float workspace: start at the first 8-byte boundary (at most one float on)
    double *partial = reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(workspace) + 7) & ~(uintptr_t)7);
    const int64_t room = (ws_floats - 1) / 2 / C;                  // blocks whose C doubles fit
    MMLF_CHECK_ARG(room >= 1, "%s: bias gradient alone: the workspace holds %lld floats", who, (long long)ws_floats);
    const int nrows = gr.B * gr.R;
    int nblocks = nrows < BIAS_GRAD_MAX_BLOCKS ? nrows : BIAS_GRAD_MAX_BLOCKS;
    if (nblocks > room) nblocks = (int)room;
    hipLaunchKernelGGL(bias_grad_rows_kernel, dim3(nblocks), dim3(ROW_THREADS), 0, st, g, cs_g, C, g_shift, gr.P, nrows, partial);
    hipLaunchKernelGGL(bias_grad_finish_kernel, dim3(C), dim3(64), 0, st, partial, nblocks, C, gb, accumulate);
    return mmlf_launch_status(who);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static int wgrad_nsplit(int nslice)
{
    int n = 512 / nslice;       // two 256-thread blocks per CU on 256 CUs
    n = n / 8 * 8;
    if (n < 8) n = 8;
    return n;
}

// split-arithmetic kernel configuration for a layer: MB 16-row blocks of input channels (+ ones row) per
// slice, NB 16-column blocks of output channels, and the (slice x position-split) grid
struct Wgrad16Cfg { int mb, nb, nslice, nsplit; };
// nchunks: 32-position chunks of the launch, or -1 for the largest layout (workspace sizing)
static inline bool wgrad16_cfg(int Cin, int Cout, long long nchunks, Wgrad16Cfg *c)
{
    if (Cout <= 0 || Cout > 288) return false;
    c->nb = Cout <= 32 ? 2 : Cout <= 80 ? 5 : Cout <= 128 ? 8 : 18;
    if (c->nb == 18) {           // wgrad4tap_x6w_kernel: one 512-thread workgroup per CU, persistent over the items (wgrad_map.h)
        c->mb = 3;
        wgrad_wide_splits(Cin, nchunks, device_cus(), c->nslice, c->nsplit);
    } else {                     // wgrad4tap_x6n_kernel: two 256-thread workgroups per CU
        c->mb = (c->nb <= 5 && Cin + 1 > 32 && Cin + 1 <= 80) ? 5 : 2;
        // 128 columns (the 108-class DPP head): 48-row slices from 128 input channels on -- six slices of 281 rows instead of
        // nine, the gradient tile staged six times: 4.88 -> 4.47 ms at 280 -> 108 (96-row slices spill: 18.7 ms)
        if (c->nb == 8 && Cin + 1 >= 128) c->mb = 3;
        c->nslice = (Cin + 1 + 16 * c->mb - 1) / (16 * c->mb);
        c->nsplit = wgrad_nsplit(c->nslice);
    }
    return true;
}

// Column blocks of the gradient tensor (288 < Cout <= 512): the first 288 output channels, then the rest, each block a
// launch of its own on the kernel its width takes by wgrad16_cfg / pick_nt, followed by its own reduction into its rows of the
// OIHW master (co is the slowest index there: the blocks' rows do not interleave).  The launches run one after the other on
// one stream and share the partial-sum region, which is sized by the larger block.  (The convolutions' packed layouts
// have a block rule of their own, conv.hip wide_np: this kernel reads the unpacked gradient, so nothing ties the two.)
constexpr int WGRAD_MAX_COUT = 288, WGRAD_MAX_COUT_WIDE = 512;
static inline int wgrad_col_blocks(int Cout) { return Cout > WGRAD_MAX_COUT ? 2 : 1; }
static inline int wgrad_block_cout(int Cout, int b) { return b == 0 ? (Cout < WGRAD_MAX_COUT ? Cout : WGRAD_MAX_COUT) : Cout - WGRAD_MAX_COUT; }

// ---------------------------------------------------------------------------------------------
// The launch plan of a weight gradient: per column block the kernel that runs it, its grid and the layout of its partial
// sums -- computed HERE and nowhere else; the entry points launch and reduce by it, the workspace queries return its sizes
// and the bounds audits derive their ends from it.
// ---------------------------------------------------------------------------------------------
struct WgradBlock {
    int c0, cout;                 // output channels [c0, c0 + cout) of the layer
    int nt;                       // the exact-f32 kernel on nt 32-column tiles (pick_nt), or 0: ...
    Wgrad16Cfg cfg;               // ... the split-arithmetic kernel of this configuration
    int nslice, nsplit;           // the launch grid (wgrad_block_map)
    int CIP, NP;                  // rows and columns of the partial sums [nsplit][taps][CIP][NP] ...
    int64_t part_floats;          // ... and their floats
};
struct WgradPlan {
    int nblocks;
    WgradBlock blk[2];
    int64_t part_floats;          // partial sums of the largest block's launch
    // floats of the workspace region the blocks' partial sums share, behind which the f16 split's chunk scales lie: the
    // largest layout either kernel may choose for a block (so that one workspace serves every arithmetic path and batch)
    int64_t scales_off;
};
// the exact-f32 kernel of a ks x ks filter: 32-channel ci slices (+1: the ones row that yields the bias gradient),
// WgradF32Shape<ks>::BPS workgroups per slice
static bool wgrad_f32_block(int ks, int Cin, int c0, int cout, WgradBlock &k)
{
    k = {};
    k.c0 = c0; k.cout = cout; k.nt = pick_nt(cout);
    if (k.nt < 0) return false;
    const int ci_slices = (Cin + 1 + 31) / 32;
    k.nslice = (ks == 2 ? WgradF32Shape<2>::BPS : WgradF32Shape<3>::BPS) * ci_slices;
    k.nsplit = wgrad_nsplit(k.nslice);
    k.CIP = ci_slices * 32; k.NP = k.nt * 32;
    k.part_floats = (int64_t)k.nsplit * ks * ks * k.CIP * k.NP;
    return true;
}
static void wgrad_split_block(const Wgrad16Cfg &c, WgradBlock &k)
{
    k.nt = 0; k.cfg = c; k.nslice = c.nslice; k.nsplit = c.nsplit;
    k.CIP = c.nslice * 16 * c.mb; k.NP = 16 * c.nb;
    k.part_floats = (int64_t)k.nsplit * 4 * k.CIP * k.NP;
}
// 2x2.  planes: 0 = exact-f32 MFMA, 3 = bf16 split, 2 = f16 split; nchunks: 32-position chunks of the launch (< 0: none,
// the plan is read for scales_off alone)
static bool wgrad_plan(int planes, int Cin, int Cout, long long nchunks, WgradPlan &p)
{
    p = {};
    if (Cout > WGRAD_MAX_COUT_WIDE) return false;
    p.nblocks = wgrad_col_blocks(Cout);
    for (int b = 0, c0 = 0; b < p.nblocks; c0 += p.blk[b++].cout) {
        WgradBlock &k = p.blk[b];
        WgradBlock largest = {};
        Wgrad16Cfg c;
        if (!wgrad_f32_block(2, Cin, c0, wgrad_block_cout(Cout, b), k)) return false;
        int64_t sized = k.part_floats;
        if (wgrad16_cfg(Cin, k.cout, -1, &c)) {
            wgrad_split_block(c, largest);
            if (largest.part_floats > sized) sized = largest.part_floats;
        }
        sized = (sized + 3) / 4 * 4;
        if (sized > p.scales_off) p.scales_off = sized;
        if (planes && wgrad16_cfg(Cin, k.cout, nchunks, &c)) wgrad_split_block(c, k);
        if (k.part_floats > p.part_floats) p.part_floats = k.part_floats;
    }
    return true;
}

extern "C" int64_t mmlf_wgrad_workspace_floats(int Cin, int Cout, int B, int H, int W)
{
    WgradPlan p;
    if (!wgrad_plan(0, Cin, Cout, -1, p) || B <= 0 || H <= 0 || W <= 0) return -1;
    return p.scales_off + 2 * (make_grid(B, H, W).NQpad / WG_KQ) + 4;  // + the f16 split's per-chunk operand scales and the two tensor scales
}

template <int KS, int NT>
static int launch_wgrad_f32(const WgradArgs &a, hipStream_t st)
{
    using S = WgradF32Shape<KS>;
    const dim3 grid(wgrad_grid_blocks(a.nslice, a.nsplit)), block(64 * S::WAVES);
    if constexpr (KS == 2) hipLaunchKernelGGL(wgrad4tap_kernel<NT>, grid, block, S::lds_bytes(NT), st, a);
    else hipLaunchKernelGGL(wgrad9tap_kernel<NT>, grid, block, S::lds_bytes(NT), st, a);
    return mmlf_launch_status(KS == 2 ? "mmlf_conv2x2_wgrad" : "mmlf_conv3x3_wgrad");
}

template <int MB, int NB, int PL>
static int launch_wgrad16(const WgradArgs &a, hipStream_t st)
{
    constexpr size_t lds = 2 * PL * 34 * 32 * (MB | 1) + PL * WG_KQ * 32 * (NB | 1);
    static PerDeviceOnce attr_once;
    if (attr_once.run([] { return mmlf_allow_lds(reinterpret_cast<const void *>(wgrad4tap_x6n_kernel<MB, NB, PL>), lds, "mmlf_conv2x2_wgrad_split"); }))
        return 1;
    hipLaunchKernelGGL((wgrad4tap_x6n_kernel<MB, NB, PL>), dim3(wgrad_grid_blocks(a.nslice, a.nsplit)), dim3(256), lds, st, a);
    return mmlf_launch_status("mmlf_conv2x2_wgrad_split");
}

// MMLF_WGRAD_PERSIST=0 (read once per process): the wide kernel as one workgroup per item (wgrad_map.h wgrad_wide_grid)
static bool wgrad_persist()
{
    static const bool on = [] { const char *e = getenv("MMLF_WGRAD_PERSIST"); return !e || atoi(e) != 0; }();
    return on;
}

template <int PL>
static int launch_wgrad_wide(const WgradArgs &a, hipStream_t st)
{
    constexpr size_t lds = 2 * (2 * PL * 34 * 32 * (3 | 1) + PL * WG_KQ * 32 * (18 | 1));
    static PerDeviceOnce attr_once;
    if (attr_once.run([] { return mmlf_allow_lds(reinterpret_cast<const void *>(wgrad4tap_x6w_kernel<3, 9, PL>), lds, "mmlf_conv2x2_wgrad_split(wide)"); }))
        return 1;
    hipLaunchKernelGGL((wgrad4tap_x6w_kernel<3, 9, PL>), dim3(wgrad_wide_grid(a.items, device_cus(), wgrad_persist())), dim3(512), lds, st, a);
    return mmlf_launch_status("mmlf_conv2x2_wgrad_split");
}

template <int PL>
static int launch_wgrad_split(const Wgrad16Cfg &c, const WgradArgs &a, hipStream_t st)
{
    switch (10 * c.mb + c.nb) {
    case 22: return launch_wgrad16<2, 2, PL>(a, st);
    case 52: return launch_wgrad16<5, 2, PL>(a, st);
    case 25: return launch_wgrad16<2, 5, PL>(a, st);
    case 55: return launch_wgrad16<5, 5, PL>(a, st);
    case 28: return launch_wgrad16<2, 8, PL>(a, st);
    case 38: return launch_wgrad16<3, 8, PL>(a, st);
    default: return launch_wgrad_wide<PL>(a, st);
    }
}

// the launch arguments every weight-gradient entry point fills the same way; alloc = positions the tensors' allocation
// rule gives them, part_floats = floats of partial sums the workspace holds
static WgradArgs wgrad_args(const float *in, int cs_in, int Cin, const float *g, int cs_g, int g_shift, float *workspace,
                            const Grid &gr, long long alloc, long long part_floats)
{
    WgradArgs a = {};
    a.in = in; a.g = g; a.part = workspace; a.NQpad = gr.NQpad;
    a.cs_in = cs_in; a.cin = Cin; a.cs_g = a.g_cols = cs_g; a.g_shift = g_shift; a.P = gr.P;
    a.in_bytes = alloc * cs_in * 4; a.g_bytes = alloc * cs_g * 4;
    a.part_floats = part_floats;
    a.nchunks = (int)(gr.NQpad / WG_KQ);
    return a;
}
// the launch grid: nslice slice blocks (wgrad_block_map) x nsplit splits of the positions
static void wgrad_set_grid(WgradArgs &a, int nslice, int nsplit)
{
    a.nslice = nslice;
    a.nsplit = nsplit;
    a.chunks_per_split = (a.nchunks + nsplit - 1) / nsplit;
    a.items = (int)wgrad_grid_blocks(nslice, nsplit);
}

// sum the launch's partial sums [a.nsplit][KS*KS][CIP][NP] into the OIHW gradient
template <int KS>
static int wgrad_reduce(const WgradArgs &a, float *gw, float *gb, int Cin, int Cout, int CIP, int NP, int variant,
                        int accumulate, hipStream_t st)
{
    const int total = KS * KS * (Cin + 1) * Cout;
    hipLaunchKernelGGL(wgrad_reduce_kernel<KS * KS>, dim3((total + 255) / 256), dim3(256), 0, st, a.part, gw, gb, Cin, Cout,
                       CIP, NP, a.nsplit, variant, accumulate);
    return mmlf_launch_status(KS == 2 ? "mmlf_conv2x2_wgrad(reduce)" : "mmlf_conv3x3_wgrad(reduce)");
}

// one planned block of a KS x KS weight gradient: its launch (planes: the split kernel's, when the plan chose it), then the
// reduction of its partial sums into gw / gb (the block's rows of the OIHW master and of the bias gradient)
template <int KS>
static int wgrad_run_block(WgradArgs &a, const WgradBlock &k, int planes, float *gw, float *gb, int Cin, int variant,
                           int accumulate, hipStream_t st)
{
    wgrad_set_grid(a, k.nslice, k.nsplit);
    int rc = 1;
    if constexpr (KS == 2) {
        if (!k.nt) rc = planes == 3 ? launch_wgrad_split<3>(k.cfg, a, st) : launch_wgrad_split<2>(k.cfg, a, st);
    }
    if (k.nt) switch (k.nt) {
    case 1: rc = launch_wgrad_f32<KS, 1>(a, st); break;
    case 3: rc = launch_wgrad_f32<KS, 3>(a, st); break;
    case 4: rc = launch_wgrad_f32<KS, 4>(a, st); break;
    default: rc = launch_wgrad_f32<KS, 9>(a, st); break;
    }
    if (rc) return rc;
    return wgrad_reduce<KS>(a, gw, gb, Cin, k.cout, k.CIP, k.NP, variant, accumulate, st);
}

// planes: 0 = exact-f32 MFMA, 3 = bf16 split, 2 = f16 split (needs in_amax / g_amax)
static int wgrad_impl(const float *in, int cs_in, int Cin, const float *g, int cs_g, int Cout, int g_shift,
                      float *gw, float *gb, int variant, int accumulate, float *workspace, int B, int H, int W,
                      void *stream, int planes, const float *in_amax = nullptr, const float *g_amax = nullptr);

extern "C" int mmlf_conv2x2_wgrad(const float *in, int cs_in, int Cin, const float *g, int cs_g, int Cout,
                                  int g_shift, float *gw, float *gb, int variant, int accumulate,
                                  float *workspace, int B, int H, int W, void *stream)
{
    return wgrad_impl(in, cs_in, Cin, g, cs_g, Cout, g_shift, gw, gb, variant, accumulate, workspace, B, H, W,
                      stream, 0);
}

extern "C" int mmlf_conv2x2_wgrad_split(const float *in, int cs_in, int Cin, const float *g, int cs_g, int Cout,
                                        int g_shift, float *gw, float *gb, int variant, int accumulate,
                                        float *workspace, int B, int H, int W, void *stream)
{
    return wgrad_impl(in, cs_in, Cin, g, cs_g, Cout, g_shift, gw, gb, variant, accumulate, workspace, B, H, W,
                      stream, 3);
}

extern "C" int mmlf_conv2x2_wgrad_h2(const float *in, int cs_in, int Cin, const float *g, int cs_g, int Cout,
                                     int g_shift, float *gw, float *gb, int variant, int accumulate,
                                     float *workspace, int B, int H, int W, const float *in_amax,
                                     const float *g_amax, void *stream)
{
    MMLF_CHECK_ARG(in_amax && g_amax, "mmlf_conv2x2_wgrad_h2: the f16 split needs max |in| and max |g|");
    return wgrad_impl(in, cs_in, Cin, g, cs_g, Cout, g_shift, gw, gb, variant, accumulate, workspace, B, H, W,
                      stream, 2, in_amax, g_amax);
}

static int wgrad_impl(const float *in, int cs_in, int Cin, const float *g, int cs_g, int Cout, int g_shift,
                      float *gw, float *gb, int variant, int accumulate, float *workspace, int B, int H, int W,
                      void *stream, int planes, const float *in_amax, const float *g_amax)
{
    MMLF_CHECK_ARG(in && g && (gw || gb) && workspace, "mmlf_conv2x2_wgrad: null pointer");
    MMLF_CHECK_ARG(cs_in % 4 == 0 && cs_g % 4 == 0, "mmlf_conv2x2_wgrad: strides must be multiples of 4");
    MMLF_CHECK_ARG(Cin > 0 && Cin <= cs_in && Cout > 0 && Cout <= cs_g, "mmlf_conv2x2_wgrad: channels vs strides");
    MMLF_CHECK_ARG(Cout <= WGRAD_MAX_COUT_WIDE, "mmlf_conv2x2_wgrad: Cout=%d not supported (max %d)", Cout, WGRAD_MAX_COUT_WIDE);
    MMLF_CHECK_ARG(variant >= 0 && variant <= 2, "mmlf_conv2x2_wgrad: bad variant");
    Grid gr = make_grid(B, H, W);
    MMLF_CHECK_ARG(g_shift >= 0 && g_shift <= gr.P + 1, "mmlf_conv2x2_wgrad: g_shift=%d", g_shift);
    WgradPlan p;
    MMLF_CHECK_ARG(wgrad_plan(planes, Cin, Cout, gr.NQpad / WG_KQ, p), "mmlf_conv2x2_wgrad: no launch plan");   // (refused above)
    WgradArgs a = wgrad_args(in, cs_in, Cin, g, cs_g, g_shift, workspace, gr, grid_alloc_positions(gr), p.scales_off);
    a.in_amax = in_amax; a.g_amax = g_amax;
    hipStream_t st = (hipStream_t)stream;
    if (!gw)                    // the bias gradient alone: one pass over g, partial sums where the weight gradient keeps its own
        return bias_grad_only("mmlf_conv2x2_wgrad", g, cs_g, Cout, g_shift, gb, accumulate, workspace, p.scales_off, gr, st);
    if (planes == 2) {          // per-chunk operand scales, behind the partial sums in the workspace
        MMLF_CHECK_ARG(gr.NQpad + 2 * gr.P + 64 < (1ll << 31), "mmlf_conv2x2_wgrad_h2: batch x image too large");
        ChunkScaleArgs ca;
        ca.in_amax = in_amax; ca.g_amax = g_amax; ca.out = workspace + p.scales_off;
        ca.NQ = gr.NQ; ca.nchunks = a.nchunks; ca.P = gr.P; ca.g_shift = g_shift;
        ca.nrows = (int)amax_rows(gr);
        ca.divP = make_magic((unsigned)gr.P);
        hipLaunchKernelGGL(wgrad_chunk_scales_kernel, dim3((a.nchunks + 255) / 256), dim3(256), 0, st, ca);
        a.chunk_scales = ca.out;
    }
    const WgradArgs whole = a;
    for (int b = 0; b < p.nblocks; ++b) {
        // column block b: output channels [c0, c0 + cout) of g, rows c0 .. of the OIHW master and of the bias gradient
        const int c0 = p.blk[b].c0;
        a = whole;
        a.g = g + c0; a.g_cols = cs_g - c0; a.g_bytes = whole.g_bytes - 4ll * c0;
        const int rc = wgrad_run_block<2>(a, p.blk[b], planes, gw + (size_t)c0 * Cin * 4, gb ? gb + c0 : nullptr, Cin, variant,
                                          accumulate, st);
        if (rc) return rc;
    }
    return 0;
}

// weight + bias gradient of a thin convolution: wave-private sums over its positions, reduced by wgrad_reduce_kernel.
// Four positions per iteration with every load issued up front (the loop is latency-bound otherwise); the wave index
// is made scalar so that the gradients -- the same address for all lanes -- come in through the scalar cache.
__global__ __launch_bounds__(256) void thin_wgrad_kernel(ThinArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const long long nwaves = gridDim.x * 4ll;
    float acc[2][4][THIN_MAXN][4];                        // [half][tap][o][channel of the float4]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int o = 0; o < THIN_MAXN; ++o)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[h][t][o][k] = 0.f;
    float gsum[THIN_MAXN] = {0.f, 0.f};
    const bool first = 4 * lane < a.cs_in, second = 256 + 4 * lane < a.cs_in;
    const int offs[4] = {0, 1, a.P, a.P + 1};
    constexpr int U = 4;
    // a wave owns runs of U consecutive positions: p0 = U * (wave + k * nwaves)
    for (long long p0 = U * wave; p0 < a.npos; p0 += U * nwaves) {
        float4 x0[U], x1[U];
        float gt[U][4][THIN_MAXN];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long p = p0 + u < a.npos ? p0 + u : a.npos - 1;      // (clamped: its gradients are zeroed below)
            const float *row = a.in + (size_t)p * a.cs_in;
            x0[u] = first ? *reinterpret_cast<const float4 *>(row + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
            x1[u] = second ? *reinterpret_cast<const float4 *>(row + 256 + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                // in[p] is tap t's operand of output position p - off_t, whose gradient sits at g[p - off_t + g_shift]
                const long long q = p0 + u - offs[t];
                const bool ok = p0 + u < a.npos && q >= 0 && q < a.NQ;
                // unconditional loads from a clamped position (a select per load would serialise them behind branches);
                // cs_g >= 2: both columns exist, column 1 is a zero pad channel when N == 1
                const float2 gv = *reinterpret_cast<const float2 *>(a.g + (size_t)((ok ? q : 0) + a.g_shift) * a.cs_g);
                gt[u][t][0] = ok ? gv.x : 0.f;
                gt[u][t][1] = ok ? gv.y : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float xs[2][4] = {{x0[u].x, x0[u].y, x0[u].z, x0[u].w}, {x1[u].x, x1[u].y, x1[u].z, x1[u].w}};
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int o = 0; o < THIN_MAXN; ++o)
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[h][t][o][k] = fmaf(xs[h][k], gt[u][t][o], acc[h][t][o][k]);
#pragma unroll
            for (int o = 0; o < THIN_MAXN; ++o) gsum[o] += gt[u][0][o];    // tap 0: every gradient position once
        }
    }
    float *pp = a.wpart + (size_t)wave * 4 * a.CIP * THIN_MAXN;           // [tap][ci][o]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 256 * h + 4 * lane + k;
                if (c < a.C)
#pragma unroll
                    for (int o = 0; o < THIN_MAXN; ++o) pp[((size_t)t * a.CIP + c) * THIN_MAXN + o] = acc[h][t][o][k];
            }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int o = 0; o < THIN_MAXN; ++o) pp[((size_t)t * a.CIP + a.C) * THIN_MAXN + o] = t == 0 ? gsum[o] : 0.f;   // bias row
    }
}

static int thin_wgrad_waves() { return 4 * 4 * device_cus(); }

extern "C" int64_t mmlf_conv2x2_wgrad_thin_workspace_floats(int Cin)
{
    if (Cin <= 0) return -1;
    return (int64_t)thin_wgrad_waves() * 4 * (Cin + 1) * THIN_MAXN;
}

extern "C" int mmlf_conv2x2_wgrad_thin(const float *in, int cs_in, int Cin, const float *g, int cs_g, int Cout, int g_shift,
                                       float *gw_oihw, float *gb, int variant, int accumulate, float *workspace, int B,
                                       int H, int W, void *stream)
{
    MMLF_CHECK_ARG(in && g && (gw_oihw || gb) && workspace, "mmlf_conv2x2_wgrad_thin: null pointer");
    MMLF_CHECK_ARG(Cout >= 1 && Cout <= THIN_MAXN && Cout <= cs_g && Cin >= 1 && Cin <= cs_in && cs_in % 4 == 0 && cs_in <= 512,
                   "mmlf_conv2x2_wgrad_thin: Cin=%d Cout=%d cs_in=%d", Cin, Cout, cs_in);
    MMLF_CHECK_ARG(B > 0 && H > 0 && W > 0 && variant >= 0 && variant <= 2, "mmlf_conv2x2_wgrad_thin: bad shape");
    const Grid gr = make_grid(B, H, W);
    MMLF_CHECK_ARG(g_shift >= 0 && g_shift <= gr.P + 1, "mmlf_conv2x2_wgrad_thin: g_shift=%d", g_shift);
    ThinArgs a = {};
    a.in = in; a.g = g; a.wpart = workspace; a.NQ = gr.NQ; a.npos = gr.NQ + gr.P + 2;
    a.cs_in = cs_in; a.C = Cin; a.N = Cout; a.cs_g = cs_g; a.g_shift = g_shift; a.P = gr.P; a.CIP = Cin + 1;
    hipStream_t st = (hipStream_t)stream;
    if (!gw_oihw)
        return bias_grad_only("mmlf_conv2x2_wgrad_thin", g, cs_g, Cout, g_shift, gb, accumulate, workspace,
                              mmlf_conv2x2_wgrad_thin_workspace_floats(Cin), gr, st);
    const int nwaves = thin_wgrad_waves();
    hipLaunchKernelGGL(thin_wgrad_kernel, dim3(nwaves / 4), dim3(256), 0, st, a);
    const int total = 4 * (Cin + 1) * Cout;
    hipLaunchKernelGGL(wgrad_reduce_wave_kernel, dim3((total + 3) / 4), dim3(256), 0, st, workspace, gw_oihw, gb, Cin, Cout,
                       Cin + 1, THIN_MAXN, nwaves, variant, accumulate);
    return mmlf_launch_status("mmlf_conv2x2_wgrad_thin");
}

extern "C" int mmlf_audit_wgrad_h2(int cs_in, int Cin, int cs_g, int Cout, int g_shift, int B, int H, int W,
                                   int64_t *ends /* [MMLF_AUDIT_WGRAD_N] */)
{
    MMLF_CHECK_ARG(B > 0 && H > 0 && W > 0 && ends && Cin > 0 && Cout > 0, "mmlf_audit_wgrad_h2: bad argument");
    const Grid g = make_grid(B, H, W);
    const long long nchunks = g.NQpad / WG_KQ;
    WgradPlan p;
    MMLF_CHECK_ARG(wgrad_plan(2, Cin, Cout, nchunks, p) && !p.blk[0].nt && !p.blk[p.nblocks - 1].nt,     // (split kernels throughout)
                   "mmlf_audit_wgrad_h2: Cout=%d", Cout);
    const long long last_c = (nchunks - 1) * WG_KQ;
    ends[0] = (last_c + g.P + 32 + 1) * cs_in * 4;                            // in: segment 1, row 32
    ends[1] = (last_c + g_shift + 31 + 1) * cs_g * 4;                         // g
    ends[2] = (int64_t)Cout * Cin * 4 * 4;                                    // gw (OIHW)
    ends[3] = (int64_t)Cout * 4;                                              // gb
    ends[4] = (p.part_floats                                                  // workspace: partial sums of this launch ...
               > p.scales_off ? -1                                              // (must fit the sized region: else the scales overlap them)
               : p.scales_off + 2 * nchunks + 2) * 4;                           // ... then the per-chunk and the two tensor scales
    ends[5] = (MMLF_AMAX_HEAD + amax_rows(g)) * 4;                            // in_amax (the scale kernel clamps rows to amax_rows - 1)
    ends[6] = ends[5];                                                        // g_amax
    return 0;
}

// ---------------------------------------------------------------------------------------------
// weight + bias gradient of the 3x3 ("same", pad 1) convolution, exact-f32 MFMA (wgrad9tap_kernel = wgrad_f32_taps<3, NT>
// above, g_shift = P + 1): entry points
// ---------------------------------------------------------------------------------------------
// launch layout of the 3x3 weight gradient: one block (wgrad_f32_block), 3 * (ci slices) x position splits
static inline bool wgrad9_plan(int Cin, int Cout, WgradBlock &k) { return Cin > 0 && wgrad_f32_block(3, Cin, 0, Cout, k); }

extern "C" int64_t mmlf_wgrad3x3_workspace_floats(int Cin, int Cout, int B, int H, int W)
{
    WgradBlock k;
    if (!wgrad9_plan(Cin, Cout, k) || B <= 0 || H <= 0 || W <= 0) return -1;
    return k.part_floats;
}

extern "C" int mmlf_conv3x3_wgrad(const float *in, int cs_in, int Cin, const float *g, int cs_g, int Cout, float *gw_oihw,
                                  float *gb, int variant, int accumulate, float *workspace, int B, int H, int W, void *stream)
{
    MMLF_CHECK_ARG(in && g && (gw_oihw || gb) && workspace, "mmlf_conv3x3_wgrad: null pointer");
    MMLF_CHECK_ARG(B > 0 && H > 0 && W > 0, "mmlf_conv3x3_wgrad: bad shape B=%d H=%d W=%d", B, H, W);
    MMLF_CHECK_ARG(cs_in % 4 == 0 && cs_g % 4 == 0, "mmlf_conv3x3_wgrad: strides must be multiples of 4");
    MMLF_CHECK_ARG(Cin > 0 && Cin <= cs_in && Cout > 0 && Cout <= cs_g, "mmlf_conv3x3_wgrad: channels vs strides");
    MMLF_CHECK_ARG(variant >= 0 && variant <= 2, "mmlf_conv3x3_wgrad: bad variant");
    WgradBlock k;
    MMLF_CHECK_ARG(wgrad9_plan(Cin, Cout, k), "mmlf_conv3x3_wgrad: Cout=%d not supported", Cout);
    const Grid gr = make_grid(B, H, W);
    MMLF_CHECK_ARG(gr.NQpad + 2 * gr.P + 64 < (1ll << 31), "mmlf_conv3x3_wgrad: batch x image too large");
    if (!gw_oihw)
        return bias_grad_only("mmlf_conv3x3_wgrad", g, cs_g, Cout, gr.P + 1, gb, accumulate, workspace, k.part_floats, gr,
                              (hipStream_t)stream);
    WgradArgs a = wgrad_args(in, cs_in, Cin, g, cs_g, gr.P + 1, workspace, gr, grid_alloc_positions_k3(gr), k.part_floats);
    return wgrad_run_block<3>(a, k, 0, gw_oihw, gb, Cin, variant, accumulate, (hipStream_t)stream);
}

// Bounds audit of one mmlf_conv3x3_wgrad launch (ends[MMLF_AUDIT_WG_IN .. MMLF_AUDIT_WG_WORKSPACE]): chunk c stages
// in[32 c + dy P .. + 33] and g[32 c + P + 1 .. + 31], c < NQpad / 32.
extern "C" int mmlf_audit_wgrad3x3(int cs_in, int Cin, int cs_g, int Cout, int B, int H, int W, int64_t *ends /* [5] */)
{
    WgradBlock k;
    MMLF_CHECK_ARG(B > 0 && H > 0 && W > 0 && ends && wgrad9_plan(Cin, Cout, k), "mmlf_audit_wgrad3x3: bad argument");
    const Grid g = make_grid(B, H, W);
    const long long last_c = g.NQpad - WG_KQ;
    // (k.CIP: channels the last slice stages, k.NP: gradient columns a workgroup stages -- below the strides only)
    ends[0] = ((last_c + 2 * g.P + WG_KQ + 1) * cs_in + (k.CIP < cs_in ? k.CIP : cs_in)) * 4;   // in
    ends[1] = ((last_c + g.P + 1 + WG_KQ - 1) * cs_g + (k.NP < cs_g ? k.NP : cs_g)) * 4;        // g
    ends[2] = (int64_t)Cout * Cin * 9 * 4;                                    // gw (OIHW)
    ends[3] = (int64_t)Cout * 4;                                              // gb
    ends[4] = k.part_floats * 4;                                              // workspace
    return 0;
}
