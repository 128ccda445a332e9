// conv.hip -- MFMA implicit-GEMM kernels for the k=2 and k=3 convolutions of the EPI-stack CNN, forward and data gradient,
// on the padded NHWC grid (the weight + bias gradient: wgrad.hip; shared device helpers: conv_device.h).  gfx950 only.
// Arithmetic paths with the same interfaces: exact-f32 MFMA (conv_f32_taps<KS, NT>, the one body behind conv4tap_kernel for
// k=2 and conv9tap_kernel for k=3) and, for k=2, the split paths at f32 accuracy (conv4tap_x6s_kernel, conv4tap_rs_kernel:
// bf16x6 / f16x3).
//
// Arithmetic replaced: nn.Conv2d(k=2, pad 1|0) forward / backward as used by
// reference mmlf/model/feed_forward.py:123,125 (autograd via mmlf/train/cli.py:257).
//
// All three are 4-tap correlations over the flat grid position q with tap offsets
// {0, 1, P, P+1} (include/mmlf_hip.h).  v_mfma_f32_32x32x2_f32 is an exact f32 fma chain, so the
// exact-f32 path is float32-exact up to summation order.
#include "conv_device.h"


#ifdef MMLF_BOUNDS_DEBUG
// (every translation unit counts into its own device array, common.h: this one's plus the weight-gradient unit's)
extern "C" int mmlf_debug_oob_counts(unsigned long long *host8, int reset)
{
    unsigned long long other[8];
    if (hipMemcpyFromSymbol(host8, HIP_SYMBOL(g_mmlf_oob), sizeof(unsigned long long) * 8) != hipSuccess) return 1;
    if (reset) {
        const unsigned long long z[8] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_mmlf_oob), z, sizeof(z)) != hipSuccess) return 1;
    }
    if (mmlf_oob_counts_wgrad(other, reset)) return 1;
    for (int k = 0; k < 8; ++k) host8[k] += other[k];
    return 0;
}
#endif

// ---------------------------------------------------------------------------------------------
// Column blocks of the wide 2x2 layers (288 < N <= 512).  Such a layer is computed as TWO blocks of 160, 192
// or 256 packed columns each (G = 10, 12, 16 sixteen-column groups; 320, 384 or 512 packed columns in all: nothing wasted at
// N = 320, 384 and 512, an eighth at 448), by the kernel bodies the narrower layers run, one launch per block.  Block b owns
// output channels [b * npb, (b + 1) * npb): its own packed filter (the blocks lie back to back, each a complete packed
// filter of npb columns -- for the f16 split with its columns' unscale tail), its bias / output / reference offsets, its
// range of the BatchNorm partials and its quarter (256 of every 512) of the transposed ReLU mask words.
// wide_np is the ONE rule: the size queries, packing, the launches and the audit all go through it (x6_np / f32_np below),
// and a packed-column total above 288 can only have come from it, which is how the packing kernels find a column's block.
// ---------------------------------------------------------------------------------------------
constexpr int MMLF_MAX_N = 288;          // packed columns of one launch
constexpr int MMLF_MAX_N_WIDE = 512;     // ... of a layer in column blocks (2x2 filters)
static inline int wide_np(int N)         // total packed columns of a wide layer
{
    if (N <= MMLF_MAX_N || N > MMLF_MAX_N_WIDE) return -1;
    return N <= 320 ? 320 : N <= 384 ? 384 : 512;
}
__host__ __device__ static inline int col_blocks(int np_total) { return np_total > MMLF_MAX_N ? 2 : 1; }
// packed column n of np_total -> its block, its column there, the block's columns
__device__ __forceinline__ void col_block_of(int n, int np_total, int &blk, int &nl, int &npb)
{
    npb = np_total / col_blocks(np_total);
    blk = n >= npb ? 1 : 0;
    nl = n - blk * npb;
}
// What ONE column block of npb packed columns over nchunk chunks of 8 input channels takes in a packed filter, per layout.
// The packing kernels place a block by these; the size queries, the launches and the audit read them through ConvPlan.
//  exact f32: [chunk][tap(taps)][kh(2)][npb][4] floats
__host__ __device__ static inline size_t packed_f32_block_floats(int taps, int nchunk, int npb)
{
    return (size_t)nchunk * taps * 2 * npb * 4;
}
//  split: [chunk][plane(planes)][tap(4)][npb][8] 16-bit values, planes = 3 (bf16) or 2 (f16) ...
__host__ __device__ static inline size_t packed_split_planes_bytes(int planes, int nchunk, int npb)
{
    return (size_t)nchunk * planes * 4 * npb * 16;
}
//  ... and, behind the f16 planes, 1 / scale of every column of the block
__host__ __device__ static inline size_t packed_split_block_bytes(int planes, int nchunk, int npb)
{
    return packed_split_planes_bytes(planes, nchunk, npb) + (planes == 2 ? (size_t)npb * 4 : 0);
}

// ---------------------------------------------------------------------------------------------
// filter packing, exact f32: OIHW master (Cout, Cin, KS, KS) -> [chunk][tap(KS*KS)][kh][NP][4] with k = 8*chunk + 4*kh + s.
// dgrad = 1 packs the data gradient's filter: taps rotated by 180 degrees, Cin / Cout swapped.
// ---------------------------------------------------------------------------------------------
template <int KS>
__global__ void pack_filter_f32_kernel(const float *__restrict__ w, float *__restrict__ out, int Cout, int Cin,
                                       int variant, int dgrad, int nchunk, int NP)
{
    constexpr int TAPS = KS * KS;
    const long long total = (long long)nchunk * TAPS * 2 * NP * 4;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        int s = idx & 3;
        long long r = idx >> 2;
        int n = r % NP; r /= NP;
        int kh = r & 1; r >>= 1;
        int t = r % TAPS; r /= TAPS;
        int c = (int)r;
        int k = 8 * c + 4 * kh + s;
        int ci, co, tsrc;
        if (!dgrad) { ci = k; co = n; tsrc = t; }
        else { co = k; ci = n; tsrc = TAPS - 1 - t; }
        float v = 0.f;
        if (ci < Cin && co < Cout) v = w[((size_t)co * Cin + ci) * TAPS + master_tap<KS>(tsrc, variant)];
        int blk, nl, npb;                  // (one block: the linear index idx)
        col_block_of(n, NP, blk, nl, npb);
        out[blk * packed_f32_block_floats(TAPS, nchunk, npb) + ((((size_t)c * TAPS + t) * 2 + kh) * npb + nl) * 4 + s] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// forward / data-gradient kernel
// ---------------------------------------------------------------------------------------------
struct ConvArgs {
    const float *in;
    const float *wp;
    const float *bias;
    float *out;
    const float *ref;
    long long NQ;
    int cs_in, nchunk, cs_out, n_store, n_true, out_shift, vh, vw, P, G, relu, cs_ref;
    int a_pieces, seg_slot, seg_delta;   // split kernel: A window geometry (see conv4tap_x6s_kernel): 32-position pieces,
    int a_per_seg, a_tail;               // ... pieces per segment, positions the last piece of a segment has to fetch
    int nw;                              // waves per workgroup the launch uses (8, or 16: 512-position tiles)
    const float *in_amax;                // f16 split: amax array of `in` (common.h): per-wave power-of-two operand scales
    const float *w_unscale;              // f16 split: 1 / (power-of-two scale of packed column n), [NP]
    float *out_amax;                     // optional: amax array of `out` (tensor and grid-row maxima, atomic max)
    Magic divP, divR;                    // q / P and row / R without integer division
    int R;
    double *bn_partial;                  // optional (f16 split): per-workgroup sums of out and out^2 per channel,
                                         // [block][2][bn_stride] doubles, the input of the BatchNorm finalize
    int bn_stride;                       // channels of the whole layer (= n_true unless the launch is a column block of it)
    unsigned *relu_mask_out;             // optional: (out > 0) as bits, [tile][wave][8 rows][64 lanes] words, bit = column block
    const unsigned *relu_mask_in;        // optional: such a mask instead of relu_ref (same launch geometry and N)
    // bytes the caller's buffers hold behind `out` / `ref` by the ABI's contract (mmlf_grid_alloc_positions): the epilogue's
    // buffer descriptors carry what is left of them as num_records, so that a store or load past the allocation would be
    // DROPPED by the address unit instead of faulting (round 5; until then the range check was switched off).  None is
    // expected: tests/test_bounds_audit.py derives every launch's extents, and a -DMMLF_BOUNDS_DEBUG build counts them.
    long long out_bytes, ref_bytes;
    long long in_bytes, amax_n, mask_words;   // read by the MMLF_BOUNDS_DEBUG build only
};


// epilogue shared by the f32 and the split-bf16 kernels: D[row = position][col = channel]; a lane
// holds column i of every N tile and rows (r&3)+8(r>>2)+4kh of its wave's 32 positions.
// Epilogues.  All eight waves of a workgroup run theirs at the same time, so the matrix cores idle
// meanwhile: written for few instructions and few serialized memory round trips.
//  * row validity: lane l classifies row l&31 of the wave's 32 positions (ONE division per lane) and a
//    ballot makes the 32-bit row mask;
//  * addressing: buffer instructions on a wave-uniform tile descriptor + 32-bit per-lane byte offsets
//    (the column-block offset folds into the instruction's immediate);
//  * bias and (data-gradient) ReLU-reference values are loaded in batches ahead of their use.
__device__ __forceinline__ unsigned wave_row_mask(const ConvArgs &a, long long Q0, int w, int lane)
{
    const unsigned qrow = (unsigned)Q0 + 32 * w + (lane & 31);
    const unsigned row = fastdiv(qrow, a.divP);                 // global grid row
    const int x = (int)(qrow - row * a.P), y = (int)(row - fastdiv(row, a.divR) * a.R);
    return (unsigned)__ballot((long long)qrow < a.NQ && y < a.vh && x < a.vw);
}

// 32x32 tiling: lane (i, kh) holds column i of each 32-column block, rows (r&3) + 8*(r>>2) + 4*kh.
template <int NT>
__device__ __forceinline__ void conv_epilogue(const ConvArgs &a, const f32x16 (&acc)[NT], long long Q0, int w, int i,
                                              int kh)
{
    const unsigned m = wave_row_mask(a, Q0, w, i) >> (4 * kh);
    const long long qb = Q0 + 32 * w + a.out_shift;                                     // wave-uniform
    const __amdgpu_buffer_rsrc_t ob = __builtin_amdgcn_make_buffer_rsrc(
        a.out + (size_t)qb * a.cs_out, 0, mmlf_records_left(a.out_bytes, qb * a.cs_out * 4ll), MMLF_BUF_FLAGS);
    const bool has_ref = a.ref != nullptr;
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(has_ref ? a.ref + (size_t)qb * a.cs_ref : a.out), 0,
        has_ref ? mmlf_records_left(a.ref_bytes, qb * a.cs_ref * 4ll) : 0, MMLF_BUF_FLAGS);
    unsigned lo = ((unsigned)(4 * kh) * a.cs_out + i) * 4u;
    unsigned lr = ((unsigned)(4 * kh) * a.cs_ref + i) * 4u;
    // the per-row offsets derived from these are tile-invariant: opaque to the optimiser so that it does
    // not hoist 32 of them out of the persistent loop and hold them in VGPRs through the main loop
    asm volatile("" : "+v"(lo), "+v"(lr));
    float bv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ch = 32 * nt + i;
        bv[nt] = (a.bias && ch < a.n_true) ? a.bias[ch] : 0.f;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (32 * nt + i >= a.n_store) continue;
        unsigned keep = m;                 // bit rc: row valid (and, for a data gradient, reference > 0)
        if (has_ref) {
            float rv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                rv[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                    rb, lr + (unsigned)((r & 3) + 8 * (r >> 2)) * a.cs_ref * 4u + 128 * nt, 0, 0));
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (!(rv[r] > 0.f)) keep &= ~(1u << ((r & 3) + 8 * (r >> 2)));
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rc = (r & 3) + 8 * (r >> 2);
            float v = acc[nt][r] + bv[nt];
            if (a.relu) v = fmaxf(v, 0.f);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((keep >> rc & 1) ? v : 0.f), ob,
                                                  lo + (unsigned)rc * a.cs_out * 4u + 128 * nt, 0, 0);
        }
    }
}

// f16-split filter packing: [chunk][plane(2)][tap(4)][NP][8 f16] of w * scale[n], one workgroup per packed
// column n (= output channel of the launch).  Every column carries its own power-of-two scale (its max |w|
// goes to [2^14, 2^15)), so an output channel whose weights are small as a whole keeps its 22 bits;
// unscale[n] = 1 / scale[n] is what the convolution's epilogue multiplies column n by.
// `packed`: the filter's whole packed image, NP its packed columns in all: column n lies in a column block of its own
// (col_block_of) whose planes are followed by its columns' unscale factors.
__device__ __forceinline__ void pack_filter_h2_column(const float *__restrict__ w, void *__restrict__ packed,
                                                      int Cout, int Cin, int variant, int dgrad, int nchunk, int NP,
                                                      int n, float *red)
{
    const int tid = threadIdx.x;
    int blk, nl, npb;
    col_block_of(n, NP, blk, nl, npb);
    char *const base = reinterpret_cast<char *>(packed) + blk * packed_split_block_bytes(2, nchunk, npb);
    unsigned short *const out = reinterpret_cast<unsigned short *>(base);
    float *const unscale = reinterpret_cast<float *>(base + packed_split_planes_bytes(2, nchunk, npb));
    const int K = dgrad ? Cout : Cin, N = dgrad ? Cin : Cout;
    auto at = [&](int k, int tap) -> size_t {      // OIHW index of (packed row k, column n, master tap)
        return dgrad ? ((size_t)k * Cin + n) * 4 + tap : ((size_t)n * Cin + k) * 4 + tap;
    };
    float m = 0.f;
    if (n < N)
        for (int e = tid; e < 4 * K; e += 256) m = fmaxf(m, fabsf(w[at(e >> 2, e & 3)]));
    m = mmlf_wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    const float sc = pow2_scale_for(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
    if (tid == 0) unscale[nl] = 1.f / sc;
    for (int e = tid; e < 4 * nchunk; e += 256) {
        const int c = e >> 2, t = e & 3;
        const int tap = master_tap<2>(dgrad ? 3 - t : t, variant);
        unsigned short h[8], l[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * c + j;
            const float v = (k < K && n < N) ? w[at(k, tap)] * sc : 0.f;
            const _Float16 hh = (_Float16)v, ll = (_Float16)(v - (float)hh);
            h[j] = __builtin_bit_cast(unsigned short, hh);
            l[j] = __builtin_bit_cast(unsigned short, ll);
        }
        uint4 vh, vl;
        vh.x = h[0] | (unsigned)h[1] << 16; vh.y = h[2] | (unsigned)h[3] << 16;
        vh.z = h[4] | (unsigned)h[5] << 16; vh.w = h[6] | (unsigned)h[7] << 16;
        vl.x = l[0] | (unsigned)l[1] << 16; vl.y = l[2] | (unsigned)l[3] << 16;
        vl.z = l[4] | (unsigned)l[5] << 16; vl.w = l[6] | (unsigned)l[7] << 16;
        *reinterpret_cast<uint4 *>(out + ((((size_t)c * 2 + 0) * 4 + t) * npb + nl) * 8) = vh;
        *reinterpret_cast<uint4 *>(out + ((((size_t)c * 2 + 1) * 4 + t) * npb + nl) * 8) = vl;
    }
}

__global__ __launch_bounds__(256) void pack_filter_h2_kernel(const float *__restrict__ w, void *__restrict__ packed,
                                                             int Cout, int Cin, int variant, int dgrad, int nchunk, int NP)
{
    __shared__ float red[4];
    pack_filter_h2_column(w, packed, Cout, Cin, variant, dgrad, nchunk, NP, blockIdx.x, red);
}

// many filters, one launch: workgroup b packs column b - col0 of the filter whose column range holds b
__global__ __launch_bounds__(256) void pack_filters_h2_kernel(const mmlf_pack_desc *__restrict__ table, int n)
{
    __shared__ float red[4];
    int lo = 0, hi = n - 1;                          // last descriptor with col0 <= blockIdx.x (wave-uniform search)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].col0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const mmlf_pack_desc d = table[lo];
    const int K = d.dgrad ? d.Cout : d.Cin;
    const int nchunk = (K + 7) / 8;
    pack_filter_h2_column(d.w_oihw, d.packed, d.Cout, d.Cin, d.variant, d.dgrad, nchunk, d.np, (int)blockIdx.x - d.col0, red);
}

// split-precision filter packing: [chunk][plane(3)][tap(4)][NP][8 bf16], k = 8*chunk+j
__global__ void pack_filter_split_kernel(const float *__restrict__ w, unsigned short *__restrict__ out, int Cout,
                                         int Cin, int variant, int dgrad, int nchunk, int NP)
{
    const long long total = (long long)nchunk * 2 * 2 * NP * 8;   // one thread per (chunk,u,kh,n,j)
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int j = idx & 7;
        long long r = idx >> 3;
        const int n = r % NP; r /= NP;
        const int kh = r & 1; r >>= 1;
        const int u = r & 1; r >>= 1;
        const int c = (int)r;
        const int k = 8 * c + j, t = 2 * u + kh;
        int ci, co, tsrc;
        if (!dgrad) { ci = k; co = n; tsrc = t; }
        else { co = k; ci = n; tsrc = 3 - t; }
        float v = 0.f;
        if (ci < Cin && co < Cout) v = w[((size_t)co * Cin + ci) * 4 + master_tap<2>(tsrc, variant)];
        unsigned p[3];
        split3(v, p[0], p[1], p[2]);
        int blk, nl, npb;
        col_block_of(n, NP, blk, nl, npb);
        unsigned short *const ob = out + blk * packed_split_block_bytes(3, nchunk, npb) / 2;
        for (int pl = 0; pl < 3; ++pl) {
            ob[((((size_t)c * 3 + pl) * 4 + t) * npb + nl) * 8 + j] = (unsigned short)p[pl];
        }
    }
}


// ---------------------------------------------------------------------------------------------
// forward / data-gradient kernel, split-bf16 arithmetic ("bf16x6"):
// every f32 operand is split EXACTLY into three bf16 (hi+mid+lo) and each product is evaluated as the
// six leading cross terms on the bf16 matrix cores with f32 accumulation (dropped terms are
// <= 2^-26 relative).  Measured on gfx950 (tools/bf16x6_accuracy.hip): error vs a double reference
// 1.4e-8*sum|a*b| mean, 1.0e-7 max at K=1120 -- slightly BELOW the f32 MFMA fma chain (1.7e-8 /
// 1.9e-7) -- at 16/6 = 2.67x the f32 MFMA rate.
// ---------------------------------------------------------------------------------------------

// 16x16 tiling: lane (r16, q4) holds column r16 of each 16-column block and rows 16*mb + 4*q4 + r.
// unscale_a undoes this wave's activation scale, a.w_unscale[n] column n's weight scale (powers of two: exact).
// With a.out_amax the wave also raises the output's amax array: its 32 positions lie in at most two grid rows
// when P >= 32 (exact row maxima); for smaller pitches the rows behind the first get the common maximum
// (an upper bound, which is all the consumers need).
// EPI selects what the epilogue is compiled for: EPI_GENERIC reads every option from the launch arguments at run
// time; the other values are the launch kinds of a training step, each compiled WITHOUT the code of the others (the
// generic form carries the registers and branches of all options through every launch: 2-3 % of a 280-channel one).
enum { EPI_GENERIC = -1, EPI_PLAIN = 0, EPI_RELU = 1, EPI_STATS = 2, EPI_BITS_IN = 4, EPI_REF_IN = 8, EPI_MASK_OUT = 16 };
template <int G, int EPI>
__device__ __forceinline__ void conv_epilogue16(const ConvArgs &a, const f32x4 (&acc)[2][G], long long Q0, int w,
                                                int r16, int q4, float unscale_a, float &run_max,
                                                double *stats_in /* this wave's [16*G][2] sums, or null */)
{
    constexpr bool GEN = EPI == EPI_GENERIC;
    const bool do_relu = GEN ? a.relu != 0 : (EPI & EPI_RELU) != 0;
    double *const stats = (GEN || (EPI & EPI_STATS)) ? stats_in : nullptr;
    const bool mask_out = GEN ? a.relu_mask_out != nullptr : (EPI & EPI_MASK_OUT) != 0;
    const unsigned m = wave_row_mask(a, Q0, w, r16 + 16 * q4) >> (4 * q4);
    const long long qb = Q0 + 32 * w + a.out_shift;                                     // wave-uniform
    const int ob_left = mmlf_records_left(a.out_bytes, qb * a.cs_out * 4ll);
    const __amdgpu_buffer_rsrc_t ob =
        __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)qb * a.cs_out, 0, ob_left, MMLF_BUF_FLAGS);
    const bool has_ref = GEN ? a.ref != nullptr : (EPI & EPI_REF_IN) != 0;
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(has_ref ? a.ref + (size_t)qb * a.cs_ref : a.out), 0,
        has_ref ? mmlf_records_left(a.ref_bytes, qb * a.cs_ref * 4ll) : 0, MMLF_BUF_FLAGS);
    unsigned lo = ((unsigned)(4 * q4) * a.cs_out + r16) * 4u;
    unsigned lr = ((unsigned)(4 * q4) * a.cs_ref + r16) * 4u;
    asm volatile("" : "+v"(lo), "+v"(lr));   // see conv_epilogue
    float mk[8];                             // max |out| per position this lane holds (over the column blocks)
#pragma unroll
    for (int k = 0; k < 8; ++k) mk[k] = 0.f;
    // ReLU masks as bits: the forward pass leaves (out > 0) of every element it wrote in the accumulator layout of
    // THIS kernel -- word (tile, wave, row k, lane), bit = column block -- and the data gradient of the layer above
    // (same grid, same N, hence the same layout) reads its eight words with eight coalesced loads up front instead of
    // 8 x G scattered loads of the activations between its stores (a fifth of that launch)
    const bool use_bits = GEN ? a.relu_mask_in != nullptr : (EPI & EPI_BITS_IN) != 0;
    const size_t mbase = ((size_t)(Q0 / MMLF_TILE) * 8 + w) * 512 + (r16 + 16 * q4);
    unsigned mw[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) mw[k] = use_bits ? a.relu_mask_in[mbase + 64 * k] : 0u;
    MMLF_OOB(OOB_MASK, (use_bits || mask_out) && (long long)mbase + 64 * 7 >= a.mask_words);
    // bias and weight-unscale of all of this lane's columns up front: a load between the stores makes the compiler
    // wait for the wave's vector-memory counter to reach zero there, i.e. for every store issued so far (and every DMA
    // piece in flight) -- once per column block
    float bv[G], uwv[G];
#pragma unroll
    for (int nb = 0; nb < G; ++nb) {
        const int ch = 16 * nb + r16;
        bv[nb] = (a.bias && ch < a.n_true) ? a.bias[ch] : 0.f;
        uwv[nb] = (a.w_unscale && ch < 16 * G) ? a.w_unscale[ch] : 1.f;
    }
#pragma unroll
    for (int nb = 0; nb < G; ++nb) asm volatile("" : "+v"(bv[nb]), "+v"(uwv[nb]));   // loaded HERE, not sunk to their uses
#pragma unroll
    for (int nb = 0; nb < G; ++nb) {
        const int ch = 16 * nb + r16;
        if (ch >= a.n_store) continue;
        const float bvn = bv[nb];
        const float uw = uwv[nb];
        unsigned keep = m;
        float s1 = 0.f, s2 = 0.f;
        if (use_bits) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (!(mw[k] >> nb & 1)) keep &= ~(1u << (16 * (k >> 2) + (k & 3)));
        } else if (has_ref) {
            float rv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k)
            {
                MMLF_OOB(OOB_REF, (qb * a.cs_ref * 4ll) + lr + (long long)(16 * (k >> 2) + (k & 3)) * a.cs_ref * 4 + 64 * nb >= a.ref_bytes);
                rv[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                    rb, lr + (unsigned)(16 * (k >> 2) + (k & 3)) * a.cs_ref * 4u + 64 * nb, 0, 0));
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (!(rv[k] > 0.f)) keep &= ~(1u << (16 * (k >> 2) + (k & 3)));
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int rc = 16 * (k >> 2) + (k & 3);
            float v = fmaf(acc[k >> 2][nb][k & 3] * unscale_a, uw, bvn);   // the products are exact (powers of two): one rounding, as before
            if (do_relu) v = fmaxf(v, 0.f);
            v = (keep >> rc & 1) ? v : 0.f;
            if (mask_out) mw[k] |= (v > 0.f ? 1u : 0u) << nb;
            asm("v_max_f32 %0, %1, |%2|" : "=v"(mk[k]) : "v"(mk[k]), "v"(v));   // (fmaxf canonicalises its operand first: two instructions)
            s1 += v;
            s2 = fmaf(v, v, s2);
            // row offset in the scalar offset operand, column block in the immediate: no address arithmetic per element
            MMLF_OOB(OOB_OUT, (long long)lo + 64 * nb + (long long)rc * a.cs_out * 4 >= ob_left);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ob, lo + 64 * nb, (unsigned)rc * a.cs_out * 4u, 0);
        }
        if (stats) {            // BatchNorm statistics: this wave's 32 positions of channel 16*nb + r16
            s1 += __shfl_xor(s1, 16); s1 += __shfl_xor(s1, 32);
            s2 += __shfl_xor(s2, 16); s2 += __shfl_xor(s2, 32);
            if (q4 == 0) {      // one owner lane per channel: plain read-modify-write, fixed order
                stats[2 * (16 * nb + r16)] += (double)s1;
                stats[2 * (16 * nb + r16) + 1] += (double)s2;
            }
        }
    }
    if (mask_out) {
#pragma unroll
        for (int k = 0; k < 8; ++k) a.relu_mask_out[mbase + 64 * k] = mw[k];
    }
    if (a.out_amax) {
        const unsigned d0 = (unsigned)qb;                       // first destination position of the wave
        const unsigned rd0 = fastdiv(d0, a.divP);
        const int nfirst = (int)((rd0 + 1) * (unsigned)a.P - d0);   // wave positions [0, nfirst) lie in grid row rd0
        float m_lo = 0.f, m_hi = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int pos = 16 * (k >> 2) + 4 * q4 + (k & 3);
            if (pos < nfirst) m_lo = fmaxf(m_lo, mk[k]);
            else m_hi = fmaxf(m_hi, mk[k]);
        }
        m_lo = mmlf_wave_max(m_lo);
        m_hi = mmlf_wave_max(m_hi);
        if (r16 + 16 * q4 == 0) {
            MMLF_OOB(OOB_AMAX, MMLF_AMAX_HEAD + (long long)fastdiv(d0 + 31, a.divP) >= a.amax_n);
            if (m_lo > 0.f) mmlf_amax_raise_nowait(a.out_amax + MMLF_AMAX_HEAD + rd0, m_lo);
            if (m_hi > 0.f) {
                const unsigned rdl = fastdiv(d0 + 31, a.divP);
                for (unsigned r = rd0 + 1; r <= rdl; ++r) mmlf_amax_raise_nowait(a.out_amax + MMLF_AMAX_HEAD + r, m_hi);
            }
            run_max = fmaxf(run_max, fmaxf(m_lo, m_hi));        // lane 0 carries the tensor maximum
        }
    }
}

// ---------------------------------------------------------------------------------------------
// TRANSPOSED epilogue (round 5).  The MFMA is symmetric in its two operands: with the weights as the A operand and the
// activations as B the same instruction yields the transposed tile -- lane (r16, q4) then holds FOUR CONSECUTIVE CHANNELS
// 16 nb + 4 q4 + r of ONE position 16 mb + r16 per accumulator tile instead of one channel of four positions.  What that buys:
//  * the tile is stored with 16-byte instructions (the four lanes of a position write 64 consecutive bytes): 2 G store
//    instructions per wave and tile instead of 8 G.  The epilogue's store tail is bound by the ISSUE of its vector-memory
//    instructions, not by their bytes (round 2: all eight waves stand in it at once and the matrix cores idle meanwhile);
//  * a position's validity / ReLU bits are per lane and row block, not per value: the row mask is two bits per lane,
//    the ReLU mask words hold (nb, r) as bit 4 (nb % 8) + r of word nb / 8: 2 ceil(G / 8) words per lane instead of 8
//    (a third of the mask traffic on the 280-wide layers, a quarter on the 70-wide ones);
//  * bias and weight-unscale of a lane's four channels are two ds_read_b128 from a table the workgroup put into LDS once
//    per launch (global loads between the stores made every column block wait for all stores issued so far).
// The values are formed exactly as in conv_epilogue16 -- fma(acc * unscale_a, uw, bias), one rounding -- so the two
// orientations write the same bits (tests/test_gpu_kernels.py::test_transposed_epilogue_writes_the_same_bits).
// Launch kinds: plain, ReLU, ReLU + mask-out, mask-in (three of a training block's four convolution launches); the
// statistics kind keeps conv_epilogue16 (its sums run over positions = along a lane's registers there, across lanes here).
// Needs n_store % 4 == 0 and a 16-byte aligned `out` (the host checks; channel slices at odd offsets take the other form).
// ---------------------------------------------------------------------------------------------
template <int G> constexpr int tr_mask_words() { return (G + 7) / 8; }
template <int G, int EPI>
__device__ __forceinline__ void conv_epilogue16_tr(const ConvArgs &a, const f32x4 (&acc)[2][G], long long Q0, int w,
                                                   int r16, int q4, float unscale_a, float &run_max,
                                                   const float *coef /* LDS: [16 G] weight-unscale, [16 G] bias */)
{
    static_assert(EPI >= 0 && !(EPI & (EPI_STATS | EPI_REF_IN)), "kinds of the transposed epilogue");
    constexpr int NP = 16 * G, MW = tr_mask_words<G>();
    constexpr bool do_relu = (EPI & EPI_RELU) != 0, mask_out = (EPI & EPI_MASK_OUT) != 0, use_bits = (EPI & EPI_BITS_IN) != 0;
    const unsigned m = wave_row_mask(a, Q0, w, r16 + 16 * q4);      // bit p: position p of the wave's 32 is a valid output
    const long long qb = Q0 + 32 * w + a.out_shift;                   // wave-uniform
    const int ob_left = mmlf_records_left(a.out_bytes, qb * a.cs_out * 4ll);
    const __amdgpu_buffer_rsrc_t ob =
        __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)qb * a.cs_out, 0, ob_left, MMLF_BUF_FLAGS);
    unsigned lo = ((unsigned)r16 * a.cs_out + 4u * q4) * 4u;
    asm volatile("" : "+v"(lo));             // (tile-invariant: kept out of the persistent loop's registers, see conv_epilogue)
    const size_t mbase = ((size_t)(Q0 / MMLF_TILE) * 8 + w) * 512 + (r16 + 16 * q4);
    unsigned mw[2][MW];
    bool ok[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        ok[mb] = (m >> (16 * mb + r16) & 1u) != 0;
#pragma unroll
        for (int j = 0; j < MW; ++j) {
            mw[mb][j] = use_bits ? a.relu_mask_in[mbase + 64 * (MW * mb + j)] : 0u;
            if (use_bits && !ok[mb]) mw[mb][j] = 0u;        // an invalid position keeps nothing
        }
    }
    MMLF_OOB(OOB_MASK, (use_bits || mask_out) && (long long)mbase + 64 * (2 * MW - 1) >= a.mask_words);
    float mk[2] = {0.f, 0.f};                 // max |out| of this lane's two positions
    // the table values of column block nb + 1 are requested while block nb is worked on; the fences keep the scheduler from
    // pulling ALL blocks' reads to the front (8 registers per block: the wide kernel has none to spare)
    const float *cl = coef + 4 * q4;
    f32x4 uw_n = *reinterpret_cast<const f32x4 *>(cl), b_n = *reinterpret_cast<const f32x4 *>(cl + NP);
#pragma unroll
    for (int nb = 0; nb < G; ++nb) {
        const int c0 = 16 * nb + 4 * q4;
        const f32x4 uw4 = uw_n, b4 = b_n;
        if (nb + 1 < G) {
            uw_n = *reinterpret_cast<const f32x4 *>(cl + 16 * (nb + 1));
            b_n = *reinterpret_cast<const f32x4 *>(cl + NP + 16 * (nb + 1));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            u32x4 st;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = fmaf(acc[mb][nb][r] * unscale_a, uw4[r], b4[r]);   // the products are exact (powers of two): one rounding
                if (do_relu) v = fmaxf(v, 0.f);
                if (use_bits) {              // 0 or ~0 from the bit: two instructions per value
                    const int keep = ((int)(mw[mb][nb >> 3] << (31 - (4 * (nb & 7) + r)))) >> 31;
                    v = __uint_as_float(__float_as_uint(v) & (unsigned)keep);
                } else {
                    v = ok[mb] ? v : 0.f;
                }
                if (mask_out) mw[mb][nb >> 3] |= (v > 0.f ? 1u : 0u) << (4 * (nb & 7) + r);
                asm("v_max_f32 %0, %1, |%2|" : "=v"(mk[mb]) : "v"(mk[mb]), "v"(v));
                st[r] = __float_as_uint(v);
            }
            if (c0 < a.n_store) {
                MMLF_OOB(OOB_OUT, (long long)lo + 64 * nb + (long long)(16 * mb) * a.cs_out * 4 + 12 >= ob_left);
                __builtin_amdgcn_raw_buffer_store_b128(st, ob, lo + 64 * nb, (unsigned)(16 * mb) * a.cs_out * 4u, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (mask_out) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int j = 0; j < MW; ++j) a.relu_mask_out[mbase + 64 * (MW * mb + j)] = mw[mb][j];
    }
    if (a.out_amax) {
        const unsigned d0 = (unsigned)qb;                       // first destination position of the wave
        const unsigned rd0 = fastdiv(d0, a.divP);
        const int nfirst = (int)((rd0 + 1) * (unsigned)a.P - d0);   // wave positions [0, nfirst) lie in grid row rd0
        float m_lo = 0.f, m_hi = 0.f;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            if (16 * mb + r16 < nfirst) m_lo = fmaxf(m_lo, mk[mb]);
            else m_hi = fmaxf(m_hi, mk[mb]);
        }
        m_lo = mmlf_wave_max(m_lo);
        m_hi = mmlf_wave_max(m_hi);
        if (r16 + 16 * q4 == 0) {
            MMLF_OOB(OOB_AMAX, MMLF_AMAX_HEAD + (long long)fastdiv(d0 + 31, a.divP) >= a.amax_n);
            if (m_lo > 0.f) mmlf_amax_raise_nowait(a.out_amax + MMLF_AMAX_HEAD + rd0, m_lo);
            if (m_hi > 0.f) {
                const unsigned rdl = fastdiv(d0 + 31, a.divP);
                for (unsigned r = rd0 + 1; r <= rdl; ++r) mmlf_amax_raise_nowait(a.out_amax + MMLF_AMAX_HEAD + r, m_hi);
            }
            run_max = fmaxf(run_max, fmaxf(m_lo, m_hi));        // lane 0 carries the tensor maximum
        }
    }
}
// the workgroup's table of per-column weight-unscale and bias values (transposed epilogue), filled once per launch
template <int NP>
__device__ __forceinline__ void conv_fill_coef(const ConvArgs &a, float *coef, int tid, int nthreads)
{
    for (int k = tid; k < NP; k += nthreads) {
        coef[k] = a.w_unscale ? a.w_unscale[k] : 1.f;
        coef[NP + k] = (a.bias && k < a.n_true) ? a.bias[k] : 0.f;
    }
}

// f16 split: the power-of-two scale wave w of tile Q0 applies to its activation operand.  The wave's valid
// outputs q read in[q + {0, 1, P, P+1}], i.e. grid rows row(q0) .. row(q0 + 31) + 1 (no row is added behind a
// patch's last row: its outputs are never valid), so the scale comes from those rows' maxima alone: a wave's
// precision does not depend on what the rest of the tensor holds (neighbouring patches, far-away rows).
// Two halves so that the row loads of the NEXT tile fly during this tile's epilogue: gather (per-lane maximum of
// the rows lane, lane + 64, ... of the range) and finish (wave maximum -> scale).
__device__ __forceinline__ float wave_operand_amax_gather(const ConvArgs &a, long long Q0, int w, int lane)
{
    const long long q0 = Q0 + 32 * w;
    float m = 0.f;
    if (q0 < a.NQ) {                                             // wave-uniform; else nothing valid in this wave
        const long long ql = q0 + 31 < a.NQ ? q0 + 31 : a.NQ - 1;
        const unsigned r0 = fastdiv((unsigned)q0, a.divP);
        unsigned r1 = fastdiv((unsigned)ql, a.divP);
        r1 += (r1 - fastdiv(r1, a.divR) * (unsigned)a.R != (unsigned)(a.R - 1)) ? 1u : 0u;
        MMLF_OOB(OOB_AMAX, lane == 0 && MMLF_AMAX_HEAD + (long long)r1 >= a.amax_n);
        for (unsigned r = r0 + lane; r <= r1; r += 64) m = fmaxf(m, a.in_amax[MMLF_AMAX_HEAD + r]);
    }
    return m;
}
__device__ __forceinline__ float wave_operand_scale(float gathered)
{
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(pow2_scale_for(mmlf_wave_max(gathered)))));
}

// The launch arguments as stored in the kernel-argument segment, behind a pointer the optimiser cannot see through:
// what is read through it is loaded where it is used (scalar loads) instead of living in SGPRs across the main
// loop.  The persistent kernel's main loop needs a handful of arguments, its epilogue some twenty -- kept live,
// they push the loop's own scalars into spill lanes (0.3 ms of an 8 ms launch).
typedef const __attribute__((address_space(4))) ConvArgs *ConvKernArgs;
__device__ __forceinline__ ConvArgs late_args()
{
#if defined(__HIP_DEVICE_COMPILE__)
    ConvKernArgs p = (ConvKernArgs)__builtin_amdgcn_kernarg_segment_ptr();   // ConvArgs is the kernel's first parameter
    asm volatile("" : "+s"(p));
    return *p;
#else
    return ConvArgs();
#endif
}

// 512 threads = 8 waves; tile = 256 positions x 16*G output channels; wave w owns positions
// [32w, 32w+32) x all channels as 2 x G accumulator tiles of v_mfma_f32_16x16x32_bf16 (under the
// chip's power-limited clock this shape sustains more FLOP/s than 32x32x16: 217 vs 204 TFLOP/s
// algorithmic at 280->280).  K is walked in chunks of 8 input channels x 4 taps = one MFMA K (lane
// quarter q4 = lane>>4 carries tap q4), double-buffered in LDS and filled by LDS-DMA
// (global_load_lds_dwordx4: no staging registers; the copy of chunk c+1 is in flight while chunk c
// is multiplied).  Activations stay f32 in LDS and are split in registers; weights arrive pre-split
// from pack_filter_split_kernel as [chunk][plane(3)][tap(4)][NP][8 bf16].
// G <= 6 (narrow layers): VGPRs capped at 128 so that TWO workgroups share a CU -- with 60 short MFMAs
// per wave per chunk the DMA latency of a single double-buffered workgroup is exposed.
// G = number of 16-column output blocks (NP = 16*G packed columns): 2, 5 (the 70-channel layers: 80
// columns instead of 96), 6, 7, 8 or 18; 10, 12 and 16 are the column blocks of the layers wider than 288 (wide_np).
// PL = operand planes: 3 = bf16 3-way split, six passes ("bf16x6"); 2 = f16 2-way split of the scaled
// operands, three passes ("f16x3").
// NW = waves per workgroup = 32-position row groups per tile: 8 (256-position tiles) or, for the narrow layers on small
// pitches, 16 (512 positions, ONE workgroup per CU instead of two: the 99-position halo is 19 % of the window instead of
// 39 %, the weights are fetched once per 512 positions, and more activation bytes are in flight per CU -- these launches
// are bound by memory concurrency, not by the matrix cores).  Layouts (masks, statistics, scales) are indexed by the
// global 32-position group, so the two variants produce the same bytes.
// TR: transposed accumulator tiles and epilogue (conv_epilogue16_tr above).
constexpr int RING16 = 3;   // pipeline depth of the sixteen-wave variant (LDS: 30 KB per buffer + 20 KB; 4 measures the same)
template <int G, int PL, int EPI = EPI_GENERIC, int NW = 8, bool TR = false>
__global__ __launch_bounds__(64 * NW, (NW == 16 || G <= 6 ? 4 : 2)) void conv4tap_x6s_kernel(ConvArgs a, int ntiles)
{
    constexpr int NP = G * 16;
    constexpr int TILE = 32 * NW;
    // pipeline buffers: two; the sixteen-wave variant has the LDS for a ring of RING16, with the DMA of chunk
    // c + D - 1 issued during chunk c and a counted wait that leaves the newest D - 2 chunks' pieces in flight
    constexpr int D = NW == 16 ? RING16 : 2;
    // EARLY: the chunk's barrier stands two column blocks before its end (the weight fragments of those two blocks are
    // in registers by then): behind it the wave requests the NEXT chunk's activation and first weight fragments and runs
    // its last twelve MFMAs while they arrive -- the LDS latency of the chunk head (both waves of a SIMD stand in it at
    // once: 12 % of a 280-wide chunk by the wave's own clock) is off the critical path.  Needs G % 3 == 0 (the rotating
    // fragment slots line up across chunks) and enough column blocks behind the DMA issue for the pieces to land.
    constexpr bool EARLY = PL == 2 && G % 3 == 0 && G >= 9;   // (the three-plane build has no registers to spare for it)
    // A: [640 slots][channel half(2)] float4.  Slot s holds position Q0 + s (+ seg_delta for s >= 320).
    // When the pitch is small (P + 257 <= 640, e.g. 96x96 training patches) ONE contiguous window
    // Q0 .. Q0+256+P serves all four taps (taps 2,3 read at slot offset P): 355 positions per tile
    // instead of 2 x 257.  Otherwise two 320-slot segments (rows y and y+1) are loaded.
    // A DMA piece is 32 positions x 32 bytes: lanes 2i, 2i+1 fetch the two 16-byte halves of position i's chunk, ONE
    // 32-byte sector request for the memory pipeline (half-major pieces of 64 positions asked for every sector twice,
    // from two instructions; the 70-channel launches are bound by that request rate).
    constexpr int A_F4 = 2 * 640;
    constexpr int B_F4 = 4 * PL * NP;
    constexpr int BUF_F4 = A_F4 + B_F4;
    constexpr int N_B = B_F4 / 64;
    constexpr int PER_WAVE = (20 + N_B + NW - 1) / NW;   // upper bound (20 A pieces: two-segment mode, 512-position tiles)
    constexpr int PER_SLOT = (PER_WAVE + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *lds = reinterpret_cast<float4 *>(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q4 = lane >> 4;

    f32x4 acc[2][G];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < G; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mb][nb][r] = 0.f;

    // DMA addressing: a piece = wave-uniform 64-bit base (SGPRs) + one shared per-lane byte offset
    const unsigned voff_a = ((unsigned)(lane >> 1) * (unsigned)a.cs_in + 4u * (lane & 1)) * 4u;   // A pieces
    const unsigned voff_b = (unsigned)lane * 16u;                      // B pieces: linear
    const unsigned lds_base = (unsigned)(size_t)(lds_void_t *)smem;
    const char *in0 = reinterpret_cast<const char *>(a.in);
    const char *wp_base = reinterpret_cast<const char *>(a.wp);
    const size_t tile_bytes = (size_t)TILE * a.cs_in * 4;
    // Piece ownership, fixed for the launch: of the chunk's pieces j = 0 .. a_pieces + N_B - 1 (activation
    // pieces first) wave w issues j = w, w+8, ...: nA activation pieces, then nB weight pieces that are
    // 8 KiB apart in both the packed filter and LDS.  The first half of them goes out in slot 0.
    const int n_a = a.a_pieces;
    const int nA = (n_a - w + NW - 1) / NW;
    const int jb0 = w + NW * nA - n_a;
    const int nB = (N_B - jb0 + NW - 1) / NW;
    int n_mine = nA + nB;                                   // re-made opaque every chunk (see below)
    unsigned a_src[3], a_dst[3];                            // activation pieces: byte offset in the tile, LDS byte
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int j = w + NW * k;
        const int seg = j >= a.a_per_seg, idx = j - seg * a.a_per_seg;   // two-segment mode: 320-slot segments
        const int slot = 320 * seg + 32 * idx;
        a_src[k] = (unsigned)(slot + seg * a.seg_delta) * (unsigned)a.cs_in * 4u;
        // bit 0 marks the last piece of a window (of a segment): only its first a_tail positions are ever read; the
        // other lanes re-fetch the last of those instead of positions nobody uses
        a_dst[k] = (unsigned)slot * 32u + (idx == a.a_per_seg - 1 ? 1u : 0u);
    }
    const unsigned tail_lim = ((unsigned)(a.a_tail - 1) * (unsigned)a.cs_in + 4u) * 4u;
    const unsigned b_src0 = 1024u * jb0, b_dst0 = (unsigned)(A_F4 + 64 * jb0) * 16u;

#ifdef MMLF_BOUNDS_DEBUG      // the piece's last source byte against the buffer (the address is made scalar again for the asm)
#define MMLF_DMA_SRC_CHECK()                                                                             \
    do {                                                                                                 \
        MMLF_OOB(OOB_IN, (long long)(sb_ - in0) + vo_ + 16 > a.in_bytes);                                \
        const unsigned long long u_ = (unsigned long long)sb_;                                           \
        sb_ = reinterpret_cast<const char *>(                                                            \
            ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(u_ >> 32)) << 32) |           \
            (unsigned)__builtin_amdgcn_readfirstlane((unsigned)u_));                                     \
    } while (0)
#else
#define MMLF_DMA_SRC_CHECK() do { } while (0)
#endif
    // slot 0 = this wave's pieces k < PER_SLOT, slot 1 = the rest; k is a compile-time index
#define X6_DMA_PIECE(tl, c, buf, k)                                                                      \
    do {                                                                                                 \
        if ((k) < PER_WAVE && (k) < n_mine) {                                                            \
            const char *sb_;                                                                             \
            unsigned vo_, d_;                                                                            \
            if ((k) < nA) {                                                                              \
                sb_ = in0 + (size_t)(tl) * tile_bytes + 32u * (c) + a_src[(k) < 3 ? (k) : 0];            \
                d_ = a_dst[(k) < 3 ? (k) : 0];                                                           \
                vo_ = min(voff_a, (d_ & 1u) ? tail_lim : 0xffffffffu);                                   \
                d_ &= ~1u;                                                                               \
                MMLF_DMA_SRC_CHECK();                                                                    \
            } else {                                                                                     \
                const unsigned kb_ = (1024u * NW) * (unsigned)((k) - nA);                                \
                sb_ = wp_base + (size_t)(c) * (B_F4 * 16) + b_src0 + kb_;                                \
                vo_ = voff_b;                                                                            \
                d_ = b_dst0 + kb_;                                                                       \
            }                                                                                            \
            d_ = __builtin_amdgcn_readfirstlane(d_ + lds_base + (buf) * (BUF_F4 * 16));                  \
            unsigned keep_;                                                                              \
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"                       \
                         "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"                           \
                         : "=&s"(keep_) : "v"(vo_), "s"(sb_), "s"(d_) : "memory");                      \
        }                                                                                                \
    } while (0)
#define X6_DMA_SLOT(tl, c, buf, slot)                                                                    \
    do {                                                                                                 \
        _Pragma("unroll") for (int k_ = 0; k_ < PER_SLOT; ++k_)                                          \
            X6_DMA_PIECE(tl, c, buf, (slot) * PER_SLOT + k_);                                            \
    } while (0)
#define X6_DMA_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define X6_CHUNK_WAIT()                                                                                  \
    do {                                                                                                 \
        if (D > 2 && more) {      /* in-order counter: everything but this wave's newest (D - 2) x n_mine pieces has landed */ \
            static_assert(PER_WAVE <= 3 || D == 2, "counted waits are written for up to three pieces per wave");             \
            if (n_mine == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(1 * (D - 2)) : "memory");            \
            else if (n_mine == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (D - 2)) : "memory");       \
            else if (n_mine == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (D - 2)) : "memory");       \
            else X6_DMA_WAIT();                                                                          \
        } else {                                                                                         \
            X6_DMA_WAIT();                                                                               \
        }                                                                                                \
    } while (0)

    // Persistent over tiles: the chunk pipeline runs on across tile boundaries, so the DMA of the next
    // tile's first chunk is in flight while this tile's last chunk multiplies and its epilogue stores.
    // XCD-aware tile order: blocks b and b+8 share an XCD (one L2).  Give every XCD a CONTIGUOUS run of
    // tiles per sweep so that the halo rows two neighbouring tiles both read are served by one L2
    // (speed only: any placement computes the same result).
    const int per_xcd = (int)gridDim.x >> 3;
    const int first_tile = (gridDim.x & 7) == 0 ? (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3)
                                                : (int)blockIdx.x;
    int tile = first_tile, c = 0;          // chunk being multiplied
    int ntile = tile, nc = 0;              // chunk being fetched (one ahead)
    if (tile >= ntiles) return;
    // optional BatchNorm statistics of the output: per-wave double sums behind the two pipeline buffers
    // behind the pipeline buffers: the transposed epilogue's per-column table (TR), or the statistics' per-wave double sums
    float *coef = reinterpret_cast<float *>(lds + D * BUF_F4);               // [2][NP]
    double *stats_all = reinterpret_cast<double *>(lds + D * BUF_F4);        // [NW waves][NP][2]
    if constexpr (TR) conv_fill_coef<NP>(late_args(), coef, tid, 64 * NW);   // ordered by the barrier below
    else if (late_args().bn_partial)
        for (int k = tid; k < NW * NP * 2; k += 64 * NW) stats_all[k] = 0.0;
    // f16 split: operand scales (powers of two) and what undoes them in the epilogue
    float scale_a = 1.f, unscale_a = 1.f, run_max = 0.f;
    if constexpr (PL == 2) {
        scale_a = wave_operand_scale(wave_operand_amax_gather(late_args(), (long long)tile * TILE, w, lane));
        unscale_a = 1.f / scale_a;
    }
#pragma unroll
    for (int d = 0; d < D - 1; ++d) {
        if (ntile < ntiles) {
            X6_DMA_SLOT(ntile, nc, d, 0);
            X6_DMA_SLOT(ntile, nc, d, 1);
        }
        if (++nc == a.nchunk) { nc = 0; ntile += gridDim.x; }
    }
    X6_DMA_WAIT();
    __syncthreads();
    int buf = 0;
    float4 ra[2][2];                                           // activation fragments of the chunk about to be split
    bf16x8 bq[3][PL];                                          // rotating [slot][plane] weight fragments
    const int a_lane = 2 * (32 * w + r16 + (q4 & 1) + (q4 >> 1) * a.seg_slot);   // float4 index: + 32*mb + half
    const int b_lane = q4 * NP + r16;                                            // bf16x8 index: + pl*4*NP + 16*nb
    if constexpr (EARLY) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) ra[mb][hf] = lds[a_lane + 32 * mb + hf];
#pragma unroll
        for (int g0 = 0; g0 < 2; ++g0)
#pragma unroll
            for (int pl = 0; pl < PL; ++pl)
                bq[g0][pl] = (reinterpret_cast<const bf16x8 *>(lds + A_F4) + b_lane)[pl * 4 * NP + 16 * g0];
    }

    while (tile < ntiles) {
        // opaque to the optimiser: keeps the per-piece address terms derived from it from being hoisted out
        // of the persistent loop into (spilled) SGPRs; they are recomputed on the scalar unit instead
        asm volatile("" : "+s"(n_mine));
        const bool more = ntile < ntiles;
        const int fb = buf == 0 ? D - 1 : buf - 1;             // the buffer multiplied last: free for chunk c + D - 1
        const float4 *base = lds + buf * BUF_F4;
        const float4 *nbase = lds + (buf + 1 == D ? 0 : buf + 1) * BUF_F4;   // the next chunk's buffer
        // lane (r16, q4): row r16 of a 16-position block, tap q4 -> slot offset (q4&1) + (q4>>1)*seg_slot
        const float4 *ap = base + a_lane;                                                    // + 32*mb + half
        const bf16x8 *bp = reinterpret_cast<const bf16x8 *>(base + A_F4) + b_lane;           // + pl*4*NP + 16*nb
        const bf16x8 *bpn = reinterpret_cast<const bf16x8 *>(nbase + A_F4) + b_lane;
        const bool tile_end = c + 1 == a.nchunk;

        if constexpr (!EARLY) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) ra[mb][hf] = ap[32 * mb + hf];
#pragma unroll
            for (int g0 = 0; g0 < 2; ++g0)
#pragma unroll
                for (int pl = 0; pl < PL; ++pl) bq[g0][pl] = bp[pl * 4 * NP + 16 * g0];
        }
        bf16x8 asp[2][PL];                                     // [row block][plane] split activations
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            unsigned hh[4], mm[4], ll[4];
            if constexpr (PL == 3) {
                split3_pair(ra[mb][0].x, ra[mb][0].y, hh[0], mm[0], ll[0]);
                split3_pair(ra[mb][0].z, ra[mb][0].w, hh[1], mm[1], ll[1]);
                split3_pair(ra[mb][1].x, ra[mb][1].y, hh[2], mm[2], ll[2]);
                split3_pair(ra[mb][1].z, ra[mb][1].w, hh[3], mm[3], ll[3]);
                const u32x4_t vm = {mm[0], mm[1], mm[2], mm[3]};
                asp[mb][1] = __builtin_bit_cast(bf16x8, vm);
            } else {
                split2_pair_f16(ra[mb][0].x, ra[mb][0].y, scale_a, hh[0], ll[0]);
                split2_pair_f16(ra[mb][0].z, ra[mb][0].w, scale_a, hh[1], ll[1]);
                split2_pair_f16(ra[mb][1].x, ra[mb][1].y, scale_a, hh[2], ll[2]);
                split2_pair_f16(ra[mb][1].z, ra[mb][1].w, scale_a, hh[3], ll[3]);
            }
            const u32x4_t vh = {hh[0], hh[1], hh[2], hh[3]}, vl = {ll[0], ll[1], ll[2], ll[3]};
            asp[mb][0] = __builtin_bit_cast(bf16x8, vh);
            asp[mb][PL - 1] = __builtin_bit_cast(bf16x8, vl);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (EARLY && g == G - 2) {
                // every LDS read of this chunk has been requested (weights run two column blocks ahead): wait for them and
                // for the next chunk's DMA pieces, pass the barrier, then ask for the next chunk's activations
                X6_CHUNK_WAIT();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __syncthreads();
                if (!tile_end) {            // (at a tile's end they would live through the epilogue: requested behind it)
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                        for (int hf = 0; hf < 2; ++hf) ra[mb][hf] = (nbase + a_lane)[32 * mb + hf];
                }
            }
            if (g + 2 < G) {
#pragma unroll
                for (int pl = 0; pl < PL; ++pl) bq[(g + 2) % 3][pl] = bp[pl * 4 * NP + 16 * (g + 2)];
            } else if (EARLY && !tile_end) {   // behind the barrier: the next chunk's first two column blocks (G % 3 == 0)
#pragma unroll
                for (int pl = 0; pl < PL; ++pl) bq[(g + 2) % 3][pl] = bpn[pl * 4 * NP + 16 * (g + 2 - G)];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (more) {   // both slots of a wave in one go, as early as the buffer is free; the two waves of a SIMD apart
                if (w < NW / 2) {
                    if (g == 0) { X6_DMA_SLOT(ntile, nc, fb, 0); X6_DMA_SLOT(ntile, nc, fb, 1); }
                } else {
                    if (g == (PL == 2 && G >= 8 ? G / 8 : G / 4)) { X6_DMA_SLOT(ntile, nc, fb, 0); X6_DMA_SLOT(ntile, nc, fb, 1); }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // cross terms, small ones first; the two row blocks alternate so that consecutive MFMAs never
            // wait on each other's accumulator
#define X6_TERM(pa, pb)                                                                                      \
    _Pragma("unroll") for (int mb = 0; mb < 2; ++mb)                                                         \
        acc[mb][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(asp[mb][pa], bq[g % 3][pb], acc[mb][g], 0, 0, 0)
#define H2_TERM(pa, pb)                                                                                      \
    _Pragma("unroll") for (int mb = 0; mb < 2; ++mb)                                                         \
        acc[mb][g] = TR ? __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, bq[g % 3][pb]),   \
                                                                 __builtin_bit_cast(f16x8, asp[mb][pa]), acc[mb][g], 0, 0, 0) \
                        : __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, asp[mb][pa]),     \
                                                                 __builtin_bit_cast(f16x8, bq[g % 3][pb]), acc[mb][g], 0, 0, 0)
            if constexpr (PL == 3) {
                X6_TERM(2, 0);
                X6_TERM(0, 2);
                X6_TERM(1, 1);
                X6_TERM(1, 0);
                X6_TERM(0, 1);
                X6_TERM(0, 0);
            } else {
                H2_TERM(1, 0);
                H2_TERM(0, 1);
                H2_TERM(0, 0);
            }
#undef X6_TERM
#undef H2_TERM
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more && ++nc == a.nchunk) { nc = 0; ntile += gridDim.x; }
        // the next chunk's DMA pieces must have landed before the barrier; at a tile end wait for them
        // BEFORE the epilogue, so that its stores (same counter) stay in flight across the barrier
        if constexpr (!EARLY) X6_CHUNK_WAIT();
        if (++c == a.nchunk) {
            const ConvArgs e = late_args(); // epilogue-only arguments: loaded here, dead again at the barrier
            float next_amax = 0.f;          // the next tile's row maxima: loads in flight during the epilogue
            if constexpr (PL == 2)
                if (tile + (int)gridDim.x < ntiles)
                    next_amax = wave_operand_amax_gather(e, (long long)(tile + gridDim.x) * TILE, w, lane);
            if constexpr (TR)
                conv_epilogue16_tr<G, EPI>(e, acc, (long long)tile * TILE, w, r16, q4, unscale_a, run_max, coef);
            else
                conv_epilogue16<G, EPI>(e, acc, (long long)tile * TILE, w, r16, q4, unscale_a, run_max,
                                        e.bn_partial ? stats_all + (size_t)w * NP * 2 : nullptr);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < G; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[mb][nb][r] = 0.f;
            c = 0;
            tile += gridDim.x;
            if constexpr (PL == 2) {
                if (tile < ntiles) {
                    scale_a = wave_operand_scale(next_amax);
                    unscale_a = 1.f / scale_a;
                }
            }
            if constexpr (EARLY) {          // the next tile's first fragments (its chunk 0 passed the barrier above)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) ra[mb][hf] = (nbase + a_lane)[32 * mb + hf];
#pragma unroll
                for (int g0 = 0; g0 < 2; ++g0)
#pragma unroll
                    for (int pl = 0; pl < PL; ++pl) bq[g0][pl] = bpn[pl * 4 * NP + 16 * g0];
            }
        }
        if constexpr (!EARLY) __syncthreads();
        buf = buf + 1 == D ? 0 : buf + 1;
    }
    if constexpr (EARLY) __syncthreads();                       // orders the last tile's wave sums
    const ConvArgs e = late_args();
    if (e.out_amax) mmlf_amax_update(run_max, e.out_amax, blockIdx.x * NW + w);      // one atomic per wave per launch
    if (e.bn_partial) {                                         // the loop's last barrier ordered the wave sums
        for (int k = tid; k < 2 * e.n_true; k += 64 * NW) {
            const int ch = k % e.n_true, which = k / e.n_true;
            double t = 0.0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) t += stats_all[((size_t)ww * NP + ch) * 2 + which];
            e.bn_partial[((size_t)blockIdx.x * 2 + which) * e.bn_stride + ch] = t;
        }
    }
#undef X6_DMA_PIECE
#undef MMLF_DMA_SRC_CHECK
#undef X6_DMA_SLOT
#undef X6_DMA_WAIT
#undef X6_CHUNK_WAIT
}



// ---------------------------------------------------------------------------------------------
// Narrow layers, f16 split, round 4: conv4tap_rs_kernel -- "register-streamed".  The stream layers (27 -> 70, 70 -> 70:
// reference feed_forward.py:139-157) have K = 4 x 72 at most and 80 packed columns: 30 MFMAs per wave and 8-channel
// chunk, against which the tiled kernel's per-chunk costs (barrier, chunk head, DMA wait: half of its time by the wave's
// own clock) do not amortise, and whose 355- / 611-position windows come from HBM 1.4-1.5 times.  Here
//  * the WHOLE packed filter (NCH x 10 KB, 92 KB at 72 channels) is copied into LDS once per workgroup and stays;
//  * a wave owns a 32-position group at a time, end to end: every lane loads the full channel row of its (position, tap)
//    straight into registers -- 2 x NCH 16-byte loads per row block, consecutive bytes per lane, issued in one burst so
//    that a 128-byte line is touched by eight back-to-back instructions -- multiplies, runs the common epilogue, moves on;
//  * no LDS traffic for activations, no DMA, NO barrier in the loop: the two waves of a SIMD drift apart by themselves,
//    one multiplies while the other waits for its loads and stores (counted vmcnt waits per chunk: loads return in order);
//  * groups are dealt so that the waves of one XCD work on neighbouring groups at any time: the row a group reads as
//    taps 2, 3 is the row three groups further on read as taps 0, 1 -- an L2 hit instead of a second HBM read.
// Layouts (mask words, statistics, amax, scales) are indexed by the global 32-position group exactly as in
// conv4tap_x6s_kernel (tile = group / 8, wave = group % 8): the two kernels write the same bytes.
// ---------------------------------------------------------------------------------------------
template <int G, int NCH, int EPI, bool TR = false>
__global__ __launch_bounds__(512, 2) void conv4tap_rs_kernel(ConvArgs a, int ngroups)
{
    constexpr int NP = G * 16;
    constexpr int WBYTES = NCH * 2 * 4 * NP * 16;            // [chunk][plane][tap][NP][8 f16]
    // K order.  A "full" MFMA step is ONE tap x 32 channels: lane quarter q4 carries channel octet q4 of the step, so the
    // four lanes of a position read 128 consecutive bytes of its row (one or two cache lines per position and
    // instruction; with quarter = tap, as in the tiled kernel's LDS image, every lane of a load instruction sits in
    // another line and the L1 tag rate, one line per clock, made the loads cost as much as a full HBM stream).  The
    // channels left over (NCH % 4 == 1: 64..71 of 72) form one last step in the quarter = tap layout.  The packed filter
    // needs no other layout: a lane's fragment of step (tap t, octets 4s .. 4s+3) is chunk 4s + q4 of tap t.
    constexpr int NS = NCH / 4, REM = NCH % 4;
    static_assert(REM == 0 || REM == 1, "input channels: a multiple of 32, or one octet more");
    constexpr int NSTEP = 4 * NS + REM, NLOAD = 4 * NSTEP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q4 = lane >> 4;

    for (int o = tid * 16; o < WBYTES; o += 512 * 16)
        *reinterpret_cast<uint4 *>(smem + o) = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(a.wp) + o);
    float *coef = reinterpret_cast<float *>(smem + WBYTES);                   // transposed epilogue: [2][NP]
    double *stats_all = reinterpret_cast<double *>(smem + WBYTES);            // statistics: [8 waves][NP][2]
    if constexpr (TR) conv_fill_coef<NP>(a, coef, tid, 512);
    else if (a.bn_partial)
        for (int k = tid; k < 8 * NP * 2; k += 512) stats_all[k] = 0.0;
    __syncthreads();

    // this wave's groups: XCD x (blocks b with b % 8 == x share it) takes the contiguous range [x * per, (x + 1) * per);
    // inside it the XCD's waves stride together
    int gi, gstep, gend;
    if ((gridDim.x & 7) == 0) {
        const int per = (ngroups + 7) >> 3, nbx = (int)gridDim.x >> 3;
        const int x = (int)blockIdx.x & 7;
        gi = x * per + ((int)blockIdx.x >> 3) * 8 + w;
        gstep = nbx * 8;
        gend = min(ngroups, (x + 1) * per);
    } else {
        gi = (int)blockIdx.x * 8 + w;
        gstep = (int)gridDim.x * 8;
        gend = ngroups;
    }

    f32x4 acc[2][G];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < G; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mb][nb][r] = 0.f;
    float run_max = 0.f;
    const bf16x8 *bpF = reinterpret_cast<const bf16x8 *>(smem) + q4 * 8 * NP + r16;   // full steps: + (8 s + pl) * 4 NP + t NP + 16 nb
    const bf16x8 *bpR = reinterpret_cast<const bf16x8 *>(smem) + q4 * NP + r16;       // last step:  + (8 NS + pl) * 4 NP + 16 nb
    auto bfrag = [&](int k, int nb, int pl) -> bf16x8 {        // k, nb, pl are compile-time after unrolling
        return k < 4 * NS ? bpF[(8 * (k % NS) + pl) * 4 * NP + (k / NS) * NP + 16 * nb] : bpR[(8 * NS + pl) * 4 * NP + 16 * nb];
    };
    const size_t row_off = (size_t)r16 * a.cs_in;                                     // floats
    const size_t rem_off = (size_t)((q4 & 1) + (q4 >> 1) * a.P) * a.cs_in + 32 * NS;

    for (; gi < gend; gi += gstep) {
        const long long Q0 = (long long)(gi >> 3) * MMLF_TILE;
        const int wv = gi & 7;
        // row maxima first (their loads are the oldest: the first counted wait below covers them)
        const float gathered = wave_operand_amax_gather(a, Q0, wv, lane);
        const float *p0 = a.in + (size_t)(Q0 + 32 * wv) * a.cs_in + row_off;
        float4 raw[NSTEP][2][2];                                   // [step][row block][half]
#pragma unroll
        for (int k = 0; k < NSTEP; ++k) {
            const int t = k / NS, s_ = k % NS;                         // (full steps)
            const float *pk = k < 4 * NS ? p0 + (size_t)((t & 1) + (t >> 1) * a.P) * a.cs_in + 32 * s_ + 8 * q4 : p0 + rem_off;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf)
                {
                    MMLF_OOB(OOB_IN, (long long)((pk + (size_t)(16 * mb) * a.cs_in + 4 * hf + 4) - a.in) * 4 > a.in_bytes);
                    raw[k][mb][hf] = reinterpret_cast<const float4 *>(pk + (size_t)(16 * mb) * a.cs_in)[hf];
                }
            __builtin_amdgcn_sched_barrier(0);          // step order: the counted waits below rely on it
        }
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLOAD > 63 ? 63 : NLOAD) : "memory");
        const float scale_a = wave_operand_scale(gathered);
        const float unscale_a = 1.f / scale_a;
        bf16x8 bq[3][2];
#pragma unroll
        for (int g0 = 0; g0 < 2; ++g0)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) bq[g0][pl] = bfrag(0, g0, pl);
#pragma unroll
        for (int k = 0; k < NSTEP; ++k) {
            // loads come back in order: step k's four are done once at most 4 (NSTEP - 1 - k) younger ones are outstanding
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (NSTEP - 1 - k) > 63 ? 63 : 4 * (NSTEP - 1 - k)) : "memory");
            bf16x8 asp[2][2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                unsigned hh[4], ll[4];
                float4 &r0 = raw[k][mb][0], &r1 = raw[k][mb][1];
                asm volatile("" : "+v"(r0.x), "+v"(r0.y), "+v"(r0.z), "+v"(r0.w), "+v"(r1.x), "+v"(r1.y), "+v"(r1.z), "+v"(r1.w));
                split2_pair_f16(r0.x, r0.y, scale_a, hh[0], ll[0]);
                split2_pair_f16(r0.z, r0.w, scale_a, hh[1], ll[1]);
                split2_pair_f16(r1.x, r1.y, scale_a, hh[2], ll[2]);
                split2_pair_f16(r1.z, r1.w, scale_a, hh[3], ll[3]);
                const u32x4_t vh = {hh[0], hh[1], hh[2], hh[3]}, vl = {ll[0], ll[1], ll[2], ll[3]};
                asp[mb][0] = __builtin_bit_cast(bf16x8, vh);
                asp[mb][1] = __builtin_bit_cast(bf16x8, vl);
            }
            // The split is inline assembly: the compiler's hazard recognizer does not see a vector write in front of the
            // matrix instruction that reads it (VALU write -> MFMA source read needs wait states), and its scheduler is
            // free to put an MFMA between the two row blocks' splits.  Fenced on both sides: without the fences the nop
            // moved up and column block 0 of whichever row block was split last came out with wrong low bits.
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 4" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                constexpr int NB = NSTEP * G;
                const int idx = k * G + g;                      // block index in the (step, column block) stream
                if (idx + 2 < NB) {
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) bq[(idx + 2) % 3][pl] = bfrag((idx + 2) / G, (idx + 2) % G, pl);
                }
#define RS_TERM(pa, pb)                                                                                      \
    _Pragma("unroll") for (int mb = 0; mb < 2; ++mb)                                                         \
        acc[mb][g] = TR ? __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, bq[idx % 3][pb]), \
                                                                 __builtin_bit_cast(f16x8, asp[mb][pa]), acc[mb][g], 0, 0, 0) \
                        : __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, asp[mb][pa]),     \
                                                                 __builtin_bit_cast(f16x8, bq[idx % 3][pb]), acc[mb][g], 0, 0, 0)
                RS_TERM(1, 0);
                RS_TERM(0, 1);
                RS_TERM(0, 0);
#undef RS_TERM
            }
        }
        // (round 4 also measured this epilogue with ROW stores -- values through a wave-private LDS image, 16-byte stores of
        // consecutive addresses, 1 KB per wave instruction instead of 64-byte segments: 0.96-1.0 ms either way, removed)
        if constexpr (TR)
            conv_epilogue16_tr<G, EPI>(a, acc, Q0, wv, r16, q4, unscale_a, run_max, coef);
        else
            conv_epilogue16<G, EPI>(a, acc, Q0, wv, r16, q4, unscale_a, run_max,
                                    a.bn_partial ? stats_all + (size_t)w * NP * 2 : nullptr);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < G; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[mb][nb][r] = 0.f;
    }
    if (a.out_amax) mmlf_amax_update(run_max, a.out_amax, blockIdx.x * 8 + w);      // one atomic per wave per launch
    if (a.bn_partial) {
        __syncthreads();                                        // orders the waves' sums
        for (int k = tid; k < 2 * a.n_true; k += 512) {
            const int ch = k % a.n_true, which = k / a.n_true;
            double t = 0.0;
#pragma unroll
            for (int ww = 0; ww < 8; ++ww) t += stats_all[((size_t)ww * NP + ch) * 2 + which];
            a.bn_partial[((size_t)blockIdx.x * 2 + which) * a.bn_stride + ch] = t;
        }
    }
}

// Exact-f32 forward / data-gradient kernels of both filter sizes: one body on KS = 2 (conv4tap_kernel, taps
// {0, 1, P, P+1}) or 3 (conv9tap_kernel, taps dy*P + dx with dy, dx in {0, 1, 2}).
// 512 threads = 8 waves; tile = 256 positions x NT*32 output channels; wave w owns positions
// [32w, 32w+32) x all channels (NT accumulator tiles of 32x32).  K is walked in chunks of 8 input
// channels x KS*KS taps, double-buffered in LDS and filled by LDS-DMA (global_load_lds_dwordx4: no
// staging registers; the copy of chunk c+1 is in flight while chunk c is multiplied):
//   A (activations): [dy(KS)][kh(2)][320] float4  -- rows dy of the window, positions Q0 + dy*P + 0 .. 255 + KS-1
//   B (weights)    : [tap(KS*KS)][kh(2)][NP] float4
// One DMA wave-instruction ("piece") writes 64 consecutive float4 slots (1 KiB); its per-lane SOURCE
// address does the gather (A: one position per lane; B: linear).  A lane (i = lane&31, kh = lane>>5)
// reads ONE float4 = channels 4kh..4kh+3 of its position (A) or of its output channel (B): four K=2
// MFMA steps pairing channel s of half 0 with 4+s of half 1.
// Column blocks: the workgroup computes block `cb` of `ncb` blocks of NP columns of a filter packed np_total = ncb*NP
// columns wide (blockIdx.x = tile*ncb + cb, so the column blocks of a tile run side by side and share its activation
// window in L2).  The 2x2 launch has one block.  LDS budget of 3x3: 9 taps of B at 288 columns plus the 3-row window,
// double-buffered, would be 227 KB (160 KiB per CU), so the columns per workgroup are bounded instead: NT <= 4 (<= 132 KiB
// double-buffered), 288 columns as three blocks of 96.  Single-buffering B would keep 288 columns per workgroup but expose
// the weight DMA once per chunk.
template <int KS, int NT>
struct ConvF32Lds {                                 // LDS layout of one pipeline buffer, in float4 (body and launcher)
    static constexpr int A_STRIDE = 320;            // slots per (dy, kh) array: 5 DMA pieces (256 + KS - 1 used)
    static constexpr int A_F4 = 2 * KS * A_STRIDE;
    static constexpr int B_F4 = KS * KS * 2 * NT * 32;
    static constexpr int BUF_F4 = A_F4 + B_F4;
    static constexpr size_t BYTES = 2 * BUF_F4 * sizeof(float4);
    static_assert(BYTES <= 160 * 1024, "exact-f32 convolution kernel: LDS per CU");
};

template <int KS, int NT>
__device__ __forceinline__ void conv_f32_taps(const ConvArgs &a, const int ncb, const int np_total)
{
    using L = ConvF32Lds<KS, NT>;
    constexpr int TAPS = KS * KS;
    constexpr int WIN = 256 + KS - 1;           // positions of a window row
    constexpr int NP = NT * 32;
    constexpr int A_STRIDE = L::A_STRIDE, A_F4 = L::A_F4, B_F4 = L::B_F4, BUF_F4 = L::BUF_F4;
    constexpr int N_A = 10 * KS;                // DMA pieces for A per chunk
    constexpr int N_PIECES = N_A + B_F4 / 64;   // + B pieces
    constexpr int PER_WAVE = (N_PIECES + 7) / 8;
    static_assert(B_F4 % 64 == 0 && PER_WAVE <= (KS == 2 ? 2 : 1) * TAPS,
                  "piece schedule: piece k of a wave is issued at tap k (2x2: k = t and t + 4)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *lds = reinterpret_cast<float4 *>(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, kh = lane >> 5;
    const int tile = blockIdx.x / ncb, cb = blockIdx.x - tile * ncb;
    const long long Q0 = (long long)tile * MMLF_TILE;

    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    // per-lane DMA sources of this wave's pieces j = w, w+8, ...; chunk c adds c*step floats.
    // Destinations (float4 slot index inside a buffer) are wave-uniform.
    const float *src[PER_WAVE];
    int dst_f4[PER_WAVE];
    int step[PER_WAVE];
#pragma unroll
    for (int k = 0; k < PER_WAVE; ++k) {
        const int j = w + 8 * k;
        if (j < N_A) {
            const int arr = j / 5, blk = j - 5 * arr;           // arr = dy*2 + kh
            int p = 64 * blk + lane;
            p = p < WIN ? p : WIN - 1;                           // lanes past the window re-read its last position
            src[k] = a.in + (size_t)(Q0 + (arr >> 1) * a.P + p) * a.cs_in + 4 * (arr & 1);
            dst_f4[k] = arr * A_STRIDE + 64 * blk;
            step[k] = 8;
        } else {
            const int b = (j < N_PIECES ? j : N_PIECES - 1) - N_A;
            const int s = 64 * b + lane, tk = s / NP;           // tk = tap*2 + kh: the row of the packed chunk
            // column cb*NP + (s - tk*NP) of row tk, written so that one column block (np_total == NP, cb == 0) is the
            // linear s without a division
            src[k] = a.wp + (size_t)(s + tk * (np_total - NP) + cb * NP) * 4;
            dst_f4[k] = A_F4 + 64 * b;
            step[k] = TAPS * 2 * np_total * 4;
        }
    }
    const unsigned lds_base = (unsigned)(size_t)(lds_void_t *)smem;

    // One LDS-DMA piece.  Inline asm: with the builtin, hipcc drains vmcnt(0) before every LDS read
    // that might alias the in-flight copy; completion is awaited by hand before the barrier.
#define CONV_DMA_PIECE(c, buf, k)                                                                 \
    do {                                                                                          \
        if ((k) < PER_WAVE && w + 8 * (k) < N_PIECES) {                                           \
            const float *g_ = src[k] + (size_t)(c) * step[k];                                     \
            const unsigned d_ = lds_base + (unsigned)(((buf) * BUF_F4 + dst_f4[k]) * 16);         \
            unsigned keep_;                                                                       \
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"                \
                         "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"                   \
                         : "=&s"(keep_) : "v"(g_), "s"(d_) : "memory");                          \
        }                                                                                         \
    } while (0)
#define CONV_DMA_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

#pragma unroll
    for (int k = 0; k < PER_WAVE; ++k) CONV_DMA_PIECE(0, 0, k);
    CONV_DMA_WAIT();
    __syncthreads();

    for (int c = 0; c < a.nchunk; ++c) {
        const int buf = c & 1;
        const bool more = c + 1 < a.nchunk;
        const float4 *base = lds + buf * BUF_F4;
        const float4 *ap = base + kh * A_STRIDE + 32 * w + i;
        const float4 *bp = base + A_F4 + kh * NP + i;
        // Software pipeline over the taps: ALL fragment reads of tap t+1 are issued, then the 4*NT
        // MFMAs of tap t run back to back while those reads land (sched_barrier pins the regions;
        // left alone, hipcc sinks each read to just before its first use).  The DMA pieces of chunk
        // c+1 are spread over the taps (a wave's piece k at tap k; 2x2 has fewer taps than a wave has
        // pieces: k = t and t + 4), and the two waves that share a SIMD (w, w+4) issue theirs at
        // different points of the MFMA stream.  MFMAs stay accumulator-major (4 dependent K=2 steps
        // per accumulator): measured faster here than the independent order.
        float4 a_cur = ap[0], b_cur[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b_cur[nt] = bp[32 * nt];
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            float4 a_nxt = a_cur, b_nxt[NT];
            if (t < TAPS - 1) {
                const int dy = (t + 1) / KS, dx = (t + 1) - KS * dy;
                a_nxt = ap[dy * 2 * A_STRIDE + dx];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) b_nxt[nt] = bp[(t + 1) * 2 * NP + 32 * nt];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (more && w < 4) { CONV_DMA_PIECE(c + 1, buf ^ 1, t); if (KS == 2) CONV_DMA_PIECE(c + 1, buf ^ 1, t + TAPS); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                if (nt == NT / 2) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (more && w >= 4) { CONV_DMA_PIECE(c + 1, buf ^ 1, t); if (KS == 2) CONV_DMA_PIECE(c + 1, buf ^ 1, t + TAPS); }
                    __builtin_amdgcn_sched_barrier(0);
                }
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.x, b_cur[nt].x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.y, b_cur[nt].y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.z, b_cur[nt].z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.w, b_cur[nt].w, acc[nt], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (t < TAPS - 1) {
                a_cur = a_nxt;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) b_cur[nt] = b_nxt[nt];
            }
        }
        CONV_DMA_WAIT();   // this wave's pieces of chunk c+1 have landed ...
        __syncthreads();   // ... and so have everyone else's; all reads of buffer `buf` are done
    }
#undef CONV_DMA_PIECE
#undef CONV_DMA_WAIT

    // this column block's slice of the output channels: the shared epilogue on shifted pointers
    ConvArgs e = a;
    const int c0 = cb * NP;
    e.out = a.out + c0;
    e.out_bytes = a.out_bytes - 4ll * c0;
    e.bias = a.bias ? a.bias + c0 : nullptr;
    if (a.ref) { e.ref = a.ref + c0; e.ref_bytes = a.ref_bytes - 4ll * c0; }
    e.n_store = a.n_store - c0;
    e.n_true = a.n_true - c0;
    conv_epilogue<NT>(e, acc, Q0, w, i, kh);
}

template <int NT>
__global__ __launch_bounds__(512) void conv4tap_kernel(ConvArgs a)
{
    conv_f32_taps<2, NT>(a, 1, NT * 32);
}

template <int NT>
__global__ __launch_bounds__(512) void conv9tap_kernel(ConvArgs a, int ncb, int np_total)
{
    conv_f32_taps<3, NT>(a, ncb, np_total);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int mmlf_conv_cus(void) { return device_cus(); }

// exact-f32 packed filters of both sizes (ks = 2 or 3): [chunk][tap(ks*ks)][kh(2)][NP][4] floats
// packed columns of the exact-f32 kernels: pick_nt's 32-column tiles, and for 2x2 filters the column blocks above 288
static inline int f32_np(int ks, int N)
{
    const int nt = pick_nt(N);
    return nt > 0 ? nt * 32 : (ks == 2 ? wide_np(N) : -1);
}
// Packed column count NP of the split forward/dgrad kernels: 32, 80, then 16-column granularity up to
// 128, then 288; above that the column blocks of wide_np.  Packing and launch pick by this one rule, so the layouts always agree.
static inline int x6_np(int N)
{
    if (N > MMLF_MAX_N) return wide_np(N);
    if (N <= 0) return -1;
    if (N <= 32) return 32;
    if (N <= 80) return 80;
    if (N <= 128) return (N + 15) / 16 * 16;
    return 288;
}

// The sixteen-wave variant (512-position tiles) serves the 80-column f16 kernels on pitches whose 513 + P position
// window fits the 640-slot activation buffer (MMLF_CONV_NW16=0 turns it off).
static bool conv_sixteen_waves(int planes, int np, const Grid &g)
{
    static const int on = [] { const char *e = getenv("MMLF_CONV_NW16"); return e ? atoi(e) : 1; }();
    return on && planes == 2 && np == 80 && g.P + 513 <= 640;
}
// the register-streamed narrow kernel (conv4tap_rs_kernel) serves 80 packed columns over 4 or 9 input chunks (27 -> 70,
// 70 -> 70) in the f16 split.
// Where it runs (measured, profiles/r04_ab_bench_rs.log): on 96x96 training patches the two kernels take the same time
// (0.94 ms per 70 -> 70 launch at bs=512 either way; whole step 1122-1127 patches/s both), so the tiled sixteen-wave
// kernel keeps those launches; on pitches where that variant's 512 + P position window does not fit (full frames: the
// 70 members of a 512x512 ESE scene) the tiled kernel falls back to eight waves and two window segments, and the
// register-streamed kernel is 4.7 % faster end to end (0.436 vs 0.457 s per scene).  MMLF_CONV_RS=1 / 0 forces it on /
// off for every eligible launch (A/B).
static bool conv_rs_shape(int planes, int np, int nchunk, int nw)
{
    static const int mode = [] { const char *e = getenv("MMLF_CONV_RS"); return e ? atoi(e) : -1; }();
    if (!(planes == 2 && np == 80 && (nchunk == 9 || nchunk == 4))) return false;
    return mode < 0 ? nw == 8 : mode != 0;
}

// ---------------------------------------------------------------------------------------------
// The launch plan of a 2x2 convolution: everything about one launch of a layer that follows from (arithmetic path, input
// channel stride, N, B, H, W) -- computed HERE and nowhere else.  The entry points copy it into ConvArgs and launch by it,
// the size queries return its figures (mmlf_conv2x2_blocks: `blocks`, the rows of bn_partial; mmlf_packed_filter_*: the
// bytes), and the bounds audit (mmlf_audit_conv_h2) derives every end from its fields, so what the audit certifies is the
// launch itself.
// How the fetched positions follow (positions are grid positions q; a buffer of channel stride cs holds alloc = NQpad + P +
// 72 of them): the activation window of the LAST tile (first position NQpad - tile) is one contiguous window of tile + 1 + P
// positions when that fits the 640 slots, else two 320-slot segments (rows y and y + 1) of 257 positions each, the second
// one seg_delta + 320 further on; either way it ends at position NQpad + P.  The last piece of a window / segment fetches
// a_tail positions only, the other lanes re-fetch the last of those.  The register-streamed kernel reads positions
// Q0 + 32 w + 16 mb + r16 + {0, 1, P, P + 1} for every position of the padded grid: the same end.
// A layer wider than 288 columns is ncb = 2 launches of this kind on column blocks (wide_np): the same tiles, windows and
// workgroup count each, the packed filter's blocks back to back.
// ---------------------------------------------------------------------------------------------
constexpr int CONV_A_SLOTS = 640, CONV_SEG_SLOTS = 320;   // activation slots of conv4tap_x6s_kernel's LDS buffer; of a segment
struct ConvPlan {
    Grid g;
    int np, ncb, npb, G;          // packed columns of the layer; column blocks (a launch each); columns, 16-column groups of one
    int nw, tile;                 // waves per workgroup (8 or 16) and the positions of their tile
    bool rs;                      // the register-streamed kernel runs the launch
    int a_pieces, a_per_seg, a_tail, seg_slot, seg_delta;   // the tiled split kernels' activation window, as in ConvArgs
    long long ntiles, ngroups;    // tiles, 32-position groups of the padded grid
    int blocks;                   // workgroups of a launch (persistent: each walks tiles / groups b, b + blocks, ...)
    size_t block_bytes;           // packed filter of one column block ...
    long long unscale_off;        // ... and where behind its planes the columns' unscale factors start (f16 split; else -1)
    long long last_in;            // last activation position a launch fetches (split paths)
};
// planes: 2 = f16 split, 3 = bf16 split, 0 = exact f32 (256-position tiles, one workgroup each; no window of this kind).
// False: no such launch (what the entry points' argument checks refuse by name).
static bool conv_plan(int planes, int cs_in, int N, int B, int H, int W, ConvPlan &p)
{
    p = {};
    const Grid &g = p.g = make_grid(B, H, W);
    p.np = planes ? x6_np(N) : f32_np(2, N);
    if (p.np <= 0 || cs_in <= 0 || B <= 0 || H <= 0 || W <= 0) return false;
    const int nchunk = cs_in / 8, cus = device_cus();
    p.ncb = col_blocks(p.np); p.npb = p.np / p.ncb; p.G = p.npb / 16;
    p.nw = conv_sixteen_waves(planes, p.npb, g) ? 16 : 8;
    p.tile = 32 * p.nw;
    p.ntiles = g.NQpad / p.tile; p.ngroups = g.NQpad / 32;
    p.rs = conv_rs_shape(planes, p.npb, nchunk, p.nw);
    if (!planes) {
        p.blocks = (int)p.ntiles;
        p.block_bytes = packed_f32_block_floats(4, nchunk, p.npb) * sizeof(float);
        p.unscale_off = -1;
        return true;
    }
    const int span = g.P + p.tile + 1;
    if (span <= CONV_A_SLOTS) {   // one contiguous window of tile + 1 + P positions
        p.a_pieces = p.a_per_seg = (span + 31) / 32; p.seg_slot = g.P; p.seg_delta = 0;
    } else {                      // two segments: rows y and y+1, positions Q0 .. Q0 + 256 of each
        p.a_per_seg = (MMLF_TILE + 1 + 31) / 32; p.a_pieces = 2 * p.a_per_seg; p.seg_slot = CONV_SEG_SLOTS; p.seg_delta = g.P - CONV_SEG_SLOTS;
    }
    p.a_tail = (p.seg_delta ? MMLF_TILE + 1 : span) - 32 * (p.a_per_seg - 1);
    // persistent launches: one workgroup per CU (two for the narrow eight-wave variants); the register-streamed kernel's
    // workgroups take eight groups at a time
    const long long grid = p.rs ? cus : (p.G <= 6 && p.nw == 8 ? 2ll : 1ll) * cus, work = p.rs ? (p.ngroups + 7) / 8 : p.ntiles;
    p.blocks = (int)(grid > work ? work : grid);
    p.block_bytes = packed_split_block_bytes(planes, nchunk, p.npb);
    p.unscale_off = planes == 2 ? (long long)packed_split_planes_bytes(planes, nchunk, p.npb) : -1;
    const int seg = p.a_pieces / p.a_per_seg - 1;      // the segment of the window's last piece
    p.last_in = p.rs ? g.NQpad - 1 + g.P + 1
                     : (g.NQpad - p.tile) + seg * (CONV_SEG_SLOTS + p.seg_delta) + 32 * (p.a_per_seg - 1) + p.a_tail - 1;
    return true;
}
// (the byte figures do not depend on the frame)
static int64_t packed_filter_bytes(int planes, int K, int N)
{
    ConvPlan p;
    if (K <= 0 || !conv_plan(planes, (K + 7) / 8 * 8, N, 1, 1, 1, p)) return -1;
    return (int64_t)p.ncb * p.block_bytes;
}
static int64_t packed_filter_f32_floats(int ks, int K, int N)
{
    if (ks == 2) return packed_filter_bytes(0, K, N) < 0 ? -1 : packed_filter_bytes(0, K, N) / 4;
    const int np = f32_np(ks, N);      // (3x3: ONE launch walks its column blocks, conv9_shape)
    if (np < 0 || K <= 0) return -1;
    return (int64_t)packed_f32_block_floats(ks * ks, (K + 7) / 8, np);
}

static int pack_filter_f32(const char *who, int ks, const float *w, float *packed, int Cout, int Cin, int variant,
                           int dgrad, void *stream)
{
    MMLF_CHECK_ARG(w && packed, "%s: null pointer", who);
    MMLF_CHECK_ARG(variant >= 0 && variant <= 2, "%s: bad variant %d", who, variant);
    MMLF_CHECK_ARG(Cout > 0 && Cin > 0, "%s: bad channels %d x %d", who, Cout, Cin);
    const int K = dgrad ? Cout : Cin, N = dgrad ? Cin : Cout;
    const int NP = f32_np(ks, N);
    MMLF_CHECK_ARG(NP > 0, "%s: N=%d not supported (max %d)", who, N, ks == 2 ? MMLF_MAX_N_WIDE : MMLF_MAX_N);
    const int nchunk = (K + 7) / 8;
    const long long total = (long long)packed_f32_block_floats(ks * ks, nchunk, NP);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(ks == 2 ? pack_filter_f32_kernel<2> : pack_filter_f32_kernel<3>, dim3(blocks), dim3(256), 0,
                       (hipStream_t)stream, w, packed, Cout, Cin, variant, dgrad, nchunk, NP);
    return mmlf_launch_status(who);
}

extern "C" int64_t mmlf_packed_filter_floats(int K, int N) { return packed_filter_f32_floats(2, K, N); }

extern "C" int mmlf_pack_filter(const float *w, float *packed, int Cout, int Cin, int variant, int dgrad,
                                void *stream)
{
    return pack_filter_f32("mmlf_pack_filter", 2, w, packed, Cout, Cin, variant, dgrad, stream);
}

// What the ABI's contract says the caller's buffers hold (bytes behind the pointers as passed), alloc = the positions the
// grid's allocation rule gives them.  `out` may be a channel slice of a wider buffer (out = base + c_off with c_off +
// N_store <= cs_out): the bound below is what is left behind the LARGEST such offset, so it never cuts a store the
// contract allows and never exceeds the allocation.
static void conv_buffer_bytes(ConvArgs &a, const Grid &g, long long alloc)
{
    a.out_bytes = (alloc * a.cs_out - (a.cs_out - a.n_store)) * 4;
    a.ref_bytes = a.ref ? alloc * a.cs_ref * 4 : 0;
    a.in_bytes = alloc * a.cs_in * 4;
    a.amax_n = amax_entries(g);
    a.mask_words = g.NQpad / MMLF_TILE * 4096;
}

// The argument checks and the ConvArgs fields that every forward / data-gradient entry point shares.  who = the entry
// point as the caller named it, ks = filter size (window slack: taps reach (ks-1)(P+1) past a tile), np = packed columns
// by the path's own rule (<= 0: N not supported), g = make_grid(B, H, W).
static int conv_common_args(const char *who, int ks, int np, ConvArgs &a, const Grid &g, const float *in, int cs_in, int K,
                            const void *packed, const float *bias, int N, float *out, int cs_out, int N_store,
                            int out_shift, int vh, int vw, int B, int H, int W, int relu, const float *relu_ref, int cs_ref)
{
    MMLF_CHECK_ARG(in && packed && out, "%s: null pointer", who);
    MMLF_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    MMLF_CHECK_ARG(cs_in > 0 && cs_in % 8 == 0, "%s: cs_in=%d must be a multiple of 8", who, cs_in);
    MMLF_CHECK_ARG(K > 0 && (K + 7) / 8 * 8 == cs_in, "%s: K=%d does not match cs_in=%d", who, K, cs_in);
    MMLF_CHECK_ARG(np > 0, "%s: N=%d not supported (max %d)", who, N, ks == 2 ? MMLF_MAX_N_WIDE : MMLF_MAX_N);
    MMLF_CHECK_ARG(N_store > 0 && N_store <= cs_out && N_store <= np, "%s: N_store=%d vs cs_out=%d NP=%d", who,
                   N_store, cs_out, np);
    MMLF_CHECK_ARG(out_shift >= 0 && out_shift <= g.P + 1, "%s: out_shift=%d", who, out_shift);
    MMLF_CHECK_ARG(!relu_ref || cs_ref >= N_store, "%s: cs_ref=%d < N_store", who, cs_ref);
    MMLF_CHECK_ARG(g.NQpad + (ks - 1) * g.P + 64 < (1ll << 31), "%s: batch x image too large for 32-bit grid positions", who);
    a = {};
    a.in = in; a.wp = reinterpret_cast<const float *>(packed); a.bias = bias; a.out = out; a.ref = relu_ref;
    a.NQ = g.NQ; a.cs_in = cs_in; a.nchunk = cs_in / 8; a.cs_out = cs_out; a.n_store = N_store; a.n_true = N;
    a.out_shift = out_shift; a.vh = vh; a.vw = vw; a.P = g.P; a.G = g.G; a.R = g.R; a.relu = relu; a.cs_ref = cs_ref;
    a.divP = make_magic((unsigned)g.P); a.divR = make_magic((unsigned)g.R);
    conv_buffer_bytes(a, g, ks == 3 ? grid_alloc_positions_k3(g) : grid_alloc_positions(g));
    return 0;
}

// Column block b of a 2x2 layer (the only one, or one of a wide layer's: wide_np): the launch arguments of the whole layer
// `a`, narrowed to the block's p.npb packed columns and its part of the packed filter.  False: the block stores nothing (a
// channel slice that ends in front of it).
static bool conv_block_args(const ConvArgs &a, const ConvPlan &p, int b, ConvArgs &ab)
{
    ab = a;
    const int c0 = b * p.npb, npb = p.npb;
    if (a.n_store <= c0) return false;
    ab.n_store = a.n_store - c0 < npb ? a.n_store - c0 : npb;
    ab.n_true = a.n_true - c0 < npb ? a.n_true - c0 : npb;
    const char *wp = reinterpret_cast<const char *>(a.wp) + (size_t)b * p.block_bytes;
    ab.wp = reinterpret_cast<const float *>(wp);
    ab.w_unscale = p.unscale_off >= 0 ? reinterpret_cast<const float *>(wp + p.unscale_off) : nullptr;
    if (a.bias) ab.bias = a.bias + c0;
    ab.out = a.out + c0;
    ab.out_bytes = a.out_bytes - 4ll * c0;
    if (a.ref) { ab.ref = a.ref + c0; ab.ref_bytes = a.ref_bytes - 4ll * c0; }
    if (a.bn_partial) ab.bn_partial = a.bn_partial + c0;
    // transposed mask words: 2 x 2 words per lane and block (G <= 16), i.e. 256 of the 512 words of a (tile, wave)
    if (a.relu_mask_out) ab.relu_mask_out = a.relu_mask_out + 256 * b;
    if (a.relu_mask_in) ab.relu_mask_in = a.relu_mask_in + 256 * b;
    ab.mask_words = a.mask_words - 256 * b;
    return true;
}

// ncb column blocks of NT*32 columns per tile (2x2: always one)
template <int KS, int NT>
static int launch_conv_f32(const ConvArgs &a, long long ntiles, int ncb, hipStream_t st)
{
    constexpr const char *who = KS == 2 ? "mmlf_conv2x2" : "mmlf_conv3x3";
    constexpr size_t lds = ConvF32Lds<KS, NT>::BYTES;
    static PerDeviceOnce attr_once;
    if constexpr (KS == 2) {
        if (attr_once.run([] { return mmlf_allow_lds(reinterpret_cast<const void *>(conv4tap_kernel<NT>), lds, who); })) return 1;
        hipLaunchKernelGGL(conv4tap_kernel<NT>, dim3((unsigned)ntiles), dim3(512), lds, st, a);
    } else {
        if (attr_once.run([] { return mmlf_allow_lds(reinterpret_cast<const void *>(conv9tap_kernel<NT>), lds, who); })) return 1;
        hipLaunchKernelGGL(conv9tap_kernel<NT>, dim3((unsigned)(ntiles * ncb)), dim3(512), lds, st, a, ncb, ncb * NT * 32);
    }
    return mmlf_launch_status(who);
}

extern "C" int mmlf_conv2x2(const float *in, int cs_in, int K, const float *packed, const float *bias, int N,
                            float *out, int cs_out, int N_store, int out_shift, int vh, int vw, int B, int H,
                            int W, int relu, const float *relu_ref, int cs_ref, void *stream)
{
    ConvPlan p;
    const bool planned = conv_plan(0, cs_in, N, B, H, W, p);
    ConvArgs a;
    if (conv_common_args("mmlf_conv2x2", 2, p.np, a, p.g, in, cs_in, K, packed, bias, N, out, cs_out, N_store, out_shift, vh,
                         vw, B, H, W, relu, relu_ref, cs_ref))
        return 1;
    MMLF_CHECK_ARG(planned, "mmlf_conv2x2: no launch plan");      // (the checks above refuse what conv_plan refuses)
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < p.ncb; ++b) {
        ConvArgs ab;
        if (!conv_block_args(a, p, b, ab)) continue;
        int rc;
        switch (p.npb / 32) {
        case 1: rc = launch_conv_f32<2, 1>(ab, p.blocks, 1, st); break;
        case 3: rc = launch_conv_f32<2, 3>(ab, p.blocks, 1, st); break;
        case 4: rc = launch_conv_f32<2, 4>(ab, p.blocks, 1, st); break;
        case 5: rc = launch_conv_f32<2, 5>(ab, p.blocks, 1, st); break;
        case 6: rc = launch_conv_f32<2, 6>(ab, p.blocks, 1, st); break;
        case 8: rc = launch_conv_f32<2, 8>(ab, p.blocks, 1, st); break;
        default: rc = launch_conv_f32<2, 9>(ab, p.blocks, 1, st); break;
        }
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------ split-bf16 ("bf16x6") entry points
extern "C" int64_t mmlf_packed_filter_split_bytes(int K, int N) { return packed_filter_bytes(3, K, N); }

extern "C" int mmlf_pack_filter_split(const float *w, void *packed, int Cout, int Cin, int variant, int dgrad,
                                      void *stream)
{
    MMLF_CHECK_ARG(w && packed, "mmlf_pack_filter_split: null pointer");
    MMLF_CHECK_ARG(variant >= 0 && variant <= 2, "mmlf_pack_filter_split: bad variant %d", variant);
    const int K = dgrad ? Cout : Cin, N = dgrad ? Cin : Cout;
    const int NP = x6_np(N);
    MMLF_CHECK_ARG(NP > 0, "mmlf_pack_filter_split: N=%d not supported (max %d)", N, MMLF_MAX_N_WIDE);
    const int nchunk = (K + 7) / 8;
    const long long total = (long long)nchunk * 32 * NP;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_filter_split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w,
                       (unsigned short *)packed, Cout, Cin, variant, dgrad, nchunk, NP);
    return mmlf_launch_status("mmlf_pack_filter_split");
}

// The transposed epilogue (conv_epilogue16_tr) serves the launch kinds plain / ReLU / ReLU + mask-out / mask-in when the
// output rows can take 16-byte stores.  MMLF_CONV_TR=0 turns it off for the whole process (A/B; the ReLU mask words then
// have the other layout, for their producer and their consumer alike).
static bool conv_tr_enabled()
{
    static const int on = [] { const char *e = getenv("MMLF_CONV_TR"); return e ? atoi(e) : 1; }();
    return on != 0;
}
static bool conv_tr_fits(const ConvArgs &a)
{
    return a.n_store % 4 == 0 && a.cs_out % 4 == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
}

// ---- launch kind -> epilogue build
// The launch kinds of a training step get an epilogue build of their own on the hot shapes (f16 split: the 70- and 280-wide
// layers, the column blocks of the wider ones); every other combination of options runs the generic one, whose mask words
// have conv_epilogue16's layout for producer and consumer alike.  A kernel family says which kinds it has builds of, in
// which orientation, and conv_launch_epi picks by that -- the one place that does.
struct EpiBuilds {
    unsigned std, tr;        // bit k: launch kind k (the EPI_* bits of a launch's options) has a build in the standard / transposed form
    // the plain kind runs its transposed build.  Not on the 80-column kernels, where it measured 3 % slower
    // (profiles/r05_kbench_tr.log; their transposed plain builds are compiled and never launched)
    bool tr_plain;
    // transposed on one-segment activation windows only: with two segments (full frames, pitch > 383) the 288-column tiled
    // kernel's ReLU launches measured 26.7 ms against 24.3 in the other orientation, profiles/r05_ese_tr_kernel_stats.log,
    // while at training pitches they are 0.5-2 % faster.  The condition depends on (B, H, W) and the kernel alone, so a
    // mask's producer and its consumer always agree.
    bool tr_one_segment;
    // Column blocks of a wide layer: ReLU mask words in the transposed form ONLY -- its 2 x 2 words per lane let the two
    // blocks share a tile's 4096 words, conv_epilogue16's eight words per lane do not.  (The blocks' plain and ReLU kinds
    // are built in the transposed form alone: a launch that cannot take 16-byte stores runs the generic build, which
    // spills at G = 16.)
    bool masks_tr_only;
};
constexpr unsigned epi_bit(int kind) { return 1u << kind; }
constexpr unsigned EPI_TR_KINDS = epi_bit(EPI_PLAIN) | epi_bit(EPI_RELU) | epi_bit(EPI_RELU | EPI_MASK_OUT) | epi_bit(EPI_BITS_IN);
constexpr EpiBuilds EPI_BUILDS_RS = {EPI_TR_KINDS | epi_bit(EPI_STATS), EPI_TR_KINDS, false, false, false};       // register-streamed
constexpr EpiBuilds EPI_BUILDS_G5 = {EPI_TR_KINDS | epi_bit(EPI_STATS) | epi_bit(EPI_REF_IN), EPI_TR_KINDS, false, false, false};
constexpr EpiBuilds EPI_BUILDS_G18 = {EPI_TR_KINDS | epi_bit(EPI_STATS) | epi_bit(EPI_REF_IN), EPI_TR_KINDS, true, true, false};
constexpr EpiBuilds EPI_BUILDS_WIDE = {epi_bit(EPI_STATS) | epi_bit(EPI_REF_IN), EPI_TR_KINDS, true, false, true};   // G = 10, 12, 16
constexpr EpiBuilds EPI_BUILDS_NONE = {0, 0, false, false, false};                                                    // generic only

// the tiled kernels (conv4tap_x6s_kernel) of G 16-column groups and PL operand planes
template <int G, int PL>
struct ConvTiledKernels {
    static constexpr EpiBuilds builds = PL != 2 ? EPI_BUILDS_NONE : G == 5 ? EPI_BUILDS_G5 : G == 18 ? EPI_BUILDS_G18
                                        : (G == 10 || G == 12 || G == 16) ? EPI_BUILDS_WIDE : EPI_BUILDS_NONE;
    template <int EPI, bool TR> static int launch(const ConvArgs &a, const ConvPlan &p, hipStream_t st);
};
template <int G, int PL>
template <int EPI, bool TR>
int ConvTiledKernels<G, PL>::launch(const ConvArgs &a, const ConvPlan &p, hipStream_t st)
{
    constexpr size_t lds_pipe = 2 * (2 * 640 + 4 * PL * G * 16) * sizeof(float4);
    constexpr size_t lds_stats = 8 * (G * 16) * 2 * sizeof(double);
    constexpr size_t lds_coef = 2 * (G * 16) * sizeof(float);
    static PerDeviceOnce attr_once;
    if (attr_once.run([] { return mmlf_allow_lds(reinterpret_cast<const void *>(conv4tap_x6s_kernel<G, PL, EPI, 8, TR>),
                                                 lds_pipe + (TR ? lds_coef : PL == 2 ? lds_stats : 0), "mmlf_conv2x2_h2"); }))
        return 1;
    if constexpr (PL == 2 && G == 5) {
        if (a.nw == 16) {
            constexpr size_t lds_stats16 = 16 * (G * 16) * 2 * sizeof(double);
            constexpr size_t lds_pipe16 = RING16 * (2 * 640 + 4 * PL * G * 16) * sizeof(float4);
            static PerDeviceOnce attr_once16;
            if (attr_once16.run([] { return mmlf_allow_lds(reinterpret_cast<const void *>(conv4tap_x6s_kernel<G, PL, EPI, 16, TR>),
                                                           lds_pipe16 + (TR ? lds_coef : lds_stats16), "mmlf_conv2x2_h2(16 waves)"); }))
                return 1;
            const size_t lds16 = lds_pipe16 + (TR ? lds_coef : a.bn_partial ? lds_stats16 : 0);
            hipLaunchKernelGGL((conv4tap_x6s_kernel<G, PL, EPI, 16, TR>), dim3((unsigned)p.blocks), dim3(1024), lds16, st, a, (int)p.ntiles);
            return mmlf_launch_status("mmlf_conv2x2_h2(16 waves)");
        }
    }
    const size_t lds = lds_pipe + (TR ? lds_coef : a.bn_partial ? lds_stats : 0);
    hipLaunchKernelGGL((conv4tap_x6s_kernel<G, PL, EPI, 8, TR>), dim3((unsigned)p.blocks), dim3(512), lds, st, a, (int)p.ntiles);
    return mmlf_launch_status(PL == 3 ? "mmlf_conv2x2_split" : "mmlf_conv2x2_h2");
}

// the register-streamed kernels (conv4tap_rs_kernel; where they run: conv_rs_shape) over NCH input chunks
template <int G, int NCH>
struct ConvRsKernels {
    static constexpr EpiBuilds builds = EPI_BUILDS_RS;
    template <int EPI, bool TR> static int launch(const ConvArgs &a, const ConvPlan &p, hipStream_t st);
};
template <int G, int NCH>
template <int EPI, bool TR>
int ConvRsKernels<G, NCH>::launch(const ConvArgs &a, const ConvPlan &p, hipStream_t st)
{
    constexpr size_t lds = (size_t)NCH * 2 * 4 * (G * 16) * 16 + (TR ? 2 * (G * 16) * sizeof(float) : 8 * (G * 16) * 2 * sizeof(double));
    static PerDeviceOnce attr_once;
    if (attr_once.run([] { return mmlf_allow_lds(reinterpret_cast<const void *>(conv4tap_rs_kernel<G, NCH, EPI, TR>), lds, "mmlf_conv2x2_h2(register-streamed)"); }))
        return 1;
    hipLaunchKernelGGL((conv4tap_rs_kernel<G, NCH, EPI, TR>), dim3((unsigned)p.blocks), dim3(512), lds, st, a, (int)p.ngroups);
    return mmlf_launch_status("mmlf_conv2x2_h2(register-streamed)");
}

// kernel family K (its `builds`), launch options of `a` -> the epilogue build that runs
template <class K, int KIND>
static bool conv_launch_kind(int kind, bool tr, const ConvArgs &a, const ConvPlan &p, hipStream_t st, int &rc)
{
    constexpr EpiBuilds F = K::builds;
    if (kind != KIND) return false;
    if constexpr ((F.tr & epi_bit(KIND)) != 0) {
        if (tr && (KIND != EPI_PLAIN || F.tr_plain)) { rc = K::template launch<KIND, true>(a, p, st); return true; }
    }
    if constexpr ((F.std & epi_bit(KIND)) != 0) { rc = K::template launch<KIND, false>(a, p, st); return true; }
    return false;            // (a kind without a build in the orientation the launch takes: the generic one)
}
template <class K>
static int conv_launch_epi(const ConvArgs &a, const ConvPlan &p, hipStream_t st)
{
    constexpr EpiBuilds F = K::builds;
    if constexpr ((F.std | F.tr) != 0) {
        const int kind = (a.relu ? EPI_RELU : 0) | (a.bn_partial ? EPI_STATS : 0) | (a.relu_mask_in ? EPI_BITS_IN : 0) |
                         (a.ref ? EPI_REF_IN : 0) | (a.relu_mask_out ? EPI_MASK_OUT : 0);
        const bool masks = a.relu_mask_in || a.relu_mask_out, shape = !F.tr_one_segment || a.seg_delta == 0;
        const bool tr = conv_tr_enabled() && shape && conv_tr_fits(a);      // the transposed form, for the kinds that have one
        if (masks && !tr && F.masks_tr_only)
            return mmlf_fail("mmlf_conv2x2_h2: N > %d keeps ReLU mask words in the transposed layout only (n_store %% 4 == 0, a "
                             "16-byte aligned output, MMLF_CONV_TR not 0)", MMLF_MAX_N);
        if (masks && !tr && conv_tr_enabled() && shape)
            return mmlf_fail("mmlf_conv2x2_h2: ReLU mask words need n_store %% 4 == 0 and a 16-byte aligned output");
        int rc = 0;
        if (conv_launch_kind<K, EPI_PLAIN>(kind, tr, a, p, st, rc) || conv_launch_kind<K, EPI_RELU>(kind, tr, a, p, st, rc) ||
            conv_launch_kind<K, EPI_RELU | EPI_MASK_OUT>(kind, tr, a, p, st, rc) || conv_launch_kind<K, EPI_BITS_IN>(kind, tr, a, p, st, rc) ||
            conv_launch_kind<K, EPI_STATS>(kind, tr, a, p, st, rc) || conv_launch_kind<K, EPI_REF_IN>(kind, tr, a, p, st, rc))
            return rc;
        if (masks && F.masks_tr_only)
            return mmlf_fail("mmlf_conv2x2_h2: N > %d: this combination of ReLU mask options has no build", MMLF_MAX_N);
    }
    return K::template launch<EPI_GENERIC, false>(a, p, st);
}

template <int G, int PL>
static int launch_conv_x6s(const ConvArgs &a, const ConvPlan &p, hipStream_t st)
{
    if constexpr (PL == 2 && G == 5) {
        if (p.rs) return a.nchunk == 9 ? conv_launch_epi<ConvRsKernels<G, 9>>(a, p, st) : conv_launch_epi<ConvRsKernels<G, 4>>(a, p, st);
    }
    return conv_launch_epi<ConvTiledKernels<G, PL>>(a, p, st);
}

template <int PL>
static int launch_conv_split(const ConvArgs &a, const ConvPlan &p, hipStream_t st)
{
    switch (p.npb) {
    case 32: return launch_conv_x6s<2, PL>(a, p, st);
    case 80: return launch_conv_x6s<5, PL>(a, p, st);
    case 96: return launch_conv_x6s<6, PL>(a, p, st);
    case 112: return launch_conv_x6s<7, PL>(a, p, st);
    case 128: return launch_conv_x6s<8, PL>(a, p, st);
    case 160: return launch_conv_x6s<10, PL>(a, p, st);      // (160, 192, 256: column blocks of a wide layer)
    case 192: return launch_conv_x6s<12, PL>(a, p, st);
    case 256: return launch_conv_x6s<16, PL>(a, p, st);
    default: return launch_conv_x6s<18, PL>(a, p, st);
    }
}

static int conv_split_impl(const char *who, int planes, const float *in, int cs_in, int K, const void *packed,
                           const float *bias, int N, float *out, int cs_out, int N_store, int out_shift, int vh,
                           int vw, int B, int H, int W, int relu, const float *relu_ref, int cs_ref,
                           const float *in_amax, float *out_amax, double *bn_partial, void *stream,
                           unsigned *relu_mask_out = nullptr, const unsigned *relu_mask_in = nullptr)
{
    ConvPlan p;
    const bool planned = conv_plan(planes, cs_in, N, B, H, W, p);
    ConvArgs a;
    if (conv_common_args(who, 2, p.np, a, p.g, in, cs_in, K, packed, bias, N, out, cs_out, N_store, out_shift, vh, vw, B, H, W, relu,
                         relu_ref, cs_ref))
        return 1;
    MMLF_CHECK_ARG(planned, "%s: no launch plan", who);           // (the checks above refuse what conv_plan refuses)
    MMLF_CHECK_ARG(!(relu_ref && relu_mask_in), "%s: relu_ref and relu_mask_in are alternatives", who);
    MMLF_CHECK_ARG((long long)cs_in * 4 * 64 < (1ll << 31), "%s: cs_in too large", who);
    MMLF_CHECK_ARG(planes == 3 || in_amax, "%s: the f16 split needs the input's max |x|", who);
    MMLF_CHECK_ARG(!bn_partial || (planes == 2 && N_store >= N), "%s: BatchNorm statistics need the f16 split path", who);
    a.in_amax = in_amax; a.out_amax = out_amax; a.bn_partial = bn_partial; a.bn_stride = N;
    a.relu_mask_out = relu_mask_out; a.relu_mask_in = relu_mask_in;
    a.nw = p.nw;
    a.a_pieces = p.a_pieces; a.a_per_seg = p.a_per_seg; a.a_tail = p.a_tail; a.seg_slot = p.seg_slot; a.seg_delta = p.seg_delta;
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < p.ncb; ++b) {    // one launch; a wide layer: one per column block, same tiles and workgroups
        ConvArgs ab;
        if (!conv_block_args(a, p, b, ab)) continue;
        const int rc = planes == 3 ? launch_conv_split<3>(ab, p, st) : launch_conv_split<2>(ab, p, st);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int mmlf_conv2x2_split(const float *in, int cs_in, int K, const void *packed, const float *bias, int N,
                                  float *out, int cs_out, int N_store, int out_shift, int vh, int vw, int B, int H,
                                  int W, int relu, const float *relu_ref, int cs_ref, void *stream)
{
    return conv_split_impl("mmlf_conv2x2_split", 3, in, cs_in, K, packed, bias, N, out, cs_out, N_store, out_shift,
                           vh, vw, B, H, W, relu, relu_ref, cs_ref, nullptr, nullptr, nullptr, stream);
}

// ------------------------------------------------------------------ f16 2-way split ("f16x3") entry points
extern "C" int64_t mmlf_packed_filter_h2_bytes(int K, int N) { return packed_filter_bytes(2, K, N); }

extern "C" int mmlf_pack_filter_h2(const float *w, void *packed, int Cout, int Cin, int variant, int dgrad,
                                   void *stream)
{
    MMLF_CHECK_ARG(w && packed, "mmlf_pack_filter_h2: null pointer");
    MMLF_CHECK_ARG(variant >= 0 && variant <= 2, "mmlf_pack_filter_h2: bad variant %d", variant);
    const int K = dgrad ? Cout : Cin, N = dgrad ? Cin : Cout;
    const int NP = x6_np(N);
    MMLF_CHECK_ARG(NP > 0, "mmlf_pack_filter_h2: N=%d not supported (max %d)", N, MMLF_MAX_N_WIDE);
    const int nchunk = (K + 7) / 8;
    // (the per-column unscale factors sit behind the packed planes of their column block)
    hipLaunchKernelGGL(pack_filter_h2_kernel, dim3(NP), dim3(256), 0, (hipStream_t)stream, w, packed, Cout, Cin, variant, dgrad,
                       nchunk, NP);
    return mmlf_launch_status("mmlf_pack_filter_h2");
}

extern "C" int mmlf_packed_filter_h2_columns(int N) { return x6_np(N); }

extern "C" int mmlf_pack_filters_h2(const mmlf_pack_desc *table, int n, int total_columns, void *stream)
{
    MMLF_CHECK_ARG(table && n > 0 && total_columns > 0, "mmlf_pack_filters_h2: empty table");
    hipLaunchKernelGGL(pack_filters_h2_kernel, dim3((unsigned)total_columns), dim3(256), 0, (hipStream_t)stream, table, n);
    return mmlf_launch_status("mmlf_pack_filters_h2");
}

extern "C" int mmlf_conv2x2_h2(const float *in, int cs_in, int K, const void *packed, const float *bias, int N,
                               float *out, int cs_out, int N_store, int out_shift, int vh, int vw, int B, int H,
                               int W, int relu, const float *relu_ref, int cs_ref, const float *in_amax,
                               float *out_amax, double *bn_partial, uint32_t *relu_mask_out,
                               const uint32_t *relu_mask_in, void *stream)
{
    return conv_split_impl("mmlf_conv2x2_h2", 2, in, cs_in, K, packed, bias, N, out, cs_out, N_store, out_shift, vh,
                           vw, B, H, W, relu, relu_ref, cs_ref, in_amax, out_amax, bn_partial, stream, relu_mask_out,
                           relu_mask_in);
}

extern "C" int64_t mmlf_relu_mask_words(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    return make_grid(B, H, W).NQpad / MMLF_TILE * 4096;        // [tile][8 waves][8 rows][64 lanes]
}

extern "C" int mmlf_conv2x2_blocks(int K, int N, int B, int H, int W)
{
    ConvPlan p;
    if (K <= 0 || !conv_plan(2, (K + 7) / 8 * 8, N, B, H, W, p)) return -1;
    return p.blocks;                                             // (column blocks: the same grid each)
}

// ---------------------------------------------------------------------------------------------
// "thin" convolutions: N <= 2 output channels over a wide input (the first convolution of the BASE / UPR head,
// reference feed_forward.py:179-182: 280 -> 1 | 2).  On the MFMA kernels such a layer pays for 32 columns to
// use one or two and runs for 2.9 ms forward and 6.3 ms in the weight gradient at bs=512; it is a matrix-VECTOR
// product, bound by reading the input once: plain float32 FMAs (no operand split), one wave per grid position.
//   forward : part[p][t][o] = sum_c in[p][c] * W[o][c][tap t]        (thin_rowdot_kernel, reads `in` once)
//             out[q + shift][o] = valid(q) ? act(b[o] + sum_t part[q + off_t][t][o]) : 0   (thin_combine_kernel)
//   weights : dW[o][c][t] += sum_p in[p][c] * g[p - off_t + g_shift][o]                    (thin_wgrad_kernel)
// ---------------------------------------------------------------------------------------------

// A wave takes 64 consecutive positions.  Channels go through LDS in slices of 32: the slice is read from global
// memory in whole 128-byte row segments (lane = (row, float4)), and consumed with lane = position, so the dot
// products need no cross-lane reduction (eight of them per position through ds_bpermute made this kernel LDS-bound);
// the filter values of a slice are wave-uniform and come through the scalar cache.
__global__ __launch_bounds__(256) void thin_rowdot_kernel(ThinArgs a)
{
    __shared__ float tile[4][64][33];                     // [wave][position][channel of the slice] (+1: conflict-free columns)
    __shared__ float4 wt[4][32][2];                       // [wave][channel of the slice][o] = the four taps of W[o][c]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + wv));
    const long long nwaves = gridDim.x * 4ll;
    const int nslice = (a.C + 31) / 32;
    for (long long p0 = 64 * wave; p0 < a.npos; p0 += 64 * nwaves) {
        float acc[4][THIN_MAXN];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int o = 0; o < THIN_MAXN; ++o) acc[t][o] = 0.f;
        for (int sl = 0; sl < nslice; ++sl) {
            // 64 rows x 8 float4: lane (r8 = lane >> 3, f = lane & 7) loads rows r8, r8 + 8, ...
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int r = (lane >> 3) + 8 * j, f = lane & 7;
                const long long p = p0 + r < a.npos ? p0 + r : a.npos - 1;
                const int c = 32 * sl + 4 * f;
                v[j] = *reinterpret_cast<const float4 *>(a.in + (size_t)p * a.cs_in + (c < a.cs_in ? c : 0));
                if (c >= a.cs_in) v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            {   // this slice's filter values: lane (c = lane & 31, o = lane >> 5), taps in packed order
                const int c = 32 * sl + (lane & 31), o = lane >> 5;
                float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < a.C && o < a.N) {
                    const float *wp = a.w + ((size_t)o * a.C + c) * 4;
                    w4 = make_float4(wp[master_tap<2>(0, a.variant)], wp[master_tap<2>(1, a.variant)], wp[master_tap<2>(2, a.variant)],
                                     wp[master_tap<2>(3, a.variant)]);
                }
                wt[wv][lane & 31][o] = w4;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int r = (lane >> 3) + 8 * j, f = lane & 7;
                tile[wv][r][4 * f + 0] = v[j].x; tile[wv][r][4 * f + 1] = v[j].y;
                tile[wv][r][4 * f + 2] = v[j].z; tile[wv][r][4 * f + 3] = v[j].w;
            }
            // (one wave reads what it wrote: program order + the compiler's lgkmcnt waits suffice)
#pragma unroll 8
            for (int k = 0; k < 32; ++k) {                // channels past C carry zero weights
                const float x = tile[wv][lane][k];
                const float4 w0 = wt[wv][k][0], w1 = wt[wv][k][1];
                acc[0][0] = fmaf(x, w0.x, acc[0][0]); acc[1][0] = fmaf(x, w0.y, acc[1][0]);
                acc[2][0] = fmaf(x, w0.z, acc[2][0]); acc[3][0] = fmaf(x, w0.w, acc[3][0]);
                acc[0][1] = fmaf(x, w1.x, acc[0][1]); acc[1][1] = fmaf(x, w1.y, acc[1][1]);
                acc[2][1] = fmaf(x, w1.z, acc[2][1]); acc[3][1] = fmaf(x, w1.w, acc[3][1]);
            }
        }
        const long long p = p0 + lane;
        if (p < a.npos) {
            float4 *dst = reinterpret_cast<float4 *>(a.part + (size_t)p * 4 * THIN_MAXN);
            dst[0] = make_float4(acc[0][0], acc[0][1], acc[1][0], acc[1][1]);
            dst[1] = make_float4(acc[2][0], acc[2][1], acc[3][0], acc[3][1]);
        }
    }
}

// one workgroup per DESTINATION grid row: writes every position of the row (zeros outside the valid extent)
__global__ __launch_bounds__(128) void thin_combine_kernel(ThinArgs a)
{
    const int drow = blockIdx.x;                          // global grid row of the destination
    float mx = 0.f;
    for (int x = threadIdx.x; x < a.P; x += blockDim.x) {
        const long long d = (long long)drow * a.P + x, q = d - a.out_shift;
        float v[THIN_MAXN] = {0.f, 0.f};
        bool valid = false;
        if (q >= 0 && q < a.NQ) {
            const unsigned row = fastdiv((unsigned)q, a.divP);
            const int qx = (int)(q - (long long)row * a.P), qy = (int)(row - fastdiv(row, a.divR) * a.R);
            valid = qy < a.vh && qx < a.vw;
        }
        if (valid) {
            const int offs[4] = {0, 1, a.P, a.P + 1};
#pragma unroll
            for (int o = 0; o < THIN_MAXN; ++o) {
                float s = (a.bias && o < a.N) ? a.bias[o] : 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) s += a.part[((size_t)(q + offs[t]) * 4 + t) * THIN_MAXN + o];
                if (a.relu) s = fmaxf(s, 0.f);
                v[o] = o < a.N ? s : 0.f;
            }
        }
        float *dst = a.out + (size_t)d * a.cs_out;
        for (int o = 0; o < a.cs_out; ++o) dst[o] = o < THIN_MAXN ? v[o] : 0.f;
        mx = fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1])));
    }
    if (a.out_amax) mmlf_amax_update_row(mx, a.out_amax, drow);
}

extern "C" int64_t mmlf_conv2x2_thin_workspace_floats(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    const Grid g = make_grid(B, H, W);
    return (g.NQ + g.P + 2) * 4 * THIN_MAXN;
}

extern "C" int mmlf_conv2x2_thin(const float *in, int cs_in, int K, const float *w_oihw, const float *bias, int N,
                                 float *out, int cs_out, int out_shift, int vh, int vw, int B, int H, int W, int relu,
                                 int variant, float *workspace, float *out_amax, void *stream)
{
    MMLF_CHECK_ARG(in && w_oihw && out && workspace, "mmlf_conv2x2_thin: null pointer");
    MMLF_CHECK_ARG(N >= 1 && N <= THIN_MAXN && K >= 1 && K <= cs_in && cs_in % 4 == 0 && cs_in <= 512,
                   "mmlf_conv2x2_thin: N=%d K=%d cs_in=%d (N <= 2, cs_in <= 512)", N, K, cs_in);
    MMLF_CHECK_ARG(B > 0 && H > 0 && W > 0 && cs_out >= THIN_MAXN && variant >= 0 && variant <= 2, "mmlf_conv2x2_thin: bad shape");
    const Grid g = make_grid(B, H, W);
    MMLF_CHECK_ARG(out_shift >= 0 && out_shift <= g.P + 1 && g.NQpad + 2 * g.P + 64 < (1ll << 31), "mmlf_conv2x2_thin: out_shift / size");
    ThinArgs a = {};
    a.in = in; a.w = w_oihw; a.bias = bias; a.part = workspace; a.out = out; a.out_amax = out_amax;
    a.NQ = g.NQ; a.npos = g.NQ + g.P + 2; a.cs_in = cs_in; a.C = K; a.N = N; a.cs_out = cs_out; a.out_shift = out_shift;
    a.vh = vh; a.vw = vw; a.P = g.P; a.R = g.R; a.relu = relu; a.variant = variant;
    a.divP = make_magic((unsigned)g.P); a.divR = make_magic((unsigned)g.R);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(thin_rowdot_kernel, dim3(4 * device_cus()), dim3(256), 0, st, a);
    hipLaunchKernelGGL(thin_combine_kernel, dim3((unsigned)(B * g.R)), dim3(128), 0, st, a);
    return mmlf_launch_status("mmlf_conv2x2_thin");
}

// ---------------------------------------------------------------------------------------------
// what this binary is (round 5): ABI version, source revision and the bounds-debug switch in one string; bench.py prints it in
// its line.  The product sources have no result-changing build switch any more (tools/README.md "Removed", EXPERIMENTS.md),
// so mmlf_build_is_ablation() is 0 here; the loader still refuses a variant built from an older tree that reports 1
// (mmlf_amd/_lib.py)
// ---------------------------------------------------------------------------------------------
#ifndef MMLF_GIT_HASH
#define MMLF_GIT_HASH "unknown"
#endif
#ifdef MMLF_BOUNDS_DEBUG
#define MMLF_BOUNDS_DEBUG_VALUE 1
#else
#define MMLF_BOUNDS_DEBUG_VALUE 0
#endif
extern "C" int mmlf_build_is_ablation(void) { return 0; }
extern "C" const char *mmlf_build_info(void)
{
    static char text[448];
    static std::once_flag once;
    std::call_once(once, [] {
        snprintf(text, sizeof(text), "abi=%d git=%s src=%s MMLF_BOUNDS_DEBUG=%d ablation=%d", MMLF_ABI_VERSION, MMLF_GIT_HASH,
                 MMLF_SRC_HASH, MMLF_BOUNDS_DEBUG_VALUE, mmlf_build_is_ablation());
    });
    return text;
}

// ---------------------------------------------------------------------------------------------
// Bounds audit (round 5).  For one launch of the given shape: the END (largest byte offset + 1) of what the launch may
// read or write behind each pointer argument, derived here from the same launch geometry the entry points compute
// (window pieces, tile counts, grids).  tests/test_bounds_audit.py holds every end against what the size queries of this
// ABI tell the caller to allocate, over a sweep of shapes; the -DMMLF_BOUNDS_DEBUG build counts violations on the GPU.
// Derivations (positions are grid positions q; a buffer of channel stride cs holds alloc = NQpad + P + 72 of them):
//  conv, f16 split: the launch geometry is the launch's own ConvPlan (its comment derives the last activation position
//    fetched, NQpad + P).  Output: position q + out_shift,
//    q < NQpad, n_store channels; the ReLU reference likewise.  Row maxima: rows up to the one behind the last position
//    read (input) / written (output).  Mask words: [tile][8][8][64].  Statistics: [workgroup][2][N] doubles.
//    A layer wider than 288 columns is two launches of this kind on column blocks (wide_np): the same tiles, windows and
//    workgroup count each, the packed filter's blocks back to back (the same byte total), the blocks' channels side by side
//    in out / ref / bias / the statistics, and each block's mask words inside its tile's 4096: the ends below hold as they are.
//  weight gradient: chunk c stages in[32 c .. 32 c + 32 + P] and g[32 c + g_shift .. + 31], c < NQpad / 32.
// ---------------------------------------------------------------------------------------------
extern "C" int mmlf_audit_conv_h2(int cs_in, int K, int N, int cs_out, int N_store, int out_shift, int cs_ref, int B, int H, int W,
                                  int64_t *ends /* [MMLF_AUDIT_CONV_N] */)
{
    ConvPlan p;
    MMLF_CHECK_ARG(conv_plan(2, cs_in, N, B, H, W, p) && K > 0 && (K + 7) / 8 * 8 == cs_in && ends, "mmlf_audit_conv_h2: bad argument");
    const Grid &g = p.g;
    const long long last_out = g.NQpad - 1 + out_shift;
    ends[0] = (p.last_in + 1) * cs_in * 4;                                    // in
    ends[1] = (int64_t)p.ncb * p.block_bytes;                                 // packed (per block: planes, then the columns' 1 / scale)
    ends[2] = (int64_t)N * 4;                                                 // bias
    ends[3] = (last_out * cs_out + N_store) * 4;                              // out
    ends[4] = cs_ref ? (last_out * cs_ref + N_store) * 4 : 0;                 // relu_ref
    ends[5] = (MMLF_AMAX_HEAD + ((g.NQ - 1) / g.P + 1) + 1) * 4;              // in_amax: rows read by the last valid wave, + 1
    ends[6] = (MMLF_AMAX_HEAD + last_out / g.P + 1) * 4;                      // out_amax
    ends[7] = (int64_t)p.blocks * 2 * N * 8;                                            // bn_partial (doubles)
    ends[8] = g.NQpad / MMLF_TILE * 4096 * 4;                                 // relu mask words (in or out)
    return 0;
}


// ---------------------------------------------------------------------------------------------
// 3x3 ("same", pad 1) convolution, exact-f32 MFMA: nn.Conv2d(k=3, padding=1) forward and data gradient
// (reference feed_forward.py:123,125 with --model_ksize 3).  Nine taps at q + dy*P + dx, dy, dx in {0, 1, 2}; the
// output goes to q + P + 1 (extent (H, W) at grid offset (1, 1)); the data gradient is the same correlation with the
// taps rotated by 180 degrees and Cin / Cout swapped (pack_filter_f32_kernel<3>, dgrad = 1).  The kernel is
// conv9tap_kernel = conv_f32_taps<3, NT> above; here its launch shape and entry points.
// ---------------------------------------------------------------------------------------------
// 3x3 launch shape: NT 32-column tiles per workgroup, ncb column blocks
static inline bool conv9_shape(int N, int *nt, int *ncb)
{
    const int n = pick_nt(N);
    if (n < 0) return false;
    *nt = n == 9 ? 3 : n;
    *ncb = n == 9 ? 3 : 1;
    return true;
}

extern "C" int64_t mmlf_packed_filter3x3_floats(int K, int N) { return packed_filter_f32_floats(3, K, N); }

extern "C" int mmlf_pack_filter3x3(const float *w, float *packed, int Cout, int Cin, int variant, int dgrad, void *stream)
{
    return pack_filter_f32("mmlf_pack_filter3x3", 3, w, packed, Cout, Cin, variant, dgrad, stream);
}

extern "C" int mmlf_conv3x3(const float *in, int cs_in, int K, const float *packed, const float *bias, int N,
                            float *out, int cs_out, int N_store, int B, int H, int W, int relu, const float *relu_ref,
                            int cs_ref, void *stream)
{
    int nt = -1, ncb = 1;
    conv9_shape(N, &nt, &ncb);
    ConvArgs a;
    const Grid g = make_grid(B, H, W);
    // the output goes to q + P + 1 (P = W + GRID_PAD), valid extent (H, W)
    if (conv_common_args("mmlf_conv3x3", 3, nt * ncb * 32, a, g, in, cs_in, K, packed, bias, N, out, cs_out, N_store,
                         W + GRID_PAD + 1, H, W, B, H, W, relu, relu_ref, cs_ref))
        return 1;
    const long long ntiles = g.NQpad / MMLF_TILE;
    hipStream_t st = (hipStream_t)stream;
    switch (nt) {
    case 1: return launch_conv_f32<3, 1>(a, ntiles, ncb, st);
    case 3: return launch_conv_f32<3, 3>(a, ntiles, ncb, st);
    default: return launch_conv_f32<3, 4>(a, ntiles, ncb, st);
    }
}

// Bounds audit of one mmlf_conv3x3 launch (ends[MMLF_AUDIT_IN .. MMLF_AUDIT_REF]): the last tile's window reads positions
// NQpad - 256 + 2P + 0..257, B pieces read the whole packed filter, the epilogue writes q + P + 1 for q < NQpad.
extern "C" int mmlf_audit_conv3x3(int cs_in, int K, int N, int cs_out, int N_store, int cs_ref, int B, int H, int W,
                                  int64_t *ends /* [5] */)
{
    int nt, ncb;
    MMLF_CHECK_ARG(conv9_shape(N, &nt, &ncb) && K > 0 && (K + 7) / 8 * 8 == cs_in && B > 0 && H > 0 && W > 0 && ends,
                   "mmlf_audit_conv3x3: bad argument");
    const Grid g = make_grid(B, H, W);
    const long long last_in = (g.NQpad - MMLF_TILE) + 2 * g.P + 257;
    const long long last_out = g.NQpad - 1 + g.P + 1;
    ends[0] = (last_in + 1) * cs_in * 4;                                       // in
    ends[1] = mmlf_packed_filter3x3_floats(cs_in, N) * 4;                      // packed
    ends[2] = (int64_t)N * 4;                                                  // bias
    ends[3] = (last_out * cs_out + N_store) * 4;                               // out
    ends[4] = cs_ref ? (last_out * cs_ref + N_store) * 4 : 0;                  // relu_ref
    return 0;
}
