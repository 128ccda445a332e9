// row_walk.h -- how the threads of a 256-thread block walk one row of the padded grid, which of its positions are interior,
// and the tile sizes of the layout and reduction kernels: plain integer functions of the launch's numbers, shared by the
// kernels and wrappers (elementwise.hip) and by the host program that lists a walk thread by thread (tools/row_walk.hip;
// tests/test_elementwise_cpu.py holds the listing to its rules).  Nothing here reads the device or the environment.
//
// The bound the walk gives, for every row kernel (bn_rows_kernel, relu_slice_rows_kernel, bn_apply4_kernel, the write-out
// of shift_pack_kernel).  A block takes grid rows row = blockIdx.x, + gridDim.x, ... < nrows = B * R; its threads meet every
// (x, cg) of [0, limit) x [0, cvn) exactly once (the listing shows it: each thread starts at tid = x * cvn + cg and moves on
// by 256 = dx * cvn + dc in that numbering) and nothing outside.  Every access of such a kernel is at the float index
//     (row * P + x) * cs + off + V * cg + k,   row < B * R,  x < limit <= P,  cg < cvn,  k < V,
// and the wrappers admit only off + C <= cs for the C channels a kernel stores (the last group is cut short at C where C
// is no multiple of V): a store's index is below B * R * P * cs = NQ * cs, the buffer's grid part.  Reads happen at interior
// positions only, x <= W = P - 2: a whole-group read whose slice ends inside the group runs fewer than V floats on, into
// the next position of the same row, and stays below NQ * cs as well.
#pragma once

constexpr int ROW_THREADS = 256;            // threads of a row kernel's block

// groups of v channels that hold the first c channels
__host__ __device__ __forceinline__ int row_groups(int c, int v) { return (c + v - 1) / v; }

// A thread's walk over the (position, group) pairs of a row, group fastest, 256 pairs on per step without a division:
// (x, cg) += (dx, dc), and one carry where cg runs past cvn (dc < cvn, so one is enough; that holds past 256 groups too,
// where dx = 0 and dc = 256).
struct RowWalk { int cvn, dx, dc; };
__host__ __device__ __forceinline__ RowWalk row_walk(int cvn)
{
    RowWalk w;
    w.cvn = cvn;
    w.dx = ROW_THREADS / cvn;
    w.dc = ROW_THREADS - w.dx * cvn;
    return w;
}
// where thread tid starts; false: the row has nothing for it (limit = the pitch, or the positions of a piece of the row)
__host__ __device__ __forceinline__ bool row_walk_start(const RowWalk &w, int tid, int limit, int &x, int &cg)
{
    x = tid / w.cvn;
    cg = tid - x * w.cvn;
    return x < limit;
}
// the thread's next pair; false: it has left the row
__host__ __device__ __forceinline__ bool row_walk_step(const RowWalk &w, int limit, int &x, int &cg)
{
    x += w.dx;
    cg += w.dc;
    if (cg >= w.cvn) { cg -= w.cvn; ++x; }
    return x < limit;
}

// Grid row `row` of a (B, R = H + pad, P = W + pad) grid holds interior positions / position x of such a row is one:
// the border (y = 0, y > H, x = 0, x > W) is written as zeros and never read.
__host__ __device__ __forceinline__ bool grid_row_interior(int row, int R, int H)
{
    const int y = row % R;
    return y >= 1 && y <= H;
}
__host__ __device__ __forceinline__ bool grid_pos_interior(int x, int W) { return x >= 1 && x <= W; }

// Positions per transpose tile of pack_nchw_kernel and shift_pack_kernel, [cs][xt | 1] floats: 128, halved until the tile
// fits 32 KB (wide tensors: DPP with many views packs a gradient of 4 * views * 3 channels; at 64 KB two workgroups per CU
// packed the 108-channel DPP gradient 0.5 ms slower), not below 4.  A power of two.
static inline int pack_tile_positions(int cs)
{
    int xt = 128;
    while (xt > 4 && (size_t)cs * (xt | 1) * sizeof(float) > 32 * 1024) xt >>= 1;
    return xt;
}
// ... and of unpack_nchw_kernel, [xt][C | 1] floats: 32, halved likewise, not below 1
static inline int unpack_tile_positions(int C)
{
    int xt = 32;
    while (xt > 1 && (size_t)xt * (C | 1) * sizeof(float) > 32 * 1024) xt >>= 1;
    return xt;
}

// bn_reduce_body: a thread keeps ONE channel group, and the block takes ppi positions of a row per iteration (threads
// from ppi * cvn on are idle)
__host__ __device__ __forceinline__ void reduce_walk(int C, int v, int &cvn, int &ppi)
{
    cvn = row_groups(C, v);
    ppi = ROW_THREADS / cvn;
}
