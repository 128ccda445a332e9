// wgrad_map.h -- which (input-channel slice, position split) item a block of a weight-gradient launch runs, how many position
// splits the wide kernel's launch is cut into and how many workgroups it takes: plain integer functions of the launch's
// numbers, shared by the kernels (wgrad.hip) and by the host program that lists a launch item by item
// (tools/wgrad_items.hip; tests/test_wgrad_persistent.py holds the listing to its rules).  Nothing here reads the device or the
// environment: wgrad.hip passes device_cus() and MMLF_WGRAD_PERSIST in.
#pragma once

// Block -> (slice, position split).  Blocks b, b + 8, ... land on one XCD (round-robin dispatch): the slices of one split are
// placed there and share its L2 for their gradient reads.  nsplit need not be a multiple of 8: the 8 * (nsplit / 8) regular
// splits are numbered as they always were (same partial-sum order), the slices of the remaining ones are dealt behind them,
// `per` blocks to an XCD, consecutive slices together (their gradient reads come from memory once per XCD they touch: a few
// percent of the launch's reads at 2 of 42 splits).
// b: the block's number in the one-shot launch (blockIdx.x there; the persistent wide kernel walks b = blockIdx.x, + gridDim.x,
// ... and its grid is a multiple of 8, so b & 7 -- the XCD -- is the same for all items of a workgroup).
__host__ __device__ __forceinline__ bool wgrad_block_map(int b, int nslice, int nsplit, int &slice, int &split)
{
    const int x = b & 7, j = b >> 3;
    const int reg = (nsplit >> 3) * nslice;           // regular blocks per XCD
    if (j < reg) {
        slice = j % nslice;
        split = (j / nslice) * 8 + x;
        return true;
    }
    const int left = (nsplit & 7) * nslice, per = (left + 7) >> 3;
    const int m = x * per + (j - reg);
    slice = m % nslice;
    split = (nsplit & ~7) + m / nslice;
    return m < left;
}

// blocks of the one-shot launch = items of the persistent one (a multiple of 8; the surplus ones map to nothing)
static inline unsigned wgrad_grid_blocks(int nslice, int nsplit)
{
    return 8u * (unsigned)((nsplit >> 3) * nslice + ((nsplit & 7) * nslice + 7) / 8);
}

// wgrad4tap_x6w_kernel (48-row slices of the Cin + 1 rows): slices and position splits of a launch of nchunks 32-position
// chunks on `cus` compute units; nchunks < 0: the largest layout (workspace sizing).
// Small batches: ONE item per CU on 256 CUs (42 splits = 252 items at six slices; a third of the partial sums to
// write and reduce: -2...-4 % per launch at 64 patches, +0.9 % per 64-patch step).  From ~150 patches on, three
// items per CU (128 splits, 768 items) are 0.8 % faster inside the step (profiles/r04_wgrad_nsplit.log).  The split
// counts -- and with them the partial sums and the order they are added in -- are what they were when every item was
// a workgroup of its own and 768 of them three dispatch rounds; the launch now places wgrad_wide_grid() workgroups once and
// each walks its items.
// (the workspace is sized by the LARGER of the two counts at 256 CUs: a part with fewer CUs only lowers one_round)
static inline void wgrad_wide_splits(int Cin, long long nchunks, int cus, int &nslice, int &nsplit)
{
    nslice = (Cin + 1 + 47) / 48;
    if (cus > 256 || nchunks < 0) cus = 256;
    const int one_round = cus / nslice, three_rounds = (768 / nslice + 7) / 8 * 8;
    nsplit = nchunks < 0 ? (one_round > three_rounds ? one_round : three_rounds)
                         : (nchunks >= 42 * 1024 ? three_rounds : one_round);
    if (nsplit < 8) nsplit = 8;
}

// Workgroups of the wide kernel's launch over `items` (slice, split) items.  The kernel takes a whole CU (155.9 KB of LDS, 2 x 232
// registers per SIMD lane), so at most one workgroup per CU is ever resident: 768 one-shot workgroups (128 splits x 6 slices)
// were three dispatch rounds on 256 CUs, and between two rounds a CU stood free for whatever else was waiting -- the
// BatchNorm-backward workgroups that run beside conv1's gradient (engine.py, MMLF_OVERLAP_WGRAD) took its registers, and the
// next weight-gradient workgroup could not be placed until they had drained.  The persistent launch places one workgroup per
// CU ONCE and lets it walk its items (three trips at 768 items): the CU is never handed back in mid-launch.  A multiple of 8
// workgroups, so that the items of a workgroup stay on its XCD (wgrad_block_map).  persist = false (MMLF_WGRAD_PERSIST=0)
// launches one workgroup per item as before: the same kernel on one trip, the same bits.
static inline unsigned wgrad_wide_grid(int items, int cus, bool persist)
{
    if (!persist) return (unsigned)items;
    int resident = cus / 8 * 8;
    if (resident < 8) resident = 8;
    return (unsigned)(items < resident ? items : resident);
}
