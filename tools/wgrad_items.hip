// Lists a launch of the wide weight gradient (wgrad4tap_x6w_kernel) item by item, on the host, by the very functions the
// kernel and its launch use (mmlf_amd/csrc/wgrad_map.h): no GPU needed.
//   hipcc --offload-arch=gfx950 -I mmlf_amd/csrc tools/wgrad_items.hip -o wgrad_items
//   ./wgrad_items CIN NCHUNKS CUS PERSIST     (NCHUNKS = 32-position chunks of the launch, CUS = what MMLF_CONV_CUS leaves,
//                                              PERSIST = 0: one workgroup per item, MMLF_WGRAD_PERSIST=0)
// prints one JSON object: "dims" = [workgroups, trips, slices, splits], "items" = for every workgroup g and trip t (g-major)
// the [slice, split] it runs there -- the kernel's loop b = g; b < items; b += workgroups -- or [-1, -1] where it has none.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include "wgrad_map.h"

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s CIN NCHUNKS CUS PERSIST\n", argv[0]);
        return 2;
    }
    const int Cin = atoi(argv[1]), cus = atoi(argv[3]);
    const long long nchunks = atoll(argv[2]);
    const bool persist = atoi(argv[4]) != 0;
    if (Cin <= 0 || nchunks <= 0 || cus <= 0) return 2;
    int nslice, nsplit;
    wgrad_wide_splits(Cin, nchunks, cus, nslice, nsplit);
    const int n = (int)wgrad_grid_blocks(nslice, nsplit);
    const int grid = (int)wgrad_wide_grid(n, cus, persist), trips = (n + grid - 1) / grid;
    printf("{\"dims\": [%d, %d, %d, %d], \"items\": [", grid, trips, nslice, nsplit);
    for (int g = 0; g < grid; ++g)
        for (int t = 0; t < trips; ++t) {
            int slice = -1, split = -1;
            const int b = g + t * grid;
            if (!(b < n && wgrad_block_map(b, nslice, nsplit, slice, split))) slice = split = -1;
            printf("%s[%d, %d]", g || t ? ", " : "", slice, split);
        }
    printf("]}\n");
    return 0;
}
