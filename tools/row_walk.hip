// Lists the thread walk of the row kernels (bn_rows_kernel, relu_slice_rows_kernel, bn_apply4_kernel, shift_pack_kernel's
// write-out) over one grid row, and the tile sizes of the layout and reduction kernels, on the host, by the very functions
// the kernels and their wrappers use (mmlf_amd/csrc/row_walk.h): no GPU needed.
//   hipcc --offload-arch=gfx950 -I mmlf_amd/csrc tools/row_walk.hip -o row_walk
//   ./row_walk walk CVN [LIMIT ...]     (CVN = channel groups per position, LIMIT = positions: the pitch, or a piece of it)
//     prints one JSON object: "walk" = [cvn, dx, dc], "rows" = per LIMIT {"limit", "threads" = for each of the 256 threads
//     [pairs visited, carries taken inside the row, 1 if the last of them took it out of the row], "hits" = how often pair
//     (x, cg) was visited, at index x * cvn + cg, "outside" = visits that fell outside [0, LIMIT) x [0, cvn)}
//   ./row_walk sizes N
//     prints {"groups" = groups of four that hold N channels, "pack_xt" / "unpack_xt" = positions per transpose tile of
//     mmlf_pack_nchw at cs = N / of mmlf_unpack_nchw at C = N, "reduce" = bn_reduce_body's [cvn, ppi] at C = N}
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "row_walk.h"

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "sizes") && atoi(argv[2]) > 0) {
        const int n = atoi(argv[2]);
        int cvn, ppi;
        reduce_walk(n, 4, cvn, ppi);
        printf("{\"groups\": %d, \"pack_xt\": %d, \"unpack_xt\": %d, \"reduce\": [%d, %d]}\n", row_groups(n, 4),
               pack_tile_positions(n), unpack_tile_positions(n), cvn, ppi);
        return 0;
    }
    if (argc < 3 || strcmp(argv[1], "walk") || atoi(argv[2]) <= 0) {
        fprintf(stderr, "usage: %s walk CVN [LIMIT ...] | %s sizes N\n", argv[0], argv[0]);
        return 2;
    }
    const RowWalk w = row_walk(atoi(argv[2]));
    printf("{\"walk\": [%d, %d, %d], \"rows\": [", w.cvn, w.dx, w.dc);
    for (int a = 3; a < argc; ++a) {
        const int limit = atoi(argv[a]);
        if (limit <= 0) return 2;
        std::vector<int> hits((size_t)limit * w.cvn, 0);
        int outside = 0;
        printf("%s{\"limit\": %d, \"threads\": [", a > 3 ? ", " : "", limit);
        for (int tid = 0; tid < ROW_THREADS; ++tid) {
            int x, cg, seen = 0, carries = 0, left = 0;
            bool in = row_walk_start(w, tid, limit, x, cg);
            while (in) {
                ++seen;
                if (x >= 0 && x < limit && cg >= 0 && cg < w.cvn) ++hits[(size_t)x * w.cvn + cg];
                else ++outside;
                const int x0 = x;
                in = row_walk_step(w, limit, x, cg);
                const bool carry = x - x0 != w.dx && x0 + w.dx < limit;        // taken while still inside the row
                carries += carry;
                left = !in && carry;                            // inside after (dx, dc), outside after the carry
            }
            printf("%s[%d, %d, %d]", tid ? ", " : "", seen, carries, left);
        }
        printf("], \"hits\": [");
        for (size_t i = 0; i < hits.size(); ++i) printf("%s%d", i ? ", " : "", hits[i]);
        printf("], \"outside\": %d}", outside);
    }
    printf("]}\n");
    return 0;
}
