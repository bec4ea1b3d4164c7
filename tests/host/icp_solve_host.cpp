// Stand-alone host build of the ICP kernels' shared point-to-plane solve (csrc/icp_solve.h solve_plane, what lane 0 of icp.hip and
// icp_dense.hip runs): no device, no launch.  tests/test_icp_solve_host_cpu.py compiles it under the address / undefined-behaviour
// sanitizers and checks what it writes against NumPy.
//
//     icp_solve_host <in> <out>
//
// in:  int32 count, then per system float64 sums[28] (the 21 upper entries of A row by row, b (6), the inlier count), R[9], t[3], s
// out: per system int32 status, float64 angle, translation, R[9], t[3] (the state as the solve leaves it: untouched when status != 0)
#include "../../tg-pose_amd/csrc/icp_solve.h"

#include <cstdio>

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: icp_solve_host <in> <out>\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb");
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) {
        fprintf(stderr, "icp_solve_host: cannot open the files\n");
        if (in) fclose(in);
        return 2;
    }
    int32_t count = 0;
    int rc = fread(&count, sizeof count, 1, in) == 1 ? 0 : 1;
    for (int32_t k = 0; k < count && rc == 0; ++k) {
        double rec[ICP_NV + 13];
        if (fread(rec, sizeof(double), ICP_NV + 13, in) != (size_t)(ICP_NV + 13)) { rc = 1; break; }
        IcpShared sh = {};
        for (int i = 0; i < 9; ++i) sh.R[i] = rec[ICP_NV + i];
        for (int i = 0; i < 3; ++i) sh.t[i] = rec[ICP_NV + 9 + i];
        sh.s = rec[ICP_NV + 12];
        double res[14] = {0.0, 0.0};
        const int32_t status = solve_plane(rec, sh, res[0], res[1]);
        for (int i = 0; i < 9; ++i) res[2 + i] = sh.R[i];
        for (int i = 0; i < 3; ++i) res[11 + i] = sh.t[i];
        if (fwrite(&status, sizeof status, 1, out) != 1 || fwrite(res, sizeof(double), 14, out) != 14) rc = 1;
    }
    fclose(in);
    if (fclose(out) != 0) rc = 1;
    return rc;
}
