// Stand-alone host build of the per-cloud persistence algorithm: csrc/persistence.hip's pd::pd_run with one lane (tid 0, nt 1),
// no device, no launch.  tests/test_pd_exact_cpu.py compiles it (plain and under the address / undefined-behaviour sanitizers) and
// checks what it writes with exact arithmetic.
//
//     pd_host <in> <out>
//
// in:  int32 count, then per cloud int32 n, int32 tet_cap, float32 points[n * 3]
// out: per cloud int32 status, int32 ntet, int32 counts[2], int32 tets[ntet * 4], float64 h1[counts[0] * 2], float64 h2[counts[1] * 2]
#include "../../tg-pose_amd/csrc/persistence.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

static bool get(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static bool put(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: pd_host <in> <out>\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb");
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) {
        fprintf(stderr, "pd_host: cannot open the files\n");
        if (in) fclose(in);
        return 2;
    }
    const size_t ws_bytes = pd::layout().total;
    void *ws = aligned_alloc(256, ws_bytes);
    std::vector<double> h1(2 * (size_t)pd::PAIRCAP), h2(2 * (size_t)pd::PAIRCAP);
    std::vector<int32_t> tets(4 * (size_t)pd::TCAP);
    std::vector<float> pc;
    int32_t count = 0;
    int rc = ws && get(in, &count, sizeof count) ? 0 : 1;
    for (int32_t k = 0; k < count && rc == 0; ++k) {
        int32_t hdr[2];
        if (!get(in, hdr, sizeof hdr) || hdr[0] < 1 || hdr[0] > pd::NMAX || hdr[1] < 0) { rc = 1; break; }
        pc.resize(3 * (size_t)hdr[0]);
        if (!get(in, pc.data(), pc.size() * sizeof(float))) { rc = 1; break; }
        int32_t counts[2] = {0, 0}, status = 0, ntet = 0;
        tgp_pd_args a = {};
        a.B = 1;
        a.N = hdr[0];
        a.pcl = pc.data();
        a.workspace = ws;
        a.h1 = h1.data();
        a.h2 = h2.data();
        a.counts = counts;
        a.status = &status;
        a.tets = tets.data();
        a.ntet = &ntet;
        a.tet_cap = hdr[1];
        int sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        pd::Cloud c = pd::cloud_at(a, 0);
        c.sc = sc;
        pd::pd_run(c, 0, 1);
        const int32_t head[4] = {status, ntet, counts[0], counts[1]};
        if (!put(out, head, sizeof head) || !put(out, tets.data(), sizeof(int32_t) * 4 * (size_t)ntet)
            || !put(out, h1.data(), sizeof(double) * 2 * (size_t)counts[0]) || !put(out, h2.data(), sizeof(double) * 2 * (size_t)counts[1]))
            rc = 1;
    }
    free(ws);
    fclose(in);
    if (fclose(out) != 0) rc = 1;
    if (rc) fprintf(stderr, "pd_host: short read or write\n");
    return rc;
}
