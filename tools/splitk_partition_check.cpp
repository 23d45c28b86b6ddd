// Stand-alone host check of the split-K partition and workspace arithmetic (csrc/splitk_partition.h), meant to be built with
// the host sanitizers and run directly:
//     g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I pytorch_pose_proposal_network_amd/csrc \
//         tools/splitk_partition_check.cpp -o splitk_partition_check && ./splitk_partition_check
// For each shape it allocates a byte per workspace element of EXACTLY ws_bytes / 4, walks every (channel tile, pixel tile,
// slab, lane) store the partial kernel makes and every load the reduce kernel makes with the same index expressions, and
// checks: the slabs tile [0, nsteps) without gap or overlap, every store lands inside the buffer (the sanitizer sees one
// that does not), no element is stored twice, and every element the reduce kernel loads was stored.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "splitk_partition.h"

using namespace ppnsplitk;

static int check(bool f32, int cin, int ksize, long long m, int cout, int cout_pad, int want_slabs) {
    Partition p;
    const int k_total = ksize * ksize * cin;
    if (!partition(f32, k_total, m, cout_pad, &p)) { printf("partition refused %d %lld %d\n", k_total, m, cout_pad); return 1; }
    if (p.slabs != want_slabs) { printf("K %d %s: %d slabs, expected %d\n", k_total, f32 ? "f32" : "16-bit", p.slabs, want_slabs); return 1; }
    int next = 0;
    for (int s = 0; s < p.slabs; ++s) {
        int s0, s1;
        slab_steps(p, s, &s0, &s1);
        if (s0 != next || s1 <= s0 || s1 - s0 > p.steps_per_slab) { printf("slab %d covers [%d, %d)\n", s, s0, s1); return 1; }
        next = s1;
    }
    if (next != p.nsteps) { printf("slabs end at step %d of %d\n", next, p.nsteps); return 1; }
    std::vector<unsigned char> ws((size_t)(p.ws_bytes / 4), 0);
    unsigned char* w = ws.data();                       // raw pointer: an index past the end is the sanitizer's to catch
    const long long n_pt = (m + kTileP - 1) / kTileP;
    const int n_ct = cout_pad / kTileC;
    for (int s = 0; s < p.slabs; ++s)
        for (long long pt = 0; pt < n_pt; ++pt)
            for (int ct = 0; ct < n_ct; ++ct)
                for (int px = 0; px < kTileP; ++px)
                    for (int c4 = 0; c4 < kTileC; c4 += 4) {        // one lane's 16-byte store
                        const long long mm = pt * kTileP + px;
                        if (mm >= m) continue;
                        for (int r = 0; r < 4; ++r) {
                            unsigned char& e = w[ws_index(p, s, mm, ct * kTileC + c4 + r)];
                            if (e) { printf("element stored twice\n"); return 1; }
                            e = 1;
                        }
                    }
    for (long long mm = 0; mm < m; ++mm)
        for (int c = 0; c < cout; c += 8)
            for (int s = 0; s < p.slabs; ++s)
                for (int r = 0; r < 8; ++r)
                    if (!w[ws_index(p, s, mm, c + r)]) { printf("reduce loads an element nobody stored\n"); return 1; }
    printf("ok  %s K %5d  M %4lld  cout %3d/%3d  slabs %d  workspace %lld bytes\n", f32 ? "f32   " : "16-bit", k_total, m, cout,
           cout_pad, p.slabs, p.ws_bytes);
    return 0;
}

int main() {
    int bad = 0;
    // the shapes of tests/test_splitk_gpu.py, then K = exactly one slab and one step, and a 24 x 24 512-wide layer
    bad += check(false, 128, 3, 99, 200, 256, 3) + check(true, 128, 3, 99, 200, 256, 3);
    bad += check(false, 512, 1, 70, 64, 64, 1) + check(true, 512, 1, 70, 64, 64, 1);
    bad += check(false, 576, 1, 70, 64, 64, 2) + check(true, 576, 1, 70, 64, 64, 2);
    bad += check(false, 64, 3, 70, 128, 128, 2) + check(true, 64, 3, 70, 128, 128, 2);
    bad += check(false, 64, 3, 36, 40, 64, 2) + check(false, 64, 3, 216, 64, 64, 2);
    bad += check(false, 64, 1, 1, 8, 64, 1) + check(true, 32, 1, 129, 72, 128, 1);
    bad += check(false, 512, 3, 576, 512, 512, 9) + check(true, 512, 3, 576, 512, 512, 9);
    Partition p;
    if (partition(false, 0, 1, 64, &p) || partition(false, 100, 1, 64, &p) || partition(true, 64, 0, 64, &p) ||
        partition(true, 64, 1LL << 31, 64, &p)) { printf("a bad shape was accepted\n"); ++bad; }
    printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
