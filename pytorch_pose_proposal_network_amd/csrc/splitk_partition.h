// Slab partition and workspace arithmetic of the split-K convolution (conv_splitk.hip).  Host-only, no HIP types: the same
// functions are compiled into libppn.so and into tools/splitk_partition_check.cpp, a stand-alone program that walks every
// workspace index the kernels form and runs under the host sanitizers.
#pragma once
#include <cstdint>

namespace ppnsplitk {

// K ELEMENTS per slab.  512 = one 3x3 tap of a 512-wide layer = 8 K steps of 64 in the 16-bit modes, 16 steps of 32 in the
// f32 mode: a slab is the same piece of the sum in every dtype (so the workspace has one size per layer, not one per dtype),
// it is long enough that the 2-stage pipeline's prologue and the accumulator store are a small part of a workgroup's
// life, and the 512-wide 3x3 layers -- the ones whose lone launch leaves most CUs idle -- cut into 9 slabs.
// A function of K alone: never of M, the batch or the CU count, so image i's sums are formed identically whether it runs
// alone or beside others.
constexpr int kSlabElems = 512;
constexpr int kTileP = 128, kTileC = 64;   // pixel x channel tile of one partial workgroup

struct Partition {
    int bk;                // K elements per step: 32 (f32) / 64 (16-bit)
    int nsteps;            // k_total / bk
    int steps_per_slab;    // kSlabElems / bk
    int slabs;             // ceil(nsteps / steps_per_slab); the last slab may be ragged
    long long m;           // output pixels
    int cout_pad;          // workspace row length (f32 elements)
    long long ws_bytes;    // slabs * m * cout_pad * 4
};

// false: the shape cannot be partitioned (k_total not a positive multiple of the K step, or sizes out of range)
inline bool partition(bool f32, int k_total, long long m, int cout_pad, Partition* p) {
    const int bk = f32 ? 32 : 64;
    if (k_total < bk || k_total % bk != 0 || m < 1 || m > 0x7fffffffLL || cout_pad < 1 || cout_pad > (1 << 20)) return false;
    p->bk = bk;
    p->nsteps = k_total / bk;
    p->steps_per_slab = kSlabElems / bk;
    p->slabs = (p->nsteps + p->steps_per_slab - 1) / p->steps_per_slab;
    p->m = m;
    p->cout_pad = cout_pad;
    // slabs <= 2^26 / 8, m < 2^31, cout_pad <= 2^20: below 2^63 by construction
    p->ws_bytes = (long long)p->slabs * m * cout_pad * 4;
    return true;
}

// K steps [*s0, *s1) of slab `slab`
inline void slab_steps(const Partition& p, int slab, int* s0, int* s1) {
    *s0 = slab * p.steps_per_slab;
    const int e = *s0 + p.steps_per_slab;
    *s1 = e < p.nsteps ? e : p.nsteps;
}

// f32 index of (slab, pixel m, channel c) in workspace[slab][pixel][cout_pad]
inline long long ws_index(const Partition& p, int slab, long long m, int c) {
    return ((long long)slab * p.m + m) * p.cout_pad + c;
}

}  // namespace ppnsplitk
