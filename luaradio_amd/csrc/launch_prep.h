// launch_prep.h - what a launch settles before it goes: the kernel's dynamic-LDS limit, its resident workgroups per CU, the grid of a persistent kernel.
#pragma once
#include "common.h"

namespace lrhip {

// One table per process (one device per process, no use after fork(): ensure_init), behind a mutex: the library is entered from several host threads
// (CopyPool's comment), and stages share kernels.  An entry is a launch shape that has been prepared; threads = 0: its LDS size was allowed, no more
struct KernelPrep {
    struct Entry { const void *kern; int threads; size_t lds_bytes; int per_cu; };
    std::mutex m;
    std::vector<Entry> seen;
    // (m held) The limit only ever goes up: a stage that needs less than another one sharing the kernel must not take the other's launches away
    int allow_lds(const void *kern, size_t lds_bytes)
    {
        if (lds_bytes <= 48 * 1024) return 0;
        for (const Entry &e : seen)
            if (e.kern == kern && e.lds_bytes >= lds_bytes) return 0;
        LR_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        seen.push_back({kern, 0, lds_bytes, 0});
        return 0;
    }
};
inline KernelPrep kernel_prep;

// a launch with lds_bytes of dynamic LDS is allowed (one-shot grids, which need no occupancy figure).  0, or -1 with the message set
template <typename K>
inline int kernel_allow_lds(K kern, size_t lds_bytes)
{
    std::lock_guard<std::mutex> lk(kernel_prep.m);
    return kernel_prep.allow_lds((const void *)kern, lds_bytes);
}

// resident workgroups per CU (at least 1) of a launch of `threads` threads and lds_bytes of dynamic LDS, which is allowed from here on: asked of
// the runtime once per (kernel, threads, lds_bytes).  -1 with the message set
template <typename K>
inline int kernel_slots(K kern, int threads, size_t lds_bytes)
{
    const void *kp = (const void *)kern;
    std::lock_guard<std::mutex> lk(kernel_prep.m);
    for (const KernelPrep::Entry &e : kernel_prep.seen)
        if (e.kern == kp && e.threads == threads && e.lds_bytes == lds_bytes) return e.per_cu;
    if (kernel_prep.allow_lds(kp, lds_bytes)) return -1;
    int nb = 0;
    LR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kp, threads, lds_bytes));
    kernel_prep.seen.push_back({kp, threads, lds_bytes, nb < 1 ? 1 : nb});
    return kernel_prep.seen.back().per_cu;
}
// ... on the whole chip
template <typename K>
inline long chip_slots(K kern, int threads, size_t lds_bytes)
{
    const int per_cu = kernel_slots(kern, threads, lds_bytes);
    return per_cu < 0 ? -1 : (long)ctx().num_cus * per_cu;
}

// Tile order of a persistent kernel: 0 = as many workgroups as are resident, each striding through the work; rounds > 0 = workgroups of `rounds`
// consecutive items, handed out in address order (grid_for's comment).  A launch that fits the resident slots has nothing to order.
inline int persistent_rounds(long work, long slots, int knob) { return work > slots && knob > 0 ? knob : 0; }
inline unsigned persistent_grid(long work, long slots, int rounds)
{
    return rounds > 0 ? (unsigned)((work + rounds - 1) / rounds) : (unsigned)(work < slots ? work : slots);
}

}  // namespace lrhip
