// kz_launch.hpp — host-side launch plumbing the kernel translation units share.
#pragma once
#include <hip/hip_runtime.h>

#include <iterator>  // std::size, std::index_sequence: the launchers fold over their instance tables
#include <utility>

namespace kz {

// A kernel that takes more than 64 KB of dynamic LDS must be allowed to, per device: call this before every launch of
// it with the largest size any launch asks for.  The attribute is set once per (kernel, device, host thread); every
// later call costs hipGetDevice and one bit test.  Keyed by the KERNEL, not by its function type: two kernels of one type
// (kz_board_conv_f16 / kz_board_conv_split16, the instances of a kernel template) each have a mask of their own.
template <auto Kernel>
inline void allow_dynamic_lds(int bytes) {
    static thread_local unsigned long long done_mask = 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!((done_mask >> (dev & 63)) & 1)) {
        (void)hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        done_mask |= 1ull << (dev & 63);
    }
}

}  // namespace kz
