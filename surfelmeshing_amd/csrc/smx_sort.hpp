// smx_sort.hpp -- the LSD radix sort of smx_nn.hip (u64 key with u32 value, 8 bits per pass, stable), for the other
// translation units that order records on the device (internal).  The kernels stay in smx_nn.hip.
#pragma once

#include "smx_common.hpp"

namespace smx {

// Words of `hist` a sort of n records needs: the per-tile digit histograms and the levels of their scan.
size_t radix_sort_workspace_elems(size_t n);
// Sorts (keys[0], vals[0]) by the low `bits` bits; returns the index (0 / 1) of the buffers that hold the result.
int radix_sort(const DevBuf<unsigned long long> (&key_bufs)[2], const DevBuf<uint32_t> (&val_bufs)[2], uint32_t n, int bits,
               uint32_t* hist, hipStream_t st);

}  // namespace smx
