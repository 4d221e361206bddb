// operands.hpp — the interval test behind the operand rule of include/bx_hal.h ("Operand overlap").  Host-only and free of HIP headers:
// ctx.hpp includes it for the entry points, tests/operand_overlap_check.cpp includes it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/bx_hal.h"

namespace bx {

// Do the byte intervals [dptr, dptr + 4 * len) of two operands share a byte?
// An empty buffer overlaps nothing, whatever its pointer.  Written with distances, never with an end address: a buffer that ends at
// the top of the address space (or a hostile len) must not wrap into a small `end` and pass.
inline bool bufs_overlap(bx_buf a, bx_buf b) {
    if (!a.len || !b.len) return false;
    const uintptr_t pa = (uintptr_t)a.dptr, pb = (uintptr_t)b.dptr;
    const uintptr_t gap = pa <= pb ? pb - pa : pa - pb;  // the lower buffer reaches the higher one if it is longer than the gap
    const size_t low_len = pa <= pb ? a.len : b.len;
    return gap / 4 < low_len;
}
// the same start and the same length: the only overlap an element-wise entry point accepts
inline bool bufs_same(bx_buf a, bx_buf b) { return a.dptr == b.dptr && a.len == b.len; }

}  // namespace bx
