// gfw_layout.h — host only, no HIP: the layout of a block that goes to the device in one copy.  gfw_hostmem.h includes it for the entry points; the packers
// (gfw_*_host.h) include it alone, so that the CPU test tier compiles them without a HIP runtime.
#pragma once
#include <stddef.h>

// Parts back to back, each starting on a multiple of 8 (the blocks hold doubles and 64-bit keys behind arrays of any length).
struct BlockLayout {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t at = total; total = at + (bytes + 7) / 8 * 8; return at; }
};
