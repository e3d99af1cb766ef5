// The PACKED fp16 matrix layout of the ViT kernels (include/imagescry_hip.h), in elements.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

// The embedding bank's layout (bank_layout.h, which counts in bytes and K steps): rows in tiles of 256, columns in K steps
// of 64 halves, stored [tile][K step][row][64 halves].  The 256 x 128 B block one K step of one tile needs is 32 KiB of
// contiguous memory and every 1 KiB LDS-DMA instruction reads one contiguous KiB; a head's 64 q / k / v values of a token
// are exactly one 128-byte segment, consecutive tokens 128 bytes apart, which is what the attention kernels read.
// (Measured on the ViT-B shapes: the GEMMs run at the same speed from row-major operands -- their cost is the
// epilogue traffic and the staging volume, not the access pattern.)
// Element (row, col) of a packed matrix of `cols` columns:
__host__ __device__ __forceinline__ size_t pk_offset(long long row, int col, int cols) {
    return (((size_t)(row >> 8) * (size_t)(cols >> 6) + (size_t)(col >> 6)) * 256 + (size_t)(row & 255)) * 64 + (size_t)(col & 63);
}
