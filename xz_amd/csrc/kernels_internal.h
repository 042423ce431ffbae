// kernels_internal.h -- what one HIP unit of the encoder calls in another: C++ linkage, hidden, not in kernels_api.h.
#ifndef XZAMD_KERNELS_INTERNAL_H
#define XZAMD_KERNELS_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// lzma_build.hip, for xzk_span_plan: *order_out (one of val_a / val_b) = 0..n-1 stably sorted by the keys in key_a.
// key_b, val_a, val_b: n u32 of scratch each; tmp: xzk_sort_temp_bytes(n, 32) bytes.
__attribute__((visibility("hidden")))
hipError_t sort_launch_order(uint32_t* key_a, uint32_t* key_b, uint32_t* val_a, uint32_t* val_b, uint32_t n,
        void* tmp, size_t tmp_bytes, uint32_t** order_out, hipStream_t st);

#endif
