// hip_shims.hip -- one-line HIP runtime wrappers of kernels_api.h (memory, copies, streams, events, device queries).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_api.h"

extern "C" {

// --- thin runtime shims so the plain-C host layer needs no HIP headers ---------------------
int xzk_malloc(void** p, uint64_t bytes) { return (int)hipMalloc(p, bytes); }
int xzk_free(void* p) { return (int)hipFree(p); }
int xzk_host_alloc(void** p, uint64_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
int xzk_host_free(void* p) { return (int)hipHostFree(p); }
int xzk_h2d(void* d, const void* h, uint64_t bytes, void* st) { return (int)hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, (hipStream_t)st); }
int xzk_d2h(void* h, const void* d, uint64_t bytes, void* st) { return (int)hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, (hipStream_t)st); }
int xzk_d2d(void* d, const void* s, uint64_t bytes, void* st) { return (int)hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, (hipStream_t)st); }
int xzk_memset(void* d, int v, uint64_t bytes, void* st) { return (int)hipMemsetAsync(d, v, bytes, (hipStream_t)st); }
int xzk_sync(void* st) { return (int)hipStreamSynchronize((hipStream_t)st); }
int xzk_set_device(int dev) { return (int)hipSetDevice(dev); }
int xzk_get_device(int* dev) { return (int)hipGetDevice(dev); }
int xzk_device_count(int* n) { return (int)hipGetDeviceCount(n); }
int xzk_cu_count(int dev, int* cus) { return (int)hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev); }
int xzk_stream_create(void** st) { return (int)hipStreamCreateWithFlags((hipStream_t*)st, hipStreamNonBlocking); }
// lowest-priority stream of the device (work on it only fills slots the caller's stream leaves free)
int xzk_stream_create_low(void** st)
{
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    return (int)hipStreamCreateWithPriority((hipStream_t*)st, hipStreamNonBlocking, least);
}
int xzk_stream_wait_event(void* st, void* ev) { return (int)hipStreamWaitEvent((hipStream_t)st, (hipEvent_t)ev, 0); }
int xzk_stream_destroy(void* st) { return (int)hipStreamDestroy((hipStream_t)st); }
int xzk_event_create(void** ev) { return (int)hipEventCreate((hipEvent_t*)ev); }
int xzk_event_destroy(void* ev) { return (int)hipEventDestroy((hipEvent_t)ev); }
int xzk_event_record(void* ev, void* st) { return (int)hipEventRecord((hipEvent_t)ev, (hipStream_t)st); }
int xzk_event_elapsed_ms(void* a, void* b, float* ms) { return (int)hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b); }
int xzk_event_query(void* ev) { return (int)hipEventQuery((hipEvent_t)ev); }
const char* xzk_error_string(int e) { return hipGetErrorString((hipError_t)e); }
int xzk_mem_info(uint64_t* free_b, uint64_t* total_b)
{
    size_t f = 0, t = 0;
    hipError_t e = hipMemGetInfo(&f, &t);
    *free_b = f; *total_b = t;
    return (int)e;
}

} // extern "C"
