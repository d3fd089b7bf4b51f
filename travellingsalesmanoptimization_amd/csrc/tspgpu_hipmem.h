// The HIP backend of tspgpu_mem.h: the only place of the engine that allocates or frees device and pinned memory.
// fill and copy are asynchronous on `stream` (copy: device to device).
#pragma once
#include <hip/hip_runtime_api.h>
#include "tspgpu_mem.h"

struct __attribute__((visibility("hidden"))) HipMem {
    typedef hipError_t error;
    static constexpr error ok = hipSuccess;
    hipStream_t stream = nullptr;
    static error alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { hipFree(p); }
    static error alloc_pinned(void **p, size_t bytes) { return hipHostMalloc(p, bytes); }
    static void free_pinned(void *p) { hipHostFree(p); }
    error fill(void *p, int byte, size_t bytes) const { return hipMemsetAsync(p, byte, bytes, stream); }
    error copy(void *dst, const void *src, size_t bytes) const { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream); }
    error sync() const { return hipStreamSynchronize(stream); }
};
template <class T> using DevBuf = tspmem::DevBuf<HipMem, T>;
template <class T> using PinBuf = tspmem::PinBuf<HipMem, T>;
