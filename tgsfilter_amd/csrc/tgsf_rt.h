// tgsf_rt.h -- the host-side runtime layer of libtgsf and libtgsf_text: streams, events, copies, launches, the context's
// allocator and its error text.  Included by tgsf_lib.hip and tgsf_text.hip behind their kernels and their kErrorCap.  It is the include switch
// of the host layer: the HIP runtime here, the serial emulation's stand-ins (test infrastructure) from tgsf_emul_rt.h --
// same names, so the code that enqueues work is written once and has no conditional.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/tgsf.h"

#if defined(TGSF_EMUL)
#include "tgsf_emul_rt.h"
#else
#include <hip/hip_runtime.h>
typedef hipStream_t rt_stream;
typedef hipEvent_t rt_event;
static int rt_set_device(int device) { return (int)hipSetDevice(device); }
static int rt_malloc(void** p, size_t n) { return (int)hipMalloc(p, n ? n : 1); }
static void rt_free(void* p) { (void)hipFree(p); }
static void rt_host_free(void* p) { (void)hipHostFree(p); }
static int rt_memset(void* p, int v, size_t n, rt_stream s) { return (int)hipMemsetAsync(p, v, n, s); }
static int rt_h2d(void* d, const void* s, size_t n, rt_stream st) { return (int)hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, st); }
static int rt_d2h(void* d, const void* s, size_t n, rt_stream st) { return (int)hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, st); }
static int rt_stream_create(rt_stream* s) { return (int)hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
static void rt_stream_destroy(rt_stream s) { (void)hipStreamDestroy(s); }
static int rt_sync(rt_stream s) { return (int)hipStreamSynchronize(s); }
static int rt_device_sync() { return (int)hipDeviceSynchronize(); }
static int rt_stream_wait(rt_stream s, rt_event e) { return (int)hipStreamWaitEvent(s, e, 0); }
static int rt_event_create(rt_event* e) { return (int)hipEventCreate(e); }
static void rt_event_destroy(rt_event e) { if (e) (void)hipEventDestroy(e); }
static int rt_event_record(rt_event e, rt_stream s) { return (int)hipEventRecord(e, s); }
static int rt_event_sync(rt_event e) { return (int)hipEventSynchronize(e); }
static int rt_event_ms(float* ms, rt_event a, rt_event b) { return (int)hipEventElapsedTime(ms, a, b); }
static int rt_last_error() { return (int)hipGetLastError(); }         // (and clears it)
static const char* rt_errstr(int e) { return hipGetErrorString((hipError_t)e); }
#define TGSF_LAUNCH(kernel, grid, block, stream, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (stream), __VA_ARGS__)
#define TGSF_LAUNCH_COOP TGSF_LAUNCH
static unsigned grid_cap(unsigned g) { return g; }
#endif

// What tgsf_ctx and tgsf_text share: the device, the text of the last error, and the device memory handed out by dev_alloc,
// which dev_free_all releases at destroy.  alloc_slack: bytes added to every allocation -- libtgsf's kernels may read a
// little past an array's end (64); libtgsf_text's arrays are exact (0: its text has TGSF_TEXT_PAD instead).
struct rt_ctx {
    int device = 0;
    std::string error;
    std::vector<void*> allocs;
    size_t alloc_slack = 0;
};

static thread_local std::string g_create_error;       // the error of a create call that returned no object

static int fail(rt_ctx* c, int code, const char* fmt, ...)
{
    char buf[kErrorCap];                                  // (the including library's: its messages are cut where they were)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->error = buf; else g_create_error = buf;
    return code;
}

template <class T>
static int dev_alloc(rt_ctx* c, T** p, size_t count)
{
    void* v = nullptr;
    int e = rt_malloc(&v, count * sizeof(T) + c->alloc_slack);
    if (e) return fail(c, TGSF_E_HIP, "device allocation of %zu bytes failed: %s", count * sizeof(T), rt_errstr(e));
    c->allocs.push_back(v);
    *p = (T*)v;
    return 0;
}

static void dev_free_all(rt_ctx* c) { for (void* p : c->allocs) rt_free(p); }
