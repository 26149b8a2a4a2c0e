// host_resources.h - owning wrappers of the device resources the host layer holds: memory, events, streams, and a
// timed span (two events and a "recorded, not yet read" flag).  Host-only; every hipMalloc / hipFree, event and stream
// creation and destruction of libtangency is in this file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

// The one decision about device calls.  destroy_handle / destroy_batch decide ONCE whether the runtime still answers
// (tangency_api.cpp: lifetime) and clear this flag around their `delete`: the destructors below then drop their handles without a
// HIP call.  Thread-local: every host thread tears down its own objects.
inline thread_local bool t_device_calls = true;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {                                   // the explicit early free
        if (p && t_device_calls) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // grow-only; a failed allocation leaves the buffer empty and no sticky error behind for the next launch's check
    hipError_t reserve(size_t want) {
        if (bytes >= want) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return e; }
        bytes = want;
        return hipSuccess;
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e && t_device_calls) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s && t_device_calls) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipError_t create_high_priority() {
        if (s) return hipSuccess;
        int lo = 0, hi = 0;                            // numerically lower = higher priority
        const hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        return e != hipSuccess ? e : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi);
    }
    operator hipStream_t() const { return s; }
};

// begin(stream) ... end(stream) bracket work on a stream; read() waits for the stop event, stores the elapsed time and
// clears the flag (no-op when nothing is pending).
struct Span {
    Event t0, t1;
    bool pending = false;                              // recorded by end(), not yet read
    hipError_t create() { const hipError_t e = t0.create(); return e != hipSuccess ? e : t1.create(); }
    hipError_t begin(hipStream_t st) { pending = false; return hipEventRecord(t0, st); }   // (an unread span is lost)
    hipError_t end(hipStream_t st) {
        const hipError_t e = hipEventRecord(t1, st);
        pending = e == hipSuccess;
        return e;
    }
    bool busy() const { return pending && hipEventQuery(t1) != hipSuccess; }   // recorded and still running
    hipError_t read(double& ms) {
        if (!pending) return hipSuccess;
        hipError_t e = hipEventSynchronize(t1);
        float f = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&f, t0, t1);
        if (e != hipSuccess) return e;
        ms = f;
        pending = false;
        return hipSuccess;
    }
};
