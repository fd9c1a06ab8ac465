// gc_host_hip.h -- HIP error checks, launch geometry and device temporaries of the host code.
#pragma once

#define HIPCHK(x)                                                                   \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

static inline int grid_for(int n) { return (n + BLOCK - 1) / BLOCK; }
// one lane per slot of a table of `slots` entries
static inline unsigned grid_for_slots(size_t slots) { return (unsigned)((slots + BLOCK - 1) / BLOCK); }

// GC_ALLOC_FILL=<hex byte> (per call; tests): every fresh device or pinned host allocation is
// filled with that byte before it is handed out, so a read of memory nothing wrote shows as a
// wrong result instead of the zeroes a fresh process usually gets.  -1: unset (or not a byte).
static std::atomic<unsigned long long> g_fill_allocs{0}, g_fill_bytes{0};
static int alloc_fill_byte() {
    const char* s = getenv("GC_ALLOC_FILL");
    if (!s || !*s) return -1;
    char* end = nullptr;
    const unsigned long v = strtoul(s, &end, 16);
    return (end == s || *end || v > 0xFF) ? -1 : (int)v;
}
static void alloc_fill_count(size_t bytes) {
    g_fill_allocs++;
    g_fill_bytes += bytes;
}
// a fresh device buffer: the fill is complete on return, whichever stream the caller uses next
static int dev_fill(void* p, size_t bytes) {
    const int fb = alloc_fill_byte();
    if (fb < 0) return 0;
    hipError_t e = hipMemset(p, fb, bytes);  // (the null stream; the library's own are non-blocking)
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(std::string("alloc fill: ") + hipGetErrorString(e));
    alloc_fill_count(bytes);
    return 0;
}
// its twin for a fresh hipHostMalloc'd buffer (the explicit initial stores follow it)
static void host_fill(void* p, size_t bytes) {
    const int fb = alloc_fill_byte();
    if (fb < 0) return;
    memset(p, fb, bytes);
    alloc_fill_count(bytes);
}

template <class T>
static int dalloc(T** p, size_t count) {
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)p, count * sizeof(T));
    if (e != hipSuccess) return fail(std::string("hipMalloc: ") + hipGetErrorString(e));
    if (dev_fill(*p, count * sizeof(T))) {
        (void)hipFree(*p);
        *p = nullptr;
        return -1;
    }
    return 0;
}

// One call's device temporaries: every buffer it hands out (dalloc: a synchronous hipMalloc, at
// the point of the call) is hipFree'd, and every event destroyed, when the holder goes out of
// scope.  With a stream, that stream is drained first: nothing in flight may still use them.
class Temps {
public:
    Temps() = default;
    explicit Temps(hipStream_t drain) : drain_(drain), has_drain_(true) {}
    Temps(const Temps&) = delete;
    Temps& operator=(const Temps&) = delete;
    ~Temps() {
        if (has_drain_) (void)hipStreamSynchronize(drain_);
        for (void* p : bufs_) (void)hipFree(p);
        for (hipEvent_t ev : evs_) (void)hipEventDestroy(ev);
    }
    template <class T>
    int alloc(T** p, size_t count) {
        if (dalloc(p, count)) return -1;
        bufs_.push_back(*p);
        return 0;
    }
    // free p now (a buffer that is outgrown within the call)
    template <class T>
    void drop(T*& p) {
        forget(p);
        (void)hipFree(p);
        p = nullptr;
    }
    // p outlives the call: its new owner frees it
    void keep(void* p) { forget(p); }
    // a timing event, or null
    hipEvent_t event() {
        hipEvent_t ev = nullptr;
        if (hipEventCreate(&ev) != hipSuccess) return nullptr;
        evs_.push_back(ev);
        return ev;
    }
    const std::vector<hipEvent_t>& events() const { return evs_; }

private:
    void forget(void* p) {
        for (size_t k = 0; k < bufs_.size(); k++)
            if (bufs_[k] == p) {
                bufs_.erase(bufs_.begin() + (long)k);
                return;
            }
    }
    std::vector<void*> bufs_;
    std::vector<hipEvent_t> evs_;
    hipStream_t drain_ = nullptr;
    bool has_drain_ = false;
};
