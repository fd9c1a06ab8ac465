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

template <class T>
static int dalloc(T** p, size_t count) {
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)p, count * sizeof(T));
    if (e != hipSuccess) return fail(std::string("hipMalloc: ") + hipGetErrorString(e));
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
