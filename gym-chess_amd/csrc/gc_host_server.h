// gc_host_server.h -- host side of the resident servers: the exit-time registry, the one
// server slot per device and the mailbox client shared by gc_env and gc_engine.
#pragma once

// ---- resident servers at process exit: a server wave exits after SRV_IDLE_MS without a
// request, so a process that ends right after its last call (without destroying the env or
// engine) could end with the wave still resident.  Every running server is registered here;
// an atexit handler asks each to QUIT through its host-mapped mailbox and waits (host memory
// only, no HIP call: the runtime may be tearing down) until it has marked its exit.
struct SrvReg {
    u32 *req_seq, *op, *exited;      // the mailbox (host-mapped)
    const u32 *seq, *launch;         // the owner's last served sequence number and launch id
};
static std::mutex g_srvreg_mu;
static std::vector<std::pair<const void*, SrvReg>> g_srvreg;
static void srv_quit_all() {
    std::lock_guard<std::mutex> lk(g_srvreg_mu);
    const bool log = getenv("GC_SRV_EXIT_LOG") != nullptr;  // (tests: which servers this stopped)
    for (auto& it : g_srvreg) {
        const SrvReg& r = it.second;
        if (!*r.launch || __atomic_load_n(r.exited, __ATOMIC_ACQUIRE) == *r.launch) continue;
        __atomic_store_n(r.op, (u32)SRV_QUIT, __ATOMIC_RELAXED);
        __atomic_store_n(r.req_seq, *r.seq + 1, __ATOMIC_RELEASE);
        const auto t0 = std::chrono::steady_clock::now();
        while (__atomic_load_n(r.exited, __ATOMIC_ACQUIRE) != *r.launch &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(2 * SRV_IDLE_MS)) {
        }
        if (log)
            fprintf(stderr, "gymchess: server of %p %s at exit\n", it.first,
                    __atomic_load_n(r.exited, __ATOMIC_ACQUIRE) == *r.launch ? "stopped" : "did not answer");
    }
    g_srvreg.clear();
}
static void srv_register(const void* owner, const SrvReg& r) {
    std::lock_guard<std::mutex> lk(g_srvreg_mu);
    static bool hooked = false;
    if (!hooked) {
        std::atexit(srv_quit_all);
        hooked = true;
    }
    for (auto& it : g_srvreg)
        if (it.first == owner) return;
    g_srvreg.emplace_back(owner, r);
}
static void srv_unregister(const void* owner) {
    std::lock_guard<std::mutex> lk(g_srvreg_mu);
    for (size_t k = 0; k < g_srvreg.size(); k++)
        if (g_srvreg[k].first == owner) {
            g_srvreg.erase(g_srvreg.begin() + (long)k);
            return;
        }
}

// ---- one resident server per device.  A resident wave holds its hardware
// queue until it exits, and HIP maps a process's streams onto GPU_MAX_HW_QUEUES (4 on the box)
// queues: with more streams than that, work on a stream that shares a queue with a resident
// server waits behind it until it idles out (SRV_IDLE_MS) -- ~50 ms per call for single-board
// envs stepped round-robin, or env.step mixed with ChessEngine calls.  So at most one server
// runs per device: a request to another owner's server, and every launch of this library on
// the device (SRV_QUIESCE, devsrv_quiesce), first stops the resident one (QUIT, its stream
// drained).  The slot's mutex is held for a whole server call (lock order: an engine's own
// mutex, then the slot's), so a server's state is only touched under it.
#define GC_MAX_DEVICES 64
struct DevSrv {
    std::recursive_mutex mu;
    std::atomic<void*> owner{nullptr};  // the env / engine whose server may be resident
    int (*stop)(void*) = nullptr;       // its stop (QUIT + drain)
};
static DevSrv g_devsrv[GC_MAX_DEVICES];
static DevSrv& devsrv(int dev) { return g_devsrv[(unsigned)dev % GC_MAX_DEVICES]; }
// (held: s.mu)
static int devsrv_stop_locked(DevSrv& s) {
    void* o = s.owner.exchange(nullptr, std::memory_order_acq_rel);
    return o ? s.stop(o) : 0;
}
// (Lock-free when no server is resident.  Callers on other threads may claim the slot between
// this check and their own launch: that launch then queues behind the new server until the
// server stops -- at the next call of another owner, or by itself after SRV_IDLE_MS without a
// request -- a delay, never a wrong result.)
static int devsrv_quiesce(int dev) {
    DevSrv& s = devsrv(dev);
    if (!s.owner.load(std::memory_order_acquire)) return 0;
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    return devsrv_stop_locked(s);
}
// (held: s.mu) the slot for `owner`: another owner's server is stopped first
static int devsrv_claim(DevSrv& s, void* owner, int (*stop)(void*)) {
    void* o = s.owner.load(std::memory_order_acquire);
    if (o && o != owner && devsrv_stop_locked(s)) return -1;
    s.stop = stop;
    s.owner.store(owner, std::memory_order_release);
    return 0;
}
static void devsrv_release(DevSrv& s, void* owner) {
    void* o = owner;
    s.owner.compare_exchange_strong(o, nullptr, std::memory_order_acq_rel);
}

// ---- the host side of one resident server (k_single_server for a gc_env, k_engine_server for
// a gc_engine): its mailbox `Box` (host-mapped; words req_seq / op / resp_seq / exited), its
// stream, the last request served, the launch running (0: none).  Held by value in its owner.
template <class Box>
struct SrvClient {
    const char* label;  // of its messages
    Box* box = nullptr;
    Box* box_d = nullptr;  // the mailbox's device address
    hipStream_t stream = nullptr;
    u32 seq = 0, launch = 0, next_launch = 0;

    // stop the server (if one runs) and wait until it has drained
    int stop(int device, void* owner) {
        DevSrv& s = devsrv(device);
        std::lock_guard<std::recursive_mutex> lk(s.mu);
        devsrv_release(s, owner);
        if (!launch) return 0;
        __atomic_store_n(&box->op, (u32)SRV_QUIT, __ATOMIC_RELAXED);
        __atomic_store_n(&box->req_seq, seq + 1, __ATOMIC_RELEASE);  // (never served: QUIT)
        const hipError_t he = hipStreamSynchronize(stream);
        __atomic_store_n(&box->req_seq, seq, __ATOMIC_RELEASE);
        launch = 0;
        if (he != hipSuccess) return fail(std::string(label) + ": " + hipGetErrorString(he));
        return 0;
    }
    // One request through the server, started on demand; the response is in *box afterwards.
    // write_request(box) stores the request's fields (relaxed; it may stop the server first, and
    // then claims the slot again); req_seq follows with release.  before_launch() runs ahead of
    // every (re)start, launch_fn(box_d, seq, launch) starts the kernel on `stream`; the server
    // serves every request past the seq it is started with.  stop_fn is the owner's stop.
    template <class WriteRequest, class BeforeLaunch, class Launch>
    int call(int device, void* owner, int (*stop_fn)(void*), WriteRequest write_request, BeforeLaunch before_launch,
             Launch launch_fn) {
        HIPCHK(hipSetDevice(device));
        DevSrv& s = devsrv(device);
        std::lock_guard<std::recursive_mutex> lk(s.mu);
        if (devsrv_claim(s, owner, stop_fn)) return -1;
        if (!box) {
            HIPCHK(hipHostMalloc((void**)&box, sizeof(Box), hipHostMallocMapped | hipHostMallocCoherent));
            host_fill(box, sizeof(Box));
            memset(box, 0, sizeof(Box));
            HIPCHK(hipHostGetDevicePointer((void**)&box_d, box, 0));
            HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        }
        if (write_request(box)) return -1;
        const u32 want = seq + 1;
        __atomic_store_n(&box->req_seq, want, __ATOMIC_RELEASE);  // last: the device reads the request at once
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned k = 0;; k++) {
            if (!launch || __atomic_load_n(&box->exited, __ATOMIC_ACQUIRE) == launch) {
                // no server, or it exited (idle) before seeing this request: (re)start it
                if (launch) HIPCHK(hipStreamSynchronize(stream));  // drained (idle exit)
                if (before_launch()) return -1;
                launch = ++next_launch;
                srv_register(owner, SrvReg{&box->req_seq, &box->op, &box->exited, &seq, &launch});
                launch_fn(box_d, seq, launch);
                HIPCHK(hipGetLastError());
            }
            if (__atomic_load_n(&box->resp_seq, __ATOMIC_ACQUIRE) == want) break;
            if ((k & 1023) == 1023) {  // a faulted server: the stream says so
                const hipError_t q = hipStreamQuery(stream);
                if (q != hipSuccess && q != hipErrorNotReady) return fail(std::string(label) + ": " + hipGetErrorString(q));
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
                    (void)stop(device, owner);
                    return fail(std::string(label) + ": no answer within 10 s");
                }
            }
        }
        seq = want;
        return 0;
    }
    // (the owner goes away: stopped and unregistered before)
    void destroy() {
        if (stream) (void)hipStreamDestroy(stream);
        if (box) (void)hipHostFree(box);
    }
};
