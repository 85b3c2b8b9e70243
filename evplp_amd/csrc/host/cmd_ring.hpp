// What crosses from the caller's thread to a rank's worker thread (group.cpp), and what the workers meet at: a task with inline storage, the
// single-producer / single-consumer ring that carries it, and the workers' barrier.  Host only and free of HIP, so that
// tools/host_fuzz/cmd_ring_check.cpp can run all three under ThreadSanitizer and AddressSanitizer (tests/test_cmd_ring_host.py).
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>

#pragma GCC visibility push(hidden)
namespace evplp {
constexpr int kRing = 64;
constexpr int kSpinBeforeSleep = 200000;     // ~1-2 ms of polling before an idle worker goes to sleep on its condition variable

// A callable `int (W &)` held in Capacity bytes of its own: making, copying and running one never allocates.  Copyable, because every
// worker of a group gets its own copy of a posted task; a state that is not plain data (the shared samples of a batched path trace) is
// copied and destroyed through `manage`, plain data by memcpy.
template <class W, size_t Capacity>
class Task {
    int (*call)(void *, W &) = nullptr;
    void (*manage)(void *dst, const void *src) = nullptr;      // src ? copy-construct *dst from *src : destroy *dst; null for plain data
    uint32_t bytes = 0;
    alignas(8) unsigned char state[Capacity];
    void take(const Task &o) {
        call = o.call; manage = o.manage; bytes = o.bytes;
        if (manage) manage(state, o.state); else std::memcpy(state, o.state, bytes);
    }
public:
    Task() {}
    template <class F, class = std::enable_if_t<!std::is_same<std::decay_t<F>, Task>::value>>
    Task(F f) {
        static_assert(sizeof(F) <= Capacity, "the captured state does not fit a task: capture less, or raise the capacity and look at the ring slot's size");
        static_assert(alignof(F) <= 8, "the captured state is aligned more strictly than a task's storage");
        static_assert(std::is_nothrow_copy_constructible<F>::value, "a task is copied into every worker's ring");
        new (state) F(std::move(f));
        bytes = (uint32_t)sizeof(F);
        call = [](void *s, W &w) -> int { return (*static_cast<F *>(s))(w); };
        if (!(std::is_trivially_copyable<F>::value && std::is_trivially_destructible<F>::value))
            manage = [](void *dst, const void *src) { if (src) new (dst) F(*static_cast<const F *>(src)); else static_cast<F *>(dst)->~F(); };
    }
    Task(const Task &o) { take(o); }
    Task &operator=(const Task &o) { if (this != &o) { reset(); take(o); } return *this; }
    ~Task() { reset(); }
    void reset() { if (manage) manage(state, nullptr); call = nullptr; manage = nullptr; bytes = 0; }
    int operator()(W &w) { return call(state, w); }
};

// Single producer (post, drain), single consumer (consume).  While the consumer polls, a post takes no contended lock and makes no system
// call; a consumer that found nothing for `spin_before_sleep` polls sleeps on the condition variable, and the producer -- which reads
// `sleeping` under the mutex, behind its seq_cst store of `tail` -- wakes it.
template <class T>
struct Ring {
    T slot[kRing];
    alignas(64) std::atomic<uint64_t> head{ 0 };      // consumed
    alignas(64) std::atomic<uint64_t> tail{ 0 };      // posted
    std::mutex m; std::condition_variable cv; bool sleeping = false;
    int spin_before_sleep = kSpinBeforeSleep;
    uint64_t full_waits = 0;                          // posts that met a full ring (the producer's)
    uint64_t sleeps = 0;                              // times the consumer slept and was woken (the consumer's)

    void post(const T &task) {
        const uint64_t t = tail.load(std::memory_order_relaxed);
        if (t - head.load(std::memory_order_acquire) >= (uint64_t)kRing) {      // (the ring is full: the caller is 64 calls ahead)
            full_waits++;
            while (t - head.load(std::memory_order_acquire) >= (uint64_t)kRing) std::this_thread::yield();
        }
        slot[t % kRing] = task;
        tail.store(t + 1, std::memory_order_seq_cst);
        std::lock_guard<std::mutex> lk(m);            // (uncontended while the consumer polls; pairs with the consumer's check before it sleeps)
        if (sleeping) cv.notify_one();
    }
    // the consumer's loop: every task in post order, run where it lies; a task that returns non-zero ends the loop.  The slot goes back to
    // the producer only when the task has finished and its state is destroyed.
    template <class W>
    void consume(W &w) {
        for (;;) {
            const uint64_t h = head.load(std::memory_order_relaxed);
            int spins = 0;
            while (tail.load(std::memory_order_acquire) == h) {
                if (++spins < spin_before_sleep) { if ((spins & 63) == 0) std::this_thread::yield(); continue; }
                std::unique_lock<std::mutex> lk(m);
                sleeping = true;
                cv.wait(lk, [&] { return tail.load(std::memory_order_acquire) != h; });
                sleeping = false;
                sleeps++;
                spins = 0;
            }
            T &task = slot[h % kRing];
            const int quit = task(w);
            task.reset();
            head.store(h + 1, std::memory_order_release);
            if (quit) return;
        }
    }
    // (the producer's, or any thread's that only wants the consumer idle) until everything posted has run
    void drain() { int spins = 0; while (head.load(std::memory_order_acquire) != tail.load(std::memory_order_acquire)) { if (++spins > 1000) std::this_thread::yield(); } }
};

// sense-reversing barrier of the workers (spins: the waits are microseconds long, in front of a collective).  wait(flag) returns ONE
// verdict for all parties of a generation: the last arriver reads `flag` once, in front of flipping the sense, and everybody leaves with
// what it read -- a rank that fails right behind the barrier cannot make its peers disagree about whether the collective is entered.
struct SpinBarrier {
    std::atomic<int> count{ 0 }; std::atomic<int> sense{ 0 }; std::atomic<int> verdict{ 0 }; int n = 1;
    int wait(const std::atomic<int> *flag = nullptr) {
        const int s = sense.load(std::memory_order_acquire);
        if (count.fetch_add(1, std::memory_order_acq_rel) == n - 1) {
            count.store(0, std::memory_order_relaxed);
            verdict.store(flag ? flag->load(std::memory_order_acquire) : 0, std::memory_order_relaxed);
            sense.store(s ^ 1, std::memory_order_release);
        } else { int spins = 0; while (sense.load(std::memory_order_acquire) == s) { if (++spins > 2000) std::this_thread::yield(); } }
        // (the verdict of THIS generation: the next one's last arriver cannot overwrite it before every party of this one has arrived there,
        // i.e. has returned from here)
        return verdict.load(std::memory_order_relaxed);
    }
};
} // namespace evplp
#pragma GCC visibility pop
