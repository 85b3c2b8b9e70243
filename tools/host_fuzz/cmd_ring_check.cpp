// What carries a group call from the caller's thread to a rank's worker (csrc/host/cmd_ring.hpp) without a GPU, for
// tests/test_cmd_ring_host.py, which builds this once with ThreadSanitizer and once with AddressSanitizer + UndefinedBehaviorSanitizer:
// the ring's order, back-pressure and sleep / wake-up handshake, the lifetime of a task's captured state, and the barrier's one verdict
// per generation.  Prints one line of counts; a failed check prints FAILED and exits 1.
#include "cmd_ring.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

using namespace evplp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

namespace {
constexpr size_t kCapacity = 96;          // group.cpp's kTaskBytes
struct Consumer;
using CTask = Task<Consumer, kCapacity>;
struct Consumer {
    Ring<CTask> ring;
    std::thread th;
    uint64_t next = 0;                    // the sequence number the next task must carry
    uint64_t bad = 0;                     // tasks out of order, or with a damaged state
    int nap_every = 0;                    // > 0: a short sleep every so many tasks, so that the producer meets a full ring
    void ran(uint64_t seq, bool intact) {
        if (seq != next || !intact) bad++;
        next++;
        if (nap_every && next % (uint64_t)nap_every == 0) std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
};

// the three sizes of plain state: none (the consumer's own count says which task it must be), 16 bytes, the capacity
struct Small { uint64_t seq, not_seq; int operator()(Consumer &c) const { c.ran(seq, (seq ^ not_seq) == ~0ull); return 0; } };
struct Full {
    uint64_t seq; unsigned char fill[kCapacity - 8];
    explicit Full(uint64_t s) : seq(s) { for (size_t i = 0; i < sizeof fill; i++) fill[i] = (unsigned char)(s * 31 + i); }
    int operator()(Consumer &c) const { bool same = true; for (size_t i = 0; i < sizeof fill; i++) same = same && fill[i] == (unsigned char)(seq * 31 + i); c.ran(seq, same); return 0; }
};
static_assert(sizeof(Full) == kCapacity, "the largest state a task takes");

static void start(Consumer &c, int spin_before_sleep) { c.ring.spin_before_sleep = spin_before_sleep; c.th = std::thread([&c] { c.ring.consume(c); }); }
static void quit(Consumer &c) { c.ring.post(CTask([](Consumer &) { return 1; })); c.th.join(); }

// One producer, four consumers: every consumer sees its tasks once and in post order; the napping one fills its ring; the producer's pauses,
// longer than the consumers' spin, put them to sleep, and the next post wakes them.
static void order_and_wakeup(uint64_t per_consumer, uint64_t &tasks, uint64_t &full_waits, uint64_t &sleeps) {
    constexpr int n = 4;
    std::vector<Consumer> cs(n);
    cs[0].nap_every = 5000;
    for (Consumer &c : cs) start(c, 200);
    for (uint64_t seq = 0; seq < per_consumer; seq++) {
        for (Consumer &c : cs) {
            if (seq % 3 == 0) c.ring.post(CTask([](Consumer &k) { k.ran(k.next, k.next % 3 == 0); return 0; }));
            else if (seq % 3 == 1) c.ring.post(CTask(Small{ seq, ~seq }));
            else c.ring.post(CTask(Full(seq)));
        }
        if (seq % 20000 == 19999) {        // a burst ends: nothing is lost or late -- once drained, all of it has run -- and the consumers go to sleep
            for (Consumer &c : cs) { c.ring.drain(); CHECK(c.next == seq + 1); }
            std::this_thread::sleep_for(std::chrono::milliseconds(3));
        }
    }
    for (Consumer &c : cs) { c.ring.drain(); CHECK(c.next == per_consumer && c.bad == 0); }
    for (Consumer &c : cs) { quit(c); tasks += c.next; full_waits += c.ring.full_waits; sleeps += c.ring.sleeps; }
    CHECK(cs[0].ring.full_waits > 0);
}

// A state that is not plain data, as the samples of a batched path trace are: a shared block of 768 bytes, and a member that counts its
// constructions and destructions and knows whether its task is running.
struct Samples { uint32_t word[192]; };
static std::atomic<uint64_t> g_constructed{ 0 }, g_destroyed{ 0 }, g_destroyed_running{ 0 };
struct Counted {
    bool running = false;
    Counted() { g_constructed++; }
    Counted(const Counted &) noexcept { g_constructed++; }
    ~Counted() { g_destroyed++; if (running) g_destroyed_running++; }
};
struct Shared {
    uint64_t seq; std::shared_ptr<const Samples> samples; Counted counted;
    int operator()(Consumer &c) {
        counted.running = true;
        bool same = samples.use_count() >= 1;
        for (int i = 0; i < 192; i++) same = same && samples->word[i] == (uint32_t)(seq * 192 + (uint64_t)i);
        c.ran(seq, same);
        counted.running = false;
        return 0;
    }
};
static void state_lifetime(uint64_t per_consumer, uint64_t &tasks) {
    constexpr int n = 2;
    {
        std::vector<Consumer> cs(n);
        cs[1].nap_every = 7000;
        for (Consumer &c : cs) start(c, 200);
        for (uint64_t seq = 0; seq < per_consumer; seq++) {         // (the ring is overrun ~1 500 times: every slot is constructed into and destroyed again)
            auto s = std::make_shared<Samples>();
            for (int i = 0; i < 192; i++) s->word[i] = (uint32_t)(seq * 192 + (uint64_t)i);
            const CTask task(Shared{ seq, std::move(s), Counted() });
            for (Consumer &c : cs) c.ring.post(task);                // every consumer its own copy, as post_all gives every worker
        }
        for (Consumer &c : cs) { c.ring.drain(); CHECK(c.next == per_consumer && c.bad == 0); }
        for (Consumer &c : cs) { quit(c); tasks += c.next; }
    }
    CHECK(g_constructed.load() > per_consumer * n && g_constructed.load() == g_destroyed.load() && g_destroyed_running.load() == 0);
}

// n parties, `generations` barriers; one party, picked at random, raises the flag right behind a random generation.  Every party keeps the
// verdict of every generation: all agree, 0 up to the generation the flag was raised behind, non-zero from the next one on.
static void barrier_verdicts(int n, int generations, uint32_t seed) {
    SpinBarrier barrier; barrier.n = n;
    std::atomic<int> failed{ 0 };
    std::mt19937 rng(seed);
    const int who = (int)(rng() % (uint32_t)n), when = (int)(rng() % (uint32_t)(generations - 1));
    std::vector<std::vector<char>> seen((size_t)n, std::vector<char>((size_t)generations, 0));
    auto party = [&](int p) {
        for (int gen = 0; gen < generations; gen++) {
            seen[(size_t)p][(size_t)gen] = (char)(barrier.wait(&failed) != 0);
            if (p == who && gen == when) failed.store(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> th;
    for (int p = 1; p < n; p++) th.emplace_back(party, p);
    party(0);
    for (std::thread &t : th) t.join();
    for (int gen = 0; gen < generations; gen++) {
        for (int p = 1; p < n; p++) CHECK(seen[(size_t)p][(size_t)gen] == seen[0][(size_t)gen]);
        CHECK(seen[0][(size_t)gen] == (gen > when ? 1 : 0));
    }
}

} // namespace

int main() {
    uint64_t tasks = 0, full_waits = 0, sleeps = 0, generations = 0;
    order_and_wakeup(200000, tasks, full_waits, sleeps);
    state_lifetime(100000, tasks);
    for (int n : { 2, 3, 8 }) { barrier_verdicts(n, 100000, 1000u + (uint32_t)n); generations += 100000; }
    std::printf("tasks %llu full_waits %llu sleeps %llu generations %llu constructed %llu destroyed %llu\n", (unsigned long long)tasks, (unsigned long long)full_waits,
                (unsigned long long)sleeps, (unsigned long long)generations, (unsigned long long)g_constructed.load(), (unsigned long long)g_destroyed.load());
    return 0;
}
