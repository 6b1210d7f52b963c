// Host threads of libfdx: the process's CPU budget and the standing pool of the restated cKDTree's build (kdtree_host.cpp).
// Pure C++17 - no HIP, nothing of fdx_internal.h -, so the sanitizer programs of hosttest/ compile it with plain g++.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <vector>

namespace fdx {

// Host threads this process may keep busy: the hardware's count, cut to the CPU bandwidth quota of the control group the process
// runs in (containers: /sys/fs/cgroup/cpu.max or the v1 pair).  A burst on more threads than the quota covers gets the whole
// process - its main thread included - throttled for the rest of the scheduler period: on a 256-thread host with a 16-CPU quota
// the 128 query threads of one tie remedy cost the NEXT calls 10-30 ms stalls in unrelated places (measured; round 5).
unsigned host_cpu_budget();

// ---- one standing pool of host threads for everything the build does in parallel ------------------------------------------------
// The build's critical path is the chain root -> child -> grandchild: bounds, selection and partition of a million, half a
// million, a quarter of a million points, each a serial pass in scipy (12 + 6 + 3 ms of the 21 ms a million lattice points cost
// with the subtrees already on threads of their own).  Starting threads per pass costs more than the pass (tried, round 5);
// threads that are already waiting do not.  Everything parallel is a TASK of this pool - the chunks of a top node's pass
// (`parallel`), the `less` subtree of a large node (`spawn`) - and whoever waits for tasks of its own runs other tasks meanwhile
// (`wait_help`), so several nodes have their passes under way at once on the same 16 threads, and the process never has more
// than its share of the host's CPUs busy: a burst on 70 threads (teams per level + a thread per subtree, the first form of this
// round) leaves a 5 ms scheduler slice stranded on every CPU it touched, and a 16-CPU quota then throttles a whole period
// (3 of 28 periods in a 20-fit run: 10 ms steps among 32 ms ones).
// (What a build runs per pass is defined here, in the class, so that it inlines into the build; what starts, parks and ends the
// threads is in host_threads.cpp.)
class KdPool {
public:
    static KdPool& get() { static KdPool p; return p; }
    // members (the caller included) this build may keep busy; creates what is missing
    void want(int members);
    int size() const { return active_.load(); }
    // a task; *pending (may be NULL) is decremented when it has run
    void spawn(std::function<void()> fn, std::atomic<int>* pending) {
        if (pending) pending->fetch_add(1, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lk(m_);
            q_.push_back(Task{std::move(fn), pending});
            n_queued_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_one();
    }
    // runs tasks until *pending is zero
    // (a waiter with nothing to run spins briefly, then SLEEPS until a task is queued or a counter reaches zero: 32 members
    // spinning through a 10 ms build were 0.3 CPU-seconds per fit, and a 16-CPU quota throttled one step in five)
    void wait_help(std::atomic<int>& pending) {
        int idle = 0;
        while (pending.load(std::memory_order_acquire) != 0) {
            if (run_one()) { idle = 0; continue; }
            if (++idle < 400) { __builtin_ia32_pause(); continue; }
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return pending.load(std::memory_order_acquire) == 0 || !q_.empty(); });
            idle = 0;
        }
    }
    // f(tid, nt) for tid < nt, the caller taking tid 0 and whatever else nobody has started yet
    // (a chunk that throws - out of memory - sets *failed; the caller looks at it when the build is over)
    template <class F>
    void parallel(int nt, const F& f, std::atomic<bool>* failed) {
        if (nt <= 1) { f(0, 1); return; }
        std::atomic<int> pending{nt - 1};
        {                                                             // all chunks under one lock, one wake-up for everybody
            std::lock_guard<std::mutex> lk(m_);
            for (int tid = 1; tid < nt; ++tid)
                q_.push_back(Task{[&f, tid, nt, failed] { try { f(tid, nt); } catch (...) { failed->store(true); } }, &pending});
            n_queued_.fetch_add(nt - 1, std::memory_order_release);
        }
        cv_.notify_all();
        try { f(0, nt); } catch (...) { failed->store(true); }
        wait_help(pending);
    }
    ~KdPool();
private:
    struct Task { std::function<void()> fn; std::atomic<int>* pending; };
    bool run_one() {
        if (n_queued_.load(std::memory_order_acquire) == 0) return false;
        Task t;
        {
            std::lock_guard<std::mutex> lk(m_);
            if (q_.empty()) return false;
            t = std::move(q_.back());                                 // newest first: the chunks of a pass that has just been cut run
            q_.pop_back();                                            // before subtrees queued earlier - the passes are the critical path
            n_queued_.fetch_sub(1, std::memory_order_release);
        }
        t.fn();                                                       // (tasks catch what they throw)
        if (t.pending && t.pending->fetch_sub(1, std::memory_order_acq_rel) == 1) {
            { std::lock_guard<std::mutex> lk(m_); }                   // (a waiter between its test and its sleep holds this)
            cv_.notify_all();
        }
        return true;
    }
    void loop(int wid);
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Task> q_;
    std::atomic<int> n_queued_{0};
    std::vector<std::thread> th_;
    std::atomic<int> active_{1};
    bool stop_ = false;
    std::atomic<pid_t> pid_{getpid()};
};

}  // namespace fdx
