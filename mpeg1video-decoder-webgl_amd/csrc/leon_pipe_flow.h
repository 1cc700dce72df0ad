// leon_pipe_flow.h -- the thread protocol of leon_pipeline: who waits for what, who wakes them, who owns a GOP's job, a window
// and an arena at every moment.  Plain C++17 with no HIP include: leon_pipeline_impl.h does the device and parse work between the
// calls, tests/native/flow_check.cpp drives the same header with fake jobs and windows under ThreadSanitizer.
//
// THE PROTOCOL.  One mutex, one condition variable; every change of state below ends in notify_all, which is what keeps all the
// predicates live (the waiters are few, the wake-ups cheap: do not narrow one into notify_one).
//
//   who waits                     for what                                                          who wakes them
//   parser thread, take_gop       a free arena and a GOP of the run not yet taken                   release / retire (arena), seek (run)
//   parser thread, await_bytes    valid >= need, or the run replaced                                feed, seek
//   submit thread, take_window    windows of the run left and a free ring entry,                    release / retire (entry), seek (run)
//                                 then every GOP of the window parsed, or the run replaced          hand_parsed, seek
//   notify thread, next_event     a submitted window; else the submit thread's exit; else every     submitted, submit_exited,
//                                 window of the run delivered and its 'ended' not yet out           callback_returned, seek
//   caller, wait_run              finished, or the current run's 'ended' callback returned          ended_returned, finish
//   caller, seek                  no callback under way                                             callback_returned, ended_returned
//
// An arena is the ticket to parse ahead (there are W * (R + 1) of them), a ring entry the ticket to submit a window.  A job holds
// its arena from take_gop until it is retired, a window its ring entry and its jobs from take_window until it is retired: retire()
// is the one place either goes back, whichever way the job or window ends (released, drained after a seek, dropped at stop).
//
// A SEEK replaces the run and starts next_gop, run_submitted, run_done and run_ended over; window ids count on (the seek reports the
// next one).  What was parsed for the old run is retired at once.  What the threads still hold of it they find out themselves, by
// comparing the run they took with the current one: a parser drops its job (await_bytes, hand_parsed), the submit thread gives its
// ring entry back and takes a window of the new run (the id it took stays consumed), the notify thread retires a window of the old
// run that came back without error instead of delivering it.  A window past that point is delivered: the seek waits for its
// callback to return, so no delivery of the old run follows the seek's return.  Held windows stay held.
//
// STOP (fail, or stop_quiet at tear-down) ends every wait of the parser and submit threads: take_gop, await_bytes and take_window
// give back what they hold and report it, and the threads return.  The notify thread does not look at stop except to leave 'ended'
// out: it drains what was submitted, then exits once the submit thread has, and finish() lets wait_run go.  wait_run and seek do not
// wait for stop itself: a seek of a failed pipeline is refused, and a callback under way always returns.
#pragma once

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace leon_flow {

// One position of the pipeline: the one leon_pipeline_create starts at, then one per leon_pipeline_seek.  The parser and
// submit threads work for the current run only; what they hold of an earlier one is dropped.
struct PipeRun {
    uint64_t id = 0;             // counts the runs of the process (make_run): what was remembered of a run is recognised by it
    std::vector<uint32_t> mine;  // key-map ids the run decodes, in order (this shard's, from the entry it starts with)
    uint32_t first_key = 0;      // the key-map entry it starts with
    uint64_t total_gops = 0;     // mine.size() * loop
    int64_t total_windows = 0;
    double exact_ms = -1;        // LEON_PIPELINE_SEEK_EXACT: the first GOP's frames start at the one on screen at this time; < 0: all
};

// Of a Job the flow needs `run`, `gop`, `arena` (a ticket: any copyable type, never looked into) and `status`; of a Window `run`,
// `id`, `ring`, `jobs` (a std::vector<std::unique_ptr<Job>>) and `status`.  A status of 0 is "no error".
template <class Job, class Window>
class Flow {
public:
    using Run = std::shared_ptr<const PipeRun>;
    using Ticket = decltype(Job::arena);
    using Clock = std::chrono::steady_clock;

    // ---- before the threads start -------------------------------------------------------------------------------------------
    void begin(Run run, size_t valid)
    {
        std::lock_guard<std::mutex> lk(mu_);
        run_ = std::move(run);
        valid_ = valid;
    }
    void equip(int gops_per_window, int ring_entries, const std::vector<Ticket>& arenas)
    {
        std::lock_guard<std::mutex> lk(mu_);
        W_ = gops_per_window;
        ring_owner_.assign((size_t)ring_entries, -1);
        free_arenas_.assign(arenas.begin(), arenas.end());
    }

    // ---- parser threads -----------------------------------------------------------------------------------------------------
    // the next GOP of the run with an arena to parse it into: a job with run, gop and arena set; nullptr: stop.  Once every GOP of
    // the run is taken the thread waits here for a seek.
    std::unique_ptr<Job> take_gop()
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || (!free_arenas_.empty() && next_gop_ < run_->total_gops); });
        if (stop_) return nullptr;
        Run run = run_;
        const uint64_t g = next_gop_++;
        const Ticket arena = free_arenas_.front();
        free_arenas_.pop_front();
        lk.unlock();
        auto job = std::make_unique<Job>();
        job->run = std::move(run);
        job->gop = g;
        job->arena = arena;
        return job;
    }
    // a stream that is still arriving: the GOP's bytes [.., need) must be there
    enum class Bytes { Arrived, Replaced, Stop };       // Replaced (seeked away from while waiting), Stop: the job is retired
    Bytes await_bytes(std::unique_ptr<Job>& job, uint64_t need)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || valid_ >= need || run_ != job->run; });
        if (stop_) { retire(std::move(job)); return Bytes::Stop; }
        if (run_ == job->run) return Bytes::Arrived;
        retire(std::move(job));
        lk.unlock();
        cv_.notify_all();
        return Bytes::Replaced;
    }
    // a parsed job (whatever its status) waits for the submit thread; a GOP of a run seeked away from is retired
    void hand_parsed(std::unique_ptr<Job> job)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (run_ == job->run) {
                const uint64_t g = job->gop;
                parsed_[g] = std::move(job);
            } else retire(std::move(job));
        }
        cv_.notify_all();
    }

    // ---- submit thread ------------------------------------------------------------------------------------------------------
    // A window of the current run to submit (once the run is all submitted the thread waits for a seek), a free entry of the ring,
    // then every GOP of the window parsed: the window with run, id, ring and jobs set; nullptr: stop.  A seek in between: the ring
    // entry goes back, and the window is taken from the new run.  *got_ring, *got_gops: when the two waits ended.
    std::unique_ptr<Window> take_window(Clock::time_point* got_ring, Clock::time_point* got_gops)
    {
        auto w = std::make_unique<Window>();
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] {
                if (stop_) return true;
                if (run_submitted_ >= run_->total_windows) return false;
                return free_ring_entry() >= 0;
            });
            if (stop_) return nullptr;
            *got_ring = Clock::now();
            w->run = run_;
            w->id = next_window_++;
            w->ring = free_ring_entry();
            ring_owner_[(size_t)w->ring] = w->id;
            const uint64_t g0 = (uint64_t)run_submitted_ * (uint64_t)W_, g1 = std::min<uint64_t>(g0 + (uint64_t)W_, w->run->total_gops);
            cv_.wait(lk, [&] {
                if (stop_ || run_ != w->run) return true;
                for (uint64_t g = g0; g < g1; g++)
                    if (!parsed_.count(g)) return false;
                return true;
            });
            if (stop_ || run_ != w->run) {
                ring_owner_[(size_t)w->ring] = -1;
                if (stop_) return nullptr;
                continue;
            }
            *got_gops = Clock::now();
            for (uint64_t g = g0; g < g1; g++) {
                w->jobs.push_back(std::move(parsed_[g]));
                parsed_.erase(g);
            }
            run_submitted_++;
            return w;
        }
    }
    // a submitted window (whatever its status, and whatever became of its run meanwhile) goes to the notify thread
    void submitted(std::unique_ptr<Window> w)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            to_notify_.push_back(std::move(w));
            windows_submitted_++;
        }
        cv_.notify_all();
    }
    void submit_exited()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            submit_exited_ = true;
        }
        cv_.notify_all();
    }

    // ---- notify thread ------------------------------------------------------------------------------------------------------
    // what the notify thread does next: a submitted window to wait for; else, once the submit thread has exited, leave; else the
    // 'ended' callback of a run whose windows are all delivered (in_callback is set: the thread stays for the next seek)
    struct Event {
        std::unique_ptr<Window> window;
        Run ended;
        bool quiet = false;      // tear-down has begun: no callbacks
        bool exit() const { return !window && !ended; }
    };
    Event next_event()
    {
        Event e;
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !to_notify_.empty() || submit_exited_ || (!stop_ && !run_ended_ && run_done_ == run_->total_windows); });
        if (!to_notify_.empty()) {
            e.window = std::move(to_notify_.front());
            to_notify_.pop_front();
        } else if (!submit_exited_) {
            run_ended_ = true;
            in_callback_ = true;
            e.ended = run_;
        }
        e.quiet = quiet_;
        return e;
    }
    void ended_returned(const Run& ended)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            in_callback_ = false;
            ended_run_ = ended;
        }
        cv_.notify_all();
    }
    // A window whose launches have finished.  One of a run seeked away from that came back without error is drained: retired (its
    // ring entry and arenas go back) and never delivered, `w` is empty then.  Any other is about to be delivered: once a window is
    // past this point a seek waits for its callback to return.
    bool keep_or_retire(std::unique_ptr<Window>& w)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (w->run == run_ || w->status != 0) {
                in_callback_ = true;
                return true;
            }
            retire(std::move(w));
        }
        cv_.notify_all();
        return false;
    }
    // the window is out for delivery until release(): the pointer stays good that long.  `seconds`: since the pipeline started.
    const Window* deliver(std::unique_ptr<Window> w, double seconds, bool* quiet)
    {
        std::lock_guard<std::mutex> lk(mu_);
        const Window* out = w.get();
        const int64_t id = w->id;
        delivered_[id] = std::move(w);
        seconds_ = seconds;
        if (window_done_.size() < 4096) window_done_.push_back(seconds);
        *quiet = quiet_;
        return out;
    }
    void callback_returned(const Run& of_window)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            windows_done_++;
            if (of_window == run_) run_done_++;
            in_callback_ = false;
        }
        cv_.notify_all();
    }
    void finish()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            finished_ = true;
        }
        cv_.notify_all();
    }

    // ---- callers ------------------------------------------------------------------------------------------------------------
    void feed(size_t valid)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (valid > valid_) valid_ = valid;
        }
        cv_.notify_all();
    }
    bool release(int64_t window)         // false: not out for delivery
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = delivered_.find(window);
            if (it == delivered_.end()) return false;
            retire(std::move(it->second));
            delivered_.erase(it);
        }
        cv_.notify_all();
        return true;
    }
    // a delivered window, looked at under the lock (the notify thread and release need it: look up and copy, nothing more);
    // false: not out for delivery, `look` is not called
    template <class Look> bool with_delivered(int64_t window, Look&& look) const
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = delivered_.find(window);
        if (it == delivered_.end()) return false;
        const Window& w = *it->second;
        look(w);
        return true;
    }
    int wait_run()                       // the current run's end (or the pipeline's); the status
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return finished_ || ended_run_ == run_; });
        return status_;
    }
    // false: the pipeline has failed, nothing changed.  What was parsed for the old position goes back; GOPs still on the parser
    // threads are dropped when they are done, windows submitted and not delivered are drained by the notify thread, held windows
    // stay held.  A callback under way returns first.
    bool seek(Run run, int64_t* first_window)
    {
        std::unique_lock<std::mutex> lk(mu_);
        if (status_ != 0) return false;
        run_ = std::move(run);
        next_gop_ = 0;
        run_submitted_ = run_done_ = 0;
        run_ended_ = false;
        *first_window = next_window_;
        for (auto& kv : parsed_) retire(std::move(kv.second));
        parsed_.clear();
        cv_.notify_all();
        cv_.wait(lk, [&] { return !in_callback_; });
        return true;
    }
    void fail(int code, const std::string& msg)      // the first status and text win
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (status_ == 0) {
            status_ = code;
            err_ = msg;
        }
        stop_ = true;
        cv_.notify_all();
    }
    void stop_quiet()                    // tear-down begins: no callbacks from here on
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
            quiet_ = true;
        }
        cv_.notify_all();
    }
    // after the threads have been joined (and the device is idle): every window and job still here is retired
    void tear_down()
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto& w : to_notify_) retire(std::move(w));
        to_notify_.clear();
        for (auto& kv : delivered_) retire(std::move(kv.second));
        delivered_.clear();
        for (auto& kv : parsed_) retire(std::move(kv.second));
        parsed_.clear();
    }

    int status() const
    {
        std::lock_guard<std::mutex> lk(mu_);
        return status_;
    }
    bool quiet() const
    {
        std::lock_guard<std::mutex> lk(mu_);
        return quiet_;
    }
    const char* error() const            // stays valid: the text is set once
    {
        std::lock_guard<std::mutex> lk(mu_);
        return err_.c_str();
    }
    Run run() const
    {
        std::lock_guard<std::mutex> lk(mu_);
        return run_;
    }
    struct Counts {
        int64_t windows_submitted, windows_done;     // over all runs
        double seconds;                               // when the last window was delivered
        size_t free_arenas, ring_held, parsed, to_notify, delivered;
    };
    Counts counts() const
    {
        std::lock_guard<std::mutex> lk(mu_);
        size_t held = 0;
        for (int64_t o : ring_owner_) held += o >= 0;
        return Counts{windows_submitted_, windows_done_, seconds_, free_arenas_.size(), held, parsed_.size(), to_notify_.size(), delivered_.size()};
    }
    std::vector<double> window_done() const          // when each of the first 4096 windows was delivered
    {
        std::lock_guard<std::mutex> lk(mu_);
        return window_done_;
    }

private:
    // (mu_ held) the arena goes back to the free list, the job is destroyed
    void retire(std::unique_ptr<Job> job)
    {
        if (!job) return;
        free_arenas_.push_back(job->arena);
    }
    // (mu_ held) its jobs are retired, its ring entry is freed
    void retire(std::unique_ptr<Window> w)
    {
        if (!w) return;
        for (auto& j : w->jobs) retire(std::move(j));
        ring_owner_[(size_t)w->ring] = -1;
    }
    int free_ring_entry() const
    {
        for (size_t r = 0; r < ring_owner_.size(); r++)
            if (ring_owner_[r] < 0) return (int)r;
        return -1;
    }

    mutable std::mutex mu_;
    std::condition_variable cv_;
    int W_ = 1;                                       // GOPs per window
    size_t valid_ = 0;                                // how much of the stream has arrived (feed)
    // the current run and how far it is; a seek replaces the run and starts these over
    Run run_, ended_run_;                             // ended_run_: the last run whose 'ended' callback has returned
    uint64_t next_gop_ = 0;                           // next GOP of the run for a parser thread
    int64_t run_submitted_ = 0, run_done_ = 0;        // windows of the run submitted / delivered
    bool run_ended_ = false;                          // its 'ended' callback is out
    int64_t next_window_ = 0;                         // window ids count on across runs
    bool in_callback_ = false;                        // the notify thread is inside the callback
    std::map<uint64_t, std::unique_ptr<Job>> parsed_; // waiting for the submit thread (GOP of the current run -> job)
    std::deque<Ticket> free_arenas_;
    std::deque<std::unique_ptr<Window>> to_notify_;
    std::vector<int64_t> ring_owner_;                 // window id holding a ring entry, -1 free
    std::map<int64_t, std::unique_ptr<Window>> delivered_;       // waiting for release
    int64_t windows_submitted_ = 0, windows_done_ = 0;
    bool stop_ = false, finished_ = false, quiet_ = false, submit_exited_ = false;
    int status_ = 0;
    std::string err_;
    double seconds_ = 0;
    std::vector<double> window_done_;
};

}  // namespace leon_flow
