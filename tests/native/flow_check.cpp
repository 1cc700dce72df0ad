// flow_check.cpp -- the thread protocol of csrc/leon_pipe_flow.h with fake jobs and windows.  A stand-alone program
// (tests/test_pipe_flow.py builds it under ThreadSanitizer and under the address and undefined-behaviour sanitizers and runs each
// with a time limit): the three thread roles of leon_pipeline run on real threads, "parse", "submit" and "event wait" are a seeded
// mix of nothing, yield and short sleeps.  Every scenario prints its name, thread count, loops and seed before it starts, so that a
// deadlock leaves the scenario as the last line printed.
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_pipe_flow.h"

#include <atomic>
#include <cstdio>
#include <functional>
#include <random>
#include <thread>

using leon_flow::PipeRun;

namespace {

constexpr int kW = 2, kR = 2, kArenas = 6, kGops = 7;       // the smallest shapes at which every path exists; the last window is short
constexpr int kFailed = -7;

std::atomic<int> g_failed_checks{0};
#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) { g_failed_checks++; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

std::atomic<int> g_live_jobs{0}, g_live_windows{0};
std::atomic<int> g_arena_users[kArenas];

struct FakeJob {
    std::shared_ptr<const PipeRun> run;
    uint64_t gop = 0;
    int arena = -1;
    int status = 0;
    bool counted = false;        // the parser thread has entered it in g_arena_users
    FakeJob() { g_live_jobs++; }
    ~FakeJob()
    {
        g_live_jobs--;
        if (counted) g_arena_users[arena]--;
    }
};
struct FakeWindow {
    std::shared_ptr<const PipeRun> run;
    int64_t id = 0;
    int ring = 0;
    std::vector<std::unique_ptr<FakeJob>> jobs;
    int status = 0;
    FakeWindow() { g_live_windows++; }
    ~FakeWindow() { g_live_windows--; }
};
using Flow = leon_flow::Flow<FakeJob, FakeWindow>;
using Run = Flow::Run;

Run make_run(uint32_t first_key, int loops)
{
    static std::atomic<uint64_t> next_id{1};
    auto run = std::make_shared<PipeRun>();
    run->id = next_id++;
    run->first_key = first_key;
    for (uint32_t k = first_key; k < (uint32_t)kGops; k++) run->mine.push_back(k);
    run->total_gops = (uint64_t)run->mine.size() * (uint64_t)loops;
    run->total_windows = (int64_t)((run->total_gops + kW - 1) / kW);
    return run;
}
constexpr uint64_t kGopBytes = 100;          // key-map entry k is the bytes [100 k, 100 k + 100)

using Rng = std::mt19937_64;
void jitter(Rng& rng)
{
    const unsigned r = (unsigned)(rng() & 7);
    if (r < 3) return;
    if (r < 5) { std::this_thread::yield(); return; }
    std::this_thread::sleep_for(std::chrono::microseconds(10 + rng() % 40));
}

// waits for a state the threads reach by themselves (20 s at the most: the caller CHECKs the result)
bool until(const std::function<bool()>& reached)
{
    const auto give_up = std::chrono::steady_clock::now() + std::chrono::seconds(20);
    while (!reached()) {
        if (std::chrono::steady_clock::now() > give_up) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    return true;
}

// leon_pipeline's threads around a Flow: what leon_pipeline_impl.h does between the calls is jitter here
struct Pipe {
    Flow flow;
    uint64_t seed = 0;
    std::vector<std::thread> parsers;
    std::thread submitter, notifier;
    std::atomic<int64_t> fail_gop{-1};       // the parser gives this GOP a status
    std::atomic<int> hold_first{0};          // the callback keeps this many windows; the others it releases at once

    std::mutex mu;               // what the callbacks record, and what the seeking thread tells them to expect
    std::map<std::pair<uint64_t, uint64_t>, int> parsed_times;       // (run, GOP) -> how often handed over
    std::map<uint64_t, uint64_t> next_gop_of;                        // run -> the GOP its next delivered window starts with
    std::map<uint64_t, int> ended_of;                                // run -> 'ended' callbacks
    std::vector<std::pair<int64_t, int>> delivered;                  // (window, status), in order
    std::vector<int64_t> held;
    int64_t last_id = -1;
    int finals = 0, final_status = 0;
    bool seeking = false;
    int64_t floor_id = 0;
    uint64_t cur_run = 0, pending_run = 0;

    void start(int K, uint64_t seed_, Run run, size_t valid)
    {
        seed = seed_;
        cur_run = run->id;
        flow.begin(std::move(run), valid);
        std::vector<int> arenas;
        for (int i = 0; i < kArenas; i++) arenas.push_back(i);
        flow.equip(kW, kR, arenas);
        for (int i = 0; i < K; i++) parsers.emplace_back([this, i] { parser_main(i); });
        submitter = std::thread([this] { submit_main(); });
        notifier = std::thread([this] { notify_main(); });
    }
    void parser_main(int i)
    {
        Rng rng(seed * 1000 + 10 + (uint64_t)i);
        for (;;) {
            std::unique_ptr<FakeJob> job = flow.take_gop();
            if (!job) return;
            CHECK(job->arena >= 0 && job->arena < kArenas && g_arena_users[job->arena]++ == 0);      // one live job per ticket
            job->counted = true;
            const std::shared_ptr<const PipeRun> run = job->run;
            const uint64_t g = job->gop;
            CHECK(g < run->total_gops);
            const uint32_t key = run->mine[g % run->mine.size()];
            const Flow::Bytes bytes = flow.await_bytes(job, (key + 1) * kGopBytes);
            if (bytes == Flow::Bytes::Stop) { CHECK(!job); return; }
            if (bytes == Flow::Bytes::Replaced) { CHECK(!job); continue; }
            jitter(rng);
            if ((int64_t)g == fail_gop) job->status = kFailed;
            {
                std::lock_guard<std::mutex> lk(mu);
                parsed_times[{run->id, g}]++;
            }
            flow.hand_parsed(std::move(job));
        }
    }
    void submit_main()
    {
        Rng rng(seed * 1000 + 1);
        for (;;) {
            auto t_ring = Flow::Clock::now(), t_gops = t_ring;
            std::unique_ptr<FakeWindow> w = flow.take_window(&t_ring, &t_gops);
            if (!w) break;
            int rc = 0;
            for (const auto& j : w->jobs)
                if (j->status != 0 && rc == 0) rc = j->status;
            jitter(rng);
            w->status = rc;
            if (rc != 0) flow.fail(rc, "first failure");
            flow.submitted(std::move(w));
            if (rc != 0) break;
        }
        flow.submit_exited();
    }
    void notify_main()
    {
        Rng rng(seed * 1000 + 2);
        for (;;) {
            Flow::Event ev = flow.next_event();
            if (ev.exit()) break;
            if (ev.ended) {
                if (!ev.quiet) {
                    std::lock_guard<std::mutex> lk(mu);
                    ended_of[ev.ended->id]++;
                }
                flow.ended_returned(ev.ended);
                continue;
            }
            jitter(rng);
            if (!flow.keep_or_retire(ev.window)) { CHECK(!ev.window); continue; }
            const int64_t id = ev.window->id;
            const int st = ev.window->status;
            const Run run = ev.window->run;
            bool quiet = false;
            const FakeWindow* out = flow.deliver(std::move(ev.window), 0.0, &quiet);
            if (!quiet) on_window(rng, id, st == 0 ? out : nullptr, st, run->id);
            else CHECK(flow.release(id));
            flow.callback_returned(run);
        }
        if (!flow.quiet()) {
            std::lock_guard<std::mutex> lk(mu);
            finals++;
            final_status = flow.status();
        }
        flow.finish();
    }
    // the callback: `frames` stands for the frames of a window delivered without error
    void on_window(Rng& rng, int64_t id, const FakeWindow* frames, int st, uint64_t run)
    {
        bool keep;
        {
            std::lock_guard<std::mutex> lk(mu);
            CHECK(id > last_id);         // strictly increasing: no id twice
            last_id = id;
            delivered.emplace_back(id, st);
            CHECK(id >= floor_id);       // nothing of before the last seek that returned
            CHECK(run == cur_run || (seeking && run == pending_run));
            if (frames) {
                uint64_t& next = next_gop_of[run];
                CHECK(!frames->jobs.empty() && frames->jobs[0]->gop == next && next % kW == 0);
                for (const auto& j : frames->jobs) {
                    CHECK(j->gop == next && j->run->id == run);
                    next++;
                }
                CHECK(next % kW == 0 || next == frames->run->total_gops);
            }
            keep = (int)held.size() < hold_first;
            if (keep) held.push_back(id);
        }
        if (!keep) {
            jitter(rng);
            CHECK(flow.release(id));
        }
    }
    // leon_pipeline_seek from a caller's thread
    void seek(uint32_t first_key)
    {
        const Run run = make_run(first_key, 1);
        {
            std::lock_guard<std::mutex> lk(mu);
            seeking = true;
            pending_run = run->id;
        }
        int64_t first = -1;
        CHECK(flow.seek(run, &first));
        std::lock_guard<std::mutex> lk(mu);
        CHECK(first >= floor_id);
        floor_id = first;
        cur_run = run->id;
        seeking = false;
    }
    // every GOP of the run parsed once, delivered once and in order, one 'ended'
    void check_run_complete(const Run& run)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (uint64_t g = 0; g < run->total_gops; g++) CHECK((parsed_times[{run->id, g}]) == 1);
        CHECK(next_gop_of[run->id] == run->total_gops);
        CHECK(ended_of[run->id] == 1);
    }
    // nothing in flight: arenas are free or with a live job, ring entries with the windows out for delivery; the submit thread
    // holds the one blank window it waits with
    void check_quiescent()
    {
        CHECK(until([&] {        // (the submit thread may still be on its way back into take_window)
            const Flow::Counts c = flow.counts();
            return c.to_notify == 0 && (int)c.free_arenas + g_live_jobs == kArenas && c.ring_held == c.delivered && g_live_windows == (int)c.delivered + 1;
        }));
    }
    // leon_pipeline_destroy
    void destroy()
    {
        flow.stop_quiet();
        for (auto& t : parsers) t.join();
        submitter.join();
        notifier.join();
        flow.tear_down();
        const Flow::Counts c = flow.counts();
        CHECK(c.free_arenas == (size_t)kArenas && c.ring_held == 0 && c.parsed == 0 && c.to_notify == 0 && c.delivered == 0);
        CHECK(g_live_jobs == 0 && g_live_windows == 0);
        for (auto& users : g_arena_users) CHECK(users == 0);
        for (const auto& kv : parsed_times) CHECK(kv.second == 1);
        for (const auto& kv : ended_of) CHECK(kv.second == 1);
    }
};

// ---- the scenarios: (parser threads, loops, seed) ---------------------------------------------------------------------------------

void plain_run(int K, int loops, uint64_t seed)
{
    Pipe p;
    const Run run = make_run(0, loops);
    p.start(K, seed, run, kGops * kGopBytes);
    CHECK(p.flow.wait_run() == 0);
    p.check_run_complete(run);           // 'ended' came before wait returned
    p.check_quiescent();
    {
        std::lock_guard<std::mutex> lk(p.mu);
        CHECK((int64_t)p.delivered.size() == run->total_windows);
        for (size_t i = 0; i < p.delivered.size(); i++) CHECK(p.delivered[i].first == (int64_t)i && p.delivered[i].second == 0);
    }
    p.destroy();
    CHECK(p.finals == 0 && p.ended_of.size() == 1);      // tear-down is quiet: no final callback
}

// the callback keeps R windows: everything stalls (parsers on arenas, the submit thread on the ring) until another thread releases
void held_windows(int K, int loops, uint64_t seed)
{
    for (const bool destroy_held : {false, true}) {
        Pipe p;
        p.hold_first = kR;
        const Run run = make_run(0, loops);
        p.start(K, seed, run, kGops * kGopBytes);
        // R windows out with W jobs each; the two arenas left are parsed into and nobody can go on
        CHECK(until([&] { const Flow::Counts c = p.flow.counts(); return c.delivered == (size_t)kR && c.free_arenas == 0 && c.parsed == 2; }));
        Flow::Counts c = p.flow.counts();
        CHECK(c.windows_submitted == kR && c.ring_held == (size_t)kR && c.to_notify == 0 && g_live_jobs == kArenas);
        if (!destroy_held) {
            // (a window is released once its callback has returned, or from inside it: the callbacks have the ids by then)
            CHECK(until([&] { std::lock_guard<std::mutex> lk(p.mu); return p.held.size() == (size_t)kR; }));
            for (int64_t id = 0; id < kR; id++) CHECK(p.flow.release(id));
            CHECK(!p.flow.release(0));
            CHECK(p.flow.wait_run() == 0);
            p.check_run_complete(run);
            p.check_quiescent();
        }
        p.destroy();
    }
}

// a stream that arrives in steps that end inside a GOP; then a seek while parsers wait for bytes
void stream_arriving(int K, int loops, uint64_t seed)
{
    Rng rng(seed);
    {
        Pipe p;
        const Run run = make_run(0, loops);
        p.start(K, seed, run, 0);
        for (size_t valid = 130; valid < kGops * kGopBytes + 130; valid += 130) {
            jitter(rng);
            p.flow.feed(std::min<size_t>(valid, kGops * kGopBytes));
        }
        p.flow.feed(10);                 // (never backwards)
        CHECK(p.flow.wait_run() == 0);
        p.check_run_complete(run);
        p.check_quiescent();
        p.destroy();
    }
    {
        Pipe p;
        p.start(K, seed, make_run(0, loops), kGopBytes + 50);
        // GOP 0 is parsed, every parser thread waits with a job for bytes that have not come, the submit thread for GOP 1
        const auto waiting = [&] {
            const Flow::Counts c = p.flow.counts();
            return c.parsed == 1 && (int)c.free_arenas == kArenas - 1 - K && g_live_jobs == 1 + K && c.ring_held == 1 && c.windows_submitted == 0;
        };
        CHECK(until(waiting));
        p.seek(0);                       // their jobs are dropped, the arenas come back: the same state for the new run
        CHECK(until(waiting));
        p.flow.feed(kGops * kGopBytes);
        const Run run = p.flow.run();
        CHECK(p.flow.wait_run() == 0);
        p.check_run_complete(run);
        p.check_quiescent();
        p.destroy();
    }
}

void seeks(int K, int, uint64_t seed)
{
    Rng rng(seed);
    Pipe p;
    p.start(K, seed, make_run(0, 1), kGops * kGopBytes);
    for (int i = 0; i < 30; i++) {
        switch (rng() % 5) {
        case 0: break;
        case 1: CHECK(p.flow.wait_run() == 0); break;                // from the end of a run
        default: std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));
        }
        p.seek((uint32_t)(rng() % kGops));
    }
    const Run run = p.flow.run();
    CHECK(p.flow.wait_run() == 0);
    p.check_run_complete(run);
    p.check_quiescent();
    p.destroy();
}

void failure(int K, int loops, uint64_t seed)
{
    Pipe p;
    p.fail_gop = 3;                      // in window 1
    p.start(K, seed, make_run(0, loops), kGops * kGopBytes);
    CHECK(p.flow.wait_run() == kFailed);
    {
        std::lock_guard<std::mutex> lk(p.mu);
        CHECK(p.delivered.size() == 2 && p.delivered[0] == std::make_pair((int64_t)0, 0) && p.delivered[1] == std::make_pair((int64_t)1, kFailed));
        CHECK(p.finals == 1 && p.final_status == kFailed && p.ended_of.empty());      // the final callback came before wait returned
    }
    const char* text = p.flow.error();
    p.flow.fail(-9, "a later failure");
    CHECK(p.flow.status() == kFailed && p.flow.error() == text && std::string(text) == "first failure");
    int64_t first = 0;
    CHECK(!p.flow.seek(make_run(0, 1), &first));
    CHECK(p.flow.counts().windows_submitted == 2);       // the submit thread has exited
    p.destroy();
    CHECK(p.finals == 1);
}

// tear-down at every waiting point: all threads join
void stop_while_waiting(int K, int loops, uint64_t seed)
{
    {   // parsers wait for an arena, the submit thread for a ring entry
        Pipe p;
        p.hold_first = kR;
        p.start(K, seed, make_run(0, loops), kGops * kGopBytes);
        CHECK(until([&] { const Flow::Counts c = p.flow.counts(); return c.delivered == (size_t)kR && c.free_arenas == 0 && c.parsed == 2; }));
        p.destroy();
    }
    {   // parsers wait for bytes, the submit thread for the window's GOPs
        Pipe p;
        p.start(K, seed, make_run(0, loops), 0);
        CHECK(until([&] { const Flow::Counts c = p.flow.counts(); return (int)c.free_arenas == kArenas - K && c.ring_held == 1; }));
        p.destroy();
    }
    {   // everything delivered: all three roles wait for a seek
        Pipe p;
        p.start(K, seed, make_run(0, loops), kGops * kGopBytes);
        CHECK(p.flow.wait_run() == 0);
        p.destroy();
    }
    {   // a seek has just returned
        Rng rng(seed);
        Pipe p;
        p.start(K, seed, make_run(0, 1), kGops * kGopBytes);
        std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));
        p.seek((uint32_t)(rng() % kGops));
        p.destroy();
    }
    {   // nothing ever started (a create that failed before its threads)
        Flow flow;
        flow.stop_quiet();
        flow.tear_down();
    }
}

}  // namespace

int main()
{
    struct Scenario { const char* name; void (*run)(int, int, uint64_t); int seeds; bool loops; };
    const Scenario all[] = {
        {"plain run", plain_run, 24, true},
        {"held windows", held_windows, 12, true},
        {"stream still arriving", stream_arriving, 12, true},
        {"seeks", seeks, 10, false},
        {"failure", failure, 12, true},
        {"stop at every waiting point", stop_while_waiting, 12, true},
    };
    int scenarios = 0, failed = 0;
    for (const Scenario& s : all)
        for (const int K : {1, 3})
            for (const int loops : {1, 2}) {
                if (loops == 2 && !s.loops) continue;
                for (int seed = 1; seed <= s.seeds; seed++) {
                    std::printf("%s, K = %d, loops = %d, seed %d\n", s.name, K, loops, seed);
                    std::fflush(stdout);
                    const int before = g_failed_checks;
                    s.run(K, loops, (uint64_t)seed);
                    scenarios++;
                    failed += g_failed_checks != before;
                }
            }
    const int live = g_live_jobs + g_live_windows;
    std::printf("%d scenarios, %d failed, %d live at exit\n", scenarios, failed, live);
    return failed || live ? 1 : 0;
}
