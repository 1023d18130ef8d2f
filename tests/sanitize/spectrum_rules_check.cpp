// spectrum_rules_check.cpp -- csrc/spectrum_rules.hpp on stand-in events: the
// sticky ready flag of a cached spectrum row and the rule by which a retired
// row serves again.  An event is an index into a table of "completed" flags;
// every query is counted.  Prints `name value` lines;
// tests/test_spectrum_row_rules.py builds it with g++ alone (plain, and with
// -fsanitize=address,undefined), runs it and asserts the values.
#include <cstdio>
#include <map>
#include <memory>
#include <vector>

#include "spectrum_rules.hpp"

using namespace dspb;

namespace {
struct Row {
    int ready = 0;
    bool ready_seen = false;
    std::map<void *, int> used;
};
std::vector<bool> g_done;
int g_queries = 0;
bool done(int ev) {
    ++g_queries;
    return g_done[(size_t)ev];
}
}  // namespace

int main() {
    g_done.assign(4, false);
    Row r;  // ready = event 0
    // hits before the ready event completed: each waits, each queries
    int waits = 0;
    for (int i = 0; i < 3; ++i) waits += spectrum_row_must_wait(r, done);
    std::printf("pending_waits %d\npending_queries %d\npending_seen %d\n", waits, g_queries, (int)r.ready_seen);
    // the event completes: the next hit sees it, and no later hit queries or waits
    g_done[0] = true;
    g_queries = waits = 0;
    for (int i = 0; i < 5; ++i) waits += spectrum_row_must_wait(r, done);
    std::printf("done_waits %d\ndone_queries %d\ndone_seen %d\n", waits, g_queries, (int)r.ready_seen);
    // sticky: even if the event were recorded again (it is not while the key stands)
    g_done[0] = false;
    std::printf("sticky_wait %d\n", (int)spectrum_row_must_wait(r, done));
    // the row filled again for another key: the flag is cleared by the miss
    r.ready_seen = false;
    std::printf("refilled_wait %d\n", (int)spectrum_row_must_wait(r, done));

    // recycling: a retired row held by the list alone, two streams' events 1 and 2
    auto e = std::make_shared<Row>();
    int s1, s2;
    e->used[&s1] = 1;
    e->used[&s2] = 2;
    g_done = {true, true, true, true};
    std::printf("idle_all_done %d\n", (int)spectrum_row_idle(*e, e.use_count(), done));
    {
        std::shared_ptr<Row> hold = e;  // a call that is still enqueueing
        std::printf("idle_held %d\n", (int)spectrum_row_idle(*e, e.use_count(), done));
    }
    g_done[0] = false;
    std::printf("idle_ready_pending %d\n", (int)spectrum_row_idle(*e, e.use_count(), done));
    g_done[0] = true;
    g_done[2] = false;  // one stream's last launch still runs
    std::printf("idle_reader_pending %d\n", (int)spectrum_row_idle(*e, e.use_count(), done));
    g_done[2] = true;
    // the sticky flag does not stand in for the query: a row retired with the
    // flag set still asks every event
    e->ready_seen = true;
    g_done[0] = false;
    std::printf("idle_seen_but_pending %d\n", (int)spectrum_row_idle(*e, e.use_count(), done));
    g_done[0] = true;
    e->used.clear();
    std::printf("idle_no_readers %d\n", (int)spectrum_row_idle(*e, e.use_count(), done));
    return 0;
}
