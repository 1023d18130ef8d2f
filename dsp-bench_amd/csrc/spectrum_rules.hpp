// spectrum_rules.hpp -- the two rules of a cached spectrum row's events
// (capi_impl.hpp SpectrumRow, capi.cpp spectrum_row / spectrum_recycle), on any
// row type with `ready`, `ready_seen` and `used` and a query done(event) --
// hipEventQuery == hipSuccess in the library.  No HIP here:
// tests/test_spectrum_row_rules.py runs them on stand-in events with g++ alone.
#pragma once

namespace dspb {

// A hit has to make its stream wait for the row's ready event until the event
// has once been seen completed; from then on no hit waits or queries (the flag
// is sticky until the row is filled again, which clears it).  A completed event
// orders the row before every later launch on any stream.
template <class Row, class Done>
bool spectrum_row_must_wait(Row &e, Done done) {
    if (!e.ready_seen && done(e.ready)) e.ready_seen = true;
    return !e.ready_seen;
}

// A retired row serves again only when nobody but the retired list holds it
// (`holders` == 1) and its ready event and every stream's last use have
// completed.
template <class Row, class Done>
bool spectrum_row_idle(const Row &e, long holders, Done done) {
    if (holders != 1 || !done(e.ready)) return false;
    for (auto &kv : e.used)
        if (!done(kv.second)) return false;
    return true;
}

}  // namespace dspb
