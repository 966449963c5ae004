// The calling thread's state, the stream / event choreography of one call (ordering points, the stop events riding on the kernel dispatches)
// and the built-in profiler with its launch ledger.
#include "host.hpp"

namespace vsl {

thread_local std::string g_err;
thread_local vsl_handle_s* g_cur = nullptr;

int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

CallScope::CallScope(vsl_handle_s* h) {
    h->sync_used = 0; h->stop_used = 0; h->ev_n = 0;
    for (bool& d : h->ev_dirty) d = false;
    h->stop_events = h->multi_stream;
    g_cur = h;
}
CallScope::~CallScope() { g_cur = nullptr; }

// does the built-in profiler's selection ("*", one launch name, or a comma-separated list of names) name this launch?
bool prof_selected(const vsl_handle_s* h, const char* name) {
    if (!h->prof_on) return false;
    const std::string& sel = h->prof_sel;
    const size_t n = strlen(name);
    for (size_t p = 0; p <= sel.size();) {
        size_t q = sel.find(',', p);
        if (q == std::string::npos) q = sel.size();
        if ((q - p == 1 && sel[p] == '*') || (q - p == n && sel.compare(p, n, name) == 0)) return true;
        p = q + 1;
    }
    return false;
}

ProfScope::ProfScope(vsl_handle_s* h_, const char* name) : h(h_) {
    if (prof_selected(h, name)) { h->stop_events = false; h->prof_name = name; g_cur = h; }
}
ProfScope::~ProfScope() { if (g_cur == h && h->prof_name) { h->prof_name = nullptr; g_cur = nullptr; } }

// built-in profiler: a selected LAUNCH hands its name to vsl_launch_events, which puts timing events on the kernel's own packet
void Ctx::pb(const char* name) { h->prof_name = prof_selected(h, name) ? name : nullptr; }

// One ordering point: every stream of `to` (those that are not `from` itself, each once) waits for everything enqueued so far on `from`.
// ONE event for all of them (each record / wait pair leaves a bubble in the producer stream: see wgrad_async, backward.hip).
void Ctx::order_n(hipStream_t from, const hipStream_t* to, int n) {
    if (dry) return;
    hipStream_t w[2];
    int nw = 0;
    for (int i = 0; i < n && nw < 2; ++i)
        if (to[i] != from && !(nw && w[0] == to[i])) w[nw++] = to[i];
    if (!nw) return;
    for (int i = 0; i < nw; ++i) h->prof_wait(from, w[i]);
    // rides on from's last kernel -- unless `from` itself was made to wait for something after that kernel (then a marker is recorded)
    hipEvent_t e = h->last_event(from);
    if (!e) {
        if (h->sync_used == h->sync_pool.size()) { hipEvent_t t; (void)hipEventCreateWithFlags(&t, hipEventDisableTiming); h->sync_pool.push_back(t); }
        e = h->sync_pool[h->sync_used++];
        (void)hipEventRecord(e, from);
    }
    for (int i = 0; i < nw; ++i) { (void)hipStreamWaitEvent(w[i], e, 0); h->mark_waiting(w[i]); }
}

// after a fork the chain that finishes LAST should own the main stream: its join wait is then already satisfied (a wait on
// an event that has just been signalled costs 10 - 22 us).  At the headline shape the query side is the long one.
bool query_chain_is_longer(const Plan& p) {
    // (the forward's two branches are about even: forward_full.)  Backward: since the split-bf16 kernels of round 3 the QUERY side ends last (cq_bwd_d .. embed_bwd: 147 us of isolated kernels against
    // 133 for the video side), so it owns the main stream and the final join finds the video stream's event long signalled: 0.934-0.938 ->
    // 0.930 ms with optimizer (profiles/r03_notes.md).
    return p.T <= 128;          // longer videos: the video side's attention backward grows with T^2 and ends last again
}
// (Round 6 measured, same box, and dropped -- profiles/r06_notes.md: one wait instead of two on the joining stream by folding the third stream into
// the second, +0.5 %; the video chain on the main stream in the backward, +1 - 5 %; k_query_fwd held back behind the video pass' conv block, +2.5 %;
// k_query_bwd held back behind the video pass' attention backward, +0.3 %; the video pass' pointwise weight gradients on the weight-gradient stream, +3.5 %.)

void vsl_launch_events(hipStream_t s, hipEvent_t* start, hipEvent_t* stop) {
    vsl_handle_s* h = g_cur;
    if (!h || !(h->stop_events || h->prof_name)) return;
    hipEvent_t e;
    if (h->prof_name) {                      // profiled launch: timing events, start + stop, one record per kernel
        while (h->prof_pool.size() < h->prof_used + 2) { hipEvent_t t; (void)hipEventCreate(&t); h->prof_pool.push_back(t); }
        {
            vsl_handle_s::ProfRec rec{h->prof_name, h->prof_used, h->prof_used + 1, s,
                                      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h->prof_t0).count(), {0, 0, 0, 0, 0, 0}, 0};
            const int me = (int)h->prof_recs.size();
            bool seen = false;
            for (auto& kv : h->prof_last) if (kv.first == s) { if (rec.nd < 6) rec.deps[rec.nd++] = kv.second; kv.second = me; seen = true; }
            if (!seen) h->prof_last.push_back({s, me});
            for (size_t i = 0; i < h->prof_pending.size();) {
                if (h->prof_pending[i].first == s) { if (rec.nd < 6) rec.deps[rec.nd++] = h->prof_pending[i].second; h->prof_pending.erase(h->prof_pending.begin() + i); }
                else ++i;
            }
            h->prof_recs.push_back(rec);
        }
        *start = h->prof_pool[h->prof_used];
        e = h->prof_pool[h->prof_used + 1];
        h->prof_used += 2;
    } else {
        if (h->stop_used == h->stop_pool.size()) { hipEvent_t t; (void)hipEventCreateWithFlags(&t, hipEventDisableTiming); h->stop_pool.push_back(t); }
        e = h->stop_pool[h->stop_used++];
    }
    *stop = e;
    if (h->stop_events) {                    // remember the stream's last kernel for Ctx::order
        int i = 0;
        while (i < h->ev_n && h->ev_stream[i] != s) ++i;
        if (i == h->ev_n) { if (h->ev_n == 4) return; h->ev_stream[h->ev_n++] = s; }
        h->ev_last[i] = e;
        h->ev_dirty[i] = false;              // the new kernel runs behind every wait enqueued before it
    }
}

}  // namespace vsl

using namespace vsl;

extern "C" {

int vsl_profile_select(vsl_handle h, const char* kernel) {
    if (!h) return fail("null handle");
    h->prof_on = kernel != nullptr && kernel[0] != 0;
    h->prof_sel = kernel ? kernel : "";
    h->prof_recs.clear();
    h->prof_used = 0;
    h->prof_last.clear(); h->prof_pending.clear();
    h->prof_t0 = std::chrono::steady_clock::now();
    return 0;
}

// one record of the ledger: the index-th profiled launch since vsl_profile_select, in enqueue order
int vsl_profile_launch(vsl_handle h, int index, char* name, int name_cap, int32_t* stream, double* start_us, double* stop_us, double* host_us,
                       int32_t* deps /* [6] */, int32_t* ndeps) {
    if (!h) return fail("null handle");
    if (index < 0 || index >= (int)h->prof_recs.size()) return 2;
    const auto& r = h->prof_recs[index];
    float t0 = 0.f, t1 = 0.f;
    const hipEvent_t ref = h->prof_pool[h->prof_recs[0].e0];
    if (hipEventSynchronize(h->prof_pool[r.e1]) != hipSuccess || hipEventElapsedTime(&t0, ref, h->prof_pool[r.e0]) != hipSuccess ||
        hipEventElapsedTime(&t1, ref, h->prof_pool[r.e1]) != hipSuccess)
        return fail("hipEventElapsedTime failed");
    if (name && name_cap > 0) { strncpy(name, r.name, name_cap - 1); name[name_cap - 1] = 0; }
    int si = 0;
    {   // stream index in order of first appearance
        std::vector<hipStream_t> seen;
        for (const auto& q : h->prof_recs) { if (std::find(seen.begin(), seen.end(), q.s) == seen.end()) seen.push_back(q.s); if (&q == &r) break; }
        si = (int)(std::find(seen.begin(), seen.end(), r.s) - seen.begin());
    }
    if (stream) *stream = si;
    if (start_us) *start_us = 1e3 * t0;
    if (stop_us) *stop_us = 1e3 * t1;
    if (host_us) *host_us = r.host_us;
    if (deps) for (int i = 0; i < 6; ++i) deps[i] = i < r.nd ? r.deps[i] : -1;
    if (ndeps) *ndeps = r.nd;
    return 0;
}

int vsl_profile_read(vsl_handle h, int index, char* name, int name_cap, double* total_ms, int32_t* count) {
    if (!h) return fail("null handle");
    // aggregate by kernel name (synchronises on the recorded events)
    std::vector<std::pair<std::string, std::pair<double, int>>> agg;
    for (auto& r : h->prof_recs) {
        float ms = 0.f;
        if (hipEventSynchronize(h->prof_pool[r.e1]) != hipSuccess || hipEventElapsedTime(&ms, h->prof_pool[r.e0], h->prof_pool[r.e1]) != hipSuccess)
            return fail("hipEventElapsedTime failed");
        bool found = false;
        for (auto& a : agg) if (a.first == r.name) { a.second.first += ms; a.second.second++; found = true; break; }
        if (!found) agg.push_back({r.name, {ms, 1}});
    }
    if (index < 0 || index >= (int)agg.size()) return 2;       // end of list
    if (name && name_cap > 0) { strncpy(name, agg[index].first.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (total_ms) *total_ms = agg[index].second.first;
    if (count) *count = agg[index].second.second;
    return 0;
}

}  // extern "C"
