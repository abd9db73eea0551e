// vr_tuner.h -- the measured kernel choice (flavour 0): its trials and the rules that turn launch records into a kernel.
// Plain C++ with no HIP header and nothing of the context: vr_ctx.h includes it for the context's Tuner, vr_api_render.h calls tune_pick
// with the pinned kernel-time ring behind `Records`, and tests/tuner_driver compiles it for the CPU to pin the rules on invented records.
#pragma once

constexpr int kRing = 256;  // vr_kernel_times: launches remembered (launch number L records itself in slot L % kRing)

// Every kernel form is bit-identical, so the context tries the eligible ones on the caller's own frames and keeps the fastest by the
// launches' own records -- per "what is launched of what" (tune_pick).
struct Trial {
    unsigned long long key = 0;   // shader, share, viewport, frames per launch, frames in flight, scene epoch, arithmetic, layout (0 = free)
    unsigned long long shape = 0; // ... the same without the scene's epochs: a new scene starts from what the last one of this shape kept
    int n = 0, cand[6] = {};      // the eligible flavours; cand[0] = the prior's pick (what runs while nothing is known)
    int cur = 0, issued = 0;      // candidate on trial, launches it has had
    int per = 3, settle = 4;      // launches per candidate; launches before the trial starts (no launch order exists yet)
    long long launch[6][16] = {}; // launch number of every trial launch of every candidate (other shapes' launches may lie in between)
    int choice = -1;              // index into cand of the kernel kept (-1 = trial running)
    unsigned chain_ref = 0;       // longest ray chain + 1 when it was chosen: the trial re-opens when that has moved by a quarter
    float cost[6] = {};           // ms per launch measured (0 = no data)
    unsigned long long used = 0;  // (least recently used slot is recycled)
    // a new trial of key_ over the n_ flavours of cand_, `first` first, with in_flight frames in flight
    void reset(unsigned long long key_, unsigned long long shape_, int first, const int* cand_, int n_, int in_flight)
    {
        key = key_;
        shape = shape_;
        n = 0;
        cand[n++] = first;
        for (int i = 0; i < n_; ++i)
            if (cand_[i] != first && n < 6) cand[n++] = cand_[i];
        cur = 0;
        issued = 0;
        per = in_flight > 1 ? 3 * in_flight + 2 : 3;  // (<= 14: kStreams is 4)
        settle = in_flight + 3;
        choice = -1;
        chain_ref = 0;
        for (int i = 0; i < 6; ++i) {
            cost[i] = 0.0f;
            for (int q = 0; q < 16; ++q) launch[i][q] = -1;
        }
    }
};
struct Tuner {
    Trial trials[8];
    unsigned long long clock = 0;
    int mode = 1;  // VR_EXP_TUNE=0: the prior alone (round 3's thresholds)
    const Trial* latest() const  // the trial used most recently (vr_kernel_choice), nullptr if none
    {
        const Trial* t = nullptr;
        for (const auto& e : trials)
            if (e.key != 0 && e.used != 0 && (!t || e.used > t->used)) t = &e;
        return t;
    }
};

// The measured kernel choice.  `cand[0 .. n)` are the flavours that may run this launch (cand[0] = the prior's pick); returns the one to
// launch now.  `launch` is the number the coming launch records itself under -- a count of the context's march launches that nothing
// ever rewinds (vr_reset_kernel_times included: a trial that straddles a reset still names its own launches) -- and `rec` answers
// rec.span_ticks(L) / rec.end_ticks(L) for launch number L: its duration + 1 and its last workgroup's end | 1 in 100 MHz ticks, 0 while
// not known.  The caller makes that launch: a call that is followed by none would leave two entries naming one launch.
// A trial gives every candidate `per` launches in turn -- after `settle` launches of the prior, so that a launch order exists (DESIGN
// 4.6: the trial then measures what the steady state runs) -- and reads the launches' durations from the words their sorts fill (no
// synchronisation: a trial is evaluated when its last word has arrived; until then the prior runs).  One launch at a time: the shortest
// first-start-to-last-end span of a candidate's launches but its first.  Launches in flight: the mean interval between the ends of its
// consecutive launches that ran beside launches of the same candidate only (3 x in_flight + 2 launches per turn, the first and the last
// in_flight of them not used).  The trial re-opens when the scene, the tables, the launch shape or the frames-in-flight hint change (the
// key) and when the longest ray chain has moved by more than a quarter.
template <typename Records>
int tune_pick(Tuner& T, const Records& rec, long long launch, int in_flight, unsigned long long key, unsigned long long shape, const int* cand,
              int n, unsigned chain_now, bool measurable)
{
    if (n <= 1) return cand[0];
    Trial* t = nullptr;
    for (auto& e : T.trials)
        if (e.key == key) t = &e;
    if (!t) {
        // a new scene (or table, or arithmetic) of a shape that has been measured before: what that trial kept runs first, if it is
        // still eligible -- a host that edits a table frame after frame keeps its kernel while every new trial settles
        int first = cand[0];
        unsigned long long newest = 0;
        for (const auto& e : T.trials)
            if (e.key != 0 && e.shape == shape && e.choice >= 0 && e.used > newest)
                for (int i = 0; i < n; ++i)
                    if (cand[i] == e.cand[e.choice]) {
                        first = cand[i];
                        newest = e.used;
                    }
        t = &T.trials[0];
        for (auto& e : T.trials)
            if (e.used < t->used) t = &e;
        t->reset(key, shape, first, cand, n, in_flight);
    } else {
        // the eligible set may have changed under the same key (a flavour knob, a table that fits LDS no more)
        bool same = t->n == n;
        for (int i = 0; i < n && same; ++i) {
            bool found = false;
            for (int j = 0; j < t->n; ++j) found = found || t->cand[j] == cand[i];
            same = found;
        }
        if (!same) t->reset(key, shape, cand[0], cand, n, in_flight);
    }
    t->used = ++T.clock;
    if (t->choice >= 0) {
        if (chain_now != 0 && t->chain_ref != 0) {
            const unsigned lo = t->chain_ref - t->chain_ref / 4, hi = t->chain_ref + t->chain_ref / 4;
            if (chain_now < lo || chain_now > hi) t->reset(key, shape, t->cand[t->choice], cand, n, in_flight);  // (the kernel kept so far runs while the new trial settles)
        }
        if (t->choice >= 0) return t->cand[t->choice];
    }
    if (!measurable) return t->cand[0];
    if (t->settle > 0) {
        --t->settle;
        return t->cand[0];
    }
    if (t->cur < t->n) {
        const int f = t->cand[t->cur];
        t->launch[t->cur][t->issued] = launch;
        if (++t->issued == t->per) {
            ++t->cur;
            t->issued = 0;
        }
        return f;
    }
    // every candidate has had its turn: are the records in?
    const long long last = t->launch[t->n - 1][t->per - 1];
    // (a launch of the trial was never measured -- timed with events, or not ordered -- or so many launches of other shapes ran in
    // between that the trial's first ring slots are about to be written again: keep the prior)
    if (launch > last + 64 || launch - t->launch[0][0] >= kRing) {
        t->choice = 0;
        t->chain_ref = chain_now;
        return t->cand[0];
    }
    for (int i = 0; i < t->n; ++i)
        for (int q = 0; q < t->per; ++q)
            if (rec.span_ticks(t->launch[i][q]) == 0) return t->cand[0];
    int best = 0;
    for (int i = 0; i < t->n; ++i) {
        double ticks;
        if (in_flight > 1) {
            // (its first `in_flight` launches ran beside the candidate before it, its last ones beside the next: the ends of the
            // launches in between are `in_flight + 2` intervals apart that are this candidate's alone)
            const unsigned long long e0 = rec.end_ticks(t->launch[i][in_flight]);
            const unsigned long long e1 = rec.end_ticks(t->launch[i][t->per - in_flight]);
            ticks = e1 > e0 ? (double)(e1 - e0) / (double)(t->per - 2 * in_flight) : 1.0e18;
        } else {
            ticks = 1.0e18;
            for (int q = 1; q < t->per; ++q) {
                const double v = (double)rec.span_ticks(t->launch[i][q]);
                ticks = v < ticks ? v : ticks;
            }
        }
        t->cost[i] = (float)(ticks * 1.0e-5);  // 100 MHz ticks -> ms
        // (another kernel must be 2 % faster than the prior's to replace it: the spans of equal kernels differ by about that much)
        // (... with launches in flight by 5 %: a candidate's interior launches still run beside its neighbours' tails -- a trial that
        // measured march_kernel at 0.407 ms per C3 frame pipelined against 0.418 kept it, and it then ran at 0.467)
        if (i > 0 && t->cost[i] < t->cost[best] * (best == 0 ? (in_flight > 1 ? 0.95f : 0.98f) : 1.0f)) best = i;
    }
    t->choice = best;
    t->chain_ref = chain_now;
    return t->cand[best];
}
