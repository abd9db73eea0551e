// tuner_driver.cpp -- the measured kernel choice (csrc/vr_tuner.h) on the CPU, for tests/test_tuner.py: tune_pick over a model of the
// context's kernel-time ring whose spans and ends the test invents.  Plain C++, no HIP: built with g++ into tests/_build/.
//
// The model is what enqueue_render / finish_slot / vr_reset_kernel_times do to the words tune_pick reads: a launch takes the number
// `head`, zeroes slot head % kRing and advances the head (td_launch); its sort's report arrives whenever the test says (td_report) and
// writes that slot, whoever owns it by then; a reset moves the point vr_kernel_times reports from (td_reset).  `rewind` models a context
// whose reset sets the launch counter back to 0 instead: tests use it to show that the reset cases can tell the difference.
#include "vr_tuner.h"

#include <cstring>

namespace {

struct Driver {
    Tuner tuner;
    unsigned long long span[kRing] = {}, end[kRing] = {};
    long long head = 0, reported_from = 0;
    bool rewind = false;
};
struct Records {
    const Driver& d;
    unsigned long long span_ticks(long long launch) const { return d.span[launch % kRing]; }
    unsigned long long end_ticks(long long launch) const { return d.end[launch % kRing]; }
};
const Trial* find(const Driver* d, unsigned long long key)
{
    for (const auto& e : d->tuner.trials)
        if (e.key == key && key != 0) return &e;
    return nullptr;
}

}  // namespace

extern "C" {

int td_ring(void) { return kRing; }
void* td_create(int rewind) { Driver* d = new Driver(); return d->rewind = rewind != 0, d; }
void td_destroy(void* h) { delete (Driver*)h; }

// choose_flavour's call: the flavour the coming launch runs
int td_pick(void* h, unsigned long long key, unsigned long long shape, const int* cand, int n, unsigned chain_now, int measurable, int in_flight)
{
    Driver* d = (Driver*)h;
    return tune_pick(d->tuner, Records{*d}, d->head, in_flight, key, shape, cand, n, chain_now, measurable != 0);
}
// the launch itself: returns the number it took
long long td_launch(void* h)
{
    Driver* d = (Driver*)h;
    d->span[d->head % kRing] = d->end[d->head % kRing] = 0;
    return d->head++;
}
// the report of launch number `launch`'s sort
void td_report(void* h, long long launch, unsigned long long span, unsigned long long end)
{
    Driver* d = (Driver*)h;
    d->end[launch % kRing] = end;
    d->span[launch % kRing] = span;
}
void td_reset(void* h)
{
    Driver* d = (Driver*)h;
    if (d->rewind) d->head = 0;
    else d->reported_from = d->head;
}
long long td_head(void* h) { return ((Driver*)h)->head; }
// vr_kernel_times' count: launches it would report
long long td_reported(void* h)
{
    const Driver* d = (Driver*)h;
    const long long since = d->head - d->reported_from;
    return since < kRing ? since : kRing;
}
// vr_kernel_choice for the trial of `key`: candidates, costs, the one kept; returns their number, -1 if the key has no trial
int td_choice(void* h, unsigned long long key, int cand[6], float cost[6], int* chosen)
{
    const Trial* t = find((Driver*)h, key);
    if (!t) return -1;
    std::memcpy(cand, t->cand, sizeof t->cand);
    std::memcpy(cost, t->cost, sizeof t->cost);
    *chosen = t->choice;
    return t->n;
}
// the launch numbers a trial holds, [6][16] (-1 = none), and its chain_ref; returns launches per candidate, -1 if the key has no trial
int td_launches(void* h, unsigned long long key, long long launch[96], unsigned* chain_ref)
{
    const Trial* t = find((Driver*)h, key);
    if (!t) return -1;
    std::memcpy(launch, t->launch, sizeof t->launch);
    *chain_ref = t->chain_ref;
    return t->per;
}
// the keys in the eight trial slots (0 = free)
void td_slots(void* h, unsigned long long keys[8])
{
    const Driver* d = (Driver*)h;
    for (int i = 0; i < 8; ++i) keys[i] = d->tuner.trials[i].key;
}
// the key vr_kernel_choice would report (Tuner::latest), 0 if none
unsigned long long td_latest(void* h)
{
    const Trial* t = ((Driver*)h)->tuner.latest();
    return t ? t->key : 0;
}

}  // extern "C"
