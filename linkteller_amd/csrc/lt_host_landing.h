// The host side of the packed host landing (lt_influence.hip, influence_host_impl): the consumer of the value run.  Plain C++, no HIP
// include: tests/host_landing_main.cpp drives it on a CPU with a thread in the GPU's place.
//
// The packed run is two arrays of one numbering: idx[e] = where entry e goes in the caller's float64 matrix, val[e] = its fp32 value.
// The indices and the run's length arrive early in the step behind the ready word (ready[0] = total + 1, stored after ready[1] =
// total and after every index; the reader's acquire load pairs with it).  The values arrive at the step's end, one 4-byte store
// each, in no order -- and ANNOUNCE THEMSELVES: outside a call every word of the value region holds a sentinel bit pattern, each
// entry gets exactly one value store, so a word that differs from the sentinel holds its final value.  No flag, no ordering between
// words, no acquire.  The consumer walks the run front to back, places (double)v into dst and stores the sentinel back into the
// word it consumed (the line is in this core's L1): the region is armed again when the call returns, without a pass of its own.
// A word that still reads as the sentinel is passed over and comes round again (the probes' blocks finish in no particular order:
// a walk that stalled on the first missing word would sit out the arrival of all the others and only then begin to place); with
// no room to remember it, the walk stalls on it.  (Remembering the words by groups of 16, a line of values, and looking at one
// word per group measured slower than this plain list: profiles/host_poll_ab.txt.)
//
// Correctness never rests on the sentinel being impossible as a value.  Stalls are bounded by a budget; when it runs out the
// consumer calls settle() ONCE -- the stream wait -- and after its success whatever a word holds IS its value: the rest of the run
// is placed in the late form (no look at the sentinel).  A value that happens to equal the sentinel costs one budget, never a
// wrong matrix.  The budget also keeps a faulted stream from spinning for ever: settle() then reports the stream's error.
#ifndef LT_HOST_LANDING_H
#define LT_HOST_LANDING_H
#include <stddef.h>
#include <stdint.h>
#include <time.h>
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#define LT_LANDING_PAUSE() _mm_pause()
#define LT_LANDING_ACQUIRE_FENCE() __atomic_signal_fence(__ATOMIC_ACQUIRE)      // (loads are not reordered with loads: the compiler is all there is to hold)
#else
#define LT_LANDING_PAUSE() ((void)0)
#define LT_LANDING_ACQUIRE_FENCE() __atomic_thread_fence(__ATOMIC_ACQUIRE)
#endif

static inline int64_t lt_now_ns() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (int64_t)ts.tv_sec * 1000000000ll + ts.tv_nsec;
}

#define LT_LANDING_SENTINEL 0xFFFFFFFFu      // a negative NaN with full payload: sqrtf of a sum of squares of finite inputs never is
#define LT_LANDING_BUDGET_NS 200000          // three headline steps; the wait it replaces is 28 us.  A bound, not a tuned figure (and
                                             // coarse: see lt_landing::stall_ns -- about 250 us before the fallback in practice)
#define LT_LANDING_CLOCK_EVERY 1024          // looks between two reads of the clock

struct lt_landing {
    // in
    const uint32_t *idx;        // the index run
    uint32_t *val;              // the value run, as words (armed on entry)
    const unsigned *ready;      // the ready line: [0] total + 1 once published (0 before), [1] total
    double *dst;
    uint64_t lim;               // an index >= lim is not placed (its word is consumed and re-armed like any other)
    size_t cap;                 // entries the run can hold: total is clamped to it
    uint32_t sentinel;
    int64_t budget_ns;
    int (*settle)(void *);      // the stream wait: 0 = every store of the call has landed; else the error, passed through
    void *settle_arg;
    void (*on_ready)(void *, size_t total);   // optional: called once, when the ready word was seen before any settle, in front of the walk
    void *on_ready_arg;
    uint32_t *pending;          // optional scratch of pending_cap words: so many entries that are not there yet are passed over and
    size_t pending_cap;         // come round again (the order of arrival is not the run's); beyond it, and without it, the walk stalls
    bool stamps;                // take t_ready / t_first / t_last and idle_ns (clock reads around every stall)
    // out
    size_t total;               // entries of the run (0 when it was never published)
    size_t placed;              // total when every entry was consumed by look (else 0: some were placed behind settle)
    bool settled;               // settle() was called (the fallback) and succeeded
    bool published;             // the ready word was seen (before or behind settle)
    int64_t looks;              // loads that found the ready word 0 or a value word still armed: every reload of a stall, and in the
                                // rounds every entry of the pending list that a round rescanned and left there (not its first pass-over)
    int64_t late_entries;       // entries whose first look found the sentinel
    int64_t stall_ns;           // what the budget saw.  The clock is read every LT_LANDING_CLOCK_EVERY looks only.  In the ready wait and in a
                                // strict stall this is stall time, counted from the stall's first such look on (a stall of fewer looks
                                // counts nothing).  In the rounds it is ALL time since the rounds' first clock read, placing included:
                                // there the budget bounds how long the pending list may stay non-empty, not how long the host idled.
                                // With a pause of ~45 ns one clock interval is 40-50 us: the effective bound is budget_ns + one interval
    int64_t t_ready, t_first, t_last;
    int64_t idle_ns;            // (stamps) time in stalls and in rounds that placed nothing
};

static inline void lt_landing_arm(uint32_t *w, size_t words, uint32_t sentinel) {
    for (size_t i = 0; i < words; ++i) __atomic_store_n(w + i, sentinel, __ATOMIC_RELAXED);
}

// The late form: entries [from, total) behind a successful stream wait -- a word's content is its value, whatever it looks like --
// each word armed again as it is consumed.
static inline void lt_landing_place_late(const uint32_t *idx, uint32_t *val, size_t from, size_t total, double *dst, uint64_t lim,
                                         uint32_t sentinel) {
    for (size_t e = from; e < total; ++e) {
        const uint32_t x = idx[e];
        const uint32_t v = __atomic_load_n(val + e, __ATOMIC_RELAXED);
        if (x < lim) {
            float f;
            __builtin_memcpy(&f, &v, 4);
            dst[x] = (double)f;
        }
        __atomic_store_n(val + e, sentinel, __ATOMIC_RELAXED);
    }
}

// One stalled look is behind us.  True when the budget has run out.
static inline bool lt_landing_look(lt_landing &L, int64_t &mark) {
    LT_LANDING_PAUSE();
    if ((++L.looks % LT_LANDING_CLOCK_EVERY) != 0) return false;
    const int64_t now = lt_now_ns();
    if (mark) L.stall_ns += now - mark;
    mark = now;
    return L.stall_ns > L.budget_ns;
}

// Returns 0 with the matrix complete in dst and val[0, total) armed again -- L.settled tells whether the stream wait was needed --
// or settle()'s error (nothing more was placed; the caller re-arms in bulk).  A run that is not published even behind a successful
// settle() returns 0 with L.published false and L.total 0: the caller reports it.
static inline int lt_landing_consume(lt_landing &L) {
    L.total = L.placed = 0;
    L.settled = L.published = false;
    L.looks = L.late_entries = L.stall_ns = 0;
    L.t_ready = L.t_first = L.t_last = L.idle_ns = 0;
    int64_t mark = 0;
    bool out_of_budget = false;
    const uint32_t *const idx = L.idx;       // (locals: the stores below could alias the fields)
    uint32_t *const val = L.val;
    double *const dst = L.dst;
    const uint64_t lim = L.lim;
    const uint32_t sentinel = L.sentinel;
    // ---- the ready word, then total: bounded like every stall
    unsigned r = __atomic_load_n(L.ready, __ATOMIC_ACQUIRE);
    while (r == 0u) {
        if (lt_landing_look(L, mark)) { out_of_budget = true; break; }
        r = __atomic_load_n(L.ready, __ATOMIC_ACQUIRE);
    }
    mark = 0;
    size_t e = 0, np = 0;      // the walk's position; entries passed over and still out
    if (!out_of_budget) {
        L.published = true;
        const size_t published = (size_t)__atomic_load_n(L.ready + 1, __ATOMIC_RELAXED);
        L.total = published < L.cap ? published : L.cap;
        if (L.stamps) L.t_ready = lt_now_ns();
        if (L.on_ready) L.on_ready(L.on_ready_arg, L.total);
        // ---- the walk (a run of no entries looks at no value word)
        const size_t total = L.total;
        const bool stamps = L.stamps;
        uint32_t *const pend = L.pending;
        const size_t pcap = pend ? L.pending_cap : 0;
        int64_t late = 0, t_idle = 0;
        for (; e < total; ++e) {
            const uint32_t x = idx[e];
            uint32_t v = __atomic_load_n(val + e, __ATOMIC_RELAXED);
            if (v == sentinel) {
                ++late;
                if (np < pcap) { pend[np++] = (uint32_t)e; continue; }      // not there yet: later, the walk goes on
                if (stamps) t_idle = lt_now_ns();
                do {
                    if (lt_landing_look(L, mark)) { out_of_budget = true; break; }
                    v = __atomic_load_n(val + e, __ATOMIC_RELAXED);
                } while (v == sentinel);
                mark = 0;
                if (stamps) L.idle_ns += lt_now_ns() - t_idle;
                if (out_of_budget) break;
            }
            if (stamps && !L.t_first) L.t_first = lt_now_ns();
            if (x < lim) {
                float f;
                __builtin_memcpy(&f, &v, 4);
                dst[x] = (double)f;
            }
            __atomic_store_n(val + e, sentinel, __ATOMIC_RELAXED);
        }
        L.late_entries = late;
        // ---- the entries passed over, round after round (in the run's order: a sequential read of the value lines) until none is
        // left: whatever has landed is placed, in any order
        int64_t checked = L.looks;
        while (np > 0 && !out_of_budget) {
            if (stamps) t_idle = lt_now_ns();
            size_t keep = 0;
            for (size_t i = 0; i < np; ++i) {
                const uint32_t q = pend[i];
                const uint32_t v = __atomic_load_n(val + q, __ATOMIC_RELAXED);
                if (v == sentinel) { pend[keep++] = q; continue; }
                const uint32_t x = idx[q];
                if (x < lim) {
                    float f;
                    __builtin_memcpy(&f, &v, 4);
                    dst[x] = (double)f;
                }
                __atomic_store_n(val + q, sentinel, __ATOMIC_RELAXED);
            }
            L.looks += (int64_t)keep;
            if (keep == np) {       // (a round that found nothing)
                LT_LANDING_PAUSE();
                if (stamps) L.idle_ns += lt_now_ns() - t_idle;
            } else if (stamps && !L.t_first) L.t_first = lt_now_ns();
            np = keep;
            if (np > 0 && L.looks - checked >= LT_LANDING_CLOCK_EVERY) {      // the budget: the time since the rounds' first such check
                checked = L.looks;
                const int64_t now = lt_now_ns();
                if (mark) L.stall_ns += now - mark;
                mark = now;
                out_of_budget = L.stall_ns > L.budget_ns;
            }
        }
        if (!out_of_budget) L.placed = total;
        if (L.stamps) L.t_last = lt_now_ns();
        // (what was read is ordered before anything the caller reads next -- the node-id flag words)
        LT_LANDING_ACQUIRE_FENCE();
        if (!out_of_budget) return 0;
    }
    // ---- the fallback: the stream wait, once; behind it a word's content is its value, whatever it looks like
    const int rc = L.settle(L.settle_arg);
    if (rc) return rc;
    L.settled = true;
    if (!L.published) {
        if (__atomic_load_n(L.ready, __ATOMIC_ACQUIRE) == 0u) return 0;
        L.published = true;
        const size_t total = (size_t)__atomic_load_n(L.ready + 1, __ATOMIC_RELAXED);
        L.total = total < L.cap ? total : L.cap;
    }
    // (the entries passed over that are still out, then everything from where the walk stopped)
    for (size_t i = 0; i < np; ++i) lt_landing_place_late(idx, val, L.pending[i], (size_t)L.pending[i] + 1, dst, lim, sentinel);
    lt_landing_place_late(idx, val, e, L.total, dst, lim, sentinel);
    return 0;
}
#endif
