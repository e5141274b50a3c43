// Drives the consumer of the packed value run (linkteller_amd/csrc/lt_host_landing.h) on a CPU: a thread stands in for the GPU.
// Built and run by tests/test_host_landing_cpu.py under -fsanitize=thread and under -fsanitize=address,undefined.
// Exit status 0 = every case passed in every form of the walk; each failure prints a line.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "lt_host_landing.h"

namespace {
int g_failures = 0;
#define EXPECT(cond, ...)                                                   \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++g_failures;                                                   \
            std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond);    \
            std::printf(__VA_ARGS__);                                       \
            std::printf("\n");                                              \
        }                                                                   \
    } while (0)

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

enum Producer { RANDOM_BLOCKS, BEFORE_CONSUMER, AFTER_READY };
struct Case {
    const char *name;
    Producer how;
    size_t rows, ld, cols;      // dst is rows x ld, the last ld - cols columns are padding
    size_t total;               // entries of the run
    long hold;                  // entry left unwritten until settle(), or -1
    uint32_t sentinel;
    long equal_sentinel;        // entry whose VALUE is the sentinel's pattern, or -1
    long bad_index;             // entry whose index is out of bounds, or -1
    bool publish;               // false: the ready word never comes before settle()
    int settle_rc;              // what settle() returns
    int64_t budget_ns;
    unsigned seed;
};

struct World {
    std::vector<uint32_t> idx, val, want_val;
    alignas(64) unsigned ready[16];
    std::vector<double> dst, want;
    size_t region;              // words of the value region (larger than the run: the rest must stay armed)
    Case c;
    std::thread producer;
    int settles = 0;
    long held = -1;
    bool publish_in_settle = false;
};

void store_value(World &w, size_t e) { __atomic_store_n(&w.val[e], w.want_val[e], __ATOMIC_RELAXED); }
void publish(World &w) {
    __atomic_store_n(&w.ready[1], (unsigned)w.c.total, __ATOMIC_RELAXED);
    __atomic_store_n(&w.ready[0], (unsigned)w.c.total + 1u, __ATOMIC_RELEASE);
}

// the "GPU": indices first, the ready word, then the values in the order and at the pace the case names
void produce(World *wp) {
    World &w = *wp;
    std::mt19937 rng(w.c.seed);
    const size_t total = w.c.total;
    auto nap = [&](unsigned max_us) {
        const unsigned us = rng() % (max_us + 1);
        if (us) std::this_thread::sleep_for(std::chrono::microseconds(us));
    };
    if (w.c.how == AFTER_READY) {
        if (w.c.publish) publish(w);
        nap(300);
        for (size_t e = 0; e < total; ++e)
            if ((long)e != w.held) store_value(w, e);
        return;
    }
    // blocks of up to 16 entries in random order
    std::vector<size_t> blocks;
    for (size_t b0 = 0; b0 < total; b0 += 16) blocks.push_back(b0);
    std::shuffle(blocks.begin(), blocks.end(), rng);
    if (w.c.publish) publish(w);
    for (size_t b0 : blocks) {
        if (w.c.how == RANDOM_BLOCKS && rng() % 4 == 0) nap(40);
        for (size_t e = b0; e < b0 + 16 && e < total; ++e)
            if ((long)e != w.held) store_value(w, e);
    }
}

int settle(void *p) {
    World &w = *static_cast<World *>(p);
    ++w.settles;
    if (w.producer.joinable()) w.producer.join();      // the stream wait: everything the "GPU" does is done
    if (w.c.settle_rc) return w.c.settle_rc;
    if (w.held >= 0) store_value(w, (size_t)w.held);
    if (w.publish_in_settle) publish(w);
    return 0;
}

void run_case(const Case &c, size_t pending_cap) {
    World w;
    w.c = c;
    std::mt19937 rng(c.seed * 7919u + 1u);
    const size_t cells = c.rows * c.cols;
    w.region = c.total + 37;
    w.idx.assign(c.total + 1, 0xdeadbeefu);
    w.val.assign(w.region, c.sentinel);
    w.want_val.assign(c.total, 0);
    std::memset(w.ready, 0, sizeof(w.ready));
    w.dst.assign(c.rows * c.ld, 0.0);
    for (size_t i = 0; i < c.rows; ++i)
        for (size_t j = c.cols; j < c.ld; ++j) w.dst[i * c.ld + j] = 7.0;      // padding: left as it is
    w.want = w.dst;
    // distinct cells in random order, positive finite values
    std::vector<size_t> cell(cells);
    for (size_t i = 0; i < cells; ++i) cell[i] = i;
    std::shuffle(cell.begin(), cell.end(), rng);
    for (size_t e = 0; e < c.total; ++e) {
        const size_t i = cell[e] / c.cols, j = cell[e] % c.cols;
        w.idx[e] = (uint32_t)(i * c.ld + j);
        float f = std::sqrt((float)(rng() % 100000 + 1) * 1e-3f);
        uint32_t u = bits_of(f);
        if ((long)e == c.equal_sentinel) u = c.sentinel;
        else if (u == c.sentinel) u ^= 1u;
        w.want_val[e] = u;
        float back;
        std::memcpy(&back, &u, 4);
        if ((long)e == c.bad_index) w.idx[e] = (uint32_t)(c.rows * c.ld + 5);
        else w.want[w.idx[e]] = (double)back;
    }
    w.held = c.hold;
    w.publish_in_settle = !c.publish && c.settle_rc == 0 && c.hold != -2;

    lt_landing L = {};
    L.idx = w.idx.data(); L.val = w.val.data(); L.ready = w.ready; L.dst = w.dst.data();
    L.lim = (uint64_t)c.rows * c.ld; L.cap = cells; L.sentinel = c.sentinel; L.budget_ns = c.budget_ns;
    L.settle = settle; L.settle_arg = &w;
    L.stamps = true;
    std::vector<uint32_t> pending(pending_cap + 1, 0xfeedf00du);
    if (pending_cap) { L.pending = pending.data(); L.pending_cap = pending_cap; }
    if (c.how == BEFORE_CONSUMER) produce(&w);
    else w.producer = std::thread(produce, &w);
    const int rc = lt_landing_consume(L);
    if (w.producer.joinable()) w.producer.join();

    const bool expect_settle = c.hold >= 0 || c.equal_sentinel >= 0 || !c.publish;
    EXPECT(rc == c.settle_rc * (expect_settle ? 1 : 0), "%s: rc %d", c.name, rc);
    EXPECT(w.settles == (expect_settle ? 1 : 0), "%s: settle() called %d times", c.name, w.settles);
    if (rc == 0) {
        EXPECT(L.settled == expect_settle, "%s: settled %d", c.name, (int)L.settled);
        const bool never_published = !c.publish && !w.publish_in_settle;
        EXPECT(L.published == !never_published, "%s: published %d", c.name, (int)L.published);
        if (!never_published) {
            EXPECT(L.total == c.total, "%s: total %zu", c.name, L.total);
            size_t wrong = 0;
            for (size_t i = 0; i < w.dst.size(); ++i) wrong += std::memcmp(&w.dst[i], &w.want[i], 8) != 0;
            EXPECT(wrong == 0, "%s: %zu cells of the matrix differ", c.name, wrong);
            if (!expect_settle) EXPECT(L.placed == c.total, "%s: placed %zu by look", c.name, L.placed);
            if (c.total > 0 && !expect_settle) EXPECT(L.t_ready && L.t_first >= L.t_ready && L.t_last >= L.t_first, "%s: stamps", c.name);
        }
        if (c.publish || w.publish_in_settle) {
            size_t unarmed = 0;
            for (size_t e = 0; e < w.region; ++e) unarmed += __atomic_load_n(&w.val[e], __ATOMIC_RELAXED) != c.sentinel;
            EXPECT(unarmed == 0, "%s: %zu words of the value region are not armed after the call", c.name, unarmed);
        }
    }
    EXPECT(w.idx[c.total] == 0xdeadbeefu, "%s: the word behind the index run changed", c.name);
    EXPECT(pending[pending_cap] == 0xfeedf00du, "%s: the word behind the pending list changed", c.name);
}
}      // namespace

int main() {
    const uint32_t S = LT_LANDING_SENTINEL;
    const uint32_t real = bits_of(std::sqrt(2.0f));
    // The stall budget.  Where the case must NOT take the budget path: far above anything a loaded machine needs to start a thread
    // and wake it from its naps.  Where it must (a word that never comes before settle()): short, the outcome does not depend on it.
    const int64_t B = 5000000000ll, Bs = 20000000;
    const Case cases[] = {
        // name                      producer         rows ld  cols total hold  sentinel  equal bad  publish rc budget seed
        {"random, one word held",    RANDOM_BLOCKS,   23,  25, 23,  301,  137,  S,        -1,   -1,  true,   0, Bs,    1},
        {"before, one word held",    BEFORE_CONSUMER, 23,  25, 23,  301,  0,    S,        -1,   -1,  true,   0, Bs,    2},
        {"after, one word held",     AFTER_READY,     23,  25, 23,  301,  300,  S,        -1,   -1,  true,   0, Bs,    3},
        {"random, nothing held",     RANDOM_BLOCKS,   40,  40, 40,  1600, -1,   S,        -1,   -1,  true,   0, B,     4},
        {"before, nothing held",     BEFORE_CONSUMER, 9,   12, 9,   50,   -1,   S,        -1,   -1,  true,   0, B,     5},
        {"after, nothing held",      AFTER_READY,     9,   9,  9,   81,   -1,   S,        -1,   -1,  true,   0, B,     6},
        {"one entry",                AFTER_READY,     1,   1,  1,   1,    -1,   S,        -1,   -1,  true,   0, B,     7},
        {"no entries",               RANDOM_BLOCKS,   5,   5,  5,   0,    -1,   S,        -1,   -1,  true,   0, B,     8},
        {"a value is the sentinel",  RANDOM_BLOCKS,   16,  17, 16,  200,  -1,   real,     77,   -1,  true,   0, Bs,    9},
        {"the first is the sentinel",BEFORE_CONSUMER, 16,  17, 16,  200,  -1,   real,     0,    -1,  true,   0, Bs,    10},
        {"an index out of bounds",   RANDOM_BLOCKS,   16,  16, 16,  120,  -1,   S,        -1,   60,  true,   0, B,     11},
        {"published behind settle",  BEFORE_CONSUMER, 8,   8,  8,   40,   -1,   S,        -1,   -1,  false,  0, Bs,    12},
        {"never published",          BEFORE_CONSUMER, 8,   8,  8,   40,   -2,   S,        -1,   -1,  false,  0, Bs,    13},
        {"settle fails",             RANDOM_BLOCKS,   8,   8,  8,   40,   20,   S,        -1,   -1,  true,   3, Bs,    14},
    };
    // every case with the strict front-to-back walk, with room to pass over 48 entries (the walk stalls beyond), and with room for all
    for (const Case &c : cases)
        for (size_t pending_cap : {(size_t)0, (size_t)48, (size_t)2048}) run_case(c, pending_cap);
    if (g_failures) std::printf("%d failures\n", g_failures);
    else std::printf("ok %zu cases\n", sizeof(cases) / sizeof(cases[0]));
    return g_failures ? 1 : 0;
}
