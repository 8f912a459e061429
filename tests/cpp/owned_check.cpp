// Stand-alone host check of rrtmg_lw_amd/csrc/owned.hpp - Owned, GrowBuf and NoDestroy - over counting traits: every acquire and release
// is recorded with its handle, a handle is a heap object of its own (a second release of one is a double free, an unreleased one a leak):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rrtmg_lw_amd/csrc tests/cpp/owned_check.cpp -o owned_check && ./owned_check
// (tests/test_owned.py builds it plain and with the sanitizers)
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "owned.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

struct Rec { char what; int id; size_t bytes; };          // 'A' acquire, 'R' release
static std::vector<Rec> g_log;
static std::set<int> g_live, g_released;
static int g_next_id = 1, g_double = 0, g_unknown = 0;
static int g_fail_acquire = 0, g_fail_release = 0;       // the code the next call answers with (once)

struct Fake {
    using handle = int *;
    static int *make(size_t bytes = 0)
    {
        int *h = new int(g_next_id++);
        g_log.push_back({'A', *h, bytes});
        g_live.insert(*h);
        return h;
    }
    static int acquire(int **p, size_t bytes)
    {
        if (g_fail_acquire) { const int rc = g_fail_acquire; g_fail_acquire = 0; return rc; }
        *p = make(bytes);
        return 0;
    }
    static int release(int *h)        // (like hipFree: the handle is gone even when the call answers with an error)
    {
        const int id = *h;
        g_log.push_back({'R', id, 0});
        if (g_released.count(id)) g_double++;
        if (!g_live.erase(id)) g_unknown++;
        g_released.insert(id);
        delete h;
        if (g_fail_release) { const int rc = g_fail_release; g_fail_release = 0; return rc; }
        return 0;
    }
};
using Own = owned::Owned<Fake>;
using Buf = owned::GrowBuf<Fake>;

static size_t count(char what) { size_t n = 0; for (auto &r : g_log) n += r.what == what; return n; }
static bool last_is(char what, int id) { return !g_log.empty() && g_log.back().what == what && g_log.back().id == id; }

static void owned_cases()
{
    {   // construct / destroy: an empty owner releases nothing, a live one its handle, once
        Own e;
        CHECK(!e && e.get() == nullptr);
    }
    CHECK(g_log.empty());
    int id;
    {
        Own a;
        *a.slot() = Fake::make();
        id = *a.get();
        CHECK(a && g_live.count(id));
    }
    CHECK(last_is('R', id) && count('R') == 1);
    {   // move-construct: the source is empty, nothing is released by the move
        Own a;
        *a.slot() = Fake::make();
        id = *a.get();
        const size_t r0 = count('R');
        Own b(std::move(a));
        CHECK(!a && b && *b.get() == id && count('R') == r0);
        // move-assign over empty
        Own c;
        c = std::move(b);
        CHECK(!b && c && *c.get() == id && count('R') == r0);
        // move-assign over live: the old handle released exactly once, the source empty
        Own d;
        *d.slot() = Fake::make();
        const int old = *d.get();
        d = std::move(c);
        CHECK(!c && *d.get() == id && last_is('R', old) && count('R') == r0 + 1);
        // self-move keeps the handle
        Own &dd = d;
        d = std::move(dd);
        CHECK(d && *d.get() == id && count('R') == r0 + 1);
        // reset twice
        CHECK(d.reset() == 0 && !d && last_is('R', id) && count('R') == r0 + 2);
        CHECK(d.reset() == 0 && count('R') == r0 + 2);
    }
    {   // the create-into-slot accessor over a live handle releases it first
        Own a;
        *a.slot() = Fake::make();
        const int old = *a.get();
        int **s = a.slot();
        CHECK(last_is('R', old) && *s == nullptr && !a);
        *s = Fake::make();
        CHECK(a && *a.get() != old);
        // a failing release is reported by reset, and the owner is empty all the same
        g_fail_release = 7;
        CHECK(a.reset() == 7 && !a);
    }
}

static void growbuf_cases()
{
    const size_t l0 = g_log.size();                                       // (the log of the cases before)
    Buf b;
    CHECK(!b && b.bytes() == 0 && b.as<int>() == nullptr);
    CHECK(b.reserve(0, 0) == 0 && g_log.size() == l0 && !b);                 // nothing needed, nothing done
    CHECK(b.reserve(100, 164) == 0 && b && b.bytes() == 164);             // `want` honoured
    CHECK(g_log.size() == l0 + 1 && g_log[l0].what == 'A' && g_log[l0].bytes == 164);
    const int first = *b.get();
    for (size_t need : {(size_t)1, (size_t)100, (size_t)164}) {          // below / at the capacity: no traffic
        CHECK(b.reserve(need, need + 50) == 0 && g_log.size() == l0 + 1 && *b.get() == first && b.bytes() == 164);
    }
    CHECK(b.reserve(165, 165) == 0 && b.bytes() == 165);                  // above: release strictly before acquire
    CHECK(g_log.size() == l0 + 3 && g_log[l0 + 1].what == 'R' && g_log[l0 + 1].id == first && g_log[l0 + 2].what == 'A' && g_log[l0 + 2].bytes == 165);
    // a failing acquire: empty, capacity 0, the code handed back; the next reserve succeeds
    const int second = *b.get();
    g_fail_acquire = 2;
    CHECK(b.reserve(1000, 1000) == 2 && !b && b.bytes() == 0 && b.get() == nullptr && last_is('R', second));
    CHECK(b.reserve(10, 10) == 0 && b && b.bytes() == 10 && g_log.back().what == 'A' && g_log.back().bytes == 10);
    // a failing release on the growth path is reported: nothing is allocated, the buffer is empty
    const int third = *b.get();
    g_fail_release = 9;
    const size_t a0 = count('A');
    CHECK(b.reserve(20, 20) == 9 && !b && b.bytes() == 0 && last_is('R', third) && count('A') == a0);
    CHECK(b.reserve(20, 24) == 0 && b.bytes() == 24);
    // moves carry the capacity and leave the source at 0
    Buf c(std::move(b));
    CHECK(!b && b.bytes() == 0 && c && c.bytes() == 24);
    Buf d;
    CHECK(d.reserve(8, 8) == 0);
    const int old = *d.get();
    d = std::move(c);
    CHECK(!c && c.bytes() == 0 && d.bytes() == 24 && last_is('R', old));
    CHECK(*d.as<int>() == *d.get());
    Buf &dd = d;
    d = std::move(dd);
    CHECK(d && d.bytes() == 24);
    CHECK(d.reset() == 0 && !d && d.bytes() == 0);
}

struct Holder { Own o; Buf b; };
static void nodestroy_cases()
{
    using Keep = owned::NoDestroy<Holder>;
    alignas(Keep) static unsigned char room[sizeof(Keep)];
    const size_t r0 = count('R');
    Keep *keep = new (room) Keep;
    Holder *inside = &keep->get();
    *inside->o.slot() = Fake::make();
    CHECK(inside->b.reserve(32, 32) == 0);
    keep->~Keep();
    CHECK(count('R') == r0 && g_live.size() == 2);       // its destructor path released nothing
    *inside = Holder{};                                   // (whoever owns the contents releases them; `room` is still there)
    CHECK(count('R') == r0 + 2 && g_live.empty());
}

int main()
{
    owned_cases();
    growbuf_cases();
    nodestroy_cases();
    static owned::NoDestroy<Holder> at_exit;              // (a live handle in a static: nothing runs for it at exit; released by hand below)
    *at_exit.get().o.slot() = Fake::make();
    CHECK(g_live.size() == 1);
    // acquires = releases + live; no handle released twice, none that was never acquired
    CHECK(count('A') == count('R') + g_live.size());
    CHECK(g_double == 0 && g_unknown == 0);
    at_exit.get().o.reset();
    CHECK(g_live.empty() && count('A') == count('R'));
    std::printf(failures ? "owned_check: %d FAILED\n" : "owned_check: ok\n", failures);
    return failures ? 1 : 0;
}
