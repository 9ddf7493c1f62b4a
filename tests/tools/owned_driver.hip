// owned_driver.hip -- a stand-alone driver of the move-only owner of HIP objects (java-sdr_amd/csrc/common.h: Owned) for
// tests/test_owned_host.py: no device, no library.  The owner is instantiated with a plain integer handle and a destroy
// function that counts its calls and remembers which handles it was given; every rule of ownership is then asserted.
// Prints "ok <checks>" and exits 0, or names the first check that failed and exits 1.
#include "../../java-sdr_amd/csrc/common.h"
#include <utility>
#include <vector>

using namespace jsdr;

static int g_destroyed = 0;
static std::vector<int> g_seen;
static hipError_t fake_destroy(int h)
{
    g_destroyed++;
    g_seen.push_back(h);
    return hipErrorInvalidHandle;  // (the owner ignores the result)
}
typedef Owned<int, fake_destroy> Own;
static_assert(!std::is_copy_constructible<Own>::value && !std::is_copy_assignable<Own>::value, "an owner is not copied");
static_assert(std::is_nothrow_move_constructible<Own>::value && std::is_nothrow_move_assignable<Own>::value, "an owner moves, and cannot fail to");

static int g_checks = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        g_checks++;                                                   \
        if (!(cond)) {                                                \
            printf("failed: %s (line %d)\n", #cond, __LINE__);        \
            return 1;                                                 \
        }                                                             \
    } while (0)

static int times_seen(int h)
{
    int n = 0;
    for (int s : g_seen) n += s == h ? 1 : 0;
    return n;
}

int main()
{
    const long long live0 = live_objects.load();
    {  // a default-constructed owner holds nothing and destroys nothing
        Own a;
        CHECK((int)a == 0);
        a.reset();
    }
    CHECK(g_destroyed == 0);
    {  // destruction destroys exactly once
        Own a;
        a.adopt(11);
        CHECK((int)a == 11 && live_objects.load() == live0 + 1);
    }
    CHECK(g_destroyed == 1 && times_seen(11) == 1);
    {  // move construction: the source is empty, the handle is destroyed once, by the target
        Own a;
        a.adopt(21);
        Own b(std::move(a));
        CHECK((int)a == 0 && (int)b == 21 && g_destroyed == 1);
    }
    CHECK(g_destroyed == 2 && times_seen(21) == 1);
    {  // move assignment: the overwritten target is destroyed at once, once; the source is empty
        Own a, b;
        a.adopt(31);
        b.adopt(32);
        b = std::move(a);
        CHECK(g_destroyed == 3 && times_seen(32) == 1 && times_seen(31) == 0);
        CHECK((int)a == 0 && (int)b == 31);
    }
    CHECK(g_destroyed == 4 && times_seen(31) == 1 && times_seen(32) == 1);
    {  // self-move-assignment is harmless
        Own a;
        a.adopt(41);
        Own &alias = a;
        a = std::move(alias);
        CHECK((int)a == 41 && g_destroyed == 4);
    }
    CHECK(g_destroyed == 5 && times_seen(41) == 1);
    {  // reset() twice destroys once, and the destructor has nothing left to do
        Own a;
        a.adopt(51);
        a.reset();
        a.reset();
        CHECK(g_destroyed == 6 && (int)a == 0);
    }
    CHECK(g_destroyed == 6 && times_seen(51) == 1);
    {  // adopting over a held handle destroys the held one
        Own a;
        a.adopt(55);
        a.adopt(56);
        CHECK(g_destroyed == 7 && times_seen(55) == 1 && (int)a == 56);
    }
    CHECK(g_destroyed == 8 && times_seen(56) == 1);
    {  // a vector of owners that reallocates (several times) destroys each handle once, when the vector goes
        std::vector<Own> v;
        size_t moved = 0, cap = v.capacity();
        for (int i = 0; i < 100; i++) {
            Own a;
            a.adopt(1000 + i);
            v.push_back(std::move(a));
            if (v.capacity() != cap) moved++, cap = v.capacity();
        }
        CHECK(moved >= 2 && g_destroyed == 8);
        for (int i = 0; i < 100; i++) CHECK((int)v[(size_t)i] == 1000 + i);
        // an owner moved out of the vector takes its handle along (how a pool hands out an event)
        Own last = std::move(v.back());
        v.pop_back();
        CHECK((int)last == 1099 && g_destroyed == 8 && live_objects.load() == live0 + 100);
    }
    CHECK(g_destroyed == 108);
    for (int i = 0; i < 100; i++) CHECK(times_seen(1000 + i) == 1);
    {  // std::swap destroys nothing
        Own a, b;
        a.adopt(61);
        b.adopt(62);
        std::swap(a, b);
        CHECK((int)a == 62 && (int)b == 61 && g_destroyed == 108);
    }
    CHECK(g_destroyed == 110 && times_seen(61) == 1 && times_seen(62) == 1);
    CHECK(live_objects.load() == live0);  // the count of live objects is back where it was
    printf("ok %d\n", g_checks);
    return 0;
}
