// tools/dispatch_check.cpp — dev tool: dispatch.hpp (what every launch site uses to turn the handle's runtime state into template
// arguments) under the host address and undefined-behaviour sanitizers, with no GPU.
//   pick       for every combination of one to four flags: the constants handed to fn equal the runtime values, fn runs exactly once,
//              and pick returns fn's value (a void fn compiles too)
//   pick_int   every listed value arrives as itself; a negative, zero, one past the largest and INT_MAX arrive as the last listed value
//              (a ladder's `default:`), for lists whose last value is the largest, the smallest, in the middle and the only one
//   launch_grid  the grid each converted site wrote out by hand: ceil(work / per_wg), capped, floored
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Inavierstokes_amd/csrc -o /tmp/dispatch_check tools/dispatch_check.cpp && /tmp/dispatch_check
#include "dispatch.hpp"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <initializer_list>

static int bad = 0, cases = 0;

static void expect(bool ok, const char* what)
{
    if (!ok && bad++ < 40) printf("%s\n", what);
}

// the flags as a bit set, bit i = flag i, and 16 on top so that a returned 0 cannot pass for "all false"
template <class... Cs>
static int bits_of(Cs... cs)
{
    int i = 0, bits = 16;
    for (bool c : {bool(cs())...}) bits |= (c ? 1 : 0) << i++;
    return bits;
}

static void check_pick()
{
    for (int f = 0; f < 16; f++) {
        const bool b0 = f & 1, b1 = f & 2, b2 = f & 4, b3 = f & 8;
        int calls = 0;
        auto fn = [&](auto... cs) {
            static_assert((std::is_same<decltype(cs), std::bool_constant<decltype(cs)::value>>::value && ...), "pick hands over bool constants");
            calls++;
            return bits_of(cs...);
        };
        if (f < 2) cases++, expect(pick(fn, b0) == (16 | (f & 1)) && calls == 1, "pick: one flag");
        calls = 0;
        if (f < 4) cases++, expect(pick(fn, b0, b1) == (16 | (f & 3)) && calls == 1, "pick: two flags");
        calls = 0;
        if (f < 8) cases++, expect(pick(fn, b0, b1, b2) == (16 | (f & 7)) && calls == 1, "pick: three flags");
        calls = 0;
        cases++, expect(pick(fn, b0, b1, b2, b3) == (16 | f) && calls == 1, "pick: four flags");
    }
    // a fn that returns nothing, and a template argument made from the constant the way the launch sites do
    int seen = -1;
    pick([&](auto A, auto B) { seen = std::integral_constant<int, (A() ? 2 : 0) + (B() ? 1 : 0)>::value; }, true, false);
    cases++, expect(seen == 2, "pick: void fn");
    auto half = [](auto A) { return A() ? 1.5 : 0.5; };
    static_assert(std::is_same<decltype(pick(half, true)), double>::value, "pick returns what fn returns");
    cases++, expect(pick(half, true) == 1.5 && pick(half, false) == 0.5, "pick: a double comes back");
}

template <int... Vs>
static void check_pick_int(int last, int largest)
{
    auto run = [&](int v, int want) {
        int calls = 0;
        const long long got = pick_int<Vs...>(v, [&](auto V) {
            static_assert(std::is_same<decltype(V), std::integral_constant<int, decltype(V)::value>>::value, "pick_int hands over an int constant");
            calls++;
            return 1000LL + V();
        });
        cases++, expect(got == 1000LL + want && calls == 1, "pick_int: wrong constant, wrong return value or not exactly one call");
    };
    for (int v : {Vs...}) run(v, v);
    for (int v : {-1, INT_MIN, 0, largest + 1, INT_MAX}) {
        bool listed = false;
        for (int l : {Vs...}) listed = listed || l == v;
        if (!listed) run(v, last);
    }
}

static void check_launch_grid()
{
    for (int n : {0, 1, 2, 255, 256, 257, 511, 512, 513, 64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 256 * 2048 - 1, 256 * 2048, 256 * 2048 + 1, 256 * 4096 + 1,
                  INT_MAX / 2, INT_MAX - 255}) {
        int g = (n + 255) / 256; // gather / scatter / the orthogonalize update: capped, not floored
        if (g > 2048) g = 2048;
        cases++, expect(launch_grid(n, 256, 2048) == g, "launch_grid: cap 2048");
        cases++, expect(launch_grid(n, 256, 2048, 1) == (g < 1 ? 1 : g), "launch_grid: cap 2048, floor 1");
        cases++, expect(launch_grid(n, 256, 4096) == std::min((n + 255) / 256, 4096), "launch_grid: cap 4096");
        int h = (n / 2 + 255) / 256; // AXPY and the float rounding: pairs
        h = h < 1 ? 1 : (h > 2048 ? 2048 : h);
        cases++, expect(launch_grid(n / 2, 256, 2048, 1) == h, "launch_grid: pairs");
        cases++, expect(launch_grid(n, 64, 4096, 1) == std::max(1, std::min((n + 63) / 64, 4096)), "launch_grid: 64 per workgroup");
    }
    cases++, expect(launch_grid(INT_MAX, 256, 2048) == 2048 && launch_grid(INT_MAX, 1, INT_MAX) == INT_MAX, "launch_grid: INT_MAX items");
}

int main()
{
    check_pick();
    check_pick_int<4, 2>(2, 4);
    check_pick_int<4, 16, 8>(8, 16);
    check_pick_int<16, 8>(8, 16);
    check_pick_int<1, 2, 3, 4, 5, 6, 7, 8>(8, 8);
    check_pick_int<4096, 16384, 0>(0, 16384);
    check_pick_int<22, 23, 27, 24>(24, 27);
    check_pick_int<7>(7, 7);
    check_launch_grid();
    printf("dispatch cases %d\nbad %d\n", cases, bad);
    return bad != 0;
}
