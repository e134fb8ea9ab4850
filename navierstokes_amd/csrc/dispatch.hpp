// dispatch.hpp — runtime state into template arguments, once: every launch site ties a handle's flag to its kernel's template
// parameter through these and writes its launch line once.  Host only (no HIP header): tools/dispatch_check.cpp tests it with g++.
#pragma once
#include <type_traits>

// pick(fn, b0, b1, ...): fn(std::bool_constant<B0>{}, std::bool_constant<B1>{}, ...) with the flags' compile-time twins; fn's value
template <bool... Bs, class Fn>
inline auto pick(Fn&& fn)
{
    return fn(std::bool_constant<Bs>{}...);
}
template <bool... Bs, class Fn, class... R>
inline auto pick(Fn&& fn, bool b, R... r)
{
    return b ? pick<Bs..., true>(fn, r...) : pick<Bs..., false>(fn, r...);
}

// pick_int<V0, ..., Vlast>(v, fn): fn(std::integral_constant<int, V>{}) for the listed V that equals v, else for Vlast (a ladder's
// `default:`); a site that refuses an unlisted value checks its range in front of the call
template <int V0, int... Vs, class Fn>
inline auto pick_int(int v, Fn&& fn)
{
    if constexpr (sizeof...(Vs) == 0) return fn(std::integral_constant<int, V0>{});
    else return v == V0 ? fn(std::integral_constant<int, V0>{}) : pick_int<Vs...>(v, fn);
}

// workgroups of per_wg items over `work` items: at most cap, at least floor
inline int launch_grid(long long work, int per_wg, int cap, int floor = 0)
{
    long long g = (work + per_wg - 1) / per_wg;
    if (g > cap) g = cap;
    if (g < floor) g = floor;
    return (int)g;
}
