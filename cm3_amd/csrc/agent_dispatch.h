// Runtime agent count -> template argument, written once (plain C++17, no HIP: tests/test_agent_dispatch.py builds it with the host
// compiler).  agent_dispatch<1, 2, 4, 8>(n, hit, f) calls f(std::integral_constant<int, N>{}) for the N of the list that equals n,
// sets hit and returns f's value; for an n outside the list f is not called, hit is false and the result is R{} -- the caller then
// says what a miss means (fail(...) in an entry point, 0 bytes in the *_floats_for functions).  Only the listed counts are
// instantiated: the list IS the set of kernels a translation unit holds.
#pragma once
#include <type_traits>
#include <utility>

namespace cm3 {

template <int... Ns, typename F> auto agent_dispatch(int n, bool &hit, F &&f) {
  using R = std::common_type_t<decltype(f(std::integral_constant<int, Ns>{}))...>;
  R out{};
  hit = ((n == Ns ? (out = f(std::integral_constant<int, Ns>{}), true) : false) || ...);
  return out;
}

// the agent counts of the particle networks (CM3_MAX_AGENTS = 10)
template <typename F> auto agent_dispatch_1_to_10(int n, bool &hit, F &&f) {
  return agent_dispatch<1, 2, 3, 4, 5, 6, 7, 8, 9, 10>(n, hit, std::forward<F>(f));
}

}  // namespace cm3
