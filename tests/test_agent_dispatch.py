"""CPU: the agent-count dispatcher of the matrix translation units (csrc/agent_dispatch.h).

The header needs no HIP, so a small program with its own main() -- written here, compiled with the host compiler under
AddressSanitizer and UBSan and run directly -- walks n = -1 .. 12 through the three lists the sources use and prints, per (list, n),
whether a hit was reported, how often the callable ran, the N it was given and what the dispatcher returned.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cm3_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LISTS = {"all": list(range(1, 11)), "dense": [1, 2, 4, 8], "padded": [3, 5, 6, 7, 9, 10]}

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "agent_dispatch.h"
template <int N> struct Layout { static constexpr int kTotal = 1000 + 7 * N; };   // (N as a template argument, as the sources use it)
template <typename D> static void walk(const char *name, D dispatch) {
  for (int n = -1; n <= 12; ++n) {
    int calls = 0, seen = -99;
    bool hit = n & 1;                                  // (stale on purpose: the dispatcher must set it either way)
    const long r = dispatch(n, hit, [&](auto N) { ++calls; seen = decltype(N)::value; return 5L + Layout<decltype(N)::value>::kTotal; });
    printf("%s %d %d %d %d %ld\n", name, n, (int)hit, calls, seen, r);
  }
}
int main() {
  walk("all", [](int n, bool &hit, auto f) { return cm3::agent_dispatch_1_to_10(n, hit, f); });
  walk("dense", [](int n, bool &hit, auto f) { return cm3::agent_dispatch<1, 2, 4, 8>(n, hit, f); });
  walk("padded", [](int n, bool &hit, auto f) { return cm3::agent_dispatch<3, 5, 6, 7, 9, 10>(n, hit, f); });
  bool hit = false;
  const auto bytes = cm3::agent_dispatch<1, 2, 4, 8>(4, hit, [](auto N) { return (size_t)Layout<decltype(N)::value>::kTotal; });
  static_assert(std::is_same<decltype(bytes), const size_t>::value, "the callable's type comes back");
  printf("size_t %d %zu\n", (int)hit, bytes);
  return 0;
}
"""


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("agent_dispatch")
    src, exe = tmp / "dispatch.cpp", tmp / "dispatch"
    src.write_text(PROGRAM)
    san = ["-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe)]
    if shutil.which("g++"):
        subprocess.check_call(["g++"] + san + [str(src)])
    elif os.path.exists(HIPCC):
        subprocess.check_call([HIPCC, "-x", "c++"] + san + [str(src)])      # host only: the header holds no device code
    else:
        pytest.skip("no host C++ compiler")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr              # (a sanitizer report ends the program with a non-zero status)
    return [line.split() for line in out.stdout.splitlines()]


@pytest.mark.parametrize("name", sorted(LISTS))
def test_callable_runs_once_for_a_listed_count_and_never_for_another(walked, name):
    rows = [tuple(map(int, v[1:])) for v in walked if v[0] == name]
    assert [r[0] for r in rows] == list(range(-1, 13))
    for n, hit, calls, seen, result in rows:
        if n in LISTS[name]:
            assert (hit, calls, seen, result) == (1, 1, n, 5 + 1000 + 7 * n), (name, n)     # N == n, the return value passed through
        else:
            assert (hit, calls, seen, result) == (0, 0, -99, 0), (name, n)                  # a miss is reported, nothing ran


def test_return_type_is_the_callables(walked):
    assert walked[-1] == ["size_t", "1", str(1000 + 7 * 4)]


def test_header_is_plain_cxx_and_holds_no_type_erasure():
    text = open(os.path.join(CSRC, "agent_dispatch.h")).read()
    for word in ("hip/", "__device__", "std::function", "virtual", "new ", "malloc"):
        assert word not in text, word
