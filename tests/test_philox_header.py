"""CPU: csrc/philox.h itself -- the header is __host__ __device__, so a small program with its own main(), written here, compiled with
the host compiler under AddressSanitizer and UBSan and run directly (it is never loaded into Python), prints philox4x32_10,
action_block, action_words, reset_words, fmix32, rand5 and u01 over a table of full-width inputs; every word must equal what
oracle/philox.py gives, and the three Random123 known answers anchor the header itself, not only its NumPy restatement.

The table: both seeds of tests/wide_keys.py plus 0 and 2^64 - 1; env ids BASE + 18, BASE + 19 (the two sides of the carry out of the
low id word), 2^63 and 2^64 - 1; episodes 0, 1 and 2^32 - 1; steps 0 and 2^24 - 1; calls 0 .. 2.  (The gfx950-only three-input xor of
philox4x32_10 exists in the device compile only: tests/test_gpu_wide_keys.py holds that branch to the same oracle.)
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import philox
from tests import wide_keys as WK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cm3_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SEEDS = WK.SEEDS + (0, (1 << 64) - 1)
ENVS = (WK.BASE + 18, WK.BASE + 19, 1 << 63, (1 << 64) - 1)
EPISODES = (0, 1, 0xFFFFFFFF)
STEPS = (0, (1 << 24) - 1)
CALLS = (0, 1, 2)
WORDS = (0, 1, 0x33333333, 0x33333334, 0x7FFFFFFF, 0x80000000, 0xDEADBEEF, 0xFFFFFFFF)     # (0x33333334: the first word rand5 maps to 1)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def _array(name, ctype, values, suffix):
    return "static const %s %s[] = {%s};\n" % (ctype, name, ", ".join("0x%x%s" % (v, suffix) for v in values))


PROGRAM = (r"""
#include <stdint.h>
#include <stdio.h>
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#include "philox.h"
using namespace cm3;
"""
           + _array("kSeeds", "uint64_t", SEEDS, "ull") + _array("kEnvs", "uint64_t", ENVS, "ull")
           + _array("kEpisodes", "uint32_t", EPISODES, "u") + _array("kSteps", "uint32_t", STEPS, "u")
           + _array("kCalls", "uint32_t", CALLS, "u") + _array("kWords", "uint32_t", WORDS, "u")
           + "static const uint32_t kKat[][6] = {%s};\n" % ", ".join(
               "{%s}" % ", ".join("0x%xu" % v for v in c + k) for c, k, _ in KAT)
           + r"""
template <typename T, size_t N> constexpr size_t count(const T (&)[N]) { return N; }
static void put(const char *tag, const u32x4 &w) { printf("%s %08x %08x %08x %08x\n", tag, w.x, w.y, w.z, w.w); }
int main() {
  char tag[128];
  for (size_t i = 0; i < count(kKat); ++i) {
    u32x4 c;
    c.x = kKat[i][0]; c.y = kKat[i][1]; c.z = kKat[i][2]; c.w = kKat[i][3];
    snprintf(tag, sizeof tag, "kat %zu", i);
    put(tag, philox4x32_10(c, kKat[i][4], kKat[i][5]));
  }
  for (size_t s = 0; s < count(kSeeds); ++s)
    for (size_t e = 0; e < count(kEnvs); ++e)
      for (size_t c = 0; c < count(kCalls); ++c) {
        snprintf(tag, sizeof tag, "block %zu %zu %zu", s, e, c);
        put(tag, action_block(kSeeds[s], kEnvs[e], kCalls[c]));
        for (size_t p = 0; p < count(kEpisodes); ++p) {
          snprintf(tag, sizeof tag, "reset %zu %zu %zu %zu", s, e, c, p);
          put(tag, reset_words(kSeeds[s], kEnvs[e], kEpisodes[p], kCalls[c]));
          // (the raw block over the same counter: philox4x32_10 with the key words split by hand)
          u32x4 ctr;
          ctr.x = (uint32_t)kEnvs[e]; ctr.y = (uint32_t)(kEnvs[e] >> 32); ctr.z = kEpisodes[p]; ctr.w = kPurposeReset | kCalls[c];
          snprintf(tag, sizeof tag, "raw %zu %zu %zu %zu", s, e, c, p);
          put(tag, philox4x32_10(ctr, (uint32_t)kSeeds[s], (uint32_t)(kSeeds[s] >> 32)));
          for (size_t t = 0; t < count(kSteps); ++t) {
            snprintf(tag, sizeof tag, "words %zu %zu %zu %zu %zu", s, e, c, p, t);
            put(tag, action_words(kSeeds[s], kEnvs[e], kEpisodes[p], kSteps[t], kCalls[c]));
          }
        }
      }
  for (size_t i = 0; i < count(kWords); ++i)
    printf("scalar %zu %08x %d %.17g %08x\n", i, fmix32(kWords[i]), rand5(kWords[i]), u01(kWords[i]), action_word(kWords[i], 0xFFFFFFFFu, 0x00FFFFFFu));
  return 0;
}
""")


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("philox_header")
    src, exe = tmp / "philox_host.cpp", tmp / "philox_host"
    src.write_text(PROGRAM)
    san = ["-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, "-o", str(exe)]
    if shutil.which("g++"):
        subprocess.check_call(["g++"] + san + [str(src)])
    elif os.path.exists(HIPCC):
        subprocess.check_call([HIPCC, "-x", "c++"] + san + [str(src)])      # host only: compiled as plain C++, no device pass
    else:
        pytest.skip("no host C++ compiler")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr              # (a sanitizer report ends the program with a non-zero status)
    table = {}
    for line in out.stdout.splitlines():
        v = line.split()
        n_key = {"kat": 2, "block": 4, "reset": 5, "raw": 5, "words": 6, "scalar": 2}[v[0]]
        assert tuple(v[:n_key]) not in table
        table[tuple(v[:n_key])] = v[n_key:]
    return table


def _hex(words):
    return ["%08x" % int(np.asarray(w).reshape(-1)[0]) for w in words]


def test_header_meets_the_random123_known_answers(printed):
    for i, (_, _, want) in enumerate(KAT):
        assert printed[("kat", str(i))] == ["%08x" % w for w in want], i


def test_every_printed_word_equals_the_oracle(printed):
    n = 0
    for s, seed in enumerate(SEEDS):
        for e, env in enumerate(ENVS):
            gid = np.array([env], dtype=np.uint64)
            for c, call in enumerate(CALLS):
                assert printed[("block", str(s), str(e), str(c))] == _hex(philox.action_block(seed, gid, call)), (hex(seed), hex(env), call)
                for p, ep in enumerate(EPISODES):
                    want = _hex(philox.reset_words(seed, gid, ep, call))
                    assert printed[("reset", str(s), str(e), str(c), str(p))] == want, (hex(seed), hex(env), call, ep)
                    assert printed[("raw", str(s), str(e), str(c), str(p))] == want, (hex(seed), hex(env), call, ep)
                    for t, st in enumerate(STEPS):
                        want = _hex(philox.action_words(seed, gid, ep, st, call))
                        assert printed[("words", str(s), str(e), str(c), str(p), str(t))] == want, (hex(seed), hex(env), call, ep, st)
                        n += 1
    assert n == len(SEEDS) * len(ENVS) * len(CALLS) * len(EPISODES) * len(STEPS)
    assert len(printed) == len(KAT) + len(SEEDS) * len(ENVS) * len(CALLS) * (1 + len(EPISODES) * (2 + len(STEPS))) + len(WORDS)


def test_full_width_keys_are_not_the_truncated_ones(printed):
    """The table can tell a lost word: the block of (seed, env) differs from the block of every corrupted key."""
    for s, seed in enumerate(WK.SEEDS):
        for e, env in enumerate(ENVS[:2]):
            have = printed[("block", str(s), str(e), "0")]
            gid = np.array([env], dtype=np.uint64)
            for name, cseed, cids, _ in WK.corruptions(seed, gid):
                assert have != _hex(philox.action_block(cseed, cids, 0)), name
    # the two sides of the carry differ in both id words
    assert printed[("block", "0", "0", "0")] != printed[("block", "0", "1", "0")]


def test_scalar_helpers_equal_the_oracle(printed):
    w = np.array(WORDS, dtype=np.uint32)
    fm, r5, u, aw = philox.fmix32(w), philox.rand5(w), philox.u01(w), philox.action_word(w, 0xFFFFFFFF, 0x00FFFFFF)
    for i in range(len(WORDS)):
        got = printed[("scalar", str(i))]
        assert got[0] == "%08x" % int(fm[i]) and int(got[1]) == int(r5[i]) and float(got[2]) == float(u[i]) and got[3] == "%08x" % int(aw[i]), i
    assert [int(x) for x in r5] == [0, 0, 0, 1, 2, 2, 4, 4] and 0.0 < float(u[0]) and float(u[-1]) < 1.0
