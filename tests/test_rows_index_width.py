"""CPU: the rules by which the launchers of csrc/batch.hip choose 32-bit or 64-bit index arithmetic (csrc/rows_index_width.h),
checked without a GPU.

The rules are plain C++17 in one header that batch.hip includes and calls.  A small program with its own main(), written here and
compiled with the host compiler under AddressSanitizer and UBSan, includes the header alone and answers queries; nothing is loaded
into Python.  Two things are asserted for each of the five rules:

  * the exact boundary: the largest argument that is still narrow, and the next one, against a restatement by hand.  The numbers
    below are written out from the source (workgroups of 256 lanes; at most 4096 workgroups for k_rows_copy, 2048 for k_rows_tile,
    16384 for k_transitions_gather; four units / pieces per lane in the Checkers kernels and in k_transitions_gather; 16-byte pieces in
    the pack), they are not imported from it -- a constant that moves in the header without its rule moving fails here;
  * the safety property the rule exists for: at every narrow choice the largest value a lane forms in the index type I fits 32
    bits.  Per kernel (read from the kernels' index code):
      k_rows_copy / k_rows_tile    g runs from blockIdx * 256 + lane in steps of stride = blocks * 256 while g < total: the largest
                                   value formed is the last unit index plus one stride, (total - 1) + stride; a lane that starts past
                                   the end holds at most stride - 1
      k_ck_transitions_gather      g = (block of the column) * 1024 + lane + k * 256, k < 4: at most ceil(total / 1024) * 1024 - 1;
                                   every other value (row, tick, env, unit) is a quotient or remainder of a g clamped to total - 1
      k_ck_transitions_pack        pieces of 16 bytes of a ring column of `most` bytes: the piece index is at most
                                   ceil(pieces / 1024) * 1024 - 1 with pieces <= most / 16 + 2; byte offsets are formed for live
                                   (clamped) pieces only, up to the end of the last piece: < most + 16, and `first + 16` in the range
                                   test: < most + 32; ring row -> transition forms row + (ring_size - ring_start) < 2 * ring_size
      k_transitions_gather         the 32-bit casts apply to unit indices clamped below total; a lane's own counter reaches
                                   (total - 1) + 4 * stride (the counter itself is 64-bit in both forms: the rule is the stricter)
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cm3_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "rows_index_width.h"
// reads queries `rule a b` (unsigned 64-bit), prints `narrow blocks` (blocks 0 where the rule has no block cap)
int main() {
  char rule[16];
  unsigned long long a, b;
  while (scanf("%15s %llu %llu", rule, &a, &b) == 3) {
    int narrow = -1;
    size_t blocks = 0;
    if (!strcmp(rule, "copy")) { blocks = cm3::rows_copy_blocks((size_t)a); narrow = cm3::rows_stride_index_narrow((size_t)a, blocks); }
    else if (!strcmp(rule, "tile")) { blocks = cm3::rows_tile_blocks((size_t)a); narrow = cm3::rows_stride_index_narrow((size_t)a, blocks); }
    else if (!strcmp(rule, "ckg")) narrow = cm3::ck_gather_index_narrow((size_t)a);
    else if (!strcmp(rule, "pack")) narrow = cm3::ck_pack_index_narrow((size_t)a, (size_t)b);
    else if (!strcmp(rule, "trans")) { blocks = cm3::trans_blocks_for((size_t)a); narrow = cm3::trans_index_small((size_t)a, blocks * 256); }
    else return 2;
    printf("%d %llu\n", narrow, (unsigned long long)blocks);
  }
  return 0;
}
"""

TWO32 = 1 << 32


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask([(rule, a, b), ...]) -> [(narrow, blocks), ...] as the header answers"""
    tmp = tmp_path_factory.mktemp("rows_index_width")
    src, exe = tmp / "width.cpp", tmp / "width"
    src.write_text(PROGRAM)
    san = ["-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe)]
    if shutil.which("g++"):
        subprocess.check_call(["g++"] + san + [str(src)])
    elif os.path.exists(HIPCC):
        subprocess.check_call([HIPCC, "-x", "c++"] + san + [str(src)])      # host only: the header holds no device code
    else:
        pytest.skip("no host C++ compiler")

    def ask(queries):
        text = "".join("%s %d %d\n" % q for q in queries)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr          # (a sanitizer report ends the program with a non-zero status)
        rows = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
        assert len(rows) == len(queries)
        return [(bool(n), b) for n, b in rows]
    return ask


# ---- the restatement by hand: (blocks, narrow, largest value a lane forms in I) per rule -------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def _stride_loop(most, cap, at_least_one):
    blocks = min(_ceil(most, 256), cap)
    if at_least_one:
        blocks = max(blocks, 1)
    stride = blocks * 256
    return blocks, most + stride < TWO32, max(most - 1 + stride, stride - 1)


def hand_copy(most, _=0):
    return _stride_loop(most, 4096, True)


def hand_tile(most, _=0):
    return _stride_loop(most, 2048, False)


def hand_ckg(most, _=0):
    return 0, most + 4 * 256 < TWO32, _ceil(most, 1024) * 1024 - 1


def hand_pack(most, size):
    pieces = most // 16 + 2                              # both ranges of a wrapped chunk may start and end inside a piece
    largest = max(_ceil(pieces, 1024) * 1024 - 1,        # a piece index
                  most + 32,                             # a byte offset: the end of the piece behind the last one
                  2 * size - 1)                          # ring row + (ring_size - ring_start)
    return 0, most + 32 * 4 * 256 < TWO32 and 2 * size < TWO32, largest


def hand_trans(units, _=0):
    blocks = max(min(_ceil(units, 4 * 256), 16384), 1)
    stride = blocks * 256
    return blocks, units + 4 * stride < TWO32, max(units - 1 + 4 * stride, 4 * stride - 1)


HAND = {"copy": hand_copy, "tile": hand_tile, "ckg": hand_ckg, "pack": hand_pack, "trans": hand_trans}
# the largest first argument that is still narrow, written out (second argument: a ring of one row per byte at most -- never the limit)
LAST_NARROW = {"copy": TWO32 - 4096 * 256 - 1, "tile": TWO32 - 2048 * 256 - 1, "ckg": TWO32 - 1024 - 1,
               "pack": TWO32 - 32 * 1024 - 1, "trans": TWO32 - 4 * 16384 * 256 - 1}


def _check(ask, queries):
    got = ask(queries)
    for (rule, a, b), (narrow, blocks) in zip(queries, got):
        h_blocks, h_narrow, largest = HAND[rule](a, b)
        assert narrow == h_narrow, (rule, a, b)
        assert blocks == h_blocks, (rule, a, b)
        if narrow:
            assert largest < TWO32, (rule, a, b, largest)      # what the rule is for
    return got


@pytest.mark.parametrize("rule", sorted(HAND))
def test_exact_boundary_and_safety_at_it(ask, rule):
    last = LAST_NARROW[rule]
    size = 1000 if rule == "pack" else 0
    got = _check(ask, [(rule, last - 1, size), (rule, last, size), (rule, last + 1, size), (rule, last + 2, size),
                       (rule, 1, size), (rule, 255, size), (rule, 256, size), (rule, 257, size), (rule, TWO32, size),
                       (rule, TWO32 * 5 + 3, size)])
    assert [n for n, _ in got] == [True, True, False, False, True, True, True, True, False, False]


def test_pack_ring_size_arm_on_its_own(ask):
    """2 * ring_size < 2^32 with a column that is far from the byte limit (one byte per row: the done column alone)"""
    last = (1 << 31) - 1
    got = _check(ask, [("pack", last, last - 1), ("pack", last, last), ("pack", last + 1, last + 1), ("pack", 16, last + 1),
                       ("pack", 16, TWO32), ("pack", LAST_NARROW["pack"], last), ("pack", LAST_NARROW["pack"] + 1, last)])
    assert [n for n, _ in got] == [True, True, False, False, False, True, False]


@pytest.mark.parametrize("rule", sorted(HAND))
def test_safety_at_random_large_arguments(ask, rule):
    rng = random.Random(len(rule) * 7919 + 5)
    last = LAST_NARROW[rule]
    queries = []
    for k in range(1000):
        kind = k % 4
        if kind == 0:
            a = last - rng.randrange(0, 1 << 22)                 # just below the boundary
        elif kind == 1:
            a = last + 1 + rng.randrange(0, 1 << 22)             # just above
        elif kind == 2:
            a = rng.randrange(1 << 28, TWO32 + (1 << 28))        # anywhere large
        else:
            a = rng.randrange(1, 1 << 21)                        # below every block cap: the uncapped grid sizes
        b = 0
        if rule == "pack":
            b = rng.choice([a, max(a // 707, 1), (1 << 31) - rng.randrange(0, 3), (1 << 31) + rng.randrange(0, 1 << 20)])
        queries.append((rule, a, b))
    got = _check(ask, queries)
    assert {n for n, _ in got} == {True, False}
