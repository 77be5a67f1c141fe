"""CPU: the oracle side of the key-width tests (tests/wide_keys.py holds the constants, tests/test_gpu_wide_keys.py the device side).

1. The condition that lets the GPU equalities fail: at every (seed, agent count, episode, step) point the GPU file compares, the
   oracle's output under the true key and under each corrupted key (low seed word only, low id word only, no carry into the high id
   word) differ in at least a quarter of the affected entries.  A condition, not a measurement: a point that misses it is moved,
   the bound is not.
2. The inverse-CDF cases leave out rows whose uniform lies within 1e-4 of a boundary of the uniform mixture (0.2 .. 0.8), at most 1
   row in 50 of a case -- one launch, or the launches of one collect: checked here on the oracle's uniforms at the same points.
3. Known answers at full-width keys: the NumPy restatements (oracle/philox.py, oracle/actor_oracle.policy_uniforms,
   tests/qmix_ref.explore_words, tests/actor_rows_ref.rows_uniforms) against a Philox written here on Python integers, for ids given
   as Python ints, int64 arrays and uint64 arrays, and the rows stream at draw 0xFFFFFFFF.
"""
import numpy as np
import pytest

from oracle import actor_oracle as AO
from oracle import philox
from tests import actor_rows_ref as RR
from tests import qmix_ref as QR
from tests import wide_keys as WK

M = 0xFFFFFFFF
PINNED_RESET = [0x1f36c476, 0xa4c7c620, 0x2eca13aa, 0x940fe33d]     # seed SEEDS[0], env 2^40 + 12345, episode 7, call 3
PINNED_ROWS_U = 0.7863150835037231                                   # seed SEEDS[1], row 2^63 + 11, draw 0xFFFFFFFF
POINTS = WK.oracle_points()


def _philox_int(c, seed):
    """Philox4x32-10 on Python integers (Salmon et al., SC'11): counter [4], key = the two words of the seed."""
    c, k0, k1 = list(c), seed & M, (seed >> 32) & M
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M, (p0 >> 32) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c


def _fmix_int(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M
    return h ^ (h >> 16)


def _word_int(a, episode, step):
    return _fmix_int(((a ^ step) + episode * 0x9E3779B1) & M)


def _block_int(seed, gid, c2, c3):
    return _philox_int([gid & M, (gid >> 32) & M, c2, c3], seed)


def test_the_integer_philox_meets_the_random123_vectors():
    assert _philox_int([0, 0, 0, 0], 0) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox_int([M, M, M, M], (M << 32) | M) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _philox_int([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0x299f31d0 << 32) | 0xa4093822) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_constants_sit_where_the_docstring_says():
    i = WK.ids()
    assert [int(x) >> 32 for x in i[[0, 18, 19, 36]]] == [4, 4, 5, 5]
    assert int(i[18]) & M == M and int(i[19]) & M == 0 and WK.SHARD_BASE == 5 << 32 and len(i) == WK.E == 37
    assert WK.SEEDS[0] >> 63 == 1 and WK.SEEDS[0] & M not in (0, WK.SEEDS[0] >> 32) and WK.SEEDS[1] & M == 0
    names = [c[0] for c in WK.corruptions(WK.SEEDS[0], i)]
    assert names == ["seed_lo", "id_lo", "no_carry"]
    for name, seed, cid, affected in WK.corruptions(WK.SEEDS[0], i):
        assert int(affected.sum()) == (18 if name == "no_carry" else 37)
        assert (seed, cid.tolist()) != (WK.SEEDS[0], i.tolist())
    assert np.array_equal(affected, np.arange(37) >= WK.CARRY)
    # a base with bit 63 set and no carry in the batch: two corruptions remain
    assert [c[0] for c in WK.corruptions(WK.SEEDS[1], WK.ids(WK.ROWS_BASE_HIGH))] == ["seed_lo", "id_lo"]


@pytest.mark.parametrize("seed", WK.SEEDS)
def test_every_corruption_changes_a_quarter_of_the_affected_entries(seed):
    worst = {}
    for label, base, fn in POINTS:
        i = WK.ids(base)
        true = fn(seed, i)
        for name, cseed, cids, affected in WK.corruptions(seed, i):
            frac = WK.different_fraction(true, fn(cseed, cids), affected)
            worst[name] = min(worst.get(name, 1.0), frac)
            assert frac >= WK.MIN_DIFFERENT, (label, name, frac)
    assert set(worst) == {"seed_lo", "id_lo", "no_carry"}


@pytest.mark.parametrize("seed", WK.SEEDS)
def test_shard_base_is_distinguishable_too(seed):
    """The shard [19, 37) runs under a base whose low word is zero: dropping the high id word or the high seed word still shows."""
    for label, base, fn in POINTS:
        if base != WK.BASE:
            continue
        i = WK.ids(WK.SHARD_BASE, WK.E - WK.CARRY)
        true = fn(seed, i)
        assert np.array_equal(true, fn(seed, WK.ids())[WK.CARRY:]), label        # (the oracle itself is shard invariant)
        for name, cseed, cids, affected in WK.corruptions(seed, i):
            assert WK.different_fraction(true, fn(cseed, cids), affected) >= WK.MIN_DIFFERENT, (label, name)


@pytest.mark.parametrize("seed", WK.SEEDS)
def test_few_uniforms_lie_near_a_boundary_of_the_uniform_mixture(seed):
    bounds = np.array([0.2, 0.4, 0.6, 0.8])

    def near(u):
        return np.abs(u.astype(np.float64).reshape(-1, 1) - bounds).min(axis=1) < 1e-4

    for n in (1,) + tuple(sorted(set(WK.PARTICLE_N) | set(WK.CHECKERS_N))):
        # a collect is one case: its launches together (every (episode, step) point a collect can reach: more than its 8 ticks)
        marks = [near(AO.policy_uniforms(seed, WK.ids(), ep, st, n)) for ep in WK.EPISODES for st in WK.STEPS]
        assert sum(int(m.sum()) for m in marks) * 50 <= sum(m.size for m in marks), n
        # act() is one launch a case: the first two ticks after reset()
        for st in (0, 1):
            m = near(AO.policy_uniforms(seed, WK.ids(), 1, st, n))
            assert n == 1 or m.sum() * 50 <= m.size, (n, st, int(m.sum()))
    for base in WK.ROWS_BASES:
        for draw in WK.ROWS_DRAWS + (0,):
            m = near(RR.rows_uniforms(seed, WK.E, draw, base))
            assert m.sum() * 50 <= m.size, (hex(base), hex(draw), int(m.sum()))


# ---- known answers at full-width keys ------------------------------------------------------------------------------------------------
GIDS = (WK.BASE + 18, WK.BASE + 19, 1 << 63, (1 << 64) - 1)


def _forms(gids):
    """the same ids as a uint64 array, as an int64 array (two's complement) and one by one as Python ints"""
    u = np.array(gids, dtype=np.uint64)
    yield "uint64", lambda f: f(u)
    yield "int64", lambda f: f(u.view(np.int64))
    yield "int", lambda f: [np.concatenate([np.atleast_1d(x) for x in col]) for col in zip(*[f(g) for g in gids])]


@pytest.mark.parametrize("seed", WK.SEEDS + (0, (1 << 64) - 1))
def test_oracle_blocks_accept_64_bit_seeds_and_ids_in_every_form(seed):
    for episode, call in ((0, 0), (1, 2), (M, 1)):
        want_reset = [_block_int(seed, g, episode, 0x80000000 | call) for g in GIDS]
        want_block = [_block_int(seed, g, 0, call << 24) for g in GIDS]
        for form, run in _forms(GIDS):
            got = run(lambda ids: philox.reset_words(seed, ids, episode, call))
            assert [[int(w[k]) for w in got] for k in range(4)] == want_reset, (form, episode, call)
            got = run(lambda ids: philox.action_block(seed, ids, call))
            assert [[int(w[k]) for w in got] for k in range(4)] == want_block, (form, call)
        for step in (0, (1 << 24) - 1):
            got = philox.action_words(seed, np.array(GIDS, dtype=np.uint64), episode, step, call)
            assert [[int(w[k]) for w in got] for k in range(4)] == [[_word_int(x, episode, step) for x in b] for b in want_block]


@pytest.mark.parametrize("seed", WK.SEEDS)
def test_stream_restatements_at_full_width_keys(seed):
    i = WK.ids()
    for ids_form in (i, i.view(np.int64), np.arange(WK.E) + WK.BASE):
        assert np.asarray(ids_form).dtype in (np.uint64, np.int64)
        for n, ep, st in ((2, 1, 0), (5, 3, 2)):
            acts = philox.expected_actions(seed, ids_form, ep, st, n)
            uni = AO.policy_uniforms(seed, ids_form, ep, st, n)
            we, wa = QR.explore_words(seed, ids_form, ep, st, n)
            for e in (0, 18, 19, 36):
                g = int(i[e])
                for a in range(n):
                    blk = _block_int(seed, g, 0, (a // 4) << 24)
                    assert int(acts[e, a]) == (_word_int(blk[a % 4], ep, st) * 5) >> 32
                    blk = _block_int(seed, g, 0, 0x40000000 | ((a // 4) << 24))
                    assert uni[e, a] == np.float32((_word_int(blk[a % 4], ep, st) + 0.5) / 4294967296.0)
                    blk = _block_int(seed, g, 0, 0x20000000 | ((a >> 1) << 24))
                    assert (int(we[e, a]), int(wa[e, a])) == (_word_int(blk[2 * (a & 1)], ep, st), _word_int(blk[2 * (a & 1) + 1], ep, st))
    for base in WK.ROWS_BASES:
        for draw in WK.ROWS_DRAWS:
            u = RR.rows_uniforms(seed, WK.E, draw, base)
            for r in (0, 18, 19, 36):
                w = _block_int(seed, (base + r) & ((1 << 64) - 1), draw, 0x10000000)[0]
                assert u[r] == np.float32((w + 0.5) / 4294967296.0), (hex(base), hex(draw), r)


def test_pinned_words():
    """Literal words (from the integer Philox above; tests/test_philox_header.py holds csrc/philox.h to the same oracle)."""
    got = [int(w) for w in philox.reset_words(WK.SEEDS[0], np.uint64((1 << 40) + 12345), 7, 3)]
    assert got == _block_int(WK.SEEDS[0], (1 << 40) + 12345, 7, 0x80000003)
    assert got == PINNED_RESET, [hex(x) for x in got]
    assert float(RR.rows_uniforms(WK.SEEDS[1], 1, WK.DRAW_LAST, WK.ROWS_BASE_HIGH)[0]) == PINNED_ROWS_U


