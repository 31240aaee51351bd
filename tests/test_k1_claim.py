"""CPU: how a K1 launch hands its work items to its persistent waves (nanomod_amd/csrc/item_claim.hpp through
nmod_item_claim_plan).  Every item of [0, items) must be handed out exactly once for any (items, waves): by the strided rounds,
by the waves' own chunks and by the chunks drawn as tickets, in whatever order the waves draw them."""
import ctypes as C

import numpy as np
import pytest

WAVES = (1, 4, 4096)


def _items_for(waves):
    return sorted({0, 1, 3, max(waves - 1, 0), waves, waves + 1, 2 * waves + 5, 281 * 4096, 2 ** 31 // 8})


CASES = [(items, waves) for waves in WAVES for items in _items_for(waves)]


def plan_of(items, waves, flags=0):
    import nanomod_amd._lib as L
    out = (C.c_int64 * 4)()
    assert L.load().nmod_item_claim_plan(items, waves, flags, out) == 0
    rounds, first, chunk, dynamic = (int(v) for v in out)
    return rounds, first, chunk, dynamic


class Walk:
    """One wave's walk, the way ItemWalk (item_claim.hpp) does it: `rounds` strided items, the wave's own chunk, then one chunk
    per ticket; the ticket of the chunk after the one being entered is drawn on entering it.  counter: a one-element list."""

    def __init__(self, plan, items, wave, waves, counter):
        self.rounds, self.first, self.chunk, self.dynamic = plan
        self.items, self.waves, self.counter = items, waves, counter
        self.base = self.first + waves * self.chunk
        self.pend = self.first + wave * self.chunk
        if self.rounds > 0:
            self.step, self.left, self.it = waves, self.rounds - 1, wave
        else:
            self.it = self._enter()

    def _enter(self):
        it = self.pend
        self.step, self.left = 1, self.chunk - 1
        self.pend = 2 ** 32 - 1
        if self.dynamic:
            self.pend = self.base + self.counter[0] * self.chunk
            self.counter[0] += 1
        return it

    def take(self):
        """the wave's next item, or None when it is done (an item beyond the end ends the walk)"""
        if self.it >= self.items:
            return None
        it = self.it
        if self.left > 0:
            self.left -= 1
            self.it = it + self.step
        else:
            self.it = self._enter()
        return it


def test_rejects_bad_arguments():
    import nanomod_amd._lib as L
    lib = L.load()
    out = (C.c_int64 * 4)()
    assert lib.nmod_item_claim_plan(-1, 4, 0, out) == -1
    assert lib.nmod_item_claim_plan(10, 0, 0, out) == -1
    assert lib.nmod_item_claim_plan(10, 4, 0, None) == -1
    assert L.FLAG_K1_STATIC_ITEMS == 128


@pytest.mark.parametrize('items,waves', CASES)
def test_plan_hands_out_every_item_once(items, waves):
    rounds, first, chunk, dynamic = plan_of(items, waves)
    # the strided part: items w + k * waves, w < waves, k < rounds, is [0, rounds * waves) — every value once (w = item mod waves,
    # k = item div waves) — and must end where the chunks begin
    assert rounds >= 0 and first == rounds * waves and first <= items and 1 <= chunk <= 4
    # at most 3/8 of the equal share is fixed, so that the first wave to finish still finds work to draw
    assert 8 * rounds <= 3 * (items // waves)
    # chunks: consecutive intervals of `chunk` items from `first` on cover [first, items) once; tickets are needed iff the waves'
    # own chunks do not reach the end
    nchunks = -(-(items - first) // chunk)
    assert first + nchunks * chunk >= items and (nchunks == 0 or first + (nchunks - 1) * chunk < items)
    assert dynamic == (1 if nchunks > waves else 0)
    if items <= 2 * 10 ** 6:
        seen = np.zeros(items, np.int32)
        if rounds:
            strided = np.add.outer(np.arange(waves, dtype=np.int64), np.arange(rounds, dtype=np.int64) * waves).ravel()
            np.add.at(seen, strided, 1)
        starts = first + np.arange(nchunks, dtype=np.int64) * chunk
        for j in range(chunk):
            idx = starts + j
            np.add.at(seen, idx[idx < items], 1)
        assert np.array_equal(seen, np.ones(items, np.int32))


@pytest.mark.parametrize('items,waves', CASES)
def test_strided_flag_is_the_strided_walk(items, waves):
    import nanomod_amd._lib as L
    rounds, first, chunk, dynamic = plan_of(items, waves, L.FLAG_K1_STATIC_ITEMS)
    assert (rounds, first, chunk, dynamic) == (-(-items // waves), items, 1, 0)
    if items <= 20000:
        for w in range(min(waves, 64)):
            wk = Walk((rounds, first, chunk, dynamic), items, w, waves, [0])
            got = []
            while (it := wk.take()) is not None:
                got.append(it)
            assert got == list(range(w, items, waves))


@pytest.mark.parametrize('items,waves', [c for c in CASES if c[0] <= 20000] + [(281 * 64, 64), (97 * 16 + 3, 16), (12 * 4096 + 7, 4096)])
def test_walks_in_any_order_cover_the_items(items, waves):
    plan = plan_of(items, waves)
    rounds = plan[0]
    rng = np.random.default_rng(items * 31 + waves)
    for order in ('sequential', 'random', 'oldest_first'):
        counter = [0]
        walks = [Walk(plan, items, w, waves, counter) for w in range(waves)]
        seen = np.zeros(items, np.int32)
        taken = [[] for _ in range(waves)]
        live = list(range(waves))
        while live:
            if order == 'sequential':
                k = 0
            elif order == 'random':
                k = int(rng.integers(len(live)))
            else:
                k = 0 if rng.random() < 0.7 else int(rng.integers(len(live)))   # the oldest wave runs ahead, as on a SIMD
            w = live[k]
            it = walks[w].take()
            if it is None:
                live.pop(k)
                continue
            seen[it] += 1
            taken[w].append(it)
        assert np.array_equal(seen, np.ones(items, np.int32)), order
        # the fixed part of a wave is the strided walk's first items
        for w in range(min(waves, 64)):
            assert taken[w][:rounds] == list(range(w, items, waves))[:rounds]
        # tickets drawn past the end are bounded: a wave stops at its first chunk beyond the end, one more is in flight
        assert counter[0] <= -(-(items - plan[1]) // plan[2]) + 2 * waves


def test_headline_shape_plan():
    """4.6 M positions, four per item, 4 096 resident waves: a 281-item share keeps 105 rounds fixed and draws chunks of four"""
    items = -(-4_600_000 // 4)
    rounds, first, chunk, dynamic = plan_of(items, 4096)
    assert (rounds, chunk, dynamic) == ((items // 4096) * 3 // 8, 4, 1) and first == rounds * 4096
