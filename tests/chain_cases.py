"""Constructed inputs for the parts of the chain entries (K19 nmod_read_hmm, K20 nmod_read_viterbi, K22 nmod_read_class_rows /
nmod_read_classes_step) that full tiles and one sort-pass count leave unseen, as (cs, start, scores) triples over a sorted key:
  hole_reads()        reads whose valid scores have holes of whole waves and tiles, on both sides of the two class steps (a read's
                      events, NMOD_CALLS_WAVE_MAX, for the kernel that fills the rows; its entries, NMOD_HMM_WAVE_MAX, for the chain)
  sort_pass_cases()   site tables of 255 .. 2^24 + 3 sites with a few reads, for every number of passes nmod_read_class_rows' sort takes
tests/test_chain_cases.py asserts without a GPU that the cases have the properties claimed here; tests/test_chain_forms_gpu.py runs
them.  Nothing here calls the library.

THE FILL (read_hmm.hip, rh_entries_kernel) walks the sites a read covers, c_lo .. c_hi - 1 in key order, T at a time: T = 64 for a read
of up to EVENTS_MAX events, T = 256 (four waves) beyond.  Site c_lo + k is thread k % T of tile k // T, in wave (k % T) // 64; an entry's
row is the count of valid sites in front of it: the tiles before, the lower waves of its tile (the workgroup form adds their ballot
counts from shared words) and the lower lanes of its wave.  A read whose every covered site is valid has 64 in every such word."""
import functools

import numpy as np

import hmm_ref as H
from test_site_pairs import _key

EVENTS_MAX = 2048                                    # NMOD_CALLS_WAVE_MAX: the events of a read up to which a wave fills its rows
ENTRIES_MAX = H.WAVE_MAX                             # NMOD_HMM_WAVE_MAX: the entries of a read up to which a wave runs its chain
TILE, WAVE = 256, 64                                 # the sites of a tile of the workgroup form, of one of its waves
PI, LENGTH, CALL_POST = 0.3, 30.0, 0.9               # the chain of tests/test_read_hmm_gpu.py's constructed reads
VALUES = np.array([3.0, -3.0, 2.5, -2.5, 1.0, -0.5, 0.0, 40.0, -7.5])        # that file's grid without its invalid scores
INVALID = np.array([np.nan, np.inf, -np.inf])
WALK = ('cs', 'start', 'roff', 'score', 'key')

TOP = 6200                                           # the sites: every position 0 .. TOP on cs 0 ('+') and cs 1 ('-'), every 7th on cs 2
HOLE_EVENTS = (64, 65, 128, 129, 2048, 2049, 2304, 2305, 4100)
HOLE_PATTERNS = ('a', 'b', 'c', 'd', 'e')
SPARSE_EVENTS = (2049, 3000, 6000)                   # the reads on cs 2


def case_arrays(reads, key):
    """the flat arrays of the entries from (cs, start, scores) triples"""
    roff = np.zeros(len(reads) + 1, np.int64)
    roff[1:] = np.cumsum([len(r[2]) for r in reads])
    return dict(cs=np.array([r[0] for r in reads], np.int32), start=np.array([r[1] for r in reads], np.int64), roff=roff,
                score=np.concatenate([np.asarray(r[2], np.float64) for r in reads]) if reads else np.zeros(0), key=np.asarray(key, np.int64))


def covered_valid(read, key):
    """(c_lo, valid): the index of the first site the read covers and, per covered site in key order, whether its score is valid"""
    cs, start, scores = read
    n = len(scores)
    lo = int(np.searchsorted(key, _key(cs, start), 'left'))
    hi = int(np.searchsorted(key, _key(cs, min(start + n - 1, H.POS_MASK)), 'right'))
    pos = key[lo:hi] & H.POS_MASK
    i = start + n - 1 - pos if cs & 1 else pos - start
    with np.errstate(invalid='ignore'):
        return lo, np.abs(np.asarray(scores, np.float64)[i]) <= H.DBL_MAX


def wave_counts(read, key, threads=TILE):
    """int[tiles, threads / 64]: the valid sites of every wave of every tile of the fill (the last tile padded with no site)"""
    _, valid = covered_valid(read, key)
    tiles = -(-len(valid) // threads)
    padded = np.zeros(tiles * threads, np.int64)
    padded[:len(valid)] = valid
    return padded.reshape(tiles, threads // WAVE, WAVE).sum(2)


# ---------------------------------------------------------------------------------------------------------------- the reads with holes

def hole_tiles(n):
    """pattern (b)'s two tiles in a read that covers n sites: (the tile whose wave 1 is empty, the tile whose waves 0 and 2 are; None
    where the read is too short to have it)"""
    return (1, 3) if n >= 4 * TILE else ((0, 1) if n >= 2 * TILE else (0, None))


def single_site(n, t):
    """pattern (c)'s one valid site of tile t in a read that covers n sites: wave t % 4 where the tile has it"""
    return min(TILE * t + WAVE * (t % 4) + (37 * t + 5) % WAVE, n - 1)


def last_wave(n):
    """pattern (d)'s 64 valid sites in a read that covers n sites: the last wave of the last full tile (of the last full 64 below a tile)"""
    hi = TILE * (n // TILE) if n >= TILE else WAVE * (n // WAVE)
    return hi - WAVE, hi


def _valid_mask(rng, pattern, n):
    """per site in key order whether the read's score there is valid"""
    if pattern == 'a':
        return rng.random(n) >= 0.3
    if pattern == 'b':
        v = rng.random(n) < 0.25
        ta, tb = hole_tiles(n)
        for t, waves, keep in ((ta, (1,), (0, 2, 3)), (tb, (0, 2), (1, 3))):
            if t is None:
                continue
            for w in keep:                                                    # (an entry in every wave that is not emptied)
                v[min(TILE * t + WAVE * w + int(rng.integers(0, WAVE)), n - 1)] = True
            for w in waves:
                v[TILE * t + WAVE * w:TILE * t + WAVE * (w + 1)] = False
        return v
    v = np.zeros(n, bool)
    if pattern == 'c':
        v[[single_site(n, t) for t in range(-(-n // TILE))]] = True
    elif pattern == 'd':
        a, b = last_wave(n)
        v[a:b] = True
    return v


def _scores(rng, cs, valid):
    """the scores of a read, per event, from the validity of its sites in key order (every position a site)"""
    s = np.where(valid, VALUES[rng.integers(0, len(VALUES), len(valid))], INVALID[rng.integers(0, len(INVALID), len(valid))])
    return s[::-1].copy() if cs & 1 else s                                    # '-': event i lies at start + n - 1 - i


@functools.lru_cache(maxsize=None)
def hole_reads():
    """One case: dict(reads, key, tags, the flat arrays of WALK, and hoff / site / x / s of hmm_ref.entries_ref).  tags[r] is (pattern,
    events) of read r, ('sparse', events) for the reads on cs 2 and ('mixed', events) for the short ones.
    Sites: every position 0 .. TOP on cs 0 ('+') and on cs 1 ('-'), every seventh on cs 2.  Reads of HOLE_EVENTS events on cs 0 and on
    cs 1 (every event lies on a site, so a read of n events covers n sites), each in the patterns
      (a) about 30 % of the scores invalid at random;
      (b) a quarter valid at random, but wave 1 of one tile and waves 0 and 2 of another all invalid (hole_tiles), the other waves of
          those tiles with an entry: a shared word of the fill is 0 while later waves write;
      (c) one valid score per tile, in wave t % 4 of tile t (single_site);
      (d) valid only in the last wave of the read's last full tile (last_wave);
      (e) every score invalid: a long read without an entry;
    NaN, +inf and -inf all serve as invalid scores.  On cs 2 reads of SPARSE_EVENTS events with about 20 % invalid: more than EVENTS_MAX
    events and at most 858 entries, so the workgroup form fills what a wave chains.  Pattern (a) at 2 048 events keeps more than
    ENTRIES_MAX entries under the wave form of the fill, from 2 049 events under the workgroup form.  Twenty short reads of
    test_read_hmm_gpu's `mixed` kind go among them and the whole is shuffled.
    Pattern (a) alone holds 0.7 * 26 384 entries, so the case has about 27 000, not the 15 000 first meant; the restatements of K19,
    K20 and K22 still take seconds on it (tests/test_chain_cases.py runs K19's)."""
    rng = np.random.default_rng(2301)
    key = np.array([_key(cs, p) for cs in (0, 1) for p in range(TOP + 1)] + [_key(2, p) for p in range(0, TOP + 1, 7)], np.int64)
    reads, tags = [], []
    for pattern in HOLE_PATTERNS:
        for n in HOLE_EVENTS:
            for cs in (0, 1):
                reads.append((cs, int(rng.integers(0, TOP + 2 - n)), _scores(rng, cs, _valid_mask(rng, pattern, n))))
                tags.append((pattern, n))
    for n in SPARSE_EVENTS:
        reads.append((2, int(rng.integers(0, TOP + 2 - n)), _scores(rng, 2, rng.random(n) >= 0.2)))
        tags.append(('sparse', n))
    mixed = np.concatenate((VALUES, INVALID))
    for _ in range(20):
        n = int(rng.integers(1, 61))
        reads.append((int(rng.integers(0, 3)), int(rng.integers(0, TOP + 2 - n)), mixed[rng.integers(0, len(mixed), n)]))
        tags.append(('mixed', n))
    order = rng.permutation(len(reads))
    reads, tags = [reads[i] for i in order], [tags[i] for i in order]
    c = case_arrays(reads, key)
    c.update(reads=reads, tags=tags)
    c['hoff'], c['site'], c['x'], c['s'] = H.entries_ref(*[c[f] for f in WALK])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def longest_of_each_pattern(c):
    """the index of the read with the most events of every pattern of hole_reads()"""
    return [max((r for r, t in enumerate(c['tags']) if t[0] == p), key=lambda r: (c['tags'][r][1], -r)) for p in HOLE_PATTERNS + ('sparse',)]


# ---------------------------------------------------------------------------------------------------------------- the sort passes

SORT_NSITES = (255, 256, 65535, 65536, 70000, 2 ** 24 + 3)
SORT_HOST_MAX = 70000                                # beyond: device memspace and the rows alone (the key and soff take 134 MB each)
CARRIES = (1 << 8, 1 << 16, 1 << 24)


def sort_passes(nsites):
    """the bytes of the largest sort key, nsites itself (the key of a row that no read owns): nmod_read_class_rows' selector restated"""
    return max(1, -(-int(nsites).bit_length() // 8))


def sort_key(nsites):
    """sites at positions 0, 3, 6, ... on one '+' id"""
    return np.arange(nsites, dtype=np.int64) * 3


def byte_pair(nsites):
    """two sites that carry rows, equal in the bytes below the key's top byte and different in it alone; None where the table has no
    such pair beyond the second byte"""
    hi = (1 << (8 * (sort_passes(nsites) - 1))) + 1
    return (1, hi) if 1 << 16 < hi < nsites else None


@functools.lru_cache(maxsize=None)
def sort_reads(nsites):
    """The reads of the case of `nsites` sites, 60 .. 120 of 3 .. 40 events, as (cs, start, scores) triples.  A read `over` sites
    i0 .. i0 + k - 1 starts at position 3 i0.  In this order: the top sites; both sides of every byte carry of the site index the table
    has; the higher site of byte_pair; four reads over the same ten sites; 70 reads at random (half of them within the first 300 sites,
    a tenth of their scores invalid); the lower site of byte_pair; the first sites.  So the rows are far from site order, and a sort
    that stopped a pass early would leave the higher site of byte_pair in front of the lower."""
    rng = np.random.default_rng(2302 + nsites % 1000)

    def over(i0, k, invalid=0.0):
        n = max(3, 3 * (k - 1) + 1 + int(rng.integers(0, 3)))
        s = VALUES[rng.integers(0, len(VALUES), n)]
        if invalid:
            s = np.where(rng.random(n) < invalid, INVALID[rng.integers(0, len(INVALID), n)], s)
        return (0, 3 * int(i0), s)
    reads = [over(nsites - 5, 5)]
    reads += [over(c - 3, 6) for c in reversed(CARRIES) if c < nsites]
    pair = byte_pair(nsites)
    if pair:
        reads.append(over(pair[1], 1))
    reads += [over(nsites // 2, 10) for _ in range(4)]
    for i in range(70):
        k = int(rng.integers(1, 14))
        reads.append(over(rng.integers(0, min(nsites, 300) - k) if i % 2 else rng.integers(0, nsites - k), k, 0.1))
    if pair:
        reads.append(over(pair[0], 1))
    reads.append(over(0, 4))
    return tuple(reads)


def sort_pass_case(nsites):
    """(nsites, reads, key)"""
    return nsites, list(sort_reads(nsites)), sort_key(nsites)


def sort_pass_cases():
    """the cases one at a time: the last one's key takes 134 MB"""
    for nsites in SORT_NSITES:
        yield sort_pass_case(nsites)
