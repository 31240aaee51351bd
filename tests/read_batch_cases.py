"""Batches of reads larger than the grids of K11 (nmod_rescale_reads), K12 (nmod_read_calls) and K13 (nmod_read_llr), and what they
must give.  The entries define a read's outputs by the read alone, so a batch whose read i is read idx[i] of a small set of D distinct
reads has the distinct reads' outputs, gathered: per_read[idx] and per_event[ev].  The restatements (rescale_ref, readcalls_ref,
readllr_ref) loop over reads in Python and only ever see the D distinct reads; the batch and its expectation are built without a Python loop over its reads.  Nothing
here calls the library."""
import functools

import numpy as np

import readcalls_ref as Q
import readllr_ref as F
import rescale_ref as R

WAVE_MAX = R.WAVE_MAX
assert Q.WAVE_MAX == WAVE_MAX == F.WAVE_MAX       # the entries split their classes at the same length

# The grids, restated from the launch code; the tests size their batches from these and assert that they did.
WAVES_PER_BLOCK = 4                               # read_walk.hpp: kRwWaves = kRwThreads / 64, a short read takes a wave
BLOCKS_PER_CU = 8                                 # the caps: nmod_rescale_reads num_cus * 6 (table in LDS) or 8; nmod_read_calls num_cus * 2; rl_launch at most num_cus * 5 — the largest
CLASSIFY_READS_PER_CU = 16 * 256                  # read_classify_kernel: ccap = num_cus * 16 blocks of 256 threads, a thread per read
CLASSIFY_BEYOND = 100000                          # reads past the first stride of the classify grid in the second-pass batches

RESCALE_MIN_EVENTS = 30
RESCALE_FIELDS = ('shift', 'scale', 'n_used', 'status')
CALLS_ALPHA = 0.01
CALLS_EVENT_FIELDS = ('z', 'p', 'p_win')
CALLS_READ_FIELDS = ('n_sites', 'n_called', 'status')
LLR_THR = F.PARITY_THR
LLR_PRIOR_LOGIT = F.PARITY_PRIOR_LOGIT
LLR_EVENT_FIELDS = ('llr', 'llr_win', 'p_mod')
LLR_READ_FIELDS = ('n_sites', 'n_mod', 'n_can', 'status')


def short_units(cus):
    return BLOCKS_PER_CU * WAVES_PER_BLOCK * cus


def long_units(cus):
    return BLOCKS_PER_CU * cus


def calls_inner(nb):
    """the events a tile of K12 owns: kRwTile - 2 * halo, the halo whole runs of 8"""
    return 512 - 2 * 8 * ((nb + 7) // 8)


def llr_inner(window):
    """the events a tile of K13 owns: kRwTile less the halo before and the halo after, each whole runs of 8"""
    return 512 - 8 * ((window[0] + 7) // 8) - 8 * ((window[1] + 7) // 8)


# ---------------------------------------------------------------------------------------------------------------- the batch builder

def tile_batch(val, off, base, idx):
    """the batch whose read i is distinct read idx[i]: dict(val, off, base, idx, ev) with val = distinct val[ev]"""
    off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int64)
    dlens, dstart = np.diff(off), off[:-1]
    assert idx.ndim == 1 and (len(idx) == 0 or (idx.min() >= 0 and idx.max() < len(dlens)))
    lens = dlens[idx]
    boff = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(lens, out=boff[1:])
    total = int(boff[-1])
    ev = np.repeat(dstart[idx] - boff[:-1], lens) + np.arange(total, dtype=np.int64)
    return dict(val=np.asarray(val)[ev], off=boff, base=R.as_bytes(base)[ev], idx=idx, ev=ev)


def gather(small, idx, ev, read_fields, event_fields):
    """the expected outputs of a batch from those of its distinct reads; whatever else `small` holds (a margin, say) is kept"""
    out = {f: v for f, v in small.items() if f not in read_fields and f not in event_fields}
    out.update({f: small[f][idx] for f in read_fields if f in small})
    out.update({f: small[f][ev] for f in event_fields if f in small})
    return out


def _stack(reads, dtype):
    lens = [len(x) for _, x in reads]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    val = R.cast(np.concatenate([np.asarray(x, np.float64) for _, x in reads]), dtype)
    base = np.concatenate([np.asarray(b, np.uint8) for b, _ in reads])
    for a in (val, off, base):
        a.setflags(write=False)
    return val, off, base


def short_lengths(k):
    return sorted({0, 1, 2, 3, k - 1, k, 63, 64, 65, 300, 511, 512, 513, WAVE_MAX})


# ------------------------------------------------------------------------------------------------------------ the distinct sets: K11

def _status_reads(rng, n, k, center, mean, sd):
    """reads of n events that end in each failing status reachable at this length, and one that saturates int16: (name, base, x)"""
    few = np.full(n, ord('N'), np.uint8)
    few[5:5 + 20 + k - 1] = rng.choice(np.frombuffer(b'ACGT', np.uint8), 20 + k - 1)       # 20 events with a k-mer: fewer than min_events
    out = [('too_few', few, R.draw_values(rng, few, k, center, mean, sd, 0.1, 1.1))]
    out.append(('homopolymer', np.full(n, ord('A'), np.uint8), np.rint(rng.normal(0.0, 0.2, n) * 1000.0) / 1000.0))
    b, x = R.draw_read(rng, n, k, center, mean, sd, 0.0, 1.0, contaminate=False)
    out.append(('negative_slope', b, -x))
    out.append(('out_of_range',) + R.draw_read(rng, n, k, center, mean, sd, 0.0, 3.0, contaminate=False))
    b, x = R.draw_read(rng, n, k, center, mean, sd, 0.0, 0.6, contaminate=False)
    x[[7, n // 2, n - 3]] = 25.0                                                       # clipped out of the fit; 25 / 0.6 is beyond int16 milli-units
    out.append(('clamped', b, x))
    return out


@functools.lru_cache(maxsize=None)
def rescale_distinct(k, center, dtype):
    """K11's distinct reads: dict(val, off, base, mean, sd, names).  Every short length at which the code takes another path, long reads
    just past WAVE_MAX (and one of 5 000), and in both classes the failing statuses next to ordinary reads whose planted shifts and
    scales differ clearly.  The reads are the same for every dtype."""
    rng = np.random.default_rng(4100 + 100 * k + 10 * center)
    mean, sd = R.make_model(k)
    reads, names = [], []

    def add(name, b, x):
        names.append(name); reads.append((b, x))

    planted = ((-0.3, 0.8), (0.3, 1.25), (0.1, 1.0))
    for i, n in enumerate(short_lengths(k)):
        a, s = planted[i % 3]
        add('short_%d' % n, *R.draw_read(rng, n, k, center, mean, sd, a, s, n_letters=2 if i % 3 == 0 else 0))
    for name, b, x in _status_reads(rng, 400, k, center, mean, sd):
        add('short_' + name, b, x)
    for i, (a, s) in enumerate(planted):
        add('long_%d' % i, *R.draw_read(rng, WAVE_MAX + 1, k, center, mean, sd, a, s, n_letters=2 * (i % 2)))
    for name, b, x in _status_reads(rng, WAVE_MAX + 1, k, center, mean, sd):
        add('long_' + name, b, x)
    add('long_plus_tile', *R.draw_read(rng, WAVE_MAX + 1 + 512, k, center, mean, sd, -0.2, 1.2))
    add('long_5000', *R.draw_read(rng, 5000, k, center, mean, sd, 0.2, 0.9))
    val, off, base = _stack(reads, dtype)
    return dict(val=val, off=off, base=base, mean=mean, sd=sd, names=tuple(names))


@functools.lru_cache(maxsize=None)
def rescale_expected(k, center, dtype, mode=R.FIT_APPLY):
    d = rescale_distinct(k, center, dtype)
    return R.rescale(d['val'], d['off'], d['base'], k, center, d['mean'], d['sd'], mode=mode, min_events=RESCALE_MIN_EVENTS)


def rescale_gather(small, idx, ev):
    return gather(small, idx, ev, RESCALE_FIELDS, ('val', 't1000'))


# ------------------------------------------------------------------------------------------------------------ the distinct sets: K12

@functools.lru_cache(maxsize=None)
def calls_distinct(k, center, nb, dtype):
    """K12's distinct reads: dict(val, off, base, mean, sd, names).  The short lengths and the three around the tile's own events for
    this nb; reads with no eligible event, with model holes and 'N' bytes, and clean / shifted reads whose n_called differ widely; long
    reads just past WAVE_MAX, one a tile longer, one of 5 000."""
    rng = np.random.default_rng(5200 + 1000 * k + 100 * center + nb)
    mean, sd = R.make_model(k)
    inner = calls_inner(nb)
    reads, names = [], []

    def add(name, b, x):
        names.append(name); reads.append((b, x))

    for i, n in enumerate(sorted(set(short_lengths(k)) | {inner - 1, inner, inner + 1})):
        add('short_%d' % n, *R.draw_read(rng, n, k, center, mean, sd, 0.0, 1.0, contaminate=i % 2 == 0, n_letters=2 if i % 3 == 0 else 0))
    for tag, n in (('short', 600), ('long', WAVE_MAX + 1)):
        add(tag + '_none_eligible', np.full(n, ord('n'), np.uint8), np.zeros(n))
        add(tag + '_clean', *R.draw_read(rng, n, k, center, mean, sd, 0.0, 1.0, contaminate=False))
        add(tag + '_shifted', *R.draw_read(rng, n, k, center, mean, sd, 1.0, 1.0, contaminate=False))
        b = np.tile(np.frombuffer(b'AATACGGCGTAACC', np.uint8), n // 14 + 1)[:n].copy()        # (k = 3) runs through the holes of the model
        b[[n // 3, n // 3 + 1, n - 2]] = ord('N')
        add(tag + '_holes', b, R.draw_values(rng, b, k, center, mean, sd, 0.0, 1.0))
    add('long_contaminated', *R.draw_read(rng, WAVE_MAX + 1, k, center, mean, sd, 0.0, 1.0, n_letters=3))
    add('long_plus_tile', *R.draw_read(rng, WAVE_MAX + 1 + inner, k, center, mean, sd, 0.0, 1.0))
    add('long_5000', *R.draw_read(rng, 5000, k, center, mean, sd, 0.0, 1.0))
    val, off, base = _stack(reads, dtype)
    return dict(val=val, off=off, base=base, mean=mean, sd=sd, names=tuple(names))


@functools.lru_cache(maxsize=None)
def calls_expected(k, center, nb, dtype):
    d = calls_distinct(k, center, nb, dtype)
    return Q.read_calls(d['val'], d['off'], d['base'], k, center, d['mean'], d['sd'], nb, CALLS_ALPHA)


def calls_gather(small, idx, ev):
    return gather(small, idx, ev, CALLS_READ_FIELDS, CALLS_EVENT_FIELDS + ('W',))


# ------------------------------------------------------------------------------------------------------------ the distinct sets: K13

@functools.lru_cache(maxsize=None)
def llr_distinct(k, center, window, dtype):
    """K13's distinct reads: dict(val, off, base, mean, sd, alt_mean, alt_sd, names).  The short lengths and the three around the tile's
    own events for this window; reads drawn from the unmodified and from the modified table in turn (n_mod and n_can differ widely), with
    no eligible event, with the holes of both tables and 'N' bytes; long reads just past WAVE_MAX (more than a tile per wave: 4 tiles of
    at most 512 own events, and no multiple of any tile), one a tile longer, one of 5 000."""
    rng = np.random.default_rng(6300 + 1000 * k + 100 * center + 7 * window[0] + window[1])
    mean, sd = R.make_model(k)
    mean1, sd1 = F.make_alt_model(k, mean, sd)
    inner = llr_inner(window)
    assert WAVE_MAX + 1 > WAVES_PER_BLOCK * 384 and (WAVE_MAX + 1) % inner and 5000 % inner
    reads, names = [], []

    def add(name, b, x):
        names.append(name); reads.append((b, x))

    for i, n in enumerate(sorted(set(short_lengths(k)) | {inner - 1, inner, inner + 1})):
        src = (mean, sd) if i % 2 == 0 else (mean1, sd1)
        add('short_%d' % n, *R.draw_read(rng, n, k, center, src[0], src[1], 0.0, 1.0, contaminate=i % 4 < 2, n_letters=2 if i % 3 == 0 else 0))
    for tag, n in (('short', 600), ('long', WAVE_MAX + 1)):
        add(tag + '_none_eligible', np.full(n, ord('n'), np.uint8), np.zeros(n))
        add(tag + '_unmodified', *R.draw_read(rng, n, k, center, mean, sd, 0.0, 1.0, contaminate=False))
        add(tag + '_modified', *R.draw_read(rng, n, k, center, mean1, sd1, 0.0, 1.0, contaminate=False))
        b = np.tile(np.frombuffer(b'AATACGGCGTAACCCCTTTGGGACCA', np.uint8), n // 26 + 1)[:n].copy()   # (k = 3) runs through the holes of both tables
        b[[n // 3, n // 3 + 1, n - 2]] = ord('N')
        add(tag + '_holes', b, R.draw_values(rng, b, k, center, mean, sd, 0.0, 1.0))
    add('long_contaminated', *R.draw_read(rng, WAVE_MAX + 1, k, center, mean1, sd1, 0.0, 1.0, n_letters=3))
    add('long_plus_tile', *R.draw_read(rng, WAVE_MAX + 1 + inner, k, center, mean, sd, 0.0, 1.0))
    add('long_5000', *R.draw_read(rng, 5000, k, center, mean1, sd1, 0.0, 1.0))
    val, off, base = _stack(reads, dtype)
    return dict(val=val, off=off, base=base, mean=mean, sd=sd, alt_mean=mean1, alt_sd=sd1, names=tuple(names))


@functools.lru_cache(maxsize=None)
def llr_expected(k, center, window, dtype):
    d = llr_distinct(k, center, window, dtype)
    return F.restate(d['val'], d['off'], d['base'], k, center, d['mean'], d['sd'], d['alt_mean'], d['alt_sd'], window, LLR_THR, LLR_PRIOR_LOGIT)


def llr_gather(small, idx, ev):
    return gather(small, idx, ev, LLR_READ_FIELDS, LLR_EVENT_FIELDS + ('gate_llr', 'gate_L'))


# ----------------------------------------------------------------------------------------------------------------- the index vectors

def _draw_ids(rng, ids, n, weights=None):
    """n of `ids`, each at least once"""
    assert n >= len(ids)
    p = None if weights is None else np.asarray(weights, np.float64) / np.sum(weights)
    return np.concatenate([ids, rng.choice(ids, n - len(ids), p=p)])


def batch_index(off, kind, cus, seed=1):
    """idx of the 'short', 'long' or 'mixed' batch for a device of `cus` compute units: more than twice as many reads of a class as
    the largest grid has units for it, every distinct read of the class present, in a seeded order.  Most long reads are the shortest
    ones: the events of the long batches are what costs time."""
    lens = np.diff(np.asarray(off, np.int64))
    rng = np.random.default_rng(seed)
    parts = []
    if kind in ('short', 'mixed'):
        parts.append(_draw_ids(rng, np.flatnonzero(lens <= WAVE_MAX), 2 * short_units(cus) + 37))
    if kind in ('long', 'mixed'):
        ids = np.flatnonzero(lens > WAVE_MAX)
        parts.append(_draw_ids(rng, ids, 2 * long_units(cus) + 5, np.where(lens[ids] == WAVE_MAX + 1, 1.0, 0.1)))
    assert parts, kind
    return rng.permutation(np.concatenate(parts))


def classify_index(off, cus, seed=2):
    """idx of a batch just past one stride of the classify grid: 95 % of the reads have 0 .. 3 events, the rest are short-class reads
    (mostly those of up to 65 events: the batch stays at a few million events), every short distinct read at least once, and seven long
    reads among the last CLASSIFY_BEYOND indices — beyond the first stride"""
    lens = np.diff(np.asarray(off, np.int64))
    rng = np.random.default_rng(seed)
    n = CLASSIFY_READS_PER_CU * cus + CLASSIFY_BEYOND
    tiny, short, long_ = np.flatnonzero(lens <= 3), np.flatnonzero(lens <= WAVE_MAX), np.flatnonzero(lens > WAVE_MAX)
    idx = rng.choice(tiny, n)
    rest = np.flatnonzero(rng.random(n) >= 0.95)
    other = short[lens[short] > 3]
    w = np.where(lens[other] <= 65, 1.0, 0.01)
    idx[rest] = rng.choice(other, len(rest), p=w / w.sum())
    idx[rng.choice(n, len(short), replace=False)] = short
    idx[n - CLASSIFY_BEYOND + rng.choice(CLASSIFY_BEYOND, 7, replace=False)] = rng.choice(long_, 7)
    return idx


def class_counts(off):
    lens = np.diff(np.asarray(off, np.int64))
    return int((lens <= WAVE_MAX).sum()), int((lens > WAVE_MAX).sum())
