"""The window ranking of --RegionRankbyST 1 restated as a plain dict walk (no GPU, no library), and constructed inputs for it.

Written from the text of include/nanomod_hip.h (nmod_region_rank) and the docstring of nanomod_amd.detect.region_rank:

  * w = window + 1; the windows of one (chrom, strand) are centred on pk = pmin, pmin + movesize, ... below pmax, where pmin / pmax
    are the smallest / largest tested position of that (chrom, strand) and movesize is 1 (WindOvlp == 1) or w;
  * a window needs every position pk - w .. pk + w tested, non-negative and below pmax;
  * of its 2w + 1 members those whose base equals `na` contribute (all of them when `na` is empty); the window is kept when more
    than 5 contribute;
  * key = sorted(contributing values)[int(percentile * (len - 1) + 0.5)]; tie-break = |w - index of the first occurrence of the
    smallest contributing value in the unsorted contributing list|;
  * the windows are ranked by (key, tie-break) with Python's stable sorted() over generation order: (chrom, strand) keys
    ascending, centres ascending;
  * with WindOvlp == 1 a window is dropped when a better-ranked KEPT window of the same (chrom, strand) lies closer than w:
    the quadratic scan over everything kept so far, as the definition states it.

NaN values are outside the definition (a window holding one has no defined rank); no builder below produces one.

The builders take a seeded numpy.random.default_rng and return a dict of arrays (chrom, strand, pos, base, value) in record order
(sorted (chrom, strand), ascending position), with `w` where the case is built around one half-width."""
import numpy as np

CLAUSES = ('absent', 'at_pmax', 'negative', 'few')


def _chars(base):
    if isinstance(base, (bytes, bytearray)):
        return list(bytes(base).decode('latin-1'))
    return [str(b) for b in base]


def walk(chrom, strand, pos, base, value, window, wind_ovlp, percentile, na):
    """Every centre the definition visits, in generation order, as a dict: index (of the centre's record, None when the centre
    itself is not a tested position), seg, pos, failed (the subset of CLAUSES that rejects it; `few` is evaluated only when the
    window is complete), cnt, key, tb."""
    w = int(window) + 1
    movesize = 1 if wind_ovlp == 1 else w
    base = _chars(base)
    segs = {}
    for i in range(len(pos)):
        segs.setdefault((str(chrom[i]), str(strand[i])), {})[int(pos[i])] = i
    out = []
    for sk in sorted(segs):
        at = segs[sk]
        pmin, pmax = min(at), max(at)
        for pk in range(pmin, pmax, movesize):
            members = range(pk - w, pk + w + 1)
            failed = set()
            if any(p not in at for p in members):
                failed.add('absent')
            if pk + w >= pmax:
                failed.add('at_pmax')
            if pk - w < 0:
                failed.add('negative')
            c = dict(index=at.get(pk), seg=sk, pos=pk, failed=failed, cnt=None, key=None, tb=None)
            if not failed:
                vals = [float(value[at[p]]) for p in members if not na or base[at[p]] == na]
                c['cnt'] = len(vals)
                if len(vals) > 5:
                    srt = sorted(vals)
                    c['key'] = srt[int(percentile * (len(srt) - 1) + 0.5)]
                    c['tb'] = abs(w - vals.index(srt[0]))
                else:
                    failed.add('few')
            out.append(c)
    return out


def ranked_windows(chrom, strand, pos, base, value, window, wind_ovlp, percentile, na, suppress=None):
    """(kept, dropped): the ranked windows (dicts of walk()) after / removed by the overlap suppression.  `suppress` overrides
    WindOvlp == 1 as the switch of the suppression alone (False: the ranked list before it)."""
    w = int(window) + 1
    valid = [c for c in walk(chrom, strand, pos, base, value, window, wind_ovlp, percentile, na) if not c['failed']]
    order = sorted(valid, key=lambda c: (c['key'], c['tb']))
    if not (wind_ovlp == 1 if suppress is None else suppress):
        return order, []
    kept, dropped = [], []
    for c in order:
        if any(k['seg'] == c['seg'] and abs(k['pos'] - c['pos']) < w for k in kept):
            dropped.append(c)
        else:
            kept.append(c)
    return kept, dropped


def region_rank(chrom, strand, pos, base, value, window, wind_ovlp, percentile, na):
    """Indices of the records the ranked window centres sit on, best first."""
    return [c['index'] for c in ranked_windows(chrom, strand, pos, base, value, window, wind_ovlp, percentile, na)[0]]


def tally(chrom, strand, pos, base, value, window, wind_ovlp, percentile, na):
    """How the definition treats a case: centres visited, valid windows, windows rejected by exactly one clause (per clause),
    by several, and suppressed."""
    cs = walk(chrom, strand, pos, base, value, window, wind_ovlp, percentile, na)
    t = dict(centres=len(cs), valid=sum(not c['failed'] for c in cs), several=sum(len(c['failed']) > 1 for c in cs))
    for name in CLAUSES:
        t[name] = sum(c['failed'] == {name} for c in cs)
    t['suppressed'] = len(ranked_windows(chrom, strand, pos, base, value, window, wind_ovlp, percentile, na)[1])
    return t


# --------------------------------------------------------------------------------------------------------- array helpers
def segment_bounds(chrom, strand):
    """strand_lo / strand_hi of nmod_region_rank for records in (chrom, strand) order: first / last index of each record's run"""
    n = len(chrom)
    chrom, strand = np.asarray(chrom), np.asarray(strand)
    new = np.r_[True, (chrom[1:] != chrom[:-1]) | (strand[1:] != strand[:-1])] if n else np.zeros(0, bool)
    starts = np.flatnonzero(new)
    ends = np.r_[starts[1:], n] - 1
    seg = np.cumsum(new) - 1
    return starts[seg].astype(np.int32), ends[seg].astype(np.int32)


def base_bytes(base):
    """the base column as the C entry takes it: one byte per record, a blank for an empty base"""
    return ''.join((b[:1] or ' ') for b in _chars(base)).encode('latin-1')


def golden_value(exp, method, rank_use):
    """the column of a golden result table the reference ranks windows by: the KS or the combined track, p-value or statistic"""
    return exp[('ks_' if method == 'ks' else 'comb_') + ('p' if rank_use == 'pv' else ('d' if method == 'ks' else 'st'))]


def golden_records(exp, method):
    """the reference's sign_test records of a golden result table"""
    recs = []
    for i in range(len(exp['pos'])):
        tests = [(exp['mwu_u'][i], exp['mwu_p'][i]), (exp['t_t'][i], exp['t_p'][i]), (exp['ks_d'][i], exp['ks_p'][i])]
        if method != 'ks':
            tests.append((exp['comb_st'][i], exp['comb_p'][i]))
        recs.append(((str(exp['chrom'][i]), str(exp['strand'][i]), int(exp['pos'][i]), str(exp['base'][i]), int(exp['n0'][i]), int(exp['n1'][i])),
                     tests))
    return recs


SEG_KEYS = (('chr1', '+'), ('chr1', '-'), ('chr2', '+'), ('chr2', '-'), ('chr3', '+'), ('chr3', '-'))


def _assemble(parts, base=None):
    """parts: (positions, values) per segment, given the keys of SEG_KEYS in order"""
    assert len(parts) <= len(SEG_KEYS)
    sizes = [len(p) for p, _ in parts]
    case = dict(chrom=np.repeat([k[0] for k in SEG_KEYS[:len(parts)]], sizes), strand=np.repeat([k[1] for k in SEG_KEYS[:len(parts)]], sizes),
                pos=np.concatenate([np.asarray(p, dtype=np.int64) for p, _ in parts]),
                value=np.concatenate([np.asarray(v, dtype=np.float64) for _, v in parts]))
    case['base'] = np.full(len(case['pos']), 'A') if base is None else np.asarray(base)
    return case


def _gapped(rng, start, count, rate=0.08):
    """`count` ascending positions from `start`: steps of 1, and of 2..5 (a gap of 1-4 positions) at `rate`; a segment of 300
    records or more keeps records 100..219 free of gaps, so that windows of up to 45 positions fit after the first gaps"""
    step = np.where(rng.random(count) < rate, rng.integers(2, 6, count), 1)
    step[0] = 0
    if count >= 300:
        step[101:220] = 1
    return start + np.cumsum(step)


def case_segments(rng, sizes=(1, 6, 40, 300, 700)):
    """Segments of the given sizes with random gaps and continuous values.  (1, 6, 40, 300, 700): every segment boundary lies
    inside a 256-thread block; (256, 40, 1, 6, 300): the first boundary is the block boundary at index 256."""
    parts = [(_gapped(rng, int(rng.integers(0, 50)), n), rng.random(n)) for n in sizes]
    return _assemble(parts, rng.choice(list('ACGT'), sum(sizes)))


def case_shared_positions(rng, count=120):
    """The same gapped positions and the same values on (chr1, +), (chr1, -) and (chr2, +)"""
    pos, val = _gapped(rng, 30, count, rate=0.04), rng.random(count)
    return _assemble([(pos, val)] * 3)


def case_strand_ends(rng, w):
    """Gap-free segments: exactly 2w + 1 records (no window: its last member is pmax), 2w + 2 records (one window), a start at
    position 0, a start at w - 1 (its first centres lack members), and a start below 0 (complete windows with a negative member)"""
    runs = ((500, 2 * w + 1), (500, 2 * w + 2), (0, 3 * w + 4), (w - 1, 3 * w + 4), (-3, 3 * w + 6))
    parts = [(np.arange(s, s + n), rng.random(n)) for s, n in runs]
    return dict(_assemble(parts), w=w)


def case_step_phase(rng, w, count=150):
    """One segment whose second record sits one position late: from there (p - pmin) and (i - lo) differ by one, so with
    movesize = w stepping by index picks other centres than stepping by position"""
    pos = np.arange(100, 100 + count)
    pos[1:] += 1
    return dict(_assemble([(pos, rng.random(count))]), w=w)


TIE_VALUES = (0.0, -0.0, 1e-300, 0.25, 0.5, 1.0)


def case_ties(rng, w, count=400):
    """Two gap-free segments of values from TIE_VALUES: random draws (the minimum repeats inside most windows), stretches of one
    value longer than a window (runs of equal (key, tie-break)), and a stretch alternating 0.0 / -0.0 (equal, not identical).
    Bases are 'A' at about 70 %, so that na = 'A' leaves even and odd member counts."""
    parts = []
    for s in range(2):
        v = rng.choice(TIE_VALUES, count, p=(0.15, 0.15, 0.1, 0.3, 0.2, 0.1))
        v[40:40 + 4 * w + 30] = 0.25
        v[200:200 + 4 * w + 30] = np.where(np.arange(4 * w + 30) % 2 == 0, 0.0, -0.0)
        v[320:320 + 2 * w + 12] = 1.0
        parts.append((np.arange(1000 * s + 7, 1000 * s + 7 + count), v))
    return dict(_assemble(parts, np.where(rng.random(2 * count) < 0.7, 'A', 'G')), w=w)


def case_base_filter(rng, w, count=260):
    """na = 'A' on one gap-free segment with continuous values: a stretch of 'A' only (2w + 1 contributing members), random bases
    (the window minimum often sits on a base that does not contribute), two stretches of 'C' holding exactly 5 and exactly 6 'A'
    within one window, and three records with an empty base."""
    assert 3 <= w <= 14
    base = rng.choice(list('ACGT'), count, p=(0.7, 0.1, 0.1, 0.1)).astype(object)
    base[10:10 + 4 * w] = 'A'
    for centre, k in ((-(-132 // w) * w, 5), (-(-198 // w) * w, 6)):         # (multiples of w: centres of WindOvlp = 0 too)
        base[centre - 2 * w - 2:centre + 2 * w + 3] = 'C'
        base[centre - w + rng.choice(2 * w + 1, k, replace=False)] = 'A'
    base[[70, 71, 150]] = ''
    value = rng.random(count)
    low = np.flatnonzero(base != 'A')
    value[low[::2]] *= 0.01                                  # many window minima on records the filter removes
    return dict(_assemble([(np.arange(40, 40 + count), value)], base), w=w)


def case_suppression(rng, w, count=500):
    """WindOvlp = 1 on two gap-free segments of continuous values, with pairs of low values w - 1, w and w + 1 apart: at
    percentile 0 the windows centred on them are the best of their neighbourhood, at these three distances from each other.
    Two stretches of w + 1 low values make a chain at percentile 0.5: one window holds all of the lowest stretch, so its median
    is low and it ranks first; its neighbours hold w of them at the most, so their medians are ordinary and they rank below the
    window over the second stretch, far away, and are blocked by the first window alone"""
    parts = []
    for s in range(2):
        v = 0.5 + 0.5 * rng.random(count)
        for q, d, lowv in ((60, w - 1, 0.01), (160, w, 0.02), (260, w + 1, 0.03)):
            v[q], v[q + d] = lowv + 0.1 * s, lowv + 0.1 * s + 0.001
        for q, lowv in ((360, 0.10), (430, 0.20)):
            v[q:q + w + 1] = lowv + 0.1 * s + 0.01 * rng.random(w + 1)
        parts.append((np.arange(20, 20 + count), v))
    return dict(_assemble(parts), w=w)


def gpu_cases():
    """name -> (case, [(w, wind_ovlp, percentile, na), ...]): what tests/test_region_rank_gpu.py runs on the device, and what
    tests/test_region_rank.py checks the conditions of on the restatement alone"""
    rng = np.random.default_rng
    c = {}
    for layout, sizes in (('inblock', (1, 6, 40, 300, 700)), ('at256', (256, 40, 1, 6, 300))):
        for w in (3, 4, 11, 22):
            c['segments_%s_w%d' % (layout, w)] = (case_segments(rng(11), sizes), [(w, o, p, '') for o in (0, 1) for p in (0.0, 0.1, 0.5, 1.0)])
    c['shared_positions'] = (case_shared_positions(rng(12)), [(4, 1, 0.1, ''), (11, 1, 0.5, '')])
    for w in (3, 11):
        c['strand_ends_w%d' % w] = (case_strand_ends(rng(13), w), [(w, o, 0.1, '') for o in (0, 1)])
    for w in (3, 4, 22):
        c['step_phase_w%d' % w] = (case_step_phase(rng(14), w), [(w, 0, 0.1, '')])
    for w in (3, 4):
        c['ties_w%d' % w] = (case_ties(rng(15), w), [(w, o, p, na) for o in (0, 1) for p in (0.0, 0.5) for na in ('', 'A')])
    for w in (3, 11):
        c['base_filter_w%d' % w] = (case_base_filter(rng(16), w), [(w, o, p, 'A') for o in (0, 1) for p in (0.0, 0.5)])
    for w in (3, 4, 11):
        c['suppression_w%d' % w] = (case_suppression(rng(17), w), [(w, 1, p, '') for p in (0.0, 0.1, 0.5)])
    return c
