"""Constructed positions for the all-tests sorting forms of K1 (rank_hist_kernel, rank_pair_kernel) and their packing into
batches.  A case is a dict {family, name, a, b}: the two groups as integer "units" (float32 input: units * 2^-11, exact and
mostly off the milli-unit grid; int16 input: the units themselves, milli-units), or as float32 arrays for the families that
need values no unit can express (signed zeros, +-FLT_MAX: 'f32' is set).  Every generator takes the sizes m <= q of the sorted
group S and the ranked group Q and says in sorted-order terms what S and Q look like; hist_model.py proves the claims
(test_hist_model.py).  The samples of a group are shuffled in memory: the kernels sort S and scatter Q in arrival order."""
import numpy as np

import hist_model as M

F32_UNIT = 2.0 ** -11
FLT_MAX = np.finfo(np.float32).max
HIST_INSTANCES = ((8, 8), (16, 8), (16, 16), (16, 32), (16, 64))             # (R, LG): capacities 64 .. 1 024
PAIR_CLASSES = ((5, 3), (5, 4), (5, 5))                                      # size classes of (group 1, group 2)


def runs(lengths, first=0, step=1):
    """sorted values with the given run lengths: run i holds first + step * i"""
    return np.repeat(first + step * np.arange(len(lengths), dtype=np.int64), lengths)


F64_UNIT = 2.0 ** -40


def values(case, dtype):
    """the two groups as the library's input arrays.  Further dtypes of big_cases.py: 'g32' — float32 on the milli-unit grid,
    units / 1000 in float32 arithmetic (what grid_key of rank_hist.hpp accepts for |units| <= 32 767); 'f64' — float64; a case with
    'kind' set says which doubles: 'redo' 1.0 + units * 2^-40 (every float32 image is 1.0, the doubles order and tie as the units
    do: neither float32-exact nor on the grid unless every unit is 0), 'exact' units * 2^-11 (float32-exact), 'grid' units / 1000"""
    if dtype == 'f64':
        kind = case['kind']
        f = lambda u: 1.0 + u * F64_UNIT if kind == 'redo' else (u * F32_UNIT if kind == 'exact' else u / 1000.0)
        assert kind in ('redo', 'exact', 'grid') and max(np.abs(case['a']).max(), np.abs(case['b']).max()) < 2 ** 12
        return f(case['a'].astype(np.float64)), f(case['b'].astype(np.float64))
    if case.get('f32'):
        assert dtype == 'f32'
        return case['a'], case['b']
    if dtype == 'g32':
        assert max(np.abs(case['a']).max(), np.abs(case['b']).max()) <= 32767
        return case['a'].astype(np.float32) / np.float32(1000.0), case['b'].astype(np.float32) / np.float32(1000.0)
    if dtype == 'f32':
        return (case['a'] * F32_UNIT).astype(np.float32), (case['b'] * F32_UNIT).astype(np.float32)
    assert min(case['a'].min(), case['b'].min()) >= -32768 and max(case['a'].max(), case['b'].max()) <= 32767
    return case['a'].astype(np.int16), case['b'].astype(np.int16)


# ---- the families: each returns [(family, name, S, Q)] with len(S) = m <= len(Q) = q
def gen_random(m, q, rng, tag=''):
    span = max(3, (m + q) // 3)                                              # a few ties inside and across the groups
    return [('size_matrix', 'random%s_%dv%d' % (tag, m, q), rng.integers(-span, span, m), rng.integers(-span, span, q) + (m % 3))]


def gen_end_bin(m, q):
    s = np.arange(m, dtype=np.int64)
    return [('end_bin_hi', 'distinct', s, m + 5 + np.arange(q)), ('end_bin_hi', 'equal', s, np.full(q, m + 5)),
            ('end_bin_lo', 'distinct', s, -5 - np.arange(q)), ('end_bin_lo', 'equal', s, np.full(q, -5))]


def one_bin_ks(m, R):
    """bins k of S that take all of Q: at a lane boundary (lane 1, a middle lane) and mid-lane"""
    j = max(1, (m // R) // 2)
    ks = [(k, where) for k, where in ((R, 'boundary'), (R * j, 'boundary'), (R * j + R // 2, 'midlane')) if 0 < k < m]
    return sorted(set(ks))


def gen_one_bin_mid(m, q, R):
    out = []
    for k, where in one_bin_ks(m, R):
        s = np.arange(m, dtype=np.int64); s[k:] += q + 1
        out.append(('one_bin_mid', '%s_k%d' % (where, k), s, k + np.arange(q)))
    return out


def pairs_layout(n):
    """run lengths: a single, then pairs — a pair at (R - 1 | 0) across every lane boundary for any even R"""
    return [1] + [2] * ((n - 1) // 2) + [1] * ((n - 1) % 2)


def gen_pairs(m, q):
    s = runs(pairs_layout(m), 0, 2)
    return [('pairs_only', 'disjoint', s, runs(pairs_layout(q), 1, 2)), ('pairs_only', 'shared', s, runs(pairs_layout(q), 0, 2))]


def triple_layout(n, t):
    """pairs, and one run of three that starts at sorted index t"""
    head = ([1] if t % 2 else []) + [2] * (t // 2)
    rest = n - t - 3
    assert rest >= 0
    return head + [3] + [2] * (rest // 2) + [1] * (rest % 2)


def triple_starts(n, R):
    j = max(1, (n // R) // 2)
    return (('Rm2_Rm1_0', R * j - 2), ('Rm1_0_1', R * j - 1), ('midlane', R * j + R // 2 - 1))


def gen_triple(m, q, R, groups=('q', 's')):
    out = []
    for g in groups:
        n = q if g == 'q' else m
        for where, t in triple_starts(n, R):
            if t + 3 > n:
                continue
            lay = triple_layout(n, t)
            s = runs(lay if g == 's' else pairs_layout(m), 0, 2)
            qq = runs(lay if g == 'q' else pairs_layout(q), 1, 2)
            out.append(('one_triple', '%s_%s' % (g, where), s, qq))
    return out


def gen_long_runs(m, q, R, lengths=None):
    out = []
    s = 2 * np.arange(m, dtype=np.int64) + 1
    for L in (lengths or (R, R + 1, 2 * R + 1)):
        for o in (0, 1, R - 1):
            t = R + o                                                        # the run starts in lane 1 at register offset o
            if t + L > q:
                continue
            out.append(('long_runs', 'len%d_at%d' % (L, o), s, runs([1] * t + [L] + [1] * (q - t - L), 0, 2)))
    out.append(('long_runs', 'whole_q', s, np.full(q, 2 * (m // 2))))         # one run covers all of Q, in the middle of S
    out.append(('long_runs', 'whole_s', np.full(m, 2 * (q // 2)), 2 * np.arange(q)))   # ... all of S, with one sample of Q on it
    return out


def _tiled(m, q, tiles, fill):
    """S = runs of a_i copies of 6 i, Q = b_i copies of the same values; the rest of S / Q are distinct untied values (6 i + 2 /
    6 i + 4) after the tiles (fill = 'after': the first key of S is tied) or before them ('before': the last key of S is tied)"""
    na, nb = sum(a for a, _ in tiles), sum(b for _, b in tiles)
    assert na <= m and nb <= q
    t = len(tiles)
    idx = lambda n: (t + np.arange(n)) if fill == 'after' else (-1 - np.arange(n))
    s = np.concatenate([runs([a for a, _ in tiles], 0, 6), 6 * idx(m - na) + 2])
    qq = np.concatenate([runs([b for _, b in tiles], 0, 6), 6 * idx(q - nb) + 4])
    return s.astype(np.int64), qq.astype(np.int64)


def gen_s_runs(m, q, R):
    out = []
    n23 = max(1, min(m // 2, q // 3) // 2)
    out.append(('s_runs_with_q', 'a2b3_first_key',) + _tiled(m, q, [(2, 3)] * n23, 'after'))
    n32 = max(1, min(m // 3, q // 2) // 2)
    out.append(('s_runs_with_q', 'a3b2_last_key',) + _tiled(m, q, [(3, 2)] * n32, 'before'))
    nrr = min(m // R, q // (R + 1))
    if nrr >= 1:
        out.append(('s_runs_with_q', 'aR_bR1',) + _tiled(m, q, [(R, R + 1)] * nrr, 'after'))
    if m >= 8:
        mid_s = 6 * (1 + np.arange(m - 5)) + 2; mid_q = 6 * (1 + np.arange(q - 5)) + 4
        top = 6 * (max(m, q) + 2)
        out.append(('s_runs_with_q', 'first_and_last_key', np.concatenate([[0] * 3, mid_s, [top] * 2]), np.concatenate([[0] * 2, mid_q, [top] * 3])))
    if m >= 4:
        s, qq = _tiled(m, q, [(m // 2, q // 2)], 'after')
        out.append(('s_runs_with_q', 'half_half', s, qq))
    if m >= 2:
        out.append(('s_runs_with_q', 'all_but_one',) + _tiled(m, q, [(m - 1, q - 1)], 'before'))
    return [(f, n, np.asarray(s, np.int64), np.asarray(qq, np.int64)) for f, n, s, qq in out]


def gen_all_equal(m, q):
    # 750: 0.75 as milli-units and 750 * 2^-11 as float32 are both exact in binary, so the reference's means of the constant rows
    # are exact and its Welch statistic is 0 / 0 = NaN, not the quotient of two rounding errors that 0.777 gives
    return [('all_equal', 'v750', np.full(m, 750), np.full(q, 750))]


def gen_but_one(m, q):
    out = []
    for g in ('s', 'q'):
        for where, v in (('first', 700), ('last', 800)):
            s = np.full(m, 750); qq = np.full(q, 750)
            (s if g == 's' else qq)[0] = v
            out.append(('all_equal_but_one', '%s_%s' % (g, where), s, qq))
    return out


def gen_signed_zero(m, q):
    def grp(n, neg, pos):
        rest = n - neg - pos
        if rest < 0:
            neg, pos, rest = (n + 1) // 2, n // 2, 0
        other = (np.arange(rest) - rest // 2) * F32_UNIT * 3
        other = other[other != 0]
        x = np.concatenate([np.full(neg, -0.0), np.full(pos + (rest - len(other)), 0.0), other]).astype(np.float32)
        return x
    return [('signed_zero', 'mixed', grp(m, 2, 1), grp(q, 2, 2)), ('signed_zero', 'many', grp(m, m // 3, m // 4), grp(q, q // 4, q // 3))]


def gen_flt_max(m, q):
    def grp(n, hi, lo):
        hi, lo = min(hi, n), min(lo, max(n - hi, 0))
        rest = n - hi - lo
        return np.concatenate([np.full(hi, FLT_MAX), np.full(lo, -FLT_MAX), (np.arange(rest) - rest // 2) * F32_UNIT * 5]).astype(np.float32)
    return [('flt_max', 'both_groups', grp(m, 2, 1), grp(q, 3, 2)), ('flt_max', 'q_only', grp(m, 0, 0), grp(q, 4, 1)), ('flt_max', 's_only', grp(m, 3, 2), grp(q, 0, 0))]


def _emit(out, rng, gen, order=0):
    for family, name, s, q in gen:
        f32 = np.asarray(s).dtype == np.float32
        s = rng.permutation(np.asarray(s) if f32 else np.asarray(s, np.int64))
        q = rng.permutation(np.asarray(q) if f32 else np.asarray(q, np.int64))
        assert len(s) <= len(q)
        a, b = (q, s) if (order and len(s) < len(q)) else (s, q)
        out.append({'family': family, 'name': '%s/%s/%dv%d' % (family, name, len(a), len(b)), 'a': a, 'b': b, 'f32': f32})


_CACHE = {}


def hist_cases(R, LG, dtype):
    """the constructed positions of rank_hist_kernel<R, LG>: every case has n0, n1 that the classifier sends to this instance"""
    key = ('hist', R, LG, dtype)
    if key in _CACHE:
        return _CACHE[key]
    cap = R * LG
    rng = np.random.default_rng(100 * R + LG)
    inst = ('rank_hist', R, LG)
    out = []
    FULL, PAD = (cap, cap), (cap // 2 + 1, cap - 1)
    # size matrix: m in {1, 2, cap/2 + 1, cap - 1, cap} x q in {m, cap - 1, cap}, both orders.  From capacity 256 on the classifier
    # hands a group of cap/4 samples or fewer (against one above cap/2) to the WIDE form: there cap/4 + 1 and cap/4 + 2 are the
    # smallest sizes this instance sees
    small = [1, 2] if cap <= 128 else [cap // 4 + 1, cap // 4 + 2]
    seen = set()
    for m in small + [cap // 2 + 1, cap - 1, cap]:
        for q in (m, cap - 1, cap):
            for n0, n1 in ((m, q), (q, m)):
                if (n0, n1) in seen or M.instance_of(n0, n1) != inst:
                    continue
                seen.add((n0, n1))
                _emit(out, rng, gen_random(min(m, q), max(m, q), rng), order=int(n0 > n1))
    for i, (m, q) in enumerate((FULL, PAD)):
        _emit(out, rng, gen_end_bin(m, q), order=i)
        _emit(out, rng, gen_one_bin_mid(m, q, R), order=0)
        _emit(out, rng, gen_pairs(m, q), order=i)
        _emit(out, rng, gen_triple(m, q, R, ('q', 's') if i == 0 else ('q',)), order=i)
        _emit(out, rng, gen_long_runs(m, q, R, None if i == 0 else (2 * R + 1,)), order=0)
        _emit(out, rng, gen_s_runs(m, q, R), order=i)
        _emit(out, rng, gen_all_equal(m, q), order=i)
        _emit(out, rng, gen_but_one(m, q), order=i)
        if dtype == 'f32':
            _emit(out, rng, gen_signed_zero(m, q), order=i)
            _emit(out, rng, gen_flt_max(m, q), order=i)
    for c in out:
        assert M.instance_of(len(c['a']), len(c['b'])) == inst, c['name']
    _CACHE[key] = out
    return out


def row_neighbour_cases(R, LG):
    """LG = 8: a chain of full positions, each ending in the value the next one begins with (three keys of S, and two / four of Q)"""
    assert LG == 8
    if ('row', R) in _CACHE:
        return _CACHE[('row', R)]
    cap = R * LG
    rng = np.random.default_rng(7 * R)
    out = []
    for k in range(2 * (64 // LG)):
        v0, v1 = k * (cap + 10), (k + 1) * (cap + 10)
        mid = v0 + 1 + np.arange(cap - 6)
        _emit(out, rng, [('row_neighbours', 'link%d' % k, np.concatenate([[v0] * 3, mid, [v1] * 3]), np.concatenate([[v0] * 2, mid, [v1] * 4]))])
    _CACHE[('row', R)] = out
    return out


def pair_sizes(c0, c1):
    """(n0, n1) of rank_pair_kernel<2^c0, 2^c1>: group 1 at its capacity against group 2 at cap/2 + 1 and the reverse (full_vs_padded),
    both full, and an odd size in between"""
    C0, C1 = 64 << c0, 64 << c1
    return [(C0, C1 // 2 + 1), (C0 // 2 + 1, C1), (C0, C1), (C0 - 37, C1 - 212)]


def pair_cases(c0, c1, dtype):
    key = ('pair', c0, c1, dtype)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(10 * c0 + c1)
    inst = ('rank_pair', 1 << c0, 1 << c1)
    out = []
    R = 16
    for i, (n0, n1) in enumerate(pair_sizes(c0, c1)):
        m, q = min(n0, n1), max(n0, n1)
        order = int(n0 > n1)
        sub = []
        _emit(sub, rng, gen_random(m, q, rng), order)
        _emit(sub, rng, gen_all_equal(m, q), order)
        _emit(sub, rng, gen_but_one(m, q), order)
        _emit(sub, rng, gen_s_runs(m, q, R), order)
        if i < 2:                                                            # the two full_vs_padded sizes carry every other family too
            _emit(sub, rng, gen_end_bin(m, q)[:2], order)
            _emit(sub, rng, gen_pairs(m, q), order)
            _emit(sub, rng, gen_triple(m, q, R, ('q',))[:1], order)
            _emit(sub, rng, gen_long_runs(m, q, R, (2 * R + 1,)), order)
            if dtype == 'f32':
                _emit(sub, rng, gen_signed_zero(m, q)[:1], order)
                _emit(sub, rng, gen_flt_max(m, q)[:1], order)
            for c in sub[:3]:                                                # (named for what this kernel adds: the pad bookkeeping)
                out.append(dict(c, family='full_vs_padded', name='full_vs_padded/' + c['name']))
            sub = sub[3:]
        out += sub
    for c in out:
        assert M.instance_of(len(c['a']), len(c['b'])) == inst, (c['name'], M.instance_of(len(c['a']), len(c['b'])), inst)
    _CACHE[key] = out
    return out


def gen_narrow(m, q, rng):
    """int16 positions the counting forms accept (hist_model.count_window_tails): nearly all keys within a 2 048-value window —
    so ties abound —, with and without a few samples far outside it (the forms' tail list), up to both ends of the int16 range"""
    out = []
    for span in (40, 900):
        out.append(('narrow_random', 'span%d' % span, rng.integers(-span, span, m), rng.integers(-span, span, q) + (m % 3)))
    out += gen_all_equal(m, q) + gen_but_one(m, q)
    for k in (3, 100):
        out.append(('narrow_tiled', 'k%d' % k) + _tiled(m, q, [(m // k, q // k)] * k, 'after'))
    s = rng.integers(-300, 300, m); qq = rng.integers(-300, 300, q)
    s[:5] = (30000, 30000, 30000, -32768, -32768); qq[:7] = (32767, 32767, 32767, 30000, -30000, -30000, -32768)
    out.append(('narrow_outliers', 'tails', s, qq))
    return out


def pair_narrow_cases(c0, c1):
    """rank_pair_kernel's sizes once more, int16 only, on positions that the counting forms of the class (rank_count_wide_kernel,
    rank_count_value_kernel for (5, 5)) take when they are not switched off: the same position through both kinds of form"""
    key = ('narrow', c0, c1)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(1000 + 10 * c0 + c1)
    out = []
    for n0, n1 in pair_sizes(c0, c1):
        _emit(out, rng, gen_narrow(min(n0, n1), max(n0, n1), rng), int(n0 > n1))
    _CACHE[key] = out
    return out


# ---- packing
def interleave(cases):
    """an order of the cases in which neighbours are of different families wherever the counts allow it: always the family with
    the most cases left that differs from the one just placed"""
    fam = {}
    for i, c in enumerate(cases):
        fam.setdefault(c['family'], []).append(i)
    order, last = [], None
    while any(fam.values()):
        f = max((k for k in fam if fam[k] and k != last), key=lambda k: len(fam[k]), default=last)
        order.append(fam[f].pop(0))
        last = f
    return order


def rotate_pack(order, PW, fam=lambda i: i):
    """indices for one batch: `order`, padded with cases of its own to a multiple of PW, once per rotation s = 0 .. PW - 1 — so
    entry i of the padded list sits at slot (i - s) mod PW of its wave: every slot once.  fam(i): the family of case i; the last
    entry is moved and the pads are chosen so that cyclic neighbours differ in family where that is possible"""
    order = list(order)
    if PW > 1 and len(order) > 2 and fam(order[-1]) == fam(order[0]):
        x = order.pop()
        k = next((k for k in range(1, len(order)) if fam(order[k - 1]) != fam(x) != fam(order[k])), len(order))
        order.insert(k, x)
    pad = (-len(order)) % PW
    for j in range(pad):
        ok = lambda i: fam(i) != fam(order[-1]) and (j < pad - 1 or fam(i) != fam(order[0]))
        order.append(next((i for i in order if ok(i)), order[j]))
    out = []
    for s in range(PW):
        out += order[s:] + order[:s]
    return out


def split_batches(cases, PW, limit):
    """the cases as rotated batches of at most `limit` positions each (interleaved first)"""
    order = interleave(cases)
    per = max(PW, (limit // PW) // PW * PW) if PW > 1 else limit             # cases per batch, a multiple of PW
    return [rotate_pack(order[i:i + per], PW, lambda i: cases[i]['family']) for i in range(0, len(order), per)]


def triple_waves(cases, PW):
    """one_triple among fast-path wave-mates: for every triple case of full size and every slot, a wave of pairs_only positions of the
    same size with the triple at that slot -> (indices, the same batch with each triple replaced by one more pairs_only position:
    what the mates compute without it)"""
    n = lambda c: (len(c['a']), len(c['b']))
    trip = [i for i, c in enumerate(cases) if c['family'] == 'one_triple' and n(c)[0] == n(c)[1]]
    mates = [i for i, c in enumerate(cases) if c['family'] == 'pairs_only' and n(c)[0] == n(c)[1]]
    idx, without = [], []
    for t in trip:
        for s in range(PW):
            idx += [t if j == s else mates[(j + s) % len(mates)] for j in range(PW)]
            without += [mates[(j + s) % len(mates)] for j in range(PW)]
    return idx, without


def uniform_groups(cases, at_least=3):
    """{(n0, n1): [indices]} of the sizes that enough cases share: these also run as fixed-stride batches"""
    g = {}
    for i, c in enumerate(cases):
        g.setdefault((len(c['a']), len(c['b'])), []).append(i)
    return {k: v for k, v in g.items() if len(v) >= at_least}


def concat(cases, idx, dtype):
    """-> (sig0, off0, sig1, off1) of the batch"""
    va = [values(cases[i], dtype) for i in idx]
    off0 = np.zeros(len(idx) + 1, np.int64); off0[1:] = np.cumsum([len(a) for a, _ in va])
    off1 = np.zeros(len(idx) + 1, np.int64); off1[1:] = np.cumsum([len(b) for _, b in va])
    return np.concatenate([a for a, _ in va]), off0, np.concatenate([b for _, b in va]), off1
