"""Constructed positions for the large-position forms of K1 (nanomod_amd/csrc/big_rank.hpp: big_rank_kernel, big_hist_kernel,
wide_redo_kernel; the two-pass WIDE classes kWideBigBase + cs of rank_hist_kernel) and their packing into batches, in the
conventions of hist_cases.py: a case is a dict {family, name, a, b} of integer units (float32: units * 2^-11; int16: the units;
'g32': units / 1000 as float32, on the milli-unit grid; float64, the redo form: hist_cases.values), the generators speak of the
smaller group S (m samples) and the larger one Q (q samples) in sorted-order terms, and the samples are shuffled in memory.
test_big_cases.py (CPU) proves every claim made here; test_big_forms_constructed_gpu.py runs the cases.

int16 (and g32) lists hold what the domain can express: a case that needs more than 65 536 distinct values (distinct-valued
families at 65 535 samples a group) exists for float32 only, and a case whose units leave [-32 768, 32 767] is shifted as a
whole (ranks and ties do not move)."""
import numpy as np

import hist_cases as HC
import hist_model as M

THREADS = 256                     # kBigThreads: the stride of every per-thread loop of big_rank.hpp
HASH_SLOTS = 8192                 # kBigHistSlots
REDO_HITS = 351                   # rank_hist.hpp, bitmap_passes: the redo list takes a position when 2 hits + 64 > 3 * 1021 / 4


def pow2_ceil(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def form_of(n0, n1, ks_only=False):
    """classify_position (rank_stats_launch.hpp) for groups within NMOD_MAX_RANKED: 'big_rank', 'big_hist', ('wide_big', cs), or
    None for a position of the wave-resident kernels"""
    assert 1 <= n0 <= 65535 and 1 <= n1 <= 65535
    c0, c1 = M.size_class_of(n0), M.size_class_of(n1)
    s, q = min(n0, n1), max(n0, n1)
    big = min(c0, c1) >= 6 if ks_only else max(c0, c1) >= 6
    if not big:
        return None
    if not ks_only and s <= 256 and q <= 4096:
        return ('wide_big', min(c0, c1))
    if not ks_only and s <= 1024 and q <= 4096:
        return 'big_hist'
    return 'big_rank'


def emit(out, rng, gen, order, dtype):
    """hist_cases._emit for these lists: order = 1 makes Q group 1 (for equal sizes: the roles swap); int16 / g32: see above"""
    for family, name, s, q in gen:
        s, q = np.asarray(s), np.asarray(q)
        f32 = s.dtype == np.float32
        assert len(s) <= len(q) and (dtype == 'f32' or not f32)
        if not f32:
            s, q = s.astype(np.int64), q.astype(np.int64)
            lo, hi = min(s.min(), q.min()), max(s.max(), q.max())
            if dtype != 'f32' and hi - lo > 65535:
                continue
            if dtype != 'f32' and (lo < -32768 or hi > 32767):
                s, q = s - (lo + hi + 1) // 2, q - (lo + hi + 1) // 2
        s, q = rng.permutation(s), rng.permutation(q)
        a, b = (q, s) if order else (s, q)
        out.append({'family': family, 'name': '%s/%s/%dv%d' % (family, name, len(a), len(b)), 'a': a, 'b': b, 'f32': f32, 'order': order})


# ---- families
def gen_random(m, q, rng, span=None):
    span = span or max(3, (m + q) // 3)
    return [('random_ties', 'span%d' % span, rng.integers(-span, span, m), rng.integers(-span, span, q) + (m % 3))]


def gen_one_bin(m, q, ks=None):
    """all of Q, distinct, between keys k - 1 and k of a distinct S: L = U = k for every sample"""
    out = []
    for k, where in sorted({k: w for w, k in (('last', m - 1), ('mid', m // 2), ('first', 1))}.items()):
        if 0 < k < m and (ks is None or where in ks):
            s = np.arange(m, dtype=np.int64); s[k:] += q + 1
            out.append(('one_bin', '%s_k%d' % (where, k), s, k + np.arange(q)))
    return out


def gen_whole(m, q):
    """one run covers all of Q (tied with one key in the middle of a distinct S); one run covers all of S"""
    return [('one_run', 'whole_q', np.arange(m), np.full(q, m // 2)), ('one_run', 'whole_s', np.full(m, q // 2), np.arange(q))]


def gen_ends(m, q):
    """all of Q in one run just above / just below a distinct S, and two constant groups: D = 1 with the fewest values.  (The
    constants 0 and 125 are exact in binary as milli-units too — see hist_cases.gen_all_equal: the reference's Welch statistic of two
    constant rows is then -inf, not the quotient of two rounding errors.)"""
    return [('end_bin_hi', 'equal_next', np.arange(m), np.full(q, m)), ('end_bin_lo', 'equal_next', np.arange(m), np.full(q, -1)),
            ('two_halves', 'const_v_const', np.zeros(m, np.int64), np.full(q, 125))]


def tiled(m, q, tiles, fill):
    """S = runs of a_i copies of 4 i, Q = b_i copies of the same values; the rest of both groups distinct and untied (S even, Q
    odd) after the tiles ('after': tile 0 is at sorted index 0 of both groups) or before them ('before': the last tile ends both)"""
    na, nb, t = sum(a for a, _ in tiles), sum(b for _, b in tiles), len(tiles)
    assert na <= m and nb <= q
    tv = 4 * np.arange(t, dtype=np.int64)
    if fill == 'after':
        rs, rq = 4 * t + 2 * np.arange(m - na), 4 * t + 1 + 2 * np.arange(q - nb)
    else:
        rs, rq = -2 - 2 * np.arange(m - na), -1 - 2 * np.arange(q - nb)
    return np.concatenate([np.repeat(tv, [a for a, _ in tiles]), rs]), np.concatenate([np.repeat(tv, [b for _, b in tiles]), rq])


STRIDE_KINDS = (('1xL', 1, 1), ('Lx1', 1, 1), ('LxL', 1, 1), ('Lx0', 1, 0), ('0xL', 0, 1))


def stride_tile(kind, L):
    return {'1xL': (1, L), 'Lx1': (L, 1), 'LxL': (L, L), 'Lx0': (L, 0), '0xL': (0, L)}[kind]


def gen_stride_runs(m, q, lengths=(255, 256, 257, 513)):
    """runs of L equal keys against the 256-thread stride: tied runs of (1, L), (L, 1), (L, L) samples of (S, Q), a run of S with
    no sample of Q and the reverse, as many per case as the groups hold; 'first': the first tile is at sorted index 0, 'last':
    the last tile ends at n - 1 (next to the pads).  The name lists the tiles in value order."""
    out = []
    for li, L in enumerate(lengths):
        kinds = [k for k, _, _ in STRIDE_KINDS]
        kinds = kinds[li % 5:] + kinds[:li % 5]                                # another tile leads for every length
        for fill, where in (('after', 'first'), ('before', 'last')):
            cur = []
            def flush():
                if cur:
                    out.append(('stride_runs', 'L%d_%s_%s' % (L, where, '+'.join(cur)),) + tiled(m, q, [stride_tile(k, L) for k in cur], fill))
                del cur[:]
            for k in kinds:
                a, b = stride_tile(k, L)
                if a > m or b > q:
                    continue
                if sum(stride_tile(c, L)[0] for c in cur) + a > m or sum(stride_tile(c, L)[1] for c in cur) + b > q:
                    flush()
                cur.append(k)
            flush()
    return out


def gen_generic(m, q, rng, dtype):
    """the generic families at a size whose distinct values fit every dtype"""
    g = gen_random(m, q, rng) + HC.gen_end_bin(m, q) + gen_ends(m, q)[2:] + gen_one_bin(m, q) + HC.gen_pairs(m, q) + gen_whole(m, q) + HC.gen_all_equal(m, q)
    if dtype == 'f32':
        g += HC.gen_signed_zero(m, q) + HC.gen_flt_max(m, q)
    return g


def gen_reduced(m, q, rng, dtype):
    """... at a size beyond 10 000 samples: one case per family, written with the fewest distinct values"""
    span = min(max(3, (m + q) // 3), 30000 if dtype != 'f32' else 1 << 30)
    return (gen_random(m, q, rng, span) + gen_ends(m, q) + gen_one_bin(m, q, ('mid',)) + gen_whole(m, q)[:1] + HC.gen_all_equal(m, q)
            + gen_stride_runs(m, q, (257,)))


# ---- big_rank_kernel
BIG_RANK_SIZES = ((1, 4097), (1025, 2049), (2049, 2049), (4096, 4097), (8192, 8192), (8193, 5), (16384, 1025), (65535, 1), (65535, 65535))
BIG_RANK_KS_SIZES = ((2049, 2049), (2049, 65535), (8192, 8193), (65535, 65535))
_CACHE = {}


def size_cases(n0, n1, dtype):
    """the cases of one size pair and its swap -> {(n0, n1): [cases], (n1, n0): [cases]}; equal sizes: the roles alternate"""
    key = ('size', min(n0, n1), max(n0, n1), dtype)
    if key not in _CACHE:
        m, q = key[1], key[2]
        rng = np.random.default_rng(m * 70001 + q)
        gen = gen_reduced(m, q, rng, dtype) if m + q > 10000 else gen_generic(m, q, rng, dtype) + gen_stride_runs(m, q)
        if m == q:
            lst = []
            for j, g in enumerate(gen):
                emit(lst, rng, [g], j % 2, dtype)
            _CACHE[key] = {(m, q): lst}
        else:
            fwd, rev = [], []
            emit(fwd, rng, gen, 0, dtype); emit(rev, rng, gen, 1, dtype)
            _CACHE[key] = {(m, q): fwd, (q, m): rev}
    return _CACHE[key]


def big_rank_batches(dtype, ks_only=False):
    """-> [((n0, n1), [cases])]: one uniform batch per size pair and per order of the groups"""
    out = []
    for n0, n1 in (BIG_RANK_KS_SIZES if ks_only else BIG_RANK_SIZES):
        d = size_cases(n0, n1, dtype)
        out.append(((n0, n1), d[(n0, n1)]))
        if n0 != n1:
            out.append(((n1, n0), d[(n1, n0)]))
    return out


def mixed_batch(batches, family='random_ties'):
    """one case of `family` from every uniform batch: the sizes mixed in one CSR batch"""
    return [next(c for c in cases if c['family'] == family) for _, cases in batches]


# ---- big_hist_kernel
BH_M = (257, 511, 512, 513, 1023, 1024)
BH_Q = (2049, 2304, 2305, 4095, 4096)
BH_SIZES = ((257, 2049), (512, 4096), (513, 4095), (1024, 2049), (1024, 4096))
BH_FIXUP_SIZES = ((512, 4096), (1024, 4096), (1024, 2049), (511, 2304), (1023, 2305), (257, 2049), (513, 4095))   # m == P, P - 1, P / 2 + 1


def hash_slot(x):
    """big_hist_kernel's home slot of a float32 key: ((bits of x + 0.0f) * 2654435761 mod 2^32) >> 19"""
    bits = (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    return ((bits * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(19)


def key_of(units, dtype):
    """the float32 key big_hist_kernel hashes for a sample of `units`"""
    u = np.asarray(units, np.int64)
    return (u * HC.F32_UNIT).astype(np.float32) if dtype == 'f32' else u.astype(np.float32)


def chain_units(dtype, kind):
    """units whose keys collide in the hash table, found by search over the dtype's domain (float32: |units| < 2^19).
    'chain': the keys of the fullest home slot (at most 16); 'wrap': up to six keys of home slot 8 190 and six of 8 191 — at least
    three in all, so that the probe sequence runs past slot 8 191 into slot 0"""
    key = ('chain', dtype, kind)
    if key not in _CACHE:
        u = np.arange(-(1 << 19), 1 << 19) if dtype == 'f32' else np.arange(-32768, 32768)
        slot = hash_slot(key_of(u, dtype)).astype(np.int64)
        if kind == 'chain':
            best = int(np.argmax(np.bincount(slot, minlength=HASH_SLOTS)))
            _CACHE[key] = u[slot == best][:16]
        else:
            _CACHE[key] = np.concatenate([u[slot == HASH_SLOTS - 2][:6], u[slot == HASH_SLOTS - 1][:6]])
    return _CACHE[key]


def gen_hash(m, q, rng, dtype):
    out = []
    for kind in ('chain', 'wrap'):
        keys = chain_units(dtype, kind)
        lo = int(keys.min()) if dtype == 'f32' else -q
        pool = np.setdiff1d(np.arange(lo, lo + 2 * q), keys)
        for mult in ('once', 'repeated'):
            body = np.repeat(keys, 1 if mult == 'once' else 2 + np.arange(len(keys)) % 4)
            filler = rng.choice(pool, q - len(body), replace=False)            # distinct, none of them a chain key
            out.append(('hash_' + kind, mult, rng.choice(np.arange(lo, lo + 2 * q), m, replace=False), np.concatenate([body, filler])))
    if q == 4096:
        out.append(('hash_table', 'distinct_4096', rng.integers(-q, q, m), rng.permutation(np.arange(-q, q))[:q]))
        out.append(('hash_table', 'one_value_x4096', rng.integers(-q, q, m), np.full(q, 1234)))
    return out


def gen_fixup(m, q, rng):
    """the branchless search over P - 1 keys and its one more comparison: half of Q equal to, just below and just above the last /
    the first key of a distinct S (4 apart), and a quarter each in one case"""
    out = []
    s = 4 * np.arange(m, dtype=np.int64)
    for kn, key in (('last', int(s[-1])), ('first', 0)):
        for dn, d in (('equal', 0), ('below', -1), ('above', 1)):
            qq = rng.integers(-2, int(s[-1]) + 3, q); qq[:q // 2] = key + d
            out.append(('search_fixup', '%s_%s' % (kn, dn), s, qq))
        qq = rng.integers(-2, int(s[-1]) + 3, q); h = q // 4
        qq[:h] = key - 1; qq[h:2 * h] = key; qq[2 * h:3 * h] = key + 1
        out.append(('search_fixup', '%s_mixed' % kn, s, qq))
    return out


def gen_packed_bins(m, q):
    """the 16 | 16 packed bins at their fullest: every sample of Q with the same L and U — L = U = k (low and high half of bin k
    both hold q), and L = k, U = k + r with all of Q tied to a run of r keys of S (two bins, one half each)"""
    k, r = m // 2, 7
    s = np.arange(m, dtype=np.int64); s[k:] += q + 1
    t = np.concatenate([np.arange(k), np.full(r, k), k + 1 + np.arange(m - k - r)])
    return [('packed_bins', 'same_LU_k%d' % k, s, k + np.arange(q)), ('packed_bins', 'tied_run_k%d_r%d' % (k, r), t, np.full(q, k))]


def big_hist_cases(dtype):
    if ('bh', dtype) in _CACHE:
        return _CACHE[('bh', dtype)]
    rng = np.random.default_rng(4096 + (dtype == 'i16'))
    out = []
    for m in BH_M:                                                          # the size matrix, either group the larger one
        for q in BH_Q:
            for order in (0, 1):
                emit(out, rng, [('size_matrix', 'random',) + gen_random(m, q, rng)[0][2:]], order, dtype)
    for i, (m, q) in enumerate(BH_SIZES):
        gen = gen_generic(m, q, rng, dtype) + gen_stride_runs(m, q) + gen_hash(m, q, rng, dtype) + gen_packed_bins(m, q)
        emit(out, rng, gen, i % 2, dtype)
    for i, (m, q) in enumerate(BH_FIXUP_SIZES):
        emit(out, rng, gen_fixup(m, q, rng), (i + 1) % 2, dtype)
    _CACHE[('bh', dtype)] = out
    return out


# ---- the two-pass WIDE classes of rank_hist_kernel
WIDE_S = (1, 64, 65, 128, 129, 256)
WIDE_Q = (2049, 4095, 4096)


def wide_big_cases(dtype):
    """generic families only (dtype 'f32': off the grid; 'g32': on it; 'i16')"""
    if ('wb', dtype) not in _CACHE:
        rng = np.random.default_rng(49 + len(dtype) + ord(dtype[0]))
        out = []
        for i, (m, q) in enumerate((m, q) for m in WIDE_S for q in WIDE_Q):
            emit(out, rng, gen_generic(m, q, rng, dtype), i % 2, dtype)
        _CACHE[('wb', dtype)] = out
    return _CACHE[('wb', dtype)]


# ---- wide_redo_kernel
REDO_SIZES = ((7, 300), (100, 2048), (256, 4095), (40, 4096))


def redo_layout(q, t, L):
    """run lengths of a sorted Q: pairs (heavy ties: q / 2 samples find their bitmap bit set), and one run of L at sorted index t"""
    pairs = lambda n: [1] * (n % 2) + [2] * (n // 2)
    assert t + L <= q
    return pairs(t) + [L] + pairs(q - t - L)


def gen_redo(m, q, rng):
    """wide_redo_kernel gives each thread per = P / 256 consecutive sorted keys and carries the open run's start across chunks:
    runs of per, per + 1 and 3 per + 1 keys that start at a chunk's first key, at its last key and inside it, among pairs; one
    run over everything; two runs; a third of Q distinct among one heavy value; no ties at all.  S (even units, 2 is off the
    milli-unit grid) never ties with Q (odd units)."""
    per = max(64, pow2_ceil(q)) // THREADS
    assert per >= 2
    s = 2 * rng.permutation(4 * m)[:m]; s[0] = 2
    out = []
    for L in (per, per + 1, 3 * per + 1):
        for o, where in sorted({o: w for w, o in (('mid_chunk', per // 2), ('chunk_last', per - 1), ('chunk_first', 0))}.items()):
            t = (5 if q > 1024 else 3) * per + o
            out.append(('redo_runs', 'len%d_%s_at%d' % (L, where, t), s, HC.runs(redo_layout(q, t, L), 1, 2)))
    out.append(('redo_one_run', 'whole_q', s, np.full(q, 777)))
    out.append(('redo_two_runs', 'halves', s, np.repeat([-1765, 123], [q // 2, q - q // 2])))
    third = np.full(q, 123); third[::3] = 1001 + 2 * np.arange(len(third[::3]))
    out.append(('redo_heavy_value', 'every_third_distinct', s, third))
    out.append(('redo_no_ties', 'distinct', s, 1 + 2 * np.arange(q)))
    return out


def wide_redo_cases():
    if 'redo' not in _CACHE:
        rng = np.random.default_rng(2039)
        out = []
        for i, (m, q) in enumerate(REDO_SIZES):
            emit(out, rng, gen_redo(m, q, rng), i % 2, 'f32')
        _CACHE['redo'] = out
    return _CACHE['redo']


def redo_certain(case):
    """enough for the redo list: Q has at least REDO_HITS samples more than distinct values (each finds its bitmap bit set), and S
    has a sample off the grid (the bitmap form runs).  The bound is a lower one: two values may share a bit as well."""
    a, b = HC.values(case, 'f32')
    s, q = (b, a) if len(b) < len(a) else (a, b)
    off_grid = np.any(np.rint(s.astype(np.float64) * 1000) / 1000 != s.astype(np.float64))
    return bool(off_grid and len(q) - len(np.unique(q)) >= REDO_HITS)


REDO_LOOP_SIZES = ((3, 400), (7, 528))


def redo_loop_pools():
    """the smallest positions the redo list takes (a Q of 352 equal samples is the least): for wide_redo_kernel's persistent loop"""
    if 'redo_loop' not in _CACHE:
        rng = np.random.default_rng(351)
        pools = []
        for m, q in REDO_LOOP_SIZES:
            s = np.array([2, 6, 10, 14, 18, 22, 26][:m])
            gen = [('redo_one_run', 'whole_q', s, np.full(q, 777)), ('redo_two_runs', 'near_halves', s, np.repeat([-1765, 123], [q // 2 - 1, q - q // 2 + 1])),
                   ('redo_sixteens', 'runs_of_16', s, HC.runs([16] * (q // 16), 1, 2)), ('redo_heavy_value', 'one_single_first', s, np.r_[-99, np.full(q - 1, 5)])]
            lst = []
            emit(lst, rng, gen, len(pools) % 2, 'f32')
            pools.append(lst)
        _CACHE['redo_loop'] = pools
    return _CACHE['redo_loop']


# ---- big_rank_kernel<2>, the float64 redo
F64_SIZES = (1, 2, 3, 64, 200, 4096, 4097, 8193)
F64_LARGE = (5000, 3000)


def _f64_gen(n0, n1, j, rng):
    """group units |u| < 2^12 of an n0 v n1 position, family by j"""
    fam = ('random_wide', 'random_narrow', 'all_equal', 'disjoint', 'pairs_shared')[j % 5]
    if fam == 'random_wide':
        a, b = rng.integers(-4095, 4096, n0), rng.integers(-4095, 4096, n1)
    elif fam == 'random_narrow':
        a, b = rng.integers(-4, 5, n0), rng.integers(-3, 6, n1)
        a[0] = 7                                                            # (never every unit 0: the position stays class 3)
    elif fam == 'all_equal':
        a, b = np.full(n0, 1000), np.full(n1, 1000)                         # (1 + 125 * 2^-37, 125 * 2^-8, 1.0: sums of 8 193 copies are exact)
    elif fam == 'disjoint':                                                 # group 1 below group 2: D = 1
        a, b = -2 - (np.arange(n0) % 4093), 2 + (np.arange(n1) % 4093)
    else:
        a, b = 2 * ((np.arange(n0) // 2) % 2047) - 2000, 2 * ((np.arange(n1) // 2) % 2047) - 2000
    # a group beyond 8 191 samples takes even units: its sum stays below 2^14 with the last bit at 2^-39, exact in any order of
    # summation like the smaller groups' (below 2^13, last bit 2^-40) — the Welch statistic of samples 2^-28 apart around 1.0 would
    # otherwise hang on the last bit of a mean, in the reference as much as in the kernel
    a, b = [np.sign(x) * (np.abs(x) & ~1) if len(x) > 8191 else x for x in (a.astype(np.int64), b.astype(np.int64))]
    return fam, rng.permutation(a), rng.permutation(b)


def f64_cases():
    """-> cases with 'kind': the class-3 positions ('redo') of every size pair and of every size against 5, the large one, and —
    mixed in — float32-exact ('exact') and on-grid ('grid') positions with ties, which must not be redone"""
    if 'f64' not in _CACHE:
        rng = np.random.default_rng(40)
        pairs = [(x, y) for x in F64_SIZES for y in F64_SIZES] + [(x, 5) for x in F64_SIZES] + [(5, x) for x in F64_SIZES] + [F64_LARGE]
        out = []
        for j, (n0, n1) in enumerate(pairs):
            fam, a, b = _f64_gen(n0, n1, j, rng)
            out.append({'family': fam, 'name': 'redo/%s/%dv%d' % (fam, n0, n1), 'a': a, 'b': b, 'kind': 'redo'})
            if j % 4 == 0:
                kind = 'exact' if j % 8 == 0 else 'grid'
                n0, n1 = min(n0, 300), min(n1, 300)
                fam, a, b = _f64_gen(n0, n1, j // 4, rng)
                out.append({'family': fam, 'name': '%s/%s/%dv%d' % (kind, fam, n0, n1), 'a': a, 'b': b, 'kind': kind})
        _CACHE['f64'] = out
    return _CACHE['f64']


def f64_loop_pool():
    """5 v 7 doubles of every family, for the float64 redo's persistent loop"""
    if 'f64_loop' not in _CACHE:
        rng = np.random.default_rng(57)
        out = []
        for j in range(10):
            fam, a, b = _f64_gen(5, 7, j, rng)
            out.append({'family': fam, 'name': 'redo/%s/5v7/%d' % (fam, j), 'a': a, 'b': b, 'kind': 'redo'})
        _CACHE['f64_loop'] = out
    return _CACHE['f64_loop']


# ---- the persistent loops
def sizes_of(c):
    return len(c['a']), len(c['b'])


def persistent_batch(pools, G, n, after=None):
    """-> [cases] of n positions for a launch of G blocks that stride over the list: the block that takes position i takes i + G
    next.  pools: one case list per size; positions i and i + G differ in family and, with more than one pool, in size.  after:
    {family: family} — the position behind one of the first family is of the second where the pool has it (all-tied behind
    distinct, an empty hash table behind a full one)."""
    after = after or {}
    ptr = [0] * len(pools)
    out, pool_of = [], []
    for i in range(n):
        prev = out[i - G] if i >= G else None
        order = [(i + k) % len(pools) for k in range(len(pools))]
        if prev is not None and len(pools) > 1:
            order = [p for p in order if p != pool_of[i - G]]
        want = after.get(prev['family']) if prev is not None else None
        pick = None
        for fam_ok in ((lambda c: c['family'] == want), (lambda c: True)):
            for p in order:
                for k in range(len(pools[p])):
                    c = pools[p][(ptr[p] + k) % len(pools[p])]
                    if fam_ok(c) and (prev is None or c['family'] != prev['family']) and (not out or c['family'] != out[-1]['family'] or len(pools[p]) < 3):
                        pick = (p, (ptr[p] + k) % len(pools[p]))
                        break
                if pick:
                    break
            if pick:
                break
        assert pick is not None, i
        p, k = pick
        ptr[p] = (k + 1) % len(pools[p])
        out.append(pools[p][k]); pool_of.append(p)
    return out


def big_rank_loop_pools(dtype):
    return [size_cases(3, 4097, dtype)[(3, 4097)], size_cases(1025, 2049, dtype)[(1025, 2049)]]


def big_rank_ks_loop_pools(dtype):
    return [size_cases(2049, 2049, dtype)[(2049, 2049)]]


def big_hist_loop_pools(dtype):
    cases = big_hist_cases(dtype)
    return [[c for c in cases if sizes_of(c) in ((m, q), (q, m)) and c['family'] != 'size_matrix'] for m, q in ((257, 2049), (1024, 4096))]


LOOP_AFTER = {'end_bin_hi': 'all_equal', 'one_bin': 'all_equal', 'hash_table': 'all_equal', 'redo_no_ties': 'redo_one_run', 'disjoint': 'all_equal'}
