"""-m gpu: nmod_pivot_reads / nmod_select_tested / nmod_gather_tested (read_pivot.hip) past the sizes and at the edges where
they take another path, on constructed reads: more scanned entries than one round of scan_tops_kernel, more reads than the
place grid, rows at every step of the row ranking, the top of the 40-bit position range, window edges, rejected tables, the
dtype word decided by one sample and the float64 pass-through threshold.

The pivot is held to tests/pivot_ref.py (held to fast5_ingest.GroupBuilder by test_pivot_ref.py), select and gather to
cli.select_positions on the reference groups.  Every expected array is unique (read order, exact integers, exact float64
values) and every comparison is exact; every test that exists to cross a size step asserts first that it does
(tests/size_steps.py)."""
import ctypes as C

import numpy as np
import pytest

import pivot_ref as R
import size_steps as Z
from test_read_pivot_gpu import _check_pivot, _quiet

pytestmark = pytest.mark.gpu

TOP = Z.POS_LIMIT - 1
SENT = -0x0123456789ABCDEF          # what the raw calls fill their outputs with
ERR_INVALID_ARG = -1                # NMOD_ERR_INVALID_ARG


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


def _values(rng, n, kind):
    k = rng.integers(-3000, 3000, n)
    return {'f64': k / 1000.0 + rng.normal(0, 1e-7, n), 'f32': (k / 1000.0).astype(np.float32), 'i16': k.astype(np.int16)}[kind]


def _reads(rng, chrom, strand, start, lens, kind):
    lens = np.asarray(lens, dtype=np.int64)
    off = np.zeros(len(lens) + 1, np.int64); off[1:] = np.cumsum(lens)
    return dict(chrom=np.asarray(chrom), strand=np.asarray(strand), start=np.asarray(start, dtype=np.int64), off=off,
                norm_mean=_values(rng, int(off[-1]), kind), base=rng.choice(np.array(list(b'ACGT'), dtype=np.uint8), int(off[-1])).view('S1'))


def _pivot_twice(nm, reads, lo=None, hi=None, names=None):
    p = nm.engine.pivot_reads(reads, 0, lo, hi, names=names)
    q = nm.engine.pivot_reads(reads, 0, lo, hi, names=names)
    for k in ('key', 'off', 'sig', 'base'):
        a, b = p[k].cpu().numpy(), q[k].cpu().numpy()
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    return p


def _check_select(nm, d0, d1, e0, e1, min_cov):
    """engine.select_tested on the device groups against cli.select_positions on the reference groups, field by field"""
    from nanomod_amd import cli
    said, esaid = [], []                              # the 'Error not equal' lines carry group 1's bases of the first mismatches
    meta, s0, o0, s1, o1, rid = nm.engine.select_tested(d0, d1, min_cov, log=lambda *a: said.append(a))
    em, es0, eo0, es1, eo1, erid = cli.select_positions(e0, e1, min_cov, 3, lambda *a: esaid.append(a))
    assert [tuple(str(x) for x in a) for a in said] == [tuple(str(x) for x in a) for a in esaid]
    for k in ('chrom', 'strand', 'pos', 'base', 'n0', 'n1'):
        assert np.array_equal(meta[k], em[k]), k
    assert np.array_equal(o0.cpu().numpy(), eo0) and np.array_equal(o1.cpu().numpy(), eo1)
    assert np.array_equal(rid.cpu().numpy(), erid)
    g0, g1 = s0.cpu().numpy(), s1.cpu().numpy()
    assert g0.dtype == g1.dtype == es0.dtype == es1.dtype, (g0.dtype, es0.dtype)
    nan = g0.dtype.kind == 'f'
    assert np.array_equal(g0, es0, equal_nan=nan) and np.array_equal(g1, es1, equal_nan=nan)
    return meta, g0, g1, rid.cpu().numpy()


# ------------------------------------------------------------------------------------------------ long dense span
NAMES3 = ['chrA', 'chrB', 'chrC']
SEAM = Z.SCAN_ONE_ROUND_MAX


def _span_reads(rng, kind, spans, straddle):
    """a few hundred short reads over the (chrom, strand) ids of `spans` ({cs: covered span}); the dense coordinate of the
    pivot is cumulative over them in cs order.  Every span is pinned by a read at its first and at its last position; reads
    straddle chunk seams (dense 4 096 k), end at one and start at one; one read straddles every dense index of `straddle`."""
    cs, start, lens = [], [], []
    cbase = 0
    for c in sorted(spans):
        n, cmin = spans[c], 1000 * (c + 1) + 7

        def add(d0, ln):
            assert cbase <= d0 and d0 + ln <= cbase + n
            cs.append(c); start.append(cmin + d0 - cbase); lens.append(ln)
        add(cbase, 3); add(cbase + n - 2, 2)
        for d0, ln in zip(rng.integers(cbase, cbase + n - 40, 60), rng.integers(1, 40, 60)):
            add(int(d0), int(ln))
        seams = [k for k in range(cbase // Z.SCAN_CHUNK + 1, (cbase + n) // Z.SCAN_CHUNK + 1) if cbase + 16 < Z.SCAN_CHUNK * k < cbase + n - 16]
        for k in rng.choice(seams, min(len(seams), 40), replace=False):
            add(Z.SCAN_CHUNK * int(k) - int(rng.integers(1, 6)), int(rng.integers(6, 12)))
        add(Z.SCAN_CHUNK * seams[0] - 4, 4); add(Z.SCAN_CHUNK * seams[-1], 5)
        for m in straddle:
            if cbase + 16 < m < cbase + n - 16:
                add(m - 7, 20)
        cbase += n
    perm = rng.permutation(len(cs))
    cs, start, lens = np.array(cs)[perm], np.array(start)[perm], np.array(lens)[perm]
    return _reads(rng, np.array(NAMES3)[cs >> 1], np.where(cs & 1, '-', '+'), start, lens, kind)


def _dense(exp):
    """the pivot's dense coordinate of every reference row, the dense start of every (chrom, strand), and S"""
    new = np.r_[True, (exp['chrom'][1:] != exp['chrom'][:-1]) | (exp['strand'][1:] != exp['strand'][:-1])]
    heads = np.flatnonzero(new)
    cmin = np.minimum.reduceat(exp['pos'], heads); cmax = np.maximum.reduceat(exp['pos'], heads)
    cbase = np.r_[0, np.cumsum(cmax - cmin + 1)]
    g = np.cumsum(new) - 1
    return cbase[g] + exp['pos'] - cmin[g], cbase[:-1], int(cbase[-1])


@pytest.mark.parametrize('layout', ['a_strand_starts_at_the_round_seam', 'a_read_straddles_the_round_seam'])
def test_pivot_dense_span_beyond_one_scan_round(nm, layout):
    """S ~ 1.3 M dense positions (28 B of scratch each), almost all of them uncovered: the three scans over them take two
    rounds of scan_tops_kernel.  Three names give six cs; cs 2 (in the middle) and cs 5 (the last) have no read."""
    if layout.startswith('a_strand'):
        spans, straddle = {0: 600000, 1: SEAM - 600000, 3: 150000, 4: 101000}, []
    else:
        spans, straddle = {0: 600000, 1: 500000, 3: 150000, 4: 50000}, [SEAM]
    for kind, seed in (('f64', 41), ('f32', 42), ('i16', 43)):
        reads = _span_reads(np.random.default_rng(seed), kind, spans, straddle)
        exp = R.pivot_ref(reads)
        d, cbase, S = _dense(exp)
        assert S == sum(spans.values()) and S + 1 > Z.SCAN_TOPS_ROUND * Z.SCAN_CHUNK and Z.scan_blocks(S) > Z.SCAN_TOPS_ROUND
        assert len(reads['start']) < 1000 and len(cbase) == 4
        assert ((d % Z.SCAN_CHUNK == Z.SCAN_CHUNK - 1).sum() > 50) and ((d % Z.SCAN_CHUNK == 0).sum() > 50)    # rows on both sides of chunk seams
        assert (d == SEAM - 1).any() and (d == SEAM).any() and (d > SEAM).sum() > 200                          # ... and of the round seam
        if layout.startswith('a_strand'):
            assert SEAM in cbase
        else:
            assert SEAM not in cbase and np.searchsorted(cbase, SEAM - 1, 'right') == np.searchsorted(cbase, SEAM, 'right')
        _check_pivot(_pivot_twice(nm, reads, names=NAMES3), exp)


# ------------------------------------------------------------------------------------------------ more reads than the place grid
def test_pivot_more_reads_than_the_place_grid(nm):
    rng = np.random.default_rng(44)
    nreads = 270000
    assert nreads > Z.PIVOT_GRID_CAP * Z.WAVES
    reads = _reads(rng, np.full(nreads, 'c'), rng.choice(np.array(['+', '-']), nreads), rng.integers(0, 4998, nreads),
                   rng.integers(1, 4, nreads), 'i16')
    exp = R.pivot_ref(reads)
    assert exp['pos'].max() < 5000 and len(exp['pos']) > 9000
    _check_pivot(_pivot_twice(nm, reads), exp)


# ------------------------------------------------------------------------------------------------ row-size steps
ROW_SIZES_SMALL = [1, 2, 63, 64, 65, 127, 128, 129]
ROW_SIZES_LARGE = [960, 1023, 1024, 1025, 1026, 2048, 2049]


@pytest.mark.parametrize('kind', ['f64', 'i16'])
def test_pivot_row_size_steps(nm, kind):
    """one-event reads choose every position's sample count: the slots a lane holds ((n + 63) >> 6), the LDS ranking up to
    kSmallRow and the sorted list of larger rows, small and large rows as neighbours"""
    assert Z.SMALL_ROW in ROW_SIZES_LARGE and Z.SMALL_ROW + 1 in ROW_SIZES_LARGE and Z.SMALL_ROW - 1 in ROW_SIZES_LARGE
    sizes = [s for pair in zip(ROW_SIZES_SMALL, ROW_SIZES_LARGE + [960]) for s in pair][:-1]
    assert sorted(sizes) == sorted(ROW_SIZES_SMALL + ROW_SIZES_LARGE)
    rng = np.random.default_rng(45)
    pos = np.concatenate([np.repeat(100 + np.arange(len(sizes)), sizes), np.repeat(100 + np.arange(len(sizes)), sizes[::-1])])
    strand = np.repeat(np.array(['+', '-']), sum(sizes))
    perm = rng.permutation(len(pos))
    pos, strand = pos[perm], strand[perm]
    reads = _reads(rng, np.full(len(pos), 'c'), strand, pos, np.ones(len(pos), np.int64), kind)
    if kind == 'f64':
        reads['norm_mean'] = rng.permutation(len(pos)) / 8.0            # distinct: a row's order is visible in its values
    exp = R.pivot_ref(reads)
    assert list(np.diff(exp['off'])) == sizes + sizes[::-1]
    p = _pivot_twice(nm, reads)
    _check_pivot(p, exp)
    # the same from the reads directly: a row holds its reads' events in read order, its base is the last read's
    got_sig = p['sig'].cpu().numpy(); got_off = p['off'].cpu().numpy(); got_base = p['base'].cpu().numpy()
    for row in range(2 * len(sizes)):
        mine = np.flatnonzero((strand == '+-'[row >= len(sizes)]) & (pos == 100 + row % len(sizes)))
        assert np.array_equal(got_sig[got_off[row]:got_off[row + 1]], reads['norm_mean'][mine]), row
        assert got_base[row] == reads['base'].view(np.uint8)[mine[-1]], row


# ------------------------------------------------------------------------------------------------ the top of the position range
def _top_reads(rng, kind):
    chrom, strand, start, lens = [], [], [], []
    for name, sd, at_top, deepest in (('c1', '+', True, 6), ('c1', '-', False, 6), ('c2', '-', True, 5), ('c3', '+', False, 4)):
        for ln in range(1, deepest + 1):
            chrom.append(name); strand.append(sd); lens.append(ln); start.append(TOP - ln + 1 if at_top else 0)
    perm = rng.permutation(len(lens))
    pick = lambda x: np.array(x)[perm]
    return _reads(rng, pick(chrom), pick(strand), pick(start), pick(lens), kind)


def test_pivot_and_select_at_the_top_of_the_position_range(nm):
    names = ['c1', 'c2', 'c3']
    rng = np.random.default_rng(46)
    r0, r1 = _top_reads(rng, 'i16'), _top_reads(rng, 'i16')
    e0, e1 = R.pivot_ref(r0), R.pivot_ref(r1)
    ramp = [1, 2, 3, 4, 5, 6] + [6, 5, 4, 3, 2, 1] + [1, 2, 3, 4, 5] + [4, 3, 2, 1]
    assert list(np.diff(e0['off'])) == ramp and e0['pos'][5] == TOP and e0['pos'][6] == 0 and e0['pos'][16] == TOP and e0['pos'][17] == 0
    p0, p1 = _pivot_twice(nm, r0, names=names), _pivot_twice(nm, r1, names=names)
    _check_pivot(p0, e0); _check_pivot(p1, e1)
    key = p0['key'].cpu().numpy()
    assert key[5] == TOP and key[6] == Z.POS_LIMIT and key[16] == (3 << 40) | TOP and key[17] == 4 << 40
    assert list(np.diff(p0['off'].cpu().numpy())) == ramp
    # select: rows (cs, 2^40 - 1) and (cs + 1, 0) are one key apart and still two runs
    meta, _, _, rid = _check_select(nm, p0, p1, e0, e1, 1)
    assert len(rid) == len(ramp)
    assert list(rid) == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3]


def _raw_pivot(nm, cs, start, roff, nev, ncs, cap, rows_room, kind='i16', lo=-1, hi=-1):
    """nmod_pivot_reads itself on device tables as given; the outputs, pre-filled, have room for rows_room rows whatever cap says"""
    import torch
    L = nm._lib
    dev = torch.device('cuda', 0)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)
    rng = np.random.default_rng(1)
    d_cs, d_start, d_off = t(cs, np.int32), t(start, np.int64), t(roff, np.int64)
    val = _values(rng, nev, kind)
    d_val, d_base = t(val, val.dtype), t(rng.choice(np.array(list(b'ACGT'), dtype=np.uint8), nev), np.uint8)
    key = torch.full((rows_room + 1,), SENT, dtype=torch.int64, device=dev); off = torch.full((rows_room + 2,), SENT, dtype=torch.int64, device=dev)
    sig = torch.full((nev + 1,), 77, dtype=d_val.dtype, device=dev); base = torch.full((rows_room + 1,), 0x5A, dtype=torch.uint8, device=dev)
    npos, nsamp = C.c_int64(-5), C.c_int64(-5)
    prm = L.make_params(device=0, memspace=L.MEM_DEVICE, dtype=nm.engine._dtype_code(val.dtype), stream=torch.cuda.current_stream(dev).cuda_stream)
    rc = L.load().nmod_pivot_reads(C.byref(prm), len(start), ncs, d_cs.data_ptr(), d_start.data_ptr(), d_off.data_ptr(), d_val.data_ptr(),
                                   d_base.data_ptr(), lo, hi, cap, key.data_ptr(), off.data_ptr(), sig.data_ptr(), base.data_ptr(),
                                   C.byref(npos), C.byref(nsamp))
    torch.cuda.synchronize()
    untouched = bool((key == SENT).all() and (off == SENT).all() and (sig == 77).all() and (base == 0x5A).all())
    return rc, npos.value, nsamp.value, untouched, (key, off, sig, base)


def test_pivot_rejects_positions_at_and_beyond_the_limit(nm):
    L = nm._lib
    rng = np.random.default_rng(47)
    ok = _reads(rng, ['c', 'c'], ['+', '-'], [TOP - 4, 3], [5, 4], 'i16')
    assert len(nm.engine.pivot_reads(ok)['key']) == 9
    for start, ln in ((TOP - 4, 6), (Z.POS_LIMIT, 1)):           # the last position would be 2^40; the start is 2^40
        for sd in ('+', '-'):
            bad = _reads(rng, ['c', 'c'], [sd, '-'], [start, 3], [ln, 4], 'i16')
            with pytest.raises(L.NanomodLibraryError):
                nm.engine.pivot_reads(bad)
            rc, npos, nsamp, untouched, _ = _raw_pivot(nm, [0 if sd == '+' else 1, 1], [start, 3], [0, ln, ln + 4], ln + 4, 2, 16, 16)
            assert rc == ERR_INVALID_ARG and npos == 0 and nsamp == 0 and untouched
    rc, npos, nsamp, untouched, _ = _raw_pivot(nm, [0, 1], [TOP - 4, 3], [0, 5, 9], 9, 2, 16, 16)      # the same call on good tables
    assert rc == 0 and npos == 9 and nsamp == 9 and not untouched


# ------------------------------------------------------------------------------------------------ window edges
def test_pivot_window_edges(nm):
    """the inclusive event window: a read that touches it with exactly its first or its last event on either strand, reads
    outside it, a window of one position, one that starts at 0, one that leaves nothing (npos = 0, off = [0])"""
    rng = np.random.default_rng(48)
    chrom = ['c1'] * 8 + ['c2'] * 3
    strand = ['+', '+', '-', '-', '+', '-', '+', '-', '+', '-', '-']
    start = [60, 46, 46, 60, 61, 10, 40, 48, 0, 70, 0]
    lens = [5, 5, 5, 5, 3, 40, 30, 6, 50, 9, 2]
    for kind in ('f64', 'i16'):
        reads = _reads(rng, chrom, strand, start, lens, kind)
        for lo, hi, npos in ((50, 60, 16), (50, 50, 2), (60, 60, 2), (0, 46, None), (0, 0, 2), (None, 46, None), (61, None, None), (200, 300, 0)):
            exp = R.pivot_ref(reads, lo, hi)
            if npos is not None:
                assert len(exp['pos']) == npos, (lo, hi, len(exp['pos']))
            p = _pivot_twice(nm, reads, lo, hi, names=['c1', 'c2'])
            _check_pivot(p, exp)
            if npos == 0:
                assert p['key'].numel() == 0 and p['sig'].numel() == 0 and p['off'].cpu().tolist() == [0]
    # [50, 60]: the '+' read from 60 gives its first event, the one to 50 its last; on '-' the other way round
    reads = _reads(rng, chrom, strand, start, lens, 'f64')
    p = nm.engine.pivot_reads(reads, 0, 50, 60, names=['c1', 'c2'])
    key, off, sig = p['key'].cpu().numpy(), p['off'].cpu().numpy(), p['sig'].cpu().numpy()
    v, ro = reads['norm_mean'], reads['off']
    row = lambda k: list(sig[off[np.flatnonzero(key == k)[0]]:off[np.flatnonzero(key == k)[0] + 1]])
    assert row(60) == [v[ro[0]], v[ro[6] + 20]] and row(50) == [v[ro[1] + 4], v[ro[6] + 10]]
    assert row((1 << 40) | 50) == [v[ro[2]], v[ro[7] + 3]] and row((1 << 40) | 60) == [v[ro[3] + 4]]


# ------------------------------------------------------------------------------------------------ rejected tables
def test_pivot_rejects_bad_tables(nm):
    """rp_check_kernel reads cs / start / roff of its own read only and returns before it indexes anything by them (the per-cs
    atomics come after the check), the host stops on the error word before any other launch, and the row count is compared with
    cap_pos before rp_rows_kernel writes a row: none of these calls can index through a value it rejects."""
    good = dict(cs=[0, 1, 3, 0], start=[5, 7, 2, 6], roff=[0, 4, 6, 11, 14])
    exact = rows = 4 + 2 + 5                                # cs 0 covers 5..8 and 6..8: 4 rows; cs 1: 7..8; cs 3: 2..6
    rc, npos, nsamp, untouched, _ = _raw_pivot(nm, good['cs'], good['start'], good['roff'], 14, 4, exact, rows)
    assert rc == 0 and npos == exact and nsamp == 14 and not untouched
    bad = {'cs == ncs': dict(cs=[0, 1, 4, 0]), 'cs == -1': dict(cs=[0, -1, 3, 0]), 'roff[0] != 0': dict(roff=[1, 4, 6, 11, 14]),
           'roff decreases': dict(roff=[0, 6, 4, 11, 14]), 'a negative start': dict(start=[5, -1, 2, 6])}
    for what, change in bad.items():
        tab = dict(good, **change)
        rc, npos, nsamp, untouched, _ = _raw_pivot(nm, tab['cs'], tab['start'], tab['roff'], 14, 4, exact, rows)
        assert rc == ERR_INVALID_ARG and npos == 0 and nsamp == 0 and untouched, what
    rc, npos, nsamp, untouched, _ = _raw_pivot(nm, good['cs'], good['start'], good['roff'], 14, 4, exact - 1, rows)
    assert rc == ERR_INVALID_ARG and npos == 0 and nsamp == 0 and untouched, 'cap_pos one below the row count'


def test_select_rejects_bad_offsets(nm):
    """rp_check_off_kernel reads off[i] and off[i - 1] and indexes nothing by them; the host stops on its error word before
    rp_match_kernel runs"""
    import torch
    L = nm._lib
    rng = np.random.default_rng(49)
    n = 40
    g = dict(chrom=np.full(n, 'c'), strand=np.full(n, '+'), pos=np.arange(n), base=np.full(n, 'A'), off=np.arange(0, 3 * n + 1, 3, dtype=np.int64),
             sig=_values(rng, 3 * n, 'f32'))
    d = nm.engine.group_to_device(g, ['c'])
    dev = d['key'].device

    def call(off0, off1, nsig1=3 * n):
        rows0 = torch.full((n + 1,), SENT, dtype=torch.int64, device=dev); rows1 = rows0.clone(); oo0 = rows0.clone(); oo1 = rows0.clone()
        nt, ns0, ns1, odt = C.c_int64(-5), C.c_int64(-5), C.c_int64(-5), C.c_int32(-5)
        prm = L.make_params(device=0, memspace=L.MEM_DEVICE, dtype=L.DTYPE_F32, stream=torch.cuda.current_stream(dev).cuda_stream)
        o0, o1 = torch.from_numpy(np.asarray(off0, np.int64)).to(dev), torch.from_numpy(np.asarray(off1, np.int64)).to(dev)
        rc = L.load().nmod_select_tested(C.byref(prm), 1, n, d['key'].data_ptr(), o0.data_ptr(), d['sig'].data_ptr(), 3 * n,
                                         n, d['key'].data_ptr(), o1.data_ptr(), d['sig'].data_ptr(), nsig1, n, rows0.data_ptr(),
                                         rows1.data_ptr(), oo0.data_ptr(), oo1.data_ptr(), C.byref(nt), C.byref(ns0), C.byref(ns1), C.byref(odt))
        torch.cuda.synchronize()
        untouched = bool((rows0 == SENT).all() and (rows1 == SENT).all() and (oo0 == SENT).all() and (oo1 == SENT).all())
        return rc, nt.value, untouched
    good = g['off']
    rc, nt, untouched = call(good, good)
    assert rc == 0 and nt == n and not untouched
    dec = good.copy(); dec[17] = dec[16] - 1                        # decreases (and stays within [0, nsig])
    short = good.copy(); short[-1] -= 1                             # non-decreasing, ends one before nsig
    first = good.copy(); first[0] = 1
    for what, (a, b) in {'off0 decreases': (dec, good), 'off1 decreases': (good, dec), 'off1 ends before nsig': (good, short),
                         'off0 ends before nsig': (short, good), 'off0[0] != 0': (first, good)}.items():
        rc, nt, untouched = call(a, b)
        assert rc == ERR_INVALID_ARG and nt == 0 and untouched, what
    rc, nt, untouched = call(good, good, nsig1=3 * n + 1)
    assert rc == ERR_INVALID_ARG and nt == 0 and untouched, 'nsig beyond the last offset'


# ------------------------------------------------------------------------------------------------ more rows than one scan round
@pytest.fixture(scope='module')
def many_rows():
    """two groups of ~1.3 M / ~1.1 M rows of 1 or 2 samples over six (chrom, strand): gaps of 2 and 5 between positions break the
    runs often; group 2 lacks every 7th key of group 1 and has keys of its own, in the gaps and past the ends"""
    rng = np.random.default_rng(50)
    per_cs = 217000
    parts0, parts1 = [], []
    for c in range(6):
        step = rng.choice(np.array([1, 1, 1, 1, 1, 1, 2, 5]), per_cs)
        p = 10 + np.cumsum(step)
        kept = p[np.arange(per_cs) % 7 != 3]
        own = np.concatenate([p[step == 5][::3] - 2, p[-1] + 3 + 2 * np.arange(500)])
        parts0.append((c, p)); parts1.append((c, np.unique(np.concatenate([kept, own]))))

    def group(parts, seed):
        r = np.random.default_rng(seed)
        cs = np.concatenate([np.full(len(p), c) for c, p in parts]); pos = np.concatenate([p for _, p in parts])
        lens = r.integers(1, 3, len(pos))
        off = np.zeros(len(pos) + 1, np.int64); off[1:] = np.cumsum(lens)
        k = r.integers(-3000, 3000, off[-1]).astype(np.int16)
        return dict(chrom=np.array(NAMES3)[cs >> 1], strand=np.where(cs & 1, '-', '+'), pos=pos.astype(np.int64),
                    base=r.choice(np.array(list('ACGT')), len(pos)), off=off, sig=k.astype(np.float64) / 1000.0), k, (cs.astype(np.int64) << 40) | pos
    (e0, k0, key0), (e1, k1, key1) = group(parts0, 51), group(parts1, 52)
    return e0, e1, k0, k1, key0, key1


@pytest.mark.parametrize('min_cov', [1, 2])
def test_select_and_gather_beyond_one_scan_round(nm, many_rows, min_cov):
    e0, e1, k0, k1, key0, key1 = many_rows
    npos0 = len(e0['pos'])
    both = np.isin(key0, key1)
    assert npos0 > Z.SCAN_ONE_ROUND_MAX and Z.scan_blocks(npos0) > Z.SCAN_TOPS_ROUND and both.sum() > Z.SCAN_ONE_ROUND_MAX
    d0 = nm.engine.group_to_device(dict(e0, sig=k0), NAMES3)
    d1 = nm.engine.group_to_device(dict(e1, sig=k1), NAMES3)
    meta, g0, g1, rid = _check_select(nm, d0, d1, e0, e1, min_cov)
    nt = len(rid)
    if min_cov == 1:
        assert nt == both.sum() and nt > Z.SCAN_ONE_ROUND_MAX
    else:
        assert nt < Z.SCAN_ONE_ROUND_MAX < npos0 and nt > 100000
    assert g0.dtype == np.int16 and rid[-1] > nt // 10                 # runs break often
    # the rows themselves, from nmod_select_tested directly
    import torch
    L = nm._lib
    dev = d0['key'].device
    keep0, keep1 = np.flatnonzero(np.diff(e0['off']) >= min_cov), np.flatnonzero(np.diff(e1['off']) >= min_cov)
    common, i0, i1 = np.intersect1d(key0[keep0], key1[keep1], assume_unique=True, return_indices=True)
    cap = min(npos0, len(key1))
    rows0 = torch.full((cap,), -1, dtype=torch.int64, device=dev); rows1 = rows0.clone()
    oo0 = torch.full((cap + 1,), -1, dtype=torch.int64, device=dev); oo1 = oo0.clone()
    cnt, ns0, ns1, odt = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    prm = L.make_params(device=0, memspace=L.MEM_DEVICE, dtype=L.DTYPE_I16_MILLI, stream=torch.cuda.current_stream(dev).cuda_stream)
    rc = L.load().nmod_select_tested(C.byref(prm), min_cov, npos0, d0['key'].data_ptr(), d0['off'].data_ptr(), d0['sig'].data_ptr(), d0['sig'].numel(),
                                     len(key1), d1['key'].data_ptr(), d1['off'].data_ptr(), d1['sig'].data_ptr(), d1['sig'].numel(), cap,
                                     rows0.data_ptr(), rows1.data_ptr(), oo0.data_ptr(), oo1.data_ptr(), C.byref(cnt), C.byref(ns0), C.byref(ns1),
                                     C.byref(odt))
    torch.cuda.synchronize()
    assert rc == 0 and cnt.value == nt == len(common) and odt.value == L.DTYPE_I16_MILLI
    assert np.array_equal(rows0.cpu().numpy()[:nt], keep0[i0]) and np.array_equal(rows1.cpu().numpy()[:nt], keep1[i1])
    assert bool((rows0[nt:] == -1).all()) and bool((oo0[nt + 1:] == -1).all()) and bool((oo1[nt + 1:] == -1).all())
    assert ns0.value == int(oo0[nt]) == len(g0) and ns1.value == int(oo1[nt]) == len(g1)


# ------------------------------------------------------------------------------------------------ one sample decides the dtype
LENS0 = [6, 7, 2, 9, 64, 5, 8, 3, 65, 7, 128, 4]
LENS1 = [5, 9, 6, 2, 70, 6, 5, 8, 3, 129, 128, 2]
MIN_COV = 5                       # tested rows: 0, 1, 4, 5, 6, 9, 10; row 10 of group 2 has 128 samples: its last one sits in lane 63
CHANGES = [(None, 'float32'), (0.001, 'int16'), (32.768, 'float64'), (32.767, 'int16'), (0.1 + 1e-9, 'float64'), (float('nan'), 'float64')]


def _small_group(rng, lens, mult=1):
    n = len(lens)
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum(lens)
    k = 125 * rng.integers(-200, 200, off[-1]) * mult
    return dict(chrom=np.full(n, 'c'), strand=np.full(n, '+'), pos=100 + np.arange(n), base=rng.choice(np.array(list('ACGT')), n), off=off,
                sig=k / 1000.0), k


def _select_dtype(nm, e0, e1, sig0=None, sig1=None):
    """the output dtype for reference groups e0 / e1 (exact float64 values), uploaded as sig0 / sig1 when given"""
    d0 = nm.engine.group_to_device(dict(e0, sig=e0['sig'] if sig0 is None else sig0), ['c'])
    d1 = nm.engine.group_to_device(dict(e1, sig=e1['sig'] if sig1 is None else sig1), ['c'])
    meta, g0, g1, rid = _check_select(nm, d0, d1, e0, e1, MIN_COV)
    assert list(meta['pos'] - 100) == [0, 1, 4, 5, 6, 9, 10]
    return str(g0.dtype)


@pytest.mark.parametrize('value,want', CHANGES)
def test_select_dtype_decided_by_one_sample(nm, value, want):
    """float64 rows, all float32-exact and on the 0.001 grid (multiples of 0.125) but for one sample; the expected dtype and
    values are detect.encode_pair's (through cli.select_positions) on the exact values"""
    rng = np.random.default_rng(53)
    (b0, _), (b1, _) = _small_group(rng, LENS0), _small_group(rng, LENS1)
    last_tested1 = b1['off'][11] - 1
    assert last_tested1 - b1['off'][10] == 127
    for grp, at in ((1, last_tested1), (0, 0)):
        e0, e1 = dict(b0, sig=b0['sig'].copy()), dict(b1, sig=b1['sig'].copy())
        if value is not None:
            (e1 if grp else e0)['sig'][at] = value
        assert _select_dtype(nm, e0, e1) == want, (grp, at)
    # the same sample in a row below min_coverage does not decide anything: group 2's last row, group 1's row 2, group 2's row 3
    for grp, at in ((1, len(b1['sig']) - 1), (0, b0['off'][2]), (1, b1['off'][3])):
        e0, e1 = dict(b0, sig=b0['sig'].copy()), dict(b1, sig=b1['sig'].copy())
        if value is not None:
            (e1 if grp else e0)['sig'][at] = value
        assert _select_dtype(nm, e0, e1) == 'float32', (grp, at)


def test_select_dtype_of_int16_and_mixed_input(nm):
    rng = np.random.default_rng(54)
    (e0, k0), (e1, k1) = _small_group(rng, LENS0), _small_group(rng, LENS1)
    i16 = lambda k: k.astype(np.int16)
    assert np.abs(k0).max() <= 32767 and np.abs(k1).max() <= 32767
    # every k a multiple of 125: float32 holding k / 1000 exactly (compared inside _check_select)
    assert _select_dtype(nm, e0, e1, i16(k0), i16(k1)) == 'float32'
    # one other k in the last lane of the last tested row, or in the first sample: int16; in an untested row: float32 still
    for grp, at, want in ((1, e1['off'][11] - 1, 'int16'), (0, 0, 'int16'), (1, len(k1) - 1, 'float32'), (0, e0['off'][2], 'float32')):
        c0, c1 = k0.copy(), k1.copy()
        (c1 if grp else c0)[at] = 1234
        assert _select_dtype(nm, dict(e0, sig=c0 / 1000.0), dict(e1, sig=c1 / 1000.0), i16(c0), i16(c1)) == want, (grp, at)
    # one group int16, the other float32: the wrapper hands both over as exact float64 values
    f1 = e1['sig'].astype(np.float32)
    assert np.array_equal(f1.astype(np.float64), e1['sig'])
    assert _select_dtype(nm, e0, e1, i16(k0), f1) == 'float32'
    c0 = k0.copy(); c0[0] = 1234                                      # 1.234: on the grid, not float32-exact
    assert _select_dtype(nm, dict(e0, sig=c0 / 1000.0), e1, i16(c0), f1) == 'int16'
    f1 = f1.copy(); f1[e1['off'][11] - 1] = np.float32(0.1)           # float32(0.1): float32-exact, off the grid
    x1 = dict(e1, sig=f1.astype(np.float64))
    assert _select_dtype(nm, e0, x1, i16(k0), f1) == 'float32'
    assert _select_dtype(nm, dict(e0, sig=c0 / 1000.0), x1, i16(c0), f1) == 'float64'


# ------------------------------------------------------------------------------------------------ the pass-through threshold
@pytest.mark.parametrize('extra,want', [(0, 'float32'), (1, 'float64')])
def test_select_float64_pass_through_threshold(nm, extra, want):
    """float64 groups, every value float32-exact: up to kDeviceEncodeAbove tested samples over both groups the dtype is decided
    (float32), one more and the float64 values pass through unchanged.  A row below min_coverage in each group is not counted."""
    rng = np.random.default_rng(55)
    rows = Z.DEVICE_ENCODE_ABOVE // 2000
    lens0 = np.r_[np.full(rows, 1000), 3]; lens1 = np.r_[np.full(rows, 1000), 3]
    lens1[rows // 2] += extra

    def group(lens):
        off = np.zeros(len(lens) + 1, np.int64); off[1:] = np.cumsum(lens)
        return dict(chrom=np.full(len(lens), 'c'), strand=np.full(len(lens), '+'), pos=100 + np.arange(len(lens)),
                    base=rng.choice(np.array(list('ACGT')), len(lens)), off=off, sig=rng.integers(-200, 200, off[-1]) * 0.125)
    e0, e1 = group(lens0), group(lens1)
    tested = int(lens0[:rows].sum() + lens1[:rows].sum())
    assert tested == Z.DEVICE_ENCODE_ABOVE + extra and len(e0['sig']) + len(e1['sig']) > Z.DEVICE_ENCODE_ABOVE + 1
    d0, d1 = nm.engine.group_to_device(e0, ['c']), nm.engine.group_to_device(e1, ['c'])
    meta, g0, g1, rid = _check_select(nm, d0, d1, e0, e1, MIN_COV)
    assert len(rid) == rows and len(g0) + len(g1) == tested and str(g0.dtype) == want
