"""GPU: nmod_read_class_rows / nmod_read_classes_step (K22) against tests/classes_ref.py: the rows exactly; a step on constructed reads
against the device-order restatement (integers exactly) and against mpmath within the derived gates; the sums as the fixed-order sums
of the device's own per-read values; invariances as identical bytes; batches larger than the grids; the stream contract; the refusals;
the fit through the device against the restatement's loop; the chain K13 -> K22 through readllr.cluster_reads_llr and `cli readclasses`."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import classes_ref as K
import hmm_ref as H
import read_batch_cases as RB
import stream_cases as S
from nanomod_amd import _lib as L
from test_site_pairs import _key

pytestmark = pytest.mark.gpu

WALK = ('cs', 'start', 'roff', 'score', 'key')
ROWS = L.CLASS_ROWS_FIELDS
READ = L.CLASSES_READ_FIELDS
ALL = READ + L.CLASSES_SITE_FIELDS + ('w_out', 'sums')
SEAM_M = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099]
SEAM_ROWS = [L.CLASSES_SMALL - 1, L.CLASSES_SMALL, L.CLASSES_SMALL + 1, L.CLASSES_WAVE - 1, L.CLASSES_WAVE, L.CLASSES_WAVE + 1]


def same(a, b):
    """identical bytes (a -0.0 is not a 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _engine():
    from nanomod_amd import engine
    return engine


@pytest.fixture(scope='module')
def det():
    return _engine().DeviceDetector(0)


def _case(reads, key):
    """reads: (cs, start, scores) triples; the flat arrays of the entries"""
    cs = np.array([r[0] for r in reads], np.int32)
    start = np.array([r[1] for r in reads], np.int64)
    roff = np.zeros(len(reads) + 1, np.int64)
    roff[1:] = np.cumsum([len(r[2]) for r in reads])
    score = np.concatenate([np.asarray(r[2], np.float64) for r in reads]) if reads else np.zeros(0)
    return dict(cs=cs, start=start, roff=roff, score=score, key=np.asarray(key, np.int64))


def _device_rows(det, c):
    """read_sites and read_class_rows on device tensors of case c -> (rows as tensors, hoff tensor)"""
    import torch
    t = [torch.from_numpy(c[f]).cuda() for f in WALK]
    hoff, nrows = det.read_sites(*t)
    return det.read_class_rows(*t, hoff, nrows), hoff


def _rows_np(rows, hoff):
    return dict({f: v.cpu().numpy() for f, v in rows.items()}, hoff=hoff.cpu().numpy())


def _rows_dev(rows):
    import torch
    return {f: torch.from_numpy(np.ascontiguousarray(rows[f])).cuda() for f in ROWS}, torch.from_numpy(np.ascontiguousarray(rows['hoff'])).cuda()


def _step(det, rows_t, hoff_t, theta, w, **kw):
    import torch
    res = det.read_classes_step(rows_t, hoff_t, torch.from_numpy(np.ascontiguousarray(theta, np.float64).reshape(-1)).cuda(),
                                torch.from_numpy(np.ascontiguousarray(w, np.float64)).cuda(), **kw)
    return {f: v.cpu().numpy() for f, v in res.items()}


def _own_sums(res, hoff, theta):
    """sums and w_out from the device's own per-read and per-site values, in the header's fixed order"""
    sums = K.batch_sums(hoff, res['ll'], res['gamma'], theta, res['theta_out'], res['n_site'])
    return sums, (sums[K.SUMS:] / sums[1] if sums[1] > 0 else None)


# ------------------------------------------------------------------------------------------------------------ constructed reads
VALUES = np.array([0.0, 0.5, -0.5, 40.0, -40.0, 745.0, -745.0, 3.0, -2.0, 1.0])
INVALID = np.array([np.nan, np.inf, -np.inf])


@functools.lru_cache(maxsize=None)
def constructed():
    """cs 0: a site at every position 0 .. 4 104, the reads of SEAM_M entries from position 3 and forty reads with invalid scores among
    theirs; cs 1 ('-'): six sites with SEAM_ROWS reads of one event each; cs 2: a site that no read covers, one with a single read, and
    a read that covers no site"""
    rng = np.random.default_rng(2201)
    key = [_key(0, p) for p in range(max(SEAM_M) + 6)] + [_key(1, 100 + 10 * i) for i in range(len(SEAM_ROWS))] + [_key(2, 50), _key(2, 60)]
    reads = [(0, 3, VALUES[rng.integers(0, len(VALUES), m)]) for m in SEAM_M]
    for _ in range(40):
        n = int(rng.integers(1, 70))
        reads.append((0, int(rng.integers(0, 4000)), np.concatenate((VALUES, INVALID))[rng.integers(0, len(VALUES) + len(INVALID), n)]))
    for i, n in enumerate(SEAM_ROWS):
        reads += [(1, 100 + 10 * i, VALUES[rng.integers(0, len(VALUES), 1)]) for _ in range(n)]
    reads += [(2, 58, np.array([1.5, np.nan, 2.5])), (2, 70, np.full(20, 3.0)), (2, 50, np.array([np.inf]))]
    order = rng.permutation(len(reads))                                       # (the seam reads are not the first reads)
    reads = [reads[i] for i in order]
    c = _case(reads, np.array(key, np.int64))
    c['reads'] = reads
    c['rows'] = K.rows_ref(*[c[f] for f in WALK])
    return c


def _theta(nsites, nc, seed):
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0.02, 0.98, (nsites, nc))
    theta[3:6], theta[6:9] = K.LO, K.HI                                       # both clamps, every class, where every seam read has an entry
    theta[9, ::2], theta[9, 1::2] = K.LO, K.HI
    theta[-8:-2:2], theta[-7:-2:2] = K.LO, K.HI                               # ... and at the sites of the row seams
    return theta, (rng.dirichlet(np.full(nc, 3.0)) if nc > 1 else np.ones(1))


@functools.lru_cache(maxsize=None)
def constructed_ref(nc):
    c = constructed()
    theta, w = _theta(len(c['key']), nc, 2210 + nc)
    return theta, w, K.step_ref(c['rows'], theta, w), K.step_mp(c['rows'], theta, w)


def test_the_rows_are_the_entries_and_their_stable_order_by_site(det):
    import torch
    c = constructed()
    ref = c['rows']
    rows_t, hoff_t = _device_rows(det, c)
    got = _rows_np(rows_t, hoff_t)
    m = np.diff(ref['hoff'])
    assert sorted(m[m > 70].tolist()) == [v for v in SEAM_M if v > 70] and (m == 0).sum() >= 3
    per_site = np.diff(ref['soff'])
    assert per_site[-8:-2].tolist() == SEAM_ROWS and per_site[-2:].tolist() == [0, 1]
    for f in ('hoff',) + ROWS:
        assert same(got[f], ref[f]), f
    t = [torch.from_numpy(c[f]).cuda() for f in WALK]
    k19 = det.read_hmm(*t, hoff_t, len(ref['s']), want=('site',))['site'].cpu().numpy()
    assert same(got['site'], k19)                                             # nmod_read_hmm's site, byte for byte
    # soff and srow against numpy
    soff = np.zeros(len(c['key']) + 1, np.int64)
    soff[1:] = np.cumsum(np.bincount(got['site'], minlength=len(c['key'])))
    assert same(got['soff'], soff) and same(got['srow'], np.argsort(got['site'], kind='stable').astype(np.int32))
    # the host memspace and fewer outputs: the same bytes
    eng = _engine()
    host = eng.read_class_rows_host(*[c[f] for f in WALK])
    for f in ('hoff',) + ROWS:
        assert same(host[f], ref[f]), f
    for want in (('srow',), ('soff',), ('s', 'rread'), ('site', 'soff')):
        part = det.read_class_rows(*t, hoff_t, len(ref['s']), want=want)
        assert set(part) == set(want)
        for f in want:
            assert same(part[f].cpu().numpy(), ref[f]), (want, f)
    part = eng.read_class_rows_host(*[c[f] for f in WALK], ref['hoff'], want=('srow', 'soff'))
    assert same(part['srow'], ref['srow']) and same(part['soff'], ref['soff'])


@pytest.mark.parametrize('nc', range(1, 9))
def test_a_step_on_constructed_reads(det, nc):
    """Measured on one MI355X: against mpmath ll within 0.055, gamma 0.011, theta_out 0.012 and n_site 0.008 of their gates, for every
    C = 1 .. 8 (C = 4 .. 7: ll 0.055, 0.051, 0.053, 0.044; gamma 0.009, 0.008, 0.004, 0.005; theta_out and n_site below 0.008).
    The gate of ll is not a rounding count times sum |g| + S + 1 alone: at a clamped theta with a score of +-40 the definition's
    1 - (1 - th) t cancels to the clamp's 1e-9, and ll is then off by up to 1.96e-10 of sum |g| + S + 1 (printed below) whatever the
    order of operations; classes_ref's gate carries that term, X_U u sum x / (1 - x), derived in its docstring"""
    c = constructed()
    theta, w, a, exact = constructed_ref(nc)
    rows_t, hoff_t = _rows_dev(c['rows'])
    res = _step(det, rows_t, hoff_t, theta, w)
    assert set(res) == set(ALL)
    n = len(c['reads'])
    gamma = res['gamma'].reshape(n, nc)
    # integers and status exactly
    assert same(res['status'], a['status']) and same(res['status'], exact['status'])
    none = res['status'] == L.HMM_NO_SITE
    assert none.sum() >= 3 and np.all(res['cls'][none] == -1) and np.all(gamma[none] == 0.0) and np.all(res['ll'][none] == 0.0)
    ok = K.decided(exact)
    share = 1.0 - ok.sum() / float((~none).sum())
    assert share <= 0.01, 'the gate leaves the class of %.4f of the reads undecided' % share
    assert same(res['cls'][ok], a['cls'][ok]) and np.all(res['cls'][~none] == gamma[~none].argmax(1))
    # floats within the gates of mpmath
    err = K.errors_against_mp(res, exact)
    worst = {f: float(e.max()) for f, e in err.items()}
    rel = np.abs(res['ll'] - np.array([float(v) for v in exact['ll']])) / exact['scale_ll']
    print('C = %d, %d reads, %d rows: the largest errors against mpmath in units of their gates: %s; ll at most %.3g of sum |g| + S + 1; '
          '%d read(s) left to the gate of cls' % (nc, n, len(c['rows']['s']), ', '.join('%s %.3g' % kv for kv in worst.items()), rel.max(),
                                                  int((~ok & ~none).sum())))
    assert all(v <= 1.0 for v in worst.values()), worst
    if nc == 1:
        assert np.all(gamma[~none] == 1.0)
    # the device-order restatement lies as close, and equal where no library function is between them
    assert same(res['sums'][1:3], a['sums'][1:3])
    # sums and weights: the fixed-order sums of the device's own values, byte for byte
    sums, w_out = _own_sums(res, c['rows']['hoff'], theta)
    assert same(res['sums'], sums) and same(res['w_out'], w_out)
    assert sums[1] == (~none).sum() and sums[2] == len(c['rows']['s'])
    # a site without rows keeps its theta and has N = 0
    empty = np.diff(c['rows']['soff']) == 0
    assert empty.sum() >= 1 and same(res['theta_out'].reshape(-1, nc)[empty], theta[empty]) and np.all(res['n_site'].reshape(-1, nc)[empty] == 0.0)
    assert np.all((res['theta_out'] >= K.LO) & (res['theta_out'] <= K.HI))


def test_a_class_that_no_read_prefers_keeps_its_theta(det):
    """classes_ref's case of the CPU suite on the device: 40 scores of +745 per read against theta = 1e-9: gamma underflows to 0"""
    n, ns = 6, 40
    rows = K.rows_from_entries(np.arange(0, (n + 1) * ns, ns, dtype=np.int64), np.tile(np.arange(ns), n), np.full(n * ns, 745.0), ns)
    theta = np.stack((np.full(ns, 0.9), np.full(ns, K.LO)), 1)
    rows_t, hoff_t = _rows_dev(rows)
    res = _step(det, rows_t, hoff_t, theta, np.array([0.5, 0.5]))
    a = K.step_ref(rows, theta, np.array([0.5, 0.5]))
    assert np.all(res['gamma'].reshape(n, 2) == np.array([1.0, 0.0])) and np.all(res['cls'] == 0)
    assert same(res['n_site'].reshape(ns, 2), a['n_site']) and same(res['theta_out'].reshape(ns, 2)[:, 1], theta[:, 1])
    assert np.all(res['theta_out'].reshape(ns, 2)[:, 0] == K.HI) and res['w_out'].tolist() == [1.0, 0.0] and res['sums'][3] == K.HI - 0.9


# ------------------------------------------------------------------------------------------------------------ invariances
def test_host_and_device_memspace_and_fewer_outputs_give_identical_bytes(det):
    c = constructed()
    theta, w, _, _ = constructed_ref(3)
    rows_t, hoff_t = _rows_dev(c['rows'])
    dev = _step(det, rows_t, hoff_t, theta, w)
    eng = _engine()
    host = eng.read_classes_step_host(c['rows'], theta, w)
    for f in ALL:
        assert same(host[f], dev[f]), f
    for want in (('sums',), ('gamma',), ('ll',), ('cls', 'status'), ('theta_out',), ('n_site',), ('w_out',), ('w_out', 'sums'), ('ll', 'theta_out'),
                 ('gamma', 'n_site', 'sums'), ('cls', 'w_out')):
        part = _step(det, rows_t, hoff_t, theta, w, want=want)
        assert set(part) == set(want)
        for f in want:
            assert same(part[f], dev[f]), (want, f)
    part = eng.read_classes_step_host(c['rows'], theta, w, want=('sums', 'theta_out'))
    assert same(part['sums'], dev['sums']) and same(part['theta_out'], dev['theta_out'])
    for nc in (5, 8):                                                         # the slabs that scale with C, where the caller asks for none of their outputs
        theta, w = _theta(len(c['key']), nc, 2210 + nc)
        dev = _step(det, rows_t, hoff_t, theta, w)
        host = eng.read_classes_step_host(c['rows'], theta, w)
        for f in ALL:
            assert same(host[f], dev[f]), (nc, f)
        for want in (('sums',), ('w_out',), ('theta_out',), ('gamma', 'n_site', 'sums')):
            part = _step(det, rows_t, hoff_t, theta, w, want=want)
            assert set(part) == set(want)
            for f in want:
                assert same(part[f], dev[f]), (nc, want, f)


def test_a_permutation_of_the_reads_and_a_larger_batch_change_no_read(det):
    c = constructed()
    nc = 3
    theta, w, _, _ = constructed_ref(nc)
    rows_t, hoff_t = _rows_dev(c['rows'])
    dev = _step(det, rows_t, hoff_t, theta, w, want=READ)
    reads, n = c['reads'], len(c['reads'])
    rng = np.random.default_rng(2202)
    order = rng.permutation(n)
    extra = [(0, int(rng.integers(0, 4000)), VALUES[rng.integers(0, len(VALUES), int(rng.integers(1, 90)))]) for _ in range(300)]
    for batch, idx in (([reads[r] for r in order], order), (extra[:150] + reads + extra[150:], None)):
        rows = K.rows_ref(*[_case(batch, c['key'])[f] for f in WALK])
        bt, bh = _rows_dev(rows)
        got = _step(det, bt, bh, theta, w, want=READ)
        for f in READ:
            full = dev[f].reshape(n, -1)
            part = got[f].reshape(len(batch), -1)
            assert same(part, full[idx]) if idx is not None else same(part[150:150 + n], full), f
    longest = int(np.argmax(np.diff(c['rows']['hoff'])))
    for r in (longest, 7):
        rows = K.rows_ref(*[_case([reads[r]], c['key'])[f] for f in WALK])
        at, ah = _rows_dev(rows)
        alone = _step(det, at, ah, theta, w, want=READ)
        for f in READ:
            assert same(alone[f].reshape(1, -1), dev[f].reshape(n, -1)[r:r + 1]), (r, f)


# ------------------------------------------------------------------------------------------------------------ the grids
def _tile(rows, nsites, times):
    """`times` copies of a set of rows side by side: copy k has its own reads and its own sites"""
    hoff, site = rows['hoff'], rows['site']
    n, m = len(hoff) - 1, len(site)
    t_hoff = np.concatenate(([0], (hoff[1:][None, :] + m * np.arange(times)[:, None]).reshape(-1))).astype(np.int64)
    t_site = (site[None, :].astype(np.int64) + nsites * np.arange(times)[:, None]).reshape(-1)
    return K.rows_from_entries(t_hoff, t_site, np.tile(rows['s'], times), nsites * times)


def test_more_reads_and_sites_than_the_grids_have_units(det):
    """Copies of a small set of rows side by side: every copy's reads and sites have the small set's bytes.  First short reads and
    small sites, more than the classify kernels' strides and the persistent grids of the wave and 16-lane forms; then sites of the wave
    form and of the workgroup form, and reads of the workgroup form, more than their grids"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(2203)
    nc, ns = 2, 24
    cover = rng.random((23, ns)) < 0.06
    cover[0] = False
    hoff = np.zeros(24, np.int64)
    hoff[1:] = np.cumsum(cover.sum(1))
    rr, ss = np.nonzero(cover)
    small = K.rows_from_entries(hoff, ss, rng.normal(0.0, 3.0, len(rr)), ns)
    theta, w = rng.uniform(0.05, 0.95, (ns, nc)), np.array([0.4, 0.6])
    one = K.step_ref(small, theta, w)
    st, sh = _rows_dev(small)
    single = _step(det, st, sh, theta, w)
    assert same(single['cls'], one['cls']) and same(single['status'], one['status'])
    times = (RB.CLASSIFY_READS_PER_CU * cus + 5000) // 23 + 1
    assert 23 * times > RB.CLASSIFY_READS_PER_CU * cus > RB.short_units(cus) and ns * times > 16 * 256 * cus
    big = _tile(small, ns, times)
    bt, bh = _rows_dev(big)
    res = _step(det, bt, bh, np.tile(theta, (times, 1)), w)
    for f in READ + L.CLASSES_SITE_FIELDS:
        per = single[f].reshape(23 if f in READ else ns, -1)
        assert same(res[f].reshape(times, *per.shape), np.broadcast_to(per, (times,) + per.shape)), f
    sums, w_out = _own_sums(res, big['hoff'], np.tile(theta, (times, 1)))
    assert same(res['sums'], sums) and same(res['w_out'], w_out)
    # sites of the wave form (65 rows), of the workgroup form (513 rows and, under the long reads, one per entry), long reads
    top = L.HMM_WAVE_MAX + 1
    n_wave, n_block, n_long = 8 * cus * 4 + 50, 2 * cus + 20, RB.long_units(cus) + 50
    for nc in (2, 7):                                                         # ... and once more with 7 classes: the odd count with the most registers
        if nc != 2:
            theta, w = rng.uniform(0.05, 0.95, (ns, nc)), rng.dirichlet(np.full(nc, 3.0))
        for rows_per, copies in ((L.CLASSES_SMALL + 1, n_wave), (L.CLASSES_WAVE + 1, n_block)):
            unit = K.rows_from_entries(np.arange(rows_per + 1, dtype=np.int64), np.zeros(rows_per, np.int64), rng.normal(0.0, 3.0, rows_per), 1)
            ut, uh = _rows_dev(unit)
            th1 = theta[:1]
            single = _step(det, ut, uh, th1, w, want=('gamma', 'theta_out', 'n_site'))
            ref = K.step_ref(unit, th1, w)
            assert np.allclose(single['theta_out'], ref['theta_out'].reshape(-1), rtol=1e-12) and np.allclose(single['n_site'], ref['n_site'].reshape(-1), rtol=1e-12)
            big = _tile(unit, 1, copies)
            bt, bh = _rows_dev(big)
            res = _step(det, bt, bh, np.tile(th1, (copies, 1)), w, want=('gamma', 'theta_out', 'n_site'))
            for f in ('gamma', 'theta_out', 'n_site'):
                per = single[f].reshape(-1, nc)
                assert same(res[f].reshape(copies, *per.shape), np.broadcast_to(per, (copies,) + per.shape)), (rows_per, f)
        long_unit = K.rows_from_entries(np.array([0, top], np.int64), np.arange(top), rng.normal(0.0, 3.0, top), top)
        th_long = rng.uniform(0.05, 0.95, (top, nc))
        lt, lh = _rows_dev(long_unit)
        single = _step(det, lt, lh, th_long, w, want=READ)
        hoff = np.arange(0, (n_long + 1) * top, top, dtype=np.int64)
        many = K.rows_from_entries(hoff, np.tile(np.arange(top), n_long), np.tile(long_unit['s'], n_long), top)
        mt, mh = _rows_dev(many)
        res = _step(det, mt, mh, th_long, w)
        assert n_long > RB.long_units(cus) and top > 2 * cus
        for f in READ:
            assert same(res[f].reshape(n_long, -1), np.repeat(single[f].reshape(1, -1), n_long, 0)), f
        g = single['gamma'].reshape(1, nc)
        for j in (0, 1, top // 2, top - 1):                                        # a site of n_long equal rows, in the device's order
            N, Mo = K.site_ref(np.full(n_long, long_unit['s'][j]), np.repeat(g, n_long, 0), th_long[j])
            assert same(res['n_site'].reshape(top, nc)[j], N), j
            assert np.allclose(res['theta_out'].reshape(top, nc)[j], np.clip(Mo / N, K.LO, K.HI), rtol=1e-12), j
        assert res['sums'][1] == n_long and res['sums'][2] == n_long * top


# ------------------------------------------------------------------------------------------------------------ the stream
def test_side_stream_and_no_wait_for_the_work_before_it(det):
    """On a side stream the result is the default stream's; and behind a stall of stream_cases.T_MS on a fresh stream (the inputs put in
    place behind the stall, a decoy behind the call: tests/stream_cases.py) the call returns while the stall still runs, and its result
    is the one of the real inputs"""
    import torch
    c = constructed()
    theta, w, _, _ = constructed_ref(2)
    rows_t, hoff_t = _rows_dev(c['rows'])
    want = _step(det, rows_t, hoff_t, theta, w)
    real = dict(s=c['rows']['s'], theta=theta.reshape(-1), w=w)
    decoy = dict(s=-c['rows']['s'], theta=1.0 - theta.reshape(-1), w=w[::-1].copy())
    sw = S.Swapped(real, decoy)
    call = lambda out=None: det.read_classes_step(dict(rows_t, s=sw.t['s']), hoff_t, sw.t['theta'], sw.t['w'], out=out)
    side = torch.cuda.Stream()
    sw.load_real()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        first = call()
    side.synchronize()
    for f in ALL:
        assert same(first[f].cpu().numpy(), want[f]), f
    for _ in range(2):                                                        # (two streams, for stream_cases' reason: hardware queues)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            out = S.fill_sentinel({f: torch.empty_like(v) for f, v in first.items()})
        stream.synchronize()
        with torch.cuda.stream(stream):
            S.stall(stream, S.T_MS)
            event = torch.cuda.Event()
            event.record(stream)
            sw.load_real()
            got = call(out)
            sw.load_decoy()
            early = event.query()
        assert not early, 'the stall of %g ms had ended when the call returned' % S.T_MS
        stream.synchronize()
        for f in ALL:
            assert same(got[f].cpu().numpy(), want[f]), f
        assert sw.holds('decoy')


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    eng = _engine()
    lib = L.load()
    ptr = eng._np_ptr
    rows, _, _ = K.planted_rows(226, n_reads=8, n_sites=5)
    n, ns, nrows, nc = 8, 5, len(rows['s']), 2
    theta, w = np.full(ns * nc, 0.5), np.array([0.5, 0.5])
    host = L.make_params(device=0, memspace=L.MEM_HOST)
    shapes = eng._classes_shapes(ALL, n, ns, nc)
    res = {f: np.full(k, 77, np.dtype(kind)) for f, (kind, k) in shapes.items()}
    untouched = lambda: all(np.all(v == 77) for v in res.values())

    def step(prm=host, nreads=n, nsites=ns, nrows=nrows, opts=None, out=None, theta=theta, w=w, **kw):
        a = dict(rows, **kw)
        opts = opts if opts is not None else L.make_classes_opts(nc)
        out = out if out is not None else L.make_classes_out(**eng._np_ptrs(res))
        return lib.nmod_read_classes_step(C.byref(prm) if prm is not None else None, nreads, nsites, nrows, ptr(a['hoff']), ptr(a['site']), ptr(a['s']),
                                          ptr(a['rread']), ptr(a['soff']), ptr(a['srow']), C.byref(opts) if opts != 'null' else None, ptr(theta), ptr(w),
                                          C.byref(out))
    assert step(None) == -1 and step(L.make_params(device=0, memspace=5)) == -1
    assert step(nreads=-1) == -1 and step(nreads=2 ** 31) == -1 and step(nsites=-1) == -1 and step(nsites=2 ** 31 - 1) == -1
    assert step(nrows=-1) == -1 and step(nrows=2 ** 31) == -1 and step(nrows=nrows + 1) == -1 and step(nrows=nrows - 1) == -1
    for missing in ('hoff', 'site', 's', 'rread', 'soff', 'srow'):
        assert step(**{missing: None}) == -1, missing
    assert step(theta=None) == -1 and step(w=None) == -1 and step(opts='null') == -1
    for bad in (0, 9, -1):
        assert step(opts=L.make_classes_opts(bad)) == -1, bad
    short = L.make_classes_opts(nc); short.struct_size -= 4
    wrong = L.make_classes_out(**eng._np_ptrs(res)); wrong.struct_size += 8
    assert step(opts=short) == -1 and step(out=wrong) == -1
    for bad in (0.0, 1.0, 1e-10, float('nan'), float('inf'), -0.5):
        th = theta.copy(); th[3] = bad
        assert step(theta=th) == -1, bad
    for bad in ([0.5, 0.4], [1.0, 0.0], [0.5, float('nan')], [1.5, -0.5], [0.5 + 1e-8, 0.5]):
        assert step(w=np.array(bad)) == -1, bad
    down = rows['hoff'].copy(); down[n - 1] = down[n] + 1
    assert step(hoff=rows['hoff'] + 1) == -1 and step(hoff=down) == -1
    down = rows['soff'].copy(); down[ns - 1] = down[ns] + 1
    assert step(soff=rows['soff'] + 1) == -1 and step(soff=down) == -1
    assert step(nreads=0, nrows=nrows) == -1 and step(nsites=0, nrows=nrows) == -1
    assert untouched()
    # what is not refused: the call itself; one class with the weight 1; reads without an entry
    assert step() == 0 and not untouched()
    for f in ALL:
        assert same(res[f], eng.read_classes_step_host(rows, theta, w)[f]), f
    one = eng.read_classes_step_host(rows, np.full(ns, 0.5), np.ones(1))
    assert np.all(one['gamma'][one['status'] == 0] == 1.0) and one['w_out'].tolist() == [1.0] and (one['status'] == 0).sum() >= 6
    none = K.rows_from_entries(np.zeros(4, np.int64), np.zeros(0, np.int64), np.zeros(0), 3)
    out = eng.read_classes_step_host(none, np.full((3, 2), 0.25), np.array([0.3, 0.7]))
    assert out['status'].tolist() == [1, 1, 1] and out['cls'].tolist() == [-1] * 3 and not out['gamma'].any() and not out['ll'].any()
    assert out['w_out'].tolist() == [0.3, 0.7] and out['sums'].tolist() == [0.0] * 6 and np.all(out['theta_out'] == 0.25) and not out['n_site'].any()
    # the rows' entry
    key = np.array([_key(0, p) for p in (5, 9, 12)], np.int64)
    c = _case([(0, 0, np.ones(10)), (0, 3, -np.ones(10))], key)
    hoff = eng.read_sites_host(*[c[f] for f in WALK])
    nr = int(hoff[-1])
    got = {f: np.full(k, 77, np.dtype(kind)) for f, (kind, k) in eng._class_rows_shapes(nr, 3).items()}

    def class_rows(prm=host, nreads=2, hoff=hoff, nrows=nr, out=None, **kw):
        a = dict(c, **kw)
        out = out if out is not None else L.make_class_rows_out(**eng._np_ptrs(got))
        return lib.nmod_read_class_rows(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                        3, ptr(a['key']), ptr(hoff), nrows, C.byref(out))
    assert class_rows(None) == -1 and class_rows(nreads=-1) == -1 and class_rows(hoff=None) == -1 and class_rows(nrows=nr + 1) == -1
    for missing in WALK:
        assert class_rows(**{missing: None}) == -1, missing
    assert class_rows(roff=c['roff'][::-1].copy()) == -1 and class_rows(key=key[::-1].copy()) == -1 and class_rows(hoff=hoff + 1) == -1
    wrong = L.make_class_rows_out(**eng._np_ptrs(got)); wrong.struct_size += 8
    assert class_rows(out=wrong) == -1 and all(np.all(v == 77) for v in got.values())
    assert class_rows() == 0 and same(got['rread'], np.repeat(np.arange(2, dtype=np.int32), np.diff(hoff)))


# ------------------------------------------------------------------------------------------------------------ the fit
def test_the_fit_through_the_device_is_the_fit_through_the_restatement(det):
    """the planted sample from the same starts: the same number of steps within one, theta within 1e-8, the same hard classes except for
    reads whose two largest gamma differ by less than 1e-6"""
    import torch
    from nanomod_amd import readllr
    rows, z, _ = K.planted_rows()
    rows_t, hoff_t = _rows_dev(rows)
    pihat = np.full(40, 0.45)

    def step(theta, w):
        res = det.read_classes_step(rows_t, hoff_t, theta, w, want=('theta_out', 'w_out', 'sums'))
        return res['theta_out'], res['w_out'], res['sums'].cpu().tolist()
    best = None
    for i, th0 in enumerate(readllr.class_starts(pihat, 2, 4, 0)):
        dev = readllr.fit_classes(step, torch.from_numpy(th0.reshape(-1)).cuda(), torch.full((2,), 0.5, dtype=torch.float64, device='cuda'))
        ref = K.em_ref(rows, th0, np.array([0.5, 0.5]))
        theta = dev['theta'].cpu().numpy().reshape(40, 2)
        apart = np.abs(theta - ref['theta']).max()
        print('start %d: %d steps on the device, %d in the restatement; theta apart by at most %.3g; ll %.9f and %.9f'
              % (i, dev['n_iter'], ref['n_iter'], apart, dev['ll'], ref['ll']))
        assert dev['converged'] and ref['converged'] and abs(dev['n_iter'] - ref['n_iter']) <= 1
        assert apart <= 1e-8 and np.abs(dev['w'].cpu().numpy() - ref['w']).max() <= 1e-8
        last = det.read_classes_step(rows_t, hoff_t, dev['theta'], dev['w'], want=('gamma', 'cls'))
        gamma = np.sort(last['gamma'].cpu().numpy().reshape(-1, 2), 1)
        firm = gamma[:, 1] - gamma[:, 0] >= 1e-6
        assert same(last['cls'].cpu().numpy()[firm], K.step_vec(rows, ref['theta'], ref['w'])['cls'][firm]) and firm.mean() > 0.99
        if best is None or dev['ll'] > best[0]:
            best = (dev['ll'], last['cls'].cpu().numpy())
    assert K.agreement(best[1], z) >= 0.98


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def planted():
    reads, model, alt, sites, z = K.planted_reads()
    return dict(reads=reads, model=model, alt=alt, sites=sites, z=z)


def test_end_to_end_through_cluster_reads_llr(planted):
    from nanomod_amd import readllr
    lines = []
    res = readllr.cluster_reads_llr(planted['reads'], planted['model'], planted['alt'], sites=planted['sites'], classes=[1, 2, 3], thr=H.CHAIN_THR,
                                    log=lines.append)
    assert len(lines) == 4 and all(l.startswith('readclasses: ') for l in lines)
    assert [p[0] for p in res['profile']] == [1, 2, 3] and res['C'] == 2 and res['bic'] == min(p[2] for p in res['profile'])
    assert len(res['fit']) == 12 and sum(f['kept'] for f in res['fit']) == 3 and all(f['w'] == tuple(sorted(f['w'], reverse=True)) for f in res['fit'])
    t = res['reads']
    n = len(planted['z'])
    assert t['gamma_all'].shape == (n, 2) and res['theta'].shape == (len(planted['sites'][2]), 2) and res['w'][0] >= res['w'][1]
    has = t['cls'] >= 0
    assert np.all(t['status'][~has] == L.HMM_NO_SITE) and np.all(t['gamma'][has] >= 0.5) and np.all(t['n_sites'][has] > 0)
    share = K.agreement(t['cls'], planted['z'])
    print('end to end: BIC %s; weights %s; agreement with the planted classes %.4f' % (res['profile'], res['w'], share))
    assert share >= 0.98 and abs(res['w'][0] - 0.65) < 0.08
    # one count alone: the same fit of that count; the seed decides the starts
    two = readllr.cluster_reads_llr(planted['reads'], planted['model'], planted['alt'], sites=planted['sites'], classes=2, thr=H.CHAIN_THR, log=lambda *a: None)
    assert two['ll'] == res['ll'] and same(two['theta'], res['theta']) and same(two['reads']['cls'], t['cls'])


def test_the_command_line_writes_the_three_tables(planted):
    from nanomod_amd import cli, container, kmermodel
    reads = planted['reads']
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, a_path, s_path = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'alt.npz', 'sites.txt'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        for path, m in ((m_path, planted['model']), (a_path, planted['alt'])):
            kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
        open(s_path, 'w').writelines('%s %s %d\n' % (c, s, p + 1) for c, s, p in zip(*planted['sites']))
        out = os.path.join(tmp, 'out')
        assert cli.main(['readclasses', '--wrkBase1', r_path, '--model', m_path, '--altModel', a_path, '--sites', s_path, '--classes', '1,2', '--nInit', '2',
                         '--llrThreshold', repr(H.CHAIN_THR), '--FileID', 'run', '--outLevel', '3', '--outFolder', out]) == 0
        assert sorted(os.listdir(out)) == ['run_class_sites.txt', 'run_classes_fit.txt', 'run_read_classes.txt']
        rows = [l.rstrip('\n').split('\t') for l in open(os.path.join(out, 'run_read_classes.txt'))]
        assert rows[0] == ['read', 'chrom', 'strand', 'n_sites', 'class', 'gamma', 'll'] and len(rows) == len(planted['z']) + 1
        cls = np.array([int(r[4]) for r in rows[1:]])
        assert set(cls.tolist()) <= {-1, 0, 1} and K.agreement(cls, planted['z']) >= 0.98 and all(0.0 <= float(r[5]) <= 1.0 for r in rows[1:])
        rows = [l.rstrip('\n').split('\t') for l in open(os.path.join(out, 'run_class_sites.txt'))]
        assert rows[0] == ['chrom', 'strand', 'pos', 'theta_0', 'N_0', 'theta_1', 'N_1'] and len(rows) == len(planted['sites'][2]) + 1
        assert all(0.0 <= float(r[3]) <= 1.0 and float(r[4]) >= 0.0 for r in rows[1:])
        rows = [l.rstrip('\n').split('\t') for l in open(os.path.join(out, 'run_classes_fit.txt'))]
        assert rows[0] == ['C', 'start', 'weights', 'll', 'BIC', 'iterations', 'converged', 'kept'] and [r[0] for r in rows[1:]] == ['1', '1', '2', '2']
        assert sum(int(r[7]) for r in rows[1:]) == 2 and all(abs(sum(float(v) for v in r[2].split(',')) - 1.0) < 1e-5 for r in rows[1:])
