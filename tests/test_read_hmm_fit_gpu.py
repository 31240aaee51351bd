"""GPU: nmod_read_hmm_grad (K21) against tests/hmm_fit_ref.py: ll as nmod_read_hmm's bytes, g_eta and g_lam within the derived gates of the
sequential restatement, the sums as the fixed-order sum of the device's own per-read values; the seams of the scan; extremes against
mpmath; invariances as identical bytes; the stream contract; the refusals; the fit through the device against the fit through the
restatement; the chain K13 -> K21 -> K19 through readllr.smooth_reads_llr and `cli readhmm --fitHmm 1`."""
import ctypes as C
import math
import os
import tempfile

import numpy as np
import pytest

import hmm_fit_ref as F
import hmm_ref as H
import read_batch_cases as RB
import stream_cases as S
from nanomod_amd import _lib as L
from test_engine_device_args_gpu import same
from test_site_pairs import _key

pytestmark = pytest.mark.gpu

PI, LENGTH = 0.3, 30.0
READ = L.HMM_GRAD_READ_FIELDS
ALL = READ + ('sums',)
WALK = ('cs', 'start', 'roff', 'score', 'key')
TILE_GROUP = 256 * L.HMM_CHUNK


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


def _device(det, c, pi=PI, length=LENGTH, with_k19=False, **kw):
    """read_sites and read_hmm_grad on device tensors of case c -> the results as numpy, hoff among them (with_k19: nmod_read_hmm's ll too)"""
    import torch
    t = [torch.from_numpy(c[f]).cuda() for f in WALK]
    hoff, nrows = det.read_sites(*t)
    res = det.read_hmm_grad(*t, hoff, nrows, pi=pi, length=length, **kw)
    out = dict({f: v.cpu().numpy() for f, v in res.items()}, hoff=hoff.cpu().numpy())
    if with_k19:
        out['k19_ll'] = det.read_hmm(*t, hoff, nrows, pi=pi, length=length, want=('ll',))['ll'].cpu().numpy()
    return out


def _check(res, ref, what):
    """the device's per-read values against the restatement's (read_grad_ref); prints the largest errors in units of the gates' scale"""
    assert same(res['hoff'], ref['hoff']) and same(res['status'], ref['status'])
    assert same(res['ll'], res['k19_ll'])                                     # nmod_read_hmm's bytes
    err_e = np.abs(res['g_eta'] - ref['g_eta']) / (ref['abs_eta'] + 1.0)
    err_l = np.abs(res['g_lam'] - ref['g_lam']) / (ref['abs_lam'] + 1.0)
    print('%s: largest error of g_eta %.3g of abs_eta + 1, of g_lam %.3g of abs_lam + 1 (over %d reads, gates up to %.3g)'
          % (what, err_e.max() if len(err_e) else 0.0, err_l.max() if len(err_l) else 0.0, len(err_e), H.CAP))
    for f, g in (('g_eta', 'gate_eta'), ('g_lam', 'gate_lam'), ('abs_eta', 'gate_eta'), ('abs_lam', 'gate_lam')):
        scale = ref['abs_eta' if f.endswith('eta') else 'abs_lam']
        ok = F.within(res[f], ref[f], ref[g], scale)
        assert np.all(ok), (f, np.flatnonzero(~ok)[:5], res[f][~ok][:5], ref[f][~ok][:5])
    none = np.diff(ref['hoff']) == 0
    for f in ('ll', 'g_eta', 'g_lam', 'abs_eta', 'abs_lam'):
        assert np.all(res[f][none] == 0.0), f
    assert same(res['sums'], F.batch_sums(res['ll'], res['g_eta'], res['g_lam'], res['hoff']))


# ------------------------------------------------------------------------------------------------------------ constructed reads
@pytest.fixture(scope='module')
def mixed():
    """test_read_hmm_gpu.py's kind of reads: three (chrom, strand) ids with the same site positions, reads of 1 .. 60 events on all of them
    with scores at and around K13's threshold, 0, NaN and infinities; reads that cover no site, one site, two sites, and every score 0"""
    rng = np.random.default_rng(2111)
    pos = np.unique(np.concatenate((rng.choice(200, 70, replace=False), [100, 110, 111, 150, 160])))
    pos = pos[(pos < 151) | (pos > 159)]
    key = np.array([_key(cs, p) for cs in (0, 1, 2) for p in pos], np.int64)
    values = np.array([3.0, -3.0, 2.5, -2.5, 1.0, -0.5, np.nan, 0.0, np.inf, -np.inf, 40.0, -7.5])
    reads = []
    for _ in range(300):
        n = int(rng.integers(1, 61))
        reads.append((int(rng.integers(0, 3)), int(rng.integers(0, 215 - n)), values[rng.integers(0, len(values), n)]))
    reads.append((0, 300, np.full(30, 3.0)))                                  # covers no site
    reads.append((1, 152, np.full(9, 3.0)))                                   # 152 .. 160: one site ('-')
    reads.append((0, 150, np.array([3.0] + [0.0] * 9 + [-3.0])))              # 150 .. 160: two sites
    reads.append((1, 150, np.array([3.0] + [0.0] * 9 + [-3.0])))              # the same on '-'
    reads.append((2, 100, np.array([2.5] + [np.nan] * 9 + [-2.5, np.nan])))   # 110 valid, 111 not
    reads.append((2, 100, np.zeros(12)))                                      # every score 0
    c = _case(reads, key)
    c['reads'] = reads
    c['ref'] = F.read_grad_ref(*[c[f] for f in WALK], PI, LENGTH)
    return c


def test_gradient_ll_and_sums_on_constructed_reads(det, mixed):
    res = _device(det, mixed, with_k19=True)
    ref = mixed['ref']
    assert set(res) == set(ALL) | {'hoff', 'k19_ll'}
    _check(res, ref, 'constructed reads')
    m = np.diff(ref['hoff'])
    assert m[-6:-1].tolist() == [0, 1, 2, 2, 2] and m[-1] >= 3 and (m == 0).sum() > 5 and m.max() >= 20
    assert res['status'][-6:].tolist() == [1, 0, 0, 0, 0, 0] and np.all(res['g_lam'][m == 1] == 0.0) and np.all(res['abs_lam'][m == 1] == 0.0)
    assert np.all(res['abs_eta'] >= np.abs(res['g_eta'])) and np.all(res['abs_lam'] >= np.abs(res['g_lam']))
    assert res['sums'][6] == (m > 0).sum() and res['sums'][7] == m.sum() and abs(res['sums'][0] - math.fsum(res['ll'].tolist())) < 1e-9
    # the other restatement: the device's documented order lies as close
    dev_order = F.read_grad_ref(*[mixed[f] for f in WALK], PI, LENGTH, chain=F.grad_device_order)
    for f, g in (('g_eta', 'gate_eta'), ('g_lam', 'gate_lam')):
        assert np.all(F.within(res[f], dev_order[f], ref[g], ref['abs_eta' if f == 'g_eta' else 'abs_lam']))


def test_host_and_device_memspace_and_fewer_outputs_give_identical_bytes(det, mixed):
    dev = _device(det, mixed)
    eng = _engine()
    args = [mixed[f] for f in WALK]
    host = eng.read_hmm_grad_host(*args, pi=PI, length=LENGTH)
    assert same(host['hoff'], dev['hoff'])
    for f in ALL:
        assert same(host[f], dev[f]), f
    for want in (('sums',), ('ll',), ('g_eta', 'sums'), ('g_lam', 'abs_lam', 'status'), ('abs_eta',), ('ll', 'g_lam', 'sums')):
        part = _device(det, mixed, want=want)
        assert set(part) == set(want) | {'hoff'}
        for f in want:
            assert same(part[f], dev[f]), (want, f)
    part = eng.read_hmm_grad_host(*args, dev['hoff'], pi=PI, length=LENGTH, want=('sums',))
    assert same(part['sums'], dev['sums'])


def test_a_permutation_of_the_reads_and_a_read_alone_change_nothing(det, mixed):
    dev = _device(det, mixed)
    reads = mixed['reads']
    n = len(reads)
    order = np.random.default_rng(2112).permutation(n)
    perm = _device(det, _case([reads[r] for r in order], mixed['key']))
    for f in READ:
        assert same(perm[f], dev[f][order]), f
    assert same(perm['sums'], F.batch_sums(perm['ll'], perm['g_eta'], perm['g_lam'], perm['hoff']))
    longest = int(np.argmax(np.diff(dev['hoff'])))
    for r in (longest, n - 4, 7):
        alone = _device(det, _case([reads[r]], mixed['key']))
        for f in READ:
            assert same(alone[f], dev[f][r:r + 1]), (r, f)


def test_more_reads_than_either_grid_has_units(det):
    """in read_batch_cases' manner: a batch of copies of a few distinct reads, more of them than the persistent grid of either form has
    waves (workgroups), has the distinct reads' outputs, gathered; its sums are the fixed-order sums of those"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(2113)
    top = L.HMM_WAVE_MAX + 77
    key = np.array([_key(0, p) for p in range(0, 2 * top, 2)], np.int64)      # every second position
    distinct = [(0, int(rng.integers(0, 40)), rng.normal(0.0, 3.0, int(rng.integers(5, 60)))) for _ in range(23)]
    single = _device(det, _case(distinct, key))
    idx = rng.integers(0, len(distinct), RB.short_units(cus) + 1500)
    batch = _device(det, _case([distinct[i] for i in idx], key))
    assert len(idx) > RB.short_units(cus)
    for f in READ:
        assert same(batch[f], single[f][idx]), f
    assert same(batch['sums'], F.batch_sums(batch['ll'], batch['g_eta'], batch['g_lam'], batch['hoff']))
    long_read = (0, 0, rng.normal(0.0, 3.0, 2 * top - 1))                      # top entries: the workgroup form
    one = _device(det, _case([long_read], key))
    many = RB.long_units(cus) + 50
    rep = _device(det, _case([long_read] * many, key), want=('ll', 'g_eta', 'g_lam', 'sums'))
    for f in ('ll', 'g_eta', 'g_lam'):
        assert same(rep[f], np.repeat(one[f], many)), f
    assert rep['sums'][6] == many and rep['sums'][7] == many * top


# ------------------------------------------------------------------------------------------------------------ the seams of the scan
SEAM_M = [1, 4, 5, 255, 256, 257, L.HMM_WAVE_MAX, L.HMM_WAVE_MAX + 1, 2 * TILE_GROUP, 2 * TILE_GROUP + 1]


def test_the_seams_of_the_scan(det):
    """every position a candidate site, so a read of m events has m entries: a lane's chunk, a wave tile, the wave form's last size, the
    workgroup form's second and third tile; on '-' as well, where the events run against the positions"""
    assert SEAM_M == [1, 4, 5, 255, 256, 257, 1024, 1025, 2048, 2049]
    rng = np.random.default_rng(2114)
    key = np.array([_key(cs, p) for cs in (0, 1) for p in range(max(SEAM_M) + 5)], np.int64)
    reads = [(i % 2, 3, rng.normal(0.0, 3.0, m)) for i, m in enumerate(SEAM_M)]
    c = _case(reads, key)
    res = _device(det, c, length=20.0, with_k19=True)
    ref = F.read_grad_ref(*[c[f] for f in WALK], PI, 20.0)
    assert np.diff(ref['hoff']).tolist() == SEAM_M
    _check(res, ref, 'seams')
    assert np.all(np.abs(res['g_lam'][1:]) > 0.0) and res['g_lam'][0] == 0.0


# ------------------------------------------------------------------------------------------------------------ extremes
@pytest.mark.parametrize('pi,length', [(0.3, 1e6), (1e-9, 1e6), (1.0 - 1e-9, 200.0), (0.5, 1e-3), (1e-9, 1e9), (1.0 - 1e-9, 1e9)])
def test_extremes_against_mpmath(det, pi, length):
    """+-800 next to each other at distance 1, pi and length at their bounds, a gap of 60 000 bases"""
    import mpmath as mp
    key = np.array([_key(0, p) for p in (10, 11, 12, 13, 60013, 60014, 60015)], np.int64)
    scores = np.full(60010, np.nan)
    scores[[0, 1, 2, 3, 60003, 60004, 60005]] = 800.0, -800.0, 800.0, -800.0, 5.0, -5.0, 40.0
    c = _case([(0, 10, scores), (0, 10, scores[:4]), (0, 11, -scores[1:6])], key)
    res = _device(det, c, pi=pi, length=length, with_k19=True)
    hoff, _, x, s = H.entries_ref(*[c[f] for f in WALK])
    assert same(res['hoff'], hoff) and hoff.tolist() == [0, 7, 11, 14] and same(res['ll'], res['k19_ll'])
    worst = [0.0, 0.0]
    for r in range(3):
        a, b = int(hoff[r]), int(hoff[r + 1])
        exact = F.grad_mp(x[a:b], s[a:b], pi, length)
        with mp.workdps(60):
            for i, (f, scale, g) in enumerate((('g_eta', 'abs_eta', F.gate_eta(b - a)), ('g_lam', 'abs_lam', F.gate_lam(b - a)))):
                got = float(res[f][r])
                err = abs(mp.mpf(got) - exact[f]) / (exact[scale] + 1)
                worst[i] = max(worst[i], float(err))
                assert math.isfinite(got) and err <= g, (r, f, got, float(exact[f]), float(err))
                assert abs(mp.mpf(float(res[scale][r])) - exact[scale]) <= g * (exact[scale] + 1), (r, scale)
    print('pi %g length %g: largest error against mpmath: g_eta %.3g of abs_eta + 1, g_lam %.3g of abs_lam + 1' % (pi, length, worst[0], worst[1]))
    assert same(res['sums'], F.batch_sums(res['ll'], res['g_eta'], res['g_lam'], res['hoff']))


# ------------------------------------------------------------------------------------------------------------ the stream
def test_side_stream_and_no_wait_for_the_work_before_it(det, mixed):
    """On a side stream the result is the default stream's; and behind a stall of stream_cases.T_MS on a fresh stream (the inputs put in
    place behind the stall, a decoy behind the call: tests/stream_cases.py) the call returns while the stall still runs, and its result
    is the one of the real inputs"""
    import torch
    want = _device(det, mixed)
    real = {f: mixed[f] for f in WALK}
    decoy = dict(real, score=-mixed['score'])                                 # (the same entries: the offsets stay those of the call)
    sw = S.Swapped(real, decoy)
    hoff = torch.from_numpy(want['hoff']).cuda()
    nrows = int(want['hoff'][-1])
    call = lambda out=None: det.read_hmm_grad(*[sw.t[f] for f in WALK], hoff, nrows, pi=PI, length=LENGTH, out=out)
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
def test_refusals_write_nothing(mixed):
    eng = _engine()
    lib = L.load()
    ptr = eng._np_ptr
    n = 6
    c = {f: mixed[f][:n + 1 if f == 'roff' else n].copy() for f in ('cs', 'start', 'roff')}
    c['score'] = mixed['score'][:int(c['roff'][-1])].copy()
    c['key'] = mixed['key']
    hoff = eng.read_sites_host(*[c[f] for f in WALK])
    nrows, ns = int(hoff[-1]), len(c['key'])
    assert nrows > 3
    host = L.make_params(device=0, memspace=L.MEM_HOST)
    shapes = eng._hmm_grad_shapes(ALL, n)
    res = {f: np.full(k, 77, np.dtype(kind)) for f, (kind, k) in shapes.items()}
    untouched = lambda: all(np.all(v == 77) for v in res.values())

    def grad(prm=host, nreads=n, hoff=hoff, nrows=nrows, opts=None, out=None, **kw):
        a = dict(c, **kw)
        opts = opts if opts is not None else L.make_hmm_grad_opts(PI, LENGTH)
        out = out if out is not None else L.make_hmm_grad_out(**eng._np_ptrs(res))
        return lib.nmod_read_hmm_grad(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                      ns, ptr(a['key']), ptr(hoff), nrows, C.byref(opts), C.byref(out))
    assert grad(None) == -1 and grad(L.make_params(device=0, memspace=5)) == -1 and grad(nreads=2 ** 31) == -1 and grad(nreads=-1) == -1
    for missing in WALK:
        assert grad(**{missing: None}) == -1, missing
    assert grad(roff=c['roff'][::-1].copy()) == -1 and grad(key=c['key'][::-1].copy()) == -1
    for bad in (dict(pi=0.0), dict(pi=1e-10), dict(pi=1.0), dict(pi=float('nan')), dict(length=1e-4), dict(length=1.1e9), dict(length=float('inf')),
                dict(length=float('nan'))):
        assert grad(opts=L.make_hmm_grad_opts(**dict(dict(pi=PI, length=LENGTH), **bad))) == -1, bad
    short = L.make_hmm_grad_opts(PI, LENGTH); short.struct_size -= 8
    wrong = L.make_hmm_grad_out(**eng._np_ptrs(res)); wrong.struct_size += 8
    assert grad(opts=short) == -1 and grad(out=wrong) == -1
    assert lib.nmod_read_hmm_grad(C.byref(host), n, ptr(c['cs']), ptr(c['start']), ptr(c['roff']), ptr(c['score']), ns, ptr(c['key']), ptr(hoff), nrows, None,
                                  C.byref(L.make_hmm_grad_out(**eng._np_ptrs(res)))) == -1
    assert grad(hoff=None) == -1 and grad(nrows=-1) == -1 and grad(nrows=2 ** 31) == -1 and grad(nrows=nrows + 1) == -1
    down = hoff.copy()
    down[n - 1] = down[n] + 1
    assert grad(hoff=hoff + 1) == -1 and grad(hoff=down) == -1
    assert untouched()
    # what is not refused: the call itself; no reads — sums of 0; reads without an entry
    assert grad() == 0 and not untouched()
    z = np.full(8, 77.0)
    none = np.zeros(1, np.int64)
    assert lib.nmod_read_hmm_grad(C.byref(host), 0, None, None, None, None, ns, ptr(c['key']), ptr(none), 0, C.byref(L.make_hmm_grad_opts(PI, LENGTH)),
                                  C.byref(L.make_hmm_grad_out(sums=ptr(z)))) == 0
    assert np.all(z == 0.0)
    far = _case([(0, 300, np.full(30, 3.0)), (1, 151, np.full(9, 3.0))], c['key'])     # reads, none of which covers a site
    out = eng.read_hmm_grad_host(*[far[f] for f in WALK], pi=PI, length=LENGTH)
    assert out['hoff'].tolist() == [0, 0, 0] and out['status'].tolist() == [1, 1] and out['sums'].tolist() == [0.0] * 8
    assert all(out[f].tolist() == [0.0, 0.0] for f in ('ll', 'g_eta', 'g_lam', 'abs_eta', 'abs_lam'))
    with pytest.raises(ValueError):
        eng.read_hmm_grad_host(*[far[f] for f in WALK], pi=2.0)


# ------------------------------------------------------------------------------------------------------------ the fit
def test_the_fit_through_the_device_is_the_fit_through_the_restatement(det):
    """Both stop at criterion tol = 1e-10, which places each within about sqrt(tol) = 1e-5 standard errors of the maximum: they agree
    within 1e-3 standard errors in eta and lam, and their evaluation counts differ by at most one"""
    import torch
    from nanomod_amd import readllr
    reads = F.simulate_chain_reads()
    c = F.walk_inputs(reads)
    t = [torch.from_numpy(c[f]).cuda() for f in WALK]
    hoff, nrows = det.read_sites(*t)
    assert nrows == sum(len(s) for _, s in reads) and same(np.diff(hoff.cpu().numpy()), np.array([len(s) for _, s in reads]))
    dev = readllr.fit_hmm(lambda p, v: det.read_hmm_grad(*t, hoff, nrows, pi=p, length=v, want=('sums',))['sums'].cpu().tolist(), 0.5, 200.0)
    ref = readllr.fit_hmm(F.evaluator(reads), 0.5, 200.0)
    d_eta, d_lam = abs(dev['eta'] - ref['eta']) / ref['se_eta'], abs(dev['lam'] - ref['lam']) / ref['se_lam']
    print('device fit: pi %.9g length %.9g in %d evaluations; restatement: pi %.9g length %.9g in %d; apart by %.3g and %.3g standard errors'
          % (dev['pi'], dev['length'], dev['n_eval'], ref['pi'], ref['length'], ref['n_eval'], d_eta, d_lam))
    assert dev['converged'] and ref['converged'] and dev['status'] == ref['status'] == 'pi and length fitted'
    assert d_eta <= 1e-3 and d_lam <= 1e-3 and abs(dev['n_eval'] - ref['n_eval']) <= 1
    assert (dev['n_reads'], dev['n_entries']) == (ref['n_reads'], ref['n_entries']) == (len(reads), nrows)
    assert abs(dev['se_eta'] - ref['se_eta']) <= 1e-6 * ref['se_eta'] and abs(dev['se_lam'] - ref['se_lam']) <= 1e-6 * ref['se_lam']
    assert abs(dev['eta'] - readllr._logit(0.3)) < 3.0 * dev['se_eta'] and abs(dev['lam'] - math.log(150.0)) < 3.0 * dev['se_lam']


# ------------------------------------------------------------------------------------------------------------ end to end
GRID = [12.5, 25.0, 50.0, 100.0, 200.0, 400.0]
CHAIN_PI = 0.15


@pytest.fixture(scope='module')
def chain():
    import readllr_ref as RF
    reads, model, alt, sites, planted = H.chain_inputs()
    exp = RF.restate(reads['norm_mean'], reads['off'], reads['base'], model['k'], model['center'], model['mean'], model['sd'], alt['mean'], alt['sd'],
                     'kmer', H.CHAIN_THR, 0.0)
    cs = (reads['strand'] == '-').astype(np.int32)
    key = np.unique(np.array([_key(0 if s == '+' else 1, p) for s, p in zip(sites[1], sites[2])], np.int64))
    return dict(reads=reads, model=model, alt=alt, sites=sites, walk=(cs, reads['start'], reads['off'], exp['llr_win'], key))


def test_end_to_end_through_smooth_reads_llr(chain):
    from nanomod_amd import readllr
    eng = _engine()
    lines = []
    res = readllr.smooth_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], pi=CHAIN_PI, fit='mle', thr=H.CHAIN_THR, log=lines.append)
    fit = res['fit']
    assert len(lines) == 2 and lines[0].startswith('readhmm: maximum-likelihood fit: pi ') and lines[1].startswith('readhmm: 120 read(s)')
    assert fit['converged'] and fit['status'] == 'pi and length fitted' and (res['pi'], res['length']) == (fit['pi'], fit['length']) and res['profile'] == []
    assert fit['trace'][0][:2] == (CHAIN_PI, 200.0) and fit['n_reads'] <= 120 and fit['n_entries'] == len(res['entries']['post'])
    hoff = eng.read_sites_host(*chain['walk'])
    grid = [math.fsum(eng.read_hmm_host(*chain['walk'], hoff, pi=fit['pi'], length=v, want=('ll',))['ll'].tolist()) for v in GRID]
    print('fitted pi %.6g length %.6g: log-likelihood %.6f; the grid at that pi: %s' % (fit['pi'], fit['length'], fit['ll'], ', '.join('%.6f' % v for v in grid)))
    assert fit['ll'] >= max(grid)
    # the decoding used the fitted values: the reads' ll sum to the fit's
    assert abs(math.fsum(res['reads']['ll'].tolist()) - fit['ll']) <= 1e-9 * (abs(fit['ll']) + 1)
    fixed = readllr.smooth_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], pi=CHAIN_PI, fit='mle', fix_pi=True, thr=H.CHAIN_THR,
                                     decode='viterbi', log=lambda *a: None)
    assert fixed['fit']['converged'] and fixed['pi'] == CHAIN_PI and fixed['fit']['status'].startswith('length fitted alone') and 'viterbi' in fixed


def test_the_command_line_writes_the_fit_and_nothing_else_changes_without_it(chain):
    from nanomod_amd import cli, container, kmermodel
    reads = chain['reads']
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, a_path, s_path = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'alt.npz', 'sites.txt'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        for path, m in ((m_path, chain['model']), (a_path, chain['alt'])):
            kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
        open(s_path, 'w').writelines('%s %s %d\n' % (c, s, p + 1) for c, s, p in zip(*chain['sites']))
        base = ['readhmm', '--wrkBase1', r_path, '--model', m_path, '--altModel', a_path, '--sites', s_path, '--hmmPi', repr(CHAIN_PI), '--FileID', 'run',
                '--outLevel', '3']
        plain, fitted = os.path.join(tmp, 'plain'), os.path.join(tmp, 'fitted')
        assert cli.main(base + ['--outFolder', plain]) == 0
        assert sorted(os.listdir(plain)) == ['run_read_domains.txt', 'run_read_hmm.txt', 'run_site_hmm.txt']
        assert cli.main(base + ['--outFolder', fitted, '--fitHmm', '1']) == 0
        assert sorted(os.listdir(fitted)) == ['run_hmm_fit.txt', 'run_read_domains.txt', 'run_read_hmm.txt', 'run_site_hmm.txt']
        rows = [line.split() for line in open(os.path.join(fitted, 'run_hmm_fit.txt'))]
        trace = [r for r in rows if r[0].isdigit()]
        assert [r[0] for r in trace] == [str(i) for i in range(len(trace))] and len(trace) >= 2 and float(trace[0][1]) == CHAIN_PI and float(trace[0][2]) == 200.0
        tail = rows[len(trace):]
        assert [r[0] for r in tail] == ['pi', 'length', 'evaluations', 'status'] and int(tail[2][1]) >= len(trace) and tail[2][2:] == ['converged', '1', 'level', '0.95']
        assert float(tail[0][2]) < float(tail[0][1]) < float(tail[0][3]) and float(tail[1][2]) < float(tail[1][1]) < float(tail[1][3])
        assert float(tail[0][1]) == float(trace[-1][1]) and float(tail[1][1]) == float(trace[-1][2])
        assert cli.main(base + ['--outFolder', fitted, '--fitHmm', '1', '--fitLength', '50,100']) != 0
