"""GPU: nmod_read_hmm_prior, nmod_read_viterbi_prior and nmod_read_hmm_grad_prior (K23) against tests/hmm_prior_ref.py: a constant prior
(and one of NaN alone) gives the plain entries' bytes; shares of every kind, the ends of the clamp, NaN and the infinities among them,
within the gates of the restatement in the device's order; the closed forms where rho underflows; the share follows the site, not the
row; memspaces and single outputs as identical bytes; the refusals; the stream contract; the chain K13 -> K14 -> K23 through
readllr.smooth_reads_llr and `cli readhmm --sitePrior 1`."""
import ctypes as C
import filecmp
import os
import tempfile

import numpy as np
import pytest

import hmm_fit_ref as F
import hmm_prior_ref as P
import hmm_ref as H
import readllr_ref as RF
import rescale_ref as R
import stream_cases as S
from nanomod_amd import _lib as L

pytestmark = pytest.mark.gpu

PI, LENGTH, CALL_POST = 0.3, 30.0, 0.9
HMM_ALL = L.HMM_ENTRY_FIELDS + L.HMM_READ_FIELDS + L.HMM_SITE_FIELDS
VIT_ALL = L.VIT_ENTRY_FIELDS + L.VIT_READ_FIELDS + L.VIT_SITE_FIELDS
GRAD_ALL = L.HMM_GRAD_READ_FIELDS + ('sums',)
METHODS = (('read_hmm', HMM_ALL), ('read_viterbi', VIT_ALL), ('read_hmm_grad', GRAD_ALL))
SEAM_M = (1, 2, 255, 256, 257, 1024, 1025, 2048, 2049)         # the wave-tile seam, the wave -> workgroup step, the workgroup-tile seam
KINDS = np.array([1e-12, 1e-9, 0.02, 0.3, 0.5, 0.97, 1.0 - 1e-9, 1.0, 0.0, np.nan, np.inf, -np.inf])
SHARE_SEED = 2301                                               # (the reference alone leaves no entry to the device: checked on the CPU)
READ_ARGS = ('cs', 'start', 'roff', 'score', 'key')


def same(a, b):
    """identical bytes (a -0.0 is not a 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _key(cs, pos):
    return (int(cs) << 40) | int(pos)


def _engine():
    from nanomod_amd import engine
    return engine


@pytest.fixture(scope='module')
def det():
    return _engine().DeviceDetector(0)


def _case(reads, key):
    cs = np.array([r[0] for r in reads], np.int32)
    start = np.array([r[1] for r in reads], np.int64)
    roff = np.zeros(len(reads) + 1, np.int64)
    roff[1:] = np.cumsum([len(r[2]) for r in reads])
    score = np.concatenate([np.asarray(r[2], np.float64) for r in reads]) if reads else np.zeros(0)
    return dict(cs=cs, start=start, roff=roff, score=score, key=np.asarray(key, np.int64))


def _device(det, c, what, site_pi=None, pi=PI, length=LENGTH, **kw):
    """read_sites and the method `what` on device tensors of case c -> the results as numpy, hoff among them"""
    import torch
    t = [torch.from_numpy(c[f]).cuda() for f in READ_ARGS]
    hoff, nrows = det.read_sites(*t)
    if what == 'read_hmm':
        kw.setdefault('call_post', CALL_POST)
    if site_pi is not None:
        kw['site_pi'] = torch.from_numpy(np.ascontiguousarray(site_pi, np.float64)).cuda()
    res = getattr(det, what)(*t, hoff, nrows, pi=pi, length=length, **kw)
    return dict({f: v.cpu().numpy() for f, v in res.items()}, hoff=hoff.cpu().numpy())


def _shares(c, seed=SHARE_SEED):
    return KINDS[np.random.default_rng(seed).integers(0, len(KINDS), len(c['key']))]


def _with_ref(c, length=LENGTH):
    c['site_pi'] = _shares(c)
    c['ref'] = P.read_prior_ref(*[c[f] for f in READ_ARGS], c['site_pi'], PI, length, CALL_POST)
    return c


@pytest.fixture(scope='module')
def mixed():
    """test_read_hmm_gpu's `mixed`, rebuilt: three (chrom, strand) ids with the same site positions, reads of 1 .. 60 events with scores at
    and around K13's threshold, 0, NaN and infinities; reads that cover no site, one site, and sites at their first and last event"""
    rng = np.random.default_rng(1911)
    pos = np.unique(np.concatenate((rng.choice(200, 70, replace=False), [100, 110, 111, 150, 160])))
    pos = pos[(pos < 151) | (pos > 159)]
    key = np.array([_key(cs, p) for cs in (0, 1, 2) for p in pos], np.int64)
    values = np.array([3.0, -3.0, 2.5, -2.5, 1.0, -0.5, np.nan, 0.0, np.inf, -np.inf, 40.0, -7.5])
    reads = []
    for _ in range(400):
        n = int(rng.integers(1, 61))
        reads.append((int(rng.integers(0, 3)), int(rng.integers(0, 215 - n)), values[rng.integers(0, len(values), n)]))
    reads += [(0, 300, np.full(30, 3.0)), (1, 151, np.full(9, 3.0)), (1, 152, np.full(9, 3.0)), (0, 152, np.full(9, -3.0)),
              (0, 150, np.array([3.0] + [0.0] * 9 + [-3.0])), (1, 150, np.array([3.0] + [0.0] * 9 + [-3.0])),
              (2, 100, np.array([2.5] + [np.nan] * 9 + [-2.5, np.nan])), (2, 100, np.zeros(12))]
    return _with_ref(_case(reads, key))


@pytest.fixture(scope='module')
def seams():
    """every position a candidate site on '-': a read of m events has m entries, for every m of SEAM_M"""
    rng = np.random.default_rng(2302)
    key = np.array([_key(1, p) for p in range(max(SEAM_M) + 5)], np.int64)
    c = _with_ref(_case([(1, 3, rng.normal(0.0, 3.0, m)) for m in SEAM_M], key))
    assert np.diff(c['ref']['hoff']).tolist() == list(SEAM_M)
    return c


# ------------------------------------------------------------------------------------------------------------ a constant prior
@pytest.mark.parametrize('which', ['mixed', 'seams'])
def test_a_constant_prior_and_one_of_nan_alone_give_the_plain_entries_bytes(det, mixed, seams, which):
    c = dict(mixed=mixed, seams=seams)[which]
    ns = len(c['key'])
    plain = _device(det, c, 'read_hmm')
    assert set(plain) == set(HMM_ALL) | {'hoff'} and len(plain['post']) > 2000
    grad = _device(det, c, 'read_hmm_grad')
    vit = _device(det, c, 'read_viterbi')
    m = np.diff(plain['hoff'])
    for site_pi in (np.full(ns, PI), np.full(ns, np.nan)):
        got = _device(det, c, 'read_hmm', site_pi)
        for f in HMM_ALL:
            assert same(got[f], plain[f]), f
        g = _device(det, c, 'read_hmm_grad', site_pi)
        for f in ('ll', 'g_lam', 'abs_lam', 'status'):
            assert same(g[f], grad[f]), f
        assert same(g['sums'][[0, 2, 5, 6, 7]], grad['sums'][[0, 2, 5, 6, 7]]) and same(g['ll'], plain['ll'])
        gate = np.array([P.gate_eta(int(v)) if v else 0.0 for v in m])
        assert np.all(F.within(g['g_eta'], grad['g_eta'], gate, grad['abs_eta'])) and np.all(F.within(g['abs_eta'], grad['abs_eta'], gate, grad['abs_eta']))
        # K20 takes its two logarithms from the host, K23 from the device: the values agree within the gate, the integers wherever delta is no tie
        v = _device(det, c, 'read_viterbi', site_pi)
        vg = np.array([P.gate_vit(int(k)) for k in m]) * (np.abs(vit['vit']) + np.abs(plain['ll']) + 1.0)
        assert np.all(np.abs(v['vit'] - vit['vit']) <= vg) and same(v['site'], vit['site']) and same(v['site_n'], vit['site_n'])
        clear = np.abs(vit['delta']) > 1e-9
        assert clear.mean() > 0.95 and same(v['path'][clear], vit['path'][clear])


# ------------------------------------------------------------------------------------------------------------ varying shares
def _check_hmm(res, ref):
    """test_read_hmm_gpu._check for the prior entry: returns the share of the entries left to the device's decision"""
    assert same(res['hoff'], ref['hoff']) and same(res['site'], ref['site'])
    ok = H.post_within(res['post'], ref['post'], ref['gate'])
    assert np.all(ok), (np.flatnonzero(~ok)[:5], res['post'][~ok][:5], ref['post'][~ok][:5])
    g_read = np.array([P.gate(int(m)) if m else 0.0 for m in np.diff(ref['hoff'])])
    for f in ('ll', 'll_indep'):
        ok = H.ll_within(res[f], ref[f], g_read, ref['denom'])
        assert np.all(ok), (f, np.flatnonzero(~ok)[:5], res[f][~ok][:5], ref[f][~ok][:5])
    assert same(res['status'], ref['status']) and same(res['n_sites'], ref['n_sites'])
    state = H.states(res['post'], CALL_POST)                                  # the hard outputs are those of the post that was written
    assert same(res['state'], state)
    own = dict(H.per_read(res['hoff'], state), **H.per_site(res['site'], state, len(ref['site_n'])))
    for f in ('n_mod', 'n_can', 'n_runs') + L.HMM_SITE_FIELDS:
        assert same(res[f], own[f]), f
    clear = H.band_margin(ref['post'], CALL_POST, ref['gate'])
    assert same(res['state'][clear], ref['state'][clear])
    if clear.all():
        for f in ('n_mod', 'n_can', 'n_runs') + L.HMM_SITE_FIELDS:
            assert same(res[f], ref[f]), f
    big = ref['post'] > 1e-280
    print('largest relative error of post %.3g over %d entries' % (float(np.max(np.abs(res['post'][big] - ref['post'][big]) / ref['post'][big])), len(big)))
    return 1.0 - float(clear.mean()) if len(clear) else 0.0


def _check_vit(res, c):
    """vit and delta within the gates of the restatement; path the reference's wherever the exact |delta| exceeds the gate and the
    margins of the near decisions (viterbi_ref's argument); returns the share of the entries that leaves out"""
    ref = c['ref']
    hoff = ref['hoff']
    assert same(res['site'], ref['site']) and same(res['status'], ref['status']) and same(res['n_sites'], ref['n_sites'])
    assert np.all(np.abs(res['vit'] - ref['v_vit']) <= ref['v_gate']) and np.all(np.abs(res['delta'] - ref['v_delta']) <= ref['v_gate_row'])
    out = np.zeros(len(ref['site']), bool)
    for r in range(len(hoff) - 1):
        a, b = int(hoff[r]), int(hoff[r + 1])
        if b > a:
            ex = P.viterbi_mp(ref['x'][a:b], ref['s'][a:b], ref['p'][a:b], c.get('length', LENGTH), ref['v_gate'][r], dps=40)
            sure = np.abs(ex['delta']) > ref['v_gate'][r] + ex['near_loss']
            out[a:b] = ~sure
            assert same(res['path'][a:b][sure], ex['path'][sure]), r
    own = dict(n_mod=np.add.reduceat(np.concatenate((res['path'], [0])).astype(np.int32), hoff[:-1]) * (np.diff(hoff) > 0))
    assert same(res['n_mod'], own['n_mod'].astype(np.int32))
    assert same(res['site_mod'], np.bincount(res['site'][res['path'] == 1], minlength=len(c['key'])).astype(np.int32))
    assert same(res['n_runs'], np.array([len(H.runs(res['path'][hoff[r]:hoff[r + 1]])[0]) for r in range(len(hoff) - 1)], np.int32))
    return float(out.mean()) if len(out) else 0.0


@pytest.mark.parametrize('which', ['mixed', 'seams'])
def test_shares_of_every_kind_within_the_gates_of_the_restatement(det, mixed, seams, which):
    c = dict(mixed=mixed, seams=seams)[which]
    ref = c['ref']
    assert set(np.flatnonzero(np.isnan(KINDS))) and len(set(ref['p'].tolist())) == 6 and ref['p'].min() == 1e-9 and ref['p'].max() == 1.0 - 1e-9
    left = _check_hmm(_device(det, c, 'read_hmm', c['site_pi']), ref)
    left_v = _check_vit(_device(det, c, 'read_viterbi', c['site_pi']), c)
    print('left to the device: %.4f of the states, %.4f of the path' % (left, left_v))
    assert left <= 0.05 and left_v <= 0.05
    g = _device(det, c, 'read_hmm_grad', c['site_pi'])
    assert same(g['ll'], _device(det, c, 'read_hmm', c['site_pi'], want=('ll',))['ll']) and same(g['status'], ref['status'])
    for f, gate, scale in (('g_eta', 'gate_eta', 'abs_eta'), ('g_lam', 'gate_lam', 'abs_lam'), ('abs_eta', 'gate_eta', 'abs_eta'), ('abs_lam', 'gate_lam', 'abs_lam')):
        ok = F.within(g[f], ref[f], ref[gate], ref[scale])
        assert np.all(ok), (f, np.flatnonzero(~ok)[:5], g[f][~ok][:5], ref[f][~ok][:5])
    assert same(g['sums'], F.batch_sums(g['ll'], g['g_eta'], g['g_lam'], g['hoff']))


def test_closed_forms_where_rho_underflows(det, mixed):
    """length 1e-3 and gaps >= 1: rho = exp(-1000 ..) is 0 and eps 1, every site is drawn from its own law"""
    length = 1e-3
    ref = mixed['ref']
    p, s = ref['p'], ref['s']
    e0, e1 = np.where(s > 0, np.exp(-np.abs(s)), 1.0), np.where(s < 0, np.exp(-np.abs(s)), 1.0)
    want = p * e1 / ((1.0 - p) * e0 + p * e1)
    res = _device(det, mixed, 'read_hmm', mixed['site_pi'], length=length)
    assert np.all(H.post_within(res['post'], want, ref['gate']))
    m = np.diff(ref['hoff'])
    g_read = np.array([P.gate(int(v)) if v else 0.0 for v in m])
    denom = np.add.reduceat(np.concatenate((np.abs(np.log((1.0 - p) * e0 + p * e1)) + np.maximum(s, 0.0), [0.0])), ref['hoff'][:-1]) * (m > 0)
    assert np.all(H.ll_within(res['ll'], res['ll_indep'], g_read, denom)) and np.any(res['ll'] != 0.0)
    g = _device(det, mixed, 'read_hmm_grad', mixed['site_pi'], length=length)
    assert np.all(g['g_lam'] == 0.0) and np.all(g['abs_lam'] == 0.0) and same(g['ll'], res['ll'])


# ------------------------------------------------------------------------------------------------------------ the site, not the row
@pytest.fixture(scope='module')
def interleaved():
    """positions 10 .. 49 on '+' and '-': read 0 ('+') has a valid score at the even ones, read 1 ('-') at the odd ones, a third read at
    all of '+'; a distinct share at each of the 80 sites"""
    rng = np.random.default_rng(2303)
    key = np.array([_key(cs, p) for cs in (0, 1) for p in range(10, 50)], np.int64)
    even, odd, full = rng.normal(0.0, 3.0, 40), rng.normal(0.0, 3.0, 40), rng.normal(0.0, 3.0, 40)
    even[1::2] = np.nan
    odd[1::2] = np.nan                                                        # '-': event i lies at 49 - i, the valid ones at 49, 47, ...
    c = _case([(0, 10, even), (1, 10, odd), (0, 10, full)], key)
    c['site_pi'] = np.linspace(0.01, 0.99, 80)[rng.permutation(80)]
    c['ref'] = P.read_prior_ref(*[c[f] for f in READ_ARGS], c['site_pi'], PI, LENGTH, CALL_POST)
    return c


def test_the_share_follows_the_site_not_the_row(det, interleaved):
    c, ref = interleaved, interleaved['ref']
    assert np.diff(ref['hoff']).tolist() == [20, 20, 40] and len(set(ref['p'].tolist())) == 60
    assert same(ref['p'][:20], c['site_pi'][0:40:2]) and same(ref['p'][20:40], c['site_pi'][41:80:2])
    assert _check_hmm(_device(det, c, 'read_hmm', c['site_pi']), ref) <= 0.05
    n = len(c['cs'])
    reads = [(c['cs'][r], c['start'][r], c['score'][c['roff'][r]:c['roff'][r + 1]]) for r in range(n)]
    order = [2, 0, 1]
    for what, fields in METHODS:
        entry = [f for f in fields if f in L.HMM_ENTRY_FIELDS + L.VIT_ENTRY_FIELDS]
        site = [f for f in fields if f in L.HMM_SITE_FIELDS + L.VIT_SITE_FIELDS]
        per_read = [f for f in fields if f not in entry + site + ['sums']]
        dev = _device(det, c, what, c['site_pi'])
        perm = _device(det, _case([reads[r] for r in order], c['key']), what, c['site_pi'])
        rows = np.concatenate([np.arange(dev['hoff'][r], dev['hoff'][r + 1]) for r in order])
        for f in entry:
            assert same(perm[f], dev[f][rows]), (what, f)
        for f in per_read:
            assert same(perm[f], dev[f][order]), (what, f)
        for f in site:
            assert same(perm[f], dev[f]), (what, f)
        for r in range(n):
            alone = _device(det, _case([reads[r]], c['key']), what, c['site_pi'])
            for f in entry:
                assert same(alone[f], dev[f][dev['hoff'][r]:dev['hoff'][r + 1]]), (what, r, f)
            for f in per_read:
                assert same(alone[f], dev[f][r:r + 1]), (what, r, f)


# ------------------------------------------------------------------------------------------------------------ memspaces, outputs
def test_host_and_device_memspace_and_single_outputs_give_identical_bytes(det, mixed):
    eng = _engine()
    args = [mixed[f] for f in READ_ARGS]
    hoff = eng.read_sites_host(*args)
    for what, fields in METHODS:
        dev = _device(det, mixed, what, mixed['site_pi'])
        kw = dict(call_post=CALL_POST) if what == 'read_hmm' else {}
        host = getattr(eng, what + '_host')(*args, hoff, pi=PI, length=LENGTH, site_pi=mixed['site_pi'], **kw)
        assert same(host['hoff'], dev['hoff'])
        for f in fields:
            assert same(host[f], dev[f]), (what, f)
        for f in fields:
            part = _device(det, mixed, what, mixed['site_pi'], want=(f,))
            assert set(part) == {f, 'hoff'} and same(part[f], dev[f]), (what, f)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(det, mixed):
    import torch
    eng = _engine()
    lib = L.load()
    ptr = eng._np_ptr
    n = 6
    c = {f: mixed[f][:n + 1 if f == 'roff' else n].copy() for f in ('cs', 'start', 'roff')}
    c['score'] = mixed['score'][:int(c['roff'][-1])].copy()
    c['key'] = mixed['key']
    hoff = eng.read_sites_host(*[c[f] for f in READ_ARGS])
    nrows, ns = int(hoff[-1]), len(c['key'])
    host = L.make_params(device=0, memspace=L.MEM_HOST)
    site_pi = mixed['site_pi']
    makers = dict(nmod_read_hmm_prior=(lambda **k: L.make_hmm_opts(**dict(dict(pi=PI, length=LENGTH, call_post=CALL_POST), **k)), L.make_hmm_out,
                                       eng._hmm_shapes(HMM_ALL, nrows, n, ns)),
                  nmod_read_viterbi_prior=(lambda **k: L.make_vit_opts(**dict(dict(pi=PI, length=LENGTH), **k)), L.make_vit_out,
                                           eng._vit_shapes(VIT_ALL, nrows, n, ns)),
                  nmod_read_hmm_grad_prior=(lambda **k: L.make_hmm_grad_opts(**dict(dict(pi=PI, length=LENGTH), **k)), L.make_hmm_grad_out,
                                            eng._hmm_grad_shapes(GRAD_ALL, n)))
    for name, (make_opts, make_out, shapes) in makers.items():
        res = {f: np.full(k, 77, np.dtype(kind)) for f, (kind, k) in shapes.items()}

        def call(prm=host, nreads=n, hoff=hoff, nrows=nrows, opts=None, out=None, site_pi=site_pi, **kw):
            a = dict(c, **kw)
            opts = opts if opts is not None else make_opts()
            out = out if out is not None else make_out(**eng._np_ptrs(res))
            return getattr(lib, name)(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                      ns, ptr(a['key']), ptr(site_pi), ptr(hoff), nrows, C.byref(opts), C.byref(out))
        assert call(site_pi=None) == -1                                       # the refusal of its own
        assert call(None) == -1 and call(L.make_params(device=0, memspace=5)) == -1 and call(nreads=-1) == -1
        for missing in READ_ARGS:
            assert call(**{missing: None}) == -1, (name, missing)
        assert call(roff=c['roff'][::-1].copy()) == -1 and call(key=c['key'][::-1].copy()) == -1
        for bad in (dict(pi=0.0), dict(pi=1.0), dict(pi=float('nan')), dict(length=1e-4), dict(length=float('inf'))):
            assert call(opts=make_opts(**bad)) == -1, (name, bad)
        if name == 'nmod_read_hmm_prior':
            assert call(opts=make_opts(call_post=0.5)) == -1
        short = make_opts(); short.struct_size -= 8
        wrong = make_out(**eng._np_ptrs(res)); wrong.struct_size += 8
        assert call(opts=short) == -1 and call(out=wrong) == -1
        assert call(hoff=None) == -1 and call(nrows=-1) == -1 and call(nrows=nrows + 1) == -1 and call(hoff=hoff + 1) == -1
        assert all(np.all(v == 77) for v in res.values()), name
        assert call() == 0 and not all(np.all(v == 77) for v in res.values())
        # no sites: nothing to index, a NULL site_pi is not refused; the reads get NMOD_HMM_NO_SITE
        none = {f: np.full(k, 77, np.dtype(kind)) for f, (kind, k) in shapes.items() if k == n}
        z = np.zeros(n + 1, np.int64)
        assert getattr(lib, name)(C.byref(host), n, ptr(c['cs']), ptr(c['start']), ptr(c['roff']), ptr(c['score']), 0, ptr(c['key']), None, ptr(z), 0,
                                  C.byref(make_opts()), C.byref(make_out(**eng._np_ptrs(none)))) == 0
        assert np.all(none['status'] == L.HMM_NO_SITE)
    # the device methods: a wrong length, dtype or device before any device work
    t = [torch.from_numpy(c[f]).cuda() for f in READ_ARGS]
    d_hoff = torch.from_numpy(hoff).cuda()
    for what, _ in METHODS:
        for bad in (torch.zeros(ns - 1, dtype=torch.float64, device='cuda'), torch.zeros(ns, dtype=torch.float32, device='cuda'),
                    torch.zeros(ns, dtype=torch.float64), np.zeros(ns), torch.zeros(2 * ns, dtype=torch.float64, device='cuda')[::2]):
            with pytest.raises(ValueError, match='site_pi'):
                getattr(det, what)(*t, d_hoff, nrows, pi=PI, length=LENGTH, site_pi=bad)


# ------------------------------------------------------------------------------------------------------------ the stream
@pytest.mark.parametrize('what,fields', METHODS)
def test_no_wait_for_the_work_before_it(det, mixed, what, fields):
    """test_read_hmm_gpu's stalled-stream case for each prior entry (tests/stream_cases.py: the inputs, site_pi among them, put in place
    behind the stall, a decoy behind the call): the call returns while the stall still runs, and its result is the real inputs'"""
    import torch
    want = _device(det, mixed, what, mixed['site_pi'])
    real = dict({f: mixed[f] for f in READ_ARGS}, site_pi=mixed['site_pi'])
    decoy = dict(real, score=-mixed['score'], site_pi=mixed['site_pi'][::-1].copy())     # (the same entries: the offsets stay the call's)
    sw = S.Swapped(real, decoy)
    hoff = torch.from_numpy(want['hoff']).cuda()
    nrows = int(want['hoff'][-1])
    kw = dict(call_post=CALL_POST) if what == 'read_hmm' else {}
    call = lambda out=None: getattr(det, what)(*[sw.t[f] for f in READ_ARGS], hoff, nrows, pi=PI, length=LENGTH, site_pi=sw.t['site_pi'], out=out, **kw)
    side = torch.cuda.Stream()
    sw.load_real()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        first = call()
    side.synchronize()
    for f in fields:
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
        for f in fields:
            assert same(got[f].cpu().numpy(), want[f]), f
        assert sw.holds('decoy')


# ------------------------------------------------------------------------------------------------------------ end to end
HOT = (14, 22)                                                              # the candidate positions (by index) most reads are modified at


def _two_kinds_of_sites(seed=2304, n_reads=120, genome_len=640, spacing=12, stretch=8, shift=1.5):
    """hmm_ref.chain_inputs' sample with the stretches planted by site: a read that covers the positions HOT carries its stretch there
    with probability 0.8 (sites of a high share); otherwise one read in ten carries a stretch elsewhere (sites of a low share)"""
    k, center = 3, 0
    mean, sd = R.make_model(k, holes=False)
    mean1 = mean + shift * sd
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b'ACGT', np.uint8), genome_len)
    site_pos = np.arange(spacing, genome_len - spacing, spacing)
    lo, hi = RF.kmer_window(k, center)
    chrom, strand, start, vals, bases = [], [], [], [], []
    planted = np.zeros((n_reads, len(site_pos)), bool)
    for r in range(n_reads):
        minus = r % 2 == 1
        n = int(rng.integers(200, 301))
        s0 = int(rng.integers(0, genome_len - n + 1))
        pos = s0 + np.arange(n) if not minus else s0 + n - 1 - np.arange(n)
        b = genome[pos] if not minus else R._COMP[genome[pos]]
        codes = R.read_codes(b, k, center)
        level = mean[codes].copy()
        covered = np.flatnonzero((site_pos >= s0 + 4) & (site_pos <= s0 + n - 5))
        hot = np.arange(HOT[0], HOT[1])
        where = None
        if np.isin(hot, covered).all():
            where = hot if rng.random() < 0.8 else None
        elif len(covered) >= stretch and rng.random() < 0.1:
            first = int(rng.integers(0, len(covered) - stretch + 1))
            where = covered[first:first + stretch]
        for a in ([] if where is None else where):
            j = int(np.flatnonzero(pos == site_pos[a])[0])
            cover = np.arange(j - lo, j + hi + 1)
            level[cover] = mean1[codes[cover]]
            planted[r, a] = True
        chrom.append('chrT'); strand.append('-' if minus else '+'); start.append(s0); bases.append(b)
        vals.append(np.rint((level + sd[codes] * rng.normal(size=n)) * 1000.0) / 1000.0)
    off = np.zeros(n_reads + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in vals])
    reads = dict(chrom=np.array(chrom), strand=np.array(strand), start=np.array(start, np.int64), off=off,
                 norm_mean=R.cast(np.concatenate(vals), 'int16'), base=np.concatenate(bases).view('S1'))
    ones = np.ones(4 ** k, np.int64)
    ns = len(site_pos)
    sites = (np.array(['chrT'] * (2 * ns)), np.array(['+'] * ns + ['-'] * ns), np.concatenate((site_pos, site_pos)))
    return (reads, dict(k=k, center=center, mean=mean, sd=sd, n_positions=ones), dict(k=k, center=center, mean=mean1, sd=sd.copy(), n_positions=ones),
            sites, planted)


@pytest.fixture(scope='module')
def chain():
    reads, model, alt, sites, planted = _two_kinds_of_sites()
    exp = RF.restate(reads['norm_mean'], reads['off'], reads['base'], model['k'], model['center'], model['mean'], model['sd'], alt['mean'], alt['sd'],
                     'kmer', H.CHAIN_THR, 0.0)
    cs = (reads['strand'] == '-').astype(np.int32)
    key = np.unique(np.array([_key(0 if s == '+' else 1, p) for s, p in zip(sites[1], sites[2])], np.int64))
    return dict(reads=reads, model=model, alt=alt, sites=sites, planted=planted, walk=(cs, reads['start'], reads['off'], exp['llr_win'], key), key=key)


def test_end_to_end_through_smooth_reads_llr(chain):
    from nanomod_amd import readllr
    lines = []
    res = readllr.smooth_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], length=50.0, call_post=CALL_POST, thr=H.CHAIN_THR,
                                   decode='both', fit='mle', site_prior=True, log=lines.append)
    sp, fit = res['site_prior'], res['fit']
    ns = len(chain['key'])
    assert set(sp) == {'chrom', 'strand', 'pos', 'pi_hat', 'n_valid', 'prior'} and all(len(sp[f]) == ns for f in sp)
    assert any(l.startswith('readhmm: per-site prior: ') for l in lines) and len(lines) == 4
    # the fit reports the length alone; pi is the mean it was given
    assert fit['status'].startswith('length fitted alone: pi is fixed') and fit['pi'] == res['pi'] and np.isnan(fit['se_eta']) and fit['length'] == res['length']
    known = ~np.isnan(sp['pi_hat'])
    assert known.sum() > ns // 2 and abs(res['pi'] - sp['pi_hat'][known].mean()) <= 1e-12
    assert same(sp['prior'], readllr.site_prior(sp['pi_hat'], sp['n_valid'], res['pi'], 4.0)) and np.all(sp['n_valid'][known] >= 3)
    half = ns // 2
    hot = np.zeros(ns, bool)
    hot[HOT[0]:HOT[1]] = hot[half + HOT[0]:half + HOT[1]] = True
    print('priors: hot sites %.3f, the others %.3f' % (np.nanmean(sp['prior'][hot]), np.nanmean(sp['prior'][~hot])))
    assert np.nanmean(sp['prior'][hot]) > 3.0 * np.nanmean(sp['prior'][~hot])   # the stretches sit on sites of a high and of a low share
    # the three entries ran with these shares: the restatement at the same shares, pi and length
    ref = P.read_prior_ref(*chain['walk'], sp['prior'], res['pi'], res['length'], CALL_POST)
    flat = dict(res['entries'], **res['reads'], site_n=res['sites']['n'], site_mod=res['sites']['n_mod'], site_can=res['sites']['n_can'])
    assert _check_hmm(flat, ref) <= 0.05
    v = res['viterbi']
    vit = dict(v['entries'], **v['reads'], site_n=v['sites']['n'], site_mod=v['sites']['n_mod'])
    assert _check_vit(vit, dict(ref=ref, key=chain['key'], length=res['length'])) <= 0.05
    # and not with one share: the plain chain at the same pi and length calls other entries
    plain = readllr.smooth_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], pi=res['pi'], length=res['length'],
                                     call_post=CALL_POST, thr=H.CHAIN_THR, log=lambda *a: None)
    assert 'site_prior' not in plain and same(plain['entries']['hoff'], res['entries']['hoff']) and not same(plain['entries']['post'], res['entries']['post'])


def test_the_command_line_writes_the_priors_and_changes_nothing_without_the_option(chain):
    from nanomod_amd import cli, container, kmermodel, readllr
    reads = chain['reads']
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, a_path, s_path = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'alt.npz', 'sites.txt'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        for path, m in ((m_path, chain['model']), (a_path, chain['alt'])):
            kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
        open(s_path, 'w').writelines('%s %s %d\n' % (c, s, p + 1) for c, s, p in zip(*chain['sites']))
        argv = ['readhmm', '--wrkBase1', r_path, '--model', m_path, '--altModel', a_path, '--sites', s_path, '--hmmLength', '50', '--callPost', repr(CALL_POST),
                '--decode', 'both', '--fitHmm', '1', '--FileID', 'run', '--outLevel', '3']
        dirs = {n: os.path.join(tmp, n) for n in ('prior', 'none', 'zero')}
        assert cli.main(argv + ['--outFolder', dirs['prior'], '--sitePrior', '1', '--priorReads', '4']) == 0
        assert cli.main(argv + ['--outFolder', dirs['none']]) == 0
        assert cli.main(argv + ['--outFolder', dirs['zero'], '--sitePrior', '0']) == 0
        names = sorted(os.listdir(dirs['none']))
        assert names == sorted('run' + s for s in ('_hmm_fit.txt', '_read_hmm.txt', '_read_domains.txt', '_site_hmm.txt', '_read_viterbi.txt',
                                                   '_read_domains_viterbi.txt', '_site_viterbi.txt'))
        assert sorted(os.listdir(dirs['prior'])) == sorted(names + ['run_site_prior.txt']) and sorted(os.listdir(dirs['zero'])) == names
        kw = dict(sites=chain['sites'], length=50.0, call_post=CALL_POST, decode='both', fit='mle', log=lambda *a: None)
        want = readllr.smooth_reads_llr(reads, chain['model'], chain['alt'], fix_pi=False, **kw)      # the same call, without the option
        for n, (suffix, write, arg) in zip(names, sorted((('_hmm_fit.txt', readllr.write_hmm_fit, want['fit']), ('_read_hmm.txt', readllr.write_read_hmm, want),
                                                          ('_read_domains.txt', readllr.write_read_domains, want), ('_site_hmm.txt', readllr.write_site_hmm, want),
                                                          ('_read_viterbi.txt', readllr.write_read_viterbi, want['viterbi']),
                                                          ('_read_domains_viterbi.txt', readllr.write_read_domains, want['viterbi']),
                                                          ('_site_viterbi.txt', readllr.write_site_viterbi, want['viterbi'])), key=lambda x: 'run' + x[0])):
            assert n == 'run' + suffix
            write(os.path.join(tmp, 'want.txt'), arg)
            assert filecmp.cmp(os.path.join(dirs['none'], n), os.path.join(tmp, 'want.txt'), shallow=False), n
            assert filecmp.cmp(os.path.join(dirs['none'], n), os.path.join(dirs['zero'], n), shallow=False), n
        assert not filecmp.cmp(os.path.join(dirs['none'], 'run_read_hmm.txt'), os.path.join(dirs['prior'], 'run_read_hmm.txt'), shallow=False)
        res = readllr.smooth_reads_llr(reads, chain['model'], chain['alt'], site_prior=True, prior_reads=4.0, **kw)
        readllr.write_site_prior(os.path.join(tmp, 'want.txt'), res)
        text = open(os.path.join(dirs['prior'], 'run_site_prior.txt')).read()
        assert text == open(os.path.join(tmp, 'want.txt')).read() and len(text.splitlines()) == len(chain['key'])
        row = text.splitlines()[0].split()
        sp = res['site_prior']
        assert row[:3] == ['chrT', '+', str(int(sp['pos'][0]) + 1)] and int(row[3]) == sp['n_valid'][0] and len(row) == 6
        fit = open(os.path.join(dirs['prior'], 'run_hmm_fit.txt')).read()
        assert 'status length fitted alone: pi is fixed' in fit and 'status pi and length fitted' in open(os.path.join(dirs['none'], 'run_hmm_fit.txt')).read()
