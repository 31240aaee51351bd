"""GPU: the forms of the chain entries (K19 - K22) that full tiles and one table size leave unseen, on tests/chain_cases.py's inputs
(tests/test_chain_cases.py proves their properties without a device): the fill of the rows under holes of whole waves and tiles in
both of its forms, through nmod_read_hmm, nmod_read_viterbi and nmod_read_class_rows against their restatements; every number of
passes of nmod_read_class_rows' sort, byte for byte, and a step of K22 on those rows; rows that no read owns.  Floats are compared
within the gates hmm_ref, viterbi_ref and classes_ref derive (through the checks of the entries' own test files), all else as bytes."""
import time

import numpy as np
import pytest

import chain_cases as CC
import classes_ref as K
import hmm_ref as H
import test_read_classes_gpu as TC
import test_read_hmm_gpu as TH
import test_read_viterbi_gpu as TV
import viterbi_ref as V
from nanomod_amd import _lib as L
from test_read_classes_gpu import same

pytestmark = pytest.mark.gpu

WALK = CC.WALK
ROWS = L.CLASS_ROWS_FIELDS
assert (TH.PI, TH.LENGTH, TH.CALL_POST) == (CC.PI, CC.LENGTH, CC.CALL_POST) and (TV.PI, TV.LENGTH) == (CC.PI, CC.LENGTH) and TC.WALK == WALK


@pytest.fixture(scope='module')
def det():
    return TC._engine().DeviceDetector(0)


def _walk(c):
    return [c[f] for f in WALK]


def _walk_t(c):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(c[f])).cuda() for f in WALK]


# ------------------------------------------------------------------------------------------------------------ entries with holes
@pytest.fixture(scope='module')
def holes():
    c = CC.hole_reads()
    return dict(c, alone=CC.longest_of_each_pattern(c), **{f: c[f].copy() for f in WALK})   # (the case itself is read-only)


def test_the_fill_under_holes_through_the_smoothing(det, holes):
    """nmod_read_sites_count and nmod_read_hmm: hoff and site byte for byte, post / ll / ll_indep within hmm_ref's gates, states and
    counts as test_read_hmm_gpu checks them, no entry left to the device's choice; the host memspace and a read alone: the same bytes"""
    ref = H.read_hmm_ref(*_walk(holes), CC.PI, CC.LENGTH, CC.CALL_POST)
    res = TH._device(det, holes)
    assert set(res) == set(TH.ALL) | {'hoff'} and same(ref['hoff'], holes['hoff']) and len(ref['post']) > 25000
    assert TH._check(res, ref) == 0.0
    m, events = np.diff(ref['hoff']), np.diff(holes['roff'])
    none = (m == 0) & (events > CC.EVENTS_MAX)                                # long reads without an entry
    assert none.sum() >= 8 and np.all(res['status'][none] == L.HMM_NO_SITE) and np.all(res['ll'][none] == 0.0) and np.all(res['n_sites'][none] == 0)
    assert ((events > CC.EVENTS_MAX) & (m > 0) & (m <= CC.ENTRIES_MAX)).sum() >= 20 and ((events <= CC.EVENTS_MAX) & (m > CC.ENTRIES_MAX)).sum() >= 2
    eng = TC._engine()
    hoff = eng.read_sites_host(*_walk(holes))
    assert same(hoff, res['hoff'])
    host = eng.read_hmm_host(*_walk(holes), hoff, pi=CC.PI, length=CC.LENGTH, call_post=CC.CALL_POST)
    for f in TH.ALL:
        assert same(host[f], res[f]), f
    for r in holes['alone']:
        alone = TH._device(det, TH._case([holes['reads'][r]], holes['key']))
        for f in TH.ENTRY:
            assert same(alone[f], res[f][res['hoff'][r]:res['hoff'][r + 1]]), (r, f)
        for f in TH.READ:
            assert same(alone[f], res[f][r:r + 1]), (r, f)


def test_the_fill_under_holes_through_the_class_rows(det, holes):
    """nmod_read_class_rows: s is the only direct view of the score the fill wrote (post depends on the row it wrote to)"""
    ref = K.rows_ref(*_walk(holes))
    rows_t, hoff_t = TC._device_rows(det, holes)
    got = TC._rows_np(rows_t, hoff_t)
    for f in ('hoff',) + ROWS:
        assert same(got[f], ref[f]), f
    k19 = det.read_hmm(*_walk_t(holes), hoff_t, len(ref['s']), want=('site',))['site'].cpu().numpy()
    assert same(got['site'], k19)
    host = TC._engine().read_class_rows_host(*_walk(holes))
    for f in ('hoff',) + ROWS:
        assert same(host[f], got[f]), f
    for r in holes['alone']:
        one = TC._case([holes['reads'][r]], holes['key'])
        at, ah = TC._device_rows(det, one)
        alone = TC._rows_np(at, ah)
        a, b = int(ref['hoff'][r]), int(ref['hoff'][r + 1])
        assert same(alone['site'], got['site'][a:b]) and same(alone['s'], got['s'][a:b]) and same(alone['rread'], np.zeros(b - a, np.int32)), r
        assert same(alone['srow'], np.arange(b - a, dtype=np.int32)) and alone['soff'][-1] == b - a


def test_the_fill_under_holes_through_the_decoding(det, holes):
    """nmod_read_viterbi as test_read_viterbi_gpu checks its constructed reads: the device's path scored by mpmath, vit and delta within
    viterbi_ref's gate, the path the reference's wherever its margin is clear (everywhere: the restatement has no near decision here)"""
    ref = V.read_viterbi_ref(*_walk(holes), CC.PI, CC.LENGTH, exact=True)
    res = TV._device(det, holes)
    assert TV._check(res, ref) == 0.0 and ref['near'].sum() == 0
    for r in holes['alone']:
        alone = TV._device(det, TV._case([holes['reads'][r]], holes['key']))
        for f in TV.ENTRY:
            assert same(alone[f], res[f][res['hoff'][r]:res['hoff'][r + 1]]), (r, f)
        for f in TV.READ:
            assert same(alone[f], res[f][r:r + 1]), (r, f)


# ------------------------------------------------------------------------------------------------------------ the sort passes
def _rows_against_numpy(got, nsites):
    soff = np.zeros(nsites + 1, np.int64)
    soff[1:] = np.cumsum(np.bincount(got['site'], minlength=nsites))
    assert same(got['soff'], soff) and same(got['srow'], np.argsort(got['site'], kind='stable').astype(np.int32))


@pytest.mark.parametrize('nsites', CC.SORT_NSITES)
def test_every_number_of_sort_passes_gives_the_restatement_s_rows(det, nsites):
    """1, 2, 2, 3, 3 and 4 passes: after an odd number the result lands in the sort's second buffers, which srow (or the slab's spare,
    where the caller asks for none) must then be.  Up to 70 000 sites also the host memspace and one step of K22 on the device's rows;
    2^24 + 3 sites (key and soff of 134 MB each) on the device alone."""
    import torch
    _, reads, key = CC.sort_pass_case(nsites)
    c = CC.case_arrays(reads, key)
    ref = K.rows_ref(*_walk(c))
    t = _walk_t(c)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hoff_t, nrows = det.read_sites(*t)
    rows_t = det.read_class_rows(*t, hoff_t, nrows)
    torch.cuda.synchronize()
    print('%d sites, %d pass(es), %d rows: read_sites and read_class_rows took %.1f ms' % (nsites, CC.sort_passes(nsites), nrows, 1e3 * (time.perf_counter() - t0)))
    got = TC._rows_np(rows_t, hoff_t)
    for f in ('hoff',) + ROWS:
        assert same(got[f], ref[f]), f
    _rows_against_numpy(got, nsites)
    for want in (('srow',), ('soff',), ('s', 'rread'), ('site', 'srow')):
        part = det.read_class_rows(*t, hoff_t, nrows, want=want)
        assert set(part) == set(want)
        for f in want:
            assert same(part[f].cpu().numpy(), ref[f]), (want, f)
    if nsites > CC.SORT_HOST_MAX:
        return
    host = TC._engine().read_class_rows_host(*_walk(c))
    for f in ('hoff',) + ROWS:
        assert same(host[f], ref[f]), f
    rng = np.random.default_rng(2310 + nsites % 1000)
    theta, w = rng.uniform(0.05, 0.95, (nsites, 2)), np.array([0.4, 0.6])
    res = TC._step(det, rows_t, hoff_t, theta, w)
    a = K.step_ref(ref, theta, w)
    assert same(res['cls'], a['cls']) and same(res['status'], a['status'])
    per = np.diff(ref['soff'])
    multi = np.flatnonzero(per >= 3)
    assert len(multi) >= 10
    gamma = res['gamma'].reshape(-1, 2)
    for j in (multi[0], multi[len(multi) // 2], multi[-1]):
        lst = ref['srow'][ref['soff'][j]:ref['soff'][j + 1]]
        N, _ = K.site_ref(ref['s'][lst], gamma[ref['rread'][lst]], theta[j])
        assert same(res['n_site'].reshape(-1, 2)[j], N), j


# ------------------------------------------------------------------------------------------------------------ rows no read owns
@pytest.mark.parametrize('nsites', [255, 65535])
def test_rows_that_no_read_owns_sort_behind_every_site(det, nsites):
    """The device memspace does not read hoff back: with nrows above hoff[nreads] the rows beyond keep site -1, s 0.0 and rread -1,
    their sort key is nsites itself (what the pass count is chosen for), they come last in srow in ascending row index, and
    soff[nsites] stays hoff[nreads]; the owned rows and a step over all of them have the exact call's bytes"""
    import torch
    _, reads, key = CC.sort_pass_case(nsites)
    c = CC.case_arrays(reads, key)
    t = _walk_t(c)
    hoff_t, owned = det.read_sites(*t)
    exact = {f: v.cpu().numpy() for f, v in det.read_class_rows(*t, hoff_t, owned).items()}
    ref = K.rows_ref(*_walk(c))
    for f in ROWS:
        assert same(exact[f], ref[f]), f
    extra = 5
    out = dict(site=torch.full((owned + extra,), 77, dtype=torch.int32, device='cuda'), s=torch.full((owned + extra,), 77.0, dtype=torch.float64, device='cuda'),
               rread=torch.full((owned + extra,), 77, dtype=torch.int32, device='cuda'), soff=torch.full((nsites + 1,), 77, dtype=torch.int64, device='cuda'),
               srow=torch.full((owned + extra,), 77, dtype=torch.int32, device='cuda'))
    more_t = det.read_class_rows(*t, hoff_t, owned + extra, out=out)
    more = {f: v.cpu().numpy() for f, v in more_t.items()}
    assert int(hoff_t[-1]) == owned and all(len(more[f]) == owned + extra for f in ('site', 's', 'rread', 'srow'))
    assert np.all(more['site'][owned:] == -1) and same(more['s'][owned:], np.zeros(extra)) and np.all(more['rread'][owned:] == -1)
    assert same(more['srow'][owned:], np.arange(owned, owned + extra, dtype=np.int32)) and more['soff'][nsites] == owned
    for f in ('site', 's', 'rread', 'srow'):
        assert same(more[f][:owned], exact[f]), f
    assert same(more['soff'], exact['soff'])
    for want in (('srow',), ('soff',)):                                       # the slab's own srow and counts, under both parities
        part = det.read_class_rows(*t, hoff_t, owned + extra, want=want)
        assert same(part[want[0]].cpu().numpy(), more[want[0]]), want
    rng = np.random.default_rng(2320 + nsites % 1000)
    theta, w = rng.uniform(0.05, 0.95, (nsites, 2)), np.array([0.4, 0.6])
    want = TC._step(det, {f: torch.from_numpy(exact[f]).cuda() for f in ROWS}, hoff_t, theta, w)
    got = TC._step(det, more_t, hoff_t, theta, w)
    for f in TC.ALL:
        assert same(got[f], want[f]), f
    assert got['sums'][2] == owned
