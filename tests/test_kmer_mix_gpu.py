"""-m gpu: nmod_kmer_mix (K17) on the device against the restatement of tests/kmix_ref.py — the histogram and the counts as exact
integers, the EM at K8's tolerances, the bits between device runs, the stream contract, and the way up through
kmermodel.learn_alt_model, readllr.call_reads_llr and the command line."""
import os
import tempfile

import numpy as np
import pytest

import kmix_ref as R

pytestmark = pytest.mark.gpu

ROW_SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 200, 2049)          # rows start at odd 2-byte offsets; 2 049: more than two steps of a wave
DTYPES = {'i16': np.int16, 'f32': np.float32, 'f64': np.float64}
COUNTS = ('n_positions', 'n_used', 'n_outside')
_cache = {}


def _engine():
    from nanomod_amd import engine
    return engine


def _det():
    if 'det' not in _cache:
        _cache['det'] = _engine().DeviceDetector(0)
    return _cache['det']


def _as(k, dtype):
    """integers k of the 0.001 grid as samples of `dtype`"""
    k = np.asarray(k)
    return k.astype(np.int16) if dtype == 'i16' else (k.astype(np.float64) / 1000.0).astype(DTYPES[dtype])


def _device(sig, code, ncodes, mean0, sd0, off=None, stride=0, want_hist=True, **kw):
    import torch
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
    res = _det().kmer_mix(dev(sig), dev(np.asarray(code, np.int32)), ncodes, dev(np.asarray(mean0, np.float64)), dev(np.asarray(sd0, np.float64)),
                          off=dev(off), stride=stride, want_hist=want_hist, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if 'hist' in out:
        out['hist'] = out['hist'].view(np.uint32)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _same(a, b, fields=None):
    return [k for k in (fields or sorted(set(a) & set(b))) if _bits(a[k]) != _bits(b[k])]


def _check_integers(got, want, ncodes, what):
    for f in COUNTS:
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:8])
    assert np.array_equal(got['pos_status'], want['pos_status']), (what, np.flatnonzero(got['pos_status'] != want['pos_status'])[:8])
    if 'hist' in got:
        assert np.array_equal(got['hist'].reshape(ncodes, R.BINS), want['hist']), what
    unusable = ~want['usable']
    assert np.all(got['status'][unusable] == R.NO_MODEL) and np.all((got['status'][~unusable] & R.NO_MODEL) == 0), what
    few = ~unusable & (want['n_used'] < 2)
    assert np.all(got['status'][few] == R.TOO_FEW) and np.all(got['iters'][few] == 0) and np.isnan(got['pi'][few]).all(), what


# ------------------------------------------------------------------------------------------------------ histogram, exact
def hist_batch(ncodes, dtype, seed=0):
    """ragged rows over `ncodes` codes with every edge of the definition: (sig, off, code, mean0, sd0)"""
    rng = np.random.default_rng(1000 * ncodes + seed)
    mean0 = np.round(rng.uniform(-20.0, 20.0, ncodes), 3)
    sd0 = np.full(ncodes, 0.2)
    if ncodes >= 64:
        mean0[7], sd0[8], mean0[9] = np.nan, 0.0, 2000.0                       # unusable codes with positions
        mean0[10], mean0[11] = 30.0, -30.0                                     # windows next to +-32 767
    lo = R.window_lo(mean0)
    rows, code = [], []

    def add(c, n, k=None):
        centre = np.clip(1000.0 * np.nan_to_num(mean0[c]), -30000.0, 30000.0)
        k = np.rint(centre + 300.0 * rng.standard_normal(n)) if k is None else np.asarray(k, np.float64)
        rows.append(np.clip(k, -32767, 32767)); code.append(c)
    plan = []
    if ncodes == 1:
        plan = [(0, R.CHUNK + 1 + len(ROW_SIZES))]
    else:
        plan = [(0, R.CHUNK), (1, R.CHUNK + 1), (2, 1), (3 % ncodes, 2 * R.CHUNK + 3)]              # one item, two items, a single position
        plan += [(c, int(rng.integers(1, 6))) for c in range(4, min(ncodes, 40), 3)] + [(c, 2) for c in range(7, min(ncodes, 12))]
        if ncodes > 64:
            plan += [(ncodes - 1, 3), (ncodes // 2, 2)]                        # (most codes are never seen)
    i = 0
    for c, npos in plan:
        for _ in range(npos):
            add(c, ROW_SIZES[i % len(ROW_SIZES)] if npos > 1 else 9)
            i += 1
    c = 0                                                                      # the window's edges and the range's
    add(c, 0, [lo[c] - 1, lo[c], lo[c] + R.BINS - 1, lo[c] + R.BINS, -32767, 32767, lo[c]])
    add(-1, 5)
    for r, n in enumerate(ROW_SIZES[:4]):                                      # code -1 takes rows of every size along
        add(-1, n)
    order = rng.permutation(len(rows))
    rows, code = [rows[j] for j in order], np.asarray(code, np.int32)[order]
    sig, off = R.csr([_as(r, dtype) for r in rows], DTYPES[dtype])
    if dtype != 'i16':                                                         # a NaN, an inf and two halfway samples in rows that take part
        usable_rows = [j for j in range(len(rows)) if code[j] >= 0 and len(rows[j]) >= 8 and R.usable(mean0, sd0)[code[j]]]
        a, b = usable_rows[0], usable_rows[1]
        sig[off[a] + 1], sig[off[a] + 5], sig[off[b]] = np.nan, np.inf, -np.inf
        base = np.floor(mean0[code[b]])
        sig[off[b] + 2], sig[off[b] + 3] = base + 1.0 / 16.0, base + 3.0 / 16.0   # 1000 x = .. 062.5 and .. 187.5 exactly: ties to even
    return sig, off, code, mean0, sd0


@pytest.mark.parametrize('ncodes', [1, 4, 64, 4096])
@pytest.mark.parametrize('dtype', ['i16', 'f32', 'f64'])
def test_histogram_and_counts_are_the_restated_integers(dtype, ncodes):
    sig, off, code, mean0, sd0 = hist_batch(ncodes, dtype)
    want = R.hist(sig, off, code, ncodes, mean0, sd0)
    assert want['n_used'].sum() > 1000 and want['n_outside'].sum() > 0
    if dtype != 'i16':
        assert (want['pos_status'] == R.ST_NONFINITE).sum() == 2
    got = _engine().kmer_mix_host(sig, off, code, ncodes, mean0, sd0, want_hist=True, max_iter=5)
    _check_integers(got, want, ncodes, 'host %s %d' % (dtype, ncodes))
    dev = _device(sig, code, ncodes, mean0, sd0, off=off, max_iter=5)
    _check_integers(dev, want, ncodes, 'device %s %d' % (dtype, ncodes))
    assert not _same(got, dev)


def test_device_memory_codes_outside_the_table_take_no_part():
    sig, off, code, mean0, sd0 = hist_batch(64, 'i16', seed=1)
    code = code.copy()
    hit = np.flatnonzero(code >= 0)[:6]
    code[hit[:3]], code[hit[3:]] = 64, -7
    want = R.hist(sig, off, code, 64, mean0, sd0)
    assert (want['pos_status'][hit] & R.ST_NO_CODE).all()
    _check_integers(_device(sig, code, 64, mean0, sd0, off=off, max_iter=5), want, 64, 'codes outside')


def test_65536_codes_three_of_them_populated():
    import torch
    ncodes = 65536
    rng = np.random.default_rng(65536)
    mean0, sd0 = np.round(rng.uniform(-5.0, 5.0, ncodes), 3), np.full(ncodes, 0.2)
    pop = np.array([0, 40000, 65535])
    code = np.repeat(pop, [300, 5, 257]).astype(np.int32)
    rows = [np.rint(1000.0 * mean0[c] + 200.0 * rng.standard_normal(int(rng.integers(1, 80)))) for c in code]
    order = rng.permutation(len(rows))
    sig, off = R.csr([rows[j] for j in order])
    code = code[order]
    det = _det()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
    res = det.kmer_mix(dev(sig), dev(code), ncodes, dev(mean0), dev(sd0), off=dev(off), want_hist=True, max_iter=20)
    torch.cuda.synchronize()
    sub = R.hist(sig, off, np.searchsorted(pop, code), 3, mean0[pop], sd0[pop])
    h = res['hist'].view(ncodes, R.BINS)
    assert int(h.sum()) == int(sub['n_used'].sum()) and int(res['n_used'].sum()) == int(sub['n_used'].sum())
    assert np.array_equal(h[dev(pop)].cpu().numpy().view(np.uint32), sub['hist'])
    for f in COUNTS:
        assert np.array_equal(res[f][dev(pop)].cpu().numpy(), sub[f]), f
    status = res['status'].cpu().numpy()
    assert (np.delete(status, pop) == R.TOO_FEW).all() and not (status[pop] & (R.TOO_FEW | R.NO_MODEL)).any()
    for j, c in enumerate(pop):
        o = R.em(sub['hist'][j], sub['lo'][j], mean0[c], sd0[c], R.FREE, int(res['iters'][c]))
        assert abs(float(res['pi'][c]) - o['pi']) <= 1e-9 * o['pi'] and abs(float(res['mu_mod'][c]) - o['mu_mod']) <= 1e-9 * sd0[c]


def test_more_items_than_any_persistent_grid():
    """20 000 positions x 3 samples over 64 codes in stride form: some 100 items of the histogram kernel beside 64 ragged ones, and a
    second batch of 2 000 000 one-sample positions — 7 800 items, more than 8 workgroups on each of 256 CUs"""
    rng = np.random.default_rng(20000)
    mean0, sd0 = np.round(rng.uniform(-3.0, 3.0, 64), 3), np.full(64, 0.2)
    code = rng.integers(-1, 64, 20000).astype(np.int32)
    sig = np.rint(1000.0 * mean0[np.maximum(code, 0)][:, None] + 200.0 * rng.standard_normal((20000, 3))).astype(np.int16).reshape(-1)
    want = R.hist(sig, np.arange(20001) * 3, code, 64, mean0, sd0)
    got = _device(sig, code, 64, mean0, sd0, stride=3, max_iter=5)
    _check_integers(got, want, 64, 'stride 3')
    n = 2000000
    code = (np.arange(n) % 4).astype(np.int32)
    sig = (np.arange(n) % 4001 - 2000).astype(np.int16)
    got = _device(sig, code, 4, np.zeros(4), np.full(4, 0.2), stride=1, max_iter=2)
    for c in range(4):
        k = sig[c::4].astype(np.int64)
        assert np.array_equal(got['hist'].reshape(4, R.BINS)[c], np.bincount(k + R.HALF, minlength=R.BINS))
        assert got['n_used'][c] == n // 4 == got['n_positions'][c] and got['n_outside'][c] == 0


# ------------------------------------------------------------------------------------------------------------ EM parity
def _parity():
    if 'parity' not in _cache:
        rows, code, mean0, sd0 = R.parity_inputs()
        sig, off = R.csr(rows)
        _cache['parity'] = (sig, off, code, mean0, sd0, R.hist(sig, off, code, 64, mean0, sd0))
    return _cache['parity']


def _check_em(got, want, mean0, sd0, model, max_iter, tol, what, min_samples=2):
    """tests/test_mix_gpu.py::_check carried over: K8's tolerances at the device's own iteration count, its band for the stopping rule"""
    exempt = computed = 0
    for c in range(len(mean0)):
        tag = '%s code %d (n_used %d)' % (what, c, want['n_used'][c])
        it, st = int(got['iters'][c]), int(got['status'][c])
        if want['n_used'][c] < max(min_samples, 2):
            assert st == R.TOO_FEW and it == 0 and all(np.isnan(got[k][c]) for k in R.FIELDS), tag
            continue
        assert st & ~(R.NOT_CONVERGED | R.VAR_FLOORED) == 0 and 1 <= it <= max_iter, (tag, st, it)
        o = R.em(want['hist'][c], want['lo'][c], mean0[c], sd0[c], model, it)
        assert o['status'] & ~R.VAR_FLOORED == 0, tag
        g = {k: float(got[k][c]) for k in R.FIELDS}
        print('%s: iters %d status %d  err pi %.2e sd %.2e mu/s %.2e llr %.2e' % (
            tag, it, st, abs(g['pi'] - o['pi']), abs(g['sd_mod'] - o['sd_mod']), abs(g['mu_mod'] - o['mu_mod']) / sd0[c], abs(g['llr'] - o['llr'])))
        assert abs(g['pi'] - o['pi']) <= 1e-9 * o['pi'] and abs(g['pi'] - o['pi']) <= 1e-12, (tag, g['pi'], o['pi'])
        assert abs(g['sd_mod'] - o['sd_mod']) <= 1e-9 * o['sd_mod'], (tag, g['sd_mod'], o['sd_mod'])
        assert abs(g['mu_mod'] - o['mu_mod']) <= 1e-9 * sd0[c], (tag, g['mu_mod'], o['mu_mod'])
        if np.isnan(o['llr']):                                   # (pi rounded to 1: ln 0 + softplus(inf), in the definition itself)
            assert np.isnan(g['llr']), tag
        else:
            assert abs(g['llr'] - o['llr']) <= 1e-9 * abs(o['llr']) + 1e-9, (tag, g['llr'], o['llr'])
        assert bool(st & R.VAR_FLOORED) == bool(o['status'] & R.VAR_FLOORED), tag
        computed += 1
        band = lambda dl: tol > 0.0 and abs(dl - tol) <= 1e-6 * tol
        if band(o['delta']) or (it > 1 and band(o['delta_prev'])):
            exempt += 1
            continue
        stops = tol > 0.0 and o['delta'] <= tol
        if st & R.NOT_CONVERGED:
            assert it == max_iter and not stops, (tag, o['delta'])
        else:
            assert stops, (tag, o['delta'])
        if it > 1:
            assert not (tol > 0.0 and o['delta_prev'] <= tol), (tag, o['delta_prev'])
    assert exempt <= 0.01 * len(mean0), exempt
    return computed


@pytest.mark.parametrize('max_iter', [50, 200])
@pytest.mark.parametrize('model', [R.EQUAL, R.FREE])
def test_em_parity_with_the_restatement(model, max_iter):
    sig, off, code, mean0, sd0, want = _parity()
    assert want['n_used'].min() == 2 and want['n_used'].max() >= 150000
    got = _device(sig, code, 64, mean0, sd0, off=off, model=model, max_iter=max_iter, tol=1e-6)
    _check_integers(got, want, 64, 'parity')
    assert _check_em(got, want, mean0, sd0, model, max_iter, 1e-6, 'model %d max_iter %d' % (model, max_iter)) >= 60
    stopped = (got['status'] & R.NOT_CONVERGED) == 0
    assert stopped.any() and (max_iter == 200 or (~stopped).any())             # some codes stop and some do not


def test_tol_zero_runs_exactly_max_iter():
    sig, off, code, mean0, sd0, want = _parity()
    got = _device(sig, code, 64, mean0, sd0, off=off, model=R.FREE, max_iter=37, tol=0.0, want_hist=False)
    assert (got['iters'] == 37).all() and ((got['status'] & R.NOT_CONVERGED) != 0).all()
    _check_em(got, want, mean0, sd0, R.FREE, 37, 0.0, 'tol 0')


def test_too_few_and_the_variance_floor():
    mean0, sd0 = np.array([0.0, 0.5, 1.0, 1.5, 2.0]), np.full(5, 0.2)
    lo = R.window_lo(mean0)
    rows = [[9000], [510], [1010, 990, 1000] * 3, [1500] * 10, [lo[4] + 3900] * 40 + [lo[4] + 3901] * 60]       # n_used 0, 1, 9, 10, 100
    sig, off = R.csr(rows)
    code = np.arange(5, dtype=np.int32)
    want = R.hist(sig, off, code, 5, mean0, sd0)
    assert list(want['n_used']) == [0, 1, 9, 10, 100]
    got = _device(sig, code, 5, mean0, sd0, off=off, min_samples=10)
    _check_integers(got, want, 5, 'too few')
    assert list(got['status'][:3]) == [R.TOO_FEW] * 3 and not (got['status'][3:] & R.TOO_FEW).any()
    assert np.isnan(got['pi'][:3]).all() and not got['iters'][:3].any()
    _check_em(got, want, mean0, sd0, R.FREE, 200, 1e-6, 'floor', min_samples=10)
    assert got['status'][4] & R.VAR_FLOORED and got['sd_mod'][4] == pytest.approx(0.05, rel=1e-12) and got['pi'][4] > 0.999


# ------------------------------------------------------------------------------------------- bit for bit between device runs
PER_CODE = COUNTS + R.FIELDS + ('iters', 'status')


def test_bits_do_not_depend_on_order_layout_memspace_batch_or_dtype():
    rng = np.random.default_rng(4242)
    npos, n, ncodes = 3000, 40, 16
    mean0, sd0 = np.round(rng.uniform(-3.0, 3.0, ncodes), 3), np.round(rng.uniform(0.15, 0.3, ncodes), 3)
    code = rng.integers(-1, ncodes, npos).astype(np.int32)
    x = mean0[np.maximum(code, 0)][:, None] + sd0[np.maximum(code, 0)][:, None] * rng.standard_normal((npos, n))
    x += (rng.random((npos, n)) < 0.3) * 0.8
    sig = np.rint(1000.0 * x).astype(np.int16).reshape(-1)
    off = np.arange(npos + 1, dtype=np.int64) * n
    kw = dict(model=R.FREE, max_iter=60, tol=1e-6)
    base = _device(sig, code, ncodes, mean0, sd0, off=off, **kw)
    assert (base['n_used'] > 4000).all() and (base['iters'] > 3).all()
    order = rng.permutation(npos)
    perm = _device(sig.reshape(npos, n)[order].reshape(-1), code[order], ncodes, mean0, sd0, off=off, **kw)
    assert not _same(base, perm, PER_CODE + ('hist',)) and np.array_equal(perm['pos_status'], base['pos_status'][order])
    assert not _same(base, _device(sig, code, ncodes, mean0, sd0, stride=n, **kw))                         # CSR against stride
    host = _engine().kmer_mix_host(sig, off, code, ncodes, mean0, sd0, want_hist=True, **kw)              # host against device memory
    assert not _same(base, host)
    assert not _same(base, _device(sig, code, ncodes, mean0, sd0, off=off, want_hist=False, **kw))         # hist requested or not
    extra = 5000                                                                                           # other codes appended
    more_code = np.concatenate([code, rng.integers(ncodes, 2 * ncodes, extra).astype(np.int32)])
    more_sig = np.concatenate([sig, rng.integers(-3000, 3000, extra * n).astype(np.int16)])
    more = _device(more_sig, more_code, 2 * ncodes, np.concatenate([mean0, mean0]), np.concatenate([sd0, sd0]), stride=n, **kw)
    assert not [f for f in PER_CODE if _bits(more[f][:ncodes]) != _bits(base[f])]
    assert _bits(more['hist'][:ncodes * R.BINS]) == _bits(base['hist']) and (more['n_used'][ncodes:] > 0).all()
    f64 = _device(sig.astype(np.float64) / 1000.0, code, ncodes, mean0, sd0, off=off, **kw)                # int16 rows against float64
    assert not _same(base, f64)
    f32 = _device((sig.astype(np.float64) / 1000.0).astype(np.float32), code, ncodes, mean0, sd0, off=off, **kw)
    assert not _same(base, f32)


# ------------------------------------------------------------------------------------------------------ the stream contract
def test_the_device_entry_runs_on_its_stream_and_waits_for_nothing():
    """the pattern of tests/test_stream_contract_gpu.py: behind a bounded stall on a fresh stream the real inputs are put in place, the
    entry is enqueued and a decoy is written behind it; the call returns while the stall runs, and the result is the real batch's"""
    import torch
    import stream_cases as S
    rng = np.random.default_rng(99)
    npos, n, ncodes = 4000, 30, 16

    def batch(shift):
        mean0, sd0 = np.round(rng.uniform(-3.0, 3.0, ncodes), 3), np.full(ncodes, 0.2)
        code = rng.integers(-1, ncodes, npos).astype(np.int32)
        x = mean0[np.maximum(code, 0)][:, None] + 0.2 * rng.standard_normal((npos, n)) + (rng.random((npos, n)) < 0.4) * shift
        return dict(sig=np.rint(1000.0 * x).astype(np.int16).reshape(-1), code=code, mean0=mean0, sd0=sd0)
    sw = S.Swapped(batch(0.8), batch(-0.7))
    det = _det()
    call = lambda out=None: det.kmer_mix(sw.t['sig'], sw.t['code'], ncodes, sw.t['mean0'], sw.t['sd0'], stride=n, max_iter=40, want_hist=True, out=out)
    sw.load_real()
    first = call()
    torch.cuda.synchronize()
    like = lambda: {k: torch.empty_like(v) for k, v in first.items()}
    want = {k: v.cpu().numpy() for k, v in call(S.fill_sentinel(like())).items()}
    sw.load_decoy()
    torch.cuda.synchronize()
    host = _engine().kmer_mix_host(sw.real['sig'].cpu().numpy(), None, sw.real['code'].cpu().numpy(), ncodes, sw.real['mean0'].cpu().numpy(),
                                   sw.real['sd0'].cpu().numpy(), stride=n, max_iter=40, want_hist=True)
    assert not [k for k in host if _bits(host[k]) != _bits(want[k])]            # the right result: the host entry's on the real batch
    out = like()
    for _ in range(2):                                                         # two streams: they take different hardware queues
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            warm = torch.empty(8 << 20, dtype=torch.uint8, device='cuda:0')
        del warm
        stream.synchronize()
        with torch.cuda.stream(stream):
            S.stall(stream, S.T_MS)
            event = torch.cuda.Event()
            event.record(stream)
            sw.load_real()
            got = call(S.fill_sentinel(out))
            sw.load_decoy()
            early = event.query()
        assert not early, 'the stall of %g ms had ended when the call returned' % S.T_MS
        stream.synchronize()
        bad = [k for k in want if _bits(got[k].cpu().numpy()) != _bits(want[k])]
        assert not bad, bad
        assert sw.holds('decoy')


# -------------------------------------------------------------------------------------- recovery through learn_alt_model
def _recovery():
    if 'recovery' not in _cache:
        from nanomod_amd import kmermodel
        control, sample, planted = R.recovery_groups()
        model = kmermodel.build_kmer_model(control, k=R.RECOVERY['k'], center=R.RECOVERY['center'], log=lambda *a: None)
        _cache['recovery'] = (control, sample, planted, model)
    return _cache['recovery']


def test_learn_alt_model_recovers_the_two_planted_kmers():
    from nanomod_amd import kmermodel
    cfg = R.RECOVERY
    control, sample, planted, model = _recovery()
    lines = []
    alt, table = kmermodel.learn_alt_model(sample, model, min_samples=1000, min_pi=0.05, min_shift=1.0, log=lines.append)
    assert np.array_equal(np.flatnonzero(table['kept']), planted)
    assert np.all(np.abs(table['pi'][planted] - cfg['share']) <= 0.05)
    assert np.all(np.abs(table['mu_mod'][planted] - (model['mean'][planted] + cfg['shift'])) <= 0.25 * model['sd'][planted])
    assert len(lines) == 1 and lines[0].startswith('kmer mix: k = 3, ') and '2 k-mer(s) kept' in lines[0]
    assert np.array_equal(np.isfinite(alt['mean']), table['kept']) and np.array_equal(alt['mean'][planted], table['mu_mod'][planted])
    # the device agrees with the restatement on this batch too
    res = R.restated_alt(sample, kmermodel.group_codes(sample, cfg['k'], cfg['center']), model['mean'], model['sd'])
    assert np.array_equal(res['n_used'], table['n_used']) and np.array_equal(res['iters'][planted], table['iters'][planted])
    assert np.all(np.abs(res['pi'][planted] - table['pi'][planted]) <= 1e-9) and np.all(np.abs(res['mu_mod'][planted] - table['mu_mod'][planted]) <= 1e-9)


# ------------------------------------------------------------------------------------------------------------- the chain
def test_the_learnt_table_goes_through_call_reads_llr():
    """a smoke check of the hand-off, not a statistic: the table learnt at the planted base's positions (--sites) is saved, loaded and
    taken by readllr.call_reads_llr; most reads drawn from the modified levels get a positive window sum at the planted base"""
    import readllr_ref as F
    from nanomod_amd import kmermodel, readllr
    reads, model, _, planted = F.chain_inputs()
    group = _engine().reads_to_group(reads, 0)
    sites = (np.array(['chrT'] * 6), np.array(['+'] * 3 + ['-'] * 3), np.array([planted - 2, planted - 1, planted, planted, planted + 1, planted + 2]))
    full = dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, n_samples=model['n_positions'] * 100, n_clipped=model['n_positions'] * 0, **model)
    alt, table = kmermodel.learn_alt_model(group, full, sites, min_coverage=5, min_samples=50, log=lambda *a: None)
    assert 1 <= table['kept'].sum() <= 6 and table['n_positions'].sum() == 6 and (table['n_used'][table['kept']] >= 50).all()
    with tempfile.TemporaryDirectory() as tmp:
        kmermodel.save_kmer_model(os.path.join(tmp, 'alt.npz'), alt)
        alt = kmermodel.load_kmer_model(os.path.join(tmp, 'alt.npz'))
    t, s, ev = readllr.call_reads_llr(reads, full, alt, events=True, log=lambda *a: None)
    assert t['n_sites'].sum() > 0
    n = np.diff(reads['off'])
    j = np.where(reads['strand'] == '-', reads['start'] + n - 1 - planted, planted - reads['start'])
    at = ev['llr_win'][reads['off'][:-1] + j]
    drawn = (np.arange(len(n)) // 2) % 2 == 0
    ok = np.isfinite(at)
    assert ok.mean() > 0.9 and (at[ok & drawn] > 0).mean() > 0.5 and (at[ok & ~drawn] > 0).mean() < 0.5


# ---------------------------------------------------------------------------------------------------------------- the CLI
def test_kmermix_command_line(capsys):
    from nanomod_amd import cli, container, kmermodel
    control, sample, planted, model = _recovery()
    with tempfile.TemporaryDirectory() as tmp:
        s_path, m_path, out = os.path.join(tmp, 'sample.npz'), os.path.join(tmp, 'control_kmer_model.npz'), os.path.join(tmp, 'res')
        container.save_group(s_path, *[sample[f] for f in ('chrom', 'strand', 'pos', 'base', 'off', 'sig')])
        kmermodel.save_kmer_model(m_path, model)
        argv = ['kmermix', '--wrkBase1', s_path, '--kmerModel', m_path, '--outFolder', out]
        assert cli.main(argv + ['--FileID', 'run']) == 0
        printed = capsys.readouterr().out
        assert 'kmer mix: k = 3' in printed and 'Modified k-mer model is saved in' in printed
        alt = kmermodel.load_kmer_model(os.path.join(out, 'run_alt_kmer_model.npz'))
        assert np.array_equal(np.flatnonzero(np.isfinite(alt['mean'])), planted)
        rows = [ln.split() for ln in open(os.path.join(out, 'run_kmer_mix.txt')).read().splitlines()]
        assert len(rows) == 64 and all(len(r) == 13 for r in rows) and [c for c, r in enumerate(rows) if r[12] == '1'] == planted.tolist()
        assert rows[0][0] == 'AAA' and rows[63][0] == 'TTT'
        # --sites: only the listed positions are pooled
        code = kmermodel.group_codes(sample, 3, 1)
        listed = np.flatnonzero(code == planted[0])[:7]
        s_file = os.path.join(tmp, 'sites.txt')
        with open(s_file, 'w') as f:
            f.write('# chrom strand pos\n')
            f.writelines('chr1 + %d A 0.5\n' % (sample['pos'][i] + 1) for i in listed)
            f.write('chr9 + 5\n')
        assert int(rows[planted[0]][1]) > 7
        assert cli.main(argv + ['--FileID', 'few', '--sites', s_file, '--minSamples', '100']) == 0
        few = [ln.split() for ln in open(os.path.join(out, 'few_kmer_mix.txt')).read().splitlines()]
        assert int(few[planted[0]][1]) == 7 and int(few[planted[0]][2]) == 7 * 60 and sum(int(r[1]) for r in few) == 7
        assert few[planted[0]][12] == '1' and ', 7 not among the sites' not in capsys.readouterr().out
        assert cli.main(argv + ['--maxIter', '0']) == 1 and capsys.readouterr().out.startswith('Error: --maxIter')
        assert cli.main(['kmermix', '--wrkBase1', s_path, '--kmerModel', os.path.join(tmp, 'none.npz')]) == 1
        assert capsys.readouterr().out.startswith('Error: input ')
