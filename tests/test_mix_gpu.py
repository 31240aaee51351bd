"""-m gpu: nmod_mix_fraction (K8) against tests/mix_ref.py, the numpy restatement of the definition, run for the device's own
iteration count per position.  Gates: pi and sd_mod 1e-9 relative (pi also 1e-12 absolute), mu_mod 1e-9 s, llr 1e-9 relative +
1e-9 absolute, resp 2^-23 absolute, status bits equal; 1e-9 is the project's p-value gate (tests/helpers.py) and
tests/test_mix.py pins the definition's conditioning on these inputs five orders below it.  The stopping rule is checked apart,
with a slack band of 1e-6 tol around the tolerance."""
import os
import tempfile

import numpy as np
import pytest

import helpers as H
import mix_ref as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


def _encode(rows, dtype):
    """int16 milli-unit rows in the dtype under test: the same 3-decimal values as int16, float64, or their float32 images"""
    if dtype == 'i16':
        return [np.asarray(r, np.int16) for r in rows]
    if dtype == 'f64':
        return [np.asarray(r, np.float64) / 1000.0 for r in rows]
    return [(np.asarray(r, np.float64) / 1000.0).astype(np.float32) for r in rows]


def _flat(rows, dtype):
    sig, off = M.csr(rows)
    return np.ascontiguousarray(sig), off


def _run(nm, ref_rows, mix_rows, *, mix_group=1, stride=False, **kw):
    """engine.mix_fraction_host on rows given per position; returns the result dict (with resp split per position)"""
    ref, roff = _flat(ref_rows, None)
    mix, moff = _flat(mix_rows, None)
    a, b = ((ref, roff), (mix, moff)) if mix_group == 1 else ((mix, moff), (ref, roff))
    if stride:
        s0, s1 = int(a[1][1] - a[1][0]), int(b[1][1] - b[1][0])
        assert (np.diff(a[1]) == s0).all() and (np.diff(b[1]) == s1).all()
        res = nm.engine.mix_fraction_host(a[0], None, b[0], None, stride0=s0, stride1=s1, mix_group=mix_group, want_resp=True, **kw)
    else:
        res = nm.engine.mix_fraction_host(a[0], a[1], b[0], b[1], mix_group=mix_group, want_resp=True, **kw)
    res['resp_rows'] = [res['resp'][moff[i]:moff[i + 1]] for i in range(len(mix_rows))]
    return res


def _check(res, ref_rows, mix_rows, model, max_iter, tol, what):
    exempt = 0
    for i, (x, y) in enumerate(zip(ref_rows, mix_rows)):
        tag = '%s position %d (%d v %d)' % (what, i, len(x), len(y))
        it, st, resp = int(res['iters'][i]), int(res['status'][i]), res['resp_rows'][i]
        if M.degenerate_by_input(M.as_double(x), M.as_double(y)):
            assert st == M.DEGENERATE and it == 0 and np.isnan(resp).all(), tag
            assert all(np.isnan(res[k][i]) for k in M.FIELDS), tag
            continue
        assert st & ~(M.NOT_CONVERGED | M.VAR_FLOORED) == 0 and 1 <= it <= max_iter, (tag, st, it)
        o = M.em(x, y, model, it)
        assert o['status'] & M.DEGENERATE == 0, tag
        got = {k: float(res[k][i]) for k in M.FIELDS}
        print('%s: iters %d status %d  err pi %.2e sd %.2e mu/s %.2e llr %.2e resp %.2e' % (
            tag, it, st, abs(got['pi'] - o['pi']), abs(got['sd_mod'] - o['sd_mod']), abs(got['mu_mod'] - o['mu_mod']) / o['s'],
            abs(got['llr'] - o['llr']), np.abs(resp - o['resp']).max()))
        assert abs(got['pi'] - o['pi']) <= 1e-9 * o['pi'] and abs(got['pi'] - o['pi']) <= 1e-12, (tag, got['pi'], o['pi'])
        assert abs(got['sd_mod'] - o['sd_mod']) <= 1e-9 * o['sd_mod'], (tag, got['sd_mod'], o['sd_mod'])
        assert abs(got['mu_mod'] - o['mu_mod']) <= 1e-9 * o['s'], (tag, got['mu_mod'], o['mu_mod'])
        if np.isnan(o['llr']):
            assert np.isnan(got['llr']), tag
        else:
            assert abs(got['llr'] - o['llr']) <= 1e-9 * abs(o['llr']) + 1e-9, (tag, got['llr'], o['llr'])
        assert resp.dtype == np.float32 and np.abs(resp.astype(np.float64) - o['resp']).max() <= 2.0 ** -23, tag
        assert bool(st & M.VAR_FLOORED) == bool(o['status'] & M.VAR_FLOORED), tag
        # the stopping rule, with slack: a delta within 1e-6 tol of tol may fall either way
        band = lambda dl: tol > 0.0 and abs(dl - tol) <= 1e-6 * tol
        if band(o['delta']) or (it > 1 and band(o['delta_prev'])):
            exempt += 1
            continue
        stops = tol > 0.0 and o['delta'] <= tol
        if st & M.NOT_CONVERGED:
            assert it == max_iter and not stops, (tag, o['delta'])
        else:
            assert stops, (tag, o['delta'])
        if it > 1:
            assert not (tol > 0.0 and o['delta_prev'] <= tol), (tag, o['delta_prev'])       # it had not stopped an iteration earlier
    assert exempt <= 0.01 * len(ref_rows), exempt


@pytest.mark.parametrize('max_iter', [50, 200])
@pytest.mark.parametrize('mix_group', [1, 0])
@pytest.mark.parametrize('model', [M.EQUAL, M.FREE])
@pytest.mark.parametrize('dtype', ['f32', 'i16', 'f64'])
def test_parity_ragged(nm, dtype, model, mix_group, max_iter):
    """ragged CSR rows, |Y| = 2 .. 3 000 over every size class and edge of the register-resident forms and the streaming form,
    planted fractions 0 .. 1; the null positions run into max_iter"""
    ref_rows, mix_rows = M.parity_inputs()
    x, y = _encode(ref_rows, dtype), _encode(mix_rows, dtype)
    res = _run(nm, x, y, mix_group=mix_group, model=model, max_iter=max_iter, tol=1e-6)
    _check(res, x, y, model, max_iter, 1e-6, '%s model %d group %d' % (dtype, model, mix_group))
    if max_iter == 50:
        assert (res['status'] & M.NOT_CONVERGED).any() and (res['status'] == 0).any()


@pytest.mark.parametrize('n', [200, 700, 1500])
@pytest.mark.parametrize('model', [M.EQUAL, M.FREE])
@pytest.mark.parametrize('dtype', ['f32', 'i16', 'f64'])
def test_parity_stride(nm, dtype, model, n):
    rng = np.random.default_rng(n)
    rows = [M.planted_rows(rng, n, n, f, 3.0) for f in (0.0, 0.2, 0.5, 0.7, 1.0, 0.05)]
    x, y = _encode([r[0] for r in rows], dtype), _encode([r[1] for r in rows], dtype)
    res = _run(nm, x, y, stride=True, model=model, max_iter=50, tol=1e-8)
    _check(res, x, y, model, 50, 1e-8, 'stride %s model %d n %d' % (dtype, model, n))


def _edge_rows(ny=60):
    """the edge positions with mixed groups of ny samples (position 1: of one)"""
    rng = np.random.default_rng(11)
    ok_x, ok_y, _ = M.planted_rows(rng, 50, ny, 0.5, 4.0)
    x, y = [], []
    x.append(ok_x[:1]); y.append(ok_y)                                                   # 0: a reference group of 1
    x.append(ok_x); y.append(ok_y[:1])                                                   # 1: a mixed group of 1
    x.append(np.full(13, 700, np.int16)); y.append(ok_y)                                 # 2: a constant reference group
    x.append(np.array([1000, 3000], np.int16)); y.append(np.full(ny, 2000, np.int16))    # 3: all of Y equal to mu
    x.append(np.arange(-1000, 1001, 40, dtype=np.int16)); y.append(np.r_[np.full(ny // 2, 400), np.full(ny // 2, 401)].astype(np.int16))   # 4: floor
    x.append(ok_x); y.append(ok_y)                                                       # 5: an ordinary position
    return x, y


@pytest.mark.parametrize('ny', [60, 600, 1100])
@pytest.mark.parametrize('model', [M.EQUAL, M.FREE])
def test_degenerate_and_edge_statuses(nm, model, ny):
    """|Y| = 60, 600 and 1 100: the 16-lane, the whole-wave and the streaming form, which run one EM through their own row policies"""
    assert 60 <= M.SMALL < 600 <= M.WAVE < 1100
    x, y = _edge_rows(ny)
    xd, yd = _encode(x, 'f64'), _encode(y, 'f64')
    res = _run(nm, xd, yd, model=model)
    _check(res, xd, yd, model, 200, 1e-6, 'edge model %d |Y| %d' % (model, ny))
    assert list(res['status'][:3]) == [M.DEGENERATE] * 3 and list(res['iters'][:3]) == [0, 0, 0]
    # all of Y equal to mu: d = 0, every t_i = 0, r_i = 1/2, the parameters reproduce themselves: converged after one iteration.
    # In the free model v' = 0 < s2 / 16: the floor is active, sd moves from s to s / 4, and the next iterations settle
    if model == M.EQUAL:
        assert (res['pi'][3], res['mu_mod'][3], res['iters'][3], res['status'][3]) == (0.5, 2.0, 1, 0) and abs(res['llr'][3]) <= 1e-12
    else:
        assert res['mu_mod'][3] == 2.0 and res['status'][3] & M.VAR_FLOORED and res['sd_mod'][3] == 0.25
    if model == M.FREE:
        assert res['status'][4] & M.VAR_FLOORED and abs(res['sd_mod'][4] - np.sqrt(np.var(xd[4]) / 16.0)) <= 1e-14
    else:
        assert res['status'][4] & M.VAR_FLOORED == 0
    # a NaN sample in either group (float32 and float64 carry one; int16 cannot)
    for dt in (np.float32, np.float64):
        for where in (0, 1):
            xs, ys = [r.astype(dt) for r in xd], [r.astype(dt) for r in yd]
            (xs if where == 0 else ys)[5][7] = np.nan
            r2 = _run(nm, xs, ys, model=model)
            assert r2['status'][5] == M.DEGENERATE and r2['iters'][5] == 0 and np.isnan(r2['pi'][5]) and np.isnan(r2['resp_rows'][5]).all()
            (xs if where == 0 else ys)[5][7] = np.inf
            assert _run(nm, xs, ys, model=model)['status'][5] == M.DEGENERATE
    # tol = 0 runs exactly max_iter
    r3 = _run(nm, xd, yd, model=model, tol=0.0, max_iter=37)
    live = r3['status'] & M.DEGENERATE == 0
    assert (r3['iters'][live] == 37).all() and (r3['status'][live] & M.NOT_CONVERGED).all()
    _check(r3, xd, yd, model, 37, 0.0, 'tol 0 model %d |Y| %d' % (model, ny))
    r4 = _run(nm, xd, yd, model=model, max_iter=1)
    assert (r4['iters'][live] == 1).all()


def _same_bits(a, b, keys=M.FIELDS + ('iters', 'status')):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def _property_rows():
    rng = np.random.default_rng(5)
    sizes = [3, 16, 17, 200, 256, 257, 600, 1024, 1025, 2000] * 3
    rows = [M.planted_rows(rng, int(rng.integers(5, 400)), n, rng.random(), 3.5) for n in sizes]
    return [r[0] for r in rows], [r[1] for r in rows]


@pytest.mark.parametrize('model', [M.EQUAL, M.FREE])
def test_properties_bit_for_bit(nm, model):
    x, y = _property_rows()
    kw = dict(model=model, max_iter=60, tol=1e-7)
    base = _run(nm, x, y, **kw)
    assert _same_bits(base, _run(nm, x, y, **kw)) and base['resp'].tobytes() == _run(nm, x, y, **kw)['resp'].tobytes()   # two runs
    # permuting the positions permutes the outputs
    perm = np.random.default_rng(1).permutation(len(x))
    pr = _run(nm, [x[i] for i in perm], [y[i] for i in perm], **kw)
    assert _same_bits({k: base[k][perm] for k in base if k not in ('resp', 'resp_rows')}, pr)
    assert all(base['resp_rows'][j].tobytes() == pr['resp_rows'][i].tobytes() for i, j in enumerate(perm))
    # a batch of one position == the same position inside the batch, for each form
    for i in (3, 6, 9, 0, 4, 8):
        one = _run(nm, [x[i]], [y[i]], **kw)
        assert _same_bits({k: base[k][i:i + 1] for k in M.FIELDS + ('iters', 'status')}, one), i
        assert one['resp'].tobytes() == base['resp_rows'][i].tobytes(), i
    # gated == ungated on the computed positions, SKIPPED / NaN elsewhere
    gate = np.random.default_rng(2).random(len(x))
    gate[4] = np.nan
    g = _run(nm, x, y, gate=gate, gate_max=0.5, **kw)
    on = gate <= 0.5
    assert 5 < on.sum() < len(x) - 5 and not on[4]
    assert _same_bits({k: base[k][on] for k in M.FIELDS + ('iters', 'status')}, {k: g[k][on] for k in M.FIELDS + ('iters', 'status')})
    assert (g['status'][~on] == M.SKIPPED).all() and (g['iters'][~on] == 0).all() and all(np.isnan(g[k][~on]).all() for k in M.FIELDS)
    for i in range(len(x)):
        assert g['resp_rows'][i].tobytes() == base['resp_rows'][i].tobytes() if on[i] else np.isnan(g['resp_rows'][i]).all(), i


@pytest.mark.parametrize('n', [200, 700, 1500])
def test_csr_equals_stride_bit_for_bit(nm, n):
    rng = np.random.default_rng(n + 1)
    rows = [M.planted_rows(rng, n, n, f, 3.0) for f in (0.0, 0.3, 0.6, 0.9) * 5]
    x, y = [r[0] for r in rows], [r[1] for r in rows]
    for model in (M.EQUAL, M.FREE):
        a, b = _run(nm, x, y, model=model, max_iter=40), _run(nm, x, y, model=model, max_iter=40, stride=True)
        assert _same_bits(a, b) and a['resp'].tobytes() == b['resp'].tobytes()


def test_device_entry_composes_with_detect_and_fdr(nm):
    """DeviceDetector.run -> .fdr -> .mix(gate=q) on one stream, nothing synchronised or read in between.  Event-like int16 rows,
    200 v 200, spread 0.2; group 2 of the planted positions (0, 1, 99 mod 100) is shifted by 0.8 = 4 sigma as a whole, so the
    planted fraction is 1: the rejected positions come out with pi near 1 and mu_mod near the level + 0.8."""
    import torch
    npos, n, seed, begin = 20000, 200, 20240601, 50
    det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer')
    sig0 = torch.empty(npos * n, dtype=torch.int16, device='cuda:0'); sig1 = torch.empty_like(sig0)
    det.synth_fill_events(sig0, seed, begin, npos, 0, n_per_pos=n, plant_period=100, plant_shift_milli=800, spread_milli=200)
    det.synth_fill_events(sig1, seed, begin, npos, 1, n_per_pos=n, plant_period=100, plant_shift_milli=800, spread_milli=200)
    rid = torch.zeros(npos, dtype=torch.int32, device='cuda:0')
    def chain():
        res = det.run(sig0, sig1, rid, stride0=n, stride1=n, npos=npos)
        (q,), summ = det.fdr(res, tracks=('comb_p',), method='bh', alpha=0.05)
        return q, det.mix(sig0, sig1, stride0=n, stride1=n, npos=npos, gate=q, gate_max=0.05, want_resp=True)
    planted = np.isin((np.arange(npos) + begin) % 100, (0, 1, 99))

    def whole():
        q, mix = chain()
        torch.cuda.synchronize()
        qh, st = q.cpu().numpy(), mix['status'].cpu().numpy()
        on = qh <= 0.05
        assert on[planted].all() and np.array_equal((st & M.SKIPPED) != 0, ~on)
        pi, mu = mix['pi'].cpu().numpy(), mix['mu_mod'].cpu().numpy()
        assert (st[planted] & (M.DEGENERATE | M.SKIPPED) == 0).all()
        assert np.median(pi[planted]) > 0.97 and (pi[planted] > 0.9).all()
        level = sig0.view(npos, n).double().mean(1).cpu().numpy() / 1000.0
        assert np.abs(mu[planted] - level[planted] - 0.8).max() < 0.1
        resp = mix['resp'].view(npos, n).cpu().numpy()
        assert np.isnan(resp[~on]).all() and np.median(resp[planted]) > 0.95
        # the host entry on the same rows and gate gives the same bits
        host = nm.engine.mix_fraction_host(sig0.cpu().numpy(), None, sig1.cpu().numpy(), None, stride0=n, stride1=n, gate=qh, gate_max=0.05)
        assert all(host[k].tobytes() == mix[k].cpu().numpy().tobytes() for k in M.FIELDS + ('iters', 'status'))

    def settle():
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        assert nm._lib.load().nmod_trim_scratch(0) == 0
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]
    # a first pass loads every code object and whatever the runtime sets up on first use (device memory of their own), the
    # second is measured: the call holds 12 bytes per position of pool scratch, and the pool gives it back
    whole()
    free0 = settle()
    whole()
    assert free0 - settle() <= (2 << 20)


def _mix_lines(rows, mix):
    keep = [i for i in range(len(rows)) if not mix['status'][i] & M.SKIPPED]
    return ''.join('%s %s %d %s' % rows[i] + ' %.6f %.6f %.6f %.3f %d %d\n' % (
        mix['pi'][i], mix['mu_mod'][i], mix['sd_mod'][i], mix['llr'][i], mix['iters'][i], mix['status'][i]) for i in keep)


@pytest.mark.parametrize('fdr', ['', 'bh'])
@pytest.mark.parametrize('model,group', [('equal', 2), ('free', 1)])
def test_through_mtest2(nm, model, group, fdr):
    name, method = 'g50_stouffer', 'stouffer'
    fx = H.load_inputs('g50')
    exp, table = H.load_expected(name)
    with tempfile.TemporaryDirectory() as out:
        mo = H.build_moptions(fx, out, name, 2, 2.0, method)
        mo.update(nmod_mix=model, nmod_mix_group=group, nmod_mix_max_iter=80, nmod_mix_tol=1e-7)
        if fdr:
            mo['nmod_fdr'] = fdr
        nm.mfilter_coverage(mo)
        nm.mtest2(mo)
        assert open(os.path.join(out, name + '_sign_test.txt')).read() == table            # byte-identical to a run without
        got = open(os.path.join(out, name + '_sign_test_mix.txt')).read()
    mix = mo['sign_test_mix']
    rows = [tuple(ln.split(' ')[:4]) for ln in table.splitlines()]
    rows = [(c, s, int(p), b) for c, s, p, b in rows]
    assert got == _mix_lines(rows, mix)
    npos = len(rows)
    assert all(len(mix[k]) == npos for k in M.FIELDS + ('iters', 'status'))
    if fdr:
        on = mo['sign_test_fdr']['comb_q'] <= 0.05
        assert np.array_equal((mix['status'] & M.SKIPPED) != 0, ~on) and len(got.splitlines()) == on.sum()
    else:
        assert not (mix['status'] & M.SKIPPED).any() and len(got.splitlines()) == npos
    # the numbers are the definition's on the tested rows
    meta, sig0, off0, sig1, off1, rid = nm.detect.build_csr(mo)
    rows0 = [sig0[off0[i]:off0[i + 1]] for i in range(npos)]; rows1 = [sig1[off1[i]:off1[i + 1]] for i in range(npos)]
    xr, yr = (rows0, rows1) if group == 2 else (rows1, rows0)
    mid = M.MODEL_BY_NAME[model]
    for i in np.flatnonzero((mix['status'] & (M.SKIPPED | M.DEGENERATE)) == 0)[:40]:
        o = M.em(xr[i], yr[i], mid, int(mix['iters'][i]))
        assert abs(mix['pi'][i] - o['pi']) <= 1e-9 * o['pi'] and abs(mix['mu_mod'][i] - o['mu_mod']) <= 1e-9 * o['s'], i
    # without the option: no such file, none of the new keys
    with tempfile.TemporaryDirectory() as out:
        mo = H.build_moptions(fx, out, name, 2, 2.0, method)
        nm.mfilter_coverage(mo)
        nm.mtest2(mo)
        assert sorted(os.listdir(out)) == [name + '_sign_test.txt']
        assert not {k for k in mo if 'mix' in k}


def test_cli_detect_with_mix(nm, capsys):
    from nanomod_amd import cli
    from test_abi_and_host import _fixture_containers
    exp, table = H.load_expected('g50_stouffer')
    base = ['--testMethod', 'stouffer', '--topN', '5', '--FileID', 'x', '--outLevel', '1']
    with tempfile.TemporaryDirectory() as tmp:
        p0, p1 = _fixture_containers('g50', tmp)
        out_a, out_b, out_c = (os.path.join(tmp, d) for d in 'abc')
        assert cli.main(['detect', '--wrkBase1', p0, '--wrkBase2', p1, '--outFolder', out_a] + base) == 0
        plain = capsys.readouterr().out
        assert os.listdir(out_a) == ['x_sign_test.txt'] and 'MIX' not in plain
        assert cli.main(['detect', '--wrkBase1', p0, '--wrkBase2', p1, '--outFolder', out_b, '--mixFraction', 'free', '--mixGroup', '1',
                         '--mixMaxIter', '60', '--mixTol', '1e-7'] + base) == 0
        with_mix = capsys.readouterr().out
        assert sorted(os.listdir(out_b)) == ['x_sign_test.txt', 'x_sign_test_mix.txt']
        assert open(os.path.join(out_b, 'x_sign_test.txt')).read() == table == open(os.path.join(out_a, 'x_sign_test.txt')).read()
        got = open(os.path.join(out_b, 'x_sign_test_mix.txt')).read()
        assert cli.main(['detect', '--wrkBase1', p0, '--wrkBase2', p1, '--outFolder', out_c, '--mixFraction', 'equal', '--fdr', 'bh'] + base) == 0
        capsys.readouterr()
        gated = open(os.path.join(out_c, 'x_sign_test_mix.txt')).read()
        fdr_lines = open(os.path.join(out_c, 'x_sign_test_fdr.txt')).read().splitlines()
    lines, tl = got.splitlines(), table.splitlines()
    assert len(lines) == len(tl) and all(a.split(' ')[:4] == b.split(' ')[:4] and len(a.split(' ')) == 10 for a, b in zip(lines, tl))
    assert all(int(a.split(' ')[8]) <= 60 for a in lines)
    mix_lines = [ln for ln in with_mix.splitlines() if ln.startswith('MIX free group 1')]
    assert len(mix_lines) == 1 and 'computed %d of %d' % (len(tl), len(tl)) in mix_lines[0]
    same = lambda text, d: [ln.replace(d, 'OUT') for ln in text.splitlines() if not ln.startswith(('MIX ', 'Producing pvalues'))]
    assert same(with_mix, out_b) == same(plain, out_a)
    # with --fdr the table holds the positions whose combined q is at most 0.05 (the printed q has four digits: leave a margin)
    qs = np.array([float(ln.split(' ')[7]) for ln in fdr_lines])
    heads = [' '.join(ln.split(' ')[:4]) for ln in fdr_lines]
    got_heads = [' '.join(ln.split(' ')[:4]) for ln in gated.splitlines()]
    assert [h for h, q in zip(heads, qs) if q <= 0.0499] == [h for h in got_heads if qs[heads.index(h)] <= 0.0499]
    assert all(qs[heads.index(h)] <= 0.0501 for h in got_heads)


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_streaming_form_beyond_65535_samples(nm, dtype):
    """a mixed group of 70 000 samples (the size of test_deep_coverage_gpu.py's smallest case) against the oracle, both models"""
    rng = np.random.default_rng(70000)
    rows = [M.planted_rows(rng, 300, 70000, 0.25, 3.0), M.planted_rows(rng, 66000, 300, 0.5, 3.0)]
    x, y = _encode([r[0] for r in rows], dtype), _encode([r[1] for r in rows], dtype)
    for model in (M.EQUAL, M.FREE):
        res = _run(nm, x, y, model=model, max_iter=50, tol=1e-7)
        _check(res, x, y, model, 50, 1e-7, 'deep %s model %d' % (dtype, model))
        assert abs(res['pi'][0] - 0.25) < 0.05 and abs(res['pi'][1] - 0.5) < 0.1
