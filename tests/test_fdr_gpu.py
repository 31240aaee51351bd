"""-m gpu: nmod_fdr_adjust (K7) against scipy.stats.false_discovery_control on the valid elements.
BH: equal bit for bit (one division, one product, exact minima, in scipy's order).  BY: 1e-14 relative (c_m is summed
differently: any tree sum of m < 2^31 positive terms is within 32 * 2^-53 of the exact one, on both sides, plus one rounding of
the product).  tested / excluded exact; rejected / p_crit exact (BY: at a level no reference q is within 1e-12 of)."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import fdr_ref as F
import helpers as H

pytestmark = pytest.mark.gpu

TILE = 2048                  # fdr.hip: kFdrTile (= radix_sort.hpp: kRsTile), sorted elements per block
HIST_CHUNK = 4096 // 256 * TILE     # radix_sort.hpp: kRsScanChunk histogram entries = 16 tiles of elements per scan block
SUFFIX_CHUNK = 256 * TILE    # fdr_tile_suffix_kernel: tiles per round of its one block
DIRECT_SUM = 64              # fdr.hip: kFdrDirectSum, where c_m changes from the direct sum to the series
TINY = np.finfo(np.float64).tiny


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


def _check_track(nm, p, method, what, alpha=None):
    ref = F.fdr_scipy(p, method)
    if alpha is None:
        alpha = F.pick_alpha(ref) if method == 'by' else 0.05
    qs, summ = nm.engine.fdr_adjust_host(p, method=method, alpha=alpha)
    F.check_q(qs[0], ref, method, what)
    # (BY: the count is taken on the reference q; pick_alpha has made sure that none of them is near the level)
    F.same_summary(summ[0], F.summary_ref(p, ref, alpha))
    return qs[0], summ[0]


SIZES = [0, 1, 2, 63, 64, 65, DIRECT_SUM - 1, TILE - 1, TILE, TILE + 1, HIST_CHUNK - 1, HIST_CHUNK, HIST_CHUNK + 1,
         SUFFIX_CHUNK - 1, SUFFIX_CHUNK, SUFFIX_CHUNK + 1, 200000, 4600000]


@pytest.mark.parametrize('method', ['bh', 'by'])
@pytest.mark.parametrize('n', SIZES)
def test_sizes(nm, n, method):
    rng = np.random.default_rng(n + 17)
    p = rng.random(n)
    if n > 10:
        p[rng.choice(n, max(n // 100, 1), replace=False)] *= 1e-9
    q, s = _check_track(nm, p, method, 'n=%d' % n)
    assert s['tested'] == n and s['excluded'] == 0
    if n == 1:
        assert q[0] == p[0]


def _shapes(n):
    rng = np.random.default_rng(5)
    u = rng.random(n)
    planted = u.copy(); planted[rng.choice(n, n // 100, replace=False)] = rng.random(n // 100) * 1e-9
    runs = u.copy()
    runs[:3 * TILE + 5] = TINY; runs[5 * TILE - 7:7 * TILE + 3] = 0.0; runs[9 * TILE:10 * TILE + 1] = -0.0
    return {'uniform': u, 'planted': planted, 'two_decimals': np.round(u, 2), 'all_equal': np.full(n, 0.03125),
            'all_equal_small': np.full(n, 1e-12), 'all_one': np.ones(n), 'tiny_and_zero_runs': runs,
            'ascending': np.sort(planted), 'descending': np.sort(planted)[::-1].copy()}


@pytest.mark.parametrize('method', ['bh', 'by'])
@pytest.mark.parametrize('shape', ['uniform', 'planted', 'two_decimals', 'all_equal', 'all_equal_small', 'all_one', 'tiny_and_zero_runs',
                                   'ascending', 'descending'])
def test_shapes_of_data(nm, shape, method):
    p = _shapes(30 * TILE + 77)[shape]
    q, _ = _check_track(nm, p, method, shape)
    if shape.startswith('all_'):
        assert np.unique(q).size == 1


@pytest.mark.parametrize('method', ['bh', 'by'])
def test_invalid_elements(nm, method):
    n = 12 * TILE + 9
    rng = np.random.default_rng(11)
    base = np.round(rng.random(n), 3)
    base[rng.choice(n, 200, replace=False)] *= 1e-10
    bads = [np.nan, -1e-3, 1.0 + 2.0 ** -52, np.inf, -np.inf, -np.nan]
    # scattered
    p = base.copy()
    where = rng.choice(n, 600, replace=False)
    p[where] = np.array(bads)[np.arange(600) % len(bads)]
    q, s = _check_track(nm, p, method, 'scattered')
    assert np.isnan(q[where]).all() and np.isnan(q).sum() == 600 and s['excluded'] == 600
    # a whole tile of them (in input order), and more than a tile so that a whole SORTED tile is invalid too
    for lo, hi in ((4 * TILE, 5 * TILE), (TILE - 3, 4 * TILE + 5)):
        p = base.copy()
        p[lo:hi] = np.array(bads)[np.arange(hi - lo) % len(bads)]
        q, s = _check_track(nm, p, method, 'tile %d:%d' % (lo, hi))
        assert np.isnan(q[lo:hi]).all() and s['excluded'] == hi - lo
    # one valid element among invalid ones: q = p; none at all: all NaN, nothing tested
    p = np.full(n, np.nan); p[n // 2] = 0.25
    q, s = _check_track(nm, p, method, 'one valid')
    assert q[n // 2] == 0.25 and s['tested'] == 1
    for fill in (np.nan, 2.0):
        p = np.full(n, fill)
        q, s = _check_track(nm, p, method, 'none valid')
        assert np.isnan(q).all() and (s['tested'], s['excluded'], s['rejected']) == (0, n, 0) and np.isnan(s['p_crit'])


def _device_call(nm, ps, method, alpha, in_place=False):
    import torch
    det = nm.DeviceDetector(0)
    res = {'t%d' % i: torch.from_numpy(p).to('cuda:0') for i, p in enumerate(ps)}
    names = tuple(res)
    qs, summ = det.fdr(res, tracks=names, method=method, alpha=alpha, out=res if in_place else None)
    out = [q.cpu().numpy() for q in qs]
    if in_place:
        assert all(q.data_ptr() == res[k].data_ptr() for q, k in zip(qs, names))
    else:
        assert all(np.array_equal(res[k].cpu().numpy(), p, equal_nan=True) for k, p in zip(names, ps))     # the input is left alone
    return out, nm.engine.fdr_summary_dicts(summ)


@pytest.mark.parametrize('method', ['bh', 'by'])
@pytest.mark.parametrize('ntracks', [4, 8])
def test_several_tracks_in_place_and_both_entries_are_bit_equal(nm, ntracks, method):
    rng = np.random.default_rng(ntracks)
    n = 40 * TILE + 123
    ps = []
    for t in range(ntracks):
        p = rng.random(n) ** (1 + t)
        if t % 2:
            p = np.round(p, 2)
        p[rng.choice(n, 10 * t, replace=False)] = np.nan                      # a different m per track
        ps.append(p)
    alpha = 0.05
    q_all, s_all = nm.engine.fdr_adjust_host(ps, method=method, alpha=alpha)
    for t in range(ntracks):
        q1, s1 = nm.engine.fdr_adjust_host(ps[t], method=method, alpha=alpha)
        assert np.array_equal(q_all[t], q1[0], equal_nan=True)
        F.same_summary(s_all[t], s1[0])
        F.check_q(q_all[t], F.fdr_scipy(ps[t], method), method, 'track %d' % t)
    q_dev, s_dev = _device_call(nm, ps, method, alpha)
    q_inp, s_inp = _device_call(nm, ps, method, alpha, in_place=True)
    for t in range(ntracks):
        assert np.array_equal(q_dev[t], q_all[t], equal_nan=True) and np.array_equal(q_inp[t], q_all[t], equal_nan=True)
        F.same_summary(s_dev[t], s_all[t]); F.same_summary(s_inp[t], s_all[t])
    # in place through the host entry (q_out[t] == p[t])
    L = nm._lib
    work = [p.copy() for p in ps]
    arr = (C.c_void_p * ntracks)(*[w.ctypes.data for w in work])
    prm = L.make_params(device=0, memspace=L.MEM_HOST)
    assert L.load().nmod_fdr_adjust(C.byref(prm), n, ntracks, arr, L.FDR_BY_NAME[method], alpha, arr, None) == 0
    assert all(np.array_equal(w, q, equal_nan=True) for w, q in zip(work, q_all))


def test_device_entry_of_an_empty_track(nm):
    qs, summ = _device_call(nm, [np.zeros(0)], 'bh', 0.05)
    s = summ[0]
    assert qs[0].size == 0 and (s['tested'], s['excluded'], s['rejected']) == (0, 0, 0) and np.isnan(s['p_crit'])


@pytest.mark.parametrize('method', ['bh', 'by'])
def test_device_entry_composes_with_a_detect_step(nm, method):
    """DeviceDetector.run -> .fdr on one stream.  The planted sites (positions = 0, 1, 99 mod 100: 600 of 20 000) lie inside
    the run (the rows start at position 50: the combined track is 1.0 by construction on a run's first and last nb positions).
    That all of them are rejected is a statement about the tests' power, so it is asserted on scipy's q first: the levels here
    are p <= 1.5e-3 (BH) and 1.4e-4 (BY, c_m = 10.5), and the KS test at 200 v 200 samples and a 0.8 sigma shift reaches
    p = 5.4e-4 at one site in 600 under seed 77 (scipy's BY q: 0.185); the seed kept is that of the existing device-path test,
    under which scipy rejects all 600 on every track with both methods (largest planted KS p 3.9e-5)."""
    import torch
    npos, n, seed, begin = 20000, 200, 20240601, 50
    det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer')
    sig0 = torch.empty(npos * n, dtype=torch.float32, device='cuda:0')
    sig1 = torch.empty(npos * n, dtype=torch.float32, device='cuda:0')
    det.synth_fill(sig0, seed, begin, npos, 0, n, plant_period=100, plant_shift=0.8)
    det.synth_fill(sig1, seed, begin, npos, 1, n, plant_period=100, plant_shift=0.8)
    rid = torch.zeros(npos, dtype=torch.int32, device='cuda:0')
    res = det.run(sig0, sig1, rid, stride0=n, stride1=n, npos=npos)
    tracks = ('mwu_p', 't_p', 'ks_p', 'comb_p')
    alpha = 0.05
    qs, summ = det.fdr(res, tracks=tracks, method=method, alpha=alpha)          # same stream, nothing synchronised in between
    torch.cuda.synchronize()
    summ = nm.engine.fdr_summary_dicts(summ)
    planted = np.isin((np.arange(npos) + begin) % 100, (0, 1, 99))
    for name, q, s in zip(tracks, qs, summ):
        p = res[name].cpu().numpy()
        ref = F.fdr_scipy(p, method)
        F.check_q(q.cpu().numpy(), ref, method, name)
        level = F.pick_alpha(ref) if method == 'by' else alpha
        if level != alpha:                                  # a reference q sits on the level: count at another one
            s = nm.engine.fdr_summary_dicts(det.fdr(res, tracks=(name,), method=method, alpha=level)[1])[0]
        F.same_summary(s, F.summary_ref(p, ref, level))
        assert (ref[planted] <= alpha).all(), name                             # (the reference alone)
        assert (q.cpu().numpy()[planted] <= alpha).all(), name                 # the planted sites are among the rejected
        assert int((q.cpu().numpy() <= alpha).sum()) >= planted.sum() and s['tested'] == npos
    with pytest.raises(KeyError):
        nm.DeviceDetector(0, method='ks').fdr({k: v for k, v in res.items() if not k.startswith('comb')}, tracks=('comb_p',))


def _fdr_lines(meta_rows, qcols):
    return ''.join('%s %s %d %s' % row + ''.join(' %.3E' % q[i] for q in qcols) + '\n' for i, row in enumerate(meta_rows))


@pytest.mark.parametrize('inp,name,method', [('g50', 'g50_stouffer', 'stouffer'), ('g50', 'g50_ks', 'ks')])
def test_through_mtest2(nm, inp, name, method):
    fx = H.load_inputs(inp)
    exp, table = H.load_expected(name)
    with tempfile.TemporaryDirectory() as out:
        mo = H.build_moptions(fx, out, name, 2, 2.0, method)
        mo['nmod_fdr'] = 'bh'
        nm.mfilter_coverage(mo)
        nm.mtest2(mo)
        assert open(os.path.join(out, name + '_sign_test.txt')).read() == table
        got = open(os.path.join(out, name + '_sign_test_fdr.txt')).read()
    res = mo['sign_test_arrays']
    tracks = ['mwu_p', 't_p', 'ks_p'] + (['comb_p'] if method != 'ks' else [])
    assert list(mo['sign_test_fdr']) == [t[:-1] + 'q' for t in tracks] and list(mo['nmod_fdr_summary']) == tracks
    qcols = []
    for t in tracks:
        ref = F.fdr_scipy(res[t], 'bh')
        F.check_q(mo['sign_test_fdr'][t[:-1] + 'q'], ref, 'bh', t)
        F.same_summary(mo['nmod_fdr_summary'][t], F.summary_ref(res[t], ref, 0.05))
        assert mo['nmod_fdr_summary'][t]['excluded'] == int(np.isnan(res[t]).sum())
        qcols.append(ref)
    rows = [tuple(ln.split(' ')[:4]) for ln in table.splitlines()]
    rows = [(c, s, int(p), b) for c, s, p, b in rows]
    assert got == _fdr_lines(rows, qcols)
    assert got.count('NAN') == sum(int(np.isnan(q).sum()) for q in qcols)
    # without the option: no such file, none of the new keys
    with tempfile.TemporaryDirectory() as out:
        mo = H.build_moptions(fx, out, name, 2, 2.0, method)
        nm.mfilter_coverage(mo)
        nm.mtest2(mo)
        assert os.path.exists(os.path.join(out, name + '_sign_test.txt')) and not os.path.exists(os.path.join(out, name + '_sign_test_fdr.txt'))
        assert not {'sign_test_fdr', 'nmod_fdr_summary', 'nmod_fdr', 'nmod_fdr_alpha'} & set(mo)


def test_cli_detect_with_fdr(nm, capsys):
    from nanomod_amd import cli
    from test_abi_and_host import _fixture_containers
    exp, table = H.load_expected('g50_stouffer')
    base = ['--testMethod', 'stouffer', '--topN', '5', '--FileID', 'x']
    with tempfile.TemporaryDirectory() as tmp:
        p0, p1 = _fixture_containers('g50', tmp)
        out_a, out_b = os.path.join(tmp, 'a'), os.path.join(tmp, 'b')
        # without the flags: the folder and the printed lines of today
        assert cli.main(['detect', '--wrkBase1', p0, '--wrkBase2', p1, '--outFolder', out_a, '--outLevel', '1'] + base) == 0
        plain = capsys.readouterr().out
        assert os.listdir(out_a) == ['x_sign_test.txt'] and 'FDR' not in plain
        assert cli.main(['detect', '--wrkBase1', p0, '--wrkBase2', p1, '--outFolder', out_b, '--outLevel', '1',
                         '--fdr', 'by', '--fdrAlpha', '0.01'] + base) == 0
        with_fdr = capsys.readouterr().out
        assert sorted(os.listdir(out_b)) == ['x_sign_test.txt', 'x_sign_test_fdr.txt']
        assert open(os.path.join(out_b, 'x_sign_test.txt')).read() == table == open(os.path.join(out_a, 'x_sign_test.txt')).read()
        got = open(os.path.join(out_b, 'x_sign_test_fdr.txt')).read()
        # the same run through run_detect, for the p-value tracks behind the table
        a = cli.build_parser().parse_args(['detect', '--wrkBase1', p0, '--wrkBase2', p1, '--outFolder', os.path.join(tmp, 'c'),
                                           '--outLevel', '3', '--fdr', 'by', '--fdrAlpha', '0.01'] + base)
        assert not cli.validate(a)
        meta, res, order = cli.run_detect(a, log=lambda *x: None)
        capsys.readouterr()
    tracks = ('mwu_p', 't_p', 'ks_p', 'comb_p')
    refs = [F.fdr_scipy(res[t], 'by') for t in tracks]
    lines = got.splitlines()
    assert len(lines) == len(table.splitlines())
    for i, (ln, tl) in enumerate(zip(lines, table.splitlines())):
        f = ln.split(' ')
        assert f[:4] == tl.split(' ')[:4] and len(f) == 8
        for k in range(4):
            if np.isnan(refs[k][i]):
                assert f[4 + k] == 'NAN'
            else:                                     # four printed digits of a q known to 1e-14: a last-digit tie may round either way
                assert abs(float(f[4 + k]) - refs[k][i]) <= 5.01e-4 * refs[k][i]
    fdr_lines = [ln for ln in with_fdr.splitlines() if ln.startswith('FDR by')]
    assert len(fdr_lines) == 4 and all('alpha=0.01' in ln and 'tested' in ln and 'p_crit' in ln for ln in fdr_lines)
    same = lambda text, d: [ln.replace(d, 'OUT') for ln in text.splitlines() if not ln.startswith(('FDR by', 'Producing pvalues'))]
    assert same(with_fdr, out_b) == same(plain, out_a)
    for ln, t, ref in zip(fdr_lines, tracks, refs):
        s = F.summary_ref(res[t], ref, 0.01)
        assert ' %s ' % t in ln and 'tested %d excluded %d ' % (s['tested'], s['excluded']) in ln


def test_scratch_goes_back(nm):
    import torch
    L = nm._lib
    lib = L.load()
    n = 4600000
    p = torch.rand(n, dtype=torch.float64, device='cuda:0')
    det = nm.DeviceDetector(0)
    q = torch.empty_like(p)
    # a first small call: the code objects of the library's and torch's kernels are device memory too, loaded on first use
    _, warm = det.fdr({'p': p[:5000].clone()}, tracks=('p',), method='by')
    assert nm.engine.fdr_summary_dicts(warm)[0]['tested'] == 5000 and float(p.max().cpu()) <= 1.0
    del warm
    torch.cuda.synchronize()
    assert lib.nmod_trim_scratch(0) == 0
    free0 = torch.cuda.mem_get_info(0)[0]
    qs, summ = det.fdr({'p': p}, tracks=('p',), method='by', out={'p': q})
    assert nm.engine.fdr_summary_dicts(summ)[0]['tested'] == n          # (the caller reads its results: the call itself did not wait)
    assert float(q.max().cpu()) <= 1.0
    torch.cuda.synchronize()
    held = free0 - torch.cuda.mem_get_info(0)[0]
    assert held <= 26 * n + (64 << 20)                  # about 24 B per element + histogram, cached by the library's pool
    assert lib.nmod_trim_scratch(0) == 0
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info(0)[0] <= (2 << 20)
