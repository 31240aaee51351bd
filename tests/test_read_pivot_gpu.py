"""-m gpu: the read-level input of `detect` — nmod_pivot_reads / nmod_select_tested / nmod_gather_tested against the host
grouping they replace (fast5_ingest.GroupBuilder, cli.select_positions), and `cli detect` on read-level inputs against the
per-position container route, the FAST5-folder routes and the oracle."""
import os
import tempfile

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

MASK40 = (1 << 40) - 1


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


def _quiet(*a):
    pass


def _fixture_reads(group):
    """the fixture's reads of one group as the folder walk sees them (files under 'mall' or without the suffix are not read)"""
    from nanomod_amd import fast5_ingest
    with tempfile.TemporaryDirectory() as tmp:
        return fast5_ingest.ingest_folder_reads(H.write_placeholder_reads(tmp, group), None, H.placeholder_reader, log=_quiet)


def _group_builder(reads, opts):
    from nanomod_amd import fast5_ingest
    gb = fast5_ingest.GroupBuilder(opts, log=_quiet)
    v = reads['norm_mean']
    v = v.astype(np.float64) / 1000.0 if v.dtype == np.int16 else v.astype(np.float64)
    for r in range(len(reads['start'])):
        a, b = reads['off'][r], reads['off'][r + 1]
        gb.add_read(str(reads['chrom'][r]), int(reads['start'][r]), str(reads['strand'][r]), v[a:b], reads['base'][a:b].astype('U1'))
    return gb.finish()


def _as_f64(t):
    x = t.cpu().numpy()
    return x.astype(np.float64) / 1000.0 if x.dtype == np.int16 else x.astype(np.float64)


def _check_pivot(p, exp):
    names = np.array(p['names'], dtype=str)
    key = p['key'].cpu().numpy()
    assert len(key) == len(exp['pos'])
    assert np.array_equal(names[key >> 41], exp['chrom'])
    assert np.array_equal(np.where((key >> 40) & 1, '-', '+'), exp['strand'])
    assert np.array_equal(key & MASK40, exp['pos'])
    assert np.array_equal(p['off'].cpu().numpy(), exp['off'])
    assert np.array_equal(p['base'].cpu().numpy().view('S1').astype('U1'), exp['base'])
    assert np.array_equal(_as_f64(p['sig']), exp['sig'])                      # row contents AND order within rows


def _pivot_like_cli(nm, reads, opts, names=None):
    from nanomod_amd import fast5_ingest
    sel = fast5_ingest.select_reads(reads, opts, _quiet)
    lo, hi = (opts['start_pos'], opts['end_pos']) if 'start_pos' in opts and 'end_pos' in opts else (None, None)
    return nm.engine.pivot_reads(sel, 0, lo, hi, names=names)


def test_pivot_fixture_reads_equal_group_builder_and_the_reference_reader(nm):
    for g in (0, 1):
        reads = _fixture_reads(g)
        opts = {'min_lr': 500, 'min_lr_nb': 0}
        p = _pivot_like_cli(nm, reads, opts)
        exp = _group_builder(reads, opts)
        _check_pivot(p, exp)
        # the reference's own ReadAllFast5 over the same reads: the same positions, the same multiset per position
        ref = dict(np.load(os.path.join(H.GOLDEN, 'fast5_expected_g%d.npz' % g)))
        assert np.array_equal(ref['pos'], exp['pos']) and np.array_equal(ref['chrom'], exp['chrom'])
        assert np.array_equal(ref['off'], p['off'].cpu().numpy())
        got = _as_f64(p['sig']); o = ref['off']
        for i in range(len(o) - 1):
            assert np.array_equal(np.sort(got[o[i]:o[i + 1]]), np.sort(np.asarray(ref['sig'][o[i]:o[i + 1]], np.float64)))


def _random_reads(rng, nreads, kind, chroms=('chr1', 'chr2', 'chrM'), span=3000, max_len=600):
    lens = rng.integers(0, max_len, nreads)
    lens[rng.random(nreads) < 0.05] = 0
    lens[rng.random(nreads) < 0.05] = 1
    off = np.zeros(nreads + 1, np.int64); off[1:] = np.cumsum(lens)
    k = rng.integers(-3000, 3000, off[-1])
    vals = {'f64': k / 1000.0 + rng.normal(0, 1e-7, off[-1]) * (rng.random(off[-1]) < 0.3),
            'f32': (k / 1000.0).astype(np.float32), 'i16': k.astype(np.int16)}[kind]
    return dict(chrom=rng.choice(np.array(chroms), nreads), strand=rng.choice(np.array(['+', '-']), nreads),
                start=rng.integers(0, span, nreads).astype(np.int64), off=off, norm_mean=vals,
                base=rng.choice(np.array(list(b'ACGT'), dtype=np.uint8), off[-1]).view('S1'))


@pytest.mark.parametrize('kind', ['f64', 'f32', 'i16'])
def test_pivot_random_reads_equal_group_builder(nm, kind):
    rng = np.random.default_rng({'f64': 1, 'f32': 2, 'i16': 3}[kind])
    reads = _random_reads(rng, 900, kind)
    for opts in ({'min_lr': 0}, {'min_lr': 0, 'Chr': 'chr2', 'start_pos': 700, 'end_pos': 1900},
                 {'min_lr': 50, 'Chr': 'chr1', 'Pos': 100, 'Pos2': 2500}):
        _check_pivot(_pivot_like_cli(nm, reads, opts, names=['chr1', 'chr2', 'chrM']), _group_builder(reads, opts))


def test_pivot_deep_rows_and_determinism(nm):
    """one position with > 2 048 reads, one with > 65 535 one-event reads (the deep range), and two runs bit-identical"""
    rng = np.random.default_rng(9)
    n_long, n_short = 5000, 66000
    lens = np.concatenate([rng.integers(1, 40, n_long), np.ones(n_short, np.int64)])
    start = np.concatenate([500 - (rng.random(n_long) * lens[:n_long]).astype(np.int64), np.full(n_short, 900, np.int64)])
    perm = rng.permutation(len(lens))
    lens, start = lens[perm], start[perm]
    off = np.zeros(len(lens) + 1, np.int64); off[1:] = np.cumsum(lens)
    reads = dict(chrom=np.full(len(lens), 'c'), strand=np.where(start == 900, '+', rng.choice(np.array(['+', '-']), len(lens))), start=start, off=off,
                 norm_mean=rng.integers(-3000, 3000, off[-1]).astype(np.int16),
                 base=rng.choice(np.array(list(b'ACGT'), dtype=np.uint8), off[-1]).view('S1'))
    p = nm.engine.pivot_reads(reads)
    exp = _group_builder(reads, {'min_lr': 0})
    assert np.diff(exp['off']).max() > 65535 and np.sort(np.diff(exp['off']))[-2] > 2048
    _check_pivot(p, exp)
    q = nm.engine.pivot_reads(reads)
    for k in ('key', 'off', 'sig', 'base'):
        assert np.array_equal(p[k].cpu().numpy(), q[k].cpu().numpy())


@pytest.mark.parametrize('kind,want', [('f32', 'float32'), ('i16', 'int16'), ('f64', 'float64')])
def test_select_and_gather_equal_select_positions(nm, kind, want):
    from nanomod_amd import cli
    rng = np.random.default_rng(20 + len(kind))
    names = ['chr1', 'chr2', 'chrM']
    r0, r1 = _random_reads(rng, 700, kind, span=1500), _random_reads(rng, 650, kind, span=1500)
    if kind == 'i16':                                   # off the float32 grid: int16 stays int16
        r0['norm_mean'][0] = 1234; r1['norm_mean'][0] = -567
    g0, g1 = nm.engine.pivot_reads(r0, names=names), nm.engine.pivot_reads(r1, names=names)
    meta, s0, o0, s1, o1, rid = nm.engine.select_tested(g0, g1, 5, log=_quiet)
    e0, e1 = _group_builder(r0, {'min_lr': 0}), _group_builder(r1, {'min_lr': 0})
    em, es0, eo0, es1, eo1, erid = cli.select_positions(e0, e1, 5, 3, _quiet)
    assert len(erid) > 100
    for k in ('chrom', 'strand', 'pos', 'base', 'n0', 'n1'):
        assert np.array_equal(meta[k], em[k]), k
    assert np.array_equal(o0.cpu().numpy(), eo0) and np.array_equal(o1.cpu().numpy(), eo1)
    assert np.array_equal(rid.cpu().numpy(), erid)
    assert str(s0.cpu().numpy().dtype) == str(es0.dtype) == want
    assert np.array_equal(s0.cpu().numpy(), es0) and np.array_equal(s1.cpu().numpy(), es1)


def _oracle_lines(method):
    import nanomod_oracle as orc
    from nanomod_amd import cli
    e0, e1 = (dict(np.load(os.path.join(H.GOLDEN, 'fast5_expected_g%d.npz' % g))) for g in (0, 1))
    meta, sig0, off0, sig1, off1, rid = cli.select_positions(e0, e1, 5, 3, _quiet)
    s0 = np.asarray(sig0, dtype=np.float64) * (1e-3 if np.asarray(sig0).dtype == np.int16 else 1.0)
    s1 = np.asarray(sig1, dtype=np.float64) * (1e-3 if np.asarray(sig1).dtype == np.int16 else 1.0)
    out = orc.detect_batch(s0, off0, s1, off1, rid, 2, 2.0, {'ks': orc.METHOD_KS, 'stouffer': orc.METHOD_STOUFFER}[method])
    lines = []
    for i in range(len(rid)):
        rec = [(out['mwu_u'][i], out['mwu_p'][i]), (out['t_t'][i], out['t_p'][i]), (out['ks_d'][i], out['ks_p'][i])]
        if method != 'ks':
            rec.append((out['comb_st'][i], out['comb_p'][i]))
        lines.append(orc.format_sign_test_line(str(meta['chrom'][i]), str(meta['strand'][i]), int(meta['pos'][i]), str(meta['base'][i]),
                                               int(meta['n0'][i]), int(meta['n1'][i]), rec, method != 'ks'))
    return ''.join(lines)


def _run_routes(tmp, extra, containers=True):
    """the table of every route: read-level containers, folders (host), folders (--devicePivot 1), per-position containers"""
    from nanomod_amd import cli, container, fast5_ingest
    dirs = [os.path.join(tmp, 'grp%d' % g) for g in (0, 1)]
    if not os.path.isdir(dirs[0]):
        dirs = [H.write_placeholder_reads(tmp, g) for g in (0, 1)]
    rl, pp = [], []
    for g in (0, 1):
        r = fast5_ingest.ingest_folder_reads(dirs[g], None, H.placeholder_reader, log=_quiet)
        rl.append(os.path.join(tmp, 'r%d.npz' % g))
        container.save_reads(rl[-1], r['chrom'], r['strand'], r['start'], r['off'], r['norm_mean'], r['base'])
        c = fast5_ingest.ingest_folder(dirs[g], {'min_lr': 500, 'min_lr_nb': 0}, H.placeholder_reader, log=_quiet)
        pp.append(os.path.join(tmp, 'p%d.npz' % g))
        container.save_group(pp[-1], c['chrom'], c['strand'], c['pos'], c['base'], c['off'], c['sig'])
    rd = ['--fast5Reader', 'helpers:placeholder_reader']
    routes = {'reads': [rl[0], rl[1]], 'folders': [dirs[0], dirs[1]] + rd, 'folders_dev': [dirs[0], dirs[1]] + rd + ['--devicePivot', '1']}
    if containers:
        routes['containers'] = [pp[0], pp[1]]
    out = {}
    for name, args in routes.items():
        od = os.path.join(tmp, 'out_' + name + '_' + '_'.join(extra).replace(':', '-').replace('-', ''))
        rc = cli.main(['detect', '--wrkBase1', args[0], '--wrkBase2', args[1], '--outFolder', od] + args[2:] +
                      ['--FileID', 'x', '--topN', '5', '--outLevel', '3', '--MinCoverage', '5'] + extra)
        assert rc == 0, name
        out[name] = {f: open(os.path.join(od, f)).read() for f in os.listdir(od)}
    return out


@pytest.mark.parametrize('method', ['stouffer', 'ks'])
def test_cli_detect_on_read_level_inputs(nm, method, capsys):
    with tempfile.TemporaryDirectory() as tmp:
        out = _run_routes(tmp, ['--testMethod', method])
        got = out['reads']['x_sign_test.txt']
        for name in ('folders', 'folders_dev', 'containers'):
            assert out[name]['x_sign_test.txt'] == got, name
        assert got.count('\n') > 1000
        assert got == _oracle_lines(method)
        if method == 'stouffer':
            out = _run_routes(tmp, ['--mstd', '1'])
            for name in ('folders', 'folders_dev', 'containers'):
                assert out[name] == out['reads'], name
            assert out['reads']['x_meanstd.cvs'].count('\n') > 1000
            # a region of interest: the read-level part of the filter needs the reads, so only the read routes compare
            roi = 'chrB:602'                            # 21 positions a strand, each covered by >= 5 reads in both groups
            out = _run_routes(tmp, ['--Pos', roi], containers=False)
            assert out['folders'] == out['reads'] == out['folders_dev']
            assert out['reads']['x_sign_test.txt'].count('\n') == 42
    capsys.readouterr()


def test_cli_detect_with_every_read_filtered_out(nm, capsys):
    with tempfile.TemporaryDirectory() as tmp:
        out = _run_routes(tmp, ['--min_lr', '1000000'], containers=False)
        assert out['reads'] == out['folders'] == out['folders_dev']
        assert out['reads']['x_sign_test.txt'] == ''
    capsys.readouterr()


def test_pivot_many_adjacent_large_rows(nm):
    """hundreds of neighbouring rows beyond the LDS ranking (1 024 samples) at once, in two dtypes: every row's samples in read
    order and in place, and the bytes of two runs identical"""
    rng = np.random.default_rng(31)
    n = 3000
    lens = rng.integers(560, 640, n)
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum(lens)
    for vals in (rng.integers(-3000, 3000, off[-1]).astype(np.int16), rng.normal(0, 1, off[-1])):
        reads = dict(chrom=np.full(n, 'c'), strand=rng.choice(np.array(['+', '-']), n), start=rng.integers(0, 60, n).astype(np.int64),
                     off=off, norm_mean=vals, base=rng.choice(np.array(list(b'ACGT'), dtype=np.uint8), off[-1]).view('S1'))
        p = nm.engine.pivot_reads(reads)
        exp = _group_builder(reads, {'min_lr': 0})
        assert (np.diff(exp['off']) > 1024).sum() > 500
        _check_pivot(p, exp)
        q = nm.engine.pivot_reads(reads)
        for k in ('key', 'off', 'sig', 'base'):
            assert np.array_equal(p[k].cpu().numpy(), q[k].cpu().numpy())


def test_cli_detect_read_level_with_downsampling(nm, capsys):
    """--coverages on the device route: the tested rows come back to the host for the seeded down-sampling step"""
    with tempfile.TemporaryDirectory() as tmp:
        out = _run_routes(tmp, ['--coverages', '6', '--downsampling', '20'])
        for name in ('folders', 'folders_dev', 'containers'):
            assert out[name] == out['reads'], name
        base = _run_routes(tmp, [])
        assert out['reads']['x_sign_test.txt'] != base['reads']['x_sign_test.txt']     # the step changed some KS pairs
    capsys.readouterr()
