"""nmod_rescale_reads (K11) on the GPU against the numpy restatement of its definition (tests/rescale_ref.py): parity over every
length at which the code takes another path, the bit-defined apply step, every status, the independence of a read's bits from the
batch, and the read-level route through the Python layers and the command line."""
import os
import tempfile

import numpy as np
import pytest

import helpers as H
import rescale_ref as R
from nanomod_amd import rescale as _the_feature  # noqa: F401  (K11's module: without it nothing here can pass)

pytestmark = pytest.mark.gpu

GATE = dict(rel=1e-11, abs_=1e-12)                # the moment gate of the issue: scale, shift and rescaled float values


def _engine():
    from nanomod_amd import engine
    return engine


def _model(p, k, center):
    return dict(k=k, center=center, mean=p['mean'], sd=p['sd'])


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _check_against(got, exp, dtype):
    assert np.array_equal(got['status'], exp['status']), (got['status'], exp['status'])
    assert np.array_equal(got['n_used'], exp['n_used']), (got['n_used'], exp['n_used'])
    H.assert_close_stat(got['scale'], exp['scale'], name='scale', **GATE)
    H.assert_close_stat(got['shift'], exp['shift'], name='shift', **GATE)
    assert got['val'].dtype == exp['val'].dtype == np.dtype(dtype)
    if np.dtype(dtype) == np.int16:
        t = exp['t1000']
        with np.errstate(invalid='ignore'):
            near_half = np.abs(t - np.floor(t) - 0.5) <= 1e-6
        d = np.abs(got['val'].astype(np.int64) - exp['val'].astype(np.int64))
        assert (d[~near_half] == 0).all() and (d <= 1).all(), (int((d != 0).sum()), int(d.max()))
    else:
        H.assert_close_stat(got['val'], exp['val'], name='val', **GATE)


@pytest.mark.parametrize('k,center,dtype,weighted,clip_rounds', R.PARITY_CASES)
def test_parity_with_the_restatement(k, center, dtype, weighted, clip_rounds):
    p = R.parity_inputs(k, center, dtype)
    exp = R.parity_expected(k, center, dtype, weighted, clip_rounds)
    got = _engine().rescale_reads_host(p['val'], p['off'], p['base'], _model(p, k, center), weighted=weighted, clip_sigma=3.0,
                                       clip_rounds=clip_rounds, min_events=R.PARITY_MIN_EVENTS)
    lens = np.diff(p['off'])
    assert (exp['status'][lens >= 63] == 0).all() and (exp['status'][lens <= k + 1] == R.TOO_FEW).all() and lens.max() == 70000
    _check_against(got, exp, dtype)
    only = _engine().rescale_reads_host(p['val'], p['off'], p['base'], _model(p, k, center), mode='fit_only', weighted=weighted, clip_sigma=3.0,
                                        clip_rounds=clip_rounds, min_events=R.PARITY_MIN_EVENTS)
    assert 'val' not in only and all(_bits(only[f]) == _bits(got[f]) for f in ('shift', 'scale', 'n_used'))
    assert np.array_equal(only['status'], got['status'] & ~np.uint8(R.CLAMPED))


@pytest.mark.parametrize('dtype', ['int16', 'float32', 'float64'])
def test_apply_only_is_bit_exact(dtype):
    rng = np.random.default_rng(77)
    lens = [0, 1, 63, 65, 700, R.WAVE_MAX, R.WAVE_MAX + 1, 5000, 90, 33, 12, 40, 50]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    x = np.rint(rng.normal(0.0, 2.0, off[-1]) * 1000.0) / 1000.0
    x[rng.choice(len(x), 40, replace=False)] = rng.choice([32.767, -32.767, 30.0, -29.5], 40)
    val = R.cast(x, dtype)
    if dtype != 'int16':
        val[[5, 100, 3000]] = [np.nan, np.inf, -np.inf]
    shift = rng.uniform(-0.5, 0.5, len(lens))
    scale = rng.uniform(0.4, 1.6, len(lens))
    scale[4] = 0.01                                                         # int16: saturates
    shift[8], scale[9], scale[10], scale[11], shift[12] = np.nan, 0.0, -1.0, np.inf, np.inf
    exp = R.rescale(val, off, None, mode=R.APPLY_ONLY, shift=shift, scale=scale)
    got = _engine().rescale_reads_host(val, off, None, mode='apply_only', shift=shift, scale=scale)
    assert np.array_equal(got['status'], exp['status']) and not got['n_used'].any()
    assert (exp['status'][8:] == R.DEGENERATE).all() and (exp['status'][4] == R.CLAMPED) == (dtype == 'int16')
    assert _bits(got['val']) == _bits(exp['val']) and got['val'].dtype == val.dtype
    assert _bits(got['shift']) == _bits(shift) and _bits(got['scale']) == _bits(scale)          # inputs, left as they are
    assert _bits(got['val'][off[8]:]) == _bits(val[off[8]:])                                    # degenerate reads: unchanged


def _status_batch(dtype):
    """one read per status case over a 3-mer model with holes: (val, off, base, mean, sd, names)"""
    k, center = 3, 1
    rng = np.random.default_rng(314)
    mean, sd = R.make_model(k)
    reads, names = [], []

    def add(name, base, x):
        names.append(name); reads.append((np.asarray(base, np.uint8), np.asarray(x, np.float64)))

    add('fitted', *R.draw_read(rng, 400, k, center, mean, sd, 0.1, 1.1))
    add('too_few', *R.draw_read(rng, 40, k, center, mean, sd, 0.1, 1.1))
    b, x = R.draw_read(rng, 70, k, center, mean, sd, 0.0, 1.0, contaminate=False)
    x[5:30] += 3.0                                                           # 68 eligible at first, fewer than 50 after a clip
    add('too_few_after_clip', b, x)
    add('homopolymer', np.full(200, ord('A'), np.uint8), np.rint(rng.normal(0.0, 0.2, 200) * 1000.0) / 1000.0)
    b, x = R.draw_read(rng, 300, k, center, mean, sd, 0.0, 1.0, contaminate=False)
    add('negative_slope', b, -x)
    add('scale_out_of_range', *R.draw_read(rng, 300, k, center, mean, sd, 0.0, 3.0, contaminate=False))
    b, x = R.draw_read(rng, 300, k, center, mean, sd, -0.2, 0.9)
    if dtype != 'int16':
        x[[3, 50, 200]] = [np.nan, np.inf, -np.inf]
    add('nonfinite_samples', b, x)
    b = np.tile(np.frombuffer(b'AATACGGCGTAACC', np.uint8), 30)            # codes 3 (AAT), 6 (ACG), 9 (AGC: absent) ... holes of the model
    add('model_holes', b, R.draw_values(rng, b, k, center, mean, sd, 0.2, 1.2))
    b, x = R.draw_read(rng, 300, k, center, mean, sd, 0.05, 1.0)
    b[[10, 11, 150]] = [ord('N'), ord('a'), ord('c')]
    add('other_bytes', b, x)
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r[1]) for r in reads])
    return R.cast(np.concatenate([r[1] for r in reads]), dtype), off, np.concatenate([r[0] for r in reads]), mean, sd, names


@pytest.mark.parametrize('dtype', ['int16', 'float32', 'float64'])
def test_status_cases(dtype):
    k, center = 3, 1
    val, off, base, mean, sd, names = _status_batch(dtype)
    exp = R.rescale(val, off, base, k, center, mean, sd, min_events=50)
    st = dict(zip(names, exp['status'].tolist()))
    used = dict(zip(names, exp['n_used'].tolist()))
    assert st == dict(fitted=0, too_few=R.TOO_FEW, too_few_after_clip=R.TOO_FEW, homopolymer=R.DEGENERATE, negative_slope=R.DEGENERATE,
                      scale_out_of_range=R.OUT_OF_RANGE, nonfinite_samples=0, model_holes=0, other_bytes=0), st
    assert 0 < used['too_few'] < 50 and 0 < used['too_few_after_clip'] < 50 and used['homopolymer'] == 198
    i = names.index('model_holes')
    codes = R.read_codes(base[off[i]:off[i + 1]], k, center)
    assert used['model_holes'] < int((codes >= 0).sum()) - 50 and np.isin(codes, (3, 6, 12)).sum() > 50     # the holes are ineligible
    got = _engine().rescale_reads_host(val, off, base, dict(k=k, center=center, mean=mean, sd=sd), min_events=50)
    _check_against(got, exp, dtype)
    failed = np.flatnonzero(exp['status'] & (R.TOO_FEW | R.DEGENERATE | R.OUT_OF_RANGE))
    for i in failed:                                                          # unchanged, with (0, 1)
        assert got['shift'][i] == 0.0 and got['scale'][i] == 1.0 and _bits(got['val'][off[i]:off[i + 1]]) == _bits(val[off[i]:off[i + 1]])
    if dtype != 'int16':                                                      # the non-finite samples stay as they are
        j = off[names.index('nonfinite_samples')]
        assert _bits(got['val'][j + np.array([3, 50, 200])]) == _bits(val[j + np.array([3, 50, 200])])


def _permuted(p, order):
    lens = np.diff(p['off'])[order]
    off = np.zeros(len(order) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    ev = np.concatenate([np.arange(p['off'][i], p['off'][i + 1]) for i in order]) if len(order) else np.zeros(0, np.int64)
    return p['val'][ev], off, p['base'][ev]


@pytest.mark.parametrize('dtype,k', [('int16', 5), ('float64', 8), ('float32', 1)])
def test_bits_do_not_depend_on_order_batch_memspace_or_in_place(dtype, k):
    import torch
    from nanomod_amd import DeviceDetector
    p = R.parity_inputs(k, 0, dtype)
    model = _model(p, k, 0)
    kw = dict(min_events=R.PARITY_MIN_EVENTS)
    first = _engine().rescale_reads_host(p['val'], p['off'], p['base'], model, **kw)
    nreads = len(p['off']) - 1
    fields = ('shift', 'scale', 'n_used', 'status')
    for order in (np.random.default_rng(9).permutation(nreads), np.array([13, 5]), np.array([10])):
        val, off, base = _permuted(p, order)
        again = _engine().rescale_reads_host(val, off, base, model, **kw)
        assert all(_bits(again[f]) == _bits(first[f][order]) for f in fields)
        assert _bits(again['val']) == _bits(_permuted(dict(p, val=first['val']), order)[0])
    det = DeviceDetector(0)
    t = lambda x: torch.from_numpy(np.array(x)).cuda()
    d_val, d_off, d_base, d_mean, d_sd = t(p['val']), t(p['off']), t(R.as_bytes(p['base'])), t(p['mean']), t(p['sd'])
    out = det.rescale_reads(d_val, d_off, d_base, d_mean, d_sd, k, 0, **kw)
    assert all(_bits(out[f].cpu().numpy()) == _bits(first[f]) for f in fields) and _bits(out['val'].cpu().numpy()) == _bits(first['val'])
    assert _bits(d_val.cpu().numpy()) == _bits(p['val'])
    inplace = det.rescale_reads(d_val, d_off, d_base, d_mean, d_sd, k, 0, inplace=True, **kw)
    assert inplace['val'] is d_val and _bits(d_val.cpu().numpy()) == _bits(first['val'])
    assert all(_bits(inplace[f].cpu().numpy()) == _bits(first[f]) for f in fields)


def _read_set(dtype='int16', **kw):
    k, center = 3, 1
    mean, sd = R.make_model(k, holes=False)
    return R.make_read_set(4242, k, center, mean, sd, dtype=dtype, **kw), dict(k=k, center=center, mean=mean, sd=sd)


def test_device_entry_composes_with_pivot_reads():
    import torch
    from nanomod_amd import DeviceDetector, rescale
    reads, model = _read_set(contaminate=True)
    host_reads, table = rescale.rescale_reads(reads, dict(model, n_positions=np.ones(64, np.int64)), log=lambda *a: None)
    assert (table['status'] == 0).all()
    want = _engine().pivot_reads(host_reads)
    det = DeviceDetector(0)
    t = lambda x: torch.from_numpy(np.array(x)).cuda()
    with torch.cuda.stream(torch.cuda.Stream()):
        out = det.rescale_reads(t(reads['norm_mean']), t(reads['off']), t(R.as_bytes(reads['base'])), t(model['mean']), t(model['sd']), 3, 1)
        got = _engine().pivot_reads(reads, val=out['val'])
        torch.cuda.current_stream().synchronize()
    assert all(_bits(got[f].cpu().numpy()) == _bits(want[f].cpu().numpy()) for f in ('key', 'off', 'sig', 'base')) and got['names'] == want['names']
    assert _bits(out['shift'].cpu().numpy()) == _bits(table['shift']) and _bits(out['scale'].cpu().numpy()) == _bits(table['scale'])


@pytest.mark.parametrize('dtype', ['int16', 'float64'])
def test_reads_to_group_equals_the_group_builder(dtype):
    from nanomod_amd import fast5_ingest
    reads, _ = _read_set(dtype)
    gb = fast5_ingest.GroupBuilder({'min_lr': 0}, log=lambda *a: None)
    x = R.to_double(reads['norm_mean'])
    for i in range(len(reads['start'])):
        b, e = reads['off'][i], reads['off'][i + 1]
        assert gb.add_read(str(reads['chrom'][i]), int(reads['start'][i]), str(reads['strand'][i]), x[b:e], reads['base'][b:e].astype('U1'))
    want = gb.finish()
    got = _engine().reads_to_group(reads)
    assert got['sig'].dtype == np.dtype(dtype) and len(want['pos']) > 500
    for f in ('chrom', 'strand', 'pos', 'base', 'off'):
        assert np.array_equal(np.asarray(got[f]).astype(np.asarray(want[f]).dtype), want[f]), f
    assert np.array_equal(R.to_double(got['sig']), want['sig'])


def test_end_to_end_through_the_command_line():
    """kmermodel on a synthetic control, rescale on a sample whose reads carry planted shifts and scales, then kmerprofile and detect1
    reading the rescaled read-level container directly: the same outputs as the steps called as functions on reads_to_group"""
    from nanomod_amd import cli, container, kmermodel, onesample, rescale
    k, center = 3, 1
    mean, sd = R.make_model(k, holes=False)
    control = R.make_read_set(1, k, center, mean, sd, reads_per_strand=20, planted=False)
    sample = R.make_read_set(2, k, center, mean, sd, reads_per_strand=10, planted=True, contaminate=True)
    fields = ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')
    quiet = lambda *a: None
    with tempfile.TemporaryDirectory() as tmp:
        c_path, s_path, r_path, out = (os.path.join(tmp, n) for n in ('control_reads.npz', 'sample_reads.npz', 'rescaled_reads.npz', 'cli'))
        container.save_reads(c_path, *[control[f] for f in fields])
        container.save_reads(s_path, *[sample[f] for f in fields])
        # the control is read-level too: kmermodel groups it on the device
        assert cli.main(['kmermodel', '--wrkBase1', c_path, '--kmer', '3', '--kmerCenter', '1', '--outFolder', out, '--FileID', 'ctl', '--outLevel', '3']) == 0
        m_path = os.path.join(out, 'ctl_kmer_model.npz')
        model = kmermodel.load_kmer_model(m_path)
        direct = kmermodel.build_kmer_model(_engine().reads_to_group(container.load_reads(c_path)), k, center, log=quiet)
        assert all(_bits(model[f]) == _bits(direct[f]) for f in kmermodel.KMER_MODEL_FIELDS) and (model['n_positions'] > 0).all()
        assert cli.main(['rescale', '--wrkBase1', s_path, '--kmerModel', m_path, '--outReads', r_path, '--outFolder', out, '--FileID', 'smp',
                         '--outLevel', '3']) == 0
        back = container.load_reads(r_path)
        loaded = container.load_reads(s_path)
        res = _engine().rescale_reads_host(loaded['norm_mean'], loaded['off'], loaded['base'], rescale.masked_model(model, 1))
        assert back['norm_mean'].dtype == np.int16 and _bits(back['norm_mean']) == _bits(res['val']) and (res['status'] == 0).all()
        assert all(np.array_equal(back[f], loaded[f]) for f in ('chrom', 'strand', 'start', 'off', 'base'))
        # the planted pairs come back (the control carries none): loose bounds, the statistical ones are test_rescale.py's
        assert np.abs(res['shift'] - sample['a_true']).max() < 0.1 and np.abs(res['scale'] / sample['b_true'] - 1.0).max() < 0.1
        lines = open(os.path.join(out, 'smp_read_scale.txt')).read().splitlines()
        n = np.diff(loaded['off'])
        assert len(lines) == len(n) and lines[3] == '%d %s %s %d %d %d %.6f %.6f %d' % (
            3, loaded['chrom'][3], loaded['strand'][3], loaded['start'][3], n[3], res['n_used'][3], res['shift'][3], res['scale'][3], res['status'][3])
        assert cli.main(['kmerprofile', '--kmerModel', m_path, '--wrkBase1', r_path, '--outFolder', out, '--FileID', 'smp', '--outLevel', '3']) == 0
        assert cli.main(['detect1', '--wrkBase1', r_path, '--refProfile', os.path.join(out, 'smp_profile.npz'), '--outFolder', out,
                         '--FileID', 'e2e', '--outLevel', '3', '--topN', '3']) == 0
        group = _engine().reads_to_group(back)
        prof = kmermodel.model_profile(model, group, 1)
        prof_cli = onesample.load_profile(os.path.join(out, 'smp_profile.npz'))
        assert prof_cli['kind'] == 'model' and all(np.array_equal(np.asarray(prof[f]), np.asarray(prof_cli[f]))
                                               for f in ('chrom_names', 'chrom_id', 'strand', 'pos', 'base', 'mean', 'sd'))
        mo = {'ds2': ['s'], 's': {'nmod_container': group}, 'nmod_profile': prof, 'MinCoverage': 5, 'neighborPvalues': 2, 'WeightsDif': 2.0,
              'testMethod': 'stouffer', 'rankUse': 'pv', 'SaveTest': 1, 'outFolder': os.path.join(tmp, 'py'), 'FileID': 'e2e', 'outLevel': 3,
              'nmod_quiet': 1}
        onesample.mtest1(mo)
        assert len(mo['one_sample_meta']['pos']) > 500
        assert open(os.path.join(out, 'e2e_one_sample.txt')).read() == open(os.path.join(tmp, 'py', 'e2e_one_sample.txt')).read()


def test_a_read_beyond_max_deep_is_too_large_and_copied():
    """2^24 events: one more than NMOD_MAX_DEEP.  The read is flagged and copied unchanged by its workgroup; its neighbour is fitted"""
    k, center = 3, 1
    mean, sd = R.make_model(k, holes=False)
    rng = np.random.default_rng(8)
    b0, x0 = R.draw_read(rng, 200, k, center, mean, sd, 0.1, 1.1)
    n = R.MAX_DEEP + 1
    big_base = np.tile(np.frombuffer(b'ACGTTGCA', np.uint8), n // 8)
    big = (np.arange(n, dtype=np.int64) % 2001 - 1000).astype(np.int16)
    val, base = np.concatenate([big, R.cast(x0, 'int16')]), np.concatenate([big_base, b0])
    off = np.array([0, n, n + 200], np.int64)
    exp = R.rescale(val, off, base, k, center, mean, sd, min_events=50)
    assert exp['status'].tolist() == [R.TOO_LARGE, 0]
    got = _engine().rescale_reads_host(val, off, base, dict(k=k, center=center, mean=mean, sd=sd), min_events=50)
    _check_against(got, exp, 'int16')
    assert got['shift'][0] == 0.0 and got['scale'][0] == 1.0 and got['n_used'][0] == 0 and _bits(got['val'][:n]) == _bits(big)


def test_device_layers_refuse_malformed_tensors():
    import torch
    from nanomod_amd import DeviceDetector
    p = R.parity_inputs(5, 0, 'int16')
    t = lambda x: torch.from_numpy(np.array(x)).cuda()
    val, off, base, mean, sd = t(p['val']), t(p['off']), t(R.as_bytes(p['base'])), t(p['mean']), t(p['sd'])
    det = DeviceDetector(0)
    call = lambda **kw: det.rescale_reads(kw.pop('val', val), kw.pop('off', off), kw.pop('base', base), kw.pop('mean', mean), kw.pop('sd', sd),
                                          kw.pop('k', 5), kw.pop('center', 0), min_events=R.PARITY_MIN_EVENTS, **kw)
    good = call()
    for kw in (dict(val=val.int()), dict(val=val[::2]), dict(val=val.cpu()), dict(off=off.int()), dict(off=off.cpu()), dict(base=base.short()),
               dict(base=base[:-1]), dict(mean=mean[:100]), dict(sd=sd.float()), dict(mean=None), dict(k=9), dict(center=5), dict(clip_rounds=9),
               dict(mode='apply_only'), dict(mode='apply_only', shift=good['shift'][:3], scale=good['scale']),
               dict(out=dict(good, status=good['status'][:3])), dict(out={k_: v for k_, v in good.items() if k_ != 'val'})):
        with pytest.raises(ValueError):
            call(**kw)
    again = call(out=good)
    assert again is good
    reads, _ = _read_set()
    with pytest.raises(ValueError):
        _engine().pivot_reads(reads, val=torch.from_numpy(np.array(reads['norm_mean'])))          # not on the device
    with pytest.raises(ValueError):
        _engine().pivot_reads(reads, val=t(reads['norm_mean'])[:-1])
