"""nmod_rescale_reads (K11) without a GPU: the declaration, the argument checks (before any device work), the event codes against
K10's convention, the conditioning of the restated fit against exact rationals, the conditions the shared inputs must meet for the
GPU gates, what the definition recovers from clean and from contaminated reads, the command line and the table writer."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

import rescale_ref as R
from nanomod_amd import rescale as RS             # K11's module: without it nothing here can pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine


def _lib():
    import nanomod_amd._lib as L
    return L, L.load()


def test_rescale_reads_is_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, 'include', 'nanomod_hip.h')).read()
    assert 'nmod_rescale_reads' in set(re.findall(r'\b(nmod_[a-z_]+)\s*\(', header))
    assert 'nmod_rescale_reads' in L._SIGNATURES and hasattr(lib, 'nmod_rescale_reads')
    assert 'enum { NMOD_RESCALE_FIT_APPLY = 0, NMOD_RESCALE_FIT_ONLY = 1, NMOD_RESCALE_APPLY_ONLY = 2 };' in header
    assert (L.RESCALE_FIT_APPLY, L.RESCALE_FIT_ONLY, L.RESCALE_APPLY_ONLY) == (R.FIT_APPLY, R.FIT_ONLY, R.APPLY_ONLY) == (0, 1, 2)
    assert ('enum { NMOD_RESCALE_TOO_FEW = 1, NMOD_RESCALE_DEGENERATE = 2, NMOD_RESCALE_OUT_OF_RANGE = 4, NMOD_RESCALE_CLAMPED = 8, '
            'NMOD_RESCALE_TOO_LARGE = 16 };') in header
    assert (L.RESCALE_TOO_FEW, L.RESCALE_DEGENERATE, L.RESCALE_OUT_OF_RANGE, L.RESCALE_CLAMPED, L.RESCALE_TOO_LARGE) == \
        (R.TOO_FEW, R.DEGENERATE, R.OUT_OF_RANGE, R.CLAMPED, R.TOO_LARGE) == (1, 2, 4, 8, 16)
    assert '#define NMOD_RESCALE_WAVE_MAX 2048' in header and L.RESCALE_WAVE_MAX == R.WAVE_MAX == 2048 and L.MAX_DEEP == R.MAX_DEEP
    assert C.sizeof(L.NmodRescaleModel) == 24 and C.sizeof(L.NmodRescaleOpts) == 48 and C.sizeof(L.NmodRescaleOut) == 48
    assert L.NmodRescaleOpts.clip_sigma.offset == 24 and L.NmodRescaleOut.val_out.offset == 40 and L.NmodRescaleModel.mean.offset == 8
    assert '#define NMOD_ABI_VERSION 4' in header and lib.nmod_abi_version() == 4 == L.NMOD_ABI_VERSION      # a purely additive entry


def _call(lib, L, nreads=3, *, off='x', val='x', base='x', model='x', k=3, center=1, mean='x', sd='x', opts=None, out='x', val_out='x',
          shift='x', scale='x', dtype=None, memspace=None, prm=None, opts_size=None, out_size=None, **okw):
    n = nreads if 0 <= nreads < 1000 else 3
    offs = np.arange(n + 1, dtype=np.int64) * 60
    x, b = np.zeros(max(n, 1) * 60, np.int16), np.full(max(n, 1) * 60, ord('A'), np.uint8)
    mu, s = np.zeros(4 ** 8), np.ones(4 ** 8)
    res = dict(shift=np.zeros(max(n, 1)), scale=np.ones(max(n, 1)), n_used=np.zeros(max(n, 1), np.int32), status=np.zeros(max(n, 1), np.uint8),
               val_out=np.zeros_like(x))
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    m = L.NmodRescaleModel()
    m.k, m.center, m.mean, m.sd = k, center, pick(mean, mu), pick(sd, s)
    o = L.make_rescale_opts(**okw) if opts is None else opts
    if opts_size is not None:
        o.struct_size = opts_size
    r = L.make_rescale_out(shift=pick(shift, res['shift']), scale=pick(scale, res['scale']), n_used=res['n_used'].ctypes.data,
                           status=res['status'].ctypes.data, val_out=pick(val_out, res['val_out']))
    if out_size is not None:
        r.struct_size = out_size
    if prm is None:
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace,
                            dtype=L.DTYPE_I16_MILLI if dtype is None else dtype)
    return lib.nmod_rescale_reads(C.byref(prm), nreads, pick(off, offs), pick(val, x), pick(base, b), C.byref(m) if model is not None else None,
                                  C.byref(o) if opts != 'null' else None, C.byref(r) if out is not None else None)


def test_invalid_arguments_are_refused_before_any_device_work():
    """every case of the header returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone is NMOD_ERR_NO_DEVICE)"""
    L, lib = _lib()
    nan, inf = float('nan'), float('inf')
    assert _call(lib, L) == -5                                                  # the well-formed call reaches the device check
    assert _call(lib, L, memspace=L.MEM_DEVICE) == -5 and _call(lib, L, dtype=L.DTYPE_F32) == -5 and _call(lib, L, dtype=L.DTYPE_F64) == -5
    assert _call(lib, L, mode=L.RESCALE_FIT_ONLY, val_out=None) == -5
    assert _call(lib, L, mode=L.RESCALE_APPLY_ONLY, base=None, model=None) == -5
    assert _call(lib, L, k=1, center=0) == -5 and _call(lib, L, k=8, center=7) == -5 and _call(lib, L, clip_rounds=0, clip_sigma=nan) == -5
    assert _call(lib, L, clip_rounds=8) == -5 and _call(lib, L, min_events=2) == -5 and _call(lib, L, scale_lo=1.0, scale_hi=1.0) == -5
    assert _call(lib, L, 0) == 0 and _call(lib, L, 0, off=None, val=None, base=None, val_out=None) == 0        # no reads: no device needed
    assert _call(lib, L, mode=3) == -1 and _call(lib, L, mode=-1) == -1
    assert _call(lib, L, k=0, center=0) == -1 and _call(lib, L, k=9) == -1 and _call(lib, L, center=3) == -1 and _call(lib, L, center=-1) == -1
    assert _call(lib, L, clip_rounds=-1) == -1 and _call(lib, L, clip_rounds=9) == -1
    assert all(_call(lib, L, clip_sigma=v) == -1 for v in (0.0, -3.0, nan, inf))
    assert _call(lib, L, min_events=1) == -1 and _call(lib, L, min_events=0) == -1
    assert all(_call(lib, L, scale_lo=v) == -1 for v in (0.0, -0.5, nan, inf, 2.5)) and _call(lib, L, scale_hi=nan) == -1
    assert _call(lib, L, -1) == -1 and _call(lib, L, 2 ** 32 - 1) == -1 and _call(lib, L, 2 ** 40) == -1
    assert _call(lib, L, off=None) == -1 and _call(lib, L, val=None) == -1
    assert _call(lib, L, base=None) == -1 and _call(lib, L, model=None) == -1 and _call(lib, L, mean=None) == -1 and _call(lib, L, sd=None) == -1
    assert _call(lib, L, val_out=None) == -1 and _call(lib, L, mode=L.RESCALE_APPLY_ONLY, val_out=None) == -1
    assert _call(lib, L, mode=L.RESCALE_APPLY_ONLY, shift=None) == -1 and _call(lib, L, mode=L.RESCALE_APPLY_ONLY, scale=None) == -1
    assert _call(lib, L, opts_size=40) == -1 and _call(lib, L, opts_size=56) == -1 and _call(lib, L, opts='null') == -1
    assert _call(lib, L, out_size=40) == -1 and _call(lib, L, out=None) == -1
    assert _call(lib, L, dtype=3) == -1 and _call(lib, L, dtype=-1) == -1
    assert _call(lib, L, off=np.array([0, 60, 40, 180], np.int64)) == -1        # host offsets that decrease
    assert _call(lib, L, off=np.array([-1, 60, 120, 180], np.int64)) == -1
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert _call(lib, L, prm=bad) == -1
    assert lib.nmod_rescale_reads(None, 3, None, None, None, None, None, None) == -1


def test_python_layers_raise_for_the_same_inputs():
    import nanomod_amd
    from nanomod_amd import engine
    mean, sd = R.make_model(3)
    model = dict(k=3, center=1, mean=mean, sd=sd)
    val, off, base = np.zeros(120, np.int16), np.array([0, 60, 120], np.int64), np.full(120, b'A', 'S1')
    call = lambda **kw: engine.rescale_reads_host(kw.pop('val', val), kw.pop('off', off), kw.pop('base', base), kw.pop('model', model),
                                                  device=NO_SUCH_DEVICE, **kw)
    with pytest.raises(nanomod_amd._lib.NanomodLibraryError, match='nmod_rescale_reads'):
        call()                                                                  # well-formed: only the device is missing
    for kw in (dict(mode='fit'), dict(mode=7), dict(model=dict(model, k=0)), dict(model=dict(model, k=9)), dict(model=dict(model, center=3)),
               dict(model=None), dict(clip_rounds=-1), dict(clip_rounds=9), dict(clip_sigma=0.0), dict(clip_sigma=float('nan')),
               dict(min_events=1), dict(scale_range=(0.0, 2.0)), dict(scale_range=(2.5, 2.0)), dict(scale_range=(float('inf'), float('inf'))),
               dict(val=val.astype(np.int32)), dict(off=np.array([0, 70, 60], np.int64)), dict(off=np.array([0, 60, 121], np.int64)),
               dict(base=base[:100]), dict(model=dict(model, mean=mean[:10])), dict(mode='apply_only'),
               dict(mode='apply_only', shift=np.zeros(3), scale=np.ones(3))):
        with pytest.raises(ValueError):
            call(**kw)
    res = call(val=val[:0], off=np.zeros(1, np.int64), base=base[:0])           # no reads: no device needed
    assert res['shift'].shape == (0,) and res['val'].shape == (0,)
    with pytest.raises(ValueError):
        RS.rescale_reads(dict(chrom=['c'] * 2, strand=['+'] * 2, start=[0, 0], off=off, norm_mean=val, base=base),
                         dict(model, n_positions=np.ones(64, np.int64)), clip_rounds=9, device=NO_SUCH_DEVICE)
    assert nanomod_amd.rescale_reads is RS.rescale_reads and nanomod_amd.rescale_reads_host is engine.rescale_reads_host
    assert nanomod_amd.reads_to_group is engine.reads_to_group


@pytest.mark.parametrize('k', [1, 3, 5, 8])
def test_event_codes_agree_with_the_kmer_models_convention(k):
    """every read spans a whole run on its strand, so the code of an event must be the code kmermodel.kmer_codes gives its position;
    both strands, an 'N' inside the run"""
    from nanomod_amd import fast5_ingest, kmermodel
    mean, sd = R.make_model(k)
    for center in sorted({0, k - 1}):
        reads = R.make_read_set(60 + k, k, center, mean, sd, genome_len=120, reads_per_strand=3, full_span=True, n_at=(50,))
        gb = fast5_ingest.GroupBuilder({'min_lr': 0}, log=lambda *a: None)
        for i in range(len(reads['start'])):
            b, e = reads['off'][i], reads['off'][i + 1]
            gb.add_read(str(reads['chrom'][i]), int(reads['start'][i]), str(reads['strand'][i]), R.to_double(reads['norm_mean'][b:e]),
                        reads['base'][b:e].astype('U1'))
        g = gb.finish()
        gcode = kmermodel.kmer_codes(g['chrom'], g['strand'], g['pos'], g['base'], k, center)
        at = {(c, s, int(p)): int(v) for c, s, p, v in zip(g['chrom'], g['strand'], g['pos'], gcode)}
        seen_minus = seen_bad = 0
        for i in range(len(reads['start'])):
            b, e = reads['off'][i], reads['off'][i + 1]
            n = e - b
            codes = R.read_codes(reads['base'][b:e], k, center)
            minus = reads['strand'][i] == '-'
            pos = reads['start'][i] + (n - 1 - np.arange(n) if minus else np.arange(n))
            assert codes.tolist() == [at[(reads['chrom'][i], reads['strand'][i], int(p))] for p in pos], (k, center, i)
            seen_minus += int(minus); seen_bad += int((codes < 0).sum())
        assert seen_minus == 6 and seen_bad >= 12 * k and (gcode >= 0).any()


@pytest.mark.parametrize('k,center,dtype,weighted,clip_rounds', R.PARITY_CASES)
def test_conditioning_pin_and_input_conditions(k, center, dtype, weighted, clip_rounds):
    """On the parity inputs the restated fit agrees with the exact-rational one to 1e-13 (scale relative, shift absolute), far inside the
    GPU gates of 1e-11 / 1e-12; no event lies within 1e-8 of a clip boundary in any round; at most 1e-4 of the int16 events have
    1000 x' within 1e-6 of a half-integer.  (A seed that violated either condition would be replaced, not the condition.)"""
    p = R.parity_inputs(k, center, dtype)
    exp = R.parity_expected(k, center, dtype, weighted, clip_rounds)
    assert exp['clip_margin'] > 1e-8 and (clip_rounds == 0) == (exp['clip_margin'] == np.inf)
    fitted = 0
    for i in np.flatnonzero((exp['status'] & (R.TOO_FEW | R.DEGENERATE | R.OUT_OF_RANGE)) == 0):
        b, e = p['off'][i], p['off'][i + 1]
        x = R.to_double(p['val'][b:e])
        f = R.fit_read(x, R.read_codes(p['base'][b:e], k, center), p['mean'], p['sd'], weighted, 3.0, clip_rounds, R.PARITY_MIN_EVENTS)
        assert f['status'] == 0 and f['scale'] == exp['scale'][i] and f['shift'] == exp['shift'][i]
        K = f['kept']
        a, s = R.exact_fit(x[K], f['mu'][K], f['w'][K])
        assert abs(f['scale'] / float(s) - 1.0) <= 1e-13 and abs(f['shift'] - float(a)) <= 1e-13, (i, f['scale'], float(s), f['shift'], float(a))
        fitted += 1
    assert fitted >= 10
    if dtype == 'int16':
        t = exp['t1000'][np.isfinite(exp['t1000'])]
        assert len(t) > 80000 and (np.abs(t - np.floor(t) - 0.5) <= 1e-6).mean() <= 1e-4


def _recovery_reads(contaminate, n_reads=40, n=2000, seed=99):
    k, center = 5, 2
    mean, sd = R.make_model(k, holes=False)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_reads):
        a, b = rng.uniform(-0.3, 0.3), rng.uniform(0.8, 1.25)
        base, x = R.draw_read(rng, n, k, center, mean, sd, a, b, contaminate=contaminate)
        out.append((a, b, x, R.read_codes(base, k, center)))
    return mean, sd, out


def test_recovery_from_clean_reads():
    """events drawn from the model at a planted (a, b): the plain weighted fit returns both within 6 standard errors, the standard
    errors being those of weighted least squares with noise b sigma_j: var(b^) = b^2 / Smm, var(a^) = b^2 (1 / W + mb^2 / Smm)"""
    mean, sd, reads = _recovery_reads(False)
    for a, b, x, codes in reads:
        f = R.fit_read(x, codes, mean, sd, True, 3.0, 0, 50)
        assert f['status'] == 0 and f['n_used'] == int((codes >= 0).sum())
        K = f['kept']
        mu, w = f['mu'][K], f['w'][K]
        W = w.sum()
        mb = (w * mu).sum() / W
        smm = (w * (mu - mb) ** 2).sum()
        se_b, se_a = b / np.sqrt(smm), b * np.sqrt(1.0 / W + mb * mb / smm)
        assert abs(f['scale'] - b) <= 6.0 * se_b and abs(f['shift'] - a) <= 6.0 * se_a, (a, b, f['shift'], f['scale'], se_a, se_b)


def test_clipping_halves_the_shift_error_of_contaminated_reads():
    """5 % of the events + 1 unit and 1 % uniform over +-5: summed over the seeded reads, the shift error with clipping (3.0, two rounds)
    is at most half of the unclipped one"""
    mean, sd, reads = _recovery_reads(True)
    err = {0: 0.0, 2: 0.0}
    for a, b, x, codes in reads:
        for rounds in err:
            f = R.fit_read(x, codes, mean, sd, True, 3.0, rounds, 50)
            assert f['status'] == 0
            err[rounds] += abs(f['shift'] - a)
    assert err[2] <= 0.5 * err[0], err


def test_cli_parser_and_checks():
    from nanomod_amd import cli
    p = cli.build_parser()
    a = p.parse_args(['rescale', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz', '--outReads', 'o.npz'])
    assert (a.cmd, a.wrkBase1, a.kmerModel, a.outReads, a.unweighted, a.clipSigma, a.clipRounds, a.minEvents, a.scaleLo, a.scaleHi, a.minPositions,
            a.dropFailed, a.outFolder, a.FileID, a.device) == ('rescale', 'r.npz', 'm.npz', 'o.npz', False, 3.0, 2, 50, 0.5, 2.0, 1, False, 'mRes', 'mod', 0)
    a = p.parse_args(['rescale', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz', '--outReads', 'o.npz', '--unweighted', '--clipSigma', '2.5',
                      '--clipRounds', '1', '--minEvents', '80', '--scaleLo', '0.7', '--scaleHi', '1.5', '--minPositions', '3', '--dropFailed',
                      '--outFolder', 'd', '--FileID', 'id', '--device', '1'])
    assert (a.unweighted, a.clipSigma, a.clipRounds, a.minEvents, a.scaleLo, a.scaleHi, a.minPositions, a.dropFailed, a.outFolder, a.FileID, a.device) == \
        (True, 2.5, 1, 80, 0.7, 1.5, 3, True, 'd', 'id', 1)
    for argv in (['rescale'], ['rescale', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz'], ['rescale', '--wrkBase1', 'r.npz', '--outReads', 'o.npz'],
                 ['rescale', '--kmerModel', 'm.npz', '--outReads', 'o.npz']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert p.parse_args(['kmerprofile', '--kmerModel', 'm.npz', '--wrkBase1', 's.npz', '--device', '2']).device == 2
    assert cli.main(['rescale', '--wrkBase1', '/nonexistent/r.npz', '--kmerModel', '/nonexistent/m.npz', '--outReads', 'o.npz']) == 1
    with tempfile.TemporaryDirectory() as tmp:
        reads, group, other = (os.path.join(tmp, n) for n in ('r.npz', 'g.npz', 'm.npz'))
        from nanomod_amd import container
        container.save_reads(reads, ['c'], ['+'], [0], [0, 2], np.array([0.5, 0.25]), np.array([b'A', b'C']))
        container.save_group(group, ['c'], ['+'], [0], ['A'], [0, 1], np.zeros(1, np.float32))
        np.savez(other, x=np.zeros(1))
        base = ['rescale', '--kmerModel', other, '--outReads', os.path.join(tmp, 'o.npz')]
        assert cli.main(base + ['--wrkBase1', group]) == 1                      # a per-position container has no reads
        for bad in (['--clipRounds', '9'], ['--clipSigma', '0'], ['--minEvents', '1'], ['--scaleLo', '0'], ['--scaleLo', '3'], ['--minPositions', '0']):
            assert cli.main(base + ['--wrkBase1', reads] + bad) == 1
        assert container.is_read_level(reads) and not container.is_read_level(group)


def test_masked_model_selection_and_table_writer():
    mean, sd = R.make_model(3, holes=False)
    model = dict(k=np.int32(3), center=np.int32(1), mean=mean, sd=sd, n_positions=np.arange(64) % 4)
    m = RS.masked_model(model, 2)
    thin = np.arange(64) % 4 < 2
    assert (m['k'], m['center']) == (3, 1) and np.isnan(m['mean'][thin]).all() and np.isnan(m['sd'][thin]).all()
    assert np.array_equal(m['mean'][~thin], mean[~thin]) and np.array_equal(m['sd'][~thin], sd[~thin]) and np.isfinite(mean).all()
    reads = dict(chrom=np.array(['chr1', 'chr2', 'chr2']), strand=np.array(['+', '-', '+']), start=np.array([5, 70, 9], np.int64),
                 off=np.array([0, 2, 3, 6], np.int64), norm_mean=np.arange(6, dtype=np.int16), base=np.array(list('ACGTAC'), 'S1'))
    kept = RS.select_reads(reads, np.array([True, False, True]))
    assert kept['off'].tolist() == [0, 2, 5] and kept['norm_mean'].tolist() == [0, 1, 3, 4, 5] and kept['base'].tolist() == [b'A', b'C', b'T', b'A', b'C']
    assert kept['chrom'].tolist() == ['chr1', 'chr2'] and kept['start'].tolist() == [5, 9] and kept['strand'].tolist() == ['+', '+']
    table = dict(index=np.arange(3), chrom=reads['chrom'], strand=reads['strand'], start=reads['start'], events=np.array([2, 1, 3]),
                 n_used=np.array([2, 0, 3], np.int32), shift=np.array([0.1234567, 0.0, -1.5]), scale=np.array([1.0000004, 1.0, 0.75]),
                 status=np.array([0, 1, 8], np.uint8))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 't.txt')
        for src in (reads, kept, None):                                         # dropped reads: the table's own columns
            RS.write_read_scale(path, src, table)
            assert open(path).read() == ('0 chr1 + 5 2 2 0.123457 1.000000 0\n1 chr2 - 70 1 0 0.000000 1.000000 1\n'
                                         '2 chr2 + 9 3 3 -1.500000 0.750000 8\n')
