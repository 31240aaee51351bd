"""nmod_kmer_model (K10) without a GPU: the declaration, the argument checks (before any device work), kmer_codes against the
string restatement, the model container, the model profile and the command line."""
import ctypes as C
import itertools
import os
import re
import tempfile

import numpy as np
import pytest

import kmer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine


def _lib():
    import nanomod_amd._lib as L
    return L, L.load()


def test_kmer_model_is_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, 'include', 'nanomod_hip.h')).read()
    assert 'nmod_kmer_model' in set(re.findall(r'\b(nmod_[a-z_]+)\s*\(', header))
    assert 'nmod_kmer_model' in L._SIGNATURES and hasattr(lib, 'nmod_kmer_model')
    assert '#define NMOD_MAX_KMER_CODES 65536' in header and L.MAX_KMER_CODES == 65536 == R.MAX_KMER_CODES == 4 ** 8
    assert '#define NMOD_STATUS_NO_CODE 64' in header and L.STATUS_NO_CODE == 64 == R.NO_CODE
    assert (L.STATUS_EMPTY, L.STATUS_TOO_LARGE, L.STATUS_NONFINITE, L.MAX_DEEP) == (R.EMPTY, R.TOO_LARGE, R.NONFINITE, R.MAX_DEEP)
    assert C.sizeof(L.NmodKmerOut) == 56 and L.NmodKmerOut.n_positions.offset == 8 and L.NmodKmerOut.pos_status.offset == 48
    assert [n for n, _ in L.NmodKmerOut._fields_][2:] == ['n_positions', 'n_samples', 'n_clipped', 'mean', 'sd', 'pos_status']
    assert '#define NMOD_ABI_VERSION 4' in header and lib.nmod_abi_version() == 4 == L.NMOD_ABI_VERSION      # a purely additive entry


def _call(lib, L, npos=4, *, sig='x', off='x', code='x', ncodes=16, lo=None, hi=None, out='x', dtype=None, stride=0, memspace=None,
          prm=None, struct_size=None, res=None):
    n = max(npos, 1) if 0 <= npos < 1000 else 4
    x = np.zeros(n * 8, np.int16)
    offs = np.arange(n + 1, dtype=np.int64) * 8
    codes = np.arange(n, dtype=np.int32) % 4
    m = ncodes if 1 <= ncodes <= 65536 else 1
    res = res if res is not None else {k: np.zeros(m, np.int64) for k in L.KMER_COUNT_FIELDS}
    res.setdefault('mean', np.zeros(m)); res.setdefault('sd', np.zeros(m)); res.setdefault('pos_status', np.zeros(n, np.uint8))
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    o = L.make_kmer_out(**{k: a.ctypes.data for k, a in res.items()})
    if struct_size is not None:
        o.struct_size = struct_size
    if prm is None:
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace,
                            dtype=L.DTYPE_I16_MILLI if dtype is None else dtype, stride0=stride)
    return lib.nmod_kmer_model(C.byref(prm), npos, pick(sig, x), pick(off, offs), pick(code, codes), ncodes, pick(lo, None), pick(hi, None),
                               C.byref(o) if out is not None else None)


def test_invalid_arguments_are_refused_before_any_device_work():
    """every case of the header returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone is NMOD_ERR_NO_DEVICE)"""
    L, lib = _lib()
    assert _call(lib, L) == -5                                                  # the well-formed call reaches the device check
    assert _call(lib, L, memspace=L.MEM_DEVICE) == -5
    assert _call(lib, L, off=None, stride=8) == -5
    assert _call(lib, L, dtype=L.DTYPE_F32) == -5 and _call(lib, L, dtype=L.DTYPE_F64) == -5
    bounds = np.zeros(16)
    assert _call(lib, L, lo=bounds, hi=bounds) == -5
    assert _call(lib, L, ncodes=1, code=np.zeros(4, np.int32)) == -5 and _call(lib, L, ncodes=65536) == -5
    assert _call(lib, L, code=np.array([-1, 15, 0, -1], np.int32)) == -5
    assert _call(lib, L, -1) == -1 and _call(lib, L, 2 ** 31 - 1) == -1 and _call(lib, L, 2 ** 40) == -1
    assert _call(lib, L, ncodes=0) == -1 and _call(lib, L, ncodes=65537) == -1 and _call(lib, L, ncodes=-4) == -1
    assert _call(lib, L, out=None) == -1 and _call(lib, L, struct_size=48) == -1 and _call(lib, L, struct_size=64) == -1
    assert _call(lib, L, sig=None) == -1 and _call(lib, L, code=None) == -1
    assert _call(lib, L, off=None) == -1                                        # neither offsets nor a stride
    assert _call(lib, L, dtype=3) == -1 and _call(lib, L, dtype=-1) == -1
    assert _call(lib, L, lo=bounds) == -1 and _call(lib, L, hi=bounds) == -1    # exactly one of the bounds
    assert _call(lib, L, off=np.array([0, 8, 4, 12, 16], np.int64)) == -1       # host offsets that decrease
    assert _call(lib, L, off=np.array([-1, 8, 9, 12, 16], np.int64)) == -1
    assert _call(lib, L, code=np.array([0, 16, 0, 0], np.int32)) == -1          # host memory: a code outside [-1, ncodes)
    assert _call(lib, L, code=np.array([0, -2, 0, 0], np.int32)) == -1
    assert _call(lib, L, code=np.array([0, 16, 0, 0], np.int32), memspace=L.MEM_DEVICE) == -5     # (device memory: NO_CODE per position)
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert _call(lib, L, prm=bad) == -1
    assert lib.nmod_kmer_model(None, 4, None, None, None, 16, None, None, None) == -1


def test_no_positions_is_ok_with_zero_counts_and_nan_levels():
    L, lib = _lib()
    res = {k: np.full(16, 7, np.int64) for k in L.KMER_COUNT_FIELDS}
    res['mean'] = np.zeros(16); res['sd'] = np.zeros(16)
    assert _call(lib, L, 0, res=res) == 0
    assert all(not res[k].any() for k in L.KMER_COUNT_FIELDS) and np.isnan(res['mean']).all() and np.isnan(res['sd']).all()
    assert _call(lib, L, 0, sig=None, off=None, code=None) == 0
    only = {'mean': np.zeros(16)}                                               # NULL members are skipped
    o = L.make_kmer_out(mean=only['mean'].ctypes.data)
    prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST, dtype=L.DTYPE_F32)
    assert lib.nmod_kmer_model(C.byref(prm), 0, None, None, None, 16, None, None, C.byref(o)) == 0 and np.isnan(only['mean']).all()


def test_python_layers_report_the_missing_device_and_bad_shapes():
    import nanomod_amd
    from nanomod_amd import engine
    x, off, code = np.zeros(8, np.int16), np.array([0, 4, 8], np.int64), np.zeros(2, np.int32)
    with pytest.raises(nanomod_amd._lib.NanomodLibraryError, match='nmod_kmer_model'):
        engine.kmer_model_host(x, off, code, 4, device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.kmer_model_host(x.astype(np.int32), off, code, 4, device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.kmer_model_host(x, np.array([0, 4, 9], np.int64), code, 4, device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.kmer_model_host(x, off, code, 4, np.zeros(4), None, device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.kmer_model_host(x, off, code, 4, np.zeros(3), np.zeros(3), device=NO_SUCH_DEVICE)
    res = engine.kmer_model_host(x[:0], np.zeros(1, np.int64), code[:0], 4, device=NO_SUCH_DEVICE)      # no positions: no device needed
    assert not res['n_samples'].any() and np.isnan(res['sd']).all() and res['pos_status'].shape == (0,)
    assert nanomod_amd.kmer_model_host is engine.kmer_model_host and nanomod_amd.build_kmer_model is nanomod_amd.kmermodel.build_kmer_model


def _positions(rng):
    """two chromosomes x both strands in the reference's order, with gaps (run edges), an 'N' and a lower-case letter"""
    rows = []
    for chrom in ('chr1', 'chr2'):
        for strand in '+-':
            ps = [p for p in range(10, 70) if p not in (23, 24, 41)] + [200, 201, 202]
            rows += [(chrom, strand, p) for p in ps]
    base = rng.choice(list('ACGT'), len(rows))
    base[7] = 'N'
    base[len(rows) // 2 + 5] = 'a'
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=np.int64), base)


@pytest.mark.parametrize('k', [1, 3, 5, 8])
def test_kmer_codes_against_the_string_restatement(k):
    from nanomod_amd import kmermodel
    chrom, strand, pos, base = _positions(np.random.default_rng(40 + k))
    for center in range(k):
        got = kmermodel.kmer_codes(chrom, strand, pos, base, k, center)
        exp = R.kmer_codes(chrom, strand, pos, base, k, center)
        assert got.dtype == np.int32 and np.array_equal(got, exp), (k, center)
        assert (got >= 0).any() and (got < 4 ** k).all() and ((got < 0).any() or k == 1)
        if k == 1:                                                              # only the two odd letters have no 1-mer
            assert int((got < 0).sum()) == 2
    for k_, c_ in ((0, 0), (9, 0), (3, 3), (3, -1)):
        with pytest.raises(ValueError):
            kmermodel.kmer_codes(chrom, strand, pos, base, k_, c_)
    assert kmermodel.kmer_codes(chrom[:0], strand[:0], pos[:0], base[:0], 3, 1).shape == (0,)


def test_minus_strand_reads_towards_lower_positions():
    """a '-' read's first event lies at its highest position and `base` is the read's own base: the 3-mer of position 11 with
    center 0 is the bases at 11, 10, 9, with center 2 those at 13, 12, 11"""
    from nanomod_amd import kmermodel
    pos = np.array([9, 10, 11, 12, 13], dtype=np.int64)
    base = np.array(list('ACGTA'))                                              # at 9 .. 13
    chrom, minus, plus = np.array(['c'] * 5), np.array(['-'] * 5), np.array(['+'] * 5)
    code = lambda word: sum('ACGT'.index(ch) * 4 ** (2 - i) for i, ch in enumerate(word))
    assert kmermodel.kmer_codes(chrom, minus, pos, base, 3, 0).tolist() == [-1, -1, code('GCA'), code('TGC'), code('ATG')]
    assert kmermodel.kmer_codes(chrom, minus, pos, base, 3, 2).tolist() == [code('GCA'), code('TGC'), code('ATG'), -1, -1]
    assert kmermodel.kmer_codes(chrom, plus, pos, base, 3, 0).tolist() == [code('ACG'), code('CGT'), code('GTA'), -1, -1]
    assert kmermodel.kmer_codes(chrom, plus, pos, base, 3, 2).tolist() == [-1, -1, code('ACG'), code('CGT'), code('GTA')]
    assert kmermodel.kmer_string(code('GCA'), 3) == 'GCA' == R.kmer_string(code('GCA'), 3)


def _model(rng, k=3, center=1):
    m = 4 ** k
    npos = rng.integers(0, 9, m)
    return dict(version=np.int32(1), k=np.int32(k), center=np.int32(center), clip_sigma=np.float64(0.0), n_positions=npos.astype(np.int64),
                n_samples=(npos * 20).astype(np.int64), n_clipped=np.zeros(m, np.int64),
                mean=np.where(npos > 0, rng.normal(size=m), np.nan), sd=np.where(npos > 0, rng.uniform(0.1, 0.4, m), np.nan))


def test_model_round_trip_and_table():
    from nanomod_amd import kmermodel
    model = _model(np.random.default_rng(3))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'm.npz')
        kmermodel.save_kmer_model(path, model)
        back = kmermodel.load_kmer_model(path)
        assert set(back) == set(kmermodel.KMER_MODEL_FIELDS) == set(model)
        assert all(np.array_equal(back[f], model[f], equal_nan=True) for f in model) and back['mean'].dtype == np.float64
        assert back['n_samples'].dtype == np.int64 and int(back['k']) == 3 and int(back['center']) == 1
        kmermodel.save_kmer_model(path, dict(model, version=np.int32(2)))
        with pytest.raises(ValueError, match='version'):
            kmermodel.load_kmer_model(path)
        kmermodel.save_kmer_model(path, dict(model, mean=model['mean'][:5]))
        with pytest.raises(ValueError):
            kmermodel.load_kmer_model(path)
        txt = os.path.join(tmp, 'm.txt')
        kmermodel.write_kmer_table(txt, model)
        lines = open(txt).read().splitlines()
        assert len(lines) == 64 and [ln.split()[0] for ln in lines] == [''.join(w) for w in itertools.product('ACGT', repeat=3)]
        for c in (0, 17, 63):
            assert lines[c] == '%s %d %d %.6f %.6f' % (R.kmer_string(c, 3), model['n_positions'][c], model['n_samples'][c], model['mean'][c], model['sd'][c])


def test_model_profile_selects_rows_and_feeds_match_positions():
    from nanomod_amd import kmermodel, onesample
    rng = np.random.default_rng(11)
    chrom, strand, pos, base = _positions(rng)
    shuffle = rng.permutation(len(pos))                                         # a group need not be in the reference's order
    lens = rng.integers(5, 12, len(pos))
    rows = [np.rint(1000.0 * rng.normal(0.0, 0.2, n)) / 1000.0 for n in lens]
    off = np.zeros(len(pos) + 1, np.int64); off[1:] = np.cumsum(lens)
    g_sorted = dict(chrom=chrom, strand=strand, pos=pos, base=base, off=off, sig=np.concatenate(rows))
    model = _model(rng)
    model['sd'][5] = 0.0                                                        # an entry without spread predicts nothing
    codes = R.kmer_codes(chrom, strand, pos, base, 3, 1)
    assert np.array_equal(kmermodel.group_codes(g_sorted, 3, 1), codes)
    g = dict(chrom=chrom[shuffle], strand=strand[shuffle], pos=pos[shuffle], base=base[shuffle], off=None, sig=None)
    assert np.array_equal(kmermodel.group_codes(g, 3, 1), codes[shuffle])
    for min_positions in (1, 4):
        prof = kmermodel.model_profile(model, g, min_positions)
        c = np.where(codes >= 0, codes, 0)
        want = (codes >= 0) & (model['n_positions'][c] >= min_positions) & np.isfinite(model['sd'][c]) & (model['sd'][c] > 0)
        assert prof['kind'] == 'model' and 'n' not in prof and 0 < want.sum() < len(pos)
        keys = [(str(prof['chrom_names'][i]), str(s), int(p)) for i, s, p in zip(prof['chrom_id'], prof['strand'], prof['pos'])]
        assert keys == [(str(a), str(b), int(p)) for a, b, p in zip(chrom[want], strand[want], pos[want])]
        assert np.array_equal(prof['mean'], model['mean'][codes[want]]) and np.array_equal(prof['sd'], model['sd'][codes[want]])
        assert np.array_equal(prof['base'], base[want])
    prof = kmermodel.model_profile(model, g, 1)
    want = (codes >= 0) & (model['n_positions'][np.where(codes >= 0, codes, 0)] >= 1) & (np.where(codes >= 0, codes, 0) != 5)
    meta, sig, off_m, mu, sd, ref_n, rid = onesample.match_positions(g_sorted, prof, 5, lambda *a: None)
    assert ref_n is None and len(meta['pos']) == int(want.sum()) and np.array_equal(mu, model['mean'][codes[want]])
    with tempfile.TemporaryDirectory() as tmp:                                  # ... and the profile container takes it
        onesample.save_profile(os.path.join(tmp, 'p.npz'), prof)
        assert onesample.load_profile(os.path.join(tmp, 'p.npz'))['kind'] == 'model'


def test_cli_parsers():
    from nanomod_amd import cli
    p = cli.build_parser()
    a = p.parse_args(['kmermodel', '--wrkBase1', 'c.npz', '--kmer', '6', '--kmerCenter', '3', '--MinCoverage', '7', '--clipSigma', '3',
                      '--clipRounds', '1', '--outFolder', 'd', '--FileID', 'id', '--device', '1'])
    assert (a.cmd, a.wrkBase1, a.kmer, a.kmerCenter, a.MinCoverage, a.clipSigma, a.clipRounds, a.outFolder, a.FileID, a.device) == \
        ('kmermodel', 'c.npz', 6, 3, 7, 3.0, 1, 'd', 'id', 1)
    a = p.parse_args(['kmermodel', '--wrkBase1', 'c.npz'])
    assert (a.kmer, a.kmerCenter, a.MinCoverage, a.clipSigma, a.clipRounds, a.device) == (5, 2, 5, 0.0, 2, 0)
    a = p.parse_args(['kmerprofile', '--kmerModel', 'm.npz', '--wrkBase1', 's.npz', '--minPositions', '3', '--outFolder', 'o', '--FileID', 'f'])
    assert (a.cmd, a.kmerModel, a.wrkBase1, a.minPositions, a.outFolder, a.FileID) == ('kmerprofile', 'm.npz', 's.npz', 3, 'o', 'f')
    assert p.parse_args(['kmerprofile', '--kmerModel', 'm.npz', '--wrkBase1', 's.npz']).minPositions == 1
    for argv in (['kmermodel'], ['kmerprofile', '--wrkBase1', 's.npz'], ['kmerprofile', '--kmerModel', 'm.npz'],
                 ['kmermodel', '--wrkBase1', 'c.npz', '--refProfile', 'p.npz']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    # the existing sub-commands are as they were: detect1 still requires --refProfile
    for argv in (['detect1', '--wrkBase1', 'g.npz'], ['profile'], ['detect', '--wrkBase1', 'g.npz'],
                 ['detect1', '--wrkBase1', 'g', '--refProfile', 'p', '--wrkBase2', 'h'], ['detect1', '--wrkBase1', 'g', '--kmerModel', 'm']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert cli.main(['kmermodel', '--wrkBase1', '/nonexistent/c.npz']) == 1
    assert cli.main(['kmerprofile', '--kmerModel', '/nonexistent/m.npz', '--wrkBase1', '/nonexistent/s.npz']) == 1
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'c.npz')
        np.savez(path, x=np.zeros(1))
        assert cli.main(['kmermodel', '--wrkBase1', path, '--kmer', '9']) == 1 and cli.main(['kmermodel', '--wrkBase1', path, '--kmerCenter', '5']) == 1
