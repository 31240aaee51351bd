"""The read-level input of `detect` on the host: the container, the vectorised per-read filters, the folder walk, and the
argument checks of the device entry points (no GPU needed)."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import helpers as H


def _quiet(*a):
    pass


def _reads(rng, n=300, milli=True):
    lens = rng.integers(0, 900, n)
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum(lens)
    k = rng.integers(-32767, 32768, off[-1])
    v = k / 1000.0 if milli else rng.normal(0, 1, off[-1])
    return dict(chrom=rng.choice(np.array(['chr1', 'chr2']), n), strand=rng.choice(np.array(['+', '-']), n),
                start=rng.integers(0, 17000, n).astype(np.int64), off=off, norm_mean=v,
                base=rng.choice(np.array(list(b'ACGT'), np.uint8), off[-1]).view('S1'))


def test_save_and_load_reads_round_trip_with_the_int16_choice():
    from nanomod_amd import container
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as tmp:
        for milli, want in ((True, np.int16), (False, np.float64)):
            r = _reads(rng, milli=milli)
            path = os.path.join(tmp, 'r.npz')
            container.save_reads(path, r['chrom'], r['strand'], r['start'], r['off'], r['norm_mean'], r['base'])
            assert container.is_read_level(path)
            g = container.load_reads(path)
            assert g['norm_mean'].dtype == want
            v = g['norm_mean'].astype(np.float64) / 1000.0 if want == np.int16 else g['norm_mean']
            assert np.array_equal(v, r['norm_mean'])
            for k in ('chrom', 'strand', 'start', 'off', 'base'):
                assert np.array_equal(g[k], r[k]), k
            with np.load(path) as z:                               # uncompressed
                assert all(z.zip.getinfo(n).compress_type == 0 for n in z.zip.namelist())
        # per-position containers are not read-level ones, and inconsistent files are refused
        pp = os.path.join(tmp, 'p.npz')
        container.save_group(pp, ['c'], ['+'], [3], ['A'], [0, 1], [0.5])
        assert not container.is_read_level(pp)
        bad = dict(r)
        bad['off'] = r['off'].copy(); bad['off'][-1] += 1
        np.savez(os.path.join(tmp, 'bad.npz'), **bad)
        with pytest.raises(ValueError):
            container.load_reads(os.path.join(tmp, 'bad.npz'))
        bad = dict(r); bad['strand'] = np.full(len(r['start']), '*')
        np.savez(os.path.join(tmp, 'bad2.npz'), **bad)
        with pytest.raises(ValueError):
            container.load_reads(os.path.join(tmp, 'bad2.npz'))


def test_vectorised_filters_equal_read_passes_filters():
    from nanomod_amd import fast5_ingest as F
    rng = np.random.default_rng(2)
    n = 4000
    start = np.concatenate([rng.integers(0, 17000, n // 2), rng.choice([0, 5, 7990, 8003, 15995, 16010], n // 2)]).astype(np.int64)
    lens = np.concatenate([rng.integers(0, 2000, n // 2), rng.choice([490, 495, 500, 505, 510, 7995, 8000, 8010], n // 2)]).astype(np.int64)
    chrom = rng.choice(np.array(['chr1', 'chr2']), n)
    names = ['r%d' % i for i in range(n)]
    z = np.load(os.path.join(H.GOLDEN, 'fast5_reads.npz'))
    fx = (np.diff(z['off']), z['chrom'], z['start'], ['f%d' % i for i in range(len(z['start']))])
    for opts in ({}, {'min_lr': 500}, {'min_lr': 500, 'min_lr_nb': 20}, {'min_lr': 8000, 'min_lr_nb': 30},
                 {'min_lr': 100, 'Chr': 'chr1', 'Pos': 3000, 'Pos2': 9000},
                 {'min_lr': 100, 'Chr': 'chr2', 'Pos': 4000, 'start_pos': 3990, 'end_pos': 4010}):
        for nn, cc, ss, nm in ((lens, chrom, start, names), fx):
            got_log, exp_log = [], []
            got = F.filter_reads(nn, cc, ss, opts, lambda *a: got_log.append(a), nm)
            exp = np.array([F.read_passes_filters(int(nn[i]), str(cc[i]), int(ss[i]), '+', opts, lambda *a: exp_log.append(a), nm[i])
                            for i in range(len(nn))])
            assert np.array_equal(got, exp), opts
            assert got_log == exp_log


def test_ingest_folder_reads_gives_the_fixture_reads_in_walk_order():
    from nanomod_amd import fast5_ingest as F
    z = np.load(os.path.join(H.GOLDEN, 'fast5_reads.npz'))
    with tempfile.TemporaryDirectory() as tmp:
        for g in (0, 1):
            d = H.write_placeholder_reads(tmp, g)
            r = F.ingest_folder_reads(d, None, H.placeholder_reader, log=_quiet)
            rel = [os.path.relpath(p, d) for p in r['name']]
            walked = []                                   # the walk of ingest_folder, independently
            level = [d]
            while level:
                nxt = []
                for cur in level:
                    for name in os.listdir(cur):
                        path = cur + '/' + name
                        if name.endswith('.fast5') and os.path.isfile(path) and H.placeholder_reader(path) is not None:
                            walked.append(os.path.relpath(path, d))
                        elif os.path.isdir(path) and name != 'mall':
                            nxt.append(path)
                level = nxt
            assert rel == walked and len(rel) > 20
            for j, name in enumerate(rel):
                i = int(np.flatnonzero((z['group'] == g) & (z['rel'] == name))[0])
                a, b = z['off'][i], z['off'][i + 1]
                assert (r['chrom'][j], r['strand'][j], r['start'][j]) == (z['chrom'][i], z['strand'][i], z['start'][i])
                assert np.array_equal(r['norm_mean'][r['off'][j]:r['off'][j + 1]], z['norm_mean'][a:b])
                assert np.array_equal(r['base'][r['off'][j]:r['off'][j + 1]].astype('U1'), z['base'][a:b])
            # with the command line's filters: the same reads GroupBuilder keeps, same log lines
            la, lb = [], []
            rf = F.ingest_folder_reads(d, {'min_lr': 500}, H.placeholder_reader, log=lambda *a: la.append(a))
            F.ingest_folder(d, {'min_lr': 500}, H.placeholder_reader, log=lambda *a: lb.append(a))
            assert la == lb and len(rf['start']) < len(r['start'])


def test_read_pivot_entry_points_reject_bad_arguments_without_a_gpu():
    import nanomod_amd._lib as L
    lib = L.load()
    n64 = C.c_int64(0); n64b = C.c_int64(0); n64c = C.c_int64(0); d32 = C.c_int32(0)
    host = L.make_params(memspace=L.MEM_HOST)
    assert lib.nmod_pivot_reads(C.byref(host), 0, 0, None, None, None, None, None, -1, -1, 0, None, None, None, None,
                                C.byref(n64), C.byref(n64b)) == -1
    bad_dtype = L.make_params(memspace=L.MEM_DEVICE, dtype=7)
    assert lib.nmod_pivot_reads(C.byref(bad_dtype), 0, 0, None, None, None, None, None, -1, -1, 0, None, None, None, None,
                                C.byref(n64), C.byref(n64b)) == -1
    assert lib.nmod_select_tested(C.byref(host), 5, 0, None, None, None, 0, 0, None, None, None, 0, 0, None, None, None, None,
                                  C.byref(n64), C.byref(n64b), C.byref(n64c), C.byref(d32)) == -1
    assert lib.nmod_gather_tested(C.byref(host), 0, *([None] * 9), 0, *([None] * 8)) == -1
    assert lib.nmod_pivot_reads(None, 0, 0, None, None, None, None, None, -1, -1, 0, None, None, None, None,
                                C.byref(n64), C.byref(n64b)) == -1
