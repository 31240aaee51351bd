"""nmod_read_llr / nmod_site_llr (K13) without a GPU: the restatement pinned against mpmath, the conditions the shared inputs must meet
for the GPU gates, that the restated chain finds a planted base (and sees a window stated the wrong way round), the declarations and
struct layouts, the argument checks of every layer (before any device work), what reaches the library, the writers and the command
line."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import readllr_ref as F
import rescale_ref as R
from nanomod_amd import _lib as L, engine
from nanomod_amd import readllr as RL             # K13's module: without it nothing here can pass
from test_engine_marshal import rec               # noqa: F401  (the fixture: a stand-in library that records every call)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')
PROFILE = os.path.join(ROOT, 'profiles', 'read_llr.txt')
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine

SIZEOF_PARAMS = 88
SIZEOF_LLR_OPTS = 32         # 4 x i32 + 2 doubles
SIZEOF_LLR_OUT = 64          # 2 x i32 + 7 pointers
SIZEOF_SITE_LLR_OUT = 40     # 2 x i32 + 4 pointers


def test_restatement_is_pinned_against_mpmath():
    """llr at |z0| in {0, 1e-3, 1, 8, 40, 1e3} (both signs) x level gaps of {0, 0.5, 3} spreads x spread ratios {1, 0.5, 2} and p_mod at
    t in {-800, -745, -40, -1e-3, 0, 1e-3, 40, 800} against 50-digit mpmath: within 1e-13 relative, and exactly 0 (llr) or 0 / 1 (p_mod)
    where mpmath's value is or rounds there (asserted inside pin_agreement).  Measured: 2.6e-16 (llr) and 6.3e-17 (p_mod);
    profiles/read_llr.txt holds the line."""
    worst_l, worst_p = F.pin_agreement()
    print('restatement v mpmath: llr %.3g, p_mod %.3g' % (worst_l, worst_p))
    assert worst_l <= F.PIN_GATE and worst_p <= F.PIN_GATE, (worst_l, worst_p)
    assert len(F.pin_llr_cases()) == 2 * 11 * 9
    assert F.posterior(np.array([-800.0, 800.0, 40.0, 0.0])).tolist() == [0.0, 1.0, 1.0, 0.5]
    assert re.search(r'^restatement v mpmath: llr [0-9.e-]+, p_mod [0-9.e-]+$', open(PROFILE).read(), re.M)    # the recorded line


def test_restatement_by_hand():
    """a read of 7 events over a 1-mer pair, one code unusable in the modified table, one value not finite: the windows hold the eligible
    events only, are cut at the ends of the read, and look nb_lo back and nb_hi ahead"""
    mean0, sd0 = np.array([0.0, 0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0, 1.0])
    mean1, sd1 = np.array([1.0, 1.0, np.nan, 1.0]), np.array([1.0, 2.0, 1.0, 1.0])
    base = np.frombuffer(b'ACGNTAA', np.uint8)
    x = np.array([1.0, 2.0, -3.0, 0.5, np.inf, 2.0, 0.0])
    codes = R.read_codes(base, 1, 0)
    r = F.score_read(x, codes, mean0, sd0, mean1, sd1, 0, 0)
    assert r['elig'].tolist() == [True, True, False, False, False, True, True]
    # equal spreads: llr = x - 1/2 for a gap of one spread; sd1 = 2: log(1/2) + (4 - 1/4) / 2
    assert r['llr'][[0, 5, 6]].tolist() == [0.5, 1.5, -0.5] and r['llr'][1] == np.log(0.5) + 0.5 * ((2.0 - 0.5) * (2.0 + 0.5))
    assert r['llr_win'].tobytes() == r['llr'].tobytes() and np.isnan(r['llr'][[2, 3, 4]]).all()
    r = F.score_read(x, codes, mean0, sd0, mean1, sd1, 1, 5)
    l = r['llr']
    assert r['llr_win'][0] == (l[0] + l[1]) + l[5] and r['llr_win'][1] == ((l[0] + l[1]) + l[5]) + l[6]
    assert r['llr_win'][5] == l[5] + l[6] and r['llr_win'][6] == l[5] + l[6] and np.isnan(r['llr_win'][[2, 3, 4]]).all()
    r = F.score_read(x, codes, mean0, sd0, mean1, sd1, 5, 1)
    assert r['llr_win'][0] == l[0] + l[1] and r['llr_win'][6] == (l[1] + l[5]) + l[6] and r['llr_win'][5] == ((l[0] + l[1]) + l[5]) + l[6]
    assert F.kmer_window(5, 2) == (2, 2) and F.kmer_window(3, 0) == (2, 0) and F.kmer_window(6, 2) == (3, 2) and F.kmer_window(1, 0) == (0, 0)
    # a spread so small that |llr| leaves NMOD_LLR_MAX: ineligible, and so is nothing else
    r = F.score_read(np.array([0.5, 0.5]), np.array([0, 1]), [0.0, 0.0], [1e-200, 1.0], [0.0, 0.0], [1.0, 1.0], 1, 1)
    assert r['elig'].tolist() == [False, True] and r['llr_win'][1] == r['llr'][1] == 0.0
    s = F.site_llr(np.array([2.5, -2.5, 0.0, np.nan, np.inf, -np.inf, 3.0, 1.0, -1.0]), np.array([0, 3, 3, 6, 7, 9]), 2.5)
    assert s['n_valid'].tolist() == [3, 0, 0, 1, 2] and s['n_mod'].tolist() == [1, 0, 1, 1, 0] and s['n_can'].tolist() == [1, 0, 1, 0, 0]
    assert s['frac'][[0, 2, 3]].tolist() == [0.5, 0.5, 1.0] and np.isnan(s['frac'][[1, 4]]).all()


@pytest.mark.parametrize('k,center', F.PARITY_KC)
@pytest.mark.parametrize('window', F.PARITY_WINDOWS)
def test_shared_inputs_meet_the_conditions_of_the_gpu_gates(k, center, window):
    """thr_margin > 0: no window sum of the restatement lies within its gate of a threshold, so the device's counts are exact integers
    to compare; and the inputs reach every kind of event, both size classes and both calls"""
    lo, hi = F.window_of(window, k, center)
    for dtype in F.PARITY_DTYPES:
        for equal_sd in (False, True):
            p = F.parity_inputs(k, center, window, dtype, equal_sd)
            exp = F.parity_expected(k, center, window, dtype, equal_sd)
            lens = np.diff(p['off'])
            assert lens.tolist() == F.parity_lengths(k, lo, hi) and lens.max() == 70000 and (lens == F.WAVE_MAX + 1).any()
            assert exp['thr_margin'] > 0.0, (dtype, equal_sd, exp['thr_margin'])
            assert np.isnan(exp['llr_win']).sum() >= 4 and (exp['n_mod'] > 0).sum() >= 6 and (exp['n_can'] > 0).sum() >= 6
            assert (exp['n_sites'][lens >= 63] > 0).all() and not exp['status'].any()
            usable, g = F.code_table(p['mean'], p['sd'], p['alt_mean'], p['alt_sd'])
            assert usable.sum() >= 4 ** k - 7 and (not g.any()) == equal_sd     # equal spreads: g is an exact 0 for every usable code
            amb = exp['n_sites'].astype(np.int64) - exp['n_mod'] - exp['n_can']
            assert (amb >= 0).all() and (amb.sum() > 0 or lo + hi > 20)             # some events are left ambiguous (a sum of 129 hardly is)
            assert np.nanmax(exp['gate_L']) < 1e-3                                  # the gates stay far below the threshold


def test_other_shared_inputs_meet_the_conditions():
    for dtype in F.PARITY_DTYPES:
        p = F.ineligible_inputs(dtype)
        k, center = F.INELIGIBLE_KC
        exp = F.restate(p['val'], p['off'], p['base'], k, center, p['mean'], p['sd'], p['alt_mean'], p['alt_sd'], F.INELIGIBLE_WINDOW)
        assert exp['thr_margin'] > 0.0
        bad = (p['codes'] < 0) | np.isin(p['codes'], (3, 6, 9, 12, 5, 10, 15, F.TINY_SD_CODE)) | ~np.isfinite(R.to_double(p['val']))
        assert np.array_equal(np.isnan(exp['llr']), bad) and (p['codes'] == F.TINY_SD_CODE).sum() >= 20
        assert np.isin(p['codes'], (5, 10, 15)).sum() >= 20 and exp['n_sites'].tolist()[3:5] == [0, 0]
    reads, model, alt, planted = F.chain_inputs()
    assert F.restate_chain(reads, model, alt)[0]['thr_margin'] > 0.0


def test_restated_chain_finds_the_planted_base_and_sees_a_swapped_window():
    """Half of the reads of each strand are drawn from the modified table at the three events whose 3-mer covers the planted base.
    With the k-mer cover as the window, the restated frac there lies inside the binomial 99.9 % interval of 0.5 for its n_mod + n_can,
    and the base has the strand's largest n_mod and n_mod + n_can.  A base within k - 1 of it shares one or two of the shifted events,
    so its frac is near 0.5 too, from fewer confident reads: frac is the maximum over every base of the strand beyond that reach, where
    it stays below 0.1.  Stated the wrong way round — (center, k - 1 - center) — the window of the planted base holds one shifted event
    instead of three and n_mod + n_can drops there."""
    from scipy import stats
    reads, model, alt, planted = F.chain_inputs()
    k, center = model['k'], model['center']
    assert (k, center) == (3, 0) and F.kmer_window(k, center) == (2, 0)
    n = np.diff(reads['off'])
    assert len(n) == 200 and n.min() >= 300 and set(reads['strand']) == {'+', '-'}
    exp, rows, s = F.restate_chain(reads, model, alt)
    exp_sw, rows_sw, s_sw = F.restate_chain(reads, model, alt, (center, k - 1 - center))
    for strand in '+-':
        m = rows['strand'] == strand
        at = int(np.flatnonzero(m & (rows['pos'] == planted))[0])
        conf = int(s['n_mod'][at] + s['n_can'][at])
        assert np.diff(rows['off'])[at] == 100 and conf >= 90                  # every read of the strand covers it; nearly all are confident
        lo, hi = stats.binom.interval(0.999, conf, 0.5)
        print('strand %s: n_mod %d, n_can %d, frac %.4f; 99.9 %% interval of 0.5 at n = %d: [%.4f, %.4f]'
              % (strand, s['n_mod'][at], s['n_can'][at], s['frac'][at], conf, lo / conf, hi / conf))
        assert lo / conf <= s['frac'][at] <= hi / conf
        assert s['n_mod'][at] == s['n_mod'][m].max() and conf == (s['n_mod'] + s['n_can'])[m].max()
        far = m & (np.abs(rows['pos'] - planted) > k - 1)
        assert np.nanmax(s['frac'][far]) < 0.1 < s['frac'][at] and np.isfinite(s['frac'][far]).sum() > 50
        near = m & (np.abs(rows['pos'] - planted) <= k - 1)
        assert np.nanmax(s['frac'][m]) == np.nanmax(s['frac'][near])
        conf_sw = int(s_sw['n_mod'][at] + s_sw['n_can'][at])
        print('strand %s: the window the wrong way round: n_mod + n_can %d, down from %d' % (strand, conf_sw, conf))
        assert conf_sw < conf - 5


def test_entries_are_declared_and_exported():
    lib = L.load()
    header = open(HEADER).read()
    declared = set(re.findall(r'\b(nmod_[a-z_]+)\s*\(', header))
    for name in ('nmod_read_llr', 'nmod_site_llr'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name)
    assert '#define NMOD_LLR_MAX 1e300' in header and L.LLR_MAX == F.LLR_MAX == 1e300
    assert 'typedef struct nmod_llr_opts { int32_t struct_size, nb_lo, nb_hi, reserved; double thr, prior_logit; } nmod_llr_opts;' in header
    assert re.search(r'typedef struct nmod_llr_out \{ int32_t struct_size; int32_t reserved;\s+double \*llr, \*llr_win, \*p_mod;[^\n]*\n\s+'
                     r'int32_t \*n_sites, \*n_mod, \*n_can; uint8_t\* status;', header)
    assert ('typedef struct nmod_site_llr_out { int32_t struct_size; int32_t reserved; int32_t *n_valid, *n_mod, *n_can; double* frac; } '
            'nmod_site_llr_out;') in header
    assert L.LLR_EVENT_FIELDS == ('llr', 'llr_win', 'p_mod') and L.SITE_LLR_FIELDS == ('n_valid', 'n_mod', 'n_can', 'frac')
    assert '#define NMOD_ABI_VERSION 4' in header and lib.nmod_abi_version() == 4 == L.NMOD_ABI_VERSION      # purely additive entries
    assert 'd = 0.5 * ((z0 - z1) * (z0 + z1))' in header and 'g_c = log(sd0_c / sd1_c)' in header
    import nanomod_amd
    assert nanomod_amd.call_reads_llr is RL.call_reads_llr and nanomod_amd.read_llr_host is engine.read_llr_host
    assert nanomod_amd.site_llr_host is engine.site_llr_host and nanomod_amd.write_site_llr is RL.write_site_llr


def test_struct_layouts_match_the_header():
    """sizes and offsets of the three new structs from a gcc-compiled program over the header itself"""
    fields = [('nmod_llr_opts', L.NmodLlrOpts, ('struct_size', 'nb_lo', 'nb_hi', 'reserved', 'thr', 'prior_logit')),
              ('nmod_llr_out', L.NmodLlrOut, ('struct_size', 'reserved', 'llr', 'llr_win', 'p_mod', 'n_sites', 'n_mod', 'n_can', 'status')),
              ('nmod_site_llr_out', L.NmodSiteLlrOut, ('struct_size', 'reserved', 'n_valid', 'n_mod', 'n_can', 'frac'))]
    exprs, want = [], []
    for cname, cls, names in fields:
        exprs.append('sizeof(%s)' % cname); want.append(C.sizeof(cls))
        assert [n for n, _ in cls._fields_] == list(names)
        for n in names:
            exprs.append('offsetof(%s, %s)' % (cname, n)); want.append(getattr(cls, n).offset)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){size_t v[] = {%s};\nfor (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) ' \
          'printf("%%zu ", v[i]);\nreturn 0;}' % (HEADER, ', '.join(exprs))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        subprocess.check_call(['gcc', c, '-o', os.path.join(d, 't')])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).split()]
    assert got == want
    assert (C.sizeof(L.NmodLlrOpts), C.sizeof(L.NmodLlrOut), C.sizeof(L.NmodSiteLlrOut)) == (SIZEOF_LLR_OPTS, SIZEOF_LLR_OUT, SIZEOF_SITE_LLR_OUT)
    assert L.NmodLlrOpts.thr.offset == 16 and L.NmodLlrOut.llr.offset == 8 and L.NmodLlrOut.status.offset == 56 and L.NmodSiteLlrOut.frac.offset == 32


# ----------------------------------------------------------------------------------------------- the C entries' own refusals
def _call(lib, nreads=3, *, off='x', val='x', base='x', model='x', alt='x', k=3, center=1, alt_k=None, alt_center=None, mean='x', sd='x',
          alt_mean='x', alt_sd='x', opts='x', out='x', nb_lo=2, nb_hi=1, thr=2.5, prior_logit=0.0, dtype=None, memspace=None, prm=None,
          opts_size=None, out_size=None, llr='x'):
    n = nreads if 0 <= nreads < 1000 else 3
    offs = np.arange(n + 1, dtype=np.int64) * 60
    x, b = np.zeros(max(n, 1) * 60, np.int16), np.full(max(n, 1) * 60, ord('A'), np.uint8)
    mu, s = np.zeros(4 ** 8), np.ones(4 ** 8)
    ev = np.zeros(max(n, 1) * 60)
    cnt = np.zeros(max(n, 1), np.int32)
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    m0, m1 = L.NmodRescaleModel(), L.NmodRescaleModel()
    m0.k, m0.center, m0.mean, m0.sd = k, center, pick(mean, mu), pick(sd, s)
    m1.k, m1.center, m1.mean, m1.sd = k if alt_k is None else alt_k, center if alt_center is None else alt_center, pick(alt_mean, mu), pick(alt_sd, s)
    o = L.make_llr_opts(nb_lo, nb_hi, thr, prior_logit)
    if opts_size is not None:
        o.struct_size = opts_size
    r = L.make_llr_out(llr=pick(llr, ev), n_sites=cnt.ctypes.data)
    if out_size is not None:
        r.struct_size = out_size
    if prm is None:
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace,
                            dtype=L.DTYPE_I16_MILLI if dtype is None else dtype)
    return lib.nmod_read_llr(C.byref(prm), nreads, pick(off, offs), pick(val, x), pick(base, b), C.byref(m0) if model is not None else None,
                             C.byref(m1) if alt is not None else None, C.byref(o) if opts is not None else None,
                             C.byref(r) if out is not None else None)


def test_read_llr_refuses_invalid_arguments_before_any_device_work():
    """every case of the header returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone is NMOD_ERR_NO_DEVICE)"""
    lib = L.load()
    nan, inf = float('nan'), float('inf')
    call = lambda *a, **kw: _call(lib, *a, **kw)
    assert call() == -5                                                         # the well-formed call reaches the device check
    assert call(memspace=L.MEM_DEVICE) == -5 and call(dtype=L.DTYPE_F32) == -5 and call(dtype=L.DTYPE_F64) == -5
    assert call(nb_lo=0, nb_hi=0) == -5 and call(nb_lo=64, nb_hi=64) == -5 and call(nb_lo=0, nb_hi=64) == -5 and call(thr=1e-300) == -5
    assert call(prior_logit=700.0) == -5 and call(prior_logit=-700.0) == -5 and call(k=1, center=0) == -5 and call(k=8, center=7) == -5
    assert call(llr=None) == -5
    assert call(0) == 0 and call(0, off=None, val=None, base=None, mean=None, sd=None, alt_mean=None, alt_sd=None) == 0   # no reads: no device needed
    assert call(nb_lo=-1) == -1 and call(nb_lo=65) == -1 and call(nb_hi=-1) == -1 and call(nb_hi=65) == -1
    assert all(call(thr=v) == -1 for v in (0.0, -2.5, nan, inf, -inf))
    assert all(call(prior_logit=v) == -1 for v in (700.0000001, -701.0, nan, inf, -inf))
    assert call(k=0, center=0) == -1 and call(k=9) == -1 and call(center=3) == -1 and call(center=-1) == -1
    assert call(alt_k=4) == -1 and call(alt_center=0) == -1 and call(alt_center=2) == -1
    assert call(off=None) == -1 and call(val=None) == -1 and call(base=None) == -1
    assert call(model=None) == -1 and call(alt=None) == -1
    assert call(mean=None) == -1 and call(sd=None) == -1 and call(alt_mean=None) == -1 and call(alt_sd=None) == -1
    assert call(opts_size=24) == -1 and call(opts_size=40) == -1 and call(opts=None) == -1
    assert call(out_size=56) == -1 and call(out_size=72) == -1 and call(out=None) == -1
    assert call(dtype=3) == -1 and call(dtype=-1) == -1 and call(memspace=2) == -1
    assert call(-1) == -1 and call(2 ** 32 - 1) == -1 and call(2 ** 40) == -1
    assert call(off=np.array([0, 60, 40, 180], np.int64)) == -1                 # host offsets that decrease
    assert call(off=np.array([-1, 60, 120, 180], np.int64)) == -1
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert call(prm=bad) == -1
    assert lib.nmod_read_llr(None, 3, None, None, None, None, None, None, None) == -1


def _site(lib, npos=3, *, score='x', off='x', stride=0, thr=2.5, out='x', out_size=None, memspace=None, prm=None, dtype=7):
    n = npos if 0 <= npos < 1000 else 3
    offs = np.arange(n + 1, dtype=np.int64) * 5
    sc = np.zeros(max(n, 1) * 5)
    cnt, fr = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1))
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    r = L.make_site_llr_out(n_valid=cnt.ctypes.data, frac=fr.ctypes.data)
    if out_size is not None:
        r.struct_size = out_size
    if prm is None:                                                             # (dtype 7: this entry does not read it)
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace, dtype=dtype, stride0=stride)
    return lib.nmod_site_llr(C.byref(prm), npos, pick(score, sc), pick(off, offs), thr, C.byref(r) if out is not None else None)


def test_site_llr_refuses_invalid_arguments_before_any_device_work():
    lib = L.load()
    nan, inf = float('nan'), float('inf')
    site = lambda *a, **kw: _site(lib, *a, **kw)
    assert site() == -5 and site(off=None, stride=5) == -5 and site(memspace=L.MEM_DEVICE) == -5
    assert site(thr=1e300) == -5 and site(dtype=L.DTYPE_F32) == -5
    assert site(0) == 0 and site(0, score=None) == 0
    assert all(site(thr=v) == -1 for v in (0.0, -1.0, nan, inf, -inf))
    assert site(off=None) == -1 and site(off=None, stride=-5) == -1             # neither offsets nor a stride
    assert site(-1) == -1 and site(2 ** 31 - 1) == -1 and site(2 ** 40) == -1
    assert site(score=None) == -1 and site(out=None) == -1 and site(out_size=32) == -1 and site(memspace=2) == -1
    assert site(off=np.array([0, 5, 4, 15], np.int64)) == -1 and site(off=np.array([-1, 5, 10, 15], np.int64)) == -1
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert site(prm=bad) == -1
    assert lib.nmod_site_llr(None, 3, None, None, 2.5, None) == -1


# --------------------------------------------------------------------------------------------- the Python layers: refusals, marshalling
NREADS, READ_LEN = 3, 6


def _reads(first=0, dtype=np.float32, tail=2):
    off = first + np.arange(NREADS + 1, dtype=np.int64) * READ_LEN
    n = int(off[-1]) + tail
    val = np.random.default_rng(3).normal(size=n)
    val = (val * 1000).astype(np.int16) if dtype == np.int16 else val.astype(dtype)
    base = np.frombuffer(b'ACGT' * n, np.uint8)[:n].copy()
    return val, off, base


def _models(k=3, center=1):
    mean, sd = R.make_model(k, holes=False)
    return dict(k=k, center=center, mean=mean, sd=sd), dict(k=k, center=center, mean=mean + 0.5, sd=sd * 1.5)


def _refused_host():
    val, off, base = _reads()
    m0, m1 = _models()
    score, soff = np.zeros(20), np.arange(5, dtype=np.int64) * 5
    nan, inf = float('nan'), float('inf')
    rl, sl = engine.read_llr_host, engine.site_llr_host
    w = lambda **kw: (rl, (kw.pop('val', val), kw.pop('off', off), kw.pop('base', base), kw.pop('model', m0), kw.pop('alt', m1)), kw)
    cases = dict(
        lo_neg=w(window=(-1, 0)), lo_65=w(window=(65, 0)), hi_neg=w(window=(0, -1)), hi_65=w(window=(0, 65)), window_word=w(window='cover'),
        window_one=w(window=(2,)), window_none=w(window=None),
        thr_0=w(thr=0.0), thr_neg=w(thr=-2.5), thr_nan=w(thr=nan), thr_inf=w(thr=inf),
        prior_nan=w(prior_logit=nan), prior_inf=w(prior_logit=inf), prior_701=w(prior_logit=701.0), prior_neg=w(prior_logit=-700.5),
        k_0=w(model=dict(m0, k=0), alt=dict(m1, k=0)), k_9=w(model=dict(m0, k=9), alt=dict(m1, k=9)),
        center_3=w(model=dict(m0, center=3), alt=dict(m1, center=3)), center_neg=w(model=dict(m0, center=-1), alt=dict(m1, center=-1)),
        k_differs=w(alt=dict(_models(2, 1)[1])), center_differs=w(alt=dict(m1, center=0)),
        no_model=w(model=None), no_alt=w(alt=None), want=w(want=('p_win',)),
        dtype=w(val=val.astype(np.int32)), off_down=w(off=np.array([0, 12, 6, 18], np.int64)), off_neg=w(off=np.array([-1, 6, 12, 18], np.int64)),
        off_past=w(off=off + 4), off_empty=w(off=off[:0]), base_short=w(base=base[:int(off[-1]) - 1]),
        mean_len=w(model=dict(m0, mean=m0['mean'][:10])), alt_sd_len=w(alt=dict(m1, sd=np.ones(16))),
        site_thr_0=(sl, (score, soff), dict(thr=0.0)), site_thr_nan=(sl, (score, soff), dict(thr=nan)), site_thr_inf=(sl, (score, soff), dict(thr=inf)),
        site_no_rows=(sl, (score, None), {}), site_stride_0=(sl, (score, None), dict(stride=0)), site_ragged=(sl, (score, None), dict(stride=3)),
        site_short=(sl, (score[:-1], soff), {}), site_down=(sl, (score, np.array([0, 6, 4, 20], np.int64)), {}),
        site_2d=(sl, (score.reshape(4, 5), soff), {}), site_off_empty=(sl, (score, soff[:0]), {}))
    return [pytest.param(f, a, kw, id=name) for name, (f, a, kw) in cases.items()]


@pytest.mark.parametrize('fn,args,kw', _refused_host())
def test_refused_before_the_library(fn, args, kw):
    L.load()                                     # the real library: a call that reached it would be a NanomodLibraryError
    with pytest.raises(ValueError):
        fn(*args, device=NO_SUCH_DEVICE, **kw)


def test_accepted_calls_reach_the_library():
    val, off, base = _reads()
    m0, m1 = _models()
    with pytest.raises(L.NanomodLibraryError, match='nmod_read_llr'):
        engine.read_llr_host(val, off, base, m0, m1, device=NO_SUCH_DEVICE)
    with pytest.raises(L.NanomodLibraryError, match='nmod_site_llr'):
        engine.site_llr_host(np.zeros(10), np.array([0, 4, 10], np.int64), device=NO_SUCH_DEVICE)
    res = engine.read_llr_host(val[:0], np.zeros(1, np.int64), base[:0], m0, m1, want=('llr_win',), device=NO_SUCH_DEVICE)   # no reads: no device
    assert res['llr_win'].shape == (0,) and res['n_mod'].shape == (0,) and 'llr' not in res
    assert engine.site_llr_host(np.zeros(0), np.zeros(1, np.int64), device=NO_SUCH_DEVICE)['frac'].shape == (0,)


def _check_out(out, res, size):
    members = {k: v for k, v in out.items() if k not in ('struct_size', 'reserved')}
    assert out['struct_size'] == size and out['reserved'] == 0
    assert {k for k, v in members.items() if v is not None} == set(res)        # non-NULL exactly for what is returned
    for k, a in res.items():
        assert members[k] == a.ctypes.data and a.flags.c_contiguous, k


@pytest.mark.parametrize('first', [0, 2])
@pytest.mark.parametrize('want', [('llr_win',), ('llr', 'llr_win', 'p_mod'), ()])
def test_read_llr_host_marshalling(rec, want, first):
    val, off, base = _reads(first)
    m0, m1 = _models()
    res = engine.read_llr_host(val, off, base, m0, m1, window=(4, 1), thr=3.0, prior_logit=-0.25, want=want, device=1)
    prm, nreads, o, v, b, model, alt, opts, out = rec.only('nmod_read_llr')
    assert {f: prm[f] for f in ('struct_size', 'memspace', 'dtype', 'device', 'stride0')} == dict(struct_size=SIZEOF_PARAMS, memspace=0, dtype=0, device=1, stride0=0)
    assert prm['stream'] is None
    assert (nreads, o, v, b) == (NREADS, off.ctypes.data, val.ctypes.data, base.ctypes.data)
    assert model == dict(k=3, center=1, mean=m0['mean'].ctypes.data, sd=m0['sd'].ctypes.data)
    assert alt == dict(k=3, center=1, mean=m1['mean'].ctypes.data, sd=m1['sd'].ctypes.data)
    assert opts == dict(struct_size=SIZEOF_LLR_OPTS, nb_lo=4, nb_hi=1, reserved=0, thr=3.0, prior_logit=-0.25)
    assert set(res) == set(want) | {'n_sites', 'n_mod', 'n_can', 'status'}
    assert all(res[w].dtype == np.float64 and res[w].shape == val.shape and np.isnan(res[w]).all() for w in want)
    assert all(res[f].dtype == np.int32 and res[f].shape == (NREADS,) and not res[f].any() for f in ('n_sites', 'n_mod', 'n_can'))
    assert res['status'].dtype == np.uint8 and not res['status'].any()
    _check_out(out, res, SIZEOF_LLR_OUT)


def test_read_llr_host_defaults_are_the_kmer_cover(rec):
    val, off, base = _reads(dtype=np.int16)
    for (k, center), win in (((3, 1), (1, 1)), ((3, 0), (2, 0)), ((3, 2), (0, 2)), ((1, 0), (0, 0))):
        rec.calls.clear()
        m0, m1 = _models(k, center)
        engine.read_llr_host(val, off, base.view('S1'), m0, m1)
        prm, nreads, o, v, b, model, alt, opts, out = rec.only('nmod_read_llr')
        assert prm['dtype'] == 1 and b is not None and (model['k'], model['center'], alt['k'], alt['center']) == (k, center, k, center)
        assert opts == dict(struct_size=SIZEOF_LLR_OPTS, nb_lo=win[0], nb_hi=win[1], reserved=0, thr=2.5, prior_logit=0.0)


@pytest.mark.parametrize('layout', ['csr', 'stride'])
def test_site_llr_host_marshalling(rec, layout):
    score = np.random.default_rng(4).normal(size=40)
    off = np.arange(5, dtype=np.int64) * 10 if layout == 'csr' else None
    res = engine.site_llr_host(score, off, stride=10, thr=1.5, device=1)
    prm, npos, s, o, thr, out = rec.only('nmod_site_llr')
    assert {f: prm[f] for f in ('struct_size', 'memspace', 'dtype', 'device', 'stride0')} == \
        dict(struct_size=SIZEOF_PARAMS, memspace=0, dtype=2, device=1, stride0=0 if off is not None else 10)
    assert (npos, s, thr) == (4, score.ctypes.data, 1.5) and o == (off.ctypes.data if off is not None else None)
    assert set(res) == {'n_valid', 'n_mod', 'n_can', 'frac'} and np.isnan(res['frac']).all() and res['frac'].shape == (4,)
    assert all(res[f].dtype == np.int32 and res[f].shape == (4,) and not res[f].any() for f in ('n_valid', 'n_mod', 'n_can'))
    _check_out(out, res, SIZEOF_SITE_LLR_OUT)


def test_device_detector_checks_its_arguments_before_the_library(rec):
    """DeviceDetector.read_llr / site_llr on tensors that are not on a device: every refusal of the options comes first, as a ValueError,
    and a well-formed call is refused for its tensors — the library is never reached"""
    import torch
    det = engine.DeviceDetector(0)
    val, off, base = _reads()
    m0, m1 = _models()
    t = torch.from_numpy
    args = (t(val), t(off), t(base), t(m0['mean']), t(m0['sd']), t(m1['mean']), t(m1['sd']), 3, 1)
    nan, inf = float('nan'), float('inf')
    for kw, msg in ((dict(window=(65, 0)), 'window bounds'), (dict(window=(0, -1)), 'window bounds'), (dict(window='cover'), 'window must be'),
                    (dict(thr=0.0), 'thr'), (dict(thr=nan), 'thr'), (dict(thr=inf), 'thr'), (dict(prior_logit=701.0), 'prior_logit'),
                    (dict(prior_logit=nan), 'prior_logit'), (dict(want=('z',)), 'want'), ({}, 'CUDA')):
        with pytest.raises(ValueError, match=msg):
            det.read_llr(*args, **kw)
    for k, center in ((0, 0), (9, 1), (3, 3), (3, -1)):
        with pytest.raises(ValueError, match='k must be|center must be'):
            det.read_llr(*args[:7], k, center)
    with pytest.raises(ValueError, match='signals must be'):
        det.read_llr(t(val.astype(np.int32)), *args[1:])
    score = t(np.zeros(20))
    for kw, msg in ((dict(off=t(np.arange(5, dtype=np.int64) * 5), thr=0.0), 'thr'), (dict(stride=5, thr=nan), 'thr'), (dict(stride=5), 'CUDA')):
        with pytest.raises(ValueError, match=msg):
            det.site_llr(score, **kw)
    assert rec.calls == []


def test_call_reads_llr_refuses_before_any_device_work(rec):
    reads, model, alt, planted = F.chain_inputs(n_reads=4)
    call = lambda **kw: RL.call_reads_llr(kw.pop('reads', reads), kw.pop('model', model), kw.pop('alt', alt), device=NO_SUCH_DEVICE, log=None, **kw)
    for kw, msg in ((dict(alt=dict(alt, k=2, mean=alt['mean'][:16], sd=alt['sd'][:16], n_positions=alt['n_positions'][:16])), 'share k and center'),
                    (dict(alt=dict(alt, center=1)), 'share k and center'), (dict(prior=0.0), 'prior'), (dict(prior=1.0), 'prior'),
                    (dict(prior=float('nan')), 'prior'), (dict(thr=0.0), 'thr'), (dict(window=(0, 65)), 'window bounds'),
                    (dict(window='site'), 'window must be'), (dict(rescale=dict(drop_failed=True)), 'unknown option'),
                    (dict(reads=dict(reads, norm_mean=reads['norm_mean'].astype(np.int32))), 'norm_mean must be')):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    assert rec.calls == []


def test_writers():
    table = dict(index=np.arange(3), chrom=np.array(['chr1', 'chr2', 'chr2']), strand=np.array(['+', '-', '+']), start=np.array([5, 70, 9], np.int64),
                 events=np.array([200, 1, 300]), n_sites=np.array([198, 0, 297], np.int32), n_mod=np.array([4, 0, 31], np.int32),
                 n_can=np.array([150, 0, 2], np.int32), status=np.array([0, 0, 16], np.uint8))
    sites = dict(chrom=np.array(['chr1', 'chr1', 'chr2']), strand=np.array(['+', '-', '+']), pos=np.array([0, 41, 7], np.int64),
                 base=np.array(['A', 'c', 'N']), n_reads=np.array([4, 2, 1], np.int32), n_valid=np.array([4, 1, 1], np.int32),
                 n_mod=np.array([1, 0, 1], np.int32), n_can=np.array([2, 0, 0], np.int32), frac=np.array([1.0 / 3.0, np.nan, 1.0]))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 't.txt')
        RL.write_read_llr(path, table)
        assert open(path).read() == '0 chr1 + 5 200 198 4 150 0\n1 chr2 - 70 1 0 0 0 0\n2 chr2 + 9 300 297 31 2 16\n'
        RL.write_site_llr(path, sites)
        assert open(path).read() == 'chr1 + 1 A 4 4 1 2 0.333333\nchr1 - 42 c 2 1 0 0 nan\nchr2 + 8 N 1 1 1 0 1.000000\n'


def test_cli_parser_and_checks(capsys):
    from nanomod_amd import cli, container
    p = cli.build_parser()
    a = p.parse_args(['readllr', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz', '--altModel', 'a.npz'])
    assert (a.cmd, a.wrkBase1, a.kmerModel, a.altModel, a.llrThreshold, a.llrWindow, a.prior, a.minPositions, a.rescale, a.outEvents, a.outFolder,
            a.FileID, a.device, a.outLevel) == ('readllr', 'r.npz', 'm.npz', 'a.npz', 2.5, 'kmer', 0.5, 1, 0, '', 'mRes', 'mod', 0, 2)
    a = p.parse_args(['readllr', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz', '--altModel', 'a.npz', '--llrThreshold', '4', '--llrWindow', '3,0',
                      '--prior', '0.1', '--minPositions', '3', '--rescale', '1', '--outEvents', 'e.npz', '--outFolder', 'd', '--FileID', 'id',
                      '--device', '1', '--outLevel', '3'])
    assert (a.llrThreshold, a.llrWindow, a.prior, a.minPositions, a.rescale, a.outEvents, a.outFolder, a.FileID, a.device, a.outLevel) == \
        (4.0, '3,0', 0.1, 3, 1, 'e.npz', 'd', 'id', 1, 3)
    assert cli.parse_llr_window('kmer') == 'kmer' and cli.parse_llr_window('3,0') == (3, 0) and cli.parse_llr_window(' 7, 8') == (7, 8)
    assert all(cli.parse_llr_window(t) is None for t in ('', '3', '3,', '1,2,3', '-1,2', 'a,b', 'cover', '1.5,2'))
    for argv in (['readllr'], ['readllr', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz'], ['readllr', '--wrkBase1', 'r.npz', '--altModel', 'a.npz'],
                 ['readllr', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz', '--altModel', 'a.npz', '--rescale', '2']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    capsys.readouterr()
    assert cli.main(['readllr', '--wrkBase1', '/nonexistent/r.npz', '--kmerModel', '/nonexistent/m.npz', '--altModel', '/nonexistent/a.npz']) == 1
    out = capsys.readouterr().out
    assert all('Error: input /nonexistent/%s.npz does not exist' % n in out for n in 'rma')
    with tempfile.TemporaryDirectory() as tmp:
        reads, group, other = (os.path.join(tmp, n) for n in ('r.npz', 'g.npz', 'm.npz'))
        container.save_reads(reads, ['c'], ['+'], [0], [0, 2], np.array([0.5, 0.25]), np.array([b'A', b'C']))
        container.save_group(group, ['c'], ['+'], [0], ['A'], [0, 1], np.zeros(1, np.float32))
        np.savez(other, x=np.zeros(1))
        base = ['readllr', '--kmerModel', other, '--altModel', other]
        assert cli.main(base + ['--wrkBase1', group]) == 1                      # a per-position container has no reads
        assert 'Error: --wrkBase1 %s is not a read-level container (per-position containers have no reads)' % group in capsys.readouterr().out
        for bad, msg in ((['--llrWindow', '65,0'], "Error: --llrWindow should be 'kmer' or LO,HI with both in 0 .. 64"),
                         (['--llrWindow', '2'], "Error: --llrWindow should be 'kmer' or LO,HI with both in 0 .. 64"),
                         (['--llrWindow', 'site'], "Error: --llrWindow should be 'kmer' or LO,HI with both in 0 .. 64"),
                         (['--llrThreshold', '0'], 'Error: --llrThreshold should be finite and larger than 0'),
                         (['--llrThreshold', 'inf'], 'Error: --llrThreshold should be finite and larger than 0'),
                         (['--llrThreshold', 'nan'], 'Error: --llrThreshold should be finite and larger than 0'),
                         (['--prior', '0'], 'Error: --prior should lie between 0 and 1, both excluded'),
                         (['--prior', '1'], 'Error: --prior should lie between 0 and 1, both excluded'),
                         (['--minPositions', '0'], 'Error: --minPositions should be larger than 0')):
            assert cli.main(base + ['--wrkBase1', reads] + bad) == 1
            assert msg in capsys.readouterr().out
