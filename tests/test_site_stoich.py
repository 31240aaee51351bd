"""nmod_site_stoich (K14) without a GPU: the numpy restatement of the header's definition (tests/stoich_ref.py) against 50-digit mpmath
within the gates it derives, known answers, the score equation, a seeded simulation of the null law of p_null, the declarations and
struct layouts, the refusals of the C entry and of the Python layers before any device work, the marshalling, the writer and the
command line."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import readllr_ref as RF
import stoich_ref as F
from nanomod_amd import _lib as L, engine
from nanomod_amd import readllr as RL
from nanomod_amd.engine import site_stoich_host          # K14's entry: without it nothing here can pass
from test_engine_marshal import rec, NO_SUCH_DEVICE, SIZEOF_PARAMS          # noqa: F401  (rec: a stand-in library that records every call)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nanomod_hip.h')
SIZEOF_STOICH_OPTS = 32      # 4 x i32 + 2 doubles
SIZEOF_STOICH_OUT = 80       # 2 x i32 + 9 pointers


def _share(name, dev, gate, worst):
    """the deviation as a share of its gate; a deviation where the gate is 0 must be 0"""
    if gate == 0.0:
        assert dev == 0.0, '%s differs where its gate is 0' % name
        return
    worst[name] = max(worst.get(name, 0.0), dev / gate)


def test_restatement_is_pinned_against_mpmath():
    """24 seeded rows (1 .. 60 reads, separations 0.3 .. 8 sd, shares 0 .. 1, sums scaled up to x 40) and the constructed ones: every
    output within its gate of the 50-digit solution, exactly equal at either end"""
    rng = np.random.default_rng(1403)
    rows = []
    for _ in range(24):
        n = int(rng.choice([1, 2, 3, 5, 20, 60]))
        rows.append(F.simulate_row(rng, n, float(rng.choice(F.SEPARATIONS)), float(rng.choice(F.SHARES)), float(rng.choice([1, 1, 5, 40]))))
    rows += [np.array([800.0, 800.0, 800.0, -800.0]), np.array([-800.0] * 5), np.array([800.0] * 5), np.array([0.0, -0.0, 1.0, -2.0, 0.5]),
             np.array([np.nan, 2.0, -1.0, np.inf, 0.7, -np.inf, -0.2])]
    worst, ends = {}, 0
    for s in rows:
        r, x = F.row(s, min_valid=1), F.exact_row(s)
        for f in ('pi', 'pi_lo', 'pi_hi', 'stat'):
            _share(f, abs(float(x[f] - r[f])), r['gates'][f], worst)
        lo, hi = r['gates']['p_null']
        assert lo <= float(x['p_null']) <= hi, (lo, float(x['p_null']), hi)
        assert (r['pi'] == 0.0) == (x['pi'] == 0) and (r['pi'] == 1.0) == (x['pi'] == 1)
        ends += r['pi'] in (0.0, 1.0)
    print('worst deviation as a share of its gate: %s; %d of %d rows at an end' % (', '.join('%s %.3g' % kv for kv in sorted(worst.items())), ends, len(rows)))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert 3 <= ends <= len(rows) - 8                      # both kinds of row are there


def test_known_answers():
    r = F.row(np.array([800.0, 800.0, 800.0, -800.0]))
    assert abs(r['pi'] - 0.75) <= r['gates']['pi'] and r['status'] == 0 and r['n_valid'] == 4 and 0 < r['iters'] <= 60
    assert math.isfinite(r['stat']) and r['stat'] > 4000.0 and 0.0 < r['pi_lo'] < 0.75 < r['pi_hi'] < 1.0 and r['p_null'] == F.DBL_MIN
    # the likelihood is pi^3 (1 - pi): the interval is where 2 (l(3/4) - l(pi)) <= the drop
    ll = lambda p: 3.0 * math.log(p) + math.log(1.0 - p)
    for end in (r['pi_lo'], r['pi_hi']):
        assert abs(2.0 * (ll(0.75) - ll(end)) - F.CI_DROP_95) < 1e-9
    assert abs(r['stat'] - 2.0 * (2400.0 + ll(0.75))) < 1e-9
    r = F.row(np.array([-0.5, -3.0, -800.0, -1e-3]))
    assert (r['pi'], r['p_null'], r['pi_lo'], r['stat'], r['status'], r['iters']) == (0.0, 1.0, 0.0, 0.0, F.AT_ZERO, 0) and 0.0 < r['pi_hi'] < 1.0
    assert (r['resp'] == 0.0).all()
    r = F.row(np.array([800.0] * 5))
    assert (r['pi'], r['pi_hi'], r['status'], r['iters'], r['stat']) == (1.0, 1.0, F.AT_ONE, 0, 8000.0) and 0.0 < r['pi_lo'] < 1.0
    assert (r['resp'] == 1.0).all()
    assert abs(5.0 * math.log(r['pi_lo']) * -2.0 - F.CI_DROP_95) < 1e-9          # l = 5 log pi
    r = F.row(np.array([0.0, -0.0, 0.0, 0.0]))
    assert r['status'] == F.FLAT and r['n_valid'] == 4 and r['iters'] == 0 and all(np.isnan(r[f]) for f in F.FIELDS) and np.isnan(r['resp']).all()
    r = F.row(np.array([1.0, np.nan, -1.0]))
    assert r['status'] == F.TOO_FEW and r['n_valid'] == 2 and np.isnan(r['pi']) and np.isnan(r['resp']).all()
    r = F.row(np.array([1.5e308, 1.5e308, -3.0]))
    assert r['stat'] == math.inf and r['p_null'] == F.DBL_MIN and 0.0 < r['pi'] < 1.0
    r = F.row(np.array([2.0, -1.0, 0.5, -0.3]), max_iter=1)
    assert r['status'] & F.NOT_CONVERGED and r['iters'] == 1
    r = F.row(np.array([2.0, -1.0, 0.5, -0.3]), tol=0.0, max_iter=25)
    assert r['status'] & F.NOT_CONVERGED and r['iters'] == 25 and abs(r['pi'] - F.row(np.array([2.0, -1.0, 0.5, -0.3]))['pi']) < 1e-12


def test_a_single_valid_score_sits_at_an_end():
    for s, pi, st in ((5.0, 1.0, F.AT_ONE), (1e-300, 1.0, F.AT_ONE), (-5.0, 0.0, F.AT_ZERO), (-1e300, 0.0, F.AT_ZERO)):
        for pad in ([], [np.nan, np.inf]):
            r = F.row(np.array([s] + pad), min_valid=1)
            assert (r['pi'], r['status'], r['n_valid'], r['iters']) == (pi, st, 1, 0), (s, r)
            assert r['pi_lo'] <= r['pi'] <= r['pi_hi'] and r['resp'][0] == pi and np.isnan(r['resp'][1:]).all()
    assert F.row(np.array([5.0]))['status'] == F.TOO_FEW            # the default min_valid is 3


def test_mean_of_resp_is_the_estimate_at_an_interior_optimum():
    """the score equation: sum (r_i - pi^) = pi^ (1 - pi^) S(pi^)"""
    rng = np.random.default_rng(1404)
    worst, seen = 0.0, 0
    for sep in F.SEPARATIONS:
        for pi in (0.1, 0.5, 0.9):
            for n in (12, 150):
                r = F.row(F.simulate_row(rng, n, sep, pi))
                if r['status'] & (F.AT_ZERO | F.AT_ONE):
                    continue
                seen += 1
                worst = max(worst, abs(float(np.mean(r['resp'])) - r['pi']) / r['gates']['mean_resp'])
    print('mean(resp) - pi: worst share of its gate %.3g over %d interior rows' % (worst, seen))
    assert seen >= 16 and worst <= 1.0


@pytest.mark.parametrize('n', [20, 200])
@pytest.mark.parametrize('d', [1.0, 3.0])
def test_p_null_holds_its_level_on_canonical_rows(n, d):
    """4 000 rows of canonical reads, s = d x - d^2 / 2 with x ~ N(0, 1): the share of rows with p_null <= 0.05 may not exceed 0.05 by
    more than three binomial standard errors, 0.05 + 3 sqrt(0.05 0.95 / 4000) = 0.0603"""
    N = 4000
    rng = np.random.default_rng(1405 + int(n + 10 * d))
    x = rng.normal(size=(N, n))
    p = np.array([F.row(d * x[i] - 0.5 * d * d, estimate_only=True)['p_null'] for i in range(N)])
    share = float((p <= 0.05).mean())
    bound = 0.05 + 3.0 * math.sqrt(0.05 * 0.95 / N)
    print('n = %d, d = %g: %.4f of %d canonical rows at p_null <= 0.05 (bound %.4f); %.3f of them at pi^ = 0' % (n, d, share, N, bound, float((p == 1.0).mean())))
    assert abs(bound - 0.0603) < 5e-5 and share <= bound
    assert share >= 0.005                                   # the test is not void: it does reject


def test_ci_level_becomes_the_chi2_quantile():
    assert abs(F.ci_drop_of(0.95) - F.CI_DROP_95) < 1e-14 and abs(engine._stoich_opts(3, 0.95, 60, 1e-12).ci_drop - L.STOICH_CI_DROP_95) < 1e-14
    assert abs(engine._stoich_opts(3, 0.99, 60, 1e-12).ci_drop - 6.634896601021213) < 1e-12
    o = engine._stoich_opts(1, 0.5, 200, 0.0)
    assert (o.struct_size, o.max_iter, o.min_valid, o.reserved, o.tol) == (SIZEOF_STOICH_OPTS, 200, 1, 0, 0.0) and abs(o.ci_drop - 0.454936423119572) < 1e-12


# ----------------------------------------------------------------------------------------------- declarations and layouts
def test_entry_is_declared_and_exported():
    lib = L.load()
    header = open(HEADER).read()
    declared = set(re.findall(r'\b(nmod_[a-z_]+)\s*\(', header))
    assert 'nmod_site_stoich' in declared and 'nmod_site_stoich' in L._SIGNATURES and hasattr(lib, 'nmod_site_stoich')
    assert 'typedef struct nmod_stoich_opts { int32_t struct_size, max_iter, min_valid, reserved; double tol, ci_drop; } nmod_stoich_opts;' in header
    assert re.search(r'typedef struct nmod_stoich_out \{ int32_t struct_size; int32_t reserved;\s+double \*pi, \*pi_lo, \*pi_hi, \*stat, \*p_null; '
                     r'int32_t \*n_valid, \*iters; uint8_t\* status;[^\n]*\n\s+double\* resp;', header)
    assert ('enum { NMOD_STOICH_TOO_FEW = 1, NMOD_STOICH_FLAT = 2, NMOD_STOICH_NOT_CONVERGED = 4, NMOD_STOICH_AT_ZERO = 8, NMOD_STOICH_AT_ONE = 16,'
            in header and 'NMOD_STOICH_TOO_LARGE = 32 };' in header)
    assert (L.STOICH_TOO_FEW, L.STOICH_FLAT, L.STOICH_NOT_CONVERGED, L.STOICH_AT_ZERO, L.STOICH_AT_ONE, L.STOICH_TOO_LARGE) == \
        (F.TOO_FEW, F.FLAT, F.NOT_CONVERGED, F.AT_ZERO, F.AT_ONE, F.TOO_LARGE) == (1, 2, 4, 8, 16, 32)
    assert '#define NMOD_STOICH_SMALL 256' in header and '#define NMOD_STOICH_WAVE 1024' in header
    assert (L.STOICH_SMALL, L.STOICH_WAVE) == (F.SMALL, F.WAVE) == (256, 1024)
    src = open(os.path.join(os.path.dirname(HEADER), '..', 'nanomod_amd', 'csrc', 'site_stoich.hip')).read()
    assert 'constexpr int kStStage = %d;' % F.STAGE in src
    assert L.STOICH_FIELDS == F.FIELDS == ('pi', 'pi_lo', 'pi_hi', 'stat', 'p_null')
    assert '#define NMOD_ABI_VERSION 4' in header and lib.nmod_abi_version() == 4 == L.NMOD_ABI_VERSION          # a purely additive entry
    for text in ('t = -expm1(-fabs(s))', 'u = t / (1 - qt)', 'g += log1p(-qt)', 'max(0.5 erfc(sqrt(l^)), DBL_MIN)', 'ASYMPTOTIC',
                 "x' = x + S / D", 'tol == 0 runs max_iter evaluations'):
        assert text in header, text
    import nanomod_amd
    assert nanomod_amd.site_stoich_host is engine.site_stoich_host and nanomod_amd.write_site_stoich is RL.write_site_stoich


def test_struct_layouts_match_the_header():
    """sizes and offsets of the two new structs from a gcc-compiled program over the header itself"""
    fields = [('nmod_stoich_opts', L.NmodStoichOpts, ('struct_size', 'max_iter', 'min_valid', 'reserved', 'tol', 'ci_drop')),
              ('nmod_stoich_out', L.NmodStoichOut, ('struct_size', 'reserved', 'pi', 'pi_lo', 'pi_hi', 'stat', 'p_null', 'n_valid', 'iters', 'status', 'resp'))]
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
    assert (C.sizeof(L.NmodStoichOpts), C.sizeof(L.NmodStoichOut)) == (SIZEOF_STOICH_OPTS, SIZEOF_STOICH_OUT)
    assert L.NmodStoichOpts.tol.offset == 16 and L.NmodStoichOut.pi.offset == 8 and L.NmodStoichOut.resp.offset == 72


# ----------------------------------------------------------------------------------------------- the C entry's own refusals
def _site(lib, npos=3, *, score='x', off='x', stride=0, opts='x', out='x', opts_size=None, out_size=None, memspace=None, prm=None, dtype=7,
          max_iter=60, min_valid=3, tol=1e-12, ci_drop=F.CI_DROP_95):
    n = npos if 0 <= npos < 1000 else 3
    offs = np.arange(n + 1, dtype=np.int64) * 5
    sc = np.zeros(max(n, 1) * 5)
    cnt, fr = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1))
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    o = L.make_stoich_opts(max_iter, min_valid, tol, ci_drop)
    if opts_size is not None:
        o.struct_size = opts_size
    r = L.make_stoich_out(n_valid=cnt.ctypes.data, pi=fr.ctypes.data)
    if out_size is not None:
        r.struct_size = out_size
    if prm is None:                                                             # (dtype 7: this entry does not read it)
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace, dtype=dtype, stride0=stride)
    return lib.nmod_site_stoich(C.byref(prm), npos, pick(score, sc), pick(off, offs), C.byref(o) if opts is not None else None,
                                C.byref(r) if out is not None else None)


def test_site_stoich_refuses_invalid_arguments_before_any_device_work():
    """every case of the header returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone is NMOD_ERR_NO_DEVICE)"""
    lib = L.load()
    nan, inf = float('nan'), float('inf')
    site = lambda *a, **kw: _site(lib, *a, **kw)
    assert site() == -5 and site(off=None, stride=5) == -5 and site(memspace=L.MEM_DEVICE) == -5 and site(dtype=L.DTYPE_F32) == -5
    assert site(max_iter=1) == -5 and site(max_iter=200) == -5 and site(min_valid=1) == -5 and site(tol=0.0) == -5 and site(ci_drop=1e-300) == -5
    assert site(0) == 0 and site(0, score=None) == 0                            # no rows: no device needed
    assert all(site(max_iter=v) == -1 for v in (0, -1, 201)) and all(site(min_valid=v) == -1 for v in (0, -3))
    assert all(site(tol=v) == -1 for v in (-1e-12, nan, inf, -inf)) and all(site(ci_drop=v) == -1 for v in (0.0, -1.0, nan, inf, -inf))
    assert site(opts=None) == -1 and site(opts_size=24) == -1 and site(opts_size=40) == -1
    assert site(out=None) == -1 and site(out_size=72) == -1 and site(out_size=88) == -1
    assert site(off=None) == -1 and site(off=None, stride=-5) == -1             # neither offsets nor a stride
    assert site(-1) == -1 and site(2 ** 31 - 1) == -1 and site(2 ** 40) == -1
    assert site(score=None) == -1 and site(memspace=2) == -1
    assert site(off=np.array([0, 5, 4, 15], np.int64)) == -1 and site(off=np.array([-1, 5, 10, 15], np.int64)) == -1
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert site(prm=bad) == -1
    assert lib.nmod_site_stoich(None, 3, None, None, None, None) == -1


# ----------------------------------------------------------------------------------------------- the Python layers
def _refused_host():
    score, soff = np.zeros(20), np.arange(5, dtype=np.int64) * 5
    nan, inf = float('nan'), float('inf')
    w = lambda *a, **kw: ((a or (score, soff)), kw)
    cases = dict(min_valid_0=w(min_valid=0), min_valid_neg=w(min_valid=-2), min_valid_frac=w(min_valid=2.5),
                 max_iter_0=w(max_iter=0), max_iter_201=w(max_iter=201), max_iter_frac=w(max_iter=3.5),
                 tol_neg=w(tol=-1e-9), tol_nan=w(tol=nan), tol_inf=w(tol=inf),
                 ci_0=w(ci_level=0.0), ci_1=w(ci_level=1.0), ci_neg=w(ci_level=-0.5), ci_nan=w(ci_level=nan), ci_2=w(ci_level=2.0),
                 no_rows=w(score, None), stride_0=w(score, None, stride=0), ragged=w(score, None, stride=3), short=w(score[:-1], soff),
                 down=w(score, np.array([0, 6, 4, 20], np.int64)), two_d=w(score.reshape(4, 5), soff), off_empty=w(score, soff[:0]))
    return [pytest.param(a, kw, id=name) for name, (a, kw) in cases.items()]


@pytest.mark.parametrize('args,kw', _refused_host())
def test_refused_before_the_library(args, kw):
    L.load()                                     # the real library: a call that reached it would be a NanomodLibraryError
    with pytest.raises(ValueError):
        site_stoich_host(*args, device=NO_SUCH_DEVICE, **kw)


def test_accepted_calls_reach_the_library():
    with pytest.raises(L.NanomodLibraryError, match='nmod_site_stoich'):
        site_stoich_host(np.zeros(10), np.array([0, 4, 10], np.int64), device=NO_SUCH_DEVICE)
    res = site_stoich_host(np.zeros(0), np.zeros(1, np.int64), resp=True, device=NO_SUCH_DEVICE)        # no rows: no device
    assert res['pi'].shape == (0,) and res['resp'].shape == (0,) and res['status'].dtype == np.uint8


@pytest.mark.parametrize('resp', [False, True])
@pytest.mark.parametrize('layout', ['csr', 'stride'])
def test_site_stoich_host_marshalling(rec, layout, resp):
    score = np.random.default_rng(4).normal(size=40)
    off = np.arange(5, dtype=np.int64) * 10 if layout == 'csr' else None
    res = site_stoich_host(score, off, stride=10, min_valid=2, ci_level=0.9, max_iter=33, tol=1e-9, resp=resp, device=1)
    prm, npos, s, o, opts, out = rec.only('nmod_site_stoich')
    assert {f: prm[f] for f in ('struct_size', 'memspace', 'dtype', 'device', 'stride0')} == \
        dict(struct_size=SIZEOF_PARAMS, memspace=0, dtype=2, device=1, stride0=0 if off is not None else 10)
    assert (npos, s) == (4, score.ctypes.data) and o == (off.ctypes.data if off is not None else None)
    assert {k: opts[k] for k in ('struct_size', 'max_iter', 'min_valid', 'reserved', 'tol')} == \
        dict(struct_size=SIZEOF_STOICH_OPTS, max_iter=33, min_valid=2, reserved=0, tol=1e-9) and abs(opts['ci_drop'] - F.ci_drop_of(0.9)) < 1e-15
    assert set(res) == set(F.FIELDS) | {'n_valid', 'iters', 'status'} | ({'resp'} if resp else set())
    assert all(res[f].dtype == np.float64 and res[f].shape == (4,) and np.isnan(res[f]).all() for f in F.FIELDS)
    assert all(res[f].dtype == np.int32 and res[f].shape == (4,) and not res[f].any() for f in ('n_valid', 'iters'))
    assert not resp or (res['resp'].dtype == np.float64 and res['resp'].shape == (40,))
    members = {k: v for k, v in out.items() if k not in ('struct_size', 'reserved')}
    assert out['struct_size'] == SIZEOF_STOICH_OUT and out['reserved'] == 0
    assert {k for k, v in members.items() if v is not None} == set(res) and all(members[k] == a.ctypes.data for k, a in res.items())


def test_defaults(rec):
    site_stoich_host(np.zeros(10), None, stride=5)
    opts = rec.only('nmod_site_stoich')[4]
    assert (opts['max_iter'], opts['min_valid'], opts['tol']) == (60, 3, 1e-12) and abs(opts['ci_drop'] - 3.841458820694124) < 1e-14


def test_device_detector_checks_its_arguments_before_the_library(rec):
    import torch
    det = engine.DeviceDetector(0)
    score = torch.from_numpy(np.zeros(20))
    for kw, msg in ((dict(stride=5, min_valid=0), 'min_valid'), (dict(stride=5, max_iter=0), 'max_iter'), (dict(stride=5, max_iter=201), 'max_iter'),
                    (dict(stride=5, tol=-1.0), 'tol'), (dict(stride=5, tol=float('nan')), 'tol'), (dict(stride=5, ci_level=1.0), 'ci_level'),
                    (dict(stride=5, ci_level=0.0), 'ci_level'), (dict(stride=5), 'CUDA'), (dict(stride=5, resp=True), 'CUDA')):
        with pytest.raises(ValueError, match=msg):
            det.site_stoich(score, **kw)
    assert rec.calls == []


def test_call_reads_llr_refuses_stoich_options_before_any_device_work(rec):
    reads, model, alt, planted = RF.chain_inputs(n_reads=4)
    call = lambda **kw: RL.call_reads_llr(reads, model, alt, device=NO_SUCH_DEVICE, log=None, **kw)
    for kw, msg in ((dict(stoich=dict(level=0.9)), 'unknown option'), (dict(stoich=dict(ci_level=1.0)), 'ci_level'),
                    (dict(stoich=dict(min_valid=0)), 'min_valid'), (dict(stoich=dict(max_iter=500)), 'max_iter'), (dict(stoich=dict(tol=-1.0)), 'tol')):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    assert rec.calls == []


def test_writer():
    nan = np.nan
    sites = dict(chrom=np.array(['chr1', 'chr1', 'chr2']), strand=np.array(['+', '-', '+']), pos=np.array([0, 41, 7], np.int64),
                 base=np.array(['A', 'c', 'N']), n_reads=np.array([40, 2, 30], np.int32), n_valid=np.array([38, 1, 30], np.int32),
                 pi=np.array([1.0 / 3.0, nan, 0.0]), pi_lo=np.array([0.2, nan, 0.0]), pi_hi=np.array([0.5, nan, 0.0625]),
                 stat=np.array([41.23456, nan, 0.0]), p_null=np.array([6.7e-11, nan, 1.0]), iters=np.array([6, 0, 0], np.int32),
                 stoich_status=np.array([0, 1, 8], np.uint8))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 't.txt')
        RL.write_site_stoich(path, sites)
        assert open(path).read() == ('chr1 + 1 A 40 38 0.333333 0.200000 0.500000 41.235 6.700E-11 0\n'
                                     'chr1 - 42 c 2 1 nan nan nan nan nan 1\n'
                                     'chr2 + 8 N 30 30 0.000000 0.000000 0.062500 0.000 1.000E+00 8\n')
    sites['stat'][0] = np.inf
    with tempfile.TemporaryDirectory() as tmp:
        RL.write_site_stoich(os.path.join(tmp, 't.txt'), sites)
        assert open(os.path.join(tmp, 't.txt')).read().split('\n')[0].split()[9] == 'inf'


def test_cli_site_fraction_off_is_todays_behaviour(capsys, monkeypatch):
    from nanomod_amd import cli, container
    p = cli.build_parser()
    argv = ['readllr', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz', '--altModel', 'a.npz']
    a = p.parse_args(argv)
    assert (a.siteFraction, a.minValid, a.ciLevel) == (0, 3, 0.95) and vars(p.parse_args(argv + ['--siteFraction', '0'])) == vars(a)
    b = p.parse_args(argv + ['--siteFraction', '1', '--minValid', '5', '--ciLevel', '0.9'])
    assert (b.siteFraction, b.minValid, b.ciLevel) == (1, 5, 0.9)
    assert {k: v for k, v in vars(b).items() if k not in ('siteFraction', 'minValid', 'ciLevel')} == \
        {k: v for k, v in vars(a).items() if k not in ('siteFraction', 'minValid', 'ciLevel')}
    with pytest.raises(SystemExit):
        p.parse_args(argv + ['--siteFraction', '2'])
    capsys.readouterr()
    # what run_readllr hands on and writes: without the option no stoich argument and no third file
    seen = []
    table = dict(index=np.arange(1), chrom=np.array(['c']), strand=np.array(['+']), start=np.zeros(1, np.int64), events=np.array([2]),
                 n_sites=np.array([2], np.int32), n_mod=np.array([1], np.int32), n_can=np.array([0], np.int32), status=np.zeros(1, np.uint8))
    sites = dict(chrom=np.array(['c']), strand=np.array(['+']), pos=np.zeros(1, np.int64), base=np.array(['A']), n_reads=np.array([1], np.int32),
                 n_valid=np.array([1], np.int32), n_mod=np.array([1], np.int32), n_can=np.array([0], np.int32), frac=np.array([1.0]))
    more = dict(pi=np.array([1.0]), pi_lo=np.array([0.1]), pi_hi=np.array([1.0]), stat=np.array([3.0]), p_null=np.array([0.04]),
                iters=np.zeros(1, np.int32), stoich_status=np.array([16], np.uint8))

    def fake(reads, model, alt, **kw):
        seen.append(kw)
        return table, dict(sites, **more) if 'stoich' in kw else sites
    monkeypatch.setattr(RL, 'call_reads_llr', fake)
    from nanomod_amd import kmermodel
    monkeypatch.setattr(kmermodel, 'load_kmer_model', lambda path: path)
    with tempfile.TemporaryDirectory() as tmp:
        reads = os.path.join(tmp, 'r.npz')
        container.save_reads(reads, ['c'], ['+'], [0], [0, 2], np.array([0.5, 0.25]), np.array([b'A', b'C']))
        np.savez(os.path.join(tmp, 'm.npz'), x=np.zeros(1))
        base = ['readllr', '--wrkBase1', reads, '--kmerModel', os.path.join(tmp, 'm.npz'), '--altModel', os.path.join(tmp, 'm.npz')]
        for extra, name in (([], 'off'), (['--siteFraction', '0'], 'zero'), (['--siteFraction', '1', '--minValid', '2', '--ciLevel', '0.8'], 'on')):
            assert cli.main(base + extra + ['--outFolder', os.path.join(tmp, name)]) == 0
        assert 'stoich' not in seen[0] and seen[0] == seen[1] and seen[2] == dict(seen[0], stoich=dict(min_valid=2, ci_level=0.8))
        assert sorted(os.listdir(os.path.join(tmp, 'off'))) == sorted(os.listdir(os.path.join(tmp, 'zero'))) == ['mod_read_llr.txt', 'mod_site_llr.txt']
        assert sorted(os.listdir(os.path.join(tmp, 'on'))) == ['mod_read_llr.txt', 'mod_site_llr.txt', 'mod_site_stoich.txt']
        for f in ('mod_read_llr.txt', 'mod_site_llr.txt'):
            assert open(os.path.join(tmp, 'off', f)).read() == open(os.path.join(tmp, 'zero', f)).read() == open(os.path.join(tmp, 'on', f)).read()
        assert open(os.path.join(tmp, 'on', 'mod_site_stoich.txt')).read() == 'c + 1 A 1 1 1.000000 0.100000 1.000000 3.000 4.000E-02 16\n'
        capsys.readouterr()
        for bad, msg in ((['--minValid', '0'], 'Error: --minValid should be larger than 0'),
                         (['--ciLevel', '0'], 'Error: --ciLevel should lie between 0 and 1, both excluded'),
                         (['--ciLevel', '1'], 'Error: --ciLevel should lie between 0 and 1, both excluded'),
                         (['--ciLevel', 'nan'], 'Error: --ciLevel should lie between 0 and 1, both excluded')):
            assert cli.main(base + bad) == 1
            assert msg in capsys.readouterr().out
