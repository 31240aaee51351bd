"""The argument layer of DeviceDetector's secondary entries (fdr, mix, one_sample, kmer_model, rescale_reads, read_calls, site_calls,
read_llr, site_llr, site_stoich, site_diff) on the GPU: what each refuses with ValueError before the library is called (a side vector of the wrong dtype or length, a CPU tensor,
a non-contiguous slice, a malformed `out=` dict), which entries also refuse a tensor of two dimensions and which take it, that a
well-formed `out=` dict comes back as the same objects with the same values, and that each entry agrees bit for bit with its *_host
counterpart on the same data (both reach the same kernels).  Tiny shapes: 4 positions of 10 float32 samples, 4 codes, 3 reads of 6
events at k = 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NPOS, ROW, NCODES, NREADS, READ_LEN = 4, 10, 4, 3, 6
NEV = NREADS * READ_LEN
RESCALE_OPTS = dict(min_events=2)


class Ctx:
    """one detector, and the same tiny inputs on the host (h) and on the device (d)"""

    def __init__(self):
        import torch
        from nanomod_amd import engine
        self.torch, self.engine = torch, engine
        self.det = engine.DeviceDetector(0)                               # stouffer, nb = 2, weights_dif = 2.0
        rng = np.random.default_rng(7)
        h = {}
        h['sig0'] = rng.normal(size=NPOS * ROW).astype(np.float32)
        h['sig1'] = (rng.normal(size=NPOS * ROW) + np.repeat([0.0, 2.0, 0.0, 3.0], ROW)).astype(np.float32)
        h['row_off'] = np.arange(NPOS + 1, dtype=np.int64) * ROW
        h['run'] = np.zeros(NPOS, np.int32)
        h['p'] = np.array([0.001, 0.2, 0.8, 0.004])
        h['gate'] = np.array([0.01, 0.9, np.nan, 0.02])
        h['ref_mean'] = np.zeros(NPOS)
        h['ref_sd'] = np.ones(NPOS)
        h['ref_n'] = np.full(NPOS, 30, np.int32)
        h['code'] = np.array([0, 3, -1, 1], np.int32)
        h['keep_lo'] = np.full(NCODES, -2.0)
        h['keep_hi'] = np.full(NCODES, 2.0)
        # reads drawn from a k = 1 model: a shift and a scale per read, a little noise
        h['mean'] = np.array([-1.0, 0.0, 1.0, 2.0])
        h['sd'] = np.full(4, 0.25)
        h['off'] = np.arange(NREADS + 1, dtype=np.int64) * READ_LEN
        letters = rng.integers(0, 4, NEV)
        h['base'] = np.frombuffer(b'ACGT', np.uint8)[letters].copy()
        a, b = np.repeat([0.1, -0.2, 0.0], READ_LEN), np.repeat([1.1, 0.9, 1.0], READ_LEN)
        h['val'] = (a + b * (h['mean'][letters] + 0.05 * rng.normal(size=NEV))).astype(np.float32)
        h['shift'] = np.array([0.1, -0.2, 0.0])
        h['scale'] = np.array([1.1, 0.9, 1.0])
        h['score'] = rng.uniform(size=NPOS * ROW)
        h['score'][::7] = np.nan
        h['score'][3::5] *= 0.01
        # a second table for read_llr, and window sums of two samples for site_llr, site_stoich and site_diff
        h['alt_mean'] = h['mean'] + np.array([0.5, -0.4, 0.6, 0.3])
        h['alt_sd'] = np.array([0.3, 0.25, 0.2, 0.35])
        for name, share in (('lscore0', 0.2), ('lscore1', 0.7)):
            h[name] = np.where(rng.uniform(size=NPOS * ROW) < share, 4.0, -4.0) + 2.0 * rng.normal(size=NPOS * ROW)
            h[name][5::11] = np.nan
        self.h = h
        self.d = {k: torch.from_numpy(v).to('cuda:0') for k, v in h.items()}
        self.model = dict(k=1, center=0, mean=h['mean'], sd=h['sd'])
        self.alt = dict(k=1, center=0, mean=h['alt_mean'], sd=h['alt_sd'])

    def host(self, res):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.fixture(scope='module')
def ctx():
    return Ctx()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def assert_same_dict(got, exp):
    assert set(got) == set(exp)
    for k in exp:
        assert same(got[k], exp[k]), (k, got[k], exp[k])


def wrong(t, torch):
    """a side vector four wrong ways: another dtype, one element more, on the host, a strided slice of the right element count"""
    other = torch.float32 if t.dtype == torch.float64 else torch.int64 if t.dtype in (torch.int32, torch.uint8) else torch.float64
    return {'dtype': t.to(other), 'length': torch.cat([t, t[:1]]), 'cpu': t.cpu(), 'strided': t.repeat_interleave(2)[::2]}


def two_dim(t):
    return t.view(2, t.numel() // 2)


WAYS = ('dtype', 'length', 'cpu', 'strided')
# not rules of the read entries: val has three dtypes, and off of any length describes that many reads
READ_WAYS = [(n, w) for n in ('mean', 'sd', 'base', 'val', 'off') for w in WAYS if (n, w) not in (('val', 'dtype'), ('off', 'length'))]


# --------------------------------------------------------------------------------------------------------------------- fdr
@pytest.mark.parametrize('way', WAYS)
def test_fdr_refuses(ctx, way):
    p = ctx.d['p']
    with pytest.raises(ValueError):
        ctx.det.fdr({'a': p, 'b': wrong(p, ctx.torch)[way]}, tracks=('a', 'b'))


def test_fdr_refuses_two_dimensions(ctx):
    with pytest.raises(ValueError):                                       # fdr asks for dim() == 1
        ctx.det.fdr({'a': two_dim(ctx.d['p'])}, tracks=('a',))


def test_fdr_agrees_with_host(ctx):
    qs, summary = ctx.det.fdr({'a': ctx.d['p']}, tracks=('a',), method='by', alpha=0.1)
    ctx.torch.cuda.synchronize()
    hq, hs = ctx.engine.fdr_adjust_host(ctx.h['p'], method='by', alpha=0.1)
    assert len(qs) == 1 and same(qs[0].cpu().numpy(), hq[0])
    ds = ctx.engine.fdr_summary_dicts(summary)
    assert len(ds) == 1 and all(same(ds[0][f], hs[0][f]) for f in ('tested', 'excluded', 'rejected', 'p_crit'))
    assert hs[0]['rejected'] > 0


# --------------------------------------------------------------------------------------------------------------------- mix
def _mix(ctx, gate, **kw):
    d = ctx.d
    return ctx.det.mix(d['sig0'], d['sig1'], stride0=ROW, stride1=ROW, gate=gate, gate_max=0.05, want_resp=True, **kw)


@pytest.mark.parametrize('way', WAYS)
def test_mix_refuses(ctx, way):
    with pytest.raises(ValueError):
        _mix(ctx, wrong(ctx.d['gate'], ctx.torch)[way])


def test_mix_agrees_with_host_and_takes_two_dimensions(ctx):
    h = ctx.h
    got = ctx.host(_mix(ctx, ctx.d['gate']))
    exp = ctx.engine.mix_fraction_host(h['sig0'], None, h['sig1'], None, stride0=ROW, stride1=ROW, gate=h['gate'], gate_max=0.05,
                                       want_resp=True)
    assert_same_dict(got, exp)
    assert (exp['status'] & 4).tolist() == [0, 4, 4, 0]                   # the gate left positions 1 and 2 out
    assert_same_dict(ctx.host(_mix(ctx, two_dim(ctx.d['gate']))), exp)    # mix does not ask for dim() == 1
    out = _mix(ctx, ctx.d['gate'])
    assert _mix(ctx, ctx.d['gate'], out=out) is out                       # `out` is taken as it is


# -------------------------------------------------------------------------------------------------------------- one sample
def _one(ctx, **kw):
    d = ctx.d
    a = dict(ref_sd=d['ref_sd'], ref_n=d['ref_n'], run_id=d['run'])
    a.update(kw)
    out = a.pop('out', None)
    return ctx.det.one_sample(d['sig1'], d['ref_mean'], a['ref_sd'], a['ref_n'], a['run_id'], stride=ROW, out=out)


@pytest.mark.parametrize('name', ['ref_sd', 'ref_n', 'run_id'])
@pytest.mark.parametrize('way', WAYS)
def test_one_sample_refuses(ctx, way, name):
    with pytest.raises(ValueError):
        _one(ctx, **{name: wrong(ctx.d[{'run_id': 'run'}.get(name, name)], ctx.torch)[way]})


def test_one_sample_agrees_with_host_and_takes_two_dimensions(ctx):
    h = ctx.h
    got = ctx.host(_one(ctx))
    exp = ctx.engine.one_sample_host(h['sig1'], None, h['ref_mean'], h['ref_sd'], h['ref_n'], h['run'], stride=ROW)
    assert_same_dict(got, exp)
    assert_same_dict(ctx.host(_one(ctx, ref_sd=two_dim(ctx.d['ref_sd']))), exp)       # one_sample does not ask for dim() == 1
    out = _one(ctx)
    assert _one(ctx, out=out) is out


# ------------------------------------------------------------------------------------------------------------- k-mer model
def _kmer(ctx, **kw):
    d = ctx.d
    a = dict(code=d['code'], keep_lo=d['keep_lo'], keep_hi=d['keep_hi'], out=None)
    a.update(kw)
    return ctx.det.kmer_model(d['sig1'], a['code'], NCODES, a['keep_lo'], a['keep_hi'], stride=ROW, npos=NPOS, out=a['out'])


@pytest.mark.parametrize('name', ['code', 'keep_lo', 'keep_hi'])
@pytest.mark.parametrize('way', WAYS)
def test_kmer_model_refuses(ctx, way, name):
    with pytest.raises(ValueError):
        _kmer(ctx, **{name: wrong(ctx.d[name], ctx.torch)[way]})


def test_kmer_model_agrees_with_host_and_takes_two_dimensions(ctx):
    h = ctx.h
    got = ctx.host(_kmer(ctx))
    exp = ctx.engine.kmer_model_host(h['sig1'], None, h['code'], NCODES, h['keep_lo'], h['keep_hi'], stride=ROW)
    assert_same_dict(got, exp)
    assert_same_dict(ctx.host(_kmer(ctx, code=two_dim(ctx.d['code']))), exp)          # kmer_model does not ask for dim() == 1
    out = _kmer(ctx)
    assert _kmer(ctx, out=out) is out


# ------------------------------------------------------------------------------------------------------------ rescale_reads
def _rescale(ctx, mode='fit_apply', **kw):
    d = ctx.d
    a = dict(val=d['val'], off=d['off'], base=d['base'], mean=d['mean'], sd=d['sd'], shift=None, scale=None, out=None, inplace=False)
    if mode == 'apply_only':
        a.update(base=None, mean=None, sd=None, shift=d['shift'], scale=d['scale'])
    a.update(kw)
    model = (a['mean'], a['sd'], 1, 0) if mode != 'apply_only' else ()
    return ctx.det.rescale_reads(a['val'], a['off'], a['base'], *model, mode=mode, shift=a['shift'], scale=a['scale'],
                                 inplace=a['inplace'], out=a['out'], **RESCALE_OPTS)


@pytest.mark.parametrize('name,way,mode', [(n, w, 'fit_only' if n == 'sd' else 'fit_apply') for n, w in READ_WAYS]
                         + [(n, w, 'apply_only') for n in ('shift', 'scale') for w in WAYS])
def test_rescale_reads_refuses(ctx, name, way, mode):
    with pytest.raises(ValueError):
        _rescale(ctx, mode, **{name: wrong(ctx.d[name], ctx.torch)[way]})


@pytest.mark.parametrize('mode', ['fit_apply', 'fit_only', 'apply_only'])
def test_rescale_reads_agrees_with_host(ctx, mode):
    h = ctx.h
    kw = dict(shift=h['shift'], scale=h['scale']) if mode == 'apply_only' else {}
    exp = ctx.engine.rescale_reads_host(h['val'], h['off'], h['base'], None if mode == 'apply_only' else ctx.model, mode=mode, **kw,
                                        **RESCALE_OPTS)
    res = _rescale(ctx, mode)
    assert_same_dict(ctx.host(res), exp)
    if mode == 'apply_only':                                              # the caller's own pairs come back
        assert res['shift'] is ctx.d['shift'] and res['scale'] is ctx.d['scale']
    if mode == 'fit_apply':                                               # rescale_reads does not ask for dim() == 1
        assert_same_dict(ctx.host(_rescale(ctx, mean=two_dim(ctx.d['mean']))), exp)
        val = ctx.d['val'].clone()
        inplace = _rescale(ctx, val=val, inplace=True)
        assert inplace['val'] is val and same(ctx.host(inplace)['val'], exp['val'])


@pytest.mark.parametrize('mode', ['fit_apply', 'fit_only', 'apply_only'])
def test_rescale_reads_out(ctx, mode):
    torch = ctx.torch
    first = _rescale(ctx, mode)
    exp = ctx.host(first)
    again = _rescale(ctx, mode, out=first)
    assert again is first and all(again[k] is first[k] for k in exp)
    assert_same_dict(ctx.host(again), exp)
    assert set(exp) == {'shift', 'scale', 'n_used', 'status'} | ({'val'} if mode != 'fit_only' else set())
    bad = [dict(first, status=first['status'].to(torch.int32)), dict(first, shift=torch.cat([first['shift'], first['shift'][:1]])),
           dict(first, n_used=first['n_used'].cpu()), {k: v for k, v in first.items() if k != 'scale'}]
    if mode != 'fit_only':
        bad += [dict(first, val=first['val'].double()), dict(first, val=first['val'][:-1])]
    for out in bad:
        with pytest.raises(ValueError):
            _rescale(ctx, mode, out=out)


# --------------------------------------------------------------------------------------------------------------- read_calls
def _calls(ctx, want=('z', 'p', 'p_win'), **kw):
    d = ctx.d
    a = dict(val=d['val'], off=d['off'], base=d['base'], mean=d['mean'], sd=d['sd'], out=None)
    a.update(kw)
    return ctx.det.read_calls(a['val'], a['off'], a['base'], a['mean'], a['sd'], 1, 0, nb=1, alpha=0.05, want=want, out=a['out'])


@pytest.mark.parametrize('name,way', READ_WAYS)
def test_read_calls_refuses(ctx, name, way):
    with pytest.raises(ValueError):
        _calls(ctx, **{name: wrong(ctx.d[name], ctx.torch)[way]})


@pytest.mark.parametrize('name', ['mean', 'sd', 'val', 'base'])
def test_read_calls_refuses_two_dimensions(ctx, name):
    with pytest.raises(ValueError):                                       # read_calls asks for dim() == 1
        _calls(ctx, **{name: two_dim(ctx.d[name])})


@pytest.mark.parametrize('want', [('p_win',), ('z', 'p', 'p_win')])
def test_read_calls_agrees_with_host_and_out(ctx, want):
    h, torch = ctx.h, ctx.torch
    exp = ctx.engine.read_calls_host(h['val'], h['off'], h['base'], ctx.model, nb=1, alpha=0.05, want=want)
    first = _calls(ctx, want)
    assert_same_dict(ctx.host(first), exp)
    assert set(exp) == set(want) | {'n_sites', 'n_called', 'status'}
    again = _calls(ctx, want, out=first)
    assert again is first and all(again[k] is first[k] for k in exp)
    assert_same_dict(ctx.host(again), exp)
    bad = [dict(first, status=first['status'].to(torch.int32)), dict(first, p_win=first['p_win'][:-1]),
           dict(first, n_sites=first['n_sites'].cpu()), {k: v for k, v in first.items() if k != 'n_called'}]
    for out in bad:
        with pytest.raises(ValueError):
            _calls(ctx, want, out=out)


# --------------------------------------------------------------------------------------------------------------- site_calls
@pytest.mark.parametrize('way', WAYS)
def test_site_calls_refuses(ctx, way):
    score = wrong(ctx.d['score'], ctx.torch)[way]
    with pytest.raises(ValueError):                                       # ('length': 41 scores are no 5 rows of 10)
        ctx.det.site_calls(score, stride=ROW, npos=NPOS + 1 if way == 'length' else None)


@pytest.mark.parametrize('way', ['dtype', 'cpu', 'strided'])
def test_site_calls_refuses_off(ctx, way):
    with pytest.raises(ValueError):
        ctx.det.site_calls(ctx.d['score'], off=wrong(ctx.d['row_off'], ctx.torch)[way])


def test_site_calls_two_dimensions(ctx):
    with pytest.raises(ValueError):                                       # site_calls asks for dim() == 1 of the scores ...
        ctx.det.site_calls(two_dim(ctx.d['score']), stride=ROW)
    exp = ctx.engine.site_calls_host(ctx.h['score'], ctx.h['row_off'], alpha=0.05)
    got = ctx.det.site_calls(ctx.d['score'], off=ctx.d['row_off'].view(1, NPOS + 1), alpha=0.05)       # ... not of the offsets
    assert_same_dict(ctx.host(got), exp)


@pytest.mark.parametrize('layout', ['csr', 'stride'])
def test_site_calls_agrees_with_host_and_out(ctx, layout):
    h, d, torch = ctx.h, ctx.d, ctx.torch
    exp = ctx.engine.site_calls_host(h['score'], h['row_off'] if layout == 'csr' else None, stride=ROW, alpha=0.05)
    call = lambda out=None: ctx.det.site_calls(d['score'], off=d['row_off'] if layout == 'csr' else None, stride=ROW, alpha=0.05, out=out)
    first = call()
    assert_same_dict(ctx.host(first), exp)
    assert exp['n_valid'].sum() == np.isfinite(h['score']).sum() and 0 < exp['n_called'].sum() < exp['n_valid'].sum()
    again = call(first)
    assert again is first and all(again[k] is first[k] for k in exp)
    assert_same_dict(ctx.host(again), exp)
    bad = [dict(first, frac=first['frac'].float()), dict(first, n_valid=torch.cat([first['n_valid'], first['n_valid'][:1]])),
           dict(first, n_called=first['n_called'].cpu()), {k: v for k, v in first.items() if k != 'frac'}]
    for out in bad:
        with pytest.raises(ValueError):
            call(out)


# ---------------------------------------------------------------------------------------------------------------- read_llr
LLR_OPTS = dict(window=(1, 1), thr=1.0, prior_logit=0.25)
LLR_WAYS = READ_WAYS + [(n, w) for n in ('alt_mean', 'alt_sd') for w in WAYS]


def sentinel(out, torch):
    """the tensors of an out dict overwritten with values no entry writes there"""
    for t in out.values():
        t.fill_(-12345.0 if t.dtype.is_floating_point else 0xA5 if t.dtype == torch.uint8 else -77)
    return out


def _llr(ctx, want=('llr', 'llr_win', 'p_mod'), **kw):
    d = ctx.d
    a = dict(val=d['val'], off=d['off'], base=d['base'], mean=d['mean'], sd=d['sd'], alt_mean=d['alt_mean'], alt_sd=d['alt_sd'], out=None)
    a.update(kw)
    return ctx.det.read_llr(a['val'], a['off'], a['base'], a['mean'], a['sd'], a['alt_mean'], a['alt_sd'], 1, 0, want=want, out=a['out'], **LLR_OPTS)


@pytest.mark.parametrize('name,way', LLR_WAYS)
def test_read_llr_refuses(ctx, name, way):
    with pytest.raises(ValueError):
        _llr(ctx, **{name: wrong(ctx.d[name], ctx.torch)[way]})


@pytest.mark.parametrize('name', ['mean', 'sd', 'alt_mean', 'alt_sd', 'val', 'base'])
def test_read_llr_refuses_two_dimensions(ctx, name):
    with pytest.raises(ValueError):                                       # read_llr asks for dim() == 1
        _llr(ctx, **{name: two_dim(ctx.d[name])})


@pytest.mark.parametrize('want', [('llr_win',), ('llr', 'llr_win', 'p_mod')])
def test_read_llr_agrees_with_host_and_out(ctx, want):
    h, torch = ctx.h, ctx.torch
    exp = ctx.engine.read_llr_host(h['val'], h['off'], h['base'], ctx.model, ctx.alt, want=want, **LLR_OPTS)
    first = _llr(ctx, want)
    assert_same_dict(ctx.host(first), exp)
    assert set(exp) == set(want) | {'n_sites', 'n_mod', 'n_can', 'status'} and exp['n_sites'].sum() == NEV and exp['n_can'].sum() > 0
    again = _llr(ctx, want, out=sentinel(first, torch))
    assert again is first and all(again[k] is first[k] for k in exp)
    assert_same_dict(ctx.host(again), exp)
    bad = [dict(first, status=first['status'].to(torch.int32)), dict(first, llr_win=first['llr_win'][:-1]),
           dict(first, n_sites=first['n_sites'].cpu()), {k: v for k, v in first.items() if k != 'n_can'}]
    for out in bad:
        with pytest.raises(ValueError):
            _llr(ctx, want, out=out)


# ---------------------------------------------------------------------------------------------- site_llr and site_stoich
# (device method, host counterpart, options of both, an output of one element per position, an output a malformed dict leaves out)
SITE_ENTRIES = {
    'site_llr': ('site_llr', 'site_llr_host', dict(thr=1.0), 'frac', 'n_can'),
    'site_stoich': ('site_stoich', 'site_stoich_host', dict(min_valid=2), 'pi', 'p_null'),
    'site_stoich_resp': ('site_stoich', 'site_stoich_host', dict(min_valid=2, resp=True), 'pi', 'resp'),
}


def _site(ctx, entry, score, **kw):
    method, _, opts, _, _ = SITE_ENTRIES[entry]
    return getattr(ctx.det, method)(score, **dict(opts, **kw))


@pytest.mark.parametrize('entry', list(SITE_ENTRIES))
@pytest.mark.parametrize('way', WAYS)
def test_site_rows_refuse(ctx, entry, way):
    score = wrong(ctx.d['lscore1'], ctx.torch)[way]
    with pytest.raises(ValueError):                                       # ('length': 41 scores are no 5 rows of 10)
        _site(ctx, entry, score, stride=ROW, npos=NPOS + 1 if way == 'length' else None)


@pytest.mark.parametrize('entry', list(SITE_ENTRIES))
@pytest.mark.parametrize('way', ['dtype', 'cpu', 'strided'])
def test_site_rows_refuse_off(ctx, entry, way):
    with pytest.raises(ValueError):
        _site(ctx, entry, ctx.d['lscore1'], off=wrong(ctx.d['row_off'], ctx.torch)[way])


@pytest.mark.parametrize('entry', list(SITE_ENTRIES))
def test_site_rows_two_dimensions(ctx, entry):
    _, host_fn, opts, _, _ = SITE_ENTRIES[entry]
    with pytest.raises(ValueError):                                       # the entries ask for dim() == 1 of the scores ...
        _site(ctx, entry, two_dim(ctx.d['lscore1']), stride=ROW)
    exp = getattr(ctx.engine, host_fn)(ctx.h['lscore1'], ctx.h['row_off'], **opts)
    got = _site(ctx, entry, ctx.d['lscore1'], off=ctx.d['row_off'].view(1, NPOS + 1))              # ... not of the offsets
    assert_same_dict(ctx.host(got), exp)


@pytest.mark.parametrize('entry', list(SITE_ENTRIES))
@pytest.mark.parametrize('layout', ['csr', 'stride'])
def test_site_rows_agree_with_host_and_out(ctx, entry, layout):
    h, d, torch = ctx.h, ctx.d, ctx.torch
    _, host_fn, opts, per_pos, left_out = SITE_ENTRIES[entry]
    exp = getattr(ctx.engine, host_fn)(h['lscore1'], h['row_off'] if layout == 'csr' else None, stride=ROW, **opts)
    call = lambda out=None: _site(ctx, entry, d['lscore1'], off=d['row_off'] if layout == 'csr' else None, stride=ROW, out=out)
    first = call()
    assert_same_dict(ctx.host(first), exp)
    assert exp['n_valid'].sum() == np.isfinite(h['lscore1']).sum() and np.isfinite(exp[per_pos]).any()
    again = call(sentinel(first, torch))
    assert again is first and all(again[k] is first[k] for k in exp)
    assert_same_dict(ctx.host(again), exp)
    bad = [dict(first, **{per_pos: first[per_pos].float()}), dict(first, n_valid=torch.cat([first['n_valid'], first['n_valid'][:1]])),
           dict(first, n_valid=first['n_valid'].cpu()), {k: v for k, v in first.items() if k != left_out}]
    for out in bad:
        with pytest.raises(ValueError):
            call(out)


# ---------------------------------------------------------------------------------------------------------------- site_diff
DIFF_LAYOUTS = {'csr': (True, True), 'stride': (False, False), 'csr_and_stride': (True, False), 'stride_and_csr': (False, True)}


def _diff(ctx, layout='csr', interval=True, **kw):
    d = ctx.d
    csr0, csr1 = DIFF_LAYOUTS[layout]
    a = dict(score0=d['lscore0'], score1=d['lscore1'], off0=d['row_off'] if csr0 else None, off1=d['row_off'] if csr1 else None, out=None, npos=None)
    a.update(kw)
    return ctx.det.site_diff(a['score0'], a['score1'], off0=a['off0'], off1=a['off1'], stride0=ROW, stride1=ROW, npos=a['npos'], min_valid=2,
                             interval=interval, out=a['out'])


@pytest.mark.parametrize('name', ['score0', 'score1'])
@pytest.mark.parametrize('way', WAYS)
def test_site_diff_refuses(ctx, way, name):
    score = wrong(ctx.d['l' + name], ctx.torch)[way]
    with pytest.raises(ValueError):                                       # ('length': 41 scores are no 5 rows of 10)
        _diff(ctx, 'stride', **{name: score, 'npos': NPOS + 1 if way == 'length' else None})


@pytest.mark.parametrize('name', ['off0', 'off1'])
@pytest.mark.parametrize('way', WAYS)
def test_site_diff_refuses_off(ctx, way, name):
    with pytest.raises(ValueError):                                       # ('length': the two samples no longer hold the same sites)
        _diff(ctx, 'csr', **{name: wrong(ctx.d['row_off'], ctx.torch)[way]})


def test_site_diff_two_dimensions(ctx):
    for name in ('score0', 'score1'):
        with pytest.raises(ValueError):                                   # site_diff asks for dim() == 1 of the scores ...
            _diff(ctx, 'stride', **{name: two_dim(ctx.d['l' + name])})
    exp = ctx.engine.site_diff_host(ctx.h['lscore0'], ctx.h['row_off'], ctx.h['lscore1'], ctx.h['row_off'], min_valid=2)
    got = _diff(ctx, 'csr', off0=ctx.d['row_off'].view(1, NPOS + 1), off1=ctx.d['row_off'].view(NPOS + 1, 1))   # ... not of the offsets
    assert_same_dict(ctx.host(got), exp)


@pytest.mark.parametrize('interval', [True, False])
@pytest.mark.parametrize('layout', list(DIFF_LAYOUTS))
def test_site_diff_agrees_with_host_and_out(ctx, layout, interval):
    h, torch = ctx.h, ctx.torch
    csr0, csr1 = DIFF_LAYOUTS[layout]
    exp = ctx.engine.site_diff_host(h['lscore0'], h['row_off'] if csr0 else None, h['lscore1'], h['row_off'] if csr1 else None, stride0=ROW,
                                    stride1=ROW, min_valid=2, interval=interval)
    first = _diff(ctx, layout, interval)
    assert_same_dict(ctx.host(first), exp)
    assert ('delta_lo' in exp) == ('delta_hi' in exp) == interval and np.isfinite(exp['p_diff']).any() and np.nanmin(exp['p_diff']) < 0.05
    again = _diff(ctx, layout, interval, out=sentinel(first, torch))
    assert again is first and all(again[k] is first[k] for k in exp)
    assert_same_dict(ctx.host(again), exp)
    bad = [dict(first, p_diff=first['p_diff'].float()), dict(first, iters=torch.cat([first['iters'], first['iters'][:1]])),
           dict(first, status=first['status'].cpu()), {k: v for k, v in first.items() if k != 'pi_pool'}]
    if interval:
        bad.append({k: v for k, v in first.items() if k != 'delta_hi'})
    for out in bad:
        with pytest.raises(ValueError):
            _diff(ctx, layout, interval, out=out)
