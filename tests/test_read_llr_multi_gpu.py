"""nmod_read_llr_multi (K26) on the GPU: every llr and llr_win plane bit-equal to nmod_read_llr on the pair (model, alt[m - 1]), the joint
call and the counts equal to tests/multi_ref.py integer for integer, the posterior within K13's p_mod gates, the independence of a
read's bits from the batch, the order, the memspace and the outputs asked for, and the C-level refusals."""
import functools

import numpy as np
import pytest

import multi_ref as M
import read_batch_cases as B
import readllr_ref as F
import rescale_ref as R
from nanomod_amd import _lib as L, engine        # (engine.read_llr_multi_host: without K26 this import chain fails below)
from test_read_llr_multi import INVALID, c_call, refused_c_cases

assert hasattr(engine, 'read_llr_multi_host')

pytestmark = pytest.mark.gpu

EVENT_FIELDS = ('llr', 'llr_win', 'post', 'call')
READ_FIELDS = ('n_sites', 'n_can', 'n_mod', 'status')


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _det():
    from nanomod_amd import DeviceDetector
    return DeviceDetector(0)


def _t(x):
    return _torch().from_numpy(np.array(x)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _np(res):
    return {f: v.cpu().numpy() for f, v in res.items()}


def _device_args(p):
    return (_t(p['val']), _t(p['off']), _t(R.as_bytes(p['base'])), _t(p['mean']), _t(p['sd']))


def _multi(p, k, center, window, n_alt, want=EVENT_FIELDS, args=None, **kw):
    args = _device_args(p) if args is None else args
    alts = p['alts'][:n_alt]
    return _det().read_llr_multi(*args, [_t(a[0]) for a in alts], [_t(a[1]) for a in alts], k, center, window=window, thr=M.PARITY_THR,
                                 prior_logit=M.PARITY_PRIORS[:n_alt], want=want, **kw)


@functools.lru_cache(maxsize=None)
def _k13(k, center, window, dtype, m):
    """DeviceDetector.read_llr on the parity reads against alt m alone: its llr, llr_win and p_mod as numpy"""
    p = M.parity_inputs(k, center, window, dtype)
    mean1, sd1 = p['alts'][m]
    res = _det().read_llr(*_device_args(p), _t(mean1), _t(sd1), k, center, window=window, thr=M.PARITY_THR, prior_logit=M.PARITY_PRIORS[m])
    return _np(res)


@functools.lru_cache(maxsize=None)
def _run(n_alt, k, center, window, dtype):
    return _np(_multi(M.parity_inputs(k, center, window, dtype), k, center, window, n_alt))


@pytest.mark.parametrize('n_alt,k,center,window,dtype', M.parity_cases())
def test_planes_are_k13s_bits_and_the_joint_call_is_the_restated_one(n_alt, k, center, window, dtype):
    """1. every llr and llr_win plane holds the bits DeviceDetector.read_llr writes for (model, alt[m - 1]) on the same reads: both kernel
    forms (reads up to and beyond NMOD_CALLS_WAVE_MAX, one of 3 tiles per wave), both table placements, windows (0, 0), the k-mer cover and
    (64, 64), NaN entries that differ between the tables.  2. call, n_sites, n_can and n_mod are multi_ref's on those planes, integer for
    integer (the planes being bit-equal, the restated rule sees the device's own sums: no threshold margin is needed)"""
    p = M.parity_inputs(k, center, window, dtype)
    got = _run(n_alt, k, center, window, dtype)
    assert got['llr'].shape == got['llr_win'].shape == (n_alt, len(p['val'])) and got['post'].shape == (n_alt + 1, len(p['val']))
    for m in range(n_alt):
        one = _k13(k, center, window, dtype, m)
        assert _bits(got['llr'][m]) == _bits(one['llr']), 'llr plane %d' % m
        assert _bits(got['llr_win'][m]) == _bits(one['llr_win']), 'llr_win plane %d' % m
        if window == (0, 0):
            assert _bits(got['llr_win'][m]) == _bits(got['llr'][m])
    open_ = ~np.isnan(got['llr_win'])
    assert n_alt == 1 or k < 2 or (open_.any(axis=0) & ~open_.all(axis=0)).any()          # the open sets differ along the reads
    exp = M.joint(got['llr_win'], p['off'], M.PARITY_THR, M.PARITY_PRIORS[:n_alt])
    assert got['call'].dtype == np.uint8 and np.array_equal(got['call'], exp['call'])
    for f in ('n_sites', 'n_can', 'n_mod'):
        assert got[f].dtype == np.int32 and np.array_equal(got[f], exp[f]), f
    assert not got['status'].any() and set(exp['call'].tolist()) >= {0, 1, M.AMBIGUOUS}
    if n_alt == 1:                                                           # K13's own counts
        one = _k13(k, center, window, dtype, 0)
        assert np.array_equal(got['n_mod'][0], one['n_mod']) and np.array_equal(got['n_can'], one['n_can']) and np.array_equal(got['n_sites'], one['n_sites'])


POST_CASES = [c for c in M.parity_cases() if c[4] == ('int16', 'float32', 'float64')[(c[0] + c[1]) % 3]]


@pytest.mark.parametrize('n_alt,k,center,window,dtype', POST_CASES)
def test_posterior_within_k13s_gates(n_alt, k, center, window, dtype):
    """3. post against the restatement: every plane within the sum of readllr_ref.gate_L over the open planes + GATE_P_EXTRA, relative
    (absolute DBL_MIN below DBL_MIN), the NaN pattern and the zeros of closed states identical, the planes summing to 1 within 4 ulp; at
    n_alt = 1 plane 1 within K13's gate of K13's p_mod on the device"""
    p = M.parity_inputs(k, center, window, dtype)
    got = _run(n_alt, k, center, window, dtype)
    exp = M.restate(p['val'], p['off'], p['base'], k, center, p['mean'], p['sd'], p['alts'][:n_alt], window, M.PARITY_THR, M.PARITY_PRIORS[:n_alt])
    assert np.array_equal(np.isnan(got['post']), np.isnan(exp['post']))
    ok = ~np.isnan(exp['post'][0])
    assert np.abs(got['post'][:, ok].sum(axis=0) - 1.0).max() <= 4 * 2.0 ** -52
    assert np.array_equal(got['post'][:, ok] == 0.0, exp['post'][:, ok] == 0.0) or (exp['post'][:, ok] < F.DBL_MIN).any()
    g, e, gate = got['post'][:, ok], exp['post'][:, ok], exp['gate_post'][:, ok]
    tiny = e < F.DBL_MIN
    assert (np.abs(g[tiny] - e[tiny]) <= F.DBL_MIN).all()
    ratio = float((np.abs(g[~tiny] - e[~tiny]) / (gate[~tiny] * e[~tiny])).max())
    print('post: worst deviation %.3g of its gate' % ratio)
    assert ratio <= 1.0 and ((g >= 0.0) & (g <= 1.0)).all()
    closed = np.isnan(got['llr_win'])[:, ok]
    assert (g[1:][closed] == 0.0).all()
    if n_alt == 1:
        one = _k13(k, center, window, dtype, 0)
        pm, q = one['p_mod'][ok], got['post'][1, ok]
        big = pm >= F.DBL_MIN
        assert (np.abs(q[big] - pm[big]) <= (exp['gate_L'][0, ok][big] + F.GATE_P_EXTRA) * pm[big]).all() and (np.abs(q[~big] - pm[~big]) <= F.DBL_MIN).all()


def _short_heavy_index(off, cus, seed=3):
    """read_batch_cases.batch_index's 'mixed' batch with the short reads drawn mostly from those of up to 65 events: more than twice as
    many reads of each class as the largest grid has units for it, every distinct read present, in a seeded order"""
    lens = np.diff(np.asarray(off, np.int64))
    rng = np.random.default_rng(seed)
    short, long_ = np.flatnonzero(lens <= B.WAVE_MAX), np.flatnonzero(lens > B.WAVE_MAX)
    parts = [B._draw_ids(rng, short, 2 * B.short_units(cus) + 37, np.where(lens[short] <= 65, 1.0, 0.02)),
             B._draw_ids(rng, long_, 2 * B.long_units(cus) + 5, np.where(lens[long_] == B.WAVE_MAX + 1, 1.0, 0.05))]
    return rng.permutation(np.concatenate(parts))


@pytest.mark.parametrize('n_alt,k,center,window,dtype', [(2, 3, 1, (1, 1), 'int16'), (3, 3, 1, (64, 64), 'float32')])
def test_bits_do_not_depend_on_the_batch_or_the_order(n_alt, k, center, window, dtype):
    """4a. a batch of more reads of each class than twice the persistent grid, the distinct reads in a seeded order: every read's bits are
    those of the distinct batch, gathered (read_batch_cases' pattern)"""
    torch = _torch()
    p = M.parity_inputs(k, center, window, dtype)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    idx = _short_heavy_index(p['off'], cus)
    b = B.tile_batch(p['val'], p['off'], p['base'], idx)
    n_short, n_long = B.class_counts(b['off'])
    assert n_short > 2 * B.BLOCKS_PER_CU * B.WAVES_PER_BLOCK * cus and n_long > 2 * B.BLOCKS_PER_CU * cus
    print('batch at %d CUs: %d short + %d long read(s), %d event(s)' % (cus, n_short, n_long, int(b['off'][-1])))
    want = ('llr_win', 'call')
    small = _multi(p, k, center, window, n_alt, want=want)
    big = _multi(dict(p, val=b['val'], off=b['off'], base=b['base']), k, center, window, n_alt, want=want)
    idx_t, ev_t = _t(b['idx']), _t(b['ev'])
    assert torch.equal(big['llr_win'].view(torch.int64), small['llr_win'].view(torch.int64)[:, ev_t])
    assert torch.equal(big['call'], small['call'][ev_t])
    assert torch.equal(big['n_mod'], small['n_mod'][:, idx_t])
    for f in ('n_sites', 'n_can', 'status'):
        assert torch.equal(big[f], small[f][idx_t]), f
    assert set(big) == set(want) | set(READ_FIELDS)


@pytest.mark.parametrize('n_alt,k,center,window,dtype', [(1, 5, 2, (2, 2), 'float32'), (2, 4, 1, (1, 2), 'int16'), (4, 3, 1, (64, 64), 'float64')])
def test_bits_do_not_depend_on_memspace_or_requested_outputs(n_alt, k, center, window, dtype):
    """4b. the host entry, a batch of one read of either class, fewer outputs, a side stream and an `out` dict give the bits of the first
    call; a plane outside the reads keeps what it held"""
    torch = _torch()
    p = M.parity_inputs(k, center, window, dtype)
    first = _run(n_alt, k, center, window, dtype)
    m0 = dict(k=k, center=center, mean=p['mean'], sd=p['sd'])
    alts = [dict(k=k, center=center, mean=a[0], sd=a[1]) for a in p['alts'][:n_alt]]
    kw = dict(window=window, thr=M.PARITY_THR, prior_logit=M.PARITY_PRIORS[:n_alt])
    host = engine.read_llr_multi_host(p['val'], p['off'], p['base'], m0, alts, **kw)
    assert set(host) == set(first) and all(host[f].dtype == first[f].dtype and _bits(host[f]) == _bits(first[f]) for f in first)
    nreads = len(p['off']) - 1
    for i in (nreads - 1, 4):                                                # a batch of one: the workgroup form, the wave form
        a, b = int(p['off'][i]), int(p['off'][i + 1])
        one = engine.read_llr_multi_host(p['val'][a:b], np.array([0, b - a], np.int64), p['base'][a:b], m0, alts, **kw)
        assert all(_bits(one[f]) == _bits(first[f][..., a:b]) for f in EVENT_FIELDS) and all(_bits(one[f]) == _bits(first[f][..., i:i + 1]) for f in READ_FIELDS)
    shifted = engine.read_llr_multi_host(np.concatenate([p['val'][:7], p['val'], p['val'][:3]]), p['off'] + 7, np.concatenate([p['base'][:7], p['base'], p['base'][:3]]),
                                         m0, alts, **kw)                     # events before the first read and after the last belong to no read
    assert all(_bits(shifted[f][..., 7:-3]) == _bits(first[f]) for f in EVENT_FIELDS)
    assert np.isnan(shifted['post'][:, :7]).all() and np.isnan(shifted['llr'][:, -3:]).all() and (shifted['call'][:7] == M.NONE).all()
    for want in (('llr_win',), ('call',), ('post', 'llr'), ()):
        only = _np(_multi(p, k, center, window, n_alt, want=want))
        assert set(only) == set(want) | set(READ_FIELDS) and all(_bits(only[f]) == _bits(first[f]) for f in only), want
    with torch.cuda.stream(torch.cuda.Stream()):
        side = _multi(p, k, center, window, n_alt, want=('llr_win', 'post'))
        torch.cuda.current_stream().synchronize()
    assert all(_bits(v.cpu().numpy()) == _bits(first[f]) for f, v in side.items())
    out = _multi(p, k, center, window, n_alt)
    for f in EVENT_FIELDS:
        out[f].zero_()
    again = _multi(p, k, center, window, n_alt, out=out)
    assert again is out and all(_bits(out[f].cpu().numpy()) == _bits(first[f]) for f in first)
    args = _device_args(p)
    for bad in (dict(window=(65, 0)), dict(thr=0.0), dict(want=('p_mod',)), dict(prior_logit=(701.0,) * n_alt), dict(prior_logit=(0.0,) * (n_alt + 1)),
                dict(out=dict(out, status=out['status'][:3]))):
        with pytest.raises(ValueError):
            _det().read_llr_multi(*args, [_t(a[0]) for a in p['alts'][:n_alt]], [_t(a[1]) for a in p['alts'][:n_alt]], k, center, **dict(kw, **bad))
    with pytest.raises(ValueError):
        _det().read_llr_multi(*args, [_t(p['alts'][0][0])], [_t(p['alts'][0][1][:-1])], k, center)


def test_a_read_beyond_max_deep_is_too_large():
    """2^24 events: one more than NMOD_MAX_DEEP.  The read gets NaN planes, NONE calls, zero counts and its status; its neighbour is called"""
    k, center = 3, 1
    p = M.parity_inputs(k, center, (1, 1), 'int16')
    a, b = int(p['off'][3]), int(p['off'][4])
    n = M.MAX_DEEP + 1
    val = np.concatenate([(np.arange(n, dtype=np.int64) % 2001 - 1000).astype(np.int16), p['val'][a:b]])
    base = np.concatenate([np.tile(np.frombuffer(b'ACGTTGCA', np.uint8), n // 8), R.as_bytes(p['base'])[a:b]])
    off = np.array([0, n, n + b - a], np.int64)
    got = _np(_det().read_llr_multi(_t(val), _t(off), _t(base), _t(p['mean']), _t(p['sd']), [_t(p['alts'][0][0])], [_t(p['alts'][0][1])], k, center,
                                    window=(1, 1), thr=M.PARITY_THR, want=('llr_win', 'call')))
    ref = _np(_multi(p, k, center, (1, 1), 1, want=('llr_win', 'call')))
    assert got['status'].tolist() == [M.TOO_LARGE, 0] and got['n_sites'][0] == 0 and got['n_can'][0] == 0 and got['n_mod'][0, 0] == 0
    assert np.isnan(got['llr_win'][0, :n]).all() and (got['call'][:n] == M.NONE).all()
    assert _bits(got['llr_win'][0, n:]) == _bits(ref['llr_win'][0, a:b]) and got['n_sites'][1] == ref['n_sites'][3]


def test_c_entry_refuses_invalid_arguments():
    """5. every refusal of the header returns NMOD_ERR_INVALID_ARG on a device that exists (and the well-formed call runs)"""
    lib = L.load()
    assert c_call(lib, device=0) == 0 and c_call(lib, device=0, n_alt=4) == 0 and c_call(lib, 0, device=0) == 0
    for name, kw in refused_c_cases():
        kw = dict(kw)
        assert c_call(lib, kw.pop('nreads', 3), device=0, **kw) == INVALID, name
