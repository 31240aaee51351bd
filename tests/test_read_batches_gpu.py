"""K11 (nmod_rescale_reads), K12 (nmod_read_calls) and K13 (nmod_read_llr) on batches larger than their grids
(tests/read_batch_cases.py): every wave and workgroup of the persistent kernels goes round its ticket loop at least twice with real
work, many waves fill the work lists at once with partial ballot masks, and one batch per entry makes the classify kernel take a second
stride.  A batch is a small set of distinct
reads repeated in a seeded order, so its expected outputs are the distinct reads' outputs gathered — from the restatements through the
gates of the neighbouring GPU files, and bit for bit from the device's own outputs on the distinct reads.  Every output tensor is
filled with a sentinel byte before the call: a read that no unit took would keep it.  The measured times: profiles/read_batches.txt."""
import numpy as np
import pytest

import read_batch_cases as B
import rescale_ref as R
import test_read_calls_gpu as TC                  # K12's checker and gate, as they are
import test_read_llr_gpu as TL                    # K13's checker and gates, as they are
import test_rescale_gpu as TR                     # K11's checker and gate, as they are

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
RESCALE_CASES = [(3, 1, 'int16'), (6, 2, 'float32'), (3, 1, 'float64')]                  # the LDS table, the table through L2, the LDS table
CALLS_KD = [(3, 1, 'int16'), (6, 2, 'float32')]                                          # the LDS table, the table through L2
LLR_KD = [(3, 1, 'int16'), (6, 2, 'float32')]                                            # the LDS table, the table through L2


def _torch():
    import torch
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _det():
    from nanomod_amd import DeviceDetector
    return DeviceDetector(0)


def _t(x):
    return _torch().from_numpy(np.array(x)).cuda()


def _ints(t):
    torch = _torch()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _filled(shapes):
    """CUDA tensors of the given (dtype, length), every byte the sentinel"""
    torch = _torch()
    out = {}
    for name, (dt, m) in shapes.items():
        out[name] = torch.empty(m, dtype=dt, device='cuda:0')
        out[name].view(torch.uint8).fill_(SENTINEL)
    return out


def _assert_no_sentinel(res, names):
    torch = _torch()
    for f in names:
        word = _ints(torch.full((res[f].element_size(),), SENTINEL, dtype=torch.uint8, device='cuda:0').view(res[f].dtype))
        left = int((_ints(res[f]) == word).sum())
        assert left == 0, '%s: %d of %d element(s) still hold the sentinel' % (f, left, res[f].numel())


def _assert_gathered_bits(big, small, idx_t, ev_t, read_fields, event_fields):
    """the batch's outputs are, bit for bit, the device's outputs on the distinct reads, gathered"""
    torch = _torch()
    for f in read_fields:
        assert torch.equal(_ints(big[f]), _ints(small[f])[idx_t]), '%s differs from the distinct batch' % f
    for f in event_fields:
        assert torch.equal(_ints(big[f]), _ints(small[f])[ev_t]), '%s differs from the distinct batch' % f


def _guard(off, kind, cus):
    """the batch has more than twice as many reads of each class it is about as the largest grid has units for the class (B.BLOCKS_PER_CU
    is K11's cap, above K12's 2 and rl_launch's 5 a CU)"""
    n_short, n_long = B.class_counts(off)
    if kind in ('short', 'mixed'):
        assert n_short > 2 * B.BLOCKS_PER_CU * B.WAVES_PER_BLOCK * cus, (n_short, cus)
    if kind in ('long', 'mixed'):
        assert n_long > 2 * B.BLOCKS_PER_CU * cus, (n_long, cus)
    if kind == 'classify':
        assert n_short + n_long > B.CLASSIFY_READS_PER_CU * cus and n_long > 0, (n_short, n_long, cus)
        lens = np.diff(off)
        assert np.flatnonzero(lens > B.WAVE_MAX).min() >= B.CLASSIFY_READS_PER_CU * cus
    print('%s batch at %d CUs: %d short + %d long read(s), %d event(s)' % (kind, cus, n_short, n_long, int(off[-1])))


def _batch(d, kind, cus):
    idx = B.classify_index(d['off'], cus) if kind == 'classify' else B.batch_index(d['off'], kind, cus)
    b = B.tile_batch(d['val'], d['off'], d['base'], idx)
    _guard(b['off'], kind, cus)
    return b


# ------------------------------------------------------------------------------------------------------------------------------ K11

class _Rescale:
    """the distinct reads of one K11 case on the device, and calls with sentinel-filled outputs"""

    def __init__(self, k, center, dtype):
        self.k, self.center, self.dtype = k, center, dtype
        self.d = B.rescale_distinct(k, center, dtype)
        self.det = _det()
        self.mean, self.sd = _t(self.d['mean']), _t(self.d['sd'])

    def upload(self, b):
        return _t(b['val']), _t(b['off']), _t(b['base'])

    def call(self, dev, mode='fit_apply', fitted=None):
        torch = _torch()
        val, off, base = dev
        nreads = off.numel() - 1
        shapes = dict(n_used=(torch.int32, nreads), status=(torch.uint8, nreads))
        if mode != 'apply_only':
            shapes.update(shift=(torch.float64, nreads), scale=(torch.float64, nreads))
        if mode != 'fit_only':
            shapes['val'] = (val.dtype, val.numel())
        out = _filled(shapes)
        kw = {}
        if mode == 'apply_only':                                                # shift and scale are inputs here
            out.update(shift=fitted['shift'], scale=fitted['scale'])
            kw = dict(shift=fitted['shift'], scale=fitted['scale'])
        res = self.det.rescale_reads(val, off, base, self.mean, self.sd, self.k, self.center, mode=mode, min_events=B.RESCALE_MIN_EVENTS,
                                     out=out, **kw)
        assert res is out
        _assert_no_sentinel(res, shapes)
        return res


def _rescale_case(kind, k, center, dtype, host=False):
    c = _Rescale(k, center, dtype)
    b = _batch(c.d, kind, _cus())
    small = c.call(c.upload(c.d))
    dev = c.upload(b)
    big = c.call(dev)
    idx_t, ev_t = _t(b['idx']), _t(b['ev'])
    _assert_gathered_bits(big, small, idx_t, ev_t, B.RESCALE_FIELDS, ('val',))
    got = {f: big[f].cpu().numpy() for f in B.RESCALE_FIELDS + ('val',)}
    exp_small = B.rescale_expected(k, center, dtype)
    assert not (dtype == 'int16' and (exp_small['val'] == np.array([0xA5A5], np.uint16).view(np.int16)[0]).any())
    TR._check_against(got, B.rescale_gather(exp_small, b['idx'], b['ev']), dtype)
    if host:
        model = dict(k=k, center=center, mean=c.d['mean'], sd=c.d['sd'])
        h = TR._engine().rescale_reads_host(b['val'], b['off'], b['base'], model, min_events=B.RESCALE_MIN_EVENTS)
        for f in B.RESCALE_FIELDS + ('val',):
            assert h[f].dtype == got[f].dtype and TR._bits(h[f]) == TR._bits(got[f]), 'host entry: %s' % f
    return c, b, dev, big, idx_t, ev_t


@pytest.mark.parametrize('k,center,dtype', RESCALE_CASES)
@pytest.mark.parametrize('kind', ['short', 'long', 'mixed'])
def test_rescale_batches_beyond_the_grid(kind, k, center, dtype):
    _rescale_case(kind, k, center, dtype)


def test_rescale_fit_only_then_apply_only_on_the_long_batch():
    """the two halves on the long int16 batch give the bits of fit_apply: the fit without the CLAMPED bit, the apply step with nothing
    else; a failed read passes (0, 1) on and comes back unchanged"""
    torch = _torch()
    c, b, dev, both, idx_t, ev_t = _rescale_case('long', 3, 1, 'int16')
    fit = c.call(dev, mode='fit_only')
    assert 'val' not in fit and all(torch.equal(_ints(fit[f]), _ints(both[f])) for f in ('shift', 'scale', 'n_used'))
    assert torch.equal(fit['status'], both['status'] & (0xFF ^ R.CLAMPED))
    shift, scale = fit['shift'].clone(), fit['scale'].clone()
    app = c.call(dev, mode='apply_only', fitted=fit)
    assert torch.equal(app['val'], both['val']) and torch.equal(app['status'], both['status'] & R.CLAMPED) and not bool(app['n_used'].any())
    assert torch.equal(_ints(app['shift']), _ints(shift)) and torch.equal(_ints(app['scale']), _ints(scale))       # inputs, left as they are
    st = both['status'].cpu().numpy()
    assert (st == R.CLAMPED).any() and (st == R.TOO_FEW).any() and (st == R.DEGENERATE).any() and (st == R.OUT_OF_RANGE).any()
    small_fit = c.call(c.upload(c.d), mode='fit_only')
    _assert_gathered_bits(fit, small_fit, idx_t, ev_t, B.RESCALE_FIELDS, ())


def test_rescale_host_entry_on_the_mixed_batch():
    _rescale_case('mixed', 3, 1, 'int16', host=True)


def test_rescale_classify_takes_a_second_stride():
    """more reads than the classify grid covers in one pass, nearly all of them tiny, the long ones beyond the first stride"""
    c = _Rescale(3, 1, 'int16')
    b = _batch(c.d, 'classify', _cus())
    small = c.call(c.upload(c.d))
    big = c.call(c.upload(b))
    _assert_gathered_bits(big, small, _t(b['idx']), _t(b['ev']), B.RESCALE_FIELDS, ('val',))
    st = big['status'].cpu().numpy()
    assert np.array_equal(st, B.rescale_expected(3, 1, 'int16')['status'][b['idx']])


# ------------------------------------------------------------------------------------------------------------------------------ K12

class _Calls:
    def __init__(self, k, center, nb, dtype):
        self.k, self.center, self.nb, self.dtype = k, center, nb, dtype
        self.d = B.calls_distinct(k, center, nb, dtype)
        self.det = _det()
        self.mean, self.sd = _t(self.d['mean']), _t(self.d['sd'])

    def call(self, b, want=B.CALLS_EVENT_FIELDS):
        torch = _torch()
        val, off, base = _t(b['val']), _t(b['off']), _t(b['base'])
        nreads = off.numel() - 1
        shapes = {w: (torch.float64, val.numel()) for w in want}
        shapes.update(n_sites=(torch.int32, nreads), n_called=(torch.int32, nreads), status=(torch.uint8, nreads))
        out = _filled(shapes)
        res = self.det.read_calls(val, off, base, self.mean, self.sd, self.k, self.center, nb=self.nb, alpha=B.CALLS_ALPHA, want=want, out=out)
        assert res is out
        _assert_no_sentinel(res, shapes)
        return res


def _calls_case(kind, k, center, nb, dtype, host=False):
    c = _Calls(k, center, nb, dtype)
    b = _batch(c.d, kind, _cus())
    small = c.call(c.d)
    big = c.call(b)
    _assert_gathered_bits(big, small, _t(b['idx']), _t(b['ev']), B.CALLS_READ_FIELDS, B.CALLS_EVENT_FIELDS)
    got = {f: big[f].cpu().numpy() for f in B.CALLS_READ_FIELDS + B.CALLS_EVENT_FIELDS}
    del big
    TC._check_against(got, B.calls_gather(B.calls_expected(k, center, nb, dtype), b['idx'], b['ev']))
    if nb == 0:
        assert TC._bits(got['p_win']) == TC._bits(got['p'])
    if host:
        model = dict(k=k, center=center, mean=c.d['mean'], sd=c.d['sd'])
        h = TC._engine().read_calls_host(b['val'], b['off'], b['base'], model, nb=nb, alpha=B.CALLS_ALPHA)
        for f in B.CALLS_READ_FIELDS + B.CALLS_EVENT_FIELDS:
            assert h[f].dtype == got[f].dtype and TC._bits(h[f]) == TC._bits(got[f]), 'host entry: %s' % f


@pytest.mark.parametrize('k,center,dtype', CALLS_KD)
@pytest.mark.parametrize('nb', [0, 2, 64])
def test_calls_short_batch_beyond_the_grid(nb, k, center, dtype):
    _calls_case('short', k, center, nb, dtype)


@pytest.mark.parametrize('k,center,dtype', CALLS_KD)
@pytest.mark.parametrize('nb', [2, 64])
@pytest.mark.parametrize('kind', ['long', 'mixed'])
def test_calls_long_and_mixed_batches_beyond_the_grid(kind, nb, k, center, dtype):
    _calls_case(kind, k, center, nb, dtype)


def test_calls_host_entry_on_the_mixed_batch():
    _calls_case('mixed', 3, 1, 2, 'int16', host=True)


def test_calls_classify_takes_a_second_stride():
    c = _Calls(3, 1, 2, 'int16')
    b = _batch(c.d, 'classify', _cus())
    small = c.call(c.d)
    big = c.call(b)
    _assert_gathered_bits(big, small, _t(b['idx']), _t(b['ev']), B.CALLS_READ_FIELDS, B.CALLS_EVENT_FIELDS)
    exp = B.calls_expected(3, 1, 2, 'int16')
    for f in B.CALLS_READ_FIELDS:
        assert np.array_equal(big[f].cpu().numpy(), exp[f][b['idx']]), f


# ------------------------------------------------------------------------------------------------------------------------------ K13

class _Llr:
    def __init__(self, k, center, window, dtype):
        self.k, self.center, self.window, self.dtype = k, center, window, dtype
        self.d = B.llr_distinct(k, center, window, dtype)
        self.det = _det()
        self.models = [_t(self.d[f]) for f in ('mean', 'sd', 'alt_mean', 'alt_sd')]

    def call(self, b, want=B.LLR_EVENT_FIELDS):
        torch = _torch()
        val, off, base = _t(b['val']), _t(b['off']), _t(b['base'])
        nreads = off.numel() - 1
        shapes = {w: (torch.float64, val.numel()) for w in want}
        shapes.update(n_sites=(torch.int32, nreads), n_mod=(torch.int32, nreads), n_can=(torch.int32, nreads), status=(torch.uint8, nreads))
        out = _filled(shapes)
        res = self.det.read_llr(val, off, base, *self.models, self.k, self.center, window=self.window, thr=B.LLR_THR,
                                prior_logit=B.LLR_PRIOR_LOGIT, want=want, out=out)
        assert res is out
        _assert_no_sentinel(res, shapes)
        return res


def _llr_case(kind, k, center, window, dtype, host=False):
    c = _Llr(k, center, window, dtype)
    b = _batch(c.d, kind, _cus())
    small = c.call(c.d)
    big = c.call(b)
    _assert_gathered_bits(big, small, _t(b['idx']), _t(b['ev']), B.LLR_READ_FIELDS, B.LLR_EVENT_FIELDS)
    got = {f: big[f].cpu().numpy() for f in B.LLR_READ_FIELDS + B.LLR_EVENT_FIELDS}
    del big
    TL._check_against(got, B.llr_gather(B.llr_expected(k, center, window, dtype), b['idx'], b['ev']))
    if window == (0, 0):
        assert TL._bits(got['llr_win']) == TL._bits(got['llr'])
    if host:
        m0, m1 = TL._models(c.d, k, center)
        h = TL._engine().read_llr_host(b['val'], b['off'], b['base'], m0, m1, window=window, thr=B.LLR_THR, prior_logit=B.LLR_PRIOR_LOGIT)
        for f in B.LLR_READ_FIELDS + B.LLR_EVENT_FIELDS:
            assert h[f].dtype == got[f].dtype and TL._bits(h[f]) == TL._bits(got[f]), 'host entry: %s' % f


@pytest.mark.parametrize('k,center,dtype', LLR_KD)
@pytest.mark.parametrize('window', [(0, 0), (2, 0), (64, 64)])
def test_llr_short_batch_beyond_the_grid(window, k, center, dtype):
    _llr_case('short', k, center, window, dtype)


@pytest.mark.parametrize('k,center,dtype', LLR_KD)
@pytest.mark.parametrize('window', [(2, 0), (64, 64)])
@pytest.mark.parametrize('kind', ['long', 'mixed'])
def test_llr_long_and_mixed_batches_beyond_the_grid(kind, window, k, center, dtype):
    _llr_case(kind, k, center, window, dtype)


def test_llr_host_entry_on_the_mixed_batch():
    _llr_case('mixed', 3, 1, (2, 0), 'int16', host=True)


def test_llr_classify_takes_a_second_stride():
    c = _Llr(3, 1, (2, 0), 'int16')
    b = _batch(c.d, 'classify', _cus())
    small = c.call(c.d)
    big = c.call(b)
    _assert_gathered_bits(big, small, _t(b['idx']), _t(b['ev']), B.LLR_READ_FIELDS, B.LLR_EVENT_FIELDS)
    exp = B.llr_expected(3, 1, (2, 0), 'int16')
    for f in B.LLR_READ_FIELDS:
        assert np.array_equal(big[f].cpu().numpy(), exp[f][b['idx']]), f
