"""nmod_site_compose (K26) on the GPU against the numpy restatement of its definition (tests/compose_ref.py; its own checks without a
GPU: tests/test_site_compose.py): parity over every row length at which the code takes another path, n_alt = 1 against nmod_site_stoich,
the independence of a row's bits from CSR versus stride, the batch, the memspace and the outputs asked for, a row beyond NMOD_MAX_DEEP,
the C-level refusals, and the stream contract of the two K26 device entries.  The gates are those of the project's other EM with a stop
test (tests/test_mix_gpu.py): pi 1e-9 relative, ll 1e-9 relative + 1e-9 absolute, resp 2^-23 absolute."""
import functools

import numpy as np
import pytest

import compose_ref as CR
import grid_cases as G
import multi_ref as M
import stream_cases as S
from nanomod_amd import _lib as L, engine
from test_site_compose import INVALID, c_call, refused_c_cases

assert hasattr(engine, 'site_compose_host')

pytestmark = pytest.mark.gpu

INT_FIELDS = ('n_valid', 'n_partial', 'open_mask', 'status')
ALL_FIELDS = ('pi', 'll', 'stat', 'stat_m', 'p_m', 'iters', 'resp') + INT_FIELDS


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


def _close(name, got, exp, rel, abs_=0.0):
    assert np.array_equal(np.isnan(got), np.isnan(exp)), '%s: NaN pattern differs' % name
    ok = ~np.isnan(exp)
    dev = np.abs(got[ok] - exp[ok])
    gate = rel * np.abs(exp[ok]) + abs_
    worst = float((dev / np.where(gate > 0.0, gate, 1.0)).max()) if ok.any() else 0.0
    assert (dev[gate == 0.0] == 0.0).all() and worst <= 1.0, '%s: %.3g of its gate' % (name, worst)
    return worst


def _check(got, exp, off):
    """the gates of the module docstring; iters equal but where the restatement's last step lies within 1e-6 tol of tol; stat_m within the
    gates of the two ll it is the difference of; p_m is the header's function of the device's own stat_m (erfc within 1e-12 relative):
    the law jumps from 1 to 1/2 at stat_m = 0, so a p_m is compared through its stat_m, not across the jump"""
    for f in INT_FIELDS:
        assert got[f].dtype == exp[f].dtype and np.array_equal(got[f], exp[f]), f
    firm = ~exp['near_tol']
    assert np.array_equal(got['iters'][firm], exp['iters'][firm]), 'iters'
    worst = dict(pi=_close('pi', got['pi'][:, firm], exp['pi'][:, firm], CR.GATE_PI), ll=_close('ll', got['ll'][firm], exp['ll'][firm], *CR.GATE_LL),
                 stat=_close('stat', got['stat'][firm], exp['stat'][firm], CR.GATE_LL[0], 2.0 * CR.GATE_LL[1]))
    assert np.array_equal(np.isnan(got['stat_m']), np.isnan(exp['stat_m'])) and np.array_equal(np.isnan(got['p_m']), np.isnan(exp['p_m']))
    ll = np.abs(exp['ll'])[None, :]
    with np.errstate(invalid='ignore'):
        gate = 2.0 * (CR.GATE_LL[0] * (2.0 * ll + 0.5 * exp['stat_m']) + 2.0 * CR.GATE_LL[1])
        ok = ~np.isnan(exp['stat_m']) & firm[None, :]
        assert (np.abs(got['stat_m'] - exp['stat_m'])[ok] <= np.broadcast_to(gate, ok.shape)[ok]).all(), 'stat_m'
    want_p = np.array([[CR.p_boundary(float(s)) if s == s else np.nan for s in r] for r in got['stat_m']])
    _close('p_m', got['p_m'], want_p, 1e-12)
    rows = np.repeat(firm, np.diff(off))
    worst['resp'] = _close('resp', got['resp'][:, :off[-1]][:, rows], exp['resp'][:, :off[-1]][:, rows], 0.0, CR.GATE_RESP)
    print('worst deviation as a share of its gate: ' + ', '.join('%s %.3g' % kv for kv in worst.items()))


@functools.lru_cache(maxsize=None)
def _expected(n_alt):
    sc, off = CR.parity_batch(n_alt)
    return CR.site_compose(sc, off, **CR.PARITY_OPTS)


@functools.lru_cache(maxsize=None)
def _host(n_alt):
    sc, off = CR.parity_batch(n_alt)
    return engine.site_compose_host(sc, off, resp=True, **CR.PARITY_OPTS)


@pytest.mark.parametrize('n_alt', [1, 2, 3, 4])
def test_parity_with_the_restatement(n_alt):
    """1. rows of 1, 2, 3, 15, 16, 17, 255, 256, 257, 1 023, 1 024, 1 025 reads and one past the LDS-resident limit of the workgroup class,
    each with every state present, with a closed state and partial reads, with a share driven to the boundary and with |s| = 700; a row of
    all-zero scores, an all-NaN row, an empty row; TOO_FEW, NO_STATE and NOT_CONVERGED among the statuses"""
    sc, off = CR.parity_batch(n_alt)
    _check(_host(n_alt), _expected(n_alt), off)


def test_one_state_agrees_with_site_stoich():
    """2. n_alt = 1 against DeviceDetector.site_stoich on the same well-separated rows at tol = 1e-12: pi within 100 tol, stat within
    100 tol relative, p_null within the gate that follows (compose_ref.p_gate).  tests/test_site_compose.py asserts that the two
    restatements meet these gates on these rows"""
    s, off = CR.stoich_rows()
    d_s, d_off = _t(s), _t(off)
    a = _np(_det().site_compose([d_s], off=d_off, max_iter=CR.MAX_ITER, tol=CR.STOICH_TOL))
    b = _np(_det().site_stoich(d_s, off=d_off, tol=CR.STOICH_TOL))
    assert not a['status'].any() and not b['status'].any()
    dev = (np.abs(a['pi'][1] - b['pi']).max(), np.abs(a['stat_m'][0] / b['stat'] - 1.0).max(),
           (np.abs(a['p_m'][0] / b['p_null'] - 1.0) / np.array([CR.p_gate(v) for v in b['stat']])).max())
    print('site_compose against site_stoich: pi %.3g, stat %.3g relative, p %.3g of its gate' % dev)
    assert dev[0] <= CR.STOICH_GATE and dev[1] <= CR.STOICH_GATE and dev[2] <= 1.0
    assert np.abs(a['pi'][0] + a['pi'][1] - 1.0).max() <= 1e-15 and np.array_equal(a['n_valid'], b['n_valid'])


@pytest.mark.parametrize('n_alt', [1, 2, 3, 4])
def test_bits_do_not_depend_on_memspace_or_requested_outputs(n_alt):
    """3a. the device entry, a side stream, an `out` dict, fewer outputs (no per-state test, no resp) and a batch of one row give the bits
    of the host call"""
    torch = _torch()
    sc, off = CR.parity_batch(n_alt)
    first = _host(n_alt)
    d_sc, d_off = [_t(s) for s in sc], _t(off)
    dev = _det().site_compose(d_sc, off=d_off, resp=True, **CR.PARITY_OPTS)
    assert set(dev) == set(ALL_FIELDS) and all(_bits(dev[f].cpu().numpy()) == _bits(first[f]) for f in ALL_FIELDS)
    with torch.cuda.stream(torch.cuda.Stream()):
        side = _det().site_compose(d_sc, off=d_off, test=False, **CR.PARITY_OPTS)
        torch.cuda.current_stream().synchronize()
    # (the refits may add NOT_CONVERGED to status: the header says so; every other output keeps its bits)
    assert set(side) == set(ALL_FIELDS) - {'stat_m', 'p_m', 'resp'}
    assert all(_bits(side[f].cpu().numpy()) == _bits(first[f]) for f in side if f != 'status')
    assert np.array_equal(side['status'].cpu().numpy() | (first['status'] & CR.NOT_CONVERGED), first['status'])
    for f in ('pi', 'll', 'resp', 'stat_m'):
        dev[f].zero_()
    again = _det().site_compose(d_sc, off=d_off, resp=True, out=dev, **CR.PARITY_OPTS)
    assert again is dev and all(_bits(dev[f].cpu().numpy()) == _bits(first[f]) for f in ALL_FIELDS)
    for i in (0, 5, 21, 37, 49, len(off) - 4):                               # a batch of one: TOO_FEW, 16 lanes, a wave, a workgroup, past the stage, zeros
        a, b = int(off[i]), int(off[i + 1])
        one = engine.site_compose_host([s[a:b] for s in sc], np.array([0, b - a], np.int64), resp=True, **CR.PARITY_OPTS)
        assert all(_bits(one[f]) == _bits(first[f][..., i:i + 1]) for f in ALL_FIELDS if f != 'resp') and _bits(one['resp']) == _bits(first['resp'][:, a:b]), i
    assert np.diff(off)[49] == CR.stage_reads(n_alt) + 1
    for bad in (dict(max_iter=0), dict(tol=-1.0), dict(min_valid=0), dict(out=dict(dev, status=dev['status'][:3]))):
        with pytest.raises(ValueError):
            _det().site_compose(d_sc, off=d_off, resp=True, **dict(CR.PARITY_OPTS, **bad))
    with pytest.raises(ValueError):
        _det().site_compose(d_sc + [d_sc[0][:-1]], off=d_off)


@pytest.mark.parametrize('stride', [3, 40, 257, 1100])
def test_csr_equals_the_stride_form(stride):
    """3b. whole rows of one length by offsets and by prm->stride0, on the host and on the device: the same bits"""
    n_alt = 3
    rng = np.random.default_rng(stride)
    rows = 24
    S = CR.simulate_rows(rng, rows, stride, [0.4, 0.3, 0.2, 0.1], sep=2.0)   # rows x n_alt x stride
    S[::5, 2, :] = np.nan
    sc = [np.ascontiguousarray(S[:, m, :]).reshape(-1) for m in range(n_alt)]
    off = np.arange(0, rows * stride + 1, stride, dtype=np.int64)
    a = engine.site_compose_host(sc, off, resp=True, **CR.PARITY_OPTS)
    b = engine.site_compose_host(sc, None, stride=stride, resp=True, **CR.PARITY_OPTS)
    d = _np(_det().site_compose([_t(s) for s in sc], stride=stride, resp=True, **CR.PARITY_OPTS))
    assert all(_bits(a[f]) == _bits(b[f]) == _bits(d[f]) for f in ALL_FIELDS)
    _check(a, CR.site_compose(sc, off, **CR.PARITY_OPTS), off)


def test_a_batch_larger_than_the_grids():
    """3c. more than twice as many rows of each class as its persistent grid has groups (tests/test_persistent_grids_gpu.py's pattern): every
    repeat of a pool row has the bits of the pool's own call"""
    torch = _torch()
    n_alt = 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(77)
    lens = [20] * 6 + [CR.SMALL + 1] * 4 + [CR.WAVE + 1] * 3 + [CR.stage_reads(n_alt) + 1]
    rows = [CR.simulate_rows(rng, 1, n, [0.5, 0.3, 0.2], sep=(1.0, 2.0, 3.0)[i % 3])[0] for i, n in enumerate(lens)]
    rows[1][1] = np.nan
    poff = np.zeros(len(rows) + 1, np.int64)
    poff[1:] = np.cumsum(lens)
    P = np.concatenate(rows, axis=1)
    cls = np.array([0] * 6 + [1] * 4 + [2] * 4)
    counts = G.grid_counts(G.stoich_units(cus))
    idx = G.class_index([np.flatnonzero(cls == k) for k in range(3)], counts, 78, [None, None, np.array([1.0, 1.0, 1.0, 0.02])])
    t = G.tile_rows(P[0], poff, idx)
    print('K26 batch at %d CUs: %s rows per class, %d scores' % (cus, counts, int(t['off'][-1])))
    opts = dict(min_valid=3, max_iter=60, tol=1e-6)
    small = _det().site_compose([_t(P[m]) for m in range(n_alt)], off=_t(poff), resp=True, **opts)
    big = _det().site_compose([_t(P[m][t['ev']]) for m in range(n_alt)], off=_t(t['off']), resp=True, **opts)
    idx_t, ev_t = _t(idx), _t(t['ev'])
    as_int = lambda x: x.view(torch.int64) if x.dtype == torch.float64 else x
    for f in ALL_FIELDS:
        assert torch.equal(as_int(big[f]), as_int(small[f])[..., ev_t if f == 'resp' else idx_t]), f
    assert not (small['status'].cpu().numpy() & CR.TOO_FEW).any()


def test_a_row_beyond_max_deep_is_too_large():
    """2^24 reads: one more than NMOD_MAX_DEEP.  The row gets NaN outputs, zero counts and its status; its neighbour is fitted"""
    n = CR.MAX_DEEP + 1
    rng = np.random.default_rng(3)
    tail = CR.simulate_rows(rng, 1, 50, [0.5, 0.5], sep=2.0)[0, 0]
    s = np.concatenate([np.zeros(n), tail])
    off = np.array([0, n, n + 50], np.int64)
    got = _np(_det().site_compose([_t(s)], off=_t(off), **CR.PARITY_OPTS))
    exp = CR.site_compose([tail], np.array([0, 50], np.int64), **CR.PARITY_OPTS)
    assert got['status'].tolist() == [CR.TOO_LARGE, 0] and got['n_valid'].tolist() == [0, 50] and got['iters'][0] == 0 and got['open_mask'][0] == 0
    assert np.isnan(got['pi'][:, 0]).all() and np.isnan(got['ll'][0]) and np.isnan(got['p_m'][0, 0])
    assert abs(got['pi'][1, 1] - exp['pi'][1, 0]) <= CR.GATE_PI * exp['pi'][1, 0] and got['iters'][1] == exp['iters'][0]


def test_c_entry_refuses_invalid_arguments():
    lib = L.load()
    assert c_call(lib, device=0) == 0 and c_call(lib, device=0, n_alt=4) == 0 and c_call(lib, 0, device=0) == 0 and c_call(lib, device=0, off=None, stride=5) == 0
    for name, kw in refused_c_cases():
        kw = dict(kw)
        assert c_call(lib, kw.pop('npos', 3), device=0, **kw) == INVALID, name


# ------------------------------------------------------------------------------------------------------------- the stream contract
# 4. The two K26 device entries enqueue on the caller's stream only, wait for nothing and read nothing back: tests/stream_cases.py's
# stall-and-decoy method through the helpers of tests/test_stream_contract_gpu.py, with builders for the new entries.

def _multi_inputs(part=1):
    d = M.parity_inputs(S.READ_K, S.READ_CENTER, (1, 1), 'float32', 2)
    n = len(d['off']) - 1
    flat = dict(val=d['val'], off=d['off'], base=d['base'], mean=d['mean'], sd=d['sd'], alt_mean0=d['alts'][0][0], alt_sd0=d['alts'][0][1],
                alt_mean1=d['alts'][1][0], alt_sd1=d['alts'][1][1])
    return S._read_inputs(flat, np.arange(n if part == 1 else n - 2), ('mean', 'sd', 'alt_mean0', 'alt_sd0', 'alt_mean1', 'alt_sd1'))


def _multi_call(det, t, out=None):
    return det.read_llr_multi(t['val'], t['off'], t['base'], t['mean'], t['sd'], [t['alt_mean0'], t['alt_mean1']], [t['alt_sd0'], t['alt_sd1']],
                              S.READ_K, S.READ_CENTER, window=(1, 1), thr=M.PARITY_THR, prior_logit=M.PARITY_PRIORS[:2], out=out)


def _compose_inputs(part=1):
    sc, off = CR.parity_batch(2)
    idx = np.arange(len(off) - 1)
    one = lambda ix, k: dict(score0=G.tile_rows(sc[k], off, ix)['val'], score1=G.tile_rows(sc[1 - k], off, ix)['val'], off=G.tile_rows(sc[0], off, ix)['off'])
    return dict(real=S._frozen(one(idx, 0)), decoy=S._frozen(one(idx[::-1], 1)), csr=(('off', 'score0'),), classes={})


def _compose_call(det, t, out=None):
    return det.site_compose([t['score0'], t['score1']], off=t['off'], resp=True, out=out, **CR.PARITY_OPTS)


BUILDERS = {'read_llr_multi': S.Builder('read_llr_multi', _multi_inputs, _multi_call, True),
            'site_compose': S.Builder('site_compose', _compose_inputs, _compose_call, True)}


@pytest.fixture(scope='module')
def env():
    from test_stream_contract_gpu import Env
    return Env()


@pytest.mark.parametrize('name', sorted(BUILDERS))
def test_entry_runs_on_its_stream_and_waits_for_nothing(env, name):
    from test_stream_contract_gpu import STREAMS_TRIED, assert_same_outputs, stalled
    b = BUILDERS[name]
    d = b.make_inputs(1)
    sw = S.Swapped(d['real'], d['decoy'])
    want, first = env.serial(b.call, sw)
    out = env.like(first)                                                 # allocated before the stall, filled behind it
    for _ in range(STREAMS_TRIED):
        got, early, stream = stalled(env, sw, lambda: b.call(env.det, sw.t, S.fill_sentinel(out)), S.T_MS)
        assert not early, '%s: the stall of %g ms had ended when the call returned' % (name, S.T_MS)
        stream.synchronize()
        assert_same_outputs(env.numpy(got), want, name)
        assert sw.holds('decoy'), name + ': the inputs were written after the trailing copy, or the copy did not run'
    other = env.numpy(b.call(env.det, sw.t, S.fill_sentinel(env.like(first))))       # what the comparison rests on: the decoy gives other results
    from test_engine_device_args_gpu import same
    changed = [k for k in want if not same(other[k], want[k])]
    assert len(changed) * 2 >= len(want), (name, changed)
