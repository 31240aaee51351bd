"""GPU: the large-position forms of K1 — big_rank_kernel<f32 | i16> (all tests and KS-only), big_rank_kernel<2> as the float64
redo, big_hist_kernel<f32 | i16>, wide_redo_kernel and the two-pass WIDE classes of rank_hist_kernel — on constructed positions
(big_cases.py; test_big_cases.py proves on the CPU that each has the property it is named for).

Per batch, as test_rank_hist_constructed_gpu.py does for the wave-resident forms: nmod_describe_dispatch names the form for every
(n0, n1), nmod_last_dispatch_stats shows that it took every position, the integers K1 leaves in the workspace equal
k1_ints.exact_ints bit for bit (mwu_s and tie wherever the form writes them; ks_num for big_hist_kernel, the WIDE classes and
KS-only runs — big_rank_kernel with all tests writes the float form of D only, checked through ks_d), status, ks_d and mwu_u equal
the oracle's, every other track passes the project's bars (helpers.compare_outputs, helpers.t_abs_gate), CSR and — uniform
batches — fixed stride, and detect_host returns the device run's bytes.  int16 and on-grid batches of the WIDE classes run with
NMOD_FLAG_NO_COUNTING | NMOD_FLAG_NO_COUNT_WIDE and once more without: same bytes.

The persistent loops: every launch here gives a block more than one position only when the list is longer than its grid
(4 x CUs blocks for big_rank_kernel and the float64 redo, 2 x CUs for big_hist_kernel and wide_redo_kernel), so one test per
launch runs 2 G + 64 positions ordered so that a block's consecutive positions differ in family and size."""
import ctypes as C
import time

import numpy as np
import pytest

import big_cases as B
import helpers as H
import hist_cases as HC
import k1_ints as K

pytestmark = pytest.mark.gpu

ALL_TRACKS = ('mwu_u', 'mwu_p', 't_t', 't_p', 'ks_d', 'ks_p', 'comb_st', 'comb_p', 'status')
KS_TRACKS = ('ks_d', 'ks_p', 'comb_st', 'comb_p', 'status')


@pytest.fixture(scope='module')
def env():
    import torch
    import nanomod_amd as nm
    import nanomod_oracle
    import oracle_c
    L = nm._lib
    assert L.load().nmod_device_count() > 0
    return {'torch': torch, 'nm': nm, 'L': L, 'oracle': oracle_c, 'orc': nanomod_oracle, 'det': {},
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}


def _detector(env, ks_only, flags):
    key = (ks_only, flags)
    if key not in env['det']:
        L = env['L']
        env['det'][key] = env['nm'].DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=L.TEST_KS if ks_only else L.TEST_ALL, flags=flags)
    return env['det'][key]


def _describe(env, dtype, ks_only, flags, n0, n1):
    L = env['L']
    prm = L.make_params(dtype=L.DTYPE_I16_MILLI if dtype == 'i16' else L.DTYPE_F32, tests=L.TEST_KS if ks_only else L.TEST_ALL, flags=flags)
    buf = C.create_string_buffer(256)
    assert L.load().nmod_describe_dispatch(C.byref(prm), n0, n1, buf, 256) == 0
    return buf.value.decode()


def _exact(cases, idx, dtype):
    out = []
    for i in idx:
        memo = cases[i].setdefault('exact_ints', {})
        if dtype not in memo:
            memo[dtype] = K.exact_ints(*HC.values(cases[i], dtype))
        out.append(memo[dtype])
    return {'ks_num': np.array([e[0] for e in out], np.uint64), 'mwu_s': np.array([e[1] for e in out], np.uint64),
            'tie': np.array([e[2] for e in out], np.uint64)}


def _run_device(env, ks_only, flags, sig0, off0, sig1, off1, stride, ks_num_written, rational=False):
    torch = env['torch']
    det = _detector(env, ks_only, flags)
    npos = len(off0) - 1
    n0, n1 = np.diff(off0), np.diff(off1)
    a = torch.from_numpy(sig0).cuda(); b = torch.from_numpy(sig1).cuda()
    rid = torch.zeros(npos, dtype=torch.int32, device='cuda:0')
    if stride:
        res = det.run(a, b, rid, stride0=int(n0[0]), stride1=int(n1[0]), npos=npos)
    else:
        res = det.run(a, b, rid, off0=torch.from_numpy(off0).cuda(), off1=torch.from_numpy(off1).cuda(), npos=npos,
                      max_n0=int(n0.max()), max_n1=int(n1.max()))
    torch.cuda.synchronize()
    ints = K.read_k1_ints(det, npos, res, n0, n1, rational_d=rational, ks_num_written=ks_num_written)
    stats = det.dispatch_stats()
    return {k: res[k].cpu().numpy() for k in (KS_TRACKS if ks_only else ALL_TRACKS)}, ints, stats


def _oracle(env, sig0, off0, sig1, off1, ks_only):
    rid = np.zeros(len(off0) - 1, np.int32)
    if sig0.dtype == np.float64:                                             # (the C restatement takes float32 and int16 only)
        orc = env['orc']
        with np.errstate(all='ignore'):
            exp = orc.detect_batch(sig0, off0, sig1, off1, rid, 2, 2.0, orc.METHOD_STOUFFER)
        if ks_only:                                                          # neither Mann-Whitney nor Welch runs: their status bits stay clear
            exp = dict(exp, status=exp['status'] & ~np.uint8(env['L'].STATUS_MWU_ALL_IDENTICAL | env['L'].STATUS_T_NAN))
        return exp
    return env['oracle'].detect_batch(sig0, off0, sig1, off1, rid, 2, 2.0, 'stouffer', tests=1 if ks_only else 7)


def _compare_outputs(got, exp, gate, what, ks_only, rational):
    assert np.array_equal(got['status'], exp['status']), (what, np.flatnonzero(got['status'] != exp['status'])[:5])
    if rational:        # the correctly rounded quotient (read_k1_ints has checked that it is): within the float form's bound of ks_2samp's D
        assert np.all(np.abs(got['ks_d'] - exp['ks_d']) <= K.KS_D_FLOAT_FORM_ABS), what
    else:
        assert np.array_equal(got['ks_d'], exp['ks_d']), (what, np.flatnonzero(got['ks_d'] != exp['ks_d'])[:5])
    if ks_only:
        H.assert_close_p(got['ks_p'], exp['ks_p'], 1e-9, 'ks_p')
    else:
        live = (exp['status'] & 1) == 0                                      # (MWU_ALL_IDENTICAL: U and its p are NaN on both sides)
        H.compare_outputs({k: got[k][live] for k in got}, {k: exp[k][live] for k in exp}, with_comb=False, t_abs=gate[live])
        dead = ~live
        assert np.all(np.isnan(got['mwu_u'][dead])) and np.all(np.isnan(exp['mwu_u'][dead]))
        H.assert_close_p(got['mwu_p'][dead], exp['mwu_p'][dead], 1e-9, 'mwu_p')
        H.assert_close_stat(got['t_t'][dead], exp['t_t'][dead], 1e-11, gate[dead], 't_t')
        H.assert_close_p(got['t_p'][dead], exp['t_p'][dead], 1e-9, 't_p')
        H.assert_close_p(got['ks_p'][dead], exp['ks_p'][dead], 1e-9, 'ks_p')
    H.assert_close_stat(got['comb_st'], exp['comb_st'], 1e-9, 1e-12, 'comb_st')
    H.assert_close_p(got['comb_p'], exp['comb_p'], 1e-9, 'comb_p')


def _check_batch(env, cases, idx, dtype, *, form, counter, ks_only=False, flags=0, ks_num_written=True, rational=False, uniform=False,
                 f64_redo=None, int_keys=('ks_num', 'mwu_s', 'tie'), unpinned=False):
    """one batch (indices into `cases`) through every layout and the host entry; returns the number of positions.
    form / counter: what nmod_describe_dispatch must name for every size and the statistic that must equal the batch (None: not
    asserted — the float64 front end and the WIDE form's redo list decide per position); unpinned: once more with flags = 0, same bytes"""
    L = env['L']
    sig0, off0, sig1, off1 = HC.concat(cases, idx, dtype)
    npos = len(idx)
    n0, n1 = np.diff(off0), np.diff(off1)
    names = [cases[i]['name'] for i in idx]
    want = _exact(cases, idx, dtype)
    exp = _oracle(env, sig0, off0, sig1, off1, ks_only)
    gate = H.t_abs_gate(sig0, off0, sig1, off1)
    if form is not None:
        for a, b in sorted(set(zip(n0.tolist(), n1.tolist()))):
            assert form in _describe(env, dtype, ks_only, flags, a, b), (form, a, b, _describe(env, dtype, ks_only, flags, a, b))
    if uniform:
        assert len(set(n0.tolist())) == 1 and len(set(n1.tolist())) == 1
    tracks = KS_TRACKS if ks_only else ALL_TRACKS
    keys = tuple(k for k in int_keys if not (ks_only and k != 'ks_num') and not (k == 'ks_num' and not ks_num_written))
    first = first_ints = None
    for stride in ([False, True] if uniform else [False]):
        what = (form, dtype, 'ks' if ks_only else 'all', 'stride' if stride else 'csr')
        got, ints, stats = _run_device(env, ks_only, flags | (L.FLAG_KS_RATIONAL_D if rational else 0), sig0, off0, sig1, off1, stride, ks_num_written, rational)
        assert stats['positions'] == npos and (counter is None or stats[counter] == npos), (what, stats)
        assert f64_redo is None or stats['f64_redo'] == f64_redo, (what, stats, f64_redo)
        for k in keys:
            bad = np.flatnonzero(ints[k].astype(np.uint64) != want[k])
            assert bad.size == 0, (what, k, [(names[i], int(ints[k][i]), int(want[k][i])) for i in bad[:6]], bad.size)
        _compare_outputs(got, exp, gate, what, ks_only, rational)
        if first is None:
            first, first_ints = got, ints
    kw = dict(nb=2, weights_dif=2.0, method='stouffer', tests=L.TEST_KS if ks_only else L.TEST_ALL)
    host = env['nm'].detect_host(sig0, off0, sig1, off1, np.zeros(npos, np.int32), flags=flags | (L.FLAG_KS_RATIONAL_D if rational else 0), **kw)
    for k in tracks:
        assert np.array_equal(host[k].view(np.uint8), first[k].view(np.uint8)), (form, dtype, 'detect_host', k)
    if unpinned:
        for stride in ([False, True] if uniform else [False]):
            got, ints, stats = _run_device(env, ks_only, 0, sig0, off0, sig1, off1, stride, ks_num_written, rational)
            for k in keys:
                assert np.array_equal(ints[k], first_ints[k]), (form, dtype, 'without the flags', k, stats)
            for k in tracks:
                assert np.array_equal(got[k].view(np.uint8), first[k].view(np.uint8)), (form, dtype, 'without the flags', k, stats)
    return npos


def _timed(label, fn):
    t = time.perf_counter()
    out = fn()
    print('%s, %.1f s' % (label % out if isinstance(out, tuple) else label % (out,), time.perf_counter() - t))


# ---- big_rank_kernel
@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_big_rank_all_tests(env, dtype):
    batches = B.big_rank_batches(dtype)
    form = 'big_rank_kernel<%s>' % dtype
    def run():
        total = 0
        for _, cases in batches:
            total += _check_batch(env, cases, list(range(len(cases))), dtype, form=form, counter='big', ks_num_written=False, uniform=True)
        mixed = B.mixed_batch(batches)
        total += _check_batch(env, mixed, list(range(len(mixed))), dtype, form=form, counter='big', ks_num_written=False)
        return sum(len(c) for _, c in batches), total
    _timed(form + ', all tests: %d cases, %d positions', run)


@pytest.mark.parametrize('rational', [False, True], ids=['float_d', 'rational_d'])
@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_big_rank_ks_only(env, dtype, rational):
    batches = B.big_rank_batches(dtype, ks_only=True)
    form = 'big_rank_kernel<%s>' % dtype
    def run():
        total = 0
        for _, cases in batches:
            total += _check_batch(env, cases, list(range(len(cases))), dtype, form=form, counter='big', ks_only=True, rational=rational, uniform=True)
        mixed = B.mixed_batch(batches)
        total += _check_batch(env, mixed, list(range(len(mixed))), dtype, form=form, counter='big', ks_only=True, rational=rational)
        return sum(len(c) for _, c in batches), total
    _timed(form + ', KS-only%s: %%d cases, %%d positions' % (', NMOD_FLAG_KS_RATIONAL_D' if rational else ''), run)


@pytest.mark.filterwarnings('ignore:Degrees of freedom')              # (the Python oracle's variance of a group of one sample)
@pytest.mark.parametrize('ks_only', [False, True], ids=['all', 'ks'])
def test_big_rank_f64_redo(env, ks_only):
    """big_rank_kernel<2> on doubles 1.0 + u 2^-40 whose float32 images all tie: positions of 1 .. 8 193 samples a group, and
    5 000 v 3 000, where big_rank_kernel<f32> runs on the keys first; float32-exact and on-grid positions with ties in the same
    batch are not redone (f64_redo is exact).  With all tests the redo writes mwu_s, tie and the float form of D; KS-only, ks_num."""
    cases = B.f64_cases()
    redo = sum(c['kind'] == 'redo' for c in cases)
    def run():
        idx = list(range(len(cases)))
        n = _check_batch(env, cases, idx, 'f64', form=None, counter=None, ks_only=ks_only, ks_num_written=ks_only, f64_redo=redo)
        return len(cases), redo, n
    _timed('big_rank_kernel<f64> redo, %s: %%d cases (%%d class 3), %%d positions' % ('KS-only' if ks_only else 'all tests'), run)


# ---- big_hist_kernel
@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_big_hist(env, dtype):
    cases = B.big_hist_cases(dtype)
    form = 'big_hist_kernel<%s>' % dtype
    def run():
        order = HC.interleave(cases)
        total = _check_batch(env, cases, order, dtype, form=form, counter='big')                       # every size and either order: CSR
        for _, members in sorted(HC.uniform_groups(cases).items()):
            total += _check_batch(env, cases, members, dtype, form=form, counter='big', uniform=True)
        return len(cases), total
    _timed(form + ': %d cases, %d positions', run)


# ---- the two-pass WIDE classes of rank_hist_kernel
@pytest.mark.parametrize('dtype', ['f32', 'g32', 'i16'])
def test_wide_big_classes(env, dtype):
    """float32 off the grid (the bitmap form; the counting probes stay out by themselves), float32 on the grid and int16 (the
    counters): the latter two with the counting forms switched off, and once more without the flags — same bytes"""
    L = env['L']
    cases = B.wide_big_cases(dtype)
    pinned = 0 if dtype == 'f32' else (L.FLAG_NO_COUNTING | L.FLAG_NO_COUNT_WIDE)
    def run():
        total = 0
        for (n0, n1), members in sorted(HC.uniform_groups(cases).items()):
            form = 'rank_hist_kernel<%d,64,%s,wide>' % (1 << B.form_of(n0, n1)[1], 'i16' if dtype == 'i16' else 'f32')
            total += _check_batch(env, cases, members, dtype, form=form, counter='rank_hist_wide', flags=pinned, uniform=True, unpinned=pinned != 0)
        order = HC.interleave(cases)
        total += _check_batch(env, cases, order, dtype, form='wide>', counter='rank_hist_wide', flags=pinned, unpinned=pinned != 0)
        return len(cases), total
    _timed('rank_hist_kernel WIDE, larger group of 2 049 .. 4 096, %s: %%d cases, %%d positions' % dtype, run)


# ---- wide_redo_kernel
def test_wide_redo_layouts(env):
    """float32 positions whose streamed group has hundreds to thousands of tied samples off the milli-unit grid: the WIDE form
    leaves their ties inside Q to wide_redo_kernel (big_cases.redo_certain: certainly for every case of 2 048 samples and more but
    the untied one; a Q of 300 samples cannot reach the list and is finished by the WIDE form).  Which kernel added what is not
    visible from outside: tie — the sum of both — must be exact."""
    cases = B.wide_redo_cases()
    def run():
        total = _check_batch(env, cases, HC.interleave(cases), 'f32', form='wide>', counter='rank_hist_wide')
        for _, members in sorted(HC.uniform_groups(cases).items()):
            total += _check_batch(env, cases, members, 'f32', form='wide>', counter='rank_hist_wide', uniform=True)
        return len(cases), sum(B.redo_certain(c) for c in cases), total
    _timed('wide_redo_kernel: %d cases (%d certainly on the redo list), %d positions', run)


# ---- the persistent loops
def _loop(env, pools, G, dtype, **kw):
    batch = B.persistent_batch(pools, G, 2 * G + 64, B.LOOP_AFTER)
    for i in range(len(batch) - G):
        assert batch[i]['family'] != batch[i + G]['family'] and (len(pools) == 1 or B.sizes_of(batch[i]) != B.sizes_of(batch[i + G]))
    uniq = {id(c): c for c in batch}
    cases = list(uniq.values())
    index = {k: j for j, k in enumerate(uniq)}
    return _check_batch(env, cases, [index[id(c)] for c in batch], dtype, uniform=len(pools) == 1, **kw)


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_big_rank_persistent_loop_all_tests(env, dtype):
    G = 4 * env['cus']
    _timed('big_rank_kernel<%s> all tests, %d blocks: %%d positions' % (dtype, G),
           lambda: _loop(env, B.big_rank_loop_pools(dtype), G, dtype, form='big_rank_kernel<%s>' % dtype, counter='big', ks_num_written=False))


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_big_rank_persistent_loop_ks_only(env, dtype):
    G = 4 * env['cus']
    _timed('big_rank_kernel<%s> KS-only, %d blocks: %%d positions' % (dtype, G),
           lambda: _loop(env, B.big_rank_ks_loop_pools(dtype), G, dtype, form='big_rank_kernel<%s>' % dtype, counter='big', ks_only=True))


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_big_hist_persistent_loop(env, dtype):
    G = 2 * env['cus']
    _timed('big_hist_kernel<%s>, %d blocks: %%d positions' % (dtype, G),
           lambda: _loop(env, B.big_hist_loop_pools(dtype), G, dtype, form='big_hist_kernel<%s>' % dtype, counter='big'))


@pytest.mark.parametrize('ks_only', [False, True], ids=['all', 'ks'])
def test_f64_redo_persistent_loop(env, ks_only):
    G = 4 * env['cus']
    n = 2 * G + 64
    _timed('big_rank_kernel<f64> redo %s, %d blocks: %%d positions' % ('KS-only' if ks_only else 'all tests', G),
           lambda: _loop(env, [B.f64_loop_pool()], G, 'f64', form=None, counter=None, ks_only=ks_only, ks_num_written=ks_only, f64_redo=n))


def test_wide_redo_persistent_loop(env):
    G = 2 * env['cus']
    _timed('wide_redo_kernel, %d blocks: %%d positions, all certainly on the redo list' % G,
           lambda: _loop(env, B.redo_loop_pools(), G, 'f32', form='wide>', counter='rank_hist_wide'))


# ---- isolation
@pytest.mark.parametrize('form,dtype', [('big_hist', 'f32'), ('big_hist', 'i16'), ('big_rank', 'f32'), ('big_rank', 'i16')])
def test_a_position_leaves_the_others_alone(env, form, dtype):
    """one batch twice, the second time with one position replaced by a case of the same size and another family: the other
    positions' integers and every output track but the combined one (which reads the neighbours' p-values) are the same bytes"""
    if form == 'big_hist':
        cases = [c for c in B.big_hist_cases(dtype) if B.sizes_of(c) == (4096, 512)]
    else:
        cases = B.size_cases(1025, 2049, dtype)[(1025, 2049)]
    heavy = next(i for i, c in enumerate(cases) if c['family'] == 'all_equal')
    light = next(i for i, c in enumerate(cases) if c['family'] == 'one_bin')
    idx = [i for i in range(len(cases)) if i != heavy]
    at = idx.index(light)
    swapped = list(idx); swapped[at] = heavy                                 # all-tied where a distinct position was
    keep = np.arange(len(idx)) != at
    for stride in (False, True):
        a, ia, sa = _run_device(env, False, 0, *HC.concat(cases, idx, dtype), stride, form == 'big_hist')
        b, ib, sb = _run_device(env, False, 0, *HC.concat(cases, swapped, dtype), stride, form == 'big_hist')
        assert sa['big'] == sb['big'] == len(idx), (sa, sb)
        for k in ('mwu_s', 'tie') + (('ks_num',) if form == 'big_hist' else ()):
            assert np.array_equal(ia[k][keep], ib[k][keep]), (form, dtype, stride, k)
        assert ia['tie'][at] == 0 != ib['tie'][at]
        for k in ALL_TRACKS:
            if k not in ('comb_st', 'comb_p'):
                assert np.array_equal(a[k][keep].view(np.uint8), b[k][keep].view(np.uint8)), (form, dtype, stride, k)
        far = keep & (np.abs(np.arange(len(idx)) - at) > 2)                  # nb = 2: the window of the combined track
        for k in ('comb_st', 'comb_p'):
            assert np.array_equal(a[k][far].view(np.uint8), b[k][far].view(np.uint8)), (form, dtype, stride, k)
