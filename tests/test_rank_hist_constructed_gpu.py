"""GPU: the all-tests sorting forms of K1 — rank_hist_kernel's five packed instances and rank_pair_kernel's class pairs (5, 3),
(5, 4), (5, 5) — on constructed positions (hist_cases.py; test_hist_model.py proves on the CPU that each has the property it is
named for), float32 and int16, CSR and, where a batch's sizes are uniform, fixed stride.

Per batch: the exact integers K1 leaves in the workspace (ks_num, mwu_s, tie; k1_ints.read_k1_ints) equal k1_ints.exact_ints bit
for bit, mwu_u and ks_d are exact, the status equals the oracle's, every other track passes the project's bars against the C
oracle (helpers.compare_outputs, helpers.t_abs_gate), nmod_describe_dispatch names the form and nmod_last_dispatch_stats shows
that it took every position.  float32 values are multiples of 2^-11 (the counting probes stay out by themselves); int16 batches
run with NMOD_FLAG_NO_COUNTING | NMOD_FLAG_NO_COUNT_WIDE, and once more without: whatever split the probes choose, integers and
outputs are the same bytes.  The probes keep the counting forms away from rank_pair_kernel's constructed batches altogether (most
of their positions span far more than a counting window), so its classes get further int16 batches that the probes accept
(hist_cases.pair_narrow_cases), with the dispatch statistics showing that a counting form took positions.  Every batch also goes
once through detect_host: the same bytes again.

rank_pair_kernel evaluates only the float form of D and writes no ks_num (K2 reads ks_d_ref in all-tests mode): for its class
pairs mwu_s and tie are compared and D through ks_d, which must equal ks_2samp's bit for bit.

Packing (hist_cases.split_batches / triple_waves / row_neighbour_cases): a batch of one class keeps its order in the class list,
so positions PW * w .. PW * w + PW - 1 share wave item w; every case appears at every slot, with wave-mates of other families."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import hist_cases as HC
import k1_ints as K

pytestmark = pytest.mark.gpu

TRACKS = ('mwu_u', 'mwu_p', 't_t', 't_p', 'ks_d', 'ks_p', 'comb_st', 'comb_p', 'status')


@pytest.fixture(scope='module')
def env():
    import torch
    import nanomod_amd as nm
    import oracle_c
    L = nm._lib
    assert L.load().nmod_device_count() > 0
    return {'torch': torch, 'nm': nm, 'L': L, 'oracle': oracle_c, 'det': {}}


def _detector(env, flags):
    if flags not in env['det']:
        env['det'][flags] = env['nm'].DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=env['L'].TEST_ALL, flags=flags)
    return env['det'][flags]


def _describe(env, dtype, flags, n0, n1):
    L = env['L']
    prm = L.make_params(dtype=L.DTYPE_F32 if dtype == 'f32' else L.DTYPE_I16_MILLI, tests=L.TEST_ALL, flags=flags)
    buf = C.create_string_buffer(256)
    assert L.load().nmod_describe_dispatch(C.byref(prm), n0, n1, buf, 256) == 0
    return buf.value.decode()


def _exact(env, cases, idx, dtype):
    """exact_ints of the batch's positions, each case computed once"""
    out = []
    for i in idx:
        memo = cases[i].setdefault('exact_ints', {})                         # kept with the case itself: the case lists are cached
        if dtype not in memo:
            memo[dtype] = K.exact_ints(*HC.values(cases[i], dtype))
        out.append(memo[dtype])
    return out


def _run_device(env, flags, sig0, off0, sig1, off1, stride, ks_num_written):
    torch = env['torch']
    det = _detector(env, flags)
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
    ints = K.read_k1_ints(det, npos, res, n0, n1, ks_num_written=ks_num_written)
    stats = det.dispatch_stats()
    return {k: res[k].cpu().numpy() for k in TRACKS}, ints, stats


def _compare_outputs(got, exp, gate, what):
    assert np.array_equal(got['status'], exp['status']), (what, np.flatnonzero(got['status'] != exp['status'])[:5])
    assert np.array_equal(got['ks_d'], exp['ks_d']), (what, np.flatnonzero(got['ks_d'] != exp['ks_d'])[:5])
    live = (exp['status'] & 1) == 0                                          # (MWU_ALL_IDENTICAL: U and its p are NaN on both sides)
    H.compare_outputs({k: got[k][live] for k in got}, {k: exp[k][live] for k in exp}, with_comb=False, t_abs=gate[live])
    dead = ~live
    assert np.all(np.isnan(got['mwu_u'][dead])) and np.all(np.isnan(exp['mwu_u'][dead]))
    H.assert_close_p(got['mwu_p'][dead], exp['mwu_p'][dead], 1e-9, 'mwu_p')
    H.assert_close_stat(got['t_t'][dead], exp['t_t'][dead], 1e-11, gate[dead], 't_t')
    H.assert_close_p(got['t_p'][dead], exp['t_p'][dead], 1e-9, 't_p')
    H.assert_close_p(got['ks_p'][dead], exp['ks_p'][dead], 1e-9, 'ks_p')
    H.assert_close_stat(got['comb_st'], exp['comb_st'], 1e-9, 1e-12, 'comb_st')
    H.assert_close_p(got['comb_p'], exp['comb_p'], 1e-9, 'comb_p')


def _check_batch(env, cases, idx, dtype, counter, form, uniform, ks_num_written=True):
    """one batch (indices into `cases`) with the form pinned, through every layout and the host entry; returns the number of positions"""
    L = env['L']
    sig0, off0, sig1, off1 = HC.concat(cases, idx, dtype)
    npos = len(idx)
    n0, n1 = np.diff(off0), np.diff(off1)
    names = [cases[i]['name'] for i in idx]
    exact = _exact(env, cases, idx, dtype)
    want = {'ks_num': np.array([e[0] for e in exact], np.uint64), 'mwu_s': np.array([e[1] for e in exact], np.uint64),
            'tie': np.array([e[2] for e in exact], np.uint64)}
    exp = env['oracle'].detect_batch(sig0, off0, sig1, off1, np.zeros(npos, np.int32), 2, 2.0, 'stouffer', tests=7)
    gate = H.t_abs_gate(sig0, off0, sig1, off1)
    pinned = _pinned(L, dtype)
    for a, b in sorted(set(zip(n0.tolist(), n1.tolist()))):
        assert form in _describe(env, dtype, pinned, a, b), (form, a, b, _describe(env, dtype, pinned, a, b))
    if uniform:
        assert len(set(n0.tolist())) == 1 and len(set(n1.tolist())) == 1
    first = None
    for stride in ([False, True] if uniform else [False]):
        what = (form, dtype, 'stride' if stride else 'csr')
        got, ints, stats = _run_device(env, pinned, sig0, off0, sig1, off1, stride, ks_num_written)
        assert stats['positions'] == npos and stats[counter] == npos, (what, stats)        # the named form took every position
        for k in ('ks_num', 'mwu_s', 'tie'):
            if k == 'ks_num' and not ks_num_written:
                continue
            bad = np.flatnonzero(ints[k].astype(np.uint64) != want[k])
            assert bad.size == 0, (what, k, [(names[i], int(ints[k][i]), int(want[k][i])) for i in bad[:6]], bad.size)
        _compare_outputs(got, exp, gate, what)
        first = got if first is None else first
    host = env['nm'].detect_host(sig0, off0, sig1, off1, np.zeros(npos, np.int32), nb=2, weights_dif=2.0, method='stouffer',
                                 tests=L.TEST_ALL, flags=pinned)
    for k in TRACKS:
        assert np.array_equal(host[k].view(np.uint8), first[k].view(np.uint8)), (form, dtype, 'detect_host', k)
    return npos


def _pinned(L, dtype):
    return 0 if dtype == 'f32' else (L.FLAG_NO_COUNTING | L.FLAG_NO_COUNT_WIDE)


def _hist_batches(R, LG, dtype):
    """-> [(cases, indices, uniform)] of an instance"""
    PW, cap = 64 // LG, R * LG
    cases = HC.hist_cases(R, LG, dtype)
    fam = lambda i: cases[i]['family']
    out = [(cases, b, False) for b in HC.split_batches(cases, PW, 400 if cap < 1024 else 100)]   # every case at every slot, mixed sizes: CSR
    out += [(cases, HC.rotate_pack(members, PW, fam), True) for _, members in sorted(HC.uniform_groups(cases).items())]   # one size: CSR and fixed stride
    if PW > 1:                                                               # one triple among fast-path wave-mates, at every slot
        out.append((cases, HC.triple_waves(cases, PW)[0], True))
    if LG == 8:                                                              # two positions in one DPP row, tied end to start
        chain = HC.row_neighbour_cases(R, LG)
        out.append((chain, list(range(len(chain))), True))
    return out


def _pair_batches(c0, c1, dtype):
    cases = HC.pair_cases(c0, c1, dtype)
    return [(cases, HC.interleave(cases), False)] + [(cases, members, True) for _, members in sorted(HC.uniform_groups(cases).items())]


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('inst', HC.HIST_INSTANCES, ids=lambda t: 'R%d_LG%d' % t)
def test_rank_hist_instance(env, inst, dtype):
    R, LG = inst
    form = 'rank_hist_kernel<%d,%d,%s>' % (R, LG, dtype)
    total = sum(_check_batch(env, cases, idx, dtype, 'rank_hist', form, uniform) for cases, idx, uniform in _hist_batches(R, LG, dtype))
    print('%s: %d cases, %d positions' % (form, len(HC.hist_cases(R, LG, dtype)) + (16 if LG == 8 else 0), total))


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('inst', [t for t in HC.HIST_INSTANCES if t[1] < 64], ids=lambda t: 'R%d_LG%d' % t)
def test_triple_leaves_its_wave_mates_alone(env, inst, dtype):
    """one_triple sends its whole wave down seg_tie_pp's general path and may raise the wave's phase count: the pairs_only
    positions that share the wave must come out as the same bytes — integers and every output track — as in the same batch with
    one more pairs_only position in the triple's place.  (test_rank_hist_instance holds the batch with the triples to exact_ints
    and the oracle; this is the direct comparison.)"""
    R, LG = inst
    cases = HC.hist_cases(R, LG, dtype)
    with_t, without = HC.triple_waves(cases, 64 // LG)
    mates = np.array([x == y for x, y in zip(with_t, without)])
    assert 0 < mates.sum() == len(with_t) - len(with_t) // (64 // LG)
    pinned = _pinned(env['L'], dtype)
    for stride in (False, True):
        a, ia, sa = _run_device(env, pinned, *HC.concat(cases, with_t, dtype), stride, True)
        b, ib, sb = _run_device(env, pinned, *HC.concat(cases, without, dtype), stride, True)
        assert sa['rank_hist'] == sb['rank_hist'] == len(with_t), (sa, sb)
        for k in ('ks_num', 'mwu_s', 'tie'):
            assert np.array_equal(ia[k][mates], ib[k][mates]), (inst, dtype, stride, k)
        for k in TRACKS:
            assert np.array_equal(a[k][mates].view(np.uint8), b[k][mates].view(np.uint8)), (inst, dtype, stride, k)


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('cls', HC.PAIR_CLASSES, ids=lambda t: 'c%d_c%d' % t)
def test_rank_pair_class(env, cls, dtype):
    c0, c1 = cls
    form = 'rank_pair_kernel<%d,%d,%s>' % (1 << c0, 1 << c1, dtype)
    total = sum(_check_batch(env, cases, idx, dtype, 'rank_pair', form, uniform, ks_num_written=False)
                for cases, idx, uniform in _pair_batches(c0, c1, dtype))
    print('%s: %d cases, %d positions' % (form, len(HC.pair_cases(c0, c1, dtype)), total))


WELCH = ('t_t', 't_p')


@pytest.mark.parametrize('inst', HC.HIST_INSTANCES + HC.PAIR_CLASSES, ids=lambda t: '%d_%d' % t)
def test_int16_batches_without_the_flags(env, inst):
    """The int16 batches once more without NMOD_FLAG_NO_COUNTING | NMOD_FLAG_NO_COUNT_WIDE: whatever split the probes choose
    between the counting and the sorting forms, the integers and the outputs must be the same bytes as with the form pinned.

    The Welch tracks are the ones that could differ: every form sums an int16 group's moments about a key of its own (the first
    sample, the centre of its counting window, 0).  All of them — rank_pair_kernel's group_moments included — finish in
    milli_moments (rank_stats.hpp), which goes through the two integers that do not depend on that key, so t_t and t_p are the
    same bytes too; they are counted apart here so that a failure says how many positions differ and by how much.  The unpinned run
    is also held to the project's bars against the oracle.

    rank_pair_kernel's classes: the probes refuse the constructed batches whole (the counting form never runs on them), so the
    classes also run hist_cases.pair_narrow_cases, which test_hist_model.py shows the probe lets in; there the dispatch
    statistics must show rank_count_wide (which counts rank_count_value_kernel's positions too) above zero."""
    L = env['L']
    hist = inst in HC.HIST_INSTANCES
    batches = _hist_batches(*inst, 'i16') if hist else _pair_batches(*inst, 'i16')
    narrow = HC.pair_narrow_cases(*inst) if not hist else []                 # rank_pair_kernel's classes: batches the probes accept
    if narrow:
        batches = batches + [(narrow, HC.interleave(narrow), False)] + [(narrow, m, True) for _, m in sorted(HC.uniform_groups(narrow).items())]
    pinned = _pinned(L, 'i16')
    differ, runs, worst = 0, 0, {k: 0.0 for k in WELCH}
    for cases, idx, uniform in batches:
        sig0, off0, sig1, off1 = HC.concat(cases, idx, 'i16')
        exp = env['oracle'].detect_batch(sig0, off0, sig1, off1, np.zeros(len(idx), np.int32), 2, 2.0, 'stouffer', tests=7)
        gate = H.t_abs_gate(sig0, off0, sig1, off1)
        for stride in ([False, True] if uniform else [False]):
            what = (inst, 'stride' if stride else 'csr')
            a, ia, _ = _run_device(env, pinned, sig0, off0, sig1, off1, stride, hist)
            b, ib, stats = _run_device(env, 0, sig0, off0, sig1, off1, stride, hist)
            _compare_outputs(b, exp, gate, what)
            if cases is narrow:                                              # both kinds of form ran, and both hold the exact integers
                exact = _exact(env, cases, idx, 'i16')
                assert stats['rank_count_wide'] > 0 and stats['rank_count_wide'] + stats['rank_pair'] == len(idx), (what, stats)
                for j, k in ((1, 'mwu_s'), (2, 'tie')):
                    assert np.array_equal(ib[k], np.array([e[j] for e in exact], np.uint64)), (what, k)
            for k in ('mwu_s', 'tie') + (('ks_num',) if hist else ()):
                assert np.array_equal(ia[k], ib[k]), (what, k, stats)
            for k in TRACKS:
                if k not in WELCH:
                    assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k, stats)
            runs += len(idx)
            for k in WELCH:
                ne = (a[k].view(np.uint64) != b[k].view(np.uint64)) & ~(np.isnan(a[k]) & np.isnan(b[k]))
                differ += int(np.count_nonzero(ne)) if k == 't_t' else 0
                if ne.any():
                    worst[k] = max(worst[k], float(np.max(np.abs(a[k][ne] - b[k][ne]) / np.maximum(np.abs(a[k][ne]), 1e-300))))
    print('%r: t_t differs in %d of %d position runs; worst relative difference %r' % (inst, differ, runs, worst))
    assert differ == 0 and all(v == 0.0 for v in worst.values()), (inst, differ, runs, worst)


def test_reader_notices_a_moved_layout(env):
    """read_k1_ints refuses integers that do not reproduce the call's outputs: 65 positions read as 64, where mwu_s starts one
    256-byte step earlier"""
    cases = HC.hist_cases(8, 8, 'i16')
    idx = HC.interleave(cases)[:65]
    sig0, off0, sig1, off1 = HC.concat(cases, idx, 'i16')
    flags = env['L'].FLAG_NO_COUNTING | env['L'].FLAG_NO_COUNT_WIDE
    got, _, _ = _run_device(env, flags, sig0, off0, sig1, off1, False, True)
    assert K.align256(4 * 64) != K.align256(4 * 65)
    with pytest.raises(K.WorkspaceLayoutMoved):
        K.read_k1_ints(_detector(env, flags), 64, {k: v[:64] for k, v in got.items()}, np.diff(off0)[:64], np.diff(off1)[:64])


def test_reader_rational_d_branch(env):
    """read_k1_ints' exact check of ks_num: under NMOD_FLAG_KS_RATIONAL_D — a KS-only run; with all tests K2 reports the float
    form — ks_d is ks_num / (n0 n1) correctly rounded.  ks_num sits where the all-tests run leaves it, and equals exact_ints'."""
    L = env['L']
    torch = env['torch']
    cases = HC.hist_cases(16, 16, 'i16')
    idx = HC.interleave(cases)[:65]
    sig0, off0, sig1, off1 = HC.concat(cases, idx, 'i16')
    det = env['nm'].DeviceDetector(0, method='ks', tests=L.TEST_KS, flags=L.FLAG_KS_RATIONAL_D)
    res = det.run(torch.from_numpy(sig0).cuda(), torch.from_numpy(sig1).cuda(), torch.zeros(len(idx), dtype=torch.int32, device='cuda:0'),
                  off0=torch.from_numpy(off0).cuda(), off1=torch.from_numpy(off1).cuda(), npos=len(idx),
                  max_n0=int(np.diff(off0).max()), max_n1=int(np.diff(off1).max()))
    ints = K.read_k1_ints(det, len(idx), res, np.diff(off0), np.diff(off1), rational_d=True)
    assert np.array_equal(ints['ks_num'], np.array([e[0] for e in _exact(env, cases, idx, 'i16')], np.uint32))
    with pytest.raises(K.WorkspaceLayoutMoved):                              # one position off: the quotients no longer match
        K.read_k1_ints(det, len(idx) - 1, {k: v[1:] for k, v in res.items()}, np.diff(off0)[1:], np.diff(off1)[1:], rational_d=True)
