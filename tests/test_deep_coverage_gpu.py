"""-m gpu: NMOD_FLAG_DEEP — positions with a group beyond 65 535 samples on the deep form (deep_rank.hpp), against the Python
oracle (numpy / scipy restatement, any size) with the project's tolerances: U and D exact, p within 1e-9, t per t_abs_gate."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import helpers as H
import nanomod_oracle as orc

pytestmark = pytest.mark.gpu

PER_POS = ('mwu_u', 'mwu_p', 't_t', 't_p', 'ks_d', 'ks_p', 'status')
DEEP_SHAPES = [(70000, 300), (300, 66000), (100000, 100000), (150000, 5)]


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


def _rows(rng, kind, sizes, level=None):
    """one group's rows for the given sizes: float32 continuous, int16 event-like (milli-units, heavy ties), float64 off-grid"""
    parts = []
    for i, n in enumerate(sizes):
        if kind == 'f32':
            parts.append(rng.standard_normal(n).astype(np.float32) + np.float32(0.05 * (i % 3)))
        elif kind == 'i16':
            lv = int(level[i]) if level is not None else 0
            parts.append(np.clip(lv + np.rint(rng.standard_normal(n) * 200.0), -32767, 32767).astype(np.int16))
        else:
            x = rng.standard_normal(n) * 1.3 + 0.1 * (i % 3)
            x[: n // 50] = np.round(x[: n // 50], 2)                    # some exact ties between doubles that are not float32-exact
            parts.append(x)
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return np.concatenate(parts), off


def _batch(kind, seed=3, n_plain=24):
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(20, 3000)), int(rng.integers(20, 3000))) for _ in range(n_plain)]
    for k, s in enumerate(DEEP_SHAPES):
        sizes.insert(3 + 5 * k, s)
    level = rng.integers(-3000, 3000, len(sizes))
    sig0, off0 = _rows(rng, kind, [a for a, _ in sizes], level)
    sig1, off1 = _rows(rng, kind, [b for _, b in sizes], level + 30)
    rid = np.zeros(len(sizes), np.int32)
    rid[len(sizes) // 2:] = 1
    deep = np.array([max(a, b) > 65535 for a, b in sizes])
    return sig0, off0, sig1, off1, rid, deep


def _oracle(sig0, off0, sig1, off1, rid, method):
    sc = 1e-3 if sig0.dtype == np.int16 else 1.0
    m = orc.METHOD_FISHER if method == 'fisher' else orc.METHOD_STOUFFER
    return orc.detect_batch(sig0.astype(np.float64) * sc, off0, sig1.astype(np.float64) * sc, off1, rid, 2, 2.0, m)


def _check_vs_oracle(got, exp, sig0, off0, sig1, off1, sel, tests, with_comb=True):
    gate = H.t_abs_gate(sig0, off0, sig1, off1)[sel]
    g = {k: np.asarray(v)[sel] for k, v in got.items()}
    e = {k: np.asarray(v)[sel] for k, v in exp.items()}
    if tests == 7:
        H.compare_outputs(g, e, with_comb=False, t_abs=gate)
    else:
        H.assert_close_stat(g['ks_d'], e['ks_d'], 0, 0.0, 'ks_d')
        H.assert_close_p(g['ks_p'], e['ks_p'], 1e-9, 'ks_p')
    if with_comb:
        H.assert_close_stat(np.asarray(got['comb_st']), exp['comb_st'], 1e-9, 1e-12, 'comb_st')
        H.assert_close_p(np.asarray(got['comb_p']), exp['comb_p'], 1e-9, 'comb_p')


@pytest.mark.parametrize('kind', ['f32', 'i16', 'f64'])
def test_mixed_batch_host_and_device(nm, kind):
    import torch
    L, E = nm._lib, nm.engine
    sig0, off0, sig1, off1, rid, deep = _batch(kind)
    plain = ~deep
    for method in ('stouffer', 'fisher'):
        exp = _oracle(sig0, off0, sig1, off1, rid, method)
        for tests in (L.TEST_ALL, L.TEST_KS):
            ref = E.detect_host(sig0, off0, sig1, off1, rid, method=method, tests=tests)
            assert np.all(ref['status'][deep] & L.STATUS_TOO_LARGE)                  # without the flag: as before
            got = E.detect_host(sig0, off0, sig1, off1, rid, method=method, tests=tests, deep=True)
            st = L.last_dispatch_stats()
            assert st['deep'] == int(deep.sum()) and st['skipped'] == 0, st
            assert not np.any(got['status'] & L.STATUS_TOO_LARGE)
            for k in PER_POS:
                if k in ref:
                    assert np.array_equal(got[k][plain], ref[k][plain], equal_nan=True), (kind, method, tests, k)
            _check_vs_oracle(got, exp, sig0, off0, sig1, off1, np.ones(len(rid), bool), tests)
    # device-resident entry (CSR, unknown maxima)
    dev = 'cuda:0'
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for tests in (L.TEST_ALL, L.TEST_KS):
        det = E.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=tests, deep=True)
        res = det.run(tt(sig0), tt(sig1), tt(rid), off0=tt(off0), off1=tt(off1))
        torch.cuda.synchronize()
        st = det.dispatch_stats()
        assert st['deep'] == int(deep.sum()) and st['skipped'] == 0, st
        got = {k: v.cpu().numpy() for k, v in res.items()}
        _check_vs_oracle(got, _oracle(sig0, off0, sig1, off1, rid, 'stouffer'), sig0, off0, sig1, off1, np.ones(len(rid), bool), tests)


def test_at_max_deep_and_beyond(nm):
    L, E = nm._lib, nm.engine
    rng = np.random.default_rng(11)
    for n0, ok in ((L.MAX_DEEP, True), (L.MAX_DEEP + 1, False)):
        sig0 = rng.standard_normal(n0).astype(np.float32)
        sig1 = (rng.standard_normal(1000) + 0.01).astype(np.float32)
        off0 = np.array([0, n0], np.int64); off1 = np.array([0, 1000], np.int64)
        rid = np.zeros(1, np.int32)
        got = E.detect_host(sig0, off0, sig1, off1, rid, method='ks', deep=True)
        if ok:
            assert got['status'][0] == 0
            exp = _oracle(sig0, off0, sig1, off1, rid, 'stouffer')
            _check_vs_oracle(got, exp, sig0, off0, sig1, off1, np.ones(1, bool), L.TEST_ALL, with_comb=False)
        else:
            assert got['status'][0] & L.STATUS_TOO_LARGE
            assert np.isnan(got['mwu_p'][0]) and np.isnan(got['ks_p'][0]) and np.isnan(got['t_t'][0])


def test_spread_across_the_machine(nm):
    import torch
    L, E = nm._lib, nm.engine
    dev = 'cuda:0'
    # 4 x 2 000 000 v 2 000 000, fixed stride, device-resident
    npos, n = 4, 2000000
    det = E.DeviceDetector(0, nb=1, weights_dif=2.0, method='stouffer', tests=L.TEST_ALL, deep=True)
    s0 = torch.empty(npos * n, dtype=torch.float32, device=dev); s1 = torch.empty(npos * n, dtype=torch.float32, device=dev)
    det.synth_fill(s0, 5, 0, npos, 0, n, 2, 0.003)
    det.synth_fill(s1, 5, 0, npos, 1, n, 2, 0.003)
    rid = torch.zeros(npos, dtype=torch.int32, device=dev)
    res = det.run(s0, s1, rid, stride0=n, stride1=n, npos=npos)
    torch.cuda.synchronize()
    assert det.dispatch_stats()['deep'] == npos
    a0, a1 = s0.cpu().numpy(), s1.cpu().numpy()
    off = np.arange(0, (npos + 1) * n, n, dtype=np.int64)
    exp = orc.detect_batch(a0.astype(np.float64), off, a1.astype(np.float64), off, np.zeros(npos, np.int32), 1, 2.0, orc.METHOD_STOUFFER)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    _check_vs_oracle(got, exp, a0, off, a1, off, np.ones(npos, bool), L.TEST_ALL)
    del s0, s1
    # 600 x 70 000 v 70 000 event-like int16 rows through the host pipeline in 1 MiB chunks (one position per chunk), ~50 checked
    npos, n = 600, 70000
    q0 = torch.empty(npos * n, dtype=torch.int16, device=dev); q1 = torch.empty(npos * n, dtype=torch.int16, device=dev)
    det.synth_fill_events(q0, 9, 0, npos, 0, n_per_pos=n, plant_period=25, plant_shift_milli=20, spread_milli=300)
    det.synth_fill_events(q1, 9, 0, npos, 1, n_per_pos=n, plant_period=25, plant_shift_milli=20, spread_milli=300)
    b0, b1 = q0.cpu().numpy(), q1.cpu().numpy()
    del q0, q1
    off = np.arange(0, (npos + 1) * n, n, dtype=np.int64)
    rid = np.zeros(npos, np.int32)
    assert L.load().nmod_host_pipeline_config(1 << 20, 0, 0, 0) == 0
    try:
        got = E.detect_host(b0, off, b1, off, rid, method='ks', deep=True)
    finally:
        L.load().nmod_host_pipeline_config(0, 0, 0, 0)
    assert L.last_dispatch_stats()['deep'] == npos
    sel = np.arange(0, npos, 12)
    sub0 = np.concatenate([b0[off[i]:off[i + 1]] for i in sel]); sub1 = np.concatenate([b1[off[i]:off[i + 1]] for i in sel])
    soff = np.arange(0, (len(sel) + 1) * n, n, dtype=np.int64)
    exp = _oracle(sub0, soff, sub1, soff, np.zeros(len(sel), np.int32), 'stouffer')
    _check_vs_oracle({k: v[sel] for k, v in got.items()}, exp, sub0, soff, sub1, soff, np.ones(len(sel), bool), L.TEST_ALL,
                     with_comb=False)


def test_status_bits(nm):
    L, E = nm._lib, nm.engine
    n = 80000
    sig0 = np.full(n, 0.25, np.float32); sig1 = np.full(n, 0.25, np.float32)
    off = np.array([0, n], np.int64)
    got = E.detect_host(sig0, off, sig1, off, np.zeros(1, np.int32), method='ks', deep=True)
    assert got['status'][0] == (L.STATUS_MWU_ALL_IDENTICAL | L.STATUS_T_NAN)
    # mtest2 raises as the reference does
    mo = _moptions(nm, tempfile.mkdtemp(), {('c', '+'): {100: (sig0, sig1)}}, deep=1)
    with pytest.raises(ValueError, match='All numbers are identical'):
        nm.mtest2(mo)
    rng = np.random.default_rng(2)
    s0 = rng.standard_normal(n).astype(np.float32); s1 = rng.standard_normal(n).astype(np.float32)
    s0[12345] = np.nan
    for tests in (L.TEST_ALL, L.TEST_KS):
        got = E.detect_host(s0, off, s1, off, np.zeros(1, np.int32), method='ks', tests=tests, deep=True, flags=L.FLAG_CHECK_FINITE)
        assert got['status'][0] & L.STATUS_NONFINITE
        got = E.detect_host(s1, off, s1, off, np.zeros(1, np.int32), method='ks', tests=tests, deep=True, flags=L.FLAG_CHECK_FINITE)
        assert not got['status'][0] & L.STATUS_NONFINITE


def test_downsample_deep(nm, monkeypatch):
    L, E = nm._lib, nm.engine
    rng = np.random.default_rng(4)
    n = 200000
    sig0 = rng.standard_normal(2 * n).astype(np.float32); sig1 = (rng.standard_normal(2 * n) + 0.002).astype(np.float32)
    off = np.array([0, n, 2 * n], np.int64)
    with pytest.raises(RuntimeError):
        E.downsample_ks(sig0, off, sig1, off, [0], [1000], iters=20)
    d1, p1 = E.downsample_ks(sig0, off, sig1, off, [0, 1], [1000, 1000], iters=20, deep=True)
    assert np.all(np.isfinite(d1)) and np.all((p1 > 0) & (p1 <= 1))
    monkeypatch.setenv('NMOD_DOWNSAMPLE_ELEMENTS', str(50000))
    d2, p2 = E.downsample_ks(sig0, off, sig1, off, [0, 1], [1000, 1000], iters=20, deep=True)
    assert np.array_equal(d1, d2) and np.array_equal(p1, p2)
    monkeypatch.delenv('NMOD_DOWNSAMPLE_ELEMENTS')
    # cov >= n: the plain KS pair, bit for bit
    dd, pp = E.downsample_ks(sig0, off, sig1, off, [0, 1], [n, n + 7], iters=5, deep=True)
    ref = E.detect_host(sig0, off, sig1, off, np.zeros(2, np.int32), method='ks', tests=L.TEST_KS, deep=True)
    assert np.array_equal(dd, ref['ks_d']) and np.array_equal(pp, ref['ks_p'])
    # a threshold beyond 65 535 on 150 000-sample groups
    m = 150000
    off2 = np.array([0, m], np.int64)
    d3, p3 = E.downsample_ks(sig0[:m], off2, sig1[:m], off2, [0], [100000], iters=8, deep=True)
    assert np.isfinite(d3[0]) and 0 < p3[0] <= 1


def _moptions(nm, outdir, sites, deep):
    """the reference's moptions (helpers.build_moptions) over sites {(chrom, strand): {pos: (a, b)}}"""
    chrom, strand, pos, s0, s1 = [], [], [], [], []
    for (c, st), d in sites.items():
        for p, (a, b) in d.items():
            chrom.append(c); strand.append(st); pos.append(p); s0.append(np.asarray(a)); s1.append(np.asarray(b))
    offs = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    fx = {'sig0': np.concatenate(s0), 'off0': offs(s0), 'sig1': np.concatenate(s1), 'off1': offs(s1), 'chrom': np.array(chrom),
          'strand': np.array(strand), 'pos': np.array(pos), 'base0': np.array(['A'] * len(pos)), 'base1': np.array(['A'] * len(pos))}
    mo = H.build_moptions(fx, outdir, 'deep', 1, 2.0, 'stouffer')
    if deep is not None:
        mo['nmod_deep'] = deep
    return mo


def test_mtest2_deep_site(nm):
    rng = np.random.default_rng(8)
    sites = {('c', '+'): {}}
    sizes = [(40, 50), (70000, 900), (60, 45), (35, 80)]
    for i, (a, b) in enumerate(sizes):
        sites[('c', '+')][100 + i] = (np.round(rng.standard_normal(a), 3), np.round(rng.standard_normal(b) + 0.02, 3))
    lines = {}
    for deep in (None, 0, 1):
        out = tempfile.mkdtemp()
        mo = _moptions(nm, out, sites, deep)
        nm.mtest2(mo)
        with open(os.path.join(out, 'deep_sign_test.txt')) as f:
            lines[deep] = f.readlines()
        if deep:
            assert mo['nmod_flagged'] == []
            # the deep site's line as the oracle formats its numbers
            recs = [orc.getKStest(np.asarray(x), np.asarray(y)) for x, y in sites[('c', '+')].values()]
            ks_p = np.array([r[2][1] for r in recs]); ks_d = np.array([r[2][0] for r in recs])
            cst, cp = orc.combine_track(ks_d, ks_p, np.zeros(len(recs), np.int32), 1, 2.0, orc.METHOD_STOUFFER)
            exp_line = orc.format_sign_test_line('c', '+', 101, 'A', 70000, 900, recs[1] + [(cst[1], cp[1])], True)
            assert lines[1][1] == exp_line, (lines[1][1], exp_line)
        else:
            assert len(mo['nmod_flagged']) == 1
    assert lines[None] == lines[0]                                           # off by default: the output is unchanged
    # the other sites print the same per-position numbers either way (the deep site's KS p enters only their combined pair)
    for i in (0, 2, 3):
        assert lines[0][i].split()[:12] == lines[1][i].split()[:12]
