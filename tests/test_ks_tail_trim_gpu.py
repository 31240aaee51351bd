"""GPU: the KS step around the sort — K2's size term as a launch constant in fixed-stride batches, kolmogorov_sf with one exp
per branch, norm_isf by AS241 (special_math.hpp, pvalue_kernels.hpp) — on the sizes where the pieces differ:
  (5, 7)        a few samples: the dual series of kolmogorov_sf for nearly every position
  (200, 200)    the headline shape
  (193, 256)    S one past a multiple of the lanes' rows; Q fills the capacity
  (256, 200)    the groups swapped, S = the second group
  (37, 1000)    very unequal sizes (en is dominated by the small group)
Rows without any tie (a permutation of distinct values per position) and rows of few integers (ties across the groups,
runs inside S in every position).  KS-only and all tests, the claimed and the static walk (NMOD_FLAG_K1_STATIC_ITEMS).

Fixed strides take the host's size term from FinalizeArgs; the same rows as CSR work it out per position: ks_d, ks_p, comb_st,
comb_p and status must agree bit for bit (which is also the check that host and device round the term alike).  Every position
is held against the C oracle: D equal, the p-values within the gates of helpers.py.

test_batch_larger_than_the_grid: 40 001 positions of 200 v 200 are 10 001 work items of four positions, more than two per
resident wave (test_k1_uniform_gpu.py counts 35 000 items as more than eight), so waves go past their first item."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (200, 200), (193, 256), (256, 200), (37, 1000)]
NPOS = 600
TRACKS = ('ks_d', 'ks_p', 'comb_st', 'comb_p', 'status')


@pytest.fixture(scope='module')
def env():
    import torch
    import nanomod_amd as nm
    import oracle_c
    L = nm._lib
    assert L.load().nmod_device_count() > 0
    return {'torch': torch, 'nm': nm, 'L': L, 'oracle': oracle_c, 'det': {}}


def _detector(env, tests, flags):
    key = (tests, flags)
    if key not in env['det']:
        env['det'][key] = env['nm'].DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=tests, flags=flags)
    return env['det'][key]


def host_rows(kind, n0, n1, npos, seed):
    """float32 rows [npos, n0], [npos, n1].  'distinct': per position a permutation of n0 + n1 distinct values dealt to the two
    groups; 'ties': integers below half the smaller size, so that either group holds a value twice (runs inside S) and the
    groups share values.  Every third position has the second group pushed up (small p)."""
    rng = np.random.default_rng(seed)
    if kind == 'distinct':
        v = rng.permuted(np.tile(np.arange(n0 + n1, dtype=np.float32), (npos, 1)), axis=1)
        a, b = v[:, :n0].copy(), v[:, n0:].copy()
        b[::3] = b[::3] * 1.5 + 0.25                             # (multiples of 1.5 plus 0.25 are no integers: still no tie)
    else:
        g = (min(n0, n1) + 1) // 2
        a = rng.integers(0, g, (npos, n0)).astype(np.float32)
        b = rng.integers(0, g, (npos, n1)).astype(np.float32)
        b[::3] += g // 3
    return a * np.float32(0.03125), b * np.float32(0.03125)


def _rows(env, kind, n0, n1, npos, seed):
    a, b = host_rows(kind, n0, n1, npos, seed)
    return env['torch'].from_numpy(a.reshape(-1)).cuda(), env['torch'].from_numpy(b.reshape(-1)).cuda()


def _run(env, tests, flags, a, b, n0, n1, npos, csr, tracks):
    torch = env['torch']
    det = _detector(env, tests, flags)
    rid = torch.zeros(npos, dtype=torch.int32, device='cuda:0')
    if csr:
        off0 = torch.arange(npos + 1, dtype=torch.int64, device='cuda:0') * n0
        off1 = torch.arange(npos + 1, dtype=torch.int64, device='cuda:0') * n1
        res = det.run(a, b, rid, off0=off0, off1=off1, npos=npos, max_n0=n0, max_n1=n1)
    else:
        res = det.run(a, b, rid, stride0=n0, stride1=n1, npos=npos)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in tracks}


def _has_ties(a, b, n0, n1, npos):
    ha, hb = a.cpu().numpy().reshape(npos, n0), b.cpu().numpy().reshape(npos, n1)
    cross = sum(np.intersect1d(ha[i], hb[i]).size > 0 for i in range(npos))
    hs = ha if n0 <= n1 else hb                                  # S: the smaller group is the one that is sorted
    runs = sum(np.unique(hs[i]).size < hs.shape[1] for i in range(npos))
    return cross, runs


@pytest.mark.parametrize('mode', ['ks', 'all'])
@pytest.mark.parametrize('kind', ['distinct', 'ties'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dv%d' % s)
def test_strides_csr_and_oracle(env, shape, kind, mode):
    n0, n1 = shape
    L = env['L']
    tests = L.TEST_KS if mode == 'ks' else L.TEST_ALL
    a, b = _rows(env, kind, n0, n1, NPOS, 100 + n0)
    cross, runs = _has_ties(a, b, n0, n1, NPOS)
    if kind == 'distinct':
        assert cross == 0 and runs == 0
    else:
        assert cross >= NPOS // 2 and runs == NPOS, (cross, runs)
    off0 = np.arange(NPOS + 1, dtype=np.int64) * n0; off1 = np.arange(NPOS + 1, dtype=np.int64) * n1
    exp = env['oracle'].detect_batch(a.cpu().numpy(), off0, b.cpu().numpy(), off1, np.zeros(NPOS, np.int32), 2, 2.0, 'stouffer',
                                     tests=1 if mode == 'ks' else 7)
    tracks = TRACKS + (('mwu_u', 'mwu_p', 't_t', 't_p') if mode == 'all' else ())
    for flags in (0, L.FLAG_K1_STATIC_ITEMS):
        strided = _run(env, tests, flags, a, b, n0, n1, NPOS, False, tracks)
        listed = _run(env, tests, flags, a, b, n0, n1, NPOS, True, tracks)
        for k in tracks:
            assert np.array_equal(strided[k].view(np.uint8), listed[k].view(np.uint8)), (k, flags)
        assert not strided['status'].any()
        assert np.array_equal(strided['ks_d'], exp['ks_d']), flags
        H.assert_close_p(strided['ks_p'], exp['ks_p'], 1e-9, 'ks_p')
        H.assert_close_stat(strided['comb_st'], exp['comb_st'], 1e-9, 1e-12, 'comb_st')
        H.assert_close_p(strided['comb_p'], exp['comb_p'], 1e-9, 'comb_p')
        if mode == 'all':
            t_abs = H.t_abs_gate(a.cpu().numpy(), off0, b.cpu().numpy(), off1)
            H.compare_outputs(strided, exp, with_comb=True, t_abs=t_abs)
    # the sizes reach both series of kolmogorov_sf somewhere in the set (x = (en + 0.12 + 0.11/en) D against 0.82)
    en = np.sqrt(n0 * n1 / (n0 + n1))
    x = (en + 0.12 + 0.11 / en) * exp['ks_d']
    assert (x >= 0.82).any()
    if kind == 'distinct':
        assert (x < 0.82).any()


def test_batch_larger_than_the_grid(env):
    n, npos = 200, 40001
    torch, L = env['torch'], env['L']
    det = _detector(env, L.TEST_KS, 0)
    a = torch.empty(npos * n, dtype=torch.float32, device='cuda:0'); b = torch.empty(npos * n, dtype=torch.float32, device='cuda:0')
    det.synth_fill(a, 3, 0, npos, 0, n, 7, 0.8)
    det.synth_fill(b, 3, 0, npos, 1, n, 7, 0.8)
    idx = np.unique(np.concatenate([np.arange(64), np.arange(npos // 2, npos // 2 + 64), np.arange(npos - 64, npos)]))
    sel = torch.from_numpy(idx).cuda()
    ha = a.view(npos, n)[sel].cpu().numpy().reshape(-1); hb = b.view(npos, n)[sel].cpu().numpy().reshape(-1)
    off = np.arange(len(idx) + 1, dtype=np.int64) * n
    exp = env['oracle'].detect_batch(ha, off, hb, off, np.zeros(len(idx), np.int32), 0, 2.0, 'ks', tests=1)
    for flags in (0, L.FLAG_K1_STATIC_ITEMS):
        strided = _run(env, L.TEST_KS, flags, a, b, n, n, npos, False, TRACKS)
        listed = _run(env, L.TEST_KS, flags, a, b, n, n, npos, True, TRACKS)
        for k in TRACKS:
            assert np.array_equal(strided[k].view(np.uint8), listed[k].view(np.uint8)), (k, flags)
        assert not strided['status'].any()
        assert np.array_equal(strided['ks_d'][idx], exp['ks_d']), flags
        H.assert_close_p(strided['ks_p'][idx], exp['ks_p'], 1e-9, 'ks_p')
