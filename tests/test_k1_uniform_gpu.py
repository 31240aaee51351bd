"""GPU: fixed-stride batches without a position list run the UNIFORM instances of ks_rank_kernel (ks_rank.hpp), which hold the
sizes, the schedule and the chunk layout of the row loads as launch constants.  The same rows handed over as CSR
(off = arange(npos + 1) * n) are binned and take the generic instances: every output of a position depends on that position's
rows only (and on its neighbours' through the window combine), so both layouts must agree bit for bit, and a sample of the
positions is held against the C oracle (D equal, p within the project's 1e-9; with NMOD_FLAG_KS_RATIONAL_D D is the correctly
rounded rational, which the project holds to 4.5e-16 — two ulp of 1 — of the reference's float form |fl(c0/n0) - fl(c1/n1)|:
each quotient is off by up to half an ulp of a number below 1, whatever the size of their difference).

Each shape is the smallest that reaches one branch of what the uniform instance hoists:
  (2, 2), (3, 300)          rows shorter than four samples, the (8, 8) form
  (64, 64)                  S fills the capacity of the (8, 8) form
  (100, 100), (128, 65)     the (16, 8) form; the groups swapped
  (200, 200)                the headline: (16, 16), the last chunk live in two lanes
  (192, 200)                m a multiple of the chunk: no partly live chunk
  (256, 256)                S fills the capacity of the (16, 16) form
  (200, 64), (129, 1000)    no one-per-lane round / no full round of Q; swapped
  (500, 500), (512, 257)    the (16, 32) form
  (1000, 1000)              the (16, 64) form
  (2048, 1025)              the (32, 64) form
plus (203, 200) and (66, 61): a row end inside a chunk (m no multiple of four), unpacked and packed.
Batches with a group of 320 samples or more carry the counting form's gates, which selects the generic instance; those shapes
run again with NMOD_FLAG_NO_COUNT_WIDE so that their uniform instances are the ones checked."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (3, 300), (64, 64), (100, 100), (128, 65), (200, 200), (192, 200), (256, 256), (200, 64), (129, 1000),
          (500, 500), (512, 257), (1000, 1000), (2048, 1025), (203, 200), (66, 61)]
NPOS = 3001
TRACKS = ('ks_d', 'ks_p', 'comb_p', 'status')
CW_MIN_Q = 320                   # rank_stats_launch.hpp: kCwKsMinQ


def positions_per_wave(n0, n1):
    m = min(n0, n1)
    lanes = 8 if m <= 128 else 16 if m <= 256 else 32 if m <= 512 else 64
    return 64 // lanes


def counts_of(n0, n1):
    """1, PW - 1, PW + 1 and 3 001 positions (an empty batch launches nothing: PW - 1 = 0 is no case)"""
    pw = positions_per_wave(n0, n1)
    return sorted({1, pw - 1, pw + 1, NPOS} - {0})


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
        L = env['L']
        env['det'][flags] = env['nm'].DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=L.TEST_KS, flags=flags)
    return env['det'][flags]


def _flag_sets(env, n0, n1):
    L = env['L']
    sets = [0, L.FLAG_KS_RATIONAL_D, L.FLAG_K1_STATIC_ITEMS]
    if max(n0, n1) >= CW_MIN_Q:
        sets += [f | L.FLAG_NO_COUNT_WIDE for f in sets]
    return sets


def _fill(env, kind, dtype, n0, n1, npos, seed):
    """rows of `npos` positions on the device: the generator's continuous rows with a planted shift, or event rows on the
    3-decimal grid (ties across the groups and inside S)"""
    torch = env['torch']
    tdt = torch.float32 if dtype == 'f32' else torch.int16
    det = _detector(env, 0)
    a = torch.empty(npos * n0, dtype=tdt, device='cuda:0'); b = torch.empty(npos * n1, dtype=tdt, device='cuda:0')
    if kind == 'continuous':
        det.synth_fill(a, seed, 0, npos, 0, n0, 7, 0.8)
        det.synth_fill(b, seed, 0, npos, 1, n1, 7, 0.8)
    else:
        det.synth_fill_events(a, seed, 0, npos, 0, n_per_pos=n0, plant_period=7, plant_shift_milli=300, spread_milli=60)
        det.synth_fill_events(b, seed, 0, npos, 1, n_per_pos=n1, plant_period=7, plant_shift_milli=300, spread_milli=60)
    return a, b


def _oracle_sample(env, a, b, n0, n1, npos, take=24):
    """the oracle's ks_d / ks_p of the first and the last `take` positions (they depend on the position's rows only)"""
    idx = np.unique(np.concatenate([np.arange(min(take, npos)), np.arange(max(npos - take, 0), npos)]))
    sel = env['torch'].from_numpy(idx).cuda()
    ha = a.view(npos, n0)[sel].cpu().numpy().reshape(-1); hb = b.view(npos, n1)[sel].cpu().numpy().reshape(-1)
    off0 = np.arange(len(idx) + 1, dtype=np.int64) * n0; off1 = np.arange(len(idx) + 1, dtype=np.int64) * n1
    exp = env['oracle'].detect_batch(ha, off0, hb, off1, np.zeros(len(idx), np.int32), 2, 2.0, 'stouffer', tests=1)
    return idx, exp['ks_d'], exp['ks_p']


def _run(env, flags, a, b, n0, n1, npos, csr):
    torch = env['torch']
    det = _detector(env, flags)
    rid = torch.zeros(npos, dtype=torch.int32, device='cuda:0')
    if csr is None:
        res = det.run(a[:npos * n0], b[:npos * n1], rid, stride0=n0, stride1=n1, npos=npos)
    else:
        res = det.run(a[:npos * n0], b[:npos * n1], rid, off0=csr[0][:npos + 1], off1=csr[1][:npos + 1], npos=npos, max_n0=n0, max_n1=n1)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in TRACKS}


def _check(env, a, b, n0, n1, npos_all, counts, flag_sets):
    torch, L = env['torch'], env['L']
    csr = (torch.arange(npos_all + 1, dtype=torch.int64, device='cuda:0') * n0,
           torch.arange(npos_all + 1, dtype=torch.int64, device='cuda:0') * n1)
    idx, exp_d, exp_p = _oracle_sample(env, a, b, n0, n1, npos_all)
    for npos in counts:
        here = idx < npos
        for flags in flag_sets:
            strided = _run(env, flags, a, b, n0, n1, npos, None)
            listed = _run(env, flags, a, b, n0, n1, npos, csr)
            for k in TRACKS:
                assert np.array_equal(strided[k].view(np.uint8), listed[k].view(np.uint8)), (k, npos, flags)
            d, p = strided['ks_d'][idx[here]], strided['ks_p'][idx[here]]
            if flags & L.FLAG_KS_RATIONAL_D:
                assert np.all(np.abs(d - exp_d[here]) <= 4.5e-16), (npos, flags, np.abs(d - exp_d[here]).max())
            else:
                assert np.array_equal(d, exp_d[here]), (npos, flags)
            assert np.all(np.abs(p - exp_p[here]) <= 1e-9 * np.abs(exp_p[here]) + 1e-300), (npos, flags, np.abs(p - exp_p[here]).max())


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dv%d' % s)
def test_strides_and_csr_agree(env, shape, dtype):
    n0, n1 = shape
    for kind in ('continuous', 'events'):
        a, b = _fill(env, kind, dtype, n0, n1, NPOS, 11 + n0)
        _check(env, a, b, n0, n1, NPOS, counts_of(n0, n1), _flag_sets(env, n0, n1))


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_every_position_has_q_on_a_run_of_s(env, dtype):
    """constructed: S is made of runs of equal values (each value three or more times) and Q holds samples equal to them"""
    torch = env['torch']
    n, npos = 200, NPOS
    rng = np.random.default_rng(5)
    s = np.repeat(rng.integers(-40, 40, (npos, n // 4)), 4, axis=1)                  # runs of four (longer where values repeat)
    q = np.concatenate([s[:, ::5], rng.integers(-60, 60, (npos, n - s[:, ::5].shape[1]))], axis=1)
    s = rng.permuted(s, axis=1); q = rng.permuted(q, axis=1)
    assert all(np.intersect1d(s[i], q[i]).size > 0 for i in range(0, npos, 97))
    npdt = np.float32 if dtype == 'f32' else np.int16
    scale = 0.125 if dtype == 'f32' else 25
    a = torch.from_numpy((s * scale).astype(npdt).reshape(-1)).cuda(); b = torch.from_numpy((q * scale).astype(npdt).reshape(-1)).cuda()
    _check(env, a, b, n, n, npos, [npos], _flag_sets(env, n, n))
    _check(env, b, a, n, n, npos, [npos], [0])


def test_waves_draw_tickets(env):
    """140 000 positions of 200 v 200: 35 000 work items, more than eight per resident wave — chunks are claimed"""
    n, npos = 200, 140000
    a, b = _fill(env, 'continuous', 'f32', n, n, npos, 3)
    _check(env, a, b, n, n, npos, [npos], [0, env['L'].FLAG_K1_STATIC_ITEMS])
