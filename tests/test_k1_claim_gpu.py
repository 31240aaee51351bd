"""GPU: ks_rank_kernel hands a part of its work items out by chunk from a per-launch counter (item_claim.hpp).  Every position's
outputs depend on that position's rows only, so the claimed walk and the strided walk (NMOD_FLAG_K1_STATIC_ITEMS) must agree bit
for bit, on every size around one item per resident wave, when a workspace (and its counters) is used again, on a batch that
launches several size classes, and on a side stream; the numbers are checked against the C oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 200                       # 200 v 200, fixed stride: four positions per work item (16 keys x 16 lanes)
PW = 4
TRACKS = ('ks_d', 'ks_p', 'comb_st', 'comb_p', 'status')


@pytest.fixture(scope='module')
def env():
    import torch
    import nanomod_amd as nm
    import oracle_c
    L = nm._lib
    assert L.load().nmod_device_count() > 0
    # resident waves of the 200 v 200 instance: four waves per SIMD (its launch bounds), i.e. 16 per compute unit
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 16
    # the smallest launch whose waves keep a strided round of their own (and an item count that is no multiple of anything)
    items = waves
    while _plan(L, items, waves)[0] < 1:
        items += waves
    sizes = [1, 3, 4 * 4096 - 1, 4 * 4096 + 5, 40000, PW * (items + 1) - 1]
    return {'torch': torch, 'nm': nm, 'L': L, 'oracle': oracle_c, 'waves': waves, 'sizes': sizes, 'data': {}, 'exp': {}}


def _plan(L, items, waves, flags=0):
    out = (C.c_int64 * 4)()
    assert L.load().nmod_item_claim_plan(items, waves, flags, out) == 0
    return tuple(int(v) for v in out)


def _rows(env, dtype):
    """the rows of the largest size, once per dtype (smaller sizes take a prefix), on the host and on the device, and the oracle's
    ks_d / ks_p of every position (they depend on the position's rows only)"""
    if dtype not in env['data']:
        torch = env['torch']
        npos = max(env['sizes'])
        rng = np.random.default_rng(20240 + (dtype == 'i16'))
        shift = (np.arange(npos) % 5 == 0) * 0.6
        a = rng.normal(0.0, 1.0, (npos, N))
        b = rng.normal(0.0, 1.0, (npos, N)) + shift[:, None]
        if dtype == 'i16':
            a = np.clip(np.rint(a * 300), -32000, 32000).astype(np.int16)       # milli-units: ties within and between the groups
            b = np.clip(np.rint(b * 300), -32000, 32000).astype(np.int16)
        else:
            a = a.astype(np.float32); b = b.astype(np.float32)
            b[::7, :3] = a[::7, :3]                                              # a few ties between the groups
        a = a.reshape(-1); b = b.reshape(-1)
        off = np.arange(npos + 1, dtype=np.int64) * N
        exp = env['oracle'].detect_batch(a, off, b, off, np.zeros(npos, np.int32), 2, 2.0, 'stouffer', tests=1)
        env['data'][dtype] = (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.zeros(npos, dtype=torch.int32, device='cuda:0'))
        env['exp'][dtype] = exp
    return env['data'][dtype], env['exp'][dtype]


def _detector(env, flags=0):
    L = env['L']
    return env['nm'].DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=L.TEST_KS, flags=flags)


def _run(env, det, dtype, npos):
    (a, b, rid), _ = _rows(env, dtype)
    res = det.run(a[:npos * N], b[:npos * N], rid[:npos], stride0=N, stride1=N, npos=npos)
    env['torch'].cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in TRACKS}


def _same_bits(x, y):
    for k in TRACKS:
        assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), k


def _check_oracle(got, exp, npos):
    assert np.array_equal(got['ks_d'], exp['ks_d'][:npos])
    e = exp['ks_p'][:npos]
    assert np.all(np.abs(got['ks_p'] - e) <= 1e-9 * np.abs(e) + 1e-300), np.abs(got['ks_p'] - e).max()


def test_sizes_sit_around_the_boundaries(env):
    """what the sizes below exercise, from the plan itself: fewer items than waves, one per wave, tickets with one-item chunks
    and no strided round, and a launch whose strided rounds end inside every wave's walk"""
    L, waves = env['L'], env['waves']
    def launch_plan(npos):                    # the launcher's grid: one block of four waves per four items, at most the resident ones
        items = -(-npos // PW)
        return _plan(L, items, min(waves, 4 * -(-items // 4)))
    plans = {n: launch_plan(n) for n in env['sizes']}
    assert plans[1][3] == 0 and plans[3][3] == 0
    big = plans[env['sizes'][-1]]
    assert big[0] >= 1 and big[3] == 1 and big[1] < -(-env['sizes'][-1] // PW)
    if waves == 4096:
        assert plans[4 * 4096 - 1] == (0, 0, 1, 0) and plans[4 * 4096 + 5] == (0, 0, 1, 1) and plans[40000] == (0, 0, 1, 1)


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('size_index', range(6))
def test_claimed_walk_matches_oracle_and_strided_walk(env, dtype, size_index):
    npos = env['sizes'][size_index]
    _, exp = _rows(env, dtype)
    got = _run(env, _detector(env), dtype, npos)
    _check_oracle(got, exp, npos)
    strided = _run(env, _detector(env, env['L'].FLAG_K1_STATIC_ITEMS), dtype, npos)
    _same_bits(got, strided)


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_counter_is_fresh_on_every_call(env, dtype):
    """one detector, one workspace: a counter left over from an earlier launch would make waves skip chunks of the next one"""
    det = _detector(env)
    _, exp = _rows(env, dtype)
    big, small = env['sizes'][-1], 40000
    first = _run(env, det, dtype, big)
    second = _run(env, det, dtype, big)
    _same_bits(first, second)
    _check_oracle(second, exp, big)
    third = _run(env, det, dtype, small)
    _check_oracle(third, exp, small)
    _same_bits(third, _run(env, _detector(env, env['L'].FLAG_K1_STATIC_ITEMS), dtype, small))


def test_side_stream_gives_the_same_bits(env):
    torch = env['torch']
    npos = 4 * 4096 + 5
    ref = _run(env, _detector(env), 'f32', npos)
    side = torch.cuda.Stream(device=0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run(env, _detector(env), 'f32', npos)
    _same_bits(ref, got)


def test_ragged_batch_uses_one_counter_per_class(env):
    """CSR rows whose smaller group falls in three KS size classes (20, 150, 400 samples): three launches, three counters"""
    torch, L = env['torch'], env['L']
    rng = np.random.default_rng(77)
    npos = 6000
    n0 = rng.choice([20, 150, 400], npos); n1 = rng.choice([20, 150, 400], npos)
    off0 = np.concatenate([[0], np.cumsum(n0)]).astype(np.int64); off1 = np.concatenate([[0], np.cumsum(n1)]).astype(np.int64)
    a = rng.normal(0.0, 1.0, off0[-1]).astype(np.float32)
    b = (rng.normal(0.0, 1.0, off1[-1]) + np.repeat((np.arange(npos) % 4 == 0) * 0.5, n1)).astype(np.float32)
    exp = env['oracle'].detect_batch(a, off0, b, off1, np.zeros(npos, np.int32), 2, 2.0, 'stouffer', tests=1)
    dev = [torch.from_numpy(x).cuda() for x in (a, off0, b, off1)]
    rid = torch.zeros(npos, dtype=torch.int32, device='cuda:0')
    outs, shares = [], []
    for flags in (0, L.FLAG_K1_STATIC_ITEMS):
        det = _detector(env, flags)
        res = det.run(dev[0], dev[2], rid, off0=dev[1], off1=dev[3], npos=npos, max_n0=400, max_n1=400)
        torch.cuda.synchronize()
        outs.append({k: res[k].cpu().numpy() for k in TRACKS})
        shares.append(det.dispatch_stats())
    _check_oracle(outs[0], exp, npos)
    _same_bits(outs[0], outs[1])
    assert shares[0] == shares[1] and shares[0]['positions'] == npos and shares[0]['ks_rank'] > 0, shares
