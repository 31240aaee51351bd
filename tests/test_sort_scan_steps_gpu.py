"""-m gpu: the device radix sort (radix_sort.hpp) and its callers' key kernels (rank_order.hip) past the sizes at which they
take another path: more chunk sums than one round of rs_scan_tops_kernel (n > 8 388 608 pairs) and more elements than one
sweep of the capped grids (n > 2 097 152).  Every test asserts first that its size crosses the step (tests/size_steps.py,
held to the sources by test_pivot_ref.py); every expected order is unique (stable sorts), every comparison exact."""
import ctypes as C

import numpy as np
import pytest

import size_steps as Z
from test_fdr_gpu import _check_track

pytestmark = pytest.mark.gpu

N_ONE_ROUND = Z.RS_ONE_ROUND_MAX                 # 4 096 tiles, 256 chunk sums: the last size with one round
N_TWO_ROUNDS = Z.RS_ONE_ROUND_MAX + 2049         # 4 098 tiles, 257 chunk sums: the second round holds one, the carry decides it


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


def _keys64(n, seed):
    """random over all 64 bits (every digit of every byte occurs in the late tiles), a third drawn from 50 values (long equal
    runs across the seam: stability), negative keys among both"""
    rng = np.random.default_rng(seed)
    key = rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True)
    pool = rng.integers(-2 ** 63, 2 ** 63 - 1, 50, dtype=np.int64, endpoint=True)
    few = rng.random(n) < 1.0 / 3.0
    key[few] = pool[rng.integers(0, 50, int(few.sum()))]
    assert (key < 0).sum() > n // 3 and (pool < 0).any() and (pool >= 0).any()
    return key


@pytest.mark.parametrize('n', [N_ONE_ROUND, N_TWO_ROUNDS])
def test_argsort_keys_across_the_scan_round(nm, n):
    import torch
    rounds = -(-Z.rs_chunk_sums(n) // Z.RS_TOPS_ROUND)
    if n == N_ONE_ROUND:
        assert 256 * Z.rs_tiles(n) == Z.RS_TOPS_ROUND * Z.RS_SCAN_CHUNK and rounds == 1 and Z.rs_chunk_sums(n + 1) == Z.RS_TOPS_ROUND + 1
    else:
        assert 256 * Z.rs_tiles(n) > Z.RS_TOPS_ROUND * Z.RS_SCAN_CHUNK and Z.rs_tiles(n) == 4098 and rounds == 2
    assert n > Z.RANK_ONE_SWEEP_MAX                                   # (argsort_keys_kernel's grid-stride loop as well)
    key = _keys64(n, n % 1000)
    exp = np.argsort(key, kind='stable')
    got = nm.engine.argsort_device(torch.from_numpy(key).cuda()).cpu().numpy()
    assert np.array_equal(got, exp)
    if n == N_TWO_ROUNDS:                                             # host memory at the larger size
        L = nm._lib
        out = np.full(n, -1, np.int32)
        prm = L.make_params(memspace=L.MEM_HOST)
        assert L.load().nmod_argsort_keys(C.byref(prm), n, key.ctypes.data, out.ctypes.data) == 0
        assert np.array_equal(out, exp)


@pytest.mark.parametrize('descending', [False, True])
def test_rank_order_beyond_one_sweep_of_the_key_kernels(nm, descending):
    """the grid-stride loops of rank_keys_kernel / rank_iota_kernel / rank_emit_kernel; the key recipe of
    test_rank_order_radix_sort_sizes_and_key_ranges"""
    n = Z.RANK_ONE_SWEEP_MAX + 300
    assert (n + 255) // 256 > Z.RANK_GRID_CAP and n > Z.RANK_GRID_CAP * 256
    rng = np.random.default_rng(n)
    raw = rng.integers(0, 1 << 63, n, dtype=np.int64).view(np.float64)
    raw = np.where(rng.random(n) < 0.5, -raw, raw)
    k1 = np.where(rng.random(n) < 0.3, np.round(rng.normal(0, 1, n), 0), raw)
    k1[rng.random(n) < 0.01] = np.inf; k1[rng.random(n) < 0.01] = -np.inf
    k2 = rng.integers(0, 3, n).astype(np.float64) * 1e-310
    k3 = rng.normal(0, 1, n)
    img = np.where(np.isnan(k1), np.inf, k1)
    nan = np.isnan(k1).astype(np.int8)
    exp = np.lexsort((k3, k2, img, nan))
    assert nan.sum() > 0 and len(np.unique(k3)) == n                  # the third key is distinct: the order is unique
    got = nm.engine.rank_order_host(k1, k2, k3, descending=descending)
    assert np.array_equal(got, exp[::-1] if descending else exp)


@pytest.mark.parametrize('method', ['bh', 'by'])
def test_fdr_adjust_across_the_scan_round(nm, method):
    """nmod_fdr_adjust is the entry that meets such sizes (the gathered eight-GPU track has 80 M elements); checked as
    test_fdr_gpu.py::test_sizes checks its sizes"""
    n = N_TWO_ROUNDS
    assert 256 * Z.rs_tiles(n) > Z.RS_TOPS_ROUND * Z.RS_SCAN_CHUNK and Z.rs_chunk_sums(n) > Z.RS_TOPS_ROUND
    rng = np.random.default_rng(n + 17)
    p = rng.random(n)
    p[rng.choice(n, n // 100, replace=False)] *= 1e-9
    q, s = _check_track(nm, p, method, 'n=%d' % n)
    assert s['tested'] == n and s['excluded'] == 0
