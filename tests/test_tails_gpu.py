"""-m gpu: the device p-value tails (K2, finalize_kernel: special_math.hpp) and the window combine (K3, combine_kernel) against
the mpmath fixtures tests/golden/tails_k2.npz / tails_k3.npz (definitions: tail_ref.py; written by oracle/gen_tail_golden.py;
tests/test_tails.py holds the fixtures to the CPU oracles and checks that the inputs reach every branch and band).  numpy only.

D, U, pads, clamps and the convention rows are exact; every p is within 1e-9 relative of the 60-digit value (the project's
contract: helpers.compare_outputs); the statistics follow helpers.assert_close_stat at its usual bounds.  Each test prints the
worst relative error per function and band (pytest -s): profiles/pvalue_tails.txt is where the lines of a run are kept."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import tail_ref as T

pytestmark = pytest.mark.gpu

P_REL = 1e-9
P_OUTPUTS = ('ks_p', 'mwu_p', 't_p')
ALL_OUTPUTS = ('ks_d', 'ks_p', 'mwu_u', 'mwu_p', 't_t', 't_p')


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


@pytest.fixture(scope='module')
def k2():
    return T.load_k2()


@pytest.fixture(scope='module')
def k3():
    return T.load_k3()


@pytest.fixture(scope='module')
def k3_device(nm, k3):
    """(st, p) of the host entry for every fixture track: computed once, shared by the tests below, never written to"""
    out = {}
    for key, p, nb, wd, m in T.k3_tracks(k3):
        st, pv = nm.engine.combine_host(np.zeros(T.K3_N), p, k3['run_id'], nb=nb, weights_dif=float(wd), method=T.METHOD_NAME[m])
        st.setflags(write=False); pv.setflags(write=False)
        out[key] = (st, pv)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_p(got, exp, name):
    err = T.rel_err(got, exp)
    for b, n, w in T.worst_by_band(err, T.p_band(exp)):
        print('  gpu %-22s %-18s n=%-5d worst rel %.2e' % (name, b, n, w))
    i = int(err.argmax())
    assert err.max() <= P_REL, '%s: worst rel %g at position %d (got %r, expected %r)' % (name, err.max(), i, got[i], exp[i])


# ---------------------------------------------------------------------------------------------------------------- K2
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_k2_ladder_all_tests(nm, k2, dtype):
    L = nm._lib
    np_dtype = np.float32 if dtype == 'f32' else np.float64
    sig0, off0, sig1, off1 = T.k2_rows(k2['recipes'], np_dtype)
    got = nm.engine.detect_host(sig0, off0, sig1, off1, None, method='ks', tests=L.TEST_ALL,
                                flags=L.FLAG_NO_HOST_NARROW if dtype == 'f64' else 0)
    assert not got['status'].any(), np.flatnonzero(got['status'])[:8]
    assert np.array_equal(got['ks_d'], k2['ks_d']), 'D (float form) must be exact'
    assert np.array_equal(got['mwu_u'], k2['mwu_u']), 'U must be exact'
    print()
    for k in P_OUTPUTS:
        _check_p(got[k], k2[k], '%s %s' % (dtype, k))
    H.assert_close_stat(got['t_t'], k2['t_t'], 1e-11, H.t_abs_gate(sig0, off0, sig1, off1), 't_t')


@pytest.mark.parametrize('rational', [False, True])
def test_k2_ladder_ks_only(nm, k2, rational):
    L = nm._lib
    sig0, off0, sig1, off1 = T.k2_rows(k2['recipes'], np.float32)
    got = nm.engine.detect_host(sig0, off0, sig1, off1, None, method='ks', tests=L.TEST_KS,
                                flags=L.FLAG_KS_RATIONAL_D if rational else 0)
    assert not got['status'].any()
    assert np.array_equal(got['ks_d'], k2['ks_d_rational' if rational else 'ks_d']), 'D must be exact'
    print()
    _check_p(got['ks_p'], k2['ks_p'], 'ks-only%s ks_p' % (' rational' if rational else ''))


@pytest.mark.parametrize('pair', [(200, 200), (8, 8)])
def test_k2_outputs_do_not_depend_on_the_neighbouring_lanes(nm, k2, pair):
    """K2 is one thread per position and its ballots must not leak between lanes: a position's outputs are the same bits in
    ladder order, under a permutation of the positions and alone in a call"""
    L = nm._lib
    rec = k2['recipes']
    rec = rec[(rec[:, 0] == pair[0]) & (rec[:, 1] == pair[1])]
    npos = len(rec)
    assert npos >= 128
    sig0, _, sig1, _ = T.k2_rows(rec, np.float32)
    a = sig0.reshape(npos, pair[0]); b = sig1.reshape(npos, pair[1])

    def run(idx):
        return nm.engine.detect_host(np.ascontiguousarray(a[idx]).reshape(-1), None, np.ascontiguousarray(b[idx]).reshape(-1), None, None,
                                     method='ks', tests=L.TEST_ALL, stride0=pair[0], stride1=pair[1], flags=L.FLAG_NO_COUNTING)
    base = run(np.arange(npos))
    perm = np.random.default_rng(20261017).permutation(npos)
    shuffled = run(perm)
    for k in ALL_OUTPUTS:
        assert np.array_equal(_bits(shuffled[k]), _bits(base[k][perm])), '%s changes with the position\'s place in the batch' % k
    for i in np.linspace(0, npos - 1, 16).astype(int):
        alone = run(np.array([i]))
        for k in ALL_OUTPUTS:
            assert _bits(alone[k])[0] == _bits(base[k])[i], '%s of position %d differs when it runs alone' % (k, i)


# ---------------------------------------------------------------------------------------------------------------- K3
def test_k3_tracks_against_the_fixture(k3, k3_device):
    print()
    for key, _, nb, wd, m in T.k3_tracks(k3):
        st, pv = k3_device[key]
        T.check_k3_track(key, st, pv, k3, P_REL, st_rel=1e-9, st_abs=1e-12, who='gpu')


STRUCTURE = [(1, 2, 'S'), (1, 2, 'F'), (16, 3, 'S'), (16, 2, 'F'), (64, 2, 'S'), (64, 2, 'F')]


def _against_oracle(st, pv, p, run_id, nb, wd, m, what):
    import nanomod_oracle as orc
    with np.errstate(all='ignore'):
        est, ep = orc.combine_track(np.zeros(len(p)), p, run_id, nb, float(wd), orc.METHOD_STOUFFER if m == 'S' else orc.METHOD_FISHER)
    H.assert_close_stat(st, est, 1e-9, 1e-12, what + ' st')
    H.assert_close_p(pv, ep, P_REL, what + ' p')


@pytest.mark.parametrize('nb,wd,m', STRUCTURE)
def test_k3_cut_tracks(nm, k3, k3_device, nb, wd, m):
    """the track cut to lengths around the tile (256) and its halo: the oracle on the cut track, and every position whose
    window lies inside the cut is the full track's result bit for bit"""
    key = T.k3_key(nb, wd, m)
    p, run_id = k3[key + '_in'], k3['run_id']
    full_st, full_p = k3_device[key]
    for npos in sorted({1, nb, nb + 1, 255, 256, 257, 256 + nb - 1, 512 + nb + 1, T.K3_N}):
        st, pv = nm.engine.combine_host(np.zeros(npos), p[:npos], run_id[:npos], nb=nb, weights_dif=float(wd), method=T.METHOD_NAME[m])
        _against_oracle(st, pv, p[:npos], run_id[:npos], nb, wd, m, '%s cut to %d' % (key, npos))
        keep = max(npos - nb, 0)
        assert np.array_equal(_bits(st[:keep]), _bits(full_st[:keep])) and np.array_equal(_bits(pv[:keep]), _bits(full_p[:keep])), npos
        if m == 'S':                                    # the last nb windows now touch the end of the track
            assert (st[keep:] == -np.inf).all() and (pv[keep:] == 1.0).all()


@pytest.mark.parametrize('nb,wd,m', STRUCTURE)
def test_k3_run_break_next_to_the_tile_seam(nm, k3, k3_device, nb, wd, m):
    """the run break of the seam 255|256 moved to 254|255 and to 256|257: only positions within nb of it change"""
    key = T.k3_key(nb, wd, m)
    p = k3[key + '_in']
    full_st, full_p = k3_device[key]
    for brk in (255, 257):
        run_id = T.k3_run_id(breaks=(brk,) + T.K3_BREAKS[1:])
        st, pv = nm.engine.combine_host(np.zeros(T.K3_N), p, run_id, nb=nb, weights_dif=float(wd), method=T.METHOD_NAME[m])
        _against_oracle(st, pv, p, run_id, nb, wd, m, '%s break at %d' % (key, brk))
        moved = min(brk, 256)                           # the one position that changed its run
        pos = np.arange(T.K3_N)
        far = np.abs(pos - moved) > nb
        assert np.array_equal(_bits(st[far]), _bits(full_st[far])) and np.array_equal(_bits(pv[far]), _bits(full_p[far])), brk
        assert (_bits(pv[~far]) != _bits(full_p[~far])).any()


@pytest.mark.parametrize('nb,wd,m', [(16, 3, 'S'), (64, 2, 'F')])
def test_k3_device_entry_on_a_side_stream(nm, k3, k3_device, nb, wd, m):
    """nmod_combine_track with NMOD_MEM_DEVICE on torch tensors and a non-default stream: the bits of the host entry"""
    import torch
    L = nm._lib
    lib = L.load()
    key = T.k3_key(nb, wd, m)
    dev = 'cuda:0'
    p = torch.from_numpy(k3[key + '_in']).to(dev)
    run = torch.from_numpy(k3['run_id']).to(dev)
    st = torch.full((T.K3_N,), 7.0, dtype=torch.float64, device=dev); pv = torch.full((T.K3_N,), 7.0, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    prm = L.make_params(device=0, stream=side.cuda_stream, memspace=L.MEM_DEVICE, method=L.METHOD_BY_NAME[T.METHOD_NAME[m]],
                        nb=nb, weights_dif=float(wd))
    with torch.cuda.stream(side):
        rc = lib.nmod_combine_track(C.byref(prm), T.K3_N, None, C.c_void_p(p.data_ptr()), C.c_void_p(run.data_ptr()),
                                    C.c_void_p(st.data_ptr()), C.c_void_p(pv.data_ptr()))
    L.check(rc, 'nmod_combine_track')
    side.synchronize()
    host_st, host_p = k3_device[key]
    assert np.array_equal(_bits(st.cpu().numpy()), _bits(host_st)) and np.array_equal(_bits(pv.cpu().numpy()), _bits(host_p))
