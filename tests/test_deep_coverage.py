"""NMOD_FLAG_DEEP (positions with a group beyond 65 535 samples): the ABI constants, the dispatch-statistics layout, the
dispatcher's answer for deep groups and the command-line switch.  No device needed."""
import ctypes as C

import pytest

import nanomod_amd._lib as L


def _describe(n0, n1, flags=0, tests=L.TEST_ALL, dtype=L.DTYPE_F32):
    lib = L.load()
    prm = L.make_params(memspace=L.MEM_DEVICE, dtype=dtype, tests=tests, method=L.METHOD_STOUFFER, flags=flags)
    buf = C.create_string_buffer(256)
    rc = lib.nmod_describe_dispatch(C.byref(prm), n0, n1, buf, 256)
    return rc, buf.value.decode()


def test_constants():
    assert L.FLAG_DEEP == 32
    assert L.MAX_DEEP == 2 ** 24 - 1
    assert L.FLAG_DEEP not in (L.FLAG_KS_RATIONAL_D, L.FLAG_CHECK_FINITE, L.FLAG_NO_COUNTING, L.FLAG_NO_COUNT_WIDE,
                               L.FLAG_NO_HOST_NARROW, 64)


def test_dispatch_stats_deep_field_takes_the_first_reserved_slot():
    st = L.NmodDispatchStats
    assert C.sizeof(st) == 16 * 8
    assert st.deep.offset == 12 * 8 and st.deep.size == 8
    assert st.reserved.offset == 13 * 8 and st.reserved.size == 3 * 8
    assert 'deep' in [n for n, _ in st._fields_]


@pytest.mark.parametrize('n0,n1', [(100000, 50), (70000, 70000), (L.MAX_DEEP, 10), (10, L.MAX_DEEP)])
@pytest.mark.parametrize('tests', [L.TEST_ALL, L.TEST_KS])
def test_describe_dispatch_names_the_deep_kernel(n0, n1, tests):
    rc, name = _describe(n0, n1, flags=L.FLAG_DEEP, tests=tests)
    assert rc == 0 and name == 'deep_rank_kernel<f32>'
    assert _describe(n0, n1, flags=0, tests=tests)[0] == -3                  # without the flag: NMOD_ERR_TOO_LARGE, as before


def test_describe_dispatch_deep_dtypes_and_limits():
    assert _describe(70000, 5, L.FLAG_DEEP, dtype=L.DTYPE_I16_MILLI) == (0, 'deep_rank_kernel<i16>')
    assert _describe(70000, 5, L.FLAG_DEEP, dtype=L.DTYPE_F64) == (0, 'deep_rank_kernel<f64>')
    assert _describe(L.MAX_DEEP + 1, 10, L.FLAG_DEEP)[0] == -3
    assert _describe(10, L.MAX_DEEP + 1, L.FLAG_DEEP)[0] == -3
    # at or below 65 535 samples the flag changes nothing
    for n0, n1 in ((65535, 65535), (3000, 40), (200, 200)):
        assert _describe(n0, n1, L.FLAG_DEEP) == _describe(n0, n1, 0)


def test_unknown_flag_64_still_refused():
    lib = L.load()
    prm = L.make_params(memspace=L.MEM_DEVICE, flags=64)
    buf = C.create_string_buffer(64)
    assert lib.nmod_describe_dispatch(C.byref(prm), 10, 10, buf, 64) == -1
    prm = L.make_params(memspace=L.MEM_DEVICE, flags=L.FLAG_DEEP | L.FLAG_CHECK_FINITE | L.FLAG_KS_RATIONAL_D)
    assert lib.nmod_describe_dispatch(C.byref(prm), 10, 10, buf, 64) == 0


def test_cli_deep_coverage_reaches_moptions():
    from nanomod_amd import cli
    p = cli.build_parser()
    a = p.parse_args(['detect', '--wrkBase1', 'a.npz', '--wrkBase2', 'b.npz'])
    assert a.deepCoverage == 0 and cli.nmod_options(a)['nmod_deep'] == 0
    a = p.parse_args(['detect', '--wrkBase1', 'a.npz', '--wrkBase2', 'b.npz', '--deepCoverage', '1'])
    assert a.deepCoverage == 1 and cli.nmod_options(a)['nmod_deep'] == 1
    with pytest.raises(SystemExit):
        p.parse_args(['detect', '--wrkBase1', 'a.npz', '--wrkBase2', 'b.npz', '--deepCoverage', '2'])


def test_engine_entry_points_take_deep():
    import inspect
    from nanomod_amd import engine
    for fn in (engine.detect_host, engine.DeviceDetector.__init__, engine.downsample_ks):
        p = inspect.signature(fn).parameters['deep']
        assert p.default is False
