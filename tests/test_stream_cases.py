"""The builders of tests/stream_cases.py without a GPU: real and decoy are two different valid batches of one layout, every offset
array of either is a CSR over its values (so a misordered kernel reads only memory the caller owns), every class an entry has a kernel
for is in the batch, and the stall stays under its cap."""
import numpy as np
import pytest

import stream_cases as S

NAMES = [b.name for b in S.BUILDERS]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_the_thirteen_builders():
    assert len(S.ENTRY_BUILDERS) == 12 and len(set(NAMES)) == 13 and S.RUN_BUILDER.name == 'detect_batch'
    assert all(b.no_sync for b in S.BUILDERS) and set(S.KERNEL_ENTRIES) < {b.name for b in S.ENTRY_BUILDERS}


@pytest.mark.parametrize('part', [1, 3])
@pytest.mark.parametrize('name', NAMES)
def test_real_and_decoy_share_a_layout_and_differ(name, part):
    d = S.BY_NAME[name].make_inputs(part)
    real, decoy = d['real'], d['decoy']
    assert set(real) == set(decoy) and real
    for k in real:
        assert real[k].dtype == decoy[k].dtype and real[k].shape == decoy[k].shape and real[k].ndim == 1, k
    assert any(_bits(real[k]) != _bits(decoy[k]) for k in real)
    assert sum(a.nbytes for a in real.values()) < 4 << 20                 # nothing needs more than a few MB
    # the values differ, not the layout alone: a kernel that read the decoy's values through the real offsets would show as well
    assert any(_bits(real[v]) != _bits(decoy[v]) for _, v in d['csr']) or not d['csr']


@pytest.mark.parametrize('part', [1, 3])
@pytest.mark.parametrize('name', NAMES)
def test_offsets_are_valid_in_both_contents(name, part):
    d = S.BY_NAME[name].make_inputs(part)
    for off_name, val_name in d['csr']:
        ro, do = d['real'][off_name], d['decoy'][off_name]
        for off in (ro, do):
            assert off.dtype == np.int64 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(d['real'][val_name])
        assert len(ro) == len(do) and ro[-1] == do[-1]                    # the same npos and the same total ...
        assert not np.array_equal(ro, do)                                 # ... split differently
    # either content's offsets over the other's values stay inside them: whatever mixture a misordered kernel sees is in bounds
    for off_name, val_name in d['csr']:
        assert d['real'][off_name][-1] <= len(d['decoy'][val_name]) and d['decoy'][off_name][-1] <= len(d['real'][val_name])


@pytest.mark.parametrize('name', NAMES)
def test_every_class_is_present(name):
    d = S.BY_NAME[name].make_inputs(1)
    for label, (cls, need) in d['classes'].items():
        assert set(need) <= set(np.unique(cls).tolist()), (name, label)
    if name == 'detect_batch':                                            # none of nmod_detect_batch's three exceptions
        r = d['real']
        assert r['sig0'].dtype == np.float32 and max(np.diff(r['off0']).max(), np.diff(r['off1']).max()) <= S.RUN_MAX_N
        assert S.RUN_FORMS.index('big') not in d['classes']['K1 form'][0]
    if name in ('mix_fraction', 'one_sample', 'kmer_model', 'site_stoich', 'site_diff', 'rescale_reads', 'read_calls', 'read_llr'):
        assert d['classes'], name


def test_class_helpers_agree_with_the_existing_ones():
    import diff_ref as D
    import grid_cases as G
    import stoich_ref as SR
    pool = G.stoich_pool()
    assert np.array_equal(S.stoich_class_of(pool['lens']), pool['cls'])
    assert S.diff_class_of([1, D.SMALL, 3, D.WAVE + 1], [D.SMALL, D.SMALL + 1, D.WAVE, 5]).tolist() == [0, 1, 1, 2]
    assert S.read_class_of([0, S.RB.WAVE_MAX, S.RB.WAVE_MAX + 1]).tolist() == [0, 0, 1]
    assert S.stoich_class_of([2, 3, SR.SMALL, SR.SMALL + 1, SR.WAVE, SR.WAVE + 1]).tolist() == [-1, 0, 0, 1, 1, 2]
    assert S.run_class_of([2048, 1100, 400], [1500, 90, 512]).tolist() == [2, 1, 0]


def test_reverse_rows_by_hand():
    val, off = S.reverse_rows(np.array([1, 2, 3, 4, 5, 6]), np.array([0, 3, 3, 4, 6]))
    assert val.tolist() == [5, 6, 4, 1, 2, 3] and off.tolist() == [0, 2, 3, 3, 6]


def test_the_chain_inputs():
    d = S.chain2_inputs()
    assert set(d['real']) == set(d['decoy']) and len(d['reads']) == 2
    for s in (0, 1):
        v = 'val%d' % s
        assert d['real'][v].dtype == np.int16 and len(d['real'][v]) == d['reads'][s]['off'][-1] and _bits(d['real'][v]) != _bits(d['decoy'][v])
    for k in ('mean', 'sd', 'alt_mean', 'alt_sd'):
        assert d['real'][k].shape == (4 ** d['k'],) and (d['decoy']['sd'] > 0).all() and (d['decoy']['alt_sd'] > 0).all()


def test_the_stall_is_bounded():
    assert 0.0 < S.SHORT_STALL_MS < S.T_MS and S.T_MS * S.STALL_MARGIN <= S.STALL_CAP_MS == 500.0
    assert len(set(S.SENTINEL.values())) == 3
